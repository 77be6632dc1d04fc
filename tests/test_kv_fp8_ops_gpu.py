"""The FP8 K/V ring kernels (csrc/decode_fp8.hip) through the C ABI: the writers bit for bit against the host restatement of the format
(tests/kv_fp8_ref.py), the attention entry element-wise against the float64 closed form of oracle/decode_cases.py over the dequantised
rings:

    |got - ref| <= 2^-8 |ref| + B_OUT_FP8 max|ref|

B_OUT_FP8 is 4 x the largest gap, relative to max|ref|, between the rounded CPU model (oracle/decode_cases.attn_model) and the float64
reference over every case, arm and family of oracle/decode_cases.py, big_m16128 included, with kc / vc replaced by their dequantised
values -- the rule of oracle/kernel_cases.py.  Measured on the CPU:

    B_OUT_FP8   2.393e-3  d32_n3073 one piece, phantom     -> 9.6e-3      (the bf16 rings: 2.340e-3 -> 9.4e-3)

tests/test_kv_fp8_cpu.py measures every gap again against the constant and shows that the planted faults leave the bound.  The frame
checks are those of tests/test_decode_cases_gpu.py: NaN guards around every output, the partials' workspace starting as NaN, arrival
counters back at zero, identical bits on a second launch, pieces > 1 against one piece within the bound, finished rows zero rows.
"""
import pytest
import torch

from oracle import decode_cases as D
from oracle.kernel_cases import A_BF16, worst
from tests import kv_fp8_ref as R
from tests.test_decode_cases_gpu import BF, EUNSUPPORTED, Flat, _judge

pytestmark = pytest.mark.gpu

B_OUT_FP8 = 9.6e-3

# every row of D.QKV_CASES and one more dh = 16 case (six heads, t beyond the wrap)
WRITER_CASES = list(D.QKV_CASES) + [(3, 96, 16, 9, 20)]
assert {r[2] for r in WRITER_CASES} == {16, 32, 64}


def _pattern(shape, dtype, seed):
    """prior ring contents: arbitrary bytes / exponents, so that a slot the launch must not address shows if it is touched"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g).to(torch.uint8)
    return torch.randint(-100, 100, shape, generator=g).to(torch.int8)


class Rings:
    """the four tensors of a K / V ring pair between NaN-free guards of their own: integer windows cannot hold NaN, so the guards are
    a byte pattern checked for change"""

    def __init__(self, dev, B, H, M, dh, seed):
        self.start = {}
        self.full = {}
        self.view = {}
        for i, (nm, shape, dt) in enumerate((('kq', (B, H, M, dh), torch.uint8), ('ke', (B, H, M), torch.int8),
                                             ('vq', (B, H, M, dh), torch.uint8), ('ve', (B, H, M), torch.int8))):
            n = B * H * M * (dh if len(shape) == 4 else 1)
            full = _pattern((n + 128,), dt, seed + i).to(dev)
            self.start[nm] = full.cpu().clone()
            self.full[nm] = full
            self.view[nm] = full[64:64 + n].view(shape)

    def prior(self, nm):
        return self.start[nm][64:-64].view(self.view[nm].shape)

    def check(self, what):
        torch.cuda.synchronize()
        for nm, full in self.full.items():
            got = full.cpu()
            assert torch.equal(got[:64], self.start[nm][:64]) and torch.equal(got[-64:], self.start[nm][-64:]), f'{what} {nm}: wrote outside'

    def cpu(self, nm):
        return self.view[nm].cpu()


# ---------------------------------------------------------------------------------------------------------------- writers
@pytest.mark.parametrize('B,d,dh,Mring,t', WRITER_CASES)
def test_kv_append_fp8_bit_for_bit(dev, B, d, dh, Mring, t):
    """mxl_kv_append_fp8 on the qkv buffer of the case (with the zero row, the two boundary rows, the subnormal row and the fp8-subnormal
    row planted in heads of k and v): bytes and exponents of slot t mod M equal the reference's, every other slot keeps the pattern it
    started from, qr equals mxl_kv_append's, and a second launch gives the same bytes"""
    from symbolic_music_generation_amd import ops
    c = D.qkv_case(B, d, dh, Mring, t)
    H = d // dh
    x, w, rrb = c['x'].to(dev), c['w'].to(dev), c['rrb'].to(dev)
    t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
    qkv = torch.empty(B, 3 * d, device=dev, dtype=BF)
    ops.gemm_skinny(x, w, qkv, B, 3 * d, d)
    sp = R.special_rows(dh).to(dev)
    for i in range(sp.shape[0]):                                       # row i -> the i-th (sequence, head) of k, the reversed order in v
        b, h = (i % (B * H)) // H, (i % (B * H)) % H
        qkv[b, d + h * dh:d + (h + 1) * dh] = sp[i]
        qkv[b, 2 * d + h * dh:2 * d + (h + 1) * dh] = sp[sp.shape[0] - 1 - i]
    qkv_h = qkv.cpu()
    # the bf16 entry's qr
    kc, vc = torch.zeros(B, H, Mring, dh, device=dev, dtype=BF), torch.zeros(B, H, Mring, dh, device=dev, dtype=BF)
    qr_ref = torch.empty(B, d, device=dev, dtype=BF)
    ops.kv_append(qkv, kc, vc, t_dev, rrb=rrb, qr_out=qr_ref)
    res = []
    for with_qr in (True, True, False):
        r = Rings(dev, B, H, Mring, dh, seed=B * 1000 + t)
        qr = Flat(dev, (B, d), BF)
        v = r.view
        if with_qr:
            ops.kv_append_fp8(qkv, v['kq'], v['ke'], v['vq'], v['ve'], t_dev, rrb=rrb, qr_out=qr.view)
            qr.check('qr')
            assert torch.equal(qr.view.view(torch.int16), qr_ref.view(torch.int16)), 'qr differs from mxl_kv_append'
        else:
            ops.kv_append_fp8(qkv, v['kq'], v['ke'], v['vq'], v['ve'], t_dev)
            torch.cuda.synchronize()
            assert torch.isnan(qr.full.float()).all()
        r.check('kv_append_fp8')
        for third, (qn, en) in ((1, ('kq', 'ke')), (2, ('vq', 've'))):
            wq, we = R.ring_expect_fp8(qkv_h, (r.prior(qn), r.prior(en)), third, t)
            assert torch.equal(r.cpu(en), we), f'{en}: exponents'
            assert torch.equal(r.cpu(qn), wq), f'{qn}: bytes'
        res.append({k: r.cpu(k) for k in v})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]) and torch.equal(res[0][k], res[2][k]), f'{k}: a second launch gives other bytes'
    assert (res[0]['ke'][:, :, t % Mring] != Rings(dev, B, H, Mring, dh, seed=B * 1000 + t).prior('ke')[:, :, t % Mring]).any()


# (B, d, dh, M, T): T < M, T = M, T > M with M not dividing T; dh 64, 32, 16
FILL_CASES = [(2, 128, 64, 40, 17), (3, 96, 32, 24, 24), (2, 64, 16, 7, 38), (1, 128, 64, 37, 100)]


@pytest.mark.parametrize('B,d,dh,M,T', FILL_CASES)
def test_kv_fill_fp8_bit_for_bit(dev, B, d, dh, M, T):
    from symbolic_music_generation_amd import ops
    H = d // dh
    g = torch.Generator().manual_seed(B * 100 + T)
    qkv_h = (torch.randn(B, T, 3 * d, generator=g) * torch.exp2(torch.randint(-6, 7, (B, T, 1), generator=g).float())).to(BF)
    sp = R.special_rows(dh)
    for i in range(sp.shape[0]):                                       # in the last min(T, M) positions, so that they are stored
        p, h = T - 1 - (i % min(T, M)), i % H
        qkv_h[i % B, p, d + h * dh:d + (h + 1) * dh] = sp[i]
        qkv_h[i % B, p, 2 * d + h * dh:2 * d + (h + 1) * dh] = sp[sp.shape[0] - 1 - i]
    qkv = qkv_h.to(dev)
    res = []
    for _ in range(2):
        r = Rings(dev, B, H, M, dh, seed=T)
        v = r.view
        ops.kv_fill_fp8(qkv, v['kq'], v['ke'], v['vq'], v['ve'], T)
        r.check('kv_fill_fp8')
        for third, (qn, en) in ((1, ('kq', 'ke')), (2, ('vq', 've'))):
            wq, we = R.fill_expect_fp8(qkv_h, (r.prior(qn), r.prior(en)), third)
            assert torch.equal(r.cpu(en), we), f'{en}: exponents'
            assert torch.equal(r.cpu(qn), wq), f'{qn}: bytes'
        res.append({k: r.cpu(k) for k in v})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k])
    if T < M:                                                          # slots T .. M - 1 keep their pattern
        assert torch.equal(res[0]['kq'][:, :, T:], r.prior('kq')[:, :, T:]) and torch.equal(res[0]['ve'][:, :, T:], r.prior('ve')[:, :, T:])


# ---------------------------------------------------------------------------------------------------------------- attention
class AttnRunFp8:
    def __init__(self, dev, c):
        self.dev, self.c = dev, c
        self.qkv = c['qkv'].to(BF).to(dev)
        self.kq, self.ke, self.vq, self.ve = (c[k].to(dev).contiguous() for k in ('kq', 'ke', 'vq', 've'))
        self.bd, self.rwb = c['bd'].to(dev), c['rwb'].to(dev)
        self.t_dev = torch.tensor([c['t']], device=dev, dtype=torch.int32)
        self.live = None if c['live'] is None else torch.tensor(c['live'], device=dev, dtype=torch.int32)

    def launch(self, pieces):
        """two identical launches -> the output (B, H, dh) float64 on the CPU"""
        from symbolic_music_generation_amd.ops import _p, _stream, check, lib
        c, dev = self.c, self.dev
        B, H, dh, M = c['B'], c['H'], c['dh'], c['M']
        outs = []
        ws = arrived = None
        if pieces > 1:
            n = int(lib().mxl_relattn_decode_split_ws_bytes(B, H, dh, pieces))
            ws = torch.full((n // 4,), float('nan'), device=dev)
            arrived = torch.zeros(B * H, device=dev, dtype=torch.int32)
        for _ in range(2):
            out = Flat(dev, (B, H * dh), BF)
            rc = lib().mxl_relattn_decode_fp8(_p(self.qkv), _p(self.kq), _p(self.ke), _p(self.vq), _p(self.ve), _p(self.bd), _p(self.rwb),
                                              _p(out.view), _p(self.t_dev), B, H, dh, M, c['scale'], pieces, _p(ws), _p(arrived),
                                              _p(self.live), _stream())
            check(rc, f'fp8 decode attention {c["name"]} pieces {pieces}')
            out.check(f'{c["name"]} pieces {pieces} out')
            if pieces > 1:
                assert int(arrived.abs().sum().item()) == 0, 'the arrival counters must come back to zero'
            outs.append(out.view.clone())
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), 'a second identical launch gives other bits'
        return outs[0].double().cpu().view(B, H, dh)


@pytest.mark.parametrize('name', list(D.ATTN_CASES))
def test_decode_attention_fp8_against_float64(dev, name):
    c0 = D.ATTN_CASES[name]
    bad = []
    for pieces in c0['pieces']:
        for fam in D.families(c0, pieces):
            c = R.fp8_attn_case(name, fam, pieces)
            ref = D.live_zeroed(c, D.attn_ref64(c)[0])
            run = AttnRunFp8(dev, c)
            got = run.launch(pieces)
            if c['live'] is not None:
                dead = [i for i, x in enumerate(c['live']) if not x]
                assert (got[dead] == 0).all(), 'finished rows are zero rows'
            bad += _judge(f'fp8 attention {name} pieces {pieces} {fam}', got, ref, A_BF16, B_OUT_FP8)
            if pieces > 1:
                one = run.launch(1)
                bad += _judge(f'fp8 attention {name} pieces {pieces} {fam} vs one piece', got, one, A_BF16, B_OUT_FP8)
                bad += _judge(f'fp8 attention {name} one piece on the inputs of pieces {pieces} {fam}', one, ref, A_BF16, B_OUT_FP8)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_fp8_entries_reject_what_they_cannot_run(dev):
    """M beyond the shared-memory limit and a head width without an instantiation are refused, not launched: the outputs keep their NaN"""
    from symbolic_music_generation_amd.ops import _p, lib
    t = torch.zeros(64, device=dev)
    ti = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.full((256,), float('nan'), device=dev)
    L = lib()
    assert L.mxl_relattn_decode_fp8(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(out), _p(ti), 1, 1, 64, D.M_LIMIT + 1, 0.125, 1,
                                    None, None, None, None) < 0
    for dh in (8, 24, 128):
        assert L.mxl_relattn_decode_fp8(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(out), _p(ti), 1, 1, dh, 64, 0.125, 1,
                                        None, None, None, None) == EUNSUPPORTED
        assert L.mxl_kv_append_fp8(_p(t), _p(out), _p(out), _p(out), _p(out), _p(ti), 1, 4, dh, dh, None, None, None) == EUNSUPPORTED
        assert L.mxl_kv_fill_fp8(_p(t), _p(out), _p(out), _p(out), _p(out), 1, 1, 4, dh, dh, None) == EUNSUPPORTED
    assert L.mxl_relattn_decode_fp8(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(out), _p(ti), 1, 1, 64, 64, 0.125, 9,
                                    _p(t), _p(ti), None, None) < 0                       # pieces out of 1..8
    assert L.mxl_relattn_decode_fp8(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(out), _p(ti), 1, 1, 64, 64, 0.125, 2,
                                    None, None, None, None) < 0                          # pieces > 1 without a workspace
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), 'a refused call must not write'
