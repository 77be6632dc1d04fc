"""The Transformer-XL decode-step kernels (the embed, append and BD kernels of csrc/decode.hip, decode_attn_kernel of csrc/decode_attn.hip, the
mxl_decode_qkv epilogue of csrc/gemm_skinny.hip, ops.relattn_decode), every output element against the float64 closed form of oracle/decode_cases.py:

    |got - ref| <= a |ref| + b max|ref|        a = 2^-8 (bf16: the attention output) or 2^-24 (float32: BD)

`b` is 4 x the largest gap, relative to max|ref|, between the rounded CPU model (attn_model: the kernel's bf16 roundings of q + bias and
of P, float32 scores / exponentials / sums through one sequential accumulator, the piece merge; one arm per piece count a case runs)
and the float64 reference over all cases, arms and families of oracle/decode_cases.py -- the rule of oracle/kernel_cases.py.  Measured
on the CPU (largest gap, the case and arm it came from -> b, rounded up):

    B_OUT       2.340e-3  d32_n1025 one piece, phantom     -> 9.4e-3
    B_BD        1.485e-7  bd_b64_m257_h1_ld                -> 6.0e-7
    B_OUT_FULL  1.358e-3  cmp_gemm_dh32                    -> 5.5e-3      (the composite runs the random family alone: a smaller
                                                                           gap than B_OUT's, so a constant of its own)

The random arms sit at 0.2e-3 .. 2.2e-3, the edges arms at 0.5e-3 .. 1.9e-3, the phantom arms at 1.0e-3 .. 2.4e-3 (a near-zero output
is what is left of the bf16 rounding of small probabilities).  tests/test_decode_cases_cpu.py re-measures every gap against these
constants and shows that each favoured slot dropped, the positional term one distance off, the never-written slots left out of the
denominator and a merge with one piece's maximum all leave the bound.

Every launch also checks: the output sits between NaN guards (the C ABI takes no row stride for these outputs, so the guards are the
`Flat` form of tests/test_relattn_cases_gpu.py, for any dtype), every element inside is finite and the guards are untouched; a second
identical launch gives identical bits; with pieces > 1 the partials' workspace starts as NaN and the arrival counters are all zero
afterwards; the split launch and the one-piece launch of the same inputs agree within the same bound.  The ring writers and the
embedding are exact statements and are held bit for bit against plain indexing.
"""
import math

import pytest
import torch

from oracle import decode_cases as D
from oracle.kernel_cases import A_BF16, A_F32, worst

pytestmark = pytest.mark.gpu

B_OUT, B_BD, B_OUT_FULL = 9.4e-3, 6.0e-7, 5.5e-3
EUNSUPPORTED = -2
BF = torch.bfloat16


class Flat:
    """`shape` values of `dtype` between two NaN guards of 64 elements; `fill`: NaN, or the contents the window starts from"""

    def __init__(self, dev, shape, dtype=torch.float32, fill=None):
        n = math.prod(shape)
        self.full = torch.full((n + 128,), float('nan'), device=dev, dtype=dtype)
        self.view = self.full[64:64 + n].view(shape)
        if fill is not None:
            self.view.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.isfinite(self.view.float()).all(), f'{what}: an element inside the frame is not finite (left unwritten?)'
        assert torch.isnan(self.full[:64].float()).all() and torch.isnan(self.full[-64:].float()).all(), f'{what}: wrote outside its window'


def _padded(dev, x, ld):
    """rows of x (R, n) at a row stride of ld, NaN in the columns between -> the (R, n) view"""
    full = torch.full((x.shape[0], ld), float('nan'), device=dev, dtype=BF)
    full[:, :x.shape[1]] = x
    return full[:, :x.shape[1]]


def _judge(what, got, ref, a, b):
    ratio, err = worst(got, ref, a, b)
    print(f'decode {what}: device max err {err:.3e} of max|ref|  worst/bound {ratio:.3f}')
    return [] if ratio <= 1.0 else [(what, ratio, err)]


# ---------------------------------------------------------------------------------------------------------------- attention
class AttnRun:
    """the device buffers of one attention input set and its launches through the C ABI"""

    def __init__(self, dev, c):
        self.dev, self.c = dev, c
        self.qkv, self.kc, self.vc = (c[k].to(BF).to(dev) for k in ('qkv', 'kc', 'vc'))
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
            assert n == B * H * pieces * (dh + 2) * 4
            ws = torch.full((n // 4,), float('nan'), device=dev)
            arrived = torch.zeros(B * H, device=dev, dtype=torch.int32)
        for _ in range(2):
            out = Flat(dev, (B, H * dh), BF)
            args = (_p(self.qkv), _p(self.kc), _p(self.vc), _p(self.bd), _p(self.rwb), _p(out.view), _p(self.t_dev), B, H, dh, M, c['scale'])
            if self.live is not None:
                rc = lib().mxl_relattn_decode_split_live(*args, pieces, _p(ws), _p(arrived), _p(self.live), _stream())
            elif pieces > 1:
                rc = lib().mxl_relattn_decode_split(*args, pieces, _p(ws), _p(arrived), _stream())
            else:
                rc = lib().mxl_relattn_decode(*args, _stream())
            check(rc, f'decode attention {c["name"]} pieces {pieces}')
            out.check(f'{c["name"]} pieces {pieces} out')
            if pieces > 1:
                assert int(arrived.abs().sum().item()) == 0, 'the arrival counters must come back to zero'
            outs.append(out.view.clone())
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), 'a second identical launch gives other bits'
        return outs[0].double().cpu().view(B, H, dh)


@pytest.mark.parametrize('name', list(D.ATTN_CASES))
def test_decode_attention_against_float64(dev, name):
    c0 = D.ATTN_CASES[name]
    bad = []
    for pieces in c0['pieces']:
        for fam in D.families(c0, pieces):
            c = D.attn_case(name, fam, pieces)
            ref = D.live_zeroed(c, D.attn_ref64(c)[0])
            run = AttnRun(dev, c)
            got = run.launch(pieces)
            if c['live'] is not None:
                dead = [i for i, x in enumerate(c['live']) if not x]
                assert (got[dead] == 0).all(), 'finished rows are zero rows'
            bad += _judge(f'attention {name} pieces {pieces} {fam}', got, ref, A_BF16, B_OUT)
            if pieces > 1:
                one = run.launch(1)
                bad += _judge(f'attention {name} pieces {pieces} {fam} vs one piece', got, one, A_BF16, B_OUT)
                bad += _judge(f'attention {name} one piece on the inputs of pieces {pieces} {fam}', one, ref, A_BF16, B_OUT)
    assert not bad, bad


def test_decode_attention_rejects_what_it_cannot_run(dev):
    """M beyond the shared-memory limit and a head width without an instantiation are refused, not launched"""
    from symbolic_music_generation_amd.ops import _p, lib
    t = torch.zeros(64, device=dev)
    ti = torch.zeros(1, device=dev, dtype=torch.int32)
    assert lib().mxl_relattn_decode(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(ti), 1, 1, 64, D.M_LIMIT + 1, 0.125, None) < 0
    assert lib().mxl_relattn_decode(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), _p(ti), 1, 1, 24, 64, 0.125, None) == EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- BD
@pytest.mark.parametrize('name', list(D.BD_CASES))
def test_decode_bd_against_float64(dev, name):
    from symbolic_music_generation_amd.ops import _p, _stream, check, lib
    c = D.bd_case(name)
    B, H, M, d = c['B'], c['H'], c['M'], c['d']
    qr, rd = _padded(dev, c['qr'].to(BF), c['ld_qr']), _padded(dev, c['rd'].to(BF), c['ld_rd'])
    ref = D.bd_ref(c['qr'], c['rd'], H)
    outs = []
    for _ in range(2):
        bd = Flat(dev, (B, H, M))
        check(lib().mxl_decode_bd(_p(qr), _p(rd), _p(bd.view), B, H, 64, M, c['ld_qr'], c['ld_rd'], _stream()), 'mxl_decode_bd')
        bd.check(f'{name} bd')
        outs.append(bd.view.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    bad = _judge(f'bd {name}', outs[0].double().cpu(), ref, A_F32, B_BD)
    assert not bad, bad
    bd = Flat(dev, (B, H, M))
    for dh in (16, 32, 128):
        assert lib().mxl_decode_bd(_p(qr), _p(rd), _p(bd.view), B, H, dh, M, c['ld_qr'], c['ld_rd'], _stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(bd.full).all(), 'an unsupported call must not write'


# ---------------------------------------------------------------------------------------------------------------- ring writers
@pytest.mark.parametrize('B,d,dh,Mring,t', D.QKV_CASES)
def test_ring_writers_bit_for_bit(dev, B, d, dh, Mring, t):
    """mxl_decode_qkv and mxl_gemm_skinny_bf16 + mxl_kv_append: the rings against plain indexing of the qkv buffer the launch itself
    wrote, every other slot unchanged, qr = bf16(q + r_r_bias), and the fused launch equal to the pair bit for bit"""
    from symbolic_music_generation_amd import ops
    c = D.qkv_case(B, d, dh, Mring, t)
    H = d // dh
    x, w, rrb = c['x'].to(dev), c['w'].to(dev), c['rrb'].to(dev)
    t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
    res = []
    for form in ('pair', 'fused', 'append_only'):
        kc, vc = Flat(dev, (B, H, Mring, dh), BF, c['kc0']), Flat(dev, (B, H, Mring, dh), BF, c['vc0'])
        qkv, qr = Flat(dev, (B, 3 * d), BF), Flat(dev, (B, d), BF)
        if form == 'fused':
            ops.decode_qkv(x, w, qkv.view, kc.view, vc.view, t_dev, rrb, qr.view, dh)
        else:
            ops.gemm_skinny(x, w, qkv.view, B, 3 * d, d)
            if form == 'pair':
                ops.kv_append(qkv.view, kc.view, vc.view, t_dev, rrb=rrb, qr_out=qr.view)
            else:                                                    # without qr: the rings alone
                ops.kv_append(qkv.view, kc.view, vc.view, t_dev)
        for nm, f in (('kc', kc), ('vc', vc), ('qkv', qkv)) + ((('qr', qr),) if form != 'append_only' else ()):
            f.check(f'{form} {nm}')
        if form == 'append_only':
            assert torch.isnan(qr.full.float()).all()
        got = dict(qkv=qkv.view.cpu(), kc=kc.view.cpu(), vc=vc.view.cpu(), qr=qr.view.cpu())
        bits = lambda a: a.view(torch.int16)
        assert torch.equal(bits(got['kc']), bits(D.ring_expect(got['qkv'], c['kc0'], 1, t))), f'{form}: K ring'
        assert torch.equal(bits(got['vc']), bits(D.ring_expect(got['qkv'], c['vc0'], 2, t))), f'{form}: V ring'
        assert not torch.equal(got['kc'][:, :, t % Mring], c['kc0'][:, :, t % Mring])
        if form != 'append_only':
            assert torch.equal(bits(got['qr']), bits(D.qr_expect(got['qkv'], c['rrb'], d))), f'{form}: qr'
        res.append(got)
    for nm in ('qkv', 'kc', 'vc', 'qr'):
        assert torch.equal(res[0][nm].view(torch.int16), res[1][nm].view(torch.int16)), f'fused != pair: {nm}'
    assert torch.equal(res[0]['kc'].view(torch.int16), res[2]['kc'].view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize('B,d,V,T,ld,t', D.EMBED_CASES)
def test_decode_embed_bit_for_bit(dev, B, d, V, T, ld, t):
    from symbolic_music_generation_amd import ops
    c = D.embed_case(B, d, V, T, ld, t)
    ids = c['ids'].to(dev)[:, :T]
    assert ids.stride(0) == ld
    out = Flat(dev, (B, d), BF)
    ops.decode_embed(ids, torch.tensor([t], device=dev, dtype=torch.int32), c['E'].to(dev), out.view, c['scale'])
    out.check('embed')
    assert torch.equal(out.view.cpu().view(torch.int16), c['want'].view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- composite
@pytest.mark.parametrize('name', list(D.COMPOSITE_CASES))
@pytest.mark.parametrize('qr_ready', [False, True])
def test_relattn_decode_composite_against_float64(dev, name, qr_ready):
    """ops.relattn_decode: bias add (or the qr that kv_append left), BD by mxl_decode_bd or the batched GEMM, attention"""
    from symbolic_music_generation_amd import ops
    c = D.composite_case(name)
    B, H, dh, M, d = c['B'], c['H'], c['dh'], c['M'], c['d']
    qkv, kc, vc = (c[k].to(BF).to(dev) for k in ('qkv', 'kc', 'vc'))
    rd = _padded(dev, c['rd'].to(BF), d + c['ld_rd_pad'])
    rwb, rrb = c['rwb'].to(dev), c['rrb'].to(dev)
    t_dev = torch.tensor([c['t']], device=dev, dtype=torch.int32)
    qr, bd, out = Flat(dev, (B, d), BF), Flat(dev, (B, H, M)), Flat(dev, (B, d), BF)
    if qr_ready:
        kc0, vc0 = kc.clone(), vc.clone()
        ops.kv_append(qkv, kc, vc, t_dev, rrb=rrb.reshape(-1), qr_out=qr.view)
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)          # (the case's newest slot already holds the row's k / v)
    first = None
    for _ in range(2):               # every buffer the call writes is NaN again before the second launch
        out.view.fill_(float('nan'))
        bd.view.fill_(float('nan'))
        if not qr_ready:
            qr.view.fill_(float('nan'))
        ops.relattn_decode(qkv, kc, vc, rd, rwb, rrb, out.view, t_dev, H, dh, qr.view, bd.view, scale=c['scale'], qr_ready=qr_ready)
        for nm, f in (('qr', qr), ('bd', bd), ('out', out)):
            f.check(f'{name} {nm}')
        bits = (out.view.view(torch.int16).clone(), bd.view.view(torch.int32).clone())
        assert first is None or (torch.equal(first[0], bits[0]) and torch.equal(first[1], bits[1])), 'a second launch gives other bits'
        first = bits
    assert torch.equal(qr.view.cpu().view(torch.int16), D.qr_expect(c['qkv'].to(BF), c['rrb'].reshape(-1), d).view(torch.int16))
    bad = _judge(f'composite {name} bd', bd.view.double().cpu(), D.composite_bd(c), A_F32, B_BD)
    bad += _judge(f'composite {name} out', out.view.double().cpu().view(B, H, dh), D.composite_ref64(c), A_BF16, B_OUT_FULL)
    assert not bad, bad
