"""mxl_relattn_decode_fp8_owned (csrc/decode_fp8.hip) through the C ABI: the ring attention over FP8 rings read through the owner
table of indexed rings.

The geometry of tests/test_beam_owner_ops_gpu.py: 2 items x nb = 3 rows, H = 2, M = 96, dh 16 / 32 / 64, t = 5 (a short ring with
never-written slots), M - 2, M - 1 (the boundary), M + 7 and 3 M + 1 (wrapped), 1 and 3 ring pieces, the two arms with a dead row, and
the same owner table: random per item with every beam index in it, one row wholly at a sibling, one row the identity (asserted on
the CPU, for every seed the GPU tests use).  The rings are bf16 draws quantised by tests/kv_fp8_ref.quantise.
  (1) bit-equal to mxl_relattn_decode_fp8 on rings whose bytes and exponents were gathered on the host by the table (with its `live`
      argument in the dead-row arms): the same arithmetic in the same order leaves no tolerance to choose
  (2) with the identity table, bit-equal to mxl_relattn_decode_fp8 on the same rings
  (3) inside |got - ref| <= 2^-8 |ref| + B_OUT_FP8 max|ref|, the bound tests/test_kv_fp8_ops_gpu.py holds the FP8 kernel to, against
      the float64 closed form of oracle/decode_cases.py over the dequantised gathered rings
  (4) every launch of (1) has the other item's rings, and the never-written slots of its own, filled with byte 0x7F (e4m3fn NaN) and
      exponent 127: a finite result that equals the reference shows that no row reads across items or beyond what was written
  (5) dead rows are zero rows, and the arrival counters are back at zero after every launch with several pieces
  (6) one case that reaches the double-buffered batches, which M = 96 never does: dh = 64, H = 1, one piece, t = M + 7 and M the
      smallest multiple of 16 above 2 ST, ST = 4 KPW U slots per batch.  The kernel ships U = 11 (FP8_OWNED_U): KPW = 16 at dh = 64,
      ST = 704, M = 1424.
On the commit before the feature the library has no such symbol and every GPU test here fails with AttributeError."""
import numpy as np
import pytest
import torch

from oracle import decode_cases as D
from oracle.kernel_cases import A_BF16, worst
from tests import beam_owner_ref as R
from tests import kv_fp8_ref as F
from tests.test_kv_fp8_ops_gpu import B_OUT_FP8

gpu = pytest.mark.gpu

BF = torch.bfloat16
NB, ITEMS, H, M = 3, 2, 2, 96
B = NB * ITEMS
TS = (5, M - 2, M - 1, M + 7, 3 * M + 1)
U_SHIPPED = 11                                                         # FP8_OWNED_U of csrc/decode_fp8.hip
M_DEEP = (2 * 4 * (64 // (64 // 16)) * U_SHIPPED // 16 + 1) * 16       # dh = 64: KPW = 64 / (dh / 16) = 16 keys per wave instruction
DEEP = dict(dh=64, t=M_DEEP + 7, H=1, M=M_DEEP)
POISON_BYTE, POISON_EXP = 0x7F, 127


def _table(g, M):
    """(B, M) uint8: rows 0 / 3 random, row 1 wholly at sibling 2 and row 4 wholly at sibling 0, rows 2 / 5 the identity"""
    own = torch.randint(0, NB, (B, M), generator=g, dtype=torch.uint8)
    own[1], own[4] = 2, 0
    own[2], own[5] = 2, 2
    assert all(set(own[r].tolist()) == set(range(NB)) for r in (0, 3))             # every beam index occurs
    assert not torch.equal(own[0], own[3])                             # the two items draw different tables
    assert (own[1] != 1).all() and (own[4] != 1).all()                 # a row that points wholly at a sibling
    assert torch.equal(own[[2, 5]], torch.from_numpy(R.identity(B, NB, M))[[2, 5]])            # a row that is the identity
    return own


def _case(dh, t, H=H, M=M):
    """physical fp8 rings (bytes (B, H, M, dh) uint8, exponents (B, H, M) int8) quantised from bf16 draws, the table, the rings
    gathered by it, and the oracle-style case dict over the dequantised gathered rings"""
    g = torch.Generator().manual_seed(1000 * dh + t)
    r = lambda *s: torch.randn(*s, generator=g)
    d, nv = H * dh, min(t + 1, M)
    qkv, rwb, bd = r(B, 3 * d).to(BF).float(), (r(H, dh) * 0.3).to(BF).float(), (r(B, H, M) * 2).to(BF).float()
    # per-slot scales over 2^-3 .. 2^3, so that the exponents differ from slot to slot and from row to row
    kp = (r(B, H, M, dh) * torch.exp2(torch.randint(-3, 4, (B, H, M, 1), generator=g).float())).to(BF)
    vp = (r(B, H, M, dh) * torch.exp2(torch.randint(-3, 4, (B, H, M, 1), generator=g).float())).to(BF)
    own = _table(g, M)
    phys = dict(zip(('kq', 'ke'), F.quantise(kp)))
    phys.update(zip(('vq', 've'), F.quantise(vp)))
    assert len(set(phys['ke'].flatten().tolist())) > 3 and len(set(phys['ve'].flatten().tolist())) > 3
    idx = torch.from_numpy(R.gather(np.arange(B)[:, None].repeat(M, 1), own.numpy(), NB))          # (B, M): the source row of a slot
    gath = {k: torch.stack([x[idx[b], :, torch.arange(M)].transpose(0, 1) for b in range(B)]) for k, x in phys.items()}
    for x in gath.values():
        x[:, :, nv:] = 0                                               # the zero memories the existing kernel never reads
    c = dict(name=f'fp8_owned_dh{dh}_t{t}_M{M}', dh=dh, M=M, t=t, B=B, H=H, nvalid=nv, tm=t % M, d=d, scale=D.scale_of(dh), qkv=qkv,
             q=qkv[:, :d].reshape(B, H, dh), rwb=rwb, kc=F.dequantise(gath['kq'], gath['ke']), vc=F.dequantise(gath['vq'], gath['ve']),
             bd=bd, live=None)
    return c, phys, gath, own


def test_the_owner_tables_of_every_case():
    """(CPU) every case the GPU tests build: `_table` asserts what the docstring says of the table, `_case` that the exponents vary,
    and the gathered rings are the physical ones where the table is the identity and a sibling's where it points at one"""
    for dh in (16, 32, 64):
        for t in TS:
            c, phys, gath, own = _case(dh, t)
            nv = c['nvalid']
            assert torch.equal(gath['kq'][2, :, :nv], phys['kq'][2, :, :nv]) and torch.equal(gath['ve'][5, :, :nv], phys['ve'][5, :, :nv])
            assert torch.equal(gath['vq'][1, :, :nv], phys['vq'][2, :, :nv]) and torch.equal(gath['ke'][4, :, :nv], phys['ke'][3, :, :nv])
            assert not torch.equal(gath['kq'][0, :, :nv], phys['kq'][0, :, :nv])
    c, _, _, own = _case(DEEP['dh'], DEEP['t'], H=DEEP['H'], M=DEEP['M'])
    assert own.shape == (B, M_DEEP) and M_DEEP == 1424 and M_DEEP % 16 == 0 and M_DEEP - 16 <= 2 * 704 < M_DEEP and c['nvalid'] == M_DEEP


class Run:
    def __init__(self, dev, c):
        self.dev, self.c = dev, c
        self.qkv, self.bd, self.rwb = c['qkv'].to(BF).to(dev), c['bd'].to(dev), c['rwb'].to(dev)
        self.t_dev = torch.tensor([c['t']], device=dev, dtype=torch.int32)

    def launch(self, rings, pieces, owner=None, live=None):
        """one launch of the owned entry (owner given) or of mxl_relattn_decode_fp8 -> (B, H * dh) bf16 on the CPU"""
        from symbolic_music_generation_amd.ops import _p, _stream, check, lib
        c, dev = self.c, self.dev
        dh, H, M = c['dh'], c['H'], c['M']
        kq, ke, vq, ve = (rings[k].to(dev).contiguous() for k in ('kq', 'ke', 'vq', 've'))
        assert kq.dtype == torch.uint8 and ke.dtype == torch.int8 and kq.shape == (B, H, M, dh) and ve.shape == (B, H, M)
        out = torch.full((B, H * dh), float('nan'), device=dev, dtype=BF)
        ws = arrived = None
        if pieces > 1:
            ws = torch.full((int(lib().mxl_relattn_decode_split_ws_bytes(B, H, dh, pieces)) // 4,), float('nan'), device=dev)
            arrived = torch.zeros(B * H, device=dev, dtype=torch.int32)
        lv = None if live is None else torch.tensor(live, device=dev, dtype=torch.int32)
        head = (_p(self.qkv), _p(kq), _p(ke), _p(vq), _p(ve))
        tail = (_p(self.bd), _p(self.rwb), _p(out), _p(self.t_dev), B, H, dh, M, c['scale'], pieces, _p(ws), _p(arrived), _p(lv), _stream())
        if owner is not None:
            own = owner.to(dev).contiguous()
            rc = lib().mxl_relattn_decode_fp8_owned(*head, _p(own), NB, *tail)
        else:
            rc = lib().mxl_relattn_decode_fp8(*head, *tail)
        check(rc, c['name'])
        torch.cuda.synchronize()
        if pieces > 1:
            assert int(arrived.abs().sum().item()) == 0, 'the arrival counters must come back to zero'
        return out.cpu()


def _bits(x):
    return x.view(torch.int16)


def _poisoned(phys, rows, nv):
    """the physical rings with everything but the written slots of the item's rows replaced by e4m3fn NaN bytes at exponent 127"""
    out = {}
    for k, x in phys.items():
        p = torch.full_like(x, POISON_BYTE if x.dtype == torch.uint8 else POISON_EXP)
        p[rows, :, :nv] = x[rows, :, :nv]
        out[k] = p
    return out


def _check(dev, dh, t, pieces, live=None, **geom):
    c, phys, gath, own = _case(dh, t, **geom)
    run, nv = Run(dev, c), c['nvalid']
    want = run.launch(gath, pieces, live=live)                         # mxl_relattn_decode_fp8 on the gathered rings
    assert torch.isfinite(want.float()).all()
    got = torch.empty_like(want)
    for item in range(ITEMS):                                          # (4) the other item's rings and the unwritten slots are poison
        rows = slice(item * NB, (item + 1) * NB)
        got[rows] = run.launch(_poisoned(phys, rows, nv), pieces, owner=own, live=live)[rows]
    assert torch.isfinite(got.float()).all(), 'a row read another item\'s ring or a never-written slot'
    assert torch.equal(_bits(got), _bits(want)), '(1) owned entry on physical rings != mxl_relattn_decode_fp8 on gathered rings'
    same = run.launch(gath, pieces, owner=torch.from_numpy(R.identity(B, NB, c['M'])), live=live)
    assert torch.equal(_bits(same), _bits(want)), '(2) identity table != mxl_relattn_decode_fp8 on the same rings'
    ref = D.attn_ref64(c)[0]
    if live is not None:
        dead = [i for i, x in enumerate(live) if not x]
        assert (got[dead].float() == 0).all(), 'finished rows are zero rows'
        ref[dead] = 0
    ratio, err = worst(got.double().view(B, c['H'], dh), ref, A_BF16, B_OUT_FP8)
    print(f'fp8 owned attention dh {dh} t {t} M {c["M"]} pieces {pieces}: max err {err:.3e} of max|ref|  worst/bound {ratio:.3f}')
    assert ratio <= 1.0, '(3) outside the bound of the fp8 kernel'


@gpu
@pytest.mark.parametrize('pieces', [1, 3])
@pytest.mark.parametrize('t', TS)
@pytest.mark.parametrize('dh', [16, 32, 64])
def test_fp8_owned_attention_equals_the_fp8_kernel_on_gathered_rings(dev, dh, t, pieces):
    _check(dev, dh, t, pieces)


@gpu
def test_fp8_owned_attention_with_a_dead_row(dev):
    _check(dev, 64, M + 7, 3, live=(1, 0, 1, 1, 1, 1))
    _check(dev, 32, 5, 1, live=(1, 1, 1, 1, 1, 0))


@gpu
def test_fp8_owned_attention_in_double_buffered_batches(dev):
    """(6): U = 11, M = 1424 > 2 ST = 1408, so a wave consumes batch A, batch B and batch A again"""
    assert DEEP['M'] == 1424
    _check(dev, DEEP['dh'], DEEP['t'], 1, H=DEEP['H'], M=DEEP['M'])
