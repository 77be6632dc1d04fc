"""The two kernels of indexed rings through the C ABI: mxl_relattn_decode_owned (csrc/decode_attn.hip) and mxl_beam_owner_follow
(csrc/beam.hip).

Attention: 2 items x nb = 3 rows (a beam count that is no power of two), H = 2, M = 96, dh 16 / 32 / 64, t = 5 (a short ring with
never-written slots), M - 2, M - 1 (the boundary), M + 7 and 3 M + 1 (wrapped), 1 and 3 ring pieces, and one arm with a dead row.  The
owner table is random per item: every beam index occurs, one row points wholly at a sibling, one row is the identity.
  (i)   bit-equal to mxl_relattn_decode / _split / _split_live on rings gathered on the host by the same table: the same arithmetic in
        the same order leaves no tolerance to choose
  (ii)  with the identity table, bit-equal to the existing entry on the same rings
  (iii) inside the bound tests/test_decode_cases_gpu.py holds the existing kernel to against the float64 closed form of
        oracle/decode_cases.py (a = 2^-8, b = B_OUT)
  (iv)  every launch of (i) has the other item's rings, and the never-written slots of its own, filled with NaN: a finite result that
        equals the reference shows that no row reads across items or beyond what was written
The follow kernel against the numpy model of tests/beam_owner_ref.py, nb 2 / 3 / 16 and M 32 / 96, with an unmoved item, an in-place
swap and a many-to-one move in one launch, and the mark on slot 0 at t = M - 1."""
import numpy as np
import pytest
import torch

from oracle import decode_cases as D
from oracle.kernel_cases import A_BF16, worst
from tests import beam_owner_ref as R
from tests.test_decode_cases_gpu import B_OUT

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NB, ITEMS, H, M = 3, 2, 2, 96
B = NB * ITEMS
TS = (5, M - 2, M - 1, M + 7, 3 * M + 1)


def _table(g):
    """(B, M) uint8: rows 0 / 3 random, row 1 wholly at sibling 2 and row 4 wholly at sibling 0, rows 2 / 5 the identity"""
    own = torch.randint(0, NB, (B, M), generator=g, dtype=torch.uint8)
    own[1], own[4] = 2, 0
    own[2], own[5] = 2, 2
    assert all(set(own[r].tolist()) == set(range(NB)) for r in (0, 3))             # every beam index occurs
    assert not torch.equal(own[0], own[3])                             # the two items draw different tables
    return own


def _case(dh, t):
    """physical rings (B, H, M, dh), the table, and the oracle-style case dict over the rings gathered by it"""
    g = torch.Generator().manual_seed(1000 * dh + t)
    r = lambda *s: torch.randn(*s, generator=g)
    d, nv = H * dh, min(t + 1, M)
    qkv, rwb, bd = r(B, 3 * d).to(BF).float(), (r(H, dh) * 0.3).to(BF).float(), (r(B, H, M) * 2).to(BF).float()
    kp, vp = r(B, H, M, dh).to(BF), r(B, H, M, dh).to(BF)
    own = _table(g)
    idx = torch.from_numpy(R.gather(np.arange(B)[:, None].repeat(M, 1), own.numpy(), NB))          # (B, M): the source row of a slot
    ke, ve = (torch.stack([x[idx[b], :, torch.arange(M)].transpose(0, 1) for b in range(B)]) for x in (kp, vp))
    ke[:, :, nv:], ve[:, :, nv:] = 0, 0                                # the zero memories the existing kernel never reads
    c = dict(name=f'owned_dh{dh}_t{t}', dh=dh, M=M, t=t, B=B, H=H, nvalid=nv, tm=t % M, d=d, scale=D.scale_of(dh), qkv=qkv,
             q=qkv[:, :d].reshape(B, H, dh), rwb=rwb, kc=ke.float(), vc=ve.float(), bd=bd, live=None)
    return c, kp, vp, own


class Run:
    def __init__(self, dev, c):
        self.dev, self.c = dev, c
        self.qkv, self.bd, self.rwb = c['qkv'].to(BF).to(dev), c['bd'].to(dev), c['rwb'].to(dev)
        self.t_dev = torch.tensor([c['t']], device=dev, dtype=torch.int32)

    def launch(self, kc, vc, pieces, owner=None, live=None):
        """one launch of the owned entry (owner given) or of the existing entry the arm calls for -> (B, H * dh) bf16 on the CPU"""
        from symbolic_music_generation_amd.ops import _p, _stream, check, lib
        c, dev = self.c, self.dev
        dh = c['dh']
        kc, vc = kc.to(dev).contiguous(), vc.to(dev).contiguous()
        out = torch.full((B, H * dh), float('nan'), device=dev, dtype=BF)
        ws = arrived = None
        if pieces > 1:
            ws = torch.full((int(lib().mxl_relattn_decode_split_ws_bytes(B, H, dh, pieces)) // 4,), float('nan'), device=dev)
            arrived = torch.zeros(B * H, device=dev, dtype=torch.int32)
        lv = None if live is None else torch.tensor(live, device=dev, dtype=torch.int32)
        head = (_p(self.qkv), _p(kc), _p(vc))
        tail = (_p(self.bd), _p(self.rwb), _p(out), _p(self.t_dev), B, H, dh, M, c['scale'])
        if owner is not None:
            own = owner.to(dev).contiguous()
            rc = lib().mxl_relattn_decode_owned(*head, _p(own), NB, *tail, pieces, _p(ws), _p(arrived), _p(lv), _stream())
        elif live is not None:
            rc = lib().mxl_relattn_decode_split_live(*head, *tail, pieces, _p(ws), _p(arrived), _p(lv), _stream())
        elif pieces > 1:
            rc = lib().mxl_relattn_decode_split(*head, *tail, pieces, _p(ws), _p(arrived), _stream())
        else:
            rc = lib().mxl_relattn_decode(*head, *tail, _stream())
        check(rc, c['name'])
        torch.cuda.synchronize()
        if pieces > 1:
            assert int(arrived.abs().sum().item()) == 0, 'the arrival counters must come back to zero'
        return out.cpu()


def _bits(x):
    return x.view(torch.int16)


def _check(dev, dh, t, pieces, live=None):
    c, kp, vp, own = _case(dh, t)
    run, nv = Run(dev, c), c['nvalid']
    want = run.launch(c['kc'].to(BF), c['vc'].to(BF), pieces, live=live)           # the existing entry on the gathered rings
    assert torch.isfinite(want.float()).all()
    got = torch.empty_like(want)
    for item in range(ITEMS):                                          # (iv) the other item's rings and the unwritten slots are NaN
        rows = slice(item * NB, (item + 1) * NB)
        kn, vn = torch.full_like(kp, float('nan')), torch.full_like(vp, float('nan'))
        kn[rows, :, :nv], vn[rows, :, :nv] = kp[rows, :, :nv], vp[rows, :, :nv]
        got[rows] = run.launch(kn, vn, pieces, owner=own, live=live)[rows]
    assert torch.isfinite(got.float()).all(), 'a row read another item\'s ring or a never-written slot'
    assert torch.equal(_bits(got), _bits(want)), '(i) owned entry on physical rings != existing entry on gathered rings'
    same = run.launch(c['kc'].to(BF), c['vc'].to(BF), pieces, owner=torch.from_numpy(R.identity(B, NB, M)), live=live)
    assert torch.equal(_bits(same), _bits(want)), '(ii) identity table != existing entry on the same rings'
    ref = D.attn_ref64(c)[0]
    if live is not None:
        dead = [i for i, x in enumerate(live) if not x]
        assert (got[dead].float() == 0).all(), 'finished rows are zero rows'
        ref[dead] = 0
    ratio, err = worst(got.double().view(B, H, dh), ref, A_BF16, B_OUT)
    print(f'owned attention dh {dh} t {t} pieces {pieces}: max err {err:.3e} of max|ref|  worst/bound {ratio:.3f}')
    assert ratio <= 1.0, '(iii) outside the bound of the existing kernel'


@pytest.mark.parametrize('pieces', [1, 3])
@pytest.mark.parametrize('t', TS)
@pytest.mark.parametrize('dh', [16, 32, 64])
def test_owned_attention_equals_the_existing_kernel_on_gathered_rings(dev, dh, t, pieces):
    _check(dev, dh, t, pieces)


def test_owned_attention_with_a_dead_row(dev):
    _check(dev, 64, M + 7, 3, live=(1, 0, 1, 1, 1, 1))
    _check(dev, 32, 5, 1, live=(1, 1, 1, 1, 1, 0))


# ---------------------------------------------------------------------------------------------------------------- follow
@pytest.mark.parametrize('Mo', [32, 96])
@pytest.mark.parametrize('nb', [2, 3, 16])
def test_owner_follow_equals_the_numpy_model(dev, nb, Mo):
    from symbolic_music_generation_amd import ops
    rng = np.random.default_rng(nb * 100 + Mo)
    Bs, rows = 3, 3 * nb
    ident = np.arange(rows)
    src = ident.astype(np.int32)
    src[:nb] = ident[:nb][::-1]                                        # item 0: moved == 0, so what beam_idx holds for it is not read
    src[nb:nb + 2] = [nb + 1, nb]                                      # item 1: an in-place swap, the rest stays
    src[2 * nb:] = 2 * nb + rng.integers(0, nb, nb)                    # item 2: any row from any row, duplicates included
    src[2 * nb] = 2 * nb + nb - 1
    moved = np.array([0, 1, 1], dtype=np.int32)
    for t in (5, Mo - 1, 2 * Mo + 3):
        own = rng.integers(0, nb, (rows, Mo)).astype(np.uint8)
        want = R.follow(own, nb, src, moved, t)
        dev_own = torch.from_numpy(own).to(dev)
        ops.beam_owner_follow(dev_own, nb, torch.from_numpy(src).to(dev), torch.from_numpy(moved).to(dev),
                              torch.tensor([t], device=dev, dtype=torch.int32))
        torch.cuda.synchronize()
        got = dev_own.cpu().numpy()
        assert np.array_equal(got, want), (nb, Mo, t, np.argwhere(got != want)[:4].tolist())
        assert got[:, (t + 1) % Mo].tolist() == (ident % nb).tolist()              # the mark, in the unmoved item too
        rest = np.arange(Mo) != (t + 1) % Mo
        assert np.array_equal(got[:nb][:, rest], own[:nb][:, rest])    # the unmoved item: nothing but the mark (on slot 0 at t = M - 1)
