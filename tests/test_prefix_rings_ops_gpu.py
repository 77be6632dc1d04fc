"""The two launches of prompt rings under sampling through the C ABI (csrc/decode_prefix.hip): mxl_kv_append_tail and
mxl_relattn_decode_prefix.

Attention: every row gets random k / v for the positions 0..t, the n rows of a prompt sharing the positions below Tp.  The reference is
what runs today: the ring each row would own in the copied mode -- gathered from the prompt rings and the tail rings by
tests/prefix_ring_ref.py, and checked here against the ring written position by position -- through mxl_relattn_decode_split_live at the
same `pieces`.  The same arithmetic in the same order leaves no tolerance to choose, so the outputs are compared with torch.equal.  The
new launch gets NaN in every location it must not read -- prompt slots a generated position has superseded, prompt slots never written,
tail slots not yet written or no longer in the window -- so a wrong source shows as NaN and not as a near miss.
B0 = 2, H = 2, M = 32, dh 16 / 64, n 2 / 3 / 9 (G = 4 full, G = 4 partial, G = 8 with a partial second group), pieces 1 / 2, and the
(Tp, Mt, t) of prefix_ring_ref.CASES; then M = 256 (prefix_ring_ref.LONG_CASES, pieces 1 / 2 / 4), where a run of one source spans several
load batches and the pieces cut inside the runs."""
import pytest
import torch

from tests import prefix_ring_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B0, H = 2, 2
NAN = float('nan')
EINVAL, EUNSUPPORTED = -1, -2


def _scratch(dev, B, dh, pieces):
    from symbolic_music_generation_amd.ops import lib
    if pieces == 1:
        return None, None
    ws = torch.full((int(lib().mxl_relattn_decode_split_ws_bytes(B, H, dh, pieces)) // 4,), NAN, device=dev)
    return ws, torch.zeros(B * H, device=dev, dtype=torch.int32)


def _case(dev, n, dh, Tp, M, Mt, t, seed):
    """random k / v of the positions 0..t of every row (the prompt's positions shared by its rows) as the copied mode's ring, and as the
    prompt rings and tail rings with NaN wherever the launch has no business"""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    B, d, P = B0 * n, H * dh, t + 1
    x = dict(qkv=r(B, 3 * d).to(BF), rwb=(r(H, dh) * 0.3).to(BF).float().contiguous(), bd=(r(B, H, M) * 2).to(BF).float().contiguous())
    for name in ('k', 'v'):
        pos = r(B, H, P, dh).to(BF)
        npr = min(Tp, P)
        pos[:, :, :npr] = pos[::n, :, :npr].repeat_interleave(n, 0)
        ring = torch.zeros(B, H, M, dh, device=dev, dtype=BF)             # the copied mode: positions in order, slot = p mod M
        prompt = torch.full((B0, H, M, dh), NAN, device=dev, dtype=BF)
        tail = torch.full((B, H, Mt, dh), NAN, device=dev, dtype=BF)
        for p in range(P):
            ring[:, :, p % M] = pos[:, :, p]
        for p in range(max(0, Tp - M), Tp):                                # what the prompt pass leaves (mxl_kv_fill)
            if p <= t and p > t - M:                                       # ... of which only the window's positions may be read
                prompt[:, :, p % M] = pos[::n, :, p]
        for p in range(max(Tp, t - M + 1), P):                             # the window's generated positions
            tail[:, :, (p - Tp) % Mt] = pos[:, :, p]
        x[name + 'ring'], x[name + 'p'], x[name + 't'] = ring, prompt, tail
    return x


def _reference(dev, x, n, dh, M, t, pieces, live):
    from symbolic_music_generation_amd.ops import _p, _stream, check, lib
    B, d = B0 * n, H * dh
    t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
    out = torch.full((B, d), NAN, device=dev, dtype=BF)
    ws, arrived = _scratch(dev, B, dh, pieces)
    check(lib().mxl_relattn_decode_split_live(_p(x['qkv']), _p(x['kring']), _p(x['vring']), _p(x['bd']), _p(x['rwb']), _p(out), _p(t_dev), B,
                                              H, dh, M, dh ** -0.5, pieces, _p(ws), _p(arrived), _p(live), _stream()), 'split_live')
    return out


def _prefix(dev, x, n, dh, M, Mt, t, Tp, pieces, live):
    from symbolic_music_generation_amd.ops import _p, _stream, check, lib
    B, d = B0 * n, H * dh
    t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
    t0_dev = torch.tensor([Tp], device=dev, dtype=torch.int32)
    out = torch.full((B, d), NAN, device=dev, dtype=BF)
    ws, arrived = _scratch(dev, B, dh, pieces)
    check(lib().mxl_relattn_decode_prefix(_p(x['qkv']), _p(x['kp']), _p(x['vp']), _p(x['kt']), _p(x['vt']), _p(x['bd']), _p(x['rwb']),
                                          _p(out), _p(t_dev), _p(t0_dev), B0, n, H, dh, M, Mt, dh ** -0.5, pieces, _p(ws), _p(arrived),
                                          _p(live), _stream()), 'mxl_relattn_decode_prefix')
    if arrived is not None:
        assert int(arrived.abs().sum()) == 0, 'the arrival counters must come back to zero'
    return out


@pytest.mark.parametrize('dh', [16, 64])
@pytest.mark.parametrize('n', [2, 3, 9])
def test_prefix_attention_equals_the_existing_kernel_on_the_gathered_rings(dev, n, dh):
    for i, (Tp, M, Mt, t) in enumerate(R.CASES):
        x = _case(dev, n, dh, Tp, M, Mt, t, 1000 * n + 10 * dh + i)
        for name in ('k', 'v'):            # the host gather rebuilds the copied mode's ring from the poisoned rings: it reads no NaN
            got = R.gather_ring(x[name + 'p'], x[name + 't'], t, Tp, n)
            assert torch.equal(got, x[name + 'ring']), f'the reference gather is off at Tp {Tp} Mt {Mt} t {t}'
        for pieces in (1, 2):
            want = _reference(dev, x, n, dh, M, t, pieces, None)
            got = _prefix(dev, x, n, dh, M, Mt, t, Tp, pieces, None)
            what = f'n {n} dh {dh} Tp {Tp} M {M} Mt {Mt} t {t} pieces {pieces}'
            assert torch.isfinite(got.float()).all(), f'{what}: the launch read a slot from the wrong source'
            assert torch.equal(got, want), f'{what}: {(got != want).sum().item()} of {got.numel()} elements differ'


@pytest.mark.parametrize('dh', [16, 64])
@pytest.mark.parametrize('n', [3, 9])
def test_prefix_attention_over_several_load_batches(dev, n, dh):
    for i, (Tp, M, Mt, t) in enumerate(R.LONG_CASES):
        x = _case(dev, n, dh, Tp, M, Mt, t, 2000 * n + 10 * dh + i)
        for pieces in (1, 2, 4):
            want = _reference(dev, x, n, dh, M, t, pieces, None)
            got = _prefix(dev, x, n, dh, M, Mt, t, Tp, pieces, None)
            what = f'n {n} dh {dh} Tp {Tp} M {M} Mt {Mt} t {t} pieces {pieces}'
            assert torch.isfinite(got.float()).all(), f'{what}: the launch read a slot from the wrong source'
            assert torch.equal(got, want), f'{what}: {(got != want).sum().item()} of {got.numel()} elements differ'


@pytest.mark.parametrize('dh', [16, 64])
@pytest.mark.parametrize('n', [3, 9])
def test_finished_rows_read_no_tail_and_leave_zeros(dev, n, dh):
    M = 32
    for Tp, Mt, t in ((5, 32, 20), (5, 32, 70), (45, 16, 52)):
        x = _case(dev, n, dh, Tp, M, Mt, t, 7 * n + dh + t)
        live = torch.ones(B0 * n, device=dev, dtype=torch.int32)
        done = [1, n - 1] + list(range(n, 2 * n) if t == 70 else ())       # inside live groups; at t = 70 all of prompt 1 as well
        live[done] = 0
        for name in ('k', 'v'):
            x[name + 't'][done] = NAN                                      # a finished row's tail is not read
            x[name + 'ring'][done] = NAN                                   # (nor its ring by the reference)
            if t == 70:
                x[name + 'p'][1] = NAN                                     # a group with no live row reads no ring byte
        for pieces in (1, 2):
            want = _reference(dev, x, n, dh, M, t, pieces, live)
            got = _prefix(dev, x, n, dh, M, Mt, t, Tp, pieces, live)
            what = f'n {n} dh {dh} Tp {Tp} Mt {Mt} t {t} pieces {pieces}'
            assert torch.isfinite(got.float()).all(), f'{what}: a finished row\'s tail or a dead group\'s ring was read'
            assert (got[done].float() == 0).all(), f'{what}: finished rows must leave zeros'
            assert torch.equal(got, want), what
            assert (got[0].float() != 0).any()


@pytest.mark.parametrize('dh', [16, 64])
def test_append_tail_writes_kv_appends_qr_and_the_one_tail_slot(dev, dh):
    from symbolic_music_generation_amd import ops
    B, d, M, Mt, Tp = 10, H * dh, 32, 16, 7
    g = torch.Generator(device=dev).manual_seed(dh)
    qkv = torch.randn(B, 3 * d, generator=g, device=dev).to(BF)
    rrb = torch.randn(d, generator=g, device=dev)
    t0_dev = torch.tensor([Tp], device=dev, dtype=torch.int32)
    for t in (Tp, Tp + 5, Tp + Mt - 1, Tp + Mt, Tp + 2 * Mt + 3):          # the first step, and across the tail's wrap
        t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
        qr_ref = torch.zeros(B, d, device=dev, dtype=BF)
        ops.kv_append(qkv, torch.zeros(B, H, M, dh, device=dev, dtype=BF), torch.zeros(B, H, M, dh, device=dev, dtype=BF), t_dev, rrb=rrb,
                      qr_out=qr_ref)
        # a sentinel pattern that differs in every element of the two rings
        kt = (torch.arange(B * H * Mt * dh, device=dev).view(B, H, Mt, dh) % 251).to(BF)
        vt = (torch.arange(B * H * Mt * dh, device=dev).view(B, H, Mt, dh) % 241 + 300).to(BF)
        want_k, want_v = kt.clone(), vt.clone()
        want_k[:, :, (t - Tp) % Mt] = qkv[:, d:2 * d].view(B, H, dh)
        want_v[:, :, (t - Tp) % Mt] = qkv[:, 2 * d:].view(B, H, dh)
        qr = torch.zeros(B, d, device=dev, dtype=BF)
        ops.kv_append_tail(qkv, kt, vt, t_dev, t0_dev, rrb=rrb, qr_out=qr)
        assert torch.equal(qr.view(torch.int16), qr_ref.view(torch.int16)), 'qr differs from mxl_kv_append\'s'
        assert torch.equal(kt.view(torch.int16), want_k.view(torch.int16)) and torch.equal(vt.view(torch.int16), want_v.view(torch.int16)), t
    # a prompt position (t < Tp) writes no ring; without qr_out the append alone
    kt2, vt2 = want_k.clone(), want_v.clone()
    ops.kv_append_tail(qkv, kt2, vt2, torch.tensor([Tp - 1], device=dev, dtype=torch.int32), t0_dev)
    assert torch.equal(kt2, want_k) and torch.equal(vt2, want_v)


def test_argument_domain(dev):
    from symbolic_music_generation_amd.ops import _p, _stream, lib
    n, dh, M, Mt = 4, 16, 32, 16
    x = _case(dev, n, dh, 5, M, Mt, 9, 1)
    big = _case(dev, n, dh, 5, 40, 16, 9, 2)       # rings of 40 slots: M not a multiple of 16
    t_dev = torch.tensor([9], device=dev, dtype=torch.int32)
    t0_dev = torch.tensor([5], device=dev, dtype=torch.int32)
    out = torch.full((B0 * n * H * 64,), 3.0, device=dev, dtype=BF)
    ws, arrived = _scratch(dev, B0 * n, 64, 8)

    def rc(x=x, qkv=None, B0_=B0, n=n, dh=dh, M=M, Mt=Mt, pieces=1, scratch=True):
        return lib().mxl_relattn_decode_prefix(_p(x['qkv']) if qkv is None else qkv, _p(x['kp']), _p(x['vp']), _p(x['kt']), _p(x['vt']),
                                               _p(x['bd']), _p(x['rwb']), _p(out), _p(t_dev), _p(t0_dev), B0_, n, H, dh, M, Mt, 0.25, pieces,
                                               _p(ws) if scratch else None, _p(arrived) if scratch else None, None, _stream())
    assert rc(Mt=8) == EINVAL and rc(Mt=48) == EINVAL and rc(Mt=24, M=48) == EINVAL        # Mt outside 16..M, no multiple of 16
    assert rc(x=big, M=40) == EINVAL and rc(n=1) == EINVAL
    assert rc(pieces=9) == EINVAL and rc(pieces=0) == EINVAL and rc(pieces=2, scratch=False) == EINVAL
    assert rc(B0_=65536) == EINVAL and rc(B0_=40000, n=9) == EINVAL                        # the grid's second dimension above 65535
    assert rc(qkv=_p(x['qkv']) + 2) == EINVAL                                              # a misaligned buffer
    assert rc(dh=48) == EUNSUPPORTED
    kt = x['kt']
    append = lambda Mt, qkv=_p(x['qkv']): lib().mxl_kv_append_tail(qkv, _p(kt), _p(x['vt']), _p(t_dev), _p(t0_dev), B0 * n, Mt, H * dh, dh, None,
                                                                  None, _stream())
    before = kt.clone()
    assert append(8) == EINVAL and append(24) == EINVAL and append(16, _p(x['qkv']) + 2) == EINVAL
    torch.cuda.synchronize()
    assert (out == 3).all() and int(arrived.abs().sum()) == 0, 'a refused call launched something'
    assert torch.equal(kt.view(torch.int16), before.view(torch.int16))
    assert rc() == 0
    torch.cuda.synchronize()
    assert not (out[:B0 * n * H * dh] == 3).any() and (out[B0 * n * H * dh:] == 3).all()
    # the shared-memory need the header states, and its bound
    need = lambda n, dh, M, p: int(lib().mxl_relattn_decode_prefix_lds_bytes(n, dh, M, p))
    assert need(16, 64, 2048, 1) == 8 * (2048 * 4 + 16 * 64) and need(4, 64, 2048, 1) == 4 * (2048 * 4 + 16 * 64)
    assert need(16, 64, 2048, 4) == 8 * ((512 + 34 + 2) * 4 + 16 * 64) and need(9, 16, 32, 8) == 8 * (32 * 4 + 16 * 16)
    assert need(1, 64, 2048, 1) == 0 and need(16, 64, 2048, 9) == 0
    assert need(16, 64, 4096, 1) <= 160 * 1024 < need(16, 64, 8192, 1)
