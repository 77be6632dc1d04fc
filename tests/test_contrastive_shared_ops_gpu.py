"""The three launches of shared rings under contrastive search through the C ABI (csrc/decode_shared.hip): mxl_kv_stash,
mxl_relattn_decode_shared and mxl_kv_commit_shared.

Attention: a random ring per prompt and random qkv rows.  The reference is what runs today: mxl_kv_append from every row's qkv into
B0 * K copies of the rings, then mxl_relattn_decode_split_live on the copies at the same `pieces`; the same arithmetic in the same
order leaves no tolerance to choose, so the outputs are compared with torch.equal.  The shared launch gets the ring with NaN in slot
t mod M (never read: the row's own k / v stand there) and in every never-written slot, so a finite result shows what was not read.
B0 1 / 3, K 2 / 5 / 16 / 32 (minimum, a count no group size divides, the reference's value, maximum), H = 3, dh 16 / 32 / 64, M 32 / 96 /
256 (one piece-rounding unit, no power of two, several batches), t 0 / 5 / M-2 / M-1 / M / M+7 / 2M-1 / 3M (t mod M is 0, is M-1, lies
inside a piece), pieces 1 / 2 / 8 (pieces whose written range is empty at small t included); with three prompts the middle one is
finished."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H = 3
EINVAL, EUNSUPPORTED = -1, -2


def _ts(M):
    return (0, 5, M - 2, M - 1, M, M + 7, 2 * M - 1, 3 * M)


def _inputs(dev, B0, K, dh, M, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    d, B = H * dh, B0 * K
    return dict(qkv=r(B, 3 * d).to(BF), rwb=(r(H, dh) * 0.3).to(BF).float().contiguous(), bd=(r(B, H, M) * 2).to(BF).float().contiguous(),
                kc=r(B0, H, M, dh).to(BF), vc=r(B0, H, M, dh).to(BF))


def _scratch(dev, B, dh, pieces):
    from symbolic_music_generation_amd.ops import lib
    if pieces == 1:
        return None, None
    ws = torch.full((int(lib().mxl_relattn_decode_split_ws_bytes(B, H, dh, pieces)) // 4,), float('nan'), device=dev)
    return ws, torch.zeros(B * H, device=dev, dtype=torch.int32)


def _reference(dev, x, B0, K, dh, M, t, pieces, live):
    """today's path: K copies of every ring, each row's k / v appended at slot t mod M, the existing attention entry"""
    from symbolic_music_generation_amd.ops import _p, _stream, check, lib
    B, d = B0 * K, H * dh
    kc, vc = x['kc'].repeat_interleave(K, 0).contiguous(), x['vc'].repeat_interleave(K, 0).contiguous()
    t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
    check(lib().mxl_kv_append(_p(x['qkv']), _p(kc), _p(vc), _p(t_dev), B, M, d, dh, None, None, _stream()), 'mxl_kv_append')
    out = torch.full((B, d), float('nan'), device=dev, dtype=BF)
    ws, arrived = _scratch(dev, B, dh, pieces)
    check(lib().mxl_relattn_decode_split_live(_p(x['qkv']), _p(kc), _p(vc), _p(x['bd']), _p(x['rwb']), _p(out), _p(t_dev), B, H, dh, M,
                                              dh ** -0.5, pieces, _p(ws), _p(arrived), _p(live), _stream()), 'split_live')
    return out


def _shared(dev, x, B0, K, dh, M, t, pieces, live):
    from symbolic_music_generation_amd.ops import _p, _stream, check, lib
    B, d = B0 * K, H * dh
    kc, vc = x['kc'].clone(), x['vc'].clone()
    for ring in (kc, vc):                          # what the launch must not read: the step's slot and the never-written slots
        ring[:, :, t % M] = float('nan')
        ring[:, :, min(t + 1, M):] = float('nan')
    t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
    out = torch.full((B, d), float('nan'), device=dev, dtype=BF)
    ws, arrived = _scratch(dev, B, dh, pieces)
    check(lib().mxl_relattn_decode_shared(_p(x['qkv']), _p(kc), _p(vc), _p(x['bd']), _p(x['rwb']), _p(out), _p(t_dev), B0, K, H, dh, M,
                                          dh ** -0.5, pieces, _p(ws), _p(arrived), _p(live), _stream()), 'mxl_relattn_decode_shared')
    if arrived is not None:
        assert int(arrived.abs().sum()) == 0, 'the arrival counters must come back to zero'
    return out


@pytest.mark.parametrize('M', [32, 96, 256])
@pytest.mark.parametrize('dh', [16, 32, 64])
@pytest.mark.parametrize('K', [2, 5, 16, 32])
def test_shared_attention_equals_the_existing_kernel_on_ring_copies(dev, K, dh, M):
    for B0 in (1, 3):
        x = _inputs(dev, B0, K, dh, M, 7 * K + dh + M + B0)
        live = None
        if B0 == 3:                                # one finished sequence among live ones
            live = torch.ones(B0 * K, device=dev, dtype=torch.int32)
            live[K:2 * K] = 0
        for t in _ts(M):
            for pieces in (1, 2, 8):
                want = _reference(dev, x, B0, K, dh, M, t, pieces, live)
                got = _shared(dev, x, B0, K, dh, M, t, pieces, live)
                what = f'B0 {B0} K {K} dh {dh} M {M} t {t} pieces {pieces}'
                assert torch.isfinite(got.float()).all(), f'{what}: the launch read the step\'s ring slot or a never-written one'
                assert torch.equal(got, want), f'{what}: {(got != want).sum().item()} of {got.numel()} elements differ'
                if live is not None:
                    assert (got[K:2 * K].float() == 0).all() and (got[:K].float() != 0).any()


@pytest.mark.parametrize('dh', [16, 64])
def test_stash_writes_kv_appends_qr_and_the_rows_k_and_v(dev, dh):
    from symbolic_music_generation_amd import ops
    B, d, M = 10, H * dh, 32
    g = torch.Generator(device=dev).manual_seed(dh)
    qkv = torch.randn(B, 3 * d, generator=g, device=dev).to(BF)
    rrb = torch.randn(d, generator=g, device=dev)
    t_dev = torch.tensor([3], device=dev, dtype=torch.int32)
    qr_ref = torch.zeros(B, d, device=dev, dtype=BF)
    ops.kv_append(qkv, torch.zeros(B, H, M, dh, device=dev, dtype=BF), torch.zeros(B, H, M, dh, device=dev, dtype=BF), t_dev, rrb=rrb,
                  qr_out=qr_ref)
    layers = torch.full((3, B, 2 * d), 7.0, device=dev, dtype=BF)      # the stash of three layers: the launch writes its slice alone
    qr = torch.zeros(B, d, device=dev, dtype=BF)
    ops.kv_stash(qkv, layers[1], rrb=rrb, qr_out=qr)
    assert torch.equal(qr.view(torch.int16), qr_ref.view(torch.int16)), 'qr differs from mxl_kv_append\'s'
    assert torch.equal(layers[1].view(torch.int16), qkv[:, d:].contiguous().view(torch.int16))
    assert (layers[0] == 7).all() and (layers[2] == 7).all()
    again = torch.full((B, 2 * d), 7.0, device=dev, dtype=BF)          # without qr_out: the copy alone
    ops.kv_stash(qkv, again)
    assert torch.equal(again, layers[1])


@pytest.mark.parametrize('t', [0, 5, 31, 32, 75])
def test_commit_writes_the_picked_rows_slot_and_nothing_else(dev, t):
    from symbolic_music_generation_amd import ops
    B0, K, dh, M, L = 3, 5, 16, 32, 2
    d = H * dh
    g = torch.Generator(device=dev).manual_seed(t)
    # a sentinel pattern that differs in every element of every ring
    rings = [(torch.arange(B0 * H * M * dh, device=dev).view(B0, H, M, dh) % 251 + 300 * i).to(BF) for i in range(2 * L)]
    before = [r.clone() for r in rings]
    stash = torch.randn(L, B0 * K, 2 * d, generator=g, device=dev).to(BF)
    sel = torch.tensor([4, 0, 2], device=dev, dtype=torch.int32)
    ops.kv_commit_shared(rings, stash, K, torch.tensor([t], device=dev, dtype=torch.int32), sel)
    for i, (ring, was) in enumerate(zip(rings, before)):
        l, w = i % L, i // L                       # rings: the K rings of the layers, then the V rings
        want = was.clone()
        for b in range(B0):
            want[b, :, t % M] = stash[l, b * K + int(sel[b]), w * d:(w + 1) * d].view(H, dh)
        assert torch.equal(ring.view(torch.int16), want.view(torch.int16)), f'ring {i} at t {t}'
        assert not torch.equal(ring, was)


def test_argument_domain(dev):
    from symbolic_music_generation_amd.ops import _p, _stream, lib
    B0, K, dh, M = 2, 4, 16, 32
    x = _inputs(dev, B0, 33, dh, M, 1)             # rows enough for every K tried
    t_dev = torch.tensor([5], device=dev, dtype=torch.int32)
    out = torch.full((B0 * 33 * H * 64,), 3.0, device=dev, dtype=BF)
    ws, arrived = _scratch(dev, B0 * 33, 64, 9)

    def rc(K=K, dh=dh, pieces=1):
        return lib().mxl_relattn_decode_shared(_p(x['qkv']), _p(x['kc']), _p(x['vc']), _p(x['bd']), _p(x['rwb']), _p(out), _p(t_dev), B0, K,
                                               H, dh, M, 0.25, pieces, _p(ws), _p(arrived), None, _stream())
    assert rc(K=1) == EINVAL and rc(K=33) == EINVAL and rc(pieces=9) == EINVAL and rc(pieces=0) == EINVAL
    assert rc(dh=48) == EUNSUPPORTED
    assert lib().mxl_relattn_decode_shared(_p(x['qkv']), _p(x['kc']), _p(x['vc']), _p(x['bd']), _p(x['rwb']), _p(out), _p(t_dev), B0, K, H,
                                           dh, M, 0.25, 2, None, None, None, _stream()) == EINVAL      # pieces without their scratch
    torch.cuda.synchronize()
    assert (out == 3).all() and int(arrived.abs().sum()) == 0, 'a refused call launched something'
    assert rc() == 0
    torch.cuda.synchronize()
    assert not (out[:B0 * K * H * dh] == 3).any() and (out[B0 * K * H * dh:] == 3).all()
    # the shared-memory need the header states, and its bound
    need = lambda K, dh, M, p: int(lib().mxl_relattn_decode_shared_lds_bytes(K, dh, M, p))
    assert need(16, 64, 2048, 1) == 8 * (2048 * 4 + 20 * 64) and need(4, 64, 2048, 1) == 4 * (2048 * 4 + 20 * 64)
    assert need(16, 64, 2048, 4) == 8 * ((512 + 34 + 2) * 4 + 20 * 64) and need(16, 16, 32, 8) == 8 * (32 * 4 + 20 * 16)
    assert need(1, 64, 2048, 1) == 0 and need(33, 64, 2048, 1) == 0 and need(16, 64, 2048, 9) == 0
    assert need(16, 64, 8192, 1) > 160 * 1024
