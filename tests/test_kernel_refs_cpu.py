"""CPU pins of the references the kernel-level GPU tests compare with: the hand-checkable cases of the cached-step functions of
oracle/reformer_ref.py (their arithmetic is pinned on HF by test_reformer_oracle_cpu.py::test_cached_decoding_matches_hf, which
runs through them), and the inputs of the decode-shape hashing test."""
import pytest
import torch

from oracle.kernel_cases import hash_decode_case
from oracle.reformer_ref import (cached_lsh_attend, cached_lsh_window, cached_range_attend, fix_buckets, lsh_buckets,
                                 query_bucket)


@pytest.mark.parametrize('n', [64, 65, 100, 128, 129, 200])
def test_cached_window_indices(n):
    """the 128 sorted slots around the new token, written out by hand: ranked first (chunk 0: the window starts 64 slots before
    the row, i.e. wraps to its end), ranked last, and on both sides of a chunk border"""
    def slots(rank):
        return cached_lsh_window(torch.tensor(rank), n).tolist()

    assert slots(0) == [(i - 64) % n for i in range(128)]
    assert slots(0)[64:] == [i % n for i in range(64)] and slots(0)[0] == (n - 64) % n
    last = (n - 1) // 64                                   # chunk of the last slot
    assert slots(n - 1) == [((last - 1) * 64 + i) % n for i in range(128)]
    if n == 64:
        assert slots(63) == list(range(64)) * 2            # one chunk: it is its own look-back chunk
    if n == 65:
        assert slots(64) == list(range(65)) + list(range(63))          # chunk 1 holds one slot; the window runs on over the wrap
    if n == 200:
        assert slots(199) == list(range(128, 200)) + list(range(56))
    assert slots(63) == slots(0)                           # last slot of chunk 0
    if n > 64:
        assert slots(64) == [i % n for i in range(128)]    # first slot of chunk 1: chunks 0 and 1
    if n > 128:
        assert slots(127) == slots(64) and slots(128) == [(64 + i) % n for i in range(128)]


def test_cached_lsh_attend_small_known_answer():
    """n = 64, every position in one bucket, one round: the window is the whole row twice, so the result is the plain softmax
    attention over all 64 positions with the self mask (a duplicated key set does not change a softmax average); two identical
    rounds merge to the same result"""
    g = torch.Generator().manual_seed(0)
    B, H, dh, n = 2, 2, 16, 64
    q = torch.randn(B, H, dh, generator=g, dtype=torch.float64)
    qk, v = torch.randn(B, H, n, dh, generator=g, dtype=torch.float64), torch.randn(B, H, n, dh, generator=g, dtype=torch.float64)
    order = torch.arange(n).expand(B, H, 1, n)
    got = cached_lsh_attend(q, qk, v, order, n - 1)
    want = cached_range_attend(q, qk, v, 0, n, True, n - 1)
    assert got.dtype == torch.float64 and (got - want).abs().max().item() < 1e-12
    two = cached_lsh_attend(q, qk, v, order.expand(B, H, 2, n), n - 1)
    assert (two - want).abs().max().item() < 1e-12
    # count = 1 with the self mask: the only key is the token itself, the output is its value
    one = cached_range_attend(q, qk, v, n - 1, 1, True, n - 1)
    assert torch.equal(one, v[:, :, n - 1])
    # lsh off: keys scaled by 1 / sqrt(dh), no mask
    dots = torch.einsum('bhe,bhle->bhl', q, qk[:, :, 3:10]) / 4.0
    want = torch.einsum('bhl,bhle->bhe', torch.softmax(dots, -1), v[:, :, 3:10])
    assert (cached_range_attend(q, qk, v, 3, 7, False, n - 1) - want).abs().max().item() < 1e-12


@pytest.mark.parametrize('n_h,NB', [(1, 8), (2, 8), (4, 16), (3, 5)])
def test_query_bucket_widens_strictly_above(n_h, NB):
    raw = torch.arange(n_h) * NB + torch.tensor([NB - 1, 0, 3, 1][:n_h])
    b = raw - torch.arange(n_h) * NB
    for past_max in (0, n_h * NB - 2, n_h * NB - 1):                     # up to and including equality: unchanged
        assert torch.equal(query_bucket(raw, past_max, n_h, NB), raw)
    for past_max in (n_h * NB, n_h * NB + 5):                            # a pad bucket was cached: offsets r * (NB + 1)
        assert torch.equal(query_bucket(raw, torch.tensor(past_max), n_h, NB), torch.arange(n_h) * (NB + 1) + b)


def test_fix_buckets_matches_padded_hashing():
    """`fix_buckets` on unpadded bucket ids == `lsh_buckets` with the pad mask (the HF-pinned statement of HF515:746-756)"""
    g = torch.Generator().manual_seed(1)
    B, H, T, dh, n_h, NB, T_real = 2, 3, 128, 16, 4, 8, 100
    qk = torch.randn(B, H, T, dh, generator=g)
    rot = torch.randn(H, dh, n_h, NB // 2, generator=g)
    mask = (torch.arange(T) < T_real).view(1, T).expand(B, T)
    want = lsh_buckets(qk, rot, NB, pad_mask=mask).view(B * H, n_h * T)
    got = fix_buckets(lsh_buckets(qk, rot, NB).view(B * H, n_h * T), T, T_real, n_h, NB)
    assert torch.equal(got, want)
    assert got.view(B * H, n_h, T)[:, 2, T_real:].eq(2 * (NB + 1) + NB).all()
    plain = fix_buckets(lsh_buckets(qk, rot, NB).view(B * H, n_h * T), T, T, n_h, NB)          # no pad: only the offsets change
    assert torch.equal(plain, lsh_buckets(qk, rot, NB, increase_num_buckets=True).view(B * H, n_h * T))


@pytest.mark.parametrize('dh', [16, 32, 64])
def test_hash_decode_case_is_stable_across_precisions(dh):
    """the inputs of test_lsh_hash_decode_call_shape: >= 4096 bucket ids, and the oracle in float32 agrees with itself in float64
    above that test's threshold, so a kernel that sums in float32 in another order has room to pass and a wrong one has not"""
    c = hash_decode_case(dh)
    B, H, n_h = c['B'], c['H'], c['n_h']
    qk = c['qkv'][:, :H * dh].view(B, 1, H, dh).transpose(1, 2)
    b32 = lsh_buckets(qk.float(), c['rot'], c['factors'][0])
    b64 = lsh_buckets(qk.double(), c['rot'].double(), c['factors'][0])
    assert b64.numel() == B * H * n_h >= 4096
    assert (b32 == b64).float().mean().item() > 0.999
