"""CPU pins of the references the kernel-level GPU tests compare with: the hand-checkable cases of the cached-step functions of
oracle/reformer_ref.py (their arithmetic is pinned on HF by test_reformer_oracle_cpu.py::test_cached_decoding_matches_hf, which
runs through them), and the inputs of the decode-shape hashing test."""
import numpy as np
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


# ---- the dropout masks and the GEMM reference of oracle/kernel_cases.py (tests/test_gemm_cases_gpu.py holds the kernels to them)
def _h32(x):
    """mxl_hash32 in Python integers, step by step"""
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_hash_and_threshold_worked_by_hand():
    from oracle.kernel_cases import dropout_thresh, keep_hash, mxl_hash32
    # x = 1: 1 -> 1 * 0x7feb352d -> ^ (>> 15 = 0xffd6) = 0x7febcafb -> * 0x846ca68b mod 2^32 = 0x6889f849 -> ^ (>> 16 = 0x6889)
    assert (0x7feb352d >> 15) == 0xffd6 and (0x7feb352d ^ 0xffd6) == 0x7febcafb
    assert (0x7febcafb * 0x846ca68b) & 0xFFFFFFFF == 0x6889f849 and (0x6889f849 ^ 0x6889) == 0x688990c0
    assert int(mxl_hash32(np.uint32(1))) == 0x688990c0
    assert int(mxl_hash32(np.uint32(0))) == 0
    for x in (2, 0x80000000, 0xFFFFFFFF, 0x9E3779B9):
        assert int(mxl_hash32(np.uint32(x))) == _h32(x)
    assert dropout_thresh(0.0) == 0 and dropout_thresh(0.5) == 1 << 31 and dropout_thresh(0.25) == 1 << 30
    assert dropout_thresh(1.0) == 0xFFFFFFFF and dropout_thresh(0.1) == int(float(np.float32(0.1)) * 2 ** 32) == 429496736
    # one element by the formula of dropout_keep: seed = 2^32 + 5 (high word 1), site 3, index 2^32 + 7
    seed, site, idx = (1 << 32) + 5, 3, (1 << 32) + 7
    mix = (_h32(5 ^ ((3 * 0x9E3779B9) & 0xFFFFFFFF)) + 1) & 0xFFFFFFFF
    want = _h32(((7 * 0x9E3779B1) & 0xFFFFFFFF) ^ ((1 * 0x85EBCA77) & 0xFFFFFFFF) ^ mix)
    assert int(keep_hash(seed, site, np.array([idx], dtype=np.uint64))[0]) == want


def test_keep_masks():
    from oracle.kernel_cases import dropout_thresh, keep_hash, keep_mask, keep_mask32, pair_keep_mask
    idx = np.arange(20000, dtype=np.uint64)
    assert keep_mask(1, 2, idx, 0.0).all() and pair_keep_mask(1, 2, 50, 40, 0.0).all()
    base = keep_mask(11, 4, idx, 0.3)
    assert abs((~base).mean() - 0.3) < 0.02
    for other in (keep_mask(12, 4, idx, 0.3), keep_mask(11, 5, idx, 0.3), keep_mask(11 + (1 << 32), 4, idx, 0.3)):
        assert 0.3 < (other != base).mean() < 0.55                      # seed, site, high seed word: another mask (2 p (1 - p) = 0.42)
    assert np.array_equal(keep_mask32(11 + (9 << 32), 4, idx, 0.3), keep_mask(11 + (9 << 32), 4, idx, 0.3))
    top = np.array([(1 << 32) - 1], dtype=np.uint64)
    assert np.array_equal(keep_mask32(3, 1, top, 0.5), keep_mask(3, 1, top, 0.5))
    hi = idx + np.uint64(1 << 32)                                       # the high index word enters the hash
    assert 0.3 < (keep_mask(11, 4, hi, 0.3) != base).mean() < 0.55
    # the pair mask by hand: one word per pair, low half for the even column, high half for the odd one, threshold thresh >> 16
    M, N, p = 5, 7, 0.4
    pm = pair_keep_mask(21, 6, M, N, p)
    t16 = dropout_thresh(p) >> 16
    for m in range(M):
        for n in range(N):
            h = int(keep_hash(21, 6, np.array([m * N + (n & ~1)], dtype=np.uint64))[0])
            assert pm[m, n] == (((h >> 16) if n & 1 else (h & 0xFFFF)) >= t16)
    big = pair_keep_mask(21, 6, 200, 100, p)
    assert abs((~big).mean() - 0.4) < 0.02
    for other in (pair_keep_mask(22, 6, 200, 100, p), pair_keep_mask(21, 7, 200, 100, p), pair_keep_mask(21 + (1 << 32), 6, 200, 100, p)):
        assert 0.35 < (other != big).mean() < 0.6
    # a threshold whose low half is not its high half: thresh & 0xffff would be another mask
    assert (dropout_thresh(0.4) & 0xFFFF) != t16


def test_gemm_ref_two_by_two_by_hand():
    """A = [[1, 2], [3, 4]], B (N, K) = [[1, -1], [2, 0.5]]:  A B^T = [[-1, 3], [-1, 8]]; one epilogue flag at a time"""
    from oracle.kernel_cases import ADD_AUX, ATOMIC, BIAS, BWD_BITS, DROPOUT, F32, RELU, RELU_BWD, gemm_ref, gemm_ref32
    t = torch.tensor
    A, B = t([[1., 2.], [3., 4.]]), t([[1., -1.], [2., 0.5]])
    bias, aux = t([10., 20.]), t([[0., 5.], [7., 0.]])
    keep = t([[True, False], [False, True]])
    want = {
        0: [[-1, 3], [-1, 8]],
        F32: [[-1, 3], [-1, 8]],
        BIAS: [[9, 23], [9, 28]],
        RELU: [[0, 3], [0, 8]],
        DROPOUT: [[-2, 0], [0, 16]],                       # p = 0.5: kept values doubled
        RELU_BWD: [[0, 3], [-1, 0]],                       # aux > 0
        BWD_BITS: [[0, 3], [-1, 0]],
        ADD_AUX: [[-1, 8], [6, 8]],
        ATOMIC: [[99, 103], [99, 108]],                    # + c0 = 100
    }
    for ref in (gemm_ref, gemm_ref32):
        for fl, w in want.items():
            got = ref(A, B, flags=fl, bias=bias, aux=aux, keep=keep, p=0.5, c0=torch.full((2, 2), 100.) if fl == ATOMIC else None)
            assert torch.equal(got.double(), t(w).double()), (fl, got)
        assert ref(A, B).dtype == (torch.float64 if ref is gemm_ref else torch.float32)
        # the order: alpha, bias, relu, dropout, + aux:  relu(0.5 * acc + bias') * 2 * keep + aux with bias' = [0, -2]
        got = ref(A, B, alpha=0.5, flags=BIAS | RELU | DROPOUT | ADD_AUX, bias=t([0., -2.]), aux=aux, keep=keep, p=0.5)
        assert torch.equal(got.double(), t([[0., 5.], [7., 4.]]).double())
        # alpha before the bias: 0.5 * acc + bias, not 0.5 * (acc + bias)
        assert torch.equal(ref(A, B, alpha=0.5, flags=BIAS, bias=bias).double(), t([[9.5, 21.5], [9.5, 24.]]).double())
        # the storage forms: A given as (K, M), B as (K, N)
        assert torch.equal(ref(A.t().contiguous(), B.t().contiguous(), trans_a=True, trans_b=True).double(), t(want[0]).double())


def test_gemm_case_table_is_consistent():
    """names unique; leading dimensions the launcher accepts; the rows that mean the 192-wide tile get it on a 256-CU device (and
    with the CUs they reserve); the batched rows stay inside their buffers and no two items share an output element unless atomic"""
    from oracle.kernel_cases import ATOMIC, BATCHED_CASES, GEMM_CASES, batched_inputs, batched_ref, nt256_use192
    names = [c['name'] for c in GEMM_CASES]
    assert len(set(names)) == len(names)
    for c in GEMM_CASES:
        if not (c['ta'] and c['tb']):
            assert c['K'] % 8 == 0
        assert c['lda_pad'] % 8 == 0 and c['ldb_pad'] % 8 == 0
        large = not c['ta'] and not c['tb'] and c['M'] >= 256 and c['N'] >= 192 and c['K'] % 64 == 0 and not c['flags'] & ATOMIC
        assert large == (c['expect'] != 0), c['name']
        if large:
            assert (c['expect'] == 2) == nt256_use192(c['M'], c['N'], 256 - c['reserve']), c['name']
    for c in BATCHED_CASES:
        x = batched_inputs(c)
        _, written = batched_ref(c, x)
        if not c['flags'] & ATOMIC:
            assert int(written.sum()) == c['batch'] * c['M'] * c['N']
        for s in (c['sA'], c['sB']):
            assert s[0] % 8 == 0 and s[1] % 8 == 0
