"""Kernel-level tests of csrc/rf_decode.hip (and of mxl_lsh_sort / mxl_lsh_hash at the shapes cached decoding calls them with).

The end-to-end decoding tests compare logits through a whole model, where one flipped bucket reroutes a window, so they can
only assert quantiles.  Here the discrete decisions (bucket ids, sort order, positions) are INPUTS: the float part is held
against a float64 evaluation of oracle/reformer_ref.py's cached-step functions (pinned on HF by
tests/test_reformer_oracle_cpu.py::test_cached_decoding_matches_hf) at rounding-error tolerance, the integer part bit for bit.
Tolerance rule and helpers: oracle/kernel_cases.py.
"""
import math

import pytest
import torch

from oracle.kernel_cases import A_BF16, bf16_exact, check_gap, gap, hash_decode_case, worst
from oracle.reformer_ref import cached_lsh_attend, cached_range_attend, fix_buckets, lsh_buckets, query_bucket

pytestmark = pytest.mark.gpu

# |got - ref| <= A_BF16 |ref| + B_ATTN max|ref|.  Largest CPU float32-vs-float64 gap over every case below (sorted, range and
# special ones, built by the same functions): 7.4e-7 of max|ref| on one host CPU, 8.8e-7 on another (the einsum summation order
# differs) -> B_ATTN = 4 x the larger, rounded up.
B_ATTN = 3.6e-6


def _heads(x, B, H, dh):
    """(B, N, H*dh) -> (B, H, N, dh)"""
    return x.view(B, x.shape[1], H, dh).transpose(1, 2)


def _attn_inputs(B, H, dh, Tmax, ldmul, seed, qscale):
    """q: the first d columns of a (B, ldmul * d) buffer (the decoder passes its qkv row); caches (B, Tmax, d).  Every fifth
    key is 2^-10 times smaller, so that mean(k^2) is of the order of the 1e-6 in the key normalisation; channel 0 of every
    value head is position / Tmax, so a wrong slot is a wrong output and not noise."""
    g = torch.Generator().manual_seed(seed)
    d = H * dh
    buf = bf16_exact(torch.randn(B, ldmul * d, generator=g) * qscale)
    kc = torch.randn(B, Tmax, d, generator=g)
    kc[:, ::5] *= 2.0 ** -10
    vc = torch.randn(B, Tmax, d, generator=g) * 0.5
    vc.view(B, Tmax, H, dh)[..., 0] = (torch.arange(Tmax) / Tmax).view(1, Tmax, 1)
    return buf, bf16_exact(kc), bf16_exact(vc)


def _refs(fn, buf, kc, vc, B, H, dh):
    """float64 and float32 evaluation of the oracle on the bf16-exact inputs -> (ref64, ref32) as (B, d)"""
    out = []
    for dt in (torch.float64, torch.float32):
        q = buf[:, :H * dh].to(dt).view(B, H, dh)
        out.append(fn(q, _heads(kc.to(dt), B, H, dh), _heads(vc.to(dt), B, H, dh)).reshape(B, H * dh))
    return out


def _run_attn(dev, buf, kc, vc, order, B, H, dh, n_h, Tmax, n, t, start, count, lsh, used):
    """launch with positions outside `used` (bool (Tmax,)) poisoned with NaN and the output inside a NaN canary frame"""
    from symbolic_music_generation_amd import ops
    d = H * dh
    kp, vp = kc.clone(), vc.clone()
    kp[:, ~used] = float('nan')
    vp[:, ~used] = float('nan')
    frame = torch.full((B + 2, d), float('nan'), dtype=torch.bfloat16, device=dev)
    bd = buf.to(dev)
    so = None if order is None else order.to(torch.int32).contiguous().view(B * H * n_h, n).to(dev)
    ops.rf_decode_attn(bd[:, :d], kp.to(dev), vp.to(dev), so, frame[1:B + 1], B, H, dh, n_h, Tmax, n, t, start=start, count=count,
                       lsh=lsh)
    torch.cuda.synchronize()
    frame = frame.float().cpu()
    assert not torch.isnan(frame[1:B + 1]).any(), 'an output element was left unwritten (or a poisoned slot was read)'
    assert torch.isnan(frame[0]).all() and torch.isnan(frame[B + 1]).all(), 'wrote outside (B, H*dh)'
    return frame[1:B + 1]


def _judge(got, ref64, ref32, what):
    g = gap(ref32, ref64)
    ratio, err = worst(got, ref64, A_BF16, B_ATTN)
    print(f'rf_decode_attn {what}: cpu f32-vs-f64 gap {g:.3e}  device max err {err:.3e} of max|ref|  worst/bound {ratio:.3f}')
    check_gap(g, B_ATTN)
    assert ratio <= 1.0, (what, ratio, err)


# (B, H, dh, count, start, lsh, ldmul)
RANGE_CASES = [(1, 1, 16, 1, 0, 1, 2), (3, 3, 32, 1, 64, 1, 3), (1, 3, 64, 1, 0, 0, 2), (3, 1, 32, 2, 0, 1, 3), (1, 12, 16, 2, 64, 0, 2),
               (3, 3, 64, 63, 0, 1, 3), (1, 1, 32, 63, 64, 0, 2), (64, 12, 16, 64, 0, 1, 3), (3, 3, 32, 64, 128, 0, 2),
               (3, 12, 64, 65, 0, 1, 2), (1, 3, 16, 65, 64, 0, 3), (3, 1, 64, 127, 0, 0, 2), (1, 1, 32, 127, 64, 1, 3),
               (3, 3, 16, 128, 0, 1, 2), (64, 3, 64, 128, 64, 0, 3), (3, 12, 32, 128, 192, 1, 2)]


def _range_case(B, H, dh, count, start, lsh, ldmul):
    Tmax = start + count + 37
    t = start + count - 1
    buf, kc, vc = _attn_inputs(B, H, dh, Tmax, ldmul, 1000 + count + start + dh, 2.0 if lsh else 1.5)
    r64, r32 = _refs(lambda q, k, v: cached_range_attend(q, k, v, start, count, bool(lsh), t), buf, kc, vc, B, H, dh)
    return dict(buf=buf, kc=kc, vc=vc, Tmax=Tmax, t=t, r64=r64, r32=r32)


@pytest.mark.parametrize('B,H,dh,count,start,lsh,ldmul', RANGE_CASES)
def test_decode_attn_contiguous_range(dev, B, H, dh, count, start, lsh, ldmul):
    """mxl_rf_decode_attn, contiguous form (local layers; LSH layers before their first hashing), against
    `cached_range_attend` in float64.  CPU float32 gap <= 3.9e-7 of max|ref| over these cases (8.8e-7 over all attention cases)
    -> bound 2^-8 |ref| + 3.6e-6 max|ref|.  With lsh on and count = 1 the only key is the masked self position: the output is that
    row's v, bit for bit."""
    c = _range_case(B, H, dh, count, start, lsh, ldmul)
    used = torch.zeros(c['Tmax'], dtype=torch.bool)
    used[start:start + count] = True
    got = _run_attn(dev, c['buf'], c['kc'], c['vc'], None, B, H, dh, 1, c['Tmax'], c['t'] + 1, c['t'], start, count, lsh, used)
    _judge(got, c['r64'], c['r32'], f'range B{B} H{H} dh{dh} count{count} start{start} lsh{lsh}')
    if count == 1:
        assert torch.equal(got, c['vc'][:, start].float())


def _order(B, H, n_h, n, shift, seed, NBk=8):
    """bucket rows differing per (b, h, round), and the place of the new token (position n - 1) cycling over the rows:
    0 first in the sorted row (chunk 0: the window wraps to the END of the row), 1 last (the last, ragged chunk: the window wraps
    to the FRONT when n < 128, and starts mid-row otherwise), 2 wherever its random bucket puts it, 3 every position in one bucket."""
    g = torch.Generator().manual_seed(seed)
    bk = torch.randint(0, NBk, (B * H * n_h, n), generator=g)
    mode = (torch.arange(B * H * n_h) + shift) % 4
    bk[mode == 0, n - 1] = -1
    bk[mode == 1, n - 1] = NBk
    bk[mode == 3] = 3
    order = torch.argsort(n * bk + torch.arange(n), dim=-1)              # stable, on the host: the device sort has its own test
    return order.view(B, H, n_h, n)


# (B, H, dh, n_h, n, ldmul, shift)
SORTED_CASES = [(3, 3, 32, 2, 64, 3, 0), (1, 1, 16, 1, 64, 2, 1), (1, 1, 64, 1, 64, 2, 0), (3, 1, 16, 3, 65, 2, 0),
                (64, 1, 32, 4, 65, 3, 1), (1, 3, 64, 4, 100, 3, 1), (3, 3, 32, 1, 127, 2, 2), (1, 12, 64, 2, 128, 3, 3),
                (3, 3, 16, 4, 129, 3, 0), (64, 12, 64, 2, 200, 3, 1), (3, 12, 16, 3, 200, 2, 2), (3, 3, 32, 3, 1000, 2, 2),
                (1, 1, 64, 4, 1000, 3, 3), (1, 1, 32, 1, 1000, 2, 0)]


def _sorted_case(B, H, dh, n_h, n, ldmul, shift):
    Tmax = n + 24
    buf, kc, vc = _attn_inputs(B, H, dh, Tmax, ldmul, 2000 + n + dh + n_h, 2.0)
    order = _order(B, H, n_h, n, shift, 3000 + n + n_h)
    r64, r32 = _refs(lambda q, k, v: cached_lsh_attend(q, k, v, order, n - 1), buf, kc, vc, B, H, dh)
    return dict(buf=buf, kc=kc, vc=vc, Tmax=Tmax, order=order, r64=r64, r32=r32)


@pytest.mark.parametrize('B,H,dh,n_h,n,ldmul,shift', SORTED_CASES)
def test_decode_attn_sorted_window(dev, B, H, dh, n_h, n, ldmul, shift):
    """mxl_rf_decode_attn, bucket-sorted form, against `cached_lsh_attend` in float64 with the sort order as an input.  CPU
    float32 gap <= 8.8e-7 of max|ref| -> bound 2^-8 |ref| + 3.6e-6 max|ref|."""
    c = _sorted_case(B, H, dh, n_h, n, ldmul, shift)
    used = torch.arange(c['Tmax']) < n
    got = _run_attn(dev, c['buf'], c['kc'], c['vc'], c['order'], B, H, dh, n_h, c['Tmax'], n, n - 1, 0, 0, 1, used)
    _judge(got, c['r64'], c['r32'], f'sorted B{B} H{H} dh{dh} n_h{n_h} n{n}')


def _special_case(kind):
    """'dominant': one key of the window is the query itself, 8 x longer (softmax close to one-hot on it);
    'lse_gap': three rounds, only round 0's window holds that key, so its logsumexp exceeds the others' by > 20 and their merge
    weights underflow to 0"""
    B, H, dh, n, ldmul = 2, 3, 32, 1000, 3
    n_h = 1 if kind == 'dominant' else 3
    Tmax, d, star = n + 8, H * dh, 500
    buf, kc, vc = _attn_inputs(B, H, dh, Tmax, ldmul, 77, 10.0 if kind == 'lse_gap' else 3.0)
    kc[:, star] = buf[:, :d]
    bk = torch.full((B * H, n_h, n), 3)
    bk[:, 0, star] = -2                       # round 0: the key first, the new token right behind it, everything else in one bucket
    bk[:, 0, n - 1] = -1
    order = torch.argsort(n * bk + torch.arange(n), dim=-1).view(B, H, n_h, n)
    q64 = buf[:, :d].double().view(B, H, dh)
    out, lse = cached_lsh_attend(q64, _heads(kc.double(), B, H, dh), _heads(vc.double(), B, H, dh), order, n - 1, return_lse=True)
    r64, r32 = _refs(lambda q, k, v: cached_lsh_attend(q, k, v, order, n - 1), buf, kc, vc, B, H, dh)
    return dict(B=B, H=H, dh=dh, n_h=n_h, n=n, buf=buf, kc=kc, vc=vc, Tmax=Tmax, order=order, r64=r64, r32=r32, lse=lse)


@pytest.mark.parametrize('kind', ['dominant', 'lse_gap'])
def test_decode_attn_dominant_key_and_round_underflow(dev, kind):
    """a softmax that is nearly one-hot, and hash rounds whose logsumexp lies > 20 below the best one: weights underflow to 0
    cleanly (no NaN), same bound as the other cases (CPU float32 gap 7.3e-7 / 4.7e-10 of max|ref|)"""
    c = _special_case(kind)
    if kind == 'lse_gap':
        assert (c['lse'][:, :, 0] - c['lse'][:, :, 1:].max(-1).values).min().item() > 20
    used = torch.arange(c['Tmax']) < c['n']
    got = _run_attn(dev, c['buf'], c['kc'], c['vc'], c['order'], c['B'], c['H'], c['dh'], c['n_h'], c['Tmax'], c['n'], c['n'] - 1, 0,
                    0, 1, used)
    _judge(got, c['r64'], c['r32'], kind)


@pytest.mark.parametrize('rows,n_h', [(1, 1), (3, 2), (341, 3), (256, 4)])
@pytest.mark.parametrize('where', ['below', 'equal', 'above'])
@pytest.mark.parametrize('tpos', ['first', 'mid', 'last'])
def test_query_bucket_exact(dev, rows, n_h, where, tpos):
    """mxl_rf_query_bucket bit for bit against `query_bucket`: rows * n_h = 1, 6, 1023, 1024 (one workgroup holds at most 1024);
    the offsets widen only when the cached maximum lies strictly above n_h * NB - 1; only column t of the cache changes; the
    running maximum becomes max(old, new ids)"""
    from symbolic_music_generation_amd import ops
    NB, Tmax = 8, 19
    t = {'first': 0, 'mid': 7, 'last': Tmax - 1}[tpos]
    g = torch.Generator().manual_seed(rows * 7 + n_h)
    past_max = n_h * NB - 1 + {'below': -1, 'equal': 0, 'above': 1}[where]
    raw = (torch.randint(0, NB, (rows, n_h), generator=g) + NB * torch.arange(n_h)).to(torch.int32)
    if where == 'below':
        raw[:, -1].clamp_(max=past_max)            # keep the new ids at or below the running maximum in one of the settings
    cache = torch.randint(0, 1000, (rows, n_h, Tmax), generator=g).to(torch.int32)
    want = query_bucket(raw.long(), past_max, n_h, NB).to(torch.int32)
    cd, mx = cache.to(dev), torch.tensor([past_max], dtype=torch.int32, device=dev)
    ops.rf_query_bucket(raw.to(dev), cd, mx, rows, n_h, NB, Tmax, t)
    torch.cuda.synchronize()
    expect = cache.clone()
    expect[:, :, t] = want
    assert torch.equal(cd.cpu(), expect)
    assert mx.item() == max(past_max, int(want.max()))
    assert torch.equal(want, raw + torch.arange(n_h, dtype=torch.int32) * (1 if where == 'above' else 0))


@pytest.mark.parametrize('rows,n_h,T,T_real', [(5, 1, 128, 128), (5, 1, 128, 100), (7, 4, 192, 192), (7, 4, 192, 129), (36, 4, 64, 1)])
def test_fix_buckets_exact(dev, rows, n_h, T, T_real):
    """mxl_lsh_fix_buckets bit for bit against `fix_buckets`: pads to the extra bucket NB, offsets r * (NB + 1)"""
    from symbolic_music_generation_amd import ops
    NB = 16
    g = torch.Generator().manual_seed(rows + T_real)
    bk = (torch.randint(0, NB, (rows, n_h, T), generator=g) + NB * torch.arange(n_h).view(1, n_h, 1)).view(rows, n_h * T)
    frame = torch.full((rows + 2, n_h * T), -7, dtype=torch.int32, device=dev)
    frame[1:rows + 1] = bk.to(torch.int32).to(dev)
    ops.lsh_fix_buckets(frame[1:rows + 1], rows, n_h, T, T_real, NB)
    torch.cuda.synchronize()
    assert torch.equal(frame[1:rows + 1].cpu(), fix_buckets(bk, T, T_real, n_h, NB).to(torch.int32))
    assert (frame[0] == -7).all() and (frame[rows + 1] == -7).all()


@pytest.mark.parametrize('t', [0, 7, 8, 31])
def test_decode_embed_exact(dev, t):
    """mxl_rf_decode_embed: bit-equal to the float32 sum rounded once to bf16, and within one bf16 rounding (2^-8 |ref|, plus
    2^-23 max|ref| for the float32 sum itself) of the float64 sum.  A1 = 8: t = 0, A1 - 1, A1 and the last position of a 4 x 8
    table; d0 = 24 of d = 64; ids wider than t + 1; ids outside [0, V) clamp to the nearest valid row as the kernel documents"""
    from symbolic_music_generation_amd import ops
    B, V, d, d0, A0, A1 = 5, 50, 64, 24, 4, 8
    g = torch.Generator().manual_seed(t)
    E = bf16_exact(torch.randn(V, d, generator=g))
    W0, W1 = torch.randn(A0, d0, generator=g), torch.randn(A1, d - d0, generator=g)
    ids = torch.randint(0, V, (B, 40), generator=g)
    ids[1, t], ids[2, t], ids[3, t], ids[4, t] = -5, V + 3, 0, V - 1
    idc = ids.clamp(0, V - 1)
    pos = torch.cat([W0[t // A1], W1[t % A1]])
    want = (E[idc[:, t]].float() + pos).to(torch.bfloat16)
    ref64 = E[idc[:, t]].double() + pos.double()
    frame = torch.full((B + 2, d), float('nan'), dtype=torch.bfloat16, device=dev)
    ops.rf_decode_embed(ids.to(dev), t, E.to(dev), W0.to(dev), W1.to(dev), frame[1:B + 1], A1)
    torch.cuda.synchronize()
    got = frame[1:B + 1].cpu()
    assert torch.equal(got, want)
    assert worst(got, ref64, A_BF16, 2.0 ** -23)[0] <= 1.0
    assert torch.isnan(frame[0].float()).all() and torch.isnan(frame[B + 1].float()).all()


def _sort_rows(BH, S, NBT, seed):
    """random rows, and one adversarial row each: every slot in bucket 0; buckets descending; only the last bucket used"""
    g = torch.Generator().manual_seed(seed)
    bk = torch.randint(0, NBT, (BH, S), generator=g)
    bk[0] = 0
    if BH > 1:
        bk[1] = (torch.arange(S - 1, -1, -1) * NBT) // S
    if BH > 2:
        bk[2] = NBT - 1
    return bk


def _check_sort(dev, BH, S, T, NBT, seed):
    from symbolic_music_generation_amd import ops
    bk = _sort_rows(BH, S, NBT, seed)
    frame = torch.full((2, BH + 2, S), -7, dtype=torch.int32, device=dev)
    ops.lsh_sort(bk.to(torch.int32).to(dev), frame[0, 1:BH + 1], frame[1, 1:BH + 1], BH, S, T, NBT)
    torch.cuda.synchronize()
    ref = torch.argsort(S * bk + torch.arange(S), dim=-1).to(torch.int32)
    out = frame.cpu()
    assert torch.equal(out[0, 1:BH + 1], ref)                        # stable sort: bit-exact permutation
    assert torch.equal(out[1, 1:BH + 1], ref % T)
    assert (out[:, 0] == -7).all() and (out[:, BH + 1] == -7).all()


@pytest.mark.parametrize('n,NBT,BH', [(64, 9, 6), (65, 34, 64 * 12 * 4), (100, 1, 5), (127, 132, 24), (129, 3, 7), (1000, 2 * 257, 16),
                                      (2047, 4 * 33, 9), (2047, 1, 3)])
def test_lsh_sort_decode_rows(dev, n, NBT, BH):
    """mxl_lsh_sort as the decoder calls it at every step: S = T = n with a ragged last strip of 64, n_buckets_total =
    (NB + 1) * n_h (not a power of two; 1), up to 64 * 12 * 4 rows.  Reference argsort(S * bucket + index)."""
    _check_sort(dev, BH, n, n, NBT, 40 + n)


@pytest.mark.parametrize('S,T,NBT', [(2048, 2048, 2), (2048, 2048, 1024), (2049, 2049, 33), (2049, 2049, 2), (2048 + 63, 2048 + 63, 1024),
                                     (2048 + 63, 2048 + 63, 33), (4096, 2048, 2), (4096, 4096, 33), (4096, 1024, 1024), (4096, 4096, 1025),
                                     (4100, 4100, 33), (4100, 2050, 1024), (8 * 320 + 1, 8 * 320 + 1, 2), (8 * 320 + 1, 8 * 320 + 1, 33),
                                     (8 * 320 + 1, 8 * 320 + 1, 1024)])
def test_lsh_sort_eight_wave_rows(dev, S, T, NBT):
    """rows of S >= 2048 take the 8-wave kernel (each wave a segment rounded up to 64 slots: for S just above 2048 the last
    waves own a short or an empty segment); n_buckets_total = 1025 takes the single-wave kernel on a long row"""
    _check_sort(dev, 5, S, T, NBT, 50 + S + NBT)


@pytest.mark.parametrize('dh', [16, 32, 64])
def test_lsh_hash_decode_call_shape(dev, dh):
    """mxl_lsh_hash as the decoder calls it: T = 1, batch and row stride 3d (the qk columns of the qkv row); dh = 32 / 64 take the
    MFMA kernel, dh = 16 the scalar one.  6144 bucket ids; agreement threshold as test_lsh_hash_and_sort_exact (near-ties only)"""
    from symbolic_music_generation_amd import ops
    c = hash_decode_case(dh)
    B, H, n_h = c['B'], c['H'], c['n_h']
    d = H * dh
    want = lsh_buckets(c['qkv'][:, :d].double().view(B, 1, H, dh).transpose(1, 2), c['rot'].double(), c['factors'][0]).to(torch.int32)
    frame = torch.full((B + 2, H, n_h), -7, dtype=torch.int32, device=dev)
    ops.lsh_hash(c['qkv'].to(dev), 3 * d, 3 * d, c['rot'].to(dev), frame[1:B + 1], B, 1, H, dh, n_h, c['factors'])
    torch.cuda.synchronize()
    out = frame.cpu()
    agree = (out[1:B + 1] == want).float().mean().item()
    print(f'lsh_hash T=1 dh{dh}: agreement {agree:.5f} over {want.numel()} ids')
    assert want.numel() >= 4096 and agree > 0.999, agree
    assert (out[0] == -7).all() and (out[B + 1] == -7).all()
    r = torch.arange(n_h) * math.prod(c['factors'])
    assert ((out[1:B + 1] >= r) & (out[1:B + 1] < r + math.prod(c['factors']))).all()
