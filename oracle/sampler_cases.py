"""ORACLE-side statement of the samplers' random draw (test infrastructure, NOT product code): the uniform of sample_kernel /
sample_step_kernel (csrc/decode.hip) and sample_large_kernel (csrc/sample_large.hip) as integer-exact host code, the inputs on which
the kernels' arithmetic is exact (so that a token reveals the top bits of the hash), the case table of real distributions, their
float64 reference and the token-for-token checker.  Shared by tests/test_sampler_cases_cpu.py and tests/test_sampler_cases_gpu.py.

The draw is a pure function of (seed, row, rng_ctr, scores):

    h1 = hash32(hi32(ctr * 0x9E3779B97F4A7C15) ^ hash32(row + 0x85ebca6b * lo32(seed)))
    h2 = hash32(h1 + lo32(ctr) + hi32(seed))          j = h2 >> 8          u = j / 2^24

and the token is the first entry, in the sampler's order, whose inclusive cumulative probability exceeds u.

Reference.  The scores a kernel orders by are fp32(row * fp32(1 / temperature)), the repetition penalty applied as the kernels state
it (kernel_scores: plain float32 multiplies and divides, which the host reproduces bit for bit); they give the order and the ties.
Everything after that is float64: top-k (score descending, ties by ascending index), top-p (an entry stays iff the mass ordered before
it is below top_p), typical-p (the same with the order |-log p - H| ascending), the renormalisation, and the cumulative sums in the
sampler's order -- score descending / index ascending for the sort sampler, index ascending for the bisection sampler.

Band.  A draw is DECIDED when no cumulative boundary of the reference lies within delta of its u, and must then equal the reference
token; otherwise it must be one of the entries whose interval of the cumulative scale meets [u - delta, u + delta] (with one boundary
in reach: the two tokens either side of it; zero-probability entries are not part of the order).  delta is 4 x the largest gap,
over the case table, between the float64 cumulative sums and a rounded CPU model of the kernel's own (sort_model_cum: the fast exp,
sequential float32 sums of fp32(e / s); large_model_cum: 31-bit fixed-point weights with the 1-unit floor, integer sums) -- the rule of
oracle/kernel_cases.py, one delta per sampler.  The same gap is taken on the sums of the top-p stage, and the support margins
(row_ref's `margin`) are held against the same delta, so that the support is decided by the reference alone.
"""
import zlib

import numpy as np
import torch

from oracle.kernel_cases import mxl_hash32

_U32, _U64 = np.uint32, np.uint64
F32, F64 = np.float32, np.float64
M64 = (1 << 64) - 1
TWO24 = 1 << 24


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the uniform
# ----------------------------------------------------------------------------------------------------------------------------
def _u64(x):
    """python ints (any sign, taken modulo 2^64) or an integer array -> uint64 array"""
    if isinstance(x, np.ndarray):
        return x.astype(_U64)
    a = np.asarray(x, dtype=object)
    return np.array([int(v) & M64 for v in a.ravel()], dtype=_U64).reshape(a.shape)


def sampler_h2(seed, row, ctr, *, fault=None):
    """the 32-bit word of (seed, row, ctr); row and ctr broadcast.  `fault` plants a misreading of the formula (the CPU test's broken
    samplers): 'seed_hi' / 'ctr_hi' take the seed / the counter as 32-bit values"""
    seed = int(seed) & M64
    ctr = _u64(ctr)
    if fault == 'seed_hi':
        seed &= 0xFFFFFFFF
    if fault == 'ctr_hi':
        ctr = ctr & _U64(0xFFFFFFFF)
    lo_s, hi_s = seed & 0xFFFFFFFF, seed >> 32
    row = np.asarray(row).astype(_U32)
    with np.errstate(over='ignore'):
        g = ((ctr * _U64(0x9E3779B97F4A7C15)) >> _U64(32)).astype(_U32)
        h1 = mxl_hash32(g ^ mxl_hash32(row + _U32((0x85ebca6b * lo_s) & 0xFFFFFFFF)))
        return mxl_hash32(h1 + ctr.astype(_U32) + _U32(hi_s))


def sampler_u24(seed, row, ctr, *, fault=None):
    """j = h2 >> 8 as int64: the 24 bits both kernels turn into u = j / 2^24 (exact in float32 and in float64)"""
    return (sampler_h2(seed, row, ctr, fault=fault) >> _U32(8)).astype(np.int64)


def sampler_u(seed, row, ctr, *, fault=None):
    return sampler_u24(seed, row, ctr, fault=fault).astype(F64) / TWO24


def mix_seed(base_seed, step, rank=0):
    """ops.mix_seed restated (the decoder lanes and the step seeds come from it)"""
    x = (base_seed * 0x9E3779B97F4A7C15 + rank * 0xD1B54A32D192ED03 + step * 0x2545F4914F6CDD1D) & M64
    x ^= x >> 32
    x = (x * 0xD6E8FEB86659FD93) & M64
    x ^= x >> 32
    return x & 0x7FFFFFFFFFFFFFFF


# the sweep of part 2: one launch per (ctr, seed), all rows in it
SWEEP_B = 70
SWEEP_CTRS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, -1]
SWEEP_SEEDS = [0, 1, 77, 1 << 32, (1 << 32) + 77, 1234, 1234 + 7919, mix_seed(77, 3)]
LANE_STRIDE = 7919                 # generate.py: decoder lane i draws with seed + 7919 * i


def end_counters(seed=77, rows=4, n=1 << 22, edge=4):
    """counters below n at which a row's j sits at an end of the scale: -> [(row, ctr, j)] with j < edge, [(row, ctr, j)] with
    j >= 2^24 - edge"""
    j = sampler_u24(seed, np.arange(rows)[:, None], np.arange(n, dtype=np.int64)[None, :])
    lo = [(int(r), int(c), int(j[r, c])) for r, c in zip(*np.nonzero(j < edge))]
    hi = [(int(r), int(c), int(j[r, c])) for r, c in zip(*np.nonzero(j >= TWO24 - edge))]
    return lo, hi


# ----------------------------------------------------------------------------------------------------------------------------
# 2. inputs on which the kernels' arithmetic is exact
# ----------------------------------------------------------------------------------------------------------------------------
def _scattered(V, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(V, generator=g)[:n].sort().values.numpy()


def exact_cases():
    """name -> dict(large, V, top_k, row (V,) f32, token(h2) -> the token the word h2 must give).
    Sort sampler: equal scores give e = 1, s = N (a power of two), p = 1 / N and an exact running sum; ties order by index.
    Bisection sampler: equal scores weigh 2^31 each, u * tot = j * N * 2^7 is an exact integer, the crossing is floor(j N / 2^24)."""
    out = {}

    def add(name, large, V, top_k, row, token):
        out[name] = dict(name=name, large=large, V=V, top_k=top_k, row=torch.from_numpy(row.astype(F32)), token=token)

    flat = lambda V: np.full(V, -np.log(V))
    add('sort_bitonic_v2048', False, 2048, 0, flat(2048), lambda h2: (h2 >> _U32(21)).astype(np.int64))
    idx = _scattered(1190, 1024, 1)
    row = np.full(1190, -np.inf); row[idx] = -1.5
    add('sort_padded_v1190', False, 1190, 0, row, lambda h2, idx=idx: idx[(h2 >> _U32(22)).astype(np.int64)])
    idx = _scattered(1190, 64, 2)
    row = -3.0 - np.linspace(0.25, 4.0, 1190); row[idx] = -1.5
    add('sort_argmax_v1190_k64', False, 1190, 64, row, lambda h2, idx=idx: idx[(h2 >> _U32(26)).astype(np.int64)])
    for V in (2049, 4099, 262144):
        add(f'large_flat_v{V}', True, V, 0, flat(V), lambda h2, V=V: ((h2 >> _U32(8)).astype(np.int64) * V) >> 24)
    idx = _scattered(4099, 1500, 3)
    row = np.full(4099, -np.inf); row[idx] = -2.0
    add('large_subset_v4099', True, 4099, 0, row, lambda h2, idx=idx: idx[((h2 >> _U32(8)).astype(np.int64) * len(idx)) >> 24])
    return out


def end_row(V=2048, seed=5):
    """the non-uniform full-support row of the end-of-scale runs: log_softmax(randn * 2.5)"""
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(V, generator=g) * 2.5, -1)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. real distributions
# ----------------------------------------------------------------------------------------------------------------------------
CASE_SEED = (0x51ED27 << 32) | 1234          # both halves of the seed in use
CASE_CTRS = [0, 1, (1 << 32) + 1, -1]        # both halves of the counter in use
N_ROWS = 4                                   # distinct rows of a case; row b of the batch is distinct row b % 4
TH = 40                                      # history length of the repetition-penalty cases
EPS_DEV = 1e-4                               # typical-p: the deviations |-log p - H| are trusted to this (float32 sums of V terms
                                             # and the fast log / exp err by 1e-6 .. 1e-5 on values of a few nats)


def _c(name, large, V, sigma, *, k=0, p=1.0, typ=1.0, temp=1.0, rp=1.0, B=256, ninf=0, tie=False, tie_k=False, reseed=0):
    return dict(name=name, large=large, V=V, sigma=sigma, k=k, p=p, typ=typ, temp=temp, rp=rp, B=B, ninf=ninf, tie=tie, tie_k=tie_k,
                reseed=reseed)


# The warper settings are those of tests/test_decode_gpu.py and tests/test_large_vocab_gpu.py.  Sort sampler paths: arg-max
# (0 < k <= 64), bitonic (k = 0 or k > 64), bitonic with typical-p.
CASES = [
    _c('s_v2_full', False, 2, 1.0),
    _c('s_v1190_k8', False, 1190, 2.0, k=8, tie=True),
    _c('s_v1190_k50_p05_t13', False, 1190, 2.0, k=50, p=0.5, temp=1.3),
    _c('s_v1190_k8_tiek', False, 1190, 2.5, k=8, tie_k=True),
    _c('s_v1190_p09_t07', False, 1190, 1.5, p=0.9, temp=0.7),
    _c('s_v1190_ninf_rp13', False, 1190, 2.0, rp=1.3, ninf=400),
    _c('s_v1190_typ06', False, 1190, 2.5, typ=0.6),
    _c('s_v1190_rp12_typ09_k64_p09_t08', False, 1190, 2.5, rp=1.2, typ=0.9, k=64, p=0.9, temp=0.8),
    _c('s_v1190_typ02_k16_t14', False, 1190, 2.5, typ=0.2, k=16, temp=1.4),
    _c('s_v1190_rp15_typ095_p07', False, 1190, 2.5, rp=1.5, typ=0.95, p=0.7),
    _c('s_v1190_ninf_s1', False, 1190, 1.0, ninf=900, tie=True),
    _c('s_v2048_full', False, 2048, 2.5),
    _c('s_v2048_s6_k200_p097_t2', False, 2048, 6.0, k=200, p=0.97, temp=2.0, tie=True),
    _c('s_v1190_s6_k64', False, 1190, 6.0, k=64),
    _c('s_v2048_k500_p05_t09', False, 2048, 2.5, k=500, p=0.5, temp=0.9),
    _c('s_v2048_ninf_typ06', False, 2048, 1.0, ninf=1500, typ=0.6, reseed=1),
    _c('s_v2048_k64_s1', False, 2048, 1.0, k=64),
    _c('l_v1190_k8', True, 1190, 2.5, k=8, tie=True),
    _c('l_v1190_rp13', True, 1190, 2.5, rp=1.3),
    _c('l_v1190_rp12_typ09_k64_p09_t08', True, 1190, 2.5, rp=1.2, typ=0.9, k=64, p=0.9, temp=0.8),
    _c('l_v1190_ninf_s1', True, 1190, 1.0, ninf=900, tie=True),
    _c('l_v2049_full', True, 2049, 2.5),
    _c('l_v2049_s6_full', True, 2049, 6.0),
    _c('l_v2049_typ06', True, 2049, 2.5, typ=0.6),
    _c('l_v2049_k8_tiek', True, 2049, 1.0, k=8, tie_k=True),
    _c('l_v32773_k500_p05_t09', True, 32773, 2.5, k=500, p=0.5, temp=0.9),
    _c('l_v32773_s4_full', True, 32773, 4.0, tie=True),
    _c('l_v32773_ninf_rp15_typ095_p07', True, 32773, 2.5, ninf=30000, rp=1.5, typ=0.95, p=0.7),
    _c('l_v262144_k64_p09', True, 262144, 2.5, k=64, p=0.9, B=8),
]
CASE = {c['name']: c for c in CASES}


def case_inputs(c):
    """-> rows (4, V) f32 scores, hist (4, TH) int64 (the ids the repetition penalty reads)"""
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()) + c['reseed'])
    V = c['V']
    rows = torch.log_softmax(torch.randn(N_ROWS, V, generator=g) * c['sigma'], -1)
    if c['ninf']:                                            # barred tokens, as rules_mask leaves them
        for r in range(N_ROWS):
            rows[r, torch.randperm(V, generator=g)[:c['ninf']]] = float('-inf')
    hist = torch.randint(0, V, (N_ROWS, TH), generator=g)
    hist[:, 5] = hist[:, 6]
    if V > 8:
        hist[0, :8] = rows[0].topk(8).indices               # the penalty hits the head of row 0
    if c['tie'] and V > 8:                                   # an exact tie inside any support: row 1's second and third scores
        top = rows[1].topk(3).indices
        rows[1, top[2]] = rows[1, top[1]]
    if c['tie_k']:                                           # row 2: the k-th and the (k+1)-th score tie, the lower index stays
        top = rows[2].topk(c['k'] + 1).indices
        rows[2, top[c['k']]] = rows[2, top[c['k'] - 1]]
    return rows, hist


def kernel_scores(row, temp, rp, hist):
    """the float32 scores both kernels order by: row * (1 / temperature), and for every id of the history the raw score times
    (score < 0) or over (score >= 0) the penalty, then times 1 / temperature"""
    row = np.asarray(row, dtype=F32)
    invt = F32(1.0) / F32(temp)
    k = (row * invt).astype(F32)
    if rp != 1.0:
        rp = F32(rp)
        for tok in np.unique(np.asarray(hist)):
            if 0 <= tok < len(row):
                v = row[tok]
                k[tok] = F32(F32(v * rp if v < 0 else v / rp) * invt)
    return k


def fast_exp32(x):
    """the device's fast exponential: a float32 exp2 of the float32 product x * log2(e)"""
    return np.exp2((np.asarray(x, dtype=F32) * F32(1.4426950408889634)).astype(F32)).astype(F32)


def sort_model_cum(k32, tokens, head):
    """sort sampler, rounded: e = fast_exp(k - key[0]), s their sequential float32 sum, running float32 sum of fp32(e / s)"""
    e = fast_exp32(k32[tokens] - F32(head))
    s = np.cumsum(e, dtype=F32)[-1]
    return np.cumsum((e / s).astype(F32), dtype=F32).astype(F64)


def large_model_cum(k32, tokens, m):
    """bisection sampler, rounded: weights max(1, trunc(fast_exp(k - max) * 2^31)), integer sums"""
    w = np.maximum(1, (fast_exp32(k32[tokens] - F32(m)).astype(F64) * 2147483648.0).astype(np.int64))
    c = np.cumsum(w)
    return c.astype(F64) / float(c[-1])


def _softmax64(k32, keep):
    z = np.where(keep, k32.astype(F64), -np.inf)
    e = np.exp(z - z.max())
    return e / e.sum()


def row_ref(c, row, hist):
    """float64 reference of one distinct row -> dict(k32, keep (V,) bool, p (V,) f64, order: the support's tokens in the sampler's
    order, cum: their inclusive cumulative sums, margin: how far the support's own decisions are from turning over, tie_at_k, gap:
    the largest distance between `cum` (and the top-p stage's sums) and the kernel's rounded model)"""
    V = c['V']
    k32 = kernel_scores(row, c['temp'], c['rp'], hist)
    idx = np.arange(V)
    by_score = np.lexsort((idx, -k32.astype(F64)))           # score descending, ties by ascending index; -inf last
    head, m = k32[by_score[0]], k32.max()
    model = (lambda toks: large_model_cum(k32, toks, m)) if c['large'] else (lambda toks: sort_model_cum(k32, toks, head))
    keep = np.isfinite(k32)
    margin, tie_at_k, gap = np.inf, False, 0.0
    if 0 < c['k'] < V:
        kept = by_score[:c['k']]
        tie_at_k = bool(k32[by_score[c['k'] - 1]] == k32[by_score[c['k']]])
        keep = np.zeros(V, bool); keep[kept] = True; keep &= np.isfinite(k32)
    if 0.0 < c['p'] < 1.0:
        tp = float(F32(c['p']))
        toks = by_score[keep[by_score]]
        cum = np.cumsum(_softmax64(k32, keep)[toks])
        before = cum - _softmax64(k32, keep)[toks]
        n = min(int((before < tp).sum()) + 1, len(toks))     # the sort sampler's walk ends at the crossing: sums up to the first dropped entry
        gap = max(gap, np.abs(model(toks)[:n] - cum[:n]).max())
        margin = min(margin, np.abs(before[1:] - tp).min() if len(toks) > 1 else np.inf)
        keep = np.zeros(V, bool); keep[toks[before < tp]] = True
    if 0.0 < c['typ'] < 1.0:
        ty = float(F32(c['typ']))
        p = _softmax64(k32, keep)
        toks = by_score[keep[by_score]]                      # ties of the deviation: by position in the order = by index
        pt = p[toks]
        nl = np.log(pt)
        dev = np.abs(-nl - (-(pt * nl).sum()))
        o = np.argsort(dev, kind='stable')
        ds, ms = dev[o], pt[o]
        cs = np.concatenate([[0.0], np.cumsum(ms)])
        before = np.empty(len(toks)); before[o] = cs[:-1]
        stay = before < ty
        # the same decision with every deviation moved by up to EPS_DEV: the mass that can at most / must at least lie before
        hi = cs[np.searchsorted(ds, ds + 2 * EPS_DEV, 'left')] - ms
        lo = cs[np.searchsorted(ds, ds - 2 * EPS_DEV, 'right')]
        mg = np.empty(len(toks)); mg[o] = np.where(stay[o], ty - hi, lo - ty)
        margin = min(margin, mg.min())
        keep = np.zeros(V, bool); keep[toks[stay]] = True
    p = _softmax64(k32, keep)
    order = idx[keep] if c['large'] else by_score[keep[by_score]]
    cum = np.cumsum(p[order])
    gap = max(gap, np.abs(model(order) - cum).max())
    return dict(k32=k32, keep=keep, p=p, order=order, cum=cum, margin=float(margin), tie_at_k=tie_at_k, gap=float(gap))


_REFS = {}


def case_ref(name):
    """the references of a case's four distinct rows, computed once and shared"""
    if name not in _REFS:
        c = CASE[name]
        rows, hist = case_inputs(c)
        _REFS[name] = [row_ref(c, rows[r].numpy(), hist[r].numpy()) for r in range(N_ROWS)]
    return _REFS[name]


def case_u(c, *, fault=None):
    """-> u (len(CASE_CTRS), B): the uniform of every (launch, row) of the case"""
    return sampler_u(CASE_SEED, np.arange(c['B'])[None, :], _u64(CASE_CTRS)[:, None], fault=fault)


def ref_position(cum, u):
    """index into the order of the first entry whose inclusive cumulative sum exceeds u (the last one if none does)"""
    return np.minimum(np.searchsorted(cum, u, 'right'), len(cum) - 1)


def judge(tokens, ref, u, delta):
    """tokens, u: (n,) draws of one distinct row -> (decided, undecided, bad): the counts, and the indices of the draws that are
    neither the reference token of a decided draw nor within the band of an undecided one"""
    order, cum = ref['order'], ref['cum']
    pos = np.full(int(max(order.max(), np.max(tokens), 0)) + 2, -1, dtype=np.int64)
    pos[order] = np.arange(len(order))
    got = pos[np.clip(tokens, -1, len(pos) - 2)]
    lo, hi, want = ref_position(cum, u - delta), ref_position(cum, u + delta), ref_position(cum, u)
    decided = lo == hi
    ok = np.where(decided, got == want, (got >= lo) & (got <= hi))
    return int(decided.sum()), int((~decided).sum()), np.nonzero(~ok)[0]


def judge_case(name, tokens, delta, u=None):
    """tokens (len(CASE_CTRS), B) of a whole case -> (decided, undecided, [(launch, row, got, want)])"""
    c = CASE[name]
    u = case_u(c) if u is None else u
    nd = nu = 0
    bad = []
    for r, ref in enumerate(case_ref(name)):
        t, uu = np.asarray(tokens)[:, r::N_ROWS], u[:, r::N_ROWS]
        d, n, b = judge(t.ravel(), ref, uu.ravel(), delta)
        nd, nu = nd + d, nu + n
        for i in b:
            li, bi = divmod(int(i), t.shape[1])
            bad.append((li, r + N_ROWS * bi, int(t[li, bi]), int(ref['order'][ref_position(ref['cum'], uu[li, bi])])))
    return nd, nu, bad


def model_tokens(name, *, fault=None):
    """what a sampler that follows the reference draws on a case: (len(CASE_CTRS), B) tokens.  `fault` plants a wrong sampler:
    'row0' (every row draws row 0's u), 'seed_hi', 'ctr_hi', 'shift' (the walk stops one entry late), 'halfj' (j >> 1 for j),
    'reversed' (the order walked backwards)"""
    c = CASE[name]
    u = case_u(c, fault=fault if fault in ('seed_hi', 'ctr_hi') else None)
    if fault == 'row0':
        u = np.repeat(u[:, :1], c['B'], 1)
    if fault == 'halfj':
        u = np.floor(u * TWO24 / 2) / TWO24
    out = np.empty(u.shape, dtype=np.int64)
    for r, ref in enumerate(case_ref(name)):
        order, p = ref['order'], ref['p']
        if fault == 'reversed':
            order = order[::-1]
        at = ref_position(np.cumsum(p[order]), u[:, r::N_ROWS])
        if fault == 'shift':
            at = np.minimum(at + 1, len(order) - 1)
        out[:, r::N_ROWS] = order[at]
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 4. chi-square thresholds
# ----------------------------------------------------------------------------------------------------------------------------
def chi2_limit(df, tail=1e-6):
    """the chi-square quantile at upper-tail probability `tail`: scipy's where it is importable, else Wilson-Hilferty"""
    try:
        from scipy import stats
        return float(stats.chi2.isf(tail, df))
    except ImportError:
        assert tail == 1e-6
        z = 4.753424308822899                                # upper 1e-6 quantile of the normal distribution
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3


def chi2_uniform(counts):
    counts = np.asarray(counts, dtype=F64)
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def chi2_independence(a, b, n=16):
    """the contingency statistic of two arrays of cell numbers below n ((n - 1)^2 degrees of freedom)"""
    t = np.bincount(np.asarray(a).ravel() * n + np.asarray(b).ravel(), minlength=n * n).reshape(n, n).astype(F64)
    e = t.sum(1, keepdims=True) * t.sum(0, keepdims=True) / t.sum()
    return float(((t - e) ** 2 / e).sum())
