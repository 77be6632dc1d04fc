"""The host statement of beam-sample's draw (mxl_beam_sample_draw, include/musicxl.h) and of its step (mxl_beam_sample_step) that the
tests stand on: the candidate's hash word integer-exact, the warp with min_tokens_to_keep = 2 in float64, z = w - log(-log u) in
float64, the drawn set with its band, `ref_sample_step` (tests.beam_ref.ref_step under the replace-score rule), the case table of the
kernel test, and a rounded CPU model of the kernel's own float32 arithmetic from which the tolerances come.

Reference.  The scores a row is ordered by are fp32(row * fp32(1 / temperature)), as oracle/sampler_cases.py takes them; they give
the order and the ties.  Everything after is float64: top-k keeps the first max(k, 2) of the order, top-p an entry iff the mass ordered
before it is below top_p (and the two best), typical-p the same in the order |-log p - H| ascending (and its first two), then
w = log of the renormalised probability.  `margin` says how far the support's own decisions are from turning over.

Tolerances.  DELTA_W and DELTA_Z are 4 x the largest gap, over the case table, between the float64 values and the rounded model
(`warp_model`, `gumbel_model`: the fast exp2 / log2 forms, the scan and the reductions in the kernel's order) -- the rule of
oracle/kernel_cases.py.  They are computed on the CPU, never from device output; tests/test_beam_sample_cpu.py recomputes the gaps and
holds the recorded ones against them.

Band.  An item is DECIDED when it has at most 2 * nb finite candidates, or when the 2 * nb-th and the next z lie more than
2 * DELTA_Z apart: no z is then within DELTA_Z of the cut between them, and the drawn set must be the reference's.  Otherwise the set
holds every candidate above cut + DELTA_Z and none below cut - DELTA_Z."""
import zlib

import numpy as np
import torch

from oracle.kernel_cases import mxl_hash32
from oracle.sampler_cases import EPS_DEV, fast_exp32, sampler_h2
from tests import beam_ref

_U32 = np.uint32
F32, F64 = np.float32, np.float64
NEG = float('-inf')
SORT_N, THREADS = 2048, 256                     # csrc/beam_sample.hip: the LDS sort and the workgroup
PER_THREAD = SORT_N // THREADS

# the gaps the tolerances come from: the largest |model - float64| over CASES (test_beam_sample_cpu.py::test_recorded_gaps)
GAP_W = 1.6e-6                                  # w, and the top-p stage's normalised sums: measured 1.58e-6 (vm_t07_nb16)
GAP_Z = 2.4e-6                                  # z = w + Gumbel term: measured 2.32e-6 (vm_t07_nb16)
DELTA_W, DELTA_Z = 4 * GAP_W, 4 * GAP_Z


# ---------------------------------------------------------------------------------------------------------------- 1. the word
def cand_word(seed, ctr, row, v, *, fault=None):
    """the 32-bit word of candidate (global row, token): hash(h2(seed, row, ctr) ^ (v * 0x9E3779B1 + 0x85EBCA77)), h2 the samplers'
    row word; row and v broadcast.  fault: 'seed_hi' / 'ctr_hi' (the seed / the counter taken as 32 bits), 'no_row' (the row left
    out: every row draws row 0's words)"""
    row = np.asarray(row)
    if fault == 'no_row':
        row = np.zeros_like(row)
    h2 = sampler_h2(seed, row, ctr, fault=fault if fault in ('seed_hi', 'ctr_hi') else None)
    with np.errstate(over='ignore'):
        return mxl_hash32(h2 ^ (np.asarray(v).astype(_U32) * _U32(0x9E3779B1) + _U32(0x85EBCA77)))


def gumbel64(word):
    """-log(-log u), u = (j + 0.5) / 2^24, j = word >> 8, in float64"""
    u = ((np.asarray(word) >> _U32(8)).astype(F64) + 0.5) / float(1 << 24)
    return -np.log(-np.log(u))


def gumbel_model(word):
    """the kernel's float32 form: below one half -log(u) with u = (2j + 1) / 2^25 exact, above it -log1p(-(1 - u)) with 1 - u exact"""
    j = (np.asarray(word) >> _U32(8)).astype(np.int64)
    lo = j < (1 << 23)
    a = (2 * j + 1).astype(F32) * F32(2.0 ** -25)
    b = (2 * ((1 << 24) - j) - 1).astype(F32) * F32(2.0 ** -25)
    with np.errstate(divide='ignore', invalid='ignore'):
        nlu = np.where(lo, -np.log(a), -np.log1p(-b)).astype(F32)
        return (-np.log(nlu)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- 2. the warp
def _order(row, temp):
    k32 = (np.asarray(row, dtype=F32) * (F32(1.0) / F32(temp))).astype(F32)
    return k32, np.lexsort((np.arange(len(k32)), -k32.astype(F64)))          # score descending, ties by index; -inf last


def warp_ref(row, k=0, p=1.0, typ=1.0, temp=1.0):
    """float64 reference of one row -> dict(w (V,) f64, -inf outside the support; margin; top_p: (positions, normalised mass before)
    of the top-p stage, for the gap)"""
    V = len(row)
    k32, order = _order(row, temp)
    sk = k32[order].astype(F64)
    w = np.full(V, NEG)
    if not np.isfinite(sk[0]):
        return dict(w=w, margin=np.inf, top_p=None)
    n = min(max(k, 2), V) if k > 0 else V
    e = np.exp(sk - sk[0])
    margin, stage = np.inf, None
    if 0.0 < p < 1.0:
        tp = float(F32(p))
        P = e[:n] / e[:n].sum()
        before = np.cumsum(P) - P
        out = np.nonzero(~(before < tp) & (np.arange(n) >= 2))[0]
        n2 = int(out[0]) if len(out) else n
        if n > 2:
            margin = min(margin, float(np.abs(before[2:] - tp).min()))
        stage = (np.arange(2, min(n2 + 1, n)), before[2:min(n2 + 1, n)])
        n = n2
    stay = np.ones(n, bool)
    if 0.0 < typ < 1.0:
        ty = float(F32(typ))
        pt = e[:n] / e[:n].sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            nl = np.log(pt)
            ent = -np.where(pt > 0, pt * nl, 0.0).sum()
            dev = np.abs(-nl - ent)
        o = np.argsort(dev, kind='stable')                     # ties of the deviation: by position in the order
        ds, ms = dev[o], pt[o]
        cs = np.concatenate([[0.0], np.cumsum(ms)])
        before, rank = np.empty(n), np.empty(n, dtype=np.int64)
        before[o], rank[o] = cs[:-1], np.arange(n)
        by_mass = before < ty
        stay = by_mass | (rank < 2)
        # the same decisions with every deviation moved by up to EPS_DEV: the mass / the count that can at most, must at least lie before
        at_hi, at_lo = np.searchsorted(ds, ds + 2 * EPS_DEV, 'left'), np.searchsorted(ds, ds - 2 * EPS_DEV, 'right')
        hi, lo = cs[at_hi] - ms, cs[at_lo]
        first_two = np.where(at_hi - 1 < 2, np.inf, 0.0)
        not_first = np.where(at_lo >= 2, np.inf, 0.0)
        mg = np.empty(n)
        mg[o] = np.where(stay[o], np.maximum(ty - hi, first_two), np.minimum(lo - ty, not_first))    # stays: either reason holds
        mg[pt == 0] = np.inf                                    # a -inf entry is -inf either way
        margin = min(margin, float(mg.min()))
    sel = stay & np.isfinite(sk[:n])
    S = e[:n][sel].sum()
    w[order[:n][sel]] = (sk[:n][sel] - sk[0]) - np.log(S)
    return dict(w=w, margin=float(margin), top_p=stage)


def fast_log32(x):
    """the device's fast logarithm: a float32 log2 times ln 2"""
    with np.errstate(divide='ignore'):
        return (np.log2(np.asarray(x, dtype=F32)).astype(F32) * F32(0.6931471805599453)).astype(F32)


def block_scan_model(x):
    """bs_block_scan: the inclusive float32 sums of 2048 values in the kernel's order -- a running sum over the 8 values of a thread, a
    Hillis-Steele scan of the 64 thread totals of a wave, the wave totals added in wave order"""
    c = np.asarray(x, dtype=F32).reshape(THREADS, PER_THREAD).copy()
    for e in range(1, PER_THREAD):
        c[:, e] = c[:, e - 1] + c[:, e]
    t = c[:, -1].reshape(THREADS // 64, 64).copy()
    o = 1
    while o < 64:
        y = t.copy()
        t[:, o:] = y[:, :-o] + y[:, o:]
        o <<= 1
    excl = np.concatenate([np.zeros((t.shape[0], 1), F32), t[:, :-1]], 1)
    woff = np.zeros(t.shape[0], F32)
    for w in range(1, t.shape[0]):
        woff[w] = woff[w - 1] + t[w - 1, 63]
    off = (woff[:, None] + excl).astype(F32).reshape(THREADS, 1)
    return (off + c).astype(F32).reshape(SORT_N)


def block_sum_model(parts):
    """bs_block_sum: 256 thread values -> a butterfly inside each wave, then the four waves in order"""
    x = np.asarray(parts, dtype=F32).reshape(THREADS // 64, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[:, lane ^ o]).astype(F32)
    return F32(F32(F32(x[0, 0] + x[1, 0]) + x[2, 0]) + x[3, 0])


def _thread_sums(vals):
    """the running float32 sum every thread forms over its 8 positions"""
    c = np.asarray(vals, dtype=F32).reshape(THREADS, PER_THREAD)
    s = np.zeros(THREADS, F32)
    for e in range(PER_THREAD):
        s = (s + c[:, e]).astype(F32)
    return s


def warp_model(row, k=0, p=1.0, typ=1.0, temp=1.0):
    """the kernel's own arithmetic, rounded as it rounds -> dict(w (V,) f32, top_p: the normalised sums of the top-p stage)"""
    V = len(row)
    k32, order = _order(row, temp)
    w = np.full(V, NEG, dtype=F32)
    key = np.full(SORT_N, NEG, dtype=F32)
    key[:V] = k32[order]
    m = key[0]
    if not np.isfinite(m):
        return dict(w=w, top_p=None)
    pos = np.arange(SORT_N)
    n = min(max(k, 2), V) if k > 0 else V
    with np.errstate(invalid='ignore'):
        d = (key - m).astype(F32)
    e = np.where(pos < n, fast_exp32(d), F32(0)).astype(F32)
    cum = block_scan_model(e)
    stage = None
    if 0.0 < p < 1.0:
        thr = F32(F32(p) * cum[n - 1])
        i = np.arange(2, n)
        out = i[~(cum[i - 1] < thr)]
        n2 = int(out[0]) if len(out) else n
        i = np.arange(2, min(n2 + 1, n))
        stage = (i, cum[i - 1].astype(F64) / float(cum[n - 1]))
        n = n2
    S = cum[n - 1]
    drop = np.zeros(SORT_N, bool)
    if 0.0 < typ < 1.0:
        logs = fast_log32(S)
        with np.errstate(invalid='ignore'):
            nl = (d - logs).astype(F32)
        pp = np.where(pos < n, fast_exp32(nl), F32(0)).astype(F32)
        with np.errstate(invalid='ignore'):
            term = np.where((pos < n) & (pp > 0), (pp * nl).astype(F32), F32(0)).astype(F32)
        c = term.reshape(THREADS, PER_THREAD)
        part = np.zeros(THREADS, F32)
        for x in range(PER_THREAD):
            part = (part - c[:, x]).astype(F32)
        ent = block_sum_model(part)
        with np.errstate(invalid='ignore'):
            dv = np.abs(((-nl).astype(F32) - ent).astype(F32))
        before, rank = np.zeros(n, F32), np.zeros(n, np.int64)
        di, at = dv[:n], pos[:n]
        for j in range(n):
            ahead = (dv[j] < di) | ((dv[j] == di) & (j < at))
            before = (before + np.where(ahead, pp[j], F32(0))).astype(F32)
            rank += ahead
        drop[:n] = (rank >= 2) & ~(before < F32(typ))
        S = block_sum_model(_thread_sums(np.where((pos < n) & ~drop, e, F32(0))))
    logS = fast_log32(S)
    sel = (pos < n) & ~drop & np.isfinite(key)
    w[order[pos[sel]]] = (d[sel] - logS).astype(F32)
    return dict(w=w, top_p=stage)


# ---------------------------------------------------------------------------------------------------------------- 3. the draw
def z_of(w, words):
    """z = w + Gumbel term in float64, -inf where w is"""
    w = np.asarray(w, dtype=F64)
    return np.where(np.isfinite(w), w + gumbel64(words), NEG)


def draw_ref(w, words, nb, delta=DELTA_Z):
    """w, words (rows, V) -> per item dict(want: the reference's drawn flat indices j * V + v (sorted), decided, must, may: the
    sets an undecided item's draw lies between)"""
    rows, V = w.shape
    z = z_of(w, words).reshape(rows // nb, nb * V)
    out = []
    for zi in z:
        fin = np.nonzero(np.isfinite(zi))[0]
        o = fin[np.lexsort((fin, -zi[fin]))]
        if len(o) <= 2 * nb:
            out.append(dict(want=sorted(o.tolist()), decided=True, must=set(o.tolist()), may=set(o.tolist())))
            continue
        a, b = zi[o[2 * nb - 1]], zi[o[2 * nb]]
        cut = (a + b) / 2
        out.append(dict(want=sorted(o[:2 * nb].tolist()), decided=bool(a - b > 2 * delta),
                        must=set(fin[zi[fin] > cut + delta].tolist()), may=set(fin[zi[fin] >= cut - delta].tolist())))
    return out


def judge_item(ref, got, nb):
    """got: the flat indices an implementation drew for the item -> None, or what is wrong with them"""
    got = sorted(int(x) for x in got)
    if ref['decided']:
        return None if got == ref['want'] else f'decided item: drew {got}, the reference {ref["want"]}'
    s = set(got)
    if len(s) != 2 * nb or not ref['must'] <= s or not s <= ref['may']:
        return f'undecided item: drew {got}, outside the band {sorted(ref["must"])} .. {sorted(ref["may"])}'
    return None


def drawn_matrix(w, sets, nb, ldl, fill=7.0):
    """the `drawn` matrix of the reference: w (f32) at the drawn candidates, -inf elsewhere in columns 0..V-1, `fill` beyond"""
    rows, V = w.shape
    out = torch.full((rows, ldl), fill, dtype=torch.float32)
    out[:, :V] = NEG
    w32 = torch.from_numpy(np.asarray(w, dtype=F32))
    for b, s in enumerate(sets):
        for f in s:
            out[b * nb + f // V, f % V] = w32[b * nb + f // V, f % V]
    return out


# ---------------------------------------------------------------------------------------------------------------- 4. the step
def ref_sample_step(st: beam_ref.RefState, drawn: torch.Tensor, V: int, cur_len: int, eos: int, pad: int, lp: float, early: bool):
    """one mxl_beam_sample_step on the host: tests.beam_ref.ref_step under the replace-score rule -- a candidate's score is its entry
    of `drawn` itself, -inf in a row whose running score is -inf.  ref_step adds the running score, so the step runs over running
    scores of +0 (-inf stays -inf): x + 0 is x bit for bit, and -inf + anything finite is -inf.  A frozen item keeps its scores."""
    saved, frozen = st.scores.clone(), list(st.done)
    st.scores = torch.where(saved == NEG, saved, torch.zeros_like(saved))
    out = beam_ref.ref_step(st, drawn, V, cur_len, eos, pad, lp, early)
    for b, f in enumerate(frozen):
        if f:
            st.scores[b * st.nb:(b + 1) * st.nb] = saved[b * st.nb:(b + 1) * st.nb]
    return out


# ---------------------------------------------------------------------------------------------------------------- 5. the case table
MUSIC_V = 1190                                   # the degree vocabulary (tests/test_key_rule_gpu.py)
CASE_SEED = (0x51ED27 << 32) | 1234              # both halves of the seed in use
CASE_CTRS = [(1 << 32) + 1, (0x7A31 << 32) | 99, (1 << 63) + 5, (3 << 32) | 0xFFFFFFFF]      # and of the counter
NONE = dict(k=0, p=1.0, typ=1.0, temp=1.0)
ALL = dict(k=100, p=0.9, typ=0.9, temp=0.7)


def _c(name, Bs, nb, V, sigma, special=False, **warp):
    return dict(name=name, Bs=Bs, nb=nb, V=V, sigma=sigma, special=special, warp={**NONE, **warp})


# special: in every item row 1 has a single allowed token and the last row is dead; in item 0 every live row has a single allowed
# token, so that the item has fewer than 2 * nb finite candidates
CASES = [
    _c('v2_none', 3, 2, 2, 1.0),
    _c('v2_all_special', 3, 3, 2, 1.0, special=True, **ALL),
    _c('v37_k1', 5, 3, 37, 2.0, k=1),
    _c('v37_all_nb16', 3, 16, 37, 2.0, special=True, k=8, p=0.9, typ=0.9, temp=0.7),
    _c('vm_none', 3, 3, MUSIC_V, 2.0),
    _c('vm_k8', 5, 2, MUSIC_V, 2.5, k=8),
    _c('vm_k100', 1, 3, MUSIC_V, 2.5, k=100),
    _c('vm_p09', 3, 3, MUSIC_V, 2.0, p=0.9),
    _c('vm_typ09', 3, 2, MUSIC_V, 2.5, typ=0.9),
    _c('vm_t07_nb16', 1, 16, MUSIC_V, 2.0, temp=0.7),
    _c('vm_all_special', 3, 3, MUSIC_V, 2.5, special=True, **ALL),
    _c('vm_none_special', 5, 3, MUSIC_V, 1.0, special=True),
    _c('v2048_k0', 1, 3, 2048, 2.5, k=0),
    _c('v2048_all_special', 3, 2, 2048, 2.5, special=True, **ALL),
]
CASE = {c['name']: c for c in CASES}
_REFS = {}


def case_inputs(c):
    """-> logp (rows, V + 3) f32 (the columns beyond V hold 5.0, which nothing may read), beam_scores (rows,) f32, the counter"""
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    rows, V, nb = c['Bs'] * c['nb'], c['V'], c['nb']
    logp = torch.full((rows, V + 3), 5.0)
    logp[:, :V] = torch.log_softmax(torch.randn(rows, V, generator=g) * c['sigma'], -1)
    scores = -torch.rand(rows, generator=g) * 4
    if c['special']:
        for b in range(c['Bs']):
            single = range(nb - 1) if b == 0 else [1]
            for j in single:
                keep = int(torch.randint(0, V, (1,), generator=g))
                v = logp[b * nb + j, keep].item()
                logp[b * nb + j, :V] = NEG
                logp[b * nb + j, keep] = v
            scores[b * nb + nb - 1] = NEG
    return logp, scores, CASE_CTRS[zlib.crc32(c['name'].encode()) % len(CASE_CTRS)]


def case_words(c, ctr, *, fault=None):
    rows = c['Bs'] * c['nb']
    return cand_word(CASE_SEED, ctr, np.arange(rows)[:, None], np.arange(c['V'])[None, :], fault=fault)


def case_ref(name):
    """the float64 reference of a case, computed once and shared: dict(w (rows, V) f64, margin (rows,), items: draw_ref's list, logp,
    scores, ctr)"""
    if name not in _REFS:
        c = CASE[name]
        logp, scores, ctr = case_inputs(c)
        live = (scores != NEG).numpy()
        refs = [warp_ref(logp[r, :c['V']].numpy(), **c['warp']) if live[r] else dict(w=np.full(c['V'], NEG), margin=np.inf)
                for r in range(logp.shape[0])]
        w = np.stack([r['w'] for r in refs])
        _REFS[name] = dict(w=w, margin=np.array([r['margin'] for r in refs]), items=draw_ref(w, case_words(c, ctr), c['nb']),
                           logp=logp, scores=scores, ctr=ctr, live=live)
    return _REFS[name]


def model_sets(name, *, fault=None):
    """what an implementation that follows the reference draws on a case (the flat indices per item), with the words of `fault`"""
    c, ref = CASE[name], case_ref(name)
    return [it['want'] for it in draw_ref(ref['w'], case_words(c, ref['ctr'], fault=fault), c['nb'])]


def case_gaps(name):
    """-> (gap_w, gap_z, rows whose model support differs from the reference's): the largest |model - float64| of w and of the top-p
    stage's sums, and of z, over the live rows of the case whose supports agree"""
    c, ref = CASE[name], case_ref(name)
    words = case_words(c, ref['ctr'])
    gw = gz = 0.0
    differ = []
    for r in range(ref['w'].shape[0]):
        if not ref['live'][r]:
            continue
        row = ref['logp'][r, :c['V']].numpy()
        want, got = warp_ref(row, **c['warp']), warp_model(row, **c['warp'])
        fin = np.isfinite(want['w'])
        if not np.array_equal(fin, np.isfinite(got['w'])):
            differ.append(r)
            continue
        if want['top_p'] is not None:
            n = min(len(want['top_p'][1]), len(got['top_p'][1]))
            if n:
                gw = max(gw, float(np.abs(want['top_p'][1][:n] - got['top_p'][1][:n]).max()))
        gw = max(gw, float(np.abs(want['w'][fin] - got['w'][fin].astype(F64)).max()))
        zm = (got['w'][fin] + gumbel_model(words[r][fin])).astype(F32)
        gz = max(gz, float(np.abs(zm.astype(F64) - z_of(want['w'], words[r])[fin]).max()))
    return gw, gz, differ
