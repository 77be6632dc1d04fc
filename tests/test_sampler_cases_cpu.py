"""CPU side of the samplers' draw tests (no GPU): the conditions oracle/sampler_cases.py promises of its case table -- the rounded-model
gaps behind DELTA_SORT / DELTA_LARGE of tests/test_sampler_cases_gpu.py measured again, the support margins, the share of undecided
draws -- the teeth of the token-for-token checker, and the soundness of the uniform's stream on the host model that the GPU test
pins to the device bit for bit.

Measured here (largest gap over the case table -> delta = 4 x, rounded up):

    sort sampler        1.40e-6   s_v1190_ninf_rp13     -> DELTA_SORT  5.6e-6
    bisection sampler   4.18e-7   l_v32773_s4_full      -> DELTA_LARGE 1.7e-6

The smallest support margin is 6.4e-5 (sort) / 1.4e-5 (bisection); the largest share of undecided draws is 1.76 % (s_v2048_full: 2048
boundaries, each with a band of 2 delta, less what the small entries share) against the cap of 2 %.
"""
import numpy as np
import pytest

from oracle import sampler_cases as S
from oracle.kernel_cases import check_gap
from tests.test_sampler_cases_gpu import CAP, DELTA_LARGE, DELTA_SORT

NAMES = [c['name'] for c in S.CASES]
FAULTS = ['row0', 'seed_hi', 'ctr_hi', 'shift', 'halfj', 'reversed']


def _delta(c):
    return DELTA_LARGE if c['large'] else DELTA_SORT


# ---------------------------------------------------------------------------------------------------------------- the model itself
def test_uniform_model_against_plain_python():
    """the vectorised numpy statement against the formula written with python integers"""
    def h32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)

    for seed in S.SWEEP_SEEDS:
        for ctr in S.SWEEP_CTRS:
            c = ctr & S.M64
            want = []
            for row in range(S.SWEEP_B):
                h1 = h32((((c * 0x9E3779B97F4A7C15) & S.M64) >> 32) ^ h32(row + 0x85ebca6b * (seed & 0xFFFFFFFF)))
                want.append(h32(h1 + (c & 0xFFFFFFFF) + (seed >> 32)) >> 8)
            got = S.sampler_u24(seed, np.arange(S.SWEEP_B), [ctr] * S.SWEEP_B)
            assert got.tolist() == want, (seed, ctr)
    assert S.mix_seed(77, 3) == __import__('symbolic_music_generation_amd.ops', fromlist=['mix_seed']).mix_seed(77, 3)


def test_exact_inputs_agree_with_the_reference_walk():
    """the closed-form tokens of part 2 (top bits of h2) are what the float64 walk of part 3 gives on the same rows"""
    h2 = S.sampler_h2(77, np.arange(64)[None, :], S._u64(list(range(64)))[:, None]).ravel()
    u = (h2 >> np.uint32(8)).astype(np.float64) / S.TWO24
    for name, x in S.exact_cases().items():
        if x['V'] > 5000:
            continue
        c = dict(large=x['large'], V=x['V'], k=x['top_k'], p=1.0, typ=1.0, temp=1.0, rp=1.0)
        ref = S.row_ref(c, x['row'].numpy(), [])
        want = ref['order'][S.ref_position(ref['cum'], u)]
        assert (x['token'](h2) == want).all(), name
        assert ref['gap'] <= 1e-9, (name, ref['gap'])       # and the rounded models are exact on them


def test_end_counters_exist():
    lo, hi = S.end_counters()
    assert len(lo) >= 1 and len(hi) >= 1, (lo, hi)
    assert all(j < 4 for _, _, j in lo) and all(j >= S.TWO24 - 4 for _, _, j in hi)


# ---------------------------------------------------------------------------------------------------------------- the case table
def test_case_table_covers_what_it_should():
    sort = [c for c in S.CASES if not c['large']]
    large = [c for c in S.CASES if c['large']]
    assert {c['V'] for c in sort} == {2, 1190, 2048} and {c['V'] for c in large} == {1190, 2049, 32773, 262144}
    assert {c['sigma'] for c in sort} >= {1.0, 2.5, 6.0} and {c['sigma'] for c in large} >= {1.0, 2.5, 6.0}
    for group in (sort, large):
        assert any(c['ninf'] for c in group) and any(c['tie'] for c in group) and any(c['tie_k'] for c in group)
        assert any(c['rp'] != 1.0 for c in group) and any(c['typ'] < 1.0 for c in group) and any(c['p'] < 1.0 for c in group)
        assert any(c['k'] == 0 and c['p'] == 1.0 and c['typ'] == 1.0 and c['rp'] == 1.0 and not c['ninf'] for c in group)
    assert any(0 < c['k'] <= 64 for c in sort) and any(c['k'] == 0 or c['k'] > 64 for c in sort)                # arg-max, bitonic
    assert any((c['k'] == 0 or c['k'] > 64) and c['typ'] < 1.0 for c in sort)                                   # bitonic + typical-p
    assert all(c['B'] == (8 if c['V'] == 262144 else 256) for c in S.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_gap_margin_and_cap(name):
    """per case: the rounded model's gap stays under delta (so delta never drops below what the kernel's own arithmetic costs), every
    top-p / typical-p decision of the reference is further than delta from turning over, a tie at the k-th score is there on purpose,
    and at most 2 % of the draws are undecided -- a condition on the inputs, from the reference and the model of u alone"""
    c = S.CASE[name]
    delta = _delta(c)
    refs = S.case_ref(name)
    g = max(r['gap'] for r in refs)
    margin = min(r['margin'] for r in refs)
    nd, nu, bad = S.judge_case(name, S.model_tokens(name), delta)
    print(f'sampler {name}: gap {g:.3e} (delta {delta:.1e})  margin {margin:.3e}  support {[int(r["keep"].sum()) for r in refs]}  '
          f'decided {nd} undecided {nu} ({nu / (nd + nu):.2%})')
    check_gap(g, delta)
    assert margin > delta, (name, margin)
    assert [r['tie_at_k'] for r in refs] == [bool(c['tie_k']) and i == 2 for i in range(S.N_ROWS)]
    if c['tie'] and c['V'] > 8:                              # the planted tie is inside the kept support
        kept = refs[1]['k32'][refs[1]['keep']]
        assert len(np.unique(kept)) < len(kept), name
    assert not bad                                           # the unmodified model passes
    assert nd + nu == len(S.CASE_CTRS) * c['B'] and nu <= CAP * (nd + nu), (name, nu, nd)


def test_deltas_are_four_times_the_largest_gap():
    for large, delta in ((False, DELTA_SORT), (True, DELTA_LARGE)):
        g = max(r['gap'] for c in S.CASES if c['large'] == large for r in S.case_ref(c['name']))
        print(f'sampler large={large}: largest gap {g:.3e} -> 4 x = {4 * g:.3e}, delta {delta:.1e}')
        assert 0.9 * 4 * g <= delta <= 1.25 * 4 * g, (g, delta)      # 4 x the gap, to what exp2 moves it between hosts: no looser constant


# ---------------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize('fault', FAULTS)
def test_checker_rejects_broken_samplers(fault):
    """a sampler that draws every row with row 0's u, reads the seed or the counter as 32 bits, stops the walk one entry late, halves
    j or walks the order backwards fails the check of every case (V = 2 apart, where half of such draws still land right)"""
    for name in NAMES:
        c = S.CASE[name]
        nd, nu, bad = S.judge_case(name, S.model_tokens(name, fault=fault), _delta(c))
        print(f'sampler {name} with fault {fault}: {len(bad)} of {nd + nu} draws rejected')
        assert len(bad) > 0, (name, fault)
        if c['V'] > 2 and c['B'] == 256:
            assert len(bad) > 0.1 * (nd + nu), (name, fault, len(bad))


def test_sweep_detects_dropped_words():
    """part 2's sweep: the closed-form tokens of a sampler that drops hi32(seed) or hi32(ctr) differ from the model's"""
    x = S.exact_cases()['sort_bitonic_v2048']
    rows = np.arange(S.SWEEP_B)
    for fault in ('seed_hi', 'ctr_hi'):
        diff = 0
        for seed in S.SWEEP_SEEDS:
            for ctr in S.SWEEP_CTRS:
                a = x['token'](S.sampler_h2(seed, rows, [ctr] * S.SWEEP_B))
                b = x['token'](S.sampler_h2(seed, rows, [ctr] * S.SWEEP_B, fault=fault))
                diff += int((a != b).sum())
        assert diff > 1000, (fault, diff)


# ---------------------------------------------------------------------------------------------------------------- the stream
SEEDS = (77, 1234, 1234 + S.LANE_STRIDE)
_J = {}


def _stream(seed):
    """j of rows 0-63 x counters 0-16383: 2^20 values"""
    if seed not in _J:
        _J[seed] = S.sampler_u24(seed, np.arange(64)[:, None], np.arange(16384, dtype=np.int64)[None, :])
    return _J[seed]


@pytest.mark.parametrize('seed', SEEDS)
def test_stream_is_uniform(seed):
    """chi-square of the top 8 bits overall and of the top 6 bits per row, against the quantile at upper-tail probability 1e-6"""
    j = _stream(seed)
    x = S.chi2_uniform(np.bincount((j >> 16).ravel(), minlength=256))
    print(f'seed {seed}: top 8 bits chi2 {x:.1f} (limit {S.chi2_limit(255):.1f})')
    assert x < S.chi2_limit(255)
    worst = max(S.chi2_uniform(np.bincount(j[r] >> 18, minlength=64)) for r in range(64))
    print(f'seed {seed}: top 6 bits per row, worst chi2 {worst:.1f} (limit {S.chi2_limit(63):.1f})')
    assert worst < S.chi2_limit(63)


def test_stream_neighbours_are_independent():
    """16 x 16 contingency chi-squares of the top 4 bits: neighbouring rows at one counter, neighbouring counters at one row, the two
    decoder lanes (seed, seed + 7919) at the same row and counter"""
    lim = S.chi2_limit(225)
    for seed in SEEDS:
        t = _stream(seed) >> 20
        rows, ctrs = S.chi2_independence(t[:-1], t[1:]), S.chi2_independence(t[:, :-1], t[:, 1:])
        print(f'seed {seed}: (row, row + 1) chi2 {rows:.1f}  (ctr, ctr + 1) chi2 {ctrs:.1f}  (limit {lim:.1f})')
        assert rows < lim and ctrs < lim
    lanes = S.chi2_independence(_stream(1234) >> 20, _stream(1234 + S.LANE_STRIDE) >> 20)
    print(f'lanes 1234 / {1234 + S.LANE_STRIDE}: chi2 {lanes:.1f} (limit {lim:.1f})')
    assert lanes < lim


def test_chi2_limit_forms_agree():
    """the Wilson-Hilferty form is within 0.5 % of scipy's quantile where both exist"""
    try:
        from scipy import stats
    except ImportError:
        return
    for df in (63, 225, 255):
        z = 4.753424308822899
        wh = df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3
        assert abs(wh / stats.chi2.isf(1e-6, df) - 1) < 5e-3


def test_mix_seed_has_no_collisions():
    for base in (77, 1234):
        seeds = {S.mix_seed(base, step) for step in range((1 << 16) + 1)}
        assert len(seeds) == (1 << 16) + 1
