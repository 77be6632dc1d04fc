"""CPU side of the FP8 K/V ring tests (no GPU): the properties of the host restatement of the format (tests/kv_fp8_ref.py), the
rounded-model gap behind B_OUT_FP8 of tests/test_kv_fp8_ops_gpu.py measured again over every case, arm and family of
oracle/decode_cases.py with the rings replaced by their dequantised values, and the teeth of that bound on these inputs: the faults
tests/test_decode_cases_cpu.py plants, and three of the format's own -- one favoured slot's exponent off by one in K, in V, and K's
exponents applied to V."""
import numpy as np
import pytest
import torch

from oracle import decode_cases as D
from oracle.kernel_cases import A_BF16, check_gap, gap, worst
from tests import kv_fp8_ref as R
from tests.test_kv_fp8_ops_gpu import B_OUT_FP8

ARMS = list(D.attn_arms())
EDGE_ARMS = [a for a in ARMS if a[2].startswith('edges')]
PHANTOM_ARMS = [a for a in ARMS if a[2] == 'phantom']
_ids = lambda arms: [f'{n}-p{p}-{f}' for n, p, f in arms]


def _bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def _rows():
    """the rows the property tests run: the K / V rings of three attention cases (written and never-written slots), the q / k / v
    thirds of the writers' cases and the planted special rows"""
    out = []
    for name, fam in (('m301', 'random'), ('pc_tail_empty', 'edges0'), ('d16_n2048', 'phantom')):
        c = D.attn_case(name, fam, 1)
        out += [c['kc'].reshape(-1, c['dh']), c['vc'].reshape(-1, c['dh'])]
    out += [R.special_rows(dh).float() for dh in (16, 32, 64)]
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_scaled_amax_lies_in_224_448_and_values_are_bf16_exact():
    for x in _rows():
        q, e = R.quantise(x)
        amax = x.double().abs().amax(-1)
        live = (amax > 0) & (e > R.E_MIN)                              # (a row clamped at e = -126 may sit below 224)
        scaled = torch.ldexp(amax, -e.to(torch.int32))
        assert ((scaled[live] > 224) & (scaled[live] <= 448)).all()
        assert (scaled <= 448).all()
        d = R.dequantise(q, e)
        assert _bf16_exact(d)
        # the error of a stored element: half a step of e4m3fn at the row's scale, 2^-4 of the element or 2^-10 of 2^(e + ...) below
        err = (d.double() - x.double()).abs()
        assert (err <= torch.maximum(x.double().abs() * 2.0 ** -4, torch.ldexp(torch.ones_like(amax), e.to(torch.int32) - 10).unsqueeze(-1))).all()


def test_requantising_stored_values_keeps_them():
    """quantise(dequantise(q)) == q byte for byte and exponent for exponent -- but for the rows whose largest scaled element lies in
    (224, 232] and rounds DOWN to 224: their stored amax is 224 2^e = 448 2^(e - 1), so the rule gives them e - 1 and the doubled
    bytes on the second pass.  Those rows are named exactly by their largest stored byte, and they keep their VALUES, as every row
    does."""
    seen_boundary = 0
    for x in _rows():
        q, e = R.quantise(x)
        d = R.dequantise(q, e)
        q2, e2 = R.quantise(d)
        top = q.view(torch.float8_e4m3fn).float().abs().amax(-1)
        down = (top == 224) & (e > R.E_MIN)
        seen_boundary += int(down.sum())
        assert torch.equal(q2[~down], q[~down]) and torch.equal(e2[~down], e[~down])
        assert (e2[down] == e[down] - 1).all()
        assert torch.equal(R.dequantise(q2, e2), d)
    assert seen_boundary > 0                                           # (special_rows plants one: 1.7578125 -> 225 -> 224)


def test_zero_boundary_and_subnormal_rows():
    for dh in (16, 32, 64):
        rows = R.special_rows(dh)
        q, e = R.quantise(rows)
        assert (q[0] == 0).all() and e[0] == 0
        # 1.75 = 0.875 * 2^1 exactly: k = 1, e = k - 9; the next bf16 up: e = k - 8
        assert rows[1].float().abs().max() == 1.75 and e[1] == -8
        assert rows[2].float().abs().max() == 1.7578125 and e[2] == -7
        assert q[1].view(torch.float8_e4m3fn).float().abs().max() == 448
        # a bf16-subnormal row: k - 9 lies below -126
        assert 0 < rows[3].float().abs().max() < 2.0 ** -126 and e[3] == -126
        assert (q[3] & 0x7F != 0).any()
        # e4m3fn subnormals are kept: a stored byte below the smallest normal (exponent field 0), not flushed
        assert ((q[4] & 0x78) == 0).any() and ((q[4] & 0x7F) != 0)[(q[4] & 0x78) == 0].any()
    m, k = torch.frexp(torch.tensor([1.75, 1.7578125], dtype=torch.float64))
    assert m[0] == 0.875 and m[1] > 0.875 and k.tolist() == [1, 1]


def test_attention_inputs_quantise_cleanly():
    """over the attention inputs of every case: scaled amax in (224, 448] for every non-zero row, dequantised values bf16-exact, never
    written slots zero bytes with e = 0"""
    for name, c0 in D.ATTN_CASES.items():
        c = R.fp8_attn_case(name, 'random', 1)
        nv = c['nvalid']
        for q, e, x in ((c['kq'], c['ke'], D.attn_case(name, 'random', 1)['kc']), (c['vq'], c['ve'], D.attn_case(name, 'random', 1)['vc'])):
            amax = x.double().abs().amax(-1)
            scaled = torch.ldexp(amax, -e.to(torch.int32))[:, :, :nv]
            assert ((scaled > 224) & (scaled <= 448)).all(), name
            assert (q[:, :, nv:] == 0).all() and (e[:, :, nv:] == 0).all()
        assert _bf16_exact(c['kc']) and _bf16_exact(c['vc'])


# ---------------------------------------------------------------------------------------------------------------- the bound
def test_gaps_stay_under_the_bound():
    """every case, arm and family on the dequantised rings: the rounded model's gap stays under B_OUT_FP8, which is 4 x the largest"""
    top = (0.0, None)
    for name, p, fam in ARMS:
        c = R.fp8_attn_case(name, fam, p)
        g = gap(D.attn_model(c, p), D.attn_ref64(c)[0])
        print(f'fp8 decode attention {name} pieces {p} {fam}: gap {g:.3e}')
        check_gap(g, B_OUT_FP8)
        top = max(top, (g, f'{name} pieces {p} {fam}'))
    print(f'fp8 decode attention: largest gap {top[0]:.3e} ({top[1]}) -> B_OUT_FP8 {B_OUT_FP8:.2e}')
    assert 4 * top[0] <= B_OUT_FP8 <= 4.5 * top[0], 'B_OUT_FP8 is 4 x the largest gap, rounded up'


# ---------------------------------------------------------------------------------------------------------------- teeth
def _ratio(c, ref=None, **edit):
    ref = D.attn_ref64(c)[0] if ref is None else ref
    return worst(D.attn_ref64(c, **edit)[0], ref, A_BF16, B_OUT_FP8)[0]


@pytest.mark.parametrize('name,pieces,fam', EDGE_ARMS, ids=_ids(EDGE_ARMS))
def test_teeth_dropped_slot_and_shifted_distance(name, pieces, fam):
    c = R.fp8_attn_case(name, fam, pieces)
    ref = D.attn_ref64(c)[0]
    for s in c['fav']:
        r = _ratio(c, ref, drop=(s,))
        assert r > 1.0, (name, fam, s, r)
    for sh in (1, -1):
        r = _ratio(c, ref, shift=sh)
        assert r > 1.0, (name, fam, sh, r)


@pytest.mark.parametrize('name,pieces,fam', PHANTOM_ARMS, ids=_ids(PHANTOM_ARMS))
def test_teeth_never_written_slots_out_of_the_denominator(name, pieces, fam):
    c = R.fp8_attn_case(name, fam, pieces)
    ref = D.attn_ref64(c)[0]
    assert _ratio(c, ref, no_phantom_den=True) > 1.0
    assert _ratio(c, ref, drop=(c['fav'][0],)) > 1.0


MERGE_ARMS = [(n, p, 'phantom') for n in ('pc_mixed', 'pc_tail_empty', 'live_p4') for p in D.ATTN_CASES[n]['pieces'] if p > 1] \
    + [('pc_full', 8, 'edges0')]


@pytest.mark.parametrize('name,pieces,fam', MERGE_ARMS, ids=_ids(MERGE_ARMS))
def test_teeth_merge_with_one_pieces_maximum(name, pieces, fam):
    c = R.fp8_attn_case(name, fam, pieces)
    mx = D.piece_maxima(c, pieces)
    held = np.isfinite(mx).all((0, 1))
    assert held.sum() >= 2 and (mx[:, :, held].max(-1) - mx[:, :, held].min(-1)).min() > 2.0
    assert _ratio(c, merge_as=(pieces, 0)) > 1.0
    assert _ratio(c) == 0.0


def _with_exponent(c, which, s, delta):
    """the case with the exponent of slot s of ring `which` ('k' / 'v') off by delta"""
    e = c[which + 'e'].clone()
    e[:, :, s] += delta
    out = dict(c)
    out[which + 'c'] = R.dequantise(c[which + 'q'], e)
    return out


def _written_fav(c):
    return [s for s in c['fav'] if s < c['nvalid']]


V_ARMS = [a for a in EDGE_ARMS if _written_fav(D.attn_case(a[0], a[2], a[1]))]
# K's exponent moves the content term q' . k_s alone, which the edges families keep quiet (a standard deviation of 1/8 of a logit: the
# positional lift decides the shares), and it moves it by that term's own size, which is random per head.  The fault is therefore
# certain to leave the bound only where a favoured slot holds a large share: the edges arms with at most three favoured written slots.
# In every other edges arm it leaves the bound at some favoured slot, and that is what is asked there.
K_SHARP_ARMS = [a for a in V_ARMS if len(_written_fav(D.attn_case(a[0], a[2], a[1]))) <= 3]


@pytest.mark.parametrize('name,pieces,fam', V_ARMS, ids=_ids(V_ARMS))
def test_teeth_v_exponent_off_by_one_and_k_exponents_on_v(name, pieces, fam):
    """family: edges.  The value rows of the favoured slots are large and distinct and each holds at least 1 / (2 |chunk|) of a row, so
    one slot's V exponent one up or one down (its row doubled or halved) leaves the bound at every favoured written slot; K's exponents
    (quiet rows: some 2^-4 of V's scale) read for V leave it by far"""
    c = R.fp8_attn_case(name, fam, pieces)
    ref = D.attn_ref64(c)[0]
    for s in _written_fav(c):
        for dl in (1, -1):
            r = worst(D.attn_ref64(_with_exponent(c, 'v', s, dl))[0], ref, A_BF16, B_OUT_FP8)[0]
            assert r > 1.0, (name, fam, s, dl, r)
    swapped = dict(c)
    swapped['vc'] = R.dequantise(c['vq'], c['ke'])
    r = worst(D.attn_ref64(swapped)[0], ref, A_BF16, B_OUT_FP8)[0]
    print(f'fp8 teeth {name} pieces {pieces} {fam}: K exponents on V -> worst/bound {r:.1f}')
    assert r > 1.0


@pytest.mark.parametrize('name,pieces,fam', V_ARMS, ids=_ids(V_ARMS))
def test_teeth_k_exponent_off_by_one(name, pieces, fam):
    """family: edges (see K_SHARP_ARMS above for which arms promise what)"""
    c = R.fp8_attn_case(name, fam, pieces)
    ref = D.attn_ref64(c)[0]
    rs = {(s, dl): worst(D.attn_ref64(_with_exponent(c, 'k', s, dl))[0], ref, A_BF16, B_OUT_FP8)[0]
          for s in _written_fav(c) for dl in (1, -1)}
    print(f'fp8 teeth {name} pieces {pieces} {fam}: K exponent off by one -> worst/bound {min(rs.values()):.2f} .. {max(rs.values()):.2f}')
    assert max(rs.values()) > 1.0
    if (name, pieces, fam) in K_SHARP_ARMS:
        assert min(rs.values()) > 1.0, rs


def test_k_sharp_arms_cover_every_head_width():
    assert {D.ATTN_CASES[n]['dh'] for n, _, _ in K_SHARP_ARMS} == {16, 32, 64} and len(K_SHARP_ARMS) >= 10
