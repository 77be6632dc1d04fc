"""CPU side of the element-wise attention tests: the float64 closed form of oracle/relattn_cases.py against double-precision
autograd through oracle/relattn_ref.py, the operand-rounded model's gaps against the bounds tests/test_relattn_cases_gpu.py uses,
the cases' own conditions, and a check that those bounds have teeth.  The same over OWNER_CASES, the cases of the fused backward's
owner mode (tests/test_relattn_owner_cases_gpu.py), with the coverage of its visit logic and the faults it could commit."""
import pytest
import torch

from oracle.kernel_cases import check_gap, gap, worst
from oracle.relattn_cases import (CASES, OUTPUTS, OWNER_CASES, STRUCTURED_SHAPES, VISIT_CASES, arms_of, case_model, case_ref, dims,
                                  dq_split, favoured_distance, favoured_share, phantom_sets, relattn_ref64, tile_visits)
from tests.test_relattn_cases_gpu import A_OF, B_OF

IDS = [f'{s}-{f}' for s, f in CASES]
VISIT_IDS = [f'{s}-{f}' for s, f in VISIT_CASES]
OWNER_IDS = [f'{s}-{f}' for s, f in OWNER_CASES]


@pytest.mark.parametrize('shape,family', CASES + VISIT_CASES, ids=IDS + VISIT_IDS)
def test_closed_form_equals_float64_autograd(shape, family):
    """out, lse and the six gradients of relattn_ref64 against autograd through relattn_dense in float64: 1e-10 of max|ref| each"""
    from oracle.relattn_ref import relattn_dense
    c, r = case_ref(shape, family)
    leaf = {n: c[n].double().clone().requires_grad_(True) for n in ('q', 'k', 'v', 'rd', 'rwb', 'rrb')}
    out, lse = relattn_dense(leaf['q'], leaf['k'], leaf['v'], leaf['rd'], leaf['rwb'], leaf['rrb'], c['M'], scale=c['scale'], dtype=torch.float64)
    assert out.dtype == torch.float64
    out.backward(c['dout'].double())
    want = dict(out=out.detach(), lse=lse.detach(), dq=leaf['q'].grad, dk=leaf['k'].grad, dv=leaf['v'].grad, d_rd=leaf['rd'].grad,
                d_rwb=leaf['rwb'].grad, d_rrb=leaf['rrb'].grad)
    for n in OUTPUTS:
        assert gap(r[n], want[n]) <= 1e-10, (n, gap(r[n], want[n]))


@pytest.mark.parametrize('shape,family', CASES, ids=IDS)
def test_rounded_model_gap_stays_under_the_bounds(shape, family):
    """gap(operand-rounded model, float64) per output and arm stays under that output's B_* (4 x the largest gap measured)"""
    c, r = case_ref(shape, family)
    for arm in arms_of(c):
        m = case_model(shape, family, arm)
        names = list(OUTPUTS) + (['oph_all', 'oph_blk'] if c['Kc'] < c['M'] + c['T'] and c['T'] % 32 == 0 else [])
        for n in names:
            if r[n].abs().max() == 0:
                continue
            g = gap(m[n], r[n])
            key = 'oph' if n.startswith('oph') else n
            print(f'{shape} {family} {arm} {n}: gap {g:.3e}  (B {B_OF[key]:.2e})')
            check_gap(g, B_OF[key])


@pytest.mark.parametrize('shape,family', CASES + VISIT_CASES, ids=IDS + VISIT_IDS)
def test_case_conditions(shape, family):
    """every tensor bf16-exact, sequences and heads differ; the favoured cell of `diagonal` / `far-edge` holds at least half of the
    row's probability on at least 90 % of the rows; with Kc = M + T the stored key at position -M is visible to no query and its
    dk / dv are exactly zero; phantom sets are empty with full memory"""
    c, r = case_ref(shape, family)
    for n in ('q', 'k', 'v', 'rd', 'rwb', 'rrb', 'dout'):
        assert torch.equal(c[n].float().to(torch.bfloat16).float(), c[n].float()), n
    assert c['B'] >= 2 and c['H'] >= 2
    assert not torch.equal(c['q'][0], c['q'][1]) and not torch.equal(c['rwb'][0], c['rwb'][1]) and not torch.equal(c['rrb'][0], c['rrb'][1])
    fav = favoured_distance(family, c['M'])
    if fav is not None:
        share = favoured_share(c, r['P'], fav)
        print(f'{shape} {family}: favoured cell >= 1/2 on {share:.3f} of the rows')
        assert share >= 0.9
    if c['Kc'] == c['M'] + c['T']:
        assert (r['dk'][:, 0] == 0).all() and (r['dv'][:, 0] == 0).all()
        s_all, s_blk = phantom_sets(c['T'], c['M'], c['Kc'])
        assert not s_all.any() and not s_blk.any()
    assert abs(r['P'].sum(-1) - 1).max() < 1e-12


def _ratios(c, got, ref):
    return {n: worst(got[n], ref[n], A_OF[n], B_OF[n])[0] for n in OUTPUTS}


@pytest.mark.parametrize('shape', STRUCTURED_SHAPES)
def test_bounds_have_teeth(shape):
    """The float64 reference altered the way a kernel fault would must leave the bounds (worst > 1 on some output), on the
    structured cases: (a) the last visible distance d = M - 1 dropped from every row (far-edge); (b) one 32-query tile's dG shifted
    by one distance (position-coded: dout lives on the tile seams, and diagonal); (c) one d_rd row scaled by 0.9 (diagonal,
    far-edge).  No device, no broken kernel: the reference alone."""
    c, r = case_ref(shape, 'far-edge')
    M = c['M']
    bad = relattn_ref64(c, valid_edit=lambda valid, dist: valid & (dist != M - 1))
    ra = _ratios(c, bad, r)
    print(f'{shape} drop d = M - 1: {ra}')
    assert ra['out'] > 1 and ra['lse'] > 1 and max(ra['dq'], ra['d_rd']) > 1

    def shift(dG):
        dG = dG.clone()
        dG[:, :, 32:64, 1:] = dG[:, :, 32:64, :-1].clone()
        dG[:, :, 32:64, 0] = 0
        return dG
    for fam in ('position-coded', 'diagonal'):
        c, r = case_ref(shape, fam)
        ra = _ratios(c, relattn_ref64(c, dg_edit=shift), r)
        print(f'{shape} {fam} dG of tile 1 shifted: {ra}')
        assert ra['dq'] > 1 and ra['d_rd'] > 1

    for fam, row in (('diagonal', 0), ('far-edge', M - 1)):
        c, r = case_ref(shape, fam)

        def scale_row(d_rd):
            d_rd = d_rd.clone()
            d_rd[row] *= 0.9
            return d_rd
        ra = _ratios(c, relattn_ref64(c, drd_edit=scale_row), r)
        print(f'{shape} {fam} d_rd[{row}] * 0.9: {ra}')
        assert ra['d_rd'] > 1


# ------------------------------------------------------------------------------------------- owner mode of the fused backward
@pytest.mark.parametrize('shape,family', OWNER_CASES, ids=OWNER_IDS)
def test_owner_cases_rounded_model_gap(shape, family):
    """gap(operand-rounded model, float64) of arms 'fused' and 'fused_owner' stays under B_*; on the visit-logic cases also under the
    recorded largest gap, B_* / 4 -- these cases were not among those the bounds were measured over and must not be what sets them"""
    c, r = case_ref(shape, family)
    assert 'fused' in arms_of(c)
    for arm in ('fused', 'fused_owner'):
        m = case_model(shape, family, arm)
        for n in OUTPUTS:
            g = gap(m[n], r[n])
            print(f'{shape} {family} {arm} {n}: gap {g:.3e}  (B {B_OF[n]:.2e})')
            check_gap(g, B_OF[n])
            if (shape, family) in VISIT_CASES:
                assert g <= B_OF[n] / 4, (arm, n, g, B_OF[n] / 4)
    assert torch.equal(case_model(shape, family, 'fused')['dk'], case_model(shape, family, 'fused_owner')['dk'])


def _kernel_sweeps(T, M, Kc):
    """per 256-key block the 32-query tiles its sweep covers (relattn_bwd_fused.hip:585-586)"""
    p0 = T - Kc
    out = []
    for kb in range((Kc + 255) // 256):
        P0 = p0 + 256 * kb
        out.append((max(P0, 0) >> 5, min(P0 + 255 + M - 1, T - 1) >> 5))
    return out


def test_owner_cases_cover_the_visit_logic():
    """(kb_lo, kb_hi, nkb) per 32-query tile from the kernel's formulas: the union over OWNER_CASES holds every pattern the owner
    walk distinguishes.  The formulas are also held against the sweeps themselves: key block kb sweeps tile it iff kb_lo <= kb <= kb_hi."""
    seen = set()
    for shape in dict.fromkeys(s for s, _ in OWNER_CASES):
        x = dims(shape)
        B, T, H, M, Kc = x['B'], x['T'], x['H'], x['M'], x['Kc']
        vis, nkb = tile_visits(T, M, Kc)
        sweeps = _kernel_sweeps(T, M, Kc)
        for it, (lo, hi) in enumerate(vis):
            assert [kb for kb, (a, b) in enumerate(sweeps) if a <= it <= b] == list(range(lo, hi + 1)), (shape, it)
            seen.add('single visit' if lo == hi else 'first and last on different blocks')
            if hi - lo >= 2:
                seen.add('middle visit')
            if lo > 0:
                seen.add('kb_lo > 0')
            if hi < nkb - 1:
                seen.add('kb_hi < nkb - 1')
        seen.add('Kc % 256 == 0' if Kc % 256 == 0 else 'Kc % 256 != 0')
        seen.add('phantom cells' if Kc < M + T else 'no phantom cells')
        ws_bytes = ((M + 255) // 256 + 1) * B * T * H * 64 * 2          # mxl_relattn_bwd_fused_ws_bytes (bf16 slabs)
        assert ws_bytes >= B * T * H * 64 * 4                           # the float32 carry of owner mode always fits
        if ws_bytes == 2 * B * T * H * 128:
            seen.add('workspace of exactly the carry')
        print(shape, vis, nkb)
    want = {'single visit', 'first and last on different blocks', 'middle visit', 'kb_lo > 0', 'kb_hi < nkb - 1', 'Kc % 256 == 0',
            'Kc % 256 != 0', 'phantom cells', 'no phantom cells', 'workspace of exactly the carry'}
    assert seen == want, want - seen


def _owner_faults(c, r):
    """the float64 reference altered the way a fault of owner mode would alter it, one 32-query tile at a time.
    -> {fault: [worst/bound of the altered output, one per eligible tile]}  (dq for the carry / visit / phantom-term faults, d_rrb
    for its phantom part).  dq of a tile = sum over its visits kb_lo .. kb_hi of the key blocks' parts + the phantom term; the
    carry of a tile is what the scratch holds in front of its last visit: the parts of all earlier visits."""
    T, M, Kc = c['T'], c['M'], c['Kc']
    parts = dq_split(c, r['dS'], r['dG'])
    vis, nkb = tile_visits(T, M, Kc)
    phantom = r['dq'] - sum(parts)
    assert gap(phantom, -c['scale'] * r['delta'].transpose(1, 2)[..., None] * r['oph_all']) < 1e-12 or r['oph_all'].abs().max() == 0
    has_ph = Kc < M + T
    rows = lambda it: slice(32 * it, 32 * it + 32)
    carry = lambda it: sum((parts[kb][:, rows(it)] for kb in range(vis[it][0], vis[it][1])), torch.zeros_like(parts[0][:, rows(it)]))
    out = {}

    def dq_fault(name, it, delta_rows):
        bad = r['dq'].clone()
        bad[:, rows(it)] += delta_rows
        out.setdefault(name, []).append(worst(bad, r['dq'], A_OF['dq'], B_OF['dq'])[0])

    def rrb_fault(name, missing):
        out.setdefault(name, []).append(worst(r['d_rrb'] - missing, r['d_rrb'], A_OF['d_rrb'], B_OF['d_rrb'])[0])

    for it, (lo, hi) in enumerate(vis):
        if hi > lo:
            dq_fault('first visit adds a stale carry', it, carry(it))            # (the carry the previous call left: the same inputs)
            dq_fault('first visit dropped', it, -parts[lo][:, rows(it)])
            dq_fault('last visit dropped', it, -parts[hi][:, rows(it)])
            for nb in (it - 1, it + 1):
                if 0 <= nb < len(vis) and vis[nb][1] > vis[nb][0]:
                    dq_fault(f'carry of tile it {"-" if nb < it else "+"} 1', it, carry(nb) - carry(it))
        if has_ph and phantom[:, rows(it)].abs().max() > 0:
            dq_fault('phantom term omitted on a tile', it, -phantom[:, rows(it)])
            dq_fault('phantom term added twice on a tile', it, phantom[:, rows(it)])
            rrb_fault('phantom part of d_rrb missing for a tile', phantom[:, rows(it)].sum((0, 1)))
    if has_ph:
        rrb_fault('phantom part of d_rrb missing', phantom.sum((0, 1)))
    return out


def test_owner_mode_faults_leave_the_bounds():
    """every fault owner mode can commit -- on ONE query tile, the least visible form -- leaves the bounds on at least one case of
    OWNER_CASES, whichever tile it strikes: per case the smallest worst/bound over the eligible tiles, and the largest of those over
    the cases must exceed 1 (a case with a single eligible tile does not count for a one-tile fault: there the tile is the whole
    case).  No device is involved."""
    best = {}
    for shape, family in OWNER_CASES:
        c, r = case_ref(shape, family)
        for name, ratios in _owner_faults(c, r).items():
            if len(ratios) < 2 and name != 'phantom part of d_rrb missing':
                continue
            lo = min(ratios)
            if lo > best.get(name, (0.0, None))[0]:
                best[name] = (lo, f'{shape} {family}')
    for name, (ratio, case) in sorted(best.items()):
        print(f'{name}: worst/bound at least {ratio:.2f}, whichever tile, on {case}')
    want = {'first visit adds a stale carry', 'first visit dropped', 'last visit dropped', 'carry of tile it - 1', 'carry of tile it + 1',
            'phantom term omitted on a tile', 'phantom term added twice on a tile', 'phantom part of d_rrb missing for a tile',
            'phantom part of d_rrb missing'}
    assert set(best) == want, want ^ set(best)
    assert all(ratio > 1 for ratio, _ in best.values()), best
