"""CPU side of the element-wise attention tests: the float64 closed form of oracle/relattn_cases.py against double-precision
autograd through oracle/relattn_ref.py, the operand-rounded model's gaps against the bounds tests/test_relattn_cases_gpu.py uses,
the cases' own conditions, and a check that those bounds have teeth."""
import pytest
import torch

from oracle.kernel_cases import check_gap, gap, worst
from oracle.relattn_cases import (CASES, OUTPUTS, STRUCTURED_SHAPES, arms_of, case_model, case_ref, favoured_distance, favoured_share,
                                  phantom_sets, relattn_ref64)
from tests.test_relattn_cases_gpu import A_OF, B_OF

IDS = [f'{s}-{f}' for s, f in CASES]


@pytest.mark.parametrize('shape,family', CASES, ids=IDS)
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


@pytest.mark.parametrize('shape,family', CASES, ids=IDS)
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
