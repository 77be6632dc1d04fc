"""CPU side of the element-wise Reformer kernel tests: the float64 closed forms of oracle/reformer_cases.py against float64 autograd,
the numpy dropout masks against a cell-by-cell transcription of the device code, the rounded models' gaps against the bounds
tests/test_reformer_cases_gpu.py uses, the cases' own conditions, and a check that those bounds have teeth."""
import math

import numpy as np
import pytest
import torch

from oracle.kernel_cases import (axial_emb_mask, axial_pos_mask, check_gap, chunk_drop_mask, dropout_thresh, gap, single_drop_mask)
from oracle.reformer_cases import (AXIAL_CASES, CHUNK_CASES, COMBINE_CASES, HASH_CASES, PROBE_CASES, SC_MAXT, SINGLE_CASES, attn_case,
                                   attn_ref64, axial_case, axial_masks, axial_ref64, combine_case, combine_ref64, dscale_of, gap_grouped,
                                   hash_buckets, hash_case, hash_near_ties, lse_groups, probe_case, probe_zero_sets, slot_positions,
                                   worst_grouped)
from tests.test_reformer_cases_gpu import A_ATTN, AX_DROP, B_AXIAL, B_CHUNK, B_COMBINE, b_attn

ATTN_NAMES = [r['name'] for r in CHUNK_CASES + SINGLE_CASES]
GRADS = ('dq', 'dk', 'dv')


# ---------------------------------------------------------------------------------------------------------------- closed forms
def _autograd(c, use_ref_module):
    """float64 autograd of sum(out dout) + sum(lse dlse) through the forward in slot order -> dict in the kernels' layouts; dk is
    taken w.r.t. the EFFECTIVE key (a leaf of its own), dqk through the whole chain"""
    from oracle.reformer_ref import chunked_attention
    B, T, H, dh, n_h, lsh, p = (c[n] for n in ('B', 'T', 'H', 'dh', 'n_h', 'lsh', 'p'))
    S = n_h * T
    pos = slot_positions(c)
    gi = pos.unsqueeze(-1).expand(-1, -1, -1, dh)
    q = c['q'].double().permute(0, 2, 1, 3).clone().requires_grad_(True)
    v = c['v'].double().permute(0, 2, 1, 3).clone().requires_grad_(True)
    if lsh:
        keff = (q * torch.rsqrt((q * q).mean(-1, keepdim=True) + 1e-6) / math.sqrt(dh))
    else:
        kraw = c['k'].double().permute(0, 2, 1, 3).clone().requires_grad_(True)
        keff = kraw / math.sqrt(dh)
    # one leaf per SLOT for q, k', v: their gradients are the per-(round, position) slabs
    qs = q.gather(2, gi).detach().requires_grad_(True)
    ks = keff.gather(2, gi).detach().requires_grad_(True)
    vs = v.gather(2, gi).detach().requires_grad_(True)
    if use_ref_module:
        assert p == 0 and T > SC_MAXT
        out_s, lse_s = chunked_attention(qs, ks, vs, pos, 64, self_mask=bool(lsh))
    else:
        r = attn_ref64(c)
        C = T if T <= SC_MAXT else 64
        NC = S // C
        qc, kc, vc = (t.view(B, H, NC, C, dh) for t in (qs, ks, vs))
        if T > SC_MAXT:
            kc = torch.cat([torch.roll(kc, 1, 2), kc], 3)
            vc = torch.cat([torch.roll(vc, 1, 2), vc], 3)
        dots = qc @ kc.transpose(-1, -2)
        dots = torch.where(r['causal'], dots, torch.tensor(-1e9, dtype=torch.float64))
        if lsh:
            dots = torch.where(r['same'], torch.tensor(-1e5, dtype=torch.float64), dots)
        lse = torch.logsumexp(dots, -1, keepdim=True)
        P = torch.exp(dots - lse)
        if r['keep'] is not None:
            P = P * r['keep'].double() * dscale_of(p)
        out_s, lse_s = (P @ vc).reshape(B, H, S, dh), lse.reshape(B, H, S)
    rnd = (torch.arange(S) // T).view(1, 1, S).expand(B, H, S)
    bi = torch.arange(B).view(B, 1, 1).expand(B, H, S)
    hi = torch.arange(H).view(1, H, 1).expand(B, H, S)
    do_s = c['dout'].double()[bi, rnd, pos, hi]
    loss = (out_s * do_s).sum()
    if c['dlse'] is not None:
        loss = loss + (lse_s * c['dlse'].double()[bi, rnd, hi, pos]).sum()
    loss.backward()

    def slabs(t):
        o = torch.zeros(B, n_h, T, H, dh, dtype=torch.float64)
        o[bi, rnd, pos, hi] = t
        return o
    res = dict(out=slabs(out_s.detach()), dq=slabs(qs.grad), dv=slabs(vs.grad))
    res['lse'] = torch.zeros(B, n_h, H, T, dtype=torch.float64)
    res['lse'][bi, rnd, hi, pos] = lse_s.detach()
    # push the slot gradients back to the per-position leaves
    gq = torch.zeros_like(q).scatter_add_(2, gi, qs.grad)
    gk = torch.zeros_like(q).scatter_add_(2, gi, ks.grad)
    if lsh:
        res['dk'] = slabs(ks.grad)
        (dqk,) = torch.autograd.grad(keff, q, gk)
        res['dqk'] = (dqk + gq).permute(0, 2, 1, 3)
    else:
        (dk,) = torch.autograd.grad(keff, kraw, gk)
        res['dk'] = dk.permute(0, 2, 1, 3).unsqueeze(1)
    return res


@pytest.mark.parametrize('name', ATTN_NAMES)
def test_closed_form_equals_float64_autograd(name):
    """out, lse, dq, dk', dv (per round slab) and dqk of attn_ref64 against float64 autograd: through oracle.reformer_ref.chunked_attention
    where it applies (T > 64, no dropout), through the written forward otherwise (dropout under the numpy mask, the single-chunk form)"""
    c, ref, _ = attn_case(name)
    forms = [False] + ([True] if c['p'] == 0 and c['T'] > SC_MAXT else [])
    for use_ref_module in forms:
        want = _autograd(c, use_ref_module)
        for n, w in want.items():
            groups = lse_groups(w) if n == 'lse' else None
            g = gap_grouped(ref[n], w, groups)
            assert g <= 1e-10, (name, use_ref_module, n, g)


@pytest.mark.parametrize('name', list(COMBINE_CASES))
def test_combine_closed_form_equals_float64_autograd(name):
    c = combine_case(name)
    o_r = c['out_r'].double().requires_grad_(True)
    lse = c['lse'].double().requires_grad_(True)
    w = torch.softmax(lse, 1).permute(0, 1, 3, 2).unsqueeze(-1)
    out = (w * o_r).sum(1)
    out.backward(c['dout'].double())
    r = combine_ref64(c)
    assert gap(r['out'], out.detach()) <= 1e-10 and gap(r['dout_r'], o_r.grad) <= 1e-10 and gap(r['dlse'], lse.grad) <= 1e-10


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('name', list(AXIAL_CASES))
def test_axial_closed_form_equals_float64_autograd(name, p):
    c = axial_case(name)
    kw = dict(AX_DROP, p=p) if p > 0 else dict(p=0.0, seed=0, site_emb=0, site_pos=1)
    ke, kp = axial_masks(c, **kw)
    E, W0, W1 = (c[n].double().requires_grad_(True) for n in ('E', 'W0', 'W1'))
    t = torch.arange(c['T'])
    out = ke * E[c['ids']] * dscale_of(p) + kp * torch.cat([W0[t // c['A1']], W1[t % c['A1']]], -1).unsqueeze(0) * dscale_of(p)
    out.backward(c['dout'].double() + c['dout2'].double())
    r = axial_ref64(c, two=True, **kw)
    for n, w in (('out', out.detach()), ('dE', E.grad), ('dW0', W0.grad), ('dW1', W1.grad)):
        assert gap(r[n], w) <= 1e-10, (name, n)
    if p > 0:
        assert 0.05 <= 1 - ke.mean().item() <= 0.15 and 0.03 <= 1 - kp.mean().item() <= 0.17


# ---------------------------------------------------------------------------------------------------------------- masks
def _h32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _mix_int(seed, site):
    return (_h32((seed & 0xFFFFFFFF) ^ ((site * 0x9E3779B9) & 0xFFFFFFFF)) + (seed >> 32)) & 0xFFFFFFFF


def _keep_int(seed, site, idx, thresh):
    """dropout_keep of csrc/common.h, one element, python integers"""
    h = _h32((((idx & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) ^ (((idx >> 32) * 0x85EBCA77) & 0xFFFFFFFF) ^ _mix_int(seed, site))
    return h >= thresh


def _chunk_keep_int(seed, site, slot, kw, thresh):
    """chunk_drop_row / chunk_drop_words / chunk_drop_keep of csrc/reformer.hip:387-403, one cell, python integers"""
    blk = (slot >> 1) * 64
    key = (((((blk & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) ^ (((blk >> 32) * 0x85EBCA77) & 0xFFFFFFFF)) + _mix_int(seed, site)) & 0xFFFFFFFF
    w0 = _h32((key + (kw >> 1) * 0x9E3779B1) & 0xFFFFFFFF)
    w1 = ((w0 * 0x85EBCA77) & 0xFFFFFFFF) ^ (w0 >> 13)
    w = w1 if kw & 1 else w0
    return ((w >> 16) if slot & 1 else (w & 0xFFFF)) >= (thresh >> 16)


@pytest.mark.parametrize('seed,site,p', [(77, 3, 0.1), ((0x1234ABCD << 32) | 0x9E3779B9, 5, 0.5), ((1 << 63) + 12345, 0, 0.25)])
def test_numpy_masks_equal_a_cell_by_cell_transcription(seed, site, p):
    th = dropout_thresh(p)
    slots = np.array([0, 1, 2, 3, 510, 511, 77777, (1 << 27) + 5, (1 << 31) + 2, (1 << 33) + 7], dtype=np.uint64)       # blk crosses 2^32
    m = chunk_drop_mask(seed, site, slots, p)
    for i, s in enumerate(slots):
        for kw in range(128):
            assert bool(m[i, kw]) == _chunk_keep_int(seed, site, int(s), kw, th), (int(s), kw)
    B, H, T = 2, 3, 7
    sm = single_drop_mask(seed, site, B, H, T, p)
    for b in range(B):
        for h in range(H):
            for i in range(T):
                for j in range(T):
                    assert bool(sm[b, h, i, j]) == _keep_int(seed, site, (((b * H + h) * T + i) * 64 + j), th)
    B, T, A1, d = 3, 21, 8, 5
    pm, em = axial_pos_mask(seed, site, B, T, A1, p), axial_emb_mask(seed, site + 1, B, T, d, p)
    for b in range(B):
        for t in range(T):
            assert bool(pm[b, t]) == _keep_int(seed, site, b * A1 + t % A1, th)
            for k in range(d):
                assert bool(em[b, t, k]) == _keep_int(seed, site + 1, (b * T + t) * d + k, th)


# ---------------------------------------------------------------------------------------------------------------- gaps
@pytest.mark.parametrize('name', ATTN_NAMES)
def test_attention_rounded_model_gap_stays_under_the_bounds(name):
    c, ref, model = attn_case(name)
    names = ('out', 'lse') + GRADS + (('dqk', 'dv_sum') if c['lsh'] else ())
    for n in names:
        g = gap_grouped(model[n], ref[n], lse_groups(ref[n]) if n == 'lse' else None)
        print(f'GAP {"single" if c["T"] <= SC_MAXT else "chunk"} {n} {g:.3e} {name}')
        check_gap(g, b_attn(c)[n])


@pytest.mark.parametrize('name', list(PROBE_CASES))
def test_probe_rounded_model_gap_stays_under_the_bounds(name):
    """and the rounded model itself has the exact zeros the GPU test asks of the device; over the 128 launches every cell of a window is probed"""
    for k in (0, 37, 124, 127):
        c = probe_case(name, k)
        ref, model = attn_ref64(c), attn_ref64(c, rounded=True)
        for n, (zero, nonzero) in probe_zero_sets(c, ref).items():
            g = gap_grouped(model[n], ref[n])
            print(f'GAP chunk {n} {g:.3e} {name}:{k}')
            check_gap(g, B_CHUNK[n])
            assert (model[n][zero] == 0).all() and (model[n][nonzero] != 0).all()
            assert zero.any() and nonzero.any()
    # coverage: the launches are all (column group, dout shift) pairs, so for every query i and every key k of its window one launch
    # gives k a one (its group) in the column i's dout picks (shift = (k - i) mod dh)
    dh = probe_case(name, 0)['dh']
    assert {(k % (128 // dh), k // (128 // dh)) for k in range(128)} == {(g, s) for g in range(128 // dh) for s in range(dh)}


@pytest.mark.parametrize('name', list(COMBINE_CASES))
def test_combine_rounded_model_gap_stays_under_the_bounds(name):
    c = combine_case(name)
    ref, model = combine_ref64(c), combine_ref64(c, rounded=True)
    for n in ('out', 'dout_r', 'dlse'):
        g = gap(model[n], ref[n])
        print(f'GAP combine {n} {g:.3e} {name}')
        check_gap(g, B_COMBINE[n])
    if c['low']:        # the underflowing round: zeros, and its share of the reference is far below the bound
        assert (model['dout_r'][:, 1] == 0).all() and (model['dlse'][:, 1] == 0).all()


@pytest.mark.parametrize('name', list(AXIAL_CASES))
def test_axial_rounded_model_gap_stays_under_the_bounds(name):
    c = axial_case(name)
    for kw in (dict(p=0.0), AX_DROP):
        for two in (False, True):
            ref, model = axial_ref64(c, two=two, **kw), axial_ref64(c, two=two, rounded=True, **kw)
            for n in ('out', 'dE', 'dW0', 'dW1'):
                g = gap(model[n], ref[n])
                print(f'GAP axial {n} {g:.3e} {name}')
                check_gap(g, B_AXIAL[n])


# ---------------------------------------------------------------------------------------------------------------- conditions
def test_case_tables_cover_what_they_claim():
    ch = CHUNK_CASES
    assert {r['T'] for r in ch} == {128, 192, 256} and {r['dh'] for r in ch} == {16, 32, 64}
    assert {r['n_h'] for r in ch if r['lsh']} == {1, 2, 3} and {(r['B'], r['H']) for r in ch} == {(1, 1), (3, 3), (2, 4)}
    for lsh in (0, 1):
        assert {r['dh'] for r in ch if r['lsh'] == lsh} == {16, 32, 64}
        assert {r.get('p', 0.0) for r in ch if r['lsh'] == lsh} >= {0.0, 0.1, 0.5}
        assert {bool(r.get('wide')) for r in ch if r['lsh'] == lsh} == {False, True}
    assert any(r['n_h'] == 2 and r['T'] == 128 for r in ch)
    assert {r.get('kind', 'random') for r in ch} == {'random', 'poscode', 'dominant'}
    assert {r.get('order', 'random') for r in ch if r['lsh']} == {'random', 'desc', 'dup'}
    assert any(r.get('seed', 0) >> 32 for r in ch)
    sg = SINGLE_CASES
    assert {(r['T'], r['dh'], r['lsh']) for r in sg} == {(T, dh, l) for T in (1, 7, 33, 64) for dh in (16, 32, 64) for l in (0, 1)}
    assert {r['p'] for r in sg if r['B'] * r['H'] > 1 and r['T'] % 2} >= {0.1, 0.5}        # odd offsets (b H + h) T of the cell index
    assert {r['n_h'] for r in map(lambda n: combine_case(n), COMBINE_CASES)} == {1, 2, 3}
    forms = {v[7] for v in AXIAL_CASES.values()}
    assert forms == {'elem', 'rows'}
    for n, (B, T, V, d, d0, A0, A1, form) in AXIAL_CASES.items():
        assert T <= A0 * A1 and (form == 'rows') == (B * T >= 4096 and d % 32 == 0 and d0 % 32 == 0)
    assert any(B * T < 4096 <= B * (T + 3) for (B, T, *_r) in AXIAL_CASES.values())
    arms = {(('scalar' if (r['dh'] == 16 or r['off8']) else 'mfma'), 16 if sum(r['factors']) <= 32 else 32 if sum(r['factors']) <= 64 else 64)
            for r in HASH_CASES.values()}
    assert arms == {(k, n) for k in ('scalar', 'mfma') for n in (16, 32, 64)}
    assert {sum(r['factors']) // 2 for r in HASH_CASES.values()} >= {8, 16, 24, 32, 48, 64}
    assert any(r['off8'] and r['dh'] == 64 for r in HASH_CASES.values()) and any(r['mixed'] for r in HASH_CASES.values())


@pytest.mark.parametrize('name', ATTN_NAMES)
def test_attention_case_conditions(name):
    """bf16-exact inputs; heads and sequences differ; every round's slots are a permutation; the hand-built orders do what they say;
    the dropout cases drop p +- 0.05 of the live cells"""
    c, ref, _ = attn_case(name)
    B, T, H, n_h = c['B'], c['T'], c['H'], c['n_h']
    for n in ('q', 'k', 'v', 'dout'):
        assert torch.equal(c[n].float().to(torch.bfloat16).float(), c[n].float())
    if B > 1:
        assert not torch.equal(c['q'][0], c['q'][1]) and not torch.equal(c['v'][0], c['v'][1])
    if H > 1:
        assert not torch.equal(c['q'][:, :, 0], c['q'][:, :, 1]) and not torch.equal(c['v'][:, :, 0], c['v'][:, :, 1])
    pos = slot_positions(c)
    assert torch.equal(pos.view(B, H, n_h, T).sort(-1).values, torch.arange(T).expand(B, H, n_h, T))
    lse = ref['lse']
    if c['lsh']:
        alone = lse < -5e4                       # queries that see only self-masked cells
        assert alone[:, :, :, 0].all()           # position 0 always
        assert (ref['dq'][alone.permute(0, 1, 3, 2)] == 0).all()
        if c['order'] == 'desc' and T > SC_MAXT:
            per = alone.sum(-1)                  # (B, n_h, H): every chunk but the one that looks back across the wrap-around
            assert (per >= T // 64 - 1).all() and per.max() >= 2, per
            assert ((lse[alone] + 1e5).abs() < 1.0).all()
    if c['order'] == 'dup' and n_h > 1:
        kp = torch.cat([torch.roll(pos.view(B, H, -1, 64), 1, 2), pos.view(B, H, -1, 64)], 3)
        first = T // 64                          # the first chunk of round 1: its window holds every position twice
        assert (kp[:, :, first].sort(-1).values.view(B, H, 64, 2).diff(dim=-1) == 0).all()
        assert ((ref['same'][:, :, first].sum(-1)) == 2).all()
    if c['kind'] == 'dominant':
        assert (ref['P'].amax(-1) > 0.9).sum() >= B * H
    if c['p'] > 0:
        live = ref['P'] > 0
        share = 1.0 - ref['keep'][live].double().mean().item()
        print(f'{name}: {share:.4f} of the {int(live.sum())} live cells dropped (p = {c["p"]})')
        if int(live.sum()) >= 1000:             # (T = 1 and T = 7 have too few cells for a share to mean anything)
            assert c['p'] - 0.05 <= share <= c['p'] + 0.05
        else:
            assert 0 < int(live.sum())


# ---------------------------------------------------------------------------------------------------------------- teeth
def _leaves(model, ref_bad, names, A, Bd):
    """a correct kernel (stood in for by the rounded model) held against a reference with a planted fault: the worst ratio over `names`"""
    return max(worst_grouped(model[n], ref_bad[n], A[n], Bd[n], lse_groups(ref_bad[n]) if n == 'lse' else None)[0] for n in names)


@pytest.mark.parametrize('edit,name,names', [
    ('no_wrap', 'c_lsh_t128_n1_dh64', ('out', 'lse', 'dq', 'dk', 'dv')),
    ('no_wrap', 'c_lsh_t256_n3_dh64', ('out', 'lse', 'dq', 'dk', 'dv')),
    ('no_wrap', 'c_lsh_t128_n2_dh32_dup', ('lse',)),
    ('mask_shift', 'c_loc_t256_dh16', ('out', 'dq', 'dk', 'dv')),
    ('mask_shift', 'c_lsh_t192_n2_dh64_p10', ('out', 'dq', 'dk', 'dv')),
    ('parity_swap', 'c_loc_t192_dh16_p50', ('out', 'dq', 'dk', 'dv')),
    ('parity_swap', 'c_lsh_t128_n1_dh32_dom_p10', ('out', 'dq', 'dk', 'dv')),
    ('no_keyfac_chain', 'c_lsh_t128_n1_dh64', ('dqk',)),
    ('no_keyfac_chain', 's_t33_dh32_lsh', ('dqk',)),
    ('drop_round', 'c_lsh_t128_n3_dh16', ('dqk', 'dv_sum')),
    ('drop_round', 'c_lsh_t256_n3_dh64', ('dqk', 'dv_sum')),
])
def test_planted_faults_leave_the_bounds(edit, name, names):
    """each fault, planted in the REFERENCE, puts every listed output of a correct kernel outside its bound.  'no_wrap' (chunk 0 without
    its look-back at the last chunk) is asked of LSH cases only: with local attention the last chunk lies wholly in chunk 0's future and
    is masked anyway.  In the 'dup' order chunk 0 looks back at a copy of its own positions, which doubles every weight: only lse moves."""
    c, ref, model = attn_case(name)
    bad = attn_ref64(c, edit=(edit,))
    for n in names:
        r = _leaves(model, bad, (n,), A_ATTN, b_attn(c))
        print(f'{edit} {name} {n}: worst/bound {r:.1f}')
        assert r > 1.0, (edit, name, n, r)


def test_self_mask_before_causal_mask_is_the_same_function():
    """the planted fault "self mask applied before the causal one" CANNOT leave any bound: a cell with equal positions is always
    causally visible (q_pos >= k_pos), so the causal mask never touches a self cell and the two orders give the same scores, bit for
    bit.  Stated here instead of a bound that would pretend to see it.  (What the -1e5 / -1e9 pair does fix is that a self cell
    outweighs every future cell: the rows that see only themselves have lse -1e5, not -1e9, in test_attention_case_conditions.)"""
    for name in ('c_lsh_t128_n2_dh32_dup', 'c_lsh_t256_n1_dh32_desc', 's_t33_dh32_lsh'):
        c, ref, _ = attn_case(name)
        bad = attn_ref64(c, edit=('self_first',))
        for n in ('out', 'lse', 'dq', 'dk', 'dv', 'dqk'):
            assert torch.equal(bad[n], ref[n]), (name, n)


def test_delta_from_the_unrounded_out_is_below_the_bounds():
    """delta = dO . out is formed from the STORED bf16 out (reformer.hip:655, :837).  A model that takes the float32 O instead moves dq
    and dk' by less than their bounds on every dropout case, so these tests cannot tell the two apart; the figures are printed.  The
    fault would be required to leave the bounds only if its effect exceeded them."""
    seen = 0
    for r in CHUNK_CASES:
        if r.get('p', 0.0) <= 0:
            continue
        c, ref, model = attn_case(r['name'])
        other = attn_ref64(c, rounded=True, delta_unrounded=True)
        for n in ('dq', 'dk'):
            eff = gap(other[n], model[n])
            print(f'delta from unrounded out, {r["name"]} {n}: moves the model by {eff:.3e} of max (b = {B_CHUNK[n]:.2e})')
            if eff > B_CHUNK[n]:
                assert _leaves(model, other, (n,), A_ATTN, B_CHUNK) > 1.0
                seen += 1
    print(f'{seen} outputs where the effect exceeds the bound')


# ---------------------------------------------------------------------------------------------------------------- hashing
@pytest.mark.parametrize('name', list(HASH_CASES))
def test_float32_hashing_differs_from_float64_only_on_near_ties(name):
    """what the GPU test asks of the device, asked of a float32 evaluation on the CPU (sequential sum over the head dimension): every
    differing token is a near-tie and fewer than 0.2 % differ; a deliberately wrong bucket is no near-tie"""
    c = hash_case(name)
    x, r = c['qk'].float(), c['rot'].float()
    acc = torch.zeros(c['proj'].shape, dtype=torch.float32)
    for e in range(c['dh']):
        acc += x[..., e].permute(0, 2, 1)[:, :, None, :, None] * r[:, e][None, :, :, None, :]
    got = hash_buckets(acc, c['factors'])
    differ, bad = hash_near_ties(c, got)
    print(f'{name}: float32 differs on {differ} of {got.numel()} tokens')
    assert bad == 0 and differ < 0.002 * got.numel()
    ref = hash_buckets(c['proj'], c['factors'])
    assert hash_near_ties(c, ref) == (0, 0)
    wrong = (ref + 1) % math.prod(c['factors'])
    differ, bad = hash_near_ties(c, wrong)
    assert differ == ref.numel() and bad > 0.99 * ref.numel()
