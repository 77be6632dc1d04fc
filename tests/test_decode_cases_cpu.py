"""CPU side of the decode-step kernel tests (no GPU): the float64 closed form of oracle/decode_cases.py against an independent float64
evaluation, the rounded-model gaps behind B_OUT / B_BD / B_OUT_FULL of tests/test_decode_cases_gpu.py measured again, the conditions
the input families promise, and the teeth of the bound -- planted faults in the reference alone must leave it."""
import numpy as np
import pytest
import torch

from oracle import decode_cases as D
from oracle.kernel_cases import A_BF16, check_gap, gap, worst
from tests.test_decode_cases_gpu import B_BD, B_OUT, B_OUT_FULL

ARMS = list(D.attn_arms())
ARM_IDS = [f'{n}-p{p}-{f}' for n, p, f in ARMS]
EDGE_ARMS = [a for a in ARMS if a[2].startswith('edges')]
PHANTOM_ARMS = [a for a in ARMS if a[2] == 'phantom']


# ---------------------------------------------------------------------------------------------------------------- reference check
@pytest.mark.parametrize('name', list(D.ATTN_CASES))
def test_closed_form_equals_dense_reference(name):
    """attn_ref64 == oracle/relattn_ref.relattn_dense (one query, zero memories in the never-written slots) to 1e-10 of max|ref|"""
    c0 = D.ATTN_CASES[name]
    for fam in D.families(c0, c0['pieces'][-1]):
        c = D.attn_case(name, fam, c0['pieces'][-1])
        ref = D.attn_ref64(c)[0]
        other = D.dense_check(c)
        err = ((ref - other).abs().max() / ref.abs().max()).item()
        print(f'decode {name} {fam}: closed form vs dense reference {err:.2e} of max|ref|')
        assert err <= 1e-10, (name, fam, err)


@pytest.mark.parametrize('name', list(D.COMPOSITE_CASES))
def test_composite_closed_form_equals_dense_reference(name):
    """the composite from q, rd, r_r_bias: relattn_dense takes the table itself -- content operand bf16(q + r_w_bias), positional
    operand bf16(q + r_r_bias) in the two halves of a head of twice the width"""
    from oracle.relattn_ref import relattn_dense
    c = D.composite_case(name)
    B, H, dh, M, tm = c['B'], c['H'], c['dh'], c['M'], c['tm']
    qc = torch.from_numpy(D.q_biased(c['q'], c['rwb'])).double()
    qp = torch.from_numpy(D.q_biased(c['q'], c['rrb'])).double()
    order = (tm - (M - 1 - torch.arange(M))) % M
    z = torch.zeros(B, M, H, dh, dtype=torch.float64)
    k = torch.cat([c['kc'].double()[:, :, order].transpose(1, 2), z], -1)
    v = torch.cat([c['vc'].double()[:, :, order].transpose(1, 2), z], -1)
    rd = torch.cat([torch.zeros(M, H, dh, dtype=torch.float64), c['rd'].double().view(M, H, dh)], -1)
    zero = torch.zeros(H, 2 * dh, dtype=torch.float64)
    outs = []
    for b in range(B):       # (the biases of relattn_dense are per head: the difference of the two operands rides in one, per sequence)
        q = torch.cat([torch.zeros(1, 1, H, dh, dtype=torch.float64), qp[b][None, None]], -1)
        rwb = torch.cat([qc[b], -qp[b]], -1)
        o, _ = relattn_dense(q, k[b:b + 1], v[b:b + 1], rd, rwb, zero, M, scale=c['scale'], dtype=torch.float64)
        outs.append(o[0, 0, :, :dh])
    other = torch.stack(outs)
    ref = D.composite_ref64(c)
    err = ((ref - other).abs().max() / ref.abs().max()).item()
    print(f'decode {name}: composite closed form vs dense reference {err:.2e} of max|ref|')
    assert err <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- gaps
def test_gaps_stay_under_the_bounds():
    """every case and arm: the rounded model's gap stays under the absolute term built from the largest of them"""
    top = (0.0, None)
    for name, p, fam in ARMS:
        g = D.attn_gap(name, p, fam)
        print(f'decode attention {name} pieces {p} {fam}: gap {g:.3e}')
        check_gap(g, B_OUT)
        top = max(top, (g, f'{name} pieces {p} {fam}'))
    print(f'decode attention: largest gap {top[0]:.3e} ({top[1]}) -> B_OUT {B_OUT:.2e}')
    assert 4 * top[0] <= B_OUT <= 4.5 * top[0], 'B_OUT is 4 x the largest gap, rounded up'
    gb = [(D.bd_gap(n), n) for n in D.BD_CASES]
    for n in D.COMPOSITE_CASES:                                      # the composite's BD is judged under the same constant
        c = D.composite_case(n)
        gb.append((gap(D.composite_bd(c, np.float32), D.composite_bd(c)), n))
    for g, n in gb:
        print(f'decode bd {n}: gap {g:.3e}')
        check_gap(g, B_BD)
    tb = max(gb)
    print(f'decode bd: largest gap {tb[0]:.3e} ({tb[1]}) -> B_BD {B_BD:.2e}')
    assert 4 * tb[0] <= B_BD <= 4.5 * tb[0]
    tc = max((D.composite_gap(n), n) for n in D.COMPOSITE_CASES)
    for n in D.COMPOSITE_CASES:
        check_gap(D.composite_gap(n), B_OUT_FULL)
    print(f'decode composite: largest gap {tc[0]:.3e} ({tc[1]}) -> B_OUT_FULL {B_OUT_FULL:.2e}')
    assert 4 * tc[0] <= B_OUT_FULL <= 4.5 * tc[0]


# ---------------------------------------------------------------------------------------------------------------- case conditions
def _is_bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


@pytest.mark.parametrize('name,pieces,fam', ARMS, ids=ARM_IDS)
def test_case_conditions(name, pieces, fam):
    c = D.attn_case(name, fam, pieces)
    B, H, nv, M = c['B'], c['H'], c['nvalid'], c['M']
    for k in ('qkv', 'rwb', 'kc', 'vc', 'bd'):
        assert _is_bf16_exact(c[k]), k
    assert (c['kc'][:, :, nv:] == 0).all() and (c['vc'][:, :, nv:] == 0).all()
    assert 'live' in name or name == 'big_m16128' or (B >= 2 and H >= 2)
    out, p = D.attn_ref64(c)
    assert (p.sum(-1) - 1).abs().max().item() <= 1e-12
    flat = out.reshape(B * H, -1)
    for i in range(B * H):                                          # sequences and heads differ
        for j in range(i):
            assert not torch.allclose(flat[i], flat[j], rtol=1e-3, atol=0)
    if fam == 'random':
        return
    fav = c['fav']
    share = p[:, :, fav].reshape(B * H, len(fav))
    if fam == 'phantom':
        assert nv <= fav[0] < M
        assert (share >= 0.5).all(), share.min().item()
        assert out.abs().max().item() < 0.05 * c['vc'].abs().max().item()
        return
    assert fav == D.edge_chunks(c, pieces)[int(fam[5:])] and len(fav) <= D.EDGE_CHUNK
    ok = (share >= 1.0 / (2 * len(fav))).all(1).double().mean().item()
    assert ok >= 0.9, (ok, share.min().item(), 1.0 / (2 * len(fav)))
    vf = c['vc'][:, :, [s for s in fav if s < nv]]
    if vf.shape[2] > 1:                                             # large and mutually distinct value rows
        assert vf.abs().min().item() >= 2.0
        assert (torch.cdist(vf.reshape(B * H, vf.shape[2], -1), vf.reshape(B * H, vf.shape[2], -1))
                + 1e9 * torch.eye(vf.shape[2])).min().item() > 4.0


def test_favoured_sets_cover_the_index_edges():
    """the union of a case's edge chunks is the whole set, and the set names what the docstring says"""
    for name, c in D.ATTN_CASES.items():
        for p in c['pieces']:
            allf = sorted(s for ch in D.edge_chunks(c, p) for s in ch)
            assert allf == D.favoured_slots(c, p)
            want = {0, c['nvalid'] - 1, c['tm'], (c['t'] + 1) % c['M']}
            for lo, hi, plo, phi in D.piece_bounds(c['nvalid'], c['M'], p):
                want |= ({lo, hi - 1} if hi > lo else set()) | ({plo, phi - 1} if phi > plo else set())
            assert want <= set(allf)
    ST = D.steps_per_batch(64)
    assert {ST - 1, ST, 2 * ST - 1, 2 * ST} <= set(D.favoured_slots(D.ATTN_CASES['d64_n2049_above'], 1))
    assert [D.steps_per_batch(x) for x in (64, 32, 16)] == [512, 1024, 2048]


def test_piece_bounds_partition_the_ring():
    for name, c in D.ATTN_CASES.items():
        for p in c['pieces']:
            seen = np.zeros(c['M'], dtype=int)
            for lo, hi, plo, phi in D.piece_bounds(c['nvalid'], c['M'], p):
                seen[lo:hi] += 1
                seen[plo:phi] += 1
                assert hi <= c['nvalid'] <= plo
            assert (seen == 1).all(), (name, p)
    b = D.piece_bounds(40, 128, 8)
    assert [x[1] - x[0] for x in b] == [32, 8, 0, 0, 0, 0, 0, 0]             # pc_tail_empty: the last pieces hold no written slot


def test_other_inputs_are_bf16_exact():
    for n in D.BD_CASES:
        c = D.bd_case(n)
        assert _is_bf16_exact(c['qr']) and _is_bf16_exact(c['rd'])
    for n in D.COMPOSITE_CASES:
        c = D.composite_case(n)
        assert all(_is_bf16_exact(c[k]) for k in ('qkv', 'kc', 'vc', 'rwb', 'rrb', 'rd'))
    for a in D.QKV_CASES:
        assert _is_bf16_exact(D.qkv_case(*a)['rrb'])
    assert {r[0] for r in D.QKV_CASES} >= {1, 64} and all(r[3] & (r[3] - 1) for r in D.QKV_CASES)
    assert {c['B'] for c in D.BD_CASES.values()} == {1, 15, 16, 17, 48, 49, 64}
    assert {c['M'] for c in D.BD_CASES.values()} == {1, 63, 64, 65, 255, 256, 257, 300, 301, 1028}


# ---------------------------------------------------------------------------------------------------------------- teeth
def _ratio(c, **edit):
    ref = D.attn_ref64(c)[0]
    return worst(D.attn_ref64(c, **edit)[0], ref, A_BF16, B_OUT)[0]


@pytest.mark.parametrize('name,pieces,fam', EDGE_ARMS, ids=[f'{n}-p{p}-{f}' for n, p, f in EDGE_ARMS])
def test_teeth_dropped_slot_and_shifted_distance(name, pieces, fam):
    """each favoured slot removed, one at a time, and the positional term read one distance off: the faulted reference leaves the bound"""
    c = D.attn_case(name, fam, pieces)
    for s in c['fav']:
        r = _ratio(c, drop=(s,))
        print(f'decode teeth {name} pieces {pieces} {fam}: slot {s} dropped -> worst/bound {r:.1f}')
        assert r > 1.0, (name, fam, s, r)
    for sh in (1, -1):
        r = _ratio(c, shift=sh)
        print(f'decode teeth {name} pieces {pieces} {fam}: distance {sh:+d} -> worst/bound {r:.1f}')
        assert r > 1.0, (name, fam, sh, r)


@pytest.mark.parametrize('name,pieces,fam', PHANTOM_ARMS, ids=[f'{n}-p{p}' for n, p, f in PHANTOM_ARMS])
def test_teeth_never_written_slots_out_of_the_denominator(name, pieces, fam):
    c = D.attn_case(name, fam, pieces)
    r = _ratio(c, no_phantom_den=True)
    print(f'decode teeth {name} phantom: never-written slots out of the denominator -> worst/bound {r:.1f}')
    assert r > 1.0
    r = _ratio(c, drop=(c['fav'][0],))
    print(f'decode teeth {name} phantom: the favoured never-written slot dropped -> worst/bound {r:.1f}')
    assert r > 1.0


MERGE_ARMS = [(n, p, 'phantom') for n in ('pc_mixed', 'pc_tail_empty', 'live_p4') for p in D.ATTN_CASES[n]['pieces'] if p > 1] \
    + [('pc_full', 8, 'edges0')]


@pytest.mark.parametrize('name,pieces,fam', MERGE_ARMS, ids=[f'{n}-p{p}-{f}' for n, p, f in MERGE_ARMS])
def test_teeth_merge_with_one_pieces_maximum(name, pieces, fam):
    """partials scaled by different maxima merged as if every piece's maximum were piece 0's; on inputs whose piece maxima clearly
    differ: the piece that holds the favoured slot(s) sits ln(M) + 4 or more above a piece that holds none"""
    c = D.attn_case(name, fam, pieces)
    mx = D.piece_maxima(c, pieces)
    held = np.isfinite(mx).all((0, 1))
    spread = (mx[:, :, held].max(-1) - mx[:, :, held].min(-1)).min()
    assert held.sum() >= 2 and spread > 2.0, spread
    r = _ratio(c, merge_as=(pieces, 0))
    print(f'decode teeth {name} pieces {pieces} {fam}: merge with one maximum (piece maxima differ by >= {spread:.1f}) -> worst/bound {r:.1f}')
    assert r > 1.0
    assert _ratio(c) == 0.0
