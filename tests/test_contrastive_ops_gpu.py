"""The kernels of contrastive search on the device (csrc/contrastive.hip) against torch / fp64 on their smallest risky shapes:
mxl_contrastive_topk, mxl_contrastive_step (bit-equal to mxl_contrastive_select on the same inputs) and mxl_ring_slot_broadcast.
Every test here fails without the feature: the entries do not exist there."""
import pytest
import torch

from symbolic_music_generation_amd import ops

pytestmark = pytest.mark.gpu

NEG = float('-inf')
PAD = 3


def _topk(dev, logp, K, sel, t=5, unfinished=None, width=9):
    B0 = sel.numel()
    ids = torch.full((B0 * K, width), -7, dtype=torch.int64, device=dev)
    t_dev = torch.tensor([t], dtype=torch.int32, device=dev)
    probs = torch.full((B0, K), -1.0, device=dev)
    dead = torch.full((B0, K), -1, dtype=torch.int32, device=dev)
    ops.contrastive_topk(logp, logp.shape[1], sel, ids, t_dev, probs, dead, unfinished, PAD)
    torch.cuda.synchronize()
    assert (ids[:, :t + 1] == -7).all() and (ids[:, t + 2:] == -7).all()           # only column t + 1 is written
    return ids[:, t + 1].view(B0, K), probs, dead


@pytest.mark.parametrize('B0', [1, 3])
@pytest.mark.parametrize('K', [2, 4, 16, 32])
@pytest.mark.parametrize('V', [40, 1195, 2049])
def test_topk_equals_torch_topk_and_fp64_softmax(dev, V, K, B0):
    g = torch.Generator().manual_seed(V * 100 + K * 3 + B0)
    # a permutation of distinct values per row: no ties
    logp = torch.stack([torch.randperm(V, generator=g).float() * 0.37 - 20.0 for _ in range(B0 * K)]).to(dev)
    sel = (torch.arange(B0, dtype=torch.int32) * 5 + 1).remainder(K).to(dev)       # different per sequence
    toks, probs, dead = _topk(dev, logp, K, sel)
    rows = logp[torch.arange(B0, device=dev) * K + sel.long()]
    want_v, want_i = rows.topk(K, dim=-1)
    assert torch.equal(toks, want_i)
    assert torch.equal(rows.gather(1, toks), want_v)
    want_p = torch.softmax(want_v.double(), -1)
    assert (probs.double() - want_p).abs().max().item() < 1e-6
    assert (dead == 0).all()


@pytest.mark.parametrize('V', [40, 2049])
def test_topk_ties_resolve_to_the_lower_token_id(dev, V):
    K, B0 = 4, 2
    logp = torch.full((B0 * K, V), -9.0, device=dev)
    # sequence 0 (row 0): three tokens tie for the best value, two for the next, one of them across the 256-thread stride
    logp[0, [V - 1, 7, 300 % V]] = -1.0
    logp[0, [5, V - 2]] = -2.0
    # sequence 1 (row K + 2): everything ties
    sel = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    toks, probs, dead = _topk(dev, logp, K, sel)
    first = sorted([V - 1, 7, 300 % V])
    assert toks[0].tolist() == first + [5]
    assert toks[1].tolist() == [0, 1, 2, 3]
    assert (probs[1] - 0.25).abs().max().item() < 1e-6 and (dead == 0).all()


@pytest.mark.parametrize('K', [2, 4, 16])
def test_topk_dead_candidates_and_finished_sequences(dev, K):
    V, B0 = 1195, 3
    g = torch.Generator().manual_seed(K)
    logp = torch.full((B0 * K, V), NEG)
    one = 900                                                        # sequence 0: a single finite entry
    logp[0, one] = -0.5
    keep = torch.randperm(V, generator=g)[:K - 1]                    # sequence 1: K - 1 finite entries
    logp[K, keep] = -torch.rand(K - 1, generator=g) - 0.1
    logp[2 * K] = torch.randn(V, generator=g)                        # sequence 2: finished
    logp = logp.to(dev)
    unfinished = torch.ones(B0 * K, dtype=torch.int32, device=dev)
    unfinished[2 * K:] = 0
    sel = torch.zeros(B0, dtype=torch.int32, device=dev)
    toks, probs, dead = _topk(dev, logp, K, sel, unfinished=unfinished)
    assert toks[0].tolist() == [one] * K and dead[0].tolist() == [0] + [1] * (K - 1)
    assert probs[0].tolist() == [1.0] + [0.0] * (K - 1)
    want_v, want_i = logp[K].topk(K - 1)
    assert toks[1, :K - 1].tolist() == want_i.tolist() and int(toks[1, K - 1]) == int(want_i[0])
    assert dead[1].tolist() == [0] * (K - 1) + [1] and float(probs[1, K - 1]) == 0.0
    assert (probs[1, :K - 1].double() - torch.softmax(want_v.double(), -1)).abs().max().item() < 1e-6
    assert toks[2].tolist() == [PAD] * K


# ---------------------------------------------------------------------------------------------------------------- step
def _step_case(dev, S, d, K, B0=3, seed=0):
    torch.manual_seed(seed + S * 7 + d + K)
    Smax = S + 3
    ctx = torch.randn(B0, Smax, d, device=dev).to(torch.bfloat16)
    near = ctx[:, torch.arange(K) % S].float()                       # candidates near context rows: cosines of every size
    hid = (near * torch.rand(B0, K, 1, device=dev) + 0.6 * torch.randn(B0, K, d, device=dev)).to(torch.bfloat16).reshape(B0 * K, d)
    hid = hid.contiguous()
    probs = torch.softmax(torch.randn(B0, K, device=dev), -1).contiguous()
    inv = torch.zeros(B0, Smax, device=dev)
    for b in range(B0):
        ops.row_inv_norm(ctx[b, :S], inv[b, :S], S)
    return ctx, inv, hid, probs, Smax


def _run_step(dev, ctx, inv, S, hid, probs, dead, K, alpha=0.6, unfinished=None, eos=-1, ids=None, stop_later=False):
    B0 = probs.shape[0]
    if ids is None:
        ids = torch.arange(B0 * K, device=dev)[:, None].repeat(1, S + 2) + 100
    t_dev = torch.tensor([S], dtype=torch.int32, device=dev)
    score = torch.zeros(B0 * K, device=dev)
    sel = torch.full((B0,), -1, dtype=torch.int32, device=dev)
    n_done = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.contrastive_step(ctx, inv, t_dev, hid, probs, dead, alpha, score, sel, ids, unfinished, n_done, eos, PAD, stop_later)
    torch.cuda.synchronize()
    return score, sel, ids, n_done


@pytest.mark.parametrize('K', [2, 16])
@pytest.mark.parametrize('d', [8, 520])
@pytest.mark.parametrize('S', [1, 3, 4, 5, 65])
def test_step_scores_are_bit_equal_to_contrastive_select(dev, S, d, K):
    ctx, inv, hid, probs, Smax = _step_case(dev, S, d, K)
    B0 = probs.shape[0]
    want = torch.empty(B0 * K, device=dev)
    want_sel = torch.empty(B0, dtype=torch.int64, device=dev)
    ops.contrastive_select(ctx, inv, S, hid, probs, 0.6, want, want_sel)
    before_ctx, before_inv = ctx.clone(), inv.clone()
    dead = torch.zeros(B0, K, dtype=torch.int32, device=dev)
    score, sel, ids, n_done = _run_step(dev, ctx, inv, S, hid, probs, dead, K)
    assert torch.equal(score, want)                                  # the same bits
    assert torch.equal(sel.long(), want_sel)
    c, h = before_ctx[:, :S].float(), hid.float().view(B0, K, d)
    cos = torch.einsum('bsd,bkd->bks', c / c.norm(dim=-1, keepdim=True), h / h.norm(dim=-1, keepdim=True))
    formula = 0.4 * probs - 0.6 * cos.max(-1).values
    assert (score.view(B0, K) - formula).abs().max().item() < 1e-3
    # the picked token in column t of all K rows, every other column as it was
    src = torch.arange(B0, device=dev) * K + sel.long()
    assert torch.equal(ids[:, S].view(B0, K), (src + 100)[:, None].expand(B0, K))
    assert torch.equal(ids[:, :S], torch.arange(B0 * K, device=dev)[:, None].repeat(1, S) + 100)
    assert torch.equal(ids[:, S + 1], torch.arange(B0 * K, device=dev) + 100)
    # context position t = the picked hidden row and its reciprocal norm, bit for bit; nothing else moved
    assert torch.equal(ctx[:, S], hid[src])
    want_inv = torch.empty(B0, device=dev)
    ops.row_inv_norm(hid[src].contiguous(), want_inv, B0)
    assert torch.equal(inv[:, S], want_inv)
    keep = torch.ones(Smax, dtype=torch.bool, device=dev)
    keep[S] = False
    assert torch.equal(ctx[:, keep], before_ctx[:, keep]) and torch.equal(inv[:, keep], before_inv[:, keep])
    assert int(n_done) == 0


def test_step_picks_the_first_maximum_and_never_a_dead_candidate(dev):
    S, d, K, B0 = 5, 8, 4, 3
    ctx, inv, hid, probs, _ = _step_case(dev, S, d, K, B0)
    # sequence 0: candidates 1 and 3 are the same row with the same probability and beat the others -> 1
    hid = hid.view(B0, K, d).clone()
    hid[0, 3] = hid[0, 1]
    hid = hid.view(B0 * K, d).contiguous()
    probs[0] = torch.tensor([0.0, 0.5, 0.0, 0.5], device=dev)
    # sequence 1: candidate 2 would win by the formula (its probability is overwhelming), and is dead
    probs[1] = torch.tensor([0.001, 0.001, 0.997, 0.001], device=dev)
    dead = torch.zeros(B0, K, dtype=torch.int32, device=dev)
    free, _, _, _ = _run_step(dev, ctx.clone(), inv.clone(), S, hid, probs, dead, K, alpha=0.01)
    assert int(free.view(B0, K)[1].argmax()) == 2                    # the formula alone picks it
    dead[1, 2] = 1
    score, sel, _, _ = _run_step(dev, ctx, inv, S, hid, probs, dead, K, alpha=0.01)
    sc = score.view(B0, K)
    assert float(sc[0, 1]) == float(sc[0, 3]) == float(sc[0].max()) and int(sel[0]) == 1
    assert float(sc[1, 2]) == NEG and int(sel[1]) != 2 and int(sel[1]) == int(sc[1].argmax())
    assert torch.equal(sc[0], free.view(B0, K)[0]) and torch.equal(sc[2], free.view(B0, K)[2])


@pytest.mark.parametrize('stop_later', [False, True])
def test_step_stop_rule(dev, stop_later):
    S, d, K, B0 = 3, 8, 2, 3
    ctx, inv, hid, probs, _ = _step_case(dev, S, d, K, B0)
    dead = torch.zeros(B0, K, dtype=torch.int32, device=dev)
    EOS = 77
    ids = torch.arange(B0 * K, device=dev)[:, None].repeat(1, S + 2) + 100
    ids[0:K, S] = EOS                                                # sequence 0 picks eos whichever candidate wins
    unfinished = torch.ones(B0 * K, dtype=torch.int32, device=dev)
    unfinished[2 * K:] = 0                                           # sequence 2 was finished before the step
    ids[2 * K:, S] = EOS                                             # (its candidates do not count)
    score, sel, ids, n_done = _run_step(dev, ctx, inv, S, hid, probs, dead, K, unfinished=unfinished, eos=EOS, ids=ids,
                                        stop_later=stop_later)
    assert ids[0:K, S].tolist() == [EOS] * K
    assert ids[K:2 * K, S].tolist() == [100 + K + int(sel[1])] * K
    assert ids[2 * K:, S].tolist() == [PAD] * K
    assert int(n_done) == 1
    # stop_later leaves `unfinished` to the advance launch that follows
    assert unfinished.tolist() == ([1] * K if stop_later else [0] * K) + [1] * K + [0] * K


# ---------------------------------------------------------------------------------------------------------------- rings
@pytest.mark.parametrize('t', [2, 5])
def test_ring_slot_broadcast_copies_one_slot(dev, t):
    M, L, B0, K, H, dh = 4, 2, 2, 3, 2, 8
    rows = B0 * K
    g = torch.Generator().manual_seed(t)
    rings = [torch.randn(rows, H, M, dh, generator=g).to(torch.bfloat16).to(dev) for _ in range(2 * L)]
    before = [r.clone() for r in rings]
    sel = torch.tensor([2, 1], dtype=torch.int32, device=dev)
    t_dev = torch.tensor([t], dtype=torch.int32, device=dev)
    ops.ring_slot_broadcast(rings, K, t_dev, sel, table=ops.beam_table(rings))
    torch.cuda.synchronize()
    slot = t % M
    others = [s for s in range(M) if s != slot]
    for r, r0 in zip(rings, before):
        for b in range(B0):
            src = b * K + int(sel[b])
            assert not torch.equal(r0[b * K + (int(sel[b]) + 1) % K, :, slot], r0[src, :, slot])      # the rows did differ
            for k in range(K):
                assert torch.equal(r[b * K + k, :, slot], r0[src, :, slot])
        assert torch.equal(r[:, :, others], r0[:, :, others])
