"""mxl_group_beam_step at kernel level, against the one-step reference of tests/beam_ref.py (which tests/test_group_beam_cpu.py ties
to generate.group_beam_search step for step, without a GPU)."""

import pytest
import torch

from tests.beam_ref import MXL_EINVAL, NEG, DevState, RefState, compare as _compare, distinct_logp as _distinct_logp, ref_step

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the scorer
SHAPES = [(2, 2), (4, 2), (4, 4), (6, 3), (16, 2), (16, 16)]
VOCABS = [5, 257, 1190]
STEPS = 7


def scenario(ref: RefState, step: int, nb: int, ng: int, V: int, ldl: int, eos: int, pad: int, g: torch.Generator):
    """the log-probabilities of step `step` of the sweep, built from the reference state alone:
    0  a few popular tokens above the rest, the same for every row, so that later groups meet tokens that earlier ones chose
    1  an eos at rank 0 of group 0 (stored) and, with gs >= 2, a second one placed at rank gs of group 0 (skipped)
    2  popular tokens again; eos on top of every row behind group 0 but the item's last: the store holds nb - gs
    3  eos on top of every row of groups 0 and 1: group 0 fills the store -- under early_stopping the item is done there and the
       groups behind are not walked; otherwise they are, and group 1's hypotheses replace the worst entries
    4  popular tokens again, against a full store
    5  group 0 falls far below the store, an eos on top of it: rejected, and since that is group 0's best score the item is done
       without early_stopping too, the groups behind not walked
    6  every item is frozen"""
    rows, gs = ref.Bs * nb, nb // ng
    logp = _distinct_logp(rows, ldl, g)
    logp[:, eos] = -50.0 - torch.arange(rows) * 0.1
    in_item = torch.arange(rows) % nb
    if step in (0, 2, 4):
        popular = [t for t in torch.randperm(V, generator=g).tolist() if t not in (eos, pad)][:3]
        for t in popular:
            logp[:, t] = -0.7 - 0.3 * torch.rand(rows, generator=g)
    if step == 1:
        for b in range(ref.Bs):
            r0 = b * nb
            logp[r0, eos] = 0.5                                            # rank 0 of group 0
            if gs >= 2:
                rest = (logp[r0:r0 + gs, :V] + ref.scores[r0:r0 + gs, None])
                rest[:, eos] = NEG
                top = rest.reshape(-1).sort(descending=True).values
                target = (top[gs - 2].item() + top[gs - 1].item()) / 2    # behind gs - 1 others: rank gs
                logp[r0 + 1, eos] = target - ref.scores[r0 + 1].item()
    if step == 2:
        sel = (in_item >= gs) & (in_item < nb - 1)
        logp[sel, eos] = -0.01 * (1 + in_item[sel]).to(torch.float32)
    if step == 3:
        sel = in_item < gs
        logp[sel, eos] = -0.01 * (1 + in_item[sel]).to(torch.float32)
        sel = (in_item >= gs) & (in_item < 2 * gs)                         # well above group 0's, which stay the worse entries
        logp[sel, eos] = 50.0 - 0.01 * in_item[sel].to(torch.float32)
    if step == 5:
        sel = in_item < gs
        logp[sel] -= 5000.0
        logp[sel, eos] = -5000.01 - 0.01 * in_item[sel].to(torch.float32)
    return logp


def sweep_case(nb: int, ng: int, V: int, case: int):
    """(reference state, generator, the arguments of the case): 3 items, ld and ldl no multiples of 256"""
    Bs, ldl, ld = 3, V + 3, 13
    rows, eos, pad = Bs * nb, V - 2, 1
    pen = (0.3, 0.0, 1.5)[case % 3]
    lp = (1.0, 0.6)[case % 2]
    early = bool((case // 2) % 2)
    g = torch.Generator().manual_seed(1000 * nb + 100 * ng + V)
    ids = torch.randint(0, V, (rows, ld), generator=g)
    # far below what a step adds, so that a hypothesis stored late beats one stored early
    scores = (-100.0 - torch.randperm(rows, generator=g).to(torch.float32) * 0.01)
    words = torch.randperm(3 * rows, generator=g).view(3, rows) + 1
    return RefState(ids, scores, Bs, nb, words), g, dict(ldl=ldl, ld=ld, eos=eos, pad=pad, pen=pen, lp=lp, early=early)


def test_group_beam_step_follows_the_scorer(dev):
    """every shape of the sweep through seven consecutive steps (scenario); the events that the steps are built for are asserted on
    the reference, per case where the case must show them and over the sweep where a shape decides"""
    Tp, events, case = 4, {}, 0
    for nb, ng in SHAPES:
        for V in VOCABS:
            ref, g, a = sweep_case(nb, ng, V, case)
            case += 1
            d = DevState(ref, a['ld'], dev)
            cut_at = None
            for step in range(STEPS):
                logp = scenario(ref, step, nb, ng, V, a['ldl'], a['eos'], a['pad'], g)
                had_cut = 'cut' in ref.events
                beam_idx, moved = ref_step(ref, logp, V, Tp + step, a['eos'], a['pad'], a['lp'], a['early'], ng, a['pen'])
                if cut_at is None and not had_cut and 'cut' in ref.events:
                    cut_at = step
                d.step(logp.to(dev), V, Tp + step, a['eos'], a['pad'], a['lp'], a['early'], ng=ng, pen=a['pen'])
                _compare(ref, d, beam_idx, moved, (nb, ng, V, step, a))
            what = (nb, ng, V, a, ref.events)
            assert {'added', 'replaced' if not a['early'] else 'added', 'cut', 'frozen'} <= ref.events, what
            assert cut_at == (3 if a['early'] else 5) and all(ref.done), what     # group 0 filled the store / ended the item
            if nb // ng >= 2:
                assert 'skipped' in ref.events, what
            if not a['early']:
                assert 'rejected' in ref.events, what
            key = (a['pen'], a['early'])
            events[key] = events.get(key, set()) | ref.events
    assert {k[0] for k in events} == {0.3, 0.0, 1.5} and {k[1] for k in events} == {True, False}
    for (pen, early), ev in events.items():
        if pen > 0:
            assert {'hamming1', 'hamming2'} <= ev, (pen, early, ev)       # 0.3: the products are inexact in f32
        else:
            assert not {'hamming1', 'hamming2'} & ev


def _small(dev, nb, V, scores, n_words, seed, ld=8):
    g = torch.Generator().manual_seed(seed)
    rows = len(scores)
    ids = torch.randint(0, V, (rows, ld), generator=g)
    words = torch.randperm(n_words * rows, generator=g).view(n_words, rows) + 1
    ref = RefState(ids, torch.tensor(scores, dtype=torch.float32), rows // nb, nb, words)
    return ref, DevState(ref, ld, dev), g, words


def test_ties_and_the_hamming_count(dev):
    """one item of 4 beams in 2 groups, V = 11.  Group 0: two exactly equal best candidates, the lower flat index first; both
    choose token 6.  Group 1 under pen = 0.5 sees 6 lowered by exactly 1.0 (count 2): its best candidate without the penalty leaves
    the selection, and of the two that become exactly equal the lower flat index wins.  The same step with pen = 0 keeps it."""
    nb, ng, V, pad, eos = 4, 2, 11, 2, 9
    for pen in (0.5, 0.0):
        ref, d, g, _ = _small(dev, nb, V, [-1.0] * 4, 3, 7)
        logp = _distinct_logp(4, V + 3, g) - 10
        logp[0, 6] = logp[1, 6] = -0.5                                    # group 0: a tie, flat indices 6 < 11 + 6
        logp[2, 6] = -0.25                                                # group 1: best when free, -1.25 under the penalty
        logp[2, 3] = logp[3, 0] = -1.0                                    # group 1: an exact tie, flat indices 3 < 11 + 0
        beam_idx, moved = ref_step(ref, logp, V, 4, eos, pad, 1.0, True, ng, pen)
        assert beam_idx[:2] == [0, 1] and ref.ids[:2, 4].tolist() == [6, 6]
        if pen:
            assert beam_idx[2:] == [2, 3] and ref.ids[2:, 4].tolist() == [3, 0] and 'hamming2' in ref.events
            assert ref.scores[2:].tolist() == [-2.0, -2.0]
        else:
            assert beam_idx[2:] == [2, 2] and ref.ids[2:, 4].tolist() == [6, 3]
        d.step(logp.to(dev), V, 4, eos, pad, 1.0, True, ng=ng, pen=pen)
        _compare(ref, d, beam_idx, moved, ('ties', pen))


def test_dead_rows_do_not_count(dev):
    """2 items of 4 beams in 2 groups.  Item 0, group 0: one finite candidate for two beams, so its second row continues at -inf:
    it gets pad, -inf and a cleared `unfinished` word -- and does not count: pad is group 1's best token, and stays it under a
    penalty that would push it out if the dead row's pad counted.  Item 1, group 1 starts dead: its children are dead whatever
    their log-probabilities say."""
    nb, ng, V, pad, eos, pen = 4, 2, 11, 2, 9, 3.0
    ref, d, g, words = _small(dev, nb, V, [-1.0] * 4 + [-1.0, -1.0, NEG, NEG], 4, 8)
    ref.words[0, 6:8] = 0
    d.words[0, 6:8] = 0
    logp = _distinct_logp(8, V + 3, g) - 10
    logp[0:2, :V] = NEG
    logp[1, 4] = -0.25                                                    # item 0 group 0: row 1 token 4, then a -inf candidate
    logp[2, pad], logp[3, 4], logp[3, 5] = -0.5, -0.75, -1.0              # item 0 group 1: pad first; 4 is counted once, behind 5
    beam_idx, moved = ref_step(ref, logp, V, 4, eos, pad, 1.0, True, ng, pen)
    assert beam_idx[:2] == [1, 0] and ref.ids[:2, 4].tolist() == [4, pad] and ref.scores[1].item() == NEG
    assert {'dead', 'dead_uncounted', 'hamming1'} <= ref.events
    assert beam_idx[2] == 2 and ref.ids[2, 4].item() == pad and ref.scores[2].item() == -1.5
    assert beam_idx[3] == 3 and ref.ids[3, 4].item() == 5                 # ... while the live row's 4 did count
    assert beam_idx[6:] == [6, 6] and ref.ids[6:, 4].tolist() == [pad, pad]
    d.step(logp.to(dev), V, 4, eos, pad, 1.0, True, ng=ng, pen=pen)
    _compare(ref, d, beam_idx, moved, 'dead')
    assert d.scores[1].item() == NEG and d.words[0, 1].item() == 0
    assert d.words[1:, 1].tolist() == words[1:, 0].tolist()               # the other words are the source's
    # the next step: item 0's dead row is overwritten by a second child of its live neighbour; item 1's dead group stays dead
    logp = _distinct_logp(8, V + 3, g) - 10
    beam_idx, moved = ref_step(ref, logp, V, 5, eos, pad, 1.0, True, ng, pen)
    assert beam_idx[:2] == [0, 0] and ref.scores[1].item() > NEG
    assert ref.scores[6:].tolist() == [NEG, NEG] and ref.ids[6:, 5].tolist() == [pad, pad] and ref.words[0, 6:].tolist() == [0, 0]
    d.step(logp.to(dev), V, 5, eos, pad, 1.0, True, ng=ng, pen=pen)
    _compare(ref, d, beam_idx, moved, 'dead, next step')


def test_rule_words_follow_their_beams_inside_the_groups(dev):
    nb, ng, V, ld = 4, 2, 40, 8
    ref, d, g, words = _small(dev, nb, V, [-1.0] * 4, 8, 9)
    logp = _distinct_logp(nb, V + 3, g) - 10
    logp[1, 30], logp[0, 31] = -0.1, -0.2                                 # group 0: a swap
    logp[3, 5], logp[3, 6] = -0.1, -0.2                                   # group 1: a duplicate
    beam_idx, moved = ref_step(ref, logp, V, 4, V - 1, 0, 1.0, True, ng, 0.0)
    assert beam_idx == [1, 0, 3, 3] and moved == [1]
    d.step(logp.to(dev), V, 4, V - 1, 0, 1.0, True, ng=ng, pen=0.0)
    _compare(ref, d, beam_idx, moved, 'words')
    assert d.words.cpu().tolist() == words[:, [1, 0, 3, 3]].tolist()
    # without the word buffer the same step leaves it alone
    ref2, d2, _, _ = _small(dev, nb, V, [-1.0] * 4, 8, 9)
    d2.step(logp.to(dev), V, 4, V - 1, 0, 1.0, True, words=False, ng=ng, pen=0.0)
    assert d2.beam_idx.tolist() == [1, 0, 3, 3] and torch.equal(d2.words.cpu().to(torch.int64), words)
    assert torch.equal(d2.ids.cpu(), ref.ids)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_argument_errors(dev):
    from symbolic_music_generation_amd._lib import lib
    L = lib()
    i32 = dict(device=dev, dtype=torch.int32)
    f = torch.zeros(64, 16, device=dev)
    ids = torch.zeros(64, 8, device=dev, dtype=torch.int64)
    z = torch.zeros(64, **i32)
    P = lambda t: t.data_ptr()

    def step(nb=4, ng=2, pen=0.5, Bs=2, hyp_n=P(z), words=None, n_words=0, V=16):
        return L.mxl_group_beam_step(P(f), 16, P(f), P(ids), 8, P(z), Bs, nb, ng, pen, V, 3, 0, 1.0, 1, P(ids), P(z), P(f), hyp_n, P(z),
                                     P(z), P(z), P(z), words, n_words, 64, None)
    assert step(nb=6, ng=4) == MXL_EINVAL                                 # nb % ng != 0
    assert step(ng=1) == MXL_EINVAL
    assert step(nb=17, ng=17) == MXL_EINVAL and step(nb=34, ng=2) == MXL_EINVAL
    assert step(pen=-0.5) == MXL_EINVAL and step(pen=float('inf')) == MXL_EINVAL
    assert step(ng=8) == MXL_EINVAL                                       # more groups than beams
    assert step(hyp_n=None) == MXL_EINVAL and step(words=P(z), n_words=0) == MXL_EINVAL and step(V=1) == MXL_EINVAL
    torch.cuda.synchronize()
    assert not f.any() and not ids.any() and not z.any()                  # nothing was launched
