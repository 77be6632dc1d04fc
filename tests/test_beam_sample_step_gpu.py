"""mxl_beam_sample_step at kernel level against tests/beam_sample_ref.ref_sample_step (tests.beam_ref.ref_step under the
replace-score rule), exact in ids, words, indices, scores and store; mxl_beam_step on the same state still gives its old result; and a
chain of (draw, step, advance) rounds over synthetic log-probabilities against the reference chain.  Fails without the feature: the
entries do not exist."""
import numpy as np
import pytest
import torch

from tests import beam_sample_ref as R
from tests.beam_ref import NEG, DevState, RefState, compare, ref_step

pytestmark = pytest.mark.gpu
FILL = 7.0


class SampleDev(DevState):
    def sample_step(self, drawn, V, cur_len, eos, pad, lp, early, set_t=True):
        from symbolic_music_generation_amd import ops
        if set_t:
            self.t.fill_(cur_len - 1)
        ops.beam_sample_step(drawn, V, self.scores, self.ids, self.t, self.hyp_len.shape[1], eos, pad, lp, early, self.hyp_ids,
                             self.hyp_len, self.hyp_score, self.hyp_n, self.done, self.n_done, self.beam_idx, self.moved,
                             words=self.words, n_words=self.words.shape[0])


def _drawn(Bs, nb, V, ldl, g, eos, n_finite=None):
    """a host-built `drawn`: per item 2 * nb (or n_finite[b]) finite entries at distinct cells outside the eos column, pairwise distinct
    values in (-20, -10); -inf elsewhere in the V columns, FILL beyond"""
    d = torch.full((Bs * nb, ldl), FILL)
    d[:, :V] = NEG
    cells = [c for c in range(nb * V) if c % V != eos]
    for b in range(Bs):
        n = 2 * nb if n_finite is None else n_finite[b]
        pick = torch.randperm(len(cells), generator=g)[:n].tolist()
        vals = -10.0 - 10.0 * torch.randperm(1000, generator=g)[:n].to(torch.float32) / 1000
        for k, i in enumerate(pick):
            d[b * nb + cells[i] // V, cells[i] % V] = vals[k]
    return d


def _set_eos(d, b, nb, V, eos, j, value):
    """put an eos candidate into item b's row j in place of the item's lowest non-eos candidate: the item keeps its count"""
    blk = d[b * nb:(b + 1) * nb, :V]
    body = blk.clone()
    body[:, eos] = float('inf')
    body[~torch.isfinite(blk)] = float('inf')
    low = int(body.reshape(-1).argmin())
    blk[low // V, low % V] = NEG
    blk[j, eos] = value


@pytest.mark.parametrize('early', [True, False])
@pytest.mark.parametrize('lp', [1.0, 0.6])
@pytest.mark.parametrize('nb,V', [(2, 7), (3, 300), (16, 37), (5, 2048)])
def test_sample_step_follows_the_scorer(dev, nb, V, lp, early):
    """six consecutive steps on one state.  0: a plain step, in which item 1 has fewer finite candidates than beams (a dead row), and
    on which mxl_beam_step still gives its own result.  1: an eos at rank 0 (stored, with a poor score) and a second at rank nb
    (skipped); a finite entry in the dead row counts for nothing.  2: every beam's eos on top: the store fills and the last replaces
    the worst.  3: without early_stopping a poor eos at rank 0 against a full store (rejected), after which the item is done.
    4, 5: frozen items."""
    Bs, ldl, ld, Tp = 3, V + 3, 12, 4
    rows, eos, pad = Bs * nb, V - 2, 1
    g = torch.Generator().manual_seed(1000 * nb + V)
    ids = torch.randint(0, V, (rows, ld), generator=g)
    scores = -torch.rand(rows, generator=g) * 3
    words = torch.randperm(3 * rows, generator=g).view(3, rows) + 1
    ref = RefState(ids, scores, Bs, nb, words)
    d = SampleDev(ref, ld, dev)
    for step in range(6):
        cur_len = Tp + step
        drawn = _drawn(Bs, nb, V, ldl, g, eos, n_finite=[2 * nb, nb - 1, 2 * nb] if step == 0 else None)
        if step == 0:                                                          # the same state and matrix under plain beam search
            plain, dp = RefState(ids, scores, Bs, nb, words), DevState(RefState(ids, scores, Bs, nb, words), ld, dev)
            bi, mv = ref_step(plain, drawn, V, cur_len, eos, pad, lp, early)
            dp.step(drawn.to(dev), V, cur_len, eos, pad, lp, early)
            compare(plain, dp, bi, mv, ('plain', nb, V))
        if step == 1:
            dead = [r for r in range(nb, 2 * nb) if ref.scores[r] == NEG]
            assert dead
            drawn[dead[0], 0] = -0.001                                         # the best value of the matrix, in a dead row
            for b in range(Bs):
                _set_eos(drawn, b, nb, V, eos, 0, -9.0)                        # rank 0: every other value is below -10
                live = [j for j in range(nb) if ref.scores[b * nb + j] != NEG]
                blk = drawn[b * nb:(b + 1) * nb, :V].clone()
                blk[:, eos] = NEG
                blk[[j for j in range(nb) if j not in live]] = NEG
                top = blk.reshape(-1).sort(descending=True).values
                if len(live) > 1 and torch.isfinite(top[nb - 1]):
                    _set_eos(drawn, b, nb, V, eos, live[1], (top[nb - 2].item() + top[nb - 1].item()) / 2)      # rank nb
        if step == 2:
            for b in range(Bs):
                for j in range(nb):
                    _set_eos(drawn, b, nb, V, eos, j, -0.01 * (1 + j))
        if step == 3:
            for b in range(Bs):
                _set_eos(drawn, b, nb, V, eos, 0, -9.5)
        beam_idx, moved = R.ref_sample_step(ref, drawn, V, cur_len, eos, pad, lp, early)
        d.sample_step(drawn.to(dev), V, cur_len, eos, pad, lp, early)
        compare(ref, d, beam_idx, moved, (step, nb, V, lp, early))
        fin = ref.scores != NEG                                                # a running score is an entry of the matrix, bit for bit
        assert all(bool((drawn[:, :V] == s).any()) for b in range(Bs) if not ref.done[b] for s in ref.scores[b * nb:(b + 1) * nb][
            fin[b * nb:(b + 1) * nb]]), step
    # (under early_stopping an item is done once its store is full: nothing is weighed against a full store)
    assert {'added', 'skipped', 'replaced', 'dead', 'frozen'} | (set() if early else {'rejected'}) <= ref.events, ref.events
    assert all(ref.done)


def test_chain_of_draw_step_advance(dev):
    """12 rounds of mxl_beam_sample_draw, mxl_beam_sample_step and mxl_decode_advance on one state against the reference chain: every
    round's warped rows and drawn sets against the float64 reference (the chain follows the device's set where an item is undecided,
    and takes the device's w as the scores, which the step must hand on bit for bit), the step exact, the counter one further"""
    from symbolic_music_generation_amd import ops
    Bs, nb, V, ldl, ld, Tp = 3, 3, 37, 40, 20, 4
    rows, eos, pad, lp, early = Bs * nb, 5, 1, 1.0, False
    warp = dict(k=8, p=0.95, typ=1.0, temp=0.9)
    seed, ctr0 = R.CASE_SEED, (7 << 32) | 0xFFFFFFFA                           # the low half of the counter wraps inside the chain
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(0, V, (rows, ld), generator=g)
    scores = torch.tensor(([0.0] + [-1e9] * (nb - 1)) * Bs)
    words = torch.randperm(3 * rows, generator=g).view(3, rows) + 1
    ref = RefState(ids, scores, Bs, nb, words)
    d = SampleDev(ref, ld, dev)
    d.t.fill_(Tp - 1)
    rng = torch.tensor([ctr0], dtype=torch.int64, device=dev)
    undecided = 0
    for rnd in range(12):
        cur_len = Tp + rnd
        raw = torch.randn(rows, V, generator=g) * 1.5
        raw[:, eos] += 1.5 if rnd >= 2 else -20.0                              # eos becomes likely from the third round on
        raw[torch.rand(rows, V, generator=g) < 0.2] = NEG                      # what the rules would bar
        raw[:, 9] = 0.0                                                        # (one token always allowed)
        if rnd == 4:
            raw[nb] = NEG                                                      # item 1: two allowed tokens in its first row ...
            raw[nb, 9], raw[nb, 11] = 0.0, -0.5
        logp = torch.full((rows, ldl), 5.0)
        logp[:, :V] = torch.log_softmax(raw, -1)
        if rnd == 4:
            logp[nb + 1:2 * nb, :V] = NEG                                      # ... and none in the others: a beam must die
        drawn, ow = torch.full((rows, ldl), FILL, device=dev), torch.empty(rows, V, device=dev)
        ops.beam_sample_draw(logp.to(dev), V, d.scores, nb, rng, seed, drawn, top_k=warp['k'], top_p=warp['p'],
                             temperature=warp['temp'], typical_p=warp['typ'], out_warped=ow)
        live = (ref.scores != NEG).numpy()
        refs = [R.warp_ref(logp[r, :V].numpy(), **warp) if live[r] else dict(w=np.full(V, NEG), margin=np.inf) for r in range(rows)]
        w = np.stack([r['w'] for r in refs])
        got, fin = ow.cpu().numpy().astype(np.float64), np.isfinite(w)
        sure = np.array([r['margin'] > R.DELTA_W for r in refs])
        assert np.array_equal(np.isfinite(got)[sure], fin[sure]), rnd
        both = fin & np.isfinite(got)
        assert np.abs(got[both] - w[both]).max() <= R.DELTA_W, rnd
        words_now = R.cand_word(seed, ctr0 + rnd, np.arange(rows)[:, None], np.arange(V)[None, :])
        host = drawn.cpu()
        at = torch.isfinite(host[:, :V])
        assert torch.equal(host[:, :V][at].view(torch.int32), ow.cpu()[at].view(torch.int32)) and (host[:, V:] == FILL).all()
        for b, it in enumerate(R.draw_ref(w, words_now, nb)):
            if sure[b * nb:(b + 1) * nb].all():
                verdict = R.judge_item(it, at.view(Bs, -1)[b].nonzero().view(-1).tolist(), nb)
                assert verdict is None, (rnd, b, verdict)
            undecided += not it['decided']
        beam_idx, moved = R.ref_sample_step(ref, host, V, cur_len, eos, pad, lp, early)
        d.sample_step(drawn, V, cur_len, eos, pad, lp, early, set_t=False)
        compare(ref, d, beam_idx, moved, ('chain', rnd))
        ops.decode_advance(d.t, rng)
        assert int(d.t) == cur_len and int(rng) == ctr0 + rnd + 1
    print('events', sorted(ref.events), 'undecided items', undecided, 'done', ref.done)
    assert {'added', 'dead'} <= ref.events and undecided <= 2
