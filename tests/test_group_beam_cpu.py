"""`generate.group_beam_search` on the CPU, over tests/test_beam_cpu.py's stand-in decoder: the `allowed=` mask that makes it the
host reference of the rules under group beam search on the device, and the one-step Python reference of tests/beam_ref.py against
it and against `generate.beam_search` step for step -- which ties what the kernel tests compare mxl_beam_step and
mxl_group_beam_step with to the host functions, without a GPU."""
import pytest
import torch

from symbolic_music_generation_amd.generate import _beam_finalize, _BeamHyps, beam_search, group_beam_search
from tests.test_beam_cpu import CASES, L, TP, V, _finished_early, _model_and_prompt, _OracleDecoder
from tests.beam_ref import RefState, ref_step

KW = dict(num_beams=4, num_beam_groups=2, num_return_sequences=2, return_scores=True)


@torch.no_grad()
@pytest.mark.parametrize('diversity_penalty', [0.0, 0.8])
@pytest.mark.parametrize('seed,eos,early', CASES)
def test_a_mask_that_allows_everything_changes_nothing(seed, eos, early, diversity_penalty):
    model, prompt = _model_and_prompt(seed, eos)
    kw = dict(KW, diversity_penalty=diversity_penalty, eos_token_id=eos)
    want, w_sc = group_beam_search(_OracleDecoder(model, 8, L), prompt, L, **kw)
    seen = []

    def allowed(ids):
        seen.append(ids.shape[1])
        return torch.ones(ids.shape[0], V, dtype=torch.bool)
    got, g_sc = group_beam_search(_OracleDecoder(model, 8, L), prompt, L, allowed=allowed, **kw)
    assert torch.equal(got, want) and torch.equal(g_sc, w_sc)
    assert seen[0] == TP and seen == list(range(TP, TP + len(seen)))       # asked once per step, with the rows so far
    assert _finished_early(want, eos) == early


@torch.no_grad()
@pytest.mark.parametrize('diversity_penalty', [0.0, 0.8])
@pytest.mark.parametrize('seed,eos', [(1, 7), (2, 0)])
def test_a_barred_token_is_never_emitted(seed, eos, diversity_penalty):
    model, prompt = _model_and_prompt(seed, eos)
    kw = dict(KW, diversity_penalty=diversity_penalty, eos_token_id=eos)
    free, _ = group_beam_search(_OracleDecoder(model, 8, L), prompt, L, **kw)
    barred = sorted(set(free[:, TP:].reshape(-1).tolist()) - {eos})[::2]   # every other token that the free search emits
    assert barred
    mask = torch.ones(V, dtype=torch.bool)
    mask[barred] = False
    got, sc = group_beam_search(_OracleDecoder(model, 8, L), prompt, L, allowed=lambda ids: mask.expand(ids.shape[0], V), **kw)
    assert torch.equal(got[:, :TP], prompt.repeat_interleave(2, 0))
    assert not set(got[:, TP:].reshape(-1).tolist()) & set(barred)
    assert torch.isfinite(sc).all() and not torch.equal(got, free)


class _Recorder(_OracleDecoder):
    """keeps what every step of the search ranks: (log-probabilities, ids before the step)"""

    def __init__(self, *a):
        super().__init__(*a)
        self.seen = []

    def beam_logp(self):
        self.seen.append((self.logp.clone(), self.ids.clone()))
        return self.logp


@torch.no_grad()
@pytest.mark.parametrize('nb,ng', [(4, 2), (4, 4), (6, 3), (3, 1), (2, 1)])
@pytest.mark.parametrize('diversity_penalty', [0.0, 0.8])
@pytest.mark.parametrize('seed,eos,early', CASES)
def test_the_one_step_reference_is_the_host_function(seed, eos, early, diversity_penalty, nb, ng):
    """the kernel tests' ref_step, fed the log-probabilities that group_beam_search (ng = 1: beam_search, which the diversity
    penalty does not reach) ranked, leaves the ids that the search left, step after step, and its store and running scores finalise
    to the returned rows and scores"""
    model, prompt = _model_and_prompt(seed, eos)
    rows, gs = 2 * nb, nb // ng
    for stopping in (True, False):
        dec = _Recorder(model, rows, L)
        kw = dict(num_beams=nb, early_stopping=stopping, num_return_sequences=2, eos_token_id=eos, return_scores=True)
        if ng == 1:
            want, w_sc = beam_search(dec, prompt, L, **kw)
        else:
            want, w_sc = group_beam_search(dec, prompt, L, num_beam_groups=ng, diversity_penalty=diversity_penalty, **kw)
        scores = torch.full((2, nb), -1e9)
        scores[:, ::gs] = 0
        ref = RefState(dec.seen[0][1], scores.view(-1), 2, nb, torch.ones(1, rows, dtype=torch.int64))
        after = [ids for _, ids in dec.seen[1:]] + [dec.ids]
        for k, (logp, _) in enumerate(dec.seen):
            cur_len = TP + k
            ref_step(ref, logp, V, cur_len, eos, eos, 1.0, stopping, ng, diversity_penalty)
            assert torch.equal(ref.ids[:, :cur_len + 1], after[k][:, :cur_len + 1]), (stopping, k)
        hyps = []
        for b in range(2):
            h = _BeamHyps(nb, 1.0, stopping)
            h.beams, h.done = [(sc, torch.tensor(row)) for sc, row in ref.hyp[b]], ref.done[b]
            hyps.append(h)
        got, g_sc = _beam_finalize(hyps, nb, 2, ref.ids, TP + len(dec.seen), ref.scores, L, eos, eos, True)
        assert torch.equal(got, want) and torch.equal(g_sc, w_sc), stopping
        if (nb, ng) == (4, 2):                                             # the shape that CASES was chosen with
            assert _finished_early(want, eos) == early or not stopping
            assert ('added' in ref.events) == early, ref.events
            if diversity_penalty and seed == 1:
                assert {'hamming1', 'hamming2'} & ref.events, ref.events
