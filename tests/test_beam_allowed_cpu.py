"""`generate.beam_search(..., allowed=)` on the CPU decoder of tests/test_beam_cpu.py: the argument off changes nothing, and a token
that it bars stays out of every hypothesis."""
import pytest
import torch

from symbolic_music_generation_amd.generate import beam_search
from tests.test_beam_cpu import CASES, L, TP, V, _model_and_prompt, _OracleDecoder


def _run(model, prompt, eos, **kw):
    dec = _OracleDecoder(model, prompt.shape[0] * 3, L)
    return beam_search(dec, prompt, L, num_beams=3, num_return_sequences=2, eos_token_id=eos, return_scores=True, **kw)


@pytest.mark.parametrize('seed,eos,early', CASES)
def test_allowed_none_and_allow_all_change_nothing(seed, eos, early):
    model, prompt = _model_and_prompt(seed, eos)
    ids, sc = _run(model, prompt, eos)
    ids2, sc2 = _run(model, prompt, eos, allowed=None)
    assert torch.equal(ids, ids2) and torch.equal(sc, sc2)
    seen = []

    def everything(x):
        seen.append(tuple(x.shape))
        return torch.ones(x.shape[0], V, dtype=torch.bool)
    ids3, sc3 = _run(model, prompt, eos, allowed=everything)
    assert torch.equal(ids, ids3) and torch.equal(sc, sc3)
    assert seen[0] == (6, TP) and all(b[1] == a[1] + 1 for a, b in zip(seen, seen[1:]))     # it is shown ids[:, :cur_len]


@pytest.mark.parametrize('seed,eos,early', CASES)
def test_a_barred_token_stays_out_of_every_hypothesis(seed, eos, early):
    model, prompt = _model_and_prompt(seed, eos)
    free, _ = _run(model, prompt, eos)
    gen = free[:, TP:]
    cand = [t for t in gen.flatten().tolist() if t != eos]
    barred = max(set(cand), key=cand.count)                         # the token the free search uses most

    def allowed(x):
        ok = torch.ones(x.shape[0], V, dtype=torch.bool)
        ok[:, barred] = False
        return ok
    ids, sc = _run(model, prompt, eos, allowed=allowed)
    assert torch.equal(ids[:, :TP], prompt.repeat_interleave(2, 0))
    assert not (ids[:, TP:] == barred).any() and (free[:, TP:] == barred).any()
    assert torch.isfinite(sc).all()
