"""`generate.beam_search` / `generate.group_beam_search` on the CPU: they call no kernel themselves, only the decoder's beam hooks
(beam_prefill / beam_logp / beam_reorder / beam_advance, `ids`, `B`, `Tmax`, `eng.dev`, `eng.cfg.vocab_size`), so a stand-in
decoder over the fp32 oracle model drives them, and the result is compared with the oracle's own restatement of HF 4.25.1
(`ref_beam_search` / `ref_group_beam_search`).  Both sides run the prompt in one forward and then one token per forward with
carried mems, so the log-probabilities they rank are the same numbers: ids and scores must be equal, not close."""
from types import SimpleNamespace

import pytest
import torch

from oracle.transfoxl_ref import RefTransfoXLLMHeadModel, RefXLConfig, ref_beam_search, ref_group_beam_search
from symbolic_music_generation_amd.generate import beam_search, group_beam_search

V, TP, L = 64, 5, 14


class _OracleDecoder:
    """the beam hooks of XLDecoder over the oracle model: one row per beam, mems in place of the K/V rings"""

    def __init__(self, model, rows: int, max_total_len: int):
        self.model = model
        self.eng = SimpleNamespace(dev=torch.device('cpu'), cfg=model.config)
        self.B, self.Tmax = rows, max_total_len
        self.ids = torch.zeros(rows, max_total_len + 1, dtype=torch.int64)

    def _forward(self, x, mems):
        out = self.model(x, mems=mems)
        self.mems, self.logp = out.mems, out.prediction_scores[:, -1, :]

    def beam_prefill(self, prompt):
        self.ids.zero_()
        self.ids[:, :prompt.shape[1]] = prompt
        self._forward(prompt, None)

    def beam_logp(self):
        return self.logp

    def beam_reorder(self, beam_idx):
        self.ids.copy_(self.ids.index_select(0, beam_idx))
        self.mems = [m.index_select(1, beam_idx) for m in self.mems]         # time-major mems: (M, rows, d)

    def beam_advance(self, cur_len):
        self._forward(self.ids[:, cur_len - 1:cur_len], self.mems)


def _model_and_prompt(seed: int, eos: int):
    torch.manual_seed(seed)
    cfg = RefXLConfig.from_preset('debug', vocab_size=V, max_length=32)
    cfg.eos_token_id = eos
    model = RefTransfoXLLMHeadModel(cfg).eval()
    prompt = torch.randint(0, V, (2, TP), generator=torch.Generator().manual_seed(seed + 1))
    return model, prompt


def _finished_early(ids, eos):
    # open beams never hold a generated eos (an eos candidate is never continued), so one in the generated columns is the marker
    # or the padding that finalize writes after a hypothesis shorter than the longest row
    return bool((ids[:, TP:] == eos).any())


# (seed, eos, early).  early: the oracle alone finishes a hypothesis before max_length (asserted below) -- seed 1 was chosen for
# it: with either eos id, every search below puts an eos among its best candidates, which is what exercises the heap
# (_BeamHyps.add / is_done) and the eos / pad fill of the finalisation.  With seed 2 no eos is ever ranked: every beam stays open.
CASES = [(1, 0, True), (1, 7, True), (2, 0, False)]


@torch.no_grad()
@pytest.mark.parametrize('seed,eos,early', CASES)
def test_beam_search_equals_oracle(seed, eos, early):
    model, prompt = _model_and_prompt(seed, eos)
    ref_ids, ref_sc = ref_beam_search(model, prompt, L, num_beams=3, num_return_sequences=2, return_scores=True)
    dec = _OracleDecoder(model, prompt.shape[0] * 3, L)
    ids, sc = beam_search(dec, prompt, L, num_beams=3, num_return_sequences=2, eos_token_id=eos, return_scores=True)
    assert torch.equal(ids, ref_ids)
    assert torch.equal(sc, ref_sc)
    assert _finished_early(ref_ids, eos) == early


@torch.no_grad()
@pytest.mark.parametrize('diversity_penalty', [0.0, 0.8])
@pytest.mark.parametrize('seed,eos,early', CASES)
def test_group_beam_search_equals_oracle(seed, eos, early, diversity_penalty):
    model, prompt = _model_and_prompt(seed, eos)
    ref_ids, ref_sc = ref_group_beam_search(model, prompt, L, num_beams=4, num_beam_groups=2, diversity_penalty=diversity_penalty,
                                            num_return_sequences=2, return_scores=True)
    dec = _OracleDecoder(model, prompt.shape[0] * 4, L)
    ids, sc = group_beam_search(dec, prompt, L, num_beams=4, num_beam_groups=2, diversity_penalty=diversity_penalty,
                                num_return_sequences=2, eos_token_id=eos, return_scores=True)
    assert torch.equal(ids, ref_ids)
    assert torch.equal(sc, ref_sc)
    assert _finished_early(ref_ids, eos) == early
