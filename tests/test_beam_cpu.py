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


BEAM_SAMPLE_GOLDEN = 'tests/golden/host_beam_sample.pt'
BEAM_SAMPLE = dict(num_beams=3, do_sample=True, num_return_sequences=2, top_k=16, temperature=0.9, renormalize_logits=True,
                   return_scores=True)


class _TapeDecoder:
    """the beam hooks over a tape: step k serves tape[k] (rows, V), in float64, whatever the beams did; ids follow their beams.  In
    float64 the last-place differences between the kernels of different CPUs (the order of a sum in softmax) stay far below the
    float32 that the running scores are kept in and below the spacing of the draws, so what a search returns holds on any CPU"""

    def __init__(self, tape, rows: int, max_total_len: int):
        self.tape, self.B, self.Tmax = tape, rows, max_total_len
        self.eng = SimpleNamespace(dev=torch.device('cpu'), cfg=SimpleNamespace(vocab_size=V))
        self.ids = torch.zeros(rows, max_total_len + 1, dtype=torch.int64)

    def beam_prefill(self, prompt):
        self.ids.zero_()
        self.ids[:, :prompt.shape[1]] = prompt
        self.k = 0

    def beam_logp(self):
        return self.tape[self.k].double()

    def beam_reorder(self, beam_idx):
        self.ids.copy_(self.ids.index_select(0, beam_idx))

    def beam_advance(self, cur_len):
        self.k += 1


def _beam_sample_from_tape(seed, eos, tape):
    prompt = _model_and_prompt(seed, eos)[1]
    return beam_search(_TapeDecoder(tape, prompt.shape[0] * 3 * 2, L), prompt, L, eos_token_id=eos,
                       generator=torch.Generator().manual_seed(seed), **BEAM_SAMPLE)


@torch.no_grad()
def beam_sample_record() -> dict:
    """what tests/golden/make_host_beam_sample.py records, {(seed, eos): (tape, ids, scores)} over CASES: beam-sample on
    _OracleDecoder, keeping the log-probabilities the search was served step by step (the tape), then beam-sample over that tape"""
    out = {}
    for seed, eos, _ in CASES:
        model, prompt = _model_and_prompt(seed, eos)
        dec, tape = _OracleDecoder(model, prompt.shape[0] * 3 * 2, L), []
        served = dec.beam_logp
        dec.beam_logp = lambda: tape.append(served().clone()) or tape[-1]
        beam_search(dec, prompt, L, eos_token_id=eos, generator=torch.Generator().manual_seed(seed), **BEAM_SAMPLE)
        assert len(tape) == L - TP                                 # every step to max_length was served
        out[seed, eos] = (torch.stack(tape),) + tuple(_beam_sample_from_tape(seed, eos, tape))
    return out


@torch.no_grad()
def test_beam_sample_is_what_it_was():
    """the exact pin of beam-sample: ids and scores recorded before the host loops became one, over the recorded log-probabilities
    of _OracleDecoder for CASES (same torch build on both sides: the draws of `multinomial` from a seeded generator are
    reproducible only there).  What this pin does not see: the tape serves step k whatever beam_reorder was handed, so only the
    ids' own reorder is checked here, not the one the decoder's caches follow (tests/test_group_beam_cpu.py and the device tests
    run real decoders), and the warp runs in float64 where production runs it in float32"""
    import os
    want = torch.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), BEAM_SAMPLE_GOLDEN))
    assert set(want) == {(seed, eos) for seed, eos, _ in CASES}
    for (seed, eos), (tape, w_ids, w_sc) in want.items():
        ids, sc = _beam_sample_from_tape(seed, eos, tape)
        assert torch.equal(ids, w_ids) and torch.equal(sc, w_sc), (seed, eos)
        assert ids.shape[0] == 4 and torch.equal(ids[:, :TP], _model_and_prompt(seed, eos)[1].repeat_interleave(2, 0))
