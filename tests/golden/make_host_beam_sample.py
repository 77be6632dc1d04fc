"""Beam-sample (`generate.beam_search(do_sample=True)`) over tests/test_beam_cpu.py's stand-in decoder and CASES, with num_beams=3,
num_return_sequences=2, top_k=16, temperature=0.9, renormalize_logits=True and a generator seeded with the case's seed: the
log-probabilities the search was served step by step, and the ids and scores of the same search over those served values in
float64, which tests/test_beam_cpu.py::test_beam_sample_is_what_it_was asserts with torch.equal.  (Served in float64, the search
returns the same on every CPU: the last-place differences between their kernels stay below the float32 of the scores.)

A record of behaviour: regenerate it only at the commit BEFORE a change to the host beam loop.  The same torch build must run the
generator and the test: the draws of `multinomial` are reproducible only within one build.

    python tests/golden/make_host_beam_sample.py         # writes tests/golden/host_beam_sample.pt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

if __name__ == '__main__':
    from tests.test_beam_cpu import BEAM_SAMPLE_GOLDEN, beam_sample_record
    runs = beam_sample_record()
    torch.save(runs, os.path.join(ROOT, BEAM_SAMPLE_GOLDEN))
    for k, (tape, ids, sc) in runs.items():
        print(k, tuple(tape.shape), tuple(ids.shape), sc.tolist(), f'torch {torch.__version__}')
