"""Stopping at eos (`generate(eos_token_id=...)`): the host reference of the rule and the argument handling, no GPU needed."""
import pytest
import torch

from symbolic_music_generation_amd.generate import finish_at_eos, resolve_max_length, stop_config


def test_finish_at_eos_first_generated_eos_and_pad_after():
    ids = torch.tensor([[7, 3, 5, 3, 6, 3, 8],
                        [3, 9, 3, 2, 2, 2, 2]])
    out = finish_at_eos(ids, 2, eos=3, pad=0)
    # row 0: the prompt's 3 (column 1) does not count, the first generated 3 is at column 3 and stays, later columns are pad;
    # row 1: first generated 3 at column 2.  Every row finished: cut to the later one, W = 3 + 1
    assert torch.equal(out, torch.tensor([[7, 3, 5, 3], [3, 9, 3, 0]]))
    assert torch.equal(ids[0], torch.tensor([7, 3, 5, 3, 6, 3, 8]))          # the input is not modified


def test_finish_at_eos_some_rows_never_finish():
    ids = torch.tensor([[1, 2, 4, 5, 6, 7],
                        [1, 2, 9, 9, 9, 9]])
    out = finish_at_eos(ids, 2, eos=5, pad=11)
    assert out.shape == ids.shape                                             # a live row keeps the whole width
    assert torch.equal(out[0], torch.tensor([1, 2, 4, 5, 11, 11]))
    assert torch.equal(out[1], ids[1])


def test_finish_at_eos_pad_equal_to_eos_and_first_token():
    ids = torch.tensor([[4, 4, 2, 8, 2], [4, 4, 2, 2, 9]])
    out = finish_at_eos(ids, 2, eos=2, pad=2)
    assert torch.equal(out, torch.tensor([[4, 4, 2], [4, 4, 2]]))             # every row's first token is eos: W = Tp + 1
    assert torch.equal(finish_at_eos(ids[:, :2], 2, 2, 2), ids[:, :2])       # nothing generated


def test_stop_config_is_opt_in_and_pad_fallback():
    assert stop_config(None) is None
    assert stop_config(None, pad_token_id=5, min_length=30) is None           # min_length without eos: no-op
    assert stop_config(3) == (3, 3, 0)                                        # pad: eos when neither argument nor config has one
    assert stop_config(3, config_pad_token_id=1) == (3, 1, 0)                 # then the config's
    assert stop_config(3, pad_token_id=7, config_pad_token_id=1) == (3, 7, 0)  # the argument first
    assert stop_config(3, min_length=20) == (3, 3, 20)


def test_max_new_tokens():
    assert resolve_max_length(None, 16, 40, 2048) == 56
    assert resolve_max_length(None, None, 40, 2048) == 2048
    assert resolve_max_length(100, None, 40, 2048) == 100
    with pytest.raises(ValueError):
        resolve_max_length(100, 16, 40, 2048)


def test_sampling_config_fills_the_off_values():
    import ast
    import os
    from symbolic_music_generation_amd.generate import sampling_config
    cfg = sampling_config(False, None, None, 1.0, None, None)
    assert cfg == dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0)
    assert sampling_config(True, 8, 0.9, 1.5, 1.2, 0.8) == dict(do_sample=True, top_k=8, top_p=0.9, temperature=1.5,
                                                                repetition_penalty=1.2, typical_p=0.8)
    # the same six keys as the literal dict bench.py hands to `begin` (they make up the graph key)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bench.py')).read()
    calls = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', None) == 'samp']
    assert len(calls) == 1 and set(cfg) == {k.arg for k in calls[0].value.keywords} and len(cfg) == 6
