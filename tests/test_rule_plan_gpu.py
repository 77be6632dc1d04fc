"""Where generate.RulePlan meets the device: a decoder's `generate` against its `run` under the plan that rules_config builds from the
same keywords, and XLDecoderLanes -- the one caller of RulePlan.rows -- lane by lane against a decoder of the lane's size, seed and
rows.  The model and the prompts are those of tests/test_register_rule_gpu.py; the host side is tests/test_rule_plan_cpu.py."""
import pytest
import torch

from symbolic_music_generation_amd.generate import (XLDecoder, XLDecoderLanes, check_bar_lengths, check_grammar, check_in_key,
                                                    check_register, rules_config, sampling_config, stop_config)
from tests.test_register_rule_gpu import EOS, G, KEY, PAD, REG, V, _bar_prompts, _model

pytestmark = pytest.mark.gpu

SAMPLE = dict(do_sample=True, top_k=8, temperature=1.0)
STOP = dict(eos_token_id=EOS, pad_token_id=PAD)
NEW = 38                                                           # prompts of 10 tokens: max_length 48


def test_generate_equals_run_under_the_plan(dev):
    m = _model(dev, 720, closing_bias=4.0)
    ids = _bar_prompts(4, dev)
    Tp = ids.shape[1]
    L = Tp + NEW
    rules = dict(grammar=G, n_bars=[1, 2, 1, -1], in_key=KEY, key=['CMajor', None, 'GMajor', 'AMinor'], register=REG,
                 melody_range=[(60, 72), None, (55, 80), (60, 72)], bass_range=(40, 55), bass_below=1)
    got = XLDecoder(m.engine, 4, L, seed=11).generate(ids, L, **SAMPLE, **STOP, **rules)
    plan = rules_config(batch=4, vocab_size=V, stop=stop_config(EOS, PAD), **rules)
    dec = XLDecoder(m.engine, 4, L, seed=11)
    run = dec.run(ids, L, sampling_config(**SAMPLE), plan)
    assert torch.equal(got, run) and got.shape[1] > Tp and torch.equal(got[:, :Tp], ids)
    # every rule of the plan was in force
    assert dec.rules.grammar is G and dec.rules.bars and dec.rules.in_key is KEY and dec.rules.register is REG and dec.rules.gap == 1
    assert check_grammar(got, G).tolist() == check_bar_lengths(got, G).tolist() == [-1] * 4
    assert check_in_key(got, KEY, prompt_len=Tp, key=rules['key']).tolist() == [-1] * 4
    assert check_register(got, REG, rules['melody_range'], rules['bass_range'], 1, prompt_len=Tp).tolist() == [-1] * 4
    assert not torch.equal(XLDecoder(m.engine, 4, L, seed=11).generate(ids, L, **SAMPLE, **STOP)[:, :got.shape[1]], got)


def test_every_lane_runs_the_rows_of_its_own_plan(dev):
    """five rows over two lanes, 3 + 2: lane i is an XLDecoder of its size with seed + 7919 * i, under the plan of its rows"""
    m = _model(dev, 721, closing_bias=4.0)
    ids = _bar_prompts(5, dev)
    Tp = ids.shape[1]
    L = Tp + NEW
    per_row = dict(n_bars=[1, 2, 1, 2, 1], key=['CMajor', 'GMajor', None, 'AMinor', 'CMajor'],
                   melody_range=[(60, 72), None, (55, 80), (60, 72), (48, 84)], bass_range=[(40, 55), (36, 60), None, (30, 50), (40, 55)])
    shared = dict(grammar=G, in_key=KEY, register=REG, bass_below=1)
    lanes = XLDecoderLanes(m.engine, 5, L, seed=31, lanes=2)
    assert lanes.offs == [0, 3, 5]
    out = lanes.generate(ids, L, **SAMPLE, **STOP, **shared, **per_row)
    whole = rules_config(batch=5, vocab_size=V, stop=stop_config(EOS, PAD), **shared, **per_row)
    outs = []
    for i, (lo, hi) in enumerate(((0, 3), (3, 5))):
        d = lanes.lanes[i]
        # the words that a generation leaves where `start` put them (the model's bias keeps key tokens away): this lane's rows
        assert d.seed == 31 + 7919 * i and d.rules.grange.tolist() == whole.register.bounds[lo:hi].tolist()
        assert d.rules.gkey.tolist() == whole.keys[lo:hi].tolist()
        alone = XLDecoder(m.engine, hi - lo, L, seed=d.seed).generate(ids[lo:hi], L, **SAMPLE, **STOP, **shared,
                                                                       **{k: v[lo:hi] for k, v in per_row.items()})
        w = alone.shape[1]
        assert w <= out.shape[1] and torch.equal(out[lo:hi, :w], alone) and (out[lo:hi, w:] == PAD).all(), i
        outs.append(alone)
    assert out.shape[1] == max(o.shape[1] for o in outs)
