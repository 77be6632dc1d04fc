"""Diverse (group) beam search with the scorer on the device, end to end on TransfoXL: generate.group_beam_search_device against the
host scorer generate.group_beam_search on a second decoder, the public `generate(num_beams=, num_beam_groups=)` on either path, and
the grammar and the key rule under group beam search against the host scorer with a mask built from grammar.py's host walkers."""
import pytest
import torch

from symbolic_music_generation_amd import generate as G
from symbolic_music_generation_amd.generate import (XLDecoder, check_bar_lengths, check_grammar, check_in_key, group_beam_search,
                                                    group_beam_search_device)

from tests.rules_ref import host_allowed

pytestmark = pytest.mark.gpu

# the fixtures of tests/test_beam_device_gpu.py, with a model seed and eos ids chosen on the CPU with generate.group_beam_search over
# the oracle model (tests/test_beam_cpu.py's decoder), prompts of generator seed 21: the model of seed 14 repeats 845 after prompt
# 0, and 122 and 1049 are among the tokens it gives prompt 1.  With the eos below for the shape (num_beams, num_beam_groups), under
# either early_stopping arm, either penalty and num_return_sequences 1 and 2, hypotheses end and one item fills its store and is
# done before max_length while the other stays open, and diversity_penalty = 1.5 changes the returned rows against 0.  eos = -1 is
# never emitted.
SEED, PROMPT_SEED, TP, L = 14, 21, 12, 40
EOS_EMITTED, EOS_NEVER = {(4, 2): 845, (4, 4): 122, (6, 2): 1049}, -1
PENS = (0.0, 1.5)


@pytest.fixture(scope='module')
def plain(dev):
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=64, max_length=64, seed=SEED)
    prompt = torch.randint(4, 1190, (2, TP), generator=torch.Generator().manual_seed(PROMPT_SEED)).to(dev)
    return m.eval(), prompt


def _host(monkeypatch, *args, **kw):
    """generate.group_beam_search and the hypothesis heaps it made, one per prompt"""
    made = []

    class Spy(G._BeamHyps):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)
    with monkeypatch.context() as mp:
        mp.setattr(G, '_BeamHyps', Spy)
        out = group_beam_search(*args, **kw)
    return out, made


@pytest.mark.parametrize('early', [True, False])
@pytest.mark.parametrize('nb,ng', [(4, 2), (4, 4), (6, 2)])
def test_device_scorer_equals_host_scorer(plain, monkeypatch, nb, ng, early):
    m, prompt = plain
    finished, done_early, by_pen = 0, 0, {}
    for pen in PENS:
        for eos in (EOS_EMITTED[nb, ng], EOS_NEVER):
            for keep in (1, 2):
                kw = dict(num_beams=nb, num_beam_groups=ng, diversity_penalty=pen, early_stopping=early, num_return_sequences=keep,
                          eos_token_id=eos, pad_token_id=0, return_scores=True)
                (want, w_sc), heaps = _host(monkeypatch, XLDecoder(m.engine, 2 * nb, L), prompt, L, **kw)
                dec = XLDecoder(m.engine, 2 * nb, L)
                got, g_sc = group_beam_search_device(dec, prompt, L, use_graph=True, stop_chunk=5, **kw)
                what = (pen, eos, keep)
                assert got.shape == want.shape and torch.equal(got, want), what
                assert (g_sc - w_sc).abs().max().item() < 1e-4, (what, g_sc.tolist(), w_sc.tolist())
                assert dec.beam.done.tolist() == [int(h.done) for h in heaps], what
                eager, e_sc = group_beam_search_device(XLDecoder(m.engine, 2 * nb, L), prompt, L, use_graph=False, **kw)
                assert torch.equal(eager, got) and torch.equal(e_sc, g_sc), what
                again, _ = group_beam_search_device(dec, prompt, L, use_graph=True, **kw)  # the captured step, from a new start
                assert torch.equal(again, got), what
                if eos == EOS_NEVER:
                    assert dec.steps_run == L - TP - 1 and int(dec.beam.n_done) == 0 and not (want[:, TP:] == eos).any()
                else:
                    finished += int((want[:, TP:] == eos).any())
                    done_early += int(any(h.done for h in heaps))
                by_pen[(pen, eos, keep)] = want
    # on the host result alone: the emitted eos ended hypotheses, an item was done before max_length, and the penalty changed what
    # is returned
    assert finished >= 2 and done_early >= 1, (finished, done_early)
    assert any(not torch.equal(by_pen[(PENS[0], eos, keep)], by_pen[(PENS[1], eos, keep)])
               for eos in (EOS_EMITTED[nb, ng], EOS_NEVER) for keep in (1, 2))


def test_generate_takes_either_path(plain, monkeypatch):
    m, prompt = plain
    kw = dict(input_ids=prompt, max_length=L, num_beams=4, num_beam_groups=2, diversity_penalty=1.5, num_return_sequences=2,
              early_stopping=True, eos_token_id=EOS_EMITTED[4, 2], pad_token_id=0)
    calls = []
    real = G.group_beam_search_device
    monkeypatch.setattr(G, 'group_beam_search_device', lambda *a, **k: calls.append(1) or real(*a, **k))
    plain_ids = m.generate(**kw)
    assert calls == []                                                     # without a rule the host scorer stays the default
    monkeypatch.setenv('MXL_GROUP_BEAM_DEVICE', '1')
    dev_ids = m.generate(**kw)
    assert calls == [1] and torch.equal(dev_ids, plain_ids)
    monkeypatch.setenv('MXL_BEAM_HOST', '1')
    host_ids = m.generate(**kw)
    assert calls == [1]                                                    # the knob keeps the host scorer
    assert dev_ids.shape == (4, host_ids.shape[1]) and torch.equal(dev_ids, host_ids)
    assert (host_ids[:, TP:] == EOS_EMITTED[4, 2]).any()
    monkeypatch.delenv('MXL_BEAM_HOST')
    assert torch.equal(m.generate(**kw, use_graph=False), dev_ids) and len(calls) == 2
    # a negative penalty, which the kernel refuses, keeps the host path, where it counts as none
    neg = m.generate(**{**kw, 'diversity_penalty': -1.0})
    assert len(calls) == 2 and torch.equal(neg, m.generate(**{**kw, 'diversity_penalty': 0.0})) and len(calls) == 3
    # what the host path refuses with HF's messages is still refused with them
    with pytest.raises(ValueError, match='divisible'):
        m.generate(input_ids=prompt, max_length=L, num_beams=3, num_beam_groups=2)
    with pytest.raises(ValueError, match='smaller or equal to `num_beams`'):
        m.generate(input_ids=prompt, max_length=L, num_beams=2, num_beam_groups=4)
    with pytest.raises(ValueError, match='sampling mode'):
        m.generate(input_ids=prompt, max_length=L, num_beams=4, num_beam_groups=2, do_sample=True)


# ---------------------------------------------------------------------------------------------------------------- rules
GROUPS = dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.5, num_return_sequences=2, early_stopping=True)


def _rules_case(dev, seed, budget, in_key):
    from tests.test_key_rule_gpu import EOS, FULL_BAR, PAD, RULE, TOK, _model, _prompts
    m = _model(dev, seed, closing_bias=4.0)
    ids, _ = _prompts(3, dev, FULL_BAR, keyless=False)
    Tp = ids.shape[1]
    W = Tp + 40
    g = TOK.grammar(bar_budget=budget)
    rule = RULE if in_key else None
    kw = dict(GROUPS, eos_token_id=EOS, pad_token_id=PAD)
    got = m.generate(input_ids=ids, max_length=W, grammar=g, in_key=rule, **kw)
    want = group_beam_search(XLDecoder(m.engine, ids.shape[0] * 4, W), ids, W, allowed=host_allowed(g, rule=rule), **kw)
    free = group_beam_search(XLDecoder(m.engine, ids.shape[0] * 4, W), ids, W, **kw)
    return got, want, free, g, rule, ids, EOS


def _clean(out, ids, keep, g, rule, EOS):
    """per returned row: does it keep its prompt and does every rule accept it up to and including the eos finalize writes"""
    Tp = ids.shape[1]
    assert torch.equal(out[:, :Tp], ids.repeat_interleave(keep, 0))
    ok = []
    for row in out.tolist():
        t = torch.tensor(row[:(row.index(EOS) + 1) if EOS in row else len(row)])
        good = check_grammar(t, g).tolist() == [-1]
        if g.budget is not None:
            good = good and check_bar_lengths(t, g).tolist() == [-1]
        if rule is not None:
            good = good and check_in_key(t, rule, prompt_len=Tp).tolist() == [-1]
        ok.append(good)
    return ok


@pytest.mark.parametrize('budget', [False, True])
def test_grammar_under_group_beam_search_equals_the_masked_host_scorer(dev, budget):
    """fails without the feature: generate(num_beams=4, num_beam_groups=2, grammar=) raises MusicXLError there"""
    got, want, free, g, rule, ids, EOS = _rules_case(dev, 601, budget, False)
    assert got.shape == want.shape and torch.equal(got, want)
    assert all(_clean(got, ids, 2, g, rule, EOS))
    assert not all(_clean(free, ids, 2, g, rule, EOS))                     # the free search breaks the rule: the mask is at work


def test_grammar_and_in_key_under_group_beam_search(dev):
    got, want, free, g, rule, ids, EOS = _rules_case(dev, 602, True, True)
    assert got.shape == want.shape and torch.equal(got, want)
    assert all(_clean(got, ids, 2, g, rule, EOS))
    assert not all(_clean(free, ids, 2, g, rule, EOS))


def test_in_key_alone_under_group_beam_search(dev):
    from tests.test_key_rule_gpu import EOS, PAD, RULE, _model, _prompts
    m = _model(dev, 603)
    ids, _ = _prompts(3, dev, keyless=False)
    Tp, W = ids.shape[1], ids.shape[1] + 30
    kw = dict(GROUPS, num_return_sequences=1, eos_token_id=EOS, pad_token_id=PAD)
    free = m.generate(input_ids=ids, max_length=W, **kw)
    assert (check_in_key(free, RULE, prompt_len=Tp) >= Tp).all()           # the model leaves the key without the rule
    got = m.generate(input_ids=ids, max_length=W, in_key=RULE, **kw)
    want = group_beam_search(XLDecoder(m.engine, 12, W), ids, W, allowed=host_allowed(None, rule=RULE), **kw)
    assert torch.equal(got, want) and check_in_key(got, RULE, prompt_len=Tp).tolist() == [-1] * 3
    keyed = m.generate(input_ids=ids, max_length=W, in_key=RULE, key=['GMajor', None, 'CMajor'], **kw)
    assert check_in_key(keyed, RULE, prompt_len=Tp, key=['GMajor', None, 'CMajor']).tolist() == [-1] * 3


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_keep_their_messages(dev, monkeypatch):
    from symbolic_music_generation_amd._lib import MusicXLError
    from tests.test_key_rule_gpu import EOS, PAD, RULE, TOK, _model, _prompts
    m = _model(dev, 604)
    ids, _ = _prompts(2, dev, keyless=False)
    g = TOK.grammar(bar_budget=True)
    stop = dict(eos_token_id=EOS, pad_token_id=PAD)
    arm = dict(num_beams=4, num_beam_groups=2)
    only = 'is supported for greedy decoding and sampling only'
    # any rule without an explicit eos
    for name, rk in (('grammar', dict(grammar=g)), ('in_key', dict(in_key=RULE)), ('in_key', dict(key='CMajor'))):
        with pytest.raises(MusicXLError, match=f'{name}= {only}'):
            m.generate(input_ids=ids, max_length=20, **rk, **arm)
    # n_bars, with or without the grammar that counts the bars
    for rk in (dict(grammar=g, n_bars=1), dict(n_bars=1)):
        with pytest.raises(MusicXLError, match=f'n_bars= {only}'):
            m.generate(input_ids=ids, max_length=20, **rk, **stop, **arm)
    with pytest.raises(MusicXLError, match=f'melody= {only}'):
        m.generate(input_ids=ids, max_length=40, grammar=g, melody=[1, 2, 3], **stop, **arm)
    mask = torch.ones_like(ids)
    mask[0, 0] = 0
    with pytest.raises(MusicXLError, match='padded prompts'):
        m.generate(input_ids=ids, attention_mask=mask, max_length=20, **arm)
    # every rule on the host path, and beyond 16 beams
    monkeypatch.setenv('MXL_BEAM_HOST', '1')
    for name, rk in (('grammar', dict(grammar=g)), ('in_key', dict(in_key=RULE))):
        with pytest.raises(MusicXLError, match=f'{name}= {only}'):
            m.generate(input_ids=ids, max_length=20, **rk, **stop, **arm)
    monkeypatch.delenv('MXL_BEAM_HOST')
    with pytest.raises(MusicXLError, match=f'grammar= {only}'):
        m.generate(input_ids=ids, max_length=20, grammar=g, num_beams=18, num_beam_groups=2, **stop)
    # below generate: the loop that both device searches share takes no bar count with groups, and the kernel's limits hold
    with pytest.raises(MusicXLError, match='n_bars= is not supported under group beam search'):
        G.beam_search_device(XLDecoder(m.engine, 8, 20), ids, 20, 4, eos_token_id=EOS, pad_token_id=PAD, grammar=g, n_bars=1,
                             num_beam_groups=2)
    with pytest.raises(MusicXLError, match='finite diversity_penalty'):
        group_beam_search_device(XLDecoder(m.engine, 8, 20), ids, 20, 4, 2, float('inf'), eos_token_id=EOS, pad_token_id=PAD)
    # with an eos, the argument checks of the sampling path hold
    with pytest.raises(ValueError, match='needs in_key='):
        m.generate(input_ids=ids, max_length=20, key='CMajor', **stop, **arm)
