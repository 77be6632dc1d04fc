"""The bar count of `generate(..., n_bars=k)` on the host: the rule of grammar.BarCount (allows / move / walk), its place on the
music grammar and on custom grammars, the dead ends its constructor refuses, and every refusal of the public surface that needs no
device."""
import numpy as np
import pytest
import torch

from symbolic_music_generation_amd.generate import bar_count_config, bars_after_prompt, stop_config
from symbolic_music_generation_amd.grammar import (MUSIC_BAR_COUNT_CLASSES, MUSIC_CLASSES, MUSIC_TRANSITIONS, BarCount, from_transitions,
                                                   music_budget_tables, music_grammar)
from symbolic_music_generation_amd.vocab import MusicVocabulary

VOC = MusicVocabulary()
EOS, PAD, BAR = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<bar>'))


def _ids(text):
    return [VOC.t2i(t) for t in text.split()]


def _first(typ):
    return next(tok for tok in VOC.tok2id if VOC.type(tok) == typ and 'rare' not in tok)


TEMPO, PITCH = _first('tempo'), _first('pitch')
BAR_2_4 = f'<melody> {PITCH} d_2 <bass> {PITCH} d_2'              # both channels of a 2/4 bar, one half note each
HEAD = f'TimeSig_2/4 {TEMPO} <bar>'


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_allows_and_move():
    g = VOC.grammar()
    cnt = g.bar_count
    bar, eos, pitch = (g.class_names.index(c) for c in ('<bar>', '</s>', 'pitch'))
    assert cnt.count == 1 << bar and cnt.end == 1 << eos
    for left in (-5, -1):                                          # no limit: nothing barred, nothing counted
        assert all(cnt.allows(left, c) for c in range(g.n_classes))
        assert all(cnt.move(left, c) == left for c in range(g.n_classes))
    assert not cnt.allows(0, bar) and cnt.allows(0, eos) and cnt.allows(0, pitch)
    assert cnt.allows(1, bar) and not cnt.allows(1, eos) and cnt.allows(1, pitch)
    assert cnt.allows(3, bar) and not cnt.allows(3, eos)
    assert cnt.move(3, bar) == 2 and cnt.move(1, bar) == 0 and cnt.move(0, bar) == 0
    assert cnt.move(2, eos) == 2 and cnt.move(2, pitch) == 2 and cnt.move(0, eos) == 0


def test_walk_on_hand_written_streams():
    g = VOC.grammar(bar_budget=True)
    two_more = _ids(f'{HEAD} {BAR_2_4} <bar> {BAR_2_4} <bar> {BAR_2_4} </s> [PAD] [PAD]')
    Tp = 3
    assert g.walk(two_more)[1] == -1 and g.walk_budget(two_more)[2] == -1
    gen = two_more[Tp:]
    assert g.walk_bars(gen, 2) == (0, -1)                          # exactly two more bars, then the end
    assert g.walk_bars(gen, -1) == (-1, -1)
    assert g.walk_bars(gen, 3) == (1, gen.index(EOS))              # a bar is still owed at </s>
    second = [i for i, t in enumerate(gen) if t == BAR][1]
    assert g.walk_bars(gen, 1) == (0, second)                      # a second <bar> after the only one allowed
    assert g.walk_bars(gen, 0) == (0, gen.index(BAR))
    assert g.walk_bars([-1, -1] + gen, 2) == (0, -1)               # left pads are skipped
    assert g.walk_bars(gen + [len(VOC) + 5], 2) == (0, -1)         # beyond the vocabulary: the grammar's to report
    finish_only = _ids(f'{BAR_2_4} </s> [PAD]')
    assert g.walk_bars(finish_only, 0) == (0, -1) and g.walk_bars(finish_only, 1) == (1, finish_only.index(EOS))
    assert g.bar_count.walk(torch.tensor(gen), 2) == (0, -1)       # tensors as well
    assert bars_after_prompt(torch.tensor([two_more, two_more]), g, prompt_len=Tp).tolist() == [2, 2]
    assert bars_after_prompt(torch.tensor(two_more), g).tolist() == [3]
    mask = torch.ones(1, Tp, dtype=torch.int64)
    assert bars_after_prompt(torch.tensor([two_more]), g, attention_mask=mask).tolist() == [2]


@pytest.mark.parametrize('pitch_kind', ['midi', 'step', 'degree'])
@pytest.mark.parametrize('budget', [False, True])
def test_music_grammar_carries_the_rule(pitch_kind, budget):
    v = MusicVocabulary(pitch_kind=pitch_kind)
    g = v.grammar(bar_budget=budget)
    assert (g.budget is not None) == budget
    cnt = g.bar_count
    assert isinstance(cnt, BarCount) and cnt.grammar is g
    assert cnt.count == 1 << int(g.cls[v.t2i('<bar>')]) and cnt.end == 1 << int(g.cls[v.t2i('</s>')])
    # before the first bar only a bar leads on: those are the states a row with n_bars = 0 may not start from
    assert {g.state_names[s] for s in cnt.needs_bar} == {'S0', 'S1', 'S2', 'S3'}
    assert 'BarCount' in repr(cnt) and '<bar>' in repr(cnt)


def test_from_transitions_round_trip():
    cls = music_grammar(VOC).cls
    no_tup = [t for t in MUSIC_TRANSITIONS if 'tup>' not in t[1] and '_T' not in t[0]]
    for budget in (None, music_budget_tables(VOC)):
        g = from_transitions(cls, MUSIC_CLASSES, no_tup, 'S0', accepting=['END'], budget=budget,
                             bar_count=dict(count=('<bar>',), end=('</s>',)))
        ref = music_grammar(VOC, bar_budget=budget is not None)
        assert (g.bar_count.count, g.bar_count.end) == (ref.bar_count.count, ref.bar_count.end)
        assert MUSIC_BAR_COUNT_CLASSES == dict(count=('<bar>',), end=('</s>',))
        stream = _ids(f'{HEAD} {BAR_2_4} <bar> {BAR_2_4} </s>')
        assert g.walk_bars(stream[3:], 1) == ref.walk_bars(stream[3:], 1) == (0, -1)
    assert from_transitions(cls, MUSIC_CLASSES, no_tup, 'S0').bar_count is None
    masks = from_transitions(cls, MUSIC_CLASSES, no_tup, 'S0', bar_count=dict(count=ref.bar_count.count, end=ref.bar_count.end))
    assert (masks.bar_count.count, masks.bar_count.end) == (ref.bar_count.count, ref.bar_count.end)
    with pytest.raises(ValueError, match='carries no bar count'):
        from_transitions(cls, MUSIC_CLASSES, no_tup, 'S0').walk_bars([1, 2], 1)


def test_constructor_refuses_dead_ends():
    g = VOC.grammar()
    with pytest.raises(ValueError, match='unknown token class'):
        BarCount(g, count=('<measure>',), end=('</s>',))
    with pytest.raises(ValueError, match='both'):
        BarCount(g, count=('<bar>',), end=('<bar>', '</s>'))
    with pytest.raises(ValueError, match='at least one class'):
        BarCount(g, count=(), end=('</s>',))
    with pytest.raises(ValueError, match='beyond class'):
        BarCount(g, count=1 << 20, end=('</s>',))
    # END allows only [PAD]: as `end` class it would be all a row with bars left may emit there
    with pytest.raises(ValueError, match='allows only `end` classes'):
        BarCount(g, count=('<bar>',), end=('[PAD]',))
    # a count token whose successor can only count again: after its last bar the row would be stuck there
    cls = np.array([0, 1, 2], dtype=np.uint8)
    with pytest.raises(ValueError, match='leads to state'):
        from_transitions(cls, ('a', 'b', 'c'), [('X', 'a', 'Y'), ('Y', 'a', 'X'), ('X', 'b', 'X'), ('X', 'c', 'Z'), ('Z', 'b', 'Z')], 'X',
                         bar_count=dict(count=('a',), end=('c',)))
    assert g.bar_count.count == 1 << g.class_names.index('<bar>')  # (the failed attempts above did not attach themselves)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_bar_count_config():
    g = VOC.grammar(bar_budget=True)
    stop = stop_config(EOS, PAD)
    assert bar_count_config(None, 4, None, None) is None
    k = bar_count_config(2, 3, g, stop)
    assert k.dtype == torch.int32 and k.tolist() == [2, 2, 2] and not k.is_cuda
    assert bar_count_config([0, -1, 3], 3, g, stop, repeat=2).tolist() == [0, 0, -1, -1, 3, 3]
    assert bar_count_config(torch.tensor([1, -7]), 2, g, stop).tolist() == [1, -1]
    assert bar_count_config(np.array([4]), 1, g, stop).tolist() == [4]
    with pytest.raises(ValueError, match='n_bars needs grammar='):
        bar_count_config(2, 3, None, stop)
    bare = from_transitions(g.cls, MUSIC_CLASSES, MUSIC_TRANSITIONS, 'S0')
    with pytest.raises(ValueError, match='grammar with a bar count'):
        bar_count_config(2, 3, bare, stop)
    with pytest.raises(ValueError, match='explicit eos_token_id'):
        bar_count_config(2, 3, g, None)
    with pytest.raises(ValueError, match='no `end` token'):
        bar_count_config(2, 3, g, stop_config(BAR, PAD))
    with pytest.raises(ValueError, match='no `end` token'):
        bar_count_config(2, 3, g, stop_config(len(VOC) + 1, PAD))
    with pytest.raises(ValueError, match='min_length'):
        bar_count_config(2, 3, g, stop_config(EOS, PAD, 10))
    with pytest.raises(ValueError, match='4 entries for 3 prompts'):
        bar_count_config([1, 2, 3, 4], 3, g, stop)
    with pytest.raises(ValueError, match='must be an int'):
        bar_count_config(2.5, 3, g, stop)
    with pytest.raises(ValueError, match='must be an int'):
        bar_count_config(torch.tensor([1.0, 2.0, 3.0]), 3, g, stop)


def test_bars_after_prompt_needs_the_rule():
    bare = from_transitions(VOC.grammar().cls, MUSIC_CLASSES, MUSIC_TRANSITIONS, 'S0')
    with pytest.raises(ValueError, match='bar count'):
        bars_after_prompt(torch.zeros(1, 4, dtype=torch.int64), bare)
