"""The bar budget on the music grammar (`tokenizer.grammar(bar_budget=True)`): its host side against a test-local loop that sums the
durations of every channel with fractions.Fraction, on the real streams of tests/golden/sample_score_ids.npz, on the reference's
broken generation and on hand-built prompts; constructor refusals; what stays as it was without the argument."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from symbolic_music_generation_amd.generate import check_bar_lengths, check_grammar_args
from symbolic_music_generation_amd.grammar import (NO_SIG, RARE_SLOTS, BarBudget, from_transitions, music_budget_tables,
                                                   music_grammar)
from symbolic_music_generation_amd.vocab import MusicTokenizer, MusicVocabulary

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sample_score_ids.npz')
MIDI = MusicVocabulary(pitch_kind='midi')


def channels(vocab, ids):
    """the test's own reading of a stream: [(column of the channel's opening token, sum of its durations in quarters or None when it
    holds a d_rare, closed?)] and the bar length in quarters (None = TimeSig_rare)"""
    out, bar, cur = [], None, None
    for col, t in enumerate(ids):
        tok = vocab.i2t(int(t))
        if tok.startswith('TimeSig_') and tok != vocab.rare_time_sig:
            bar = Fraction(tok[len('TimeSig_'):]) * 4
        if tok in ('<melody>', '<bass>', '<bar>', '</s>') and cur is not None:
            out.append((cur[0], cur[1], True))
            cur = None
        if tok in ('<melody>', '<bass>'):
            cur = [col, Fraction(0)]
        elif tok.startswith('d_') and cur is not None:
            cur[1] = None if tok == vocab.rare_duration or cur[1] is None else cur[1] + Fraction(tok[2:])
    if cur is not None:
        out.append((cur[0], cur[1], False))
    return out, bar


def first_broken_channel(vocab, ids):
    """index of the first channel that is not exactly one bar long (an open last channel only counts when it is already too long)"""
    chans, bar = channels(vocab, ids)
    for i, (_, total, closed) in enumerate(chans):
        if total is None or total > bar or (closed and total != bar):
            return i
    return -1


def channel_of(vocab, ids, col):
    """index of the channel that is open when the token at `col` arrives"""
    return sum(1 for t in ids[:col] if vocab.i2t(int(t)) in ('<melody>', '<bass>')) - 1


def test_the_real_stream_is_exact_and_reported_clean():
    ids = np.load(GOLD)['sample_full_midi'].astype(np.int64)
    chans, bar = channels(MIDI, ids)
    assert bar == 4 and len(chans) == 210 and all(total == 4 and closed for _, total, closed in chans)
    g = MIDI.grammar(bar_budget=True)
    assert check_bar_lengths(torch.from_numpy(ids), g).tolist() == [-1]
    assert g.walk_budget(ids) == (32, 0, -1)


def test_gen_broken_breaks_the_budget_where_the_fraction_loop_says():
    vocab = MusicVocabulary(pitch_kind='degree')
    ids = np.load(GOLD)['gen_broken'].astype(np.int64)
    chans, bar = channels(vocab, ids)
    closed = [total for _, total, done in chans if done]           # (the stream ends inside a 32nd channel)
    assert bar == 4 and len(closed) == 31 and len(chans) == 32
    assert sum(1 for total in closed if total != 4) == 17
    assert sum(1 for t in ids if vocab.i2t(int(t)) == 'd_rare') == 6
    g = vocab.grammar(bar_budget=True)
    assert g.walk(ids)[1] == -1                                   # the grammar alone passes it
    col = int(check_bar_lengths(torch.from_numpy(ids), g)[0])
    assert col >= 0
    want = first_broken_channel(vocab, ids)
    assert want >= 0 and channel_of(vocab, ids, col) == want
    # everything before that channel is clean, and the walk stopped inside it or on the token that closes it
    assert check_bar_lengths(torch.from_numpy(ids[:chans[want][0] + 1]), g).tolist() == [-1]
    assert col > chans[want][0] and (want + 1 == len(chans) or col <= chans[want + 1][0])


@pytest.mark.parametrize('kind,name', [('step', 'sample_full_step'), ('degree', 'sample_full_degree')])
def test_rare_time_signature_rows_are_unconstrained(kind, name):
    vocab = MusicVocabulary(pitch_kind=kind)
    ids = np.load(GOLD)[name].astype(np.int64)
    assert vocab.i2t(int(ids[0])) == 'TimeSig_rare'
    g = vocab.grammar(bar_budget=True)
    assert check_bar_lengths(ids, g).tolist() == [-1]
    assert g.walk_budget(ids) == (0, 0, -1)
    assert channels(vocab, ids)[1] is None                          # the test's own reading finds no bar length either


def _ids(text):
    return [MIDI.t2i(t) for t in text.split()]


@pytest.mark.parametrize('sig,bar', [('3/4', 24), ('6/8', 24)])
def test_hand_built_prompts(sig, bar):
    g = MIDI.grammar(bar_budget=True)
    head = f'TimeSig_{sig} Tempo_120 <bar> <melody>'
    n = len(head.split())
    full = 'p_1/4 d_2 p_3/4 d_1'                                   # 16 + 8 slots = 3 quarters
    ok = _ids(f'{head} {full} <bass> p_r d_3 <bar> <melody> {full} <bass> {full} </s>')
    assert g.walk(ok)[1] == -1 and g.walk_budget(ok) == (bar, 0, -1)
    # overfull by one slot: the duration that does not fit
    over = _ids(f'{head} p_1/4 d_2 p_3/4 d_9/8 <bass>')
    assert g.walk(over)[1] == -1 and g.walk_budget(over) == (bar, 8, n + 3)
    # ... and a note begun in a full channel
    assert g.walk_budget(_ids(f'{head} {full} p_1/4 d_1/8'))[2] == n + 4
    # closing with slots left: <bass>, <bar> and </s> each
    assert g.walk_budget(_ids(f'{head} p_1/4 d_2 <bass>')) == (bar, 8, n + 2)
    assert g.walk_budget(_ids(f'{head} {full} <bass> p_r d_23/8 <bar>')) == (bar, 1, n + 7)
    assert g.walk_budget(_ids(f'{head} {full} <bass> p_r d_23/8 </s>')) == (bar, 1, n + 7)
    assert g.walk_budget(_ids(f'{head} <bass>'))[2] == n            # an empty channel is an underfull one
    # a tuplet has one duration for the whole group: it fills the bar exactly, and one slot more does not fit
    tup = _ids(f'{head} <tup> p_1/4 p_3/4 p_5/4 d_3 </tup> <bass> <tup> p_1/3 p_1/3 d_3/2 </tup> p_r d_3/2 <bar>')
    assert g.walk(tup)[1] == -1 and g.walk_budget(tup) == (bar, 0, -1)
    assert g.walk_budget(_ids(f'{head} <tup> p_1/4 p_3/4 p_5/4 d_25/8 </tup>')) == (bar, bar, n + 4)
    assert g.walk_budget(_ids(f'{head} p_r d_3 <tup> p_1/4'))[2] == n + 2   # no tuplet begins in a full channel
    # d_rare inside a constrained bar
    assert g.walk_budget(_ids(f'{head} p_1/4 d_rare'))[2] == n + 1
    # pads are skipped, the walk continues from a given (bar, rem), rows of a batch are independent
    assert g.walk_budget([-1, -1] + over)[2] == n + 5
    b, r, _ = g.walk_budget(ok[:n + 2])
    assert (b, r) == (bar, 8) and g.walk_budget(ok[n + 2:], b, r) == (bar, 0, -1)
    L = max(len(ok), len(over))
    batch = torch.tensor([[-1] * (L - len(x)) + x for x in (ok, over)])
    assert check_bar_lengths(batch, g).tolist() == [-1, L - len(over) + n + 3]
    mask = torch.tensor([[0] * (L - len(x)) + [1] * len(x) for x in (ok, over)])
    pads = torch.tensor([[MIDI.t2i('[PAD]')] * (L - len(x)) + x for x in (ok, over)])
    assert check_bar_lengths(pads, g, attention_mask=mask).tolist() == [-1, L - len(over) + n + 3]


def test_tables_of_the_music_budget():
    t = music_budget_tables(MIDI)
    slots, bars = t['slots'], t['bars']
    assert slots.dtype == np.uint16 and bars.dtype == np.uint16 and slots.shape == bars.shape == (len(MIDI),)
    for tok, i in MIDI.tok2id.items():
        if tok == 'd_rare':
            assert slots[i] == RARE_SLOTS
        elif tok.startswith('d_'):
            assert Fraction(int(slots[i]), 8) == Fraction(tok[2:])   # precision 5: a slot is 1/8 quarter
        else:
            assert slots[i] == 0
        if tok == 'TimeSig_rare':
            assert bars[i] == 0
        elif tok.startswith('TimeSig_'):
            assert Fraction(int(bars[i]), 8) == Fraction(tok[8:]) * 4
        else:
            assert bars[i] == NO_SIG
    assert int(slots[MIDI.t2i('d_1/8')]) == 1 and int(bars[MIDI.t2i('TimeSig_4/4')]) == 32
    # a signature whose bar is no whole number of slots is unconstrained: 6/8 at precision 2 (slots of one quarter) is 3, 3/8 would not be
    coarse = MusicVocabulary(precision=2, pitch_kind='midi')
    tc = music_budget_tables(coarse)
    assert int(tc['bars'][coarse.t2i('TimeSig_6/8')]) == 3 and int(tc['bars'][coarse.t2i('TimeSig_12/8')]) == 6
    assert int(music_budget_tables(MusicVocabulary(precision=1))['bars'][MIDI.t2i('TimeSig_6/8')]) == 0   # 1.5 slots of 2 quarters


def test_without_the_argument_nothing_changes():
    plain, budget = MIDI.grammar(), MIDI.grammar(bar_budget=True)
    assert plain.budget is None and isinstance(budget.budget, BarBudget)
    for a in ('cls', 'allow', 'next'):
        assert np.array_equal(getattr(plain, a), getattr(budget, a))
    assert plain.state_names == budget.state_names and plain.n_states == 18    # no new automaton states
    assert MusicTokenizer(pitch_kind='midi').grammar().budget is None
    assert MusicTokenizer(pitch_kind='midi').grammar(bar_budget=True).budget is not None
    with pytest.raises(ValueError, match='bar_budget'):
        check_bar_lengths(torch.zeros(1, 4, dtype=torch.int64), plain)
    with pytest.raises(ValueError):
        plain.walk_budget([0])
    from symbolic_music_generation_amd.subword import PairMergeTokenizer
    with pytest.raises(NotImplementedError, match='class borders'):
        PairMergeTokenizer({}, pitch_kind='step').grammar(bar_budget=True)


def test_no_reachable_row_is_all_masked():
    g = MIDI.grammar(bar_budget=True)
    bud = g.budget
    assert min(bud._reach.values()) >= 1
    names = g.state_names
    reach = {(names[s], bar, rem) for s, bar, rem in bud._reach}
    assert ('M_P', 32, 1) in reach and ('B_D', 24, 0) in reach and ('M_D', 48, 48) not in reach
    # with min_length the closing <bar> stays where </s> is barred
    eos = MIDI.t2i('</s>')
    assert bud.only_token_states(eos) == []
    check_grammar_args(g, len(MIDI), (eos, MIDI.t2i('[PAD]'), 50))
    # doctored tables: no one-slot duration -> a pitch at rem == 1 has no duration to follow
    t = music_budget_tables(MIDI)
    t['slots'][MIDI.t2i('d_1/8')] = 2
    with pytest.raises(ValueError, match='every token barred'):
        BarBudget(MIDI.grammar(), **t)
    # a closer that is also a note starter can never be emitted: the melody cannot be left
    t = music_budget_tables(MIDI)
    t['need_free'] = ('pitch', '<tup>', '<bass>')
    with pytest.raises(ValueError, match='every token barred'):
        BarBudget(MIDI.grammar(), **t)
    for bad in (dict(slots=np.zeros(3)), dict(need_full=('nope',)), dict(opens=1 << 20)):
        with pytest.raises(ValueError):
            BarBudget(MIDI.grammar(), **{**music_budget_tables(MIDI), **bad})


def test_from_transitions_takes_explicit_tables():
    """a toy: tokens 0 = sig (bar 3), 1 = open, 2 = note of one slot, 3 = note of two, 4 = close"""
    cls = np.array([0, 1, 2, 2, 3], dtype=np.uint8)
    tr = [('S', 'sig', 'H'), ('H', 'open', 'N'), ('N', 'note', 'N'), ('N', 'close', 'H')]
    budget = dict(slots=[0, 0, 1, 2, 0], bars=[3, NO_SIG, NO_SIG, NO_SIG, NO_SIG], opens=['open'], need_free=[], need_full=['close'])
    g = from_transitions(cls, ['sig', 'open', 'note', 'close'], tr, 'S', budget=budget)
    assert g.budget is not None and g.budget.opens == 0b0010 and g.budget.need_full == 0b1000
    assert g.walk_budget([0, 1, 2, 3, 4, 1, 3, 2, 4]) == (3, 0, -1)
    assert g.walk_budget([0, 1, 3, 3]) == (3, 1, 3)               # 2 + 2 > 3
    assert g.walk_budget([0, 1, 3, 4]) == (3, 1, 3)               # closed one slot short
    assert from_transitions(cls, ['sig', 'open', 'note', 'close'], tr, 'S').budget is None
    with pytest.raises(ValueError, match='every token barred'):   # only two-slot notes in a bar of three
        from_transitions(cls, ['sig', 'open', 'note', 'close'], tr, 'S', budget={**budget, 'slots': [0, 0, 2, 2, 0]})
    # the min_length refusal sees the budget: with eos = close and the one-slot note gone ... close is alone at rem == 0
    with pytest.raises(ValueError, match='min_length'):
        check_grammar_args(g, 5, (4, 4, 10))
