"""The register rule on the host (`generate(register=...)`; grammar.RegisterRule): its table over the three pitch kinds against an
independent parse of the token names, `walk` on hand-written streams, the no-dead-end argument over the edge set of
tests/register_ref.py, the composition of tests/register_ref.py against the primitives token by token, and the arguments
(generate.register_config, the refusals of generate.plan_search).  The device side is tests/test_register_rule_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

from symbolic_music_generation_amd._lib import MusicXLError
from symbolic_music_generation_amd.generate import RegisterPlan, check_register, plan_search, register_config
from symbolic_music_generation_amd.grammar import (ANY_RANGE, NO_FLOOR, NO_PITCH, REG_BAR, REG_BASS, REG_MELODY, RegisterRule,
                                                   music_register_rule, pack_bounds)
from symbolic_music_generation_amd.vocab import MusicTokenizer, MusicVocabulary
from tests import register_ref, rules_ref
from tests.register_ref import EDGE_ROWS, RegWords
from tests.rules_ref import Rules, Words, token_ids

KINDS = ('midi', 'step', 'degree')
SEMITONE = {'C': 0, 'D': 2, 'E': 4, 'F': 5, 'G': 7, 'A': 9, 'B': 11}


def _midi_from_name(vocab, tok):
    """the MIDI number of a pitch token, parsed from its name without the rule's arithmetic: for the `step` kind from the letter, its
    octave as written and the accidental that the pitch index implies; for the others from index and octave"""
    body = tok[len('p_'):].split('_')
    idx, otv = (int(x) for x in body[0].split('/'))
    if vocab.pitch_kind != 'step':
        return 12 * (otv + 1) + idx - 1
    natural = 12 * (otv + 1) + SEMITONE[body[1]]                 # the letter in the octave the name states
    # the accidental moves the natural by at most two semitones to the pitch class idx - 1
    cands = [natural + a for a in (-2, -1, 0, 1, 2) if (natural + a) % 12 == idx - 1]
    assert len(cands) == 1, tok
    return cands[0]


@pytest.mark.parametrize('kind', KINDS)
def test_table_holds_the_midi_number_of_every_pitch_token(kind):
    v = MusicVocabulary(pitch_kind=kind)
    rule = v.register_rule()
    assert isinstance(rule, RegisterRule) and rule.vocab_size == len(v) and rule.reg.dtype == np.uint8
    pitched = [t for t in v.toks['pitch'] if t not in (v.rest, v.rare_pitch)]
    for t in pitched:
        assert int(rule.reg[v.tok2id[t]]) == _midi_from_name(v, t), t
    assert sorted(set(int(rule.reg[v.tok2id[t]]) for t in pitched)) == list(range(128))
    middle_c = {'midi': 'p_1/4', 'step': 'p_1/4_C', 'degree': 'p_1/4_3'}[kind]
    assert int(rule.reg[v.tok2id[middle_c]]) == 60
    # the part tokens, and 0xFF everywhere else -- the rest and the rare pitch included
    codes = {v.start_of_melody: REG_MELODY, v.start_of_bass: REG_BASS, v.start_of_bar: REG_BAR}
    for tok, i in v.tok2id.items():
        if tok in codes:
            assert int(rule.reg[i]) == codes[tok]
        elif tok not in pitched:
            assert int(rule.reg[i]) == NO_PITCH, tok
    assert int(rule.reg[v.tok2id[v.rest]]) == int(rule.reg[v.tok2id[v.rare_pitch]]) == NO_PITCH
    assert MusicTokenizer(pitch_kind=kind).register_rule().reg.tolist() == rule.reg.tolist()


def test_step_kind_octave_adjustments_are_undone():
    """B# is written an octave below the C it sounds as, C- an octave above the B: pinned by hand"""
    v = MusicVocabulary(pitch_kind='step')
    reg = v.register_rule().reg
    pins = {'p_1/4_C': 60, 'p_1/3_B': 60,                          # C4 and B#3 are both MIDI 60
            'p_12/4_B': 71, 'p_12/5_C': 71,                        # B4 and C-5 are both MIDI 71
            'p_1/-2_B': 0, 'p_1/-1_C': 0,                          # the lowest: B#-2 and C-1
            'p_12/8_B': 119, 'p_12/9_C': 119, 'p_8/9_G': 127, 'p_3/4_C': 62, 'p_10/4_B': 69, 'p_10/4_G': 69, 'p_5/4_F': 64, 'p_6/4_E': 65}
    for tok, midi in pins.items():
        assert tok in v, tok
        assert int(reg[v.tok2id[tok]]) == midi, tok


def test_sub_word_tokenizers_raise_and_bad_tables_too():
    from symbolic_music_generation_amd.subword import PairMergeTokenizer, WordPieceMusicTokenizer
    for cls in (PairMergeTokenizer, WordPieceMusicTokenizer):
        with pytest.raises(NotImplementedError, match='register rule'):
            cls.register_rule(object.__new__(cls))
    with pytest.raises(ValueError, match='no MIDI number'):
        RegisterRule([0, 5, 0x90])
    with pytest.raises(ValueError, match='non-empty'):
        RegisterRule([])


# ---------------------------------------------------------------------------------------------------------------- walk
TOK = MusicTokenizer(pitch_kind='midi')
VOC = TOK.vocab
RULE = TOK.register_rule()
HEAD = 'TimeSig_4/4 Tempo_120 '
BOUNDS = (60, 84, 36, 59)


def _walk(text, **kw):
    return RULE.walk(token_ids(VOC, text), **kw)


def test_walk_on_hand_written_streams():
    # melody C5 E4, bass A3 then E4: the E4 of the bass is inside the gap bound only without one
    s = HEAD + '<bar> <melody> p_1/5 d_1 p_5/4 d_1 <bass> p_10/3 d_1 p_5/3 d_1'
    assert _walk(s, bounds=BOUNDS, gap=1) == (2, 64, -1)
    # a bass note above hi_bass: found at its index
    s2 = HEAD + '<bar> <melody> p_1/5 d_1 <bass> p_10/3 d_1 p_1/4 d_1'
    assert _walk(s2, bounds=BOUNDS) == (2, 72, 9)
    assert _walk(s2, bounds=(60, 84, 36, 60)) == (2, 72, -1)
    # a crossing: the bass reaches the lowest melody note of the bar (E4 = 64) -- gap 0 lets it touch, gap 1 does not
    s3 = HEAD + '<bar> <melody> p_1/5 d_1 p_5/4 d_1 <bass> p_5/4 d_1'
    assert _walk(s3, gap=-1)[2] == -1 and _walk(s3, gap=0)[2] == -1 and _walk(s3, gap=1) == (2, 64, 9)
    s4 = HEAD + '<bar> <melody> p_1/5 d_1 p_5/4 d_1 <bass> p_6/4 d_1'
    assert _walk(s4, gap=0) == (2, 64, 9) and _walk(s4, gap=-1)[2] == -1
    # the floor resets at <bar>: the second bar's bass is judged against the second bar's melody only
    s5 = HEAD + '<bar> <melody> p_1/3 d_1 <bass> p_1/2 d_1 <bar> <melody> p_1/5 d_1 <bass> p_1/4 d_1'
    assert _walk(s5, gap=1) == (2, 72, -1)
    assert _walk(s5 + ' <bar>', gap=1) == (0, NO_FLOOR, -1)
    # rests and the rare pitch are ignored: they neither move the floor nor break a bound
    s6 = HEAD + '<bar> <melody> p_r d_1 p_rare d_1 p_1/5 d_1 <bass> p_r d_1 p_rare d_1'
    assert _walk(s6, bounds=(72, 72, 0, 0), gap=1) == (2, 72, -1)
    # a melody note outside its range, and pitches before any part is open (no <melody> yet) are not judged
    assert _walk(HEAD + '<bar> <melody> p_1/3 d_1', bounds=BOUNDS) == (1, NO_FLOOR, 4)
    assert _walk('p_1/3 d_1 p_1/9 d_1', bounds=BOUNDS) == (0, NO_FLOOR, -1)


def test_walk_does_not_judge_the_prompt_and_skips_pads():
    s = token_ids(VOC, HEAD + '<bar> <melody> p_1/3 d_1 p_1/5 d_1 <bass> p_1/6 d_1 p_1/2 d_1')
    assert RULE.walk(s, BOUNDS, 1) == (1, NO_FLOOR, 4)
    # the prompt columns only move the words: the low melody note still sets the floor
    assert RULE.walk(s, BOUNDS, 1, check_from=9) == (2, 48, 9)         # the floor is C3 = 48: C6 = 84 is above 47
    assert RULE.walk(s, BOUNDS, 1, check_from=11) == (2, 48, -1)       # C2 = 36 is inside [36, 47]
    assert RULE.walk(s[:11] + token_ids(VOC, 'p_1/3 d_1'), BOUNDS, 1, check_from=11) == (2, 48, 11)      # 48 > 48 - 1
    assert RULE.walk(s, BOUNDS, 1, check_from=len(s)) == (2, 48, -1)
    # a start in the middle of a bar: part and floor given
    assert RULE.walk(token_ids(VOC, 'p_1/4 d_1'), BOUNDS, 0, part=2, floor=59) == (2, 59, 0)
    assert RULE.walk(token_ids(VOC, 'p_12/3 d_1'), BOUNDS, 0, part=2, floor=59) == (2, 59, -1)
    # pads (ids < 0) and ids beyond the vocabulary are skipped, wherever they stand
    padded = [-1, -1] + s[:4] + [len(VOC) + 5] + s[4:]
    assert RULE.walk(padded, BOUNDS, 1) == (1, NO_FLOOR, 7)
    assert RULE.walk(padded, BOUNDS, 1, check_from=12) == (2, 48, 12)
    # check_register is the walk per row, on the host here
    ids = torch.tensor([s, s])
    assert check_register(ids, RULE, melody_range=[(60, 84), None], bass_range=(36, 59), bass_below=1, prompt_len=9).tolist() == [9, 9]
    assert check_register(ids, RULE, melody_range=(60, 84), prompt_len=0).tolist() == [4, 4]
    assert check_register(ids, RULE).tolist() == [-1, -1]


# ---------------------------------------------------------------------------------------------------------------- no dead end
@pytest.mark.parametrize('kind', KINDS)
def test_rest_and_rare_pitch_always_remain(kind):
    """for every (part, floor, bounds) of the edge set and every gap: the rest and the rare pitch are kept, and they are tokens of
    the grammar's class `pitch`, so wherever the grammar or the budget allows a pitch a token is left -- also where no pitched token
    is"""
    v = MusicVocabulary(pitch_kind=kind)
    rule, g = v.register_rule(), v.grammar(bar_budget=True)
    rest, rare = v.tok2id[v.rest], v.tok2id[v.rare_pitch]
    pitch = g.class_names.index('pitch')
    assert int(g.cls[rest]) == int(g.cls[rare]) == pitch
    assert int(g.budget.slots[rest]) == int(g.budget.slots[rare]) == 0      # no duration: the budget judges them by class alone
    bounds = sorted({rw.bounds for rw in EDGE_ROWS})
    floors = sorted({rw.gfloor for rw in EDGE_ROWS} | {0, 127})
    empty = 0
    for b, part, floor, gap in itertools.product(bounds, (0, 1, 2), floors, (-1, 0, 1, 127)):
        ok = rule.allowed(part, floor, b, gap)
        assert ok[rest] and ok[rare] and ok[rule.reg > 127].all()
        assert all(rule.allows(part, floor, b, gap, t) for t in (rest, rare))
        empty += not ok[rule.reg <= 127].any()
        if part == 0:
            assert ok.all()
    assert empty > 0                                                         # the set does hold bounds that leave no pitched token
    # and in every state of the grammar that allows the class, the composed keep holds a token under such bounds
    rw = EDGE_ROWS[3]
    assert not rule.allowed(rw.gpart, rw.gfloor, rw.bounds, 1)[rule.reg <= 127].any()
    for s in g.reachable():
        if (int(g.allow[s]) >> pitch) & 1:
            k = register_ref.keep(Rules(g), Words(gstate=s), rule, rw, 1, len(v))
            assert k[rest] and k[rare]


# ---------------------------------------------------------------------------------------------------------------- composition
def test_composition_is_tied_to_the_primitives():
    """register_ref.keep / move against rules_ref's and RegisterRule's own allows / move, token by token"""
    tok = MusicTokenizer(pitch_kind='degree')
    v, g = tok.vocab, tok.grammar(bar_budget=True)
    reg, key = tok.register_rule(), tok.key_rule()
    V = len(v)
    guide = token_ids(v, '<bar> <melody> p_1/3_1 d_1 <bass>')
    cases = [(Rules(g), Words(gstate=g.state('M_OPEN'))),
             (Rules(g, budget=True, count=True, key_rule=key), Words(gstate=g.state('B_D'), gbar=32, grem=8, gleft=1, gkey=0)),
             (Rules(None, key_rule=key), Words(gkey=12)),
             (Rules(g, guide=True, count=True), Words(gstate=g.state('M_OPEN'), gpos=2, gforce=1, gleft=1)),
             (Rules(g, stop=(v.t2i('</s>'), v.t2i('[PAD]'), 0)), Words(unfinished=0, gstate=g.state('B_OPEN')))]
    rng = np.random.default_rng(0)
    for (rules, w), rw, gap in itertools.product(cases, EDGE_ROWS, (-1, 1)):
        base = rules_ref.keep(rules, w, V, guide if rules.guide else None)
        got = register_ref.keep(rules, w, reg, rw, gap, V, guide if rules.guide else None)
        forced = rules.guide and g.guide.forced(w.gpos, w.gforce, guide) >= 0
        for t in range(V):
            assert got[t] == (base[t] and (forced or reg.allows(rw.gpart, rw.gfloor, rw.bounds, gap, t))), (t, rw, gap)
        for t in rng.choice(V, 60, replace=False).tolist() + [v.t2i(x) for x in ('<bar>', '<melody>', '<bass>', '</s>', 'p_r', 'p_1/3_1')] + [V + 3]:
            out0, w0 = rules_ref.move(rules, w, t, len(guide) if rules.guide else 0)
            out, w1, rw1 = register_ref.move(rules, w, reg, rw, t, len(guide) if rules.guide else 0)
            assert (out, w1) == (out0, w0)
            live = rules.stop is None or w.unfinished
            want = reg.move(rw.gpart, rw.gfloor, t) if live and t < V else (rw.gpart, rw.gfloor)
            assert (rw1.gpart, rw1.gfloor) == want and rw1.bounds == rw.bounds
    # the register group alone: no other table is needed
    alone = Rules(None, stop=(3, 1, 5))
    k = register_ref.keep(alone, Words(), reg, EDGE_ROWS[2], -1, V, cur_len=2)
    assert not k[3] and k.sum() == reg.allowed(1, NO_FLOOR, EDGE_ROWS[2].bounds, -1).sum() - 1
    assert register_ref.move(alone, Words(unfinished=0), reg, EDGE_ROWS[2], v.t2i('<bar>'))[1:] == (Words(unfinished=0), EDGE_ROWS[2])
    assert register_ref.move(alone, Words(), reg, EDGE_ROWS[2], v.t2i('p_1/3_1'))[2] == EDGE_ROWS[2]._replace(gfloor=48)
    assert register_ref.move(alone, Words(), reg, EDGE_ROWS[2], 3)[1] == Words(unfinished=0)


def test_walk_agrees_with_keep_and_move_on_a_stream():
    """a stream walked by RegisterRule.walk is clean exactly when every token is in the composed keep of the words before it"""
    ids = token_ids(VOC, HEAD + '<bar> <melody> p_1/5 d_1 p_5/4 d_1 <bass> p_10/3 d_1 p_5/4 d_1 <bar> <melody> p_1/4 d_1 <bass> p_1/4 d_1')
    for gap in (-1, 0, 1):
        rw, first = RegWords(BOUNDS), -1
        for i, t in enumerate(ids):
            if first < 0 and not register_ref.keep(Rules(None), Words(), RULE, rw, gap, len(VOC))[t]:
                first = i
            if first < 0:
                rw = register_ref.move(Rules(None), Words(), RULE, rw, t)[2]
        assert RULE.walk(ids, BOUNDS, gap) == (rw.gpart, rw.gfloor, first)
    assert first == 11


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_register_config():
    V = len(VOC)
    assert register_config(None, None, None, None, 3, V) is None
    p = register_config(RULE, (60, 84), None, None, 2, V)
    assert isinstance(p, RegisterPlan) and p.gap == -1 and p.bounds.dtype == torch.int32
    assert p.bounds.tolist() == [pack_bounds((60, 84, 0, 127))] * 2
    assert register_config(RULE, None, None, None, 2, V).bounds.tolist() == [pack_bounds(ANY_RANGE)] * 2
    p = register_config(RULE, [(60, 84), None, (0, 127)], [None, (36, 36), [40, 50]], 0, 3, V, repeat=2)
    assert p.gap == 0 and p.bounds.tolist() == [pack_bounds(b) for b in ((60, 84, 0, 127), (0, 127, 36, 36), (0, 127, 40, 50)) for _ in range(2)]
    assert p.rows(2, 4).bounds.tolist() == p.bounds.tolist()[2:4] and p.rows(2, 4).gap == 0 and p.rows(0, 1).rule is RULE
    assert register_config(p, None, None, None, 3, V, repeat=2) is p
    assert register_config(RULE, torch.tensor([[1, 2], [3, 4]]), None, 127, 2, V).bounds.tolist() == [pack_bounds((1, 2, 0, 127)), pack_bounds((3, 4, 0, 127))]
    assert pack_bounds((0, 127, 0, 127)) == 0x7F007F00 and pack_bounds((127, 127, 127, 127)) < 2 ** 31
    for bad, match in ((dict(melody_range=(70, 60)), 'above hi'), (dict(bass_range=(0, 128)), 'outside the MIDI numbers'),
                       (dict(melody_range=(-1, 5)), 'outside the MIDI numbers'), (dict(melody_range=[(1, 2)] * 3), '3 entries for 2 prompts'),
                       (dict(bass_range=[(1, 2), (5, 4)]), 'above hi'), (dict(melody_range=(1, 2, 3)), '3 entries for 2 prompts'),
                       (dict(melody_range='ab'), 'pair'), (dict(melody_range=(1.0, 2)), 'pair'), (dict(bass_below=-1), 'bass_below'),
                       (dict(bass_below=128), 'bass_below'), (dict(bass_below=1.5), 'bass_below')):
        kw = dict(melody_range=None, bass_range=None, bass_below=None)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            register_config(RULE, batch=2, vocab_size=V, **kw)
    for kw, name in ((dict(bass_below=1), 'bass_below'), (dict(melody_range=(1, 2)), 'melody_range'), (dict(bass_range=(1, 2)), 'bass_range')):
        with pytest.raises(ValueError, match=f'{name}= needs register='):
            register_config(None, **dict(dict(melody_range=None, bass_range=None, bass_below=None), **kw), batch=2, vocab_size=V)
    with pytest.raises(MusicXLError, match='spans 422 tokens'):
        register_config(RULE, None, None, None, 2, 1190)
    with pytest.raises(ValueError, match='plan holds 6 rows'):
        register_config(p, None, None, None, 2, V)


CAPS = dict(beam=16, group_beam=16, contrastive=32, beam_sample=16)


def test_plan_search_takes_and_refuses_the_rule():
    refusal = 'register= is supported for greedy decoding and sampling only'
    assert plan_search(CAPS, register=RULE).rules and plan_search(CAPS, do_sample=True, register=RULE).strategy == 'sample'
    assert plan_search(CAPS).rules                                            # the keyword defaults to None
    # the host scorers refuse it: no explicit eos, the environment switches, beam-sample without the device scorer, no device at all
    for kw in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(penalty_alpha=0.6, top_k=4),
               dict(num_beams=2, do_sample=True, eos_token_id=3), dict(penalty_alpha=0.6, top_k=64, eos_token_id=3),
               dict(num_beams=32, eos_token_id=3)):
        with pytest.raises(MusicXLError, match=refusal):
            plan_search(CAPS, register=RULE, **kw)
    with pytest.raises(MusicXLError, match=refusal):
        plan_search({}, num_beams=2, eos_token_id=3, register=RULE)
    # the device searches take it, given an explicit eos; group beam search goes to the device for it
    for kw, strategy in ((dict(num_beams=2), 'beam'), (dict(num_beams=4, num_beam_groups=2), 'group_beam'),
                         (dict(penalty_alpha=0.6, top_k=4), 'contrastive'),
                         (dict(num_beams=2, do_sample=True, device_scorer=True, renormalize_logits=True), 'beam_sample')):
        plan = plan_search(CAPS, register=RULE, eos_token_id=3, **kw)
        assert (plan.strategy, plan.device, plan.rules) == (strategy, True, True)
    assert not plan_search(CAPS, num_beams=4, num_beam_groups=2, eos_token_id=3).device
    # the refusals that stood before stand before this one
    with pytest.raises(MusicXLError, match='padded prompts'):
        plan_search(CAPS, num_beams=2, eos_token_id=3, padded=True, register=RULE)
    with pytest.raises(MusicXLError, match='melody= is'):
        plan_search(CAPS, num_beams=2, eos_token_id=3, melody=[1], register=RULE)


def test_plan_search_host_switch(monkeypatch):
    monkeypatch.setenv('MXL_BEAM_HOST', '1')
    with pytest.raises(MusicXLError, match='register= is supported'):
        plan_search(CAPS, num_beams=2, eos_token_id=3, register=RULE)
