"""The guide rule behind `generate(melody=...)` on the host (grammar.MelodyGuide): the rule on a hand-written stream,
`tokenizer.melody_guide` on a grammar-clean piece, generate.melody_config's refusals, generate.check_melody, and the argument checks
of the three entries that take the guide group (mxl_sample_step, mxl_rules_mask, mxl_rules_advance), which run before any launch.  The device side is tests/test_melody_guide_gpu.py."""
import numpy as np
import pytest
import torch

from symbolic_music_generation_amd._lib import MusicXLError
from symbolic_music_generation_amd.generate import MelodyPlan, check_melody, melody_config, stop_config
from symbolic_music_generation_amd.grammar import (MUSIC_CLASSES, MUSIC_TRANSITIONS, NO_PITCH, MelodyGuide, TokenGrammar,
                                                   from_transitions)
from symbolic_music_generation_amd.vocab import MusicTokenizer

TOK = MusicTokenizer(pitch_kind='degree')
VOC = TOK.vocab
G = TOK.grammar(bar_budget=True)
RULE = TOK.key_rule()
EOS, PAD, BAR, MEL, BASS, TUP, TUPE = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<bar>', '<melody>', '<bass>', '<tup>', '</tup>'))
P = [int(np.flatnonzero(RULE.pcs == pc)[0]) for pc in range(12)]   # one pitch token per pitch class
D = {k: VOC.t2i(f'd_{k}') for k in ('1/4', '1/2', '1', '2', '3', '4')}
STOP = stop_config(EOS, PAD)


def _ids(text):
    return [VOC.t2i(t) for t in text.split()]


HEAD = _ids('TimeSig_4/4 Tempo_120 Key_CMajor')
# three bars of 4/4 (32 slots): two plain, one with a tuplet in the melody
MEL0 = [BAR, MEL, P[0], D['2'], P[4], D['2'], BASS]
MEL1 = [BAR, MEL, TUP, P[0], P[2], P[4], D['1'], TUPE, P[5], D['3'], BASS]
MEL2 = [BAR, MEL, P[7], D['4'], BASS]
BASS0, BASS1, BASS2 = [P[0], D['4']], [P[5], D['2'], P[7], D['2']], [P[0], D['1'], P[4], D['3']]
PIECE = HEAD + MEL0 + BASS0 + MEL1 + BASS1 + MEL2 + BASS2 + [EOS]


def test_the_piece_is_clean_and_the_grammar_carries_the_rule():
    assert G.walk(PIECE)[1] == -1 and G.walk_budget(PIECE)[2] == -1 and G.accepts(PIECE)
    for g in (G, TOK.grammar()):
        assert isinstance(g.guide, MelodyGuide) and g.guide.grammar is g
        assert g.guide.enter == 1 << MUSIC_CLASSES.index('<bar>') and g.guide.leave == 1 << MUSIC_CLASSES.index('<bass>')
    # from_transitions attaches one to a grammar of the caller's own, or none
    own = from_transitions(G.cls, MUSIC_CLASSES, MUSIC_TRANSITIONS, 'S0', guide=dict(enter=('<bar>',), leave=('<bass>',)))
    assert own.guide.enter == G.guide.enter and from_transitions(G.cls, MUSIC_CLASSES, MUSIC_TRANSITIONS, 'S0').guide is None
    with pytest.raises(ValueError, match='both open and close'):
        MelodyGuide(own, ('<bar>',), ('<bar>', '<bass>'))
    with pytest.raises(ValueError, match='at least one class'):
        MelodyGuide(own, 0, ('<bass>',))
    with pytest.raises(ValueError, match='unknown token class'):
        MelodyGuide(own, ('<bar>',), ('<chord>',))


def test_walk_allows_and_move_on_a_hand_written_stream():
    r = G.guide
    guide = MEL0 + MEL1
    c = lambda t: int(G.cls[t])
    # the walk spelled out: free through the header, fed from <bar> to <bass>, free through the bass, fed again
    stream = HEAD + MEL0 + BASS0 + MEL1 + BASS1 + [EOS]
    pos, force, trace = 0, 0, []
    for t in stream:
        assert r.allows(pos, force, guide, t)
        trace.append((pos, force, r.forced(pos, force, guide)))
        pos, force = r.move(pos, force, len(guide), c(t))
    assert (pos, force) == (len(guide), 0)
    n0, nh = len(MEL0), len(HEAD)
    assert trace[:nh + 1] == [(0, 0, -1)] * (nh + 1)                                       # <bar> itself is chosen, not fed
    assert trace[nh + 1:nh + n0] == [(i, 1, MEL0[i]) for i in range(1, n0)]                # <melody> .. <bass> are fed
    assert trace[nh + n0:nh + n0 + len(BASS0) + 1] == [(n0, 0, -1)] * (len(BASS0) + 1)     # the bass and the next <bar>: free
    assert trace[nh + n0 + len(BASS0) + 1][1:] == (1, MEL1[1])
    assert r.walk(stream, guide) == (len(guide), 0, -1)
    assert r.walk(np.array(stream), torch.tensor(guide)) == (len(guide), 0, -1)
    # single moves
    assert r.move(0, 0, 5, c(BAR)) == (1, 1) and r.move(5, 0, 5, c(BAR)) == (5, 0) and r.move(0, 0, 0, c(BAR)) == (0, 0)
    assert r.move(3, 1, 9, c(P[0])) == (4, 1) and r.move(3, 1, 9, c(BASS)) == (4, 0) and r.move(3, 0, 9, c(BASS)) == (3, 0)
    assert r.forced(2, 1, guide) == guide[2] and r.forced(2, 0, guide) == -1 and r.forced(len(guide), 1, guide) == -1
    assert r.allows(2, 1, guide, guide[2]) and not r.allows(2, 1, guide, guide[2] + 1) and r.allows(2, 0, guide, guide[2] + 1)
    # a departing melody token, a bar beyond the guide, a row that starts fed; pads and ids beyond the vocabulary are skipped
    bad = list(stream)
    bad[nh + 3] = D['1']
    assert r.walk(bad, guide) == (3, 1, nh + 3)
    more = HEAD + MEL0 + BASS0 + MEL1 + BASS1 + MEL2
    assert r.walk(more, guide) == (len(guide), 0, len(more) - len(MEL2))
    assert r.walk(MEL0[1:] + BASS0, guide, 1, 1) == (n0, 0, -1)
    assert r.walk([-1, -1, len(VOC) + 5] + stream, guide) == (len(guide), 0, -1)
    assert r.split(guide) == [MEL0, MEL1]
    for broken, what in ((MEL0[1:], 'opens no guided span'), (MEL0[:-1], 'never reaches'), ([], 'empty guide'),
                         (MEL0 + BASS0, 'opens no guided span'), (MEL0 + [len(VOC)], 'outside the vocabulary')):
        with pytest.raises(ValueError, match=what):
            r.split(broken)


def test_melody_guide_round_trip():
    assert TOK.melody_guide(PIECE) == MEL0 + MEL1 + MEL2 == TOK.melody_guide(torch.tensor(PIECE))
    assert TOK.melody_guide(PIECE, first_bar=1) == MEL1 + MEL2
    assert TOK.melody_guide(PIECE, first_bar=1, n_bars=1) == MEL1 and TOK.melody_guide(PIECE, n_bars=2) == MEL0 + MEL1
    assert TOK.melody_guide(PIECE, first_bar=3) == [] and TOK.melody_guide(PIECE, n_bars=0) == []
    assert G.guide.split(TOK.melody_guide(PIECE)) == [MEL0, MEL1, MEL2]
    assert G.guide.walk(PIECE, TOK.melody_guide(PIECE))[2] == -1                           # the piece follows its own guide
    with pytest.raises(ValueError, match='asked of a piece with 3 bars'):
        TOK.melody_guide(PIECE, first_bar=2, n_bars=2)
    broken = list(PIECE)
    broken[len(HEAD) + 2], broken[len(HEAD) + 3] = broken[len(HEAD) + 3], broken[len(HEAD) + 2]     # a duration before its pitch
    with pytest.raises(MusicXLError, match=f'breaks the grammar at index {len(HEAD) + 2}'):
        TOK.melody_guide(broken)
    from symbolic_music_generation_amd.subword import PairMergeTokenizer, WordPieceMusicTokenizer
    for cls in (PairMergeTokenizer, WordPieceMusicTokenizer):
        with pytest.raises(NotImplementedError, match='melody guide'):
            cls.melody_guide(object.__new__(cls), PIECE)


def test_melody_config_and_its_refusals():
    guide = MEL0 + MEL1
    plan = melody_config(guide, 3, G, STOP)
    assert isinstance(plan, MelodyPlan) and plan.B == 3 and plan.n_bars.tolist() == [2, 2, 2] and plan.n_bars.dtype == torch.int32
    plan = melody_config([guide, None, torch.tensor(MEL2)], 3, G, STOP, repeat=2)
    assert plan.B == 6 and plan.n_bars.tolist() == [2, 2, -1, -1, 1, 1]
    tok, glen = plan.tables()
    assert tok.dtype == glen.dtype == torch.int32 and glen.tolist() == [len(guide)] * 2 + [0, 0] + [len(MEL2)] * 2
    assert tok[0].tolist() == guide and tok[4, :len(MEL2)].tolist() == MEL2 and not tok[2].any()
    half = plan.rows(2, 5)
    assert half.B == 3 and half.n_bars.tolist() == [-1, -1, 1] and half.tables()[1].tolist() == [0, 0, len(MEL2)]
    assert melody_config(plan, 3, G, STOP, repeat=2) is plan and melody_config(None, 3, None, None) is None
    plan.check_budget(G, [32] * 6)                                 # 4/4: every guided melody fills its bar
    plan.check_budget(G, [0] * 6)                                  # no known time signature: not judged
    with pytest.raises(MusicXLError, match=rf'row 0 underfills its bar at guide index {len(MEL0) - 1}: token {BASS}'):
        plan.check_budget(G, [48] * 6)                             # 6/4: the <bass> comes 16 slots early
    with pytest.raises(MusicXLError, match=rf'row 4 overfills its bar at guide index 3: token {D["4"]}'):
        plan.check_budget(G, [32, 32, 32, 32, 24, 24])             # 3/4: d_4 does not fit
    for kw, what in ((dict(grammar=None), 'needs grammar='), (dict(stop=None), 'explicit eos_token_id'),
                     (dict(n_bars=2), 'n_bars together with melody'), (dict(stop=stop_config(EOS, PAD, 5)), 'min_length'),
                     (dict(melody=[guide, guide]), '2 guides for 3 prompts'), (dict(stop=stop_config(BAR, PAD)), 'no `end` token'),
                     (dict(melody=[guide, 'x', None]), '1-D sequence of token ids')):
        args = dict(melody=guide, batch=3, grammar=G, stop=STOP)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            melody_config(**args)
    bare = TokenGrammar(G.cls, G.allow, G.next, G.start)
    with pytest.raises(ValueError, match='guide rule'):
        melody_config(guide, 3, bare, STOP)
    MelodyGuide(bare, G.guide.enter, G.guide.leave)
    with pytest.raises(ValueError, match='bar count'):
        melody_config(guide, 3, bare, STOP)
    with pytest.raises(ValueError, match='holds 6 rows'):
        melody_config(plan, 3, G, STOP)
    for broken, what in ((MEL0 + BASS0 + MEL1, 'row 1 does not split into bars'), (MEL0[:-1], 'row 1 does not split into bars'),
                         ([BAR, P[0], D['4'], BASS], 'row 1 breaks the grammar at guide index 1'),
                         (MEL0 + [BAR, MEL, P[0], P[1], BASS], f'row 1 breaks the grammar at guide index {len(MEL0) + 3}')):
        with pytest.raises(MusicXLError, match=what):
            melody_config([guide, broken, None], 3, G, STOP)


def test_check_melody():
    guide = MEL0 + MEL1
    Tp = len(HEAD)
    good = HEAD + MEL0 + BASS0 + MEL1 + BASS1 + [EOS, PAD, PAD]
    W = len(good)
    fit = lambda r: r[:W] + [PAD] * (W - len(r))
    wrong = list(good)
    wrong[Tp + 12] = P[11]                                         # inside the second melody span: a pitch of its tuplet
    short = fit(HEAD + MEL0 + BASS0 + [EOS])                       # ended with a guided bar never opened
    long_ = fit(HEAD + MEL0 + BASS0 + MEL1 + BASS1[:2] + MEL2[:3]) # a third bar opened
    cut = fit(HEAD + MEL0 + BASS0 + MEL1[:4])[:Tp + 13]            # cut by max_length inside a span: judged up to the cut
    rows = torch.tensor([good, wrong, short, long_])
    assert check_melody(rows, G, guide, prompt_len=Tp).tolist() == [-1, Tp + 12, Tp + len(MEL0) + len(BASS0),
                                                                    Tp + len(MEL0) + len(BASS0) + len(MEL1) + 2]
    assert check_melody(torch.tensor(cut), G, guide, prompt_len=Tp).tolist() == [-1]
    assert check_melody(rows, G, [guide, None, None, guide[:len(MEL0)]], prompt_len=Tp).tolist() == [-1, -1, -1, Tp + len(MEL0) + len(BASS0)]
    # a prompt that ends inside a bar: that bar is finished freely, the guide engages at the next <bar>
    mid = HEAD + [BAR, MEL, P[2], D['4'], BASS, P[2]]
    rows = torch.tensor([mid + [D['4']] + MEL0 + BASS0 + MEL1 + BASS1 + [EOS]])
    assert check_melody(rows, G, guide, prompt_len=len(mid)).tolist() == [-1]
    # left-padded: prompt_len defaults to the mask's width
    padded = torch.tensor([[PAD] * 2 + good])
    mask = torch.ones(1, 2 + Tp, dtype=torch.int64)
    mask[:, :2] = 0
    assert check_melody(padded, G, guide, attention_mask=mask).tolist() == [-1]
    padded[0, 2 + Tp + 3] = D['1']
    assert check_melody(padded, G, guide, attention_mask=mask).tolist() == [2 + Tp + 3]
    with pytest.raises(ValueError, match='guide rule'):
        check_melody(rows, TokenGrammar(G.cls, G.allow, G.next, G.start), guide)


def _rules(**given):
    """an mxl_rules (include/musicxl.h) with every group off, then `given` by field name; pointers are never followed before a
    launch, so any non-zero value stands for one"""
    import ctypes
    from symbolic_music_generation_amd import _lib
    r = _lib.struct('mxl_rules')(eos_id=3, pad_id=1)
    for k, v in given.items():
        assert hasattr(r, k), k
        setattr(r, k, v)
    return ctypes.byref(r)


def test_guided_argument_errors_without_gpu():
    """the one check of the rules runs before any launch, in all three entries, with the guide group in the struct"""
    from symbolic_music_generation_amd import _lib
    L = _lib.lib()
    decl = _lib.declared_functions()
    assert [n for n in decl if n.startswith('mxl_sample_step')] == ['mxl_sample_step']
    # the guide group crosses the ABI inside mxl_rules, behind the key group: no entry of its own
    assert not [n for n in decl if 'guided' in n or 'keyed' in n]
    fields = [f for f, _ in _lib.struct('mxl_rules')._fields_]
    at = fields.index('gkey') + 1
    assert fields[at:at + 7] == ['guide', 'ld_guide', 'glen', 'enter', 'leave', 'gpos', 'gforce']
    Pt = 4096                                                      # stands for a device pointer
    step = [Pt, 16, 16, Pt, 8, Pt, Pt, 0, 2, 0, 0, 1.0, 1.0, 1.0, 1.0, Pt, Pt, 8, 1.0, Pt]
    entries = {'mxl_sample_step': lambda r: L.mxl_sample_step(*step, r, None, None),
               'mxl_rules_mask': lambda r: L.mxl_rules_mask(Pt, 16, 2, 16, Pt, r, None),
               'mxl_rules_advance': lambda r: L.mxl_rules_advance(Pt, 8, Pt, 2, 16, r, None)}
    # nothing in force: the unfused pair returns before any launch, so 0 here means the arguments passed the check
    assert entries['mxl_rules_mask'](_rules()) == 0 and entries['mxl_rules_advance'](_rules()) == 0
    grammar = dict(cls=Pt, allow=Pt, next=Pt, C=12, gstate=Pt)
    guide = dict(guide=Pt, ld_guide=8, glen=Pt, enter=1, leave=2, gpos=Pt, gforce=Pt)
    bad = {'gpos without gforce': {**grammar, **guide, 'gforce': None},
           'gforce without gpos': {**grammar, **guide, 'gpos': None},
           'guide group without its tokens': {**grammar, **guide, 'guide': None},
           'guide group without glen': {**grammar, **guide, 'glen': None},
           'tokens alone': {**grammar, 'guide': Pt, 'ld_guide': 8},
           'guide without cls': dict(guide),
           'a guide of no columns': {**grammar, **guide, 'ld_guide': 0},
           'gkey without its tables': {**grammar, **guide, 'gkey': Pt}}
    for what, given in bad.items():
        for name, call in entries.items():
            assert call(_rules(**given)) == -1, (what, name)
    # the fused launch alone: the guide rides on the grammar there
    assert entries['mxl_sample_step'](_rules(cls=Pt, **guide)) == -1
    assert L.mxl_sample_step(None, *step[1:], _rules(**grammar, **guide), None, None) == -1                    # NULL scores
