"""generate.rules_config and the generate.RulePlan it builds, on the host: the plan's fields against the `*_config` functions it
calls, `rows` against the plan of the sliced arguments, `with_stop`, and the refusals with their order.  Where the plan meets the
device is tests/test_rule_plan_gpu.py."""
import numpy as np
import pytest
import torch

from symbolic_music_generation_amd.generate import (NO_RULES, MelodyPlan, RegisterPlan, RulePlan, bar_count_config, check_grammar_args,
                                                    key_config, melody_config, register_config, rules_config, stop_config)
from symbolic_music_generation_amd.vocab import MusicTokenizer

TOK = MusicTokenizer(pitch_kind='degree')
VOC = TOK.vocab
V = len(VOC)
G = TOK.grammar(bar_budget=True)
KEY, REG = TOK.key_rule(), TOK.register_rule()
EOS, PAD, BAR, MEL, BASS = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<bar>', '<melody>', '<bass>'))
P = [int(np.flatnonzero(KEY.pcs == pc)[0]) for pc in range(12)]    # one pitch token per pitch class
D2, D4 = VOC.t2i('d_2'), VOC.t2i('d_4')
STOP = stop_config(EOS, PAD)
MEL0 = [BAR, MEL, P[0], D2, P[4], D2, BASS]                         # bars of 4/4
MEL1 = [BAR, MEL, P[7], D4, BASS]
RANGES = [(60, 84), None, (48, 72)]

#         what                         batch  arguments of rules_config beside batch and vocab_size
TABLE = [('nothing',                   3, {}),
         ('the stop group alone',      3, dict(stop=stop_config(EOS, PAD, 7))),
         ('the grammar alone',         3, dict(grammar=G)),
         ('one n_bars for all',        3, dict(grammar=G, stop=STOP, n_bars=2)),
         ('n_bars per row',            3, dict(grammar=G, stop=STOP, n_bars=[0, -1, 3])),
         ('n_bars per row, repeated',  3, dict(grammar=G, stop=STOP, n_bars=torch.tensor([0, -1, 3]), repeat=3)),
         ('the key rule alone',        3, dict(in_key=KEY)),
         ('a key by name',             3, dict(in_key=KEY, key='AMinor')),
         ('keys per row, repeated',    3, dict(in_key=KEY, key=['CMajor', None, 5], repeat=3)),
         ('the register rule alone',   3, dict(register=REG)),
         ('ranges per row, repeated',  3, dict(register=REG, melody_range=RANGES, bass_range=(36, 60), bass_below=1, repeat=3)),
         ('a melody sets the count',   3, dict(grammar=G, stop=STOP, melody=[MEL0 + MEL1, None, MEL1], repeat=3)),
         ('one melody for all',        2, dict(grammar=G, stop=STOP, melody=MEL0)),
         ('every rule, own count',     3, dict(grammar=G, stop=STOP, n_bars=[1, 2, -1], in_key=KEY, key=[3, -1, 'GMajor'], register=REG,
                                               melody_range=RANGES, bass_below=0)),
         ('every rule, a melody',      3, dict(grammar=G, stop=STOP, melody=[MEL0, MEL1, None], in_key=KEY, key='CMajor', register=REG,
                                               bass_range=RANGES, repeat=3))]


BARE = dict(stop=None, grammar=None, n_bars=None, in_key=None, key=None, melody=None, register=None, melody_range=None,
            bass_range=None, bass_below=None)                       # every rules keyword of rules_config, off


def _same(a, b):
    """two values of one plan field: tensors by value, MelodyPlan / RegisterPlan by their parts, a rule or a grammar by identity"""
    if a is None or b is None:
        return a is b
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, MelodyPlan):
        return isinstance(b, MelodyPlan) and a.rule is b.rule and a.guides == b.guides and a.bars == b.bars and _same(a.n_bars, b.n_bars)
    if isinstance(a, RegisterPlan):
        return isinstance(b, RegisterPlan) and a.rule is b.rule and a.gap == b.gap and _same(a.bounds, b.bounds)
    return a is b or (isinstance(a, tuple) and a == b)


def _same_plan(a: RulePlan, b: RulePlan):
    return all(_same(x, y) for x, y in zip(a[:7], b[:7])) and a.B == b.B


@pytest.mark.parametrize('what,batch,kw', TABLE, ids=[t[0] for t in TABLE])
def test_builder_equals_the_parts(what, batch, kw):
    a = {**BARE, 'repeat': 1, **kw}
    plan = rules_config(batch=batch, vocab_size=V, **kw)
    guide = melody_config(a['melody'], batch, a['grammar'], a['stop'], a['n_bars'], a['repeat'])
    bars = bar_count_config(a['n_bars'], batch, a['grammar'], a['stop'], a['repeat'])
    keys = key_config(a['in_key'], a['key'], batch, V, a['repeat'])
    span = register_config(a['register'], a['melody_range'], a['bass_range'], a['bass_below'], batch, V, a['repeat'])
    assert isinstance(plan, RulePlan) and plan.stop == a['stop'] and plan.grammar is a['grammar'] and plan.in_key is a['in_key']
    assert _same(plan.melody, guide) and _same(plan.keys, keys) and _same(plan.register, span)
    assert _same(plan.n_bars, bars if guide is None else guide.n_bars)                     # a melody's bar counts take n_bars over
    rows = batch * a['repeat']
    per_row = [x for x in (plan.n_bars, plan.keys, plan.melody, plan.register) if x is not None]
    assert plan.B == (rows if per_row else None)
    assert all((x.numel() if isinstance(x, torch.Tensor) else x.B) == rows for x in per_row)
    assert plan.n_bars is None or (plan.n_bars.dtype == torch.int32 and not plan.n_bars.is_cuda)
    if what == 'nothing':
        assert plan == NO_RULES and NO_RULES == RulePlan() and all(x is None for x in NO_RULES)


def test_table_covers_what_the_plan_can_hold():
    plans = {what: rules_config(batch=batch, vocab_size=V, **kw) for what, batch, kw in TABLE}
    for field in RulePlan._fields[:7]:
        assert any(getattr(p, field) is not None for p in plans.values()) and any(getattr(p, field) is None for p in plans.values())
    assert plans['n_bars per row, repeated'].n_bars.tolist() == [0, 0, 0, -1, -1, -1, 3, 3, 3]
    assert plans['a melody sets the count'].n_bars.tolist() == [2, 2, 2, -1, -1, -1, 1, 1, 1]
    assert plans['keys per row, repeated'].keys.tolist()[3:6] == [-1] * 3
    assert all(p is not None for p in plans['every rule, a melody'][:7])


def test_rows_equal_the_plan_of_the_sliced_arguments():
    """B = 5 split 3 + 2, as XLDecoderLanes splits five rows over two lanes"""
    guides = [MEL0, None, MEL0 + MEL1, MEL1, None]
    keys = ['CMajor', None, 5, -1, 'AMinor']
    mel, bass = [(60, 84), None, (48, 72), (0, 127), (55, 55)], [None, (36, 60), (30, 40), None, (1, 2)]
    counts = [2, -1, 0, 5, 1]

    def build(lo, hi, **own):
        return rules_config(batch=hi - lo, vocab_size=V, grammar=G, stop=STOP, in_key=KEY, key=keys[lo:hi], register=REG,
                            melody_range=mel[lo:hi], bass_range=bass[lo:hi], bass_below=2, **{k: v[lo:hi] for k, v in own.items()})
    for own in (dict(melody=guides), dict(n_bars=counts)):
        whole = build(0, 5, **own)
        assert whole.B == 5 and [f for f, x in zip(RulePlan._fields, whole) if x is None] == ['melody'] * ('melody' not in own)
        for lo, hi in ((0, 3), (3, 5)):
            part = whole.rows(lo, hi)
            assert _same_plan(part, build(lo, hi, **own)) and part.B == hi - lo, (list(own), lo, hi)
        assert _same_plan(whole, build(0, 5, **own))                   # the whole plan is as it was
    assert NO_RULES.rows(0, 3) == NO_RULES
    some = rules_config(batch=5, vocab_size=V, grammar=G, in_key=KEY).rows(3, 5)     # no per-row field: nothing to cut
    assert some.B is None and some.grammar is G and some.in_key is KEY


def test_with_stop_changes_only_the_stop_group():
    plan = rules_config(batch=3, vocab_size=V, grammar=G, stop=STOP, n_bars=[1, 2, 3], in_key=KEY, key='CMajor', register=REG)
    other = plan.with_stop((EOS, PAD, 0))
    assert other.stop == (EOS, PAD, 0) and plan.stop == STOP and other is not plan
    assert all(x is y for x, y in zip(other[1:], plan[1:]))
    assert NO_RULES.with_stop((7, 7, 0)) == RulePlan(stop=(7, 7, 0)) and NO_RULES.stop is None
    with pytest.raises(AttributeError):
        plan.stop = None


def _raised(call):
    with pytest.raises(Exception) as e:
        call()
    return type(e.value), str(e.value)


#           what                              arguments of rules_config                      the same refusal from the function it belongs to
REFUSALS = [('n_bars without a grammar',      dict(stop=STOP, n_bars=2),                     lambda: bar_count_config(2, 3, None, STOP)),
            ('n_bars without an eos',         dict(grammar=G, n_bars=2),                     lambda: bar_count_config(2, 3, G, None)),
            ('n_bars with min_length',        dict(grammar=G, stop=stop_config(EOS, PAD, 5), n_bars=2),
             lambda: bar_count_config(2, 3, G, stop_config(EOS, PAD, 5))),
            ('n_bars of a wrong count',       dict(grammar=G, stop=STOP, n_bars=[1, 2]),     lambda: bar_count_config([1, 2], 3, G, STOP)),
            ('a key without the rule',        dict(key='CMajor'),                            lambda: key_config(None, 'CMajor', 3, V)),
            ('keys of a wrong count',         dict(in_key=KEY, key=[1, 2]),                  lambda: key_config(KEY, [1, 2], 3, V)),
            ('a range without the rule',      dict(melody_range=(60, 84)),
             lambda: register_config(None, (60, 84), None, None, 3, V)),
            ('bass_below without the rule',   dict(bass_below=1),                            lambda: register_config(None, None, None, 1, 3, V)),
            ('ranges of a wrong count',       dict(register=REG, bass_range=[(1, 2)] * 4),
             lambda: register_config(REG, None, [(1, 2)] * 4, None, 3, V)),
            ('a melody beside n_bars',        dict(grammar=G, stop=STOP, melody=MEL0, n_bars=1),
             lambda: melody_config(MEL0, 3, G, STOP, 1)),
            ('a melody without a grammar',    dict(stop=STOP, melody=MEL0),                  lambda: melody_config(MEL0, 3, None, STOP)),
            ('guides of a wrong count',       dict(grammar=G, stop=STOP, melody=[MEL0, MEL1]),
             lambda: melody_config([MEL0, MEL1], 3, G, STOP))]
#           over another vocabulary: (arguments, vocab_size, the function's refusal)
OTHER_VOCAB = [('a grammar',          dict(grammar=G),    lambda: check_grammar_args(G, V + 1, None)),
               ('a key rule',         dict(in_key=KEY),   lambda: key_config(KEY, None, 3, V + 1)),
               ('a register rule',    dict(register=REG), lambda: register_config(REG, None, None, None, 3, V + 1))]


@pytest.mark.parametrize('what,kw,part', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_are_those_of_the_parts(what, kw, part):
    want = _raised(part)
    assert want[0] is ValueError and _raised(lambda: rules_config(batch=3, vocab_size=V, **kw)) == want


@pytest.mark.parametrize('what,kw,part', OTHER_VOCAB, ids=[r[0] for r in OTHER_VOCAB])
def test_a_rule_over_another_vocabulary_is_refused(what, kw, part):
    from symbolic_music_generation_amd._lib import MusicXLError
    want = _raised(part)
    assert want[0] is MusicXLError and _raised(lambda: rules_config(batch=3, vocab_size=V + 1, **kw)) == want


def test_of_two_bad_arguments_the_earlier_is_refused():
    """the order: check_grammar_args, melody_config, bar_count_config, key_config, register_config"""
    by = {r[0]: r for r in REFUSALS}
    pairs = [('a melody beside n_bars', 'a key without the rule'), ('a melody without a grammar', 'a range without the rule'),
             ('n_bars without an eos', 'a key without the rule'), ('n_bars of a wrong count', 'ranges of a wrong count'),
             ('a key without the rule', 'a range without the rule'), ('keys of a wrong count', 'bass_below without the rule')]
    for first, second in pairs:
        kw = dict(by[second][1], **by[first][1])
        assert all(kw[k] == v or v is kw[k] for k, v in by[second][1].items()), (first, second)      # the pair does not collide
        assert _raised(lambda: rules_config(batch=3, vocab_size=V, **kw)) == _raised(by[first][2]), (first, second)
    # a grammar over another vocabulary comes before everything else
    for _, kw, _ in REFUSALS[:2] + REFUSALS[4:5]:
        got = _raised(lambda: rules_config(batch=3, vocab_size=V + 1, **dict(kw, grammar=G)))
        assert got == _raised(lambda: check_grammar_args(G, V + 1, None))
    assert set(BARE) == set(rules_config.__kwdefaults__) - {'repeat'}
