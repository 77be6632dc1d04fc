"""Song form, whole generations (`generate(form=...)`; include/musicxl.h, "Rules of a generation", group `repeat`): planned bars are
token-equal to the earlier generated bars they repeat, on every path of greedy decoding and sampling -- the fused and the unfused tail,
graph replay and the eager loop, one and two lanes, the large-vocabulary sampler -- and equal to a host loop that copies the same
tokens through XLDecoder.force_tokens; the melody span, the combinations with the other rules, the Reformer and the refusals.  Every
row of every generation here ends by eos: max_length leaves room for the longest bars the biased model writes.  Every test fails
without the feature: `form=` is swallowed and check_form does not exist.  Kernel level: tests/test_form_ops_gpu.py; host:
tests/test_form_cpu.py."""
import pytest
import torch

from symbolic_music_generation_amd.generate import (bars_after_prompt, check_bar_lengths, check_form, check_grammar, check_in_key,
                                                    check_register, left_pad, sampling_config)
from symbolic_music_generation_amd.grammar import NO_KEY, NO_PITCH, BarRepeat, subword_grammar
from symbolic_music_generation_amd.vocab import MusicTokenizer
from tests import form_ref
from tests.form_ref import Form, bars_of, melody_of
from tests.rules_ref import Rules, Words, fresh_generate, i32, token_ids

pytestmark = pytest.mark.gpu

TOK = MusicTokenizer(pitch_kind='degree')
VOC = TOK.vocab
V = len(VOC)
G = TOK.grammar(bar_budget=True)
RP = G.repeat
RULE = TOK.key_rule()
REG = TOK.register_rule()
EOS, PAD, TUP = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<tup>'))
D1, D2 = VOC.t2i('d_1'), VOC.t2i('d_2')
STOP = dict(eos_token_id=EOS, pad_token_id=PAD)
STOP3 = (EOS, PAD, 0)
# 2/4 is the shortest time signature of the vocabulary (16 slots): under the model's bias towards d_1 and d_2 a channel is one or two
# notes, a bar at most 2 + 4 + 1 + 4 tokens
HEADER = 'TimeSig_2/4 Tempo_120 Key_CMajor'
ONE_BAR = ' <bar> <melody> p_r d_2 <bass> p_r d_2'
MID_BAR = HEADER + ' <bar> <melody> p_r d_2 <bass> p_r'            # ends inside a bass note: that bar is finished freely, unnumbered
BAR_TOKENS = 12
TOP8 = dict(do_sample=True, top_k=8, temperature=1.0)
# Greedy decoding of a model that was never trained settles into one bar and writes it again and again, which would make every bar
# equal to every other, planned or not.  Under a repetition penalty the greedy choice depends on what the row holds already, so the
# free bars differ -- and the copied tokens are kept against the penalty too.
GREEDY = dict(do_sample=False, repetition_penalty=1.3)


def _model(dev, seed):
    """the 2-layer pair of the rule tests (V = 1190) with a head bias that favours pitches and long durations and keeps tuplets and
    key tokens away, so that bars stay short"""
    from tests.test_xl_model_gpu import _pair
    ref, m = _pair(dev, n_layer=2, mem_len=64, seed=seed, max_length=256)
    with torch.no_grad():
        b = ref.crit.out_layers[0].bias
        b[torch.from_numpy(RULE.pcs != NO_PITCH)] += 3.0
        b[torch.from_numpy(RULE.keys != NO_KEY)] -= 30.0
        b[TUP] -= 30.0
        b[D1] += 6.0
        b[D2] += 6.0
    m.load_state_dict(ref.state_dict())
    return m.eval()


@pytest.fixture(scope='module')
def model(dev):
    return _model(dev, 620)


def _prompts(kind, dev, times=1):
    """(ids, attention_mask or None) of 4 * times prompts"""
    if kind == 'header':
        return torch.tensor([token_ids(VOC, HEADER)] * 4 * times, device=dev), None
    if kind == 'mid-bar':
        return torch.tensor([token_ids(VOC, MID_BAR)] * 4 * times, device=dev), None
    texts = [HEADER, MID_BAR, HEADER + ONE_BAR, 'TimeSig_2/4 Tempo_96']                # three lengths
    ids, mask = left_pad([torch.tensor(token_ids(VOC, t)) for t in texts] * times, PAD)
    return ids.to(dev), mask.to(dev)


def _plans(form, section_bars, n):
    forms = form if isinstance(form, list) and (len(form) == 0 or not isinstance(form[0], int)) else [form] * n
    return [None if f is None else BarRepeat.plan_of(f, section_bars) for f in forms]


def _assert_follows(out, Tp, form, section_bars=1, span='bar', mask=None, varied=True):
    """every row ends by eos, obeys the grammar and the bar budget, opens exactly the planned bars and keeps check_form at -1; parsed
    into bars on the host, the bars are token-equal where the plan says so (`span`: the whole bar or its melody) -- and the free bars
    of a row are not all one bar, or the equality would show nothing"""
    n = out.shape[0]
    plans = _plans(form, section_bars, n)
    assert all(p is not None for p in plans)
    assert check_form(out, G, form, section_bars, span, prompt_len=Tp).tolist() == [-1] * n
    assert check_grammar(out, G, mask).tolist() == [-1] * n and check_bar_lengths(out, G, mask).tolist() == [-1] * n
    assert bars_after_prompt(out, G, prompt_len=Tp).tolist() == [len(p) for p in plans]
    gen = out[:, Tp:].cpu()
    first = (gen == EOS).int().argmax(1)
    for b, plan in enumerate(plans):
        assert gen[b, first[b]] == EOS and (gen[b, first[b] + 1:] == PAD).all() and (gen[b, :first[b]] != EOS).all(), b      # one </s>, then pad
        bars = bars_of(out[b].tolist(), G, Tp)
        assert len(bars) == len(plan)
        cut = (lambda x: melody_of(x, G)) if span == 'melody' else (lambda x: x)
        for k, j in enumerate(plan):
            assert j < 0 or cut(bars[k]) == cut(bars[j]), (b, k, j)
        free = {tuple(bars[k]) for k, j in enumerate(plan) if j < 0}
        assert not varied or sum(j < 0 for j in plan) < 2 or len(free) > 1, b


def _copied_by_the_host(m, ids, mask, L, plans, span):
    """the same generation from existing features alone: the bar count set by hand, every copied token written over the sampled one
    with XLDecoder.force_tokens, and the words of the rules, which moved along the sampled token, set to what the host rules make of
    the copied one; the repeat group's own words are kept here, by BarRepeat.move"""
    from symbolic_music_generation_amd.generate import XLDecoder, rules_config
    dev, n, Tp = ids.device, ids.shape[0], ids.shape[1]
    dec = XLDecoder(m.engine, n, L)
    samp = sampling_config(**GREEDY)
    n_pad = None if mask is None else (mask == 0).sum(1).to(torch.int32)
    dec.begin(ids, L, samp, False, n_pad, rules_config(batch=n, vocab_size=V, stop=STOP3, grammar=G, n_bars=[len(p) for p in plans]))
    fed = Rules(G, budget=True, count=True, stop=STOP3)
    free = fed._replace(automaton=False, budget=False, count=False)    # a row that chose: the device has moved those words itself
    four = ('gstate', 'gbar', 'grem', 'gleft')

    def read():
        return [dict(zip(four, w)) for w in zip(*(getattr(dec, k).tolist() for k in four))]

    t = Tp                                                         # the first token, sampled by begin: no row copies yet
    rows, forms = [], []
    for u, w, tok, p in zip(dec.unfinished.tolist(), read(), dec.ids[:, t].tolist(), plans):
        _, w, f, _ = form_ref.move(free, Words(1, **w), Form(0, -1, 0, (-1,) * len(p)), p, tok, t, span)
        rows.append(w._replace(unfinished=u))
        forms.append(f)
    while any(w.unfinished for w in rows) and t + 1 < L:
        dec.step(samp)
        t += 1
        kept, hist = dec.ids[:, t].tolist(), dec.ids[:, :t].tolist()
        for b, (w, now, p) in enumerate(zip(rows, read(), plans)):
            f = form_ref.forced(fed, forms[b], p, hist[b]) if w.unfinished else -1
            if f >= 0:                                             # every word from where the row stood before the step
                kept[b], rows[b], forms[b], _ = form_ref.move(fed, w, forms[b], p, f, t, span)
            else:
                kept[b], rows[b], forms[b], _ = form_ref.move(free, w._replace(**now), forms[b], p, kept[b], t, span)
        dec.force_tokens(torch.tensor(kept, device=dev))
        for k in four:
            getattr(dec, k).copy_(i32([getattr(w, k) for w in rows], dev))
        dec.unfinished.copy_(i32([w.unfinished for w in rows], dev))
        dec.alive.fill_(sum(w.unfinished for w in rows))
    return dec.ids[:, :t + 1].clone()


# ---------------------------------------------------------------------------------------------------------------- every path
@pytest.mark.parametrize('kind', ['header', 'mid-bar', 'left-padded'])
def test_greedy_form_on_every_path(dev, model, kind, monkeypatch):
    from symbolic_music_generation_amd.generate import XLDecoder, XLDecoderLanes
    m = model
    ids, mask = _prompts(kind, dev)
    Tp = ids.shape[1]
    L = Tp + 8 + 8 * BAR_TOKENS + 1                                # the bass a prompt left open, eight bars, </s>
    kw = dict(max_length=L, grammar=G, form='AABA', section_bars=2, attention_mask=mask, **STOP, **GREEDY)
    _assert_follows(fresh_generate(m, ids, **{**kw, 'repetition_penalty': None}), Tp, 'AABA', 2, mask=mask, varied=False)
    base = fresh_generate(m, ids, **kw)
    assert m._decoder.fused_sampler and torch.equal(base[:, :Tp], ids)
    _assert_follows(base, Tp, 'AABA', 2, mask=mask)
    plan = BarRepeat.plan_of('AABA', 2)
    assert m._decoder.rules.nplan.tolist() == [8] * 4 and m._decoder.rules.plan[0, :8].tolist() == plan
    assert m._decoder.rules.gbars.tolist() == [8] * 4 and m._decoder.rules.gcopy.tolist() == [-1] * 4
    assert torch.equal(fresh_generate(m, ids, use_graph=False, **kw), base)
    n_pad = None if mask is None else (mask == 0).sum(1).to(torch.int32)
    lanes = XLDecoderLanes(m.engine, 4, L, lanes=2)
    assert torch.equal(lanes.generate(ids, L, grammar=G, form='AABA', section_bars=2, n_pad=n_pad, **STOP, **GREEDY), base)
    assert [d.rules.nplan.tolist() for d in lanes.lanes] == [[8, 8], [8, 8]]
    monkeypatch.setenv('MXL_DECODE_UNFUSED', '1')
    assert torch.equal(fresh_generate(m, ids, **kw), base) and not m._decoder.fused_sampler
    assert torch.equal(fresh_generate(m, ids, use_graph=False, **kw), base)
    monkeypatch.setenv('MXL_SAMPLE_LARGE', '1')
    assert torch.equal(fresh_generate(m, ids, **kw), base)
    monkeypatch.delenv('MXL_SAMPLE_LARGE')
    monkeypatch.delenv('MXL_DECODE_UNFUSED')
    assert XLDecoder(m.engine, 2, 32).fused_sampler
    want = _copied_by_the_host(m, ids, mask, L, [plan] * 4, 0)
    assert want.shape[1] == base.shape[1] and torch.equal(want[:, Tp:], base[:, Tp:])


def test_sampled_form_on_every_path(dev, model, monkeypatch):
    """the large-vocabulary sampler draws by bisection over order keys, the sort sampler along its sorted support: the same seed
    gives them other tokens, with or without a form, so under sampling that sampler is held to the plan and to itself"""
    m = model
    ids, mask = _prompts('left-padded', dev)
    Tp = ids.shape[1]
    L = Tp + 8 + 8 * BAR_TOKENS + 1
    kw = dict(max_length=L, grammar=G, form='AABA', section_bars=2, seed=11, attention_mask=mask, **STOP, **TOP8)
    base = fresh_generate(m, ids, **kw)
    assert m._decoder.fused_sampler
    _assert_follows(base, Tp, 'AABA', 2, mask=mask)
    assert torch.equal(fresh_generate(m, ids, use_graph=False, **kw), base)
    monkeypatch.setenv('MXL_DECODE_UNFUSED', '1')
    assert torch.equal(fresh_generate(m, ids, **kw), base) and not m._decoder.fused_sampler
    assert torch.equal(fresh_generate(m, ids, use_graph=False, **kw), base)
    monkeypatch.setenv('MXL_SAMPLE_LARGE', '1')
    large = fresh_generate(m, ids, **kw)
    _assert_follows(large, Tp, 'AABA', 2, mask=mask)
    assert torch.equal(fresh_generate(m, ids, use_graph=False, **kw), large)
    monkeypatch.delenv('MXL_SAMPLE_LARGE')
    monkeypatch.delenv('MXL_DECODE_UNFUSED')
    assert not torch.equal(fresh_generate(m, ids, **{**kw, 'seed': 12}), base)             # another seed, another piece
    # the FP8 rings are another model arithmetic: another piece, the same form
    _assert_follows(fresh_generate(m, ids, kv_cache_dtype='fp8', **kw), Tp, 'AABA', 2, mask=mask)
    m._decoder = None


def test_one_and_two_lanes(dev, model, monkeypatch):
    """32 rows: generate cuts them into two free-running lanes.  Greedy rows do not depend on the cut; a sampled lane draws by its
    own seed and its rows' indices in it (XLDecoderLanes), so each lane is compared with one decoder under that seed"""
    from symbolic_music_generation_amd.generate import XLDecoder, XLDecoderLanes
    m = model
    ids, mask = _prompts('left-padded', dev, times=8)
    Tp = ids.shape[1]
    L = Tp + 8 + 8 * BAR_TOKENS + 1
    form = ['AABA', 'ABAB', [-1, 0, 1, 2, -1, 4, 0, -1], 'ABAC'] * 8
    kw = dict(max_length=L, grammar=G, form=form, section_bars=2, attention_mask=mask, **STOP)
    two = fresh_generate(m, ids, **kw, **GREEDY)
    assert isinstance(m._decoder, XLDecoderLanes) and m._decoder.n == 2
    _assert_follows(two, Tp, form, 2, mask=mask)
    monkeypatch.setenv('MXL_DECODE_LANES', '1')
    one = fresh_generate(m, ids, **kw, **GREEDY)
    assert isinstance(m._decoder, XLDecoder) and torch.equal(one, two)
    monkeypatch.delenv('MXL_DECODE_LANES')
    two = fresh_generate(m, ids, seed=31, **kw, **TOP8)
    _assert_follows(two, Tp, form, 2, mask=mask)
    n_pad = (mask == 0).sum(1).to(torch.int32)
    for lo, seed in ((0, 31), (16, 31 + 7919)):
        lane = XLDecoder(m.engine, 16, L, seed=seed).generate(ids[lo:lo + 16], L, grammar=G, form=form[lo:lo + 16], section_bars=2,
                                                               n_pad=n_pad[lo:lo + 16], **STOP, **TOP8)
        W = min(lane.shape[1], two.shape[1])
        assert torch.equal(lane[:, :W], two[lo:lo + 16, :W]) and (lane[:, W:] == PAD).all() and (two[lo:lo + 16, W:] == PAD).all()
    m._decoder = None


# ---------------------------------------------------------------------------------------------------------------- what a form is
def test_a_form_without_repeats_is_the_bar_count_and_a_row_without_a_form_is_free(dev, model):
    m = model
    ids, _ = _prompts('header', dev)
    Tp = ids.shape[1]
    L = Tp + 6 * BAR_TOKENS + 1
    kw = dict(max_length=L, grammar=G, seed=5, **STOP, **TOP8)
    assert torch.equal(fresh_generate(m, ids, form='ABC', section_bars=2, **kw), fresh_generate(m, ids, n_bars=6, **kw))
    # a None row is that row of the same call without form=, with the other rows' bar counts
    some = ['AABA', None, 'AA', None]
    got = fresh_generate(m, ids, form=some, **kw)
    assert m._decoder.rules.nplan.tolist() == [4, 0, 2, 0] and m._decoder.gleft.tolist()[1::2] == [-1, -1]
    free = fresh_generate(m, ids, n_bars=[4, -1, 2, -1], **kw)
    W = min(got.shape[1], free.shape[1])
    assert torch.equal(got[[1, 3], :W], free[[1, 3], :W]) and not torch.equal(got[[0, 2], :W], free[[0, 2], :W])
    assert check_form(got, G, some, prompt_len=Tp).tolist() == [-1] * 4
    assert check_form(free, G, some, prompt_len=Tp)[[0, 2]].min() >= Tp                    # the model repeats nothing on its own
    _assert_follows(got[[0, 2]], Tp, ['AABA', 'AA'])


def test_melody_span_writes_a_new_bass_under_the_same_melody(dev, model):
    m = model
    ids, _ = _prompts('mid-bar', dev, times=2)
    Tp = ids.shape[1]
    L = Tp + 8 + 6 * BAR_TOKENS + 1
    reg = dict(register=REG, melody_range=(55, 96), bass_range=(28, 72), bass_below=1)
    out = fresh_generate(m, ids, max_length=L, grammar=G, form='ABABAA', form_span='melody', seed=3, **reg, **STOP, **TOP8)
    _assert_follows(out, Tp, 'ABABAA', span='melody')
    assert check_register(out, REG, prompt_len=Tp, **{k: v for k, v in reg.items() if k != 'register'}).tolist() == [-1] * 8
    plan = BarRepeat.plan_of('ABABAA')
    other = 0
    for row in out.tolist():
        bars = bars_of(row, G, Tp)
        other += sum(j >= 0 and bars[k] != bars[j] for k, j in enumerate(plan))
    assert other > 0                                               # the bass was chosen, not copied
    assert check_form(out, G, 'ABABAA', form_span='bar', prompt_len=Tp).max() >= Tp


def test_combinations(dev, model):
    m = model
    # num_return_sequences and in_key, on left-padded prompts of three lengths, one of which ends mid-bar
    ids, mask = _prompts('left-padded', dev)
    Tp = ids.shape[1]
    L = Tp + 8 + 4 * BAR_TOKENS + 1
    form = ['AABA', 'ABAB', [-1, 0, 0, 0], 'AAB']
    kw = dict(max_length=L, grammar=G, form=form, in_key=RULE, num_return_sequences=3, seed=7, attention_mask=mask, **STOP, **TOP8)
    out = fresh_generate(m, ids, **kw)
    rep = [f for f in form for _ in range(3)]
    assert out.shape[0] == 12
    _assert_follows(out, Tp, rep, mask=mask.repeat_interleave(3, 0))
    assert check_in_key(out, RULE, attention_mask=mask.repeat_interleave(3, 0)).tolist()[:9] == [-1] * 9       # (row 3 has no key)
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[3], out[4])
    # one set of prompt rings per prompt returns the same ids
    assert torch.equal(fresh_generate(m, ids, prompt_rings='shared', **kw), out)
    # a prompt longer than the K/V ring, and a form that runs on past the ring's next wrap
    long_ids = torch.tensor([token_ids(VOC, HEADER + ONE_BAR * 9)] * 2, device=dev)
    Tl = long_ids.shape[1]
    assert Tl > m.config.mem_len
    for kw in (GREEDY, dict(seed=9, **TOP8)):
        out = fresh_generate(m, long_ids, max_length=Tl + 10 * BAR_TOKENS + 1, grammar=G, form='AABAA', section_bars=2, **STOP, **kw)
        _assert_follows(out, Tl, 'AABAA', 2)                       # ten bars of seven tokens or more: past column 2 * mem_len
        assert (out[:, 2 * m.config.mem_len:] != PAD).any()
    # the same decoder and the same captured step serve another plan of the same width
    from symbolic_music_generation_amd.generate import XLDecoder
    ids, _ = _prompts('header', dev)
    L = ids.shape[1] + 4 * BAR_TOKENS + 1
    dec = XLDecoder(m.engine, 4, L, seed=4)
    a = dec.generate(ids, L, grammar=G, form='AABA', **STOP, **GREEDY)
    graph, table = dec.graph, dec.rules.plan.data_ptr()
    b = dec.generate(ids, L, grammar=G, form='ABAB', **STOP, **GREEDY)
    assert graph is not None and dec.graph is graph and dec.rules.plan.data_ptr() == table
    _assert_follows(a, ids.shape[1], 'AABA')
    _assert_follows(b, ids.shape[1], 'ABAB')
    assert torch.equal(b, XLDecoder(m.engine, 4, L, seed=4).generate(ids, L, grammar=G, form='ABAB', **STOP, **GREEDY))
    assert torch.equal(dec.generate(ids, L, grammar=G, n_bars=4, **STOP, **GREEDY)[:, :ids.shape[1]], ids) and dec.graph is not graph
    m._decoder = None


def test_reformer(dev):
    """fails without the feature: the Reformer refuses form= as an option it does not cover"""
    from symbolic_music_generation_amd.reformer import MyReformerConfig, MyReformerModelWithLMHead
    cfg = MyReformerConfig('debug-large', vocab_size=V, max_position_embeddings=512, axial_pos_shape=(16, 32),
                           attn_layers=['local'] * 4)
    rf = MyReformerModelWithLMHead(cfg, device=dev, seed=9).eval()
    with torch.no_grad():                                          # the head bias is read from the engine's fp32 parameters
        bias = rf.engine.p32('lm_head.bias')
        bias[torch.from_numpy(RULE.pcs != NO_PITCH).to(dev)] += 3.0
        bias[TUP] -= 30.0
        bias[D1] += 6.0
        bias[D2] += 6.0
    ids, _ = _prompts('header', dev)
    Tp, L = ids.shape[1], ids.shape[1] + 4 * BAR_TOKENS + 1
    for kw in (dict(do_sample=False), dict(seed=3, **TOP8)):
        rf._decoder = None
        got = rf.generate(input_ids=ids, max_length=L, grammar=G, form='AABA', **STOP, **kw)
        _assert_follows(got, Tp, 'AABA', varied=False)
    got = rf.generate(input_ids=ids[:2], max_length=Tp + 2 * BAR_TOKENS + 1, grammar=G, form='AA', use_cache=False, do_sample=False, **STOP)
    _assert_follows(got, Tp, 'AA')


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_through_generate(dev, model):
    from symbolic_music_generation_amd._lib import MusicXLError
    m = model
    ids, _ = _prompts('header', dev)
    call = lambda **kw: m.generate(input_ids=ids, **{**dict(max_length=40, grammar=G, form='AABA', **STOP), **kw})
    for kw in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(num_beams=2, do_sample=True),
               dict(penalty_alpha=0.6, top_k=4)):
        with pytest.raises(MusicXLError, match='form= is supported for greedy decoding and sampling only'):
            call(**kw)
    for kw, what in ((dict(grammar=subword_grammar(G, [[v] for v in range(V)])), 'needs a grammar with a repeat rule'),
                     (dict(grammar=None), 'needs grammar='), (dict(eos_token_id=None), 'explicit eos_token_id'),
                     (dict(n_bars=2), 'n_bars together with form'), (dict(min_length=30), 'min_length'),
                     (dict(melody=[1, 2, 3]), 'melody together with form'), (dict(section_bars=0), 'section_bars'),
                     (dict(form=''), 'empty form'), (dict(form=[-1, 3]), 'plan entry 1 is 3'),
                     (dict(form=['AA'] * 3), '3 entries for 4 prompts'), (dict(form_span='bass'), "form_span is 'bar'"),
                     (dict(form=None, section_bars=2), 'need form='), (dict(form=None, form_span='bar'), 'need form=')):
        with pytest.raises(ValueError, match=what):
            call(**kw)
