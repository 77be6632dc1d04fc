"""The register rule on the device (`generate(register=...)`; include/musicxl.h, "Rules of a generation", group `register`): the mask,
the prompt scan and one sampler tail -- fused and unfused -- element-wise against the host rule grammar.RegisterRule composed with the
other groups by tests/register_ref.py, then whole generations of models whose head bias favours pitches far outside a narrow range:
without the rule every constrained row leaves its register, with it none does -- alone and combined with the grammar, the bar budget,
the bar count, the key rule, the melody guide, eos, padded prompts, num_return_sequences, lanes, graph replay, the unfused tail, the
Reformer decoders and the four device searches.  The host side is tests/test_register_rule_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from symbolic_music_generation_amd.generate import (XLDecoder, XLDecoderLanes, bars_after_prompt, beam_search, check_bar_lengths,
                                                    check_grammar, check_in_key, check_melody, check_register, contrastive_search,
                                                    group_beam_search, left_pad, sampling_config)
from symbolic_music_generation_amd.grammar import MUSIC_GUIDE_CLASSES, NO_FLOOR, NO_KEY, NO_PITCH, MelodyGuide, RegisterRule
from symbolic_music_generation_amd.vocab import MusicTokenizer
from tests import register_ref, rules_ref
from tests.register_ref import EDGE_ROWS, RegWords, device_words
from tests.rules_ref import Rules, Words, fresh_generate, i32, token_ids

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK = MusicTokenizer(pitch_kind='degree')
VOC = TOK.vocab
V = len(VOC)                                                       # 1190: the fused sampler launch carries the rule
REG = TOK.register_rule()
KEY = TOK.key_rule()
G = TOK.grammar(bar_budget=True)
EOS, PAD, BAR, MEL, BASS, TUP, REST, D1, D2 = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<bar>', '<melody>', '<bass>', '<tup>', 'p_r', 'd_1', 'd_2'))
PITCHED = REG.reg <= 127
NB = len(EDGE_ROWS)                                                # 6 rows whose words differ
PROB_TOL = 1e-5          # tests/test_key_rule_gpu.py, the sampler's out_probs against the fp64 softmax of the masked, warped row
STOP = dict(eos_token_id=EOS, pad_token_id=PAD)
SAMPLE = dict(do_sample=True, temperature=1.0, top_k=0)


def _pitch(midi, degree=1):
    return VOC.t2i(f'p_{midi % 12 + 1}/{midi // 12 - 1}_{degree}')


def _tables(vocab_size):
    """the register rule, the key rule and the grammar (budget, count and guide) of the degree vocabulary, or all padded with further
    pitch tokens (MIDI number v % 128) to a vocabulary beyond the 2048 of the sorting samplers"""
    if vocab_size == V:
        return REG, KEY, G
    from tests.test_key_rule_gpu import _rule_and_grammar
    key, big = _rule_and_grammar(vocab_size)
    MelodyGuide(big, **MUSIC_GUIDE_CLASSES)
    return RegisterRule(np.concatenate([REG.reg, (np.arange(V, vocab_size) % 128).astype(np.uint8)])), key, big


# ---------------------------------------------------------------------------------------------------------------- 1. the mask
#          state     bar rem left key pos force
ALL_ON = [('B_D',    0,  0,  -1,  -1, 0, 0), ('M_OPEN', 32, 32, 2, 0, 0, 0), ('M_OPEN', 32, 32, -1, 7, 0, 0),
          ('B_D',    24, 8,  1,   12, 0, 0), ('B_OPEN', 32, 32, 3, 23, 0, 0), ('B_OPEN', 32, 32, 1, 0, 2, 1)]
GUIDE_ROW = [BAR, MEL, _pitch(100), D1, BASS]                      # row 5 is fed a pitch that its bounds bar


@pytest.mark.parametrize('vocab_size', [V, 2500])
def test_mask_equals_the_host_rule(dev, vocab_size):
    """mxl_ranged_rules_mask with the register group alone, then with every group on: the -inf set is exactly what the host rules
    bar, every other score keeps its bits; 2500 is past the vocabulary the sorting samplers take"""
    from symbolic_music_generation_amd import ops
    reg, key, g = _tables(vocab_size)
    torch.manual_seed(6)
    logp = torch.randn(NB, vocab_size + 3)

    def check(got, keep):
        got = got.cpu()
        assert torch.equal(torch.isinf(got[:, :vocab_size]) & (got[:, :vocab_size] < 0), ~keep)
        want = logp.clone()
        want[:, :vocab_size][~keep] = float('-inf')
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))                  # every other score: the same bits

    pitched = torch.from_numpy(reg.reg <= 127)
    for gap in (-1, 0, 1):
        full = logp.to(dev)
        grange, gpart, gfloor = device_words(EDGE_ROWS, dev)
        ops.rules_mask(full[:, :vocab_size], vocab_size, None, register=reg, grange=grange, gpart=gpart, gfloor=gfloor, gap=gap)
        keep = register_ref.keep_rows(Rules(None), [Words()] * NB, reg, EDGE_ROWS, gap, vocab_size)
        check(full, keep)
        assert (grange.tolist(), gpart.tolist(), gfloor.tolist()) == tuple(map(list, zip(*[(r.grange, r.gpart, r.gfloor) for r in EDGE_ROWS])))
        assert keep[:, ~pitched].all() and keep[1].all()           # no token that is no pitch is barred; no open part: untouched
        assert keep[0].all() == (gap < 0)                           # unconstrained bounds: only the gap bars
        assert keep[3][pitched].any() == (gap < 0)                  # the floor under lo_bass: no pitched token is left
        assert int(keep[4][pitched].sum()) == int((reg.reg == 40).sum())                   # lo == hi
        assert int(keep[5][pitched].sum()) == {-1: int(pitched.sum()), 0: int((reg.reg == 0).sum()), 1: 0}[gap]
    # every group on
    cols = list(zip(*[(g.state(s), bar, rem, left, k, pos, force) for s, bar, rem, left, k, pos, force in ALL_ON]))
    gstate, gbar, grem, gleft, gkey, gpos, gforce = (i32(c, dev) for c in cols)
    guide = torch.zeros(NB, 8, dtype=torch.int32, device=dev)
    guide[5, :5] = i32(GUIDE_ROW, dev)
    glen = i32([0] * 5 + [5], dev)
    host = [Words(1, *w) for w in zip(*cols)]
    rules = Rules(g, budget=True, count=True, key_rule=key, guide=True)
    guides = [None] * 5 + [GUIDE_ROW]
    others = rules_ref.keep_rows(rules, host, vocab_size, guides)
    both = register_ref.keep_rows(rules, host, reg, EDGE_ROWS, 1, vocab_size, guides)
    assert both.any(1).all() and both[5].tolist() == (torch.arange(vocab_size) == GUIDE_ROW[2]).tolist()     # the guide overrides
    assert all(int(both[i].sum()) < int(others[i].sum()) for i in (0, 2, 3, 4)) and torch.equal(both[1], others[1])
    full = logp.to(dev)
    grange, gpart, gfloor = device_words(EDGE_ROWS, dev)
    ops.rules_mask(full[:, :vocab_size], vocab_size, None, grammar=g, gstate=gstate, gbar=gbar, grem=grem, gleft=gleft, in_key=key,
                   gkey=gkey, melody=g.guide, guide=guide, glen=glen, gpos=gpos, gforce=gforce, register=reg, grange=grange,
                   gpart=gpart, gfloor=gfloor, gap=1)
    check(full, both)


# ---------------------------------------------------------------------------------------------------------------- 2. the scan
def test_scan_equals_the_host_walk(dev):
    """mxl_register_scan (the words after the prompts, and check_register on the device) against RegisterRule.walk: pads, ids beyond
    the vocabulary, `from` inside the row, start words, prompts that end mid-melody and mid-bass"""
    from symbolic_music_generation_amd import ops
    rng = np.random.default_rng(3)
    T, n = 150, 9
    pitch = np.flatnonzero(PITCHED)
    other = np.flatnonzero(REG.reg == NO_PITCH)
    rows = rng.choice(other, (n, T))
    for b in range(n):
        rows[b, rng.choice(T, 40, replace=False)] = rng.choice(pitch, 40)
        rows[b, rng.choice(T, 12, replace=False)] = rng.choice([BAR, MEL, BASS, MEL, BASS], 12)
        rows[b, :b] = -1
    rows[4, 70] = V + 9
    rows[2, T - 4:] = [BAR, MEL, _pitch(50), D1]                   # ends mid-melody, the floor set
    rows[3, T - 2:] = [BASS, D1]                                   # ends mid-bass
    ids = torch.from_numpy(rows).to(dev)
    bounds = [(0, 127, 0, 127), (60, 72, 36, 55), (0, 127, 0, 60), (48, 48, 48, 48), (0, 0, 127, 127), (30, 100, 20, 90),
              (60, 72, 36, 55), (0, 127, 0, 127), (64, 127, 0, 63)]
    grange = i32([RegWords(b).grange for b in bounds], dev)
    ends = set()
    for gap, part, floor, frm in ((-1, 0, NO_FLOOR, 0), (1, 0, NO_FLOOR, 0), (0, 2, 64, 0), (1, 1, 127, 64), (2, 0, NO_FLOOR, 97),
                                  (1, 0, NO_FLOOR, T)):
        gpart, gfloor, bad = i32([part] * n, dev), i32([floor] * n, dev), i32([0] * n, dev)
        ops.register_scan(ids, T, REG, grange, gpart, gfloor, bad, gap, check_from=frm)
        want = [REG.walk(r, b, gap, part, floor, frm) for r, b in zip(rows, bounds)]
        assert list(zip(gpart.tolist(), gfloor.tolist(), bad.tolist())) == want, (gap, part, floor, frm)
        ends |= {w[0] for w in want if w[2] < 0}
    assert all(w[2] == -1 for w in want) and want[2][:2] == (1, 50) and want[3][0] == 2    # from = T judges nothing
    assert {1, 2} <= ends
    kw = dict(melody_range=[b[:2] for b in bounds], bass_range=[b[2:] for b in bounds], bass_below=1)
    got = check_register(ids, REG, **kw, prompt_len=20)
    assert got.tolist() == check_register(ids.cpu(), REG, **kw, prompt_len=20).tolist() == [REG.walk(r, b, 1, check_from=20)[2]
                                                                                           for r, b in zip(rows, bounds)]
    assert (got >= 20).any() and check_register(ids, REG).tolist() == [-1] * n


# ---------------------------------------------------------------------------------------------------------------- 3. one sampler tail
def _tail(dev, fused, scores, sampling, rows, gap, grammar=None, gstate=None, unfinished=None):
    """one sampler tail over `scores` (B, V) at position 2 -> (tokens, out_probs, the register words after it)"""
    stop = None if unfinished is None else (EOS, PAD, 0)
    alive = None if unfinished is None else i32([0], dev)
    grange, gpart, gfloor = device_words(rows, dev)
    toks, probs, *_ = rules_ref.tail(dev, fused, scores.clone(), sampling, 2, width=64, seed=17, gen_seed=2, fill=0, stop=stop,
                                     unfinished=unfinished, alive=alive, grammar=grammar, gstate=gstate, register=REG, grange=grange,
                                     gpart=gpart, gfloor=gfloor, gap=gap)
    assert grange.tolist() == [r.grange for r in rows]             # the bounds are never written
    return toks, probs, list(zip(gpart.tolist(), gfloor.tolist()))


def _reference_probs(scores, keep, sampling):
    """fp64 softmax of the masked, warped rows (mask, temperature, top-k; HF's processor order)"""
    s = scores.double().cpu().masked_fill(~keep, float('-inf')) / sampling['temperature']
    if sampling['top_k']:
        kth = s.topk(sampling['top_k'], -1).values[:, -1:]
        s = s.masked_fill(s < kth, float('-inf'))
    return s.softmax(-1)


@pytest.mark.parametrize('with_grammar', [False, True], ids=['register-alone', 'register+grammar'])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
def test_sampler_probabilities_and_argmax(dev, fused, with_grammar):
    """the distribution the rows are drawn from is zero on barred tokens and the fp64 softmax of the masked, warped row elsewhere;
    greedy is the argmax over the allowed tokens -- through the one fused launch and through mask / sample / advance"""
    g = VOC.grammar() if with_grammar else None
    states = ['B_OPEN', 'M_OPEN', 'M_D', 'B_D', 'B_OPEN', 'B_D']      # states that allow a pitch
    words = [Words(gstate=0 if g is None else g.state(s)) for s in states]
    keep = register_ref.keep_rows(Rules(g), words, REG, EDGE_ROWS, 1, V)
    assert keep.any(1).all()
    gen = torch.Generator(device=dev).manual_seed(8)
    scores = 2.0 * torch.randn(NB, V, device=dev, generator=gen)
    for i in (0, 2, 3, 4, 5):                                       # the best score of every row the rule touches is a pitch it bars
        scores[i, int(np.flatnonzero(~REG.allowed(EDGE_ROWS[i].gpart, EDGE_ROWS[i].gfloor, EDGE_ROWS[i].bounds, 1))[7 * i])] += 8.0
    for kw in (dict(do_sample=True, top_k=0, temperature=1.3), dict(do_sample=True, top_k=40, temperature=0.8)):
        sampling = sampling_config(**kw)
        gstate = None if g is None else i32([w.gstate for w in words], dev)
        toks, probs, after = _tail(dev, fused, scores, sampling, EDGE_ROWS, 1, grammar=g, gstate=gstate)
        want = _reference_probs(scores, keep, sampling)
        err = (probs.double() - want).abs().max().item()
        print(f'fused={fused} grammar={with_grammar} {kw}: max |p - fp64| = {err:.3e}')
        assert (probs[~keep] == 0).all()
        assert ((probs > 0) == (want > 0)).all()
        assert err < PROB_TOL, kw
        assert (want.gather(1, toks[:, None]) > 0).all() and keep[torch.arange(NB), toks].all()
        assert after == [register_ref.move(Rules(g), w, REG, rw, t)[2][1:] for w, rw, t in zip(words, EDGE_ROWS, toks.tolist())]
    gstate = None if g is None else i32([w.gstate for w in words], dev)
    toks, _, _ = _tail(dev, fused, scores, sampling_config(do_sample=False), EDGE_ROWS, 1, grammar=g, gstate=gstate)
    want = scores.cpu().masked_fill(~keep, float('-inf')).argmax(-1)
    assert torch.equal(toks, want) and all(want[i] != scores[i].argmax().item() for i in (0, 2, 3, 4, 5))


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
def test_the_words_move_and_a_finished_row_keeps_them(dev, fused):
    """scores biased so that row 0 emits <melody>, row 1 <bass>, row 2 a melody pitch that lowers the floor, row 3 <bar>, which resets
    it, row 4 eos, which still moves; row 5 was finished before the step: it emits pad and keeps its words"""
    gen = torch.Generator(device=dev).manual_seed(9)
    scores = torch.randn(NB, V, device=dev, generator=gen)
    rows = list(EDGE_ROWS)
    rows[2] = rows[2]._replace(gfloor=70)
    low = _pitch(62, 3)
    for b, t in enumerate((MEL, BASS, low, BAR, EOS, BAR)):
        scores[b, t] += 100.0
    for sampling in (sampling_config(do_sample=False), sampling_config(**SAMPLE)):
        live = i32([1, 1, 1, 1, 1, 0], dev)
        toks, _, after = _tail(dev, fused, scores, sampling, rows, 1, unfinished=live)
        assert toks.tolist() == [MEL, BASS, low, BAR, EOS, PAD]
        rules = Rules(None, stop=(EOS, PAD, 0))
        want = [register_ref.move(rules, Words(unfinished=u), REG, rw, t)[2][1:]
                for u, rw, t in zip([1, 1, 1, 1, 1, 0], rows, [MEL, BASS, low, BAR, EOS, BAR])]
        assert after == want
        assert want == [(1, 60), (2, 50), (1, 62), (0, NO_FLOOR), (2, NO_FLOOR), (2, 0)]
        assert live.tolist() == [1, 1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 4. end to end
MELODY_RANGE, BASS_RANGE = (60, 72), (40, 55)
FAR = PITCHED & ((REG.reg > 84) | (REG.reg < 30))                  # outside both ranges by an octave: the models below favour them
HEADER = 'TimeSig_2/4 Tempo_120 Key_CMajor'
MID_MELODY = HEADER + ' <bar> <melody> p_1/5_1 d_1 p_5/4_3 d_1'    # the bar's lowest melody note is E4 = 64
MID_BASS = 'TimeSig_2/4 Tempo_120 <bar> <melody> p_1/3_1 d_2 <bass> p_r d_1'               # a low melody: C3 = 48
FULL_BAR = '<bar> <melody> p_r d_2 <bass> p_r d_2'                  # 2/4: the open bar is full
BAR_TOKENS = 3 + 2 * 16 + 2 * 16                                   # the longest bar of 16 slots without tuplets


def _model(dev, seed, closing_bias=0.0, long_notes=False, far_bias=6.0, max_length=256):
    """the test pair of tests/test_xl_model_gpu.py (debug size, V = 1190) with a head bias that favours pitches, and most of all
    those far outside MELODY_RANGE and BASS_RANGE: the argmax is such a pitch, and with those barred a pitch inside; key tokens and
    tuplets are biased away.  closing_bias: tests/test_grammar_generate_gpu.py's; long_notes: tests/test_melody_guide_gpu.py's"""
    from tests.test_xl_model_gpu import _pair
    ref, m = _pair(dev, n_layer=2, mem_len=64, seed=seed, max_length=max_length)
    with torch.no_grad():
        b = ref.crit.out_layers[0].bias
        b[torch.from_numpy(PITCHED)] += far_bias / 2
        b[torch.from_numpy(FAR)] += far_bias / 2
        b[torch.from_numpy(KEY.keys != NO_KEY)] -= 30.0
        b[TUP] -= 30.0
        if long_notes:
            b[D1] += 6.0
            b[D2] += 6.0
        if closing_bias:
            b[BASS] += closing_bias
            b[BAR] += closing_bias - 2.0
            b[EOS] += closing_bias
    m.load_state_dict(ref.state_dict())
    return m.eval()


def _prompts(n, dev):
    """n prompts of one width: mid-melody and, with a low melody, mid-bass, in turn"""
    rows = [token_ids(VOC, MID_BASS if i % 2 else MID_MELODY) for i in range(n)]
    assert len(set(map(len, rows))) == 1
    return torch.tensor(rows, dtype=torch.int64, device=dev)


def test_the_far_tokens_lie_outside_both_ranges():
    lo, hi = min(MELODY_RANGE[0], BASS_RANGE[0]), max(MELODY_RANGE[1], BASS_RANGE[1])
    assert FAR.sum() > 300 and not ((REG.reg[FAR] >= lo) & (REG.reg[FAR] <= hi)).any()


@pytest.mark.parametrize('kw', [SAMPLE, dict(do_sample=False)], ids=['sample', 'greedy'])
def test_rows_keep_their_register_only_with_the_rule(dev, kw):
    """fails without the feature: generate swallows register= and the ranges, and the rows leave their registers"""
    m = _model(dev, 700)
    n, N = 8, 60
    ids = _prompts(n, dev)
    Tp = ids.shape[1]
    # rows 3 and 7 are unconstrained; without bass_below they are untouched
    mel = [None if i % 4 == 3 else MELODY_RANGE for i in range(n)]
    bass = [None if i % 4 == 3 else BASS_RANGE for i in range(n)]
    con = torch.tensor([i % 4 != 3 for i in range(n)])
    free = fresh_generate(m, ids, max_new_tokens=N, seed=3, **kw)
    bad = check_register(free, REG, melody_range=mel, bass_range=bass, prompt_len=Tp)
    print('first column out of its register without the rule:', bad.tolist())
    assert (bad[con] >= Tp).all() and (bad[~con] == -1).all()       # the control: every constrained row leaves its register
    got = fresh_generate(m, ids, max_new_tokens=N, seed=3, register=REG, melody_range=mel, bass_range=bass, **kw)
    assert got.shape == (n, Tp + N) and torch.equal(got[:, :Tp], ids)
    assert check_register(got, REG, melody_range=mel, bass_range=bass, prompt_len=Tp).tolist() == [-1] * n
    assert check_register(got.cpu(), REG, melody_range=mel, bass_range=bass, prompt_len=Tp).tolist() == [-1] * n     # the host walk
    assert torch.equal(got[~con], free[~con]) and not torch.equal(got[con], free[con])     # unconstrained: untouched, token for token
    assert PITCHED[got[con][:, Tp:].cpu().numpy()].any(1).all()    # the constrained rows still hold pitches
    # bass_below: every row's bass stays under the lowest melody note of its bar, the unconstrained rows' too -- the prompts' low
    # melody (C3) is what bounds the rows that end mid-bass
    below = dict(melody_range=mel, bass_range=bass, bass_below=1)
    assert (check_register(free, REG, **below, prompt_len=Tp)[con] >= Tp).all()
    got2 = fresh_generate(m, ids, max_new_tokens=N, seed=3, register=REG, **below, **kw)
    assert check_register(got2, REG, **below, prompt_len=Tp).tolist() == check_register(got2.cpu(), REG, **below, prompt_len=Tp).tolist() == [-1] * n
    first = got2[1::2, Tp].cpu().numpy()                            # the rows that end mid-bass under C3 = 48: at most 47
    assert (REG.reg[first] > 127).all() or int(REG.reg[first][REG.reg[first] <= 127].max()) <= 47
    assert m._decoder.rules.gap == 1


# ---------------------------------------------------------------------------------------------------------------- 5. paths agree
def _combined(m, ids, n_bars=2, **kw):
    Tp = ids.shape[1]
    return fresh_generate(m, ids, max_length=Tp + 2 * BAR_TOKENS + 1, grammar=G, n_bars=n_bars, in_key=KEY, register=REG,
                          melody_range=MELODY_RANGE, bass_range=BASS_RANGE, bass_below=1, **STOP, **kw)


def _assert_all_rules_kept(out, Tp, n_bars=2, mask=None):
    n = out.shape[0]
    assert check_grammar(out, G, mask).tolist() == [-1] * n and check_bar_lengths(out, G, mask).tolist() == [-1] * n
    assert check_in_key(out, KEY, prompt_len=Tp, attention_mask=mask).tolist() == [-1] * n
    assert check_register(out, REG, MELODY_RANGE, BASS_RANGE, 1, prompt_len=Tp, attention_mask=mask).tolist() == [-1] * n
    assert bars_after_prompt(out, G, prompt_len=Tp).tolist() == [n_bars] * n
    assert ((out[:, Tp:] == EOS).sum(1) == 1).all()


def _bar_prompts(n, dev):
    return torch.tensor([token_ids(VOC, f'{HEADER} {FULL_BAR}')] * n, dtype=torch.int64, device=dev)


def _combined_runs(m, dev, use_graph=True):
    """sampled and greedy token matrices of the combined call (also what the child process of the unfused comparison computes)"""
    ids = _bar_prompts(6, dev)
    W = ids.shape[1] + 2 * BAR_TOKENS + 1
    outs = []
    for kw in (SAMPLE, dict(do_sample=False), dict(do_sample=True, top_k=8, repetition_penalty=1.2)):
        o = _combined(m, ids, seed=7, use_graph=use_graph, **kw)
        outs.append(torch.nn.functional.pad(o, (0, W - o.shape[1]), value=PAD))
    return torch.stack(outs)


def test_graph_eager_fused_and_unfused_agree(dev, tmp_path):
    """the register rule with the grammar, the budget, the count and the key: each row walks clean under every check and ends after
    its two bars; graph replay equals the eager loop, and the fused launch equals the unfused tail run in a fresh child process"""
    m = _model(dev, 701, closing_bias=4.0)
    ids = _bar_prompts(6, dev)
    Tp = ids.shape[1]
    assert XLDecoder(m.engine, 2, 32).fused_sampler
    fused = _combined_runs(m, dev)
    for o in fused:
        _assert_all_rules_kept(o, Tp)
    # the other rules alone leave the registers: the register rule is what keeps them
    free = fresh_generate(m, ids, max_length=Tp + 2 * BAR_TOKENS + 1, grammar=G, n_bars=2, in_key=KEY, seed=7, **STOP, **SAMPLE)
    assert (check_register(free, REG, MELODY_RANGE, BASS_RANGE, 1, prompt_len=Tp) >= Tp).all()
    assert torch.equal(_combined_runs(m, dev, use_graph=False), fused)
    out = tmp_path / 'unfused.pt'
    code = ('import sys, torch\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'from tests import test_register_rule_gpu as t\n'
            'from symbolic_music_generation_amd.generate import XLDecoder\n'
            'dev = torch.device("cuda:0")\n'
            'm = t._model(dev, 701, closing_bias=4.0)\n'
            'assert not XLDecoder(m.engine, 2, 32).fused_sampler\n'
            f'torch.save(t._combined_runs(m, dev).cpu(), {str(out)!r})\n')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MXL_DECODE_UNFUSED='1'), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert torch.equal(torch.load(out), fused.cpu())


def test_two_lanes_equal_their_decoders(dev):
    """32 rows on two lanes: each lane's rows equal one decoder of its own over them, with per-row bounds"""
    m = _model(dev, 702)
    n, N = 32, 40
    ids = _prompts(n, dev)
    Tp = ids.shape[1]
    L = Tp + N
    mel = [None if i % 4 == 3 else (60 + i % 5, 72) for i in range(n)]
    bass = [None if i % 4 == 3 else (40, 50 + i % 7) for i in range(n)]
    for kw in (SAMPLE, dict(do_sample=False)):
        lanes = XLDecoderLanes(m.engine, n, L, seed=11, lanes=2)
        rk = dict(register=REG, melody_range=mel, bass_range=bass, bass_below=0)
        out = lanes.generate(ids, L, **rk, **kw)
        assert check_register(out, REG, mel, bass, 0, prompt_len=Tp).tolist() == [-1] * n
        for i in range(2):
            rows = slice(lanes.offs[i], lanes.offs[i + 1])
            one = XLDecoder(m.engine, lanes.sizes[i], L, seed=11 + 7919 * i).generate(
                ids[rows], L, register=REG, melody_range=mel[rows], bass_range=bass[rows], bass_below=0, **kw)
            assert torch.equal(out[rows], one), (kw, i)
    # generate takes the lanes from 32 rows on, and they answer like the single decoder
    two = fresh_generate(m, ids, max_length=L, seed=5, **rk, **SAMPLE)
    assert isinstance(m._decoder, XLDecoderLanes) and check_register(two, REG, mel, bass, 0, prompt_len=Tp).tolist() == [-1] * n


def test_graph_key_covers_the_rule(dev):
    """one decoder: rule -> none -> other bounds -> another gap -> a rule with another table -> the first, each equal to a fresh
    decoder's result"""
    m = _model(dev, 704)
    n, L = 4, 60
    ids = _prompts(n, dev)
    Tp = ids.shape[1]
    other = RegisterRule(np.where(PITCHED, 127 - REG.reg, REG.reg))
    kw = dict(do_sample=True, top_k=8)
    dec = XLDecoder(m.engine, n, L, seed=4)

    def again(**k):
        dec.rng.zero_()
        return dec.generate(ids, L, **kw, **k)

    def fresh(**k):
        return XLDecoder(m.engine, n, L, seed=4).generate(ids, L, **kw, **k)

    first = dict(register=REG, melody_range=MELODY_RANGE, bass_range=BASS_RANGE)
    a = again(**first)
    assert torch.equal(a, fresh(**first)) and check_register(a, REG, MELODY_RANGE, BASS_RANGE, prompt_len=Tp).tolist() == [-1] * n
    b = again()
    assert torch.equal(b, fresh()) and not torch.equal(a, b)
    wide = dict(register=REG, melody_range=[(48, 60), None, (70, 70), (0, 127)], bass_range=(30, 40))      # bounds are step state
    c = again(**wide)
    assert torch.equal(c, fresh(**wide)) and not torch.equal(c, a)
    assert check_register(c, REG, wide['melody_range'], wide['bass_range'], prompt_len=Tp).tolist() == [-1] * n
    d = again(**first, bass_below=3)                                # the gap rides on the captured launch
    assert torch.equal(d, fresh(**first, bass_below=3)) and not torch.equal(d, a)
    assert check_register(d, REG, MELODY_RANGE, BASS_RANGE, 3, prompt_len=Tp).tolist() == [-1] * n
    e = again(**dict(first, register=other))
    assert torch.equal(e, fresh(**dict(first, register=other))) and not torch.equal(e, a)
    assert check_register(e, other, MELODY_RANGE, BASS_RANGE, prompt_len=Tp).tolist() == [-1] * n
    assert torch.equal(again(**first), a)


# ---------------------------------------------------------------------------------------------------------------- 6. every rule at once
def _guides():
    """guides of two and three bars of 2/4 whose melodies sit in different places; the first holds a note outside MELODY_RANGE and a
    C sharp, which C major bars: guide notes are not judged"""
    a0 = [BAR, MEL, _pitch(72), D1, _pitch(64, 3), D1, BASS]
    a1 = [BAR, MEL, _pitch(90, 5), D1, _pitch(61), D1, BASS]
    a2 = [BAR, MEL, _pitch(55, 5), D2, BASS]
    a3 = [BAR, MEL, REST, D2, BASS]                                # no melody note: the bar has no floor
    return [a0 + a1, a2 + a0 + a3, a1 + a2, a3 + a0]


def test_every_rule_at_once(dev):
    """grammar(bar_budget=True), in_key, melody=, bass_below=1 and the ranges together: every check returns -1, each row ends after its
    guided bars, and the bass of each bar lies under that bar's guided melody"""
    m = _model(dev, 705, long_notes=True)
    guides = _guides()
    n_bars = [2, 3, 2, 2]
    ids = torch.tensor([token_ids(VOC, HEADER)] * 4, device=dev)
    Tp = ids.shape[1]
    L = Tp + 3 * (7 + 2 * 16) + 1
    rk = dict(melody_range=MELODY_RANGE, bass_range=BASS_RANGE, bass_below=1)
    for kw in (dict(do_sample=False), SAMPLE):
        out = fresh_generate(m, ids, max_length=L, grammar=G, in_key=KEY, melody=guides, register=REG, seed=3, **rk, **STOP, **kw)
        assert check_grammar(out, G).tolist() == check_bar_lengths(out, G).tolist() == [-1] * 4
        assert check_melody(out, G, guides, prompt_len=Tp).tolist() == [-1] * 4
        assert bars_after_prompt(out, G, prompt_len=Tp).tolist() == n_bars and ((out[:, Tp:] == EOS).sum(1) == 1).all()
        gen = out[:, Tp:].cpu()
        notes = 0
        for b in range(4):
            row = gen[b].tolist()
            row = row[:row.index(EOS)]
            assert row.count(BAR) == n_bars[b]
            at = [i for i, t in enumerate(row) if t == BAR] + [len(row)]
            for lo, hi in zip(at, at[1:]):                          # bar by bar, by hand: the bass against the guided melody
                bar = row[lo:hi]
                split = bar.index(BASS)
                melody = [int(REG.reg[t]) for t in bar[:split] if REG.reg[t] <= 127]
                bass = [int(REG.reg[t]) for t in bar[split:] if REG.reg[t] <= 127]
                top = min(BASS_RANGE[1], min(melody) - 1) if melody else BASS_RANGE[1]
                assert all(BASS_RANGE[0] <= p <= top for p in bass), (b, bar)
                assert all(KEY.allows(0, t) for t in bar[split:])  # the bass is in C major; the guide's C sharp stands
                notes += len(bass)
        assert notes > 0
        # guided notes outside the melody range are not judged by generate: the rule's own check finds them, and nothing in the bass
        bad = check_register(out, REG, **rk, prompt_len=Tp).tolist()
        assert bad[1] == bad[2] == Tp + 2 and bad[3] == -1 and int(out[0, bad[0]]) == _pitch(90, 5)
        assert check_register(out, REG, None, BASS_RANGE, 1, prompt_len=Tp).tolist() == [-1] * 4
    # without the register rule the bass crosses the melody
    free = fresh_generate(m, ids, max_length=L, grammar=G, in_key=KEY, melody=guides, seed=3, **STOP, **SAMPLE)
    assert (check_register(free, REG, None, BASS_RANGE, 1, prompt_len=Tp) >= Tp).all()


# ---------------------------------------------------------------------------------------------------------------- 7. combinations
def test_left_padded_prompts_and_num_return_sequences(dev):
    m = _model(dev, 706, closing_bias=4.0)
    texts = [f'{HEADER} {FULL_BAR}', f'{HEADER} {FULL_BAR} <bar> <melody> p_1/4_1 d_2 <bass> p_r d_1', MID_BASS + ' p_r d_1',
             f'TimeSig_2/4 Tempo_120 {FULL_BAR}']
    prompts = [torch.tensor(token_ids(VOC, t)) for t in texts]
    ids, mask = left_pad(prompts, PAD)
    ids, mask = ids.to(dev), mask.to(dev)
    Tp = ids.shape[1]
    L = Tp + 2 * BAR_TOKENS + 1
    mel, bass = [MELODY_RANGE, (62, 70), None, MELODY_RANGE], [BASS_RANGE, None, (36, 50), BASS_RANGE]
    rk = dict(register=REG, melody_range=mel, bass_range=bass, bass_below=1)
    out = fresh_generate(m, ids, attention_mask=mask, max_length=L, grammar=G, n_bars=2, do_sample=False, **rk, **STOP)
    assert check_grammar(out, G, mask).tolist() == check_bar_lengths(out, G, mask).tolist() == [-1] * 4
    assert check_register(out, REG, mel, bass, 1, prompt_len=Tp, attention_mask=mask).tolist() == [-1] * 4
    for b, p in enumerate(prompts):                                 # every row as if it were alone: the pads are skipped
        s = Tp - len(p)
        one = fresh_generate(m, p[None].to(dev), max_length=L - s, grammar=G, n_bars=2, do_sample=False, register=REG,
                             melody_range=mel[b], bass_range=bass[b], bass_below=1, **STOP)[0]
        W = min(one.shape[0], out.shape[1] - s)
        assert torch.equal(out[b, s:s + W], one[:W]) and (out[b, s + W:] == PAD).all() and (one[W:] == PAD).all(), b
    # num_return_sequences repeats the bounds per prompt
    two = _prompts(2, dev)
    out = fresh_generate(m, two, max_new_tokens=40, register=REG, melody_range=[(60, 62), None], bass_range=[None, (41, 43)],
                         num_return_sequences=2, **SAMPLE)
    assert out.shape[0] == 4 and torch.equal(out[:, :two.shape[1]], two.repeat_interleave(2, 0))
    assert m._decoder.grange.tolist() == [RegWords((60, 62, 0, 127)).grange] * 2 + [RegWords((0, 127, 41, 43)).grange] * 2
    assert check_register(out, REG, [(60, 62)] * 2 + [None] * 2, [None] * 2 + [(41, 43)] * 2, prompt_len=two.shape[1]).tolist() == [-1] * 4
    assert not torch.equal(out[0], out[1])


def test_reformer(dev):
    """the Reformer decoders take the rule through mask / advance: cached and uncached, greedy and sampling"""
    from symbolic_music_generation_amd._lib import MusicXLError
    from symbolic_music_generation_amd.reformer import MyReformerConfig, MyReformerModelWithLMHead
    cfg = MyReformerConfig('debug-large', vocab_size=V, max_position_embeddings=512, axial_pos_shape=(16, 32),
                           attn_layers=['local'] * 4)
    rf = MyReformerModelWithLMHead(cfg, device=dev, seed=9).eval()
    with torch.no_grad():                                          # the head bias is read from the engine's fp32 parameters
        bias = rf.engine.p32('lm_head.bias')
        bias[torch.from_numpy(PITCHED).to(dev)] += 3.0
        bias[torch.from_numpy(FAR).to(dev)] += 3.0
    ids = _prompts(4, dev)
    Tp, L = ids.shape[1], 60
    rk = dict(melody_range=[MELODY_RANGE, None, MELODY_RANGE, (0, 127)], bass_range=BASS_RANGE, bass_below=1)
    for kw in (dict(do_sample=False), SAMPLE):
        rf._decoder = None
        free = rf.generate(input_ids=ids, max_length=L, **kw)
        assert (check_register(free, REG, **rk, prompt_len=Tp) >= Tp).all()
        rf._decoder = None
        got = rf.generate(input_ids=ids, max_length=L, register=REG, **rk, **kw)
        assert got.shape == (4, L) and check_register(got, REG, **rk, prompt_len=Tp).tolist() == [-1] * 4
    got = rf.generate(input_ids=ids, max_length=Tp + 16, register=REG, **rk, use_cache=False, **SAMPLE)
    assert check_register(got, REG, **rk, prompt_len=Tp).tolist() == [-1] * 4
    for bad in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(penalty_alpha=0.6)):
        with pytest.raises(MusicXLError, match='register= is supported'):
            rf.generate(input_ids=ids, max_length=20, register=REG, **bad)


def _bounds(n, per):
    return [MELODY_RANGE + BASS_RANGE] * (n * per)


def _bodies_clean(got, ids, per, g):
    """every returned row: its prompt, then a continuation that the rules accept up to and including its eos; the prompts end inside
    a bar, so under the grammar's budget every row has to write notes before it may end -- the rows do hold pitches"""
    Tp = ids.shape[1]
    assert torch.equal(got[:, :Tp], ids.repeat_interleave(per, 0))
    pitches = 0
    for row in got.tolist():
        t = torch.tensor(row[:(row.index(EOS) + 1) if EOS in row else len(row)])
        assert check_register(t, REG, MELODY_RANGE, BASS_RANGE, 1, prompt_len=Tp).tolist() == [-1]
        if g is not None:
            assert check_grammar(t, g).tolist() == [-1]
        pitches += int(PITCHED[t[Tp:].numpy()].sum())
    assert pitches > 0


@pytest.mark.parametrize('grammar', [False, True], ids=['register-alone', 'register+grammar'])
def test_beam_search_on_the_device_equals_the_masked_host_path(dev, grammar):
    m = _model(dev, 710 + grammar, closing_bias=4.0)
    ids = _prompts(3, dev)
    g = G if grammar else None
    Tp, W = ids.shape[1], ids.shape[1] + 30
    kw = dict(num_beams=3, early_stopping=True, num_return_sequences=2, **STOP)
    rk = dict(melody_range=MELODY_RANGE, bass_range=BASS_RANGE, bass_below=1)
    free = m.generate(input_ids=ids, max_length=W, grammar=g, **kw)
    assert (check_register(free, REG, **rk, prompt_len=Tp) >= Tp).any()
    got = m.generate(input_ids=ids, max_length=W, grammar=g, register=REG, **rk, **kw)
    want = beam_search(XLDecoder(m.engine, 9, W), ids, W, allowed=register_ref.host_allowed(g, REG, _bounds(3, 3), 1, Tp), **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    _bodies_clean(got, ids, 2, g)


def test_group_beam_search_on_the_device_equals_the_masked_host_path(dev):
    m = _model(dev, 712, closing_bias=4.0)
    ids = _prompts(3, dev)
    Tp, W = ids.shape[1], ids.shape[1] + 30
    kw = dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5, early_stopping=True, num_return_sequences=1, **STOP)
    rk = dict(melody_range=MELODY_RANGE, bass_range=BASS_RANGE, bass_below=1)
    got = m.generate(input_ids=ids, max_length=W, grammar=G, register=REG, **rk, **kw)
    want = group_beam_search(XLDecoder(m.engine, 12, W), ids, W, allowed=register_ref.host_allowed(G, REG, _bounds(3, 4), 1, Tp), **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    _bodies_clean(got, ids, 1, G)
    # the rule alone takes the device path too; without the closing bias the rows write notes to the end
    alone = _model(dev, 716).generate(input_ids=ids, max_length=W, register=REG, **rk, **kw)
    _bodies_clean(alone, ids, 1, None)


def test_contrastive_search_on_the_device_equals_the_masked_host_path(dev):
    m = _model(dev, 713, closing_bias=4.0)
    ids = _prompts(3, dev)
    Tp, W = ids.shape[1], ids.shape[1] + 40
    kw = dict(top_k=4, penalty_alpha=0.6, **STOP)
    rk = dict(melody_range=MELODY_RANGE, bass_range=BASS_RANGE, bass_below=1)
    got = m.generate(input_ids=ids, max_length=W, grammar=G, register=REG, **rk, **kw)
    want = contrastive_search(XLDecoder(m.engine, 12, W), ids, W, allowed=register_ref.host_allowed(G, REG, _bounds(3, 4), 1, Tp), **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    _bodies_clean(got, ids, 1, G)
    free = m.generate(input_ids=ids, max_length=W, grammar=G, **kw)
    assert (check_register(free, REG, **rk, prompt_len=Tp) >= Tp).any()


def test_beam_sample_on_the_device_keeps_the_rule(dev):
    m = _model(dev, 714, closing_bias=4.0)
    ids = _prompts(3, dev)
    Tp, W = ids.shape[1], ids.shape[1] + 40
    kw = dict(input_ids=ids, max_length=W, num_beams=3, do_sample=True, renormalize_logits=True, early_stopping=True, top_k=0,
              device_scorer=True, num_return_sequences=2, seed=9, **STOP)
    rk = dict(register=REG, melody_range=MELODY_RANGE, bass_range=BASS_RANGE, bass_below=1)
    got = m.generate(grammar=G, **rk, **kw)
    _bodies_clean(got, ids, 2, G)
    assert torch.equal(m.generate(grammar=G, use_graph=False, **rk, **kw), got)
    free = m.generate(grammar=G, **kw)
    assert (check_register(free, REG, MELODY_RANGE, BASS_RANGE, 1, prompt_len=Tp) >= Tp).any()


def test_refusals(dev, monkeypatch):
    from symbolic_music_generation_amd import ops
    from symbolic_music_generation_amd._lib import MusicXLError
    m = _model(dev, 715)
    ids = _prompts(2, dev)
    only = 'register= is supported for greedy decoding and sampling only'
    # the searches without an explicit eos, beam-sample on the host, and the host switches
    for kw in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(penalty_alpha=0.6, top_k=4),
               dict(num_beams=2, do_sample=True, **STOP), dict(penalty_alpha=0.6, top_k=40, **STOP)):
        with pytest.raises(MusicXLError, match=only):
            m.generate(input_ids=ids, max_length=20, register=REG, **kw)
    monkeypatch.setenv('MXL_BEAM_HOST', '1')
    with pytest.raises(MusicXLError, match=only):
        m.generate(input_ids=ids, max_length=20, register=REG, num_beams=2, **STOP)
    monkeypatch.delenv('MXL_BEAM_HOST')
    with pytest.raises(MusicXLError, match='spans 422 tokens'):                            # a rule over another vocabulary
        m.generate(input_ids=ids, max_length=20, register=MusicTokenizer(pitch_kind='midi').register_rule())
    with pytest.raises(ValueError, match='3 entries for 2 prompts'):
        m.generate(input_ids=ids, max_length=20, register=REG, melody_range=[(1, 2)] * 3)
    with pytest.raises(ValueError, match='above hi'):
        m.generate(input_ids=ids, max_length=20, register=REG, bass_range=(50, 40))
    with pytest.raises(ValueError, match='bass_below= needs register='):
        m.generate(input_ids=ids, max_length=20, bass_below=1)
    with pytest.raises(ValueError, match='melody_range= needs register='):
        m.generate(input_ids=ids, max_length=20, melody_range=(60, 72))
    z = i32([0, 0], dev)
    with pytest.raises(MusicXLError, match='spans'):
        ops.rules_mask(torch.zeros(2, 64, device=dev), 64, None, register=REG, grange=z, gpart=z, gfloor=z)
    with pytest.raises(MusicXLError, match='gpart must be'):
        ops.rules_mask(torch.zeros(2, V, device=dev), V, None, register=REG, grange=z, gpart=i32([0, 1, 2], dev), gfloor=z)
    with pytest.raises(MusicXLError, match='gap must lie'):
        ops.rules_mask(torch.zeros(2, V, device=dev), V, None, register=REG, grange=z, gpart=z, gfloor=z, gap=200)
    with pytest.raises(MusicXLError, match='needs register'):
        ops.rules_mask(torch.zeros(2, V, device=dev), V, None, grange=z, gpart=z, gfloor=z)
