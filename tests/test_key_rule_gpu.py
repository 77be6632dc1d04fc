"""The key rule on the device (`generate(in_key=...)`; include/musicxl.h, "Rules of a generation", group `key`): the mask and the
move of the unfused pair and of the fused sampler launch element-wise against the host rule grammar.KeyRule, then whole generations
of models whose head bias favours off-key pitches -- without the rule every row leaves its key at once, with it none does and the
in-key ratio of the generated part is exactly 1 -- alone and combined with the grammar, the bar budget, the bar count, eos, padded
prompts, num_return_sequences, lanes, graph replay and the unfused tail.  The host side is tests/test_key_rule_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from symbolic_music_generation_amd.generate import (bars_after_prompt, check_bar_lengths, check_grammar, check_in_key, left_pad,
                                                    sampling_config)
from symbolic_music_generation_amd.grammar import (MUSIC_BAR_COUNT_CLASSES, NO_KEY, NO_PITCH, BarBudget, BarCount, KeyRule,
                                                   TokenGrammar, key_ordinal, music_budget_tables)
from symbolic_music_generation_amd.vocab import MusicTokenizer
from tests import rules_ref
from tests.rules_ref import Rules, Words, fresh_generate, i32, keep_rows, move, token_ids

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK = MusicTokenizer(pitch_kind='degree')
VOC = TOK.vocab
V = len(VOC)                                                       # 1190: the fused sampler launch carries the rule
RULE = TOK.key_rule()
EOS, PAD, BAR = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<bar>'))
KEYS5 = [-1, 0, 7, 12, 23]
# pitch classes outside C major, A minor and G major alike: the models below favour them
OFF = (1, 3, 8, 10)
PROMPT_KEYS = ('CMajor', 'AMinor', 'GMajor')
SAMPLE = dict(do_sample=True, temperature=1.0, top_k=0)
PROB_TOL = 1e-5          # tests/test_decode_gpu.py::test_sampler_distribution, the sampler's out_probs against a softmax reference


def _rule_and_grammar(vocab_size):
    """the key rule and the grammar (with bar budget and bar count) of the degree vocabulary, or both padded with further pitch
    tokens (pitch class v % 12) to a vocabulary beyond the 2048 of the sorting samplers"""
    g = VOC.grammar(bar_budget=True)
    if vocab_size == V:
        return RULE, g
    n = vocab_size - V
    rule = KeyRule(np.concatenate([RULE.keys, np.full(n, NO_KEY, dtype=np.uint8)]),
                   np.concatenate([RULE.pcs, (np.arange(V, vocab_size) % 12).astype(np.uint8)]))
    t = music_budget_tables(VOC)
    cls = np.concatenate([g.cls, np.full(n, g.class_names.index('pitch'), dtype=np.uint8)])
    big = TokenGrammar(cls, g.allow, g.next, g.start, g.accepting, g.class_names, g.state_names)
    BarBudget(big, np.concatenate([t['slots'], np.zeros(n, dtype=np.uint16)]),
              np.concatenate([t['bars'], np.full(n, 0xFFFF, dtype=np.uint16)]), t['opens'], t['need_free'], t['need_full'])
    BarCount(big, **MUSIC_BAR_COUNT_CLASSES)
    return rule, big


# ---------------------------------------------------------------------------------------------------------------- 4. the mask
#        state     bar rem left
ROWS = [('M_OPEN', 32, 32, -1), ('M_OPEN', 32, 32, 2), ('B_D', 0, 0, -1), ('B_D', 24, 0, 0), ('M_T1', 32, 8, 3)]


@pytest.mark.parametrize('vocab_size', [V, 2500])
def test_mask_equals_the_host_rule(dev, vocab_size):
    """mxl_keyed_rules_mask with the key group alone, then with the grammar, its budget and its count on as well: the -inf set is
    exactly what the host rules bar, every other score keeps its bits; 2500 is past the vocabulary the sorting samplers take"""
    from symbolic_music_generation_amd import ops
    rule, g = _rule_and_grammar(vocab_size)
    torch.manual_seed(6)
    logp = torch.randn(5, vocab_size + 3)
    full = logp.to(dev)
    gkey = i32(KEYS5, dev)
    ops.rules_mask(full[:, :vocab_size], vocab_size, None, in_key=rule, gkey=gkey)         # a row stride that is not V
    keep = keep_rows(Rules(key_rule=rule), [Words(gkey=k) for k in KEYS5], vocab_size)
    assert keep[0].all() and all(0 < int((~keep[i]).sum()) < int((rule.pcs != NO_PITCH).sum()) for i in range(1, 5))

    def check(got, keep):
        got = got.cpu()
        assert torch.equal(torch.isinf(got[:, :vocab_size]) & (got[:, :vocab_size] < 0), ~keep)
        want = logp.clone()
        want[:, :vocab_size][~keep] = float('-inf')
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))                  # every other score: the same bits

    check(full, keep)
    assert gkey.tolist() == KEYS5                                  # the mask reads the words only
    rows = ROWS
    words = [i32(col, dev) for col in zip(*[(g.state(s), bar, rem, left) for s, bar, rem, left in rows])]
    host = [Words(gstate=g.state(s), gbar=bar, grem=rem, gleft=left, gkey=k) for (s, bar, rem, left), k in zip(rows, KEYS5)]
    four = keep_rows(Rules(g, budget=True, count=True), host, vocab_size)
    both = keep_rows(Rules(g, budget=True, count=True, key_rule=rule), host, vocab_size)
    assert torch.equal(both, four & keep)
    assert all(int(both[i].sum()) < int(four[i].sum()) for i in (1, 2, 4)) and both.any(1).all()     # the key bars more; no dead end
    full = logp.to(dev)
    ops.rules_mask(full[:, :vocab_size], vocab_size, None, grammar=g, gstate=words[0], gbar=words[1], grem=words[2], gleft=words[3],
                   in_key=rule, gkey=gkey)
    check(full, both)


def test_scan_equals_the_host_walk(dev):
    """mxl_key_scan (the prompts' keys, and check_in_key on the device) against KeyRule.walk: pads, ids beyond the vocabulary,
    start keys, columns that only move the key"""
    from symbolic_music_generation_amd import ops
    rng = np.random.default_rng(3)
    T, n = 150, 9
    pitch = np.flatnonzero(RULE.pcs != NO_PITCH)
    keyt = np.flatnonzero(RULE.keys != NO_KEY)
    rows = rng.choice(np.flatnonzero((RULE.pcs == NO_PITCH) & (RULE.keys == NO_KEY)), (n, T))
    for b in range(n):
        rows[b, rng.choice(T, 30, replace=False)] = rng.choice(pitch, 30)
        rows[b, rng.choice(T, b % 4, replace=False)] = rng.choice(keyt, b % 4)
        rows[b, :b] = -1
    rows[4, 70] = V + 9
    ids = torch.from_numpy(rows).to(dev)
    for start, frm in (([-1] * n, 0), ([b % 24 for b in range(n)], 0), ([5] * n, 64), ([-1, 3, 9] * 3, T)):
        gkey, bad = i32(start, dev), i32([0] * n, dev)
        ops.key_scan(ids, T, RULE, gkey, bad, check_from=frm)
        want = [RULE.walk(r, k, frm) for r, k in zip(rows, start)]
        assert list(zip(gkey.tolist(), bad.tolist())) == want, (start, frm)
    assert any(c >= 0 for _, c in want) is False and any(k >= 0 for k, _ in want)          # from = T judges nothing
    assert check_in_key(ids, RULE).tolist() == check_in_key(ids.cpu(), RULE).tolist() == [RULE.walk(r)[1] for r in rows]


# ---------------------------------------------------------------------------------------------------------------- 5. the samplers
def _tail(dev, fused, scores, sampling, gkey, rule=RULE, grammar=None, gstate=None, unfinished=None):
    """one sampler tail over `scores` (B, V) at position 2 -> (tokens, out_probs); fused: the one launch, else mask / sample /
    advance.  The words given move in place."""
    stop = None if unfinished is None else (EOS, PAD, 0)
    alive = None if unfinished is None else i32([0], dev)
    toks, probs, *_ = rules_ref.tail(dev, fused, scores.clone(), sampling, 2, width=64, seed=17, gen_seed=2, fill=0, stop=stop,
                                     unfinished=unfinished, alive=alive, grammar=grammar, gstate=gstate, in_key=rule, gkey=gkey)
    return toks, probs


def _reference_probs(scores, keep, sampling):
    """fp64 softmax of the masked, warped rows (mask, temperature, top-k; HF's processor order)"""
    s = scores.double().cpu().masked_fill(~keep, float('-inf')) / sampling['temperature']
    if sampling['top_k']:
        kth = s.topk(sampling['top_k'], -1).values[:, -1:]
        s = s.masked_fill(s < kth, float('-inf'))
    return s.softmax(-1)


@pytest.mark.parametrize('with_grammar', [False, True], ids=['key-alone', 'key+grammar'])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
def test_sampler_probabilities_and_argmax(dev, fused, with_grammar):
    """the distribution the rows are drawn from is zero on barred tokens and the fp64 softmax of the masked, warped row elsewhere;
    greedy is the argmax over the allowed tokens -- through the one fused launch and through mask / sample / advance"""
    g = VOC.grammar() if with_grammar else None
    states = ['M_OPEN', 'B_D', 'M_T1', 'M_D', 'B_OPEN']             # states that allow a pitch
    keep = keep_rows(Rules(g, key_rule=RULE), [Words(gstate=0 if g is None else g.state(s), gkey=k) for s, k in zip(states, KEYS5)], V)
    assert keep.any(1).all()
    gen = torch.Generator(device=dev).manual_seed(8)
    scores = 2.0 * torch.randn(5, V, device=dev, generator=gen)
    for i, k in enumerate(KEYS5[1:], 1):                           # the best score of every row that has a key is a pitch outside it
        scores[i, int(np.flatnonzero(~RULE.allowed(k))[i])] += 8.0
    for kw in (dict(do_sample=True, top_k=0, temperature=1.3), dict(do_sample=True, top_k=40, temperature=0.8)):
        sampling = sampling_config(**kw)
        gkey = i32(KEYS5, dev)
        gstate = None if g is None else i32([g.state(s) for s in states], dev)
        toks, probs = _tail(dev, fused, scores, sampling, gkey, grammar=g, gstate=gstate)
        want = _reference_probs(scores, keep, sampling)
        err = (probs.double() - want).abs().max().item()
        print(f'fused={fused} grammar={with_grammar} {kw}: max |p - fp64| = {err:.3e}')
        assert (probs[~keep] == 0).all()
        assert ((probs > 0) == (want > 0)).all()
        assert err < PROB_TOL, kw
        assert (want.gather(1, toks[:, None]) > 0).all() and keep[torch.arange(5), toks].all()
        assert gkey.tolist() == KEYS5                              # no key token was drawn here: the keys stand
    gkey = i32(KEYS5, dev)
    gstate = None if g is None else i32([g.state(s) for s in states], dev)
    toks, _ = _tail(dev, fused, scores, sampling_config(do_sample=False), gkey, grammar=g, gstate=gstate)
    want = scores.cpu().masked_fill(~keep, float('-inf')).argmax(-1)
    assert torch.equal(toks, want) and (want[1:] != scores.cpu().argmax(-1)[1:]).all()


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
def test_a_key_token_moves_the_key_and_a_finished_row_keeps_it(dev, fused):
    """scores biased so that rows 1 and 2 emit a key token: gkey = KeyRule.move; row 4 was finished before the step: it emits pad
    and keeps its word whatever its scores favour; a row that emits eos in the step still moves"""
    gen = torch.Generator(device=dev).manual_seed(9)
    scores = torch.randn(5, V, device=dev, generator=gen)
    a_maj, d_min, e_maj = (VOC.t2i(f'Key_{k}') for k in ('AMajor', 'DMinor', 'EMajor'))
    scores[1, a_maj] += 100.0
    scores[2, d_min] += 100.0
    scores[3, EOS] += 100.0
    scores[4, e_maj] += 100.0
    for sampling in (sampling_config(do_sample=False), sampling_config(**SAMPLE)):
        gkey = i32(KEYS5, dev)
        live = i32([1, 1, 1, 1, 0], dev)
        toks, _ = _tail(dev, fused, scores, sampling, gkey, unfinished=live)
        assert toks[1:].tolist() == [a_maj, d_min, EOS, PAD]
        rules = Rules(key_rule=RULE, stop=(EOS, PAD, 0))
        want = [move(rules, Words(unfinished=u, gkey=k), tk)[1].gkey
                for u, k, tk in zip([1, 1, 1, 1, 0], KEYS5, toks[:4].tolist() + [e_maj])]
        assert want[4] == KEYS5[4]                                 # (the finished row: whatever token its scores favour)
        assert gkey.tolist() == want and want[1:3] == [key_ordinal('AMajor'), key_ordinal('DMinor')] and want[3] == KEYS5[3]
        assert live.tolist() == [1, 1, 1, 0, 0]
        assert RULE.allows(KEYS5[0], int(toks[0]))


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def _model(dev, seed, off_bias=6.0, closing_bias=0.0, max_length=200):
    """the test pair of tests/test_xl_model_gpu.py (debug size, V = 1190) with a head bias that favours pitches, and most of all
    those of the classes OFF, which C major, A minor and G major all bar: the argmax is an off-key pitch, and with those barred a
    pitch of the key; key tokens and tuplets are biased away, so that a row stays in the key of its
    prompt and, under the bar budget, a bar takes at most 3 + 2 * 2 * slots tokens.  closing_bias: tests/test_grammar_generate_gpu.py's"""
    from tests.test_xl_model_gpu import _pair
    ref, m = _pair(dev, n_layer=2, mem_len=64, seed=seed, max_length=max_length)
    with torch.no_grad():
        b = ref.crit.out_layers[0].bias
        b[torch.from_numpy(RULE.pcs != NO_PITCH)] += off_bias / 2
        b[torch.from_numpy(np.isin(RULE.pcs, OFF))] += off_bias / 2
        b[torch.from_numpy(RULE.keys != NO_KEY)] -= 30.0
        b[VOC.t2i('<tup>')] -= 30.0
        if closing_bias:
            b[VOC.t2i('<bass>')] += closing_bias
            b[BAR] += closing_bias - 2.0
            b[EOS] += closing_bias
    m.load_state_dict(ref.state_dict())
    return m.eval()


def _prompts(n, dev, tail='<bar> <melody>', keyless=True):
    """n headers in the keys PROMPT_KEYS in turn and their key ordinals; keyless: every fourth row has no key token -- a second
    tempo stands in its place, which no grammar accepts"""
    free = [keyless and i % 4 == 3 for i in range(n)]
    rows = [token_ids(VOC, f'TimeSig_2/4 Tempo_120 {"Tempo_96" if free[i] else "Key_" + PROMPT_KEYS[i % 3]} {tail}') for i in range(n)]
    return torch.tensor(rows, dtype=torch.int64, device=dev), [-1 if free[i] else key_ordinal(PROMPT_KEYS[i % 3]) for i in range(n)]


def _ikr(out, Tp, keys, dev):
    """ComputeMetrics' in-key ratio of the generated part of every row against its key (mode 'ins-key': the key is the third label)"""
    from symbolic_music_generation_amd.metrics import ComputeMetrics
    from symbolic_music_generation_amd.vocab import KEY_NAMES
    cm = ComputeMetrics(TOK, mode='ins-key')
    head = torch.tensor([token_ids(VOC, f'TimeSig_2/4 Tempo_120 Key_{KEY_NAMES[k]}') for k in keys], device=dev)
    seq = torch.cat([head, out[:, Tp:].to(dev)], 1)
    counts = cm.counts(seq, seq).cpu().numpy()
    assert (counts[:, :12].sum(1) > 0).all()                       # every row holds pitches
    return [cm.ikr_from_counts(counts[b:b + 1], seq[b:b + 1]) for b in range(len(keys))]


def test_off_key_models_are_off_key_for_every_prompt_key():
    for name in PROMPT_KEYS:
        assert not any((int(RULE.inkey[key_ordinal(name)]) >> pc) & 1 for pc in OFF), name


@pytest.mark.parametrize('kw', [SAMPLE, dict(do_sample=False)], ids=['sample', 'greedy'])
def test_rows_stay_in_key_only_with_the_rule(dev, kw):
    """fails without the feature: generate has no in_key="""
    m = _model(dev, 500)
    n, N = 8, 120
    ids, keys = _prompts(n, dev)
    Tp = ids.shape[1]
    con = torch.tensor([k >= 0 for k in keys])
    free = fresh_generate(m, ids, max_new_tokens=N, seed=3, **kw)
    bad = check_in_key(free, RULE, prompt_len=Tp)
    print('first off-key column without the rule:', bad.tolist())
    assert (bad[con] >= Tp).all() and (bad[~con] == -1).all()      # without the rule every row that has a key leaves it
    got = fresh_generate(m, ids, max_new_tokens=N, seed=3, in_key=RULE, **kw)
    assert got.shape == (n, Tp + N) and torch.equal(got[:, :Tp], ids)
    assert check_in_key(got, RULE, prompt_len=Tp).tolist() == [-1] * n
    assert check_in_key(got.cpu(), RULE, prompt_len=Tp).tolist() == [-1] * n               # the host walk says the same
    rows = [b for b in range(n) if keys[b] >= 0]
    assert _ikr(got[rows], Tp, [keys[b] for b in rows], dev) == [1.0] * len(rows)
    assert all(r < 1.0 for r in _ikr(free[rows], Tp, [keys[b] for b in rows], dev))
    assert torch.equal(got[~con], free[~con]) and not torch.equal(got[con], free[con])     # no key: untouched, token for token
    # key=: overrides the prompts' keys; None / -1 leaves a row unconstrained
    over = ['DbMajor', None, -1, 'CMajor', 'GMajor', 5, None, 'AMinor']
    got2 = fresh_generate(m, ids, max_new_tokens=N, seed=3, in_key=RULE, key=over, **kw)
    assert check_in_key(got2, RULE, prompt_len=Tp, key=over).tolist() == [-1] * n
    off = torch.tensor([k in (None, -1) for k in over])
    assert torch.equal(got2[off], free[off])
    assert check_in_key(got2, RULE, prompt_len=Tp)[0] >= Tp        # row 0 kept D-flat major, not its prompt's C major
    assert _ikr(got2[[0, 3]], Tp, [key_ordinal('DbMajor'), key_ordinal('CMajor')], dev) == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------- 7. combinations
STOP = dict(eos_token_id=EOS, pad_token_id=PAD)
FULL_BAR = '<bar> <melody> p_r d_2 <bass> p_r d_2'                  # 2/4: the open bar is full, so n_bars = 2 is two whole bars
BAR_TOKENS = 3 + 2 * 16 + 2 * 16                                   # the longest bar of 16 slots without tuplets


def _combined(m, ids, n_bars=2, **kw):
    Tp = ids.shape[1]
    return fresh_generate(m, ids, max_length=Tp + 2 * BAR_TOKENS + 1, grammar=TOK.grammar(bar_budget=True), n_bars=n_bars, in_key=RULE,
                **STOP, **kw)


def _assert_all_rules_kept(out, Tp, n_bars=2, mask=None, key=None):
    g = TOK.grammar(bar_budget=True)
    n = out.shape[0]
    assert check_grammar(out, g, mask).tolist() == [-1] * n and check_bar_lengths(out, g, mask).tolist() == [-1] * n
    assert check_in_key(out, RULE, prompt_len=Tp, attention_mask=mask, key=key).tolist() == [-1] * n
    assert bars_after_prompt(out, g, prompt_len=Tp).tolist() == [n_bars] * n
    assert ((out[:, Tp:] == EOS).sum(1) == 1).all()


def _combined_runs(m, dev, use_graph=True):
    """sampled and greedy token matrices of the combined call (also what the child process of the unfused comparison computes)"""
    ids, _ = _prompts(6, dev, FULL_BAR, keyless=False)
    W = ids.shape[1] + 2 * BAR_TOKENS + 1
    outs = []
    for kw in (SAMPLE, dict(do_sample=False), dict(do_sample=True, top_k=8, repetition_penalty=1.2)):
        o = _combined(m, ids, seed=7, use_graph=use_graph, **kw)
        outs.append(torch.nn.functional.pad(o, (0, W - o.shape[1]), value=PAD))
    return torch.stack(outs)


def test_with_grammar_budget_bar_count_and_eos(dev, tmp_path):
    """every rule at once: each row walks clean under all four checks and ends after its two bars; graph replay equals the eager
    loop, and the fused launch equals the unfused tail run in a fresh child process"""
    m = _model(dev, 501, closing_bias=4.0)
    ids, keys = _prompts(6, dev, FULL_BAR, keyless=False)
    Tp = ids.shape[1]
    from symbolic_music_generation_amd.generate import XLDecoder
    assert XLDecoder(m.engine, 2, 32).fused_sampler
    fused = _combined_runs(m, dev)
    for o in fused:
        _assert_all_rules_kept(o, Tp)
    # the grammar, the budget and the count alone leave the key: the key rule is what keeps it
    free = fresh_generate(m, ids, max_length=Tp + 2 * BAR_TOKENS + 1, grammar=TOK.grammar(bar_budget=True), n_bars=2, seed=7, **STOP,
                          **SAMPLE)
    assert (check_in_key(free, RULE, prompt_len=Tp) >= Tp).all()
    assert torch.equal(_combined_runs(m, dev, use_graph=False), fused)
    out = tmp_path / 'unfused.pt'
    code = ('import sys, torch\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'from tests import test_key_rule_gpu as t\n'
            'from symbolic_music_generation_amd.generate import XLDecoder\n'
            'dev = torch.device("cuda:0")\n'
            'm = t._model(dev, 501, closing_bias=4.0)\n'
            'assert not XLDecoder(m.engine, 2, 32).fused_sampler\n'
            f'torch.save(t._combined_runs(m, dev).cpu(), {str(out)!r})\n')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MXL_DECODE_UNFUSED='1'), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert torch.equal(torch.load(out), fused.cpu())


def test_two_lanes_equal_their_decoders(dev):
    from symbolic_music_generation_amd.generate import XLDecoder, XLDecoderLanes
    m = _model(dev, 502, closing_bias=4.0)
    n = 6
    ids, keys = _prompts(n, dev, FULL_BAR, keyless=False)
    Tp = ids.shape[1]
    L = Tp + 2 * BAR_TOKENS + 1
    g = TOK.grammar(bar_budget=True)
    over = ['GMajor', None, 'CMajor', 'AMinor', 3, 'CMajor']
    for kw, key in ((SAMPLE, None), (dict(do_sample=False), over)):
        lanes = XLDecoderLanes(m.engine, n, L, seed=11, lanes=2)
        out = lanes.generate(ids, L, grammar=g, n_bars=2, in_key=RULE, key=key, **STOP, **kw)
        _assert_all_rules_kept(out, Tp, key=key)
        assert [d.gkey.tolist() for d in lanes.lanes] == [[key_ordinal(k) for k in (key[:3], key[3:])[i]] if key else keys[3 * i:3 * i + 3]
                                                          for i in range(2)]
        for i in range(2):
            rows = slice(lanes.offs[i], lanes.offs[i + 1])
            one = XLDecoder(m.engine, lanes.sizes[i], L, seed=11 + 7919 * i).generate(
                ids[rows], L, grammar=g, n_bars=2, in_key=RULE, key=None if key is None else key[rows], **STOP, **kw)
            W = min(one.shape[1], out.shape[1])
            assert torch.equal(out[rows, :W], one[:, :W]) and (out[rows, W:] == PAD).all() and (one[:, W:] == PAD).all(), (kw, i)


def test_left_padded_prompts_and_num_return_sequences(dev):
    m = _model(dev, 503, closing_bias=4.0)
    g = TOK.grammar(bar_budget=True)
    texts = [f'TimeSig_2/4 Tempo_120 Key_CMajor {FULL_BAR}', f'TimeSig_2/4 Tempo_120 Key_GMajor {FULL_BAR} {FULL_BAR}',
             'TimeSig_2/4 Tempo_120 Key_AMinor <bar> <melody> p_r d_2 <bass> p_r d_1 p_r d_1', f'TimeSig_2/4 Tempo_120 {FULL_BAR}']
    prompts = [torch.tensor(token_ids(VOC, t)) for t in texts]
    ids, mask = left_pad(prompts, PAD)
    ids, mask = ids.to(dev), mask.to(dev)
    Tp = ids.shape[1]
    L = Tp + 2 * BAR_TOKENS + 1
    out = fresh_generate(m, ids, attention_mask=mask, max_length=L, grammar=g, n_bars=2, in_key=RULE, do_sample=False, **STOP)
    _assert_all_rules_kept(out, Tp, mask=mask)
    assert m._decoder.gkey.tolist() == [key_ordinal('CMajor'), key_ordinal('GMajor'), key_ordinal('AMinor'), -1]   # pads skipped
    for b, p in enumerate(prompts):
        s = Tp - len(p)
        one = fresh_generate(m, p[None].to(dev), max_length=L - s, grammar=g, n_bars=2, in_key=RULE, do_sample=False, **STOP)[0]
        W = min(one.shape[0], out.shape[1] - s)
        assert torch.equal(out[b, s:s + W], one[:W]) and (out[b, s + W:] == PAD).all() and (one[W:] == PAD).all(), b
    # num_return_sequences repeats the keys per prompt, given or found
    two, keys = _prompts(2, dev, FULL_BAR, keyless=False)
    for key, want in ((None, [keys[0]] * 2 + [keys[1]] * 2), (['EMajor', None], [key_ordinal('EMajor')] * 2 + [-1] * 2)):
        out = fresh_generate(m, two, max_length=two.shape[1] + 2 * BAR_TOKENS + 1, grammar=g, n_bars=2, in_key=RULE, key=key,
                   num_return_sequences=2, **STOP, **SAMPLE)
        assert out.shape[0] == 4 and torch.equal(out[:, :two.shape[1]], two.repeat_interleave(2, 0))
        assert m._decoder.gkey.tolist() == want
        _assert_all_rules_kept(out, two.shape[1], key=None if key is None else [k for k in key for _ in range(2)])
        assert not torch.equal(out[0], out[1])


def test_graph_key_covers_the_rule(dev):
    """one decoder: rule -> none -> a rule with other tables -> the first, each equal to a fresh decoder's result"""
    from symbolic_music_generation_amd.generate import XLDecoder
    m = _model(dev, 504)
    n, L = 4, 70
    ids, _ = _prompts(n, dev)
    other = KeyRule(RULE.keys, RULE.pcs, np.roll(RULE.inkey, 5))
    kw = dict(do_sample=True, top_k=8)
    dec = XLDecoder(m.engine, n, L, seed=4)

    def again(**k):
        dec.rng.zero_()
        return dec.generate(ids, L, **kw, **k)

    def fresh(**k):
        return XLDecoder(m.engine, n, L, seed=4).generate(ids, L, **kw, **k)

    a = again(in_key=RULE)
    assert torch.equal(a, fresh(in_key=RULE)) and check_in_key(a, RULE, prompt_len=ids.shape[1]).tolist() == [-1] * n
    b = again()
    assert torch.equal(b, fresh()) and not torch.equal(a, b)
    c = again(in_key=other)
    assert torch.equal(c, fresh(in_key=other)) and check_in_key(c, other, prompt_len=ids.shape[1]).tolist() == [-1] * n
    assert not torch.equal(c, a) and torch.equal(again(in_key=RULE), a)
    assert torch.equal(again(in_key=RULE, key=[0, -1, 7, 7]), fresh(in_key=RULE, key=[0, -1, 7, 7]))      # keys are step state


def test_reformer(dev):
    """the Reformer decoders take the rule through mask / advance: cached and uncached, greedy and sampling, with eos"""
    from symbolic_music_generation_amd.reformer import MyReformerConfig, MyReformerModelWithLMHead
    cfg = MyReformerConfig('debug-large', vocab_size=V, max_position_embeddings=512, axial_pos_shape=(16, 32),
                           attn_layers=['local'] * 4)
    rf = MyReformerModelWithLMHead(cfg, device=dev, seed=9).eval()
    with torch.no_grad():                                          # the head bias is read from the engine's fp32 parameters
        bias = rf.engine.p32('lm_head.bias')
        bias[torch.from_numpy(RULE.pcs != NO_PITCH).to(dev)] += 3.0
        bias[torch.from_numpy(np.isin(RULE.pcs, OFF)).to(dev)] += 3.0
        bias[torch.from_numpy(RULE.keys != NO_KEY).to(dev)] -= 30.0
    ids, keys = _prompts(4, dev)
    Tp, L = ids.shape[1], 80
    con = torch.tensor([k >= 0 for k in keys])
    for kw in (dict(do_sample=False), SAMPLE):
        rf._decoder = None
        free = rf.generate(input_ids=ids, max_length=L, **kw)
        assert (check_in_key(free, RULE, prompt_len=Tp)[con] >= Tp).all()
        rf._decoder = None
        got = rf.generate(input_ids=ids, max_length=L, in_key=RULE, **kw)
        assert got.shape == (4, L) and check_in_key(got, RULE, prompt_len=Tp).tolist() == [-1] * 4
        assert torch.equal(got[~con], free[~con])
    got = rf.generate(input_ids=ids, max_length=40, in_key=RULE, key='GMajor', use_cache=False, **SAMPLE)
    assert check_in_key(got, RULE, prompt_len=Tp, key='GMajor').tolist() == [-1] * 4
    rf._decoder = None
    keyed, _ = _prompts(4, dev, keyless=False)
    got = rf.generate(input_ids=keyed, max_length=L, grammar=TOK.grammar(), in_key=RULE, **SAMPLE)
    assert check_grammar(got, TOK.grammar()).tolist() == [-1] * 4 and check_in_key(got, RULE, prompt_len=Tp).tolist() == [-1] * 4
    from symbolic_music_generation_amd._lib import MusicXLError
    for bad in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2)):
        with pytest.raises(MusicXLError, match='in_key'):
            rf.generate(input_ids=ids, max_length=20, in_key=RULE, **bad)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(dev):
    from symbolic_music_generation_amd._lib import MusicXLError
    m = _model(dev, 505)
    ids, _ = _prompts(2, dev)
    for kw in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(penalty_alpha=0.6, top_k=4)):
        with pytest.raises(MusicXLError, match='in_key= is supported for greedy decoding and sampling only'):
            m.generate(input_ids=ids, max_length=20, in_key=RULE, **kw)
    with pytest.raises(MusicXLError, match='spans 422 tokens'):                            # a rule over another vocabulary
        m.generate(input_ids=ids, max_length=20, in_key=MusicTokenizer(pitch_kind='midi').key_rule())
    with pytest.raises(ValueError, match='3 entries for 2 prompts'):
        m.generate(input_ids=ids, max_length=20, in_key=RULE, key=[1, 2, 3])
    with pytest.raises(ValueError, match='unknown key'):
        m.generate(input_ids=ids, max_length=20, in_key=RULE, key='HMajor')
    with pytest.raises(ValueError, match='needs in_key='):
        m.generate(input_ids=ids, max_length=20, key='CMajor')
    from symbolic_music_generation_amd.subword import PairMergeTokenizer, WordPieceMusicTokenizer
    for cls in (PairMergeTokenizer, WordPieceMusicTokenizer):
        with pytest.raises(NotImplementedError, match='key rule'):
            cls.key_rule(object.__new__(cls))
    from symbolic_music_generation_amd import ops
    with pytest.raises(MusicXLError, match='spans'):
        ops.rules_mask(torch.zeros(2, 64, device=dev), 64, None, in_key=RULE, gkey=i32([0, 1], dev))
    with pytest.raises(MusicXLError, match='gkey must be'):
        ops.rules_mask(torch.zeros(2, V, device=dev), V, None, in_key=RULE, gkey=i32([0, 1, 2], dev))
