"""The bar budget on the device (`generate(grammar=tokenizer.grammar(bar_budget=True))`): the prompt scan, the mask and the advance
against the host rule of grammar.BarBudget, and generation under it -- every channel of every generated bar exactly as long as the
row's time signature, on a small random-weight model over the midi vocabulary (V = 422), which unconstrained breaks the rule at
once -- with the paths (fused / unfused, graph / eager, lanes, padded prompts, eos, Reformer) agreeing with one another."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from symbolic_music_generation_amd.generate import check_bar_lengths, check_grammar, finish_at_eos
from symbolic_music_generation_amd.grammar import BarBudget, TokenGrammar, music_budget_tables
from symbolic_music_generation_amd.vocab import MusicVocabulary
from tests.rules_ref import Rules, Words, host_allowed, keep_rows, move

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'sample_score_ids.npz')
NEAR_TIE = 5e-2          # tests/test_ragged_generate_gpu.py: a fork between batch shapes is legitimate only at a bf16 near-tie
VOC = MusicVocabulary(pitch_kind='midi')
V = len(VOC)
EOS, PAD, BAR, BASS = (VOC.t2i(t) for t in ('</s>', '[PAD]', '<bar>', '<bass>'))
SIGS = ('4/4', '3/4', '6/8', 'rare')
B, L = 8, 160
SAMPLE = dict(do_sample=True, temperature=1.5, top_k=0)


def _model(dev, seed, closing_bias=0.0):
    """tests/test_grammar_generate_gpu.py's model over the midi vocabulary: 2 layers, d_model 128, mem_len 64"""
    from tests.test_xl_model_gpu import _pair
    ref, m = _pair(dev, vocab=V, n_layer=2, mem_len=64, seed=seed, max_length=200)
    if closing_bias:
        with torch.no_grad():
            b = ref.crit.out_layers[0].bias
            b[BASS] += closing_bias
            b[BAR] += closing_bias - 2.0
            b[EOS] += closing_bias
        m.load_state_dict(ref.state_dict())
    m.eval()
    return ref, m


def _headers(n, dev, sigs=SIGS):
    rows = [[VOC.t2i(t) for t in (f'TimeSig_{sigs[i % len(sigs)]}', 'Tempo_120', 'Key_CMajor', '<bar>')] for i in range(n)]
    return torch.tensor(rows, dtype=torch.int64, device=dev)


def _fresh(m, n, length, seed=5):
    from symbolic_music_generation_amd.generate import XLDecoder
    return XLDecoder(m.engine, n, length, seed=seed)


def _constrained(n, sigs=SIGS):
    return torch.tensor([sigs[i % len(sigs)] != 'rare' for i in range(n)])


def _clean(out, g, mask=None):
    return check_bar_lengths(out, g, mask).tolist() == [-1] * out.shape[0] and check_grammar(out, g, mask).tolist() == [-1] * out.shape[0]


# ---------------------------------------------------------------------------------------------------------------- op level
def test_scan_equals_the_host_walk(dev):
    """the four fixtures cut at 40 columns, left-padded by different amounts, five rows a launch: bar, rem and first_bad"""
    from symbolic_music_generation_amd import ops
    z = np.load(GOLD)
    rng = np.random.default_rng(0)
    seen_bad = 0
    for kind, name in (('midi', 'sample_full_midi'), ('step', 'sample_full_step'), ('degree', 'sample_full_degree'),
                       ('degree', 'gen_broken')):
        g = MusicVocabulary(pitch_kind=kind).grammar(bar_budget=True)
        song = z[name].astype(np.int64)
        cuts = sorted({1, 2, 63, 64, 65, len(song)} | set(rng.integers(3, len(song), 60).tolist()))[:40]
        assert len(cuts) == 40
        cuts = [cuts[i] for i in rng.permutation(40)]
        for i in range(0, 40, 5):
            part = cuts[i:i + 5]
            T = max(part) + 7
            rows = []
            for j, n in enumerate(part):
                pad = int(rng.integers(0, T - n + 1)) if j else T - n
                r = np.full(T, -1, dtype=np.int64)
                r[pad:pad + n] = song[:n]                          # (pads on the left, and skipped columns after the row as well)
                rows.append(r)
            ids = torch.from_numpy(np.stack(rows)).to(dev)
            gbar = torch.full((5,), -7, device=dev, dtype=torch.int32)
            grem, bad = gbar.clone(), gbar.clone()
            ops.budget_scan(ids, T, g, gbar, grem, bad)
            want = [g.walk_budget(r) for r in rows]
            assert list(zip(gbar.tolist(), grem.tolist(), bad.tolist())) == want, (name, part)
            seen_bad += sum(1 for w in want if w[2] >= 0)
            assert check_bar_lengths(ids, g).tolist() == [w[2] for w in want]
    assert seen_bad > 0


def _padded_grammar(vocab_size):
    """the midi grammar and budget over a vocabulary padded to vocab_size (the extra tokens: pitches)"""
    g0 = VOC.grammar()
    if vocab_size == V:
        return VOC.grammar(bar_budget=True)
    t = music_budget_tables(VOC)
    n = vocab_size - V
    cls = np.concatenate([g0.cls, np.full(n, g0.class_names.index('pitch'), dtype=np.uint8)])
    g = TokenGrammar(cls, g0.allow, g0.next, g0.start, g0.accepting, g0.class_names, g0.state_names)
    BarBudget(g, np.concatenate([t['slots'], np.zeros(n, dtype=np.uint16)]),
              np.concatenate([t['bars'], np.full(n, 0xFFFF, dtype=np.uint16)]), t['opens'], t['need_free'], t['need_full'])
    return g


#         bar rem, three rows a launch
STATES = ([(32, 0), (32, 1), (32, 32)], [(0, 0), (24, 24), (24, 23)], [(48, 47), (16, 0), (0, 0)])


@pytest.mark.parametrize('vocab_size', [V, 2049])
def test_mask_and_advance_equal_the_host_rule(dev, vocab_size):
    from symbolic_music_generation_amd import ops
    g = _padded_grammar(vocab_size)
    torch.manual_seed(2)
    for states in STATES:
        logp = torch.randn(3, vocab_size + 3)
        lp = logp.to(dev)[:, :vocab_size]                           # a row stride that is not V
        gbar = torch.tensor([s[0] for s in states], device=dev, dtype=torch.int32)
        grem = torch.tensor([s[1] for s in states], device=dev, dtype=torch.int32)
        ops.rules_mask(lp, vocab_size, None, grammar=g, gbar=gbar, grem=grem)    # the budget alone
        keep = keep_rows(Rules(g, automaton=False, budget=True), [Words(gbar=bar, grem=rem) for bar, rem in states], vocab_size)
        got = lp.cpu()
        assert torch.equal(torch.isinf(got), ~keep) and torch.equal(got[keep], logp[:, :vocab_size][keep]), states
        assert keep[[i for i, s in enumerate(states) if s[0] == 0]].all()      # bar == 0: untouched
    # advance: every kind of token from every state; the row that was finished before the step keeps its words
    toks = [VOC.t2i(t) for t in ('TimeSig_3/4', 'TimeSig_rare', '<melody>', '<bass>', 'd_1/8', 'd_6', 'd_rare', 'p_r', '<bar>', '</tup>')]
    for bar, rem in ((32, 5), (0, 0), (24, 24), (48, 0)):
        n = len(toks) + 1
        ids = torch.zeros(n, 4, device=dev, dtype=torch.int64)
        ids[:, 2] = torch.tensor(toks + [toks[2]], device=dev)
        t = torch.full((1,), 2, device=dev, dtype=torch.int32)
        gbar = torch.full((n,), bar, device=dev, dtype=torch.int32)
        grem = torch.full((n,), rem, device=dev, dtype=torch.int32)
        live = torch.ones(n, device=dev, dtype=torch.int32)
        live[-1] = 0
        ops.rules_advance(ids, t, stop=(EOS, PAD, 0), unfinished=live, alive=torch.zeros_like(t), grammar=g, gbar=gbar, grem=grem)
        rules = Rules(g, automaton=False, budget=True, stop=(EOS, PAD, 0))
        want = [move(rules, Words(unfinished=u, gbar=bar, grem=rem), k)[1][2:4] for k, u in zip(toks + [toks[2]], [1] * len(toks) + [0])]
        assert want[-1] == (bar, rem)                              # the row that was finished before the step
        assert list(zip(gbar.tolist(), grem.tolist())) == want, (bar, rem)


# ---------------------------------------------------------------------------------------------------------------- the feature
@pytest.mark.parametrize('kw', [SAMPLE, dict(do_sample=False)], ids=['sample', 'greedy'])
def test_every_generated_bar_is_as_long_as_its_time_signature(dev, kw):
    """fails without the feature: `grammar(bar_budget=True)` does not exist"""
    ref, m = _model(dev, 400)
    ids = _headers(B, dev)
    Tp = ids.shape[1]
    g, plain = VOC.grammar(bar_budget=True), VOC.grammar()
    con = _constrained(B)
    m._decoder = None
    got = m.generate(input_ids=ids, max_length=L, grammar=g, seed=21, **kw)
    assert got.shape == (B, L) and torch.equal(got[:, :Tp], ids)
    assert _clean(got, g)
    assert _clean(got.cpu(), g)                                    # the host walk says the same
    # a few dozen channel borders were crossed under the constraint
    assert int(((got[con] == BAR) | (got[con] == BASS)).sum()) >= 24
    m._decoder = None
    free = m.generate(input_ids=ids, max_length=L, grammar=plain, seed=21, **kw)
    assert check_grammar(free, plain).tolist() == [-1] * B
    bad = check_bar_lengths(free, g)
    assert (bad[con] >= Tp).any(), bad                             # the grammar alone breaks the budget
    assert (bad[~con] == -1).all()
    assert torch.equal(got[~con], free[~con])                      # TimeSig_rare rows: the syntactic grammar, token for token
    assert not torch.equal(got[con], free[con])


# ---------------------------------------------------------------------------------------------------------------- exactness
def _decoder_runs(m, dev, use_graph=True):
    """greedy and sampled token matrices of a fresh decoder (also what the child process of the unfused comparison computes)"""
    g = VOC.grammar(bar_budget=True)
    prompt = _headers(B, dev)
    outs = []
    for kw in (dict(do_sample=False), SAMPLE, dict(do_sample=True, top_k=8, typical_p=0.9, repetition_penalty=1.2)):
        outs.append(_fresh(m, B, L, 7).generate(prompt, L, use_graph=use_graph, grammar=g, **kw))
    return torch.stack(outs)


def test_fused_equals_unfused_in_a_child_process(dev, tmp_path):
    ref, m = _model(dev, 401)
    dec = _fresh(m, B, L, 7)
    assert dec.fused_sampler
    fused = _decoder_runs(m, dev)
    g = VOC.grammar(bar_budget=True)
    for o in fused:
        assert _clean(o, g)
    out = tmp_path / 'unfused.pt'
    code = ('import sys, torch\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'from tests import test_bar_budget_gpu as t\n'
            'dev = torch.device("cuda:0")\n'
            'ref, m = t._model(dev, 401)\n'
            'assert not t._fresh(m, t.B, t.L, 7).fused_sampler\n'
            f'torch.save(t._decoder_runs(m, dev).cpu(), {str(out)!r})\n')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MXL_DECODE_UNFUSED='1'), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert torch.equal(torch.load(out), fused.cpu())


def test_graph_replay_equals_eager(dev):
    ref, m = _model(dev, 401)
    assert torch.equal(_decoder_runs(m, dev, use_graph=True), _decoder_runs(m, dev, use_graph=False))


def test_one_decoder_across_budget_none_budget(dev):
    """the graph key holds the budget's tables and the saved state its two words: one decoder reused equals fresh decoders"""
    ref, m = _model(dev, 402)
    prompt = _headers(B, dev)
    g, plain = VOC.grammar(bar_budget=True), VOC.grammar()
    kw = dict(do_sample=True, top_k=8)

    def fresh(**k):
        return _fresh(m, B, L, 4).generate(prompt, L, **kw, **k)

    dec = _fresh(m, B, L, 4)

    def again(**k):
        dec.rng.zero_()
        return dec.generate(prompt, L, **kw, **k)

    a = again(grammar=g)
    assert dec.graph is not None and torch.equal(a, fresh(grammar=g)) and _clean(a, g)
    # what the device holds after the run is what the host walk of the output says
    walks = [g.walk_budget(r) for r in a.cpu()]
    assert list(zip(dec.gbar.tolist(), dec.grem.tolist())) == [w[:2] for w in walks]
    b = again()
    assert torch.equal(b, fresh()) and not torch.equal(a, b)
    c = again(grammar=plain)
    assert torch.equal(c, fresh(grammar=plain)) and not torch.equal(a, c)
    assert torch.equal(again(grammar=g), a)
    g2 = VOC.grammar(bar_budget=True)                              # equal tables at other addresses: captured anew, same result
    assert torch.equal(again(grammar=g2), a)


def test_two_lanes_equal_one(dev):
    from symbolic_music_generation_amd.generate import XLDecoderLanes
    ref, m = _model(dev, 403)
    n = 10                                                         # lanes of 5 rows: the signatures fall differently in each
    prompt = _headers(n, dev)
    g = VOC.grammar(bar_budget=True)
    for kw in (SAMPLE, dict(do_sample=False)):
        lanes = XLDecoderLanes(m.engine, n, L, seed=11, lanes=2)
        out = lanes.generate(prompt, L, grammar=g, **kw)
        assert _clean(out, g)
        for i in range(2):
            rows = slice(lanes.offs[i], lanes.offs[i + 1])
            one = _fresh(m, lanes.sizes[i], L, 11 + 7919 * i).generate(prompt[rows], L, grammar=g, **kw)
            assert torch.equal(out[rows], one), (kw, i)


# ---------------------------------------------------------------------------------------------------------------- with eos
def test_eos_and_min_length_with_the_budget(dev):
    ref, m = _model(dev, 404, closing_bias=9.0)
    prompt = _headers(B, dev)
    Tp = prompt.shape[1]
    g = VOC.grammar(bar_budget=True)
    END = g.state('END')
    for kw in (SAMPLE, dict(do_sample=False)):
        full = _fresh(m, B, L, 9).generate(prompt, L, grammar=g, **kw)
        assert _clean(full, g)
        ended = (full[:, Tp:] == EOS).any(1)
        assert ended.any(), kw
        dec = _fresh(m, B, L, 9)
        got = dec.generate(prompt, L, grammar=g, eos_token_id=EOS, pad_token_id=PAD, **kw)
        assert torch.equal(got, finish_at_eos(full, Tp, EOS, PAD)), kw
        done = dec.unfinished.cpu() == 0
        assert torch.equal(done, ended.cpu()) and (dec.gstate.cpu()[done] == END).all()
        # every finished row ends on a full bass channel: nothing is left of it, and the token before </s> closed a note
        assert (dec.grem.cpu()[done] == 0).all()
        for r in got[done].cpu():
            e = int((r[Tp:] == EOS).int().argmax()) + Tp
            bar, rem, bad = g.walk_budget(r[:e])
            assert bad == -1 and rem == 0 and g.state_names[g.walk(r[:e])[0]] == 'B_D'
        # min_length: </s> barred where grammar and budget allow it; <bar> is still there, so no row is ever all-masked
        first = int((full[:, Tp:] == EOS).int().argmax(1)[ended].min()) + Tp
        m_len = first + 12
        got = _fresh(m, B, L, 9).generate(prompt, L, grammar=g, eos_token_id=EOS, pad_token_id=PAD, min_length=m_len, **kw)
        assert not (got[:, :m_len] == EOS).any() and _clean(got, g), kw


# ---------------------------------------------------------------------------------------------------------------- other paths
def test_left_padded_rows_equal_the_prompt_alone(dev):
    from symbolic_music_generation_amd.generate import left_pad
    ref, m = _model(dev, 405)
    ref.eval()
    song = torch.from_numpy(np.load(GOLD)['sample_full_midi'].astype(np.int64))
    prompts = [song[:n] for n in (4, 9, 17, 30, 12, 6)]            # cut inside channels as well: rem comes from the scan
    ids, mask = left_pad(prompts, PAD)
    ids, mask = ids.to(dev), mask.to(dev)
    Tp, length = ids.shape[1], 130
    g = VOC.grammar(bar_budget=True)
    m._decoder = None
    out = m.generate(input_ids=ids, attention_mask=mask, max_length=length, do_sample=False, grammar=g)
    assert torch.equal(out[:, :Tp], ids) and _clean(out, g, mask)
    m._decoder = None
    assert _clean(m.generate(input_ids=ids, attention_mask=mask, max_length=length, grammar=g, **SAMPLE), g, mask)
    for b, p in enumerate(prompts):
        s = Tp - len(p)
        m._decoder = None
        one = m.generate(input_ids=p[None].to(dev), max_length=length - s, do_sample=False, grammar=g)[0].cpu()
        row = out[b, s:].cpu()
        mism = (row != one).nonzero()
        if mism.numel():                                            # legitimate only at a near-tie of the masked oracle scores
            t0 = int(mism[0, 0])
            with torch.no_grad():
                lp = ref(one[None, :t0]).prediction_scores[0, -1].float()
            top2 = lp.masked_fill(~host_allowed(g)(one[None, :t0])[0], float('-inf')).topk(2).values
            print(f'row {b}: fork at {t0}, margin {(top2[0] - top2[1]).item():.4f}')
            assert (top2[0] - top2[1]).item() < NEAR_TIE, (b, t0)


def test_num_return_sequences(dev):
    ref, m = _model(dev, 406)
    g = VOC.grammar(bar_budget=True)
    m._decoder = None
    out = m.generate(input_ids=_headers(3, dev), max_length=L, grammar=g, num_return_sequences=3, **SAMPLE)
    assert out.shape == (9, L) and _clean(out, g)
    assert len({tuple(r) for r in out[:3].tolist()}) == 3          # three different continuations of one 4/4 prompt
    m._decoder = None
    out = m.generate(input_ids=_headers(3, dev), grammar=g, num_return_sequences=3, eos_token_id=EOS, pad_token_id=PAD,
                     max_new_tokens=60, **SAMPLE)
    assert out.shape[0] == 9 and out.shape[1] <= 64 and _clean(out, g)


def test_reformer(dev):
    from symbolic_music_generation_amd.reformer import MyReformerConfig, MyReformerModelWithLMHead
    cfg = MyReformerConfig('debug-large', vocab_size=V, max_position_embeddings=512, axial_pos_shape=(16, 32),
                           attn_layers=['local'] * 4)
    rf = MyReformerModelWithLMHead(cfg, device=dev, seed=9).eval()
    g, plain = VOC.grammar(bar_budget=True), VOC.grammar()
    prompt = _headers(4, dev)
    con = _constrained(4)
    for kw in (dict(do_sample=False), SAMPLE):
        rf._decoder = None
        got = rf.generate(input_ids=prompt, max_length=120, grammar=g, **kw)
        assert got.shape == (4, 120) and _clean(got, g), kw
        rf._decoder = None
        free = rf.generate(input_ids=prompt, max_length=120, grammar=plain, **kw)
        assert (check_bar_lengths(free, g)[con] >= 0).any() and torch.equal(free[~con], got[~con]), kw
    got = rf.generate(input_ids=prompt, max_length=48, grammar=g, use_cache=False, **SAMPLE)
    assert got.shape == (4, 48) and _clean(got, g)
    # eos: rows finished keep their words
    rf._decoder = None
    full = rf.generate(input_ids=prompt, max_length=120, grammar=g, **SAMPLE)
    eos = int(full[0, 10])
    rf._decoder = None
    got = rf.generate(input_ids=prompt, max_length=120, grammar=g, eos_token_id=eos, pad_token_id=0, **SAMPLE)
    assert torch.equal(got, finish_at_eos(full, prompt.shape[1], eos, 0))


def test_prompt_that_breaks_the_budget_raises(dev):
    from symbolic_music_generation_amd._lib import MusicXLError
    ref, m = _model(dev, 407)
    g = VOC.grammar(bar_budget=True)
    head = 'TimeSig_3/4 Tempo_120 <bar> <melody>'
    rows = [f'{head} p_1/4 d_3 <bass>', f'{head} p_1/4 d_3 <bass>', f'{head} p_1/4 d_2 <bass>', f'{head} p_1/4 d_3 <bass>']
    ids = torch.tensor([[VOC.t2i(t) for t in r.split()] for r in rows], device=dev)
    with pytest.raises(MusicXLError, match=r'row 2 underfills a bar at column 6'):
        m.generate(input_ids=ids, max_new_tokens=10, do_sample=False, grammar=g)
    ids[2, 5] = VOC.t2i('d_25/8')
    with pytest.raises(MusicXLError, match=r'row 2 overfills a bar at column 5'):
        m.generate(input_ids=ids, max_new_tokens=10, do_sample=False, grammar=g)
    # the grammar alone takes both, and the mended prompt runs
    m.generate(input_ids=ids, max_new_tokens=10, do_sample=False, grammar=VOC.grammar())
    ids[2, 5] = VOC.t2i('d_3')
    out = m.generate(input_ids=ids, max_new_tokens=40, do_sample=False, grammar=g)
    assert _clean(out, g)
    for kw in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(penalty_alpha=0.6, top_k=4)):
        with pytest.raises(MusicXLError, match='grammar'):
            m.generate(input_ids=ids, max_length=20, grammar=g, **kw)
