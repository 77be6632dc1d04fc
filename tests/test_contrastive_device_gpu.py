"""Contrastive search with its step on the device, end to end on TransfoXL: generate.contrastive_search_device against the
host-driven generate.contrastive_search on a second decoder, the public `generate(penalty_alpha=, top_k=)` on either path, and the
grammar and key rules under contrastive search against the host path with a mask built from grammar.py's host walkers."""
import pytest
import torch

from symbolic_music_generation_amd import generate as G
from symbolic_music_generation_amd.generate import (XLDecoder, check_bar_lengths, check_grammar, check_in_key, contrastive_search,
                                                    contrastive_search_device)
from tests.rules_ref import host_allowed

pytestmark = pytest.mark.gpu

# The model is tests/test_xl_model_gpu.py's pair at n_layer 2, mem_len 64, with init_std 0.4.  On the CPU,
# oracle.transfoxl_ref.ref_contrastive_search(return_trace=True), restated to record the log-probability gap as well, showed that at
# the default init_std 0.02 the debug model's log-probabilities are nearly flat: with model seed 13 and prompt seeds 0..5 the K-th and
# the (K+1)-th log-probability at K = 16 came within 2e-5 .. 8.3e-4 of each other in every run of 68 steps (and within 1.5e-3 at K =
# 4), so no seed of that model makes the demand for equal tokens fair.  The wider initialisation spreads them.  The bf16
# model leaves the fp32 oracle's trajectory within a few tokens, so the gaps that count are those of the host path itself: model seed
# 3 and, per (K, alpha), the prompt seed in PROMPT_SEED were chosen from generate.contrastive_search(trace=) over model seeds 1..3 and
# prompt seeds 0..15 (two prompts x 68 steps each, every sequence emitting at least 8 distinct tokens) as the ones with the largest
# smallest gap.  GAPS holds what was measured then, (smallest score gap, smallest log-probability gap) over the 136 decisions of the
# run without eos; the smallest of all is 0.01175.  The test asserts the condition on the host path's own trace and prints what it
# measures.
SEED, INIT_STD, TP, L = 3, 0.4, 12, 80
PROMPT_SEED = {(2, 0.3): 8, (2, 0.6): 6, (4, 0.3): 9, (4, 0.6): 4, (16, 0.3): 8, (16, 0.6): 8}
GAPS = {(2, 0.3): (0.05981, 0.01175), (2, 0.6): (0.01957, 0.0264), (4, 0.3): (0.03668, 0.02726), (4, 0.6): (0.01604, 0.01646),
        (16, 0.3): (0.0589, 0.01515), (16, 0.6): (0.01505, 0.01675)}
FAIR = 1e-3
EOS_NEVER = -1


@pytest.fixture(scope='module')
def plain(dev):
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=64, max_length=L, seed=SEED, init_std=INIT_STD)
    return m.eval()


def _prompt(dev, seed):
    return torch.randint(4, 1190, (2, TP), generator=torch.Generator().manual_seed(seed)).to(dev)


def _assert_fair(trace, what):
    """over the steps in which a sequence was live: the two best contrastive scores and the K-th and (K+1)-th log-probability are
    further apart than FAIR, so that another implementation may be held to the same tokens"""
    live = torch.stack([t[0] for t in trace])
    sg = torch.stack([t[1] for t in trace])[live].min().item()
    lg = torch.stack([t[2] for t in trace])[live].min().item()
    print(f'contrastive search {what}: smallest score gap {sg:.5f}, smallest log-probability gap {lg:.5f} over {int(live.sum())} decisions')
    assert sg > FAIR and lg > FAIR, (what, sg, lg)


@pytest.mark.parametrize('alpha', [0.3, 0.6])
@pytest.mark.parametrize('K', [2, 4, 16])
def test_device_path_equals_host_path(plain, dev, K, alpha):
    m, prompt = plain, _prompt(dev, PROMPT_SEED[(K, alpha)])
    kw = dict(top_k=K, penalty_alpha=alpha, pad_token_id=0)
    trace = []
    want = contrastive_search(XLDecoder(m.engine, 2 * K, L), prompt, L, eos_token_id=EOS_NEVER, trace=trace, **kw)
    _assert_fair(trace, f'K={K} alpha={alpha} eos never')
    assert want.shape == (2, L)
    dec = XLDecoder(m.engine, 2 * K, L)
    got = contrastive_search_device(dec, prompt, L, eos_token_id=EOS_NEVER, use_graph=True, stop_chunk=5, **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    assert dec.steps_run == L - TP - 1 and int(dec.cs.n_done) == 0
    eager = contrastive_search_device(XLDecoder(m.engine, 2 * K, L), prompt, L, eos_token_id=EOS_NEVER, use_graph=False, **kw)
    assert torch.equal(eager, got)
    again = contrastive_search_device(dec, prompt, L, eos_token_id=EOS_NEVER, use_graph=True, **kw)   # the captured step, replayed
    assert torch.equal(again, got)                                                                   # from a new start
    # an eos that is emitted: a token sequence 0 generates part of the way in
    eos = int(want[0, TP + 20])
    trace = []
    want_e = contrastive_search(XLDecoder(m.engine, 2 * K, L), prompt, L, eos_token_id=eos, trace=trace, **kw)
    _assert_fair(trace, f'K={K} alpha={alpha} eos {eos}')
    assert (want_e[0, TP:] == eos).any()
    got_e = contrastive_search_device(dec, prompt, L, eos_token_id=eos, use_graph=True, stop_chunk=5, **kw)
    assert got_e.shape == want_e.shape and torch.equal(got_e, want_e)
    eager_e = contrastive_search_device(dec, prompt, L, eos_token_id=eos, use_graph=False, stop_chunk=7, **kw)
    assert torch.equal(eager_e, got_e)


def test_generate_takes_either_path(plain, dev, monkeypatch):
    m, prompt = plain, _prompt(dev, PROMPT_SEED[(4, 0.6)])
    calls = []
    real = G.contrastive_search_device
    monkeypatch.setattr(G, 'contrastive_search_device', lambda *a, **k: (calls.append(k.get('top_k')), real(*a, **k))[1])
    kw = dict(input_ids=prompt, max_length=L, penalty_alpha=0.6, top_k=4, eos_token_id=EOS_NEVER, pad_token_id=0)
    dev_ids = m.generate(**kw)
    assert calls == [4]
    monkeypatch.setenv('MXL_CONTRASTIVE_HOST', '1')
    host_ids = m.generate(**kw)
    assert calls == [4] and dev_ids.shape == (2, L) and torch.equal(dev_ids, host_ids)
    monkeypatch.delenv('MXL_CONTRASTIVE_HOST')
    assert torch.equal(m.generate(**kw, use_graph=False), dev_ids) and calls == [4, 4]
    # 33 candidates are more than the device step takes: the host path
    wide = m.generate(**{**kw, 'top_k': 33, 'max_length': TP + 8})
    assert calls == [4, 4]
    want = contrastive_search(XLDecoder(m.engine, 2 * 33, TP + 8), prompt, TP + 8, top_k=33, penalty_alpha=0.6, eos_token_id=EOS_NEVER,
                              pad_token_id=0)
    assert torch.equal(wide, want)
    # with next to no penalty the pick is the most probable candidate: greedy decoding
    m._decoder = None
    greedy = m.generate(input_ids=prompt, max_length=L, eos_token_id=EOS_NEVER, pad_token_id=0)
    assert torch.equal(m.generate(**{**kw, 'penalty_alpha': 1e-9}), greedy)


# ---------------------------------------------------------------------------------------------------------------- rules
K_RULES, ALPHA_RULES = 4, 0.6


def _rules_case(dev, seed, grammar, budget, in_key, closing_bias=4.0, new=40):
    from tests.test_key_rule_gpu import EOS, FULL_BAR, PAD, RULE, TOK, _model, _prompts
    m = _model(dev, seed, closing_bias=closing_bias)
    ids, _ = _prompts(3, dev, FULL_BAR, keyless=False) if grammar else _prompts(3, dev, keyless=False)
    Tp = ids.shape[1]
    W = Tp + new
    g = TOK.grammar(bar_budget=budget) if grammar else None
    rule = RULE if in_key else None
    kw = dict(top_k=K_RULES, penalty_alpha=ALPHA_RULES, eos_token_id=EOS, pad_token_id=PAD)
    got = m.generate(input_ids=ids, max_length=W, grammar=g, in_key=rule, **kw)
    seen = []
    want = contrastive_search(XLDecoder(m.engine, ids.shape[0] * K_RULES, W), ids, W, allowed=host_allowed(g, rule=rule, seen=seen),
                              **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    # every returned row: its prompt, then a continuation that every rule accepts up to and including its eos
    assert torch.equal(got[:, :Tp], ids)
    for row in got.tolist():
        t = torch.tensor(row[:(row.index(EOS) + 1) if EOS in row else len(row)])
        if g is not None:
            assert check_grammar(t, g).tolist() == [-1]
            if budget:
                assert check_bar_lengths(t, g).tolist() == [-1]
        if rule is not None:
            assert check_in_key(t, rule, prompt_len=Tp).tolist() == [-1]
    return got, seen, m, ids


@pytest.mark.parametrize('in_key', [False, True])
@pytest.mark.parametrize('budget', [False, True])
def test_grammar_under_contrastive_search_equals_the_masked_host_path(dev, budget, in_key):
    """fails without the feature: generate(penalty_alpha=, top_k=, grammar=) raises MusicXLError there"""
    got, seen, _, _ = _rules_case(dev, 611 + 2 * budget + in_key, True, budget, in_key)
    if budget:
        # the forced <bass> / <bar> states of the budget grammar leave fewer tokens than candidates: dead candidates occurred
        assert any(0 < n < K_RULES for n in seen)


def test_in_key_alone_under_contrastive_search(dev):
    from tests.test_key_rule_gpu import EOS, PAD, RULE
    got, _, m, ids = _rules_case(dev, 615, False, False, True, closing_bias=0.0, new=30)
    Tp = ids.shape[1]
    free = m.generate(input_ids=ids, max_length=Tp + 30, top_k=K_RULES, penalty_alpha=ALPHA_RULES, eos_token_id=EOS, pad_token_id=PAD)
    assert (check_in_key(free, RULE, prompt_len=Tp) >= Tp).all()           # the model leaves the key without the rule


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_keep_their_messages(dev, monkeypatch):
    from symbolic_music_generation_amd._lib import MusicXLError
    from tests.test_key_rule_gpu import EOS, PAD, RULE, TOK, _model, _prompts
    m = _model(dev, 616)
    ids, _ = _prompts(2, dev, keyless=False)
    g = TOK.grammar(bar_budget=True)
    stop = dict(eos_token_id=EOS, pad_token_id=PAD)
    cs = dict(penalty_alpha=0.6, top_k=4)
    only = 'is supported for greedy decoding and sampling only'
    # rules without an explicit eos_token_id
    for name, rk in (('grammar', dict(grammar=g)), ('in_key', dict(in_key=RULE)), ('in_key', dict(key='CMajor'))):
        with pytest.raises(MusicXLError, match=f'{name}= {only}'):
            m.generate(input_ids=ids, max_length=20, **rk, **cs)
    # n_bars, with or without a grammar and an eos; melody; padded prompts
    with pytest.raises(MusicXLError, match=f'n_bars= {only}'):
        m.generate(input_ids=ids, max_length=20, grammar=g, n_bars=1, **stop, **cs)
    with pytest.raises(MusicXLError, match=f'n_bars= {only}'):
        m.generate(input_ids=ids, max_length=20, n_bars=1, **stop, **cs)
    with pytest.raises(MusicXLError, match=f'melody= {only}'):
        m.generate(input_ids=ids, max_length=40, grammar=g, melody=[1, 2, 3], **stop, **cs)
    mask = torch.ones_like(ids)
    mask[0, 0] = 0
    with pytest.raises(MusicXLError, match='padded prompts'):
        m.generate(input_ids=ids, attention_mask=mask, max_length=20, **cs)
    # rules on the host path: more candidates than the device step takes, or MXL_CONTRASTIVE_HOST=1
    for name, rk in (('grammar', dict(grammar=g)), ('in_key', dict(in_key=RULE))):
        with pytest.raises(MusicXLError, match=f'{name}= {only}'):
            m.generate(input_ids=ids, max_length=20, penalty_alpha=0.6, top_k=33, **rk, **stop)
    monkeypatch.setenv('MXL_CONTRASTIVE_HOST', '1')
    for name, rk in (('grammar', dict(grammar=g)), ('in_key', dict(in_key=RULE))):
        with pytest.raises(MusicXLError, match=f'{name}= {only}'):
            m.generate(input_ids=ids, max_length=20, **rk, **stop, **cs)
    monkeypatch.delenv('MXL_CONTRASTIVE_HOST')
    # with an eos, the argument checks of the sampling path hold under contrastive search
    with pytest.raises(ValueError, match='needs in_key='):
        m.generate(input_ids=ids, max_length=20, key='CMajor', **stop, **cs)
