"""Contrastive search over shared rings, end to end on TransfoXL: `generate(penalty_alpha=, top_k=, contrastive_rings='shared')` against
the default mode of the same call.  The model is tests/test_contrastive_device_gpu.py's (2 layers, mem_len 64, init_std 0.4); at that
mem_len both modes run the ring in one piece, so the attention output of every candidate row is the copied mode's bit for bit
(tests/test_contrastive_shared_ops_gpu.py) and the ids are held to torch.equal -- no tolerance, whatever the gaps between candidates."""
import pytest
import torch

from symbolic_music_generation_amd import generate as G
from symbolic_music_generation_amd.generate import XLDecoder, contrastive_search_device

pytestmark = pytest.mark.gpu

SEED, INIT_STD, TP, L, MEM = 3, 0.4, 12, 80, 64          # L > MEM + TP: the generation runs across the wrap of the ring
EOS_NEVER = -1


@pytest.fixture(scope='module')
def plain(dev):
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=MEM, max_length=L, seed=SEED, init_std=INIT_STD)
    return m.eval()


def _prompt(dev, n, seed, Tp=TP):
    return torch.randint(4, 1190, (n, Tp), generator=torch.Generator().manual_seed(seed)).to(dev)


def _both(m, **kw):
    """the call in the default mode and over shared rings"""
    return m.generate(**kw), m.generate(**kw, contrastive_rings='shared')


@pytest.mark.parametrize('alpha', [0.3, 0.6])
@pytest.mark.parametrize('K', [2, 4, 16])
def test_shared_rings_return_the_ids_of_the_default_mode(plain, dev, K, alpha):
    kw = dict(max_length=L, penalty_alpha=alpha, top_k=K, eos_token_id=EOS_NEVER, pad_token_id=0)
    for n in (3, 1):
        ids = _prompt(dev, n, 10 * K + n)
        want, got = _both(plain, input_ids=ids, **kw)
        assert want.shape == (n, L) and torch.equal(got, want), (n, (got != want).nonzero()[:4].tolist())
        eager = plain.generate(input_ids=ids, **kw, contrastive_rings='shared', use_graph=False)
        assert torch.equal(eager, want)
        assert len(set(want[0, TP:].tolist())) >= 4                    # (the model says something)


def test_a_prompt_longer_than_the_ring(plain, dev):
    ids = _prompt(dev, 2, 5, Tp=MEM + 6)
    kw = dict(input_ids=ids, max_length=MEM + 30, penalty_alpha=0.6, top_k=4, eos_token_id=EOS_NEVER, pad_token_id=0)
    want, got = _both(plain, **kw)
    assert want.shape == (2, MEM + 30) and torch.equal(got, want)
    assert torch.equal(plain.generate(**kw, contrastive_rings='shared', use_graph=False), want)


def test_a_sequence_that_finishes_while_another_runs_on(plain, dev):
    ids = _prompt(dev, 3, 8)
    kw = dict(input_ids=ids, max_length=L, penalty_alpha=0.6, top_k=4, pad_token_id=0)
    free = plain.generate(**kw, eos_token_id=EOS_NEVER)
    eos = int(free[0, TP + 20])                                        # a token sequence 0 emits part of the way in
    want, got = _both(plain, **kw, eos_token_id=eos)
    ends = [(row[TP:] == eos).nonzero()[:1].flatten().tolist() for row in want]
    assert ends[0] and len({tuple(e) for e in ends}) > 1, 'the sequences were meant to finish at different steps, or not at all'
    assert torch.equal(got, want)
    assert torch.equal(plain.generate(**kw, eos_token_id=eos, contrastive_rings='shared', use_graph=False), want)


def test_shared_then_copied_then_shared_on_one_model(plain, dev):
    """the stale-graph case: the ring mode is part of the capture key, and no call leaves the next one a decoder of the other mode"""
    ids = _prompt(dev, 2, 21)
    kw = dict(input_ids=ids, max_length=L, penalty_alpha=0.6, top_k=4, eos_token_id=EOS_NEVER, pad_token_id=0)
    a = plain.generate(**kw, contrastive_rings='shared')
    b = plain.generate(**kw, contrastive_rings='copied')
    c = plain.generate(**kw, contrastive_rings='shared')
    assert torch.equal(a, b) and torch.equal(c, b)
    # one decoder object, two searches: the second replays the graph captured by the first
    dec = XLDecoder(plain.engine, 2 * 4, L, shared_rings=4)
    args = dict(top_k=4, penalty_alpha=0.6, eos_token_id=EOS_NEVER, pad_token_id=0, contrastive_rings='shared')
    first = contrastive_search_device(dec, ids, L, **args)
    again = contrastive_search_device(dec, _prompt(dev, 2, 22), L, **args)
    assert torch.equal(first, b) and torch.equal(again, plain.generate(**{**kw, 'input_ids': _prompt(dev, 2, 22)}))
    with pytest.raises(ValueError, match='built for the other ring mode'):
        contrastive_search_device(dec, ids, L, **{**args, 'contrastive_rings': 'copied'})
    with pytest.raises(ValueError, match='built for the other ring mode'):
        contrastive_search_device(XLDecoder(plain.engine, 2 * 4, L), ids, L, **args)


def test_grammar_with_bar_budget_and_key_under_shared_rings(dev):
    from tests.test_key_rule_gpu import EOS, FULL_BAR, PAD, RULE, TOK, _model, _prompts
    m = _model(dev, 614, closing_bias=4.0)
    ids, _ = _prompts(3, dev, FULL_BAR, keyless=False)
    W = ids.shape[1] + 40
    g = TOK.grammar(bar_budget=True)
    kw = dict(input_ids=ids, max_length=W, top_k=4, penalty_alpha=0.6, eos_token_id=EOS, pad_token_id=PAD, grammar=g, in_key=RULE)
    want, got = _both(m, **kw)
    assert torch.equal(got, want) and (want[:, ids.shape[1]:] == EOS).any()
    assert torch.equal(m.generate(**kw, contrastive_rings='shared', use_graph=False), want)
    # the grammar given as the tokenizer's plain form, and a key named by the call
    kw2 = dict(kw, grammar=TOK.grammar(), key='GMajor')
    want2, got2 = _both(m, **kw2)
    assert torch.equal(got2, want2)


def test_register_alone_under_shared_rings(dev):
    from tests.test_register_rule_gpu import BASS_RANGE, MELODY_RANGE, REG, STOP, _model, _prompts
    m = _model(dev, 716)
    ids = _prompts(3, dev)
    kw = dict(input_ids=ids, max_length=ids.shape[1] + 30, top_k=4, penalty_alpha=0.6, register=REG, melody_range=MELODY_RANGE,
              bass_range=BASS_RANGE, bass_below=1, **STOP)
    want, got = _both(m, **kw)
    assert torch.equal(got, want)


def test_the_decoder_holds_one_ring_per_prompt_and_the_prompt_pass_one_row(plain, dev, monkeypatch):
    made, passes = [], []
    real = G.XLDecoder

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(G, 'XLDecoder', Spy)
    forward = plain.engine.forward
    monkeypatch.setattr(plain.engine, 'forward', lambda x, *a, **k: (passes.append(tuple(x.shape)), forward(x, *a, **k))[1])
    B0, K = 3, 4
    ids = _prompt(dev, B0, 31)
    kw = dict(input_ids=ids, max_length=TP + 10, penalty_alpha=0.6, top_k=K, eos_token_id=EOS_NEVER, pad_token_id=0)
    want = plain.generate(**kw)
    got = plain.generate(**kw, contrastive_rings='shared')
    assert torch.equal(got, want)
    copied, shared = made
    assert copied.shared_K == 0 and shared.shared_K == K and copied.B == shared.B == B0 * K
    for a, b in zip(copied.kc + copied.vc, shared.kc + shared.vc):
        assert a.shape == (B0 * K, *a.shape[1:]) and b.shape == (B0, *a.shape[1:])
    numel = lambda d: sum(t.numel() for t in d.kc + d.vc)
    assert numel(shared) * K == numel(copied)
    assert shared.stash.shape == (2, B0 * K, 2 * plain.config.d_model) and shared.logp.shape[0] == B0 * K
    assert passes == [(B0 * K, TP), (B0, TP)], 'the prompt pass of the shared mode runs once per prompt'
    # MXL_CONTRASTIVE_RINGS sets the default of a call without the keyword, and is ignored where the mode does not apply
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'shared')
    del made[:]
    assert torch.equal(plain.generate(**kw), want) and made[0].shared_K == K
    assert torch.equal(plain.generate(**kw, contrastive_rings='copied'), want) and made[1].shared_K == 0
    sample = dict(input_ids=ids, max_length=TP + 10, do_sample=True, top_k=8, seed=5)
    plain._decoder = None
    drawn = plain.generate(**sample)
    monkeypatch.delenv('MXL_CONTRASTIVE_RINGS')
    plain._decoder = None
    assert torch.equal(plain.generate(**sample), drawn)
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'sharedd')
    with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
        plain.generate(**kw)
