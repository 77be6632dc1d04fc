"""Sampling n variations of a prompt over prompt rings, end to end on TransfoXL: `generate(do_sample=True, num_return_sequences=n,
prompt_rings='shared')` against the default mode of the same call with the same seed.  The model is
tests/test_contrastive_shared_generate_gpu.py's (2 layers, mem_len 64, init_std 0.4); at that mem_len both modes run the ring in one
piece, so the attention output of every row is the copied mode's bit for bit (tests/test_prefix_rings_ops_gpu.py), the draw is keyed by
(seed, row, step), and the ids are held to torch.equal -- no tolerance.  Every call starts from a fresh decoder (a kept decoder carries
its draw counter on).  At most 27 rows, so one lane, except in the lanes case."""
import pytest
import torch

from symbolic_music_generation_amd import generate as G
from symbolic_music_generation_amd._lib import MusicXLError
from symbolic_music_generation_amd.generate import XLDecoder

pytestmark = pytest.mark.gpu

SEED, INIT_STD, TP, L, MEM = 3, 0.4, 12, 92, 64          # L > MEM + TP: the generation runs across the wrap of the ring
SAMPLE = dict(do_sample=True, top_k=8)


@pytest.fixture(scope='module')
def plain(dev):
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=MEM, max_length=L, seed=SEED, init_std=INIT_STD)
    return m.eval()


def _prompt(dev, n, seed, Tp=TP):
    return torch.randint(4, 1190, (n, Tp), generator=torch.Generator().manual_seed(seed)).to(dev)


def _fresh(m, **kw):
    m._decoder = None
    return m.generate(**kw)


def _both(m, **kw):
    """the call in the default mode and over prompt rings, each on a fresh decoder"""
    return _fresh(m, **kw), _fresh(m, **kw, prompt_rings='shared')


def _decoders(m):
    return getattr(m._decoder, 'lanes', [m._decoder])


@pytest.mark.parametrize('B0', [1, 3])
@pytest.mark.parametrize('n', [2, 5, 9])
def test_prompt_rings_return_the_ids_of_the_default_mode(plain, dev, n, B0):
    ids = _prompt(dev, B0, 10 * n + B0)
    kw = dict(input_ids=ids, max_length=L, seed=11, **SAMPLE, num_return_sequences=n)
    want, got = _both(plain, **kw)
    assert want.shape == (B0 * n, L) and torch.equal(got, want), (got != want).nonzero()[:4].tolist()
    assert len({tuple(r) for r in want[:n, TP:].tolist()}) == n                # (the variations of a prompt differ)
    # the layout: one pair of prompt rings per prompt, one pair of tail rings per row, of the stated length
    dec, c = plain._decoder, plain.config
    Mt = min(MEM, (L - TP + 15) // 16 * 16)
    assert dec.prompt_n == n and dec.B == B0 * n and len(dec.kc) == len(dec.kt) == c.n_layer
    for ring in dec.kc + dec.vc:
        assert ring.shape == (B0, c.n_head, MEM, c.d_head)
    for ring in dec.kt + dec.vt:
        assert ring.shape == (B0 * n, c.n_head, Mt, c.d_head)
    assert int(dec.t0_dev) == TP


def test_eager_steps_and_a_short_tail(plain, dev):
    ids = _prompt(dev, 2, 77)
    kw = dict(input_ids=ids, max_length=TP + 21, seed=5, **SAMPLE, num_return_sequences=5)
    want, got = _both(plain, **kw)
    assert torch.equal(got, want)
    assert plain._decoder.kt[0].shape == (10, plain.config.n_head, 32, plain.config.d_head)   # 21 generated positions: Mt = 32 < mem_len
    assert torch.equal(_fresh(plain, **kw, prompt_rings='shared', use_graph=False), want)
    long = dict(kw, max_length=L)
    assert torch.equal(_fresh(plain, **long, prompt_rings='shared', use_graph=False), _fresh(plain, **long))


def test_a_prompt_longer_than_the_ring(plain, dev):
    ids = _prompt(dev, 2, 5, Tp=MEM + 6)
    kw = dict(input_ids=ids, max_length=MEM + 40, seed=9, **SAMPLE, num_return_sequences=3)
    want, got = _both(plain, **kw)
    assert want.shape == (6, MEM + 40) and torch.equal(got, want)
    assert torch.equal(_fresh(plain, **kw, prompt_rings='shared', use_graph=False), want)


def test_rows_of_one_prompt_that_finish_at_different_steps(plain, dev):
    ids = _prompt(dev, 2, 8)
    kw = dict(input_ids=ids, max_length=L, seed=21, **SAMPLE, num_return_sequences=5, pad_token_id=0)
    free = _fresh(plain, **kw)
    eos = int(free[0, TP + 15])                                        # a token row 0 emits part of the way in
    want, got = _both(plain, **kw, eos_token_id=eos)
    ends = [(row[TP:] == eos).nonzero()[:1].flatten().tolist() for row in want[:5]]
    assert ends[0] and len({tuple(e) for e in ends}) > 1, 'the rows of prompt 0 were meant to finish at different steps, or not at all'
    assert torch.equal(got, want)
    assert torch.equal(_fresh(plain, **kw, eos_token_id=eos, prompt_rings='shared', use_graph=False), want)


def test_two_left_padded_prompts_of_different_lengths(plain, dev):
    a, b = _prompt(dev, 1, 31, Tp=TP)[0], _prompt(dev, 1, 32, Tp=TP - 5)[0]
    ids, mask = G.left_pad([a, b], 0)
    kw = dict(input_ids=ids.to(dev), attention_mask=mask.to(dev), max_length=L, seed=13, **SAMPLE, num_return_sequences=4)
    want, got = _both(plain, **kw)
    assert want.shape == (8, L) and torch.equal(got, want)
    assert torch.equal(got[4:, :5], ids[1:, :5].to(dev).expand(4, 5))          # the pad columns come back as given


def test_shared_then_copied_then_shared_on_one_model(plain, dev):
    """the stale-graph case: the ring mode is part of the capture key, and no call leaves the next one a decoder of the other mode"""
    ids = _prompt(dev, 2, 21)
    kw = dict(input_ids=ids, max_length=L, seed=4, **SAMPLE, num_return_sequences=3)
    plain._decoder = None
    a = plain.generate(**kw, prompt_rings='shared')
    b = plain.generate(**kw, prompt_rings='copied')
    c = plain.generate(**kw, prompt_rings='shared')
    assert torch.equal(a, b) and torch.equal(c, b)
    # one decoder object, two generations with prompts of two lengths: the second replays the graph captured by the first (the prompt
    # length is step state, t0_dev)
    sampling = G.sampling_config(True, 8, None, 1.0, None, None)
    dec = XLDecoder(plain.engine, 6, L, seed=4, prompt_rings=3)
    first = dec.run(ids.repeat_interleave(3, 0), L, sampling)
    assert torch.equal(first, b)
    graph = dec.graph
    short = _prompt(dev, 2, 22, Tp=TP - 3)
    again = dec.run(short.repeat_interleave(3, 0), L, sampling)
    assert dec.graph is graph and int(dec.t0_dev) == TP - 3
    ref = XLDecoder(plain.engine, 6, L, seed=4)
    ref.run(ids.repeat_interleave(3, 0), L, sampling)                          # (the draw counter moves with the generations)
    assert torch.equal(again, ref.run(short.repeat_interleave(3, 0), L, sampling))
    # a decoder of this mode takes sampling alone, rows in prompt order, and no more positions than its tails hold
    with pytest.raises(MusicXLError, match='serves sampling alone'):
        dec.beam_begin(ids.repeat_interleave(3, 0), L, 3, 1, 0, 1.0, True)
    with pytest.raises(MusicXLError, match='every prompt 3 times in a row'):
        dec.run(_prompt(dev, 6, 23), L, sampling)
    with pytest.raises(MusicXLError, match='tail rings of this decoder hold 16 generated positions'):
        XLDecoder(plain.engine, 6, L, prompt_rings=3, tail_len=10).run(ids.repeat_interleave(3, 0), TP + 30, sampling)


def test_grammar_with_bar_budget_bar_count_and_key_under_prompt_rings(dev):
    from tests.test_key_rule_gpu import EOS, FULL_BAR, PAD, RULE, TOK, _model, _prompts
    m = _model(dev, 614, closing_bias=4.0)
    ids, _ = _prompts(3, dev, FULL_BAR, keyless=False)
    W = ids.shape[1] + 60
    kw = dict(input_ids=ids, max_length=W, seed=6, **SAMPLE, num_return_sequences=4, eos_token_id=EOS, pad_token_id=PAD,
              grammar=TOK.grammar(bar_budget=True), n_bars=2, in_key=RULE)
    want, got = _both(m, **kw)
    assert torch.equal(got, want) and (want[:, ids.shape[1]:] == EOS).any()
    assert torch.equal(_fresh(m, **kw, prompt_rings='shared', use_graph=False), want)


def test_lanes_cut_between_prompts(plain, dev):
    """4 prompts x 8 variations, 32 rows: two lanes in both modes, and the default's half-batch cut falls between two prompts"""
    ids = _prompt(dev, 4, 41)
    kw = dict(input_ids=ids, max_length=TP + 40, seed=8, **SAMPLE, num_return_sequences=8)
    want, got = _both(plain, **kw)
    assert want.shape == (32, TP + 40) and torch.equal(got, want)
    lanes = _decoders(plain)
    assert len(lanes) == 2 and all(d.prompt_n == 8 and d.B == 16 and d.kc[0].shape[0] == 2 and d.kt[0].shape[0] == 16 for d in lanes)
    # one prompt: one lane, whatever the row count
    _fresh(plain, input_ids=ids[:1], max_length=TP + 8, seed=8, **SAMPLE, num_return_sequences=33, prompt_rings='shared')
    assert isinstance(plain._decoder, XLDecoder) and plain._decoder.kc[0].shape[0] == 1 and plain._decoder.B == 33


def test_the_prompt_pass_runs_once_per_prompt_and_the_knob(plain, dev, monkeypatch):
    passes = []
    forward = plain.engine.forward
    monkeypatch.setattr(plain.engine, 'forward', lambda x, *a, **k: (passes.append(tuple(x.shape)), forward(x, *a, **k))[1])
    B0, n = 3, 4
    ids = _prompt(dev, B0, 31)
    kw = dict(input_ids=ids, max_length=TP + 10, seed=2, **SAMPLE, num_return_sequences=n)
    want, got = _both(plain, **kw)
    assert torch.equal(got, want)
    assert passes == [(B0 * n, TP), (B0, TP)], 'the prompt pass of the shared mode runs once per prompt'
    shared = plain._decoder
    numel = lambda d: sum(t.numel() for t in d.kc + d.vc + d.kt + d.vt)
    assert numel(shared) * MEM == 2 * 2 * shared.kc[0][0].numel() * (B0 * MEM + B0 * n * 16)     # 10 generated positions: Mt = 16
    # MXL_PROMPT_RINGS sets the default of a call without the keyword, and is ignored where the mode does not apply
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'shared')
    assert torch.equal(_fresh(plain, **kw), want) and plain._decoder.prompt_n == n
    assert torch.equal(_fresh(plain, **kw, prompt_rings='copied'), want) and plain._decoder.prompt_n == 0
    one = dict(input_ids=ids, max_length=TP + 10, seed=2, **SAMPLE)
    drawn = _fresh(plain, **one)
    assert plain._decoder.prompt_n == 0
    monkeypatch.delenv('MXL_PROMPT_RINGS')
    assert torch.equal(_fresh(plain, **one), drawn)
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'sharedd')
    with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
        plain.generate(**kw)


def test_refusals(plain, dev):
    ids = _prompt(dev, 2, 51)
    base = dict(input_ids=ids, max_length=TP + 6)
    with pytest.raises(ValueError, match="prompt_rings='prefix': expected None, 'copied' or 'shared'"):
        plain.generate(**base, **SAMPLE, num_return_sequences=3, prompt_rings='prefix')
    serves = "prompt_rings='shared' serves sampling with num_return_sequences >= 2"
    stop = dict(eos_token_id=1, pad_token_id=0)
    for arm in (SAMPLE, dict(SAMPLE, num_return_sequences=1), dict(), dict(num_beams=2, **stop),
                dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.0, **stop),
                dict(num_beams=2, do_sample=True, renormalize_logits=True, num_return_sequences=2, **stop),
                dict(num_beams=2, do_sample=True, renormalize_logits=True, device_scorer=True, **stop),
                dict(penalty_alpha=0.6, top_k=4), dict(SAMPLE, num_return_sequences=3, kv_cache_dtype='fp8')):
        with pytest.raises(ValueError, match=serves):
            plain.generate(**base, **arm, prompt_rings='shared')
    with pytest.raises(ValueError):
        XLDecoder(plain.engine, 6, L, prompt_rings=3, kv_dtype='fp8')
    with pytest.raises(MusicXLError, match='2 or more rows per prompt'):
        XLDecoder(plain.engine, 7, L, prompt_rings=3)


def test_a_model_the_attention_does_not_take(dev):
    from tests.test_xl_model_gpu import _pair
    _, odd = _pair(dev, n_layer=1, mem_len=72, max_length=40, seed=SEED, init_std=INIT_STD)
    ids = _prompt(dev, 1, 3)
    kw = dict(input_ids=ids, max_length=TP + 4, **SAMPLE, num_return_sequences=2)
    with pytest.raises(MusicXLError, match='mem_len that is a multiple of 16, not 72'):
        odd.eval().generate(**kw, prompt_rings='shared')
    assert odd.generate(**kw).shape == (2, TP + 4)
