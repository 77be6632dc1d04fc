"""`generate(..., beam_rings='indexed_fp8')` end to end: the device beam searches over FP8 K/V rings that are never moved and are read
through the owner table (mxl_relattn_decode_fp8_owned).  The 2-layer model, the prompts and the constants of
tests/test_beam_indexed_gpu.py: mem_len = 32, a prompt of 12 and max_length = 80, so the ring wraps while beams are live.

The reference is the same search on one FP8 decoder with `beam_rings='copied', use_graph=False`: XLDecoder's reference mode, which moves
bytes and exponents with torch.index_select.  Ids and scores under 'indexed' must equal it exactly (the kernel gives the bits of
mxl_relattn_decode_fp8 on gathered rings, tests/test_beam_fp8_owned_ops_gpu.py), and the public call must return the decoder-level
result.  Against bf16 rings nothing is asserted but finite scores: K and V are rounded to four significant bits, the difference of the
best hypothesis's score per prompt is printed.  On the commit before the feature every call here raises ValueError (FP8 rings under a
search, an unknown mode)."""
import pytest
import torch

from symbolic_music_generation_amd import generate as G
from symbolic_music_generation_amd._lib import MusicXLError
from tests.test_beam_indexed_gpu import EOS_EMITTED, EOS_NEVER, L, MEM, TP, _Modes, plain  # noqa: F401  (plain: a fixture)

pytestmark = pytest.mark.gpu


def _fp8(m, rows, **kw):
    return G.XLDecoder(m.engine, rows, L, kv_dtype='fp8', **kw)


def _held(search, dec, prompt, use_graph, **kw):
    """the search on `dec` in the reference mode, then under 'indexed' -> (ids, scores) of the latter, after holding it to the former"""
    want, w_sc = search(dec, prompt, L, return_scores=True, beam_rings='copied', **dict(kw, use_graph=False))
    got, g_sc = search(dec, prompt, L, return_scores=True, beam_rings='indexed', **dict(kw, use_graph=use_graph))
    assert dec.beam_rings == 'indexed' and dec.kv_dtype == 'fp8'
    assert torch.equal(got, want) and torch.equal(g_sc, w_sc), (kw, g_sc.tolist(), w_sc.tolist())
    assert torch.isfinite(g_sc).all()
    return got, g_sc


def _public(m, modes, want, **kw):
    got = m.generate(beam_rings='indexed_fp8', **kw)
    dec = modes.decoders[-1]
    assert dec.beam_rings == 'indexed' and dec.kv_dtype == 'fp8' and dec.owner is not None
    assert got.shape == want.shape and torch.equal(got, want), kw
    return dec


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('early', [True, False])
@pytest.mark.parametrize('nb', [2, 3])
def test_plain_beam(plain, monkeypatch, nb, early, use_graph):
    m, prompt = plain
    modes, fired = _Modes(monkeypatch), 0
    dh = m.config.d_head
    for eos in (EOS_EMITTED, EOS_NEVER):
        kw = dict(num_beams=nb, early_stopping=early, num_return_sequences=2, eos_token_id=eos, pad_token_id=0)
        dec = _fp8(m, 2 * nb)
        got, g_sc = _held(G.beam_search_device, dec, prompt, use_graph, **kw)
        if eos == EOS_NEVER:
            assert got.shape[1] == L and dec.steps_run == L - TP - 1 > 2 * MEM - TP        # the ring wrapped with every beam live
            foreign = (dec.owner.cpu() != (torch.arange(2 * nb) % nb)[:, None]).float().mean().item()
            print(f'fp8 plain beam nb {nb} early {early} graph {use_graph}: {100 * foreign:.0f} % of the last window is held by a sibling')
            assert foreign > 0.1                                       # beams moved: the table is what the attention read through
            assert all(r.dtype == torch.uint8 for r in dec.kc + dec.vc) and all(e.dtype == torch.int8 for e in dec.ke + dec.ve)
            bf = G.XLDecoder(m.engine, 2 * nb, L)
            size = lambda rings: sum(r.numel() * r.element_size() for r in rings)
            assert size(dec.kc + dec.vc + dec.ke + dec.ve) * 2 * dh == size(bf.kc + bf.vc) * (dh + 1)      # (dh + 1) / (2 dh) of the bytes
            b_ids, b_sc = G.beam_search_device(bf, prompt, L, return_scores=True, beam_rings='indexed', use_graph=use_graph, **kw)
            assert torch.isfinite(b_sc).all() and torch.isfinite(g_sc).all()
            best = (g_sc[::2] - b_sc[::2]).abs()                       # (two hypotheses per prompt, the best first)
            print(f'fp8 against bf16 indexed rings, nb {nb} early {early} graph {use_graph}: best-hypothesis score differs by '
                  f'{[round(x, 5) for x in best.tolist()]} (scores {[round(x, 4) for x in g_sc[::2].tolist()]} against '
                  f'{[round(x, 4) for x in b_sc[::2].tolist()]}), largest {best.max().item():.3e}; '
                  f'{int((got != b_ids).any(1).sum())} of {got.shape[0]} returned rows differ in an id')
        fired += int((got[:, TP:] == eos).any())
        _public(m, modes, got, input_ids=prompt, max_length=L, use_graph=use_graph, **kw)
    assert fired == 1


@pytest.mark.parametrize('use_graph', [True, False])
def test_group_beam(plain, monkeypatch, use_graph):
    m, prompt = plain
    modes = _Modes(monkeypatch)
    monkeypatch.setenv('MXL_GROUP_BEAM_DEVICE', '1')
    for eos in (EOS_EMITTED, EOS_NEVER):
        kw = dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.5, early_stopping=True, eos_token_id=eos, pad_token_id=0)
        got, _ = _held(G.group_beam_search_device, _fp8(m, 8), prompt, use_graph, **kw)
        _public(m, modes, got, input_ids=prompt, max_length=L, use_graph=use_graph, **kw)


@pytest.mark.parametrize('use_graph', [True, False])
def test_beam_sample(plain, monkeypatch, use_graph):
    m, prompt = plain
    modes = _Modes(monkeypatch)
    kw = dict(num_beams=3, early_stopping=True, top_k=0, eos_token_id=EOS_NEVER, pad_token_id=0)
    got, _ = _held(G.beam_sample_device, _fp8(m, 6, seed=5), prompt, use_graph, **kw)
    _public(m, modes, got, input_ids=prompt, max_length=L, use_graph=use_graph, do_sample=True, renormalize_logits=True, device_scorer=True,
            seed=5, **kw)


def test_rules_under_indexed_fp8_rings(dev, monkeypatch):
    """the grammar with its bar budget and the key rule: the rule words follow the beams inside mxl_beam_step, whatever the rings are"""
    from tests.test_key_rule_gpu import EOS, FULL_BAR, PAD, RULE, TOK, _prompts
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=MEM, max_length=L, seed=601)
    m.eval()
    ids, _ = _prompts(2, dev, FULL_BAR, keyless=False)
    modes = _Modes(monkeypatch)
    kw = dict(num_beams=3, early_stopping=False, eos_token_id=EOS, pad_token_id=PAD, grammar=TOK.grammar(bar_budget=True), in_key=RULE)
    got, _ = _held(G.beam_search_device, _fp8(m, 6), ids, True, **kw)
    dec = _public(m, modes, got, input_ids=ids, max_length=L, **kw)
    print('rules under indexed fp8 rings: prompt', ids.shape[1], 'returned', tuple(got.shape), 'steps', dec.steps_run)


def test_two_calls_in_a_row_and_the_environment_default(plain, monkeypatch):
    """one FP8 decoder, two beam counts: the table is reset and rebuilt per beam_begin and the beam count is part of the graph key; a
    greedy generation on the used decoder reads every row's own ring again; MXL_BEAM_RINGS=indexed_fp8 without the keyword takes the
    path, and is ignored where it does not apply"""
    m, prompt = plain
    kw = dict(early_stopping=True, eos_token_id=EOS_NEVER, pad_token_id=0)
    prompts = torch.cat([prompt, prompt[:1].flip(1)])
    dec, other, keys = _fp8(m, 6), _fp8(m, 6), []
    for nb in (3, 2):
        want = G.beam_search_device(other, prompts[:6 // nb], L, num_beams=nb, beam_rings='copied', use_graph=False, **kw)
        got = G.beam_search_device(dec, prompts[:6 // nb], L, num_beams=nb, beam_rings='indexed', use_graph=True, **kw)
        assert dec.beam_rings == 'indexed' and torch.equal(got, want), nb
        keys.append(dec._graph_key)
        assert dec.owner.shape == (6, MEM) and int(dec.owner.max()) == nb - 1      # rebuilt for this beam count
    assert keys[0] != keys[1], keys
    twice = prompts.repeat(2, 1)
    greedy = dec.generate(twice, L, use_graph=True)                    # greedy on the used decoder: every row reads its own ring again
    assert dec.beam_rings == 'copied'
    assert torch.equal(greedy, _fp8(m, 6).generate(twice, L, use_graph=True))

    modes = _Modes(monkeypatch)
    call = dict(input_ids=prompt, max_length=L, num_beams=2, use_graph=True, **kw)
    want = m.generate(beam_rings='indexed_fp8', **call)
    monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed_fp8')
    assert torch.equal(m.generate(**call), want) and modes.last() == 'indexed' and modes.decoders[-1].kv_dtype == 'fp8'
    m.generate(beam_rings='copied', **call)
    assert modes.last() == 'copied' and modes.decoders[-1].kv_dtype is None
    assert m.generate(input_ids=prompt, max_length=TP + 4).shape == (2, TP + 4)    # the default is ignored where it does not apply
    monkeypatch.delenv('MXL_BEAM_RINGS')
    with pytest.raises(ValueError, match="beam_rings='indexed_fp8' serves"):
        m.generate(input_ids=prompt, max_length=TP + 4, beam_rings='indexed_fp8')


def test_refusals(plain):
    m, prompt = plain
    kw = dict(num_beams=2, eos_token_id=EOS_NEVER, pad_token_id=0)
    dec = _fp8(m, 4)
    with pytest.raises(MusicXLError, match='index_select'):            # the reference mode is eager only
        G.beam_search_device(dec, prompt, L, beam_rings='copied', use_graph=True, **kw)
    with pytest.raises(ValueError, match="expected 'copied' or 'indexed'"):
        G.beam_search_device(dec, prompt, L, beam_rings='indexed_fp8', **kw)       # the decoder's modes are two; fp8 is how it was built
    with pytest.raises(ValueError, match='fp8 K/V rings'):
        dec.beam_prefill(prompt.repeat_interleave(2, 0))
    with pytest.raises(ValueError, match='fp8 K/V rings'):
        dec.contrastive_begin(prompt.repeat_interleave(2, 0), L, 2, 0.6, None, 0)
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8' is not supported under beam search"):
        m.generate(input_ids=prompt, max_length=L, beam_rings='indexed_fp8', kv_cache_dtype='fp8', **kw)
