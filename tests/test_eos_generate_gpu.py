"""Stopping at eos in batched greedy decoding and sampling (`generate(eos_token_id=...)`, HF greedy_search / sample).  Rows are
independent and draws are per (seed, row, step), so a run with eos equals the run without it post-processed by
`generate.finish_at_eos` (pad after each row's first generated eos, cut to the longest row): that equality is checked with
torch.equal on every path -- fused and unfused samplers, the large-vocabulary sampler, graph and eager, lanes, padded prompts,
the Reformer decoder."""
import pytest
import torch

from symbolic_music_generation_amd.generate import finish_at_eos

pytestmark = pytest.mark.gpu

V = 1190
NEAR_TIE = 5e-2


def _model(dev, seed, head_bias=None, **kw):
    """the test pair of tests/test_xl_model_gpu.py.  Its greedy rows repeat their first generated token for ever (tied head);
    head_bias = s draws the head's bias with standard deviation s, so that rows settle on a few tokens that they share"""
    from tests.test_xl_model_gpu import _pair
    kw.setdefault('max_length', 160)
    ref, m = _pair(dev, n_layer=2, mem_len=64, seed=seed, **kw)
    if head_bias:
        with torch.no_grad():
            b = ref.crit.out_layers[0].bias
            b.copy_((torch.randn(b.shape, generator=torch.Generator().manual_seed(seed)) * head_bias).to(torch.bfloat16).float())
        m.load_state_dict(ref.state_dict())
    return ref, m


def _prompts(B, Tp, seed, vocab=V):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(4, vocab, (B, Tp), generator=g)


def _first_cols(gen, tok):
    """column (within gen) of each row's first `tok`, or None"""
    out = []
    for r in gen.tolist():
        out.append(r.index(tok) if tok in r else None)
    return out


def _pick_eos(full, Tp, mode):
    """an id of the generated part of a run without eos.  mode 'spread': rows finish at two or more different columns and at
    least one row never does; 'some': some rows finish, some never; 'all': every row has it (then the one whose last
    first-occurrence is earliest)"""
    gen = full[:, Tp:].cpu()
    best = None
    for tok in torch.unique(gen).tolist():
        cols = _first_cols(gen, tok)
        hit = [c for c in cols if c is not None]
        if mode == 'spread' and len(set(hit)) >= 2 and len(hit) < len(cols):
            return tok
        if mode == 'some' and 0 < len(hit) < len(cols):
            return tok
        if mode == 'all' and len(hit) == len(cols) and (best is None or max(hit) < best[1]):
            best = (tok, max(hit))
    return None if best is None else best[0]


def _dgen(dec, *a, **kw):
    """a decoder's generate from the start of its random stream: the draw counter carries on from one call to the next"""
    for d in getattr(dec, 'lanes', [dec]):
        d.rng.zero_()
    return dec.generate(*a, **kw)


def _mgen(m, **kw):
    """model.generate with a fresh decoder (see _dgen)"""
    m._decoder = None
    return m.generate(**kw)


def _pick_any(full, Tp):
    eos = _pick_eos(full, Tp, 'all')
    return _pick_eos(full, Tp, 'spread') if eos is None else eos


def test_ring_attention_skips_finished_rows(dev):
    """mxl_relattn_decode_split_live: live rows bit-identical to the unmasked launch, finished rows' slices zero; pieces 1 and 4,
    launches back to back (a finished row must leave the pieces' arrival counters as they were)"""
    from symbolic_music_generation_amd import ops
    torch.manual_seed(0)
    B, H, dh, M = 6, 4, 64, 1024
    d = H * dh
    bf = dict(device=dev, dtype=torch.bfloat16)
    qkv = torch.randn(B, 3 * d, **bf)
    kc, vc = torch.randn(B, H, M, dh, **bf), torch.randn(B, H, M, dh, **bf)
    rd = torch.randn(M, d, **bf) * 0.1
    rwb, rrb = torch.randn(H, dh, device=dev) * 0.1, torch.randn(H, dh, device=dev) * 0.1
    t_dev = torch.tensor([1500], device=dev, dtype=torch.int32)
    qr, bd = torch.empty(B, d, **bf), torch.empty(B, H, M, device=dev, dtype=torch.float32)
    live = torch.tensor([1, 0, 1, 1, 0, 0], device=dev, dtype=torch.int32)
    for pieces in (1, 4):
        split = ops.relattn_decode_split_scratch(B, H, dh, pieces, dev)

        def run(unfinished):
            out = torch.full((B, d), float('nan'), **bf)
            ops.relattn_decode(qkv, kc, vc, rd, rwb, rrb, out, t_dev, H, dh, qr, bd, split=split, pieces=pieces,
                               unfinished=unfinished)
            return out
        ref = run(None)
        a = run(live)
        b = run(live)
        ref2 = run(None)
        allon = run(torch.ones_like(live))
        torch.cuda.synchronize()
        keep = live.bool()
        for got in (a, b):
            assert torch.equal(got[keep], ref[keep]), pieces
            assert (got[~keep] == 0).all(), pieces
        assert torch.equal(ref2, ref) and torch.equal(allon, ref), pieces
        assert not torch.isnan(ref).any()
        if split is not None:
            assert (split[1] == 0).all()


def test_greedy_rows_stop_at_eos(dev):
    """greedy: some rows finish, the others run to max_length (greedy rows of these small models settle on one token at once,
    so they cannot finish at different columns: the sampling tests below cover that)"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 80, head_bias=3.0)
    m.eval()
    B, Tp, L = 6, 8, 120
    ids = _prompts(B, Tp, 81).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=3)
    for kw in (dict(do_sample=False), dict(do_sample=False, repetition_penalty=1.3)):
        full = _dgen(dec, ids, L, **kw)
        eos = _pick_eos(full, Tp, 'some')
        assert eos is not None
        want = finish_at_eos(full, Tp, eos, 1)
        got = _dgen(dec, ids, L, eos_token_id=eos, pad_token_id=1, **kw)
        assert got.shape == (B, L) and torch.equal(got, want)
        assert (got[:, -1] == 1).any() and (got[:, -1] != 1).any()
        # through the model; the default pad is eos (the TransfoXL config has none)
        assert torch.equal(_mgen(m, input_ids=ids, max_length=L, eos_token_id=eos, pad_token_id=1, **kw), want)
        assert torch.equal(_mgen(m, input_ids=ids, max_length=L, eos_token_id=eos, **kw), finish_at_eos(full, Tp, eos, eos))


def test_sampling_rows_stop_at_eos(dev):
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 82)
    m.eval()
    B, Tp, L = 6, 10, 100
    ids = _prompts(B, Tp, 83).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=9)
    for kw in (dict(top_k=8), dict(top_k=0, top_p=0.9, temperature=0.8), dict(top_k=20, typical_p=0.9),
               dict(top_k=30, repetition_penalty=1.2)):
        full = _dgen(dec, ids, L, do_sample=True, **kw)
        for mode in ('spread', 'all'):
            eos = _pick_eos(full, Tp, mode)
            if eos is None:
                continue
            got = _dgen(dec, ids, L, do_sample=True, eos_token_id=eos, pad_token_id=2, **kw)
            assert torch.equal(got, finish_at_eos(full, Tp, eos, 2)), (kw, mode)


def test_early_exit(dev):
    """every row finishes (a head bias makes the rows share tokens): the call returns narrower, after at most two chunks of
    steps beyond the last row's eos"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 83, head_bias=6.0)
    m.eval()
    B, Tp, L, k = 6, 10, 120, 4
    ids = _prompts(B, Tp, 84).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=9)
    for kw in (dict(top_k=8), dict(top_k=30, temperature=1.5)):
        full = _dgen(dec, ids, L, do_sample=True, **kw)
        eos = _pick_eos(full, Tp, 'all')
        assert eos is not None, kw
        got = _dgen(dec, ids, L, do_sample=True, eos_token_id=eos, pad_token_id=2, stop_chunk=k, **kw)
        W = got.shape[1]
        assert torch.equal(got, finish_at_eos(full, Tp, eos, 2)) and W < L, kw
        assert dec.steps_run <= (W - Tp) + 2 * k, (kw, W, dec.steps_run)
        print('early exit', kw, 'width', W, 'of', L, 'steps issued', dec.steps_run, 'of', L - Tp - 1)


def test_graph_and_eager(dev):
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 84)
    m.eval()
    B, Tp, L = 6, 8, 90
    ids = _prompts(B, Tp, 101).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=2)
    kw = dict(do_sample=True, top_k=8)
    full = _dgen(dec, ids, L, use_graph=False, **kw)
    assert torch.equal(full, _dgen(dec, ids, L, use_graph=True, **kw))
    eos = _pick_any(full, Tp)
    assert eos is not None
    want = finish_at_eos(full, Tp, eos, 5)
    for use_graph in (False, True, False):
        assert torch.equal(_dgen(dec, ids, L, use_graph=use_graph, eos_token_id=eos, pad_token_id=5, **kw), want), use_graph


def test_lanes(dev):
    """B = 32 through model.generate takes two lanes, which stop on their own"""
    ref, m = _model(dev, 84)
    m.eval()
    B, Tp, L = 32, 6, 110
    ids = _prompts(B, Tp, 85).to(dev)
    kw = dict(do_sample=True, top_k=8)
    m._decoder = None
    full = _mgen(m, input_ids=ids, max_length=L, **kw)
    assert type(m._decoder).__name__ == 'XLDecoderLanes'
    eos = _pick_any(full, Tp)
    assert eos is not None
    want = finish_at_eos(full, Tp, eos, 5)
    out = _mgen(m, input_ids=ids, max_length=L, eos_token_id=eos, pad_token_id=5, **kw)
    assert torch.equal(out, want)
    lanes = m._decoder
    print('lane steps', [d.steps_run for d in lanes.lanes], 'width', out.shape[1])
    # each lane alone: its own width, its rows right-filled with pad up to the common one
    for i, d in enumerate(lanes.lanes):
        rows = slice(lanes.offs[i], lanes.offs[i + 1])
        w = finish_at_eos(full[rows], Tp, eos, 5).shape[1]
        assert (out[rows, w:] == 5).all()
    eos = _pick_eos(full, Tp, 'spread')
    if eos is not None:
        out = _mgen(m, input_ids=ids, max_length=L, eos_token_id=eos, pad_token_id=5, **kw)
        assert torch.equal(out, finish_at_eos(full, Tp, eos, 5))


def test_padded_prompts_with_eos(dev):
    """left-padded prompts: the equality holds; per row, the same as the row alone with eos (pads stripped, right-filled with pad
    beyond its own width) wherever the runs without eos agree; an eos inside a prompt does not finish the row"""
    from symbolic_music_generation_amd.generate import left_pad
    ref, m = _model(dev, 86, head_bias=3.0)
    m.eval()
    L = 90
    g = torch.Generator().manual_seed(87)
    prompts = [torch.randint(4, V, (n,), generator=g) for n in (5, 12, 20, 9, 14, 3)]
    for kw in (dict(do_sample=False), dict(do_sample=True, top_k=8)):
        ids, mask = left_pad(prompts, 0)
        full0 = _mgen(m, input_ids=ids.to(dev), attention_mask=mask.to(dev), max_length=L, **kw)
        Tp = ids.shape[1]
        eos = _pick_eos(full0, Tp, 'some')
        assert eos is not None
        ps = [p.clone() for p in prompts]
        ps[3][1] = eos                                             # an eos inside a prompt
        ids, mask = left_pad(ps, 0)
        ids, mask = ids.to(dev), mask.to(dev)
        full = _mgen(m, input_ids=ids, attention_mask=mask, max_length=L, **kw)
        got = _mgen(m, input_ids=ids, attention_mask=mask, max_length=L, eos_token_id=eos, pad_token_id=3, **kw)
        assert torch.equal(got, finish_at_eos(full, Tp, eos, 3))
        assert int(got[3, Tp]) != 3 or int(full[3, Tp]) == 3       # row 3 generates although its prompt holds eos
        if kw['do_sample']:
            continue                                               # (a row alone draws with another row index)
        checked = 0
        for b, p in enumerate(ps):
            s = Tp - len(p)
            one_full = _mgen(m, input_ids=p[None].to(dev), max_length=L - s, **kw)[0]
            if not torch.equal(one_full, full[b, s:]):
                continue                                           # a bf16 near-tie fork between batch shapes
            one = _mgen(m, input_ids=p[None].to(dev), max_length=L - s, eos_token_id=eos, pad_token_id=3, **kw)[0]
            row = got[b, s:]
            assert torch.equal(row[:one.numel()], one), b
            assert (row[one.numel():] == 3).all(), b
            checked += 1
        assert checked >= 4


def test_first_token_eos_replays_nothing(dev):
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 88)
    m.eval()
    B, Tp, L = 4, 7, 60
    ids = _prompts(1, Tp, 89).repeat(B, 1).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=3)
    first = int(_dgen(dec, ids, Tp + 1, do_sample=False)[0, Tp])
    out = _dgen(dec, ids, L, do_sample=False, eos_token_id=first)
    assert out.shape == (B, Tp + 1) and (out[:, Tp] == first).all() and torch.equal(out[:, :Tp], ids)
    assert dec.steps_run == 0


def _oracle_min_length(ref, prompt, L, eos, m_len):
    """HF greedy_search with MinLengthLogitsProcessor and eos stopping, over the fp32 oracle (one full forward per token)"""
    seq = prompt.clone()
    for cur in range(prompt.numel(), L):
        with torch.no_grad():
            lp = ref(seq[None]).prediction_scores[0, -1].float()
        if cur < m_len:
            lp[eos] = float('-inf')
        tok = int(lp.argmax())
        seq = torch.cat([seq, torch.tensor([tok])])
        if tok == eos:
            break
    return seq


def test_min_length(dev):
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 90)
    ref.eval(); m.eval()
    B, Tp, L = 3, 10, 40                                           # within the 64-slot ring: the oracle's full forward agrees
    ids = _prompts(B, Tp, 91)
    dec = XLDecoder(m.engine, B, L, seed=3)
    full = _dgen(dec, ids.to(dev), L, do_sample=False)
    eos = int(full[0, Tp])                                         # row 0 would stop at once
    m_len = Tp + 6
    got = _dgen(dec, ids.to(dev), L, do_sample=False, eos_token_id=eos, min_length=m_len).cpu()
    assert not (got[:, Tp:m_len] == eos).any()
    # min_length without eos: a no-op
    assert torch.equal(_mgen(m, input_ids=ids.to(dev), max_length=L, do_sample=False, min_length=m_len), full)

    def score_fn(b):
        def fn(prefix):
            with torch.no_grad():
                lp = ref(prefix[None]).prediction_scores[0, -1].float()
            if prefix.numel() < m_len:
                lp[eos] = float('-inf')
            return lp
        return fn
    for b in range(B):
        want = _oracle_min_length(ref, ids[b], L, eos, m_len)
        row = got[b, :want.numel()]
        mism = (row != want).nonzero()
        if mism.numel():
            t0 = int(mism[0, 0])
            top2 = score_fn(b)(want[:t0]).topk(2).values
            assert (top2[0] - top2[1]).item() < NEAR_TIE, (b, t0)
        else:
            assert (got[b, want.numel():] == eos).all()            # pad defaults to eos


def test_max_new_tokens(dev):
    ref, m = _model(dev, 92)
    m.eval()
    ids = _prompts(3, 12, 93).to(dev)
    a = _mgen(m, input_ids=ids, max_new_tokens=30, do_sample=False)
    b = _mgen(m, input_ids=ids, max_length=42, do_sample=False)
    assert a.shape == (3, 42) and torch.equal(a, b)
    with pytest.raises(ValueError):
        _mgen(m, input_ids=ids, max_length=42, max_new_tokens=30)


def test_graph_key_covers_stop(dev):
    """one decoder: no eos -> eos -> no eos, each equal to a fresh decoder's result"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 94)
    m.eval()
    B, Tp, L = 5, 8, 80
    ids = _prompts(B, Tp, 95).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=4)
    full = _dgen(dec, ids, L, do_sample=True, top_k=8)
    eos = _pick_any(full, Tp)
    assert eos is not None
    kw_eos = dict(do_sample=True, top_k=8, eos_token_id=eos, pad_token_id=0)
    got = _dgen(dec, ids, L, **kw_eos)
    assert torch.equal(got, XLDecoder(m.engine, B, L, seed=4).generate(ids, L, **kw_eos))
    assert torch.equal(got, finish_at_eos(full, Tp, eos, 0))
    again = _dgen(dec, ids, L, do_sample=True, top_k=8)
    assert torch.equal(again, full)
    assert torch.equal(again, XLDecoder(m.engine, B, L, seed=4).generate(ids, L, do_sample=True, top_k=8))


@pytest.mark.parametrize('path', ['unfused', 'large'])
def test_unfused_and_large_vocab_paths(dev, monkeypatch, path):
    from symbolic_music_generation_amd.generate import XLDecoder
    vocab = V
    if path == 'unfused':
        monkeypatch.setenv('MXL_DECODE_UNFUSED', '1')
        ref, m = _model(dev, 96)
    else:
        vocab = 4096
        ref, m = _model(dev, 96, vocab=vocab, cutoffs=(1000,))
    m.eval()
    B, Tp, L = 6, 8, 90
    ids = _prompts(B, Tp, 97, vocab=vocab).to(dev)
    dec = XLDecoder(m.engine, B, L, seed=6)
    assert not dec.fused_sampler
    for kw in (dict(do_sample=False), dict(do_sample=True, top_k=8)):
        full = _dgen(dec, ids, L, **kw)
        for mode in ('spread', 'all'):
            eos = _pick_eos(full, Tp, mode)
            if eos is None:
                continue
            got = _dgen(dec, ids, L, eos_token_id=eos, pad_token_id=1, **kw)
            assert torch.equal(got, finish_at_eos(full, Tp, eos, 1)), (kw, mode)
        eos = int(full[0, Tp])
        got = _dgen(dec, ids, L, eos_token_id=eos, min_length=Tp + 5, **kw)
        assert not (got[:, Tp:Tp + 5] == eos).any(), kw


def _reformer(dev):
    from symbolic_music_generation_amd.reformer import MyReformerConfig, MyReformerModelWithLMHead
    cfg = MyReformerConfig('debug-large', vocab_size=120, max_position_embeddings=512, axial_pos_shape=(16, 32),
                           attn_layers=['local'] * 4)
    return MyReformerModelWithLMHead(cfg, device=dev, seed=9).eval()


def test_reformer_stops_at_eos(dev):
    rf = _reformer(dev)
    B, Tp, L = 4, 20, 200
    ids = _prompts(B, Tp, 98, vocab=120).to(dev)
    for kw in (dict(do_sample=False), dict(do_sample=True, top_k=8)):
        full = _mgen(rf, input_ids=ids, max_length=L, **kw)
        assert full.shape == (B, L)
        for mode in ('all', 'spread'):
            eos = _pick_eos(full, Tp, mode)
            if eos is None:
                continue
            got = _mgen(rf, input_ids=ids, max_length=L, eos_token_id=eos, pad_token_id=0, **kw)
            assert torch.equal(got, finish_at_eos(full, Tp, eos, 0)), (kw, mode)
            if mode == 'all':
                assert got.shape[1] < L and rf._decoder.steps_run <= (got.shape[1] - Tp) + 2 * 16
    # max_new_tokens, and min_length keeps eos out of the first columns
    a = _mgen(rf, input_ids=ids, max_new_tokens=15, do_sample=False)
    full = _mgen(rf, input_ids=ids, max_length=L, do_sample=False)
    assert a.shape == (B, Tp + 15) and torch.equal(a, full[:, :Tp + 15])
    eos = int(_mgen(rf, input_ids=ids, max_length=Tp + 1, do_sample=False)[0, Tp])
    got = _mgen(rf, input_ids=ids, max_length=L, do_sample=False, eos_token_id=eos, min_length=Tp + 4)
    assert not (got[:, Tp:Tp + 4] == eos).any()


def test_num_return_sequences_with_eos(dev):
    ref, m = _model(dev, 99)
    m.eval()
    Tp, L = 9, 100
    ids = _prompts(3, Tp, 100).to(dev)
    kw = dict(do_sample=True, top_k=8, num_return_sequences=2)
    m._decoder = None
    full = _mgen(m, input_ids=ids, max_length=L, **kw)
    assert full.shape == (6, L)
    eos = _pick_any(full, Tp)
    assert eos is not None
    got = _mgen(m, input_ids=ids, max_length=L, eos_token_id=eos, pad_token_id=4, **kw)
    assert torch.equal(got, finish_at_eos(full, Tp, eos, 4))
