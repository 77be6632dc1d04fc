"""Generation from left-padded prompts of different lengths in one batch (`model.generate(attention_mask=...)`): every row,
its pad columns dropped, decodes as it would alone.  A left pad is an extra zero-memory slot once its K / V are zero in every
layer (mxl_kv_zero_pad), and the samplers' repetition penalty skips the -1 held for it in the id history."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 1190
NEAR_TIE = 5e-2          # same policy as tests/test_fullsize_gpu.py: a fork is legitimate only at a bf16 near-tie


def _model(dev, seed, **kw):
    from tests.test_xl_model_gpu import _pair
    kw.setdefault('max_length', 160)
    return _pair(dev, n_layer=2, mem_len=64, seed=seed, **kw)


def _prompts(lengths, seed, vocab=V):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(4, vocab, (n,), generator=g) for n in lengths]


def _batch(prompts, pad_id, dev):
    from symbolic_music_generation_amd.generate import left_pad
    ids, mask = left_pad(prompts, pad_id)
    return ids.to(dev), mask.to(dev)


def _repetition_scores(logp, history, penalty):
    """HF RepetitionPenaltyLogitsProcessor on one row of log-probabilities"""
    s = logp.clone()
    if penalty != 1.0:
        h = torch.unique(history)
        v = s[h]
        s[h] = torch.where(v < 0, v * penalty, v / penalty)
    return s


def _check_fork(got, want, score_fn, what):
    """got == want token for token, or they first differ at a position where the scores that picked want's token (score_fn(prefix))
    have a top-2 margin below NEAR_TIE; the comparison stops there.  Returns the fork position or None."""
    assert got.shape == want.shape, what
    mism = (got != want).nonzero()
    if mism.numel() == 0:
        return None
    t0 = int(mism[0, 0])
    s = score_fn(want[:t0])
    top2 = s.topk(2).values
    margin = (top2[0] - top2[1]).item()
    print(f'{what}: first fork at position {t0} (top-2 margin {margin:.4f})')
    assert margin < NEAR_TIE, f'{what}: diverges at position {t0} with margin {margin}'
    return t0


def test_kv_zero_pad_kernel_bit_exact(dev):
    from symbolic_music_generation_amd import ops
    torch.manual_seed(0)
    B, T, d = 6, 37, 136
    qkv = torch.randn(B, T, 3 * d, device=dev).to(torch.bfloat16)
    n_pad = torch.tensor([0, T, 1, 17, T - 1, 5], dtype=torch.int32, device=dev)
    want = qkv.clone()
    for b, s in enumerate(n_pad.tolist()):
        want[b, :s, d:] = 0
    got = qkv.clone()
    ops.kv_zero_pad(got, n_pad, B, T, d)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got[:, :, :d], qkv[:, :, :d])                       # queries untouched
    assert torch.equal(got[0], qkv[0]) and (got[1, :, d:] == 0).all()


@pytest.mark.parametrize('use_graph', [False, True])
def test_ragged_greedy_matches_oracle_per_row(dev, use_graph):
    """Tp = 90 > mem_len, one row with 83 pad columns (> mem_len), generation past the ring's wrap: row b without its pads equals
    the oracle's greedy loop on that prompt alone (to max_length - s_b)"""
    ref, m = _model(dev, 61)
    ref.eval(); m.eval()
    lengths = [7, 16, 24, 40, 90]
    prompts = _prompts(lengths, 62)
    ids, mask = _batch(prompts, 0, dev)
    Tp, L = ids.shape[1], 150
    out = m.generate(input_ids=ids, attention_mask=mask, max_length=L, do_sample=False, use_graph=use_graph).cpu()
    assert out.shape == (5, L) and torch.equal(out[:, :Tp], ids.cpu())
    for b, p in enumerate(prompts):
        s = Tp - len(p)
        want = ref.greedy_generate(p[None], L - s)[0]

        def oracle_scores(prefix):
            with torch.no_grad():
                return ref(prefix[None]).prediction_scores[0, -1]
        _check_fork(out[b, s:], want, oracle_scores, f'row {b} (prompt {len(p)}, pads {s})')


def test_ragged_trace_logprobs_match_one_shot_forward(dev):
    """log-probabilities of every row at every one of its positions, ragged batch under hipGraph replay with forced tokens, against
    the one-shot forward of that row alone"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 63)
    m.eval()
    lengths, G = [7, 30, 64, 90], 40
    seqs = _prompts([n + G for n in lengths], 64)
    prompts = [s[:n] for s, n in zip(seqs, lengths)]
    ids, mask = _batch(prompts, 0, dev)
    B, Tp = ids.shape
    n_pad = (mask == 0).sum(1).to(torch.int32)
    cont = torch.stack([s[n:] for s, n in zip(seqs, lengths)]).to(dev)       # (B, G) forced tokens
    dec = XLDecoder(m.engine, B, Tp + G + 1, seed=3)
    dec.trace = torch.zeros(B, Tp + G + 2, V, device=dev)
    samp = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0)
    steps = dec.begin(ids, Tp + G + 1, samp, use_graph=True, n_pad=n_pad)
    assert steps == G and dec.graph is not None
    for i in range(G):
        dec.force_tokens(cont[:, i])
        dec.replay_once()
    torch.cuda.synchronize()
    for b, (s, n) in enumerate(zip(n_pad.tolist(), lengths)):
        full = m(input_ids=seqs[b][None].to(dev)).prediction_scores[0]     # (n + G, V)
        got = dec.trace[b, s + n - 1:Tp + G]                                  # positions n - 1 .. n + G - 1 of the row
        err = (got - full[n - 1:n + G]).abs().max().item()
        assert err < 4e-2, (b, err)


def _single_rows(m, prompts, L, Tp, **kw):
    """each prompt alone through model.generate, to max_length L - (its pad count)"""
    outs = []
    for p in prompts:
        m._decoder = None
        outs.append(m.generate(input_ids=p[None].to(m.device), max_length=L - (Tp - len(p)), **kw)[0].cpu())
    m._decoder = None
    return outs


def _penalised_scores(m, penalty):
    def fn(prefix):
        lp = m(input_ids=prefix[None].to(m.device)).prediction_scores[0, -1].float().cpu()
        return _repetition_scores(lp, prefix, penalty)
    return fn


def _pad_probe(m, lengths, vocab, penalty, seeds):
    """(prompts, row, token): the first prompt set, among `seeds`, with a padded row whose greedy first token t is not in its own
    prompt, wins by more than NEAR_TIE, and loses by more than NEAR_TIE once t is penalised as history.  With t as the pad id, a
    sampler that counted the pads as history would change that row's first generated token."""
    for seed in seeds:
        prompts = _prompts(lengths, seed, vocab=vocab)
        for b, p in enumerate(prompts):
            if len(p) == max(lengths):
                continue
            lp = m(input_ids=p[None].to(m.device)).prediction_scores[0, -1].float().cpu()
            s = _repetition_scores(lp, p, penalty)
            top = s.topk(2)
            t = int(top.indices[0])
            if t in set(p.tolist()) or (top.values[0] - top.values[1]).item() <= NEAR_TIE:
                continue
            s2 = _repetition_scores(lp, torch.cat([p, torch.tensor([t])]), penalty)
            if (s2.max() - s2[t]).item() > NEAR_TIE:
                return prompts, b, t
    raise AssertionError('no prompt set with a pad-sensitive row: the test would not see pads counted as history')


@pytest.mark.parametrize('vocab', [V, 4096])
def test_ragged_repetition_penalty_ignores_pads(dev, vocab):
    """greedy with repetition_penalty 1.3, the pad id a token that a padded row generates first without having it in its prompt:
    ragged rows equal single-row generation (pads counted as history would penalise that token and change the row).  vocab 4096
    takes the bisection sampler (csrc/sample_large.hip) instead of the fused one; both with the adaptive head (cutoff 1000)."""
    ref, m = _model(dev, 65, vocab=vocab, cutoffs=(1000,))
    m.eval()
    lengths = [9, 20, 33, 70, 80]
    prompts, probe, pad_id = _pad_probe(m, lengths, vocab, 1.3, range(66, 76))
    Tp, L = max(lengths), 130
    kw = dict(do_sample=False, repetition_penalty=1.3)
    single = _single_rows(m, prompts, L, Tp, **kw)
    assert int(single[probe][len(prompts[probe])]) == pad_id
    ids, mask = _batch(prompts, pad_id, dev)
    for use_graph in (False, True):
        m._decoder = None
        out = m.generate(input_ids=ids, attention_mask=mask, max_length=L, use_graph=use_graph, **kw).cpu()
        assert torch.equal(out[:, :Tp], ids.cpu())
        for b, p in enumerate(prompts):
            _check_fork(out[b, Tp - len(p):], single[b], _penalised_scores(m, 1.3), f'graph={use_graph} row {b} pad id {pad_id}')


def test_ragged_lanes_equal_single_decoder(dev):
    """32 ragged rows: model.generate takes XLDecoderLanes; row for row the same tokens as one XLDecoder"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 67, max_length=128)
    m.eval()
    g = torch.Generator().manual_seed(68)
    lengths = torch.randint(3, 61, (32,), generator=g).tolist()
    lengths[5] = 60
    prompts = _prompts(lengths, 69)
    ids, mask = _batch(prompts, 1, dev)
    n_pad = (mask == 0).sum(1).to(torch.int32)
    m._decoder = None
    out = m.generate(input_ids=ids, attention_mask=mask, max_length=110, do_sample=False)
    assert type(m._decoder).__name__ == 'XLDecoderLanes'
    one = XLDecoder(m.engine, 32, 128, seed=3).generate(ids, 110, do_sample=False, use_graph=True, n_pad=n_pad)
    assert torch.equal(out, one)
    assert torch.equal(out[:, :ids.shape[1]], ids)


def test_ragged_sampling(dev):
    """top_k = 8: hipGraph replay equals eager under the same seed, prompt and pad columns come back as given (an out-of-range pad
    id included), every row's first draw is one of the 8 best tokens of that row's own log-probabilities"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 70)
    m.eval()
    lengths = [5, 18, 41, 77]
    prompts = _prompts(lengths, 71)
    ids, mask = _batch(prompts, 99999, dev)
    n_pad = (mask == 0).sum(1).to(torch.int32)
    B, Tp = ids.shape
    kw = dict(do_sample=True, top_k=8)
    a = XLDecoder(m.engine, B, 140, seed=5).generate(ids, 140, use_graph=True, n_pad=n_pad, **kw)
    b = XLDecoder(m.engine, B, 140, seed=5).generate(ids, 140, use_graph=False, n_pad=n_pad, **kw)
    assert torch.equal(a, b)
    assert torch.equal(a[:, :Tp], ids) and (a[:, Tp:] >= 0).all() and (a[:, Tp:] < V).all()
    for r, p in enumerate(prompts):
        lp = m(input_ids=p[None].to(dev)).prediction_scores[0, -1]
        kth = lp.topk(8).values[-1].item()
        assert lp[int(a[r, Tp])].item() >= kth - NEAR_TIE, (r, int(a[r, Tp]))
    # through the model: num_return_sequences expands the mask with the ids
    m._decoder = None
    out = m.generate(input_ids=ids, attention_mask=mask, max_length=100, num_return_sequences=2, **kw)
    assert out.shape == (2 * B, 100) and torch.equal(out[:, :Tp], ids.repeat_interleave(2, 0))
    assert (out[:, Tp:] >= 0).all() and (out[:, Tp:] < V).all()


def test_all_ones_mask_changes_nothing(dev):
    ref, m = _model(dev, 72)
    m.eval()
    ids = torch.stack(_prompts([24] * 3, 73)).to(dev)
    ones = torch.ones_like(ids)
    for kw in (dict(do_sample=False), dict(do_sample=True, top_k=8, repetition_penalty=1.2)):
        m._decoder = None
        a = m.generate(input_ids=ids, max_length=120, **kw)
        m._decoder = None
        b = m.generate(input_ids=ids, attention_mask=ones, max_length=120, **kw)
        assert torch.equal(a, b), kw


def test_graph_recaptured_when_a_trace_is_attached(dev):
    """a step graph captured without a trace must not be replayed once one is attached (the trace would stay zero)"""
    from symbolic_music_generation_amd.generate import XLDecoder
    ref, m = _model(dev, 74)
    m.eval()
    prompts = _prompts([12, 30], 75)
    ids, mask = _batch(prompts, 0, dev)
    n_pad = (mask == 0).sum(1).to(torch.int32)
    B, Tp = ids.shape
    samp = dict(do_sample=False, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0)
    L = 100

    def run(dec, use_graph):
        dec.trace = torch.zeros(B, L + 1, V, device=dev)
        for _ in range(dec.begin(ids, L, samp, use_graph=use_graph, n_pad=n_pad)):
            dec.replay_once()
        torch.cuda.synchronize()
        return dec.trace, dec.ids[:, :L].clone()

    dec = XLDecoder(m.engine, B, L, seed=3)
    dec.generate(ids, L, use_graph=True, n_pad=n_pad)               # captured without a trace
    tr, got = run(dec, True)
    want_tr, want = run(XLDecoder(m.engine, B, L, seed=3), False)
    assert torch.equal(got, want)
    assert (tr[:, Tp - 1:L - 1].abs().sum(-1) > 0).all()
    assert torch.equal(tr, want_tr)


def test_padded_mask_rejected_where_unsupported(dev):
    from symbolic_music_generation_amd._lib import MusicXLError
    from symbolic_music_generation_amd.reformer import MyReformerConfig, MyReformerModelWithLMHead
    ref, m = _model(dev, 76)
    m.eval()
    ids, mask = _batch(_prompts([6, 10], 77), 0, dev)
    for kw in (dict(num_beams=2), dict(num_beams=4, num_beam_groups=2), dict(penalty_alpha=0.6, top_k=4),
               dict(max_new_tokens=8)):
        with pytest.raises(MusicXLError):
            m.generate(input_ids=ids, attention_mask=mask, max_length=30, **kw)
    with pytest.raises(MusicXLError):
        m.engine.forward(ids, train=False, mems=[torch.zeros(2, 64, 128, device=dev, dtype=torch.bfloat16)] * 2,
                         n_pad=(mask == 0).sum(1).to(torch.int32))
    with pytest.raises(MusicXLError):                                 # right padding
        m.generate(input_ids=ids, attention_mask=mask.flip(1), max_length=30)
    cfg = MyReformerConfig('debug-large', vocab_size=120, max_position_embeddings=512, axial_pos_shape=(16, 32),
                           attn_layers=['local'] * 4)
    rf = MyReformerModelWithLMHead(cfg, device=dev, seed=9).eval()
    rids = ids % 120
    with pytest.raises(MusicXLError):
        rf.generate(input_ids=rids, attention_mask=mask, max_length=30)
    a = rf.generate(input_ids=rids, attention_mask=torch.ones_like(mask), max_length=30, do_sample=False)
    b = rf.generate(input_ids=rids, max_length=30, do_sample=False)
    assert torch.equal(a, b)
