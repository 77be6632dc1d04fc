"""Host side of generation from left-padded prompts: attention-mask validation, left_pad / strip_left_pad, the tokenizer's
left padding and attention mask, and the C ABI's argument checks of mxl_kv_zero_pad.  No GPU."""
import pytest
import torch


def test_left_pad_counts_accepts_left_padding_only():
    from symbolic_music_generation_amd._lib import MusicXLError
    from symbolic_music_generation_amd.generate import left_pad_counts
    ok = torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 1]])
    assert left_pad_counts(ok, (3, 4)) == [2, 0, 3]
    assert left_pad_counts(ok.bool(), (3, 4)) == [2, 0, 3]
    with pytest.raises(MusicXLError, match='left'):                      # right padding: the message names left padding
        left_pad_counts(torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]]), (2, 4))
    with pytest.raises(MusicXLError, match='without any token'):        # a fully padded row
        left_pad_counts(torch.tensor([[0, 0, 0, 0], [1, 1, 1, 1]]), (2, 4))
    with pytest.raises(MusicXLError, match='0 .pad. and 1'):             # not 0 / 1
        left_pad_counts(torch.tensor([[0, 2, 1, 1]]), (1, 4))
    with pytest.raises(MusicXLError, match='shape'):
        left_pad_counts(torch.ones(2, 5, dtype=torch.int64), (2, 4))
    with pytest.raises(MusicXLError):                                     # a hole inside the prompt
        left_pad_counts(torch.tensor([[0, 1, 0, 1]]), (1, 4))


def test_left_pad_strip_left_pad_round_trip():
    from symbolic_music_generation_amd.generate import left_pad, strip_left_pad
    prompts = [torch.tensor([5, 6, 7]), torch.tensor([8]), torch.tensor([9, 10, 11, 12, 13])]
    ids, mask = left_pad(prompts, pad_token_id=1)
    assert ids.tolist() == [[1, 1, 5, 6, 7], [1, 1, 1, 1, 8], [9, 10, 11, 12, 13]]
    assert mask.tolist() == [[0, 0, 1, 1, 1], [0, 0, 0, 0, 1], [1, 1, 1, 1, 1]]
    assert ids.dtype == mask.dtype == torch.int64
    back = strip_left_pad(ids, mask)
    assert [r.tolist() for r in back] == [p.tolist() for p in prompts]
    # generated output: (B, L) with L > Tp, the mask still covers the prompt columns only
    gen = torch.cat([ids, torch.tensor([[20, 21], [22, 23], [24, 25]])], 1)
    rows = strip_left_pad(gen, mask)
    assert [r.tolist() for r in rows] == [[5, 6, 7, 20, 21], [8, 22, 23], [9, 10, 11, 12, 13, 24, 25]]


def _tok():
    from symbolic_music_generation_amd.vocab import MusicTokenizer
    return MusicTokenizer()


def _texts(tok):
    v = tok.vocab
    return [f'{v.start_of_bar} {v.start_of_bar}', v.start_of_bar, f'{v.start_of_bar} {v.end_of_song} {v.start_of_bar}']


def test_tokenizer_left_padding_and_attention_mask():
    tok = _tok()
    texts = _texts(tok)
    plain = [tok.encode(t) for t in texts]
    tok.padding_side = 'left'
    out = tok(texts, padding=True, return_tensors='pt', return_attention_mask=True)
    pad = tok.pad_token_id
    W = max(len(e) for e in plain)
    assert out['input_ids'].tolist() == [[pad] * (W - len(e)) + e for e in plain]
    assert out['attention_mask'].tolist() == [[0] * (W - len(e)) + [1] * len(e) for e in plain]
    tok.padding_side = 'right'
    out = tok(texts, padding='longest', return_attention_mask=True)
    assert out['input_ids'] == [e + [pad] * (W - len(e)) for e in plain]
    assert out['attention_mask'] == [[1] * len(e) + [0] * (W - len(e)) for e in plain]
    one = tok(texts[0], return_attention_mask=True)
    assert one['attention_mask'] == [1] * len(plain[0])


def test_tokenizer_default_output_unchanged():
    tok = _tok()
    texts = _texts(tok)
    plain = [tok.encode(t) for t in texts]
    pad = tok.pad_token_id
    W = max(len(e) for e in plain)
    assert tok.padding_side == 'right'
    out = tok(texts, padding=True, return_tensors='pt')
    assert set(out) == {'input_ids'}
    assert out['input_ids'].tolist() == [e + [pad] * (W - len(e)) for e in plain]
    assert tok(texts) == {'input_ids': plain}
    assert tok(texts[1]) == {'input_ids': plain[1]}
    assert tok(texts, padding='max_length', max_length=6)['input_ids'] == [e + [pad] * (6 - len(e)) for e in plain]


def test_kv_zero_pad_argument_errors_without_gpu():
    from symbolic_music_generation_amd import _lib
    L = _lib.lib()
    assert 'mxl_kv_zero_pad' in _lib.declared_functions()
    assert L.mxl_kv_zero_pad(None, None, 1, 1, 8, None) == -1
    assert L.mxl_kv_zero_pad(16, 16, 1, 1, 12, None) == -1          # d % 8 != 0
    assert L.mxl_kv_zero_pad(16, 16, 0, 1, 8, None) == -1           # B = 0
    assert L.mxl_kv_zero_pad(16, 16, 1, 0, 8, None) == -1           # T = 0
