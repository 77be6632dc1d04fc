"""What batched generation from left-padded prompts of different lengths buys at the C5 model shape (12L/768d, M = 2048):
64 prompts of 200-400 tokens generated to max_length 1024 with top_k = 8,

  (a) one ragged call:   model.generate(input_ids=ids, attention_mask=mask, ...)   (64 rows, two decode lanes)
  (b) one call per song: model.generate(input_ids=prompt_b[None], max_length=1024 - s_b, ...)   (B = 1 each)

and the cost of the padded prompt pass: pad columns are computed and thrown away, at most (Tp - p_min) / Tp of the prefill.

    python3 scripts/perf_ragged_generate.py         # env: SINGLE (single-row calls timed, default 8 of the 64), SEED (77)

(b) times SINGLE of the 64 single-row calls (spread over the length range) and scales by 64 / SINGLE."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd.transformer_xl import MyTransfoXLConfig, MyTransfoXLLMHeadModel
from symbolic_music_generation_amd.generate import XLDecoder, left_pad

dev = torch.device('cuda:0')
V, M, B, L = 1190, 2048, 64, 1024
SINGLE, SEED = int(os.environ.get('SINGLE', 8)), int(os.environ.get('SEED', 77))
cfg = MyTransfoXLConfig('base', max_length=2048, vocab_size=V, mem_len=M, cutoffs=[])
model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()
g = torch.Generator().manual_seed(SEED)
lengths = torch.randint(200, 401, (B,), generator=g).tolist()
prompts = [torch.randint(4, V, (n,), generator=g).to(dev) for n in lengths]
ids, mask = left_pad(prompts, 0)
Tp = ids.shape[1]
n_pad = (mask == 0).sum(1).to(torch.int32)
kw = dict(do_sample=True, top_k=8)
new_tokens = sum(L - Tp for _ in lengths)            # every row gets L - Tp new tokens
print(f'64 prompts, lengths {min(lengths)}..{max(lengths)} (mean {sum(lengths) / B:.1f}), Tp = {Tp}, max_length {L}, '
      f'{L - Tp} new tokens per row', flush=True)


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


# (a) one ragged call (first call warms up: library attributes, graph capture, workspaces)
with torch.no_grad():
    model.generate(input_ids=ids, attention_mask=mask, max_length=Tp + 16, **kw)
    model._decoder = None
    model.generate(input_ids=ids, attention_mask=mask, max_length=L, **kw)
    t_a, out = timed(lambda: model.generate(input_ids=ids, attention_mask=mask, max_length=L, **kw))
print(f'(a) one ragged call, B = 64: {t_a:.3f} s, {new_tokens / t_a / 1e3:.1f} k new tok/s, '
      f'decoder {type(model._decoder).__name__}', flush=True)

# (b) one call per song, B = 1 (each row to L - s_b: the same new tokens as its row of (a))
pick = sorted(range(B), key=lambda b: lengths[b])[::max(1, B // SINGLE)][:SINGLE]
with torch.no_grad():
    model._decoder = None
    model.generate(input_ids=prompts[pick[0]][None], max_length=L, **kw)     # decoder for L positions + graph, reused below
    tot = 0.0
    for b in pick:
        t, _ = timed(lambda: model.generate(input_ids=prompts[b][None], max_length=L - (Tp - lengths[b]), **kw))
        tot += t
t_b = tot * B / len(pick)
print(f'(b) 64 single-row calls (timed {len(pick)}, scaled): {t_b:.3f} s, {new_tokens / t_b / 1e3:.2f} k new tok/s; '
      f'(a) is {t_b / t_a:.1f}x faster', flush=True)

# prompt pass: the padded batch against the same rows cut to one common length (no pads), one decoder of 64 rows
samp = dict(do_sample=True, top_k=8, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0)
dec = XLDecoder(model.engine, B, L, seed=77)
model._decoder = None
with torch.no_grad():
    dec.prefill(ids, samp, n_pad)
    t_pad, _ = timed(lambda: dec.prefill(ids, samp, n_pad), reps=5)
    mean_len = round(sum(lengths) / B)
    flat = torch.stack([p[:mean_len] if len(p) >= mean_len else torch.cat([p, p[:mean_len - len(p)]]) for p in prompts])
    dec.prefill(flat, samp)
    t_flat, _ = timed(lambda: dec.prefill(flat, samp), reps=5)
waste = float(n_pad.sum()) / (B * Tp)
print(f'prompt pass, 64 x {Tp} padded: {1e3 * t_pad:.2f} ms ({100 * waste:.1f} % of its columns are pads, bound '
      f'(Tp - p_min) / Tp = {100 * (Tp - min(lengths)) / Tp:.1f} %); 64 x {mean_len} unpadded (the same token count): '
      f'{1e3 * t_flat:.2f} ms; pad overhead {1e3 * (t_pad - t_flat):.2f} ms = {100 * (t_pad - t_flat) / t_a:.2f} % of the ragged call',
      flush=True)
