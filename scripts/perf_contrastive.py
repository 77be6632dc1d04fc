"""Contrastive search with its step on the device against the host-driven loop, at the C5 decode shape of bench.py (12L/768d,
M = 2048, V = 1190), 256-token prompts, 256 new tokens, an eos that never fires, through model.generate, at two settings:

  ref   the reference's settings (musicnlp/trainer/eval.py:549): one prompt, top_k = 16, penalty_alpha = 0.3   (16 decoder rows)
  b4k8  four prompts, top_k = 8                                                                                 (32 decoder rows)

  device        generate.contrastive_search_device: rules mask, mxl_contrastive_topk, advance, model, mxl_contrastive_step,
                mxl_ring_slot_broadcast -- one captured graph per step, the finished count read a chunk late
  device eager  the same launches without the graph (use_graph=False)
  host          MXL_CONTRASTIVE_HOST=1, generate.contrastive_search: topk, softmax, mxl_contrastive_select, index_select + copy_
                over ids and the 2 * n_layer whole rings, two more index_selects, bool(unfinished.any()) per step, eager launches

The three are alternated in one process on one device, RUNS (5) times each after one warm-up call each (every call builds its
decoder, runs the prompt pass and, on the graph path, captures the step); reports the median and the min..max of the generated
tokens per second, the library launches per step of either path (the host path's torch launches come on top), and the bytes the
ring step moves per token, computed from the shapes: whole-ring copies before (index_select reads every ring, writes a copy, copy_
reads and writes it again), one slot per ring, head and row after.

    python3 scripts/perf_contrastive.py                  # env: RUNS (5), NEW (256), ONLY (ref | b4k8), MODE (device | eager | host:
                                                         # one call of that path alone, for a kernel trace)

RINGS=shared compares the two ring modes of the device path instead (generate(contrastive_rings=)): 'copied', one set of rings per
candidate row, and 'shared', one per prompt read by its K candidates (mxl_kv_stash / mxl_relattn_decode_shared /
mxl_kv_commit_shared).  The two are alternated, RUNS calls each after a warm-up call each, with equal ids asserted, at four shapes:
ref and b4k8 above, b8k16 (8 prompts x top_k 16, 256-token prompts) and b8k16full (the same with 2048-token prompts: a full ring from
the first step).  Reports the median, the slowest and the fastest run of each mode, the ring memory of either decoder from its
tensors, and whether the slowest shared run beats the fastest copied run (the criterion of profiles/beam_step.txt).

    RINGS=shared python3 scripts/perf_contrastive.py     # env: RUNS (5), NEW (256), ONLY (ref | b4k8 | b8k16 | b8k16full)
"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd import ops
from symbolic_music_generation_amd.transformer_xl import MyTransfoXLConfig, MyTransfoXLLMHeadModel

dev = torch.device('cuda:0')
V, M, Tp = 1190, 2048, 256
NEW, RUNS = int(os.environ.get('NEW', 256)), int(os.environ.get('RUNS', 5))
L = Tp + NEW
SETTINGS = {'ref': (1, 16, 0.3), 'b4k8': (4, 8, 0.3)}
cfg = MyTransfoXLConfig('base', max_length=2048, vocab_size=V, mem_len=M, cutoffs=[])
model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()

calls = [0]
_check = ops.check


def counting_check(code, what=''):
    calls[0] += 1
    return _check(code, what)


def run(kw, mode, **extra):
    if mode == 'host':
        os.environ['MXL_CONTRASTIVE_HOST'] = '1'
    else:
        os.environ.pop('MXL_CONTRASTIVE_HOST', None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(**{**kw, 'use_graph': mode == 'device', **extra})
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def compare_rings():
    from symbolic_music_generation_amd import generate as G
    built = []
    real = G.XLDecoder

    class Recorded(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            built.append(self)
    G.XLDecoder = Recorded
    shapes = dict(SETTINGS, b8k16=(8, 16, 0.3), b8k16full=(8, 16, 0.3))
    for name, (B, K, alpha) in shapes.items():
        if os.environ.get('ONLY', name) != name:
            continue
        tp = M if name.endswith('full') else Tp
        ids = torch.randint(4, V, (B, tp), generator=torch.Generator().manual_seed(77)).to(dev)
        kw = dict(input_ids=ids, max_length=tp + NEW, top_k=K, penalty_alpha=alpha, eos_token_id=V + 1, pad_token_id=0)
        outs, mem, pieces = {}, {}, {}
        for mode in G.CONTRASTIVE_RINGS:                                        # warm-up of either mode
            del built[:]
            outs[mode] = run(kw, 'device', contrastive_rings=mode)[1]
            dec = built[0]
            mem[mode] = sum(t.numel() * t.element_size() for t in dec.kc + dec.vc + ([dec.stash] if dec.shared_K else []))
            pieces[mode] = dec.pieces
        del built[:], dec
        # equal by construction where both decoders cut the ring alike; with other piece counts the attention outputs may differ in
        # the last bf16 bit (mxl_relattn_decode_split), so a difference there is reported, not asserted away
        same = torch.equal(outs['copied'], outs['shared'])
        assert same or pieces['copied'] != pieces['shared'], f'{name}: the ids of the two ring modes differ at equal piece counts'
        agree = int((outs['copied'] == outs['shared']).all(0).int().cumprod(0).sum()) - tp
        times = {mode: [] for mode in G.CONTRASTIVE_RINGS}
        for _ in range(RUNS):
            for mode in G.CONTRASTIVE_RINGS:
                t, out = run(kw, 'device', contrastive_rings=mode)
                assert torch.equal(out, outs[mode])
                times[mode].append(t)
                del built[:]
        tps = {mode: sorted(B * NEW / t for t in times[mode]) for mode in times}
        print(f'contrastive search [{name}], C5 decode shape: {B} prompt(s) x {tp}, top_k {K} ({B * K} rows), penalty_alpha {alpha}, '
              f'{NEW} new tokens, eos never fires, captured step; shared ids == copied ids: {same}'
              + ('' if same else f' (the first {agree} of {NEW} generated columns agree)'))
        for mode in times:
            print(f'{mode:6s}: {statistics.median(tps[mode]):9.1f} tok/s median of {RUNS} (slowest {tps[mode][0]:.1f}, fastest '
                  f'{tps[mode][-1]:.1f}); {statistics.median(times[mode]):.3f} s per call; rings{" + stash" if mode == "shared" else ""} '
                  f'{mem[mode] / 1e6:.1f} MB, {pieces[mode]} ring piece(s) per attention workgroup set')
        c, sh = tps['copied'], tps['shared']
        verdict = 'faster' if sh[0] > c[-1] else ('slower' if sh[-1] < c[0] else 'level')
        print(f'shared / copied = {statistics.median(sh) / statistics.median(c):.3f}x; the slowest shared run ({sh[0]:.1f} tok/s) against '
              f'the fastest copied run ({c[-1]:.1f} tok/s): shared is {verdict}')
    G.XLDecoder = real


MODES = ('device', 'eager', 'host')
if os.environ.get('RINGS') == 'shared':
    with torch.no_grad():
        compare_rings()
    sys.exit(0)
with torch.no_grad():
    for name, (B, K, alpha) in SETTINGS.items():
        if os.environ.get('ONLY', name) != name:
            continue
        ids = torch.randint(4, V, (B, Tp), generator=torch.Generator().manual_seed(77)).to(dev)
        kw = dict(input_ids=ids, max_length=L, top_k=K, penalty_alpha=alpha, eos_token_id=V + 1, pad_token_id=0)
        if os.environ.get('MODE'):
            run(kw, os.environ['MODE'])
            t, _ = run(kw, os.environ['MODE'])
            print(f'{name}: one {os.environ["MODE"]} call after a warm-up call, {t:.3f} s')
            continue
        # library launches per step: one short eager call of either path, the prompt pass's share taken off with a second, shorter one
        ops.check = counting_check
        per_step = {}
        for mode in ('eager', 'host'):
            n = []
            for new in (3, 11):
                calls[0] = 0
                run(kw, mode, max_length=Tp + new)
                n.append(calls[0])
            per_step[mode] = (n[1] - n[0]) / 8
        per_step['device'] = per_step['eager']
        ops.check = _check
        outs = {mode: run(kw, mode)[1] for mode in MODES}                       # warm-up of every path
        same = torch.equal(outs['device'], outs['host']) and torch.equal(outs['eager'], outs['host'])
        agree = int((outs['device'] == outs['host']).all(0).int().cumprod(0).sum()) - Tp
        times = {mode: [] for mode in MODES}
        for _ in range(RUNS):
            for mode in MODES:
                times[mode].append(run(kw, mode)[0])
        c = model.engine.cfg
        rows, n_rings = B * K, 2 * c.n_layer
        ring_bytes = rows * c.n_head * M * c.d_head * 2
        before = n_rings * ring_bytes * 4                  # index_select: read + write; copy_: read + write
        after = n_rings * B * c.n_head * c.d_head * 2 * K  # one slot: K - 1 writes and the reads of the picked row's
        print(f'contrastive search [{name}], C5 decode shape: {B} prompt(s) x {Tp}, top_k {K} ({rows} rows), penalty_alpha {alpha}, '
              f'{NEW} new tokens, eos never fires; device ids == eager ids == host ids: {same}'
              + ('' if same else f' (the first {agree} of {NEW} generated columns agree)'))
        tps = {mode: sorted(B * NEW / t for t in times[mode]) for mode in MODES}
        notes = {'device': 'no host read per step, one graph replay', 'eager': 'no host read per step, eager launches',
                 'host': '1 sync per step (unfinished.any()), eager launches'}
        for mode in MODES:
            print(f'{mode:6s}: {statistics.median(tps[mode]):9.1f} tok/s median of {RUNS} (min {tps[mode][0]:.1f}, max {tps[mode][-1]:.1f}); '
                  f'{statistics.median(times[mode]):.3f} s per call; {per_step[mode]:.1f} library launches per step, {notes[mode]}')
        print(f'ring step, bytes moved per token: {before / 1e6:.1f} MB before (2 x {n_rings} whole-ring passes of {ring_bytes / 1e6:.1f} MB), '
              f'{after / 1e3:.1f} kB after (one slot of {n_rings} rings x {c.n_head} heads x {K} rows)')
        for mode in ('device', 'eager'):
            d, h = tps[mode], tps['host']
            gap = statistics.median(d) / statistics.median(h)
            clear = d[0] > h[-1]
            print(f'{mode} / host = {gap:.3f}x; the slowest {mode} run is {"above" if clear else "NOT above"} the fastest host run '
                  f'({d[0]:.1f} vs {h[-1]:.1f} tok/s)')
