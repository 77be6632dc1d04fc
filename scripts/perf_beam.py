"""Beam search with the scorer on the device against the host scorer, at the C5 decode shape of bench.py (12L/768d, M = 2048,
V = 1190): 8 prompts of 256 tokens, num_beams = 4 (32 decoder rows), 256 new tokens, an eos that never fires, through
model.generate.

  device  generate.beam_search_device: rules mask, mxl_beam_step, mxl_beam_reorder over the ring table, advance, model -- one
          captured graph per step, the done count read a chunk late
  host    MXL_BEAM_HOST=1, generate.beam_search: topk, three .tolist() reads, the Python walk, three uploads, index_select + copy_
          over ids and the 2 * n_layer rings, eager launches

The two are alternated in one process on one device, RUNS (5) times each after one warm-up call each; reports the median and the
min..max of the tokens per second (new tokens of the best hypothesis per prompt: 8 x 256 per call) and the library launches per
step of either path (the host path's torch launches -- topk, the index_select / copy_ pairs, the uploads -- come on top).

    python3 scripts/perf_beam.py                  # env: RUNS (5), NEW (256)

GROUPS=2 (and DIVERSITY=1.5) measures diverse beam search instead, num_beam_groups = GROUPS with that diversity_penalty:
generate.group_beam_search_device (mxl_group_beam_step in place of mxl_beam_step) against generate.group_beam_search, which runs
the topk, the reads, the walk and the uploads once per group and step.

    GROUPS=2 python3 scripts/perf_beam.py         # the reference's 'beam' strategy: num_beams=4, num_beam_groups=2

SAMPLE=1 measures beam-sample with the reference's settings (num_beams = 3, do_sample=True, renormalize_logits=True, top_k = 50:
HF's `beam_sample`), for one prompt and for eight: generate.beam_sample_device (`device_scorer=True`: rules mask, mxl_beam_sample_draw,
mxl_beam_sample_step, mxl_beam_reorder, advance, model in one captured graph per step) against generate.beam_search(do_sample=True)
(`_warp` on a (rows, V) matrix, torch.multinomial, three .tolist() reads, the walk, three uploads, index_select + copy_ over the
rings).  The two draw from different random streams, so their ids differ; with an eos that never fires both emit NEW tokens per prompt.

    SAMPLE=1 python3 scripts/perf_beam.py

RINGS=indexed measures the device path against itself: beam_rings='copied' (mxl_beam_reorder moves whole ring rows) against
beam_rings='indexed' (the rings stay, mxl_beam_owner_follow keeps the owner table and mxl_relattn_decode_owned reads through it),
alternated in one process, RUNS timed calls each after a warm-up call each, ids compared.  Also reports the mean share of decoder
rows with src != j per step, counted in one eager 'copied' call: the copy's cost depends on it, and a randomly initialised model (the
weights here: seed 77) may move few beams.  TP sets the prompt length: TP=2048 is the full-ring point, t >= M throughout, where the
copy is largest.

    RINGS=indexed python3 scripts/perf_beam.py
    RINGS=indexed TP=2048 python3 scripts/perf_beam.py

RINGS=indexed_fp8 measures beam_rings='indexed' (bf16 rings) against beam_rings='indexed_fp8' (FP8 rings, never moved either, read by
mxl_relattn_decode_fp8_owned) by the same procedure.  K and V rounded to four significant bits give other scores, so the ids are not
expected to be equal: the rows that differ are counted, not checked.  Also reports the ring bytes of either decoder.

    RINGS=indexed_fp8 python3 scripts/perf_beam.py
    RINGS=indexed_fp8 TP=2048 python3 scripts/perf_beam.py
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
V, M, B, Tp, NB = 1190, 2048, 8, int(os.environ.get('TP', 256)), 4
NEW, RUNS = int(os.environ.get('NEW', 256)), int(os.environ.get('RUNS', 5))
GROUPS, DIVERSITY = int(os.environ.get('GROUPS', 1)), float(os.environ.get('DIVERSITY', 1.5))
SAMPLE = os.environ.get('SAMPLE') == '1'
RINGS = os.environ.get('RINGS')
assert RINGS in (None, 'indexed', 'indexed_fp8'), RINGS
PAIR = ('indexed', 'indexed_fp8') if RINGS == 'indexed_fp8' else ('copied', 'indexed')       # (the baseline, the mode measured)
L = Tp + NEW
cfg = MyTransfoXLConfig('base', max_length=max(2048, L), vocab_size=V, mem_len=M, cutoffs=[])
model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()
ids = torch.randint(4, V, (B, Tp), generator=torch.Generator().manual_seed(77)).to(dev)
kw = dict(input_ids=ids, max_length=L, num_beams=NB, early_stopping=True, eos_token_id=V + 1, pad_token_id=0)
if GROUPS > 1:
    kw.update(num_beam_groups=GROUPS, diversity_penalty=DIVERSITY)

calls = [0]
_check = ops.check


def counting_check(code, what=''):
    calls[0] += 1
    return _check(code, what)


def run(host: bool, **extra):
    if host:
        os.environ['MXL_BEAM_HOST'] = '1'
    else:
        os.environ.pop('MXL_BEAM_HOST', None)
    os.environ['MXL_GROUP_BEAM_DEVICE'] = '1'         # (group beam search without a rule takes the device path only when asked to)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(**{**kw, **extra})
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


with torch.no_grad():
    if SAMPLE:
        arm = dict(num_beams=3, do_sample=True, top_k=50, renormalize_logits=True)
        for n in (1, B):
            sub = dict(arm, input_ids=ids[:n])
            run(False, device_scorer=True, **sub), run(True, **sub)              # warm-up of both paths
            times = {False: [], True: []}
            for _ in range(RUNS):
                times[False].append(run(False, device_scorer=True, **sub)[0])
                times[True].append(run(True, **sub)[0])
            print(f'beam-sample, C5 decode shape: {n} prompt(s) x {Tp}, num_beams 3 ({3 * n} rows), top_k 50, {NEW} new tokens, '
                  'eos never fires')
            d, h = sorted(n * NEW / t for t in times[False]), sorted(n * NEW / t for t in times[True])
            for name, tps, ts in (('device', d, times[False]), ('host  ', h, times[True])):
                print(f'{name}: {statistics.median(tps):9.1f} tok/s median of {RUNS} (min {tps[0]:.1f}, max {tps[-1]:.1f}); '
                      f'{statistics.median(ts):.3f} s per call')
            clear = d[0] > h[-1]
            print(f'device / host = {statistics.median(d) / statistics.median(h):.3f}x; the slowest device run is '
                  f'{"above" if clear else "NOT above"} the fastest host run ({d[0]:.1f} vs {h[-1]:.1f} tok/s)')
        sys.exit(0)
    if RINGS:
        from symbolic_music_generation_amd.generate import XLDecoder
        # the share of rows that move: one eager 'copied' call, beam_idx != the row itself summed on the device after every select
        real_select, seen = XLDecoder.beam_select, {}

        def counting_select(dec):
            r = real_select(dec)
            rows = torch.arange(dec.B, device=dec.beam.beam_idx.device, dtype=torch.int32)
            seen['rows'] = seen.get('rows', 0) + (dec.beam.beam_idx != rows).sum()
            seen['items'] = seen.get('items', 0) + (dec.beam.moved != 0).sum()
            seen['steps'] = seen.get('steps', 0) + 1
            return r
        XLDecoder.beam_select = counting_select
        run(False, beam_rings='copied', use_graph=False)
        XLDecoder.beam_select = real_select
        share, items = float(seen['rows']) / (seen['steps'] * B * NB), float(seen['items']) / (seen['steps'] * B)
        base, new = PAIR
        (_, a), (_, b) = run(False, beam_rings=base), run(False, beam_rings=new)   # warm-up; copied and indexed return the same ids
        same = torch.equal(a, b)
        times = {base: [], new: []}
        for _ in range(RUNS):
            for mode in times:
                times[mode].append(run(False, beam_rings=mode)[0])
        what = 'beam search' if GROUPS == 1 else f'group beam search ({GROUPS} groups, diversity_penalty {DIVERSITY})'
        print(f'{what} on the device, C5 decode shape: {B} prompts x {Tp}, num_beams {NB} ({B * NB} rows), {NEW} new tokens, eos never '
              f'fires, weights: random initialisation (seed 77); '
              + (f'{new} ids == {base} ids: {same}' if RINGS == 'indexed' else
                 f'{int((a != b).any(1).sum())} of {a.shape[0]} returned rows differ from the bf16 rings\' in an id (not expected equal)'))
        if RINGS == 'indexed_fp8':
            slots, dh = B * NB * cfg.n_layer * 2 * cfg.n_head * M, cfg.d_head
            print(f'ring memory: bf16 {slots * dh * 2 / 1e9:.3f} GB, fp8 bytes and exponents {slots * (dh + 1) / 1e9:.3f} GB '
                  f'({(dh + 1) / (2 * dh):.3f} of it)')
        print(f'rows with src != j: {100 * share:.1f} % per step on average, items that moved: {100 * items:.1f} % ({seen["steps"]} selects); '
              f'slots written at the first step {min(Tp, M)} of {M}, at the last {min(L - 1, M)}')
        tps = {m: sorted(B * NEW / t for t in ts) for m, ts in times.items()}
        for m in times:
            print(f'{m:11s}: {statistics.median(tps[m]):9.1f} tok/s median of {RUNS} (min {tps[m][0]:.1f}, max {tps[m][-1]:.1f}); '
                  f'{statistics.median(times[m]):.3f} s per call')
        clear = tps[new][0] > tps[base][-1]
        print(f'{new} / {base} = {statistics.median(tps[new]) / statistics.median(tps[base]):.3f}x; the slowest {new} run is '
              f'{"above" if clear else "NOT above"} the fastest {base} run ({tps[new][0]:.1f} vs {tps[base][-1]:.1f} tok/s): the '
              f'gap {"exceeds" if clear else "does not exceed"} the run-to-run spread')
        sys.exit(0)
    # library launches per step: one short eager call of either path, the prompt pass's share taken off with a second, shorter one
    ops.check = counting_check
    per_step = {}
    for host in (False, True):
        n = []
        for new in (3, 11):
            calls[0] = 0
            run(host, max_length=Tp + new, use_graph=False)
            n.append(calls[0])
        per_step[host] = (n[1] - n[0]) / 8
    ops.check = _check
    (_, a), (_, b) = run(False), run(True)                                     # warm-up of both paths; they return the same ids
    same = torch.equal(a, b)
    times = {False: [], True: []}
    for _ in range(RUNS):
        for host in (False, True):
            times[host].append(run(host)[0])
    what = 'beam search' if GROUPS == 1 else f'group beam search ({GROUPS} groups, diversity_penalty {DIVERSITY})'
    print(f'{what}, C5 decode shape: {B} prompts x {Tp}, num_beams {NB} ({B * NB} rows), {NEW} new tokens, eos never fires; '
          f'device ids == host ids: {same}')
    for host, name in ((False, 'device'), (True, 'host  ')):
        tps = sorted(B * NEW / t for t in times[host])
        print(f'{name}: {statistics.median(tps):9.1f} tok/s median of {RUNS} (min {tps[0]:.1f}, max {tps[-1]:.1f}); '
              f'{statistics.median(times[host]):.3f} s per call; {per_step[host]:.1f} library launches per step, '
              f'{f"{3 * GROUPS} host reads + {3 * GROUPS} uploads + {GROUPS} sync per step" if host else "no host read per step, one graph replay"}')
    d, h = sorted(B * NEW / t for t in times[False]), sorted(B * NEW / t for t in times[True])
    gap = statistics.median(d) / statistics.median(h)
    clear = d[0] > h[-1]
    print(f'device / host = {gap:.3f}x; the slowest device run is {"above" if clear else "NOT above"} the fastest host run '
          f'({d[0]:.1f} vs {h[-1]:.1f} tok/s): the gap {"exceeds" if clear else "does not exceed"} the run-to-run spread')
