"""Sampling n variations of a prompt, `generate(do_sample=True, num_return_sequences=n)`, in its two ring modes (generate(prompt_rings=)):
'copied', every row owns a full set of rings and the prompt pass runs on all rows, and 'shared', one set of prompt rings per prompt and
a tail ring per row (mxl_kv_append_tail / mxl_relattn_decode_prefix, csrc/decode_prefix.hip).  C5 decode shape of bench.py (12L/768d,
M = 2048, V = 1190, randomly initialised weights), top_k = 8, 256 new tokens, at

  p1n16   1 prompt  x 16 variations      p8n8   8 prompts x 8      p8n16   8 prompts x 16      with 256-token prompts
  ...full                                the same three with 2048-token prompts: a full ring from the first step

The two modes are alternated in one process on one device, RUNS (5) times each after one warm-up each.  Two numbers per run:
  decode   generated tokens per second over the replayed steps alone (decoder.begin, then the timed replay_once loop)
  wall     seconds of the whole model.generate call to the returned ids -- decoder, prompt pass, capture and steps; this is where the
           n-fold prompt pass shows
Reports the slowest..fastest of each, the ring bytes of either mode computed from the shapes, whether the ids agree (they must where both
decoders cut the ring into the same number of pieces; elsewhere the attention outputs may differ in the last bf16 bit and the first
differing column is reported), and calls a shape "faster" only where the slowest shared run beats the fastest copied run.

    python3 scripts/perf_variations.py               # env: RUNS (5), NEW (256), ONLY (p1n16 | p8n8 | p8n16 | p1n16full | ...)

MODE=attn times the attention launch alone at a full ring (Tp = M = 2048, dh = 64, 12 heads): mxl_relattn_decode_split_live on the
B0 * n ring copies against mxl_relattn_decode_prefix on the B0 prompt rings and B0 * n tails, each with the ring pieces
ops.decode_ring_pieces gives its workgroup count, with 1, 256 and 2048 generated positions in the window (a tail of one slot, the end of
the runs above, and no prompt slot left).  Alternated, ROUNDS (7) rounds of N (30) launches between device events over rotating ring
sets; the outputs are held equal at one piece count first.

    MODE=attn python3 scripts/perf_variations.py     # env: ROUNDS (7), N (30), B0 (8), NV (16)
"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd import generate as G
from symbolic_music_generation_amd import ops

dev = torch.device('cuda:0')
V, M = 1190, 2048
NEW, RUNS = int(os.environ.get('NEW', 256)), int(os.environ.get('RUNS', 5))
SHAPES = {'p1n16': (1, 16, 256), 'p8n8': (8, 8, 256), 'p8n16': (8, 16, 256), 'p1n16full': (1, 16, M), 'p8n8full': (8, 8, M),
          'p8n16full': (8, 16, M)}
MODES = ('copied', 'shared')


def generation():
    from symbolic_music_generation_amd.transformer_xl import MyTransfoXLConfig, MyTransfoXLLMHeadModel
    cfg = MyTransfoXLConfig('base', max_length=M + NEW, vocab_size=V, mem_len=M, cutoffs=[])
    model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()
    c = model.engine.cfg
    slot = c.n_head * c.d_head * 2 * 2 * c.n_layer                              # bytes of one K and one V slot of every layer
    sampling = G.sampling_config(True, 8, None, 1.0, None, None)

    def wall(kw, mode):
        model._decoder = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(**kw, prompt_rings=mode)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def decode(ids, n, mode):
        """the steps alone, on the decoder generate builds for the mode"""
        B0, tp = ids.shape
        rows, L = B0 * n, tp + NEW
        lanes = 2 if rows >= 32 else 1
        more = {}
        if mode == 'shared':
            lanes = min(lanes, B0)
            more = dict(prompt_rings=n, tail_len=NEW)
        dec = (G.XLDecoderLanes(model.engine, rows, L, seed=77, lanes=lanes, **more) if lanes > 1
               else G.XLDecoder(model.engine, rows, L, seed=77, **more))
        steps = dec.begin(ids.repeat_interleave(n, 0), L, sampling, True, None, G.NO_RULES)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            dec.replay_once()
        if lanes > 1:
            dec.join()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        pieces = getattr(dec, 'lanes', [dec])[0].pieces
        return rows * steps / t, pieces, lanes

    for name, (B0, n, tp) in SHAPES.items():
        if os.environ.get('ONLY', name) != name:
            continue
        ids = torch.randint(4, V, (B0, tp), generator=torch.Generator().manual_seed(77)).to(dev)
        kw = dict(input_ids=ids, max_length=tp + NEW, do_sample=True, top_k=8, num_return_sequences=n, seed=77)
        rows = B0 * n
        mem = {'copied': rows * M * slot, 'shared': (B0 * M + rows * G.prompt_tail_len(M, NEW)) * slot}
        outs, info = {}, {}
        for mode in MODES:                                                      # warm-up of either mode
            outs[mode] = wall(kw, mode)[1]
            info[mode] = decode(ids, n, mode)[1:]
        same = torch.equal(outs['copied'], outs['shared'])
        assert same or info['copied'] != info['shared'], f'{name}: the ids of the two ring modes differ at equal piece and lane counts'
        agree = int((outs['copied'] == outs['shared']).all(0).int().cumprod(0).sum()) - tp
        walls, tps = {m: [] for m in MODES}, {m: [] for m in MODES}
        for _ in range(RUNS):
            for mode in MODES:
                t, out = wall(kw, mode)
                assert torch.equal(out, outs[mode])
                walls[mode].append(t)
                tps[mode].append(decode(ids, n, mode)[0])
        print(f'sampling [{name}], C5 decode shape: {B0} prompt(s) x {tp} tokens x {n} variations ({rows} rows), top_k 8, {NEW} new tokens, '
              f'captured step; shared ids == copied ids: {same}' + ('' if same else f' (the first {agree} of {NEW} generated columns agree)'))
        for mode in MODES:
            d, w = sorted(tps[mode]), sorted(walls[mode])
            print(f'{mode:6s}: decode {d[0]:9.1f} .. {d[-1]:9.1f} tok/s (median {statistics.median(d):9.1f}); wall {w[0]:.3f} .. {w[-1]:.3f} s to '
                  f'the ids (median {statistics.median(w):.3f}); rings {mem[mode] / 1e6:8.1f} MB; {info[mode][0]} ring piece(s), '
                  f'{info[mode][1]} lane(s)')
        for what, val in (('decode', tps), ('wall', {m: [1 / t for t in walls[m]] for m in MODES})):
            c_, s_ = sorted(val['copied']), sorted(val['shared'])
            verdict = 'faster' if s_[0] > c_[-1] else ('slower' if s_[-1] < c_[0] else 'level')
            print(f'{what}: shared / copied = {statistics.median(s_) / statistics.median(c_):.3f}x in rate; the slowest shared run against the '
                  f'fastest copied run: shared is {verdict}')
        print(f'ring memory: shared / copied = {mem["shared"] / mem["copied"]:.3f}x')


def attention():
    from symbolic_music_generation_amd.ops import _p, _stream, check, lib
    H, dh = 12, 64
    B0, n = int(os.environ.get('B0', 8)), int(os.environ.get('NV', 16))
    ROUNDS, N = int(os.environ.get('ROUNDS', 7)), int(os.environ.get('N', 30))
    B, d, Tp = B0 * n, H * dh, M
    Gq = 4 if n <= 4 else 8
    groups = ops.prefix_attn_groups(n)
    SETS = max(2, min(6, (1 << 30) // (B * H * M * dh * 2)))             # ring sets: up to 1 GiB per K or V, past the Infinity Cache
    qkv = torch.randn(B, 3 * d, device=dev).bfloat16()
    bd = torch.randn(B, H, M, device=dev)
    rwb = torch.randn(H, dh, device=dev) * .1
    out = torch.empty(B, d, device=dev, dtype=torch.bfloat16)
    t0_dev = torch.tensor([Tp], device=dev, dtype=torch.int32)
    live = torch.ones(B, device=dev, dtype=torch.int32)
    pieces = {'copies': ops.decode_ring_pieces(B, H, M), 'prefix': ops.decode_ring_pieces(B0 * groups, H, M)}
    split = {f: ops.relattn_decode_split_scratch(B, H, dh, p, dev) or (None, None) for f, p in pieces.items()}
    print(f'ring attention of a sampling step at a full ring: {B0} prompts x {n} variations x {H} heads, M {M}, dh {dh}, prompt of {Tp}; '
          f'{ROUNDS} alternated rounds of {N} launches over {SETS} ring sets')
    for gen in (1, 256, M):
        t, Mt = Tp + gen - 1, G.prompt_tail_len(M, gen)
        t_dev = torch.tensor([t], device=dev, dtype=torch.int32)
        kp = [torch.randn(B0, H, M, dh, device=dev).bfloat16() for _ in range(SETS)]
        vp = [torch.randn(B0, H, M, dh, device=dev).bfloat16() for _ in range(SETS)]
        kt = [torch.randn(B, H, Mt, dh, device=dev).bfloat16() for _ in range(SETS)]
        vt = [torch.randn(B, H, Mt, dh, device=dev).bfloat16() for _ in range(SETS)]
        # the copies: the ring every row would own, slot by slot from the source the layout names
        src = torch.tensor([(t - ((t - s) % M)) for s in range(M)], device=dev)
        tail, at = src >= Tp, (src - Tp) % Mt
        kcc, vcc = [], []
        for i in range(SETS):
            for own, tl, to in ((kp[i], kt[i], kcc), (vp[i], vt[i], vcc)):
                ring = own.repeat_interleave(n, 0).contiguous()
                ring[:, :, tail] = tl[:, :, at[tail]]
                to.append(ring)

        def run(form, i, p=None):
            p = p or pieces[form]
            ws, arrived = split[form] if p == pieces[form] else ops.relattn_decode_split_scratch(B, H, dh, p, dev) or (None, None)
            if form == 'copies':
                check(lib().mxl_relattn_decode_split_live(_p(qkv), _p(kcc[i % SETS]), _p(vcc[i % SETS]), _p(bd), _p(rwb), _p(out), _p(t_dev),
                                                          B, H, dh, M, 0.125, p, _p(ws), _p(arrived), _p(live), _stream()), form)
            else:
                j = i % SETS
                check(lib().mxl_relattn_decode_prefix(_p(qkv), _p(kp[j]), _p(vp[j]), _p(kt[j]), _p(vt[j]), _p(bd), _p(rwb), _p(out), _p(t_dev),
                                                      _p(t0_dev), B0, n, H, dh, M, Mt, 0.125, p, _p(ws), _p(arrived), _p(live), _stream()), form)
        outs = {}
        for f in ('copies', 'prefix'):                                         # the contract, at one piece count
            run(f, 0, pieces['prefix'])
            torch.cuda.synchronize()
            outs[f] = out.clone()
        assert torch.equal(outs['copies'].view(torch.int16), outs['prefix'].view(torch.int16)), 'prompt rings: other bits than the copies'
        FORMS = ('copies', 'prefix')
        for f in FORMS:
            for i in range(3):
                run(f, i)
        us = {f: [] for f in FORMS}
        for _ in range(ROUNDS):
            for f in FORMS:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for i in range(N):
                    run(f, i)
                e.record()
                torch.cuda.synchronize()
                us[f].append(s.elapsed_time(e) / N * 1e3)
        g = min(gen, M)
        slot = H * dh * 2 * 2                                                  # K and V of one slot, all heads
        byt = {'copies': B * M * slot, 'prefix': (B0 * groups * (M - g) + B * g) * slot}
        print(f'{gen} generated position(s) in the window (tail rings of {Mt} slots); prefix output == output on the copies: True')
        for f in FORMS:
            m = statistics.median(us[f])
            print(f'  {f:6s}: {m:7.1f} us median (min {min(us[f]):.1f}, max {max(us[f]):.1f}), {pieces[f]} piece(s); reads {byt[f] / 1e6:7.1f} MB '
                  f'of rings, {byt[f] / m / 1e6:5.2f} TB/s')
        verdict = 'faster' if max(us['prefix']) < min(us['copies']) else ('slower' if min(us['prefix']) > max(us['copies']) else 'level')
        print(f'  prefix / copies = {statistics.median(us["prefix"]) / statistics.median(us["copies"]):.3f}x in time, '
              f'{byt["prefix"] / byt["copies"]:.3f}x in ring bytes ({groups} group(s) of {Gq} queries); slowest against fastest round: prefix is '
              f'{verdict}')
        del kp, vp, kt, vt, kcc, vcc


with torch.no_grad():
    attention() if os.environ.get('MODE') == 'attn' else generation()
