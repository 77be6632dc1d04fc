"""FP8 K/V rings against bf16 rings at the C5 decode shape of bench.py (12L/768d, M = 2048, V = 1190): 64 prompts of 256 tokens,
do_sample with top_k = 8, to 2048 tokens, through model.generate (two lanes of 32 rows, one captured graph each).

  bf16  generate(...)                         rings (B, H, M, dh) bf16; projection + append in one launch (mxl_decode_qkv)
  fp8   generate(..., kv_cache_dtype='fp8')   rings of e4m3fn bytes + one int8 exponent per slot and head; projection
                                              (mxl_gemm_skinny_bf16), mxl_kv_append_fp8, mxl_relattn_decode_fp8
  bf16x2  the bf16 rings with the projection and the append as two launches (mxl_gemm_skinny_bf16, mxl_kv_append): what the one
          launch per layer that the fp8 path has more costs, apart from everything else that differs

The three are alternated in one process on one device, RUNS (3) rounds after one warm-up call each; reports the median and the min..max
of the tokens per second (64 x 1792 new tokens per call), the allocated ring bytes of either decoder, and the ring attention launch's
time at a full ring for both (one lane's launch: 32 sequences x 12 heads, one piece, over 12 ring sets in turn so that no set is
served from a cache; median of REPS (20) rounds of 12 launches, timed with events).

    python3 scripts/perf_kv_fp8.py                # env: RUNS (3), REPS (20), TO (2048), ONLY_ATTN=1 (the launch timing alone)
"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd import ops
from symbolic_music_generation_amd.ops import _p, _stream, check, lib
from symbolic_music_generation_amd.transformer_xl import MyTransfoXLConfig, MyTransfoXLLMHeadModel

dev = torch.device('cuda:0')
V, M, B, Tp = 1190, 2048, 64, 256
RUNS, REPS, TO = int(os.environ.get('RUNS', 3)), int(os.environ.get('REPS', 20)), int(os.environ.get('TO', 2048))
ONLY_ATTN = os.environ.get('ONLY_ATTN') == '1'      # the launch timing alone (A/B builds of the library through MXL_LIB_PATH)
cfg = MyTransfoXLConfig('base', max_length=2048, vocab_size=V, mem_len=M, cutoffs=[])
model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()
ids = torch.randint(4, V, (B, Tp), generator=torch.Generator().manual_seed(77)).to(dev)
kw = dict(input_ids=ids, max_length=TO, do_sample=True, top_k=8, seed=77)
H, dh, L = model.engine.cfg.n_head, model.engine.cfg.d_head, model.engine.cfg.n_layer


def ring_bytes(dec):
    lanes = getattr(dec, 'lanes', [dec])
    return sum(t.numel() * t.element_size() for d in lanes for t in d.kc + d.vc + list(d.ke) + list(d.ve))


_fused_qkv = ops.decode_qkv


def _two_launches(x, wqkv, qkv, kc, vc, t_dev, rrb, qr_out, dh):
    """what mxl_decode_qkv fuses, as the two launches the fp8 path runs: projection, then append"""
    Bx, d = x.shape
    ops.gemm_skinny(x, wqkv, qkv, Bx, 3 * d, d)
    ops.kv_append(qkv, kc, vc, t_dev, rrb=rrb, qr_out=qr_out)


def run(arm: str):
    """one generate call on a new decoder (so every call captures its own step): 'bf16', 'fp8', or 'bf16x2' = bf16 rings with the
    projection and the append as two launches, which prices the one launch per layer the fp8 path has more"""
    model._decoder = None
    ops.decode_qkv = _two_launches if arm == 'bf16x2' else _fused_qkv
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(**kw, kv_cache_dtype='fp8' if arm == 'fp8' else None)
    torch.cuda.synchronize()
    ops.decode_qkv = _fused_qkv
    return time.perf_counter() - t0, out


def attn_launch_us():
    """the ring attention launch of one lane at a full ring, bf16 and fp8, microseconds per launch"""
    Bl = B // 2
    g = torch.Generator(device=dev).manual_seed(5)
    qkv = torch.randn(Bl, 3 * H * dh, device=dev, generator=g).to(torch.bfloat16)
    bd = torch.randn(Bl, H, M, device=dev, generator=g)
    rwb = torch.randn(H, dh, device=dev, generator=g) * 0.3
    out = torch.empty(Bl, H * dh, device=dev, dtype=torch.bfloat16)
    t_dev = torch.tensor([M + 100], device=dev, dtype=torch.int32)
    scale = dh ** -0.5
    res = {}
    for name in ('bf16', 'fp8'):
        if name == 'bf16':
            sets = [(torch.randn(Bl, H, M, dh, device=dev, generator=g).to(torch.bfloat16),
                     torch.randn(Bl, H, M, dh, device=dev, generator=g).to(torch.bfloat16)) for _ in range(L)]

            def launch(i):
                k, v = sets[i]
                check(lib().mxl_relattn_decode(_p(qkv), _p(k), _p(v), _p(bd), _p(rwb), _p(out), _p(t_dev), Bl, H, dh, M, scale, _stream()), 'attn')
        else:
            # magnitudes below 0x78 with a random sign bit: finite e4m3fn values; exponents around those of unit-scale rows
            mk = lambda: (torch.randint(0, 0x78, (Bl, H, M, dh), device=dev, generator=g)
                          | (torch.randint(0, 2, (Bl, H, M, dh), device=dev, generator=g) << 7)).to(torch.uint8)
            me = lambda: torch.randint(-9, -6, (Bl, H, M), device=dev, generator=g).to(torch.int8)
            sets = [(mk(), me(), mk(), me()) for _ in range(L)]

            def launch(i):
                k, ke, v, ve = sets[i]
                check(lib().mxl_relattn_decode_fp8(_p(qkv), _p(k), _p(ke), _p(v), _p(ve), _p(bd), _p(rwb), _p(out), _p(t_dev), Bl, H, dh, M,
                                                   scale, 1, None, None, None, _stream()), 'attn fp8')
        for i in range(L):
            launch(i)
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(L):
                launch(i)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1000 / L)
        nbytes = sum(t.numel() * t.element_size() for t in sets[0])
        res[name] = (statistics.median(ts), min(ts), max(ts), nbytes)
        del sets
    return res


with torch.no_grad():
    new = B * (TO - Tp)
    ARMS = ('bf16', 'bf16x2', 'fp8')
    sizes, times = {}, {a: [] for a in ARMS}
    for arm in ARMS if not ONLY_ATTN else ():
        run(arm)
        sizes[arm] = ring_bytes(model._decoder)
    for _ in range(RUNS if not ONLY_ATTN else 0):
        for arm in ARMS:
            times[arm].append(run(arm)[0])
    if not ONLY_ATTN:
        print(f'C5 decode shape: {B} prompts x {Tp}, top_k 8, to {TO} tokens ({new} new tokens per call), {RUNS} alternating rounds')
        tps = {a: sorted(new / t for t in times[a]) for a in ARMS}
        for arm in ARMS:
            print(f'{arm:6s}: {statistics.median(tps[arm]):9.1f} tok/s median of {RUNS} (min {tps[arm][0]:.1f}, max {tps[arm][-1]:.1f}); '
                  f'{statistics.median(times[arm]):.3f} s per call; rings {sizes[arm] / 1e9:.3f} GB')
        clear = tps['fp8'][0] > tps['bf16'][-1]
        print(f'fp8 / bf16 = {statistics.median(tps["fp8"]) / statistics.median(tps["bf16"]):.3f}x; the slowest fp8 run is '
              f'{"above" if clear else "NOT above"} the fastest bf16 run ({tps["fp8"][0]:.1f} vs {tps["bf16"][-1]:.1f} tok/s)')
        print(f'one launch per layer more (bf16x2 / bf16) = {statistics.median(tps["bf16x2"]) / statistics.median(tps["bf16"]):.4f}x: '
              f'{(statistics.median(times["bf16x2"]) - statistics.median(times["bf16"])) / (TO - Tp) * 1e6:+.1f} us per step of '
              f'{statistics.median(times["bf16"]) / (TO - Tp) * 1e6:.0f}')
        print(f'ring bytes fp8 / bf16 = {sizes["fp8"] / sizes["bf16"]:.4f} ((dh + 1) / (2 dh) = {(dh + 1) / (2 * dh):.4f})')
    model._decoder = None
    torch.cuda.empty_cache()
    for name, (med, lo, hi, nbytes) in attn_launch_us().items():
        print(f'ring attention launch, full ring, {B // 2} x {H} rings, {name}: {med:.1f} us median (min {lo:.1f}, max {hi:.1f}); '
              f'{nbytes / 1e6:.1f} MB of rings per launch -> {nbytes / med / 1e6:.2f} TB/s')
