"""The ring-attention launch of one lane at a full ring (32 rows x 12 heads, M = 2048, dh = 64: 8 items of nb = 4 beams), in three
forms: the existing entry (mxl_relattn_decode), the owned entry with the identity table (what the indirection itself costs) and
the owned entry with a scrambled table, every slot drawn from a random sibling (the worst locality: a workgroup's stream is cut
into 128-byte rows of four rings).  The forms are alternated, ROUNDS (7) rounds of N (30) launches each between device events, over
six rotating ring sets so that nothing is served from the Infinity Cache; reports each form's median and min..max microseconds
per launch and streamed TB/s, and whether the identity form's fastest round is slower than the existing form's slowest.

The same three forms over FP8 rings of the same shape (e4m3fn bytes, one int8 exponent per slot and head: (dh + 1) / (2 dh) of the
bytes) ride in the same rounds: mxl_relattn_decode_fp8, and mxl_relattn_decode_fp8_owned with the identity and the scrambled table.

    python3 scripts/perf_decode_owned.py            # env: ROUNDS (7), N (30), B (32), NB (4)
"""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd.ops import _p, _stream, check, lib

dev = torch.device('cuda:0')
H, dh, M = 12, 64, 2048
B, nb = int(os.environ.get('B', 32)), int(os.environ.get('NB', 4))
ROUNDS, N, SETS = int(os.environ.get('ROUNDS', 7)), int(os.environ.get('N', 30)), 6
d = H * dh
kc = [torch.randn(B, H, M, dh, device=dev).bfloat16() for _ in range(SETS)]
vc = [torch.randn(B, H, M, dh, device=dev).bfloat16() for _ in range(SETS)]
qkv = torch.randn(B, 3 * d, device=dev).bfloat16()
bd = torch.randn(B, H, M, device=dev)
rwb = torch.randn(H, dh, device=dev) * .1
out = torch.empty(B, d, device=dev, dtype=torch.bfloat16)
t_dev = torch.tensor([3 * M + 5], device=dev, dtype=torch.int32)
ident = (torch.arange(B, device=dev) % nb).to(torch.uint8)[:, None].expand(B, M).contiguous()
scrambled = torch.randint(0, nb, (B, M), device=dev, generator=torch.Generator(device=dev).manual_seed(5)).to(torch.uint8)
# fp8 rings: finite e4m3fn bytes (magnitude field below 0x7F, any sign) and exponents in -3 .. 3
fp8_bytes = lambda: (torch.randint(0, 0x7F, (B, H, M, dh), device=dev) | (torch.randint(0, 2, (B, H, M, dh), device=dev) << 7)).to(torch.uint8)
kc8, vc8 = [fp8_bytes() for _ in range(SETS)], [fp8_bytes() for _ in range(SETS)]
ke = [torch.randint(-3, 4, (B, H, M), device=dev).to(torch.int8) for _ in range(SETS)]
ve = [torch.randint(-3, 4, (B, H, M), device=dev).to(torch.int8) for _ in range(SETS)]


def run(form, i):
    if form.startswith('fp8'):
        rings = (_p(kc8[i % SETS]), _p(ke[i % SETS]), _p(vc8[i % SETS]), _p(ve[i % SETS]))
        tail = (_p(bd), _p(rwb), _p(out), _p(t_dev), B, H, dh, M, 0.125, 1, 0, 0, 0, _stream())
        if form == 'fp8':
            check(lib().mxl_relattn_decode_fp8(_p(qkv), *rings, *tail), form)
        else:
            own = ident if form == 'fp8_identity' else scrambled
            check(lib().mxl_relattn_decode_fp8_owned(_p(qkv), *rings, _p(own), nb, *tail), form)
        return
    k, v = kc[i % SETS], vc[i % SETS]
    if form == 'existing':
        check(lib().mxl_relattn_decode(_p(qkv), _p(k), _p(v), _p(bd), _p(rwb), _p(out), _p(t_dev), B, H, dh, M, 0.125, _stream()), form)
    else:
        own = ident if form == 'identity' else scrambled
        check(lib().mxl_relattn_decode_owned(_p(qkv), _p(k), _p(v), _p(own), nb, _p(bd), _p(rwb), _p(out), _p(t_dev), B, H, dh, M, 0.125,
                                             1, 0, 0, 0, _stream()), form)


FORMS = ('existing', 'identity', 'scrambled', 'fp8', 'fp8_identity', 'fp8_scrambled')
outs = {}
for f in FORMS:
    for i in range(3):
        run(f, i)
    run(f, 0)
    torch.cuda.synchronize()
    outs[f] = out.clone()
assert torch.equal(outs['existing'].view(torch.int16), outs['identity'].view(torch.int16)), 'identity table: other bits'
assert torch.equal(outs['fp8'].view(torch.int16), outs['fp8_identity'].view(torch.int16)), 'fp8 identity table: other bits'
assert torch.isfinite(outs['fp8_scrambled'].float()).all()
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
byt = B * H * M * dh * 2 * 2
byt8 = B * H * M * (dh + 1) * 2
print(f'ring attention, one lane at a full ring: {B} rows ({B // nb} items x {nb} beams) x {H} heads, M {M}, dh {dh}; '
      f'{ROUNDS} alternated rounds of {N} launches; identity-table output == existing output: True')
for f in FORMS:
    m = statistics.median(us[f])
    print(f'{f:13s}: {m:7.1f} us median (min {min(us[f]):.1f}, max {max(us[f]):.1f})  {(byt8 if f.startswith("fp8") else byt) / m / 1e6:5.2f} TB/s')
slower = min(us['identity']) > max(us['existing'])
print(f'identity / existing = {statistics.median(us["identity"]) / statistics.median(us["existing"]):.3f}x, scrambled / existing = '
      f'{statistics.median(us["scrambled"]) / statistics.median(us["existing"]):.3f}x; the fastest identity round is '
      f'{"above" if slower else "NOT above"} the slowest existing round: the indirection {"costs more" if slower else "does not cost more"} '
      'than the run-to-run spread')
slower = min(us['fp8_identity']) > max(us['fp8'])
faster = max(us['fp8_identity']) < min(us['identity'])
print(f'fp8 rings ({byt8 / byt:.3f} of the bytes): fp8_identity / fp8 = {statistics.median(us["fp8_identity"]) / statistics.median(us["fp8"]):.3f}x, '
      f'fp8_scrambled / fp8 = {statistics.median(us["fp8_scrambled"]) / statistics.median(us["fp8"]):.3f}x; the fastest fp8_identity round is '
      f'{"above" if slower else "NOT above"} the slowest fp8 round; fp8_identity / identity = '
      f'{statistics.median(us["fp8_identity"]) / statistics.median(us["identity"]):.3f}x, the slowest fp8_identity round is '
      f'{"below" if faster else "NOT below"} the fastest identity round')
