"""The ring-attention launch of a contrastive step at a full ring (B0 prompts x K candidates x 12 heads, M = 2048, dh = 64) in its
two forms: mxl_relattn_decode_split_live on the B0 * K ring copies (what runs under contrastive_rings='copied') and
mxl_relattn_decode_shared on the B0 rings (csrc/decode_shared.hip), each with the ring pieces ops.decode_ring_pieces gives its
workgroup count.  The forms are alternated, ROUNDS (7) rounds of N (30) launches each between device events, over rotating ring sets
so that nothing is served from the Infinity Cache; reports each form's median and min..max microseconds per launch, the bytes it
reads from the rings and the TB/s that makes, and the shared form's multiply-adds per second (it does the same K * M * dh * 2
per head as the copies, over 1 / K of the bytes when one group holds the K queries).

    python3 scripts/perf_decode_shared.py            # env: ROUNDS (7), N (30), B0 (8), K (16)
"""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd import ops
from symbolic_music_generation_amd.ops import _p, _stream, check, lib

dev = torch.device('cuda:0')
H, dh, M = 12, 64, 2048
B0, K = int(os.environ.get('B0', 8)), int(os.environ.get('K', 16))
ROUNDS, N = int(os.environ.get('ROUNDS', 7)), int(os.environ.get('N', 30))
B, d = B0 * K, H * dh
G = 4 if K <= 4 else 8
groups = (K + G - 1) // G
SETS = max(2, min(6, (1 << 30) // (B * H * M * dh * 2)))             # the copies' sets: up to 1 GiB per K or V
SETS_SH = 6
kc = [torch.randn(B0, H, M, dh, device=dev).bfloat16() for _ in range(SETS_SH)]
vc = [torch.randn(B0, H, M, dh, device=dev).bfloat16() for _ in range(SETS_SH)]
kcc = [kc[i].repeat_interleave(K, 0).contiguous() for i in range(SETS)]
vcc = [vc[i].repeat_interleave(K, 0).contiguous() for i in range(SETS)]
qkv = torch.randn(B, 3 * d, device=dev).bfloat16()
bd = torch.randn(B, H, M, device=dev)
rwb = torch.randn(H, dh, device=dev) * .1
out = torch.empty(B, d, device=dev, dtype=torch.bfloat16)
t_dev = torch.tensor([3 * M + 5], device=dev, dtype=torch.int32)
live = torch.ones(B, device=dev, dtype=torch.int32)
pieces = {'copies': ops.decode_ring_pieces(B, H, M), 'shared': ops.decode_ring_pieces(B0 * groups, H, M)}
split = {f: ops.relattn_decode_split_scratch(B, H, dh, p, dev) or (None, None) for f, p in pieces.items()}


def run(form, i, p=None):
    p = p or pieces[form]
    ws, arrived = split[form] if p == pieces[form] else ops.relattn_decode_split_scratch(B, H, dh, p, dev) or (None, None)
    if form == 'copies':
        check(lib().mxl_relattn_decode_split_live(_p(qkv), _p(kcc[i % SETS]), _p(vcc[i % SETS]), _p(bd), _p(rwb), _p(out), _p(t_dev), B, H,
                                                  dh, M, 0.125, p, _p(ws), _p(arrived), _p(live), _stream()), form)
    else:
        check(lib().mxl_relattn_decode_shared(_p(qkv), _p(kc[i % SETS_SH]), _p(vc[i % SETS_SH]), _p(bd), _p(rwb), _p(out), _p(t_dev), B0, K,
                                              H, dh, M, 0.125, p, _p(ws), _p(arrived), _p(live), _stream()), form)


# the contract, at one piece count: the copies hold the rows' own k / v in the step's slot, as mxl_kv_append leaves them
tm = int(t_dev) % M
for i in range(SETS):
    kcc[i][:, :, tm] = qkv[:, d:2 * d].view(B, H, dh)
    vcc[i][:, :, tm] = qkv[:, 2 * d:].view(B, H, dh)
outs = {}
for f in ('copies', 'shared'):
    run(f, 0, pieces['shared'])
    torch.cuda.synchronize()
    outs[f] = out.clone()
assert torch.equal(outs['copies'].view(torch.int16), outs['shared'].view(torch.int16)), 'shared rings: other bits than the copies'
FORMS = ('copies', 'shared')
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
ring = H * M * dh * 2 * 2                                                  # K and V of one row or prompt
byt = {'copies': B * ring, 'shared': B0 * groups * ring}
fma = B * H * M * dh * 2
print(f'ring attention of a contrastive step at a full ring: {B0} prompts x {K} candidates x {H} heads, M {M}, dh {dh}; {ROUNDS} alternated '
      f'rounds of {N} launches; shared output == output on the copies: True')
for f in FORMS:
    m = statistics.median(us[f])
    print(f'{f:7s}: {m:7.1f} us median (min {min(us[f]):.1f}, max {max(us[f]):.1f}), {pieces[f]} piece(s); reads {byt[f] / 1e6:7.1f} MB of rings, '
          f'{byt[f] / m / 1e6:5.2f} TB/s; {fma / m / 1e6:5.2f} T multiply-adds/s')
faster = max(us['shared']) < min(us['copies'])
print(f'shared / copies = {statistics.median(us["shared"]) / statistics.median(us["copies"]):.3f}x in time, {byt["shared"] / byt["copies"]:.3f}x '
      f'in ring bytes ({groups} group(s) of {G} queries read the ring {groups} time(s)); the slowest shared round is '
      f'{"below" if faster else "NOT below"} the fastest copies round')
