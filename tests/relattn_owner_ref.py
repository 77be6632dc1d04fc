"""Cases and CPU models for the two dq forms of mxl_relattn_bwd_fused (tests/test_relattn_fused_owner_gpu.py; not a test module).

oracle/relattn_cases.build_case takes a named shape, so the owner-mode shapes -- chosen for the visit logic: a query tile seen by
one, two and three key blocks, a first visit that is not key block 0, M off the 256 grid, stored and phantom keys together, no
phantom term -- get their inputs here, in the layout relattn_ref64 takes.  `dq_models` (oracle/relattn_cases.py: arms 'fused' and
'fused_owner' of the operand-rounded model) evaluates both summations on the CPU: per-block mode rounds every key block's partial to
bf16 in front of the float32 sum, owner mode carries the float32 sum; both round the finished dq to bf16 once.
"""
import functools
import math

import torch

from oracle.kernel_cases import bf16_exact
from oracle.relattn_cases import dq_models, relattn_ref64      # noqa: F401  (dq_models: for the users of this module)

# name: (B, T, H, dh, M, Kc)
OWNER_SHAPES = {
    'mode_r': (2, 768, 2, 64, 768, 768),                 # three key blocks, 1 to 3 visits per tile
    'short_window': (2, 512, 2, 64, 96, 512),            # first visit is not key block 0; single-visit tiles
    'm_off_256': (2, 640, 2, 64, 608, 640),              # M not a multiple of 256
    'partial_mem': (2, 256, 2, 64, 512, 512),            # stored and phantom keys together
    'full_mem': (2, 256, 2, 64, 256, 512),               # oph = None: no phantom term
}


def build_owner_case(name, seed=0):
    B, T, H, dh, M, Kc = OWNER_SHAPES[name]
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(q=rn(B, T, H, dh) * 0.8, k=rn(B, Kc, H, dh) * 0.8, v=rn(B, Kc, H, dh) * 0.8, rd=rn(M, H, dh) * 0.8,
             rwb=rn(H, dh) * 0.5, rrb=rn(H, dh) * 0.5, dout=rn(B, T, H, dh))
    c = dict(shape=name, family='random', B=B, T=T, H=H, dh=dh, M=M, Kc=Kc, scale=1.0 / math.sqrt(dh))
    c.update({n: bf16_exact(x) for n, x in t.items()})
    return c


@functools.lru_cache(maxsize=None)
def owner_case_ref(name, seed=0):
    """-> (case, float64 reference): built once per process and shared; callers leave both unchanged"""
    c = build_owner_case(name, seed)
    return c, relattn_ref64(c)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()
