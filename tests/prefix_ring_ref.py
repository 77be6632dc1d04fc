"""Host reference of the prompt-ring layout (csrc/decode_prefix.hip, generate(prompt_rings='shared')): where ring slot s of a row comes
from at step t, and the gather that rebuilds the ring the row would own in the copied mode.

A prompt of Tp positions sits in the prompt's ring (slot = position mod M, the last min(Tp, M) positions); position p >= Tp of a row
sits in slot (p - Tp) mod Mt of the row's tail ring.  Ring slot s stands, at step t, for the latest position <= t that maps to it."""
import torch

NEVER, PROMPT, TAIL = 'never', 'prompt', 'tail'

# (Tp, M, Mt, t) at M = 32: Tp below, at and above the ring length; the step before the first generated position (all prompt), the first
# step (t = Tp), t across the ring's wrap, t - Tp >= M (no prompt slot left) and beyond (the tail itself wrapped), and tails shorter
# than the ring (Mt < M) from their first to their last admissible step (t - Tp + 1 <= Mt)
CASES = [(Tp, 32, 32, t) for Tp, ts in ((5, (4, 5, 6, 20, 31, 32, 33, 36, 37, 40, 63, 64, 70, 101)),
                                       (32, (31, 32, 33, 40, 62, 63, 64, 65, 100)),
                                       (45, (44, 45, 46, 50, 63, 64, 76, 77, 95, 96, 120))) for t in ts]
CASES += [(5, 32, 16, t) for t in (5, 12, 20)] + [(32, 32, 16, t) for t in (32, 40, 47)] + [(45, 32, 16, t) for t in (45, 52, 60)]
# the same at M = 256, where a run of slots spans several load batches of the attention kernel and a ring piece is cut inside a run
LONG_CASES = [(100, 256, 256, t) for t in (100, 101, 200, 255, 256, 300, 355, 356, 500, 700)]
LONG_CASES += [(256, 256, 256, 400), (300, 256, 256, 430), (300, 256, 64, 300), (300, 256, 64, 363), (40, 256, 48, 87)]


def slot_source(t: int, Tp: int, M: int, Mt: int, s: int):
    """(NEVER, None) | (PROMPT, slot of the prompt's ring) | (TAIL, slot of the row's tail ring) for ring slot s at step t"""
    p = t - ((t - s) % M)              # the latest position <= t with p mod M == s
    if p < 0:
        return NEVER, None
    if p >= Tp:
        return TAIL, (p - Tp) % Mt
    return PROMPT, s


def gather_ring(prompt_ring: torch.Tensor, tail_ring: torch.Tensor, t: int, Tp: int, n: int, fill: float = 0.0) -> torch.Tensor:
    """prompt_ring (B0, H, M, dh), tail_ring (B0 * n, H, Mt, dh) -> (B0 * n, H, M, dh): the ring every row would own in the copied mode
    at step t; never-written slots hold `fill`"""
    B0, H, M, dh = prompt_ring.shape
    Mt = tail_ring.shape[2]
    out = torch.full((B0 * n, H, M, dh), fill, dtype=prompt_ring.dtype, device=prompt_ring.device)
    own = prompt_ring.repeat_interleave(n, 0)
    for s in range(M):
        kind, at = slot_source(t, Tp, M, Mt, s)
        if kind == PROMPT:
            out[:, :, s] = own[:, :, at]
        elif kind == TAIL:
            out[:, :, s] = tail_ring[:, :, at]
    return out
