"""Numpy model of the owner table of indexed rings (include/musicxl.h, mxl_beam_owner_follow), and of the two ways a beam search keeps
its K/V rings: copy whole ring rows every step, or never copy and gather by the table.  Test infrastructure, not product code.

owner[r][s] = j: slot s of row r's history is held in the ring of row (r // nb) * nb + j.  A step is: select (src per row), follow,
mark, the position moves on, every row writes slot t mod M of its OWN ring."""
import numpy as np


def identity(rows, nb, M):
    """the table after the prompt pass: every row holds its own prompt"""
    return np.repeat((np.arange(rows) % nb).astype(np.uint8)[:, None], M, 1)


def follow(owner, nb, beam_idx, moved, t, mark='always'):
    """one mxl_beam_owner_follow launch -> the new table.  beam_idx (rows,) absolute source rows, moved (rows // nb,), t the position
    before the advance.  mark: 'always' (the rule), or 'moved' -- the broken model that marks only the items it permuted."""
    rows, M = owner.shape
    new = owner.copy()
    for b in range(rows // nb):
        r0 = b * nb
        if moved[b]:
            for j in range(nb):
                s = int(beam_idx[r0 + j]) - r0
                if 0 <= s < nb:
                    new[r0 + j] = owner[r0 + s]
        if mark == 'always' or moved[b]:
            new[r0:r0 + nb, (t + 1) % M] = np.arange(nb, dtype=np.uint8)
    return new


def gather(rings, owner, nb):
    """the effective rings: out[r, s] = rings[(r // nb) * nb + owner[r, s], s]; rings (rows, M, ...)"""
    rows, M = owner.shape
    base = (np.arange(rows) // nb * nb)[:, None]
    return rings[base + owner.astype(np.int64), np.arange(M)[None, :]]


def run(srcs, nb, M, Tp, mark='always'):
    """Both bookkeepings over the steps `srcs` (each (rows,) absolute source rows) from a prompt of Tp positions: yields, per step,
    (t, copied rings, effective indexed rings) after the step's write.  A ring holds one integer per slot: the id of the (row, position)
    that wrote it, 0 = never written."""
    rows = len(srcs[0])
    tag = lambda t: (t + 1) * rows + np.arange(rows) + 1
    copied = np.zeros((rows, M), dtype=np.int64)
    for p in range(max(0, Tp - M), Tp):
        copied[:, p % M] = tag(p)
    kept, owner, t = copied.copy(), identity(rows, nb, M), Tp - 1
    ident = np.arange(rows)
    for src in srcs:
        src = np.asarray(src)
        moved = (src != ident).reshape(-1, nb).any(1)
        copied = copied[src]                                  # mxl_beam_reorder (an unmoved item is the identity)
        owner = follow(owner, nb, src, moved, t, mark)
        t += 1
        copied[:, t % M] = tag(t)                             # the forward pass: every row appends to its own ring
        kept[:, t % M] = tag(t)
        yield t, copied, gather(kept, owner, nb)
