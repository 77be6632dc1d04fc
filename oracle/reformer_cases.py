"""ORACLE-side statement of the Reformer training kernels of csrc/reformer.hip in float64 (test infrastructure, NOT product code),
the model of the roundings those kernels make, and the cases a CPU test and a GPU test share.

`attn_ref64(c)` is the closed form of the chunked attention, forward and backward, in slot order (csrc/ = symbolic_music_generation_amd/csrc/):

    slots s = 0 .. S-1, S = n_h T (sorted order for LSH, identity for local); chunk = 64 slots; the queries of chunk c see the 128 keys
    of chunks (c - 1 mod NC, c) -- circular, so chunk 0 looks back at the last chunk and, with n_h > 1, the first chunk of a round at
    the last chunk of the round before.  T <= 64: one chunk of T slots that sees itself only (the single-chunk kernels).
    x[s,k] = f_k (q_s . x_k)      local: f = 1 / sqrt(dh)      LSH: x = the shared qk, f_k = rsqrt(mean(x_k^2) + 1e-6) / sqrt(dh)
    causal mask on ORIGINAL positions (pos_q >= pos_k, else -1e9), then, LSH only, the self mask (pos_q == pos_k -> -1e5)
    lse = logsumexp_k x       P = exp(x - lse)       Pd = keep P / (1 - p)       out = Pd v
    delta = dO . out          dP = dO . v            dS = P (keep dP / (1 - p) - delta) + dlse P     (0 on masked cells: constant score)
    dq_s = sum_k dS f_k x_k   dv_k = sum_s Pd dO_s   dk'_k = sum_s dS q_s  (LSH: w.r.t. the EFFECTIVE key k' = f_k x_k)   local: dk = f dk'
    dk', dv (and dq) are per (round, position): one (T, d) slab per hash round.
    dqk = sum_r dq_r + f sum_r dk'_r - x (sum_r dk'_r . x) (m + 1e-6)^(-3/2) / dh^(3/2),  m = mean(x^2)      (the key-normalisation chain)

tests/test_reformer_cases_cpu.py pins it on float64 autograd through oracle.reformer_ref.chunked_attention (p = 0) and through the
written forward above (with dropout, the single-chunk form, the key chain).

`attn_ref64(c, rounded=True)` is the same evaluation with the roundings the kernels make and nothing else.  It is NOT the expected
value: `gap(model, ref)` measures what those roundings cost on a case, and 4 x the largest gap is the absolute term `b` of the
tolerance rule of oracle/kernel_cases.py.  The roundings, with their sources (reformer.hip):
  chunked kernels (T > 64)
    the key factor f and the scores q . x in float32 (MFMA float32 accumulators; modelled by a sequential float32 sum)   :487, :530-534, :543
    exponentials (__expf = 2^(x log2e), the product a float32) and their row sum in float32, lse = mx + __logf(sum) as float32   :554-559
    the unnormalised exponentials (after dropout) rounded to bf16 before P V; 1 / sum and 1 / (1 - p) applied once to O   :572-585, :557
    out stored as bf16 (:608), and delta formed from that stored out and the bf16 dout                                  :655, :837
    P = exp(x - lse) from the stored float32 lse                                                                        :697, :904
    dS f rounded to bf16 before the dq product (:719); Pd and dS (local: dS f) rounded to bf16 before dv / dk'          :923-926
    dq, dk', dv stored as float32 slabs (:756, :982-984) or, n_h == 1, as bf16 (dq16 / dk16 / dv16)                     :748, :981-983
  single-chunk kernels (T <= 64): everything in float32, sequential sums in the kernel's own order; delta = sum_j P dPd, not from the
    stored out; out bf16, gradients float32 or bf16                                                                    :1164-1257
  key-normalisation chain: float32 throughout, dqk (and the summed dv) stored as bf16                                  :1024-1039, :1021
  hash-round combine: float32, out / dout_r bf16, dlse float32, the backward reads the STORED bf16 out                  :1052-1066, :1084-1105
  axial embedding: float32 products and sums, out bf16; tables accumulated in float32 (sequential sum modelled)          :27-33, :44-54, :94-100

Arms of mxl_chunk_attn_fwd / mxl_chunk_attn_bwd / mxl_lsh_keynorm_bwd[_rounds] (reformer.hip:1357-1430) -> cases that take them:
    T <= 64, launch_single<16|32|64>, forward and backward, local and LSH ....... SINGLE_CASES s_t{1,7,33,64}_dh{16,32,64}_{loc,lsh}
    T > 64,  launch_chunk<16> ................................................... c_loc_t256_dh16, c_loc_t192_dh16_p50, c_lsh_t128_n3_dh16,
                                                                                   c_lsh_t192_n1_dh16, c_lsh_t256_n2_dh16_desc_p50
             launch_chunk<32> ................................................... c_loc_t192_dh32, c_lsh_t128_n2_dh32_dup, c_lsh_t256_n1_dh32_desc,
                                                                                   c_lsh_t128_n1_dh32_dom_p10
             launch_chunk<64> ................................................... c_loc_t128_dh64, c_loc_t128_dh64_dom_p50, c_lsh_t128_n1_dh64,
                                                                                   c_lsh_t192_n2_dh64_p10, c_lsh_t256_n3_dh64
    lsh = 0 / lsh = 1 ........................................................... c_loc_* / c_lsh_*
    n_h = 1 / 2 / 3 (float32 slabs; dlse given when n_h > 1) .................... *_n1_* and c_loc_* / *_n2_* / *_n3_*
    dq16 / dk16 / dv16 (n_h == 1 only) .......................................... every n_h == 1 case, chunked and single
    mxl_lsh_keynorm_bwd (one slab) .............................................. every LSH case with n_h == 1
    mxl_lsh_keynorm_bwd_rounds, dv == null / dv given ........................... every LSH case (n_h = 1, 2, 3), both forms
    xcd_block, groups % 8 == 0 / otherwise ...................................... (B, H) = (2, 4) / (1, 1), (3, 3)
    odd NC (the last workgroup of the forward and query-owner grids has one live chunk)   *_t192_*
Not reachable from these entry points: dh other than 16 / 32 / 64 (MXL_EUNSUPPORTED) and the MXL_EINVAL argument checks.
"""
import functools
import math
import zlib

import numpy as np
import torch

from oracle.kernel_cases import (axial_emb_mask, axial_pos_mask, bf16_exact, chunk_drop_mask, single_drop_mask)

SC_MAXT = 64
ATTN_OUTPUTS = ('out', 'lse', 'dq', 'dk', 'dv')


def _bf(x):
    return x.float().to(torch.bfloat16).double()


def _f32(x):
    return x.float().double()


def _id(x):
    return x


LOG2E_F32 = float(np.float32(1.4426950408889634))
LN2_F32 = float(np.float32(0.6931471805599453))


def _expf(x):
    """the fast exponential of the kernels (__expf): 2^(x log2e) with the product rounded to float32, the result a float32"""
    return _f32(torch.exp2(_f32(_f32(x) * LOG2E_F32)))


def _logf(x):
    """the fast logarithm (__logf): log2(x) ln2, both steps float32"""
    return _f32(_f32(torch.log2(x)) * LN2_F32)


def _seqmm32(a, b):
    """a (..., m, k) @ b (..., k, n) with ONE sequential float32 accumulator over k (the least favourable order) -> float64"""
    a32, b32 = a.float(), b.float()
    acc = torch.zeros(a32.shape[:-1] + (b32.shape[-1],), dtype=torch.float32)
    for i in range(a32.shape[-1]):
        acc += a32[..., :, i, None] * b32[..., i, None, :]
    return acc.double()


def _seqsum32(x):
    """sequential float32 sum over the last dimension -> float64"""
    x32 = x.float()
    acc = torch.zeros(x32.shape[:-1], dtype=torch.float32)
    for i in range(x32.shape[-1]):
        acc += x32[..., i]
    return acc.double()


def dscale_of(p):
    """1 / (1 - p) as the kernels form it (float32 p, float32 quotient)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


# ----------------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------------
def slot_positions(c):
    """(B, H, S) original position of every slot"""
    B, T, H, n_h = c['B'], c['T'], c['H'], c['n_h']
    if c['spos'] is not None:
        return c['spos'].long()
    return torch.arange(n_h * T).view(1, 1, -1).expand(B, H, -1)


def attn_keep(c, swap_parity=False):
    """the keep mask of a case as numpy says it: (B, H, NC, C, W) bool over (chunk, query in chunk, key in window); None without dropout"""
    B, T, H, n_h, p = c['B'], c['T'], c['H'], c['n_h'], c['p']
    if p <= 0:
        return None
    S = n_h * T
    if T <= SC_MAXT:
        return torch.from_numpy(single_drop_mask(c['seed'], c['site'], B, H, T, p)).view(B, H, 1, T, T)
    m = chunk_drop_mask(c['seed'], c['site'], np.arange(B * H * S, dtype=np.uint64), p, 128, swap_parity)
    return torch.from_numpy(m).view(B, H, S // 64, 64, 128)


def attn_ref64(c, rounded=False, edit=(), delta_unrounded=False):
    """c: a case (dict from `build_attn_case`).  -> dict of float64 tensors in the kernels' layouts: out (B, n_h, T, H, dh),
    lse (B, n_h, H, T), dq / dk / dv (B, n_h, T, H, dh) [dk: w.r.t. the effective key for LSH], and, LSH, dqk (B, T, H, dh) and
    dv_sum (B, T, H, dh); P, keep (B, H, NC, C, W) and live (same shape) for the tests of the cases' conditions.
    `edit`: faults the CPU test plants in the REFERENCE ('no_wrap', 'self_first', 'mask_shift', 'parity_swap', 'no_keyfac_chain',
    'drop_round').  `delta_unrounded` (rounded model only): delta from the float32 O instead of the stored bf16 out."""
    B, T, H, dh, n_h, lsh, p = (c[n] for n in ('B', 'T', 'H', 'dh', 'n_h', 'lsh', 'p'))
    S = n_h * T
    single = T <= SC_MAXT
    C = T if single else 64
    NC = S // C
    all32 = rounded and single                     # the single-chunk kernels: float32 everywhere
    r32 = _f32 if all32 else _id
    mm = _seqmm32 if all32 else torch.matmul
    rsum = _seqsum32 if all32 else (lambda t: t.sum(-1))
    q = c['q'].double().permute(0, 2, 1, 3)       # (B, H, T, dh)
    x = c['k'].double().permute(0, 2, 1, 3)
    v = c['v'].double().permute(0, 2, 1, 3)
    scale = 1.0 / math.sqrt(dh)
    if rounded:
        scale = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
        if lsh:      # rsqrtf(ss / DH + 1e-6f) * scale, float32
            ss = _seqsum32(_f32(x * x)).float()
            f = (torch.rsqrt(ss / np.float32(dh) + np.float32(1e-6)) * np.float32(scale)).double()
        else:
            f = torch.full(x.shape[:-1], scale, dtype=torch.float64)
    else:
        f = torch.rsqrt((x * x).mean(-1) + 1e-6) / math.sqrt(dh) if lsh else torch.full(x.shape[:-1], scale, dtype=torch.float64)
    pos = slot_positions(c)                                              # (B, H, S)
    gi = pos.unsqueeze(-1).expand(-1, -1, -1, dh)
    rnd = (torch.arange(S) // T).view(1, 1, S).expand(B, H, S)
    bi = torch.arange(B).view(B, 1, 1).expand(B, H, S)
    hi = torch.arange(H).view(1, H, 1).expand(B, H, S)
    qs, xs, vs, fs = q.gather(2, gi), x.gather(2, gi), v.gather(2, gi), f.gather(2, pos)
    do_s = c['dout'].double()[bi, rnd, pos, hi]                          # (B, H, S, dh)
    dl_s = c['dlse'].double()[bi, rnd, hi, pos] if c['dlse'] is not None else torch.zeros(B, H, S, dtype=torch.float64)

    def win(t, fill=None):
        tc = t.reshape(B, H, NC, C, *t.shape[3:])
        if single:
            return tc
        prev = torch.roll(tc, 1, 2)
        if fill is not None:
            prev = prev.clone()
            prev[:, :, 0] = fill
        return torch.cat([prev, tc], 3)

    def fold(w):
        if single:
            return w.reshape(B, H, S, -1)
        return (w[:, :, :, C:] + torch.roll(w[:, :, :, :C], -1, 2)).reshape(B, H, S, -1)

    qc, doc = qs.view(B, H, NC, C, dh), do_s.view(B, H, NC, C, dh)
    xw, vw, fw = win(xs), win(vs), win(fs)
    qp = pos.view(B, H, NC, C)
    kp = win(pos, fill=(1 << 40) if 'no_wrap' in edit else None)
    if all32:        # the factor is folded into the key rows first (:1191)
        dots = _seqmm32(qc, _f32(xw * fw[..., None]).transpose(-1, -2))
    else:
        dots = (_seqmm32(qc, xw.transpose(-1, -2)) if rounded else qc @ xw.transpose(-1, -2)) * fw[..., None, :]
    if rounded:
        dots = _f32(dots)
    causal = qp[..., None] >= kp[..., None, :]
    same = qp[..., None] == kp[..., None, :]
    if 'self_first' in edit and lsh:
        dots = torch.where(same, torch.tensor(-1e5, dtype=torch.float64), dots)
        dots = torch.where(causal, dots, torch.tensor(-1e9, dtype=torch.float64))
    else:
        dots = torch.where(causal, dots, torch.tensor(-1e9, dtype=torch.float64))
        if lsh:
            dots = torch.where(same, torch.tensor(-1e5, dtype=torch.float64), dots)
    live = causal & ~same if lsh else causal
    keep = attn_keep(c, swap_parity='parity_swap' in edit)
    if keep is not None and 'mask_shift' in edit:
        keep = torch.roll(keep, 1, -1)
    ds_ = dscale_of(p)
    kf = torch.ones_like(dots) if keep is None else keep.double()
    if rounded:
        mx = dots.max(-1, keepdim=True).values
        e = _expf(dots - mx)
        ssum = _seqsum32(e).unsqueeze(-1)
        lse = _f32(mx + _logf(ssum))
        P = _expf(dots - lse)                                  # what the backward regenerates from the stored lse
        if all32:
            o32 = _seqmm32(_f32(P * kf * ds_), vw)                       # :1220
            delta = None
        else:
            o32 = (_bf(e * kf) @ vw) * _f32(ds_ / ssum)
        out = _bf(o32)
    else:
        lse = torch.logsumexp(dots, -1, keepdim=True)
        P = torch.exp(dots - lse)
        out = (P * kf * ds_) @ vw
    # backward
    dP = mm(doc, vw.transpose(-1, -2))
    g = r32(dP * kf * ds_)
    if all32:
        delta = _seqsum32(_f32(P * g)).unsqueeze(-1)                     # :1235
        dl_c = torch.zeros_like(delta)                                   # (the single-chunk kernels take no dlse)
    else:
        o_for_delta = o32 if (rounded and delta_unrounded) else out
        delta = (doc * o_for_delta).sum(-1, keepdim=True)
        dl_c = dl_s.view(B, H, NC, C, 1)
    dS = torch.where(live, r32(P * (g - delta)) + dl_c * P, torch.zeros((), dtype=torch.float64))
    Pd = P * kf * ds_
    if rounded and not all32:
        dq_s = (_bf(dS * fw[..., None, :]) @ xw)
        dkw = _bf(dS if lsh else dS * fw[..., None, :]).transpose(-1, -2) @ qc
        dvw = _bf(Pd).transpose(-1, -2) @ doc
    elif all32:
        xk = _f32(xw * fw[..., None])
        dq_s = _seqmm32(dS, xk)
        dkw = _seqmm32(dS.transpose(-1, -2), qc)
        if not lsh:
            dkw = _f32(dkw * scale)
        dvw = _seqmm32(_f32(Pd).transpose(-1, -2), doc)
    else:
        dq_s = (dS * fw[..., None, :]) @ xw
        dkw = (dS if lsh else dS * fw[..., None, :]).transpose(-1, -2) @ qc
        dvw = Pd.transpose(-1, -2) @ doc
    dq_s = dq_s.reshape(B, H, S, dh)
    dk_s, dv_s = fold(dkw), fold(dvw)
    if rounded:
        dq_s, dk_s, dv_s = _f32(dq_s), _f32(dk_s), _f32(dv_s)

    def slabs(t):
        o = torch.zeros(B, n_h, T, H, dh, dtype=torch.float64)
        o[bi, rnd, pos, hi] = t.reshape(B, H, S, dh)
        return o

    res = dict(out=slabs(out), dq=slabs(dq_s), dk=slabs(dk_s), dv=slabs(dv_s), P=P, keep=keep, live=live, same=same, causal=causal)
    l_ = torch.zeros(B, n_h, H, T, dtype=torch.float64)
    l_[bi, rnd, hi, pos] = lse.reshape(B, H, S)
    res['lse'] = l_
    if lsh:
        res.update(keynorm_ref64(c['k'], res['dq'], res['dk'], res['dv'], rounded=rounded, edit=edit))
    return res


def keynorm_ref64(qk, dq, dk, dv, rounded=False, edit=()):
    """the key-normalisation chain over per-round slabs.  qk (B, T, H, dh) bf16-exact; dq, dk, dv (B, n_h, T, H, dh) -> dict(dqk, dv_sum) (B, T, H, dh)"""
    x = qk.double()
    dh = x.shape[-1]
    n_h = dq.shape[1]
    rounds = range(n_h - 1) if ('drop_round' in edit and n_h > 1) else range(n_h)
    if rounded:
        q_ = torch.zeros_like(dq[:, 0]); k_ = torch.zeros_like(q_); v_ = torch.zeros_like(q_)
        for r in rounds:
            q_, k_, v_ = _f32(q_ + dq[:, r]), _f32(k_ + dk[:, r]), _f32(v_ + dv[:, r])
        m = _f32(_f32(_seqsum32(_f32(x * x)) / dh) + float(np.float32(1e-6)))
        dot = _seqsum32(_f32(k_ * x))
        rs = _f32(torch.rsqrt(m))
        f = _f32(rs * float(np.float32(1.0) / np.sqrt(np.float32(dh))))
        cc = _f32(dot * rs * rs * rs / float(np.float32(dh) * np.sqrt(np.float32(dh))))
        return dict(dqk=_bf(q_ + f[..., None] * k_ - x * cc[..., None]), dv_sum=_bf(v_))
    q_, k_, v_ = (sum(t[:, r] for r in rounds) for t in (dq, dk, dv))
    m = (x * x).mean(-1, keepdim=True) + 1e-6
    f = m ** -0.5 / math.sqrt(dh)
    if 'no_keyfac_chain' in edit:
        f = torch.ones_like(f)
    dqk = q_ + f * k_ - x * (k_ * x).sum(-1, keepdim=True) * m ** -1.5 / dh ** 1.5
    return dict(dqk=dqk, dv_sum=v_)


def lse_groups(ref_lse):
    """rows whose lse is about -1e5 (only self-masked cells are visible) are judged as their own group: they must not set max|ref| for
    the ordinary rows, and the ordinary rows must not lend them a bound.  -> list of bool masks (empty groups left out)"""
    low = ref_lse < -5e4
    return [m for m in (low, ~low) if m.any()]


def worst_grouped(got, ref, a, b, groups=None):
    """oracle.kernel_cases.worst over each group of elements with that group's own max|ref| -> (largest ratio, largest error / max|ref|)"""
    got, ref = got.double(), ref.double()
    if groups is None:
        groups = [torch.ones_like(ref, dtype=torch.bool)]
    ratio = err_ = 0.0
    for m in groups:
        r, g = ref[m], got[m]
        err = (g - r).abs()
        mxr = r.abs().max().clamp_min(1e-300)
        ratio = max(ratio, (err / (a * r.abs() + b * mxr)).max().item())
        err_ = max(err_, (err.max() / mxr).item())
    return ratio, err_


def gap_grouped(model, ref, groups=None):
    """max over the groups of max|model - ref| / max|ref| within the group"""
    return worst_grouped(model, ref, 0.0, 1.0, groups)[0]


def _poscode(shape, mul, mod, div):
    """values that encode their own (b, t, h, e) [or (b, r, t, h, e)] index: a swapped row, head or sequence changes them"""
    idx = torch.zeros(shape, dtype=torch.long)
    for ax, m in enumerate(mul):
        view = [1] * len(shape)
        view[ax] = shape[ax]
        idx = idx + m * torch.arange(shape[ax]).view(view)
    return bf16_exact(((idx % mod) - mod // 2).float() / div)


def _order(g, kind, B, H, T, n_h):
    """(B, H, S) sorted positions: every round's T slots hold a permutation of 0 .. T-1.
    'random': a stable sort of random bucket ids (8 per round), as the hashing gives.
    'desc': each round's chunks in DESCENDING position order, a random order inside a chunk: the smallest position of chunk c is smaller
            than every position of the chunk before it, so that query sees only later positions and itself (all but the chunk that
            looks back across the wrap-around).
    'dup': round r is the identity rotated by 64 r: the first chunk of round 1 holds the very positions of the chunk it looks back at,
           so every one of its windows holds each position twice, once per round."""
    S = n_h * T
    if kind == 'random':
        bk = torch.randint(0, 8, (B, H, n_h, T), generator=g) + 8 * torch.arange(n_h).view(1, 1, -1, 1)
        return torch.argsort(S * bk.view(B, H, S) + torch.arange(S).view(1, 1, -1), -1) % T
    if kind == 'desc':
        nc = T // 64
        out = torch.empty(B, H, n_h, nc, 64, dtype=torch.long)
        for b in range(B):
            for h in range(H):
                for r in range(n_h):
                    for ch in range(nc):
                        out[b, h, r, ch] = (nc - 1 - ch) * 64 + torch.randperm(64, generator=g)
        return out.view(B, H, S)
    assert kind == 'dup'
    one = torch.stack([(torch.arange(T) + 64 * r) % T for r in range(n_h)]).view(1, 1, S)
    return one.expand(B, H, S).contiguous()


def build_attn_case(name, T, n_h, lsh, dh, B, H, kind='random', order='random', wide=False, p=0.0, seed=0, site=0):
    """-> dict: q, k, v (B, T, H, dh) bf16 (k is q for LSH), spos (B, H, S) int64 or None, dout (B, n_h, T, H, dh) bf16,
    dlse (B, n_h, H, T) float32 (n_h > 1) or None, and the scalars.  kind: 'random', 'poscode' (position-coded q / k / v / dout) or
    'dominant' (query 40 of every head has one key, position 5, that outweighs the rest)."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    if kind == 'poscode':
        q = _poscode((B, T, H, dh), (7, 3, 5, 1), 13, 4.0)
        k = q if lsh else _poscode((B, T, H, dh), (3, 5, 11, 2), 17, 4.0)
        v = _poscode((B, T, H, dh), (17, 1, 11, 2), 31, 8.0)
        dout = _poscode((B, n_h, T, H, dh), (5, 19, 3, 7, 1), 29, 8.0)
    else:
        q = bf16_exact(torch.randn(B, T, H, dh, generator=g))
        k = q if lsh else bf16_exact(torch.randn(B, T, H, dh, generator=g))
        v = bf16_exact(torch.randn(B, T, H, dh, generator=g))
        dout = bf16_exact(torch.randn(B, n_h, T, H, dh, generator=g))
        if kind == 'dominant' and T > 40:
            if lsh:
                q[:, 40] = bf16_exact(3.0 * q[:, 5].float())
            else:
                k[:, 5] = bf16_exact(4.0 * q[:, 40].float())
    spos = None
    if lsh and T > SC_MAXT:
        spos = _order(g, order, B, H, T, n_h)
    dlse = torch.randn(B, n_h, H, T, generator=g) if n_h > 1 else None
    return dict(name=name, T=T, n_h=n_h, lsh=int(lsh), dh=dh, B=B, H=H, kind=kind, order=order, wide=wide, p=p, seed=seed, site=site,
                q=q, k=k, v=v, spos=spos, dout=dout, dlse=dlse)


HI_SEED = (0x1234ABCD << 32) | 0x9E3779B9           # a seed with a non-zero high word


def _chunk_rows():
    R = []

    def add(name, T, n_h, lsh, dh, B, H, **kw):
        R.append(dict(name=name, T=T, n_h=n_h, lsh=lsh, dh=dh, B=B, H=H, **kw))
    add('c_loc_t128_dh64', 128, 1, 0, 64, 1, 1)
    add('c_loc_t192_dh32', 192, 1, 0, 32, 3, 3, kind='poscode', wide=True)
    add('c_loc_t256_dh16', 256, 1, 0, 16, 2, 4, wide=True, p=0.1, seed=77, site=3)
    add('c_loc_t128_dh64_dom_p50', 128, 1, 0, 64, 2, 4, kind='dominant', p=0.5, seed=HI_SEED, site=5)
    add('c_loc_t192_dh16_p50', 192, 1, 0, 16, 3, 3, p=0.5, seed=HI_SEED + 1, site=2, wide=True)
    add('c_lsh_t128_n1_dh64', 128, 1, 1, 64, 3, 3, wide=True)
    add('c_lsh_t128_n2_dh32_dup', 128, 2, 1, 32, 2, 4, order='dup')
    add('c_lsh_t128_n3_dh16', 128, 3, 1, 16, 1, 1, wide=True)
    add('c_lsh_t192_n1_dh16', 192, 1, 1, 16, 2, 4, kind='poscode')
    add('c_lsh_t192_n2_dh64_p10', 192, 2, 1, 64, 1, 1, wide=True, p=0.1, seed=HI_SEED + 2, site=7)
    add('c_lsh_t256_n1_dh32_desc', 256, 1, 1, 32, 1, 1, order='desc')
    add('c_lsh_t256_n3_dh64', 256, 3, 1, 64, 3, 3, wide=True)
    add('c_lsh_t256_n2_dh16_desc_p50', 256, 2, 1, 16, 3, 3, order='desc', p=0.5, seed=HI_SEED + 3, site=1)
    add('c_lsh_t128_n1_dh32_dom_p10', 128, 1, 1, 32, 2, 4, kind='dominant', order='dup', p=0.1, seed=12345, site=4, wide=True)
    return R


def _single_rows():
    R, i = [], 0
    for T in (1, 7, 33, 64):
        for dh in (16, 32, 64):
            for lsh in (0, 1):
                B, H = ((1, 1), (3, 3), (2, 4))[i % 3]
                p = (0.0, 0.1, 0.5)[(i // 2) % 3]
                R.append(dict(name=f's_t{T}_dh{dh}_{"lsh" if lsh else "loc"}', T=T, n_h=1, lsh=lsh, dh=dh, B=B, H=H,
                              kind=('random', 'poscode')[(i // 3) % 2], wide=bool(i % 2), p=p, seed=HI_SEED + i if i % 4 < 2 else 100 + i,
                              site=i % 5))
                i += 1
    return R


CHUNK_CASES = _chunk_rows()
SINGLE_CASES = _single_rows()
ATTN_CASES = {r['name']: r for r in CHUNK_CASES + SINGLE_CASES}


@functools.lru_cache(maxsize=None)
def attn_case(name):
    """-> (case, float64 reference, rounded model), computed once and shared (treat as read-only)"""
    c = build_attn_case(**ATTN_CASES[name])
    return c, attn_ref64(c), attn_ref64(c, rounded=True)


# dropout probes: one-hot V and dout.  A probe launch `k` of a case gives every key slot one value column and lets only the keys of
# one column group carry a one (V) and every query one gradient column (dout): `out` is then, per column, exactly the sum of the kept
# probabilities of at most a few cells, a row of dq is exactly zero iff its probed cell is dropped (g = 0 and delta = 0), and dv
# is, per column, the kept probability of single cells.  PROBE_CASES: (name, build arguments)
PROBE_CASES = {
    'p_loc_t256_dh16': dict(T=256, n_h=1, lsh=0, dh=16, B=1, H=2, p=0.5, seed=HI_SEED + 9, site=6),
    'p_lsh_t128_n2_dh64': dict(T=128, n_h=2, lsh=1, dh=64, B=1, H=1, order='random', p=0.1, seed=4242, site=2),
}


def probe_case(name, k):
    """probe launch k (0 .. 127) of PROBE_CASES[name]: V[pos] is one-hot at column pos % dh for the positions of column group
    (pos % 128) // dh == k % (128 // dh), zero elsewhere; dout[.., pos, ..] is one-hot at column (pos + k // (128 // dh)) % dh."""
    a = PROBE_CASES[name]
    c = build_attn_case(name, **a)
    B, T, H, dh, n_h = c['B'], c['T'], c['H'], c['dh'], c['n_h']
    ng = 128 // dh
    grp, shift = k % ng, k // ng
    t = torch.arange(T)
    e = torch.arange(dh)
    v = ((t[:, None] % dh == e[None, :]) & ((t[:, None] % 128) // dh == grp)).float()
    c['v'] = bf16_exact(v.view(1, T, 1, dh).expand(B, T, H, dh).contiguous())
    do = ((t[:, None] + shift) % dh == e[None, :]).float()
    c['dout'] = bf16_exact(do.view(1, 1, T, 1, dh).expand(B, n_h, T, H, dh).contiguous())
    c['dlse'] = None
    return c


def probe_zero_sets(c, ref):
    """-> {name: (must_be_zero, must_be_nonzero)} bool masks over out, dq, dv of a probe launch.  out and dv are exactly zero where no
    kept visible cell feeds them, and non-zero elsewhere.  A row of dq is exactly zero where its probed cells are all dropped or
    invisible -- then g = 0 and delta = dO . out = 0 -- and non-zero where the float64 row is non-zero; a row whose ONLY visible cell is
    the probed one has P = 1 and dS = P (g - delta) = 0 in exact arithmetic but not after out was rounded to bf16: nothing is asked of
    its zeros."""
    delta = (c['dout'].double() * ref['out']).sum(-1, keepdim=True)                 # (B, n_h, T, H, 1)
    sets = {n: (ref[n] == 0, ref[n] != 0) for n in ('out', 'dv')}
    sets['dq'] = ((delta == 0).expand_as(ref['dq']), ref['dq'] != 0)
    return sets


# ----------------------------------------------------------------------------------------------------------------------------
# hash-round combine
# ----------------------------------------------------------------------------------------------------------------------------
COMBINE_CASES = {
    'cb_n1_dh64': dict(B=2, T=70, H=3, dh=64, n_h=1, low=False),
    'cb_n2_dh16': dict(B=2, T=70, H=3, dh=16, n_h=2, low=False),
    'cb_n3_dh32': dict(B=3, T=65, H=2, dh=32, n_h=3, low=False),
    'cb_n3_dh64_low': dict(B=1, T=130, H=4, dh=64, n_h=3, low=True),
}


@functools.lru_cache(maxsize=None)
def combine_case(name):
    """-> dict: out_r (B, n_h, T, H, dh) bf16, lse (B, n_h, H, T) float32, dout (B, T, H, dh) bf16.  `low`: round 1 of three has its
    lse lower by 100, so its weight underflows in float32 (with two rounds every gradient would be of the size of that weight)"""
    a = COMBINE_CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    B, T, H, dh, n_h = a['B'], a['T'], a['H'], a['dh'], a['n_h']
    out_r = bf16_exact(torch.randn(B, n_h, T, H, dh, generator=g))
    lse = torch.randn(B, n_h, H, T, generator=g) * 2.0
    if a['low']:
        lse[:, 1] -= 100.0
    dout = bf16_exact(torch.randn(B, T, H, dh, generator=g))
    return dict(a, name=name, out_r=out_r, lse=lse, dout=dout)


def combine_ref64(c, rounded=False):
    """out = sum_r w_r out_r, w = softmax_r(lse);  dout_r = w_r dout;  dlse_r = w_r dout . (out_r - out)
    -> dict(out (B, T, H, dh), dout_r (B, n_h, T, H, dh), dlse (B, n_h, H, T))"""
    o_r, lse, dout = c['out_r'].double(), c['lse'].double(), c['dout'].double()
    if not rounded:
        w = torch.softmax(lse, 1)
        wv = w.permute(0, 1, 3, 2).unsqueeze(-1)                        # (B, n_h, T, H, 1)
        out = (wv * o_r).sum(1)
        dlse = (w * (dout.unsqueeze(1) * (o_r - out.unsqueeze(1))).sum(-1).permute(0, 1, 3, 2))
        return dict(out=out, dout_r=wv * dout.unsqueeze(1), dlse=dlse)
    mx = lse.max(1, keepdim=True).values
    e = _expf(lse - mx)
    e = torch.where(e < 2.0 ** -126, torch.zeros((), dtype=torch.float64), e)         # the fast exp flushes denormals
    den = _seqsum32(e.permute(0, 2, 3, 1)).unsqueeze(1)
    ev = e.permute(0, 1, 3, 2).unsqueeze(-1)
    acc = torch.zeros_like(o_r[:, 0])
    for r in range(o_r.shape[1]):
        acc = _f32(acc + _f32(ev[:, r] * o_r[:, r]))
    out = _bf(acc / den[:, 0].permute(0, 2, 1).unsqueeze(-1))
    w = _f32(e / den)
    wv = w.permute(0, 1, 3, 2).unsqueeze(-1)
    dot = _seqsum32(_f32(dout.unsqueeze(1) * _f32(o_r - out.unsqueeze(1)))).permute(0, 1, 3, 2)
    return dict(out=out, dout_r=_bf(wv * dout.unsqueeze(1)), dlse=_f32(w * dot))


# ----------------------------------------------------------------------------------------------------------------------------
# axial position embeddings
# ----------------------------------------------------------------------------------------------------------------------------
# name -> (B, T, V, d, d0, A0, A1, form): 'rows' = the row-owner form of the position tables (B T >= 4096, d % 32 == 0, d0 % 32 == 0),
# 'elem' = the element-wise form
AXIAL_CASES = {
    'ax_small_d0_16': (3, 100, 50, 64, 16, 8, 16, 'elem'),              # T < A0 A1, T % A1 != 0, d0 % 32 != 0
    'ax_tiny_t_below_a1': (2, 10, 40, 64, 32, 4, 16, 'elem'),           # W1 rows 10 .. 15 and W0 rows 1 .. 3 untouched
    'ax_below_switch': (2, 2047, 300, 64, 32, 33, 64, 'elem'),          # B T = 4094
    'ax_above_switch': (2, 2050, 300, 64, 32, 33, 64, 'rows'),          # B T = 4100, T % A1 = 2, W0 row 32 holds two positions
    'ax_above_switch_d0_16': (2, 2050, 300, 96, 16, 33, 64, 'elem'),    # d0 % 32 != 0 keeps the element-wise form
}


@functools.lru_cache(maxsize=None)
def axial_case(name):
    """-> dict: ids (B, T) int64 -- multiples of 3 only, so two thirds of the word table stay untouched, with 0, V-1 and a run of one
    repeated id at the head of the first row --, E (V, d) bf16, W0 (A0, d0), W1 (A1, d - d0) float32, dout, dout2 (B, T, d) bf16, and the
    non-zero patterns the three gradient tables start from"""
    B, T, V, d, d0, A0, A1, form = AXIAL_CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    ids = torch.randint(0, V // 3, (B, T), generator=g) * 3
    head = torch.tensor([0, V - 1, 6, 6, 6, 6, 6])[:T]
    ids[0, :head.numel()] = head
    pat = lambda shape: (torch.randint(32, 160, shape, generator=g).float() / 256.0) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    return dict(name=name, B=B, T=T, V=V, d=d, d0=d0, A0=A0, A1=A1, form=form, ids=ids, E=bf16_exact(torch.randn(V, d, generator=g)),
                W0=torch.randn(A0, d0, generator=g), W1=torch.randn(A1, d - d0, generator=g),
                dout=bf16_exact(torch.randn(B, T, d, generator=g)), dout2=bf16_exact(torch.randn(B, T, d, generator=g)),
                pat=dict(dE=pat((V, d)), dW0=pat((A0, d0)), dW1=pat((A1, d - d0))))


def axial_masks(c, p, seed, site_emb, site_pos):
    """-> (keep_e (B, T, d), keep_p (B, T, 1)) float64 0 / 1 (all ones without dropout)"""
    B, T, d = c['B'], c['T'], c['d']
    if p <= 0:
        return torch.ones(B, T, d, dtype=torch.float64), torch.ones(B, T, 1, dtype=torch.float64)
    return (torch.from_numpy(axial_emb_mask(seed, site_emb, B, T, d, p)).double(),
            torch.from_numpy(axial_pos_mask(seed, site_pos, B, T, c['A1'], p)).double().unsqueeze(-1))


def axial_ref64(c, p=0.0, seed=0, site_emb=0, site_pos=1, two=False, rounded=False):
    """out[b,t] = keep_e E[ids] / (1-p) + keep_p cat(W0[t // A1], W1[t % A1]) / (1-p); the three table gradients of
    g = dout (+ dout2) under the SAME masks -> dict(out (B, T, d), dE (V, d), dW0 (A0, d0), dW1 (A1, d - d0)); the gradients are the
    ADDED amounts (the tables' starting patterns are subtracted by the caller; the rounded model adds to them in float32 first)"""
    B, T, V, d, d0, A0, A1 = (c[n] for n in ('B', 'T', 'V', 'd', 'd0', 'A0', 'A1'))
    ke, kp = axial_masks(c, p, seed, site_emb, site_pos)
    ds_ = dscale_of(p)
    t = torch.arange(T)
    pos = torch.cat([c['W0'].double()[t // A1], c['W1'].double()[t % A1]], -1).unsqueeze(0)
    e = c['E'].double()[c['ids']]
    g = c['dout'].double() + (c['dout2'].double() if two else 0.0)
    if rounded:
        g = _f32(g)
        out = _bf(_f32(ke * _f32(e * ds_)) + _f32(kp * _f32(pos * ds_)))
    else:
        out = ke * e * ds_ + kp * pos * ds_
    ge, gp = ke * g * ds_, (kp * g * ds_)
    if rounded:
        ge, gp = _f32(ge), _f32(gp)
    flat = lambda x, n: x.reshape(B * T, n)
    idx = dict(dE=c['ids'].reshape(-1), dW0=(t // A1).repeat(B), dW1=(t % A1).repeat(B))
    src = dict(dE=flat(ge, d), dW0=flat(gp[..., :d0], d0), dW1=flat(gp[..., d0:], d - d0))
    res = dict(out=out)
    for n, rows in (('dE', V), ('dW0', A0), ('dW1', A1)):
        if rounded:      # one float32 accumulator per element, token by token, on top of the starting pattern
            acc = c['pat'][n].clone().float()
            acc.index_add_(0, idx[n], src[n].float())
            res[n] = acc.double() - c['pat'][n].double()
        else:
            res[n] = torch.zeros(rows, src[n].shape[1], dtype=torch.float64).index_add_(0, idx[n], src[n])
    return res


def axial_untouched(c):
    """bool row masks of the three tables: rows no id / position of the case touches"""
    t = torch.arange(c['T'])
    def un(n, idx):
        m = torch.ones(n, dtype=torch.bool)
        m[idx] = False
        return m
    return dict(dE=un(c['V'], c['ids'].reshape(-1)), dW0=un(c['A0'], t // c['A1']), dW1=un(c['A1'], t % c['A1']))


# ----------------------------------------------------------------------------------------------------------------------------
# LSH hashing
# ----------------------------------------------------------------------------------------------------------------------------
# kernel arms of mxl_lsh_hash (reformer.hip:1329-1338): dh = 32 / 64 and 16-byte aligned, 8-element strides -> lsh_hash_mfma_kernel<1 | 2 | 4>
# for R2 <= 16 | <= 32 | <= 64; otherwise (dh = 16, or a qk pointer off 16 bytes) lsh_hash_kernel<16 | 32 | 64>.  R2 = sum(factors) / 2.
HASH_FACTORS = ([16], [32], [4, 8, 32], [16, 32], [64], [32, 64], [128])           # R2 = 8, 16, 22, 24, 32, 48, 64
HASH_SHAPES = {1: (128, 4, 2), 17: (8, 4, 2), 513: (1, 2, 2)}                       # T -> (B, H, n_h): 1024 / 1088 / 2052 tokens


def _hash_rows():
    R = []
    for i, dh in enumerate((16, 32, 64)):
        for j, fac in enumerate(HASH_FACTORS):
            T = (1, 17, 513)[(i + j) % 3]
            R.append(dict(name=f'h_dh{dh}_r{sum(fac) // 2}_t{T}', dh=dh, factors=fac, T=T, strided=bool((i + j) % 2), mixed=j % 3 == 1, off8=False))
    for fac in ([16], [64], [128]):      # a qk pointer 8 bytes off 16-byte alignment: the scalar kernel at dh = 64
        R.append(dict(name=f'h_dh64_r{sum(fac) // 2}_t17_off8', dh=64, factors=fac, T=17, strided=True, mixed=False, off8=True))
    return R


HASH_CASES = {r['name']: r for r in _hash_rows()}


@functools.lru_cache(maxsize=None)
def hash_case(name):
    """-> dict: qk (B, T, H, dh) bf16, rot (H, dh, n_h, R2) float32 (`mixed`: columns scaled by 1e-3, 1, 1e3 in turn, so the low terms
    of the three-term bf16 split of a rotation carry weight), and the float64 projections proj (B, H, n_h, T, R2)"""
    a = HASH_CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    B, H, n_h = HASH_SHAPES[a['T']]
    R2 = sum(a['factors']) // 2
    qk = bf16_exact(torch.randn(B, a['T'], H, a['dh'], generator=g))
    rot = torch.randn(H, a['dh'], n_h, R2, generator=g)
    if a['mixed']:
        rot = rot * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(R2) % 3]
    proj = torch.einsum('bthe,herc->bhrtc', qk.double(), rot.double())
    absp = torch.einsum('bthe,herc->bhrtc', qk.double().abs(), rot.double().abs())
    return dict(a, B=B, H=H, n_h=n_h, R2=R2, qk=qk, rot=rot, proj=proj, absp=absp)


def hash_buckets(proj, factors):
    """bucket ids WITHOUT the round offset from projections (..., R2): per factor the first maximum of [v, -v] (torch.argmax), combined
    in mixed radix -> int64 (...)"""
    bucket, cur, prod = 0, 0, 1
    for f in factors:
        v = proj[..., cur:cur + f // 2]
        bucket = bucket + prod * torch.argmax(torch.cat([v, -v], -1), -1)
        prod *= f
        cur += f // 2
    return bucket


def hash_near_ties(c, got):
    """got (B, H, n_h, T) bucket ids without the round offset.  -> (number of tokens that differ from the float64 ids, number of those
    that are NOT near-ties): in every factor where the digits differ the device's choice must lie within 2^-20 sum_e |x_e| |R_ec|
    (c = the column it chose) of the float64 maximum of that factor"""
    ref = hash_buckets(c['proj'], c['factors'])
    diff = got.long() != ref
    bad = torch.zeros_like(diff)
    cur, prod = 0, 1
    for f in c['factors']:
        half = f // 2
        dg, dr = (got.long() // prod) % f, (ref // prod) % f
        v = c['proj'][..., cur:cur + half]
        both = torch.cat([v, -v], -1)
        ab = torch.cat([c['absp'][..., cur:cur + half]] * 2, -1)
        chosen = both.gather(-1, dg.unsqueeze(-1)).squeeze(-1)
        tol = 2.0 ** -20 * ab.gather(-1, dg.unsqueeze(-1)).squeeze(-1)
        bad |= (dg != dr) & ~(both.max(-1).values - chosen <= tol)
        prod *= f
        cur += half
    return int(diff.sum()), int(bad.sum())
