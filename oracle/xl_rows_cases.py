"""ORACLE-side statement of the HBM-bound row kernels of csrc/elementwise.hip, the adaptive-softmax head of csrc/head.hip and the
optimiser of csrc/optim.hip (test infrastructure, NOT product code): case tables, bf16-exact inputs generated on the CPU from a seed
derived from the case name, and for every op a reference in two forms (csrc/ = symbolic_music_generation_amd/csrc/):

  float64 closed form  (`dt=torch.float64`): the formulas of include/musicxl.h, dropout masks from keep_mask / keep_mask32 of
                       oracle/kernel_cases.py, dscale = 1 / (1 - float32(p)).
  rounded model        (`dt=torch.float32`): the same evaluation with the roundings the kernel sources make and sums through ONE
                       sequential float32 accumulator (numpy cumsum).  It is NOT the expected value: gap(model, float64) is what
                       float32 costs on a case, and 4 x the largest gap is the absolute term `b` of the rule of oracle/kernel_cases.py.

Roundings modelled, with their sources:
  elementwise.hip
    z = bf16(res + drop(x) dscale): one float32 product, one float32 sum, one bf16 rounding -- no reduction, IEEE-exact ...... :106-111
    row sum / d -> mean; sum (z - mean)^2 / d + eps -> rsqrtf; (z - mean) rstd gamma + beta in float32, y bf16 ............... :116-138
    partial form: slabs summed in slab order, + bias, bf16, + res, bf16 (exact as well), then the same statistics ........... :176-188
    backward: dy + dy2, xhat = (z - mean) rstd, g = dy gamma, the two row means, dz = rstd (g - s1 - xhat s2) in float32 ... :269-288
    dres = bf16(dz + dadd); dx = bf16(keep dz dscale), or (add_drop) bf16(keep dscale * the STORED dres) ..................... :290-311
    dgamma / dbeta: float32 row sums per column (modelled: sequential over rows, onto the prior contents) .................... :274, :336-373
    dxsum: float32 column sums of the STORED bf16 dx ....................................................................... :312-318
    embedding: E scale (exact: 16 significant bits), times dscale (one rounding), bf16; backward (dout + dout2) scale dscale
      added to dE by float32 atomics (modelled: sequential over token rows, onto the prior contents) ........................ :47-51, :62-66
    sinusoid: 2k / d, powf, 1 / ., p inv_freq, sinf / cosf all float32, times dscale, bf16 ................................... :18-29
    dropout: bf16(x dscale) where kept (exact); transpose: a copy ............................................................ :476, :492-495
  head.hip
    lse = max + __logf(sum __expf(l - max)) in float32, the sum sequential in the model; one- and two-pass forms alike ...... :24-50
    nll = (head_lse - l[label]) or (head_lse - l[V + ci - 1]) + (tail_lse - l[label]), float32 ............................. :89-92
    acc2[0]: float32 sum of the nll (modelled sequential); acc2[1] a count ................................................... :99-106
    d = __expf(l - stored float32 lse) - onehot, times grad_scale / count, hi = bf16(d), lo = bf16(d - hi) .................. :135-153
    log-probabilities l - head_lse, or (l[V + ci - 1] - head_lse) + (l - tail_lse) ........................................... :164-169
  optim.hip
    sum of squares in float32 (modelled sequential over the elements, onto the prior value) .................................. :15-23
    coef = gscale min(1, max_norm / (sqrtf(sumsq) gscale + 1e-6)); p (1 - lr wd); m, v, sqrtf(v) / bc2_sqrt + eps; p -= (lr / bc1)
      (m / denom), every step a float32 statement; w16 = bf16(p) ............................................................ :32-48

Branches of the launch functions -> cases that take them:
  ln_res_fwd_kernel<1> / ln_res_bwd_kernel<1[, CS]>  (d <= 512) ............ ln_d8_*, ln_d504_*, ln_d512_*  (d = 8: lane 0 alone)
  <2>  (d <= 1024; d = 520: the second chunk has one owner, lane 0) ........ ln_d520_*, ln_d1024_*
  <LN_MAXCH>  (d > 1024; backward: LDS-atomic dgamma / dbeta) .............. ln_d1032_*, ln_d2048_*
  forward 4 rows per block ragged, backward LNB_ROWS = 64 boundary ......... N = 1, 3, 63, 65, 130 / N = 63, 64, 65; three blocks: N = 130
  mxl_ln_residual_bwd_colsum, mxl_ln_residual_bwd_add_drop[ + dxsum] ....... every ln_* case with d <= 1024
  wave_lse_range one pass (range <= 2048) / two passes ..................... h_v300, h_v1190, h_v500_c3, h_v2048, head of h_v5000_c1000
                                                                             / h_v2049, tail of h_v5000_c1000, head of h_v5000_c3000
  n_extra = 0 / 1 / 3 (cluster columns as `extra`) ......................... no cutoffs / one cutoff / h_v500_c3
  mxl_adaptive_nll_bwd_split, grad_scale = 0.5, ncl = 3 .................... every head case (split), h_*_gs / h_v500_c3
  sumsq_kernel grid stride, n & 3 tail ..................................... sq_n2097159 / n = 1, 2, 3, 5, 1023, 2097159
  adamw_kernel grid stride / dropout_kernel grid stride .................... aw_big_* (n = 524545) / n = 8 (2048 * 256 + 3)
"""
import functools
import zlib

import numpy as np
import torch

from oracle.kernel_cases import bf16_exact, keep_mask, keep_mask32, worst

F64, F32 = torch.float64, torch.float32
LN_EPS = float(np.float32(1e-5))
LOG2E_F32 = float(np.float32(1.4426950408889634))
LN2_F32 = float(np.float32(0.6931471805599453))


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _seed_site(name):
    h = zlib.crc32(name.encode())
    return ((h << 21) ^ 0x1234ABCD9E3779B9) & 0x7FFFFFFFFFFFFFFF, 3 + h % 11


def dscale32(p):
    """1.f / (1.f - p) as the launch functions compute it"""
    return float(np.float32(1) / (np.float32(1) - np.float32(p))) if p > 0 else 1.0


def dscale64(p):
    return 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0


def _dscale(p, dt):
    return dscale32(p) if dt == F32 else dscale64(p)


def ssum(x, dim):
    """float64: the sum; float32: ONE sequential float32 accumulator along `dim` (numpy's cumsum adds in order)"""
    if x.dtype == F64:
        return x.sum(dim)
    a = np.cumsum(x.contiguous().numpy(), axis=dim, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.take(a, -1, axis=dim)))


def sum_onto(pat, terms, dt):
    """what accumulating `terms` (R, ...) row by row onto the prior contents `pat` ADDS to them -> float64"""
    if dt == F64:
        return terms.sum(0)
    return ssum(torch.cat([pat.float().unsqueeze(0), terms], 0), 0).double() - pat.double()


def bf(x):
    """one rounding to bf16, returned as float64 for comparing"""
    return x.float().to(torch.bfloat16).double()


def pattern(shape, mul=0.37, mod=17):
    """a non-zero float32 starting pattern for accumulated outputs"""
    n = int(np.prod(shape))
    return (((torch.arange(n) * 7) % mod).float() * mul - 2.5).view(shape)


def flat_keep(seed, site, shape, p, form32=True, site_fault=False):
    """the keep mask of a compact array whose flat element index is the dropout index"""
    n = int(np.prod(shape))
    f = keep_mask32 if form32 else keep_mask
    return torch.from_numpy(f(seed, site + (1 if site_fault else 0), np.arange(n, dtype=np.uint64), p).reshape(shape))


def groups_worst(got, ref, a, b, groups=None):
    """`worst` per group of rows (boolean masks over dim 0), the largest of them: rows of another magnitude class (a constant row's
    rstd of eps^-1/2, an lse of 3e4) are not judged with the others' max|ref|"""
    out = (0.0, 0.0)
    for g in (groups or [torch.ones(ref.shape[0], dtype=torch.bool)]):
        if g.any():
            out = max(out, worst(got[g], ref[g], a, b))
    return out


def groups_gap(model, ref, groups=None):
    return groups_worst(model, ref, 0.0, 1.0, groups)[0]


# ======================================================================================================================== LayerNorm
LN_STRESS = ('offset', 'const', 'zero')
_LN_PLAN = {8: (3, 63, 65), 504: (1, 64, 65), 512: (3, 63, 130), 520: (3, 64, 65), 1024: (63, 65, 130), 1032: (3, 63, 130),
            2048: (1, 64, 130)}


def _ln_rows():
    rows = {}
    for di, (d, Ns) in enumerate(_LN_PLAN.items()):
        for i, N in enumerate(Ns):
            p = (0.0, 0.1, 0.5)[(i + di) % 3]
            rows[f'ln_d{d}_n{N}'] = dict(name=f'ln_d{d}_n{N}', d=d, N=N, p=p, res=not (p == 0.0 and di % 2 == 0), dy2=(i + di) % 2 == 0)
    return rows


LN_CASES = _ln_rows()
LN_KS = 3


@functools.lru_cache(maxsize=4)
def ln_case(name, stress):
    """inputs of one LayerNorm case.  The rows `special` (0, N - 1 and 63 / 64 / 65 where present) carry the stress pattern:
    'offset' mean about 30 standard deviations from zero, 'const' constant after the bf16 rounding of z (res = 256 swallows a small
    positive x; without res: x = 1.5), 'zero' all zeros"""
    c = dict(LN_CASES[name])
    g = _gen(name + stress)
    N, d = c['N'], c['d']
    r = lambda *s: bf16_exact(torch.randn(*s, generator=g))
    x, res, resp = r(N, d), r(N, d), r(N, d)
    slabs = torch.randn(LN_KS, N, d, generator=g) * 0.5
    bias = (torch.randn(d, generator=g).abs() * 0.1).clamp_max(0.3)
    sp = sorted({0, N - 1} | {k for k in (63, 64, 65) if k < N})
    small = bf16_exact((torch.randn(len(sp), d, generator=g).abs() * 0.2).clamp_max(0.4))
    if stress == 'offset':
        res[sp] = 30.0
        resp[sp] = 30.0
        if not c['res']:
            x[sp] = bf16_exact(x[sp].float() + 30.0)
    elif stress == 'const':
        res[sp] = 256.0
        resp[sp] = 256.0
        slabs[:, sp] = slabs[:, sp].abs().clamp_max(0.1)
        x[sp] = small if c['res'] else torch.full_like(small, 1.5)
    else:
        x[sp] = 0
        res[sp] = 0
        resp[sp] = 0
        slabs[:, sp] = 0
    special = torch.zeros(N, dtype=torch.bool)
    special[sp] = True
    seed, site = _seed_site(name)
    c.update(x=x, res=res if c['res'] else None, resp=resp, slabs=slabs, bias=bias, gamma=torch.randn(d, generator=g) * 0.5 + 1.0,
             beta=torch.randn(d, generator=g) * 0.5, dy=r(N, d), dy2=r(N, d) if c['dy2'] else None, dadd=r(N, d), special=special,
             groups=[special, ~special], seed=seed, site=site, stress=stress,
             pat=dict(dgamma=pattern((d,)), dbeta=pattern((d,), 0.21, 13), dxsum=pattern((d,), 0.45, 11)))
    return c


def ln_keep(c, p=None, site_fault=False):
    p = c['p'] if p is None else p
    return None if p <= 0 else flat_keep(c['seed'], c['site'], (c['N'], c['d']), p, site_fault=site_fault)


def ln_z_exact(c, p=None, site_fault=False):
    """the stored z = bf16(res + drop(x) dscale) as the IEEE-exact float32 statement -> float32 tensor of bf16 values"""
    p = c['p'] if p is None else p
    a = c['x'].float()
    if p > 0:
        a = torch.where(ln_keep(c, p, site_fault), a * dscale32(p), torch.zeros(()))
    if c['res'] is not None:
        a = a + c['res'].float()
    return a.to(torch.bfloat16).float()


def ln_partial_z_exact(c):
    """bf16(bf16(sum of slabs + bias) + res): slabs added in order from zero, float32"""
    a = torch.zeros_like(c['slabs'][0])
    for s in c['slabs']:
        a = a + s
    t = (a + c['bias']).to(torch.bfloat16).float() + c['resp'].float()
    return t.to(torch.bfloat16).float()


def ln_stats(z, gamma, beta, dt, fault=None):
    """LayerNorm of the stored z -> dict(mean, rstd, y (before the bf16 rounding)).  Faults (CPU test): 'var_e2' variance as
    E[x^2] - mu^2, 'gamma_shift' gamma one column off, 'drop_last_chunk' the last 8 columns left out of the statistics"""
    z = z.to(dt)
    d = z.shape[1]
    zs = z[:, :d - 8] if fault == 'drop_last_chunk' else z
    mu = ssum(zs, 1) / d
    t = z - mu[:, None]
    ts = t[:, :d - 8] if fault == 'drop_last_chunk' else t
    var = ssum(ts * ts, 1) / d
    if fault == 'var_e2':
        var = ssum(z * z, 1) / d - mu * mu
    rs = 1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=dt))
    gm = gamma.to(dt).roll(1) if fault == 'gamma_shift' else gamma.to(dt)
    return dict(mean=mu, rstd=rs, y=t * rs[:, None] * gm + beta.to(dt))


def ln_bwd(c, z, st, dt, p=0.0, dadd=False, site_fault=False):
    """backward from the stored z and the statistics `st` of the same precision -> dict(dres, dx (both before the bf16 rounding), dgamma,
    dbeta (the amounts added to c['pat'])).  With `dadd` the add form: dres = dz + dadd, and dx is NOT stated here (the add_drop call
    derives it from the stored dres: `drop_stored`)"""
    z = z.to(dt)
    d = z.shape[1]
    dyv = c['dy'].to(dt) + (c['dy2'].to(dt) if c['dy2'] is not None else 0)
    xhat = (z - st['mean'][:, None]) * st['rstd'][:, None]
    gg = dyv * c['gamma'].to(dt)
    s1 = ssum(gg, 1) / d
    s2 = ssum(gg * xhat, 1) / d
    dz = st['rstd'][:, None] * (gg - s1[:, None] - xhat * s2[:, None])
    out = dict(dgamma=sum_onto(c['pat']['dgamma'], dyv * xhat, dt), dbeta=sum_onto(c['pat']['dbeta'], dyv, dt))
    if dadd:
        out['dres'] = dz + c['dadd'].to(dt)
        return out
    out['dres'] = dz
    out['dx'] = dz if p <= 0 else torch.where(ln_keep(c, p, site_fault), dz * _dscale(p, dt), torch.zeros((), dtype=dt))
    return out


def drop_stored(c, stored, p):
    """dropout of STORED bf16 values under the case's mask: bf16(v dscale) where kept, 0 elsewhere -- exact (one float32 product)"""
    v = stored.float()
    return torch.where(ln_keep(c, p), v * dscale32(p), torch.zeros(())).to(torch.bfloat16)


def colsum_stored(pat, stored, dt):
    """what the column sums of STORED bf16 values add to the prior contents"""
    return sum_onto(pat, stored.to(dt), dt)


LN_FORMS = dict(plain=dict(dadd=False), add=dict(dadd=True))


@functools.lru_cache(maxsize=4)
def ln_expect(name, stress):
    """-> (case, float64 references, float32 models) of the forward (from the exact z), the partial forward and the backward forms"""
    c = ln_case(name, stress)
    z, zp = ln_z_exact(c), ln_partial_z_exact(c)
    out = {}
    for dt in (F32, F64):
        st, stp = ln_stats(z, c['gamma'], c['beta'], dt), ln_stats(zp, c['gamma'], c['beta'], dt)
        b0, b1 = ln_bwd(c, z, st, dt, p=c['p']), ln_bwd(c, z, st, dt, dadd=True)
        r = dict(y=st['y'], mean=st['mean'], rstd=st['rstd'], y_partial=stp['y'], dres=b0['dres'], dx=b0['dx'], dgamma=b0['dgamma'],
                 dbeta=b0['dbeta'], dres_add=b1['dres'])
        if dt == F32:
            stored = b0['dx'].to(torch.bfloat16)
        # dxsum: column sums of ONE set of stored bf16 values (the model's), in each precision; on the device: of the device's own
        r['dxsum'] = colsum_stored(c['pat']['dxsum'], stored, dt)
        out[dt] = {k: v.double() for k, v in r.items()}
    return c, z, out[F64], out[F32]


LN_OUT = dict(y='y', mean='mean', rstd='rstd', y_partial='y', dres='dres', dx='dx', dgamma='dgamma', dbeta='dbeta', dres_add='dres',
              dxsum='dxsum')                     # reference entry -> the bound it is judged under
LN_ROWWISE = ('y', 'mean', 'rstd', 'y_partial', 'dres', 'dx', 'dres_add')


def ln_gaps(name, stress):
    c, _, ref, model = ln_expect(name, stress)
    return {k: groups_gap(model[k], ref[k], c['groups'] if k in LN_ROWWISE else None) for k in ref}


# ======================================================================================================================== embedding
EMB_V = 97
EMB_SCALE = 27.75          # bf16-exact
EMB_CASES = {r['name']: r for r in [
    dict(name='emb_d8_n1_rand', d=8, N=1, ids='rand', p=0.0, two=False),
    dict(name='emb_d8_n257_same', d=8, N=257, ids='same', p=0.3, two=True),
    dict(name='emb_d8_n300_unique', d=8, N=300, ids='unique', p=0.3, two=False),
    dict(name='emb_d520_n257_rand', d=520, N=257, ids='rand', p=0.3, two=True),
    dict(name='emb_d520_n300_same', d=520, N=300, ids='same', p=0.0, two=False),
    dict(name='emb_d520_n1_unique', d=520, N=1, ids='unique', p=0.3, two=True),
    dict(name='emb_d768_n300_rand', d=768, N=300, ids='rand', p=0.0, two=True),
    dict(name='emb_d768_n257_unique', d=768, N=257, ids='unique', p=0.0, two=False),
    dict(name='emb_d768_n300_same', d=768, N=300, ids='same', p=0.3, two=False),
]}


@functools.lru_cache(maxsize=2)
def emb_case(name):
    """ids 'same': every row names id 41; 'unique': each id at most once (a shuffled subset of rows names distinct ids, every other row
    an id OUTSIDE [0, V): -1, -100, V, V + 5); 'rand': ids drawn from [0, V), one row outside"""
    c = dict(EMB_CASES[name])
    g = _gen(name)
    N, d, V = c['N'], c['d'], EMB_V
    if c['ids'] == 'same':
        ids = torch.full((N,), 41, dtype=torch.int64)
    elif c['ids'] == 'unique':
        ids = torch.tensor([-1, -100, V, V + 5], dtype=torch.int64)[torch.arange(N) % 4]
        rows = torch.randperm(N, generator=g)[:min(N, V - 7)]
        ids[rows] = torch.randperm(V, generator=g)[:len(rows)]
    else:
        ids = torch.randint(0, V, (N,), generator=g)
        if N > 1:
            ids[N // 2] = V
    seed, site = _seed_site(name)
    r = lambda *s: bf16_exact(torch.randn(*s, generator=g))
    c.update(V=V, ids=ids, E=r(V, d), dout=r(N, d), dout2=r(N, d) if c['two'] else None, pat=pattern((V, d), 0.29, 19), seed=seed,
             site=site, valid=(ids >= 0) & (ids < V))
    return c


def emb_ref(c, dt, site_fault=False):
    """-> dict(out (before the bf16 rounding; rows with an id outside [0, V) read table row 0), dE (the amount added; such rows add nothing))"""
    N, d, p = c['N'], c['d'], c['p']
    keep = flat_keep(c['seed'], c['site'], (N, d), p, form32=False, site_fault=site_fault) if p > 0 else torch.ones(N, d, dtype=torch.bool)
    ds = _dscale(p, dt)
    zero = torch.zeros((), dtype=dt)
    idc = torch.where(c['valid'], c['ids'], torch.zeros_like(c['ids']))
    out = torch.where(keep, c['E'].to(dt)[idc] * EMB_SCALE * ds, zero)
    gsum = c['dout'].to(dt) + (c['dout2'].to(dt) if c['dout2'] is not None else 0)
    gr = torch.where(keep, gsum * EMB_SCALE * ds, zero)
    dE = torch.zeros(c['V'], d, dtype=F64)
    for v in torch.unique(c['ids'][c['valid']]).tolist():
        dE[v] = sum_onto(c['pat'][v], gr[c['ids'] == v], dt)
    return dict(out=out.double(), dE=dE)


# ======================================================================================================================== sinusoid table
SIN_CASES = {f'sin_m{M}_d{d}_c{cl}_p{int(p * 100)}': dict(M=M, d=d, clamp=cl, p=p)
             for (M, d, cl) in ((1, 2, 0), (300, 6, 200), (300, 128, 200), (4099, 64, 0)) for p in (0.0, 0.1)}


def sin_ref(name, dt, fault=None):
    """-> out (M, d) before the bf16 rounding.  Faults: 'cos_no_half' the cosine half's mask indexed without the d / 2 offset"""
    c = SIN_CASES[name]
    M, d, cl, p = c['M'], c['d'], c['clamp'], c['p']
    half = d // 2
    seed, site = _seed_site(name)
    dist = torch.arange(M)
    pos = (dist.clamp_max(cl) if cl > 0 else dist).to(dt)
    k2 = (2 * torch.arange(half)).to(dt)
    e = k2 / torch.tensor(float(d), dtype=dt)
    pw = torch.pow(torch.tensor(10000.0, dtype=F64), e.double()).to(dt)         # float32: a correctly rounded powf of the float32 exponent
    a = pos[:, None] * (1.0 / pw)[None, :]
    s, co = torch.sin(a.double()).to(dt), torch.cos(a.double()).to(dt)
    if p > 0:
        i0 = (dist.numpy().astype(np.uint64)[:, None] * np.uint64(d) + np.arange(half, dtype=np.uint64)[None, :])
        i1 = i0 if fault == 'cos_no_half' else i0 + np.uint64(half)
        ds = _dscale(p, dt)
        zero = torch.zeros((), dtype=dt)
        s = torch.where(torch.from_numpy(keep_mask(seed, site, i0, p)), s * ds, zero)
        co = torch.where(torch.from_numpy(keep_mask(seed, site, i1, p)), co * ds, zero)
    return torch.cat([s, co], 1).double()


def sin_mask_counts(name):
    c = SIN_CASES[name]
    seed, site = _seed_site(name)
    k = keep_mask(seed, site, np.arange(c['M'] * c['d'], dtype=np.uint64), c['p'])
    return int(k.sum()), int((~k).sum())


# ======================================================================================================================== dropout, transpose
DROPOUT_N = (8, 8 * 257, 8 * (2048 * 256 + 3))
DROPOUT_P = (0.1, 0.5)
TRANSPOSE_SHAPES = ((1, 1), (63, 65), (64, 64), (130, 70))


def dropout_case(n, p):
    """-> (x bf16 (n,), expected y bf16 (n,), seed, site): y = bf16(x dscale) where kept, exact"""
    name = f'drop_n{n}_p{p}'
    x = bf16_exact(torch.randn(n, generator=_gen(name)))
    seed, site = _seed_site(name)
    keep = flat_keep(seed, site, (n,), p)
    return x, torch.where(keep, x.float() * dscale32(p), torch.zeros(())).to(torch.bfloat16), seed, site, keep


# ======================================================================================================================== adaptive head
HEAD_CASES = {r['name']: r for r in [
    dict(name='h_v300', V=300, cut=(), B=3, T=17, pad=0, gs=1.0),
    dict(name='h_v300_all_ignored', V=300, cut=(), B=1, T=2, pad=3, gs=1.0, all_ignored=True),
    dict(name='h_v1190', V=1190, cut=(1000,), B=5, T=13, pad=3, gs=1.0),
    dict(name='h_v1190_gs', V=1190, cut=(1000,), B=1, T=2, pad=0, gs=0.5),
    dict(name='h_v500_c3', V=500, cut=(64, 65, 300), B=5, T=13, pad=3, gs=0.5),
    dict(name='h_v2048', V=2048, cut=(), B=3, T=17, pad=3, gs=1.0),
    dict(name='h_v2049', V=2049, cut=(), B=3, T=17, pad=0, gs=0.5),
    dict(name='h_v5000_c1000', V=5000, cut=(1000,), B=5, T=13, pad=0, gs=1.0),
    dict(name='h_v5000_c3000', V=5000, cut=(3000,), B=3, T=17, pad=3, gs=0.5),
]}


@functools.lru_cache(maxsize=2)
def head_case(name):
    """float32 logits of a few units (B T, V + ncl); rows 1, 5, 9, .. carry one column 60 above the rest, on a column that is not
    the row's label and, for a tail label, inside the label's own cluster or on its cluster column; rows 2, 12, 22, .. are shifted by
    +3e4 as a whole (`shifted`).  Labels: valid ids mixed with -100, one label >= V, batch row B - 1 entirely -100"""
    c = dict(HEAD_CASES[name])
    g = _gen(name)
    V, cut, B, T = c['V'], c['cut'], c['B'], c['T']
    ncl = len(cut)
    R = B * T
    logits = torch.randn(R, V + ncl, generator=g) * 1.5
    labels = torch.randint(0, V, (B, T), generator=g)
    edges = [0] + list(cut) + [V]
    for i in range(B):                       # every cluster is some label's
        for t in range(T):
            k = (i * T + t) % (ncl + 1)
            labels[i, t] = edges[k] + int(torch.randint(0, edges[k + 1] - edges[k], (1,), generator=g))
    labels[torch.rand(B, T, generator=g) < 0.2] = -100
    if c.get('all_ignored'):
        labels[:] = -100
    else:
        if B > 1:
            labels[B - 1] = -100
        labels[0, 1] = 7 % V                 # row 0 has a live label whatever was drawn
        if T > 3:
            labels[0, 3] = V + 2             # one label outside the vocabulary
    shifted = torch.zeros(R, dtype=torch.bool)
    for row in range(R):
        b, t = divmod(row, T)
        lab = int(labels[b, t + 1]) if t < T - 1 else -100
        if row % 4 == 1:
            col = (row * 37) % V
            if 0 <= lab < V:
                ci = sum(1 for e in cut if lab >= e)
                lo, hi = edges[ci], edges[ci + 1]
                col = lo + (row * 37) % (hi - lo)
                if col == lab:
                    col = lab + 1 if lab + 1 < hi else (lab - 1 if lab - 1 >= lo else V + ci - 1)     # a one-column cluster: its cluster column
            logits[row, col] += 60.0
        elif row % 10 == 2:
            logits[row] += 3e4
            shifted[row] = True
    c.update(ncl=ncl, R=R, logits=logits, labels=labels, edges=edges, shifted=shifted, groups=[shifted, ~shifted])
    return c


def _expf(x):
    """float32: the fast exponential, 2^(x log2e) with the product rounded to float32"""
    return torch.exp(x) if x.dtype == F64 else torch.exp2(x * LOG2E_F32)


def _logf(x):
    return torch.log(x) if x.dtype == F64 else torch.log2(x) * LN2_F32


def _lse(vals, dt):
    m = vals.max()
    return m + _logf(ssum(_expf(vals - m), 0))


def head_ref(c, dt, fault=None):
    """-> dict(nll (B, T - 1), lse (R, 2), acc0, count, dlogits (R, V + ncl) before the bf16 rounding and the two-term split, logprob
    (R, V)).  Faults: 'tail_short' a tail lse without its last column, 'cluster_col' column V + ci taken for V + ci - 1 (labels of the
    clusters below the last)"""
    V, ncl, B, T, R, edges = c['V'], c['ncl'], c['B'], c['T'], c['R'], c['edges']
    L = c['logits'].to(dt)
    nll = torch.zeros(B, T - 1, dtype=dt)
    lse = torch.zeros(R, 2, dtype=dt)
    logprob = torch.zeros(R, V, dtype=dt)
    hl = torch.zeros(R, dtype=dt)
    for row in range(R):
        l = L[row]
        hl[row] = _lse(torch.cat([l[:edges[1]], l[V:V + ncl]]), dt)
        logprob[row, :edges[1]] = l[:edges[1]] - hl[row]
        for ci in range(1, ncl + 1):
            tl = _lse(l[edges[ci]:edges[ci + 1]], dt)
            logprob[row, edges[ci]:edges[ci + 1]] = (l[V + ci - 1] - hl[row]) + (l[edges[ci]:edges[ci + 1]] - tl)
    live = []
    for row in range(R):
        b, t = divmod(row, T)
        if t == T - 1:
            continue
        lab = int(c['labels'][b, t + 1])
        if lab < 0 or lab >= V:
            continue
        l = L[row]
        ci = sum(1 for e in c['cut'] if lab >= e)
        if ci == 0:
            v, tl = hl[row] - l[lab], torch.zeros((), dtype=dt)
        else:
            hi = edges[ci + 1] - (1 if fault == 'tail_short' else 0)
            tl = _lse(l[edges[ci]:hi], dt)
            col = V + ci - 1 + (1 if fault == 'cluster_col' and ci < ncl else 0)
            v = (hl[row] - l[col]) + (tl - l[lab])
        nll[b, t] = v
        lse[row, 0], lse[row, 1] = hl[row], tl
        live.append((row, lab, ci))
    flat = nll.reshape(-1)
    acc0 = ssum(flat, 0)
    count = int((flat != 0).sum())
    gs = torch.tensor(c['gs'], dtype=dt) / torch.tensor(float(max(count, 1)), dtype=dt)
    dl = torch.zeros(R, V + ncl, dtype=dt)
    for row, lab, ci in live:
        b, t = divmod(row, T)
        if nll[b, t] == 0:
            continue
        l = L[row]
        d = torch.zeros(V + ncl, dtype=dt)
        d[:edges[1]] = _expf(l[:edges[1]] - lse[row, 0])
        d[V:] = _expf(l[V:] - lse[row, 0])
        if ci == 0:
            d[lab] -= 1.0
        else:
            d[V + ci - 1] -= 1.0
            d[edges[ci]:edges[ci + 1]] = _expf(l[edges[ci]:edges[ci + 1]] - lse[row, 1])
            d[lab] -= 1.0
        dl[row] = d * gs
    return dict(nll=nll.double(), lse=lse.double(), acc0=acc0.double().reshape(1), count=count, dlogits=dl.double(), logprob=logprob.double())


@functools.lru_cache(maxsize=2)
def head_expect(name):
    c = head_case(name)
    return c, head_ref(c, F64), head_ref(c, F32)


def split_terms(model_dl):
    """the two bf16 terms the split call stores for float32 values: hi = bf16(d), lo = bf16(d - hi)"""
    hi = model_dl.float().to(torch.bfloat16)
    lo = (model_dl.float() - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


HEAD_KEYS = ('nll', 'lse', 'acc0', 'dlogits', 'logprob')


def head_groups(c, k):
    """the rows shifted by 3e4 are a magnitude class of their own for lse; nll and logprob are differences of order 1 to 70 in every row"""
    return c['groups'] if k == 'lse' else None


def head_gaps(name):
    c, ref, model = head_expect(name)
    if ref['count'] == 0:
        return {k: 0.0 for k in HEAD_KEYS if k != 'logprob'} | dict(logprob=groups_gap(model['logprob'], ref['logprob']))
    return {k: groups_gap(model[k], ref[k], head_groups(c, k)) for k in HEAD_KEYS}


# ======================================================================================================================== optimiser
SUMSQ_N = (1, 2, 3, 4, 5, 1023, 4 * (2048 * 256) + 7)
SUMSQ_PRIOR = 3.25


def sumsq_case(n, spiky=False):
    """x (n,) f32; `spiky`: elements of 1e-3 with a few of 1e3 among them"""
    g = _gen(f'sq_n{n}_{spiky}')
    x = torch.randn(n, generator=g)
    if spiky:
        x = x * 1e-3
        x[torch.randint(0, n, (min(n, 5),), generator=g)] = 1e3
    return x


def sumsq_key(n):
    """the bound a size is judged under: sums over one grid pass (2048 * 256 vectors of 4) have a sequential-sum gap of their own"""
    return 'sumsq_big' if n // 4 > 2048 * 256 else 'sumsq'


def sumsq_ref(x, dt):
    """the value left in the accumulator"""
    return (torch.tensor(SUMSQ_PRIOR, dtype=F64) + sum_onto(torch.tensor([SUMSQ_PRIOR]), (x.to(dt) * x.to(dt)).unsqueeze(1), dt)).reshape(1)


_AW = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)
ADAMW_CASES = {r['name']: r for r in [
    dict(name='aw_n1', n=1, n_decay=0, clip='none', w16=True, step0=1, gs=1.0),
    dict(name='aw_n255_above', n=255, n_decay=255, clip='above', w16=True, step0=1, gs=0.5),
    dict(name='aw_n255_below', n=255, n_decay=100, clip='below', w16=False, step0=100000, gs=0.5),
    dict(name='aw_n10007_above', n=10007, n_decay=4099, clip='above', w16=True, step0=100000, gs=1.0),
    dict(name='aw_n10007_nosumsq', n=10007, n_decay=10007, clip='nosumsq', w16=True, step0=1, gs=0.5),
    dict(name='aw_n10007_maxnorm0', n=10007, n_decay=0, clip='maxnorm0', w16=False, step0=1, gs=1.0),
    dict(name='aw_big_above', n=2048 * 256 + 257, n_decay=2048 * 256 + 3, clip='above', w16=True, step0=1, gs=0.5),
    dict(name='aw_big_below', n=2048 * 256 + 257, n_decay=2048 * 256 + 257, clip='below', w16=True, step0=100000, gs=1.0),
]}
ADAMW_STEPS = 3


@functools.lru_cache(maxsize=2)
def adamw_case(name):
    """p, m, v and three gradients.  Elements n // 3 .. n // 3 + 3 (n >= 16) have g = 0 and v = 0 in every step (eps alone is the
    denominator), m tiny or zero.  sumsq: the float32 sum of squares of each gradient, GIVEN to the kernel and to the reference alike;
    max_norm twice / a quarter of the scaled norm ('below' / 'above')"""
    c = dict(ADAMW_CASES[name])
    g = _gen(name)
    n = c['n']
    p, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    gr = [torch.randn(n, generator=g) * (0.5 + k) for k in range(ADAMW_STEPS)]
    z0 = n // 3
    if n >= 16:
        for t in gr:
            t[z0:z0 + 4] = 0
        v[z0:z0 + 4] = 0
        m[z0:z0 + 4] = torch.tensor([0.0, 1e-7, -3e-8, 0.0])
    if 0 < c['n_decay'] < n:                 # the two elements at the decay boundary are of order 1
        p[c['n_decay'] - 1], p[c['n_decay']] = 1.5, -1.25
    sumsq = [float(np.float32(float((t.double() ** 2).sum()))) for t in gr]
    norm = [np.sqrt(s) * c['gs'] for s in sumsq]
    max_norm = [float(np.float32({'below': 2.0, 'above': 0.25}.get(c['clip'], 1.0) * x)) for x in norm]
    if c['clip'] == 'maxnorm0':
        max_norm = [0.0] * ADAMW_STEPS
    c.update(p=p, m=m, v=v, g=gr, sumsq=sumsq, max_norm=max_norm, **{k: float(np.float32(x)) for k, x in _AW.items()})
    return c


def adamw_consts(c, step, fault=None):
    s = step - 1 if fault == 'bias_step' else step
    bc1 = float(np.float32(1.0 - c['b1'] ** s))
    bc2s = float(np.float32(np.sqrt(1.0 - c['b2'] ** s)))
    return bc1, bc2s


def adamw_step_ref(c, st, k, dt, fault=None):
    """one step of include/musicxl.h's formula on state `st` = (p, m, v) with gradient k -> new (p, m, v).  The float32 lr, betas, eps,
    weight decay and the launch function's float32 bias corrections are given constants.  Faults: 'decay_le' decay at i <= n_decay,
    'bias_step' the bias corrections of step - 1, 'clip_no_gs' the clip coefficient from the unscaled norm"""
    f = np.float32 if dt == F32 else np.float64
    step = c['step0'] + k
    bc1, bc2s = adamw_consts(c, step, fault)
    lr, b1, b2, eps, wd, gs = (f(c[x]) for x in ('lr', 'b1', 'b2', 'eps', 'wd', 'gs'))
    coef = gs
    if c['max_norm'][k] > 0 and c['clip'] != 'nosumsq':
        norm = f(np.sqrt(f(c['sumsq'][k]))) * (f(1) if fault == 'clip_no_gs' else gs)
        coef = f(coef * min(f(f(c['max_norm'][k]) / f(norm + f(1e-6))), f(1)))
    p, m, v = (t.to(dt) for t in st)
    gi = c['g'][k].to(dt) * float(coef)
    nd = c['n_decay'] + (1 if fault == 'decay_le' else 0)
    p = p.clone()
    p[:nd] = p[:nd] * float(f(f(1) - f(lr * wd)))
    m = float(b1) * m + float(f(f(1) - b1)) * gi
    v = float(b2) * v + float(f(f(1) - b2)) * gi * gi
    denom = torch.sqrt(v) / float(f(bc2s)) + float(eps)
    p = p - float(f(lr / f(bc1))) * (m / denom)
    return p, m, v


def adamw_chain(c, dt, fault=None):
    """ADAMW_STEPS consecutive steps on carried state -> list of (p, m, v) as float64"""
    st = (c['p'], c['m'], c['v'])
    out = []
    for k in range(ADAMW_STEPS):
        st = adamw_step_ref(c, st, k, dt, fault)
        out.append(tuple(t.double() for t in st))
    return out
