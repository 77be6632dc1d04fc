"""Every dispatch arm of the GEMM launcher (csrc/gemm.hip: gemm_bf16_kernel, gemm_nt256_kernel at both tile widths, gemm_nt256w4_kernel,
gemm_tt256_kernel, the batched form) and the skinny forms (csrc/gemm_skinny.hip), element-wise against a float64 reference by the rule
of oracle/kernel_cases.py:  |got - ref| <= a |ref| + b max|ref|,  a = 2^-8 for bf16 outputs, 2^-24 for float32 outputs.  The rows are
in oracle/kernel_cases.py (GEMM_CASES and the smaller tables; the comment above the table maps launcher arms to rows).  Inputs are
bf16-exact; bias, alpha and prior contents are float32 values.

What is bit-exact instead: everything outside [0, M) x [0, N) of an output allocated with ldc > N, spare rows and (some rows) an
offset from 16-byte alignment keeps its sentinel bit pattern; the zeros of a dropout output are exactly ~keep_mask / ~pair_keep_mask
(the host statements of the masks) wherever the undropped float64 value is above the bound's absolute term; mxl_dropout_bf16 draws
keep_mask; repeats of the non-atomic forms are bit-identical; the kernel a row means to reach is the one mxl_gemm_last_nt_kernel names.

b per kernel family = 4 x the largest CPU gap between a sequential-float32 and the float64 evaluation over the family's rows
(measured on each row's sub-block: first / last 24 rows x first / last 64 columns; re-measured and held under b in every test).
The float64 reference of the rows with M N K >= 2^26 is torch's float64 matmul on the device (rocBLAS: an implementation that shares
nothing with the kernels here); the smaller ones are evaluated on the CPU.  Every element of every row is compared (share 1.0: all
edge tiles and all interior tiles).

    family (rows)                                   CPU gap    b         largest device error / max|ref|  (MI355X)
    generic  (g_*: gemm_bf16_kernel, K <= 1032)     5.3e-7     2.2e-6    float32 out 1.4e-7 (0.06 of the bound), bf16 out 3.4e-3
    nt       (nt_*, w4_*: large tiles, K <= 192)    2.1e-7     8.8e-7    float32 out 1.7e-7 (0.18), bf16 out 3.8e-3
    nt_k3072 (K = 3072, eight and four waves)       1.2e-6     4.9e-6    bf16 out 3.2e-3
    tt256    (tt_*: K = 8192 ... 16384)             4.3e-6     1.8e-5    6.2e-7 (0.03)
    batched  (BATCHED_CASES)                        1.4e-7     5.5e-7    float32 out 9.8e-8 (0.17), bf16 out 2.8e-3
    skinny   (SKINNY_CASES, the partial form too)   5.8e-7     2.4e-6    float32 out 9.2e-8 (0.04), bf16 out 2.8e-3
    colsum   (fused column sums over 16384 rows)    1.8e-6     7.4e-6    3.0e-7 (0.04)
    head-dot delta: 0.38 of its bound.  A bf16 output's error is its one rounding (up to 2^-8 |ref|: 0.99 of the bound at the
    worst element of every family); the float32 outputs show what the accumulation itself costs.
Wall time of the module on the device: 9 s (117 tests).
"""
import numpy as np
import pytest
import torch

from oracle.kernel_cases import (A_BF16, A_F32, ADD_AUX, ATOMIC, BATCHED_CASES, BIAS, BWD_BITS, COLSUM_CASES, DROPOUT, F32, GEMM_CASES,
                                 MASK_BITS_CASES, RELU, RELU_BWD, SAVE_MASK, SKINNY_CASES, batched_inputs, batched_ref, bf16_exact,
                                 case_gap, case_inputs, case_keep, check_gap, gap, gemm_ref, gemm_ref32, keep_mask, pair_keep_mask,
                                 skinny_inputs, sub_block, worst)

pytestmark = pytest.mark.gpu

# 4 x the CPU gaps in the module docstring
B = {'generic': 2.2e-6, 'nt': 8.8e-7, 'nt_k3072': 4.9e-6, 'tt256': 1.8e-5, 'batched': 5.5e-7, 'skinny': 2.4e-6, 'colsum': 7.4e-6}

SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5          # NaN bit patterns no kernel produces (a float add would quieten them: 0x7FE5...)
GARBAGE = 30000.0                            # operand padding: finite, and ruinous if it is ever multiplied into an output


def frame(rows, ld, off, f32, dev):
    """-> (flat sentinel buffer, its (rows, ld) view starting `off` elements in) -- the view is what a kernel is given as C"""
    flat = torch.full((off + rows * ld + 16,), SENT32 if f32 else SENT16, dtype=torch.int32 if f32 else torch.int16, device=dev)
    return flat, flat.view(torch.float32 if f32 else torch.bfloat16)[off:off + rows * ld].view(rows, ld)


def untouched(flat, off, rows, ld, M, N):
    """every element of the buffer outside [0, M) x [0, N) of the view still holds the sentinel"""
    out = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
    out[off:off + rows * ld].view(rows, ld)[:M, :N] = False
    sent = SENT32 if flat.dtype == torch.int32 else SENT16
    return bool((flat[out] == sent).all())


def store(X, trans, pad, dev, spare=128):
    """operand storage of a logical (R, K) matrix: (R, K + pad), or transposed (K + spare, ceil8(R) + pad) -- the padding and the
    spare rows (a K-slice that ran past K would read them) hold GARBAGE"""
    R, K = X.shape
    if trans:
        st = torch.full((K + spare, (R + 7) // 8 * 8 + pad), GARBAGE, dtype=torch.bfloat16)
        st[:K, :R] = X.t()
    else:
        st = torch.full((R, K + pad), GARBAGE, dtype=torch.bfloat16)
        st[:, :K] = X
    return st.to(dev), st.shape[1]


def padded(v, dev):
    """a float32 vector with 8 spare GARBAGE elements behind it"""
    st = torch.full((v.numel() + 8,), GARBAGE)
    st[:v.numel()] = v
    return st.to(dev)


class reserved_cus:
    def __init__(self, k):
        self.k = k

    def __enter__(self):
        from symbolic_music_generation_amd import ops
        if self.k:
            ops.check(ops.lib().mxl_set_reserved_cus(self.k), 'mxl_set_reserved_cus')

    def __exit__(self, *exc):
        from symbolic_music_generation_amd import ops
        ops.check(ops.lib().mxl_set_reserved_cus(0), 'mxl_set_reserved_cus')


def set_w4(monkeypatch, w4):
    if w4 is None:
        monkeypatch.delenv('MXL_GEMM_W4', raising=False)
    else:
        monkeypatch.setenv('MXL_GEMM_W4', w4)


def zero_pattern_ok(got, x, c, keep, und, b):
    """the dropped set of a dropout output == ~keep exactly, wherever the undropped float64 value `und` is above the bound's absolute
    term (a float32 sum may cancel to zero where float64 leaves 1e-9).  With ADD_AUX the dropped elements are those that equal aux
    bit for bit (0 + aux is exact), compared where the kept term is at least 2^-5 |aux| (four bf16 steps of aux: it cannot round away)"""
    sig = und.abs() > b * und.abs().max()
    if c['flags'] & ADD_AUX:
        aux = x['aux'].to(got.device)
        sig &= und.abs() >= 2.0 ** -5 * aux.double().abs()
        dropped = got == aux
    else:
        dropped = got == 0
    return bool(((dropped == ~keep) | ~sig).all()), sig.double().mean().item()


@pytest.mark.parametrize('c', GEMM_CASES, ids=[c['name'] for c in GEMM_CASES])
def test_gemm_case(dev, monkeypatch, c):
    """one row of GEMM_CASES: values against float64, padding, kernel choice, repeatability, dropout zero pattern, CPU gap"""
    from symbolic_music_generation_amd import ops
    M, N, K, flags, fam = c['M'], c['N'], c['K'], c['flags'], c['fam']
    b = B[fam]
    x = case_inputs(c)
    keep = case_keep(c, x['seed'], x['site'])
    f32 = bool(flags & (F32 | ATOMIC))
    a_d, lda = store(x['A'], c['ta'], c['lda_pad'], dev)
    b_d, ldb = store(x['B'], c['tb'], c['ldb_pad'], dev)
    bias_d = padded(x['bias'], dev) if flags & BIAS else None
    aux_d, ldaux = None, None
    if x['aux'] is not None:
        ldaux = N + c['ldaux_pad']
        aux_st = torch.full((M, ldaux), GARBAGE, dtype=torch.bfloat16)
        aux_st[:, :N] = x['aux']
        aux_d = aux_st.to(dev)
    rows, ldc, off = M + 2, N + c['ldc_pad'], c['c_off']
    set_w4(monkeypatch, c['w4'])
    outs = []
    with reserved_cus(c['reserve']):
        for _ in range(2):
            flat, cv = frame(rows, ldc, off, f32, dev)
            if flags & ATOMIC:
                cv[:M, :N] = x['c0'].to(dev)
            ops.gemm(a_d, b_d, cv, M, N, K, trans_a=c['ta'], trans_b=c['tb'], flags=flags, alpha=c['alpha'], bias=bias_d, aux=aux_d,
                     ksplits=c['ksplits'], lda=lda, ldb=ldb, ldc=ldc, ldaux=ldaux, drop_p=c['p'], seed=x['seed'], site=x['site'])
            assert ops.lib().mxl_gemm_last_nt_kernel() == c['expect'], 'the row is not on the kernel it was written for'
            outs.append((flat, cv))
    torch.cuda.synchronize()
    (flat, cv), (flat2, _) = outs
    assert untouched(flat, off, rows, ldc, M, N), 'a store outside [0, M) x [0, N)'
    if not (flags & ATOMIC):
        assert torch.equal(flat, flat2), 'repeat calls differ'
    rdev = dev if M * N * K >= 2 ** 26 else torch.device('cpu')

    def on(t):
        return None if t is None else t.to(rdev)
    kw = dict(trans_a=False, trans_b=False, alpha=c['alpha'], bias=on(x['bias']))
    ref = gemm_ref(on(x['A']), on(x['B']), flags=flags, aux=on(x['aux']), keep=on(keep), p=c['p'], c0=on(x['c0']), **kw)
    got = cv[:M, :N].to(rdev)
    w, e = worst(got, ref, A_F32 if f32 else A_BF16, b)
    g = case_gap(c, x, keep)
    print(f"{c['name']}: worst {w:.3f} of the bound, max error {e:.2e} of max|ref|, CPU gap {g:.2e} (b {b:.1e})")
    check_gap(g, b)
    assert w <= 1.0, (c['name'], w, e)
    if keep is not None:
        und = gemm_ref(on(x['A']), on(x['B']), flags=flags & (BIAS | RELU), **kw)
        ok, share = zero_pattern_ok(got, x, c, on(keep), und, b)
        assert ok, 'the zeros of the output are not the dropped set of the host mask'
        assert share > (0.3 if flags & RELU else 0.9)           # (relu leaves half of the elements without a say)


@pytest.mark.parametrize('n,p,seed,site', [(4096, 0.1, 5, 3), (1000 * 8, 0.5, (7 << 32) | 5, 3), (2056, 0.25, 2 ** 63 - 1, 0xFFFFFFFF),
                                           (3072 * 40, 0.1, 0x9E3779B97F4A7C15 >> 1, 17)])
def test_dropout_kernel_draws_keep_mask(dev, n, p, seed, site):
    """mxl_dropout_bf16 on n elements: zeros exactly where keep_mask(seed, site, flat index, p) says drop, the rest x / (1 - p)
    -- the mask the DROPOUT / BIAS | DROPOUT / ADD_AUX | DROPOUT epilogues are held to in test_gemm_case, so the contract
    between the GEMM epilogue and the kernels that regenerate its mask rests on the one host statement"""
    from symbolic_music_generation_amd import ops
    g = torch.Generator().manual_seed(n)
    xs = bf16_exact(torch.randn(n, generator=g).abs() + 0.5)
    y = torch.empty(n, dtype=torch.bfloat16, device=dev)
    ops.dropout(xs.to(dev), y, p, seed=seed, site=site)
    torch.cuda.synchronize()
    keep = torch.from_numpy(keep_mask(seed, site, np.arange(n, dtype=np.uint64), p))
    y = y.cpu()
    assert torch.equal(y == 0, ~keep)
    ref = torch.where(keep, xs.double() / (1.0 - float(np.float32(p))), torch.zeros((), dtype=torch.float64))
    assert worst(y, ref, A_BF16, 1e-7)[0] <= 1.0
    assert abs((~keep).double().mean().item() - p) < 5 * (p * (1 - p) / n) ** 0.5          # five standard deviations of a fair draw


@pytest.mark.parametrize('name,M,N,K', COLSUM_CASES, ids=[c[0] for c in COLSUM_CASES])
def test_fused_colsum_against_float64(dev, monkeypatch, name, M, N, K):
    """mxl_gemm_bf16_colsum with RELU_BWD on the large-tile path: colsum += column sums of the epilogue's values, on top of non-zero
    contents, against the float64 column sums of the float64 epilogue values (a = 2^-24; the CPU gap is that of a float32
    evaluation of the same sums, one sequential accumulator over K and one over the rows, on 64 columns); C as in test_gemm_case"""
    from symbolic_music_generation_amd import ops
    set_w4(monkeypatch, None)
    c = dict(name=name, M=M, N=N, K=K, flags=RELU_BWD, alpha=1.25, p=0.0)
    x = case_inputs(c)
    a_d, b_d, aux_d = x['A'].to(dev), x['B'].to(dev), x['aux'].to(dev)
    cs0 = torch.randn(N, generator=torch.Generator().manual_seed(M + N))
    cs = cs0.to(dev)
    flat, cv = frame(M + 2, N + 8, 0, False, dev)
    ops.gemm(a_d, b_d, cv, M, N, K, flags=RELU_BWD, alpha=1.25, aux=aux_d, ldc=N + 8, colsum=cs)
    assert ops.lib().mxl_gemm_last_nt_kernel() == 1
    torch.cuda.synchronize()
    assert untouched(flat, 0, M + 2, N + 8, M, N)
    ref = gemm_ref(a_d, b_d, flags=RELU_BWD, alpha=1.25, aux=aux_d)
    w, e = worst(cv[:M, :N], ref, A_BF16, B['nt'])
    ci = torch.arange(N - 64, N)
    r32 = gemm_ref32(x['A'], x['B'][ci], flags=RELU_BWD, alpha=1.25, aux=x['aux'][:, ci])
    s32 = cs0[ci].clone()
    for m in range(M):
        s32 += r32[m]
    sref = cs0.double().to(dev) + ref.sum(0)
    g = gap(s32, sref[ci.to(dev)].cpu())
    ws, es = worst(cs, sref, A_F32, B['colsum'])
    print(f'{name}: C worst {w:.3f} ({e:.2e}); colsum worst {ws:.3f}, max error {es:.2e} of max|ref|, CPU gap {g:.2e} (b {B["colsum"]:.1e})')
    check_gap(g, B['colsum'])
    assert w <= 1.0 and ws <= 1.0, (w, ws)


def _grid(shape, g, step, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float() * step


@pytest.mark.parametrize('name,M,N,K,p', MASK_BITS_CASES, ids=[c[0] for c in MASK_BITS_CASES])
def test_relu_mask_bits_against_float64(dev, monkeypatch, name, M, N, K, p):
    """SAVE_RELU_MASK then RELU_BWD_BITS (alone and with the fused column sums): the forward activations against float64 with
    pair_keep_mask, the backward result against gemm_ref with aux = (float64 activations > 0).
    Condition on the inputs: x, w are multiples of 1/8 in [-1/2, 1/2], the bias an odd multiple of 1/128, K = 64 -- every
    pre-activation is an odd multiple of 1/128, exact in float32 in any summation order, so none lies within the bound of zero and no
    element is excluded (counted on the float64 reference, cap 0)."""
    from symbolic_music_generation_amd import ops
    set_w4(monkeypatch, None)
    g = torch.Generator().manual_seed(M + K)
    xs, w1 = _grid((M, K), g, 0.125, 4).bfloat16(), _grid((N, K), g, 0.125, 4).bfloat16()
    b1 = (2 * torch.randint(-64, 64, (N,), generator=g) + 1).float() / 128
    nbytes = ops.gemm_relu_mask_bytes(M, N)
    assert nbytes == M * N // 8
    fl = BIAS | RELU | (DROPOUT if p > 0 else 0)
    seed, site = (3 << 32) | 9, 2
    keep = torch.from_numpy(pair_keep_mask(seed, site, M, N, p)).to(dev) if p > 0 else None
    x_d, w_d, b_d = xs.to(dev), w1.to(dev), b1.to(dev)
    bits = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    flat, act = frame(M + 2, N + 8, 0, False, dev)
    ops.gemm(x_d, w_d, act, M, N, K, flags=fl | SAVE_MASK, aux=bits, bias=b_d, ldc=N + 8, drop_p=p, seed=seed, site=site)
    assert ops.lib().mxl_gemm_last_nt_kernel() == 1
    pre = gemm_ref(x_d, w_d, flags=BIAS, bias=b_d)
    assert int((pre.abs() < 1.0 / 256).sum().item()) == 0                       # excluded elements: none (cap 0)
    act64 = gemm_ref(x_d, w_d, flags=fl, bias=b_d, keep=keep, p=p)
    wf, ef = worst(act[:M, :N], act64, A_BF16, B['nt'])
    assert untouched(flat, 0, M + 2, N + 8, M, N)
    if p > 0:
        assert torch.equal(act[:M, :N] == 0, ~(keep & (pre > 0)))
    g2 = torch.Generator().manual_seed(N + K)
    dy, w2 = bf16_exact(torch.randn(M, K, generator=g2) * 0.5), bf16_exact(torch.randn(N, K, generator=g2) * 0.5)
    dy_d, w2_d = dy.to(dev), w2.to(dev)
    alpha = 1.0 / (1.0 - p)
    ref = gemm_ref(dy_d, w2_d, flags=BWD_BITS, alpha=alpha, aux=act64 > 0)
    cs0 = torch.randn(N, generator=g2)
    res = []
    for with_sums in (False, True):
        cs = cs0.to(dev)
        flat, d = frame(M + 2, N + 8, 0, False, dev)
        ops.gemm(dy_d, w2_d, d, M, N, K, flags=BWD_BITS, aux=bits, alpha=alpha, ldc=N + 8, colsum=cs if with_sums else None)
        assert ops.lib().mxl_gemm_last_nt_kernel() == 1
        assert untouched(flat, 0, M + 2, N + 8, M, N)
        res.append((worst(d[:M, :N], ref, A_BF16, B['nt']), cs))
    ws, es = worst(res[1][1], cs0.double().to(dev) + ref.sum(0), A_F32, B['colsum'])
    ri, ci = sub_block(M, N)
    kw = dict(flags=BWD_BITS, alpha=alpha, aux=(act64 > 0)[ri.to(dev)][:, ci.to(dev)].cpu())
    gp = gap(gemm_ref32(dy[ri], w2[ci], **kw), gemm_ref(dy[ri], w2[ci], **kw))
    print(f'{name}: forward worst {wf:.3f} ({ef:.2e}); backward worst {res[0][0][0]:.3f} ({res[0][0][1]:.2e}), with sums '
          f'{res[1][0][0]:.3f}; colsum worst {ws:.3f} ({es:.2e}); CPU gap {gp:.2e}')
    check_gap(gp, B['nt'])
    assert wf <= 1.0 and res[0][0][0] <= 1.0 and res[1][0][0] <= 1.0 and ws <= 1.0


@pytest.mark.parametrize('Bt,T,H,K', [(8, 2048, 16, 128), (64, 256, 16, 64)])
def test_headdot_against_float64(dev, monkeypatch, Bt, T, H, K):
    """mxl_gemm_bf16_headdot on the four-wave kernel: C against float64 by the rule, and delta[b, h, t] = sum_e C O against the
    float64 sum.  The kernel forms delta from the bf16 values it stores, so each of the 64 terms carries one bf16 rounding of C: the
    rule's rounding term applies per term,  |got - ref| <= 2^-8 sum_e |C O| + b max_rows(sum_e |C O|)"""
    from symbolic_music_generation_amd import ops
    set_w4(monkeypatch, None)
    M, N = Bt * T, H * 64
    c = dict(name=f'headdot_{Bt}_{T}', M=M, N=N, K=K, flags=ADD_AUX, alpha=1.0, p=0.0)        # (aux: the O operand)
    x = case_inputs(c)
    a_d, b_d, o_d = x['A'].to(dev), x['B'].to(dev), x['aux'].to(dev)
    flat, cv = frame(M + 2, N + 8, 0, False, dev)
    delta = torch.full((Bt, H, T), float('nan'), device=dev)
    took = ops.gemm_headdot(a_d, b_d, cv, M, N, K, o_d, T, delta, ldc=N + 8)
    assert took and ops.lib().mxl_gemm_last_nt_kernel() == 3
    torch.cuda.synchronize()
    assert untouched(flat, 0, M + 2, N + 8, M, N)
    ref = gemm_ref(a_d, b_d)
    w, e = worst(cv[:M, :N], ref, A_BF16, B['nt'])
    terms = (ref * o_d.double()).view(Bt, T, H, 64)
    dref, dabs = terms.sum(-1).permute(0, 2, 1), terms.abs().sum(-1).permute(0, 2, 1)
    wd = ((delta.double() - dref).abs() / (A_BF16 * dabs + B['nt'] * dabs.max())).max().item()
    g = case_gap(dict(c, flags=0), dict(x, aux=None, c0=None), None)
    print(f'headdot {Bt} x {T}: C worst {w:.3f} ({e:.2e}); delta worst {wd:.3f}; CPU gap {g:.2e}')
    check_gap(g, B['nt'])
    assert w <= 1.0 and wd <= 1.0


@pytest.mark.parametrize('c', BATCHED_CASES, ids=[c['name'] for c in BATCHED_CASES])
def test_batched_case(dev, c):
    """mxl_gemm_bf16_batched against a loop of single float64 GEMMs at the header's offsets (by / bdiv) * s1 + (by % bdiv) * s2; every
    element of C that no item owns keeps its sentinel"""
    from symbolic_music_generation_amd import ops
    x = batched_inputs(c)
    ref, written = batched_ref(c, x)
    f32 = bool(c['flags'] & (F32 | ATOMIC))
    flat, cv = frame(1, x['nC'], 0, f32, dev)
    if c['flags'] & ATOMIC:
        cv[0][written.to(dev)] = x['c0'][written].to(dev)
    ops.gemm_batched(x['A'].to(dev), x['B'].to(dev), cv, c['M'], c['N'], c['K'], lda=c['lda'], ldb=c['ldb'], ldc=c['ldc'],
                     trans_a=c['ta'], trans_b=c['tb'], flags=c['flags'], alpha=c['alpha'], ksplits=c['ksplits'], batch=c['batch'],
                     bdiv=c['bdiv'], sA=c['sA'], sB=c['sB'], sC=c['sC'])
    torch.cuda.synchronize()
    fl = flat.cpu()
    sent = SENT32 if f32 else SENT16
    assert bool((fl[:x['nC']][~written] == sent).all()) and bool((fl[x['nC']:] == sent).all())
    got = cv[0].cpu()[written]
    w, e = worst(got, ref[written], A_F32 if f32 else A_BF16, B['batched'])
    r32, _ = batched_ref(c, x, ref=gemm_ref32)
    g = gap(r32[written].float(), ref[written])
    print(f"{c['name']}: worst {w:.3f}, max error {e:.2e} of max|ref|, CPU gap {g:.2e} (b {B['batched']:.1e})")
    check_gap(g, B['batched'])
    assert w <= 1.0


@pytest.mark.parametrize('M,N,K', SKINNY_CASES)
def test_skinny_case(dev, M, N, K):
    """mxl_gemm_skinny_bf16 (BIAS | RELU to bf16; OUT_F32 plain and with BIAS) and mxl_gemm_skinny_partial (KS slabs summed in
    float64, a = 2^-24), with lda, ldw above the minimum, ldc > N and sentinel padding; repeats are bit-identical"""
    from symbolic_music_generation_amd import ops
    a, w_, bias = skinny_inputs(M, N, K)
    a_d, lda = store(a, False, 8, dev)
    w_d, ldw = store(w_, False, 16, dev)
    bias_d = padded(bias, dev)
    b, gmax = B['skinny'], 0.0
    for fl in (BIAS | RELU, F32, F32 | BIAS):
        f32 = bool(fl & F32)
        outs = []
        for _ in range(2):
            flat, cv = frame(M + 1, N + 3, 1, f32, dev)
            ops.gemm_skinny(a_d, w_d, cv, M, N, K, flags=fl, bias=bias_d if fl & BIAS else None, lda=lda, ldw=ldw, ldc=N + 3)
            outs.append(flat)
        torch.cuda.synchronize()
        assert untouched(flat, 1, M + 1, N + 3, M, N) and torch.equal(outs[0], outs[1])
        ref = gemm_ref(a, w_, bias=bias, flags=fl)
        gmax = max(gmax, gap(gemm_ref32(a, w_, bias=bias, flags=fl), ref))
        wv, e = worst(cv[:M, :N].cpu(), ref, A_F32 if f32 else A_BF16, b)
        print(f'skinny ({M}, {N}, {K}) flags {fl:#x}: worst {wv:.3f}, max error {e:.2e} of max|ref|')
        assert wv <= 1.0
    ref = gemm_ref(a, w_)
    for KS in (1, 3, 16):
        flat, slabs = frame(KS * 64, N, 0, True, dev)
        ops.gemm_skinny_partial(a_d, w_d, slabs, M, N, K, KS)
        torch.cuda.synchronize()
        sl = slabs.view(KS, 64, N)
        wr = torch.zeros(KS, 64, N, dtype=torch.bool, device=dev)
        wr[:, :M] = True
        assert bool((flat[:KS * 64 * N][~wr.view(-1)] == SENT32).all()) and bool((flat[KS * 64 * N:] == SENT32).all())
        wv, e = worst(sl[:, :M].double().sum(0).cpu(), ref, A_F32, b)
        print(f'skinny partial ({M}, {N}, {K}) KS {KS}: worst {wv:.3f}, max error {e:.2e} of max|ref|')
        assert wv <= 1.0
    check_gap(gmax, b)


def test_invalid_arguments_are_refused_before_any_launch(dev):
    """host-side refusals (include/musicxl.h: negative = argument error): the documented code, and C keeps its sentinel"""
    from symbolic_music_generation_amd import ops
    lib = ops.lib()
    M, N, K = 64, 64, 64
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
    aux = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
    bias = torch.zeros(N, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    EINVAL, EUNSUPPORTED = -1, -2

    def call(flags, ksplits=1, f32=False, aux_t=None, M_=M, N_=N):
        flat, cv = frame(M_, N_, 0, f32, dev)
        rc = lib.mxl_gemm_bf16(a.data_ptr(), w.data_ptr(), cv.data_ptr(), M_, N_, K, K, K, N_, 0, 0, flags, 1.0, bias.data_ptr(),
                               0 if aux_t is None else aux_t.data_ptr(), N_, ksplits, 0.0, 0, 0, s)
        torch.cuda.synchronize()
        return rc, untouched(flat, 0, M_, N_, 0, 0)

    assert call(F32, ksplits=2, f32=True) == (EINVAL, True)                        # K-split without the atomic flag
    assert call(RELU_BWD | ADD_AUX, aux_t=aux) == (EINVAL, True)
    assert call(BIAS | RELU | SAVE_MASK, aux_t=aux) == (EUNSUPPORTED, True)        # no mask bits at these sizes
    assert ops.gemm_relu_mask_bytes(M, N) == 0
    flat, cv = frame(2 * M, N, 0, False, dev)
    rc = lib.mxl_gemm_bf16_batched(a.data_ptr(), w.data_ptr(), cv.data_ptr(), M // 2, N, K, K, K, N, 0, 0, RELU_BWD, 1.0, 1, 2, 1,
                                   (M // 2) * K, 0, 0, 0, (M // 2) * N, 0, s)
    torch.cuda.synchronize()
    assert rc == EINVAL and untouched(flat, 0, 2 * M, N, 0, 0)
