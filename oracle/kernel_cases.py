"""ORACLE-side helpers of the kernel-level tests (test infrastructure, NOT product code): how a device result is held against
a float64 reference, and the inputs that a CPU test and a GPU test must share.

Tolerance rule.  A float kernel is compared element-wise with a float64 evaluation `ref` of the same formula on the same
(bf16-exact) inputs:

    |got - ref| <= a * |ref| + b * max|ref|

`a` is the one rounding to the kernel's output type: 2^-8 for bf16 outputs (8 significant bits), 2^-24 for float32 outputs.
`b` is 4 x the largest gap, relative to max|ref|, between a float32 evaluation of the reference formula on the CPU (before the
output rounding) and the float64 one over all the cases of the test: what float32 accumulation costs on these very inputs, with
a factor 4 for another summation order and the fast exp / log.  Sums are evaluated with a sequential float32 accumulator, the
least favourable order.  The gaps were measured on the CPU and are written, with the resulting `b`, in each test's docstring.
They move by some tens of per cent with the host's BLAS (its summation order), so every test measures its gap again on its own
inputs and `check_gap` only asks that it stays under `b`, i.e. that the bound never drops below what float32 itself costs.
"""
import numpy as np
import torch

A_BF16 = 2.0 ** -8
A_F32 = 2.0 ** -24


def bf16_exact(x):
    """round to bf16 and back: inputs every precision represents exactly"""
    return x.to(torch.bfloat16)


def gap(r32, r64):
    """max |r32 - r64| / max |r64|: the float32-vs-float64 gap of a reference on one case"""
    return ((r32.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300)).item()


def worst(got, ref, a, b):
    """-> (max over elements of |got - ref| / (a |ref| + b max|ref|), max |got - ref| / max|ref|); the first must be <= 1"""
    ref = ref.double()
    err = (got.double() - ref).abs()
    lim = a * ref.abs() + b * ref.abs().max()
    return (err / lim).max().item(), (err.max() / ref.abs().max().clamp_min(1e-300)).item()


def check_gap(g, b):
    """the CPU float32 gap of this case stays under the bound's absolute term (built as 4 x the largest gap measured)"""
    assert g <= b, (g, b)


def hash_decode_case(dh, seed=7):
    """the decoder's `mxl_lsh_hash` call: one new token per sequence (T = 1), its shared qk the first d columns of a (B, 3d)
    bf16 qkv row.  B * H * n_h = 6144 bucket ids, so that the agreement threshold 0.999 leaves room for 6 flipped near-ties.
    -> dict(B, H, dh, n_h, factors, qkv (B, 3d) bf16, rot (H, dh, n_h, R2) f32)"""
    g = torch.Generator().manual_seed(seed + dh)
    B, H, n_h, factors = 128, 12, 4, [16]
    d = H * dh
    qkv = bf16_exact(torch.randn(B, 3 * d, generator=g))
    rot = torch.randn(H, dh, n_h, sum(factors) // 2, generator=g)
    return dict(B=B, H=H, dh=dh, n_h=n_h, factors=factors, qkv=qkv, rot=rot)


# ----------------------------------------------------------------------------------------------------------------------------
# Dropout masks as plain host code (from include/musicxl.h, MXL_GEMM_DROPOUT, and the comments at dropout_keep in csrc/common.h).
# Integer-exact: numpy uint32 arithmetic wraps modulo 2^32 like the device's.
# ----------------------------------------------------------------------------------------------------------------------------
_U32 = np.uint32


def mxl_hash32(x):
    """the lowbias32-style round of common.h on a uint32 array (or scalar)"""
    x = np.asarray(x).astype(_U32)
    with np.errstate(over='ignore'):
        x = x ^ (x >> _U32(16)); x = x * _U32(0x7feb352d)
        x = x ^ (x >> _U32(15)); x = x * _U32(0x846ca68b)
        x = x ^ (x >> _U32(16))
    return x


def dropout_thresh(p):
    """p * 2^32 as a uint32, saturated; the drop probability is taken as the float32 the C ABI passes"""
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    return int(min(p * 4294967296.0, 4294967295.0))


def _mix(seed, site):
    seed, site = int(seed) & 0xFFFFFFFFFFFFFFFF, int(site) & 0xFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    return (int(mxl_hash32(_U32(lo ^ ((site * 0x9E3779B9) & 0xFFFFFFFF)))) + hi) & 0xFFFFFFFF


def keep_hash(seed, site, idx):
    """the 32-bit random word of element `idx` (uint64 array): the low index word spread by 0x9E3779B1, the high one by 0x85EBCA77"""
    idx = np.asarray(idx).astype(np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(_U32)
    hi = (idx >> np.uint64(32)).astype(_U32)
    with np.errstate(over='ignore'):
        return mxl_hash32((lo * _U32(0x9E3779B1)) ^ (hi * _U32(0x85EBCA77)) ^ _U32(_mix(seed, site)))


def keep_mask(seed, site, idx, p):
    """dropout_keep: element `idx` (flat index, any value below 2^64) is KEPT iff its random word >= p * 2^32"""
    return keep_hash(seed, site, idx) >= _U32(dropout_thresh(p))


def keep_mask32(seed, site, idx, p):
    """dropout_keep32: the same decision for idx < 2^32, without the high-word term"""
    idx = np.asarray(idx)
    assert (idx.astype(np.uint64) < np.uint64(1 << 32)).all()
    with np.errstate(over='ignore'):
        h = mxl_hash32((idx.astype(_U32) * _U32(0x9E3779B1)) ^ _U32(_mix(seed, site)))
    return h >= _U32(dropout_thresh(p))


def pair_keep_mask(seed, site, M, N, p):
    """the RELU | DROPOUT mask of an (M, N) output: one random word per pair (m, n), (m, n + 1), n even -- the word of flat index
    m * N + n -- whose low 16 bits decide (m, n) and high 16 bits (m, n + 1), each kept iff >= (p * 2^32) >> 16"""
    m = np.arange(M, dtype=np.uint64)[:, None]
    n = np.arange(N, dtype=np.uint64)[None, :]
    h = keep_hash(seed, site, m * np.uint64(N) + (n & ~np.uint64(1)))
    half = np.where((n & np.uint64(1)) == 0, h & _U32(0xFFFF), h >> _U32(16))
    return half >= _U32(dropout_thresh(p) >> 16)


def chunk_drop_mask(seed, site, slots, p, n_keys=128, swap_parity=False):
    """the ChunkDrop rule of the chunked Reformer attention kernels (csrc/reformer.hip:377-403): keep decisions (len(slots), n_keys)
    of the cells (query slot s = (b * H + h) * S + qslot, key index kw in that slot's window).  One hash per 2 x 2 block of cells:
    the block row's key is the spread of blk = (s >> 1) * 64 PLUS the seed / site mix; block column kw >> 1 adds its multiple of
    0x9E3779B1 and gives two words (the hash, and a multiply-xorshift of it); the key's parity picks the word, the slot's parity the
    16-bit half (odd: the high one), kept iff >= (p * 2^32) >> 16.  `swap_parity`: the halves taken the other way round (a fault the
    CPU test plants)"""
    slots = np.asarray(slots).astype(np.uint64).reshape(-1)
    blk = (slots >> np.uint64(1)) * np.uint64(64)
    lo = (blk & np.uint64(0xFFFFFFFF)).astype(_U32)
    hi = (blk >> np.uint64(32)).astype(_U32)
    kw = np.arange(n_keys, dtype=_U32)
    with np.errstate(over='ignore'):
        key = ((lo * _U32(0x9E3779B1)) ^ (hi * _U32(0x85EBCA77))) + _U32(_mix(seed, site))
        w0 = mxl_hash32(key[:, None] + (kw >> _U32(1))[None, :] * _U32(0x9E3779B1))
        w1 = (w0 * _U32(0x85EBCA77)) ^ (w0 >> _U32(13))
    w = np.where((kw & _U32(1))[None, :] == 1, w1, w0)
    odd = ((slots & np.uint64(1)) == 1)[:, None] ^ bool(swap_parity)
    half = np.where(odd, w >> _U32(16), w & _U32(0xFFFF))
    return half >= _U32(dropout_thresh(p) >> 16)


def single_drop_mask(seed, site, B, H, T, p):
    """the single-chunk attention kernels' cells (csrc/reformer.hip:1212-1215): flat index ((b * H + h) * T + i) * 64 + j -> (B, H, T, T)"""
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    i = np.arange(T, dtype=np.uint64).reshape(1, 1, T, 1)
    j = np.arange(T, dtype=np.uint64).reshape(1, 1, 1, T)
    return keep_mask(seed, site, ((bh * np.uint64(T) + i) * np.uint64(64) + j), p)


def axial_pos_mask(seed, site, B, T, A1, p):
    """the axial embedding's 2-D position dropout (csrc/reformer.hip:31): one decision per (sequence, t % A1) -> (B, T)"""
    b = np.arange(B, dtype=np.uint64)[:, None]
    t = np.arange(T, dtype=np.uint64)[None, :]
    return keep_mask(seed, site, b * np.uint64(A1) + t % np.uint64(A1), p)


def axial_emb_mask(seed, site, B, T, d, p):
    """the axial embedding's word-vector dropout (csrc/reformer.hip:30): one decision per flat element -> (B, T, d)"""
    return keep_mask(seed, site, np.arange(B * T * d, dtype=np.uint64), p).reshape(B, T, d)


# ----------------------------------------------------------------------------------------------------------------------------
# GEMM references.  Flags as in include/musicxl.h.
# ----------------------------------------------------------------------------------------------------------------------------
F32, ATOMIC, BIAS, RELU, DROPOUT, RELU_BWD, ADD_AUX, SAVE_MASK, BWD_BITS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x100, 0x200


def _epilogue(acc, dt, alpha, bias, flags, aux, keep, p, c0):
    """the order epilogue_vals documents: alpha, bias, relu, dropout, relu-backward mask, + aux (, + c0: the atomic form)"""
    v = acc * torch.tensor(float(np.float32(alpha)), dtype=dt, device=acc.device)
    if flags & BIAS:
        v = v + bias.to(dt)
    if flags & RELU:
        v = v.clamp_min(0)
    if flags & DROPOUT and p > 0:
        scale = 1.0 / (1.0 - float(np.float32(p)))
        v = torch.where(keep, v * torch.tensor(scale, dtype=dt, device=acc.device), torch.zeros((), dtype=dt, device=acc.device))
    if flags & (RELU_BWD | BWD_BITS):
        v = torch.where(aux > 0, v, torch.zeros((), dtype=dt, device=acc.device))
    if flags & ADD_AUX:
        v = v + aux.to(dt)
    if c0 is not None:
        v = v + c0.to(dt)
    return v


def gemm_ref(A, B, *, trans_a=False, trans_b=False, alpha=1.0, bias=None, flags=0, aux=None, keep=None, p=0.0, c0=None):
    """float64 value of C = epilogue(alpha * op(A) op(B)).  A is (M, K), or (K, M) with trans_a; B is (N, K), or (K, N) with trans_b
    (the storage of mxl_gemm_bf16).  bias (N,), aux (M, N) [the activations of RELU_BWD, a boolean or 0/1 array for RELU_BWD_BITS, the
    residual of ADD_AUX], keep (M, N) bool with drop probability p, c0 (M, N) the prior contents of the atomic form"""
    a = (A.t() if trans_a else A).double()
    b = (B if trans_b else B.t()).double()
    return _epilogue(a @ b, torch.float64, alpha, bias, flags, aux, keep, p, c0)


def gemm_ref32(A, B, *, trans_a=False, trans_b=False, alpha=1.0, bias=None, flags=0, aux=None, keep=None, p=0.0, c0=None):
    """the same formula in float32 with ONE sequential accumulator over K (rank-1 updates; a product of two bf16 values is exact
    in float32, so each step is one rounding): the least favourable summation order, for the float32-vs-float64 gap"""
    a = (A.t() if trans_a else A).float().contiguous()
    b = (B if trans_b else B.t()).float().contiguous()
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32, device=a.device)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, k, :]
    return _epilogue(acc, torch.float32, alpha, bias, flags, aux, keep, p, c0)


def nt256_use192(M, N, n_cu=256):
    """the large-tile kernel's tile-width choice (csrc/gemm.hip): 192-wide tiles when they waste less of the chip"""
    tm = (M + 255) // 256
    t256, t192 = tm * ((N + 255) // 256), tm * ((N + 191) // 192)
    return -(-t192 // n_cu) * 192 < -(-t256 // n_cu) * 256


# ----------------------------------------------------------------------------------------------------------------------------
# The GEMM case table.  Arms of gemm_launch (csrc/gemm.hip) -> rows:
#   generic kernel gemm_bf16_kernel<AT, BT, BN>, the four layouts, BN = 128 ............. g_{nn,nt,tn,tt}_{edge,relu_bwd,atomic1,atomic3}
#   the same with BN = 64 (N <= 64) ..................................................... g_*_k8_bias_f32, g_*_n40_atomic3
#   SWAP arm (TT + atomic, no other flag), BN = 128 / BN = 64 ........................... g_tt_atomic1, g_tt_atomic3 / g_tt_n40_atomic3
#   generic kernel with the dropout / residual epilogues (M < 256) ...................... g_nn_{drop,bias_drop,bias_relu_drop,bias_aux_drop,aux}
#   large-tile kernel, compile-time epilogue arms (one row per shape class _i _r _e _o):
#     0 | BIAS | BIAS|OUT_F32 | BIAS|RELU | BIAS|RELU|DROPOUT | RELU_BWD | ADD_AUX | ADD_AUX|DROPOUT | BIAS|ADD_AUX |
#     BIAS|ADD_AUX|DROPOUT ............................................................. nt_{plain,bias,bias_f32,bias_relu,bias_relu_drop,
#                                                                                             relu_bwd,aux,aux_drop,bias_aux,bias_aux_drop}_*
#   large-tile kernel, run-time arm (-1): alpha != 1 with BIAS; flag sets not in the list  nt_rt_alpha_bias_*, nt_rt_{drop,bias_drop,f32}_*
#   K = 64 (one step pair per tile) / K = 3072 .......................................... every nt_*_{i,r,e,o} row / nt_bias_k3072, w4_plain_k3072
#   several tiles per workgroup under mxl_set_reserved_cus .............................. nt_bias_relu_drop_reserve
#   four-wave kernel: plain, BIAS (head-dot: test_headdot_against_float64) .............. w4_plain, w4_bias, w4_plain_k3072
#   RELU_BWD | colsum, RELU_BWD_BITS [| colsum], SAVE_RELU_MASK [with DROPOUT] .......... COLSUM_CASES, MASK_BITS_CASES (their own tests)
#   gemm_tt256_kernel: slices exact / with a remainder / slice count set by reserved CUs   tt_exact, tt_k8224, tt_reserve
#   mxl_gemm_bf16_batched .............................................................. BATCHED_CASES;  skinny forms: SKINNY_CASES
# Shape classes of the large-tile rows: _i interior (M, N multiples of 256; MXL_GEMM_W4=0 keeps plain / BIAS on the eight-wave
# kernel), _r M = 256 k + 1, _e (513, 522): 192-wide tiles with a ragged last tile and N % 4 == 2, _o interior with an odd ldc and
# C one element off 16-byte alignment (falls off the four-wave kernel and the paired stores).
# `expect` = mxl_gemm_last_nt_kernel() after the call on a 256-CU device (0 generic / TT, 1 / 2 eight waves 256- / 192-wide, 3 four waves).
# ----------------------------------------------------------------------------------------------------------------------------
def _row(name, fam, M, N, K, lay='nn', flags=0, alpha=1.0, p=0.0, ksplits=1, lda_pad=0, ldb_pad=0, ldc_pad=8, c_off=0, ldaux_pad=0,
         w4=None, reserve=0, expect=0):
    return dict(name=name, fam=fam, M=M, N=N, K=K, ta=lay[0] == 't', tb=lay[1] == 't', flags=flags, alpha=alpha, p=p, ksplits=ksplits,
                lda_pad=lda_pad, ldb_pad=ldb_pad, ldc_pad=ldc_pad, c_off=c_off, ldaux_pad=ldaux_pad, w4=w4, reserve=reserve,
                expect=expect)


def _gemm_cases():
    rows = []
    for lay in ('nn', 'nt', 'tn', 'tt'):
        # K of 8 would break "K % 8 == 0 unless both operands are transposed" nowhere; the TT rows take an odd K instead
        rows += [
            _row(f'g_{lay}_edge', 'generic', 129, 127, 75 if lay == 'tt' else 72, lay, lda_pad=8, ldb_pad=16, ldc_pad=3),
            _row(f'g_{lay}_k8_bias_f32', 'generic', 127, 63, 8, lay, flags=BIAS | F32, ldc_pad=1),
            _row(f'g_{lay}_relu_bwd', 'generic', 200, 130, 192, lay, flags=RELU_BWD, alpha=1.25, ldaux_pad=1, ldc_pad=2),
            _row(f'g_{lay}_atomic1', 'generic', 127, 129, 136, lay, flags=ATOMIC, alpha=0.5, ksplits=1, ldc_pad=5),
            _row(f'g_{lay}_atomic3', 'generic', 200, 130, 520, lay, flags=ATOMIC, alpha=0.5, ksplits=3, lda_pad=8, ldc_pad=5),
            _row(f'g_{lay}_n40_atomic3', 'generic', 136, 40, 200, lay, flags=ATOMIC, alpha=-2.0, ksplits=3, ldc_pad=1),
        ]
    rows += [
        _row('g_nn_drop', 'generic', 130, 264, 128, flags=DROPOUT, p=0.25, ldc_pad=8),
        _row('g_nn_bias_drop', 'generic', 129, 65, 64, flags=BIAS | DROPOUT, p=0.1, ldc_pad=1),
        _row('g_nn_bias_relu_drop', 'generic', 130, 262, 128, flags=BIAS | RELU | DROPOUT, p=0.25, ldc_pad=2),
        _row('g_nn_bias_aux_drop', 'generic', 129, 65, 64, flags=BIAS | ADD_AUX | DROPOUT, p=0.1, ldaux_pad=2, ldc_pad=1),
        _row('g_nn_aux', 'generic', 255, 191, 64, flags=ADD_AUX, ldaux_pad=3, ldc_pad=1),
        _row('g_nt_bias_relu', 'generic', 64, 72, 1032, 'nt', flags=BIAS | RELU, ldc_pad=0),
    ]
    arms = [('plain', 0, 1.0, 0.0), ('bias', BIAS, 1.0, 0.0), ('bias_f32', BIAS | F32, 1.0, 0.0), ('bias_relu', BIAS | RELU, 1.0, 0.0),
            ('bias_relu_drop', BIAS | RELU | DROPOUT, 1.0, 0.1), ('relu_bwd', RELU_BWD, 1.25, 0.0), ('aux', ADD_AUX, 1.0, 0.0),
            ('aux_drop', ADD_AUX | DROPOUT, 1.0, 0.1), ('bias_aux', BIAS | ADD_AUX, 1.0, 0.0),
            ('bias_aux_drop', BIAS | ADD_AUX | DROPOUT, 1.0, 0.1), ('rt_alpha_bias', BIAS, 0.5, 0.0), ('rt_drop', DROPOUT, 1.0, 0.25),
            ('rt_bias_drop', BIAS | DROPOUT, 0.75, 0.25), ('rt_f32', F32, 1.0, 0.0)]
    for nm, fl, al, p in arms:
        rows += [
            _row(f'nt_{nm}_i', 'nt', 16384, 1024, 64, flags=fl, alpha=al, p=p, w4='0', expect=1),
            _row(f'nt_{nm}_r', 'nt', 16129, 1024, 64, flags=fl, alpha=al, p=p, expect=1),
            _row(f'nt_{nm}_e', 'nt', 513, 522, 64, flags=fl, alpha=al, p=p, ldc_pad=6, ldaux_pad=1, expect=2),
            _row(f'nt_{nm}_o', 'nt', 16384, 1024, 64, flags=fl, alpha=al, p=p, ldc_pad=1, c_off=1, expect=1),
        ]
    rows += [
        _row('nt_bias_k3072', 'nt_k3072', 16384, 1024, 3072, flags=BIAS, w4='0', expect=1),
        _row('nt_bias_relu_drop_reserve', 'nt', 16384, 1024, 192, flags=BIAS | RELU | DROPOUT, p=0.1, reserve=128, expect=1),
        _row('w4_plain', 'nt', 16384, 1024, 64, expect=3),
        _row('w4_bias', 'nt', 16384, 1024, 128, flags=BIAS, expect=3),
        _row('w4_plain_k3072', 'nt_k3072', 16384, 1024, 3072, expect=3),
        _row('tt_exact', 'tt256', 512, 256, 8192, 'tt', flags=ATOMIC, alpha=0.5, ldc_pad=8),
        _row('tt_k8224', 'tt256', 256, 256, 8224, 'tt', flags=ATOMIC, alpha=0.5, ldc_pad=8),
        _row('tt_reserve', 'tt256', 1536, 1024, 16384, 'tt', flags=ATOMIC, alpha=0.5, ldc_pad=8, reserve=128),
    ]
    return rows


GEMM_CASES = _gemm_cases()

# mxl_gemm_bf16_colsum with the sums fused into the large-tile epilogue (M, N multiples of 256, 256-wide tiles): (name, M, N, K)
COLSUM_CASES = [('colsum_relu_bwd', 16384, 1024, 64)]
# SAVE_RELU_MASK -> RELU_BWD_BITS (without and with the fused column sums): (name, M, N, K, p)
MASK_BITS_CASES = [('bits_drop', 16384, 1024, 64, 0.1), ('bits_plain', 16384, 1024, 64, 0.0)]
# mxl_gemm_bf16_batched: operand element offsets (by / bdiv) * s1 + (by % bdiv) * s2.  Sizes are those of the two callers in ops.py
# (decode: per-head q . rd^T into a (B, H * M) f32 buffer; dRd fallback: per (sequence, head) dg^T . qr accumulated over sequences)
# and one bf16 form whose six strides are all different.
BATCHED_CASES = [
    dict(name='bat_decode_nn_f32', M=5, N=40, K=32, lda=96, ldb=96, ldc=120, ta=False, tb=False, flags=F32, alpha=1.0, ksplits=1,
         batch=3, bdiv=1, sA=(32, 0), sB=(32, 0), sC=(40, 0)),
    dict(name='bat_drd_tt_atomic', M=24, N=16, K=40, lda=24, ldb=48, ldc=48, ta=True, tb=True, flags=ATOMIC, alpha=1.0, ksplits=1,
         batch=6, bdiv=3, sA=(3 * 40 * 24, 40 * 24), sB=(40 * 48, 16), sC=(0, 16)),
    dict(name='bat_drd_tt_atomic_k2', M=24, N=16, K=200, lda=24, ldb=48, ldc=48, ta=True, tb=True, flags=ATOMIC, alpha=0.5, ksplits=2,
         batch=6, bdiv=3, sA=(3 * 200 * 24, 200 * 24), sB=(200 * 48, 16), sC=(0, 16)),
    dict(name='bat_nn_bf16_bdiv2', M=70, N=130, K=72, lda=80, ldb=72, ldc=133, ta=False, tb=False, flags=0, alpha=1.0, ksplits=1,
         batch=6, bdiv=2, sA=(2 * 70 * 80 + 16, 70 * 80 + 8), sB=(2 * 130 * 72 + 24, 130 * 72), sC=(2 * 70 * 133 + 7, 70 * 133 + 3)),
]
# skinny forms: (M, N, K); N = 48 is on the kernel's 16-column granularity, 50 and 1190 are off it
SKINNY_CASES = [(M, N, K) for M in (1, 3, 64) for (N, K) in ((48, 136), (50, 768), (1190, 64))]


def case_inputs(c):
    """the bf16-exact inputs of a GEMM_CASES row, on the CPU: A (M, K), B (N, K) logical operands, bias (N,) f32, aux (M, N) bf16
    (relu-like, half zeros, for RELU_BWD; a residual otherwise), c0 (M, N) f32 prior contents of the atomic form, seed / site"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    M, N, K = c['M'], c['N'], c['K']
    A = bf16_exact(torch.randn(M, K, generator=g) * 0.5)
    B = bf16_exact(torch.randn(N, K, generator=g) * 0.5)
    bias = torch.randn(N, generator=g)
    aux = None
    if c['flags'] & (RELU_BWD | ADD_AUX):
        aux = torch.randn(M, N, generator=g)
        aux = bf16_exact(aux.clamp_min(0) if c['flags'] & RELU_BWD else aux)
    c0 = torch.randn(M, N, generator=g) if c['flags'] & ATOMIC else None
    seed = (zlib.crc32(c['name'].encode()) << 13) ^ 0x5DEECE66D
    return dict(A=A, B=B, bias=bias, aux=aux, c0=c0, seed=seed, site=len(c['name']))


def case_keep(c, seed, site):
    """the keep mask a GEMM_CASES row expects (None without dropout)"""
    if not (c['flags'] & DROPOUT) or c['p'] <= 0:
        return None
    M, N = c['M'], c['N']
    if c['flags'] & RELU:
        return torch.from_numpy(pair_keep_mask(seed, site, M, N, c['p']))
    return torch.from_numpy(keep_mask(seed, site, np.arange(M * N, dtype=np.uint64), c['p']).reshape(M, N))


def sub_block(M, N, rows=24, cols=64):
    """row / column indices of the block the float32 gap is measured on: the first and last `rows` rows and `cols` columns"""
    ri = torch.unique(torch.cat([torch.arange(min(rows, M)), torch.arange(max(0, M - rows), M)]))
    ci = torch.unique(torch.cat([torch.arange(min(cols, N)), torch.arange(max(0, N - cols), N)]))
    return ri, ci


def case_gap(c, x, keep):
    """float32-vs-float64 gap of a GEMM_CASES row on its sub-block (CPU)"""
    ri, ci = sub_block(c['M'], c['N'])
    def cut(t):
        return None if t is None else t[ri][:, ci]
    kw = dict(alpha=c['alpha'], bias=x['bias'][ci], flags=c['flags'], aux=cut(x['aux']), keep=cut(keep), p=c['p'], c0=cut(x['c0']))
    return gap(gemm_ref32(x['A'][ri], x['B'][ci], **kw), gemm_ref(x['A'][ri], x['B'][ci], **kw))


def batched_inputs(c):
    """flat bf16-exact operand buffers of a BATCHED_CASES row and, for the atomic form, the prior contents of the flat C"""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    b1, b2 = (c['batch'] - 1) // c['bdiv'], min(c['bdiv'], c['batch']) - 1
    ra, rb = (c['K'] if c['ta'] else c['M']), (c['K'] if c['tb'] else c['N'])
    nA = b1 * c['sA'][0] + b2 * c['sA'][1] + ra * c['lda']
    nB = b1 * c['sB'][0] + b2 * c['sB'][1] + rb * c['ldb']
    nC = b1 * c['sC'][0] + b2 * c['sC'][1] + c['M'] * c['ldc']
    return dict(A=bf16_exact(torch.randn(nA, generator=g) * 0.5), B=bf16_exact(torch.randn(nB, generator=g) * 0.5),
                c0=torch.randn(nC, generator=g), nC=nC)


def batched_ref(c, x, ref=gemm_ref):
    """-> (flat float64 C, flat bool `written`): a loop of single GEMMs, item `by` at element offsets (by // bdiv) * s1 + (by % bdiv) * s2
    of A, B and C (include/musicxl.h); the atomic form adds to c0, the others store"""
    M, N, K = c['M'], c['N'], c['K']
    atomic = bool(c['flags'] & ATOMIC)
    out = x['c0'].double().clone() if atomic else torch.zeros(x['nC'], dtype=torch.float64)
    written = torch.zeros(x['nC'], dtype=torch.bool)
    for by in range(c['batch']):
        q, r = by // c['bdiv'], by % c['bdiv']
        oa, ob, oc = (q * c[k][0] + r * c[k][1] for k in ('sA', 'sB', 'sC'))
        a = x['A'].as_strided((K, M) if c['ta'] else (M, K), (c['lda'], 1), oa)
        b = x['B'].as_strided((K, N) if c['tb'] else (N, K), (c['ldb'], 1), ob)
        v = ref(a, b, trans_a=c['ta'], trans_b=c['tb'], alpha=c['alpha']).double()
        cv = out.as_strided((M, N), (c['ldc'], 1), oc)
        if atomic:
            cv += v
        else:
            cv.copy_(v)
        written.as_strided((M, N), (c['ldc'], 1), oc).fill_(True)
    return out, written


def skinny_inputs(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    return (bf16_exact(torch.randn(M, K, generator=g) * 0.5), bf16_exact(torch.randn(N, K, generator=g) * 0.5),
            torch.randn(N, generator=g))
