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
