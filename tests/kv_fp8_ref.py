"""Host restatement of the FP8 K/V ring format (test infrastructure, NOT product code), with torch on the CPU.

A ring (B, H, M, dh) of bf16 is held as (B, H, M, dh) uint8 of OCP e4m3fn bytes and (B, H, M) int8 exponents, one per slot and head;
the stored value is fp8 * 2^e.  For a row x of dh bf16 elements with amax = max|x| = m 2^k, m in [0.5, 1) (frexp):

    e = k - 9 if m <= 0.875 else k - 8      (the smallest e with amax 2^-e <= 448), clamped to [-126, 127]
    amax = 0: e = 0 and zero bytes
    byte j = e4m3fn(x_j 2^-e), round to nearest even, subnormals kept (torch's .to(torch.float8_e4m3fn))

The scale is a power of two: x 2^-e is exact in float64 (and in float32 wherever the kernel computes it), and every dequantised value
is a bf16 value.
"""
import functools

import torch

E_MIN, E_MAX = -126, 127
FP8_MAX = 448.0


def row_exponent(amax: torch.Tensor) -> torch.Tensor:
    """amax (...) >= 0, float -> e (...) int8"""
    m, k = torch.frexp(amax.double())
    e = torch.where(m <= 0.875, k - 9, k - 8).clamp(E_MIN, E_MAX)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int8)


def quantise(x: torch.Tensor):
    """x (..., dh) of bf16 values (any float dtype) -> (bytes (..., dh) uint8, e (...) int8)"""
    x = x.double()
    e = row_exponent(x.abs().amax(-1))
    scaled = torch.ldexp(x, -e.to(torch.int32).unsqueeze(-1))            # exact: a power of two in float64
    return scaled.float().to(torch.float8_e4m3fn).view(torch.uint8), e    # (|scaled| <= 448: float32 holds it exactly)


def dequantise(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """(bytes (..., dh) uint8, e (...) int8) -> the stored values, float32 (each one a bf16 value)"""
    return torch.ldexp(q.view(torch.float8_e4m3fn).float().double(), e.to(torch.int32).unsqueeze(-1)).float()


def roundtrip(x: torch.Tensor) -> torch.Tensor:
    """dequantise(quantise(x)) in x's dtype"""
    return dequantise(*quantise(x)).to(x.dtype)


def ring_expect_fp8(qkv: torch.Tensor, ring0, third: int, t: int):
    """ring_expect of oracle/decode_cases.py on fp8 rings: ring0 = (bytes (B, H, M, dh) uint8, e (B, H, M) int8); slot t mod M of both
    <- the quantised third (1 = k, 2 = v) of the (B, 3d) qkv rows, every other slot as it was"""
    q0, e0 = ring0
    B, H, M, dh = q0.shape
    d = H * dh
    q, e = quantise(qkv[:, third * d:(third + 1) * d].reshape(B, H, dh))
    qo, eo = q0.clone(), e0.clone()
    qo[:, :, t % M] = q
    eo[:, :, t % M] = e
    return qo, eo


def fill_expect_fp8(qkv: torch.Tensor, ring0, third: int):
    """mxl_kv_fill_fp8: the last min(T, M) positions p of a (B, T, 3d) qkv buffer in slot p mod M, every other slot as it was"""
    q0, e0 = ring0
    B, H, M, dh = q0.shape
    d = H * dh
    T = qkv.shape[1]
    qo, eo = q0.clone(), e0.clone()
    for p in range(max(0, T - M), T):
        q, e = quantise(qkv[:, p, third * d:(third + 1) * d].reshape(B, H, dh))
        qo[:, :, p % M] = q
        eo[:, :, p % M] = e
    return qo, eo


def special_rows(dh: int) -> torch.Tensor:
    """(5, dh) bf16 rows the writers' tests plant: a zero row, amax with m = 0.875 exactly (e = k - 9) and the next bf16 up
    (e = k - 8), a bf16-subnormal row (e clamped to -126), and a row whose small elements land on e4m3fn subnormals"""
    g = torch.Generator().manual_seed(dh)
    small = (torch.rand(5, dh, generator=g) - 0.5).to(torch.bfloat16)
    rows = torch.zeros(5, dh, dtype=torch.bfloat16)
    rows[1] = small[1]
    rows[1, 3] = 1.75                                                   # 0.875 * 2^1
    rows[2] = small[2]
    rows[2, dh - 1] = -(torch.tensor(1.75, dtype=torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16)
    rows[3] = (torch.randint(1, 128, (dh,), generator=g).to(torch.int16)).view(torch.bfloat16)         # subnormal bit patterns
    rows[3, 1] = -rows[3, 1]
    rows[4] = (small[4].float() * 2.0 ** -12).to(torch.bfloat16)
    rows[4, 0] = 1.0
    return rows


@functools.lru_cache(maxsize=8)
def fp8_attn_case(name: str, family: str, pieces: int = 1) -> dict:
    """oracle/decode_cases.attn_case with its rings quantised: kc / vc are the dequantised values (what the float64 reference and
    the rounded model read), kq / ke / vq / ve the bytes and exponents the kernel reads"""
    from oracle import decode_cases as D
    c = dict(D.attn_case(name, family, pieces))
    c['kq'], c['ke'] = quantise(c['kc'])
    c['vq'], c['ve'] = quantise(c['vc'])
    c['kc'], c['vc'] = dequantise(c['kq'], c['ke']), dequantise(c['vq'], c['ve'])
    return c
