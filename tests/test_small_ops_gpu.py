"""Kernel-level tests of the small index-arithmetic kernels that only whole-model runs reached: mxl_mem_update, mxl_kv_fill,
mxl_add_rowbias_bf16, mxl_center_columns_bf16, mxl_label_guard, mxl_cast_f32_bf16, mxl_cast_bf16_f32.  Copies and casts are bit-exact;
the one float reduction (column centring) is held against float64 by the rule of oracle/kernel_cases.py.
"""
import numpy as np
import pytest
import torch

from oracle.kernel_cases import A_BF16, bf16_exact, check_gap, gap, worst

pytestmark = pytest.mark.gpu

B_CENTER = 4.5e-7     # center_columns: sequential float32 column sums, gap 1.1e-7 of max|ref| (M = 4097)


def bits(x):
    return x.contiguous().view(torch.int16)


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('M,T', [(64, 16), (64, 64), (64, 100), (8, 1)])
def test_mem_update_exact(dev, B, M, T):
    """mxl_mem_update == cat(mem, hid)[:, -M:] bit for bit, for T < M, T == M and T > M"""
    from symbolic_music_generation_amd import ops
    g = torch.Generator().manual_seed(M + T)
    d = 24
    mem, hid = bf16_exact(torch.randn(B, M, d, generator=g)), bf16_exact(torch.randn(B, T, d, generator=g))
    frame = torch.full((B * M + 2, d), float('nan'), dtype=torch.bfloat16, device=dev)
    ops.mem_update(mem.to(dev), hid.to(dev), frame[1:B * M + 1])
    torch.cuda.synchronize()
    out = frame.cpu()
    assert torch.equal(bits(out[1:B * M + 1]).view(B, M, d), bits(torch.cat([mem, hid], 1)[:, -M:]).view(B, M, d))
    assert torch.isnan(out[0].float()).all() and torch.isnan(out[B * M + 1].float()).all()


@pytest.mark.parametrize('dh', [8, 32])
@pytest.mark.parametrize('T,M', [(5, 16), (16, 16), (20, 16), (35, 16), (1, 16), (17, 1)])
def test_kv_fill_exact(dev, T, M, dh):
    """mxl_kv_fill: head-major rings (B, H, M, dh), position p of the last min(T, M) in slot p % M, bit for bit; slots that
    no position maps to keep their sentinel.  T < M, T == M, T > M, T = 2M + 3"""
    from symbolic_music_generation_amd import ops
    g = torch.Generator().manual_seed(T * 3 + M + dh)
    B, H = 3, 2
    d = H * dh
    qkv = bf16_exact(torch.randn(B, T, 3 * d, generator=g))
    kc = torch.full((B, H, M, dh), float('nan'), dtype=torch.bfloat16, device=dev)
    vc = torch.full_like(kc, float('nan'))
    wk, wv = kc.cpu().clone(), vc.cpu().clone()
    for p in range(max(0, T - M), T):
        wk[:, :, p % M] = qkv[:, p, d:2 * d].view(B, H, dh)
        wv[:, :, p % M] = qkv[:, p, 2 * d:].view(B, H, dh)
    ops.kv_fill(qkv.to(dev), kc, vc, T)
    torch.cuda.synchronize()
    assert torch.equal(bits(kc.cpu()), bits(wk)) and torch.equal(bits(vc.cpu()), bits(wv))


@pytest.mark.parametrize('B,T,n', [(2, 33, 64), (1, 1, 8), (3, 700, 768)])
def test_add_rowbias_strided(dev, B, T, n):
    """mxl_add_rowbias_bf16 on the q columns of a (B, T, 3n) buffer (row stride 3n, batch stride T * 3n as a long long):
    equal to bf16(x.double() + bias) bit for bit -- the float32 sum of a bf16 and a float32 value of similar size is exact in
    float64 and rounds the same way"""
    from symbolic_music_generation_amd import ops
    g = torch.Generator().manual_seed(B + T + n)
    qkv = bf16_exact(torch.randn(B, T, 3 * n, generator=g))
    bias = torch.randn(n, generator=g)
    frame = torch.full((B * T + 2, n), float('nan'), dtype=torch.bfloat16, device=dev)
    ops.add_rowbias(qkv.to(dev), T * 3 * n, 3 * n, bias.to(dev), frame[1:B * T + 1], B, T, n)
    torch.cuda.synchronize()
    out = frame.cpu()
    want = (qkv[:, :, :n].double() + bias.double()).float().to(torch.bfloat16).view(B * T, n)
    assert torch.equal(bits(out[1:B * T + 1]), bits(want))
    assert torch.isnan(out[0].float()).all() and torch.isnan(out[B * T + 1].float()).all()


def _center_case(M, N):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, N, generator=g)
    x[:, ::2] = 100 + 0.1 * x[:, ::2]            # every other column: mean 100, spread 0.1 (bf16 keeps steps of 0.5 there)
    x = bf16_exact(x)
    x64 = x.double()
    ref = x64 - x64.mean(0, keepdim=True)
    seq_mean = torch.from_numpy(np.cumsum(x.float().numpy(), axis=0, dtype=np.float32)[-1]) / M     # numpy: a sequential float32 sum
    return x, ref, x.float() - seq_mean


@pytest.mark.parametrize('N', [8, 768])
@pytest.mark.parametrize('M', [1, 255, 256, 257, 4097])
def test_center_columns(dev, M, N):
    """mxl_center_columns_bf16 against the float64 centring of the bf16 input, with columns of mean 100 and spread 0.1, where a
    sum that loses the low bits shows.  CPU gap of a sequential float32 column sum: 1.1e-7 of max|ref| (bf16 values near 100 are
    multiples of 0.5, their float32 sums are exact) -> bound 2^-8 |ref| + 4.5e-7 max|ref|; the column means of the result are zero to the same bound (each element carries at most one
    bf16 rounding of itself)."""
    from symbolic_music_generation_amd import ops
    x, ref, r32 = _center_case(M, N)
    frame = torch.full((M + 2, N), float('nan'), dtype=torch.bfloat16, device=dev)
    ops.center_columns(x.to(dev), frame[1:M + 1])
    torch.cuda.synchronize()
    out = frame.float().cpu()
    assert torch.isnan(out[0]).all() and torch.isnan(out[M + 1]).all()
    got = out[1:M + 1]
    if M == 1:
        assert (got == 0).all()
        return
    gp = gap(r32, ref)
    check_gap(gp, B_CENTER)
    ratio, err = worst(got, ref, A_BF16, B_CENTER)
    print(f'center_columns M{M} N{N}: cpu sequential-sum gap {gp:.2e} device err {err:.2e} worst/bound {ratio:.3f}')
    assert ratio <= 1.0, (ratio, err)
    scale = ref.abs().max().item()
    assert got.double().mean(0).abs().max().item() <= (A_BF16 + B_CENTER) * scale


@pytest.mark.parametrize('T', [2, 257, 1025])
@pytest.mark.parametrize('case', ['none_valid', 'valid_last', 'valid_only_at_0', 'valid_mid'])
def test_label_guard(dev, T, case):
    """mxl_label_guard (transformer_xl.py:176-182): when every label of row 0 from position 1 on is -100, labels[0, 1] = eos;
    position 0 does not count; nothing else changes"""
    from symbolic_music_generation_amd import ops
    eos = 3
    lab = torch.full((2, T), -100, dtype=torch.int64)
    lab[1, 0] = 11
    if case == 'valid_last':
        lab[0, T - 1] = 42
    elif case == 'valid_only_at_0':
        lab[0, 0] = 42
    elif case == 'valid_mid':
        lab[0, max(1, T // 2)] = 0
    want = lab.clone()
    if case in ('none_valid', 'valid_only_at_0'):
        want[0, 1] = eos
    ld = lab.to(dev)
    ops.label_guard(ld, eos)
    torch.cuda.synchronize()
    assert torch.equal(ld.cpu(), want)


def test_casts_exact(dev):
    """mxl_cast_bf16_f32 over all 65536 bf16 bit patterns and mxl_cast_f32_bf16 over random float32 bit patterns (subnormals,
    +-inf and NaN among them) plus hand-picked round-to-nearest-even ties: bit-exact with Tensor.to, NaN stays NaN; lengths that
    are no multiple of any vector width; nothing written past n"""
    from symbolic_music_generation_amd import ops
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    n = allb.numel() - 5
    y = torch.full((n + 3,), -777.0, device=dev)
    ops.cast_f32(allb[:n].to(dev), y[:n])
    torch.cuda.synchronize()
    assert torch.equal(y[:n].cpu().view(torch.int32), allb[:n].float().view(torch.int32)) and (y[n:] == -777.0).all()
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-2 ** 31, 2 ** 31, (100003,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).clone()
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20,
                         float('inf'), float('-inf'), float('nan'), 0.0, -0.0, 1e-40, -1e-40, 2.0 ** -133, 3.3895e38, 3.4e38])
    x[:ties.numel()] = ties
    want = x.to(torch.bfloat16)
    assert want[0] == 1.0 and want[1] == 1 + 2.0 ** -6 and want[3] == 1 + 2.0 ** -7 and want[4] == 1.0   # ties go to even
    n = x.numel()
    z = torch.full((n + 3,), -777.0, dtype=torch.bfloat16, device=dev)
    ops.cast_bf16(x.to(dev), z[:n])
    torch.cuda.synchronize()
    z = z.cpu()
    nan = torch.isnan(x)
    assert nan.sum() > 100 and torch.isnan(z[:n][nan].float()).all()
    assert torch.equal(bits(z[:n][~nan]), bits(want[~nan])) and (z[n:] == -777.0).all()
