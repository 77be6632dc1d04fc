"""Kernel-level tests of the pieces under the large-vocabulary head (csrc/head_large.hip).  tests/test_large_vocab_gpu.py judges
them through a whole layer (loss to 2e-3, gradient norms to 6 %); each piece is simple enough to be held to rounding error
against a float64 reference, or bit for bit where it only copies.  Tolerance rule and helpers: oracle/kernel_cases.py.
"""
import numpy as np
import pytest
import torch

from oracle.kernel_cases import A_BF16, A_F32, bf16_exact, check_gap, gap, worst

pytestmark = pytest.mark.gpu

# CPU float32-vs-float64 gaps (largest over the cases of each test) and the absolute terms 4 x gap they give:
B_LSE = 2.0e-7      # rows_lse_pick: torch.logsumexp in float32, gap 4.6e-8 of max|lse|
B_SUM = 3.7e-6      # bucket_nll_finish: sequential float32 sum of the token losses on top of the start value, gap 9.1e-7
B_GRAD = 2.5e-7     # rows_softmax_grad: float32 evaluation, gap 6.2e-8 of max|grad|


def bits(x):
    return x.contiguous().view(torch.int16)


@pytest.mark.parametrize('d,n', [(8, 1), (512, 3), (520, 4), (768, 5), (1024, 4099), (520, 4099), (8, 4099), (768, 1), (1024, 4)])
def test_gather_and_scatter_add_rows_exact(dev, d, n):
    """mxl_gather_rows_bf16 copies bit for bit; mxl_scatter_add_rows_bf16 gives bf16(float(dst) + float(src)) bit for bit on the
    touched rows and leaves every other row and the columns d .. ld alone.  d = 520: one 16-byte piece beyond the 512-column
    stride of a wave; n = 4099: a last workgroup with rows to spare; source / destination rows wider than d; idx without repeats"""
    from symbolic_music_generation_amd import ops
    g = torch.Generator().manual_seed(d + n)
    R, ld = n + 13, d + 8
    idx = torch.randperm(R, generator=g)[:n].to(torch.int32)
    wide = bf16_exact(torch.randn(R, ld, generator=g))
    frame = torch.full((n + 2, d), float('nan'), dtype=torch.bfloat16, device=dev)
    ops.gather_rows(wide.to(dev)[:, :d], idx.to(dev), frame[1:n + 1], n)
    torch.cuda.synchronize()
    out = frame.cpu()
    assert torch.equal(bits(out[1:n + 1]), bits(wide[idx.long(), :d]))
    assert torch.isnan(out[0].float()).all() and torch.isnan(out[n + 1].float()).all()
    src = bf16_exact(torch.randn(n, d, generator=g))
    src[0, 0] = 0.0
    dst = wide.to(dev)
    ops.scatter_add_rows(src.to(dev), idx.to(dev), dst[:, :d], n)
    torch.cuda.synchronize()
    want = wide.clone()
    want[idx.long(), :d] = (wide[idx.long(), :d].float() + src.float()).to(torch.bfloat16)
    assert torch.equal(bits(dst.cpu()), bits(want))


def _logit_rows(n_rows, ncols, ld, off, g):
    """(n_rows, ld) float32 rows inside a flat buffer, starting `off` floats into it (off = 1: base not 16-byte aligned);
    columns ncols .. ld hold 1e30, so a kernel that reads them cannot pass.  Row 0: maximum in the last column; row 1: maximum
    in the first column; row 2: -1e4 next to the maximum and in the first and last column"""
    flat = torch.full((n_rows * ld + 8,), 1e30)
    x = torch.randn(n_rows, ncols, generator=g) * 3
    x[0, ncols - 1] = 14.0
    x[1, 0] = 15.0
    if ncols >= 3:
        m = int(x[2].argmax())
        x[2, [0, ncols - 1]] = -1e4
        x[2, m] = 9.0
        x[2, m + 1 if m + 1 < ncols else m - 1] = -1e4
    rows = flat[off:off + n_rows * ld].view(n_rows, ld)
    rows[:, :ncols] = x
    return flat, x


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('ld_pad', [0, 1, 3, 6])
@pytest.mark.parametrize('ncols', [1, 3, 4, 5, 255, 256, 257, 10000, 62144])
def test_rows_lse_pick(dev, ncols, ld_pad, off):
    """mxl_rows_lse_pick against float64 logsumexp; the picked logit bit for bit.  ld = ncols + pad covers ld % 4 == 0 and != 0,
    `off` an unaligned base (scalar path) and an aligned one, ncols % 4 the scalar tail after the vector loop.  Both addressing
    forms: rows_idx (results land at lse_out[rows_idx[j]], other entries keep their sentinel) and row0 > 0.  Targets -1 (pick 0),
    0, ncols - 1.  CPU float32 gap 4.6e-8 of max|lse| -> bound 2^-24 |ref| + 2e-7 max|ref|."""
    from symbolic_music_generation_amd import ops
    g = torch.Generator().manual_seed(ncols * 8 + ld_pad)
    n_rows, ld, n_tok = 7, ncols + ld_pad, 16
    flat, x = _logit_rows(n_rows, ncols, ld, off, g)
    ref = torch.logsumexp(x.double(), -1)
    gp = gap(torch.logsumexp(x, -1), ref)
    check_gap(gp, B_LSE)
    fd = flat.to(dev)
    logits = fd[off:off + n_rows * ld].view(n_rows, ld)
    assert (logits.data_ptr() % 16 == 0) == (off == 0)
    for rows_idx, row0 in ((torch.randperm(n_tok, generator=g)[:n_rows], 0), (None, 5)):
        toks = rows_idx if rows_idx is not None else torch.arange(row0, row0 + n_rows)
        tgt = torch.full((n_tok,), -1, dtype=torch.int32)
        tj = torch.tensor([-1, 0, ncols - 1, int(torch.randint(0, ncols, (1,), generator=g)), ncols - 1, 0, ncols // 2])
        tgt[toks] = tj.to(torch.int32)
        lse = torch.full((n_tok,), -777.0, device=dev)
        pick = torch.full((n_tok,), -777.0, device=dev)
        ops.rows_lse_pick(logits, ncols, n_rows, tgt.to(dev), lse, pick,
                          rows_idx=None if rows_idx is None else rows_idx.to(torch.int32).to(dev), row0=row0)
        torch.cuda.synchronize()
        lse, pick = lse.cpu(), pick.cpu()
        ratio, err = worst(lse[toks], ref, A_F32, B_LSE)
        print(f'rows_lse_pick ncols{ncols} ld{ld} off{off} idx{rows_idx is not None}: cpu gap {gp:.2e} device err {err:.2e} worst/bound {ratio:.3f}')
        assert ratio <= 1.0, (ratio, err)
        want_pick = torch.where(tj >= 0, x[torch.arange(n_rows), tj.clamp(min=0)], torch.zeros(n_rows))
        assert torch.equal(pick[toks], want_pick)
        rest = torch.ones(n_tok, dtype=torch.bool)
        rest[toks] = False
        assert (lse[rest] == -777.0).all() and (pick[rest] == -777.0).all()


def _nll_case(B, T):
    g = torch.Generator().manual_seed(B * T)
    N = B * T
    kind = torch.randint(0, 3, (N,), generator=g)                       # 0 shortlist, 1 tail, 2 ignored
    kind.view(B, T)[:, T - 1] = 2                                        # hidden[:, :-1]: the last position has no label
    kind[0] = 0
    th = torch.where(kind == 2, -1, torch.randint(0, 100, (N,), generator=g)).to(torch.int32)
    tt = torch.where(kind == 1, torch.randint(0, 100, (N,), generator=g), -1).to(torch.int32)
    hl, tl = torch.rand(N, generator=g) * 3 + 8, torch.rand(N, generator=g) * 3 + 9
    hp, tp = torch.randn(N, generator=g), torch.randn(N, generator=g)
    hp[0] = hl[0]                                                        # token 0: a loss of exactly 0
    tok = torch.where(kind == 2, torch.zeros(N), (hl - hp) + torch.where(kind == 1, tl - tp, torch.zeros(N)))
    tok64 = torch.where(kind == 2, 0.0, (hl.double() - hp.double()) + torch.where(kind == 1, tl.double() - tp.double(), 0.0))
    start = torch.tensor([5.5, 3.0])
    ref_sum = start[0].double() + tok64.sum()
    seq = np.cumsum(torch.cat([start[:1], tok]).numpy(), dtype=np.float32)[-1]     # numpy: a sequential float32 accumulator
    gp = abs(float(seq) - ref_sum.item()) / ref_sum.item()
    return dict(th=th, tt=tt, hl=hl, hp=hp, tl=tl, tp=tp, tok=tok, start=start, ref_sum=ref_sum, gap=gp)


@pytest.mark.parametrize('B,T', [(1, 2), (3, 700), (4, 1024)])
def test_bucket_nll_finish(dev, B, T):
    """mxl_bucket_nll_finish: per-token loss (head_lse - head_pick) [+ (tail_lse - tail_pick)] bit-equal to the same float32
    expression; 0 for ignored rows; the (B, T-1) layout without the last row of each sequence; acc2 = (sum, count of nonzero) on
    top of a nonzero start; a token whose loss is exactly 0 is not counted.  Sum: CPU gap of a sequential float32 sum 9.1e-7
    -> bound 2^-24 |ref| + 3.7e-6 max|ref|; the count is exact."""
    from symbolic_music_generation_amd import ops
    c = _nll_case(B, T)
    N = B * T
    th, tt, hl, hp, tl, tp, tok, start, ref_sum, gp = (c[k] for k in ('th', 'tt', 'hl', 'hp', 'tl', 'tp', 'tok', 'start', 'ref_sum', 'gap'))
    check_gap(gp, B_SUM)
    nll = torch.full((B * (T - 1) + 3,), -777.0, device=dev)
    nll_tok = torch.full((N + 3,), -777.0, device=dev)
    acc = start.to(dev)
    ops.bucket_nll_finish(hl.to(dev), hp.to(dev), tl.to(dev), tp.to(dev), th.to(dev), tt.to(dev), nll, nll_tok, acc, B, T)
    torch.cuda.synchronize()
    nll, nll_tok, acc = nll.cpu(), nll_tok.cpu(), acc.cpu()
    assert torch.equal(nll_tok[:N], tok) and (nll_tok[N:] == -777.0).all()
    assert torch.equal(nll[:B * (T - 1)].view(B, T - 1), tok.view(B, T)[:, :T - 1]) and (nll[B * (T - 1):] == -777.0).all()
    assert tok[0] == 0 and acc[1].item() == 3.0 + (tok != 0).sum().item()
    ratio, err = worst(acc[:1], ref_sum.view(1), A_F32, B_SUM)
    print(f'bucket_nll_finish B{B} T{T}: cpu sequential-sum gap {gp:.2e} device err {err:.2e} worst/bound {ratio:.3f}')
    assert ratio <= 1.0, (ratio, err)


def _grad_case(ncols, count):
    g = torch.Generator().manual_seed(ncols + int(count))
    n_rows, ld, n_tok, gscale = 9, ncols + 3, 20, 1.7
    x = torch.randn(n_rows, ld, generator=g) * 3
    x[:, ncols:] = 1e30
    lse32 = torch.logsumexp(x[:, :ncols].double(), -1).float()
    tj = torch.randint(0, ncols, (n_rows,), generator=g)
    tj[0], tj[1], tj[2] = -1, 0, ncols - 1
    lossj = torch.rand(n_rows, generator=g) + 0.5
    lossj[3] = 0.0                                                       # a loss of exactly 0: dropped by `losses != 0`
    live = (tj >= 0) & (lossj != 0)
    gs32 = torch.tensor(gscale) / max(count, 1.0)

    def formula(dt):
        p = torch.exp(x[:, :ncols].to(dt) - lse32.to(dt).unsqueeze(1))
        p[torch.arange(n_rows)[tj >= 0], tj[tj >= 0]] -= 1
        return torch.where(live.unsqueeze(1), p * gs32.to(dt), torch.zeros((), dtype=dt))

    ref, r32 = formula(torch.float64), formula(torch.float32)
    gp = gap(r32, ref)
    return dict(g=g, n_rows=n_rows, n_tok=n_tok, gscale=gscale, x=x, lse32=lse32, tj=tj, lossj=lossj, live=live, ref=ref, gap=gp)


@pytest.mark.parametrize('count', [0.0, 37.0])
@pytest.mark.parametrize('with_lo', [True, False])
@pytest.mark.parametrize('ncols,ldo', [(5, 8), (257, 272), (1000, 1000)])
def test_rows_softmax_grad(dev, ncols, ldo, with_lo, count):
    """mxl_rows_softmax_grad against float64 (softmax - onehot) * grad_scale / max(count, 1) with lse, targets and counts as
    inputs.  out_hi: one bf16 rounding of the value (2^-8 |ref| + b); hi + lo: two-term precision (2^-16 |ref| + b); CPU float32
    gap 6.2e-8 of max|ref| -> b = 2.5e-7 max|ref|.  Pad columns ncols .. ldo, ignored rows and rows whose loss is exactly 0 are
    all zero; count = 0 divides by 1; out_lo may be absent; both row addressing forms."""
    from symbolic_music_generation_amd import ops
    c = _grad_case(ncols, count)
    g, n_rows, n_tok, gscale, x, lse32, tj, lossj, live, ref, gp = (c[k] for k in ('g', 'n_rows', 'n_tok', 'gscale', 'x', 'lse32', 'tj', 'lossj', 'live', 'ref', 'gap'))
    check_gap(gp, B_GRAD)
    for rows_idx, row0 in ((torch.randperm(n_tok, generator=g)[:n_rows], 0), (None, 7)):
        toks = rows_idx if rows_idx is not None else torch.arange(row0, row0 + n_rows)
        tgt = torch.full((n_tok,), -1, dtype=torch.int32); tgt[toks] = tj.to(torch.int32)
        lse = torch.full((n_tok,), float('nan')); lse[toks] = lse32
        loss = torch.full((n_tok,), float('nan')); loss[toks] = lossj
        hi = torch.full((n_rows + 2, ldo), float('nan'), dtype=torch.bfloat16, device=dev)
        lo = torch.full((n_rows + 2, ldo), float('nan'), dtype=torch.bfloat16, device=dev) if with_lo else None
        ops.rows_softmax_grad(x.to(dev), ncols, n_rows, tgt.to(dev), lse.to(dev), loss.to(dev), torch.tensor([3.25, count], device=dev),
                              gscale, hi[1:n_rows + 1], out_lo=None if lo is None else lo[1:n_rows + 1],
                              rows_idx=None if rows_idx is None else rows_idx.to(torch.int32).to(dev), row0=row0)
        torch.cuda.synchronize()
        for buf in (hi, lo):
            if buf is not None:
                b = buf.float().cpu()
                assert torch.isnan(b[0]).all() and torch.isnan(b[n_rows + 1]).all()
                assert (b[1:n_rows + 1, ncols:] == 0).all() and (b[1:n_rows + 1][~live] == 0).all()
        h = hi[1:n_rows + 1, :ncols].float().cpu()
        ratio, err = worst(h, ref, A_BF16, B_GRAD)
        assert ratio <= 1.0, ('hi', ratio, err)
        msg = f'rows_softmax_grad ncols{ncols} count{count}: cpu gap {gp:.2e} hi err {err:.2e} worst/bound {ratio:.3f}'
        if lo is not None:
            two = h.double() + lo[1:n_rows + 1, :ncols].float().cpu().double()
            ratio, err = worst(two, ref, 2.0 ** -16, B_GRAD)
            assert ratio <= 1.0, ('hi + lo', ratio, err)
            msg += f'; hi+lo err {err:.2e} worst/bound {ratio:.3f}'
        print(msg)
