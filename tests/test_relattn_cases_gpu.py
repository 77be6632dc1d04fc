"""The banded relative-position attention kernels (csrc/relattn_fwd.hip, relattn_bwd.hip, relattn_bwd_fused.hip,
relattn_drd_phantom.hip), every output element-wise against the float64 closed form of oracle/relattn_cases.py:

    |got - ref| <= a |ref| + b max|ref|        a = 2^-8 (bf16 outputs: out, dq, dk, dv, oph) or 2^-24 (float32: lse, d_rd, d_rwb, d_rrb)

`b` per output is 4 x the largest gap, relative to max|ref|, between the operand-rounded CPU model (relattn_ref64(rounded=True),
every arm the shape can take) and the float64 reference over all the cases of oracle/relattn_cases.CASES -- the rule of
oracle/kernel_cases.py with the kernels' bf16 / fp16 operand roundings in the place of float32 accumulation.  Measured on the CPU
(largest gap, the case and arm it came from -> b, rounded up):

    B_OUT   4.86e-3  t70_dh16_zero random three              -> 1.95e-2
    B_LSE   1.02e-3  t320_m256_part diagonal three           -> 4.1e-3
    B_DQ    8.99e-3  t100_dh32_part_scale diagonal three     -> 3.6e-2
    B_DK    8.40e-3  t100_dh32_part_scale diagonal three     -> 3.4e-2
    B_DV    5.88e-3  t96_dh32_m256_zero random three         -> 2.4e-2
    B_D_RD  1.37e-2  t320_m256_part far-edge three           -> 5.5e-2
    B_D_RWB 6.08e-3  t100_dh32_part_scale far-edge three     -> 2.5e-2
    B_D_RRB 8.90e-3  t320_m256_part far-edge three           -> 3.6e-2
    B_OPH   3.01e-3  t96_m256_zero diagonal                  -> 1.21e-2

The random cases alone sit at 2e-3 .. 5e-3 on every tensor; the structured ones (most of a row's mass on one cell) cost more on the
gradients because dS = P (dP - delta) cancels there.  tests/test_relattn_cases_cpu.py re-measures every gap against these bounds and
shows that a dropped band-edge cell, a dG tile shifted by one distance and a d_rd row off by 10 % leave them.

Every launch also checks: outputs sit in NaN canary frames (row strides larger than H dh wherever the C ABI takes one), every
element inside is finite and the frame is untouched; d_rd, d_rwb, d_rrb start from a non-zero pattern and must come back as
pattern + reference; dk / dv of a key no query sees (position -M with full memory) are exactly zero; the fused pass gets a
workspace of exactly the size it asks for, NaN-filled between two NaN guards that must stay intact.

The fused pass runs here in per-block mode, forced (dq_mode='slabs': neither the dispatch rule nor MXL_FUSED_OWNER decides);
tests/test_relattn_owner_cases_gpu.py runs it in owner mode through the same `Run` / `run_backward`.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from oracle.kernel_cases import A_BF16, A_F32, check_gap, gap, worst
from oracle.relattn_cases import CASES, arms_of, case_model, case_ref, dims

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B_OUT, B_LSE, B_DQ, B_DK, B_DV, B_D_RD, B_D_RWB, B_D_RRB, B_OPH = 1.95e-2, 4.1e-3, 3.6e-2, 3.4e-2, 2.4e-2, 5.5e-2, 2.5e-2, 3.6e-2, 1.21e-2
B_OF = dict(out=B_OUT, lse=B_LSE, dq=B_DQ, dk=B_DK, dv=B_DV, d_rd=B_D_RD, d_rwb=B_D_RWB, d_rrb=B_D_RRB, oph=B_OPH)
A_OF = dict(out=A_BF16, lse=A_F32, dq=A_BF16, dk=A_BF16, dv=A_BF16, d_rd=A_F32, d_rwb=A_F32, d_rrb=A_F32, oph=A_BF16)
PAD = 8          # extra elements per row of a framed buffer
IDS = [f'{s}-{f}' for s, f in CASES]


# ---------------------------------------------------------------------------------------------------------------- canary frames
class Framed:
    """a (B, R, d) [or (R, d) with B = None] window inside a NaN buffer of one more row on either side and PAD more columns"""

    def __init__(self, dev, B, R, d, dtype, pad=PAD):
        lead = () if B is None else (B,)
        self.full = torch.full(lead + (R + 2, d + pad), float('nan'), device=dev, dtype=dtype)
        self.view = self.full[..., 1:R + 1, :d]
        self.rs = d + pad
        self.bs = (R + 2) * (d + pad)

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.isfinite(self.view.float()).all(), f'{what}: an element inside the frame is not finite (left unwritten?)'
        f = self.full.float().clone()
        f[..., 1:-1, :self.view.shape[-1]] = float('nan')
        assert torch.isnan(f).all(), f'{what}: wrote outside its window'


class Flat:
    """`shape` float32 values between two NaN guards of 64 elements"""

    def __init__(self, dev, shape, fill=float('nan')):
        n = math.prod(shape)
        self.full = torch.full((n + 128,), float('nan'), device=dev)
        self.view = self.full[64:64 + n].view(shape)
        self.view.fill_(fill) if not isinstance(fill, torch.Tensor) else self.view.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        assert torch.isfinite(self.view).all(), f'{what}: an element inside the frame is not finite (left unwritten?)'
        assert torch.isnan(self.full[:64]).all() and torch.isnan(self.full[-64:]).all(), f'{what}: wrote outside its window'


class Packed:
    """dq, dk, dv as the training engine passes them: column slices of one NaN-filled (B, Kc, 3 d) buffer, dq in its last T rows
    (row stride 3 d for all three, batch stride Kc 3 d).  Afterwards the dq columns of the first Kc - T rows are still NaN and every
    other element is finite."""

    def __init__(self, dev, B, T, Kc, d):
        self.full = torch.full((B, Kc, 3 * d), float('nan'), device=dev, dtype=torch.bfloat16)
        self.T, self.Kc, self.d = T, Kc, d

    def parts(self):
        import types
        T, Kc, d = self.T, self.Kc, self.d
        views = (self.full[:, Kc - T:, :d], self.full[:, :, d:2 * d], self.full[:, :, 2 * d:])
        return tuple(types.SimpleNamespace(view=v, rs=3 * d, bs=Kc * 3 * d, check=self.check) for v in views)

    def check(self, what):
        torch.cuda.synchronize()
        f = self.full.float().clone()
        assert torch.isnan(f[:, :self.Kc - self.T, :self.d]).all(), f'{what}: the dq columns of the memory rows were written'
        f[:, :self.Kc - self.T, :self.d] = 0
        assert torch.isfinite(f).all(), f'{what}: an element of the packed gradients is not finite (left unwritten?)'


def check_ws(ws, used):
    """the workspace of the fused backward (a Flat): its guards are untouched, and everything beyond the first `used` floats (owner
    mode: the float32 carry, B T H 64 of them, whatever M is) is still the NaN it was filled with"""
    torch.cuda.synchronize()
    assert torch.isnan(ws.full[:64]).all() and torch.isnan(ws.full[-64:]).all(), 'ws: wrote outside the workspace'
    if used is not None:
        assert torch.isnan(ws.view[used:]).all(), 'ws: owner mode wrote beyond its carry'


def _pattern(shape, seed):
    """the known non-zero float32 contents an accumulated output starts from: multiples of 2^-8 in +-[1/8, 5/8]"""
    g = torch.Generator().manual_seed(seed)
    p = (torch.randint(32, 160, shape, generator=g).float() / 256.0)
    return p * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------- launches
class Run:
    """the device buffers of one case: inputs, framed forward outputs, and `forward` / `backward` launches"""

    def __init__(self, dev, c, packed=False):
        """packed: q, k, v are column slices of one (B, Kc, 3 d) buffer and dq, dk, dv of another, as the training engine passes them"""
        self.dev, self.c, self.packed = dev, c, packed
        B, T, H, dh, M, Kc = (c[n] for n in ('B', 'T', 'H', 'dh', 'M', 'Kc'))
        d = H * dh
        self.d = d
        self.q = c['q'].reshape(B, T, d).to(dev)
        self.k = c['k'].reshape(B, Kc, d).to(dev)
        self.v = c['v'].reshape(B, Kc, d).to(dev)
        self.rd = c['rd'].reshape(M, d).to(dev)
        self.rwb, self.rrb = c['rwb'].float().to(dev), c['rrb'].float().to(dev)
        self.out = Framed(dev, B, T, d, torch.bfloat16)
        self.dout = Framed(dev, B, T, d, torch.bfloat16)            # (shares the batch / row strides of out in the C ABI)
        self.dout.view.copy_(c['dout'].reshape(B, T, d))
        self.lse = Flat(dev, (B, H, T))
        self.st = dict(B=B, T=T, H=H, dh=dh, M=M, Kc=Kc, q_bs=T * d, q_rs=d, kv_bs=Kc * d, kv_rs=d, rd_rs=d, o_bs=self.out.bs,
                       o_rs=self.out.rs, scale=c['scale'])
        self.oph = self.mph = self.ph = None
        if packed:       # the rows of the q columns that belong to memory positions stay NaN: nothing may read them
            qkv = torch.full((B, Kc, 3 * d), float('nan'), device=dev, dtype=torch.bfloat16)
            qkv[:, Kc - T:, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:] = self.q, self.k, self.v
            self.q, self.k, self.v = qkv[:, Kc - T:, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
            self.st.update(q_bs=Kc * 3 * d, q_rs=3 * d, kv_bs=Kc * 3 * d, kv_rs=3 * d)

    def forward(self, oph=None, ph_buf=False):
        """oph: None (mxl_relattn_fwd), 'blk' (mxl_relattn_fwd_phantom), 'all' (mxl_relattn_fwd_phantom2, with the records if ph_buf)"""
        from symbolic_music_generation_amd import ops
        c, dev = self.c, self.dev
        extra = {}
        if oph is not None:
            self.oph = Framed(dev, c['B'], c['T'], self.d, torch.bfloat16)
            self.mph = Flat(dev, (c['B'], c['H'], c['T']))
            extra = dict(oph=self.oph.view, mph=self.mph.view, oph_all=oph == 'all')
            if ph_buf:
                n = int(ops.lib().mxl_relattn_drd_phantom_ws_bytes(c['B'], c['T'], c['H']))
                assert n > 0
                self.ph = torch.full((n,), 0xFF, device=dev, dtype=torch.uint8)
                extra['ph_buf'] = self.ph
        ops.relattn_fwd(self.q, self.k, self.v, self.rd, self.rwb, self.rrb, self.out.view, self.lse.view, **self.st, **extra)
        self.out.check('out'); self.lse.check('lse')
        got = dict(out=self.out.view.double().cpu().view(c['B'], c['T'], c['H'], c['dh']), lse=self.lse.view.double().cpu())
        if oph is not None:
            self.oph.check('oph'); self.mph.check('mph')
            f = torch.exp2(self.mph.view.double() - self.lse.view.double() / math.log(2.0)).cpu()          # 2^(mph - lse2)
            got['oph'] = f.transpose(1, 2)[..., None] * self.oph.view.double().cpu().view(c['B'], c['T'], c['H'], c['dh'])
            got['oph_raw'] = self.oph.view.float().cpu()
        return got

    def backward(self, arm, dg_seqs=None, records='prep', delta_ready=False, dq_mode='slabs', delta_in=None, launch=None):
        """arm: 'plain' / 'dq8' / 'sparse' / 'sparse_oph' (ops.relattn_bwd; the caller has set the knobs) or 'fused' (dq_mode: the form
        that produces dq, 'slabs' = per-block mode or 'owner', forced: no environment variable and no dispatch rule decides; None
        leaves it to the dispatch rule, and the caller reads the mode from the returned workspace.  delta_in: the delta a
        delta_ready call supplies, instead of the host's float64 one.  launch: stands in for ops.relattn_bwd_fused)"""
        from symbolic_music_generation_amd import ops
        c, dev, d = self.c, self.dev, self.d
        B, T, H, dh, M, Kc = (c[n] for n in ('B', 'T', 'H', 'dh', 'M', 'Kc'))
        dq = Framed(dev, B, T, d, torch.bfloat16)
        dk, dv = Framed(dev, B, Kc, d, torch.bfloat16), Framed(dev, B, Kc, d, torch.bfloat16)
        if self.packed:
            dq, dk, dv = Packed(dev, B, T, Kc, d).parts()
        pat = dict(d_rd=_pattern((M, d), 1), d_rwb=_pattern((H, dh), 2), d_rrb=_pattern((H, dh), 3))
        d_rwb, d_rrb = Flat(dev, (H, dh), pat['d_rwb'].to(dev)), Flat(dev, (H, dh), pat['d_rrb'].to(dev))
        delta = Flat(dev, (B, H, T))
        qr_buf = torch.full((B, T, d), float('nan'), device=dev, dtype=torch.bfloat16)
        kw = dict(self.st, dq_bs=dq.bs, dq_rs=dq.rs, dkv_bs=dk.bs, dkv_rs=dk.rs)
        args = (self.q, self.k, self.v, self.rd, self.rwb, self.rrb, self.out.view, self.dout.view, self.lse.view, delta.view, dq.view,
                dk.view, dv.view)
        if arm == 'fused':
            assert ops.fused_bwd_applies(T=T, dh=dh, M=M, Kc=Kc, B=B, H=H)
            d_rd = Framed(dev, None, M, d, torch.float32)           # the C ABI takes d_rd's row stride
            d_rd.view.copy_(pat['d_rd'])
            assert dq_mode in (None, 'slabs', 'owner')
            n_ws = ops.relattn_bwd_fused_ws_numel(B, T, H, dh, M)
            assert n_ws * 4 == ((M + 255) // 256 + 1) * B * T * H * 128          # one bf16 slab per key block a tile can touch
            ws = Flat(dev, (n_ws,))          # exactly the floats requested, NaN-filled, between two NaN guards
            if delta_ready:      # delta on the host, in float64 from the device's bf16 out, rounded to float32
                dl = torch.einsum('bihe,bihe->bhi', self.dout.view.double().view(B, T, H, dh), self.out.view.double().view(B, T, H, dh))
                delta.view.copy_(dl.float() if delta_in is None else delta_in)
            fused = launch or ops.relattn_bwd_fused
            fused(*args, d_rd.view, d_rwb.view, d_rrb.view, ws.view, qr_buf, oph=None if self.oph is None else self.oph.view,
                  mph=None if self.mph is None else self.mph.view, ph_buf=self.ph if records == 'fwd' else None,
                  ph_ready=records == 'fwd', delta_ready=delta_ready, dq_mode=dq_mode, **kw)
            check_ws(ws, B * T * H * 64 if dq_mode == 'owner' else None)
        else:
            d_rd = Flat(dev, (M, d), pat['d_rd'].to(dev))
            n = B if dg_seqs is None else dg_seqs
            dg = torch.full((n, H, T, M), float('nan'), device=dev, dtype=torch.bfloat16)
            with_oph = arm == 'sparse_oph'
            ops.relattn_bwd(*args, dg, d_rwb.view, d_rrb.view, d_rd=d_rd.view, qr_buf=qr_buf, oph=self.oph.view if with_oph else None,
                            mph=self.mph.view if with_oph else None, **kw)
        for nm, f in (('dq', dq), ('dk', dk), ('dv', dv), ('d_rd', d_rd), ('d_rwb', d_rwb), ('d_rrb', d_rrb), ('delta', delta)):
            f.check(nm)
        got = dict(dq=dq.view.double().cpu().view(B, T, H, dh), dk=dk.view.double().cpu().view(B, Kc, H, dh),
                   dv=dv.view.double().cpu().view(B, Kc, H, dh), delta=delta.view.cpu())
        if arm == 'fused':
            got['ws'] = ws
            got['bits'] = {nm: f.view.cpu().contiguous().view(torch.int16) for nm, f in (('dq', dq), ('dk', dk), ('dv', dv))}
        # accumulated outputs: pattern + reference (`=` for `+=` or a double add shows as an error of the pattern's size, 1/8 .. 5/8 per
        # element, far above b max|ref| wherever the reference is small; the float32 add itself costs 2^-24 of that, inside b)
        for nm, f in (('d_rd', d_rd), ('d_rwb', d_rwb), ('d_rrb', d_rrb)):
            got[nm] = (f.view.double().cpu() - pat[nm].double()).view((M, H, dh) if nm == 'd_rd' else (H, dh))
        if Kc == M + T:          # key position -M: visible to no query
            assert (got['dk'][:, 0] == 0).all() and (got['dv'][:, 0] == 0).all(), 'dk / dv of an invisible key must be exactly zero'
        return got


def _judge(what, got, ref, model, names):
    bad = []
    for n in names:
        key = 'oph' if n.startswith('oph') else n
        g = gap(model[n], ref[n])
        ratio, err = worst(got[key], ref[n], A_OF[key], B_OF[key])
        print(f'relattn {what} {n}: cpu rounded-model gap {g:.3e}  device max err {err:.3e} of max|ref|  worst/bound {ratio:.3f}')
        check_gap(g, B_OF[key])
        if not ratio <= 1.0:
            bad.append((n, ratio, err))
    assert not bad, (what, bad)


GRADS = ('dq', 'dk', 'dv', 'd_rd', 'd_rwb', 'd_rrb')
MODEL_ARM = dict(plain='three', dq8='three', sparse='sparse', sparse_oph='sparse_oph', fused='fused')


def device_arms(c):
    """the launches a case's shape can take (oracle.relattn_cases.arms_of, with the two forms of the query-owner kernel)"""
    arms = ['plain'] + (['dq8'] if c['dh'] == 64 and c['T'] % 32 == 0 else [])
    return arms + [a for a in arms_of(c) if a != 'three']


def run_backward(dev, shape, family, arm, setenv, packed=False, **kw):
    """forward + backward of one case on one arm, judged; `setenv(name, value)` sets a knob ops.py reads per call.  -> the outputs"""
    from symbolic_music_generation_amd import ops
    c, ref = case_ref(shape, family)
    B, T, H, dh, M, Kc = (c[n] for n in ('B', 'T', 'H', 'dh', 'M', 'Kc'))
    zero_mem = Kc < M + T
    setenv('MXL_NO_DQ8', '1' if arm == 'plain' else '0')
    setenv('MXL_DG_RECOMPUTE', '0' if arm == 'dq8' else '1')
    setenv('MXL_NO_OPH', '0')
    setenv('MXL_NO_FUSED_BWD', '0')
    calls = []
    real = ops.gemm_batched
    ops.gemm_batched = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        run = Run(dev, c, packed)
        if arm == 'sparse_oph':
            assert ops.phantom_sum_applies(T=T, dh=dh, M=M, Kc=Kc)
            fwd = run.forward(oph='blk')
        elif arm == 'fused' and zero_mem:
            fwd = run.forward(oph='all', ph_buf=kw.get('records') == 'fwd')
        else:
            fwd = run.forward()
        got = run.backward(arm, **kw)
    finally:
        ops.gemm_batched = real
    if arm != 'fused':      # the dRd contraction: the streaming kernel, or (rc == -2) the batched GEMM
        streaming = dh == 64 and T % 32 == 0 and M % 8 == 0
        assert bool(calls) == (not streaming), (arm, calls)
        if arm in ('sparse', 'sparse_oph'):
            assert dh == 64 and T % 32 == 0 and M % 256 == 0 and zero_mem
    got.update(fwd)
    model = case_model(shape, family, 'fused_owner' if kw.get('dq_mode') == 'owner' else MODEL_ARM[arm])
    _judge(f'{shape} {family} {arm} {"packed " if packed else ""}{kw or ""}', got, ref, model, ('out', 'lse') + GRADS)
    return got


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize('shape,family', CASES, ids=IDS)
def test_forward(dev, shape, family):
    """mxl_relattn_fwd at dh = 16, 32, 64: ragged T, T = 1, T < M on zero memories, partial and full memory, an own scale"""
    c, ref = case_ref(shape, family)
    got = Run(dev, c).forward()
    _judge(f'{shape} {family} fwd', got, ref, case_model(shape, family, 'three'), ('out', 'lse'))


def _phantom_modes(shape):
    """'blk' needs whole 256-distance blocks, 'all' the first stored key on a 64-key tile, the records a dh = 64 shape"""
    x = dims(shape)
    if x['Kc'] >= x['M'] + x['T'] or x['T'] % 32 != 0:
        return []
    return ((['blk'] if x['M'] % 256 == 0 else []) + (['all'] if (x['T'] - x['Kc']) % 64 == 0 and x['M'] % 32 == 0 else [])
            + (['all+records'] if (x['T'] - x['Kc']) % 64 == 0 and x['M'] % 32 == 0 and x['dh'] == 64 else []))


PH_CASES = [(s, f, m) for s, f in CASES for m in _phantom_modes(s)]


@pytest.mark.parametrize('shape,family,mode', PH_CASES, ids=[f'{s}-{f}-{m}' for s, f, m in PH_CASES])
def test_forward_phantom_sum(dev, shape, family, mode):
    """mxl_relattn_fwd_phantom (oph over the all-phantom 256-distance blocks) and mxl_relattn_fwd_phantom2 (over every phantom cell,
    without and with the records of the phantom cells' dRd kernel): out and lse as the plain forward, and the value-sum through the
    reference-free product 2^(mph - lse2) oph[i] = sum over the set's cells of P[i,d] Rd[d] (mph alone is an arbitrary reference point)"""
    c, ref = case_ref(shape, family)
    run = Run(dev, c)
    got = run.forward(oph='blk' if mode == 'blk' else 'all', ph_buf=mode == 'all+records')
    name = 'oph_blk' if mode == 'blk' else 'oph_all'
    model = case_model(shape, family, 'three')
    if ref[name].abs().max() == 0:       # no cell in the set (M = 256: no all-phantom block): zeros, exactly
        assert (got['oph_raw'] == 0).all()
        _judge(f'{shape} {family} fwd {mode}', got, ref, model, ('out', 'lse'))
    else:
        _judge(f'{shape} {family} fwd {mode}', got, ref, model, ('out', 'lse', name))
    if mode == 'all+records':
        assert not (run.ph.view(-1, 4352) == 0xFF).all(1).any(), 'a record was left unwritten'


# ---------------------------------------------------------------------------------------------------------------- backward
BWD = [(s, f, a) for s, f in CASES if dims(s)['T'] > 1 for a in device_arms(dims(s))]      # (T = 1 is a forward shape)


@pytest.mark.parametrize('shape,family,arm', BWD, ids=[f'{s}-{f}-{a}' for s, f, a in BWD])
def test_backward(dev, monkeypatch, shape, family, arm):
    """every case on every backward arm its shape can take: the plain three-kernel form (d_rrb from the query-owner kernel; the dRd
    contraction streaming or, off its shapes, the batched GEMM), the 8-wave form with the streaming mxl_relattn_drd, the sparse-dG
    pair with mxl_relattn_drd_recompute, the same with the forward's phantom sum, and the fused pass (records from the prep pass) in
    per-block mode; tests/test_relattn_owner_cases_gpu.py runs the fused pass in owner mode"""
    run_backward(dev, shape, family, arm, monkeypatch.setenv, **(dict(dq_mode='slabs') if arm == 'fused' else {}))


@pytest.mark.parametrize('shape,family,arm', [('t320_m256_part', 'random', 'dq8'), ('t320_m256_part', 'far-edge', 'sparse'),
                                              ('t100_dh32_part_scale', 'position-coded', 'plain')])
def test_backward_with_a_dg_buffer_of_fewer_sequences(dev, monkeypatch, shape, family, arm):
    """a dG buffer of one sequence for a batch of two or three: the batch is walked in chunks, the batch-summed outputs accumulate"""
    run_backward(dev, shape, family, arm, monkeypatch.setenv, dg_seqs=1)


FUSED = [(s, f) for s, f in CASES if 'fused' in arms_of(dims(s))]


@pytest.mark.parametrize('records,delta_ready', [('fwd', False), ('prep', True), ('fwd', True)])
@pytest.mark.parametrize('shape,family', FUSED, ids=[f'{s}-{f}' for s, f in FUSED])
def test_backward_fused_records_and_delta(dev, monkeypatch, shape, family, records, delta_ready):
    """mxl_relattn_bwd_fused with the phantom records written by the forward, and with `delta` supplied by the caller (computed on
    the host in float64 from the device's out, rounded to float32); test_backward covers the prep pass with the kernel's own delta"""
    run_backward(dev, shape, family, 'fused', monkeypatch.setenv, records=records, delta_ready=delta_ready, dq_mode='slabs')


def _balance_multipliers(T, M, Kc, B, H):
    """host side of mxl_relattn_drd_phantom with MXL_DRD_PH_BALANCE = 1: batch groups per workgroup of each 256-distance block"""
    nk, spb, pz = (M + 255) // 256, T // 32, T - Kc
    nph = [0 if 256 * k + pz < -256 else max(0, min(spb, (256 * k + pz) // 32 + 8)) for k in range(nk)]
    groups = min(B, max(1, (6 * 512 + nk * H - 1) // (nk * H)))
    bgroup = (B + groups - 1) // groups
    groups = (B + bgroup - 1) // bgroup
    out = []
    for k in range(nk):
        m = 1
        while nph[k] > 0 and 2 * m * nph[k] <= max(nph) and 2 * m <= groups:
            m *= 2
        out.append(m)
    return out


def test_backward_fused_with_balanced_phantom_groups_in_a_child_process(dev):
    """MXL_DRD_PH_BALANCE is read once per process (a static in mxl_relattn_drd_phantom), so it is exercised in a fresh child: at
    T = 320, M = 288, Kc = T + 128 the short first distance block takes two batch groups per workgroup, the second one"""
    shape = 't320_m288_part128'
    c, _ = case_ref(shape, 'random')
    assert _balance_multipliers(c['T'], c['M'], c['Kc'], c['B'], c['H']) == [2, 1]
    code = ('import os, sys, torch\n'
            f'sys.path.insert(0, {ROOT!r})\n'
            'from tests import test_relattn_cases_gpu as t\n'
            f't.run_backward(torch.device("cuda:0"), {shape!r}, "random", "fused", os.environ.__setitem__, dq_mode="slabs")\n'
            f't.run_backward(torch.device("cuda:0"), {shape!r}, "far-edge", "fused", os.environ.__setitem__, records="fwd", dq_mode="slabs")\n')
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MXL_DRD_PH_BALANCE='1'), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('worst/bound') == 16
