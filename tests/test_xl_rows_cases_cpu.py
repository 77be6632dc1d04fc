"""CPU side of the element-wise tests of the Transformer-XL row kernels, head and optimiser: the float64 closed forms of
oracle/xl_rows_cases.py against float64 autograd (the head: against oracle.transfoxl_ref.ProjectedAdaptiveLogSoftmax), the rounded
models' gaps against the bounds tests/test_xl_rows_cases_gpu.py uses, the case tables' own conditions, and a check that those bounds
have teeth: every planted fault leaves the bound of its output."""
import numpy as np
import pytest
import torch

from oracle import xl_rows_cases as X
from oracle.kernel_cases import A_BF16, A_F32, check_gap, gap, keep_mask, worst
from tests.test_xl_rows_cases_gpu import A_EMB, A_HEAD, A_LN, A_SPLIT, B_EMB, B_HEAD, B_LN, B_OPT

F64, F32 = X.F64, X.F32
TIGHT = 1e-10


# ---------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize('stress', X.LN_STRESS)
@pytest.mark.parametrize('name', list(X.LN_CASES))
def test_layernorm_closed_forms_equal_float64_autograd(name, stress):
    """y, mean, rstd of the stored z and of the partial form against torch's float64 layer_norm; dres, dx, dgamma, dbeta and the add form
    against float64 autograd through z = res + keep dscale x (value pinned to the stored z)"""
    c, z, ref, _ = X.ln_expect(name, stress)
    N, d, p = c['N'], c['d'], c['p']
    eps = X.LN_EPS
    gamma = c['gamma'].double().requires_grad_(True)
    beta = c['beta'].double().requires_grad_(True)
    x = c['x'].double().requires_grad_(True)
    res = (c['res'].double() if c['res'] is not None else torch.zeros(N, d, dtype=F64)).requires_grad_(True)
    keep = X.ln_keep(c).double() * X.dscale64(p) if p > 0 else torch.ones(N, d, dtype=F64)
    lin = res + keep * x
    zz = lin + (z.double() - lin).detach()
    y = torch.nn.functional.layer_norm(zz, (d,), gamma, beta, eps)
    dyv = c['dy'].double() + (c['dy2'].double() if c['dy2'] is not None else 0)
    y.backward(dyv)
    want = dict(y=y.detach(), mean=z.double().mean(1), rstd=1 / torch.sqrt(z.double().var(1, unbiased=False) + eps), dres=res.grad, dx=x.grad,
                dgamma=gamma.grad, dbeta=beta.grad, dres_add=res.grad + c['dadd'].double(),
                y_partial=torch.nn.functional.layer_norm(X.ln_partial_z_exact(c).double(), (d,), c['gamma'].double(), c['beta'].double(), eps))
    for k, w in want.items():
        g = X.groups_gap(ref[k], w, c['groups'] if k in X.LN_ROWWISE else None)
        assert g <= 1e-9, (name, stress, k, g)


@pytest.mark.parametrize('name', list(X.EMB_CASES))
def test_embedding_closed_form_equals_float64_autograd(name):
    c = X.emb_case(name)
    ref = X.emb_ref(c, F64)
    N, d, p = c['N'], c['d'], c['p']
    E = c['E'].double().requires_grad_(True)
    keep = (X.flat_keep(c['seed'], c['site'], (N, d), p, form32=False).double() * X.dscale64(p)) if p > 0 else torch.ones(N, d, dtype=F64)
    out = torch.nn.functional.embedding(c['ids'].clamp(0, c['V'] - 1), E)[c['valid']] * X.EMB_SCALE * keep[c['valid']]
    gsum = c['dout'].double() + (c['dout2'].double() if c['dout2'] is not None else 0)
    out.backward(gsum[c['valid']])
    assert gap(ref['out'][c['valid']], out.detach()) <= TIGHT and gap(ref['dE'], E.grad) <= TIGHT
    # rows with an id outside [0, V): the forward gives the row of id 0
    if (~c['valid']).any():
        assert torch.equal(ref['out'][~c['valid']], (c['E'].double()[0] * X.EMB_SCALE * keep)[~c['valid']])


@pytest.mark.parametrize('name', [n for n, c in X.SIN_CASES.items() if c['p'] == 0])
def test_sinusoid_closed_form_equals_the_reference_module(name):
    from oracle.transfoxl_ref import PositionalEmbedding
    c = X.SIN_CASES[name]
    pe = PositionalEmbedding(c['d']).double()
    pos = torch.arange(c['M'], dtype=F64)
    if c['clamp'] > 0:
        pos = pos.clamp_max(c['clamp'])
    inv = 1 / (10000 ** (torch.arange(0.0, c['d'], 2.0, dtype=F64) / c['d']))
    want = torch.cat([torch.outer(pos, inv).sin(), torch.outer(pos, inv).cos()], 1)
    assert gap(X.sin_ref(name, F64), want) <= TIGHT
    # the module's inv_freq buffer is built in float32: one rounding, 2^-24 relative, of arguments up to max(pos)
    assert gap(pe(pos).reshape(c['M'], c['d']), want) <= float(pos.max()) * 2.0 ** -23 + 1e-9


@pytest.mark.parametrize('name', list(X.HEAD_CASES))
def test_head_closed_form_equals_the_reference_module(name):
    """nll (kept in token order), the log-probabilities and, through float64 autograd of loss = sum(nll[nll != 0]) / count, dlogits
    against ProjectedAdaptiveLogSoftmax fed identity weights (hidden = the logits).  The module indexes a label >= V without cutoffs:
    that label is handed to it as -100, which is what the kernel treats it as"""
    from oracle.transfoxl_ref import ProjectedAdaptiveLogSoftmax
    c, ref, _ = X.head_expect(name)
    V, ncl, B, T = c['V'], c['ncl'], c['B'], c['T']
    nc = V + ncl
    mod = ProjectedAdaptiveLogSoftmax(V, nc, nc, list(c['cut'])).double()
    with torch.no_grad():
        mod.out_layers[0].weight.copy_(torch.eye(V, nc, dtype=F64))
        mod.out_layers[0].bias.zero_()
        if ncl:
            mod.cluster_weight.copy_(torch.cat([torch.zeros(ncl, V, dtype=F64), torch.eye(ncl, dtype=F64)], 1))
    for q in mod.parameters():
        q.requires_grad_(False)
    hid = c['logits'].double().view(B, T, nc).clone().requires_grad_(True)
    labels = torch.where(c['labels'] >= V, torch.full_like(c['labels'], -100), c['labels'])
    nll = mod(hid, labels, keep_order=True).view(B, T - 1)
    assert gap(ref['nll'], nll.detach()) <= TIGHT or ref['count'] == 0
    assert (ref['nll'] != 0).sum() == ref['count'] and gap(ref['acc0'], nll.detach().sum().reshape(1)) <= TIGHT or ref['count'] == 0
    loss = nll[nll != 0].sum() / max(ref['count'], 1) * c['gs']
    loss.backward()
    assert (ref['dlogits'] - hid.grad.view(-1, nc)).abs().max() <= 1e-12
    lp = mod(c['logits'].double().view(B, T, nc))
    assert gap(ref['logprob'], lp) <= TIGHT
    # lse columns: the head's and the label cluster's log-sum-exp
    e = c['edges']
    L = c['logits'].double()
    for row in range(c['R']):
        if ref['lse'][row, 0] != 0:
            assert abs(ref['lse'][row, 0] - torch.logsumexp(torch.cat([L[row, :e[1]], L[row, V:]]), 0)) <= 1e-9 * abs(ref['lse'][row, 0])


@pytest.mark.parametrize('name', [n for n, c in X.ADAMW_CASES.items() if c['n'] <= 10007])
def test_adamw_closed_form_equals_torch_adamw(name):
    """three steps of torch.optim.AdamW (float64) on grad_scale g clipped by clip_grad_norm_'s rule; the float32 rounding of the bias
    corrections and of the given sum of squares is the only difference (<= 1e-6)"""
    c = X.adamw_case(name)
    ref = X.adamw_chain(c, F64)
    n, nd = c['n'], c['n_decay']
    pa = c['p'][:nd].double().clone().requires_grad_(True)
    pb = c['p'][nd:].double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([dict(params=[pa], weight_decay=c['wd']), dict(params=[pb], weight_decay=0.0)], lr=c['lr'], betas=(c['b1'], c['b2']),
                            eps=c['eps'])
    for q, lo, hi in ((pa, 0, nd), (pb, nd, n)):
        s = opt.state[q]
        s['step'] = torch.tensor(float(c['step0'] - 1))
        s['exp_avg'], s['exp_avg_sq'] = c['m'][lo:hi].double().clone(), c['v'][lo:hi].double().clone()
    for k in range(X.ADAMW_STEPS):
        g = c['g'][k].double() * c['gs']
        if c['max_norm'][k] > 0 and c['clip'] != 'nosumsq':
            g = g * min(1.0, c['max_norm'][k] / (g.norm().item() + 1e-6))
        pa.grad, pb.grad = g[:nd].clone(), g[nd:].clone()
        opt.step()
        got = (torch.cat([pa.detach(), pb.detach()]), torch.cat([opt.state[pa]['exp_avg'], opt.state[pb]['exp_avg']]),
               torch.cat([opt.state[pa]['exp_avg_sq'], opt.state[pb]['exp_avg_sq']]))
        for i in range(3):
            assert gap(ref[k][i], got[i]) <= 2e-6, (name, k, 'pmv'[i], gap(ref[k][i], got[i]))


# ---------------------------------------------------------------------------------------------------------------- gaps
def test_every_gap_stays_under_its_bound():
    """the rounded models against the float64 forms on every case, under the b of tests/test_xl_rows_cases_gpu.py; prints the table of
    that module's docstring"""
    best = {}

    def upd(fam, k, g, nm, b):
        check_gap(g, b)
        if g > best.get((fam, k), (-1.0, ''))[0]:
            best[(fam, k)] = (g, nm)
    for n in X.LN_CASES:
        for s in X.LN_STRESS:
            for k, g in X.ln_gaps(n, s).items():
                upd('ln', X.LN_OUT[k], g, f'{n}/{s}', B_LN[X.LN_OUT[k]])
    for n in X.EMB_CASES:
        c = X.emb_case(n)
        r, m = X.emb_ref(c, F64), X.emb_ref(c, F32)
        for k in r:
            upd('emb', k, gap(m[k], r[k]), n, B_EMB[k])
    for n in X.SIN_CASES:
        upd('emb', 'sin', gap(X.sin_ref(n, F32), X.sin_ref(n, F64)), n, B_EMB['sin'])
    for n in X.HEAD_CASES:
        for k, g in X.head_gaps(n).items():
            upd('head', k, g, n, B_HEAD[k])
    for n in X.SUMSQ_N:
        for sp in (False, True):
            x = X.sumsq_case(n, sp)
            upd('opt', X.sumsq_key(n), gap(X.sumsq_ref(x, F32), X.sumsq_ref(x, F64)), f'sq_n{n}_{sp}', B_OPT[X.sumsq_key(n)])
    for n in X.ADAMW_CASES:
        c = X.adamw_case(n)
        r, m = X.adamw_chain(c, F64), X.adamw_chain(c, F32)
        for k in range(X.ADAMW_STEPS):
            for i, q in enumerate('pmv'):
                upd('opt', q, gap(m[k][i], r[k][i]), f'{n} step {k}', B_OPT[q])
    for (fam, k), (g, nm) in sorted(best.items()):
        print(f'{fam:5s} {k:8s} {g:.2e}  {nm}')
    # every bound is matched by a measured gap and is no more than 4 x it, rounded up to two digits
    bounds = {('ln', k): v for k, v in B_LN.items()} | {('emb', k): v for k, v in B_EMB.items()} | {('head', k): v for k, v in B_HEAD.items()} \
        | {('opt', k): v for k, v in B_OPT.items()}
    assert set(bounds) == set(best)
    for key, b in bounds.items():
        assert b <= 4.0 * best[key][0] * 1.3, (key, b, best[key])


# ---------------------------------------------------------------------------------------------------------------- the tables' conditions
def test_case_tables_reach_every_named_branch():
    ds = {c['d'] for c in X.LN_CASES.values()}
    assert ds == {8, 504, 512, 520, 1024, 1032, 2048}
    for d in ds:
        Ns = [c['N'] for c in X.LN_CASES.values() if c['d'] == d]
        assert any(n % 4 and n % 64 for n in Ns) and any(n <= 64 for n in Ns) and any(n > 64 for n in Ns), d
    assert {c['N'] for c in X.LN_CASES.values()} == {1, 3, 63, 64, 65, 130}
    assert {c['p'] for c in X.LN_CASES.values()} == {0.0, 0.1, 0.5}
    assert {c['res'] for c in X.LN_CASES.values()} == {True, False} and {c['dy2'] for c in X.LN_CASES.values()} == {True, False}
    for lo, hi in ((0, 512), (512, 1024), (1024, 2048)):
        assert any(lo < d <= hi for d in ds)
    ranges = []
    for c in X.HEAD_CASES.values():
        e = [0] + list(c['cut']) + [c['V']]
        ranges += [e[i + 1] - e[i] for i in range(len(e) - 1)]
    assert any(r <= 2048 for r in ranges) and any(r > 2048 for r in ranges) and 2048 in ranges and 2049 in ranges and 1 in ranges
    assert {len(c['cut']) for c in X.HEAD_CASES.values()} >= {0, 1, 3} and {c['gs'] for c in X.HEAD_CASES.values()} == {1.0, 0.5}
    assert {c['B'] * c['T'] for c in X.HEAD_CASES.values()} == {2, 51, 65}
    one_pass = 2048 * 256
    assert max(X.SUMSQ_N) // 4 > one_pass and any(n & 3 for n in X.SUMSQ_N) and max(X.DROPOUT_N) // 8 > one_pass
    assert max(c['n'] for c in X.ADAMW_CASES.values()) > one_pass
    assert any(c['n_decay'] % 256 and 0 < c['n_decay'] < c['n'] for c in X.ADAMW_CASES.values())
    assert {c['clip'] for c in X.ADAMW_CASES.values()} == {'none', 'above', 'below', 'nosumsq', 'maxnorm0'}
    assert {c['step0'] for c in X.ADAMW_CASES.values()} == {1, 100000} and not all(c['w16'] for c in X.ADAMW_CASES.values())
    unnamed = False
    for n in X.EMB_CASES:
        c = X.emb_case(n)
        ids = c['ids'][c['valid']]
        if EMB_KIND[n] == 'unique':
            assert len(torch.unique(ids)) == len(ids)
        unnamed |= len(torch.unique(ids)) < c['V']
    assert unnamed


EMB_KIND = {n: c['ids'] for n, c in X.EMB_CASES.items()}


@pytest.mark.parametrize('name', list(X.HEAD_CASES))
def test_no_nll_is_zero_and_labels_are_mixed(name):
    c, ref, model = X.head_expect(name)
    lab = c['labels'][:, 1:]
    live = (lab >= 0) & (lab < c['V'])
    assert ((ref['nll'] != 0) == live).all() and ((model['nll'] != 0) == live).all()
    if c.get('all_ignored'):
        assert ref['count'] == 0 and (ref['dlogits'] == 0).all()
        return
    assert live.any() and ((lab == -100).any() or c['R'] <= 2) and (ref['nll'].max() > 40 or c['R'] <= 2)
    if c['B'] > 1:
        assert (c['labels'][c['B'] - 1] == -100).all()
    if c['T'] > 3:
        assert (c['labels'] >= c['V']).any()
    if c['R'] > 2:
        assert c['shifted'].any()


def test_every_mask_has_kept_and_dropped_cells():
    for n, c in X.LN_CASES.items():
        if c['p'] > 0:
            k = X.ln_keep(X.ln_case(n, 'zero'))
            assert k.any() and (~k).any(), n
    for n, c in X.EMB_CASES.items():
        if c['p'] > 0 and c['N'] * c['d'] >= 64:
            cc = X.emb_case(n)
            k = X.flat_keep(cc['seed'], cc['site'], (c['N'], c['d']), c['p'], form32=False)
            assert k.any() and (~k).any(), n
    for n, c in X.SIN_CASES.items():
        if c['p'] > 0 and c['M'] > 1:
            kept, dropped = X.sin_mask_counts(n)
            assert kept and dropped, n
    for n in X.DROPOUT_N:
        for p in X.DROPOUT_P:
            if n > 8:
                k = X.dropout_case(n, p)[4]
                assert k.any() and (~k).any()


# ---------------------------------------------------------------------------------------------------------------- the bounds have teeth
def _leaves(got, ref, a, b, groups=None):
    return X.groups_worst(got, ref, a, b, groups)[0] > 1.0


def test_planted_layernorm_faults_leave_their_bounds():
    # variance as E[x^2] - mu^2 in float32 on the offset-mean rows -> rstd
    c, z, ref, model = X.ln_expect('ln_d512_n63', 'offset')
    bad = X.ln_stats(z, c['gamma'], c['beta'], F32, fault='var_e2')
    assert _leaves(bad['rstd'].double(), ref['rstd'], A_F32, B_LN['rstd'], c['groups'])
    assert not _leaves(model['rstd'], ref['rstd'], A_F32, B_LN['rstd'], c['groups'])
    # gamma shifted by one column -> y
    bad = X.ln_stats(z, c['gamma'], c['beta'], F32, fault='gamma_shift')
    assert _leaves(X.bf(bad['y']), ref['y'], A_BF16, B_LN['y'], c['groups'])
    assert not _leaves(X.bf(model['y']), ref['y'], A_BF16, B_LN['y'], c['groups'])
    # the last chunk of a d = 520 row left out of the statistics -> mean, rstd
    c, z, ref, model = X.ln_expect('ln_d520_n65', 'offset')
    bad = X.ln_stats(z, c['gamma'], c['beta'], F32, fault='drop_last_chunk')
    assert _leaves(bad['mean'].double(), ref['mean'], A_F32, B_LN['mean'], c['groups'])
    assert _leaves(bad['rstd'].double(), ref['rstd'], A_F32, B_LN['rstd'], c['groups'])
    # the mask of site + 1 -> the stored z (compared bit for bit) and dx
    name = next(n for n, r in X.LN_CASES.items() if r['p'] == 0.5)
    c, z, ref, model = X.ln_expect(name, 'zero')
    assert not torch.equal(X.ln_z_exact(c, site_fault=True), z)
    st = X.ln_stats(z, c['gamma'], c['beta'], F32)
    bad = X.ln_bwd(c, z, st, F32, p=c['p'], site_fault=True)
    assert _leaves(X.bf(bad['dx']), ref['dx'], A_BF16, B_LN['dx'], c['groups'])
    assert not _leaves(X.bf(model['dx']), ref['dx'], A_BF16, B_LN['dx'], c['groups'])


def test_planted_mask_faults_leave_their_bounds():
    name = 'emb_d520_n257_rand'
    c = X.emb_case(name)
    ref = X.emb_ref(c, F64)
    bad = X.emb_ref(c, F32, site_fault=True)
    assert _leaves(X.bf(bad['out']), ref['out'], A_EMB['out'], B_EMB['out']) and _leaves(bad['dE'], ref['dE'], A_EMB['dE'], B_EMB['dE'])
    good = X.emb_ref(c, F32)
    assert not _leaves(X.bf(good['out']), ref['out'], A_EMB['out'], B_EMB['out']) and not _leaves(good['dE'], ref['dE'], A_EMB['dE'], B_EMB['dE'])
    # the cosine half's mask indexed without the d / 2 offset
    for n, cc in X.SIN_CASES.items():
        if cc['p'] > 0 and cc['M'] > 1:
            ref = X.sin_ref(n, F64)
            assert _leaves(X.bf(X.sin_ref(n, F32, fault='cos_no_half')), ref, A_EMB['sin'], B_EMB['sin']), n
            assert not _leaves(X.bf(X.sin_ref(n, F32)), ref, A_EMB['sin'], B_EMB['sin']), n


def test_planted_head_faults_leave_their_bounds():
    for name in ('h_v1190', 'h_v5000_c1000'):          # a tail lse without its last column (of 190, of 4000): lse and nll
        c, ref, model = X.head_expect(name)
        bad = X.head_ref(c, F32, fault='tail_short')
        assert _leaves(bad['lse'], ref['lse'], A_HEAD['lse'], B_HEAD['lse'], c['groups']), name
        assert _leaves(bad['nll'], ref['nll'], A_HEAD['nll'], B_HEAD['nll']) or name != 'h_v1190', name      # one of 4000 columns: under nll's bound
        assert not _leaves(model['nll'], ref['nll'], A_HEAD['nll'], B_HEAD['nll'])
        assert not _leaves(model['lse'], ref['lse'], A_HEAD['lse'], B_HEAD['lse'], c['groups'])
    c, ref, model = X.head_expect('h_v500_c3')
    bad = X.head_ref(c, F32, fault='cluster_col')
    assert _leaves(bad['nll'], ref['nll'], A_HEAD['nll'], B_HEAD['nll'])
    assert not _leaves(model['nll'], ref['nll'], A_HEAD['nll'], B_HEAD['nll'])
    # lo omitted under the 2^-16 bound; hi + lo meets it; hi alone meets the bf16 bound
    for name in X.HEAD_CASES:
        c, ref, model = X.head_expect(name)
        if ref['count'] == 0:
            continue
        hi, lo = X.split_terms(model['dlogits'])
        # only elements above a third of max|ref| can show the missing term (2^-9 |d| against b max|ref|): the cases with several rows
        assert _leaves(hi, ref['dlogits'], A_SPLIT, B_HEAD['dlogits']) or c['R'] <= 2, name
        assert not _leaves(hi + lo, ref['dlogits'], A_SPLIT, B_HEAD['dlogits']), name
        assert not _leaves(hi, ref['dlogits'], A_BF16, B_HEAD['dlogits']), name


def test_planted_optimiser_faults_leave_their_bounds():
    def chain_leaves(name, fault, i):
        c = X.adamw_case(name)
        ref, bad, good = X.adamw_chain(c, F64), X.adamw_chain(c, F32, fault), X.adamw_chain(c, F32)
        q = 'pmv'[i]
        assert not any(_leaves(good[k][i], ref[k][i], A_F32, B_OPT[q]) for k in range(X.ADAMW_STEPS))
        return c, ref, bad, _leaves(bad[0][i], ref[0][i], A_F32, B_OPT[q])
    # weight decay applied at i <= n_decay: element n_decay moves
    c, ref, bad, out = chain_leaves('aw_n10007_above', 'decay_le', 0)
    assert out and worst(bad[0][0][c['n_decay']:c['n_decay'] + 1], ref[0][0][c['n_decay']:c['n_decay'] + 1], A_F32, B_OPT['p'])[0] > 1
    # bias correction of step - 1, planted at step 2 on the state the sound model left after step 1
    c = X.adamw_case('aw_n255_above')
    ref, good = X.adamw_chain(c, F64), X.adamw_chain(c, F32)
    bad = X.adamw_step_ref(c, tuple(t.float() for t in good[0]), 1, F32, 'bias_step')
    assert _leaves(bad[0].double(), ref[1][0], A_F32, B_OPT['p']) and not _leaves(good[1][0], ref[1][0], A_F32, B_OPT['p'])
    # the clip coefficient without grad_scale (grad_scale = 0.5, norm above max_norm)
    assert chain_leaves('aw_n255_above', 'clip_no_gs', 1)[3]
    # a sum of squares that misses its n & 3 tail
    x = X.sumsq_case(5, False)
    assert _leaves(X.sumsq_ref(x[:4], F32), X.sumsq_ref(x, F64), A_F32, B_OPT['sumsq']) and not _leaves(X.sumsq_ref(x, F32), X.sumsq_ref(x, F64), A_F32, B_OPT['sumsq'])
