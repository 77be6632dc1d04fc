"""The samplers' random draw -- sample_kernel / sample_step_kernel (the LDS sort of csrc/decode.hip) and sample_large_kernel (the
bisections of csrc/sample_large.hip) -- token for token against the host statement of oracle/sampler_cases.py.

1. The stream.  On inputs where the kernels' arithmetic is exact (equal scores: p = 1 / N with N a power of two under the sort sampler,
   weights of 2^31 and an integer u * tot under the bisection sampler) the token IS the top bits of the hash word, so every
   (row, counter, seed) of the sweep -- 70 rows, counters either side of 2^32 and at 2^64 - 1, seeds with and without a high word, the
   two decoder lanes -- must give exactly the token of the integer model: no tolerance.  The same at the counters where j = h2 >> 8
   sits at an end of its scale (j <= 3, j >= 2^24 - 4), there also on a non-uniform row, and through the fused step with its counter
   advance.
2. The draw.  On the case table (real distributions, every warper, both samplers, all three paths of the sort sampler) the kept support
   must equal the float64 reference's exactly and out_probs must agree within 2e-5; a DECIDED draw -- u further than delta from every
   cumulative boundary of the reference -- must be the reference's token, an undecided one must lie within the band.

delta = 4 x the largest gap between the float64 cumulative sums and the rounded CPU model of each kernel's own sums over the case
table (the rule of oracle/kernel_cases.py; measured on the CPU, re-measured by tests/test_sampler_cases_cpu.py):

    sort sampler        1.40e-6   s_v1190_ninf_rp13     -> DELTA_SORT  5.6e-6
    bisection sampler   4.18e-7   l_v32773_s4_full      -> DELTA_LARGE 1.7e-6

At most CAP = 2 % of a case's draws are undecided; that is a property of the inputs which the CPU test asserts (largest: 1.76 %,
s_v2048_full).  The counts per case of a run on the MI355X are in profiles/sampler_cases.txt.
"""
import numpy as np
import pytest
import torch

from oracle import sampler_cases as S

pytestmark = pytest.mark.gpu

DELTA_SORT, DELTA_LARGE = 5.6e-6, 1.7e-6
CAP = 0.02
PROBS_TOL = 2e-5


def _signed(ctr):
    ctr &= S.M64
    return ctr - (1 << 64) if ctr >= (1 << 63) else ctr


def _draw(dev, monkeypatch, scores, ctrs, seed, *, large, hist=None, probs=None, **kw):
    """one ops.sample launch per counter on scores (B, V) -> tokens (len(ctrs), B) on the host"""
    from symbolic_music_generation_amd import ops
    B, V = scores.shape
    assert large or V <= 2048
    monkeypatch.setenv('MXL_SAMPLE_LARGE', '1' if large else '0')
    th = 1 if hist is None else hist.shape[1]
    ids = torch.zeros(B, th + 8, dtype=torch.int64, device=dev)
    if hist is not None:
        ids[:, :th] = hist.to(dev)
    t = torch.full((1,), th - 1, device=dev, dtype=torch.int32)
    rng = torch.zeros(1, device=dev, dtype=torch.int64)
    out = []
    for ctr in ctrs:
        rng.fill_(_signed(int(ctr)))
        ops.sample(scores, ids, t, rng, seed, do_sample=True, out_probs=probs, **kw)
        out.append(ids[:, th].clone())
    tok = torch.stack(out).cpu().numpy()
    assert int(t.item()) == th - 1 and _signed(int(rng.item())) == _signed(int(ctrs[-1]))      # the unfused sampler advances nothing
    return tok


EXACT = S.exact_cases()


@pytest.mark.parametrize('name', list(EXACT))
def test_stream_pinned_bit_for_bit(dev, name, monkeypatch):
    """the sweep: one launch per (counter, seed) with all 70 rows; every token equals the integer model's"""
    x = EXACT[name]
    scores = x['row'].to(dev).expand(S.SWEEP_B, x['V']).contiguous()
    rows = np.arange(S.SWEEP_B)
    bad = []
    for seed in S.SWEEP_SEEDS:
        tok = _draw(dev, monkeypatch, scores, S.SWEEP_CTRS, seed, large=x['large'], top_k=x['top_k'])
        for i, ctr in enumerate(S.SWEEP_CTRS):
            want = x['token'](S.sampler_h2(seed, rows, [ctr] * S.SWEEP_B))
            bad += [(seed, ctr, int(r), int(tok[i, r]), int(want[r])) for r in np.nonzero(tok[i] != want)[0]]
    print(f'sampler stream {name}: {len(S.SWEEP_SEEDS) * len(S.SWEEP_CTRS) * S.SWEEP_B} draws, {len(bad)} mismatches')
    assert not bad, bad[:8]


def test_stream_at_the_ends_of_the_scale(dev, monkeypatch):
    """the counters (found on the host model) at which a row draws j <= 3 or j >= 2^24 - 4: the exact inputs still give the model's
    token in every row, and on a non-uniform full-support row the token is the first entry of the sampler's order (small j) or the last
    entry with a non-zero probability (large j) -- under the sort sampler through the fallback, the float32 running sum ending below
    u; under the bisection sampler next to the clamp of the target.  The band rule of the case tests holds there as well."""
    lo, hi = S.end_counters()
    assert lo and hi
    seed, nrows = 77, 4
    rows = np.arange(nrows)
    ctrs = [c for _, c, _ in lo + hi]
    bad = []
    for name, x in EXACT.items():
        tok = _draw(dev, monkeypatch, x['row'].to(dev).expand(nrows, x['V']).contiguous(), ctrs, seed, large=x['large'], top_k=x['top_k'])
        for i, ctr in enumerate(ctrs):
            want = x['token'](S.sampler_h2(seed, rows, [ctr] * nrows))
            bad += [(name, ctr, int(r), int(tok[i, r]), int(want[r])) for r in np.nonzero(tok[i] != want)[0]]
    row = S.end_row()
    scores = row.to(dev).expand(nrows, row.numel()).contiguous()
    for large, delta in ((False, DELTA_SORT), (True, DELTA_LARGE)):
        ref = S.row_ref(dict(large=large, V=row.numel(), k=0, p=1.0, typ=1.0, temp=1.0, rp=1.0), row.numpy(), [])
        assert ref['keep'].all() and ref['p'][ref['order'][0]] > 8 / S.TWO24 and ref['p'][ref['order'][-1]] > 0
        tok = _draw(dev, monkeypatch, scores, ctrs, seed, large=large)
        u = S.sampler_u(seed, rows[None, :], S._u64(ctrs)[:, None])
        _, _, off = S.judge(tok.ravel(), ref, u.ravel(), delta)
        bad += [('band', large, int(i)) for i in off]
        for i, (r, ctr, j) in enumerate(lo + hi):
            want = ref['order'][0] if j < 4 else ref['order'][-1]
            print(f'sampler ends large={large}: row {r} ctr {ctr} j {j} -> token {tok[i, r]} (expected {want})')
            if tok[i, r] != want:
                bad.append(('end', large, r, ctr, j, int(tok[i, r]), int(want)))
    assert not bad, bad[:8]


def test_fused_step_draws_and_advances(dev):
    """ops.sample_step with the rules off, three consecutive steps from rng_ctr = 2^32 - 2: every row's token at step s is the model's
    at ctr0 + s (no row reads the counter after the last arrival has bumped it), and the counters end at ctr0 + 3, t0 + 3 and 0"""
    from symbolic_music_generation_amd import ops
    x = EXACT['sort_bitonic_v2048']
    B, V, d, t0, ctr0, seed = S.SWEEP_B, x['V'], 64, 1, (1 << 32) - 2, (1 << 32) + 77
    scores = x['row'].to(dev).expand(B, V).contiguous()
    E = torch.randn(V, d, device=dev).to(torch.bfloat16)
    emb = torch.zeros(B, d, device=dev, dtype=torch.bfloat16)
    ids = torch.zeros(B, 8, dtype=torch.int64, device=dev)
    t = torch.full((1,), t0, device=dev, dtype=torch.int32)
    rng = torch.full((1,), ctr0, device=dev, dtype=torch.int64)
    counter = torch.zeros(1, device=dev, dtype=torch.int32)
    for s in range(3):
        ops.sample_step(scores, V, ids, t, rng, seed, E, emb, 1.0, counter, do_sample=True)
    torch.cuda.synchronize()
    got = ids.cpu().numpy()
    for s in range(3):
        want = x['token'](S.sampler_h2(seed, np.arange(B), [ctr0 + s] * B))
        assert (got[:, t0 + 1 + s] == want).all(), (s, np.nonzero(got[:, t0 + 1 + s] != want)[0][:8])
    assert int(rng.item()) == ctr0 + 3 and int(t.item()) == t0 + 3 and int(counter.item()) == 0
    assert torch.equal(emb, E[ids[:, t0 + 3]])              # and the last step's embedding rows (scale 1) are the drawn tokens'


@pytest.mark.parametrize('name', [c['name'] for c in S.CASES])
def test_draws_token_for_token(dev, name, monkeypatch):
    """a case of the table: 4 launches (the counters of CASE_CTRS) of B rows, 4 distinct rows repeated"""
    c = S.CASE[name]
    delta = DELTA_LARGE if c['large'] else DELTA_SORT
    rows, hist = S.case_inputs(c)
    reps = c['B'] // S.N_ROWS
    scores = rows.repeat(reps, 1).to(dev)
    probs = torch.zeros(c['B'], c['V'], device=dev)
    tok = _draw(dev, monkeypatch, scores, S.CASE_CTRS, S.CASE_SEED, large=c['large'], hist=hist.repeat(reps, 1), probs=probs,
                top_k=c['k'], top_p=c['p'], temperature=c['temp'], repetition_penalty=c['rp'], typical_p=c['typ'])
    refs = S.case_ref(name)
    got = probs.cpu().numpy().reshape(reps, S.N_ROWS, c['V'])             # (the last launch's; the support does not depend on u)
    keep, p = np.stack([r['keep'] for r in refs]), np.stack([r['p'] for r in refs])
    wrong = (got > 0) != keep[None]
    assert not wrong.any(), (name, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    err = float(np.abs(got - p[None]).max())
    assert err < PROBS_TOL, (name, err)
    nd, nu, bad = S.judge_case(name, tok, delta)
    print(f'sampler {name}: decided {nd} undecided {nu} ({nu / (nd + nu):.2%}) mismatches {len(bad)}  max |out_probs - ref| {err:.2e}')
    assert not bad, bad[:8]
