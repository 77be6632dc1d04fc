"""mxl_beam_sample_draw at kernel level against tests/beam_sample_ref.py: the warped rows (`out_warped`) element-wise against the
float64 warp, and the drawn set of every item against the float64 Gumbel-top-k -- exactly where the reference decides, within the band
where it does not.  The tolerances are the module's DELTA_W / DELTA_Z, computed on the CPU.  Fails without the feature: the entry does
not exist."""
import numpy as np
import pytest
import torch

from tests import beam_sample_ref as R
from tests.beam_ref import MXL_EINVAL

pytestmark = pytest.mark.gpu
NEG = float('-inf')
FILL = 7.0


def _signed(ctr):
    return ctr - (1 << 64) if ctr >= (1 << 63) else ctr


def _launch(dev, c, ref, out_warped=True):
    from symbolic_music_generation_amd import ops
    rows, V = ref['w'].shape
    logp, scores = ref['logp'].to(dev), ref['scores'].to(dev)
    rng = torch.tensor([_signed(ref['ctr'])], dtype=torch.int64, device=dev)
    drawn = torch.full((rows, logp.shape[1]), FILL, device=dev)
    ow = torch.full((rows, V), FILL, device=dev) if out_warped else None
    w = c['warp']
    ops.beam_sample_draw(logp, V, scores, c['nb'], rng, R.CASE_SEED, drawn, top_k=w['k'], top_p=w['p'], temperature=w['temp'],
                         typical_p=w['typ'], out_warped=ow)
    assert torch.equal(logp.cpu().view(torch.int32), ref['logp'].view(torch.int32))         # the inputs are read only
    assert torch.equal(scores.cpu().view(torch.int32), ref['scores'].view(torch.int32))
    assert _signed(ref['ctr']) == int(rng)                                                    # the counter is not advanced
    return drawn.cpu(), None if ow is None else ow.cpu()


@pytest.mark.parametrize('name', [c['name'] for c in R.CASES])
def test_draw_against_the_float64_reference(dev, name):
    c, ref = R.CASE[name], R.case_ref(name)
    nb, V = c['nb'], c['V']
    drawn, ow = _launch(dev, c, ref)
    again, ow2 = _launch(dev, c, ref)
    assert torch.equal(drawn.view(torch.int32), again.view(torch.int32)) and torch.equal(ow.view(torch.int32), ow2.view(torch.int32))
    alone, _ = _launch(dev, c, ref, out_warped=False)                                         # the hook changes nothing
    assert torch.equal(drawn.view(torch.int32), alone.view(torch.int32))

    # out_warped: the reference's support, its values, every row normalised; no NaN, nothing but -inf outside the support
    got = ow.numpy().astype(np.float64)
    assert not np.isnan(got).any() and (got[~np.isfinite(got)] == NEG).all()
    sure = ref['margin'] > R.DELTA_W
    fin = np.isfinite(ref['w'])
    assert np.array_equal(np.isfinite(got)[sure], fin[sure])
    both = fin & np.isfinite(got)
    gap = np.abs(got[both] - ref['w'][both]).max()
    has = np.isfinite(got).any(1)
    lse = np.abs(np.log(np.exp(got[has]).sum(1))).max()
    print(name, 'largest |w - ref|', gap, 'largest |logsumexp|', lse, 'delta_w', R.DELTA_W)
    assert gap <= R.DELTA_W and lse <= R.DELTA_W
    assert not np.isfinite(got[~ref['live']]).any()                                           # a dead row contributes nothing

    # drawn: out_warped bit for bit at its finite entries, -inf elsewhere in the V columns, the columns beyond untouched
    assert (drawn[:, V:] == FILL).all() and not torch.isnan(drawn).any()
    d = drawn[:, :V]
    at = torch.isfinite(d)
    assert torch.equal(d[at].view(torch.int32), ow[at].view(torch.int32)) and (d[~at] == NEG).all()

    # the drawn sets
    flat = at.view(c['Bs'], nb * V)
    undecided = 0
    for b, it in enumerate(ref['items']):
        verdict = R.judge_item(it, flat[b].nonzero().view(-1).tolist(), nb)
        assert verdict is None, (name, b, verdict)
        undecided += not it['decided']
    print(name, 'undecided items', undecided, 'of', len(ref['items']))


def test_another_counter_or_seed_draws_another_set(dev):
    from symbolic_music_generation_amd import ops
    c, ref = R.CASE['vm_none'], R.case_ref('vm_none')
    logp, scores = ref['logp'].to(dev), ref['scores'].to(dev)
    sets = []
    for seed, ctr in ((R.CASE_SEED, 5), (R.CASE_SEED, 5 + (1 << 32)), (R.CASE_SEED + (1 << 32), 5), (R.CASE_SEED + 1, 5), (R.CASE_SEED, 6)):
        drawn = torch.full(tuple(logp.shape), FILL, device=dev)
        ops.beam_sample_draw(logp, c['V'], scores, c['nb'], torch.tensor([ctr], device=dev), seed, drawn)
        got = torch.isfinite(drawn[:, :c['V']]).cpu()
        words = R.cand_word(seed, ctr, np.arange(logp.shape[0])[:, None], np.arange(c['V'])[None, :])
        for b, it in enumerate(R.draw_ref(ref['w'], words, c['nb'])):
            assert R.judge_item(it, got.view(c['Bs'], -1)[b].nonzero().view(-1).tolist(), c['nb']) is None, (seed, ctr, b)
        sets.append(got)
    assert all(not torch.equal(a, b) for i, a in enumerate(sets) for b in sets[:i])


def test_argument_errors(dev):
    from symbolic_music_generation_amd._lib import MusicXLError, lib
    from symbolic_music_generation_amd import ops
    L = lib()
    f = torch.zeros(32, 16, device=dev)
    g = torch.zeros(32, 16, device=dev)
    s = torch.zeros(32, device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    P = lambda t: t.data_ptr()

    def draw(V=16, nb=2, Bs=2, ldl=16, drawn=P(g), ctr_=P(ctr), temperature=1.0, top_p=1.0, typical_p=1.0, top_k=0):
        return L.mxl_beam_sample_draw(P(f), ldl, V, P(s), Bs, nb, ctr_, 77, top_k, top_p, temperature, typical_p, drawn, None, None)
    assert draw(V=1) == MXL_EINVAL and draw(V=2049, ldl=4096) == MXL_EINVAL and draw(ldl=8) == MXL_EINVAL
    assert draw(nb=1) == MXL_EINVAL and draw(nb=17, Bs=1) == MXL_EINVAL and draw(Bs=0) == MXL_EINVAL
    assert draw(drawn=None) == MXL_EINVAL and draw(drawn=P(f)) == MXL_EINVAL and draw(ctr_=None) == MXL_EINVAL
    assert draw(temperature=0.0) == MXL_EINVAL and draw(top_p=0.0) == MXL_EINVAL and draw(typical_p=0.0) == MXL_EINVAL
    assert draw(top_k=-1) == MXL_EINVAL
    torch.cuda.synchronize()
    assert not g.any() and not f.any()                                                        # nothing was launched
    with pytest.raises(MusicXLError, match='beyond the 2048'):
        ops.beam_sample_draw(torch.zeros(4, 2049, device=dev), 2049, s[:4], 2, ctr, 77, torch.zeros(4, 2049, device=dev))
