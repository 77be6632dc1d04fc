"""Indexed rings on the CPU (no GPU): the owner table's bookkeeping against whole-ring copies in the numpy model of
tests/beam_owner_ref.py, the argument checks of the two new entries through the library, and the refusals of `generate(beam_rings=)`
where it raises before a device is touched (the harness of tests/golden/make_generate_dispatch.py: the unbound methods on a stub
`self`, recorders in place of the decoders and the searches)."""
import importlib.util
import os

import numpy as np
import pytest

from symbolic_music_generation_amd import _lib, generate
from tests import beam_owner_ref as R

M, TP = 32, 4
EUNSUPPORTED = -2


def _srcs(rng, Bs, nb, steps, still_after_wrap):
    """random source rows per step; items stay put with probability 0.4, and (still_after_wrap) in the two steps that write slots 0 and
    1 of a wrapped ring nothing moves at all"""
    out, t = [], TP - 1
    for _ in range(steps):
        src = np.arange(Bs * nb)
        for b in range(Bs):
            if rng.random() >= 0.4:
                src[b * nb:(b + 1) * nb] = b * nb + rng.integers(0, nb, nb)
        if still_after_wrap and t + 1 >= M and (t + 1) % M in (0, 1):
            src = np.arange(Bs * nb)
        out.append(src)
        t += 1
    return out


@pytest.mark.parametrize('nb', [2, 3, 16])
def test_gather_by_owner_equals_copying_the_rings(nb):
    """over more than 2 M steps every row has the same effective ring at every step, whichever way the rings are kept; the model that
    marks only the items it moved does not, once nothing moves directly after a wrap"""
    broken = 0
    for seed in range(6):
        srcs = _srcs(np.random.default_rng(100 * nb + seed), 2, nb, 2 * M + 20, still_after_wrap=seed % 2 == 0)
        moves = sum(int((s != np.arange(len(s))).any()) for s in srcs)
        assert 0 < moves < len(srcs)                                   # both kinds of step occur
        for t, copied, indexed in R.run(srcs, nb, M, TP):
            assert np.array_equal(copied, indexed), (nb, seed, t)
        if seed % 2 == 0:
            broken += any(not np.array_equal(c, i) for _, c, i in R.run(srcs, nb, M, TP, mark='moved'))
    assert broken == 3, 'the unmoved steps after the wrap must bite a model without the unconditional mark'


def test_stale_owner_after_a_wrap_is_what_the_unconditional_mark_removes():
    """one swap, then nothing moves: row 0 inherited every slot of row 1's table, the never-written ones and -- at the wrap -- the
    prompt's slot 0 among them, and writes each into its own ring; the first unmoved step already reads a stale owner"""
    srcs = [np.array([1, 0])] + [np.arange(2)] * M
    steps = list(R.run(srcs, 2, M, TP))
    assert all(np.array_equal(c, i) for _, c, i in steps)
    bad = [t for t, c, i in R.run(srcs, 2, M, TP, mark='moved') if not np.array_equal(c, i)]
    assert bad[0] == TP + 1 and M in bad and M + 1 in bad              # (position M lands on slot 0, which row 0 held from row 1)


def test_identity_and_follow_shapes():
    own = R.identity(6, 3, M)
    assert own.dtype == np.uint8 and own[:, 0].tolist() == [0, 1, 2, 0, 1, 2]
    new = R.follow(own, 3, np.array([1, 0, 2, 3, 4, 5]), np.array([1, 0]), M - 1)
    assert new[0, 1:].tolist() == [1] * (M - 1) and new[1, 1:].tolist() == [0] * (M - 1)
    assert new[:, 0].tolist() == [0, 1, 2, 0, 1, 2]                    # the mark at (t + 1) % M = 0, in the unmoved item too


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_new_entries_refuse_bad_arguments_before_any_launch():
    decl, L = _lib.declared_functions(), _lib.lib()
    assert len(decl['mxl_beam_owner_follow'][1]) == 8 and len(decl['mxl_relattn_decode_owned'][1]) == 19
    Pt = 4096                                                          # stands for a device pointer: nothing is followed before a launch
    fol = dict(owner=Pt, Bs=2, nb=3, M=32, beam_idx=Pt, moved=Pt, t_dev=Pt)
    for bad in (dict(owner=None), dict(beam_idx=None), dict(moved=None), dict(t_dev=None), dict(nb=0), dict(nb=17), dict(M=40), dict(M=0),
                dict(Bs=0), dict(Bs=65536), dict(owner=Pt + 8)):
        assert L.mxl_beam_owner_follow(*{**fol, **bad}.values(), None) == -1, bad
    att = dict(qkv=Pt, kc=Pt, vc=Pt, owner=Pt, nb=3, bd=Pt, rwb=Pt, out=Pt, t_dev=Pt, B=6, H=2, dh=64, M=96, scale=0.125, pieces=1, ws=None,
               arrived=None, live=None)
    for bad in (dict(qkv=None), dict(kc=None), dict(vc=None), dict(owner=None), dict(bd=None), dict(rwb=None), dict(out=None),
                dict(t_dev=None), dict(nb=0), dict(nb=17), dict(M=100), dict(B=7), dict(B=0), dict(pieces=0), dict(pieces=9),
                dict(pieces=3), dict(M=16128), dict(owner=Pt + 4)):
        assert L.mxl_relattn_decode_owned(*{**att, **bad}.values(), None) == -1, bad
    assert L.mxl_relattn_decode_owned(*{**att, 'dh': 24}.values(), None) == EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- generate(beam_rings=)
def _maker():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'make_generate_dispatch.py')
    spec = importlib.util.spec_from_file_location('make_generate_dispatch', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def harness():
    mk = _maker()
    return mk, mk.fixtures()


def _call(harness, model='xl', **kw):
    """`generate` on the stub model -> (name of the search reached, its beam_rings) or raises what generate raises"""
    mk, fx = harness
    cls, make = fx['models'][model]
    seen = {}
    names = ('beam_search_device', 'group_beam_search_device', 'beam_sample_device')
    with mk.patched():
        saved = {n: getattr(generate, n) for n in names}
        for name in names:
            def rec(*a, _name=name, **k):
                seen.update(name=_name, beam_rings=k.get('beam_rings'))
                raise mk.Reached(_name)
            setattr(generate, name, rec)
        mk._Decoder.built = []
        try:
            cls.generate(make(), input_ids=fx['prompt'], max_length=mk.MAX_LENGTH, **kw)
        except mk.Reached as r:
            seen.setdefault('name', str(r).split(' ')[0])
        finally:
            for n, f in saved.items():
                setattr(generate, n, f)
    return seen.get('name'), seen.get('beam_rings')


BEAM = dict(num_beams=2, eos_token_id=1, pad_token_id=0)
GROUP = dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.5, eos_token_id=1, pad_token_id=0)
SAMPLE = dict(num_beams=2, do_sample=True, renormalize_logits=True, eos_token_id=1, pad_token_id=0)


def test_beam_rings_reaches_the_device_searches(harness, monkeypatch):
    monkeypatch.delenv('MXL_BEAM_RINGS', raising=False)
    monkeypatch.setenv('MXL_GROUP_BEAM_DEVICE', '1')
    for arm, name in ((BEAM, 'beam_search_device'), (GROUP, 'group_beam_search_device'),
                      (dict(SAMPLE, device_scorer=True), 'beam_sample_device')):
        assert _call(harness, **arm) == (name, 'copied')
        assert _call(harness, beam_rings='copied', **arm) == (name, 'copied')
        assert _call(harness, beam_rings='indexed', **arm) == (name, 'indexed')
        monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed')                # the default of a call that does not pass the keyword
        assert _call(harness, **arm) == (name, 'indexed')
        assert _call(harness, beam_rings='copied', **arm) == (name, 'copied')
        monkeypatch.delenv('MXL_BEAM_RINGS')


def test_beam_rings_refusals(harness, monkeypatch):
    monkeypatch.delenv('MXL_BEAM_RINGS', raising=False)
    with pytest.raises(ValueError, match="beam_rings='shared'"):
        _call(harness, beam_rings='shared', **BEAM)
    elsewhere = [dict(), dict(do_sample=True), dict(penalty_alpha=0.6, top_k=4), dict(num_beams=17), SAMPLE, dict(BEAM, kv_cache_dtype='fp8'),
                 dict(kv_cache_dtype='fp8'), dict(GROUP)]              # (group beam without a rule keeps the host scorer)
    for arm in elsewhere:
        with pytest.raises(ValueError, match="beam_rings='indexed' serves|kv_cache_dtype='fp8' is not supported"):
            _call(harness, beam_rings='indexed', **arm)
    monkeypatch.setenv('MXL_BEAM_HOST', '1')
    with pytest.raises(ValueError, match="beam_rings='indexed' serves"):
        _call(harness, beam_rings='indexed', **BEAM)
    monkeypatch.delenv('MXL_BEAM_HOST')
    # the environment's default is ignored where 'indexed' does not apply: these calls run as they always did
    monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed')
    for arm, name in ((dict(), 'greedy'), (dict(do_sample=True), 'sample'), (dict(penalty_alpha=0.6, top_k=4), 'contrastive_search_device'),
                      (dict(num_beams=17), 'beam_search'), (SAMPLE, 'beam_search')):
        assert _call(harness, **arm)[0] == name, arm
    monkeypatch.delenv('MXL_BEAM_RINGS')
    # the Reformer refuses it as it refuses every option it does not cover
    for arm in (dict(), BEAM):
        with pytest.raises(NotImplementedError, match="generation options not covered: \\['beam_rings'\\]"):
            _call(harness, model='rf', beam_rings='indexed', **arm)
