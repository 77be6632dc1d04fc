"""Shared rings under contrastive search on the CPU (no GPU): the table of generate.resolve_contrastive_rings, the refusals of
`generate(contrastive_rings=)` where it raises before a device is touched (the harness of tests/golden/make_generate_dispatch.py: the
unbound methods on a stub `self`, recorders in place of the decoders and the searches), what a call without the keyword builds, and the
argument checks of the new entries through the library."""
import importlib.util
import os

import pytest

from symbolic_music_generation_amd import _lib, generate

EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------- the resolve function
def test_resolve_table(monkeypatch):
    R = generate.resolve_contrastive_rings
    monkeypatch.delenv('MXL_CONTRASTIVE_RINGS', raising=False)
    assert generate.CONTRASTIVE_RINGS == ('copied', 'shared')
    for applies in (False, True):
        assert R(None, applies) == 'copied' and R('copied', applies) == 'copied'
    assert R('shared', True) == 'shared'
    with pytest.raises(ValueError, match="contrastive_rings='shared' serves contrastive search"):
        R('shared', False)
    for bad in ('indexed', 'Shared', '', 'fp8'):
        for applies in (False, True):
            with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
                R(bad, applies)
    # the environment sets the default of a call that names none, and is ignored where the mode does not apply
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'shared')
    assert R(None, True) == 'shared' and R(None, False) == 'copied' and R('copied', True) == 'copied'
    with pytest.raises(ValueError, match='serves contrastive search'):
        R('shared', False)
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'copied')
    assert R(None, True) == 'copied' and R('shared', True) == 'shared'
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', '')
    assert R(None, True) == 'copied'
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'both')
    with pytest.raises(ValueError, match="contrastive_rings='both'"):
        R(None, False)


# ---------------------------------------------------------------------------------------------------------------- generate(contrastive_rings=)
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
    """`generate` on the stub model -> (name of the entry reached, the keywords its decoders were built with, the contrastive_rings the
    device search was handed) or raises what generate raises"""
    mk, fx = harness
    cls, make = fx['models'][model]
    seen, built = {}, []
    with mk.patched():
        stub, search = generate.XLDecoder, generate.contrastive_search_device

        class Dec(stub):
            def __init__(self, engine, batch, max_total_len, *a, **k):
                super().__init__(engine, batch, max_total_len, *a, **k)
                built.append((batch, {n: v for n, v in k.items() if n != 'seed'}))

        def rec(*a, **k):
            seen.update(name='contrastive_search_device', rings=k.get('contrastive_rings', 'absent'))
            raise mk.Reached('contrastive_search_device')
        generate.XLDecoder, generate.contrastive_search_device = Dec, rec
        try:
            cls.generate(make(), input_ids=fx['prompt'], max_length=mk.MAX_LENGTH, **kw)
        except mk.Reached as r:
            seen.setdefault('name', str(r).split(' ')[0])
        finally:
            generate.XLDecoder, generate.contrastive_search_device = stub, search
    return seen.get('name'), built, seen.get('rings')


CS = dict(penalty_alpha=0.6, top_k=4)
STOP = dict(eos_token_id=1, pad_token_id=0)


def test_the_keyword_reaches_the_device_search_and_its_decoder(harness, monkeypatch):
    monkeypatch.delenv('MXL_CONTRASTIVE_RINGS', raising=False)
    monkeypatch.delenv('MXL_CONTRASTIVE_HOST', raising=False)
    B0 = harness[1]['prompt'].shape[0]
    # without the keyword: the decoder that was built before, with no keyword of this mode, and a search that is handed none
    for kw in (dict(), dict(contrastive_rings=None), dict(contrastive_rings='copied')):
        for stop in (dict(), STOP):
            assert _call(harness, **CS, **stop, **kw) == ('contrastive_search_device', [(B0 * 4, {})], 'absent')
    for stop in (dict(), STOP):
        assert _call(harness, contrastive_rings='shared', **CS, **stop) == ('contrastive_search_device', [(B0 * 4, dict(shared_rings=4))],
                                                                            'shared')
    assert _call(harness, contrastive_rings='shared', penalty_alpha=0.3, top_k=16)[1] == [(B0 * 16, dict(shared_rings=16))]
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'shared')            # the default of a call that does not pass the keyword
    assert _call(harness, **CS) == ('contrastive_search_device', [(B0 * 4, dict(shared_rings=4))], 'shared')
    assert _call(harness, contrastive_rings='copied', **CS) == ('contrastive_search_device', [(B0 * 4, {})], 'absent')


def test_refusals(harness, monkeypatch):
    monkeypatch.delenv('MXL_CONTRASTIVE_RINGS', raising=False)
    monkeypatch.delenv('MXL_CONTRASTIVE_HOST', raising=False)
    with pytest.raises(ValueError, match="contrastive_rings='indexed': expected None, 'copied' or 'shared'"):
        _call(harness, contrastive_rings='indexed', **CS)
    with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
        _call(harness, contrastive_rings='fp8')
    serves = "contrastive_rings='shared' serves contrastive search with its step on the device"
    elsewhere = [dict(), dict(do_sample=True), dict(do_sample=True, top_k=4, penalty_alpha=0.6),           # greedy, sampling
                 dict(num_beams=2, **STOP), dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.5, **STOP),
                 dict(num_beams=2, do_sample=True, renormalize_logits=True, **STOP),
                 dict(num_beams=2, do_sample=True, renormalize_logits=True, device_scorer=True, **STOP), dict(num_beams=17),
                 dict(penalty_alpha=0.6, top_k=33),                    # the host-driven loop: more candidates than the device step takes
                 dict(CS, kv_cache_dtype='fp8'), dict(kv_cache_dtype='fp8')]
    for arm in elsewhere:
        with pytest.raises(ValueError, match=serves):
            _call(harness, contrastive_rings='shared', **arm)
    monkeypatch.setenv('MXL_CONTRASTIVE_HOST', '1')
    with pytest.raises(ValueError, match=serves):
        _call(harness, contrastive_rings='shared', **CS)
    monkeypatch.delenv('MXL_CONTRASTIVE_HOST')
    monkeypatch.setenv('MXL_KV_DTYPE', 'fp8')
    with pytest.raises(ValueError, match=serves):
        _call(harness, contrastive_rings='shared', **CS)
    monkeypatch.delenv('MXL_KV_DTYPE')
    # the environment's default is ignored where 'shared' does not apply: these calls run as they always did
    monkeypatch.setenv('MXL_CONTRASTIVE_RINGS', 'shared')
    for arm, name in ((dict(), 'greedy'), (dict(do_sample=True), 'sample'), (dict(num_beams=2, **STOP), 'beam_search_device'),
                      (dict(num_beams=17), 'beam_search'), (dict(penalty_alpha=0.6, top_k=33), 'contrastive_search')):
        got, built, _ = _call(harness, **arm)
        assert got == name and all('shared_rings' not in k for _, k in built), arm
    monkeypatch.setenv('MXL_CONTRASTIVE_HOST', '1')
    got, built, _ = _call(harness, **CS)
    assert got == 'contrastive_search' and all('shared_rings' not in k for _, k in built)
    monkeypatch.delenv('MXL_CONTRASTIVE_HOST')
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8' is not supported under contrastive search"):
        _call(harness, kv_cache_dtype='fp8', **CS)                    # (as before, with the knob set or not)
    monkeypatch.delenv('MXL_CONTRASTIVE_RINGS')
    # the Reformer refuses the keyword as it refuses every option it does not cover
    for arm in (dict(), CS):
        with pytest.raises(NotImplementedError, match="generation options not covered: \\['contrastive_rings'\\]"):
            _call(harness, model='rf', contrastive_rings='shared', **arm)


def test_the_search_refuses_a_decoder_of_the_other_mode():
    from types import SimpleNamespace
    import torch
    dec = SimpleNamespace(eng=SimpleNamespace(cfg=SimpleNamespace(vocab_size=10), dev=torch.device('cpu')), B=8, Tmax=20, shared_K=0)
    prompt = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="contrastive_rings='shared' on a decoder built for the other ring mode"):
        generate.contrastive_search_device(dec, prompt, 10, top_k=4, penalty_alpha=0.6, contrastive_rings='shared')
    dec.shared_K = 4
    with pytest.raises(ValueError, match="contrastive_rings='copied' on a decoder built for the other ring mode"):
        generate.contrastive_search_device(dec, prompt, 10, top_k=4, penalty_alpha=0.6, contrastive_rings='copied')
    with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
        generate.contrastive_search_device(dec, prompt, 10, top_k=4, penalty_alpha=0.6, contrastive_rings='indexed')


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_new_entries_refuse_bad_arguments_before_any_launch():
    decl, L = _lib.declared_functions(), _lib.lib()
    assert [len(decl[n][1]) for n in ('mxl_kv_stash', 'mxl_relattn_decode_shared', 'mxl_kv_commit_shared',
                                      'mxl_relattn_decode_shared_lds_bytes')] == [7, 18, 11, 4]
    Pt = 4096                                                          # stands for a device pointer: nothing is followed before a launch
    att = dict(qkv=Pt, kc=Pt, vc=Pt, bd=Pt, rwb=Pt, out=Pt, t_dev=Pt, B0=2, K=16, H=2, dh=64, M=96, scale=0.125, pieces=1, ws=None,
               arrived=None, live=None)
    for bad in (dict(qkv=None), dict(kc=None), dict(vc=None), dict(bd=None), dict(rwb=None), dict(out=None), dict(t_dev=None), dict(K=1),
                dict(K=0), dict(K=33), dict(B0=0), dict(H=0), dict(M=0), dict(pieces=0), dict(pieces=9), dict(pieces=3), dict(qkv=Pt + 8),
                dict(kc=Pt + 2), dict(M=8192), dict(B0=32768), dict(dh=48, K=33)):
        assert L.mxl_relattn_decode_shared(*{**att, **bad}.values(), None) == EINVAL, bad
    for dh in (48, 8, 128, 0):
        assert L.mxl_relattn_decode_shared(*{**att, 'dh': dh}.values(), None) == EUNSUPPORTED
    st = dict(qkv=Pt, stash=Pt, B=4, d=64, rrb=Pt, qr=Pt)
    for bad in (dict(qkv=None), dict(stash=None), dict(B=0), dict(d=0), dict(d=12), dict(rrb=None), dict(stash=Pt + 8), dict(qr=Pt + 8)):
        assert L.mxl_kv_stash(*{**st, **bad}.values(), None) == EINVAL, bad
    cm = dict(table=Pt, L=2, stash=Pt, B0=2, K=4, H=2, M=32, dh=16, t_dev=Pt, sel=Pt)
    for bad in (dict(table=None), dict(stash=None), dict(t_dev=None), dict(sel=None), dict(L=0), dict(L=40000), dict(B0=0), dict(B0=65536),
                dict(K=1), dict(K=33), dict(H=0), dict(M=0), dict(dh=0), dict(dh=12), dict(stash=Pt + 8)):
        assert L.mxl_kv_commit_shared(*{**cm, **bad}.values(), None) == EINVAL, bad
    # the shared memory the header states: G * (cap * 4 + 20 * dh), G = 4 up to four candidates, else 8
    need = L.mxl_relattn_decode_shared_lds_bytes
    assert need(16, 64, 2048, 1) == 8 * (2048 * 4 + 20 * 64) and need(4, 64, 2048, 1) == 4 * (2048 * 4 + 20 * 64)
    assert need(32, 32, 96, 2) == 8 * ((48 + 34 + 2) * 4 + 20 * 32) and need(5, 16, 32, 8) == 8 * (32 * 4 + 20 * 16)
    assert need(1, 64, 2048, 1) == 0 and need(33, 64, 2048, 1) == 0 and need(16, 64, 2048, 9) == 0 and need(16, 64, 0, 1) == 0
    assert need(16, 64, 4096, 1) <= 160 * 1024 < need(16, 64, 8192, 1)
