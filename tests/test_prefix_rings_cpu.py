"""Prompt rings under sampling on the CPU (no GPU): the slot-source rule of tests/prefix_ring_ref.py against a ring written position by
position, the table of generate.resolve_prompt_rings, what `generate(prompt_rings=)` builds and refuses before a device is touched (the
harness of tests/golden/make_generate_dispatch.py), and the argument checks of the new entries through the library."""
import importlib.util
import os

import pytest
import torch

from symbolic_music_generation_amd import _lib, generate
from tests import prefix_ring_ref as R

EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------- the slot-source rule
def _brute(t, Tp, M, Mt):
    """positions 0..t written in order into an M-slot ring, each tagged with where the layout keeps it; the tail ring is written in
    order too, so a tail slot that a later position has overwritten shows"""
    ring, tail = [(R.NEVER, None)] * M, [None] * Mt
    for p in range(t + 1):
        if p >= Tp:
            tail[(p - Tp) % Mt] = p
            ring[p % M] = (R.TAIL, (p - Tp) % Mt, p)
        else:
            ring[p % M] = (R.PROMPT, p % M, p)
    return ring, tail


def _grid():
    for M in (16, 32, 48):
        for Tp in (1, 5, M - 1, M, M + 1, 2 * M + 3):                     # below, at and above the ring length
            for Mt in sorted({16, M}):
                for gen in (0, 1, 2, 7, 15, 16, M - Tp - 1, M - Tp, M - Tp + 1, M - 1, M, M + 1, 2 * M, 3 * M + 5):
                    if gen < 0 or (Mt < M and gen + 1 > Mt):               # a tail shorter than the ring holds Mt generated positions
                        continue
                    yield Tp, M, Mt, Tp + gen                              # t = Tp: the first step
            yield Tp, M, M, Tp - 1                                         # the last prompt position: no tail slot yet
    yield from R.CASES
    yield from R.LONG_CASES


def test_slot_source_against_a_ring_written_in_order():
    seen = set()
    for Tp, M, Mt, t in _grid():
        ring, tail = _brute(t, Tp, M, Mt)
        for s in range(M):
            kind, at = R.slot_source(t, Tp, M, Mt, s)
            assert (kind, at) == ring[s][:2], (Tp, M, Mt, t, s)
            if kind == R.TAIL:                                             # ... and the tail slot still holds that position
                assert tail[at] == ring[s][2], f'tail slot {at} was overwritten: Tp {Tp} M {M} Mt {Mt} t {t} s {s}'
        kinds = [k for k, *_ in ring]
        seen.add((R.NEVER in kinds, R.PROMPT in kinds, R.TAIL in kinds, t - Tp >= M, t >= M, Mt < M))
    # the grid holds what it is meant to: rings with never-written slots, prompt and tail together across the wrap, no prompt slot
    # left, no tail slot yet, and short tails
    assert (True, True, True, False, False, False) in seen and (False, True, True, False, True, False) in seen
    assert (False, False, True, True, True, False) in seen and (False, True, False, False, True, False) in seen
    assert any(k[5] and k[2] for k in seen)


def test_gather_rebuilds_the_ring_of_the_copied_mode():
    g = torch.Generator().manual_seed(0)
    B0, n, H, M, Mt, dh, Tp, t = 2, 3, 2, 16, 16, 4, 21, 30
    pos = torch.randn(B0 * n, H, t + 1, dh, generator=g)
    pos[:, :, :Tp] = pos[::n, :, :Tp].repeat_interleave(n, 0)
    want = torch.zeros(B0 * n, H, M, dh)
    prompt, tail = torch.full((B0, H, M, dh), float('nan')), torch.full((B0 * n, H, Mt, dh), float('nan'))
    for p in range(t + 1):
        want[:, :, p % M] = pos[:, :, p]
        if p >= Tp:
            tail[:, :, (p - Tp) % Mt] = pos[:, :, p]
        elif p > t - M:
            prompt[:, :, p % M] = pos[::n, :, p]
    assert torch.equal(R.gather_ring(prompt, tail, t, Tp, n), want)


# ---------------------------------------------------------------------------------------------------------------- the resolve function
def test_resolve_table(monkeypatch):
    P = generate.resolve_prompt_rings
    monkeypatch.delenv('MXL_PROMPT_RINGS', raising=False)
    assert generate.PROMPT_RINGS == ('copied', 'shared')
    for applies in (False, True):
        assert P(None, applies) == 'copied' and P('copied', applies) == 'copied'
    assert P('shared', True) == 'shared'
    with pytest.raises(ValueError, match="prompt_rings='shared' serves sampling with num_return_sequences >= 2"):
        P('shared', False)
    for bad in ('indexed', 'Shared', '', 'fp8'):
        for applies in (False, True):
            with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
                P(bad, applies)
    # the environment sets the default of a call that names none, and is ignored where the mode does not apply
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'shared')
    assert P(None, True) == 'shared' and P(None, False) == 'copied' and P('copied', True) == 'copied'
    with pytest.raises(ValueError, match='serves sampling'):
        P('shared', False)
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'copied')
    assert P(None, True) == 'copied' and P('shared', True) == 'shared'
    monkeypatch.setenv('MXL_PROMPT_RINGS', '')
    assert P(None, True) == 'copied'
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'both')
    with pytest.raises(ValueError, match="prompt_rings='both'"):
        P(None, False)


def test_tail_length_and_the_model_checks():
    from types import SimpleNamespace
    T = generate.prompt_tail_len
    assert [T(64, g) for g in (1, 15, 16, 17, 33, 64, 65, 500)] == [16, 16, 16, 32, 48, 64, 64, 64] and T(2048, 256) == 256
    cfg = lambda **k: SimpleNamespace(**{**dict(mem_len=64, d_head=16, n_head=2), **k})
    assert generate.prompt_rings_misfit(cfg(), 5, 15) is None
    assert 'head width of 16, 32 or 64, not 48' in generate.prompt_rings_misfit(cfg(d_head=48), 5, 15)
    assert 'multiple of 16, not 72' in generate.prompt_rings_misfit(cfg(mem_len=72), 5, 15)
    assert 'KiB of shared memory' in generate.prompt_rings_misfit(cfg(mem_len=8192, d_head=64, n_head=12), 8, 256)
    assert generate.prompt_rings_misfit(cfg(mem_len=2048, d_head=64, n_head=12), 16, 16) is None


# ---------------------------------------------------------------------------------------------------------------- generate(prompt_rings=)
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
    """`generate` on the stub model -> (name of the entry reached, (rows, keywords) of the decoders built) or raises what generate raises"""
    mk, fx = harness
    cls, make = fx['models'][model]
    seen, built = {}, []
    with mk.patched():
        stubs = generate.XLDecoder, generate.XLDecoderLanes

        def spy(stub):
            class Dec(stub):
                def __init__(self, engine, batch, max_total_len, *a, **k):
                    super().__init__(engine, batch, max_total_len, *a, **k)
                    built.append((batch, {n: v for n, v in k.items() if n not in ('seed', 'kv_dtype', 'lanes')}))
            return Dec
        generate.XLDecoder, generate.XLDecoderLanes = spy(stubs[0]), spy(stubs[1])
        try:
            cls.generate(make(), input_ids=fx['prompt'], max_length=mk.MAX_LENGTH, **kw)
        except mk.Reached as r:
            seen.setdefault('name', str(r).split(' ')[0])
        finally:
            generate.XLDecoder, generate.XLDecoderLanes = stubs
    return seen.get('name'), built


SAMPLE = dict(do_sample=True, top_k=8)
STOP = dict(eos_token_id=1, pad_token_id=0)


def test_the_keyword_reaches_the_decoder(harness, monkeypatch):
    monkeypatch.delenv('MXL_PROMPT_RINGS', raising=False)
    B0, Tp = harness[1]['prompt'].shape
    mk = harness[0]
    tail = mk.MAX_LENGTH - Tp
    # without the keyword: the decoder that was built before, with no keyword of this mode
    for kw in (dict(), dict(prompt_rings=None), dict(prompt_rings='copied')):
        assert _call(harness, **SAMPLE, num_return_sequences=3, **kw) == ('sample', [(B0 * 3, {})])
        assert _call(harness, **SAMPLE, **kw) == ('sample', [(B0, {})])
    assert _call(harness, **SAMPLE, num_return_sequences=3, prompt_rings='shared') == ('sample', [(B0 * 3, dict(prompt_rings=3, tail_len=tail))])
    assert _call(harness, **SAMPLE, **STOP, num_return_sequences=2, prompt_rings='shared')[1] == [(B0 * 2, dict(prompt_rings=2, tail_len=tail))]
    # from 32 rows on: lanes, cut between prompts
    assert _call(harness, **SAMPLE, num_return_sequences=16, prompt_rings='shared')[1] == [(B0 * 16, dict(prompt_rings=16, tail_len=tail))]
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'shared')                   # the default of a call that does not pass the keyword
    assert _call(harness, **SAMPLE, num_return_sequences=3)[1] == [(B0 * 3, dict(prompt_rings=3, tail_len=tail))]
    assert _call(harness, **SAMPLE, num_return_sequences=3, prompt_rings='copied')[1] == [(B0 * 3, {})]
    # ... ignored where the mode does not apply: these calls run as they always did
    for arm, name in ((dict(), 'greedy'), (SAMPLE, 'sample'), (dict(num_beams=2, **STOP), 'beam_search_device'),
                      (dict(penalty_alpha=0.6, top_k=4), 'contrastive_search_device'),
                      (dict(SAMPLE, num_return_sequences=3, kv_cache_dtype='fp8'), 'sample')):
        got, built = _call(harness, **arm)
        assert got == name and all('prompt_rings' not in k for _, k in built), arm


def test_refusals(harness, monkeypatch):
    monkeypatch.delenv('MXL_PROMPT_RINGS', raising=False)
    with pytest.raises(ValueError, match="prompt_rings='indexed': expected None, 'copied' or 'shared'"):
        _call(harness, prompt_rings='indexed', **SAMPLE, num_return_sequences=3)
    with pytest.raises(ValueError, match="expected None, 'copied' or 'shared'"):
        _call(harness, prompt_rings='fp8')
    serves = "prompt_rings='shared' serves sampling with num_return_sequences >= 2"
    elsewhere = [SAMPLE, dict(SAMPLE, num_return_sequences=1),            # one row per prompt
                 dict(), dict(top_k=4),                                    # greedy decoding
                 dict(num_beams=2, **STOP), dict(num_beams=2, num_return_sequences=2, **STOP),
                 dict(num_beams=4, num_beam_groups=2, diversity_penalty=1.5, **STOP),
                 dict(num_beams=2, do_sample=True, renormalize_logits=True, num_return_sequences=2, **STOP),
                 dict(num_beams=2, do_sample=True, renormalize_logits=True, device_scorer=True, **STOP), dict(num_beams=17),
                 dict(penalty_alpha=0.6, top_k=4), dict(penalty_alpha=0.6, top_k=33),
                 dict(SAMPLE, num_return_sequences=3, kv_cache_dtype='fp8')]
    for arm in elsewhere:
        with pytest.raises(ValueError, match=serves):
            _call(harness, prompt_rings='shared', **arm)
    monkeypatch.setenv('MXL_KV_DTYPE', 'fp8')
    with pytest.raises(ValueError, match=serves):
        _call(harness, prompt_rings='shared', **SAMPLE, num_return_sequences=3)
    monkeypatch.delenv('MXL_KV_DTYPE')
    with pytest.raises(ValueError, match='num_return_sequences has to be 1 when doing greedy search'):
        _call(harness, num_return_sequences=2)                            # (as before)
    # the Reformer refuses the keyword as it refuses every option it does not cover
    for arm in (dict(), dict(SAMPLE, num_return_sequences=3)):
        with pytest.raises(NotImplementedError, match="generation options not covered: \\['prompt_rings'\\]"):
            _call(harness, model='rf', prompt_rings='shared', **arm)


def test_a_model_the_kernel_does_not_take(harness, monkeypatch):
    """an explicit 'shared' raises MusicXLError for a head width or a mem_len the attention launch refuses; the environment's default is
    ignored there"""
    mk, fx = harness
    cls, make = fx['models']['xl']

    def run(**cfg):
        m = make()
        for k, v in cfg.items():
            setattr(m.config, k, v)
        with mk.patched():
            try:
                cls.generate(m, input_ids=fx['prompt'], max_length=mk.MAX_LENGTH, **SAMPLE, num_return_sequences=3, **run.kw)
            except mk.Reached as r:
                return str(r).split(' ')[0]
    run.kw = dict(prompt_rings='shared')
    monkeypatch.delenv('MXL_PROMPT_RINGS', raising=False)
    with pytest.raises(_lib.MusicXLError, match='head width of 16, 32 or 64, not 48'):
        run(d_head=48)
    with pytest.raises(_lib.MusicXLError, match='mem_len that is a multiple of 16, not 72'):
        run(mem_len=72)
    with pytest.raises(_lib.MusicXLError, match='KiB of shared memory'):
        run(mem_len=65536)
    run.kw = {}
    monkeypatch.setenv('MXL_PROMPT_RINGS', 'shared')
    assert run(d_head=48) == 'sample' and run(mem_len=72) == 'sample' and run(mem_len=65536) == 'sample'


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_new_entries_refuse_bad_arguments_before_any_launch():
    decl, L = _lib.declared_functions(), _lib.lib()
    assert [len(decl[n][1]) for n in ('mxl_kv_append_tail', 'mxl_relattn_decode_prefix', 'mxl_relattn_decode_prefix_lds_bytes')] == [12, 22, 4]
    Pt = 4096                                                          # stands for a device pointer: nothing is followed before a launch
    att = dict(qkv=Pt, kp=Pt, vp=Pt, kt=Pt, vt=Pt, bd=Pt, rwb=Pt, out=Pt, t_dev=Pt, t0_dev=Pt, B0=2, n=16, H=2, dh=64, M=96, Mt=32,
               scale=0.125, pieces=1, ws=None, arrived=None, live=None)
    for bad in (dict(qkv=None), dict(kp=None), dict(vp=None), dict(kt=None), dict(vt=None), dict(bd=None), dict(rwb=None), dict(out=None),
                dict(t_dev=None), dict(t0_dev=None), dict(n=1), dict(n=0), dict(B0=0), dict(H=0), dict(M=0), dict(M=100), dict(M=8),
                dict(Mt=0), dict(Mt=8), dict(Mt=40), dict(Mt=112), dict(pieces=0), dict(pieces=9), dict(pieces=3), dict(qkv=Pt + 8),
                dict(kp=Pt + 2), dict(vp=Pt + 4), dict(kt=Pt + 8), dict(vt=Pt + 8), dict(M=8192, Mt=16), dict(B0=32768),
                dict(B0=65536, n=4), dict(dh=48, n=1)):
        assert L.mxl_relattn_decode_prefix(*{**att, **bad}.values(), None) == EINVAL, bad
    for dh in (48, 8, 128, 0):
        assert L.mxl_relattn_decode_prefix(*{**att, 'dh': dh}.values(), None) == EUNSUPPORTED
    ap = dict(qkv=Pt, kt=Pt, vt=Pt, t_dev=Pt, t0_dev=Pt, B=4, Mt=32, d=64, dh=16, rrb=Pt, qr=Pt)
    for bad in (dict(qkv=None), dict(kt=None), dict(vt=None), dict(t_dev=None), dict(t0_dev=None), dict(B=0), dict(Mt=0), dict(Mt=8),
                dict(Mt=24), dict(d=0), dict(d=12), dict(dh=0), dict(dh=12), dict(dh=24), dict(rrb=None), dict(qkv=Pt + 8), dict(kt=Pt + 8),
                dict(vt=Pt + 2), dict(qr=Pt + 8)):
        assert L.mxl_kv_append_tail(*{**ap, **bad}.values(), None) == EINVAL, bad
    # the shared memory the header states: G * (cap * 4 + 16 * dh), G = 4 up to four rows per prompt, else 8
    need = L.mxl_relattn_decode_prefix_lds_bytes
    assert need(16, 64, 2048, 1) == 8 * (2048 * 4 + 16 * 64) and need(4, 64, 2048, 1) == 4 * (2048 * 4 + 16 * 64)
    assert need(40, 32, 96, 2) == 8 * ((48 + 34 + 2) * 4 + 16 * 32) and need(5, 16, 32, 8) == 8 * (32 * 4 + 16 * 16)
    assert need(1, 64, 2048, 1) == 0 and need(16, 64, 2048, 9) == 0 and need(16, 64, 0, 1) == 0
    assert need(16, 64, 4096, 1) <= 160 * 1024 < need(16, 64, 8192, 1)
