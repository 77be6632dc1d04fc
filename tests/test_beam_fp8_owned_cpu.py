"""Indexed FP8 rings on the CPU (no GPU): the argument checks of mxl_relattn_decode_fp8_owned through the library (nothing is launched:
every call here is refused before a device is touched), its declaration in the header, and where `generate(beam_rings='indexed_fp8')`
goes -- the harness of tests/test_beam_owner_cpu.py (the unbound `generate` on a stub `self`, recorders in place of the decoders and
the searches), with the stub decoder's constructor recording the ring format it was asked for."""
import os

import pytest

from symbolic_music_generation_amd import _lib
from symbolic_music_generation_amd._lib import MusicXLError
from tests.test_beam_owner_cpu import BEAM, EUNSUPPORTED, GROUP, SAMPLE, _call, harness  # noqa: F401  (harness: a fixture)

ENTRY = 'mxl_relattn_decode_fp8_owned'


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_entry_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    Pt = 4096                                                          # stands for a device pointer: nothing is followed before a launch
    att = dict(qkv=Pt, kc8=Pt, ke=Pt, vc8=Pt, ve=Pt, owner=Pt, nb=3, bd=Pt, rwb=Pt, out=Pt, t_dev=Pt, B=6, H=2, dh=64, M=96, scale=0.125,
               pieces=1, ws=None, arrived=None, live=None)
    f = getattr(L, ENTRY)
    for bad in (dict(nb=0), dict(nb=17), dict(B=7), dict(B=0), dict(M=100), dict(M=0), dict(owner=Pt + 4), dict(owner=Pt + 8),
                dict(pieces=0), dict(pieces=9), dict(pieces=3), dict(pieces=2, ws=Pt), dict(pieces=2, arrived=Pt),
                dict(qkv=None), dict(kc8=None), dict(ke=None), dict(vc8=None), dict(ve=None), dict(owner=None), dict(bd=None),
                dict(rwb=None), dict(out=None), dict(t_dev=None), dict(kc8=Pt + 8), dict(vc8=Pt + 8),
                dict(M=12912)):                                        # M * 5 + 1024 bytes of shared memory beyond 64 KiB
        assert f(*{**att, **bad}.values(), None) == -1, bad
    assert (12896 * 5 + 1024) <= 64 * 1024 < (12912 * 5 + 1024) and 12912 % 16 == 0
    for dh in (8, 24, 128):
        assert f(*{**att, 'dh': dh}.values(), None) == EUNSUPPORTED, dh


def test_the_header_declares_the_entry():
    decl = _lib.declared_functions()
    assert ENTRY in decl
    assert len(decl[ENTRY][1]) == 21                                   # mxl_relattn_decode_fp8's 19 arguments, and owner and nb
    assert len(decl['mxl_relattn_decode_fp8'][1]) == 19 and len(decl['mxl_relattn_decode_owned'][1]) == 19        # as they were
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'musicxl.h')
    assert f'int {ENTRY}(' in open(header).read()


# ---------------------------------------------------------------------------------------------------------------- generate(beam_rings=)
@pytest.fixture
def built(harness, monkeypatch):
    """the ring format every stub decoder of a call was built with (None: bf16 rings), newest last"""
    mk, _ = harness
    formats = []
    real = mk._Decoder.__init__

    def init(self, *a, **k):
        formats.append(k.get('kv_dtype'))
        real(self, *a, **k)
    monkeypatch.setattr(mk._Decoder, '__init__', init)
    return formats


DEVICE_ARMS = ((BEAM, 'beam_search_device'), (GROUP, 'group_beam_search_device'), (dict(SAMPLE, device_scorer=True), 'beam_sample_device'))


def test_indexed_fp8_reaches_the_device_searches_with_an_fp8_decoder(harness, built, monkeypatch):
    monkeypatch.delenv('MXL_BEAM_RINGS', raising=False)
    monkeypatch.setenv('MXL_GROUP_BEAM_DEVICE', '1')
    for arm, name in DEVICE_ARMS:
        del built[:]
        assert _call(harness, beam_rings='indexed_fp8', **arm) == (name, 'indexed') and built == ['fp8'], (name, built)
        del built[:]
        monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed_fp8')            # the default of a call that does not pass the keyword
        assert _call(harness, **arm) == (name, 'indexed') and built == ['fp8'], (name, built)
        del built[:]
        assert _call(harness, beam_rings='indexed', **arm) == (name, 'indexed') and built == [None]     # the keyword wins
        del built[:]
        assert _call(harness, beam_rings='copied', **arm) == (name, 'copied') and built == [None]
        monkeypatch.delenv('MXL_BEAM_RINGS')
        del built[:]
        assert _call(harness, **arm) == (name, 'copied') and built == [None]           # a call that names nothing runs what it ran
        del built[:]
        assert _call(harness, beam_rings='indexed', **arm) == (name, 'indexed') and built == [None]


def test_indexed_fp8_refusals(harness, built, monkeypatch):
    monkeypatch.delenv('MXL_BEAM_RINGS', raising=False)
    elsewhere = [dict(), dict(do_sample=True), dict(penalty_alpha=0.6, top_k=4), dict(num_beams=17), SAMPLE, dict(GROUP)]
    for arm in elsewhere:                                              # (group beam without a rule keeps the host scorer)
        with pytest.raises(ValueError, match="beam_rings='indexed_fp8' serves"):
            _call(harness, beam_rings='indexed_fp8', **arm)
    monkeypatch.setenv('MXL_BEAM_HOST', '1')
    with pytest.raises(ValueError, match="beam_rings='indexed_fp8' serves"):
        _call(harness, beam_rings='indexed_fp8', **BEAM)
    monkeypatch.delenv('MXL_BEAM_HOST')
    # the two-keyword spelling keeps raising as it did, with this value as with 'indexed'
    for arm in (BEAM, dict(SAMPLE, device_scorer=True)):
        with pytest.raises(ValueError, match="kv_cache_dtype='fp8' is not supported under"):
            _call(harness, beam_rings='indexed_fp8', kv_cache_dtype='fp8', **arm)
    # the environment's default is ignored where the mode does not apply: these calls run as they always did, on bf16 rings
    monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed_fp8')
    for arm, name in ((dict(), 'greedy'), (dict(do_sample=True), 'sample'), (dict(penalty_alpha=0.6, top_k=4), 'contrastive_search_device'),
                      (dict(num_beams=17), 'beam_search'), (SAMPLE, 'beam_search')):
        del built[:]
        assert _call(harness, **arm)[0] == name, arm
        assert built and all(f is None for f in built), (arm, built)
    monkeypatch.delenv('MXL_BEAM_RINGS')
    for arm in (dict(), BEAM):                                         # the Reformer refuses it as it refuses every option it does not cover
        with pytest.raises(NotImplementedError, match="generation options not covered: \\['beam_rings'\\]"):
            _call(harness, model='rf', beam_rings='indexed_fp8', **arm)


def test_head_widths_fp8_rings_do_not_take(harness, built, monkeypatch):
    """a head width other than 16, 32 or 64: naming 'indexed_fp8' raises MusicXLError, the environment's is ignored"""
    from symbolic_music_generation_amd import generate
    mk, fx = harness
    monkeypatch.delenv('MXL_BEAM_RINGS', raising=False)
    assert generate.resolve_beam_rings('indexed_fp8', True, 32) == 'indexed_fp8'
    assert generate.resolve_beam_rings('indexed', True, 24) == 'indexed'
    with pytest.raises(MusicXLError, match='head width of 16, 32 or 64, not 24'):
        generate.resolve_beam_rings('indexed_fp8', True, 24)
    monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed_fp8')
    assert generate.resolve_beam_rings(None, True, 24) == 'copied'
    assert generate.resolve_beam_rings(None, True, 16) == 'indexed_fp8'
    assert generate.resolve_beam_rings(None, False, 16) == 'copied'
    monkeypatch.delenv('MXL_BEAM_RINGS')
    cls, make = fx['models']['xl']
    wide = make()
    wide.config.d_head = 128
    with mk.patched():
        with pytest.raises(MusicXLError, match='head width of 16, 32 or 64, not 128'):
            cls.generate(wide, input_ids=fx['prompt'], max_length=mk.MAX_LENGTH, beam_rings='indexed_fp8', **BEAM)
    assert generate.BEAM_RINGS == ('copied', 'indexed', 'indexed_fp8') and generate.DECODER_BEAM_RINGS == ('copied', 'indexed')
