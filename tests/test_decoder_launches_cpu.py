"""What XLDecoder allocates, launches and refuses in every K/V ring mode, against the table recorded by
tests/golden/make_decoder_launches.py (which explains the harness: decoders on the CPU over a stub engine, recorders in place of the
launching functions of `ops`; no GPU, no library load).  The table pins the ring tensors of every mode, the launches of the prompt
pass with the rows it feeds and the rows it writes, of a decode step, of a beam step and of a contrastive step with their
arguments, which captures share a graph key, and the refusals with their types and messages."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# every launch that tells one ring mode from another must still be reached: (decoder, part of the record, launch)
REACHED = [('plain8', 'token', 'decode_qkv('), ('plain65', 'token', 'kv_append('), ('plain8', 'token', 'relattn_decode('),
           ('fp8', 'token', 'kv_append_fp8('), ('fp8', 'token', 'relattn_decode_fp8('), ('fp8', 'begin', 'kv_fill_fp8('),
           ('shared4', 'token', 'kv_stash('), ('shared8', 'token', 'relattn_decode_shared('), ('shared4', 'contrastive', 'kv_commit_shared('),
           ('prompt4', 'token', 'kv_append_tail('), ('prompt8', 'token', 'relattn_decode_prefix('), ('prompt4', 'begin', 'kv_fill('),
           ('plain8', 'beam', 'beam_reorder('), ('plain8', 'beam', 'beam_owner_follow('), ('fp8', 'beam', 'beam_owner_follow('),
           ('plain8', 'beam', 'owner=owner, nb=4'), ('fp8', 'beam', 'owner=owner, nb=4'), ('plain8', 'contrastive', 'ring_slot_broadcast('),
           ('plain8', 'begin', 'sample_step('), ('prompt4', 'begin', 'sample_step(')]


def _maker():
    spec = importlib.util.spec_from_file_location('make_decoder_launches', os.path.join(GOLDEN, 'make_decoder_launches.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _diff(got, want, path=''):
    """the paths at which two records differ"""
    if isinstance(got, dict) and isinstance(want, dict):
        return [d for k in sorted(set(got) | set(want)) for d in
                (_diff(got[k], want[k], f'{path}/{k}') if k in got and k in want else [f'{path}/{k}: only in one'])]
    if isinstance(got, list) and isinstance(want, list) and len(got) == len(want):
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in _diff(g, w, f'{path}[{i}]')]
    return [] if got == want else [f'{path}: {got!r} != {want!r}']


def _strings(x):
    if isinstance(x, str):
        yield x
    elif isinstance(x, (list, dict)):
        for v in (x.values() if isinstance(x, dict) else x):
            yield from _strings(v)


def test_decoders_launch_and_refuse_what_the_table_says():
    maker = _maker()
    with open(os.path.join(GOLDEN, 'decoder_launches.json')) as f:
        want = maker.unpack(json.load(f))
    got = maker.record()
    wrong = _diff(got, want)
    assert not wrong, (len(wrong), wrong[:8])
    # every decoder of the table and every part of its record is there, and the record cannot silently stop reaching a launch
    assert set(got) == {name for name, _ in maker.DECODERS} | {'refusals'}
    for name, _ in maker.DECODERS:
        assert set(got[name]) == {'build', 'token', 'begin', 'beam', 'contrastive', 'keys'}
    for name, part, launch in REACHED:
        assert any(launch in s for s in _strings(got[name][part])), (name, part, launch)
    # each mode refuses the entry points it does not serve, and serves its own
    assert got['shared4']['begin']['plain']['how'] == 'refused' and got['shared4']['contrastive']['own']['how'] == 'ok'
    assert got['prompt4']['beam']['copied']['how'] == 'refused' and got['prompt4']['begin']['plain']['how'] == 'ok'
    assert got['fp8']['contrastive']['own']['how'] == 'refused' and got['fp8']['beam']['indexed']['how'] == 'ok'
    # a second generation with another prompt length shares the graph; another sampler, stop rule or ring mode does not
    for name in ('plain8', 'fp8', 'prompt4'):
        same = [v['same_key_as'] for v in got[name]['keys'].values()]
        assert same[:4] == [0, 0, 2, 3], (name, same)
    assert [v['same_key_as'] for v in got['plain8']['keys'].values()][4:] == [4, 5, 6]
