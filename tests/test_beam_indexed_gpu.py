"""`generate(..., beam_rings='indexed')` end to end: the device beam searches with the K/V rings left where the forward pass wrote them
and read through the owner table, against the same call with 'copied' (whole ring rows moved every step).  The 2-layer model of
tests/test_beam_device_gpu.py with mem_len = 32 and max_length = 80, so the ring wraps while beams are live; ids and scores must be
equal, exactly.  On the commit before the feature every call here raises TypeError (an unknown keyword)."""
import pytest
import torch

from symbolic_music_generation_amd import generate as G

pytestmark = pytest.mark.gpu

# the model and the prompts of tests/test_beam_device_gpu.py: eos = 1121 ends hypotheses of prompt 1 at once, eos = -1 never fires
SEED, PROMPT_SEED, TP, MEM, L = 13, 21, 12, 32, 80
EOS_EMITTED, EOS_NEVER = 1121, -1


@pytest.fixture(scope='module')
def plain(dev):
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=MEM, max_length=L, seed=SEED)
    prompt = torch.randint(4, 1190, (2, TP), generator=torch.Generator().manual_seed(PROMPT_SEED)).to(dev)
    return m.eval(), prompt


class _Modes:
    """records the decoder of every beam_begin, so that a test can read the mode a `generate` call ran in"""

    def __init__(self, monkeypatch):
        self.decoders = []
        real = G.XLDecoder.beam_begin

        def begin(dec, *a, **k):
            self.decoders.append(dec)
            return real(dec, *a, **k)
        monkeypatch.setattr(G.XLDecoder, 'beam_begin', begin)

    def last(self):
        return self.decoders[-1].beam_rings


def _both(m, modes, **kw):
    """the call under both modes -> the indexed result, after holding it to the copied one"""
    want = m.generate(beam_rings='copied', **kw)
    assert modes.last() == 'copied'
    got = m.generate(beam_rings='indexed', **kw)
    assert modes.last() == 'indexed' and modes.decoders[-1].owner is not None
    assert got.shape == want.shape and torch.equal(got, want), kw
    return got


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('early', [True, False])
@pytest.mark.parametrize('nb', [2, 3])
def test_plain_beam(plain, monkeypatch, nb, early, use_graph):
    m, prompt = plain
    modes, fired = _Modes(monkeypatch), 0
    for eos in (EOS_EMITTED, EOS_NEVER):
        kw = dict(num_beams=nb, early_stopping=early, num_return_sequences=2, eos_token_id=eos, pad_token_id=0, use_graph=use_graph)
        dec = G.XLDecoder(m.engine, 2 * nb, L)
        want, w_sc = G.beam_search_device(dec, prompt, L, return_scores=True, beam_rings='copied', **kw)
        got, g_sc = G.beam_search_device(dec, prompt, L, return_scores=True, beam_rings='indexed', **kw)      # the same decoder: a new key
        assert torch.equal(got, want) and torch.equal(g_sc, w_sc), (eos, g_sc.tolist(), w_sc.tolist())
        if eos == EOS_NEVER:
            assert got.shape[1] == L and dec.steps_run == L - TP - 1 > 2 * MEM - TP        # the ring wrapped with every beam live
            foreign = (dec.owner.cpu() != (torch.arange(2 * nb) % nb)[:, None]).float().mean().item()
            print(f'plain beam nb {nb} early {early} graph {use_graph}: {100 * foreign:.0f} % of the last window is held by a sibling')
            assert foreign > 0.1                                       # beams moved: the table is what the attention read through
        fired += int((got[:, TP:] == eos).any())
        assert torch.equal(_both(m, modes, input_ids=prompt, max_length=L, **kw), got)          # the public interface
    assert fired == 1


@pytest.mark.parametrize('use_graph', [True, False])
def test_group_beam(plain, monkeypatch, use_graph):
    m, prompt = plain
    modes = _Modes(monkeypatch)
    monkeypatch.setenv('MXL_GROUP_BEAM_DEVICE', '1')
    for eos in (EOS_EMITTED, EOS_NEVER):
        _both(m, modes, input_ids=prompt, max_length=L, num_beams=4, num_beam_groups=2, diversity_penalty=1.5, early_stopping=True,
              eos_token_id=eos, pad_token_id=0, use_graph=use_graph)


@pytest.mark.parametrize('use_graph', [True, False])
def test_beam_sample(plain, monkeypatch, use_graph):
    m, prompt = plain
    modes = _Modes(monkeypatch)
    _both(m, modes, input_ids=prompt, max_length=L, num_beams=3, do_sample=True, renormalize_logits=True, early_stopping=True, top_k=0,
          device_scorer=True, seed=5, eos_token_id=EOS_NEVER, pad_token_id=0, use_graph=use_graph)


def test_rules_under_indexed_rings(dev, monkeypatch):
    """the grammar with its bar budget and the key rule: the rule words follow the beams inside mxl_beam_step in both modes"""
    from tests.test_key_rule_gpu import EOS, FULL_BAR, PAD, RULE, TOK, _prompts
    from tests.test_xl_model_gpu import _pair
    _, m = _pair(dev, n_layer=2, mem_len=MEM, max_length=L, seed=601)
    ids, _ = _prompts(2, dev, FULL_BAR, keyless=False)
    modes = _Modes(monkeypatch)
    got = _both(m.eval(), modes, input_ids=ids, max_length=L, num_beams=3, early_stopping=False, eos_token_id=EOS, pad_token_id=PAD,
                grammar=TOK.grammar(bar_budget=True), in_key=RULE)
    print('rules under indexed rings: prompt', ids.shape[1], 'returned', tuple(got.shape), 'steps', modes.decoders[-1].steps_run)


def test_two_calls_in_a_row_and_the_environment_default(plain, monkeypatch):
    """one decoder, two beam counts: the table is reset and rebuilt per beam_begin and the mode is part of the graph key; then
    MXL_BEAM_RINGS=indexed without the keyword takes the indexed path, and is ignored where it does not apply"""
    m, prompt = plain
    kw = dict(early_stopping=True, eos_token_id=EOS_NEVER, pad_token_id=0, use_graph=True)
    prompts = torch.cat([prompt, prompt[:1].flip(1)])
    dec, keys, outs = G.XLDecoder(m.engine, 6, L), [], {}
    for nb, mode in ((3, 'indexed'), (2, 'indexed'), (2, 'copied'), (3, 'copied'), (3, 'indexed')):
        out = G.beam_search_device(dec, prompts[:6 // nb], L, num_beams=nb, beam_rings=mode, **kw)
        assert dec.beam_rings == mode
        keys.append(dec._graph_key)
        assert torch.equal(outs.setdefault(nb, out), out), (nb, mode)  # whatever ran before, and in either mode
    assert all(a != b for a, b in zip(keys, keys[1:])), keys
    assert dec.owner.shape == (6, MEM) and int(dec.owner.max()) <= 2
    dec.generate(prompts.repeat(2, 1), L, use_graph=True)               # greedy on the used decoder: every row reads its own ring again
    assert dec.beam_rings == 'copied'

    modes = _Modes(monkeypatch)
    call = dict(input_ids=prompt, max_length=L, num_beams=2, **kw)
    want = m.generate(**call)
    assert modes.last() == 'copied'
    monkeypatch.setenv('MXL_BEAM_RINGS', 'indexed')
    assert torch.equal(m.generate(**call), want) and modes.last() == 'indexed'
    assert torch.equal(m.generate(beam_rings='copied', **call), want) and modes.last() == 'copied'
    greedy = m.generate(input_ids=prompt, max_length=TP + 4)           # the default is ignored where it does not apply
    assert greedy.shape == (2, TP + 4)
    monkeypatch.delenv('MXL_BEAM_RINGS')
    with pytest.raises(ValueError, match="beam_rings='indexed' serves"):
        m.generate(input_ids=prompt, max_length=TP + 4, beam_rings='indexed')
