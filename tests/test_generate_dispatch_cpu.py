"""What both models' `generate` reach or refuse for a grid of arguments, against the table recorded by
tests/golden/make_generate_dispatch.py (which explains the harness: the unbound methods on a stub `self`, recorders in place of the
decoders and the searches; no GPU, no library load).  The table pins the strategy choice, the refusals with their types, messages
and precedence, the decoder rows and the eos / pad every search is handed."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _maker():
    spec = importlib.util.spec_from_file_location('make_generate_dispatch', os.path.join(GOLDEN, 'make_generate_dispatch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


only = 'is supported for greedy decoding and sampling only, not for'
# every class of outcome the grid must keep reaching, per model: (label prefix, outcome prefix)
REACHED = [('xl', s) for s in (
    'beam_search ', 'group_beam_search ', 'beam_search_device ', 'group_beam_search_device ', 'contrastive_search ',
    'contrastive_search_device ', 'greedy ', 'sample ',
    'MusicXLError: padded prompts: max_new_tokens and stopping_criteria',
    'MusicXLError: padded prompts (attention_mask with zeros) are supported',
    f'MusicXLError: melody= {only} beam, group-beam or contrastive', f'MusicXLError: grammar= {only} beam, group-beam or contrastive',
    f'MusicXLError: n_bars= {only} beam, group-beam or contrastive', f'MusicXLError: in_key= {only} beam, group-beam or contrastive',
    'ValueError: `num_beam_groups` has to be smaller or equal to `num_beams`', 'ValueError: Diverse beam search cannot be used',
    'ValueError: num_return_sequences has to be 1 when doing greedy search', 'ValueError: Both `max_new_tokens` and `max_length`',
)] + [('rf', s) for s in (
    'beam_search ', 'group_beam_search ', 'greedy ', 'sample ',
    f'MusicXLError: melody= {only} beam, group-beam or contrastive', f'MusicXLError: grammar= {only} beam or group-beam search',
    f'MusicXLError: n_bars= {only} beam, group-beam or contrastive', f'MusicXLError: in_key= {only} beam, group-beam or contrastive',
    'MusicXLError: MyReformerModelWithLMHead.generate does not support padded prompts',
    "ValueError: MyReformerModelWithLMHead **can't** be used for contrastive search",
    'ValueError: `num_beam_groups` has to be smaller or equal to `num_beams`', 'ValueError: Diverse beam search cannot be used',
    'ValueError: num_return_sequences has to be 1 when doing greedy search', 'ValueError: Both `max_new_tokens` and `max_length`',
)]


def test_generate_reaches_and_refuses_what_the_table_says():
    with open(os.path.join(GOLDEN, 'generate_dispatch.json')) as f:
        table = json.load(f)
    want = [table['outcomes'][i] for i in table['cases']]
    labels, got = _maker().record()
    assert len(got) == len(want)
    wrong = [(lab, g, w) for lab, g, w in zip(labels, got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])
    # the grid cannot silently stop reaching a branch
    for model, start in REACHED:
        assert any(lab.startswith(model + ' ') and g.startswith(start) for lab, g in zip(labels, got)), (model, start)
    # beam-sample is reached as beam search with do_sample, on rows x num_return_sequences
    assert any(g.startswith('beam_search rows=[16]') and 'do_sample=True' in g and 'nrs=2' in g for g in got)
