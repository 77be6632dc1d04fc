"""Drop-in surface for `musicnlp.models.transformer_xl` (reference: musicnlp/models/transformer_xl.py:15-241).

Same names, constructor arguments, presets and output fields as the reference's `MyTransfoXLConfig` /
`MyTransfoXLLMHeadModel`; the arithmetic the reference inherits from HuggingFace `TransfoXLLMHeadModel` runs here on
the HIP engine (`xl_engine.XLEngine`).  Public tensors keep the reference's conventions: `input_ids`/`labels` (B, T)
int64, `mems` = list of n_layer tensors shaped (mem_len, B, d_model) (time-major, as upstream returns them),
`prediction_scores` = log-probabilities (B, T, V).
"""
import json
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import torch

from ._lib import MusicXLError
from .module import EngineModule
from .xl_engine import XLEngine

__all__ = ['MyTransfoXLConfig', 'MyTransfoXLLMHeadModel', 'TransfoXLLMHeadModelOutput']


class MyTransfoXLConfig:
    # reference presets, transformer_xl.py:16-23
    presets = {
        'debug': dict(d_model=128, n_head=8, n_layer=4),
        'debug-large': dict(d_model=128, n_head=8, n_layer=4),
        'tiny': dict(d_model=256, n_head=8, n_layer=6),
        'small': dict(d_model=512, n_head=8, n_layer=12),
        'base': dict(d_model=768, n_head=12, n_layer=12),
        'large': dict(d_model=1024, n_head=16, n_layer=18),
    }
    size2max_length = {'debug': 64, 'debug-large': 128, 'tiny': 512, 'small': 1024, 'base': 2048, 'large': 2048}
    model_type = 'transfo-xl'

    # upstream TransfoXLConfig defaults that stay in force (logged config, notebook/train/transformer-xl.ipynb cell 10)
    _hf_defaults = dict(
        vocab_size=267735, cutoffs=[20000, 40000, 200000], same_length=True, attn_type=0, untie_r=True, pre_lnorm=False,
        dropout=0.1, dropatt=0.0, adaptive=True, sample_softmax=-1, tie_projs=[False], tie_word_embeddings=True,
        layer_norm_epsilon=1e-5, init='normal', init_range=0.01, init_std=0.02, proj_init_std=0.01, eos_token_id=0,
        pad_token_id=None, div_val=1, proj_share_all_but_first=True,
    )

    def __init__(self, model_size: str = 'base', tokenizer=None, max_length: int = None, **kwargs):
        config = dict(self._hf_defaults)
        preset = dict(MyTransfoXLConfig.presets[model_size])
        hd_sz, n_head = preset['d_model'], preset['n_head']
        assert hd_sz % n_head == 0
        if 'debug' in model_size:
            m_len, c_len = 64, 64                                                  # :30-31
        else:
            m_len = max(128, self.size2max_length[model_size] // 8)               # :33
            c_len = max(1024, self.size2max_length[model_size] // 2)              # :34
        preset.update(d_embed=hd_sz, d_inner=hd_sz * 4, d_head=hd_sz // n_head, mem_len=m_len, clamp_len=c_len, div_val=1)
        config.update(preset)
        if tokenizer is not None:                                                  # :55-66
            vsz = config['vocab_size'] = tokenizer.vocab_size
            if vsz >= 32768 * 8:
                config['cutoffs'] = [20000, 40000, 200000]
            elif vsz >= 32768:
                config['cutoffs'] = [10000]
            elif vsz >= 16384:
                config['cutoffs'] = [5000]
            elif vsz >= 1000:
                config['cutoffs'] = [1000]
            else:
                config['cutoffs'] = []
        config.update(kwargs)                                                      # :67
        for k, v in config.items():
            setattr(self, k, v)
        self.model_size = model_size
        self.max_length_ = max_length or MyTransfoXLConfig.size2max_length[model_size]  # :70
        self.use_return_dict = True
        if self.dropatt != 0.0:
            raise NotImplementedError('dropatt != 0 is never used by the reference (HF default 0.0)')
        if len(self.cutoffs) > 3:
            raise NotImplementedError('at most 3 adaptive-softmax cutoffs')

    @property
    def model_meta(self) -> Dict[str, Any]:                                        # :72-77
        return dict(n_layer=self.n_layer, hidden_size=self.d_embed, ff_size=self.d_inner, seg_len=self.mem_len,
                    max_len=self.max_length_, vocab_size=self.vocab_size)

    def to_dict(self) -> Dict[str, Any]:
        return {k: v for k, v in self.__dict__.items() if not k.startswith('_') and k != 'use_return_dict'}

    def save_pretrained(self, path: str):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, 'config.json'), 'w') as f:
            json.dump(self.to_dict(), f, indent=2)

    @classmethod
    def from_pretrained(cls, path: str) -> 'MyTransfoXLConfig':
        with open(os.path.join(path, 'config.json')) as f:
            d = json.load(f)
        size = d.pop('model_size', 'base')
        max_length = d.pop('max_length_', None)
        return cls(model_size=size, max_length=max_length, **d)


@dataclass
class TransfoXLLMHeadModelOutput:
    """Fields of the reference's output class (transformer_xl.py:81-124)."""
    losses: Optional[torch.Tensor] = None
    prediction_scores: Any = None
    mems: Optional[List[torch.Tensor]] = None
    hidden_states: Any = None
    attentions: Any = None
    loss: Optional[torch.Tensor] = None

    @property
    def logits(self):  # log-probabilities, "behave the same way logits do" (:117-124)
        return self.prediction_scores

    def __getitem__(self, k):
        if isinstance(k, str):
            return getattr(self, k)
        return tuple(v for v in (self.loss, self.prediction_scores, self.losses, self.mems) if v is not None)[k]


class MyTransfoXLLMHeadModel(EngineModule):
    """`torch.nn.Module` (module.EngineModule): parameters are fp32 views into the engine's flat buffer under upstream's
    state-dict names, and a train-mode `loss` carries an autograd node whose backward is the engine's HIP backward -- the
    reference's `Trainer` loop (`loss.backward(); clip_grad_norm_; optimizer.step()`) drives it unchanged."""
    cls_name = 'TransformerXl'

    def __init__(self, config: MyTransfoXLConfig, device='cuda:0', seed: int = 77):
        super().__init__()
        self.config = config
        self.engine = XLEngine(config, device, seed=seed)
        self.device = torch.device(device)
        # upstream ties crit.out_layers.0.weight to the embedding (tie_word_embeddings, div_val == 1)
        self._bind_parameters(tied={'crit.out_layers.0.weight': 'transformer.word_emb.emb_layers.0.weight'})

    def save_pretrained(self, path: str):
        """HF layout: config.json + pytorch_model.bin with upstream parameter names."""
        self.config.save_pretrained(path)
        torch.save(self.state_dict(), os.path.join(path, 'pytorch_model.bin'))

    @classmethod
    def from_pretrained(cls, path: str, device='cuda:0'):
        config = MyTransfoXLConfig.from_pretrained(path)
        model = cls(config, device=device)
        model.load_state_dict(torch.load(os.path.join(path, 'pytorch_model.bin'), map_location='cpu'))
        return model

    # -- mems: API is upstream's time-major list; the engine is batch-major
    @staticmethod
    def _mems_in(mems):
        return None if mems is None else [m.transpose(0, 1).contiguous().to(torch.bfloat16) for m in mems]

    @staticmethod
    def _mems_out(mems):
        return None if mems is None else [m.transpose(0, 1) for m in mems]

    def forward(self, key_scores=None, input_ids: Optional[torch.Tensor] = None, mems=None, head_mask=None,
                inputs_embeds=None, labels: Optional[torch.Tensor] = None, output_attentions=None,
                output_hidden_states=None, return_dict=None):
        """Same contract as the reference forward (transformer_xl.py:130-221)."""
        if input_ids is None:
            raise ValueError('You have to specify input_ids (inputs_embeds is not used by the reference call sites)')
        if head_mask is not None or inputs_embeds is not None or output_attentions or output_hidden_states:
            raise NotImplementedError('head_mask / inputs_embeds / attention & hidden-state outputs are never requested '
                                      'by the reference (ignore_keys_for_eval, train.py:588)')
        input_ids = input_ids.to(self.device)
        if labels is not None:
            labels = labels.to(self.device)
        if mems is not None and len(mems) and mems[0].size(0) != self.config.mem_len:
            raise ValueError('mems must hold exactly mem_len rows (upstream init_mems/_update_mems invariant)')
        mems_in = self._mems_in(mems)
        out = self._run_engine(lambda: self.engine.forward(input_ids, mems=mems_in, labels=labels, train=self.training),
                               differentiable=self.training and labels is not None)
        in_eval = not self.training
        prediction_scores = out['logprobs'] if (labels is None or in_eval) else ()
        res = TransfoXLLMHeadModelOutput(loss=out['loss'], prediction_scores=prediction_scores, losses=out['losses'],
                                         mems=self._mems_out(out['mems']))
        if return_dict is False:
            return res[:]
        return res

    def prepare_inputs_for_generation(self, input_ids, past=None, **model_kwargs):
        """transformer_xl.py:223-241"""
        inputs = {}
        if past:
            assert isinstance(past, list)
            if isinstance(past[0], list):
                past = [torch.stack(p, dim=0) for p in past]
            inputs['mems'] = past
            inputs['input_ids'] = input_ids[:, -1].unsqueeze(-1)
        else:
            inputs['input_ids'] = input_ids
        return inputs

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor = None, max_length: int = None, do_sample: bool = False,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: float = 1.0, num_beams: int = 1,
                 penalty_alpha=None, typical_p=None, repetition_penalty=None, early_stopping=None,
                 renormalize_logits=None, num_return_sequences: int = 1, num_beam_groups: int = 1, length_penalty: float = 1.0,
                 use_graph: bool = True, seed: int = 77, attention_mask: Optional[torch.Tensor] = None,
                 eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, max_new_tokens: Optional[int] = None,
                 min_length: Optional[int] = None, grammar=None, n_bars=None, in_key=None, key=None, melody=None,
                 device_scorer: bool = False, register=None, melody_range=None, bass_range=None, bass_below=None,
                 kv_cache_dtype: Optional[str] = None, beam_rings: Optional[str] = None,
                 contrastive_rings: Optional[str] = None, prompt_rings: Optional[str] = None, form=None, section_bars=None,
                 form_span=None, **unused) -> torch.Tensor:
        """`model.generate(**inputs, **args)` as called at musicnlp/trainer/eval.py:333: the greedy, sample, contrastive and beam
        strategies (eval.py:277-321), beam search in its plain, sampling and diverse-group forms.  `num_return_sequences` expands the
        prompts as HF does (repeat_interleave).  Mode selection follows HF 4.25.1 `generate`: contrastive search when
        `penalty_alpha > 0`, `top_k > 1`, `do_sample` false and one beam; group beam search when `num_beam_groups > 1`.

        `attention_mask` (B, Tp) in HF's decoder-only layout: prompts of different lengths left-padded to one width (0 on the pad
        columns, then 1 on the prompt; `generate.left_pad` builds it).  Greedy and sampling decode every row as if it were alone:
        row b without its pad columns equals `generate(input_ids=ids[b:b+1, s_b:], max_length=max_length - s_b)` (DESIGN.md,
        ragged prompts).  The output keeps the input columns as given, pad ids included.  Beam, group-beam and contrastive
        search take no padded mask.

        Stopping at eos is opt-in: only an explicit `eos_token_id=` turns it on (the config's eos, 0 = [OMIT], is not adopted, so
        a call without it runs every row to max_length as before).  Then greedy decoding and sampling follow HF greedy_search /
        sample: a row that emits eos emits pad from then on (`pad_token_id`, else the config's, else eos), the call returns once
        every row has finished, cut to the longest row; `min_length` bars eos while a row is shorter.  `max_new_tokens` = n on an
        unpadded batch is max_length = prompt length + n (both given: ValueError, as HF).  Beam, group-beam and contrastive search
        keep their own eos handling, with an explicit eos_token_id / pad_token_id in place of the config's.

        `grammar` (a `grammar.TokenGrammar`, e.g. `tokenizer.grammar()`): greedy decoding and sampling in which every row may only
        emit tokens that its grammar state allows, so the output parses (`TimeSig Tempo [Key] (<bar> <melody> .. <bass> ..)* </s>`,
        a pitch before its duration, closed tuplets).  The state of every row is kept on the device and moves inside the sampler
        launch; barred tokens are masked after the repetition penalty and `min_length` and before the warpers, as an HF logits
        processor would.  It combines with `num_return_sequences`, padded prompts, `eos_token_id` / `min_length` /
        `max_new_tokens`; the prompts must obey the grammar themselves (MusicXLError otherwise).  That constraint is syntactic;
        `tokenizer.grammar(bar_budget=True)` adds the bar budget, under which every channel of every generated bar is also exactly
        as long as the row's time signature (rows with TimeSig_rare stay syntactic).  Plain beam search, group beam search and
        contrastive search take it too (below); beam-sample takes it with `device_scorer=True` only.

        `n_bars` (with `grammar` and an explicit `eos_token_id`; greedy decoding and sampling): length in bars.  An int, or a
        sequence or tensor of one int per prompt (repeated per prompt under `num_return_sequences`); a negative entry leaves that
        row unlimited.  A row with k >= 0 emits exactly k `<bar>` tokens: the bar that is open at the end of its prompt is
        completed and not counted, so 0 means "finish the open bar and stop".  While the row may still open bars eos is barred,
        once it has opened k a further `<bar>` is; under `tokenizer.grammar(bar_budget=True)` the row therefore emits eos exactly
        when its k-th bar is full, and pad from then on.  Without a budget (`tokenizer.grammar()`, or a row with TimeSig_rare)
        the rule still bars a further `<bar>` and an early eos but cannot force the stop: such a row may run to `max_length`.  A
        row that reaches `max_length` first is cut there.  The count lives on the device beside the grammar state and moves in the
        same sampler launch.  It combines with everything `grammar` combines with except `min_length` (ValueError).

        `in_key` (a `grammar.KeyRule`, `tokenizer.key_rule()`; greedy decoding and sampling): a row whose key is known emits only
        pitches of that key -- the pitches the in-key ratio (`metrics.ComputeMetrics`) counts as in key; rests and the rare-pitch
        token are never barred.  With `key=None` the key of a row is the last `Key_*` token of its prompt (pad columns skipped); a
        row without one stays unconstrained.  `key` = a key name ('AMinor', 'Key_AMinor') or ordinal in `vocab.KEY_NAMES`, or a
        sequence of one per prompt with None / -1 = unconstrained (repeated per prompt under `num_return_sequences`), overrides the
        prompts' keys.  The prompt only supplies the key: its own pitches are not judged.  A generated `Key_*` token sets the row's
        key from then on.  The key lives on the device beside the other rules' words and the mask sits in the same sampler launch,
        in the same place.  It needs no `grammar` and combines with everything greedy decoding and sampling take, and with
        plain beam search, group beam search and contrastive search (below); beam-sample takes it with `device_scorer=True` only.

        `melody` (with `grammar` and an explicit `eos_token_id`; greedy decoding and sampling): here is a melody, write the bass
        under it.  A guide is the concatenation of the `<bar> <melody> ... <bass>` spans of its bars, each bar up to and including
        its `<bass>` token (`tokenizer.melody_guide(ids, first_bar, n_bars)` cuts one from a piece); `melody` is one guide for every
        prompt or a list of one per prompt (repeated per prompt under `num_return_sequences`), where None leaves that row unguided.
        In every guided bar the span is fed to the row, not sampled -- on the device, inside the sampler launch of the captured
        step, as the mask "every token but this one is barred" -- and the row chooses the bass given all of it.  A bar that is open
        at the end of the prompt is finished freely; the guide engages at the next `<bar>`.  The row opens exactly the guide's bars
        and then ends: the guide sets the bar count, so `n_bars` is refused beside it, as is `min_length` (ValueError); under
        `tokenizer.grammar(bar_budget=True)` the row emits eos exactly when the bass of its last guided bar is full.  The guide must
        split into such bars, the grammar must accept them, and under a bar budget a guided melody must fill its bar exactly in a
        row whose time signature is known (MusicXLError naming row, guide index and token).  Guide tokens are not judged by
        `in_key`: real melodies hold off-key notes, as prompts do.  It combines with everything `grammar` combines with;
        `generate.check_melody` verifies an output.  Beam, group-beam and contrastive search take no `melody`.

        `register` (a `grammar.RegisterRule`, `tokenizer.register_rule()`) with `melody_range`, `bass_range` and `bass_below`: every
        part stays in its register, and the bass under the melody.  A range is an inclusive pair `(lo, hi)` of MIDI numbers (60 =
        `p_1/4`, middle C), one for every prompt or a sequence of one per prompt with None = unconstrained (repeated per prompt under
        `num_return_sequences`); between `<melody>` and `<bass>` a row emits only pitches inside its melody range, between `<bass>`
        and the next `<bar>` only pitches inside its bass range.  `bass_below=g` (g >= 0 semitones) also keeps every bass pitch at
        least g under the lowest melody note of its bar: 0 lets the bass touch that note, 1 keeps it strictly below.  The bound is
        per bar and not aligned in time -- "under the lowest melody note of the bar" is sufficient to keep the parts from crossing,
        not necessary.  Rests and the rare-pitch token are never barred, so a row always has a token left where a pitch may follow,
        even when its bounds leave no pitched one.  The prompt only sets the open part and the bar's lowest melody note, its pitches
        are not judged; notes fed by `melody=` are not judged either but do set the bound of their bar, so `melody=` with
        `bass_below=` writes the bass under the given melody.  The words live on the device beside the other rules' and the mask
        sits in the same sampler launch, in the same place.  It needs no `grammar` and combines with everything `in_key` combines
        with, the device searches included (given an explicit `eos_token_id=`); the host scorers refuse it.
        `generate.check_register` verifies an output.

        `form` (with `grammar` and an explicit `eos_token_id`; greedy decoding and sampling) with `section_bars` (default 1) and
        `form_span` ('bar', the default, or 'melody'): song form.  A row's generated bars are the bars it opens after its prompt,
        numbered from 0 (the bar open at the end of the prompt is finished freely and has no number, as `n_bars` counts).  `form` is
        a string of sections, one character each and `section_bars` bars long -- the first occurrence of a character is free, a
        later one repeats the first bar by bar, so 'AABA' with `section_bars=2` is the plan [-1, -1, 0, 1, -1, -1, 0, 1] -- or such
        a plan itself (entry k is -1 or an earlier bar j < k), or a list of one string, plan or None per prompt (repeated per prompt
        under `num_return_sequences`), where None leaves that row without a plan and without a bar limit.  A repeating bar is not
        sampled: behind its `<bar>` the row is fed the tokens of the source bar out of its own output -- on the device, inside the
        sampler launch of the captured step, as the mask "every token but this one is barred", exactly as `melody=` feeds a guide, so
        no launch and no host round trip is added -- with `form_span='bar'` the whole bar, with 'melody' up to and including its
        `<bass>`, after which the row writes a new bass under the same melody (with `register=` and `bass_below=`, under it).  The
        row opens exactly the planned bars and then ends: the plan sets the bar count, so `n_bars`, `melody` and `min_length` are
        refused beside it (ValueError), as are `section_bars` / `form_span` without `form`, `section_bars < 1`, an empty form, a plan
        entry outside -1..k-1, a wrong number of forms and any other `form_span`; under `tokenizer.grammar(bar_budget=True)` the row
        emits eos exactly when its last bar is full.  Copied tokens are not judged by the other rules but move their words; a form
        without repeats ('ABC') is `n_bars`.  Only generated bars can be sources, never bars of the prompt.  It combines with
        everything `melody` combines with; `generate.check_form` verifies an output.  Beam, group-beam and contrastive search take no
        `form`, nor do the sub-word tokenizers, whose grammar carries no repeat rule.

        Plain beam search (`num_beams` 2..16, `num_beam_groups=1`, `do_sample=False`) runs with its scorer on the device
        (`generate.beam_search_device`: mxl_beam_step / mxl_beam_reorder inside the captured step) and takes `grammar`, `n_bars` and
        `in_key` / `key` with the checks above, given an explicit `eos_token_id=` (without one they stay refused, as before); per-prompt values are shared by the prompt's beams, a barred token is -inf before
        the running scores are added, and a prompt left with fewer than `num_return_sequences` hypotheses raises MusicXLError.
        `MXL_BEAM_HOST=1` keeps the host scorer (`generate.beam_search`), which takes no rules.

        Group (diverse) beam search (`num_beam_groups` 2.., dividing `num_beams` 2..16, `diversity_penalty`, `do_sample=False` -- the
        reference's 'beam' strategy runs `num_beams=4, num_beam_groups=2`) can run with its scorer on the device too
        (`generate.group_beam_search_device`: mxl_group_beam_step, which walks the groups of every prompt in order inside one launch,
        then mxl_beam_reorder, inside the captured step) and returns what the host path returns.  That path is taken when a rule is
        given, or with `MXL_GROUP_BEAM_DEVICE=1`; a call without a rule keeps the host scorer until the device path has been measured
        against it (profiles/group_beam_step.txt).  It takes `grammar` (with or without
        a bar budget) and `in_key` / `key` with the checks above, given an explicit `eos_token_id=` (without one they stay refused):
        per-prompt values are shared by the prompt's beams, a barred token is -inf before the diversity penalty and the running
        scores are added, and a beam that continues at -inf does not count as a choice of its token.  `n_bars`, `melody` and padded
        prompts stay refused.  `MXL_BEAM_HOST=1` keeps the host scorer here as well (`generate.group_beam_search`, no rules), as
        does a `diversity_penalty` that is negative or infinite.

        Beam-sample (`num_beams` 2.., `num_beam_groups=1`, `do_sample=True` -- the reference's default 'beam' settings) runs its
        scorer on the host (`generate.beam_search(do_sample=True)`: `_warp`, torch.multinomial from a generator seeded with `seed`)
        and takes no rules.  `device_scorer=True` (opt-in) runs it on the device instead (`generate.beam_sample_device`: the rules
        mask, mxl_beam_sample_draw -- the warpers with two tokens kept, the renormalisation and the draw of `2 * num_beams`
        candidates per item without replacement, by Gumbel-top-k -- and mxl_beam_sample_step inside the captured step).  It is no
        default because its draw is another random stream than torch.multinomial's: the same `seed` returns other ids, while a call
        without the keyword returns what it always did.  With the keyword the call takes `grammar` (with or without a bar budget)
        and `in_key` / `key` with the checks above, given an explicit `eos_token_id=`; per-prompt values are shared by the
        prompt's `num_return_sequences` items and their beams.  `n_bars`, `melody` and padded prompts stay refused.  The keyword
        raises MusicXLError without `renormalize_logits=True` (the reference always sets it), for a vocabulary above 2048 tokens,
        for `num_beams` outside 2..16 and under `MXL_BEAM_HOST=1`, and ValueError with any other strategy or with a
        `repetition_penalty` other than None / 1.0 (the beam arms apply none).

        Contrastive search (`penalty_alpha > 0`, `top_k` 2..32) runs with its whole step on the device
        (`generate.contrastive_search_device`: mxl_contrastive_topk / mxl_contrastive_step / mxl_ring_slot_broadcast inside the captured
        step; `use_graph` is honoured) and returns what the host path returns.  It takes `grammar` (with or without a bar budget) and
        `in_key` / `key` with the checks above, given an explicit `eos_token_id=` (without one they stay refused, as before): per-prompt
        values are shared by the prompt's `top_k` rows, a barred token is -inf before the top-k, where HF's logits processors sit, and
        a barred candidate is never picked.  `n_bars`, `melody` and padded prompts stay refused.  `top_k > 32` or
        `MXL_CONTRASTIVE_HOST=1` keeps the host-driven loop (`generate.contrastive_search`), which takes no rules here.

        `kv_cache_dtype` (greedy decoding and sampling): the format of the decoder's K/V rings.  None or 'bf16': bf16, as ever.  'fp8'
        (alias 'fp8_e4m3'): OCP e4m3fn bytes with one power-of-two int8 exponent per ring slot and head (DESIGN.md, FP8 rings) --
        (dh + 1) / (2 dh) of the ring memory and of the attention launch's bytes, at the price of K and V rounded to four
        significant bits, so the output is another one than the bf16 rings give.  It combines with everything greedy decoding and
        sampling take (rules, eos, padded prompts, `num_return_sequences`, the two-lane decoder, `use_graph`, the large-vocabulary
        sampler).  Beam, beam-sample, group-beam and contrastive search refuse 'fp8' (ValueError): they move rings with
        mxl_beam_reorder / mxl_ring_slot_broadcast, which know the bf16 layout alone.  Any other string is a ValueError.
        `MXL_KV_DTYPE=fp8` sets the default of calls that do not pass the keyword (an A/B knob; unset, nothing changes).

        `beam_rings` (plain beam, group beam and beam-sample with `device_scorer=True`, scorer on the device): how the K/V rings follow
        the beams.  None or 'copied': every step copies whole ring rows (mxl_beam_reorder), as ever.  'indexed' (opt-in): the rings
        stay where the forward pass wrote them; a ring slot written for a position never changes, so a beam points at the slot in
        its ancestor's ring, an owner table of `mem_len` bytes per row follows the beams (mxl_beam_owner_follow) and the attention
        reads through it (mxl_relattn_decode_owned; DESIGN.md, indexed rings).  The ids and scores are the ones 'copied' returns, with
        every rule those paths take and with `use_graph` on and off; `mem_len` must be a multiple of 16.  An explicit 'indexed' is a
        ValueError under greedy decoding, sampling and contrastive search, under the host scorers (`MXL_BEAM_HOST=1`, more than 16
        beams, beam-sample without `device_scorer`) and with `kv_cache_dtype='fp8'`; any other string is a ValueError.
        `MXL_BEAM_RINGS=indexed` sets the default of calls that do not pass the keyword and is ignored where 'indexed' does not apply.
        'indexed_fp8' (opt-in, the same searches): 'indexed' over FP8 rings -- the search's decoder is built with the ring format of
        `kv_cache_dtype='fp8'`, the rings are never moved and mxl_relattn_decode_fp8_owned reads bytes and exponents through the owner
        table: (dh + 1) / (2 dh) of the ring memory, so twice the beams, prompts or `mem_len` in the same memory.  K and V are rounded
        to four significant bits, so ids and scores are other ones than the bf16 rings give.  It applies and is refused exactly where
        'indexed' is (and `MXL_BEAM_RINGS=indexed_fp8` is ignored there); a `d_head` other than 16, 32 or 64 is a MusicXLError.  The
        spelling is this one value: `kv_cache_dtype='fp8'` keeps raising under every search, with either `beam_rings`.

        `contrastive_rings` (contrastive search with its step on the device): how the K/V rings are held.  None or 'copied': every one of
        the `top_k` candidate rows of a prompt owns a full set of rings, and the one slot a step writes follows the pick
        (mxl_ring_slot_broadcast), as ever.  'shared' (opt-in): those rows differ in that one slot alone, so a prompt keeps one set of
        rings, (prompts, H, mem_len, dh) per layer -- 1 / `top_k` of the ring memory -- the prompt pass runs once per prompt, and the
        attention of a step reads a prompt's ring once per group of 8 candidates (4 for `top_k` <= 4) for all of them, each taking the
        step's own slot from its own row (mxl_kv_stash / mxl_relattn_decode_shared / mxl_kv_commit_shared; DESIGN.md, shared rings).
        The attention output is the copied mode's bit for bit at the same number of ring pieces, so the ids are the ones 'copied'
        returns with every rule that path takes and with `use_graph` on and off -- by construction for `mem_len` < 1024, where both
        modes run one piece, and wherever else `generate.XLDecoder.pieces` agrees (MXL_DECODE_PIECES pins it); `d_head` must be 16, 32
        or 64 and the scores of a workgroup must fit 160 KiB of shared memory (any `mem_len` up to 4096 does), else MusicXLError.  An
        explicit 'shared' is a ValueError under greedy decoding, sampling and every beam arm, under the host-driven loop
        (`top_k > 32`, `MXL_CONTRASTIVE_HOST=1`) and with `kv_cache_dtype='fp8'`; any other string is a ValueError.
        `MXL_CONTRASTIVE_RINGS=shared` sets the default of calls that do not pass the keyword and is ignored where 'shared' does not
        apply.

        `prompt_rings` (sampling with `num_return_sequences` = n >= 2): how the K/V rings of the n rows of a prompt are held.  None or
        'copied': the batch is expanded and every row owns a full set of rings, filled by a prompt pass over all rows, as ever.
        'shared' (opt-in): the rows of a prompt differ only in the positions generated after it, so a prompt keeps one set of prompt
        rings, (prompts, H, mem_len, dh) per layer, written once by a prompt pass of the unexpanded batch, and every row a tail ring,
        (rows, H, Mt, dh) with Mt = min(mem_len, max_length - prompt length rounded up to 16), for what it generates; the attention of
        a step takes each ring slot from the one or the other by its position (mxl_kv_append_tail / mxl_relattn_decode_prefix;
        DESIGN.md, prompt rings).  The attention output is the copied mode's bit for bit at the same number of ring pieces and the draw
        is keyed by seed, row and step, so the ids are the ones 'copied' returns for the same seed, with every rule sampling takes
        (`grammar`, `n_bars`, `in_key` / `key`, `register`, `melody`), eos / `min_length` / `max_new_tokens`, left-padded prompts,
        `use_graph` on and off, the large-vocabulary sampler and the adaptive head -- below 32 rows, and from 32 rows on when the
        default's half-batch lane cut falls between two prompts (the lanes here are cut between prompts; otherwise the lane seeds
        differ and the output is another valid sample); and for `mem_len` >= 1024 wherever `generate.XLDecoder.pieces` agrees
        (MXL_DECODE_PIECES pins it).  `d_head` must be 16, 32 or 64, `mem_len` a multiple of 16 whose scores fit 160 KiB of shared
        memory (any `mem_len` up to 4096 does), else MusicXLError.  An explicit 'shared' is a ValueError with `num_return_sequences`
        == 1, under greedy decoding, every beam arm and contrastive search, and with `kv_cache_dtype='fp8'`; any other string is a
        ValueError.  `MXL_PROMPT_RINGS=shared` sets the default of calls that do not pass the keyword and is ignored where 'shared'
        does not apply."""
        from .generate import (BEAM_MAX, CONTRASTIVE_MAX, XLDecoder, XLDecoderLanes, beam_generate, beam_sample_device,
                               beam_search_device, check_grammar_args, contrastive_search, contrastive_search_device, form_config,
                               group_beam_search_device, left_pad_counts, plan_search, prompt_rings_misfit, prompt_tail_len,
                               resolve_beam_rings, resolve_contrastive_rings, resolve_kv_dtype, resolve_prompt_rings,
                               resolve_max_length, rules_config, sampling_config, stop_config)
        kv_dtype = resolve_kv_dtype(kv_cache_dtype)
        n_pad = None
        if attention_mask is not None:
            pads = left_pad_counts(attention_mask, tuple(input_ids.shape))
            if any(pads):
                n_pad = torch.tensor(pads, dtype=torch.int32)
        # HF 4.25.1 fills unspecified generation arguments from the model config; PretrainedConfig's default top_k is 50, so
        # `generate(do_sample=True)` without top_k samples from the 50 best tokens (the reference relies on these defaults)
        top_k = getattr(self.config, 'top_k', 50) if top_k is None else top_k
        diversity_penalty = unused.pop('diversity_penalty', None)
        if n_pad is not None and (max_new_tokens is not None or unused.get('stopping_criteria') is not None):
            raise MusicXLError('padded prompts: max_new_tokens and stopping_criteria are not supported (give max_length; '
                               'eos_token_id stops rows)')
        stop = stop_config(eos_token_id, pad_token_id, min_length, self.config.pad_token_id)
        self._maybe_resync()
        max_length = resolve_max_length(max_length, max_new_tokens, input_ids.shape[1], self.config.max_length_)
        check_grammar_args(grammar, self.config.vocab_size, stop)
        plan = plan_search(dict(beam=BEAM_MAX, group_beam=BEAM_MAX, contrastive=CONTRASTIVE_MAX, beam_sample=BEAM_MAX),   # on the device
                           num_beams=num_beams, num_beam_groups=num_beam_groups, do_sample=do_sample, penalty_alpha=penalty_alpha,
                           top_k=top_k, diversity_penalty=diversity_penalty, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                           config_eos=self.config.eos_token_id, config_pad=self.config.pad_token_id, padded=n_pad is not None,
                           grammar=grammar, n_bars=n_bars, in_key=in_key, key=key, melody=melody, form=form, device_scorer=device_scorer,
                           repetition_penalty=repetition_penalty, renormalize_logits=renormalize_logits,
                           vocab_size=self.config.vocab_size, register=register)
        # (before the fp8 refusal: an explicit 'shared' beside kv_cache_dtype='fp8' is refused for what it asks, wherever it is asked)
        shared = resolve_contrastive_rings(contrastive_rings, plan.strategy == 'contrastive' and plan.device and kv_dtype is None) == 'shared'
        per_prompt = resolve_prompt_rings(prompt_rings, plan.strategy == 'sample' and bool(do_sample) and num_return_sequences >= 2
                                          and kv_dtype is None) == 'shared'
        if kv_dtype is not None and plan.strategy != 'sample':
            name = dict(beam='beam', beam_sample='beam-sample', group_beam='group-beam', contrastive='contrastive')[plan.strategy]
            raise ValueError(f"kv_cache_dtype='{kv_dtype}' is not supported under {name} search: it moves rings with "
                             'mxl_beam_reorder / mxl_ring_slot_broadcast, which take bf16 rings alone; greedy decoding and sampling do')
        rings = resolve_beam_rings(beam_rings, plan.device and plan.strategy in ('beam', 'group_beam', 'beam_sample') and kv_dtype is None
                                   and self.config.mem_len % 16 == 0, self.config.d_head)
        # 'indexed_fp8' is the decoder's 'indexed' mode on a decoder with FP8 rings; every other call builds the decoder it built
        fp8_rings = dict(kv_dtype='fp8') if rings == 'indexed_fp8' else {}
        rings = 'indexed' if fp8_rings else rings
        B0 = input_ids.shape[0]
        ranges = dict(register=register, melody_range=melody_range, bass_range=bass_range, bass_below=bass_below)
        feed = form_config(form, section_bars, form_span, B0, grammar, stop, n_bars, melody, min_length, num_return_sequences)
        rules = rules_config(batch=B0, vocab_size=self.config.vocab_size, stop=stop, grammar=grammar, n_bars=n_bars, in_key=in_key,
                             key=key, melody=melody if feed is None else feed, **ranges, repeat=num_return_sequences)
        if rules.register is None:
            ranges = {}                                     # (a call without the rule hands nothing of it on)
        ends = dict(eos_token_id=plan.eos, pad_token_id=plan.pad)
        if plan.strategy == 'contrastive':
            # shared rings are another decoder; every other call builds the decoder it built
            dec = XLDecoder(self.engine, B0 * top_k, max_length, seed=seed, **(dict(shared_rings=top_k) if shared else {}))
            if plan.device:
                return contrastive_search_device(dec, input_ids, max_length, top_k=top_k, penalty_alpha=penalty_alpha, use_graph=use_graph,
                                                 grammar=grammar, in_key=in_key, key=key, **ranges, **ends,
                                                 **(dict(contrastive_rings='shared') if shared else {}))
            return contrastive_search(dec, input_ids, max_length, top_k=top_k, penalty_alpha=penalty_alpha, **ends)
        if plan.device:                                     # (the device searches plan per-prompt values per beam themselves)
            beams = dict(num_beams=num_beams, early_stopping=bool(early_stopping), length_penalty=length_penalty,
                         num_return_sequences=num_return_sequences, use_graph=use_graph, grammar=grammar, in_key=in_key, key=key, **ranges,
                         **ends, beam_rings=rings)
            if plan.strategy == 'beam_sample':
                dec = XLDecoder(self.engine, B0 * num_return_sequences * num_beams, max_length, seed=seed, **fp8_rings)
                return beam_sample_device(dec, input_ids, max_length, top_k=top_k, top_p=top_p, temperature=temperature,
                                          typical_p=typical_p, **beams)
            dec = XLDecoder(self.engine, B0 * num_beams, max_length, seed=seed, **fp8_rings)
            if plan.strategy == 'beam':
                return beam_search_device(dec, input_ids, max_length, n_bars=n_bars, **beams)
            return group_beam_search_device(dec, input_ids, max_length, num_beam_groups=num_beam_groups,
                                            diversity_penalty=diversity_penalty or 0.0, **beams)
        if plan.strategy != 'sample':
            return beam_generate(lambda rows: XLDecoder(self.engine, rows, max_length, seed=seed), input_ids, max_length,
                                 num_beams=num_beams, num_beam_groups=num_beam_groups, do_sample=do_sample,
                                 num_return_sequences=num_return_sequences, seed=seed, top_k=top_k, top_p=top_p,
                                 temperature=temperature, typical_p=typical_p, early_stopping=early_stopping,
                                 renormalize_logits=renormalize_logits, length_penalty=length_penalty,
                                 diversity_penalty=diversity_penalty, **ends)
        if num_return_sequences > 1:
            if not do_sample:
                raise ValueError('num_return_sequences has to be 1 when doing greedy search')       # HF's message
            input_ids = input_ids.repeat_interleave(num_return_sequences, 0)
            if n_pad is not None:
                n_pad = n_pad.repeat_interleave(num_return_sequences, 0)
        B = input_ids.shape[0]
        dec = getattr(self, '_decoder', None)
        # two free-running half-batch lanes from 32 rows on (generate.XLDecoderLanes); MXL_DECODE_LANES=1 keeps one decoder
        lanes = max(1, int(os.environ.get('MXL_DECODE_LANES', '2'))) if (B >= 32 and use_graph) else 1
        # prompt rings (opt-in) are another decoder: one set of prompt rings per prompt, a tail ring per row, lanes cut between prompts
        rings = {}
        if per_prompt:
            cut = min(lanes, B0)
            misfit = prompt_rings_misfit(self.config, num_return_sequences, -(-B0 // cut) * num_return_sequences)
            if misfit and prompt_rings is not None:
                raise MusicXLError(misfit)
            if not misfit:                                  # (the environment's default is ignored where the model does not fit)
                lanes, rings = cut, dict(prompt_rings=num_return_sequences, tail_len=max_length - input_ids.shape[1])
        # the ring format, the rows per prompt ring and the slots of a tail ring: what the cached decoder must have been built for
        spec = (kv_dtype, rings.get('prompt_rings', 0), prompt_tail_len(self.config.mem_len, rings['tail_len']) if rings else None)
        if dec is None or dec.B != B or dec.Tmax < max_length or getattr(dec, 'n', 1) != lanes or dec.ring_spec != spec:
            dec = self._decoder = (XLDecoderLanes(self.engine, B, max_length, seed=seed, lanes=lanes, kv_dtype=kv_dtype, **rings)
                                   if lanes > 1 else XLDecoder(self.engine, B, max_length, seed=seed, kv_dtype=kv_dtype, **rings))
        dec.invalidate_tables()
        return dec.run(input_ids.to(self.device), max_length,
                       sampling_config(do_sample, top_k, top_p, temperature, repetition_penalty, typical_p), rules, use_graph,
                       None if n_pad is None else n_pad.to(self.device))
