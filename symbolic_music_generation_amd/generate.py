"""Autoregressive generation for the TransfoXL engine: the on-device counterpart of `model.generate(...)` as the
reference calls it (musicnlp/trainer/eval.py:277-333; HF 4.25.1 GenerationMixin.greedy_search / sample).

    prompt forward (whole prompt, zero mems)  ->  K/V rings filled
    loop:  [embed -> L x (qkv GEMM, kv append, ring attention, o GEMM, LN, FFN GEMMs, LN) -> head GEMM -> log-softmax
            -> sampler -> advance]            one hipGraph replay per token, no host round trip

Strategies mirrored from `MusicGenerator` (eval.py:277-326): greedy (do_sample=False) and sampling with
`top_k`, `top_p`, `typical_p`, `temperature`, `repetition_penalty` and renormalised logits -- every key the `sample`
strategy accepts (eval.py:279) -- and beam search (`strategy='beam'`, eval.py:302-321: HF `beam_search` / `beam_sample` with
`BeamSearchScorer`), which runs the same per-token kernels eagerly with the beam bookkeeping between steps (beam_search).
Contrastive search (`strategy='contrastive'`, eval.py:296-302) runs over the Transformer-XL mems with one decoder row per
candidate: its whole step on the device, captured like the sampling step (contrastive_search_device), with the host-driven loop
(contrastive_search) as the reference.  The Reformer (`past_buckets_states`) cannot serve it, as in the reference.
"""
import math
import os
from collections import deque, namedtuple
from contextlib import nullcontext
from typing import Optional

import torch

from . import ops
from ._lib import MusicXLError
from .rings import FP8Rings, PromptRings, RingLayout, SharedRings, prompt_tail_len        # noqa: F401 (prompt_tail_len: re-exported)


STOP_CHUNK = 16          # decode steps per chunk between reads of the live-row count (run_until_finished)


def stop_config(eos_token_id: Optional[int], pad_token_id: Optional[int] = None, min_length: Optional[int] = None,
                config_pad_token_id: Optional[int] = None) -> Optional[tuple]:
    """(eos, pad, min_length) of a generation that stops at eos, or None when no eos is given: stopping is opt-in, an explicit
    `eos_token_id=` argument.  pad: the argument, else the config's pad_token_id, else eos (HF 4.25.1).  min_length (HF
    MinLengthLogitsProcessor) acts only together with an eos; 0 = off."""
    if eos_token_id is None:
        return None
    eos = int(eos_token_id)
    pad = pad_token_id if pad_token_id is not None else config_pad_token_id
    pad = eos if pad is None else int(pad)
    return eos, pad, max(int(min_length or 0), 0)


def sampling_config(do_sample: bool = False, top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: float = 1.0,
                    repetition_penalty: Optional[float] = None, typical_p: Optional[float] = None) -> dict:
    """the sampler arguments of one generation as every decoder passes them on (`begin`, `step`, ops.sample / ops.sample_step): a
    plain dict of these six keys with the 'off' values filled in (top_k 0; top_p, repetition_penalty, typical_p 1.0).  Its sorted
    items are part of XLDecoder's graph key."""
    return dict(do_sample=do_sample, top_k=top_k or 0, top_p=1.0 if top_p is None else top_p, temperature=temperature,
                repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty,
                typical_p=1.0 if typical_p is None else typical_p)


def sample_unfused(scores: torch.Tensor, V: int, ids: torch.Tensor, t_dev: torch.Tensor, rng: torch.Tensor, seed: int, sampling: dict,
                   rules: Optional[ops.RuleState] = None):
    """The sampler tail as separate launches (what mxl_sample_step does in one): next token of every row from the first V columns
    of `scores` -> ids[:, t + 1], position and RNG counters advanced, under those of `rules` (an ops.RuleState) that are in force;
    the repeat rule's mask reads `ids` as the rows' history.  The mask writes into `scores` in place.  Four launches, two where no
    rule is in force."""
    rules = (ops.RuleState() if rules is None else rules).in_force()
    sc = scores[:, :V] if scores.shape[1] != V else scores
    # HF's processor order is penalty, min_length, grammar, warpers; here the penalty runs inside the sampler, after the mask: -inf
    # stays -inf under it, so the result is the same
    ops.rules_mask(sc, V, t_dev, rules, hist=ids if rules.repeat is not None else None)
    ops.sample(sc, ids, t_dev, rng, seed, **sampling)
    ops.decode_advance(t_dev, rng)
    # the words move before the stop rule rewrites `unfinished`, which still tells which rows chose their token
    ops.rules_advance(ids, t_dev, rules)


def resolve_max_length(max_length: Optional[int], max_new_tokens: Optional[int], prompt_len: int, default: int) -> int:
    """HF 4.25.1: max_new_tokens = n stands for max_length = prompt length + n; giving both raises ValueError"""
    if max_new_tokens is not None:
        if max_length is not None:
            raise ValueError('Both `max_new_tokens` and `max_length` have been set but they serve the same purpose -- setting a '
                             'limit to the generated output length. Remove one of those arguments.')
        return int(prompt_len) + int(max_new_tokens)
    return int(max_length or default)


def finish_at_eos(ids: torch.Tensor, prompt_len: int, eos: int, pad: int) -> torch.Tensor:
    """Host reference of stopping at eos, applied to the output of a run without it: in every row, each column after the first
    GENERATED eos (column >= prompt_len) becomes pad; the result is cut to W = (last such eos column over the rows) + 1 when
    every row has one, else kept whole.  Rows are independent and sampling draws per (seed, row, step), so a run with
    eos_token_id returns exactly this (HF greedy_search / sample: next = next * unfinished + pad * (1 - unfinished))."""
    out = ids.clone()
    gen = out[:, prompt_len:]
    if gen.shape[1] == 0:
        return out
    hit = gen == eos
    has = hit.any(1)
    first = torch.where(has, hit.int().argmax(1), torch.full_like(has, gen.shape[1], dtype=torch.int64))
    col = torch.arange(gen.shape[1], device=ids.device)[None, :]
    gen.masked_fill_(col > first[:, None], pad)
    if bool(has.all()):
        return out[:, :prompt_len + int(first.max()) + 1]
    return out


def stop_width(ids: torch.Tensor, unfinished: torch.Tensor, prompt_len: int, max_length: int, eos: int) -> int:
    """returned width of a generation with stopping: max_length if a row is still live, else the last first-eos column + 1"""
    if bool((unfinished != 0).any()):
        return max_length
    first = (ids[:, prompt_len:max_length] == eos).int().argmax(1)
    return prompt_len + int(first.max()) + 1


def check_grammar_args(grammar, vocab_size: int, stop: Optional[tuple]):
    """what generation under a grammar (grammar.TokenGrammar) needs on the host: the grammar classifies exactly the model's
    vocabulary, and with min_length no reachable state allows the eos token alone -- min_length bars eos, which would leave such a
    row with every token barred"""
    if grammar is None:
        return
    if grammar.vocab_size != int(vocab_size):
        raise MusicXLError(f'the grammar classifies {grammar.vocab_size} tokens, the model has vocab_size {int(vocab_size)}')
    if stop is not None and stop[2] > 0:
        only = grammar.only_token_states(stop[0])
        if only:
            raise ValueError(f'min_length with a grammar whose state {grammar.state_names[only[0]]} allows only the eos token '
                             f'{stop[0]}: below min_length that row would have every token barred')
        only = grammar.budget.only_token_states(stop[0]) if grammar.budget is not None else []
        if only:
            s, bar, rem = only[0]
            raise ValueError(f'min_length with a bar budget under which state {grammar.state_names[s]} with bar {bar} and {rem} slots '
                             f'free allows only the eos token {stop[0]}: below min_length that row would have every token barred')


def bar_count_config(n_bars, batch: int, grammar, stop: Optional[tuple], repeat: int = 1) -> Optional[torch.Tensor]:
    """`n_bars` of a generation as the decoders take it: None, or a (batch * repeat,) int32 CPU tensor of the bars every row may
    still open, negative = no limit.  n_bars: an int, or a sequence or tensor of `batch` ints, one per prompt; `repeat` =
    num_return_sequences (every prompt's value repeated, as the prompts are).  Raises ValueError for what the rule cannot work
    with: no grammar or a grammar without a bar count; no explicit eos (only the eos rule finishes a row: stopping stays opt-in);
    an eos that is no `end` token of the grammar (the rule would bar it while bars are left and have no say over the real end);
    min_length (it bars eos where the count may leave nothing else: a row with every token barred); a wrong length."""
    if n_bars is None:
        return None
    if grammar is None:
        raise ValueError('n_bars needs grammar=: bars are counted by the token grammar (tokenizer.grammar(bar_budget=True))')
    cnt = grammar.bar_count
    if cnt is None:
        raise ValueError('n_bars needs a grammar with a bar count (grammar.BarCount; the music grammar has one), this one has none')
    if stop is None:
        raise ValueError('n_bars needs an explicit eos_token_id=: a row ends by emitting eos, and stopping at eos is opt-in')
    eos = stop[0]
    if not 0 <= eos < grammar.vocab_size or not (cnt.end >> int(grammar.cls[eos])) & 1:
        raise ValueError(f'n_bars: eos_token_id {eos} is no `end` token of the grammar\'s bar count {cnt!r}')
    if stop[2] > 0:
        raise ValueError('n_bars together with min_length: min_length bars eos where the bar count may allow nothing else, which '
                         'would leave a row with every token barred')
    if isinstance(n_bars, (bool, float)) or (isinstance(n_bars, torch.Tensor) and (n_bars.is_floating_point() or n_bars.dtype == torch.bool)):
        raise ValueError('n_bars must be an int or a sequence or tensor of ints')
    if isinstance(n_bars, int):
        k = torch.full((batch,), n_bars, dtype=torch.int64)
    else:
        k = torch.as_tensor(n_bars).detach().cpu().to(torch.int64).reshape(-1)
        if k.numel() != batch:
            raise ValueError(f'n_bars holds {k.numel()} entries for {batch} prompts: give an int or one per prompt')
    return k.clamp(-1, 2 ** 31 - 1).to(torch.int32).repeat_interleave(int(repeat), 0).contiguous()


def key_config(in_key, key, batch: int, vocab_size: int, repeat: int = 1) -> Optional[torch.Tensor]:
    """`in_key` / `key` of a generation as the decoders take them: None (no rule, or every row takes the key of its prompt), or a
    (batch * repeat,) int32 CPU tensor of key ordinals, -1 = the row is unconstrained -- it overrides the prompts' keys.  key: a key
    name ('AMinor' or 'Key_AMinor') or ordinal in vocab.KEY_NAMES, or a sequence or tensor of `batch` of them, one per prompt, with
    None / -1 for an unconstrained row; `repeat` = num_return_sequences.  Raises MusicXLError for a rule over another vocabulary and
    ValueError for a key without the rule, an unknown key or a wrong length."""
    from .grammar import key_ordinal
    if in_key is None:
        if key is not None:
            raise ValueError('key= needs in_key=, the key rule (tokenizer.key_rule())')
        return None
    if in_key.vocab_size != int(vocab_size):
        raise MusicXLError(f'the key rule spans {in_key.vocab_size} tokens, the model has vocab_size {int(vocab_size)}')
    if key is None:
        return None
    if isinstance(key, torch.Tensor):
        key = key.detach().cpu().reshape(-1).tolist() if key.dim() else int(key)
    one = isinstance(key, (str, int)) and not isinstance(key, bool)
    ks = [key_ordinal(key)] * batch if one else [key_ordinal(k) for k in key]
    if len(ks) != batch:
        raise ValueError(f'key holds {len(ks)} entries for {batch} prompts: give one key or one per prompt')
    return torch.tensor(ks, dtype=torch.int32).repeat_interleave(int(repeat), 0).contiguous()


class RegisterPlan:
    """The register rule of one generation as the decoders take it (register_config): `rule` (a grammar.RegisterRule), `bounds`
    (B,) int32 on the CPU, every row's lo_melody, hi_melody, lo_bass, hi_bass packed as the rule's `range` word, and `gap` (-1 = the
    bass is not tied to the melody)"""

    def __init__(self, rule, bounds: torch.Tensor, gap: int):
        self.rule, self.bounds, self.gap = rule, bounds, int(gap)

    @property
    def B(self) -> int:
        return self.bounds.numel()

    def rows(self, lo: int, hi: int) -> 'RegisterPlan':
        return RegisterPlan(self.rule, self.bounds[lo:hi].contiguous(), self.gap)


def _ranges_per_row(r, batch: int, what: str) -> list:
    """`melody_range` / `bass_range` as generate takes them -> one (lo, hi) per prompt: None = unconstrained, one pair of MIDI
    numbers for every prompt, or a sequence of `batch` pairs with None for an unconstrained row"""
    def pair(x):
        if x is None:
            return (0, 127)
        x = x.tolist() if isinstance(x, torch.Tensor) else x
        if isinstance(x, (str, bytes)) or not hasattr(x, '__len__') or len(x) != 2 or any(
                isinstance(v, (bool, float, str)) or not hasattr(v, '__index__') for v in x):
            raise ValueError(f'{what} is a pair (lo, hi) of MIDI numbers, None, or one of those per prompt')
        lo, hi = int(x[0]), int(x[1])
        if not (0 <= lo <= 127 and 0 <= hi <= 127):
            raise ValueError(f'{what}: ({lo}, {hi}) lies outside the MIDI numbers 0..127')
        if lo > hi:
            raise ValueError(f'{what}: lo {lo} is above hi {hi}')
        return (lo, hi)
    if isinstance(r, torch.Tensor):
        r = r.detach().cpu().tolist()
    if r is None or (isinstance(r, (list, tuple)) and len(r) == 2 and all(hasattr(v, '__index__') and not isinstance(v, bool)
                                                                            for v in r)):
        return [pair(r)] * batch
    if not isinstance(r, (list, tuple)):
        raise ValueError(f'{what} is a pair (lo, hi) of MIDI numbers, None, or one of those per prompt')
    if len(r) != batch:
        raise ValueError(f'{what} holds {len(r)} entries for {batch} prompts: give one pair or one per prompt')
    return [pair(x) for x in r]


def register_config(register, melody_range, bass_range, bass_below, batch: int, vocab_size: int, repeat: int = 1) -> Optional[RegisterPlan]:
    """`register` / `melody_range` / `bass_range` / `bass_below` of a generation as the decoders take them: None (no rule), or a
    RegisterPlan over batch * repeat rows (`repeat` = num_return_sequences: every prompt's bounds repeated, as the prompts are).
    melody_range / bass_range: one inclusive pair (lo, hi) of MIDI numbers or one per prompt, None = unconstrained.  bass_below: None
    (the bass is not tied to the melody) or g >= 0: the bass stays at least g semitones under the lowest melody note of its bar.  A
    RegisterPlan passes through.  Raises MusicXLError for a rule over another vocabulary and ValueError for lo > hi, a value outside
    0..127, a wrong count, or a range or bass_below without the rule."""
    from .grammar import pack_bounds
    if isinstance(register, RegisterPlan):
        if register.B != batch * int(repeat):
            raise ValueError(f'the register plan holds {register.B} rows, the batch {batch * int(repeat)}')
        return register
    if register is None:
        for v, name in ((melody_range, 'melody_range'), (bass_range, 'bass_range'), (bass_below, 'bass_below')):
            if v is not None:
                raise ValueError(f'{name}= needs register=, the register rule (tokenizer.register_rule())')
        return None
    if register.vocab_size != int(vocab_size):
        raise MusicXLError(f'the register rule spans {register.vocab_size} tokens, the model has vocab_size {int(vocab_size)}')
    if bass_below is not None and (isinstance(bass_below, (bool, float)) or not hasattr(bass_below, '__index__')
                                   or not 0 <= int(bass_below) <= 127):
        raise ValueError(f'bass_below is None or a number of semitones in 0..127, got {bass_below!r}')
    mel, bass = _ranges_per_row(melody_range, batch, 'melody_range'), _ranges_per_row(bass_range, batch, 'bass_range')
    bounds = torch.tensor([pack_bounds(m + b) for m, b in zip(mel, bass)], dtype=torch.int32)
    return RegisterPlan(register, bounds.repeat_interleave(int(repeat), 0).contiguous(), -1 if bass_below is None else int(bass_below))


SearchPlan = namedtuple('SearchPlan', 'strategy device rules eos pad')


def rules_refusal(what: str, searches: str = 'beam, group-beam or contrastive search') -> MusicXLError:
    """the refusal of a rule (or of padded prompts) under a search that does not take it"""
    return MusicXLError(f'{what} supported for greedy decoding and sampling only, not for {searches}')


def plan_search(caps: dict, *, num_beams=1, num_beam_groups=1, do_sample=False, penalty_alpha=None, top_k=None, diversity_penalty=None,
                eos_token_id=None, pad_token_id=None, config_eos=None, config_pad=None, padded=False, grammar=None, n_bars=None,
                in_key=None, key=None, melody=None, device_scorer=False, repetition_penalty=None, renormalize_logits=None,
                vocab_size=None, register=None, form=None) -> SearchPlan:
    """Which search a `generate` call runs -- a plain value: `strategy` = 'sample' (greedy decoding / sampling), 'beam', 'beam_sample',
    'group_beam' or 'contrastive' (chosen as HF 4.25.1 `generate` does); `device`: with its scorer on the device; `rules`: it takes
    grammar / n_bars / in_key / key / register; `eos`, `pad`: what the search arms stop at and fill with (the arguments, else the config's) --
    or MusicXLError for the rules and the padded prompts that search does not take.  caps: the most beams of 'beam' and 'group_beam'
    search and the most candidates of 'contrastive' search the model runs on the device; an absent key = host only.  The only reader
    of the environment switches.  A strategy takes the rules if it is greedy decoding / sampling, or runs on the device with an
    explicit eos_token_id=: a hypothesis ends only by emitting eos, the config's eos (0 = [OMIT]) is no end token of the grammar,
    and the stop group that the explicit eos turns on is how the device scorers retire rows.
    device_scorer (opt-in, beam-sample only): the draw and the scorer of beam-sample on the device (`beam_sample_device`), which then
    takes grammar / in_key / key like the other device searches.  It is no default because the device draw is another random stream
    than torch.multinomial's: the same seed gives other ids.  caps['beam_sample'] = its most beams; with the keyword the call's
    repetition_penalty, renormalize_logits and vocab_size are judged too: ValueError for a call that is no beam-sample or carries a
    repetition penalty, MusicXLError for what the device path cannot run."""
    nb, ng = num_beams, num_beam_groups
    explicit_eos = eos_token_id is not None
    host_scorer = os.environ.get('MXL_BEAM_HOST') == '1'
    strategy, device = 'sample', False
    if penalty_alpha is not None and penalty_alpha > 0 and top_k is not None and top_k > 1 and not do_sample and nb == 1:
        strategy = 'contrastive'
        device = top_k <= caps.get('contrastive', 0) and os.environ.get('MXL_CONTRASTIVE_HOST') != '1'
    elif ng != 1:
        strategy = 'group_beam'
        # on the device for groups that divide the beams; what the host path refuses with HF's ValueError goes there to be refused,
        # and a negative or infinite diversity_penalty, which the kernel refuses, keeps the host path and what it does with it
        device = (ng > 1 and not do_sample and 1 < nb <= caps.get('group_beam', 0) and ng <= nb and nb % ng == 0
                  and 0.0 <= float(diversity_penalty or 0.0) < math.inf and not host_scorer)
        # this path has not been measured against the host scorer yet (profiles/group_beam_step.txt), so it is taken when a rule
        # asks for it, or with MXL_GROUP_BEAM_DEVICE=1; a call without a rule keeps the host scorer
        device = device and (os.environ.get('MXL_GROUP_BEAM_DEVICE') == '1' or (
            explicit_eos and (grammar is not None or in_key is not None or key is not None or register is not None)))
    elif nb > 1:
        strategy = 'beam_sample' if do_sample else 'beam'
        device = not do_sample and nb <= caps.get('beam', 0) and not host_scorer
    if device_scorer:
        if strategy != 'beam_sample':
            raise ValueError('device_scorer=True selects the device path of beam-sample (num_beams > 1, num_beam_groups=1, '
                             f"do_sample=True); this call runs '{strategy}'")
        if repetition_penalty is not None and repetition_penalty != 1.0:
            raise ValueError('device_scorer=True: the beam arms apply no repetition_penalty and the device path must not differ; '
                             'leave it None or 1.0')
        if 'beam_sample' not in caps:
            raise MusicXLError('device_scorer=True: this model runs no beam-sample on the device (the Reformer scores its beams on '
                               'the host)')
        if host_scorer:
            raise MusicXLError('device_scorer=True contradicts MXL_BEAM_HOST=1, which keeps every beam scorer on the host')
        if not renormalize_logits:
            raise MusicXLError('device_scorer=True needs renormalize_logits=True: the device draw always renormalises the warped '
                               'scores, as the reference does')
        if vocab_size is not None and vocab_size > 2048:
            raise MusicXLError(f'device_scorer=True: the device draw sorts a row in LDS, a vocabulary of {vocab_size} tokens is '
                               'beyond its 2048')
        if not 2 <= nb <= caps['beam_sample']:
            raise MusicXLError(f"device_scorer=True: beam-sample on the device takes 2..{caps['beam_sample']} beams, not {nb}")
        device = True
    is_search = strategy != 'sample'
    # contrastive search called with num_beam_groups != 1 runs, but has never taken the rules
    rules = not is_search or (device and explicit_eos and not (strategy == 'contrastive' and ng != 1))
    # the bar count is untested under contrastive search, under several groups and under a sampled search, and needs the grammar
    # that counts the bars
    no_bar_count = not rules or strategy in ('contrastive', 'group_beam', 'beam_sample') or (strategy == 'beam' and grammar is None)
    if padded and is_search:                            # in this order: the first that applies is the one raised
        raise rules_refusal('padded prompts (attention_mask with zeros) are')
    if melody is not None and is_search:
        raise rules_refusal('melody= is')
    if form is not None and is_search:
        raise rules_refusal('form= is')
    if grammar is not None and not rules:
        raise rules_refusal('grammar= is')
    if n_bars is not None and no_bar_count:
        raise rules_refusal('n_bars= is')
    if (in_key is not None or key is not None) and not rules:
        raise rules_refusal('in_key= is')
    if register is not None and not rules:
        raise rules_refusal('register= is')
    return SearchPlan(strategy, device, rules, config_eos if eos_token_id is None else eos_token_id,
                      config_pad if pad_token_id is None else pad_token_id)


def _guides_per_row(melody, batch: int) -> list:
    """`melody` as generate takes it -> one entry per prompt, each None or a list of token ids: one guide (a 1-D tensor or a flat
    sequence of ints) stands for every prompt, a sequence of guides (None = that row is unguided) gives one per prompt"""
    def flat(g):
        if g is None:
            return None
        if isinstance(g, torch.Tensor):
            if g.dim() != 1 or g.is_floating_point():
                raise ValueError('a guide is a 1-D sequence of token ids')
            return [int(t) for t in g.detach().cpu().tolist()]
        if isinstance(g, (str, bytes)) or not hasattr(g, '__iter__'):
            raise ValueError('a guide is a 1-D sequence of token ids')
        out = list(g)
        if any(isinstance(t, (bool, float, str)) or not hasattr(t, '__index__') for t in out):
            raise ValueError('a guide is a 1-D sequence of token ids')
        return [int(t) for t in out]
    if isinstance(melody, torch.Tensor) and melody.dim() == 2:
        melody = list(melody)
    one = isinstance(melody, torch.Tensor) or (isinstance(melody, (list, tuple)) and len(melody) > 0
                                                and all(hasattr(t, '__index__') and not isinstance(t, torch.Tensor) for t in melody))
    if one:
        return [flat(melody)] * batch
    if not isinstance(melody, (list, tuple)):
        raise ValueError('melody is one guide (a sequence of token ids) or a list of one guide per prompt')
    if len(melody) != batch:
        raise ValueError(f'melody holds {len(melody)} guides for {batch} prompts: give one guide or one per prompt')
    return [flat(g) for g in melody]


class MelodyPlan:
    """The guides of one generation as the decoders take them (melody_config): `rule` (the grammar's MelodyGuide), per row `guides`
    (None or the guide's tokens) and `bars` (None or the guide split into bars), and `n_bars` (B,) int32, the start value of gleft:
    the number of bars in the row's guide, -1 in an unguided row"""

    def __init__(self, rule, guides: list, bars: list):
        self.rule, self.guides, self.bars = rule, guides, bars
        self.n_bars = torch.tensor([-1 if b is None else len(b) for b in bars], dtype=torch.int32)

    @property
    def B(self) -> int:
        return len(self.guides)

    def rows(self, lo: int, hi: int) -> 'MelodyPlan':
        return MelodyPlan(self.rule, self.guides[lo:hi], self.bars[lo:hi])

    def tables(self):
        """(guide (B, W) int32, glen (B,) int32) on the CPU: the rows' guides, right-filled with 0; W >= 1"""
        W = max([1] + [len(g) for g in self.guides if g is not None])
        tok = torch.zeros(self.B, W, dtype=torch.int32)
        for b, g in enumerate(self.guides):
            if g is not None:
                tok[b, :len(g)] = torch.tensor(g, dtype=torch.int32)
        return tok, torch.tensor([0 if g is None else len(g) for g in self.guides], dtype=torch.int32)

    def check_budget(self, grammar, gbar: list):
        """under a bar budget, rows with a known bar length gbar[b] > 0: every guide bar walked through BarBudget.walk from (bar, 0)
        must fit -- a melody that overfills or underfills its bar would leave the row where nothing is allowed, so it raises
        MusicXLError naming the row, the guide index and the token"""
        bud = grammar.budget
        for b, bars in enumerate(self.bars):
            if bars is None or gbar[b] <= 0:
                continue
            at = 0
            for bar in bars:
                _, _, bad = bud.walk(bar, gbar[b], 0)
                if bad >= 0:
                    tok = bar[bad]
                    how = 'underfills' if (bud.need_full >> int(grammar.cls[tok])) & 1 else 'overfills'
                    raise MusicXLError(f'the guide of row {b} {how} its bar at guide index {at + bad}: token {tok} does not fit the '
                                       f'{gbar[b]} slots of the row\'s time signature')
                at += len(bar)


def melody_config(melody, batch: int, grammar, stop: Optional[tuple], n_bars=None, repeat: int = 1) -> Optional[MelodyPlan]:
    """`melody` of a generation as the decoders take it: None, or a MelodyPlan over batch * repeat rows (`repeat` =
    num_return_sequences: every prompt's guide repeated, as the prompts are).  melody: one guide for every prompt or a list of one
    per prompt, None = that row is unguided (_guides_per_row); a MelodyPlan passes through.  Raises ValueError for what the rule
    cannot work with -- no grammar, a grammar without a MelodyGuide or a bar count, no explicit eos, n_bars (the guide sets the
    count), min_length, a wrong number of guides -- and MusicXLError for a guide that does not split into bars or whose bars the
    grammar does not accept after a token that opens a bar."""
    if melody is None:
        return None
    if isinstance(melody, (MelodyPlan, FormPlan)):                    # (a FormPlan travels the same way: form_config)
        if melody.B != batch * int(repeat):
            raise ValueError(f'the {"melody" if isinstance(melody, MelodyPlan) else "form"} plan holds {melody.B} rows, the batch '
                             f'{batch * int(repeat)}')
        if n_bars is not None and isinstance(melody, FormPlan):
            raise ValueError('n_bars together with form: the form sets the number of bars')
        return melody
    if grammar is None:
        raise ValueError('melody needs grammar=: the guide is fed by the token grammar (tokenizer.grammar(bar_budget=True))')
    rule = getattr(grammar, 'guide', None)
    if rule is None:
        raise ValueError('melody needs a grammar with a guide rule (grammar.MelodyGuide; the music grammar has one), this one has none')
    if grammar.bar_count is None:
        raise ValueError('melody needs a grammar with a bar count (grammar.BarCount): the count of the guide\'s bars ends the row')
    if stop is None:
        raise ValueError('melody needs an explicit eos_token_id=: a row ends by emitting eos, and stopping at eos is opt-in')
    if n_bars is not None:
        raise ValueError('n_bars together with melody: the guide sets the number of bars')
    if stop[2] > 0:
        raise ValueError('melody together with min_length: the bar count ends a guided row, and min_length may bar eos where '
                         'nothing else is allowed')
    guides = _guides_per_row(melody, batch)
    enters = [s for s in grammar.reachable() if int(grammar.allow[s]) & grammar.populated & rule.enter]
    bars = []
    for b, g in enumerate(guides):
        if g is None:
            bars.append(None)
            continue
        try:
            split = rule.split(g)
        except ValueError as e:
            raise MusicXLError(f'the guide of row {b} does not split into bars: {e}') from None
        at = 0
        for bar in split:
            for s0 in enters:
                _, bad = grammar.walk(bar, s0)
                if bad >= 0:
                    raise MusicXLError(f'the guide of row {b} breaks the grammar at guide index {at + bad}: token {bar[bad]} is not '
                                       f'allowed there (bar walked from state {grammar.state_names[s0]})')
            at += len(bar)
        bars.append(split)
    plan = MelodyPlan(rule, guides, bars)
    bar_count_config(plan.n_bars, batch, grammar, stop)               # the eos must be an `end` token of the count
    r = int(repeat)
    return plan if r == 1 else MelodyPlan(rule, [g for g in guides for _ in range(r)], [x for x in bars for _ in range(r)])


def _forms_per_row(form, batch: int) -> list:
    """`form` as generate takes it -> one entry per prompt, each None, a string of sections or a plan (a list of ints): one string
    or one plan (a 1-D tensor or a flat sequence of ints) stands for every prompt, a sequence of them (None = that row has no plan)
    gives one per prompt -- as _guides_per_row tells one guide from many"""
    def one_plan(f):
        if isinstance(f, torch.Tensor):
            if f.dim() != 1 or f.is_floating_point() or f.dtype == torch.bool:
                raise ValueError('a plan is a 1-D sequence of ints')
            return [int(j) for j in f.detach().cpu().tolist()]
        return f
    if isinstance(form, str):
        return [form] * batch
    if isinstance(form, torch.Tensor) and form.dim() == 2:
        form = list(form)
    if isinstance(form, torch.Tensor) or (isinstance(form, (list, tuple)) and len(form) > 0
                                          and all(hasattr(j, '__index__') and not isinstance(j, torch.Tensor) for j in form)):
        return [one_plan(form)] * batch
    if not isinstance(form, (list, tuple)):
        raise ValueError('form is a string of sections, a plan (a sequence of ints) or a list of one of them per prompt')
    if len(form) == 0:
        raise ValueError('an empty form plans no bar')
    if len(form) != batch:
        raise ValueError(f'form holds {len(form)} entries for {batch} prompts: give one form or one per prompt')
    return [one_plan(f) for f in form]


class FormPlan:
    """The forms of one generation as the decoders take them (form_config): `rule` (the grammar's BarRepeat), per row `plans` (None
    or the row's plan: per generated bar -1 = free or the earlier generated bar it repeats), `span` (0 = a repeat copies the whole
    bar, 1 = its melody), and `n_bars` (B,) int32, the start value of gleft: the length of the row's plan, -1 in a row without one"""

    def __init__(self, rule, plans: list, span: int):
        self.rule, self.plans, self.span = rule, plans, int(span)
        self.n_bars = torch.tensor([-1 if p is None else len(p) for p in plans], dtype=torch.int32)

    @property
    def B(self) -> int:
        return len(self.plans)

    def rows(self, lo: int, hi: int) -> 'FormPlan':
        return FormPlan(self.rule, self.plans[lo:hi], self.span)

    def tables(self):
        """(plan (B, W) int32, nplan (B,) int32) on the CPU: the rows' plans, right-filled with -1; W >= 1"""
        W = max([1] + [len(p) for p in self.plans if p is not None])
        plan = torch.full((self.B, W), -1, dtype=torch.int32)
        for b, p in enumerate(self.plans):
            if p is not None:
                plan[b, :len(p)] = torch.tensor(p, dtype=torch.int32)
        return plan, torch.tensor([0 if p is None else len(p) for p in self.plans], dtype=torch.int32)


def form_config(form, section_bars, form_span, batch: int, grammar, stop: Optional[tuple], n_bars=None, melody=None,
                min_length: Optional[int] = None, repeat: int = 1) -> Optional[FormPlan]:
    """`form` / `section_bars` / `form_span` of a generation as the decoders take them: None, or a FormPlan over batch * repeat rows
    (`repeat` = num_return_sequences: every prompt's plan repeated, as the prompts are).  form: one string of sections ('AABA'), one
    plan, or a list of one string, plan or None per prompt (_forms_per_row; grammar.BarRepeat.plan_of makes and checks the plans); a
    FormPlan passes through.  section_bars (default 1): the bars of a section of a string.  form_span (default 'bar'): 'bar' = a
    repeat copies the whole bar, 'melody' = its melody, under which the row writes a new bass.  Raises ValueError for what the rule
    cannot work with -- section_bars or form_span without form, no grammar, a grammar without a BarRepeat or a bar count, no explicit
    eos, n_bars or melody beside it (the plan sets the count; a row is fed from one place), min_length, section_bars < 1, an empty
    form, a plan entry outside -1..k-1, a wrong number of forms, another form_span."""
    from .grammar import BarRepeat
    if form is None:
        if section_bars is not None or form_span is not None:
            raise ValueError('section_bars= and form_span= need form=')
        return None
    if isinstance(form, FormPlan):
        if form.B != batch * int(repeat):
            raise ValueError(f'the form plan holds {form.B} rows, the batch {batch * int(repeat)}')
        return form
    if grammar is None:
        raise ValueError('form needs grammar=: bars are told apart by the token grammar (tokenizer.grammar(bar_budget=True))')
    rule = getattr(grammar, 'repeat', None)
    if rule is None:
        raise ValueError('form needs a grammar with a repeat rule (grammar.BarRepeat; the music grammar has one), this one has none')
    if grammar.bar_count is None:
        raise ValueError('form needs a grammar with a bar count (grammar.BarCount): the count of the planned bars ends the row')
    if stop is None:
        raise ValueError('form needs an explicit eos_token_id=: a row ends by emitting eos, and stopping at eos is opt-in')
    if n_bars is not None:
        raise ValueError('n_bars together with form: the form sets the number of bars')
    if melody is not None:
        raise ValueError('melody together with form: a row is fed from its guide or from its own bars, not both')
    if stop[2] > 0 or (min_length or 0) > 0:
        raise ValueError('form together with min_length: the bar count ends a planned row, and min_length may bar eos where '
                         'nothing else is allowed')
    span = BarRepeat.SPANS.get(form_span if form_span is not None else 'bar') if isinstance(form_span, (str, type(None))) else None
    if span is None:
        raise ValueError(f"form_span is 'bar' (a repeat copies the whole bar) or 'melody' (its melody alone), got {form_span!r}")
    plans = [None if f is None else BarRepeat.plan_of(f, 1 if section_bars is None else section_bars)
             for f in _forms_per_row(form, batch)]
    BarRepeat.plan_of([-1], 1 if section_bars is None else section_bars)                # (section_bars is judged whatever the forms are)
    plan = FormPlan(rule, plans, span)
    bar_count_config(plan.n_bars, batch, grammar, stop)               # the eos must be an `end` token of the count
    r = int(repeat)
    return plan if r == 1 else FormPlan(rule, [p for p in plans for _ in range(r)], span)


class RulePlan(namedtuple('RulePlan', 'stop grammar n_bars in_key keys melody register B', defaults=(None,) * 8)):
    """The rules of one generation as every layer between `generate` and RowRules.start hands them down (rules_config builds it):
    `stop` = (eos, pad, min_length) or None, `grammar`, `n_bars` (None or (B,) int32 on the CPU), `in_key` with `keys` (None or (B,)
    int32), `melody` (None, a MelodyPlan or a FormPlan: what rows are fed from, their guides or their own earlier bars -- the two
    exclude each other, so they share the field; `guide` and `form` tell them apart), `register` (None or a RegisterPlan), and `B`,
    the rows the per-row fields were built for (None: no field is per row)."""
    __slots__ = ()

    @property
    def guide(self) -> Optional[MelodyPlan]:
        """the MelodyPlan of a generation under melody=, else None"""
        return self.melody if isinstance(self.melody, MelodyPlan) else None

    @property
    def form(self) -> Optional[FormPlan]:
        """the FormPlan of a generation under form=, else None"""
        return self.melody if isinstance(self.melody, FormPlan) else None

    def rows(self, lo: int, hi: int) -> 'RulePlan':
        """the plan of rows lo..hi-1: every per-row field cut to them (how XLDecoderLanes hands each lane its own)"""
        cut = lambda x: None if x is None else x[lo:hi]
        part = lambda x: None if x is None else x.rows(lo, hi)
        return self._replace(n_bars=cut(self.n_bars), keys=cut(self.keys), melody=part(self.melody), register=part(self.register),
                             B=None if self.B is None else hi - lo)

    def with_stop(self, stop: Optional[tuple]) -> 'RulePlan':
        """the same rules under another stop group (the device searches keep (eos, pad, 0) on)"""
        return self._replace(stop=stop)


NO_RULES = RulePlan()


def rules_config(*, batch: int, vocab_size: int, stop: Optional[tuple] = None, grammar=None, n_bars=None, in_key=None, key=None,
                 melody=None, register=None, melody_range=None, bass_range=None, bass_below=None, repeat: int = 1) -> RulePlan:
    """The rules arguments of one `generate` call over `batch` prompts -> the RulePlan of its batch * repeat rows (`repeat` =
    num_return_sequences, or the rows a search keeps per prompt: every prompt's value repeated, as the prompts are).  The one place
    the arguments are checked, in this order: check_grammar_args, melody_config, bar_count_config, key_config, register_config, which
    say what each refuses.
    stop = (eos, pad, min_length) (stop_config) or None: HF greedy_search / sample stopping -- a row that emits eos is finished and
    emits pad from then on, the call ends once every row has finished, and the output is cut to the width of the longest row
    (finish_at_eos); min_length bars eos below that width.
    grammar (a grammar.TokenGrammar, e.g. `tokenizer.grammar()`): every row may only emit tokens its grammar state allows; the
    state lives on the device and moves inside the sampler launch of the captured step.  The prompts must obey the grammar.
    A grammar with a bar budget (`tokenizer.grammar(bar_budget=True)`) also keeps every channel of every generated bar exactly as
    long as the row's time signature: the free slots of the open channel live and move beside the state.
    n_bars (an int or one per prompt, negative = no limit; needs grammar and an eos): every row opens exactly that many further
    bars -- the bar open at the end of its prompt is finished and not counted -- and, under a bar budget, emits eos when the last
    of them is full.  Without a budget the rule bars a further bar and an early eos but cannot force the end.
    in_key (a grammar.KeyRule, e.g. `tokenizer.key_rule()`; needs no grammar): a row whose key is known emits only pitches of
    that key.  key=None: every row's key is the last key token of its prompt (none: the row is unconstrained); key = a key name
    or ordinal, or one per prompt with None / -1 = unconstrained, overrides the prompts.  A generated key token sets the row's key.
    melody (one guide or one per prompt, None = unguided, or a MelodyPlan; needs grammar and an eos, takes no n_bars or
    min_length): each guide is the `<bar> <melody> ... <bass>` spans of its bars (`tokenizer.melody_guide`); the row is fed them bar
    by bar inside the sampler launch and chooses the bass under each, then ends: the plan's bar counts become n_bars.
    register (a grammar.RegisterRule, e.g. `tokenizer.register_rule()`, or a RegisterPlan; needs no grammar) with melody_range /
    bass_range (one inclusive pair of MIDI numbers or one per prompt, None = unconstrained) and bass_below (None or g >= 0
    semitones): the pitches of every part stay inside its bounds, and the bass at least g under the lowest melody note of its bar.
    A FormPlan as `melody` (form_config builds it from generate's form / section_bars / form_span and refuses what cannot stand beside
    it) passes through like a MelodyPlan: song form -- a planned bar repeats an earlier bar the row generated, copied token by token
    from the row's own ids inside the sampler launch; the plans' lengths become n_bars.  A row is fed from its guide or from its own
    bars, never both, so the two plans share the field (RulePlan.guide / RulePlan.form)."""
    check_grammar_args(grammar, vocab_size, stop)
    guide = melody_config(melody, batch, grammar, stop, n_bars, repeat)
    bars = bar_count_config(n_bars, batch, grammar, stop, repeat) if guide is None else guide.n_bars
    keys = key_config(in_key, key, batch, vocab_size, repeat)
    span = register_config(register, melody_range, bass_range, bass_below, batch, vocab_size, repeat)
    per_row = any(x is not None for x in (bars, keys, guide, span))
    return RulePlan(stop, grammar, bars, in_key, keys, guide, span, batch * int(repeat) if per_row else None)


def check_bar_count_start(grammar, n_bars: torch.Tensor, gstate: torch.Tensor):
    """rows asked for n_bars = 0 whose prompt stops where only a bar can follow (BarCount.needs_bar: the music grammar's header
    states -- no bar is open yet, and a song has one): MusicXLError naming the row, since every token would be barred there.
    Reads gstate (after the prompt scan) only when some row has 0."""
    zero = [b for b, k in enumerate(n_bars.tolist()) if k == 0]
    if not zero:
        return
    states = gstate.tolist()
    for b in zero:
        if states[b] in grammar.bar_count.needs_bar:
            raise MusicXLError(f'n_bars = 0 for row {b}, whose prompt ends in state {grammar.state_names[states[b]]}: no bar is open '
                               'there to finish and only a new bar can follow; give that row n_bars >= 1')


def raise_on_bad_prompt(grammar, ids: torch.Tensor, first_bad: torch.Tensor):
    """first_bad (B,) from ops.grammar_scan over ids, or (2, B) from RowRules.start (one read either way): raises MusicXLError naming
    row, column and token of the first prompt that breaks the grammar (a constraint that starts from an undefined state guarantees
    nothing), or whose bars the budget does not accept"""
    bad = first_bad.tolist()
    bad, over = bad if first_bad.dim() == 2 else (bad, [])
    for b, col in enumerate(bad):
        if col >= 0:
            tok = int(ids[b, col])
            raise MusicXLError(f'the prompt of row {b} breaks the grammar at column {col}: token {tok} is not allowed there '
                               f'({sum(1 for c in bad if c >= 0)} of {len(bad)} rows break it)')
    for b, col in enumerate(over):
        if col >= 0:
            tok = int(ids[b, col])
            how = 'overfills' if grammar.budget.slots_need(int(grammar.budget.slots[tok])) > 0 else 'underfills'
            raise MusicXLError(f'the prompt of row {b} {how} a bar at column {col}: token {tok} does not fit the slots its time '
                               f'signature leaves there ({sum(1 for c in over if c >= 0)} of {len(over)} rows break the bar budget)')


class RowRules:
    """The rules of one generation and their per-row state on the device, as every decoder keeps them: `stop` = (eos, pad,
    min_length) or None, `grammar` (with its bar budget, if it has one) or None, `bars` = the grammar's bar count is on.  One packed
    int32 buffer holds the words the sampler launches move -- unfinished (1 = live), gstate (automaton state), gbar / grem (bar
    length and free slots), gleft (bars the row may still open, < 0 = no limit), gkey (the row's key under `in_key`, a
    grammar.KeyRule; < 0 = none), gpos / gforce (the next index into the row's guide and whether the row is being fed from it, under
    `melody`, a grammar.MelodyGuide), grange / gpart / gfloor (the row's bounds, its open part and the lowest melody pitch of its open bar,
    under `register`, a grammar.RegisterRule, with the generation's `gap`), each (B,) -- then gbad (2, B), the first prompt
    column that breaks the grammar / the budget, and alive (1,), the live-row count.  The guide group also keeps two tables of its
    own here, `guide` (B, ld) int32 and `glen` (B,) int32, refilled by every `start` and regrown only for a longer guide, so that a
    captured step finds the next generation's guides where it found the last one's.  The repeat group (`repeat`, a grammar.BarRepeat,
    with the generation's `span`) has the words gbars / gcopy / gstop (bars opened, the column of the row's own ids the next token is
    copied from, and where the copy ends) and three tables kept the same way: `plan` (B, ld) and `nplan` (B,) int32, uploaded by
    `start`, and `barcol` (B, ld) int32, which the device writes.  A further rule is a row here, a field in RulePlan and in
    ops.RuleState, and a line in rules_config, `start`, `state` and `graph_key` ("adding a rule")."""
    WORDS = ('unfinished', 'gstate', 'gbar', 'grem', 'gleft', 'gkey', 'gpos', 'gforce', 'grange', 'gpart', 'gfloor', 'gbars', 'gcopy',
             'gstop')
    STATE = WORDS + ('alive',)

    def __init__(self, batch: int, dev):
        self.B, n = batch, len(self.WORDS)
        self.buf = torch.zeros((n + 2) * batch + 1, device=dev, dtype=torch.int32)
        for k, row in zip(self.WORDS, self.buf[:n * batch].view(n, batch)):
            setattr(self, k, row)
        self.gbad = self.buf[n * batch:(n + 2) * batch].view(2, batch)
        self.alive = self.buf[(n + 2) * batch:]
        self.unfinished.fill_(1)
        self.gleft.fill_(-1)
        self.gkey.fill_(-1)
        self.gcopy.fill_(-1)
        self.stop = self.grammar = self.n_bars = self.in_key = self.melody = self.melody_plan = self.register = self.repeat = None
        self.bars, self.gap, self.span, self._state = False, -1, 0, None
        self._reset_register()
        self.guide = torch.zeros(batch, 64, device=dev, dtype=torch.int32)
        self.glen = torch.zeros(batch, device=dev, dtype=torch.int32)
        self.plan = torch.full((batch, 64), -1, device=dev, dtype=torch.int32)
        self.barcol = torch.full((batch, 64), -1, device=dev, dtype=torch.int32)
        self.nplan = torch.zeros(batch, device=dev, dtype=torch.int32)

    def _reset_register(self):
        from .grammar import ANY_RANGE, NO_FLOOR, pack_bounds
        self.grange.fill_(pack_bounds(ANY_RANGE))
        self.gpart.zero_()
        self.gfloor.fill_(NO_FLOOR)

    def start(self, ids: torch.Tensor, Tp: int, vocab_size: int, plan: RulePlan):
        """the rules of a new generation (`plan`, from rules_config) over the prompts in columns 0..Tp-1 of ids (ids < 0: left pads,
        skipped): every row live, its grammar state and, under a bar budget, its bar length and free slots after its prompt computed
        on the device, gleft = the plan's n_bars (None: no bar count).  Under in_key gkey = the plan's keys or, without them, the last
        key token of every row's prompt, found on the device (-1 in a row without one).  Under melody the rows' guides and their
        lengths go to the device tables and every row starts free at guide index 0 -- a bar open at the end of the prompt is finished
        freely, the guide engages at the next bar -- and n_bars must be the guides' own.  Under register grange = the plan's bounds,
        gpart and gfloor = the open part and the floor every row's prompt leaves it in, found on the device.  Under form the rows'
        plans and their lengths go to the device tables, barcol is filled with -1, every row starts with no bar opened and no copy
        under way -- a bar open at the end of the prompt is finished freely and has no number -- and n_bars must be the plans' own.
        No rule judges the prompt's pitches.  A plan built for another decoder (row count, vocabulary, grammar) raises."""
        stop, grammar, n_bars, in_key, keys, melody, register = plan[:7]
        form, melody = plan.form, plan.guide              # (the field `melody` holds the one or the other)
        self._state = None
        check_grammar_args(grammar, vocab_size, stop)
        if register is not None and (register.rule.vocab_size != int(vocab_size) or register.B != self.B):
            raise MusicXLError(f'the register rule must span the model\'s {int(vocab_size)} tokens and hold one entry per row '
                               '(register_config)')
        self.register, self.gap = (None, -1) if register is None else (register.rule, register.gap)
        self._reset_register()
        if register is not None:
            self.grange.copy_(register.bounds)
            ops.register_scan(ids, Tp, register.rule, self.grange, self.gpart, self.gfloor, torch.empty_like(self.gpart), self.gap)
        if melody is not None and (grammar is None or melody.rule is not getattr(grammar, 'guide', None) or melody.B != self.B
                                   or n_bars is None or n_bars.tolist() != melody.n_bars.tolist()):
            raise MusicXLError('melody needs the grammar its guide rule belongs to, one guide entry per row and n_bars = the bars '
                               'of the guides (melody_config)')
        self.melody_plan, self.melody = melody, None if melody is None else melody.rule
        self.gpos.zero_()
        self.gforce.zero_()
        if melody is not None:
            tok, glen = melody.tables()
            if tok.shape[1] > self.guide.shape[1]:
                self.guide = torch.zeros(self.B, (tok.shape[1] + 63) // 64 * 64, device=self.guide.device, dtype=torch.int32)
            self.guide[:, :tok.shape[1]].copy_(tok)
            self.glen.copy_(glen)
        else:
            self.glen.zero_()
        if form is not None and (grammar is None or form.rule is not getattr(grammar, 'repeat', None) or form.B != self.B or stop is None
                                 or n_bars is None or n_bars.tolist() != form.n_bars.tolist()):
            raise MusicXLError('form needs the grammar its repeat rule belongs to, the eos rule, one plan entry per row and n_bars = '
                               'the lengths of the plans (form_config)')
        self.repeat, self.span = (None, 0) if form is None else (form.rule, form.span)
        self.gbars.zero_()
        self.gcopy.fill_(-1)
        self.gstop.zero_()
        if form is not None:
            tab, nplan = form.tables()
            if tab.shape[1] > self.plan.shape[1]:
                W = (tab.shape[1] + 63) // 64 * 64
                self.plan = torch.empty(self.B, W, device=self.plan.device, dtype=torch.int32)
                self.barcol = torch.empty_like(self.plan)
            self.plan.fill_(-1)
            self.plan[:, :tab.shape[1]].copy_(tab)
            self.nplan.copy_(nplan)
            self.barcol.fill_(-1)
        else:
            self.nplan.zero_()
        if in_key is not None and in_key.vocab_size != int(vocab_size):
            raise MusicXLError(f'the key rule spans {in_key.vocab_size} tokens, the model has vocab_size {int(vocab_size)}')
        if keys is not None and (in_key is None or keys.numel() != self.B):
            raise MusicXLError('keys need the key rule and one entry per row (key_config)')
        self.in_key = in_key
        if n_bars is not None and (grammar is None or grammar.bar_count is None or stop is None or n_bars.numel() != self.B):
            raise MusicXLError('n_bars needs a grammar with a bar count, the eos rule and one entry per row (bar_count_config)')
        self.stop, self.grammar, self.n_bars, self.bars = stop, grammar, n_bars, n_bars is not None
        self.unfinished.fill_(1)
        self.alive.fill_(self.B)
        if self.bars:
            self.gleft.copy_(n_bars.to(torch.int32))
        else:
            self.gleft.fill_(-1)
        if grammar is not None:
            ops.grammar_scan(ids, Tp, grammar, self.gstate, self.gbad[0])
            if grammar.budget is not None:
                ops.budget_scan(ids, Tp, grammar, self.gbar, self.grem, self.gbad[1])
            else:
                self.gbad[1].fill_(-1)
        if keys is not None:
            self.gkey.copy_(keys.to(torch.int32))
        else:
            self.gkey.fill_(-1)
            if in_key is not None:
                ops.key_scan(ids, Tp, in_key, self.gkey, torch.empty_like(self.gkey))

    def check_prompt(self, ids: torch.Tensor):
        """after `start`: raises for a prompt that breaks the grammar or the bar budget, or that leaves a row asked for 0 bars where
        only a bar can follow, or for a guide that does not fit the bar length of its row (one device read, one more only if some
        row has n_bars = 0)"""
        if self.grammar is not None and self.melody_plan is not None and self.grammar.budget is not None:
            host, n = self.buf.cpu(), len(self.WORDS)                 # the words and gbad in the one read
            raise_on_bad_prompt(self.grammar, ids, host[n * self.B:(n + 2) * self.B].view(2, self.B))
            at = self.WORDS.index('gbar') * self.B
            self.melody_plan.check_budget(self.grammar, host[at:at + self.B].tolist())
        elif self.grammar is not None:
            raise_on_bad_prompt(self.grammar, ids, self.gbad)
        if self.bars:
            check_bar_count_start(self.grammar, self.n_bars, self.gstate)

    def state(self) -> ops.RuleState:
        """the rules and their state as ops.sample_step and sample_unfused take them, gathered once per `start`: every member is
        fixed from there on, the regrown guide / plan / barcol included -- a rule attribute assigned after `start` does not reach it"""
        if self._state is None:
            self._state = ops.RuleState(
                stop=self.stop, unfinished=self.unfinished, alive=self.alive, grammar=self.grammar, gstate=self.gstate, gbar=self.gbar,
                grem=self.grem, gleft=self.gleft if self.bars else None, in_key=self.in_key, gkey=self.gkey, melody=self.melody,
                guide=self.guide, glen=self.glen, gpos=self.gpos, gforce=self.gforce, register=self.register, grange=self.grange,
                gpart=self.gpart, gfloor=self.gfloor, gap=self.gap, repeat=self.repeat, plan=self.plan, nplan=self.nplan,
                barcol=self.barcol, span=self.span, gbars=self.gbars, gcopy=self.gcopy, gstop=self.gstop)
        return self._state

    def graph_key(self, dev) -> tuple:
        """what a captured sampler launch holds of the rules: which of them are on, the identity of the grammar's and the budget's
        device tables and their class masks, the presence of the key rule and the identity of its tables, the presence of the guide
        rule with its class masks and the identity of its guide buffer, the presence of the register rule with the identity of its
        table and the gap, the presence of the repeat rule with its class masks, the span and the identity and stride of its
        plan, nplan and barcol tables.  The per-row words, the keys and the guide positions among
        them, the guide tokens and the plans themselves are step state and not part of it.  (A call without the repeat rule keeps
        the key it had: the entry is appended only when the rule is on.)"""
        g = self.grammar
        return (self.stop,
                None if g is None else tuple(t.data_ptr() for t in g.to(dev)) + (g.n_classes,),
                None if g is None or g.budget is None else
                tuple(t.data_ptr() for t in g.budget.to(dev)) + (g.budget.opens, g.budget.need_free, g.budget.need_full),
                (g.bar_count.count, g.bar_count.end) if self.bars else None,
                None if self.in_key is None else tuple(t.data_ptr() for t in self.in_key.to(dev)),
                None if self.melody is None else (self.melody.enter, self.melody.leave, self.guide.data_ptr(), self.guide.stride(0),
                                                  self.glen.data_ptr()),
                None if self.register is None else (self.register.to(dev).data_ptr(), self.gap)) + (
            () if self.repeat is None else ((self.repeat.enter, self.repeat.leave, self.span, self.plan.data_ptr(), self.plan.stride(0),
                                             self.nplan.data_ptr(), self.barcol.data_ptr(), self.barcol.stride(0)),))

    def snapshot(self) -> tuple:
        """everything the sampler launches write: the packed words and the repeat group's barcol"""
        return self.buf.clone(), self.barcol.clone()

    def restore(self, saved: tuple):
        self.buf.copy_(saved[0])
        self.barcol.copy_(saved[1])


def check_grammar(ids: torch.Tensor, grammar, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 on the CPU: for every row of ids (B, T) the column of the first token the grammar does not allow, -1 = the row
    obeys it -- e.g. to verify the output of an unconstrained run.  attention_mask (B, Tp): left-pad columns (0) are skipped.  Rows
    on the GPU are walked there (mxl_grammar_scan), host tensors by TokenGrammar.walk."""
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    x = ids.to(torch.int64).clone()
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask).to(x.device)
        x[:, :m.shape[1]].masked_fill_(m == 0, -1)
    if not x.is_cuda:
        return torch.tensor([grammar.walk(r)[1] for r in x], dtype=torch.int64)
    x = x.contiguous()
    gstate = torch.empty(x.shape[0], device=x.device, dtype=torch.int32)
    bad = torch.empty_like(gstate)
    ops.grammar_scan(x, x.shape[1], grammar, gstate, bad)
    return bad.cpu().to(torch.int64)


def check_bar_lengths(ids: torch.Tensor, grammar, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 on the CPU, as check_grammar: for every row of ids (B, T) the column of the first token the bar budget of
    `grammar` (tokenizer.grammar(bar_budget=True)) does not allow -- a duration that overfills its channel, a channel closed before
    it is full, a duration of unknown length -- and -1 where every channel is as long as the row's time signature says.  Rows whose
    time signature sets no bar length are reported clean.  Rows on the GPU are walked there (mxl_budget_scan), host tensors by
    TokenGrammar.walk_budget."""
    if grammar.budget is None:
        raise ValueError('check_bar_lengths needs a grammar with a bar budget: tokenizer.grammar(bar_budget=True)')
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    x = ids.to(torch.int64).clone()
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask).to(x.device)
        x[:, :m.shape[1]].masked_fill_(m == 0, -1)
    if not x.is_cuda:
        return torch.tensor([grammar.walk_budget(r)[2] for r in x], dtype=torch.int64)
    x = x.contiguous()
    gbar = torch.empty(x.shape[0], device=x.device, dtype=torch.int32)
    grem, bad = torch.empty_like(gbar), torch.empty_like(gbar)
    ops.budget_scan(x, x.shape[1], grammar, gbar, grem, bad)
    return bad.cpu().to(torch.int64)


def bars_after_prompt(ids: torch.Tensor, grammar, prompt_len: Optional[int] = None,
                      attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 on the CPU, as check_bar_lengths: for every row of ids (B, T) the number of tokens after the prompt that open a
    bar -- tokens of a `count` class of the grammar's bar count (<bar>) from column prompt_len on -- which is what
    `generate(n_bars=)` sets.  prompt_len: the width of the prompt; default the width of attention_mask (the mask given to
    generate), else 0 = the whole row.  Ids < 0 and ids beyond the vocabulary count nothing.  The count runs where ids lives."""
    if grammar.bar_count is None:
        raise ValueError('bars_after_prompt needs a grammar with a bar count (grammar.BarCount; the music grammar has one)')
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    if prompt_len is None:
        prompt_len = 0 if attention_mask is None else int(torch.as_tensor(attention_mask).shape[1])
    x = ids[:, int(prompt_len):].to(torch.int64)
    V = grammar.vocab_size
    cls = grammar.to(x.device)[0].to(torch.int64)
    ok = (x >= 0) & (x < V)
    hit = (torch.bitwise_right_shift(torch.full_like(x, grammar.bar_count.count), cls[x.clamp(0, V - 1)]) & 1).bool() & ok
    return hit.sum(1).cpu().to(torch.int64)


def check_in_key(ids: torch.Tensor, rule, prompt_len: Optional[int] = None, attention_mask: Optional[torch.Tensor] = None,
                 key=None) -> torch.Tensor:
    """(B,) int64 on the CPU, as check_grammar: for every row of ids (B, T) the first generated column (>= prompt_len) that holds a
    pitch outside the row's key under `rule` (a grammar.KeyRule, `tokenizer.key_rule()`), -1 = none -- what `generate(in_key=rule)`
    keeps at -1.  The row's key is the last key token before that column, the generated ones included; the prompt only supplies
    the key, its pitches are not judged, and a row without a key is clean.  prompt_len: the width of the prompt; default the width
    of attention_mask (the mask given to generate), else 0 = every column is judged.  attention_mask (B, Tp): left-pad columns (0)
    are skipped.  key: as generate's `key=` (one key or one per row, None / -1 = unconstrained): the rows start the generated part
    in these keys whatever their prompts say.  Rows on the GPU are walked there (mxl_key_scan), host tensors by KeyRule.walk."""
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    x = ids.to(torch.int64).clone()
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask).to(x.device)
        x[:, :m.shape[1]].masked_fill_(m == 0, -1)
    if prompt_len is None:
        prompt_len = 0 if attention_mask is None else int(torch.as_tensor(attention_mask).shape[1])
    prompt_len = int(prompt_len)
    start = key_config(rule, key, x.shape[0], rule.vocab_size)
    if start is not None:                                # the given keys stand for the prompt
        x, off = x[:, prompt_len:], prompt_len
        prompt_len = 0
    else:
        start, off = torch.full((x.shape[0],), -1, dtype=torch.int32), 0
    if not x.is_cuda:
        bad = torch.tensor([rule.walk(r, int(k), prompt_len)[1] for r, k in zip(x, start.tolist())], dtype=torch.int64)
    else:
        x = x.contiguous()
        gkey = start.to(x.device)
        first = torch.empty_like(gkey)
        ops.key_scan(x, x.shape[1], rule, gkey, first, check_from=prompt_len)
        bad = first.cpu().to(torch.int64)
    return torch.where(bad >= 0, bad + off, bad)


def check_register(ids: torch.Tensor, rule, melody_range=None, bass_range=None, bass_below=None, prompt_len: Optional[int] = None,
                   attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 on the CPU, as check_in_key: for every row of ids (B, T) the first generated column (>= prompt_len) that holds a
    pitch outside the bounds of its part under `rule` (a grammar.RegisterRule, `tokenizer.register_rule()`), -1 = none -- what
    `generate(register=rule, ...)` keeps at -1.  melody_range / bass_range / bass_below: as generate's (one pair or one per row).  The
    prompt only moves the row's open part and floor, its pitches are not judged.  prompt_len: the width of the prompt; default the
    width of attention_mask, else 0 = every column is judged.  attention_mask (B, Tp): left-pad columns (0) are skipped.  Rows on the
    GPU are walked there (mxl_register_scan), host tensors by RegisterRule.walk."""
    from .grammar import NO_FLOOR
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    x = ids.to(torch.int64).clone()
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask).to(x.device)
        x[:, :m.shape[1]].masked_fill_(m == 0, -1)
    if prompt_len is None:
        prompt_len = 0 if attention_mask is None else int(torch.as_tensor(attention_mask).shape[1])
    plan = register_config(rule, melody_range, bass_range, bass_below, x.shape[0], rule.vocab_size)
    if not x.is_cuda:
        unpack = lambda w: (w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, (w >> 24) & 0xFF)
        return torch.tensor([rule.walk(r, unpack(int(w)), plan.gap, check_from=int(prompt_len))[2]
                             for r, w in zip(x, plan.bounds.tolist())], dtype=torch.int64)
    x = x.contiguous()
    grange = plan.bounds.to(x.device)
    gpart, gfloor = torch.zeros_like(grange), torch.full_like(grange, NO_FLOOR)
    first = torch.empty_like(grange)
    ops.register_scan(x, x.shape[1], rule, grange, gpart, gfloor, first, plan.gap, check_from=int(prompt_len))
    return first.cpu().to(torch.int64)


def check_melody(ids: torch.Tensor, grammar, melody, prompt_len: Optional[int] = None,
                 attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 on the CPU, as check_grammar: for every row of ids (B, T) the first generated column (>= prompt_len) that departs
    from the row's guide, -1 = none -- what `generate(melody=)` keeps at -1.  melody: as generate's (one guide or one per row, None
    = the row is unguided and clean).  A column departs if it holds another token than the guide feeds there (the span from a
    `<bar>` to its `<bass>`), if it opens a bar beyond the guide, or if it ends the row (a token of an `end` class of the grammar's
    bar count) while guided bars were never opened.  A row cut by max_length is judged up to the cut.  prompt_len: the width of the
    prompt; default the width of attention_mask, else 0.  The walk runs on the host (MelodyGuide.walk)."""
    rule = getattr(grammar, 'guide', None)
    if rule is None or grammar.bar_count is None:
        raise ValueError('check_melody needs a grammar with a guide rule and a bar count (the music grammar has both)')
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    if prompt_len is None:
        prompt_len = 0 if attention_mask is None else int(torch.as_tensor(attention_mask).shape[1])
    prompt_len = int(prompt_len)
    guides = _guides_per_row(melody, ids.shape[0])
    end, cls, V = grammar.bar_count.end, grammar.cls, grammar.vocab_size
    out = []
    for row, g in zip(ids[:, prompt_len:].cpu().tolist(), guides):
        if g is None:
            out.append(-1)
            continue
        stop_at = next((i for i, t in enumerate(row) if 0 <= t < V and (end >> int(cls[t])) & 1), None)
        pos, _, bad = rule.walk(row if stop_at is None else row[:stop_at], g)
        if bad < 0 and stop_at is not None and pos < len(g):
            bad = stop_at
        out.append(bad + prompt_len if bad >= 0 else -1)
    return torch.tensor(out, dtype=torch.int64)


def check_form(ids: torch.Tensor, grammar, form, section_bars: int = 1, form_span: str = 'bar', prompt_len: Optional[int] = None,
               attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,) int64 on the CPU, as check_melody: for every row of ids (B, T) the first generated column (>= prompt_len) that departs
    from the row's plan, -1 = none -- what `generate(form=)` keeps at -1.  form / section_bars / form_span: as generate's (one form
    or one per row, None = the row has no plan and is clean).  A column departs if, inside a repeat, it holds another token than the
    source bar holds there (form_span='bar': the whole bar; 'melody': up to and including its `<bass>`), if it opens a bar beyond
    the plan, or if it ends the row (a token of an `end` class of the grammar's bar count) while planned bars were never opened.  A
    row cut by max_length is judged up to the cut.  prompt_len: the width of the prompt; default the width of attention_mask, else 0.
    attention_mask (B, Tp): left-pad columns (0) are skipped.  The walk runs on the host (BarRepeat.walk)."""
    from .grammar import BarRepeat
    rule = getattr(grammar, 'repeat', None)
    if rule is None or grammar.bar_count is None:
        raise ValueError('check_form needs a grammar with a repeat rule and a bar count (the music grammar has both)')
    if form_span not in BarRepeat.SPANS:
        raise ValueError(f"form_span is 'bar' or 'melody', got {form_span!r}")
    ids = torch.as_tensor(ids)
    if ids.dim() == 1:
        ids = ids.view(1, -1)
    x = ids.to(torch.int64).cpu().clone()
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask).cpu()
        x[:, :m.shape[1]].masked_fill_(m == 0, -1)
    if prompt_len is None:
        prompt_len = 0 if attention_mask is None else int(torch.as_tensor(attention_mask).shape[1])
    prompt_len = int(prompt_len)
    cnt, cls, V = grammar.bar_count, grammar.cls, grammar.vocab_size
    out = []
    for row, f in zip(x.tolist(), _forms_per_row(form, x.shape[0])):
        if f is None:
            out.append(-1)
            continue
        plan = BarRepeat.plan_of(f, section_bars)
        kind = lambda t, mask: 0 <= t < V and (mask >> int(cls[t])) & 1
        end_at = next((i for i in range(prompt_len, len(row)) if kind(row[i], cnt.end)), None)
        opened = [i for i in range(prompt_len, len(row) if end_at is None else end_at) if kind(row[i], cnt.count)]
        cut = len(row) if end_at is None else end_at
        if len(opened) > len(plan):                                   # a bar beyond the plan: judged up to it
            cut = opened[len(plan)]
        _, bad = rule.walk(row[:cut], plan, BarRepeat.SPANS[form_span], prompt_len)
        if bad < 0 and len(opened) > len(plan):
            bad = cut
        if bad < 0 and end_at is not None and len(opened) < len(plan):
            bad = end_at
        out.append(bad)
    return torch.tensor(out, dtype=torch.int64)


class _AlivePoll:
    """live-row counts of one decoder read back without stalling its stream: after each chunk of steps a non-blocking copy of
    `alive` into pinned host memory and an event; `wait(keep)` blocks until at most `keep` such reads are outstanding"""

    def __init__(self, alive: torch.Tensor, target: int = 0):
        self.alive, self.target = alive, target       # target: the count at which the decoder is finished (beam search: n_done == items)
        self.bufs = [torch.empty(1, dtype=torch.int32, pin_memory=True) for _ in range(3)]
        self.pend, self.i, self.done = deque(), 0, False

    def mark(self):
        buf = self.bufs[self.i % 3]
        self.i += 1
        buf.copy_(self.alive, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pend.append((ev, buf))

    def wait(self, keep: int) -> bool:
        while len(self.pend) > keep:
            ev, buf = self.pend.popleft()
            ev.synchronize()
            if int(buf[0]) == self.target:
                self.done = True
        return self.done


def run_until_finished(decoders, n: int, chunk: int = STOP_CHUNK) -> list:
    """Early exit without a per-step sync.  decoders: [(decoder, stream or None)] after a `begin` that stops: `begin(...,
    stop=...)`, `beam_begin` or `contrastive_begin`.  A decoder names the device counter it is finished by and that counter's target
    in `finished_by` -- XLDecoder's three begins set it: the live rows at 0, the done items of a beam search at their number, the
    finished sequences of a contrastive search at theirs; a decoder without the attribute is finished by `alive` at 0.  Each one
    replays up to n steps in chunks of `chunk` on its stream, the counter is copied back after the prompt pass and after every
    chunk, and chunk i + 2 is enqueued only once chunk i's count has been read: a decoder stops when that count is the target.  At
    most two chunks are in flight, and the steps beyond the last live one skip the ring attention.  The count after the prompt pass
    is waited for, so a batch whose first tokens are all eos replays nothing.  Returns the steps issued per decoder."""
    chunk = max(1, int(chunk))
    polls = []
    for dec, s in decoders:
        with (torch.cuda.stream(s) if s is not None else nullcontext()):
            p = _AlivePoll(*getattr(dec, 'finished_by', (dec.alive, 0)))
            p.mark()
        polls.append(p)
    issued = [0] * len(decoders)
    for p in polls:
        p.wait(0)
    live = True
    while live:
        live = False
        for i, (dec, s) in enumerate(decoders):
            if issued[i] >= n or polls[i].wait(1):
                continue
            k = min(chunk, n - issued[i])
            with (torch.cuda.stream(s) if s is not None else nullcontext()):
                for _ in range(k):
                    dec.replay_once()
                polls[i].mark()
            issued[i] += k
            live = True
    return issued


def decode_lanes(dec, lanes, streams, prompt: torch.Tensor, max_length: int, sampling: dict, use_graph: bool, n_pad, stop_chunk,
                 rules: RulePlan) -> torch.Tensor:
    """The body of `generate` for one decoder (lanes = [dec], streams = [None]) or for an XLDecoderLanes with its lanes and their
    streams: `dec.begin` under `rules`, then every remaining step through `dec.replay_once` -- or, with a stop group in the plan,
    each lane on its own until its rows have finished (run_until_finished) -- then the lanes' rows in order, cut to the width of
    the longest lane and right-filled with pad where a lane stopped earlier.  Sets `steps_run` on every lane and on dec (the most
    of any lane).  The prompt columns of left-padded prompts (n_pad) come back as given."""
    Tp, stop = prompt.shape[1], rules.stop
    if max_length - Tp <= 0:
        return prompt[:, :max_length]
    n = dec.begin(prompt, max_length, sampling, use_graph, n_pad, rules)
    if stop is None:
        for _ in range(n):
            dec.replay_once()
        steps = [n] * len(lanes)
    else:
        steps = run_until_finished(list(zip(lanes, streams)), n, stop_chunk)
    for s in streams:
        if s is not None:
            torch.cuda.current_stream().wait_stream(s)
    for d, k in zip(lanes, steps):
        d.steps_run = k
    dec.steps_run = max(steps)
    widths = [max_length if stop is None else stop_width(d.ids, d.unfinished, Tp, max_length, stop[0]) for d in lanes]
    W = max(widths)
    out = torch.cat([d.ids[:, :W] for d in lanes], 0) if len(lanes) > 1 else dec.ids[:, :W].clone()
    row = 0
    for d, w in zip(lanes, widths):
        if w < W:
            out[row:row + d.B, w:] = stop[1]
        row += d.B
    if n_pad is not None:
        out[:, :Tp].copy_(prompt)
    return out


class RuledGenerate:
    """`generate` and `run` of XLDecoder, XLDecoderLanes and rf_generate.RFDecoder: greedy decoding and sampling under the rules.
    A decoder brings `begin` / `replay_once`, `B`, and `lanes` with their `streams` where it is more than one decoder."""

    def _admit(self, max_length: int):
        """what a decoder refuses before the rules are judged"""

    def generate(self, prompt: torch.Tensor, max_length: int, do_sample: bool = False, top_k: Optional[int] = None,
                 top_p: Optional[float] = None, temperature: float = 1.0, repetition_penalty: Optional[float] = None,
                 typical_p: Optional[float] = None, use_graph: bool = True, n_pad: Optional[torch.Tensor] = None,
                 eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, min_length: Optional[int] = None,
                 stop_chunk: int = STOP_CHUNK, grammar=None, n_bars=None, in_key=None, key=None, melody=None, register=None,
                 melody_range=None, bass_range=None, bass_below=None, stop: Optional[tuple] = None, form=None, section_bars=None,
                 form_span=None) -> torch.Tensor:
        """Returns (B, max_length) ids = prompt + continuation.  Like the reference (eos_token_id stays HF's default 0 =
        [OMIT]) decoding runs to max_length.  n_pad: (B,) int32 device tensor of left-pad counts (XLDecoder.prefill);
        the prompt columns, pads included, come back as given.  use_graph: one captured step replayed per token, where the decoder
        captures one (RFDecoder does not).
        eos_token_id (opt-in) with pad_token_id (default: eos) and min_length, or the group whole as stop = (eos, pad, min_length)
        (stop_config): rows finish at eos.  The decode steps are replayed in chunks of `stop_chunk` with the live-row count read back
        one chunk late (run_until_finished): no per-step host round trip.  Over lanes every lane stops on its own; the output is the
        lanes' rows cut to the common width and right-filled with pad where a lane stopped earlier.
        grammar, n_bars, in_key / key, melody, register with melody_range / bass_range / bass_below, form with section_bars /
        form_span: the rules, one value per row
        where they are per row, as rules_config describes and checks them; each lane keeps the words of its own rows."""
        self._admit(max_length)
        stop = stop_config(eos_token_id, pad_token_id, min_length) if stop is None else stop
        feed = form_config(form, section_bars, form_span, self.B, grammar, stop, n_bars, melody)
        rules = rules_config(batch=self.B, vocab_size=getattr(self, 'lanes', [self])[0].eng.cfg.vocab_size,
                             stop=stop, grammar=grammar,
                             n_bars=n_bars, in_key=in_key, key=key, melody=melody if feed is None else feed, register=register,
                             melody_range=melody_range,
                             bass_range=bass_range, bass_below=bass_below)
        return self.run(prompt, max_length, sampling_config(do_sample, top_k, top_p, temperature, repetition_penalty, typical_p), rules,
                        use_graph, n_pad, stop_chunk)

    @torch.no_grad()
    def run(self, prompt: torch.Tensor, max_length: int, sampling: dict, rules: RulePlan = NO_RULES, use_graph: bool = True,
            n_pad: Optional[torch.Tensor] = None, stop_chunk: int = STOP_CHUNK) -> torch.Tensor:
        """`generate` from a finished plan: sampling from sampling_config, rules from rules_config over this decoder's B rows"""
        return decode_lanes(self, getattr(self, 'lanes', [self]), getattr(self, 'streams', [None]), prompt, max_length, sampling,
                            use_graph, n_pad, stop_chunk, rules)


BEAM_MAX = 16            # beams per item of mxl_beam_step / mxl_beam_reorder
CONTRASTIVE_MAX = ops.CONTRASTIVE_MAX     # candidates per sequence of contrastive search on the device


class BeamStore:
    """The scorer's state of a beam search on the device, as mxl_beam_step reads and writes it: `scores` (rows,) f32, the running
    score of every row; the finished hypotheses of every item, `hyp_ids` (Bs, nb, ld) int64 with `hyp_len` and `hyp_score` (Bs, nb),
    slots 0..hyp_n[b]-1 in use; `hyp_n` and `done` (Bs,) and `n_done` (1,), the number of done items, which the host reads a chunk
    late; and what a step hands to the ring reorder, `beam_idx` (rows,) and `moved` (Bs,).  The int32 words share one buffer."""

    def __init__(self, Bs: int, nb: int, ld_ids: int, dev):
        self.Bs, self.nb = Bs, nb
        rows = Bs * nb
        self.scores = torch.zeros(rows, device=dev, dtype=torch.float32)
        self.hyp_ids = torch.zeros(Bs, nb, ld_ids, device=dev, dtype=torch.int64)
        self.hyp_score = torch.zeros(Bs, nb, device=dev, dtype=torch.float32)
        self.ints = torch.zeros(rows + 2 * Bs + 1, device=dev, dtype=torch.int32)
        self.hyp_len, self.hyp_n, self.done, self.n_done = self._words(self.ints)
        self.beam_idx = torch.zeros(rows, device=dev, dtype=torch.int32)
        self.moved = torch.zeros(Bs, device=dev, dtype=torch.int32)

    def _words(self, ints: torch.Tensor) -> tuple:
        """hyp_len, hyp_n, done, n_done in the word buffer, or in a copy of it"""
        Bs, rows = self.Bs, self.Bs * self.nb
        return ints[:rows].view(Bs, self.nb), ints[rows:rows + Bs], ints[rows + Bs:rows + 2 * Bs], ints[rows + 2 * Bs:]

    def start(self, ng: int = 1):
        """an empty store; the first beam of every item -- of every one of its ng groups -- starts at score 0, the others at -1e9
        (HF beam_search / group_beam_search)"""
        self.ints.zero_()
        self.scores.fill_(-1e9)
        self.scores.view(self.Bs, self.nb)[:, ::self.nb // ng] = 0

    def read(self) -> tuple:
        """the host's copy once the steps have run: hyp_len, hyp_n, done and hyp_score as lists, scores as a tensor"""
        hyp_len, hyp_n, done, _ = self._words(self.ints.cpu())
        return hyp_len.tolist(), hyp_n.tolist(), done.tolist(), self.hyp_score.cpu().tolist(), self.scores.cpu()


class ContrastiveStore:
    """The state of a contrastive search on the device, as mxl_contrastive_topk / mxl_contrastive_step read and write it: `ctx`
    (B0, Smax, d) bf16 and `inv` (B0, Smax) f32, the last-layer hidden state of every position of every sequence and its reciprocal
    norm; `probs` (B0, K) and `score` (B0 * K,) f32 of the step's candidates; and the int32 words `dead` (B0, K), `sel` (B0,), the
    candidate picked last, and `n_done` (1,), the number of finished sequences, which the host reads a chunk late.  The words share
    one buffer."""

    def __init__(self, B0: int, K: int, Smax: int, d: int, dev):
        self.B0, self.K = B0, K
        self.ctx = torch.zeros(B0, Smax, d, device=dev, dtype=torch.bfloat16)
        self.inv = torch.zeros(B0, Smax, device=dev, dtype=torch.float32)
        self.probs = torch.zeros(B0, K, device=dev, dtype=torch.float32)
        self.score = torch.zeros(B0 * K, device=dev, dtype=torch.float32)
        self.ints = torch.zeros(B0 * K + B0 + 1, device=dev, dtype=torch.int32)
        self.dead = self.ints[:B0 * K].view(B0, K)
        self.sel, self.n_done = self.ints[B0 * K:B0 * K + B0], self.ints[B0 * K + B0:]

    def start(self, hid: torch.Tensor):
        """a new search: hid (B0, Tp, d) = the last-layer hidden states of the prompts; every word zero (sel = 0: the K rows of a
        sequence are equal after the prompt pass, its first candidates come from row 0)"""
        Tp = hid.shape[1]
        self.ints.zero_()
        self.ctx[:, :Tp].copy_(hid)
        for b in range(self.B0):
            ops.row_inv_norm(self.ctx[b, :Tp], self.inv[b, :Tp], Tp)


KV_DTYPES = {None: None, 'bf16': None, 'fp8': 'fp8', 'fp8_e4m3': 'fp8'}


def resolve_kv_dtype(kv_cache_dtype: Optional[str]) -> Optional[str]:
    """the K/V ring format of a call: None / 'bf16' -> None (bf16 rings), 'fp8' / 'fp8_e4m3' -> 'fp8'; a call that names none takes
    MXL_KV_DTYPE (an A/B knob: unset, nothing changes).  Anything else is a ValueError."""
    if kv_cache_dtype is None:
        kv_cache_dtype = os.environ.get('MXL_KV_DTYPE') or None
    if kv_cache_dtype not in KV_DTYPES:
        raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r}: expected None, 'bf16', 'fp8' or 'fp8_e4m3'")
    return KV_DTYPES[kv_cache_dtype]


BEAM_RINGS = ('copied', 'indexed', 'indexed_fp8')         # what `generate(beam_rings=)` takes
DECODER_BEAM_RINGS = BEAM_RINGS[:2]                        # what XLDecoder.beam_begin takes: 'indexed_fp8' is 'indexed' on an fp8 decoder


def _resolve_opt_in(name: str, value: Optional[str], allowed: tuple, env: str, applies: bool, serves: str) -> str:
    """the one body of the ring opt-ins: `value` of keyword `name`, one of `allowed` (the first, 'copied', is what None means); a call
    that names none takes the environment's `env` (an A/B knob: unset, nothing changes).  Any other string is a ValueError; so is an
    explicit opt-in where it does not apply ("<name>='<value>' serves <serves>"), while the environment's is ignored there."""
    explicit = value is not None
    mode = value if explicit else (os.environ.get(env) or allowed[0])
    if mode not in allowed:
        raise ValueError(f"{name}={mode!r}: expected None, {', '.join(map(repr, allowed[:-1]))} or {allowed[-1]!r}")
    if mode != allowed[0] and not applies:
        if explicit:
            raise ValueError(f"{name}='{mode}' serves {serves}")
        mode = allowed[0]
    return mode


def resolve_beam_rings(beam_rings: Optional[str], applies: bool, d_head: int = 64) -> str:
    """`generate(beam_rings=)`, which describes the modes: how the K/V rings of a device beam search follow their beams -- 'copied'
    (None), 'indexed' or 'indexed_fp8' (the caller builds the search's decoder with kv_dtype='fp8' and runs its 'indexed' mode) -- by
    _resolve_opt_in with MXL_BEAM_RINGS.  applies: the call is a beam, group-beam or beam-sample search with its scorer on the device,
    without kv_cache_dtype, over a mem_len that is a multiple of 16.  d_head: FP8 rings take head widths 16, 32 and 64 -- an explicit
    'indexed_fp8' with another is a MusicXLError, the environment's is ignored."""
    mode = _resolve_opt_in('beam_rings', beam_rings, BEAM_RINGS, 'MXL_BEAM_RINGS', applies,
                           'beam, group-beam and beam-sample search with the scorer on the device'
                           f"{' over bf16 rings' if beam_rings == 'indexed' else ''}: "
                           'not greedy decoding, sampling or contrastive search, not the host scorers (MXL_BEAM_HOST=1, '
                           "more than 16 beams, beam-sample without device_scorer=True), not kv_cache_dtype='fp8', not a mem_len "
                           'that is no multiple of 16')
    if mode == 'indexed_fp8' and d_head not in (16, 32, 64):
        if beam_rings is not None:
            raise MusicXLError(f"beam_rings='indexed_fp8': fp8 K/V rings need a head width of 16, 32 or 64, not {d_head}")
        mode = 'copied'
    return mode


CONTRASTIVE_RINGS = ('copied', 'shared')                   # what `generate(contrastive_rings=)` takes


def resolve_contrastive_rings(contrastive_rings: Optional[str], applies: bool) -> str:
    """`generate(contrastive_rings=)`, which describes the modes: the K/V rings of a contrastive search on the device -- 'copied' (None:
    one set per candidate row) or 'shared' (one per prompt, XLDecoder(shared_rings=K)) -- by _resolve_opt_in with MXL_CONTRASTIVE_RINGS.
    applies: the call is a contrastive search with its step on the device (top_k <= 32, no MXL_CONTRASTIVE_HOST=1) over bf16 rings."""
    return _resolve_opt_in('contrastive_rings', contrastive_rings, CONTRASTIVE_RINGS, 'MXL_CONTRASTIVE_RINGS', applies,
                           'contrastive search with its step on the device over bf16 rings: not greedy decoding, sampling or a beam '
                           "search, not the host-driven loop (top_k > 32, MXL_CONTRASTIVE_HOST=1), not kv_cache_dtype='fp8'")


PROMPT_RINGS = ('copied', 'shared')                        # what `generate(prompt_rings=)` takes


def resolve_prompt_rings(prompt_rings: Optional[str], applies: bool) -> str:
    """`generate(prompt_rings=)`, which describes the modes: the K/V rings of sampling with num_return_sequences = n >= 2 -- 'copied'
    (None: a full set per row) or 'shared' (one set of prompt rings per prompt and a tail ring per row, XLDecoder(prompt_rings=n)) --
    by _resolve_opt_in with MXL_PROMPT_RINGS.  applies: the call samples (do_sample=True, one beam) with n >= 2 over bf16 rings."""
    return _resolve_opt_in('prompt_rings', prompt_rings, PROMPT_RINGS, 'MXL_PROMPT_RINGS', applies,
                           'sampling with num_return_sequences >= 2 over bf16 rings: not num_return_sequences=1, greedy decoding, a '
                           "beam search or contrastive search, not kv_cache_dtype='fp8'")


prompt_rings_misfit = PromptRings.misfit         # (cfg, n, rows): why a model cannot run prompt_rings='shared' so, None: it can


class XLDecoder(RuledGenerate):
    def __init__(self, engine, batch: int, max_total_len: int, seed: int = 77, kv_dtype: Optional[str] = None,
                 shared_rings: int = 0, prompt_rings: int = 0, tail_len: Optional[int] = None):
        """kv_dtype, shared_rings, prompt_rings and tail_len select the layout of the K/V rings (rings.py; `_layout`): bf16 or
        kv_dtype='fp8' rings, one per row; shared_rings = K > 0, a decoder for contrastive search alone whose `batch` = B0 * K rows keep
        one set of rings per prompt (rings.SharedRings); prompt_rings = n > 0, a decoder for sampling alone whose `batch` = B0 * n rows
        keep one set of prompt rings per prompt and a tail ring of prompt_tail_len(M, tail_len) slots each (rings.PromptRings).
        `self.layout` holds the rings and everything that differs between the modes; everything per row stays `batch` rows here, and
        the layout's tensors and numbers are readable here under the names in RingLayout.SHOWN."""
        self.eng, self.B, self.Tmax = engine, batch, max_total_len
        c, dev = engine.cfg, engine.dev
        d, M, Fi, H, dh = c.d_model, c.mem_len, c.d_inner, c.n_head, c.d_head
        bf = dict(device=dev, dtype=torch.bfloat16)
        self.layout = lay = self._layout(kv_dtype, shared_rings, prompt_rings, tail_len)
        lay.build(c, batch, dev)
        for k in RingLayout.SHOWN:
            setattr(self, k, getattr(lay, k))
        self.ring_spec = (lay.kv_dtype, lay.prompt_n, lay.Mt)       # what `generate` rebuilds its cached decoder for
        self.rd = None                                 # per-layer Rd tables (eval: no dropout on pos_emb)
        self.ids = torch.zeros(batch, max_total_len + 1, device=dev, dtype=torch.int64)
        self.t_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        self.rng = torch.zeros(1, device=dev, dtype=torch.int64)
        self.seed = seed
        self.h = [torch.empty(batch, d, **bf) for _ in range(2)]
        self.qkv = torch.empty(batch, 3 * d, **bf)
        self.av = torch.empty(batch, d, **bf)
        self.qr = torch.empty(batch, d, **bf)
        self.slabs = torch.zeros(4, 64, d, device=dev, dtype=torch.float32)   # K-slice partials of the FFN output projection
        self.bd = torch.empty(batch, H, M, device=dev, dtype=torch.float32)
        self.split = ops.relattn_decode_split_scratch(batch, H, dh, lay.pieces, dev)
        self.tmp = torch.empty(batch, d, **bf)
        self.h1 = torch.empty(batch, d, **bf)
        self.a = torch.empty(batch, Fi, **bf)
        self.logits = torch.empty(batch, engine.layout.head_rows_padded, device=dev, dtype=torch.float32)
        self.logp = torch.empty(batch, c.vocab_size, device=dev, dtype=torch.float32)
        self.graph = None
        self._graph_key = None
        # Round 6: sampler + the sampled token's embedding row (the next step's input) + counter advance in ONE launch
        # (mxl_sample_step), and no log-softmax launch where nothing reads log-probabilities: 2 launches per step around the layers
        # instead of 5.  MXL_DECODE_UNFUSED=1 keeps the five (A/B runs, tests).
        self.fused_sampler = c.vocab_size <= 2048 and os.environ.get('MXL_DECODE_UNFUSED') != '1'
        self.step_ctr = torch.zeros(1, device=dev, dtype=torch.int32)
        # optional (B, Tmax, V) f32 buffer: row t receives the log-probs computed FROM position t (parity tests compare them
        # with a one-shot forward); written on the device by position, so it also works under hipGraph replay
        self.trace = None
        self.steps_run = 0                              # decode steps issued by the last generate() (early exit: fewer)
        self.beam = None                                # BeamStore of a beam search on the device (beam_begin)
        # how the rings follow the beams of that search, fixed per beam_begin: 'copied' (mxl_beam_reorder) or 'indexed' -- the rings
        # stay and `owner` (B, M) uint8 says which row of its item holds each slot of a row's history (mxl_beam_owner_follow)
        self.beam_rings = 'copied'
        self.owner = None
        self.drawn = None                               # (B, V) f32: the drawn candidates of a beam-sample step (beam_begin, sample)
        self.cs = None                                  # ContrastiveStore of a contrastive search on the device (contrastive_begin)
        # the rules of the current generation (eos, grammar, bar budget, bar count) and their per-row words, which the sampler
        # launch reads and moves; the words are readable here under their names
        self.rules = RowRules(batch, dev)
        for k in RowRules.STATE:
            setattr(self, k, getattr(self.rules, k))

    @staticmethod
    def _layout(kv_dtype: Optional[str], shared_rings: int, prompt_rings: int, tail_len: Optional[int]) -> RingLayout:
        """the ring layout (rings.py) of a decoder's ring arguments, not yet built: the one place that tells the modes apart"""
        if kv_dtype not in (None, 'fp8'):
            raise ValueError(f"kv_dtype={kv_dtype!r}: expected None (bf16 rings) or 'fp8'")
        K, n = int(shared_rings), int(prompt_rings)
        if n:
            if kv_dtype is not None or K:
                raise ValueError('prompt rings are bf16 rings under sampling: neither kv_dtype nor shared_rings goes with them')
            return PromptRings(n, tail_len)
        if K:
            if kv_dtype is not None:
                raise ValueError(f'shared rings are bf16 rings: kv_dtype={kv_dtype!r} is not supported')
            return SharedRings(K)
        return FP8Rings() if kv_dtype == 'fp8' else RingLayout()

    def _tables(self):
        if self.rd is None:
            e, c = self.eng, self.eng.cfg
            phi = ops.sinusoid_table(c.mem_len, c.d_model, c.clamp_len, e.dev)
            self.rd = []
            for l in range(c.n_layer):
                rd = torch.empty(c.mem_len, c.d_model, device=e.dev, dtype=torch.bfloat16)
                ops.gemm(phi, e._lw(l, 'dec_attn.r_net.weight'), rd, c.mem_len, c.d_model, c.d_model)
                self.rd.append(rd)

    def invalidate_tables(self):
        """call after the weights change (r_net feeds the cached Rd tables)"""
        self.rd = None
        self.graph = None

    # ---------------------------------------------------------------- prompt
    def prefill(self, prompt: torch.Tensor, sampling: dict, n_pad: Optional[torch.Tensor] = None, rules: RulePlan = NO_RULES,
                search: str = 'beam'):
        """Whole prompt through the training-shape kernels with zero mems (upstream first step), rings filled from the
        per-layer qkv buffers, first new token sampled from the last position.
        n_pad: (B,) int32 device tensor, left-padded prompts: the first n_pad[b] columns of row b are pads.  Their K / V are zero
        in every layer (= extra zero-memory slots, so each row computes what it computes alone), they are embedded as id 0 and
        held as -1 in `ids`, which the samplers' repetition penalty skips.
        rules: the RulePlan of the generation (rules_config; RowRules.start sets the rows' words from it on the device, pads
        skipped).  Every row starts live, and the first token sampled here counts.  A prompt that breaks the grammar, overfills or
        underfills a bar under a bar budget, or a guide that does not fit its row's bar length raises (RowRules.check_prompt).
        search: what a call without `sampling` is the prompt pass of, 'beam' or 'contrastive'; its caller picks the token from logp.
        Under a layout with one ring per `unit` rows (rings.py) `prompt` and n_pad still hold all B rows, the pass runs on every
        unit-th of them and the layout spreads the last position's log-probabilities; ids and the rule words start in all B rows."""
        e, c, lay = self.eng, self.eng.cfg, self.layout
        B, Tp = prompt.shape
        assert B == self.B and Tp + 1 <= self.Tmax + 1
        if lay.serves not in (None, 'sample' if sampling is not None else search):
            raise MusicXLError(lay.alone)
        u, rows = lay.unit, B // lay.unit
        self._tables()
        self.beam_rings = 'copied'                          # every row reads its own ring until a beam_begin says otherwise
        x = prompt.to(e.dev)
        lay.check_prompt(x)
        for k in lay.tensors():                             # (fp8: zero bytes with e = 0 are the zero memories)
            k.zero_()
        self.ids.zero_()
        self.ids[:, :Tp].copy_(x)
        if n_pad is not None:
            n_pad = n_pad.to(e.dev, torch.int32).contiguous()
            pad = torch.arange(Tp, device=e.dev)[None, :] < n_pad[:, None]
            self.ids[:, :Tp].masked_fill_(pad, -1)
            x = x.masked_fill(pad, 0)
        self.rules.start(self.ids, Tp, c.vocab_size, rules)
        if u > 1:                                           # one prompt row per ring
            x, n_pad = x[::u].contiguous(), None if n_pad is None else n_pad[::u].contiguous()
        out = e.forward(x, mems=None, labels=None, train=False, want_logprobs=False, kv_sink=lambda l, qkv: lay.kv_sink(l, qkv, Tp),
                        n_pad=n_pad)
        ws = e._last
        # log-probs of the last prompt position only
        if ws.logits is None:       # bucketed (large-vocabulary) head: the (N, V) logits were never formed; project B rows here
            lay.spread(ws.hid.view(rows, Tp, -1)[:, Tp - 1], self.tmp)
            self._head(self.tmp)
        else:
            logp = self.logp if u == 1 else torch.empty(rows, c.vocab_size, device=e.dev, dtype=torch.float32)
            ops.adaptive_logprob(ws.logits.view(rows, Tp, -1)[:, Tp - 1], logp, rows, c.vocab_size, tuple(c.cutoffs))
            if u > 1:
                lay.spread(logp, self.logp)
        self.t_dev.fill_(Tp - 1)
        if lay.t0_dev is not None:
            lay.t0_dev.fill_(Tp)
        self._trace()
        self.rules.check_prompt(self.ids)
        if sampling is not None:                       # None: the caller picks the token from self.logp (a search)
            self._sample_advance(self.logp, sampling)  # t = Tp: position of the token just sampled
        return out

    def _sample_advance(self, scores, sampling: dict):
        """next token of every row from `scores` (log-probabilities, or the head's logits: see mxl_sample_step) -> ids[:, t + 1];
        position and RNG counters advanced.  Short chain: the same launch leaves the token's embedding row in h[0] for the next step."""
        c = self.eng.cfg
        state = self.rules.state()
        if self.fused_sampler:      # the masks, the stop rule, the live-row count and the state advance ride on the sampler launch
            ops.sample_step(scores, c.vocab_size, self.ids, self.t_dev, self.rng, self.seed,
                            self.eng.w16('transformer.word_emb.emb_layers.0.weight'), self.h[0], math.sqrt(c.d_model), self.step_ctr,
                            state, **sampling)
        else:
            sample_unfused(scores, c.vocab_size, self.ids, self.t_dev, self.rng, self.seed, sampling, state)

    # ---------------------------------------------------------------- one token
    def force_tokens(self, tokens: torch.Tensor):
        """teacher forcing / constrained decoding: `tokens` (B,) replace the ids at the current position t (what the sampler just
        wrote) before the next `step`; with the fused sampler the embedding row the sampler left for that step follows"""
        self.ids.index_copy_(1, self.t_dev.to(torch.int64), tokens.to(self.ids.device, torch.int64).unsqueeze(1))
        if self.fused_sampler:
            c = self.eng.cfg
            ops.decode_embed(self.ids, self.t_dev, self.eng.w16('transformer.word_emb.emb_layers.0.weight'), self.h[0], math.sqrt(c.d_model))

    def step(self, sampling: dict, want_logp: bool = False):
        """one more token for every row.  want_logp: self.logp is needed after the step (it always holds the log-probabilities when
        a trace is attached, the head is adaptive or a repetition penalty is in force)"""
        # the log-softmax launch is only needed for what reads log-probabilities: the trace, an adaptive (clustered) head, and the
        # repetition penalty (sign-dependent); every other warper and the draw itself are shift-invariant (mxl_sample_step)
        raw = (self.fused_sampler and self.trace is None and not want_logp and not tuple(self.eng.cfg.cutoffs)
               and sampling.get('repetition_penalty', 1.0) == 1.0)
        self._forward_token(embed=not self.fused_sampler, want_logp=not raw)
        self._sample_advance(self.logits if raw else self.logp, sampling)

    def _forward_token(self, embed: bool = True, want_logp: bool = True):
        """the token at position t (ids[:, t], t on the device) through the model: K/V appended to the rings at slot t mod M,
        self.logp = log-probabilities of position t + 1 (want_logp=False: only self.logits, the head's raw rows).
        embed=False: h[0] already holds the token's embedding row (written by the previous step's sampler launch)."""
        e, c = self.eng, self.eng.cfg
        B, d, Fi, L = self.B, c.d_model, c.d_inner, c.n_layer
        E = e.w16('transformer.word_emb.emb_layers.0.weight')
        G = ops.gemm_skinny if B <= 64 else ops.gemm     # weight-streaming form for decode batches
        # indexed rings: the attention of every layer reads a slot from the row the one table names (the append stays each row's own)
        owned = dict(owner=self.owner, nb=self._beam_args[0]) if self.beam_rings == 'indexed' else {}
        live = None if self.rules.stop is None else self.unfinished
        if embed:
            ops.decode_embed(self.ids, self.t_dev, E, self.h[0], math.sqrt(d))
        for l in range(L):
            h_in, h_out = self.h[l & 1], self.h[(l + 1) & 1]
            self.layout.layer(self, l, h_in, live, owned)       # projection, ring append and ring attention: h_in -> self.av
            G(self.av, e._lw(l, 'dec_attn.o_net.weight'), self.tmp, B, d, d)
            ops.ln_residual_fwd(self.tmp, h_in, e._lw(l, 'dec_attn.layer_norm.weight', e.P),
                                e._lw(l, 'dec_attn.layer_norm.bias', e.P), self.h1, eps=c.layer_norm_epsilon)
            G(self.h1, e._lw(l, 'pos_ff.CoreNet.0.weight'), self.a, B, Fi, d, flags=ops.GEMM_BIAS | ops.GEMM_RELU,
              bias=e._lw(l, 'pos_ff.CoreNet.0.bias', e.P))
            if B <= 64:
                # N = d columns are only d/16 workgroups: slice K four ways as well; the slabs are summed by the LayerNorm launch
                ops.gemm_skinny_partial(self.a, e._lw(l, 'pos_ff.CoreNet.3.weight'), self.slabs, B, d, Fi, 4)
                ops.ln_residual_fwd_partial(self.slabs, 4, e._lw(l, 'pos_ff.CoreNet.3.bias', e.P), self.h1,
                                            e._lw(l, 'pos_ff.layer_norm.weight', e.P), e._lw(l, 'pos_ff.layer_norm.bias', e.P),
                                            h_out, eps=c.layer_norm_epsilon)
            else:
                G(self.a, e._lw(l, 'pos_ff.CoreNet.3.weight'), self.tmp, B, d, Fi, flags=ops.GEMM_BIAS,
                  bias=e._lw(l, 'pos_ff.CoreNet.3.bias', e.P))
                ops.ln_residual_fwd(self.tmp, self.h1, e._lw(l, 'pos_ff.layer_norm.weight', e.P),
                                    e._lw(l, 'pos_ff.layer_norm.bias', e.P), h_out, eps=c.layer_norm_epsilon)
        self._head(self.h[L & 1], want_logp)
        if want_logp:
            self._trace()

    def _head(self, hid, want_logp: bool = True):
        """(B, d) hidden states -> self.logp: all head rows (vocabulary + cluster rows) in one weight-streaming GEMM, then the
        adaptive log-softmax over the row (HF `ProjectedAdaptiveLogSoftmax.log_prob`, the labels=None branch)"""
        e, c = self.eng, self.eng.cfg
        B, d = self.B, c.d_model
        G = ops.gemm_skinny if B <= 64 else ops.gemm
        nrow, nrow_p = e.layout.n_head_rows, e.layout.head_rows_padded
        head_w = e.W[:nrow_p * d].view(nrow_p, d)
        boff = e.layout.entries['crit.out_layers.0.bias'][0]
        G(hid, head_w, self.logits, B, nrow, d, flags=ops.GEMM_OUT_F32 | ops.GEMM_BIAS, bias=e.P[boff:boff + nrow])
        if want_logp:
            ops.adaptive_logprob(self.logits, self.logp, B, c.vocab_size, tuple(c.cutoffs))

    # ---------------------------------------------------------------- beam-search hooks (see beam_search below)
    def _bf16_rings_only(self, what: str):
        """the searches move rings with mxl_beam_reorder / mxl_ring_slot_broadcast / index_select, which know the bf16 layout alone"""
        if not self.layout.movable:
            raise ValueError(f'{what} does not take {self.layout.kv_dtype} K/V rings')

    def beam_prefill(self, prompt: torch.Tensor):
        self._bf16_rings_only('beam search')
        self.prefill(prompt, None)

    def beam_logp(self) -> torch.Tensor:
        return self.logp

    def beam_reorder(self, beam_idx: torch.Tensor):
        """rows follow their beams: id history and both rings of every layer (HF `_reorder_cache`: index_select on the mems)"""
        self.ids.copy_(self.ids.index_select(0, beam_idx))
        for ring in self.layout.rings():
            ring.copy_(ring.index_select(0, beam_idx))

    def beam_advance(self, cur_len: int):
        """the token at position cur_len - 1 through the model -> log-probs of position cur_len"""
        self.t_dev.fill_(cur_len - 1)
        self._forward_token()

    # ---------------------------------------------------------------- beam search on the device (beam_search_device below)
    def beam_begin(self, prompt: torch.Tensor, max_length: int, nb: int, eos: int, pad: int, length_penalty: float,
                   early_stopping: bool, use_graph: bool = True, rules: RulePlan = NO_RULES, ng: int = 1,
                   diversity_penalty: float = 0.0, sample: bool = False, top_k: Optional[int] = None, top_p: Optional[float] = None,
                   temperature: float = 1.0, typical_p: Optional[float] = None, beam_rings: str = 'copied') -> int:
        """prompt pass (one row per beam, `rules` started as `prefill` starts them, with the stop group (eos, pad, 0) always on:
        its `unfinished` word is how mxl_beam_step retires dead rows and done items) + the scorer's state + (use_graph) capture of
        one beam step (`_capture`; the hypothesis store, the running scores and the log-probabilities are this step's own state);
        returns the number of `replay_once()` calls before the last selection (`beam_select`).
        ng > 1: diverse beam search, the nb beams of an item in ng groups with `diversity_penalty` between them (mxl_group_beam_step
        in place of mxl_beam_step); both are part of the graph key.
        sample: beam-sample, ng = 1 -- the step draws its candidates (mxl_beam_sample_draw under the warpers top_k / top_p / temperature
        / typical_p with the decoder's seed, into the decoder's `drawn` buffer) and walks them with mxl_beam_sample_step; the draw
        counter starts at 0, so a seed gives one result.  The flag and the warpers are part of the graph key, `drawn` is step state.
        beam_rings: 'copied' -- the step moves whole ring rows with mxl_beam_reorder -- or 'indexed': the rings stay where the forward
        pass wrote them, the `owner` table (identity after the prompt pass: every row holds its own prompt) follows the beams with
        mxl_beam_owner_follow and the attention reads through it (mxl_relattn_decode_owned); M % 16 == 0.  The mode is part of the
        graph key, the table is step state.
        A decoder with kv_dtype='fp8' takes 'indexed': every step appends to the row's own slot (mxl_kv_append_fp8) -- the slot the
        follow kernel marks as the row's own -- and mxl_relattn_decode_fp8_owned reads through the table, so no ring is ever moved.
        'copied' on such a decoder is the reference of the tests and nothing else (rings.FP8Rings.follow_beams: index_select, a temporary
        copy of every ring per step): eager only (MusicXLError under use_graph) and not reachable from `generate`."""
        if beam_rings not in DECODER_BEAM_RINGS:
            raise ValueError(f"beam_rings={beam_rings!r}: expected 'copied' or 'indexed'")
        if not self.layout.movable and beam_rings == 'copied' and use_graph:
            raise MusicXLError(f"beam search on the device moves {self.layout.kv_dtype} K/V rings with index_select alone, the eager reference "
                               "of the tests: use_graph=False, or beam_rings='indexed'")
        if beam_rings == 'indexed' and self.eng.cfg.mem_len % 16:
            raise MusicXLError(f"beam_rings='indexed' takes a mem_len that is a multiple of 16, not {self.eng.cfg.mem_len}")
        if max_length > self.Tmax:
            raise MusicXLError(f'max_length {max_length} exceeds the decoder buffer {self.Tmax}')
        if nb < 2 or nb > BEAM_MAX or self.B % nb:
            raise MusicXLError(f'beam search on the device takes 2..{BEAM_MAX} beams and one decoder row per beam')
        if ng < 1 or nb % ng or not 0.0 <= diversity_penalty < math.inf:
            raise MusicXLError(f'group beam search on the device takes groups that divide the {nb} beams and a finite diversity_penalty '
                               '>= 0')
        if sample and (ng != 1 or self.eng.cfg.vocab_size > 2048):
            raise MusicXLError('beam-sample on the device takes one group and a vocabulary of at most 2048 tokens')
        self.prefill(prompt, None, None, rules.with_stop((int(eos), int(pad), 0)))
        if self.beam is None or self.beam.nb != nb:
            self.beam = BeamStore(self.B // nb, nb, self.ids.shape[1], self.eng.dev)
            self.ring_table = ops.beam_table(self.layout.rings())
        self.beam.start(ng)
        self._beam_args = (int(nb), int(eos), int(pad), float(length_penalty), bool(early_stopping), int(ng), float(diversity_penalty),
                           bool(sample), int(top_k or 0), float(1.0 if top_p is None else top_p),
                           float(1.0 if temperature is None else temperature), float(1.0 if typical_p is None else typical_p))
        extra = ()
        self.beam_rings = beam_rings
        if beam_rings == 'indexed':
            if self.owner is None:
                self.owner = torch.empty(self.B, self.eng.cfg.mem_len, device=self.eng.dev, dtype=torch.uint8)
            self.owner.copy_((torch.arange(self.B, device=self.eng.dev) % nb).to(torch.uint8)[:, None].expand_as(self.owner))
            extra = (self.owner,)
        if sample:
            self.rng.zero_()
            if self.drawn is None:
                self.drawn = torch.empty_like(self.logp)
            extra += (self.drawn,)
        self._use_graph, self._step, self.finished_by = use_graph, ('beam_step',), (self.beam.n_done, self.beam.Bs)
        steps = max_length - prompt.shape[1] - 1
        if steps > 0 and use_graph:
            key = (('beam', beam_rings) + self.layout.key + self._beam_args + (None if self.trace is None else self.trace.data_ptr(),)
                   + self.rules.graph_key(self.eng.dev))
            st = self.beam               # (logp: the step starts from the log-probabilities the last one left)
            self._capture(key, (st.scores, st.hyp_ids, st.hyp_score, st.ints, self.logp) + extra)
        return max(steps, 0)

    def beam_select(self):
        """rules mask -> mxl_beam_step (mxl_group_beam_step under ng > 1; under `sample` mxl_beam_sample_draw into `drawn`, then
        mxl_beam_sample_step over it): the beams of every item chosen, finished hypotheses stored, ids and the rule words reordered,
        the chosen tokens at column t + 1"""
        V, st = self.eng.cfg.vocab_size, self.beam
        nb, eos, pad, lp, early, ng, pen, sample, top_k, top_p, temperature, typical_p = self._beam_args
        rules = self.rules.state().in_force()
        ops.rules_mask(self.logp, V, self.t_dev, rules)
        store = (st.hyp_ids, st.hyp_len, st.hyp_score, st.hyp_n, st.done, st.n_done, st.beam_idx, st.moved)
        words = dict(words=self.rules.buf, n_words=len(RowRules.WORDS))
        if sample:
            ops.beam_sample_draw(self.logp, V, st.scores, nb, self.rng, self.seed, self.drawn, top_k, top_p, temperature, typical_p)
            ops.beam_sample_step(self.drawn, V, st.scores, self.ids, self.t_dev, nb, eos, pad, lp, early, *store, **words)
            return rules
        ops.beam_step(self.logp, V, st.scores, self.ids, self.t_dev, nb, eos, pad, lp, early, *store, **words, ng=ng, diversity_penalty=pen)
        return rules

    def beam_step(self):
        """one whole beam step, no host read: beam_select, the K/V rings of every layer follow their beams (one launch over a
        table of the rings; under beam_rings='indexed' the owner table follows in their place, M bytes per row), the position moves
        on, the rule words move along the chosen tokens (rows that mxl_beam_step retired keep theirs), and the chosen tokens go
        through the model"""
        rules = self.beam_select()
        if self.beam_rings == 'indexed':
            ops.beam_owner_follow(self.owner, self._beam_args[0], self.beam.beam_idx, self.beam.moved, self.t_dev)
        else:                       # whole ring rows move: mxl_beam_reorder, or the fp8 layout's index_select reference
            self.layout.follow_beams(self)
        ops.decode_advance(self.t_dev, self.rng)
        if rules.moves_words:
            ops.rules_advance(self.ids, self.t_dev, rules)
        self._forward_token()

    # ---------------------------------------------------------------- contrastive search on the device (contrastive_search_device)
    def contrastive_begin(self, prompt: torch.Tensor, max_length: int, K: int, alpha: float, eos: Optional[int], pad: int,
                          use_graph: bool = True, rules: RulePlan = NO_RULES) -> int:
        """prompt pass (one row per candidate: the K rows of a sequence hold the same prompt; `rules` started as `prefill` starts
        them, with the stop group (eos, pad, 0) always on -- eos None: -1, never emitted) + the store + (use_graph) capture of one
        contrastive step (`_capture`) + the first token, chosen by one step run here; returns the number of `replay_once()` calls that
        complete the generation to max_length.  The store's words and the log-probabilities are this step's own state (its context
        rows need no snapshot: a step writes position t and reads those below it)."""
        self._bf16_rings_only('contrastive search')
        if max_length > self.Tmax:
            raise MusicXLError(f'max_length {max_length} exceeds the decoder buffer {self.Tmax}')
        if K < 2 or K > CONTRASTIVE_MAX or self.B % K:
            raise MusicXLError(f'contrastive search on the device takes 2..{CONTRASTIVE_MAX} candidates and one decoder row per '
                               'candidate')
        c, Tp = self.eng.cfg, prompt.shape[1]
        self.layout.admit_candidates(K)     # (under shared rings the pass runs on every K-th row: the K of a prompt hold the same)
        self.prefill(prompt, None, None, rules.with_stop((-1 if eos is None else int(eos), int(pad), 0)), search='contrastive')
        if self.cs is None or self.cs.K != K:
            self.cs = ContrastiveStore(self.B // K, K, self.Tmax, c.d_model, self.eng.dev)
            self.ring_table = ops.beam_table(self.layout.rings())
        u = self.layout.unit        # the model saw every u-th row: the first row of every sequence is every (K / u)-th of those
        self.cs.start(self.eng._last.h[c.n_layer & 1].view(self.B // u, Tp, c.d_model)[::K // u])
        self._cs_args = (int(K), float(alpha), self.rules.stop[0], int(pad))
        self._use_graph, self._step, self.finished_by = use_graph, ('contrastive_step',), (self.cs.n_done, self.cs.B0)
        steps = max_length - Tp - 1
        if steps > 0 and use_graph:
            key = (('contrastive',) + self.layout.key + self._cs_args
                   + (None if self.trace is None else self.trace.data_ptr(),) + self.rules.graph_key(self.eng.dev))
            self._capture(key, (self.cs.ints, self.logp))
        self.contrastive_step()                       # the first token: column Tp
        return max(steps, 0)

    def contrastive_step(self):
        """one whole contrastive step, no host read: the rules mask on the log-probabilities, the K candidates of every sequence
        from its picked row (mxl_contrastive_topk), the position moves on, the candidates go through the model, one is picked and
        written to all K rows (mxl_contrastive_step), the rule words move along it, and the one ring slot the step wrote follows the
        pick in every layer (mxl_ring_slot_broadcast; the invariant is stated in csrc/contrastive.hip) -- or, with shared rings, the
        picked row's stashed k / v go into the prompt's rings (the layout's `settle`)"""
        c, cs = self.eng.cfg, self.cs
        K, alpha, eos, pad = self._cs_args
        rules = self.rules.state().in_force()
        ruled = rules.moves_words
        if ruled:
            ops.rules_mask(self.logp, c.vocab_size, self.t_dev, rules)
        ops.contrastive_topk(self.logp, c.vocab_size, cs.sel, self.ids, self.t_dev, cs.probs, cs.dead, self.unfinished, pad)
        ops.decode_advance(self.t_dev, self.rng)
        self._forward_token()
        # under a rule the advance launch applies the stop rule to `unfinished` itself, after it has moved the words of the rows
        # that were live when they chose the token
        ops.contrastive_step(cs.ctx, cs.inv, self.t_dev, self.h[c.n_layer & 1], cs.probs, cs.dead, alpha, cs.score, cs.sel, self.ids,
                             self.unfinished, cs.n_done, eos, pad, stop_later=ruled)
        if ruled:
            ops.rules_advance(self.ids, self.t_dev, rules)
        self.layout.settle(self, K)     # the slot of the step follows the pick, or the picked row's stash is committed to it

    def _trace(self):
        if self.trace is not None:
            self.trace.index_copy_(1, self.t_dev.to(torch.int64), self.logp.unsqueeze(1))

    # ---------------------------------------------------------------- loop
    def begin(self, prompt: torch.Tensor, max_length: int, sampling: dict, use_graph: bool = True,
              n_pad: Optional[torch.Tensor] = None, rules: RulePlan = NO_RULES) -> int:
        """prompt pass + first sampled token + (use_graph) capture of one decode step; returns the number of `replay_once()`
        calls that complete the generation to max_length.  n_pad: left-padded prompts (prefill); the decode step is the same,
        every row's last prompt token sits at column Tp - 1.  rules: the RulePlan of the generation (rules_config).  The captured
        step is another launch under every rule, and it reads the rules' device tables: which rules are on, the identity of their
        tables and their class masks, the guide buffer and the register gap are part of the graph key (RowRules.graph_key).  The
        per-row values -- bar counts, keys, guide tokens and positions, bounds, parts and floors -- are step state, so a later
        generation with other values, such as another guide that fits the buffer, replays the same graph"""
        if max_length > self.Tmax:
            raise MusicXLError(f'max_length {max_length} exceeds the decoder buffer {self.Tmax}')
        if self.Mt is not None and self.Mt < min(self.eng.cfg.mem_len, max_length - prompt.shape[1]):
            raise MusicXLError(f'the tail rings of this decoder hold {self.Mt} generated positions, the call asks for '
                               f'{max_length - prompt.shape[1]} (XLDecoder(tail_len=))')
        self._use_graph, self._step, self.finished_by = use_graph, ('step', sampling), (self.alive, 0)
        self.prefill(prompt, sampling, n_pad, rules)
        steps = max_length - prompt.shape[1] - 1
        if steps > 0 and use_graph:
            # step() picks its launches from the sampling keys, the sampler form and whether a trace is attached (the trace buffer
            # itself is written by the captured launches): a graph captured without a trace would replay without writing one
            key = (tuple(sorted(sampling.items())), self.fused_sampler,
                   None if self.trace is None else self.trace.data_ptr()) + self.rules.graph_key(self.eng.dev) + (self.layout.key,)
            self._capture(key, (self.h[0],))      # (short chain: the next step's embedding row is step state too)
        return max(steps, 0)

    def _step_once(self):
        """the step of the last begin: `_step` = (its method's name, its arguments).  The bound method itself, kept on the decoder,
        would tie it into a reference cycle; a decoder then dies in the cycle collector, which may run inside another decoder's
        capture, where freeing a graph and device memory aborts the process"""
        getattr(self, self._step[0])(*self._step[1:])

    def _capture(self, key: tuple, extra: tuple):
        """one step captured in `graph` under `key`, unless the graph at hand was captured under that key: a warm-up step on a
        side stream (first launches set function attributes), then the capture, and the state that the two extra steps consumed is
        put back -- the position, the draw counter, ids, the rings, the rule words and `extra`, the tensors that only this step form
        carries from one step to the next"""
        if self.graph is not None and self._graph_key == key:
            return
        live = (self.t_dev, self.rng, self.ids, *self.layout.tensors(), *extra)
        saved, words = [t.clone() for t in live], self.rules.snapshot()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step_once()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()       # hipGraph on ROCm
        with torch.cuda.graph(self.graph):
            self._step_once()
        self._graph_key = key
        for t, v in zip(live, saved):
            t.copy_(v)
        self.rules.restore(words)

    def replay_once(self):
        """one more step of what the last begin / beam_begin / contrastive_begin started (on the current stream)"""
        if self._use_graph:
            self.graph.replay()
        else:
            self._step_once()


class XLDecoderLanes(RuledGenerate):
    """The batch as `lanes` independent XLDecoders of B / lanes sequences, each with its own hipGraph, replayed on its own
    stream.  A decode step is ~100 small dependent launches around 12 ring-attention launches: alone, the small launches run at
    launch / latency cost with the chip idle and the ring streaming waits for them; with two lanes one lane's small launches
    overlap the other's ring streaming (sequences are independent: the lanes never synchronise until the generation ends).
    Same interface as XLDecoder for `generate` / `begin` / `replay_once`; rows keep their order."""

    def __init__(self, engine, batch: int, max_total_len: int, seed: int = 1234, lanes: int = 2, kv_dtype: Optional[str] = None,
                 prompt_rings: int = 0, tail_len: Optional[int] = None):
        """prompt_rings = n > 0: every lane is an XLDecoder(prompt_rings=n), and the lanes are cut at prompt boundaries -- the batch / n
        prompts are dealt to the lanes as the rows are otherwise, so lanes <= batch / n.  The ids equal the default mode's exactly when
        both put every row at the same index of the same lane (the draw is keyed by the lane's seed and the row's index in it): when
        the default's cut falls between two prompts."""
        unit = XLDecoder._layout(kv_dtype, 0, prompt_rings, tail_len).unit        # the rows that share a ring stay in one lane
        assert batch % unit == 0 and 1 <= lanes <= batch // unit
        self.B, self.Tmax, self.n, self.kv_dtype, self.prompt_n = batch, max_total_len, lanes, kv_dtype, int(prompt_rings)
        units = batch // unit
        self.sizes = [(units // lanes + (1 if i < units % lanes else 0)) * unit for i in range(lanes)]
        self.offs = [sum(self.sizes[:i]) for i in range(lanes + 1)]
        more = dict(prompt_rings=prompt_rings, tail_len=tail_len) if prompt_rings else {}
        # (the sampler draws per (seed, row, step): a different seed per lane keeps the lanes' draws independent)
        self.lanes = [XLDecoder(engine, b, max_total_len, seed=seed + 7919 * i, kv_dtype=kv_dtype, **more)
                      for i, b in enumerate(self.sizes)]
        self.ring_spec = self.lanes[0].ring_spec
        self.streams = [torch.cuda.Stream() for _ in range(lanes)]

    def invalidate_tables(self):
        for d in self.lanes:
            d.invalidate_tables()

    def begin(self, prompt, max_length, sampling, use_graph=True, n_pad=None, rules: RulePlan = NO_RULES) -> int:
        steps = [d.begin(prompt[lo:hi], max_length, sampling, use_graph, None if n_pad is None else n_pad[lo:hi], rules.rows(lo, hi))
                 for d, lo, hi in zip(self.lanes, self.offs, self.offs[1:])]
        for s in self.streams:                       # the lanes start from the prompt passes and captures issued above
            s.wait_stream(torch.cuda.current_stream())
        return steps[0]

    def replay_once(self):
        for d, s in zip(self.lanes, self.streams):
            with torch.cuda.stream(s):
                d.replay_once()

    def join(self):
        for s in self.streams:
            torch.cuda.current_stream().wait_stream(s)


class _BeamHyps:
    """HF 4.25.1 generation/beam_search.py `BeamHypotheses`: the best finished hypotheses of one batch item"""

    def __init__(self, num_beams: int, length_penalty: float, early_stopping: bool):
        self.num_beams, self.length_penalty, self.early_stopping = num_beams, length_penalty, early_stopping
        self.beams, self.worst_score = [], 1e9
        self.done = False                   # HF BeamSearchScorer._done of this item

    def add(self, hyp: torch.Tensor, sum_logprobs: float):
        score = sum_logprobs / (hyp.shape[-1] ** self.length_penalty)
        if len(self.beams) < self.num_beams or score > self.worst_score:
            self.beams.append((score, hyp))
            if len(self.beams) > self.num_beams:
                ranked = sorted((sc, i) for i, (sc, _) in enumerate(self.beams))
                del self.beams[ranked[0][1]]
                self.worst_score = ranked[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs: float, cur_len: int) -> bool:
        if len(self.beams) < self.num_beams:
            return False
        if self.early_stopping:
            return True
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty

    def walk(self, toks, scores, rows, n: int, eos: int, ids: torch.Tensor, cur_len: int):
        """HF `BeamSearchScorer.process` for this item: its 2 * n candidates in score order (token, running score, decoder row of
        the beam each continues).  An eos among the first n ranks puts that beam's ids[row, :cur_len] on the heap, the first n
        other candidates continue: returns their (scores, tokens, rows), and `done` is updated."""
        n_s, n_t, n_i = [], [], []
        for rank, (tok, s_, src) in enumerate(zip(toks, scores, rows)):
            if tok == eos:
                if rank >= n:
                    continue
                self.add(ids[src, :cur_len].clone(), s_)
            else:
                n_s.append(s_); n_t.append(tok); n_i.append(src)
            if len(n_s) == n:
                break
        if len(n_s) < n:
            raise MusicXLError(f'at most {n} tokens in the top {2 * n} can be eos')
        self.done = self.done or self.is_done(max(scores), cur_len)
        return n_s, n_t, n_i


def _beam_finalize(hyps, nb: int, keep: int, ids: torch.Tensor, cur_len: int, beam_scores: torch.Tensor, max_length: int, eos: int,
                   pad: int, return_scores: bool):
    """HF `BeamSearchScorer.finalize`: the open beams (rows b * nb .. of ids, their running scores) of every item that is not done
    join its heap, the best `keep` of each heap are returned as (len(hyps) * keep, L) ids, each followed by eos where there is
    room and padded with pad, L = the longest + 1 capped at max_length"""
    final = beam_scores.tolist()
    for b, hyp in enumerate(hyps):
        if not hyp.done:
            for j in range(nb):
                hyp.add(ids[b * nb + j, :cur_len].clone(), final[b * nb + j])
    best, scores = [], []
    for hyp in hyps:
        ranked = sorted(hyp.beams, key=lambda x: x[0])
        for _ in range(keep):
            sc_, h = ranked.pop()
            best.append(h); scores.append(sc_)
    L = min(max(len(h) for h in best) + 1, max_length)
    out = torch.full((len(best), L), pad, dtype=torch.int64, device=ids.device)
    for i, h in enumerate(best):
        out[i, :len(h)] = h
        if len(h) < L:
            out[i, len(h)] = eos
    return (out, torch.tensor(scores)) if return_scores else out


def _beam_loop(dec, prompt: torch.Tensor, max_length: int, nb: int, ng: int, pen: float, Bs: int, keep: int, pick,
               early_stopping: bool, length_penalty: float, eos: int, pad: Optional[int], return_scores: bool, allowed):
    """The one host beam loop, under `beam_search` (ng = 1, pen = 0) and `group_beam_search`: Bs items of nb beams in ng groups, one
    decoder row per beam.  Per step ONE forward for all beams (the kernels of `step`), then the groups in order: group g's
    log-probabilities, lowered by pen x (how many beams of the EARLIER groups of the same item chose that token at this step;
    HammingDiversityLogitsProcessor), plus the running scores give the 2 x group size candidates per item in score order -- the
    best, or `pick(scores (Bs * group size, V))` -- the scorer walks them on the host (a data-dependent loop over a handful of
    scalars, as in HF 4.25.1; one hypothesis heap and one done flag per item, shared by its groups), and the K/V rings and the id
    history follow their beams (HF `_reorder_cache`).  The rows of a done item stay where they are, as mxl_beam_step leaves them,
    filled with pad at running score 0; what they hold in `dec.ids` and in the running scores from then on is part of no contract:
    `_beam_finalize` skips done items, so the returned ids and scores do not depend on it."""
    dev, V, pad = dec.eng.dev, dec.eng.cfg.vocab_size, eos if pad is None else pad
    (B0, Tp), gs, rows = prompt.shape, nb // ng, Bs * nb
    if keep > nb:
        raise MusicXLError('num_return_sequences has to be smaller or equal to num_beams')
    if dec.B != rows or max_length > dec.Tmax:
        raise MusicXLError(f'the decoder was built for {dec.B} rows x {dec.Tmax} positions, {"group " * (ng > 1)}beam search needs '
                           f'{rows} x {max_length}')
    dec.beam_prefill(prompt.repeat_interleave(rows // B0, 0).to(dev))
    beam_scores = torch.tensor(([0.0] + [-1e9] * (gs - 1)) * (Bs * ng), device=dev)      # the first beam of every group leads
    hyps = [_BeamHyps(nb, length_penalty, early_stopping) for _ in range(Bs)]
    cur_len, ident = Tp, torch.arange(rows, device=dev)
    group_rows = ident.view(Bs, ng, gs).transpose(0, 1).reshape(ng, Bs * gs)       # the decoder rows of every group, item by item
    while True:
        logp = dec.beam_logp()                                   # (rows, V), every beam of every group
        if allowed is not None:
            logp = logp.masked_fill(~torch.as_tensor(allowed(dec.ids[:, :cur_len])).to(logp.device, torch.bool), float('-inf'))
        if ng > 1:                                               # this step's running scores, tokens and source rows, filled group by group
            new_scores, tokens, beam_idx = beam_scores.clone(), torch.zeros(rows, dtype=torch.int64, device=dev), ident.clone()
        for g in range(ng):
            g0, gidx = g * gs, group_rows[g]
            sc, run = logp, beam_scores                          # (one group: no gather)
            if ng > 1:
                sc, run = logp.index_select(0, gidx), beam_scores.index_select(0, gidx)
            if pen > 0.0 and g > 0:
                # the tokens the earlier groups of the same item have just chosen; under `allowed`, a -inf continuation is no choice
                prev = tokens.view(Bs, nb)[:, :g0]
                live = torch.ones_like(prev, dtype=torch.float32)
                if allowed is not None:
                    live = torch.isfinite(new_scores.view(Bs, nb)[:, :g0]).to(torch.float32)
                sc = sc - pen * torch.zeros(Bs, V, device=dev).scatter_add_(1, prev, live).repeat_interleave(gs, 0)
            sc = sc + run[:, None]
            top_s, top_i = pick(sc) if pick is not None else sc.view(Bs, gs * V).topk(2 * gs, dim=1, largest=True, sorted=True)
            top_b, top_t, top_sl = (top_i // V).tolist(), (top_i % V).tolist(), top_s.tolist()
            # what a done item keeps: score 0, token pad, its rows where they are
            n_s, n_t = [[0.0] * gs for _ in range(Bs)], [[pad] * gs for _ in range(Bs)]
            n_i = [list(range(b * nb + g0, b * nb + g0 + gs)) for b in range(Bs)]
            for b in range(Bs):
                if not hyps[b].done:
                    n_s[b], n_t[b], n_i[b] = hyps[b].walk(top_t[b], top_sl[b], [b * nb + g0 + j for j in top_b[b]], gs, eos, dec.ids,
                                                          cur_len)
            up = [torch.tensor(x, device=dev).view(-1) for x in (n_s, n_t, n_i)]
            if ng == 1:
                new_scores, tokens, beam_idx = up
            else:
                new_scores[gidx], tokens[gidx], beam_idx[gidx] = up
        beam_scores = new_scores
        if not torch.equal(beam_idx, ident):
            dec.beam_reorder(beam_idx)
        dec.ids[:, cur_len] = tokens
        cur_len += 1
        if all(h.done for h in hyps) or cur_len >= max_length:
            break
        dec.beam_advance(cur_len)
    return _beam_finalize(hyps, nb, keep, dec.ids, cur_len, beam_scores, max_length, eos, pad, return_scores)


def beam_search(dec, prompt: torch.Tensor, max_length: int, num_beams: int = 3, do_sample: bool = False,
                top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: float = 1.0,
                typical_p: Optional[float] = None, early_stopping: bool = True, length_penalty: float = 1.0,
                num_return_sequences: int = 1, eos_token_id: int = 0, pad_token_id: Optional[int] = None,
                renormalize_logits: bool = True, generator: Optional[torch.Generator] = None, return_scores: bool = False,
                allowed=None):
    """HF 4.25.1 `beam_search` (do_sample=False) / `beam_sample` (do_sample=True) with `BeamSearchScorer.process / finalize`,
    as `model.generate(num_beams=...)` reaches them from musicnlp/trainer/eval.py:302-333.  `dec` is an XLDecoder or an
    rf_generate.RFDecoder (anything with beam_prefill / beam_logp / beam_reorder / beam_advance and `ids`) with one row per beam:
    B * num_beams rows (times num_return_sequences for beam_sample, as HF expands its scorer batch, keeping one hypothesis of
    each).  `_beam_loop` with one group: the 2 * num_beams best (or sampled) continuations per item, then the walk on the host.
    Returns (B * num_return_sequences, L) ids, padded with pad_token_id (= eos when the config has none, as HF does).
    allowed: None, or a callable (ids[:, :cur_len]) -> (rows, V) bool; a token it bars has its log-probability set to -inf before
    the running scores are added, as a logits processor would -- the host reference of the rules under beam_search_device."""
    if num_beams < 2:
        raise MusicXLError('beam search needs num_beams > 1')
    Bs, keep = (prompt.shape[0] * num_return_sequences, 1) if do_sample else (prompt.shape[0], num_return_sequences)

    def sampled(sc):                      # HF beam_sample: warp log p + beam score, renormalise, draw 2 * num_beams, sort
        flat = _warp(sc, top_k, top_p, typical_p, temperature, min_keep=2, renormalize=renormalize_logits).view(Bs, -1)
        pick = torch.multinomial(torch.softmax(flat, -1), 2 * num_beams, generator=generator)
        top_s, order = flat.gather(-1, pick).sort(descending=True, dim=1)
        return top_s, pick.gather(-1, order)
    return _beam_loop(dec, prompt, max_length, num_beams, 1, 0.0, Bs, keep, sampled if do_sample else None, early_stopping, length_penalty,
                      eos_token_id, pad_token_id, return_scores, allowed)


def beam_search_device(dec, prompt: torch.Tensor, max_length: int, num_beams: int = 3, early_stopping: bool = True,
                       length_penalty: float = 1.0, num_return_sequences: int = 1, eos_token_id: int = 0,
                       pad_token_id: Optional[int] = None, use_graph: bool = True, stop_chunk: int = STOP_CHUNK, grammar=None,
                       n_bars=None, in_key=None, key=None, return_scores: bool = False, num_beam_groups: int = 1,
                       diversity_penalty: float = 0.0, register=None, melody_range=None, bass_range=None, bass_below=None,
                       beam_rings: str = 'copied'):
    """`beam_search` (do_sample=False) with the scorer on the device: per step the rules mask, mxl_beam_step (select, walk, store,
    reorder ids and the rule words), mxl_beam_reorder over the K/V rings, the position advance, the rules advance and the model --
    no host read, captured once under use_graph (XLDecoder.beam_begin / beam_step).  The steps are replayed in chunks of
    `stop_chunk`; the number of done items is read back one chunk late (run_until_finished) and the loop
    ends when every item is done or at max_length.  Then the store and the running scores are read once and `_beam_finalize`
    builds the output, as beam_search does.  dec: an XLDecoder with prompt rows x num_beams rows, num_beams <= 16.
    grammar / n_bars / in_key / key / register with melody_range, bass_range and bass_below: the rules as rules_config takes them, one
    value per prompt where they are per row (each prompt's is shared by its beams); a barred token is -inf before the running scores
    are added, the rules' words follow the beams, and a row that can only continue from a barred token is dead: it emits pad at score
    -inf and never returns.  An item that ends with fewer than num_return_sequences hypotheses of finite score raises MusicXLError.
    num_beam_groups > 1 with diversity_penalty: the same loop over mxl_group_beam_step (group_beam_search_device).
    beam_rings: 'copied' or 'indexed', how the rings follow the beams (XLDecoder.beam_begin); the output is the same."""
    V = dec.eng.cfg.vocab_size
    nb = int(num_beams)
    pad = eos_token_id if pad_token_id is None else pad_token_id
    B0, Tp = prompt.shape
    keep = int(num_return_sequences)
    if keep > nb:
        raise MusicXLError('num_return_sequences has to be smaller or equal to num_beams')
    if n_bars is not None and num_beam_groups != 1:
        raise MusicXLError('n_bars= is not supported under group beam search: the bar count is untested under several groups')
    rows = B0 * nb
    if dec.B != rows or max_length > dec.Tmax:
        raise MusicXLError(f'the decoder was built for {dec.B} rows x {dec.Tmax} positions, beam search needs {rows} x {max_length}')
    rules = rules_config(batch=B0, vocab_size=V, stop=(int(eos_token_id), int(pad), 0), grammar=grammar, n_bars=n_bars, in_key=in_key,
                         key=key, register=register, melody_range=melody_range, bass_range=bass_range, bass_below=bass_below, repeat=nb)
    return _beam_device(dec, prompt, max_length, nb, keep, early_stopping, length_penalty, eos_token_id, pad, use_graph, stop_chunk,
                        rules, return_scores, 'beam search', ng=int(num_beam_groups), diversity_penalty=float(diversity_penalty),
                        beam_rings=beam_rings)


def _beam_device(dec, items: torch.Tensor, max_length: int, nb: int, keep: int, early_stopping: bool, length_penalty: float, eos: int,
                 pad: int, use_graph: bool, stop_chunk: int, rules: RulePlan, return_scores: bool, what: str, **arm):
    """The loop of the device beam searches over `items` (Bs, Tp), one prompt per item, nb decoder rows each: `beam_begin` (with
    `rules`, built for the Bs * nb rows, and `arm`: the groups and their penalty, or the sample flag and its warpers, and beam_rings), the chunked
    replay, the last selection, one read of the store and `_beam_finalize` keeping `keep` hypotheses per item."""
    B0, Tp = items.shape
    n = dec.beam_begin(items.repeat_interleave(nb, 0).to(dec.eng.dev), max_length, nb, eos, pad, length_penalty, early_stopping,
                       use_graph, rules, **arm)
    issued, = run_until_finished([(dec, None)], n, stop_chunk)
    dec.beam_select()                   # the last selection needs no forward after it; items that are done ignore it
    dec.steps_run = issued
    cur_len = Tp + issued + 1
    st = dec.beam
    hyp_len, hyp_n, done, hyp_score, final = st.read()
    hyps = []
    for b in range(B0):
        h = _BeamHyps(nb, length_penalty, early_stopping)
        h.beams = [(hyp_score[b][j], st.hyp_ids[b, j, :hyp_len[b][j]]) for j in range(hyp_n[b])]
        h.worst_score = min([sc for sc, _ in h.beams], default=1e9)
        h.done = bool(done[b])
        finite = sum(math.isfinite(sc) for sc, _ in h.beams)
        if not h.done:
            finite += sum(math.isfinite(x) for x in final[b * nb:(b + 1) * nb].tolist())
        if finite < keep:
            raise MusicXLError(f'{what} found {finite} hypotheses for item {b}, fewer than num_return_sequences = {keep}: the '
                               'rules bar every continuation of its other beams')
        hyps.append(h)
    return _beam_finalize(hyps, nb, keep, dec.ids, cur_len, final, max_length, eos, pad, return_scores)


def beam_sample_device(dec, prompt: torch.Tensor, max_length: int, num_beams: int = 3, top_k: Optional[int] = None,
                       top_p: Optional[float] = None, temperature: float = 1.0, typical_p: Optional[float] = None,
                       early_stopping: bool = True, length_penalty: float = 1.0, num_return_sequences: int = 1, eos_token_id: int = 0,
                       pad_token_id: Optional[int] = None, use_graph: bool = True, stop_chunk: int = STOP_CHUNK, grammar=None,
                       in_key=None, key=None, return_scores: bool = False, register=None, melody_range=None, bass_range=None,
                       bass_below=None, beam_rings: str = 'copied'):
    """`beam_search(do_sample=True)` (HF 4.25.1 `beam_sample` with renormalize_logits) with the draw and the scorer on the device:
    `beam_search_device`'s loop -- chunked replay of one captured step, the number of done items read a chunk late, the last selection
    without a forward, `_beam_finalize` -- whose step is the rules mask, mxl_beam_sample_draw (the warpers with two tokens kept, the
    renormalisation and the draw of 2 * num_beams candidates per item without replacement, by Gumbel-top-k from the decoder's seed and
    its draw counter) and mxl_beam_sample_step (the walk, with the warped value as the new running score).  As HF expands its scorer
    batch, an item is one of prompts x num_return_sequences and keeps one hypothesis.  dec: an XLDecoder with prompts x
    num_return_sequences x num_beams rows, 2 <= num_beams <= 16, a vocabulary of at most 2048 tokens.  grammar / in_key / key as in
    `beam_search_device`, each prompt's value shared by its items and beams (no n_bars: the exact-bar-count promise is untested under
    a sampled search).  The draw is another random stream than torch.multinomial's: a seed gives other ids than the host path's.
    An item that ends with no hypothesis of finite score raises MusicXLError."""
    V = dec.eng.cfg.vocab_size
    nb, nrs = int(num_beams), int(num_return_sequences)
    pad = eos_token_id if pad_token_id is None else pad_token_id
    B0 = prompt.shape[0]
    rows = B0 * nrs * nb
    if V > 2048:
        raise MusicXLError(f'beam-sample on the device sorts a row in LDS: a vocabulary of {V} tokens is beyond its 2048')
    if nb < 2 or nb > BEAM_MAX:
        raise MusicXLError(f'beam-sample on the device takes 2..{BEAM_MAX} beams, not {nb}')
    if nrs < 1 or dec.B != rows or max_length > dec.Tmax:
        raise MusicXLError(f'the decoder was built for {dec.B} rows x {dec.Tmax} positions, beam-sample needs {rows} x {max_length}')
    rules = rules_config(batch=B0, vocab_size=V, grammar=grammar, in_key=in_key, key=key, register=register, melody_range=melody_range,
                         bass_range=bass_range, bass_below=bass_below, repeat=nrs * nb)
    return _beam_device(dec, prompt.repeat_interleave(nrs, 0), max_length, nb, 1, early_stopping, length_penalty, eos_token_id, pad,
                        use_graph, stop_chunk, rules, return_scores, 'beam-sample', sample=True, top_k=top_k, top_p=top_p,
                        temperature=temperature, typical_p=typical_p, beam_rings=beam_rings)


def group_beam_search(dec, prompt: torch.Tensor, max_length: int, num_beams: int = 4, num_beam_groups: int = 2,
                      diversity_penalty: float = 0.0, early_stopping: bool = True, length_penalty: float = 1.0,
                      num_return_sequences: int = 1, eos_token_id: int = 0, pad_token_id: Optional[int] = None,
                      return_scores: bool = False, allowed=None):
    """HF 4.25.1 `group_beam_search` (diverse beam search, Vijayakumar et al.) with `BeamSearchScorer(num_beam_groups=...)` and
    `HammingDiversityLogitsProcessor`, as `model.generate(num_beams=, num_beam_groups=, diversity_penalty=)` reaches them from
    the reference's 'beam' strategy (musicnlp/trainer/eval.py:303-317: num_beam_groups set => do_sample False): `_beam_loop` with
    num_beam_groups groups and the Hamming term between them.
    allowed: as in `beam_search`, the host reference of the rules under group_beam_search_device: a token it bars is -inf before the
    Hamming term and the running score are added, and a row that continues at -inf does not count in the Hamming frequency."""
    if num_beam_groups < 2 or num_beams % num_beam_groups != 0:
        raise ValueError('`num_beams` should be divisible by `num_beam_groups` for group beam search.')      # HF's message
    return _beam_loop(dec, prompt, max_length, num_beams, num_beam_groups, float(diversity_penalty or 0.0), prompt.shape[0],
                      num_return_sequences, None, early_stopping, length_penalty, eos_token_id, pad_token_id, return_scores, allowed)


def group_beam_search_device(dec, prompt: torch.Tensor, max_length: int, num_beams: int = 4, num_beam_groups: int = 2,
                             diversity_penalty: float = 0.0, early_stopping: bool = True, length_penalty: float = 1.0,
                             num_return_sequences: int = 1, eos_token_id: int = 0, pad_token_id: Optional[int] = None,
                             use_graph: bool = True, stop_chunk: int = STOP_CHUNK, grammar=None, in_key=None, key=None,
                             return_scores: bool = False, register=None, melody_range=None, bass_range=None, bass_below=None,
                             beam_rings: str = 'copied'):
    """`group_beam_search` with the scorer on the device: `beam_search_device`'s loop -- chunked replay of one captured step, the
    number of done items read a chunk late, the last selection without a forward, `_beam_finalize` -- over mxl_group_beam_step, which
    walks the groups of every item in order inside one launch.  dec: an XLDecoder with prompt rows x num_beams rows, num_beams <= 16
    in num_beam_groups >= 2 groups, 0 <= diversity_penalty < inf (MusicXLError otherwise).  grammar / in_key / key as there (no n_bars: the exact-bar-count promise is untested under a
    search with several groups); `group_beam_search(..., allowed=)` is the host reference."""
    nb, ng = int(num_beams), int(num_beam_groups)
    if ng < 2 or nb % ng != 0:
        raise ValueError('`num_beams` should be divisible by `num_beam_groups` for group beam search.')      # HF's message
    return beam_search_device(dec, prompt, max_length, num_beams=nb, early_stopping=early_stopping, length_penalty=length_penalty,
                              num_return_sequences=num_return_sequences, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                              use_graph=use_graph, stop_chunk=stop_chunk, grammar=grammar, in_key=in_key, key=key,
                              return_scores=return_scores, num_beam_groups=ng, diversity_penalty=float(diversity_penalty or 0.0),
                              register=register, melody_range=melody_range, bass_range=bass_range, bass_below=bass_below,
                              beam_rings=beam_rings)


def beam_generate(make_decoder, input_ids: torch.Tensor, max_length: int, *, num_beams: int, num_beam_groups: int, do_sample: bool,
                  num_return_sequences: int, eos_token_id: int, pad_token_id: Optional[int], seed: int, top_k=None, top_p=None,
                  temperature=1.0, typical_p=None, early_stopping=None, renormalize_logits=None, length_penalty: float = 1.0,
                  diversity_penalty=None) -> torch.Tensor:
    """The beam arms of both models' `generate`: group beam search when num_beam_groups != 1, else beam search / beam sample.
    make_decoder(rows) builds the model's decoder with one row per beam; eos / pad are what the model resolved from the arguments
    and its config.  beam_sample draws from a generator seeded with `seed`."""
    common = dict(num_beams=num_beams, early_stopping=bool(early_stopping), length_penalty=length_penalty,
                  num_return_sequences=num_return_sequences, eos_token_id=eos_token_id, pad_token_id=pad_token_id)
    if num_beam_groups != 1:
        if num_beams <= 1 or num_beam_groups > num_beams:
            raise ValueError('`num_beam_groups` has to be smaller or equal to `num_beams`')               # HF's message
        if do_sample:
            raise ValueError('Diverse beam search cannot be used in sampling mode. Make sure that `do_sample` is set to `False`.')
        return group_beam_search(make_decoder(input_ids.shape[0] * num_beams), input_ids, max_length, num_beam_groups=num_beam_groups,
                                 diversity_penalty=diversity_penalty or 0.0, **common)
    dec = make_decoder(input_ids.shape[0] * num_beams * (num_return_sequences if do_sample else 1))
    gen = torch.Generator(device=dec.eng.dev).manual_seed(seed) if do_sample else None
    return beam_search(dec, input_ids, max_length, do_sample=do_sample, top_k=top_k, top_p=top_p, temperature=temperature,
                       typical_p=typical_p, renormalize_logits=bool(renormalize_logits), generator=gen, **common)


def contrastive_search(dec, prompt: torch.Tensor, max_length: int, top_k: int = 4, penalty_alpha: float = 0.6,
                       eos_token_id: Optional[int] = 0, pad_token_id: Optional[int] = None, allowed=None,
                       trace: Optional[list] = None) -> torch.Tensor:
    """HF 4.25.1 `GenerationMixin.contrastive_search` over Transformer-XL mems -- the reference's 'contrastive' strategy
    (musicnlp/trainer/eval.py:296-302); the reference's `prepare_inputs_for_generation` re-stacks the per-row mems lists that
    routine builds ("to work with cosine sim generation", musicnlp/models/transformer_xl.py:229-234).  One decoder row per
    (sequence, candidate): the K = top_k rows of a sequence share its history.  Per step: (1) the top-k tokens of the current
    log-probabilities and their probabilities renormalised over those k (TopKLogitsWarper, then softmax); (2) all B * K
    candidates through one cached decode step; (3) mxl_contrastive_select scores each candidate (1 - alpha) * p - alpha * max
    cosine similarity between its last-layer hidden state and those of every earlier position, and picks the best; (4) the K
    rows of the sequence take over the picked candidate's rings and history, its log-probabilities open the next step.
    This is the host-driven reference of contrastive_search_device.  allowed: None, or a callable (ids[:, :cur_len]) -> (rows, V)
    bool, as beam_search takes it; a token it bars is -inf before the top-k, where HF's logits processors sit, and a candidate at
    -inf is dead: it scores -inf and is never picked.  trace: a list that receives, per step, (live (B0,) bool, the gap between the
    two best contrastive scores (B0,), the gap between the K-th and the (K+1)-th log-probability (B0,)) -- what decides whether
    another implementation may be held to the same tokens."""
    e, c = dec.eng, dec.eng.cfg
    dev, d, L = e.dev, c.d_model, c.n_layer
    K = int(top_k)
    if K < 2 or not penalty_alpha or penalty_alpha <= 0:
        raise ValueError('contrastive search needs top_k > 1 and penalty_alpha > 0')
    B0, Tp = prompt.shape
    rows = B0 * K
    if dec.B != rows or max_length > dec.Tmax:
        raise MusicXLError(f'the decoder was built for {dec.B} rows x {dec.Tmax} positions, contrastive search needs {rows} x {max_length}')
    pad = eos_token_id if pad_token_id is None else pad_token_id
    dec.beam_prefill(prompt.repeat_interleave(K, 0).to(dev))
    ws = e._last
    hid0 = (ws.h[L & 1]).view(rows, Tp, d)[::K]                          # last-layer output of every prompt position
    ctx = torch.empty(B0, max_length, d, device=dev, dtype=torch.bfloat16)
    inv = torch.empty(B0, max_length, device=dev, dtype=torch.float32)
    ctx[:, :Tp].copy_(hid0)
    for b in range(B0):
        ops.row_inv_norm(ctx[b, :Tp], inv[b, :Tp], Tp)
    logp = dec.beam_logp()[::K].clone()                                  # (B0, V)
    score = torch.empty(rows, device=dev, dtype=torch.float32)
    sel = torch.empty(B0, device=dev, dtype=torch.int64)
    norm = torch.empty(B0, device=dev, dtype=torch.float32)
    grp = torch.arange(B0, device=dev) * K
    unfinished = torch.ones(B0, dtype=torch.bool, device=dev)
    cur_len = Tp
    while cur_len < max_length:
        if allowed is not None:
            ok = torch.as_tensor(allowed(dec.ids[:, :cur_len]))[::K].to(dev, torch.bool)
            logp = logp.masked_fill(~ok, float('-inf'))
        top_lp, top_ids = logp.topk(K, dim=-1)
        probs = torch.softmax(top_lp.float(), dim=-1).contiguous()
        dec.ids[:, cur_len] = top_ids.reshape(-1)
        dec.beam_advance(cur_len + 1)                                    # every candidate at position cur_len
        hid = dec.h[L & 1]
        ops.contrastive_select(ctx, inv, cur_len, hid, probs, penalty_alpha, score, sel)
        if allowed is not None:                                          # dead candidates score -inf; the first maximum again
            sc = score.view(B0, K).masked_fill(top_lp == float('-inf'), float('-inf'))
            best = sc == sc.max(1, keepdim=True).values
            # (a finished sequence whose rows the mask bars whole scores NaN everywhere: it emits pad, any candidate will do)
            sel = torch.where(best, torch.arange(K, device=dev)[None, :], K - 1).min(1).values
        if trace is not None:
            two = (sc if allowed is not None else score.view(B0, K)).topk(2, dim=1).values
            edge = logp.topk(K + 1, dim=-1).values
            trace.append((unfinished.clone(), two[:, 0] - two[:, 1], edge[:, K - 1] - edge[:, K]))
        src = grp + sel
        if eos_token_id is not None:                                     # finished sequences emit pad from now on
            tok = dec.ids[src, cur_len]
            tok = torch.where(unfinished, tok, torch.full_like(tok, pad))
        dec.beam_reorder(src.repeat_interleave(K))
        if eos_token_id is not None:
            dec.ids[:, cur_len] = tok.repeat_interleave(K)
            unfinished = unfinished & (tok != eos_token_id)
        ctx[:, cur_len].copy_(hid.index_select(0, src))
        inv[:, cur_len] = ops.row_inv_norm(ctx[:, cur_len], norm, B0)     # (the kernel writes a contiguous (B0,) vector)
        logp = dec.beam_logp().index_select(0, src)
        cur_len += 1
        if eos_token_id is not None and not bool(unfinished.any()):
            break
    return dec.ids[::K, :cur_len].clone()


def contrastive_search_device(dec, prompt: torch.Tensor, max_length: int, top_k: int = 4, penalty_alpha: float = 0.6,
                              eos_token_id: Optional[int] = 0, pad_token_id: Optional[int] = None, use_graph: bool = True,
                              stop_chunk: int = STOP_CHUNK, grammar=None, in_key=None, key=None, register=None, melody_range=None,
                              bass_range=None, bass_below=None, contrastive_rings: Optional[str] = None) -> torch.Tensor:
    """`contrastive_search` with the whole step on the device: per step the rules mask, mxl_contrastive_topk, the position advance,
    the model, mxl_contrastive_step, the rules advance and mxl_ring_slot_broadcast -- no host read, no whole-ring copy, captured once
    under use_graph (XLDecoder.contrastive_begin / contrastive_step).  The steps are replayed in chunks of `stop_chunk`; the number
    of finished sequences is read back one chunk late (run_until_finished) and the loop ends when every
    sequence has finished or at max_length.  Returns what the host path returns: ids[::K] cut at the step in which the last sequence
    finished, else at max_length; the steps run beyond it inside the last chunk emit pad and are cut off.  dec: an XLDecoder with
    prompt rows x top_k rows, 2 <= top_k <= 32.  grammar (with or without a bar budget) / in_key / key / register: the rules as
    rules_config takes them, one value per prompt where they are per row (each prompt's is shared by its K rows); a barred token is -inf
    before the top-k, and a candidate that is barred is never picked.
    contrastive_rings: None (what the decoder was built for), 'copied' or 'shared' -- it must name the decoder's mode: 'shared' takes
    an XLDecoder(shared_rings=top_k), whose B0 rings serve the K candidates of their prompt (mxl_kv_stash /
    mxl_relattn_decode_shared / mxl_kv_commit_shared in place of the ring append, the attention and the broadcast); the ids are the
    ones 'copied' returns wherever both decoders cut their rings into the same number of pieces (XLDecoder.pieces)."""
    V = dec.eng.cfg.vocab_size
    K = int(top_k)
    if K < 2 or not penalty_alpha or penalty_alpha <= 0:
        raise ValueError('contrastive search needs top_k > 1 and penalty_alpha > 0')
    if contrastive_rings is not None:
        if contrastive_rings not in CONTRASTIVE_RINGS:
            raise ValueError(f"contrastive_rings={contrastive_rings!r}: expected None, 'copied' or 'shared'")
        if (contrastive_rings == 'shared') != bool(getattr(dec, 'shared_K', 0)):
            raise ValueError(f"contrastive_rings='{contrastive_rings}' on a decoder built for the other ring mode "
                             '(XLDecoder(shared_rings=top_k) is the shared one)')
    B0, Tp = prompt.shape
    rows = B0 * K
    if dec.B != rows or max_length > dec.Tmax:
        raise MusicXLError(f'the decoder was built for {dec.B} rows x {dec.Tmax} positions, contrastive search needs {rows} x {max_length}')
    if max_length <= Tp:
        return prompt.to(dec.eng.dev).clone()
    pad = eos_token_id if pad_token_id is None else pad_token_id
    rules = rules_config(batch=B0, vocab_size=V, grammar=grammar, in_key=in_key, key=key, register=register, melody_range=melody_range,
                         bass_range=bass_range, bass_below=bass_below, repeat=K)
    n = dec.contrastive_begin(prompt.repeat_interleave(K, 0).to(dec.eng.dev), max_length, K, penalty_alpha, eos_token_id,
                              0 if pad is None else pad, use_graph, rules)
    # (the count is first read once the first token is chosen: sequences that all start with eos replay nothing)
    issued, = run_until_finished([(dec, None)], n, stop_chunk)
    dec.steps_run = issued
    width = stop_width(dec.ids[::K], dec.unfinished[::K], Tp, max_length, dec.rules.stop[0])
    return dec.ids[::K, :width].clone()


def _warp(scores: torch.Tensor, top_k, top_p, typical_p, temperature, min_keep: int, renormalize: bool = True) -> torch.Tensor:
    """HF 4.25.1 logits warpers in `_get_logits_warper` order (temperature, top-k, top-p, typical-p, then
    LogitNormalization when renormalize_logits is set -- the reference sets it for every sampling call, eval.py:323) on a
    (rows, V) score matrix; min_tokens_to_keep = 2 under beam search.  Used by beam_sample only -- plain sampling runs in the
    sampler kernel.  HF applies the warpers AFTER adding the running beam scores, so with LogitNormalization every beam's row is
    renormalised to log-sum-exp 0 each step and the running score drops out of the draw; that is the reference's behaviour and
    it is kept."""
    neg = float('-inf')
    if temperature is not None and temperature != 1.0:
        scores = scores / temperature
    if top_k:
        k = min(max(top_k, min_keep), scores.shape[-1])
        scores = scores.masked_fill(scores < scores.topk(k, -1).values[..., -1:], neg)
    if top_p is not None and top_p < 1.0:
        srt, idx = scores.sort(descending=False, dim=-1)
        remove = srt.softmax(-1).cumsum(-1) <= (1 - top_p)
        remove[..., -min_keep:] = False
        scores = scores.masked_fill(remove.scatter(-1, idx, remove), neg)
    if typical_p is not None and typical_p < 1.0:
        logp = scores.log_softmax(-1)
        p = logp.exp()
        ent = -(torch.nan_to_num(logp * p, nan=0.0)).sum(-1, keepdim=True)
        shifted = ((-logp) - ent).abs()
        srt, idx = shifted.sort(descending=False, dim=-1)
        cum = scores.gather(-1, idx).softmax(-1).cumsum(-1)
        last = (cum < typical_p).sum(-1)
        last[last < 0] = 0
        remove = srt > srt.gather(-1, last.view(-1, 1).clamp(max=scores.shape[-1] - 1))
        if min_keep > 1:
            remove[..., :min_keep] = False
        scores = scores.masked_fill(remove.scatter(-1, idx, remove), neg)
    return scores.log_softmax(-1) if renormalize else scores


# -------------------------------------------------------------------- bar-aligned cuts around generation
def truncate_last_bar(ids: torch.Tensor, sob_token_id: int):
    """`MusicGenerator._truncate_last_bar` (musicnlp/trainer/eval.py:178-185) for a batch: every generated row cut just before
    its last start-of-bar token, so a bar broken off by `max_length` is not rendered.  ids: (T,) or (B, T) int64 on the GPU;
    returns a list of ints (1-D input, as the reference) or a list of such lists.  Like the reference it refuses a row with no
    start-of-bar token."""
    one = ids.dim() == 1
    x = ids.view(1, -1) if one else ids
    x = x.contiguous()
    cut = ops.find_token(x, sob_token_id, -1).tolist()
    if min(cut) < 0:
        raise MusicXLError('no start-of-bar token found in a sequence to truncate')
    host = x.cpu()
    rows = [host[b, :c].tolist() for b, c in enumerate(cut)]
    return rows[0] if one else rows


def truncate_first_n_bar(ids: torch.Tensor, sob_token_id: int, n_bar: int = 8) -> torch.Tensor:
    """`MusicGenerator.truncate_first_n_bar` (eval.py:187-198) on ids: the prefix of one song up to (not including) its
    start-of-bar number `n_bar` (0-based, i.e. the song header plus the first `n_bar` bars), with a start-of-bar appended as the
    prompt for generation.  ids: (T,) int64 on the GPU; returns a (n,) int64 device tensor."""
    assert ids.dim() == 1
    cut = int(ops.find_token(ids.view(1, -1).contiguous(), sob_token_id, n_bar).item())
    if cut < 0:
        raise MusicXLError(f'the sequence has fewer than {n_bar + 1} bars')     # the reference raises IndexError here
    return torch.cat([ids[:cut], ids.new_tensor([sob_token_id])])


# -------------------------------------------------------------------- left-padded batches of prompts of different lengths
def left_pad(prompts, pad_token_id: int):
    """Prompts of different lengths (a list of 1-D id tensors, e.g. `truncate_first_n_bar` outputs) -> (input_ids, attention_mask),
    both (B, Tp) int64 with Tp the longest prompt: row b holds Tp - len(prompts[b]) columns of pad_token_id on the left, then the
    prompt; the mask is 0 on the pads and 1 on the prompt (the HF decoder-only layout `model.generate(attention_mask=...)` takes)."""
    if not len(prompts):
        raise MusicXLError('left_pad needs at least one prompt')
    if any(p.dim() != 1 or p.numel() == 0 for p in prompts):
        raise MusicXLError('left_pad takes non-empty 1-D id tensors')
    Tp = max(p.numel() for p in prompts)
    dev = prompts[0].device
    ids = torch.full((len(prompts), Tp), int(pad_token_id), dtype=torch.int64, device=dev)
    mask = torch.zeros(len(prompts), Tp, dtype=torch.int64, device=dev)
    for b, p in enumerate(prompts):
        ids[b, Tp - p.numel():] = p.to(dev, torch.int64)
        mask[b, Tp - p.numel():] = 1
    return ids, mask


def strip_left_pad(ids: torch.Tensor, attention_mask: torch.Tensor):
    """Inverse of `left_pad` on a generated batch: (B, L) ids and the (B, Tp) prompt mask -> list of B 1-D tensors, row b without
    its left pad columns (prompt + continuation, e.g. for `truncate_last_bar` per row)"""
    n_pad = left_pad_counts(attention_mask, (ids.shape[0], attention_mask.shape[1]))
    return [ids[b, s:] for b, s in enumerate(n_pad)]


def left_pad_counts(attention_mask: torch.Tensor, shape) -> list:
    """Checks a (B, Tp) attention mask on the host and returns the number of left pad columns of every row.  The mask must hold
    0 / 1 only, and every row must be zeros then ones (left padding) with at least one 1: the prompt's last token is the column
    generation continues from."""
    B, Tp = shape
    m = torch.as_tensor(attention_mask).detach().cpu()
    if tuple(m.shape) != (B, Tp):
        raise MusicXLError(f'attention_mask has shape {tuple(m.shape)}, input_ids {(B, Tp)}')
    if m.dtype == torch.bool:
        m = m.to(torch.int64)
    if not bool(((m == 0) | (m == 1)).all()):
        raise MusicXLError('attention_mask must hold only 0 (pad) and 1 (token)')
    m = m.to(torch.int64)
    if not bool(m[:, -1].all()):
        if bool((m.sum(1) == 0).any()):
            raise MusicXLError('attention_mask has a row without any token')
        raise MusicXLError('right-padding was detected in attention_mask: this decoder-only model generates from left-padded '
                           "prompts only (padding_side='left'; generate.left_pad)")
    if bool((m[:, 1:] < m[:, :-1]).any()):
        raise MusicXLError('attention_mask rows must be zeros (left padding) then ones; a pad column inside a prompt is not supported')
    return (Tp - m.sum(1)).tolist()
