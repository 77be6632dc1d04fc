"""Thin torch-tensor front-ends over the C ABI (include/musicxl.h).

torch is used only for device memory and the current HIP stream; every function here enqueues hand-written HIP kernels
from libmusicxl.so and raises if the library is missing or a launch fails.  No CPU / eager fallbacks.
"""
import ctypes as C
import math
import os
from typing import Any, NamedTuple, Optional, Sequence

import torch

from ._lib import lib, check, struct, MusicXLError

GEMM_OUT_F32 = 0x01
GEMM_OUT_F32_ATOMIC = 0x02
GEMM_BIAS = 0x04
GEMM_RELU = 0x08
GEMM_DROPOUT = 0x10
GEMM_RELU_BWD = 0x20
GEMM_ADD_AUX = 0x40
GEMM_SAVE_RELU_MASK = 0x100
GEMM_RELU_BWD_BITS = 0x200


def mix_seed(base_seed: int, step: int) -> int:
    """Dropout / LSH-rotation seed of one step: a 63-bit mix of (base seed, data-parallel rank, step).  Under data parallelism
    every rank draws its own masks (as DDP ranks do in the reference stack) while the weight-initialisation seed stays
    common; no collisions between runs once `step` passes 2^20 (the former `(seed << 20) + step`)."""
    import torch.distributed as dist
    rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
    x = (base_seed * 0x9E3779B97F4A7C15 + rank * 0xD1B54A32D192ED03 + step * 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 32
    x = (x * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 32
    return x & 0x7FFFFFFFFFFFFFFF


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise MusicXLError(f'{name}: expected a device tensor (the HIP path has no CPU fallback)')
    if t.dtype != dtype:
        raise MusicXLError(f'{name}: expected {dtype}, got {t.dtype}')


def _cut(cutoffs: Sequence[int]):
    n = len(cutoffs)
    arr = (C.c_int * max(n, 1))(*cutoffs) if n else None
    return n, arr


KT_NAMES = ('fwd', 'delta', 'dq8', 'dkv', 'drd', 'rowbias', 'fused', 'dqfin', 'chunk_fwd', 'chunk_bwd_q', 'chunk_bwd_kv')   # MXL_KT_* ids of include/musicxl.h


def ktime_enable(on: bool):
    """per-kernel hipEvent brackets inside the attention launch functions (bench.py's roofline); off while capturing graphs"""
    check(lib().mxl_ktime_enable(int(bool(on))), 'mxl_ktime_enable')


def ktime_collect():
    """{kernel: (milliseconds summed, launches)} since the last collect; synchronises the recorded events"""
    n = len(KT_NAMES)
    ms, cnt = (C.c_float * n)(), (C.c_int * n)()
    check(lib().mxl_ktime_collect(C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), n), 'mxl_ktime_collect')
    return {KT_NAMES[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}


def gemm(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, M: int, N: int, K: int, *, trans_a=False, trans_b=False,
         flags=0, alpha=1.0, bias: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None, ksplits=1,
         lda=None, ldb=None, ldc=None, ldaux=None, drop_p=0.0, seed=0, site=0, colsum: Optional[torch.Tensor] = None):
    """C[M,N] (+)= alpha * op(A) op(B); see mxl_gemm_bf16.  Leading dimensions default to the last-dim stride.
    `colsum` (N,) f32: += the column sums of C in the same call (mxl_gemm_bf16_colsum; bf16 output, ksplits == 1)."""
    _req(a, torch.bfloat16, 'A'); _req(b, torch.bfloat16, 'B')
    lda = lda if lda is not None else a.stride(-2)
    ldb = ldb if ldb is not None else b.stride(-2)
    ldc = ldc if ldc is not None else c.stride(-2)
    if aux is not None and ldaux is None:
        ldaux = 0 if flags & (GEMM_SAVE_RELU_MASK | GEMM_RELU_BWD_BITS) else aux.stride(-2)
    if colsum is not None:
        assert ksplits == 1
        check(lib().mxl_gemm_bf16_colsum(_p(a), _p(b), _p(c), M, N, K, lda, ldb, ldc, int(trans_a), int(trans_b), flags,
                                         float(alpha), _p(bias), _p(aux), ldaux or 0, float(drop_p), seed, site, _p(colsum),
                                         _stream()), 'mxl_gemm_bf16_colsum')
        return c
    check(lib().mxl_gemm_bf16(_p(a), _p(b), _p(c), M, N, K, lda, ldb, ldc, int(trans_a), int(trans_b), flags,
                              float(alpha), _p(bias), _p(aux), ldaux or 0, ksplits, float(drop_p), seed, site,
                              _stream()), 'mxl_gemm_bf16')
    return c


def gemm_relu_mask_bytes(M: int, N: int) -> int:
    """bytes of the relu-mask bit buffer GEMM_SAVE_RELU_MASK / GEMM_RELU_BWD_BITS use for an (M, N) output; 0 = not available at
    these sizes (use GEMM_RELU_BWD with the activations)"""
    if os.environ.get('MXL_NO_RELU_BITS') == '1':
        return 0
    return int(lib().mxl_gemm_relu_mask_bytes(int(M), int(N)))


def gemm_skinny(a, w, c, M, N, K, *, flags=0, bias=None, lda=None, ldw=None, ldc=None):
    """C[M<=64, N] = A W^T (+bias)(relu): weight-streaming form used by the decode step"""
    check(lib().mxl_gemm_skinny_bf16(_p(a), _p(w), _p(c), M, N, K, lda if lda is not None else a.stride(-2),
                                     ldw if ldw is not None else w.stride(-2), ldc if ldc is not None else c.stride(-2),
                                     flags, _p(bias), _stream()), 'mxl_gemm_skinny_bf16')
    return c


def gemm_skinny_partial(a, w, slabs, M, N, K, KS):
    """K-sliced skinny product: slabs (KS, 64, N) f32 receive the partial sums (finish with ln_residual_fwd_partial)"""
    check(lib().mxl_gemm_skinny_partial(_p(a), _p(w), _p(slabs), M, N, K, a.stride(-2), w.stride(-2), KS, _stream()),
          'mxl_gemm_skinny_partial')


def ln_residual_fwd_partial(slabs, KS, bias, res, gamma, beta, y, eps=1e-5):
    """y = LayerNorm(res + bf16(sum of the KS slabs + bias)); slabs (KS, 64, d) f32, res / y (N <= 64, d) bf16"""
    N, d = res.shape
    check(lib().mxl_ln_residual_fwd_partial(_p(slabs), KS, slabs.stride(0), _p(bias), _p(res), _p(gamma), _p(beta), _p(y), N, d,
                                            float(eps), _stream()), 'mxl_ln_residual_fwd_partial')
    return y


def decode_qkv(x, wqkv, qkv, kc, vc, t_dev, rrb, qr_out, dh):
    """one decode step's qkv projection + K/V ring append + (q + r_r_bias), fused (batch <= 64)"""
    B, d = x.shape
    check(lib().mxl_decode_qkv(_p(x), _p(wqkv), _p(qkv), _p(kc), _p(vc), _p(t_dev), _p(rrb), _p(qr_out), B, d, dh, kc.shape[-2],
                               _stream()), 'mxl_decode_qkv')


_T = Optional[torch.Tensor]
_REPEAT_STATE = ('plan', 'nplan', 'barcol', 'gbars', 'gcopy', 'gstop')          # the tensors of RuleState's repeat group


class RuleState(NamedTuple):
    """The rules of one generation and their per-row state on the device, as the sampler launches take them (sample_step, rules_mask,
    rules_advance; on the device the mxl_rules of include/musicxl.h, "Rules of a generation").  Eight groups; each has a rule the
    decoder names and state tensors, (B,) int32 unless said otherwise, and a launch applies a group exactly when its state is given:
      stop      stop = (eos_id, pad_id, min_length), with unfinished (1 = live) and alive (1,) int32, the live-row count
      grammar   grammar (a grammar.TokenGrammar), with gstate: barred tokens masked and gstate advanced, with or without the eos rule
      budget    the grammar's bar budget (grammar.budget), with gbar and grem, the bar's length and its free slots
      count     the grammar's bar count (grammar.bar_count), with gleft, the bars a row may still open (< 0 = no limit)
      key       in_key (a grammar.KeyRule), with gkey, the row's key (< 0 = none): pitches outside it barred, with or without a grammar
      guide     melody (a grammar.MelodyGuide, `grammar.guide`), with guide (B, ld) int32, glen, gpos and gforce: rows fed from their guides
      register  register (a grammar.RegisterRule) and the scalar gap, with grange, gpart and gfloor: the open part's pitches kept in bounds
      repeat    repeat (a grammar.BarRepeat, `grammar.repeat`) and the scalar span, with plan and barcol (B, ld) int32, nplan, gbars,
                gcopy and gstop: planned bars repeat earlier bars of the row's own ids
    A decoder says which rules hold with stop, grammar, gleft, in_key, melody, register and repeat and may carry state of rules that
    are off (`in_force` drops it); `struct` turns a group on by its state tensor -- unfinished, gstate, gbar, gleft, gkey, gpos, gpart,
    gcopy.  The three entries also take these fields as flat keywords, in this order, in place of the object.  It is a tuple: the
    order of the fields is part of the contract (`struct` unpacks them by position), and it is compared with `is`, never with ==."""
    stop: Optional[tuple] = None; unfinished: _T = None; alive: _T = None
    grammar: Any = None; gstate: _T = None
    gbar: _T = None; grem: _T = None
    gleft: _T = None
    in_key: Any = None; gkey: _T = None
    melody: Any = None; guide: _T = None; glen: _T = None; gpos: _T = None; gforce: _T = None
    register: Any = None; grange: _T = None; gpart: _T = None; gfloor: _T = None; gap: int = -1
    repeat: Any = None; plan: _T = None; nplan: _T = None; barcol: _T = None; span: int = 0
    gbars: _T = None; gcopy: _T = None; gstop: _T = None

    def in_force(self) -> 'RuleState':
        """these rules with every group that is off back at its defaults; a rule on without its state, or beside one it excludes, raises"""
        s = self
        budget = s.grammar is not None and s.grammar.budget is not None
        if s.repeat is not None:
            if s.grammar is None or s.gleft is None or s.stop is None or s.melody is not None:
                raise MusicXLError('the repeat rule rides on a grammar, needs the bar count (gleft) and the eos rule, and excludes the guide')
            if any(getattr(s, k) is None for k in _REPEAT_STATE):
                raise MusicXLError('the repeat rule needs plan, nplan, barcol, gbars, gcopy and gstop')
        if s.stop is not None and (s.unfinished is None or s.alive is None):
            raise MusicXLError('the eos rule needs unfinished and alive')
        if s.grammar is None and s.gleft is not None:
            raise MusicXLError('the bar count rides on a grammar')
        if s.grammar is not None and s.gstate is None:
            raise MusicXLError('a grammar needs gstate')
        if budget and (s.gbar is None or s.grem is None):
            raise MusicXLError('a grammar with a bar budget needs gbar and grem')
        if s.in_key is not None and s.gkey is None:
            raise MusicXLError('the key rule needs gkey')
        if s.melody is not None and (s.grammar is None or s.guide is None or s.glen is None or s.gpos is None or s.gforce is None):
            raise MusicXLError('the guide rides on a grammar and needs guide, glen, gpos and gforce')
        if s.register is not None and (s.grange is None or s.gpart is None or s.gfloor is None):
            raise MusicXLError('the register rule needs grange, gpart and gfloor')
        groups = ((s.stop is not None, ('unfinished', 'alive')), (s.grammar is not None, ('gstate',)),
                  (budget, ('gbar', 'grem')), (s.in_key is not None, ('gkey',)),            # (the count's one tensor, gleft, is its own switch)
                  (s.melody is not None, ('guide', 'glen', 'gpos', 'gforce')),
                  (s.register is not None, ('grange', 'gpart', 'gfloor', 'gap')),
                  (s.repeat is not None, _REPEAT_STATE + ('span',)))
        off = [k for on, names in groups if not on for k in names]
        return s._replace(**{k: s._field_defaults[k] for k in off})

    @property
    def moves_words(self) -> bool:
        """a rule that keeps words of its own is on (the stop rule alone needs no mask and no advance launch of a search)"""
        return self.grammar is not None or self.in_key is not None or self.register is not None

    @property
    def vocab_size(self) -> int:
        """what the rules in force span, which must agree on it (0: no rule with a vocabulary is on)"""
        s = self
        if s.grammar is not None and s.in_key is not None and s.gkey is not None and s.grammar.vocab_size != s.in_key.vocab_size:
            raise MusicXLError(f'the grammar classifies {s.grammar.vocab_size} tokens, the key rule spans {s.in_key.vocab_size}')
        V = s.grammar.vocab_size if s.grammar is not None else (s.in_key.vocab_size if s.gkey is not None else 0)
        if s.gpart is not None:
            if V and s.register.vocab_size != V:
                raise MusicXLError(f'the register rule spans {s.register.vocab_size} tokens, the other rules {V}')
            V = s.register.vocab_size
        return V

    def struct(self, what, device, B, V=None):
        """the mxl_rules of mxl_sample_step / mxl_rules_mask / mxl_rules_advance, checked and filled by field name: a group is on
        exactly when its state tensor is given and takes its tables from `grammar`, `in_key`, `melody`, `register` and `repeat`,
        which must span the V tokens of the scores.  A field that is not set stays zero: its group is off.  (hist / ld_hist, which
        the mask alone reads, are rules_mask's to set.)"""
        (stop, unfinished, alive, grammar, gstate, gbar, grem, gleft, in_key, gkey, melody, guide, glen, gpos, gforce, register, grange,
         gpart, gfloor, gap, repeat, plan, nplan, barcol, span, gbars, gcopy, gstop) = self
        eos, pad, min_length = stop if stop is not None else (-1, 0, 0)
        f = dict(eos_id=int(eos), pad_id=int(pad), min_length=int(min_length or 0))
        # stop, grammar, budget, count
        if unfinished is not None:
            if stop is None:
                raise MusicXLError(f'{what}: unfinished needs stop = (eos, pad, min_length)')
            _req(unfinished, torch.int32, f'{what} unfinished')
        f.update(unfinished=_p(unfinished), alive=_p(alive))
        if gstate is not None or gbar is not None or grem is not None or gleft is not None or gpos is not None or gcopy is not None:
            if grammar is None:
                raise MusicXLError(f'{what}: gstate, gbar / grem, gleft and the guide ride on a grammar')
            if V is not None and grammar.vocab_size != int(V):
                raise MusicXLError(f'the grammar classifies {grammar.vocab_size} tokens, the scores span {int(V)}')
            cls, allow, nxt = grammar.to(device)
            f.update(cls=_p(cls), C=grammar.n_classes)
        if gstate is not None:
            _req(gstate, torch.int32, f'{what} gstate')
            if gstate.numel() != B:
                raise MusicXLError(f'gstate holds {gstate.numel()} rows, the scores {B}')
            f.update(allow=_p(allow), next=_p(nxt), gstate=_p(gstate))
        if gbar is not None or grem is not None:
            bud = grammar.budget
            slots, bars = _budget_state(bud, device, B, gbar, grem, what)
            f.update(slots=_p(slots), bars=_p(bars), opens=bud.opens, need_free=bud.need_free, need_full=bud.need_full, gbar=_p(gbar),
                     grem=_p(grem))
        if gleft is not None:
            cnt = grammar.bar_count
            if cnt is None:
                raise MusicXLError(f'{what}: the grammar carries no bar count (grammar.BarCount; the music grammar has one)')
            _req(gleft, torch.int32, f'{what} gleft')
            if gleft.numel() != B or not gleft.is_contiguous():
                raise MusicXLError(f'{what}: gleft must be contiguous ({B},) int32')
            f.update(count=cnt.count, end=cnt.end, gleft=_p(gleft))
        # repeat: the class masks of `repeat` (over `grammar`), the rows' plans with their lengths nplan, the table barcol the device
        # writes (same row stride as plan), the launch's span and the words
        if gcopy is None:
            if gbars is not None or gstop is not None:
                raise MusicXLError(f'{what}: gbars and gstop need gcopy')
        else:
            if repeat is None or repeat.grammar is not grammar:
                raise MusicXLError(f'{what}: gcopy needs repeat, the repeat rule of the grammar (grammar.repeat)')
            group = [(getattr(self, k), k) for k in _REPEAT_STATE]
            if any(t is None for t, _ in group):
                raise MusicXLError(f'{what}: the repeat group needs plan, nplan, barcol, gbars, gcopy and gstop')
            for t, name in group:
                _req(t, torch.int32, f'{what} {name}')
            for t, name in [g for g in group if g[1] in ('plan', 'barcol')]:    # one width serves both: the row stride, nplan's clamp
                if t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1 or not t.is_contiguous() or t.shape != plan.shape:
                    raise MusicXLError(f'{what}: {name} must be contiguous ({B}, >= 1) int32, plan and barcol of one shape')
            for t, name in [g for g in group if g[1] not in ('plan', 'barcol')]:
                if t.numel() != B or not t.is_contiguous():
                    raise MusicXLError(f'{what}: {name} must be contiguous ({B},) int32')
            if int(span) not in (0, 1):
                raise MusicXLError(f'{what}: span is 0 (the whole bar) or 1 (up to the first `leave` token), got {span}')
            f.update(plan=_p(plan), ld_plan=plan.shape[1], nplan=_p(nplan), barcol=_p(barcol), renter=repeat.enter, rleave=repeat.leave,
                     span=int(span), gbars=_p(gbars), gcopy=_p(gcopy), gstop=_p(gstop))
        # key: the tables of `in_key`
        if gkey is not None:
            if in_key is None:
                raise MusicXLError(f'{what}: gkey needs in_key, the key rule that holds its tables')
            if V is not None and in_key.vocab_size != int(V):
                raise MusicXLError(f'the key rule spans {in_key.vocab_size} tokens, the scores span {int(V)}')
            _req(gkey, torch.int32, f'{what} gkey')
            if gkey.numel() != B or not gkey.is_contiguous():
                raise MusicXLError(f'{what}: gkey must be contiguous ({B},) int32')
            keys, pcs, inkey = in_key.to(device)
            f.update(keys=_p(keys), pcs=_p(pcs), inkey=_p(inkey), gkey=_p(gkey))
        # guide: the class masks of `melody` (over `grammar`), the rows' guide tokens and their lengths glen, and the second word gforce
        if gpos is None:
            if gforce is not None:
                raise MusicXLError(f'{what}: gforce needs gpos')
        else:
            if melody is None or melody.grammar is not grammar:
                raise MusicXLError(f'{what}: gpos needs melody, the guide rule of the grammar (grammar.guide)')
            if guide is None or glen is None or gforce is None:
                raise MusicXLError(f'{what}: the guide group needs guide, glen, gpos and gforce')
            for t, name in ((guide, 'guide'), (glen, 'glen'), (gpos, 'gpos'), (gforce, 'gforce')):
                _req(t, torch.int32, f'{what} {name}')
            if guide.dim() != 2 or guide.shape[0] != B or guide.shape[1] < 1 or guide.stride(1) != 1 or guide.stride(0) < guide.shape[1]:
                raise MusicXLError(f'{what}: guide must be ({B}, >= 1) int32 rows with unit column stride')
            for t, name in ((glen, 'glen'), (gpos, 'gpos'), (gforce, 'gforce')):
                if t.numel() != B or not t.is_contiguous():
                    raise MusicXLError(f'{what}: {name} must be contiguous ({B},) int32')
            # (glen[b] <= the row width is the caller's to keep; the kernels clamp to ld_guide as well)
            f.update(guide=_p(guide), ld_guide=guide.stride(0), glen=_p(glen), enter=melody.enter, leave=melody.leave, gpos=_p(gpos),
                     gforce=_p(gforce))
        # register: the table of `register`, the rows' bounds grange, the second word gfloor, the launch's gap
        if gpart is not None:
            if register is None:
                raise MusicXLError(f'{what}: gpart needs register, the register rule that holds its table')
            if grange is None or gfloor is None:
                raise MusicXLError(f'{what}: the register group needs grange, gpart and gfloor')
            if V is not None and register.vocab_size != int(V):
                raise MusicXLError(f'the register rule spans {register.vocab_size} tokens, the scores span {int(V)}')
            for t, name in ((grange, 'grange'), (gpart, 'gpart'), (gfloor, 'gfloor')):
                _req(t, torch.int32, f'{what} {name}')
                if t.numel() != B or not t.is_contiguous():
                    raise MusicXLError(f'{what}: {name} must be contiguous ({B},) int32')
            if not -1 <= int(gap) <= 127:
                raise MusicXLError(f'{what}: gap must lie in -1..127, got {gap}')
            f.update(reg=_p(register.to(device)), grange=_p(grange), gpart=_p(gpart), gfloor=_p(gfloor), gap=int(gap))
        return struct('mxl_rules')(**f)


def _rule_state(rules: Optional[RuleState], flat: dict) -> RuleState:
    """the `rules` of an entry, or the same object from the flat keywords the entry takes in its place (an unknown one: TypeError)"""
    if rules is None:
        return RuleState(**flat)
    if flat:
        raise TypeError(f'rules= and the flat rule keywords ({", ".join(flat)}) exclude each other')
    return rules


def sample_step(scores, V, ids, t_dev, rng_ctr, seed, E, emb_out, scale, counter, rules: Optional[RuleState] = None, *, do_sample=False,
                top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0, out_probs=None, **flat):
    """sampler + embedding row of the sampled token (-> emb_out (B, d) bf16) + counter advance, one launch (V <= 2048).
    scores (B, >= V) f32: log-probabilities, or raw logits when repetition_penalty == 1.
    The rules of the generation ride on the same launch: `rules` (a RuleState, or its fields as keywords), those in force applied.
    out_probs (B, V) f32, with do_sample: the renormalised distribution the tokens were drawn from (test hook)."""
    B = scores.shape[0]
    rules = _rule_state(rules, flat).in_force().struct('sample_step', scores.device, B, V)
    if out_probs is not None:
        _req(out_probs, torch.float32, 'sample_step out_probs')
        if tuple(out_probs.shape) != (B, int(V)) or not out_probs.is_contiguous():
            raise MusicXLError(f'sample_step: out_probs must be contiguous ({B}, {int(V)}) f32')
    check(lib().mxl_sample_step(_p(scores), scores.stride(0), int(V), _p(ids), ids.stride(0), _p(t_dev), _p(rng_ctr), seed, B,
                                int(do_sample), int(top_k or 0), float(top_p if top_p is not None else 1.0), float(temperature),
                                float(repetition_penalty if repetition_penalty is not None else 1.0),
                                float(typical_p if typical_p is not None else 1.0), _p(E), _p(emb_out), emb_out.shape[1],
                                float(scale), _p(counter), C.byref(rules), _p(out_probs), _stream()), 'mxl_sample_step')


def rules_mask(scores, V, t_dev, rules: Optional[RuleState] = None, *, hist=None, **flat):
    """before sample: scores[b, v] = -inf in place for every token a rule bars (mxl_rules_mask).  `rules` (a RuleState, or its fields
    as keywords) less unfinished / alive, which the mask does not read and the flat form does not take: a group is applied exactly
    when its state is given, a row fed from its guide or copying a bar keeps that one token, and stop = (eos, pad, min_length) bars eos
    while the rows are shorter than min_length.  hist: with the repeat group, the (B, ld) int64 ids of the rows, whose own history a
    row copies from.  No launch when nothing is given."""
    if 'unfinished' in flat or 'alive' in flat:
        raise TypeError('rules_mask takes no unfinished / alive keyword: the stop rule moves in rules_advance')
    rules = _rule_state(rules, flat)._replace(unfinished=None, alive=None)
    _req(scores, torch.float32, 'rules_mask scores')
    B = scores.shape[0]
    if scores.shape[1] < V or scores.stride(1) != 1:
        raise MusicXLError('rules_mask: scores must be (B, >= V) with unit column stride')
    st = rules.struct('rules_mask', scores.device, B, V)
    if rules.gcopy is not None:
        if hist is None or hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] != B or hist.stride(1) != 1:
            raise MusicXLError('rules_mask: the repeat group needs hist, the (B, .) int64 ids of the rows')
        st.hist, st.ld_hist = _p(hist), hist.stride(0)
    check(lib().mxl_rules_mask(_p(scores), scores.stride(0), B, int(V), _p(t_dev), C.byref(st), _stream()), 'mxl_rules_mask')


def rules_advance(ids, t_dev, rules: Optional[RuleState] = None, **flat):
    """after sample + decode_advance: the words of `rules` (a RuleState, or its fields as keywords; the groups as rules_mask finds
    them) move along the token at ids[b, t] in every row that chose it, then, with unfinished and alive, that token goes through the
    stop rule stop = (eos, pad, min_length): rows with unfinished[b] == 0 get pad and keep their words (mxl_rules_advance).  No launch
    when nothing is given."""
    rules = _rule_state(rules, flat)
    B = ids.shape[0]
    if ids.dtype != torch.int64:
        raise MusicXLError('rules_advance: ids must be (B, .) int64')
    st = rules.struct('rules_advance', ids.device, B)
    check(lib().mxl_rules_advance(_p(ids), ids.stride(0), _p(t_dev), B, rules.vocab_size, C.byref(st), _stream()), 'mxl_rules_advance')


def key_scan(ids, Tp, in_key, gkey, first_bad, check_from=None):
    """gkey[b] = key of row b after columns 0..Tp-1 of ids, walked from the key gkey[b] holds now (ids < 0 skipped); columns before
    check_from (default Tp: none is judged) only move the key, first_bad[b] = the first column from there on that holds a pitch
    outside the row's key, or -1 (mxl_key_scan); the host reference is KeyRule.walk"""
    _req(gkey, torch.int32, 'key_scan gkey'); _req(first_bad, torch.int32, 'key_scan first_bad')
    B = ids.shape[0]
    if ids.dtype != torch.int64 or ids.stride(1) != 1 or Tp > ids.shape[1] or gkey.numel() != B or first_bad.numel() != B:
        raise MusicXLError('key_scan: ids must be (B, >= Tp) int64 with unit column stride, gkey and first_bad (B,)')
    if not gkey.is_contiguous() or not first_bad.is_contiguous():
        raise MusicXLError('key_scan: gkey and first_bad must be contiguous')
    keys, pcs, inkey = in_key.to(ids.device)
    check(lib().mxl_key_scan(_p(ids), ids.stride(0), int(Tp), int(Tp if check_from is None else check_from), B, in_key.vocab_size,
                             _p(keys), _p(pcs), _p(inkey), _p(gkey), _p(first_bad), _stream()), 'mxl_key_scan')


def register_scan(ids, Tp, register, grange, gpart, gfloor, first_bad, gap=-1, check_from=None):
    """(gpart[b], gfloor[b]) = the register words of row b after columns 0..Tp-1 of ids, walked from the words they hold now under
    the bounds grange[b] and `gap` (ids < 0 skipped); columns before check_from (default Tp: none is judged) only move the words,
    first_bad[b] = the first column from there on that holds a pitch outside the bounds of the row's open part, or -1
    (mxl_register_scan); the host reference is RegisterRule.walk"""
    B = ids.shape[0]
    for t, name in ((grange, 'grange'), (gpart, 'gpart'), (gfloor, 'gfloor'), (first_bad, 'first_bad')):
        _req(t, torch.int32, f'register_scan {name}')
        if t.numel() != B or not t.is_contiguous():
            raise MusicXLError(f'register_scan: {name} must be contiguous ({B},) int32')
    if ids.dtype != torch.int64 or ids.stride(1) != 1 or Tp > ids.shape[1]:
        raise MusicXLError('register_scan: ids must be (B, >= Tp) int64 with unit column stride')
    check(lib().mxl_register_scan(_p(ids), ids.stride(0), int(Tp), int(Tp if check_from is None else check_from), B, register.vocab_size,
                                  _p(register.to(ids.device)), _p(grange), int(gap), _p(gpart), _p(gfloor), _p(first_bad), _stream()),
          'mxl_register_scan')


def grammar_scan(ids, Tp, grammar, gstate, first_bad, start=None):
    """gstate[b] = state of row b after columns 0..Tp-1 of ids (ids < 0 skipped), first_bad[b] = column of its first violation or
    -1 (mxl_grammar_scan); the host reference is TokenGrammar.walk"""
    _req(gstate, torch.int32, 'grammar_scan gstate'); _req(first_bad, torch.int32, 'grammar_scan first_bad')
    B = ids.shape[0]
    if ids.dtype != torch.int64 or ids.stride(1) != 1 or Tp > ids.shape[1] or gstate.numel() != B or first_bad.numel() != B:
        raise MusicXLError('grammar_scan: ids must be (B, >= Tp) int64 rows, gstate and first_bad (B,)')
    cls, allow, nxt = grammar.to(ids.device)
    check(lib().mxl_grammar_scan(_p(ids), ids.stride(0), int(Tp), B, grammar.vocab_size, _p(cls), _p(allow), _p(nxt),
                                 grammar.n_classes, grammar.start if start is None else int(start), _p(gstate), _p(first_bad),
                                 _stream()), 'mxl_grammar_scan')


def _budget_state(budget, device, B, gbar, grem, what):
    """(slots, bars) device tables of a grammar.BarBudget, with the per-row words gbar / grem checked"""
    if budget is None:
        raise MusicXLError(f'{what}: the grammar carries no bar budget (tokenizer.grammar(bar_budget=True))')
    if gbar is None or grem is None:
        raise MusicXLError(f'{what}: a grammar with a bar budget needs gbar and grem')
    _req(gbar, torch.int32, f'{what} gbar'); _req(grem, torch.int32, f'{what} grem')
    if gbar.numel() != B or grem.numel() != B or not gbar.is_contiguous() or not grem.is_contiguous():
        raise MusicXLError(f'{what}: gbar and grem must be contiguous ({B},) int32')
    return budget.to(device)


def budget_scan(ids, Tp, grammar, gbar, grem, first_bad):
    """(gbar[b], grem[b]) = bar length and free slots of row b after columns 0..Tp-1 of ids (ids < 0 skipped), first_bad[b] = column
    of the first token the bar budget bars or -1 (mxl_budget_scan); the host reference is TokenGrammar.walk_budget"""
    _req(first_bad, torch.int32, 'budget_scan first_bad')
    B = ids.shape[0]
    if ids.dtype != torch.int64 or ids.stride(1) != 1 or Tp > ids.shape[1] or first_bad.numel() != B or not first_bad.is_contiguous():
        raise MusicXLError('budget_scan: ids must be (B, >= Tp) int64 rows and first_bad contiguous (B,)')
    cls, _, _ = grammar.to(ids.device)
    bud = grammar.budget
    slots, bars = _budget_state(bud, ids.device, B, gbar, grem, 'budget_scan')
    check(lib().mxl_budget_scan(_p(ids), ids.stride(0), int(Tp), B, grammar.vocab_size, _p(cls), _p(slots), _p(bars), bud.opens,
                                bud.need_free, bud.need_full, _p(gbar), _p(grem), _p(first_bad), _stream()), 'mxl_budget_scan')


def _beam_step_args(name, logp, V, beam_scores, ids, nb, hyp_ids, hyp_len, hyp_score, hyp_n, done, n_done, beam_idx, moved, words,
                    n_words):
    """the checks of beam_step, under either of its names; returns (rows, items)"""
    rows = ids.shape[0]
    _req(logp, torch.float32, f'{name} logp'); _req(beam_scores, torch.float32, f'{name} beam_scores')
    _req(hyp_score, torch.float32, f'{name} hyp_score')
    for t, what in ((hyp_len, 'hyp_len'), (hyp_n, 'hyp_n'), (done, 'done'), (n_done, 'n_done'), (beam_idx, 'beam_idx'), (moved, 'moved')):
        _req(t, torch.int32, f'{name} {what}')
    if nb < 1 or rows % nb or ids.dtype != torch.int64 or hyp_ids.dtype != torch.int64 or ids.stride(1) != 1 or logp.stride(1) != 1:
        raise MusicXLError(f'{name}: ids and hyp_ids must be int64 rows of nb per item, logp with unit column stride')
    Bs = rows // nb
    if logp.shape[0] != rows or logp.shape[1] < V or beam_scores.numel() != rows or beam_idx.numel() != rows:
        raise MusicXLError(f'{name}: logp must be ({rows}, >= {V}), beam_scores and beam_idx ({rows},)')
    if (tuple(hyp_ids.shape) != (Bs, nb, ids.shape[1]) or not hyp_ids.is_contiguous() or ids.stride(0) != ids.shape[1]
            or any(t.numel() != rows or not t.is_contiguous() for t in (hyp_len, hyp_score))
            or any(t.numel() != Bs or not t.is_contiguous() for t in (hyp_n, done, moved)) or n_done.numel() != 1):
        raise MusicXLError(f'{name}: the store must be hyp_ids ({Bs}, {nb}, {ids.shape[1]}), hyp_len / hyp_score ({Bs}, {nb}), '
                           f'hyp_n / done / moved ({Bs},), n_done (1,), all contiguous, over contiguous ids')
    if not beam_scores.is_contiguous() or not beam_idx.is_contiguous():
        raise MusicXLError(f'{name}: beam_scores and beam_idx must be contiguous')
    if words is not None:
        _req(words, torch.int32, f'{name} words')
        if n_words < 1 or words.numel() < n_words * rows or not words.is_contiguous():
            raise MusicXLError(f'{name}: words must hold n_words x {rows} contiguous int32')
    return rows, Bs


def beam_step(logp, V, beam_scores, ids, t_dev, nb, eos_id, pad_id, length_penalty, early_stopping, hyp_ids, hyp_len, hyp_score, hyp_n,
              done, n_done, beam_idx, moved, words=None, n_words=0, ng=1, diversity_penalty=0.0):
    """one step of beam search for every item (the nb rows of one prompt), one launch (mxl_beam_step): the 2 * nb best candidates of
    logp (rows, >= V) f32 + beam_scores (rows,) f32 in (score descending, flat index ascending) order, the scorer's walk over them --
    finished hypotheses into the store hyp_ids (Bs, nb, ld) int64 / hyp_len / hyp_score (Bs, nb) / hyp_n / done (Bs,) / n_done (1,) --
    and ids (rows, ld) int64 reordered in place along beam_idx (rows,) int32 with the chosen tokens at column t + 1; moved (Bs,) int32.
    words: the packed per-row int32 rule words (RowRules.buf), n_words words of `rows` entries each, which follow beam_idx.
    ng > 1: diverse (group) beam search (mxl_group_beam_step), the step for the ng groups of nb / ng rows of every item, walked in
    order: group g's candidates score (logp - diversity_penalty * cnt) + beam_scores with cnt[v] the live rows of the item's earlier
    groups that chose v in this step, its 2 * nb / ng best go through the walk over the item's one store of nb slots, and its rows
    continue inside the group."""
    name = 'beam_step' if ng == 1 else 'group_beam_step'
    rows, Bs = _beam_step_args(name, logp, V, beam_scores, ids, nb, hyp_ids, hyp_len, hyp_score, hyp_n, done, n_done, beam_idx, moved,
                               words, n_words)
    front = (_p(logp), logp.stride(0), _p(beam_scores), _p(ids), ids.stride(0), _p(t_dev), Bs, int(nb))
    rest = (int(V), int(eos_id), int(pad_id), float(length_penalty), int(bool(early_stopping)), _p(hyp_ids), _p(hyp_len), _p(hyp_score),
            _p(hyp_n), _p(done), _p(n_done), _p(beam_idx), _p(moved), _p(words), int(n_words) if words is not None else 0, rows, _stream())
    if ng == 1:
        check(lib().mxl_beam_step(*front, *rest), 'mxl_beam_step')
    else:
        check(lib().mxl_group_beam_step(*front, int(ng), float(diversity_penalty), *rest), 'mxl_group_beam_step')


def beam_sample_draw(logp, V, beam_scores, nb, rng_ctr, seed, drawn, top_k=0, top_p=1.0, temperature=1.0, typical_p=1.0, out_warped=None):
    """the draw of one beam-sample step (mxl_beam_sample_draw): every row of logp (rows, >= V) f32, already masked by the rules, goes
    through HF's warpers with min_tokens_to_keep = 2 and is renormalised to w; every item (nb rows) draws 2 * nb of its nb * V
    candidates without replacement with probabilities softmax(w), by Gumbel-top-k with a uniform hashed from (seed, *rng_ctr, row,
    token).  drawn (rows, logp's row stride) f32: w at the drawn candidates, -inf elsewhere in columns 0..V-1.  A row with
    beam_scores == -inf is dead and contributes nothing.  out_warped (rows, V) f32: every row's whole w (a test hook).  The counter is
    read on the device and not advanced."""
    rows = logp.shape[0]
    for t, what in ((logp, 'logp'), (beam_scores, 'beam_scores'), (drawn, 'drawn')):
        _req(t, torch.float32, f'beam_sample_draw {what}')
    if V > 2048:
        raise MusicXLError(f'beam_sample_draw: a vocabulary of {V} tokens is beyond the 2048 of the LDS sort')
    if nb < 2 or rows % nb or logp.shape[1] < V or logp.stride(1) != 1 or beam_scores.numel() != rows or not beam_scores.is_contiguous():
        raise MusicXLError(f'beam_sample_draw: logp must be (rows, >= {V}) with nb >= 2 rows per item, beam_scores (rows,)')
    if drawn.shape[0] != rows or drawn.stride(0) != logp.stride(0) or drawn.stride(1) != 1 or drawn.shape[1] < V:
        raise MusicXLError('beam_sample_draw: drawn must have the rows and the row stride of logp')
    if rng_ctr.dtype != torch.int64 or not rng_ctr.is_cuda:
        raise MusicXLError('beam_sample_draw: rng_ctr must be a device int64 counter')
    if out_warped is not None:
        _req(out_warped, torch.float32, 'beam_sample_draw out_warped')
        if tuple(out_warped.shape) != (rows, V) or not out_warped.is_contiguous():
            raise MusicXLError(f'beam_sample_draw: out_warped must be a contiguous ({rows}, {V})')
    check(lib().mxl_beam_sample_draw(_p(logp), logp.stride(0), int(V), _p(beam_scores), rows // nb, int(nb), _p(rng_ctr),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(top_k or 0), float(top_p if top_p is not None else 1.0),
                                     float(temperature if temperature is not None else 1.0),
                                     float(typical_p if typical_p is not None else 1.0), _p(drawn), _p(out_warped), _stream()),
          'mxl_beam_sample_draw')


def beam_sample_step(drawn, V, beam_scores, ids, t_dev, nb, eos_id, pad_id, length_penalty, early_stopping, hyp_ids, hyp_len, hyp_score,
                     hyp_n, done, n_done, beam_idx, moved, words=None, n_words=0):
    """beam_step over the matrix `drawn` of beam_sample_draw (mxl_beam_sample_step): a candidate's score is its entry of `drawn` itself
    (-inf in a row whose running score is -inf), not a sum with the running score; everything else is beam_step's."""
    rows, Bs = _beam_step_args('beam_sample_step', drawn, V, beam_scores, ids, nb, hyp_ids, hyp_len, hyp_score, hyp_n, done, n_done,
                               beam_idx, moved, words, n_words)
    check(lib().mxl_beam_sample_step(_p(drawn), drawn.stride(0), _p(beam_scores), _p(ids), ids.stride(0), _p(t_dev), Bs, int(nb), int(V),
                                     int(eos_id), int(pad_id), float(length_penalty), int(bool(early_stopping)), _p(hyp_ids), _p(hyp_len),
                                     _p(hyp_score), _p(hyp_n), _p(done), _p(n_done), _p(beam_idx), _p(moved), _p(words),
                                     int(n_words) if words is not None else 0, rows, _stream()), 'mxl_beam_sample_step')


def beam_reorder(bufs, nb, beam_idx, moved, table=None):
    """rows follow their beams in place (mxl_beam_reorder): bufs = one contiguous (rows, ...) tensor, or a list of them of one shape
    with `table`, their addresses as a device int64 tensor (beam_table) -- one launch for all.  Items with moved[b] == 0 are skipped
    whole, rows with beam_idx[r] == r are not written."""
    one = isinstance(bufs, torch.Tensor)
    first = bufs if one else bufs[0]
    rows = first.shape[0]
    row_bytes = first[0].numel() * first.element_size()
    _req(beam_idx, torch.int32, 'beam_reorder beam_idx'); _req(moved, torch.int32, 'beam_reorder moved')
    if nb < 1 or rows % nb or beam_idx.numel() != rows or moved.numel() != rows // nb:
        raise MusicXLError(f'beam_reorder: {rows} rows need nb rows per item, beam_idx ({rows},) and moved (rows / nb,)')
    for t in ([bufs] if one else bufs):
        if not t.is_cuda or not t.is_contiguous() or t.shape != first.shape or t.dtype != first.dtype or t.data_ptr() % 16:
            raise MusicXLError('beam_reorder: the buffers must be contiguous device tensors of one shape, 16-byte aligned')
    if row_bytes % 16:
        raise MusicXLError(f'beam_reorder: rows of {row_bytes} bytes are no multiple of 16')
    if not one and (table is None or table.dtype != torch.int64 or table.numel() != len(bufs) or not table.is_cuda):
        raise MusicXLError('beam_reorder: a list of buffers needs its table (beam_table)')
    check(lib().mxl_beam_reorder(_p(bufs) if one else None, None if one else _p(table), 1 if one else len(bufs), rows // nb, int(nb),
                                 row_bytes, _p(beam_idx), _p(moved), _stream()), 'mxl_beam_reorder')


def beam_owner_follow(owner, nb, beam_idx, moved, t_dev):
    """indexed rings in place of beam_reorder over the K/V rings (mxl_beam_owner_follow): owner (rows, M) uint8, owner[r, s] = j says
    that slot s of row r is held in the ring of row (r // nb) * nb + j.  The rows of an item with moved[b] != 0 follow beam_idx in
    place; then, in every item, each row takes slot (t + 1) % M for itself -- the slot the coming forward pass writes."""
    _req(owner, torch.uint8, 'beam_owner_follow owner')
    _req(beam_idx, torch.int32, 'beam_owner_follow beam_idx'); _req(moved, torch.int32, 'beam_owner_follow moved')
    _req(t_dev, torch.int32, 'beam_owner_follow t_dev')
    if owner.dim() != 2 or not owner.is_contiguous():
        raise MusicXLError('beam_owner_follow: owner must be a contiguous (rows, M) uint8 table')
    rows, M = owner.shape
    if nb < 1 or rows % nb or beam_idx.numel() != rows or moved.numel() != rows // nb:
        raise MusicXLError(f'beam_owner_follow: {rows} rows need nb rows per item, beam_idx ({rows},) and moved (rows / nb,)')
    check(lib().mxl_beam_owner_follow(_p(owner), rows // nb, int(nb), M, _p(beam_idx), _p(moved), _p(t_dev), _stream()),
          'mxl_beam_owner_follow')


def beam_table(bufs) -> torch.Tensor:
    """the addresses of `bufs` as a device int64 tensor, the pointer table of beam_reorder"""
    return torch.tensor([t.data_ptr() for t in bufs], dtype=torch.int64, device=bufs[0].device)


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, relu=False, out=None,
           out_f32=False, drop_p=0.0, seed=0, site=0) -> torch.Tensor:
    """y = x @ w.T (+bias)(relu)(dropout); x (N, K) bf16, w (O, K) bf16."""
    N, K = x.shape
    O = w.shape[0]
    if out is None:
        out = torch.empty(N, O, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    flags = (GEMM_OUT_F32 if out_f32 else 0) | (GEMM_BIAS if bias is not None else 0) | (GEMM_RELU if relu else 0)
    if drop_p > 0:
        flags |= GEMM_DROPOUT
    return gemm(x, w, out, N, O, K, flags=flags, bias=bias, drop_p=drop_p, seed=seed, site=site)


def sinusoid_table(M: int, d: int, clamp_len: int, device, drop_p=0.0, seed=0, site=0, out=None) -> torch.Tensor:
    if out is None:
        out = torch.empty(M, d, device=device, dtype=torch.bfloat16)
    check(lib().mxl_sinusoid_table(_p(out), M, d, clamp_len, float(drop_p), seed, site, _stream()), 'mxl_sinusoid_table')
    return out


def embed_fwd(ids: torch.Tensor, E: torch.Tensor, out: torch.Tensor, scale: float, drop_p=0.0, seed=0, site=0):
    _req(ids, torch.int64, 'ids'); _req(E, torch.bfloat16, 'E')
    N, d = ids.numel(), E.shape[1]
    check(lib().mxl_embed_fwd(_p(ids), _p(E), _p(out), N, d, E.shape[0], float(scale), float(drop_p), seed, site,
                              _stream()), 'mxl_embed_fwd')
    return out


def embed_bwd(ids: torch.Tensor, dout: torch.Tensor, dE: torch.Tensor, scale: float, drop_p=0.0, seed=0, site=0,
              dout2: Optional[torch.Tensor] = None):
    _req(ids, torch.int64, 'ids'); _req(dout, torch.bfloat16, 'dout'); _req(dE, torch.float32, 'dE')
    N, d = ids.numel(), dE.shape[1]
    check(lib().mxl_embed_bwd(_p(ids), _p(dout), _p(dout2), _p(dE), N, d, dE.shape[0], float(scale), float(drop_p), seed,
                              site, _stream()), 'mxl_embed_bwd')
    return dE


def dropout(x: torch.Tensor, y: torch.Tensor, drop_p: float, seed=0, site=0):
    check(lib().mxl_dropout_bf16(_p(x), _p(y), x.numel(), float(drop_p), seed, site, _stream()), 'mxl_dropout_bf16')
    return y


def ln_residual_fwd(x, res, gamma, beta, y, z=None, mean=None, rstd=None, eps=1e-5, drop_p=0.0, seed=0, site=0):
    _req(x, torch.bfloat16, 'x'); _req(gamma, torch.float32, 'gamma'); _req(beta, torch.float32, 'beta')
    d = x.shape[-1]
    N = x.numel() // d
    check(lib().mxl_ln_residual_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(y), _p(z), _p(mean), _p(rstd), N, d,
                                    float(eps), float(drop_p), seed, site, _stream()), 'mxl_ln_residual_fwd')
    return y


def ln_residual_bwd(dy, dy2, z, mean, rstd, gamma, dres, dx, dgamma, dbeta, drop_p=0.0, seed=0, site=0, dxsum=None):
    """`dxsum` (d,) f32: += the column sums of dx (the bias gradient of the linear layer that produced x), d <= 1024"""
    d = z.shape[-1]
    N = z.numel() // d
    if dxsum is not None and d <= 1024:
        check(lib().mxl_ln_residual_bwd_colsum(_p(dy), _p(dy2), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx),
                                               _p(dgamma), _p(dbeta), _p(dxsum), N, d, float(drop_p), seed, site, _stream()),
              'mxl_ln_residual_bwd_colsum')
        return
    check(lib().mxl_ln_residual_bwd(_p(dy), _p(dy2), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dres), _p(dx),
                                    _p(dgamma), _p(dbeta), N, d, float(drop_p), seed, site, _stream()),
          'mxl_ln_residual_bwd')
    if dxsum is not None:
        colsum(dx, dxsum, N, d)


def ln_bwd_add(dy, dy2, z, mean, rstd, gamma, dadd, dres, dgamma, dbeta):
    """dres = LayerNorm-backward(dy + dy2) + dadd"""
    d = z.shape[-1]
    N = z.numel() // d
    check(lib().mxl_ln_residual_bwd_add(_p(dy), _p(dy2), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dadd), _p(dres), _p(dgamma),
                                        _p(dbeta), N, d, _stream()), 'mxl_ln_residual_bwd_add')


def ln_bwd_add_drop(dy, dy2, z, mean, rstd, gamma, dadd, dres, dx, dxsum, dgamma, dbeta, p: float, seed: int, site: int):
    """dres = LayerNorm-backward(dy + dy2) + dadd;  dx = dropout(dres) under (seed, site);  dxsum (optional) += column sums of dx"""
    d = z.shape[-1]
    N = z.numel() // d
    check(lib().mxl_ln_residual_bwd_add_drop(_p(dy), _p(dy2), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dadd), _p(dres), _p(dx),
                                             _p(dxsum), _p(dgamma), _p(dbeta), N, d, float(p), seed, site, _stream()),
          'mxl_ln_residual_bwd_add_drop')


def dropout_colsum(x: torch.Tensor, y: torch.Tensor, out: torch.Tensor, M: int, N: int, p: float, seed: int, site: int):
    """y = dropout(x) (the mask of mxl_dropout_bf16) and out[n] += column sums of y, one pass"""
    check(lib().mxl_dropout_colsum_bf16(_p(x), _p(y), _p(out), M, N, float(p), seed, site, _stream()), 'mxl_dropout_colsum_bf16')


def colsum(x: torch.Tensor, out: torch.Tensor, M: int, N: int, ld: Optional[int] = None):
    check(lib().mxl_colsum_bf16(_p(x), _p(out), M, N, ld if ld is not None else x.stride(-2), _stream()), 'mxl_colsum_bf16')
    return out


def mem_update(mem, hid, out):
    B, M, d = mem.shape
    T = hid.shape[1]
    check(lib().mxl_mem_update(_p(mem), _p(hid), _p(out), B, M, T, d, _stream()), 'mxl_mem_update')
    return out


def phantom_sum_applies(*, T, dh, M, Kc) -> bool:
    """the shapes at which the forward can hand the backward its phantom value-sum (mxl_relattn_fwd_phantom /
    mxl_relattn_bwd_sparse_dg_oph): the ones at which relattn_bwd leaves the all-phantom dG blocks unwritten"""
    return (dh == 64 and T % 32 == 0 and M % 256 == 0 and Kc < M + T and os.environ.get('MXL_NO_DQ8') != '1'
            and os.environ.get('MXL_DG_RECOMPUTE', '1') != '0' and os.environ.get('MXL_NO_OPH') != '1')


def set_reserved_cus(k: int) -> None:
    """compute units the persistent GEMM grids leave free (mxl_set_reserved_cus; dist.GradSync sets it from MXL_RESERVE_CUS)"""
    global _RESERVED_CUS
    check(lib().mxl_set_reserved_cus(int(k)), 'mxl_set_reserved_cus')
    _RESERVED_CUS = int(k)


_RESERVED_CUS = 0
_N_CUS = {}
FUSED_OWNER_MIN_FILL = 0.9        # (csrc/relattn_bwd_fused.hip has the same constant for callers of the C ABI)


def fused_dq_owner_mode(B, H, cus, reserved=0, env=None) -> bool:
    """Which form of mxl_relattn_bwd_fused forms dq: True = owner mode (one workgroup per (sequence, head) walks every key block
    and finishes dq itself, no slabs and no finishing pass), False = per-block mode (one workgroup per key block, bf16 slabs summed by
    mxl_relattn_dq_finish).  Owner mode runs B H equally long workgroups, one per compute unit at a time, so it is chosen when they
    fill the usable units (`cus` minus the `reserved` ones of set_reserved_cus, at least 8) without a long tail: tail efficiency
    B H / (ceil(B H / usable) usable) >= FUSED_OWNER_MIN_FILL.  `env` (a mapping, e.g. os.environ): MXL_FUSED_OWNER = 0 / 1 overrides
    the rule, for A/B runs.  Pure: no device, no library."""
    ov = (env or {}).get('MXL_FUSED_OWNER')
    if ov in ('0', '1'):
        return ov == '1'
    usable = max(int(cus) - int(reserved), 8)
    wgs = int(B) * int(H)
    rounds = (wgs + usable - 1) // usable
    return wgs >= FUSED_OWNER_MIN_FILL * rounds * usable


def _n_cus(device) -> int:
    key = str(device)
    if key not in _N_CUS:
        _N_CUS[key] = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return _N_CUS[key]


def fused_bwd_applies(*, T, dh, M, Kc, B=None, H=None) -> bool:
    """the shapes mxl_relattn_bwd_fused (and, with zero memories, mxl_relattn_drd_phantom) take -- one pass over the score cells, no
    dG tensor: the training shapes of every BASELINE config; anything else stays on relattn_bwd's three kernels.  B, H (optional):
    also the 32-bit offset limits of the phantom-cell kernel's buffer addressing."""
    ok = (dh == 64 and T % 32 == 0 and M % 32 == 0 and M <= 8192 and Kc % 32 == 0 and (T - Kc) % 64 == 0
          and os.environ.get('MXL_NO_FUSED_BWD') != '1')
    if ok and B is not None and H is not None and Kc < M + T:
        ok = H * (T // 32) * 4352 < 2 ** 31 and B * H * T * 4 < 2 ** 31
    return ok


def relattn_fwd(q, k, v, rd, r_w_bias, r_r_bias, out, lse, *, B, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs,
                o_bs, o_rs, scale=None, oph=None, mph=None, oph_all=False, ph_buf=None):
    """q/k/v/out may be strided views (e.g. slices of one (B, Kc, 3*H*dh) qkv buffer); strides in elements.
    `oph` (like out) / `mph` (B, H, T) f32: also write the phantom value-sum relattn_bwd(..., oph=, mph=) consumes
    (oph_all: over every phantom cell, the form relattn_bwd_fused consumes; then `ph_buf`, mxl_relattn_drd_phantom_ws_bytes bytes,
    also receives the records of the phantom cells' dRd kernel: pass the same buffer to relattn_bwd_fused(ph_buf=, ph_ready=True))."""
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    if oph is not None and oph_all:
        check(lib().mxl_relattn_fwd_phantom2(_p(q), _p(k), _p(v), _p(rd), _p(r_w_bias), _p(r_r_bias), _p(out), _p(lse), _p(oph),
                                             _p(mph), 1, _p(ph_buf), B, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs,
                                             float(scale), _stream()), 'mxl_relattn_fwd_phantom2')
        return out
    if oph is not None:
        check(lib().mxl_relattn_fwd_phantom(_p(q), _p(k), _p(v), _p(rd), _p(r_w_bias), _p(r_r_bias), _p(out), _p(lse), _p(oph),
                                            _p(mph), B, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs, float(scale),
                                            _stream()), 'mxl_relattn_fwd_phantom')
        return out
    check(lib().mxl_relattn_fwd(_p(q), _p(k), _p(v), _p(rd), _p(r_w_bias), _p(r_r_bias), _p(out), _p(lse), B, T, H, dh,
                                M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs, float(scale), _stream()),
          'mxl_relattn_fwd')
    return out


def label_guard(labels: torch.Tensor, eos: int):
    _req(labels, torch.int64, 'labels')
    check(lib().mxl_label_guard(_p(labels), labels.shape[1], int(eos), _stream()), 'mxl_label_guard')


def adaptive_nll_fwd(logits, labels, nll, lse, acc2, B, T, V, cutoffs=()):
    n, arr = _cut(cutoffs)
    check(lib().mxl_adaptive_nll_fwd(_p(logits), logits.stride(0), _p(labels), _p(nll), _p(lse), _p(acc2), B, T, V, n,
                                     C.cast(arr, C.c_void_p) if arr is not None else None, _stream()),
          'mxl_adaptive_nll_fwd')


def adaptive_nll_bwd(logits, labels, nll, lse, acc2, dlogits, B, T, V, cutoffs=(), grad_scale=1.0, dlogits_lo=None):
    n, arr = _cut(cutoffs)
    if dlogits_lo is not None:          # two-term form: dlogits + dlogits_lo carries the gradient to 2^-16
        assert dlogits_lo.shape == dlogits.shape and dlogits_lo.stride(0) == dlogits.stride(0)
        check(lib().mxl_adaptive_nll_bwd_split(_p(logits), logits.stride(0), _p(labels), _p(nll), _p(lse), _p(acc2), _p(dlogits),
                                               _p(dlogits_lo), dlogits.stride(0), B, T, V, n,
                                               C.cast(arr, C.c_void_p) if arr is not None else None, float(grad_scale),
                                               _stream()), 'mxl_adaptive_nll_bwd_split')
        return
    check(lib().mxl_adaptive_nll_bwd(_p(logits), logits.stride(0), _p(labels), _p(nll), _p(lse), _p(acc2), _p(dlogits),
                                     dlogits.stride(0), B, T, V, n,
                                     C.cast(arr, C.c_void_p) if arr is not None else None, float(grad_scale), _stream()),
          'mxl_adaptive_nll_bwd')


def adaptive_logprob(logits, out, N, V, cutoffs=()):
    n, arr = _cut(cutoffs)
    check(lib().mxl_adaptive_logprob(_p(logits), logits.stride(0), _p(out), out.stride(0), N, V, n,
                                     C.cast(arr, C.c_void_p) if arr is not None else None, _stream()),
          'mxl_adaptive_logprob')
    return out


# ---- large-vocabulary (bucketed) adaptive softmax: see csrc/head_large.hip
def cluster_bucket(labels, V, cutoffs, perm, counts, tgt_head, tgt_tail):
    B, T = labels.shape
    n, arr = _cut(cutoffs)
    check(lib().mxl_cluster_bucket(_p(labels), B, T, V, n, C.cast(arr, C.c_void_p), _p(perm), _p(counts), _p(tgt_head),
                                   _p(tgt_tail), _stream()), 'mxl_cluster_bucket')


def gather_rows(src, idx, dst, n):
    check(lib().mxl_gather_rows_bf16(_p(src), src.stride(-2), _p(idx), _p(dst), n, src.shape[-1], _stream()), 'mxl_gather_rows_bf16')
    return dst


def scatter_add_rows(src, idx, dst, n):
    check(lib().mxl_scatter_add_rows_bf16(_p(src), _p(idx), _p(dst), dst.stride(-2), n, src.shape[-1], _stream()),
          'mxl_scatter_add_rows_bf16')


def rows_lse_pick(logits, ncols, n_rows, tgt, lse_out, pick_out, rows_idx=None, row0=0):
    check(lib().mxl_rows_lse_pick(_p(logits), logits.stride(0), ncols, n_rows, _p(rows_idx), row0, _p(tgt), _p(lse_out),
                                  _p(pick_out), _stream()), 'mxl_rows_lse_pick')


def bucket_nll_finish(hlse, hpick, tlse, tpick, tgt_head, tgt_tail, nll, nll_tok, acc2, B, T):
    check(lib().mxl_bucket_nll_finish(_p(hlse), _p(hpick), _p(tlse), _p(tpick), _p(tgt_head), _p(tgt_tail), _p(nll), _p(nll_tok),
                                      _p(acc2), B, T, _stream()), 'mxl_bucket_nll_finish')


def rows_softmax_grad(logits, ncols, n_rows, tgt, lse, nll_tok, acc2, grad_scale, out_hi, out_lo=None, rows_idx=None, row0=0):
    check(lib().mxl_rows_softmax_grad(_p(logits), logits.stride(0), ncols, n_rows, _p(rows_idx), row0, _p(tgt), _p(lse), _p(nll_tok),
                                      _p(acc2), float(grad_scale), _p(out_hi), _p(out_lo), out_hi.stride(0), _stream()),
          'mxl_rows_softmax_grad')


def sumsq(x: torch.Tensor, out_accum: torch.Tensor):
    check(lib().mxl_sumsq_f32(_p(x), x.numel(), _p(out_accum), _stream()), 'mxl_sumsq_f32')


def adamw_step(p, g, m, v, w16, n_decay, lr, beta1, beta2, eps, weight_decay, step, sumsq_buf=None, max_norm=0.0,
               grad_scale=1.0):
    check(lib().mxl_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(w16), p.numel(), n_decay, float(lr), float(beta1),
                               float(beta2), float(eps), float(weight_decay), int(step), _p(sumsq_buf), float(max_norm),
                               float(grad_scale), _stream()), 'mxl_adamw_step')


def cast_bf16(x: torch.Tensor, y: torch.Tensor):
    check(lib().mxl_cast_f32_bf16(_p(x), _p(y), x.numel(), _stream()), 'mxl_cast_f32_bf16')
    return y


def cast_f32(x: torch.Tensor, y: torch.Tensor):
    """y (f32) = x (bf16)"""
    _req(x, torch.bfloat16, 'x'); _req(y, torch.float32, 'y')
    check(lib().mxl_cast_bf16_f32(_p(x), _p(y), x.numel(), _stream()), 'mxl_cast_bf16_f32')
    return y


def center_columns(x: torch.Tensor, y: torch.Tensor):
    """y = x - mean over rows (bf16, (M, N))"""
    M, N = x.shape
    check(lib().mxl_center_columns_bf16(_p(x), _p(y), M, N, _stream()), 'mxl_center_columns_bf16')
    return y


def transpose(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, *, ld_src=None, ld_dst=None, batch=1,
              src_bstride=0, dst_bstride=0):
    """dst[b][c][r] = src[b][r][c] (bf16)"""
    _req(src, torch.bfloat16, 'src'); _req(dst, torch.bfloat16, 'dst')
    check(lib().mxl_transpose_bf16(_p(src), _p(dst), rows, cols, ld_src if ld_src is not None else cols,
                                   ld_dst if ld_dst is not None else rows, batch, src_bstride, dst_bstride, _stream()),
          'mxl_transpose_bf16')
    return dst


def gemm_batched(a, b, c, M, N, K, *, lda, ldb, ldc, trans_a=False, trans_b=False, flags=0, alpha=1.0, ksplits=1,
                 batch=1, bdiv=1, sA=(0, 0), sB=(0, 0), sC=(0, 0)):
    check(lib().mxl_gemm_bf16_batched(_p(a), _p(b), _p(c), M, N, K, lda, ldb, ldc, int(trans_a), int(trans_b), flags,
                                      float(alpha), ksplits, batch, bdiv, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1],
                                      _stream()), 'mxl_gemm_bf16_batched')
    return c


def add_rowbias(x, x_bs, x_rs, bias, out, B, T, n):
    check(lib().mxl_add_rowbias_bf16(_p(x), x_bs, x_rs, _p(bias), _p(out), B, T, n, _stream()), 'mxl_add_rowbias_bf16')
    return out


def relattn_bwd(q, k, v, rd, r_w_bias, r_r_bias, out, dout, lse, delta, dq, dk, dv, dg, d_rwb, d_rrb, *, B, T, H, dh, M,
                Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs, scale=None,
                d_rd: Optional[torch.Tensor] = None, qr_buf: Optional[torch.Tensor] = None, defer_drd: bool = False,
                oph: Optional[torch.Tensor] = None, mph: Optional[torch.Tensor] = None):
    """Backward of relattn_fwd.  If `d_rd` (M, H*dh) f32 is given, also contracts dG with (q + r_r_bias):
    d_rd[d, h, :] += sum_{b,i} dG[b,h,i,d] * (q + r_r_bias)[b,i,h,:]   (needs dg and a (B,T,H*dh) bf16 qr_buf).
    When that contraction runs as the streaming kernel (dh = 64, T % 32 == 0, M % 8 == 0) it also produces d_rrb, and the
    backward proper is launched without it -- its query-owner kernel then takes the faster 8-wave form.

    `dg` may hold FEWER sequences than B: the batch is then walked in chunks of dg.shape[0] sequences, each chunk's attention
    backward followed at once by its dRd contraction, so the un-skewed score gradient of a chunk (B_c * H * T * M * 2 bytes) is
    produced and consumed while it is still in the 256 MB Infinity Cache instead of making a round trip through HBM (per-sequence
    outputs are unaffected; the batch-summed ones are atomically accumulated in any case)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    fused_rrb = (d_rd is not None and dg is not None and dh == 64 and T % 32 == 0 and M % 8 == 0 and M >= 8
                 and os.environ.get('MXL_NO_DQ8') != '1')
    Bc = B if dg is None else min(B, dg.shape[0])
    # phantom distances (zero memories: k = v = 0) stay out of HBM: the backward leaves their dG blocks unwritten and the dRd
    # contraction rebuilds them from qr, rd, lse and delta (mxl_relattn_bwd_sparse_dg / mxl_relattn_drd_recompute)
    sparse = fused_rrb and M % 256 == 0 and Kc < M + T and os.environ.get('MXL_DG_RECOMPUTE', '1') != '0'
    assert oph is None or sparse, 'oph / mph are for the shapes phantom_sum_applies() accepts, with d_rd / dg given'

    def launch(b0, n):
        sl = slice(b0, b0 + n)
        if sparse and oph is not None:          # the forward's phantom value-sum: the all-phantom blocks are not walked at all
            check(lib().mxl_relattn_bwd_sparse_dg_oph(_p(q[sl]), _p(k[sl]), _p(v[sl]), _p(rd), _p(r_w_bias), _p(r_r_bias),
                                                      _p(out[sl]), _p(dout[sl]), _p(lse[sl]), _p(delta[sl]), _p(dq[sl]), _p(dk[sl]),
                                                      _p(dv[sl]), _p(dg), _p(d_rwb), _p(oph[sl]), _p(mph[sl]), n, T, H, dh, M, Kc,
                                                      q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs,
                                                      float(scale), _stream()), 'mxl_relattn_bwd_sparse_dg_oph')
            return
        if sparse:
            check(lib().mxl_relattn_bwd_sparse_dg(_p(q[sl]), _p(k[sl]), _p(v[sl]), _p(rd), _p(r_w_bias), _p(r_r_bias), _p(out[sl]),
                                                  _p(dout[sl]), _p(lse[sl]), _p(delta[sl]), _p(dq[sl]), _p(dk[sl]), _p(dv[sl]),
                                                  _p(dg), _p(d_rwb), n, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs,
                                                  o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs, float(scale), _stream()),
                  'mxl_relattn_bwd_sparse_dg')
            return
        check(lib().mxl_relattn_bwd(_p(q[sl]), _p(k[sl]), _p(v[sl]), _p(rd), _p(r_w_bias), _p(r_r_bias), _p(out[sl]), _p(dout[sl]),
                                    _p(lse[sl]), _p(delta[sl]), _p(dq[sl]), _p(dk[sl]), _p(dv[sl]), _p(dg), _p(d_rwb),
                                    None if fused_rrb else _p(d_rrb), n, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs,
                                    o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs, float(scale), _stream()), 'mxl_relattn_bwd')

    def drd(b0, n):
        if d_rd is not None:
            relattn_drd(q[b0:b0 + n], r_r_bias, dg, d_rd, qr_buf, B=n, T=T, H=H, dh=dh, M=M, q_bs=q_bs, q_rs=q_rs,
                        rd=rd if fused_rrb else None, rd_rs=rd_rs, d_rrb=d_rrb if fused_rrb else None,
                        d_rwb=d_rwb if fused_rrb else None,
                        recompute=dict(lse=lse[b0:b0 + n], delta=delta[b0:b0 + n], scale=scale, Kc=Kc) if sparse else None)

    if Bc >= B:
        launch(0, B)
        if defer_drd:          # (bench.py brackets the attention-backward launches alone)
            return lambda: drd(0, B)
        drd(0, B)
        return None
    for b0 in range(0, B, Bc):
        n = min(Bc, B - b0)
        launch(b0, n)
        drd(b0, n)
    return (lambda: None) if defer_drd else None


def relattn_bwd_fused_ws_numel(B, T, H, dh, M) -> int:
    """fp32 elements of the partial-dq slabs mxl_relattn_bwd_fused needs"""
    return int(lib().mxl_relattn_bwd_fused_ws_bytes(B, T, H, dh, M)) // 4


_PH_WS = {}


def _phantom_ws(B, T, H, device):
    """scratch of mxl_relattn_drd_phantom_prep (one record per sequence, head and 32-query tile), one per shape and device, allocated on
    first use; callers that capture graphs or account for every byte pass their own `ph_buf`"""
    key = (B, T, H, str(device))
    buf = _PH_WS.get(key)
    if buf is None:
        buf = torch.empty(int(lib().mxl_relattn_drd_phantom_ws_bytes(B, T, H)), device=device, dtype=torch.uint8)
        _PH_WS[key] = buf
    return buf


def gemm_headdot(a, b, c, M, N, K, o, T, delta, lda=None, ldb=None, ldc=None, ldo=None):
    """c = a @ b^T (bf16) and delta[(b_, h, t)] = sum_e c[m, 64 h + e] * o[m, 64 h + e] in the same launch (mxl_gemm_bf16_headdot).
    Returns True when delta was written; False when the problem is not the four-wave large-tile kernel's (c is written either way)."""
    rc = lib().mxl_gemm_bf16_headdot(_p(a), _p(b), _p(c), M, N, K, lda or K, ldb or K, ldc or N, _p(o), ldo or N, T, _p(delta), _stream())
    if rc == -2:      # MXL_EUNSUPPORTED: not the four-wave kernel's problem (c is written, delta is not)
        return False
    check(rc, 'mxl_gemm_bf16_headdot')
    return True


def relattn_bwd_fused(q, k, v, rd, r_w_bias, r_r_bias, out, dout, lse, delta, dq, dk, dv, d_rd, d_rwb, d_rrb, ws, qr_buf, *,
                      B, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs,
                      scale=None, oph=None, mph=None, defer_drd=False, ph_buf=None, ph_ready=False, delta_ready=False, dq_mode=None):
    """Backward of relattn_fwd in one pass over the score cells (mxl_relattn_bwd_fused): dq, dk, dv written, d_rd (M, H*dh) f32 /
    d_rwb / d_rrb accumulated.  With zero memories (Kc < M + T) `oph` / `mph` must come from relattn_fwd(..., oph_all=True), and
    the phantom cells' part of d_rd is added by mxl_relattn_drd_phantom from per-tile records (`ph_buf`,
    mxl_relattn_drd_phantom_ws_bytes bytes; ph_ready: relattn_fwd(..., ph_buf=) has filled them, otherwise
    mxl_relattn_drd_phantom_prep does; without `ph_buf` one scratch per shape is cached; `qr_buf` is no longer used by this path);
    their part of d_rrb comes out of the dq finishing kernel (per-block mode) or of the fused kernel itself (owner mode).
    delta_ready: `delta` was filled by gemm_headdot.  dq_mode: 'owner' / 'slabs' forces the form that produces dq; None leaves it
    to fused_dq_owner_mode (MXL_FUSED_OWNER = 0 / 1, read at every call, overrides that rule)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    d = H * dh
    if dq_mode is None:
        owner = fused_dq_owner_mode(B, H, _n_cus(q.device), _RESERVED_CUS, os.environ)
    else:
        if dq_mode not in ('owner', 'slabs'):
            raise ValueError(f'dq_mode must be None, "owner" or "slabs", not {dq_mode!r}')
        owner = dq_mode == 'owner'
    mode_bits = (2 if delta_ready else 0) | (4 if owner else 8)
    # (the slab sum on a side stream beside the phantom cells' dRd kernel measured 7.16 ms against 7.12 ms in sequence -- the HBM-bound
    # sum fills the chip by itself -- and left dq / d_rrb incomplete until the deferred call: removed in round 5)
    check(lib().mxl_relattn_bwd_fused(_p(q), _p(k), _p(v), _p(rd), _p(r_w_bias), _p(r_r_bias), _p(out), _p(dout), _p(lse), _p(delta),
                                      _p(dq), _p(dk), _p(dv), _p(d_rd), d_rd.stride(0), _p(d_rwb), _p(d_rrb), _p(oph), _p(mph), _p(ws),
                                      B, T, H, dh, M, Kc, q_bs, q_rs, kv_bs, kv_rs, rd_rs, o_bs, o_rs, dq_bs, dq_rs, dkv_bs, dkv_rs,
                                      float(scale), mode_bits, _stream()), 'mxl_relattn_bwd_fused')

    def phantom():
        if Kc < M + T:
            ph = ph_buf if ph_buf is not None else _phantom_ws(B, T, H, q.device)
            if not (ph_ready and ph_buf is not None):
                check(lib().mxl_relattn_drd_phantom_prep(_p(q), q_bs, q_rs, _p(r_r_bias), _p(lse), _p(ph), B, T, H, dh, float(scale),
                                                         _stream()), 'mxl_relattn_drd_phantom_prep')
            check(lib().mxl_relattn_drd_phantom(_p(ph), _p(delta), _p(d_rd), B, T, H, dh, M, d_rd.stride(0), _p(rd), int(rd_rs), Kc,
                                                _stream()), 'mxl_relattn_drd_phantom')
    if defer_drd:
        return phantom
    phantom()
    return None


def relattn_drd(q, r_r_bias, dg, d_rd, qr_buf, *, B, T, H, dh, M, q_bs, q_rs, rd=None, rd_rs=0, d_rrb=None, d_rwb=None,
                recompute=None):
    """d_rd[delta, h*dh:(h+1)*dh] (M x dh, fp32, +=) = sum_b dG[b,h]^T (M x T) @ (q + r_r_bias)[b,:,h,:] (T x dh); with rd /
    d_rrb (/ d_rwb) also d_rrb += colsum(dG) . Rd (and d_rwb -= the same): see mxl_relattn_drd"""
    d = H * dh
    add_rowbias(q, q_bs, q_rs, r_r_bias.reshape(-1), qr_buf, B, T, d)
    if recompute is not None:        # dg came from mxl_relattn_bwd_sparse_dg: its all-phantom blocks are rebuilt, not read
        check(lib().mxl_relattn_drd_recompute(_p(dg), _p(qr_buf), _p(d_rd), B, T, H, dh, M, T * d, d, d, _p(rd), int(rd_rs),
                                              _p(d_rrb), _p(d_rwb), _p(recompute['lse']), _p(recompute['delta']),
                                              float(recompute['scale']), int(recompute['Kc']), _stream()),
              'mxl_relattn_drd_recompute')
        return
    rc = lib().mxl_relattn_drd(_p(dg), _p(qr_buf), _p(d_rd), B, T, H, dh, M, T * d, d, d, _p(rd), int(rd_rs), _p(d_rrb),
                               _p(d_rwb), _stream())
    if rc == -2:      # MXL_EUNSUPPORTED shape: the batched GEMM form
        assert d_rrb is None
        gemm_batched(dg, qr_buf, d_rd, M, dh, T, lda=M, ldb=d, ldc=d, trans_a=True, trans_b=True,
                     flags=GEMM_OUT_F32_ATOMIC, batch=B * H, bdiv=H, sA=(H * T * M, T * M), sB=(T * d, dh), sC=(0, dh))
    else:
        check(rc, 'mxl_relattn_drd')


# ------------------------------------------------------------------ decode
def decode_embed(ids, t_dev, E, out, scale):
    B, d = out.shape
    check(lib().mxl_decode_embed(_p(ids), ids.stride(0), _p(t_dev), _p(E), _p(out), B, d, E.shape[0], float(scale),
                                 _stream()), 'mxl_decode_embed')


def kv_append(qkv, kc, vc, t_dev, rrb=None, qr_out=None):
    """kc / vc: head-major rings (B, H, M, dh).  With `rrb` (H*dh f32) and `qr_out` (B, H*dh) bf16 the same launch also writes
    q + r_r_bias, the operand of the step's BD product (then pass qr_ready=True to relattn_decode)."""
    B, H, M, dh = kc.shape
    check(lib().mxl_kv_append(_p(qkv), _p(kc), _p(vc), _p(t_dev), B, M, H * dh, dh, _p(rrb), _p(qr_out), _stream()),
          'mxl_kv_append')


def kv_fill(qkv, kc, vc, T):
    B, H, M, dh = kc.shape
    check(lib().mxl_kv_fill(_p(qkv), _p(kc), _p(vc), B, T, M, H * dh, dh, _stream()), 'mxl_kv_fill')


def _req_fp8_rings(kc8, ke, vc8, ve, what):
    """fp8 rings: kc8 / vc8 (B, H, M, dh) uint8 of e4m3fn bytes, ke / ve (B, H, M) int8 exponents, all contiguous"""
    for t, dt in ((kc8, torch.uint8), (vc8, torch.uint8), (ke, torch.int8), (ve, torch.int8)):
        _req(t, dt, what)
        if not t.is_contiguous():
            raise MusicXLError(f'{what}: fp8 rings and their exponents must be contiguous')
    if kc8.dim() != 4 or vc8.shape != kc8.shape or ke.shape != kc8.shape[:3] or ve.shape != kc8.shape[:3]:
        raise MusicXLError(f'{what}: expected (B, H, M, dh) byte rings with (B, H, M) exponents')


def kv_append_fp8(qkv, kc8, ke, vc8, ve, t_dev, rrb=None, qr_out=None):
    """kv_append on fp8 rings (mxl_kv_append_fp8): slot t mod M of the bytes and exponents <- the quantised k / v of the qkv rows"""
    _req_fp8_rings(kc8, ke, vc8, ve, 'kv_append_fp8')
    B, H, M, dh = kc8.shape
    check(lib().mxl_kv_append_fp8(_p(qkv), _p(kc8), _p(ke), _p(vc8), _p(ve), _p(t_dev), B, M, H * dh, dh, _p(rrb), _p(qr_out),
                                  _stream()), 'mxl_kv_append_fp8')


def kv_fill_fp8(qkv, kc8, ke, vc8, ve, T):
    """kv_fill on fp8 rings (mxl_kv_fill_fp8)"""
    _req_fp8_rings(kc8, ke, vc8, ve, 'kv_fill_fp8')
    B, H, M, dh = kc8.shape
    check(lib().mxl_kv_fill_fp8(_p(qkv), _p(kc8), _p(ke), _p(vc8), _p(ve), B, T, M, H * dh, dh, _stream()), 'mxl_kv_fill_fp8')


def kv_zero_pad(qkv, n_pad, B, T, d):
    """left-padded prompt pass: k = v = 0 in the first n_pad[b] rows of every sequence of the (B, T, 3d) bf16 qkv buffer.
    n_pad: (B,) int32 on the device"""
    _req(qkv, torch.bfloat16, 'kv_zero_pad qkv')
    _req(n_pad, torch.int32, 'kv_zero_pad n_pad')
    if not qkv.is_contiguous() or qkv.numel() != B * T * 3 * d or n_pad.numel() != B or not n_pad.is_contiguous():
        raise MusicXLError(f'kv_zero_pad: expected a contiguous ({B}, {T}, {3 * d}) qkv buffer and ({B},) n_pad')
    check(lib().mxl_kv_zero_pad(_p(qkv), _p(n_pad), B, T, d, _stream()), 'mxl_kv_zero_pad')


def decode_ring_pieces(B: int, H: int, M: int) -> int:
    """workgroups per (sequence, head) ring of a decode step (mxl_relattn_decode_split).  With fewer rings than CUs a ring per
    workgroup leaves CUs idle and every workgroup streaming 512 KB alone: two pieces up to 256 rings, four up to 96 (measured on
    the C5 shape, scripts/perf_decode_attn.py: B = 4: 27.3 -> 14.4 us, B = 8: 28.4 -> 17.7, B = 16: 29.7 -> 25.0, B = 21: 31.8 -> 27.3;
    from 384 rings on the pieces cost more than they balance: B = 32: 39.4 -> 42.7).  One piece for short rings.
    MXL_DECODE_PIECES overrides."""
    env = os.environ.get('MXL_DECODE_PIECES')
    if env:
        return max(1, min(8, int(env)))
    if M < 1024 or B * H > 256:
        return 1
    return 4 if B * H <= 96 else 2


def relattn_decode_split_scratch(B: int, H: int, dh: int, pieces: int, dev):
    """(ws, arrived) of mxl_relattn_decode_split, or None for one piece"""
    if pieces <= 1:
        return None
    n = int(lib().mxl_relattn_decode_split_ws_bytes(B, H, dh, pieces)) // 4
    return torch.empty(n, device=dev, dtype=torch.float32), torch.zeros(B * H, device=dev, dtype=torch.int32)


def relattn_decode(qkv, kc, vc, rd, rwb, rrb, out, t_dev, H, dh, qr_buf, bd_buf, scale=None, qr_ready=False, split=None, pieces=1,
                   unfinished=None, owner=None, nb=1):
    """qr_buf (B, H*dh) bf16 and bd_buf (B, H, M) f32 are scratch: BD = (q + r_r_bias) . rd^T for the whole batch.
    qr_ready: qr_buf already holds q + r_r_bias (written by kv_append).  split = relattn_decode_split_scratch(...) with the same
    `pieces`: the ring of every (sequence, head) goes to that many workgroups.  unfinished: (B,) int32 device stop state of
    generation -- finished rows (0) read no ring and get zeros in `out` (mxl_relattn_decode_split_live).
    owner: (B, M) uint8 with `nb` rows per item -- indexed rings: slot s of row b is read from the ring of row
    (b // nb) * nb + owner[b, s] (mxl_relattn_decode_owned; the BD launch is the same)."""
    B, _, M, _ = kc.shape
    d = H * dh
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    if not qr_ready:
        add_rowbias(qkv, 3 * d, 3 * d, rrb.reshape(-1), qr_buf, B, 1, d)
    if dh == 64 and B <= 64:
        check(lib().mxl_decode_bd(_p(qr_buf), _p(rd), _p(bd_buf), B, H, dh, M, d, rd.stride(0), _stream()), 'mxl_decode_bd')
    else:
        gemm_batched(qr_buf, rd, bd_buf, B, M, dh, lda=d, ldb=d, ldc=H * M, flags=GEMM_OUT_F32, batch=H, bdiv=1,
                     sA=(dh, 0), sB=(dh, 0), sC=(M, 0))
    if unfinished is not None:
        _req(unfinished, torch.int32, 'relattn_decode unfinished')
    if owner is not None:
        _req(owner, torch.uint8, 'relattn_decode owner')
        if tuple(owner.shape) != (B, M) or not owner.is_contiguous():
            raise MusicXLError(f'relattn_decode: owner must be a contiguous ({B}, {M}) uint8 table')
        n = pieces if (split is not None and pieces > 1) else 1
        check(lib().mxl_relattn_decode_owned(_p(qkv), _p(kc), _p(vc), _p(owner), int(nb), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), B, H,
                                             dh, M, float(scale), n, _p(split[0]) if n > 1 else 0, _p(split[1]) if n > 1 else 0,
                                             _p(unfinished), _stream()), 'mxl_relattn_decode_owned')
        return
    if unfinished is not None:
        n = pieces if (split is not None and pieces > 1) else 1
        check(lib().mxl_relattn_decode_split_live(_p(qkv), _p(kc), _p(vc), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), B, H, dh, M,
                                                  float(scale), n, _p(split[0]) if n > 1 else 0, _p(split[1]) if n > 1 else 0,
                                                  _p(unfinished), _stream()), 'mxl_relattn_decode_split_live')
        return
    if split is not None and pieces > 1:
        check(lib().mxl_relattn_decode_split(_p(qkv), _p(kc), _p(vc), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), B, H, dh, M,
                                             C.c_float(float(scale)), pieces, _p(split[0]), _p(split[1]), _stream()),
              'mxl_relattn_decode_split')
        return
    check(lib().mxl_relattn_decode(_p(qkv), _p(kc), _p(vc), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), B, H, dh, M,
                                   float(scale), _stream()), 'mxl_relattn_decode')


def relattn_decode_fp8(qkv, kc8, ke, vc8, ve, rd, rwb, rrb, out, t_dev, H, dh, qr_buf, bd_buf, scale=None, qr_ready=False, split=None,
                       pieces=1, unfinished=None, owner=None, nb=1):
    """relattn_decode over fp8 rings (mxl_relattn_decode_fp8): the same BD launch, then the one fp8 attention entry.
    owner: (B, M) uint8 with `nb` rows per item -- indexed rings: the bytes and the exponents of slot s of row b are read from the
    rings of row (b // nb) * nb + owner[b, s] (mxl_relattn_decode_fp8_owned)."""
    _req_fp8_rings(kc8, ke, vc8, ve, 'relattn_decode_fp8')
    B, _, M, _ = kc8.shape
    d = H * dh
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    if not qr_ready:
        add_rowbias(qkv, 3 * d, 3 * d, rrb.reshape(-1), qr_buf, B, 1, d)
    if dh == 64 and B <= 64:
        check(lib().mxl_decode_bd(_p(qr_buf), _p(rd), _p(bd_buf), B, H, dh, M, d, rd.stride(0), _stream()), 'mxl_decode_bd')
    else:
        gemm_batched(qr_buf, rd, bd_buf, B, M, dh, lda=d, ldb=d, ldc=H * M, flags=GEMM_OUT_F32, batch=H, bdiv=1,
                     sA=(dh, 0), sB=(dh, 0), sC=(M, 0))
    if unfinished is not None:
        _req(unfinished, torch.int32, 'relattn_decode_fp8 unfinished')
    n = pieces if (split is not None and pieces > 1) else 1
    if owner is not None:
        _req(owner, torch.uint8, 'relattn_decode_fp8 owner')
        if tuple(owner.shape) != (B, M) or not owner.is_contiguous():
            raise MusicXLError(f'relattn_decode_fp8: owner must be a contiguous ({B}, {M}) uint8 table')
        check(lib().mxl_relattn_decode_fp8_owned(_p(qkv), _p(kc8), _p(ke), _p(vc8), _p(ve), _p(owner), int(nb), _p(bd_buf), _p(rwb),
                                                 _p(out), _p(t_dev), B, H, dh, M, float(scale), n, _p(split[0]) if n > 1 else 0,
                                                 _p(split[1]) if n > 1 else 0, _p(unfinished), _stream()),
              'mxl_relattn_decode_fp8_owned')
        return
    check(lib().mxl_relattn_decode_fp8(_p(qkv), _p(kc8), _p(ke), _p(vc8), _p(ve), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), B, H, dh, M,
                                       float(scale), n, _p(split[0]) if n > 1 else 0, _p(split[1]) if n > 1 else 0,
                                       _p(unfinished), _stream()), 'mxl_relattn_decode_fp8')


_sample_scratch = {}


def sample(logprobs, ids, t_dev, rng_ctr, seed, do_sample=False, top_k=0, top_p=1.0, temperature=1.0,
           repetition_penalty=1.0, typical_p=1.0, out_probs=None):
    B, V = logprobs.shape
    if V > 2048 or os.environ.get('MXL_SAMPLE_LARGE') == '1':      # beyond the LDS sort: the bisection sampler (sample_large.hip)
        key = (logprobs.device, B, V)
        scratch = _sample_scratch.get(key)
        if scratch is None:
            _sample_scratch.clear()
            scratch = _sample_scratch[key] = torch.empty(B, 2 * V, device=logprobs.device, dtype=torch.float32)
        check(lib().mxl_sample_large(_p(logprobs), logprobs.stride(0), V, _p(ids), ids.stride(0), _p(t_dev), _p(rng_ctr), seed, B,
                                     int(do_sample), int(top_k or 0), float(top_p if top_p is not None else 1.0),
                                     float(temperature), float(repetition_penalty if repetition_penalty is not None else 1.0),
                                     float(typical_p if typical_p is not None else 1.0), _p(out_probs), _p(scratch), _stream()),
              'mxl_sample_large')
        return
    check(lib().mxl_sample(_p(logprobs), logprobs.stride(0), V, _p(ids), ids.stride(0), _p(t_dev), _p(rng_ctr), seed, B,
                           int(do_sample), int(top_k or 0), float(top_p if top_p is not None else 1.0),
                           float(temperature), float(repetition_penalty if repetition_penalty is not None else 1.0),
                           float(typical_p if typical_p is not None else 1.0), _p(out_probs), _stream()), 'mxl_sample')


def find_token(ids: torch.Tensor, token: int, which: int = -1) -> torch.Tensor:
    """(B,) int32: index of the last (which < 0) / which-th occurrence of `token` per row of ids (B, T) int64, -1 if none"""
    B, T = ids.shape
    out = torch.empty(B, device=ids.device, dtype=torch.int32)
    check(lib().mxl_find_token(_p(ids), ids.stride(0), B, T, int(token), int(which), _p(out), _stream()), 'mxl_find_token')
    return out


def decode_advance(t_dev, rng_ctr):
    check(lib().mxl_decode_advance(_p(t_dev), _p(rng_ctr), _stream()), 'mxl_decode_advance')


def row_inv_norm(x, out, n):
    """out[j] = 1 / ||x[j]||  (bf16 rows)"""
    check(lib().mxl_row_inv_norm_bf16(_p(x), x.stride(-2), n, x.shape[-1], _p(out), _stream()), 'mxl_row_inv_norm_bf16')
    return out


def contrastive_select(ctx, ctx_inv, S, hid, probs, alpha, score, sel):
    """see mxl_contrastive_select: ctx (B, Smax, d) bf16, ctx_inv (B, Smax) f32, hid (B*K, d) bf16, probs (B, K) f32"""
    B, K = probs.shape
    check(lib().mxl_contrastive_select(_p(ctx), ctx.stride(0), _p(ctx_inv), ctx_inv.stride(0), S, _p(hid), _p(probs), float(alpha),
                                       B, K, ctx.shape[-1], _p(score), _p(sel), _stream()), 'mxl_contrastive_select')
    return sel


CONTRASTIVE_MAX = 32     # candidates per sequence of mxl_contrastive_topk / mxl_contrastive_step / mxl_ring_slot_broadcast


def _contrastive_rows(what, probs, dead, sel, ids, unfinished):
    """(B, K) of a contrastive launch from probs (B, K) f32, with the shapes and types of the other per-row tensors checked"""
    _req(probs, torch.float32, f'{what} probs'); _req(dead, torch.int32, f'{what} dead'); _req(sel, torch.int32, f'{what} sel')
    if probs.dim() != 2 or not probs.is_contiguous():
        raise MusicXLError(f'{what}: probs must be contiguous (B, K) f32')
    B, K = probs.shape
    if K < 2 or K > CONTRASTIVE_MAX:
        raise MusicXLError(f'{what}: 2..{CONTRASTIVE_MAX} candidates per sequence, got {K}')
    if dead.numel() != B * K or not dead.is_contiguous() or sel.numel() != B or not sel.is_contiguous():
        raise MusicXLError(f'{what}: dead must be contiguous ({B}, {K}) int32 and sel ({B},) int32')
    if not ids.is_cuda or ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[0] != B * K or ids.stride(1) != 1:
        raise MusicXLError(f'{what}: ids must be ({B * K}, .) int64 device rows with unit column stride')
    if unfinished is not None:
        _req(unfinished, torch.int32, f'{what} unfinished')
        if unfinished.numel() != B * K or not unfinished.is_contiguous():
            raise MusicXLError(f'{what}: unfinished must be contiguous ({B * K},) int32, one word per row')
    return B, K


def contrastive_topk(logp, V, sel, ids, t_dev, probs, dead, unfinished=None, pad_id=0):
    """see mxl_contrastive_topk: the K = probs.shape[1] best tokens of logp[b*K + sel[b], :V] -> ids[b*K + k, t + 1], their softmax ->
    probs (B, K) f32, dead (B, K) int32; logp (B*K, >= V) f32, sel (B,) int32, unfinished (B*K,) int32 or None"""
    B, K = _contrastive_rows('contrastive_topk', probs, dead, sel, ids, unfinished)
    _req(logp, torch.float32, 'contrastive_topk logp')
    if logp.dim() != 2 or logp.shape[0] != B * K or logp.shape[1] < V or logp.stride(1) != 1:
        raise MusicXLError(f'contrastive_topk: logp must be ({B * K}, >= {V}) f32 with unit column stride')
    check(lib().mxl_contrastive_topk(_p(logp), logp.stride(0), int(V), B, K, _p(sel), _p(ids), ids.stride(0), _p(t_dev), _p(probs),
                                     _p(dead), _p(unfinished), int(pad_id), _stream()), 'mxl_contrastive_topk')


def contrastive_step(ctx, ctx_inv, t_dev, hid, probs, dead, alpha, score, sel, ids, unfinished=None, n_done=None, eos_id=-1, pad_id=0,
                     stop_later=False):
    """see mxl_contrastive_step: ctx (B, Smax, d) bf16 and ctx_inv (B, Smax) f32 (read below position t, written at it), hid (B*K, d)
    bf16, probs / dead (B, K), score (B*K,) f32 and sel (B,) int32 out, the picked token -> ids[b*K .. b*K + K-1, t]; unfinished (B*K,)
    int32 or None, n_done (1,) int32 or None; stop_later: rules_advance with the stop group follows and clears `unfinished` itself"""
    B, K = _contrastive_rows('contrastive_step', probs, dead, sel, ids, unfinished)
    _req(ctx, torch.bfloat16, 'contrastive_step ctx'); _req(hid, torch.bfloat16, 'contrastive_step hid')
    _req(ctx_inv, torch.float32, 'contrastive_step ctx_inv'); _req(score, torch.float32, 'contrastive_step score')
    d = hid.shape[-1]
    if ctx.dim() != 3 or ctx.shape[0] != B or ctx.shape[2] != d or ctx.stride(2) != 1 or ctx.stride(1) != d:
        raise MusicXLError(f'contrastive_step: ctx must be ({B}, Smax, {d}) bf16 with contiguous positions')
    if tuple(ctx_inv.shape) != (B, ctx.shape[1]) or ctx_inv.stride(1) != 1:
        raise MusicXLError(f'contrastive_step: ctx_inv must be ({B}, {ctx.shape[1]}) f32 with unit column stride')
    if tuple(hid.shape) != (B * K, d) or not hid.is_contiguous() or score.numel() != B * K or not score.is_contiguous():
        raise MusicXLError(f'contrastive_step: hid must be contiguous ({B * K}, {d}) bf16 and score ({B * K},) f32')
    if n_done is not None:
        _req(n_done, torch.int32, 'contrastive_step n_done')
    check(lib().mxl_contrastive_step(_p(ctx), ctx.stride(0), _p(ctx_inv), ctx_inv.stride(0), ctx.shape[1], _p(t_dev), _p(hid), _p(probs),
                                     _p(dead), float(alpha), B, K, d, _p(score), _p(sel), _p(ids), ids.stride(0), _p(unfinished),
                                     _p(n_done), int(eos_id), int(pad_id), int(bool(stop_later)), _stream()), 'mxl_contrastive_step')


def ring_slot_broadcast(rings, K, t_dev, sel, table=None):
    """see mxl_ring_slot_broadcast: rings = a list of contiguous (rows, H, M, dh) bf16 tensors of one shape with `table`, their
    addresses (beam_table); slot t mod M of row b*K + sel[b] -> the other K - 1 rows of sequence b, one launch for all"""
    first = rings[0]
    _req(sel, torch.int32, 'ring_slot_broadcast sel')
    if first.dim() != 4 or K < 2 or K > CONTRASTIVE_MAX or first.shape[0] % K or sel.numel() != first.shape[0] // K:
        raise MusicXLError(f'ring_slot_broadcast: (rows, H, M, dh) rings of K = 2..{CONTRASTIVE_MAX} rows per sequence and sel (rows / K,)')
    for t in rings:
        if not t.is_cuda or not t.is_contiguous() or t.shape != first.shape or t.dtype != torch.bfloat16 or t.data_ptr() % 16:
            raise MusicXLError('ring_slot_broadcast: the rings must be contiguous bf16 device tensors of one shape, 16-byte aligned')
    if table is None:
        table = beam_table(rings)
    if table.dtype != torch.int64 or table.numel() != len(rings) or not table.is_cuda:
        raise MusicXLError('ring_slot_broadcast: the table must hold one device address per ring (beam_table)')
    rows, H, M, dh = first.shape
    check(lib().mxl_ring_slot_broadcast(_p(table), len(rings), rows // K, int(K), H, M, dh, _p(t_dev), _p(sel), _stream()),
          'mxl_ring_slot_broadcast')


def kv_stash(qkv, stash, rrb=None, qr_out=None):
    """see mxl_kv_stash: the k / v thirds of the (B, 3d) bf16 qkv rows -> stash (B, 2d) bf16, one layer's slice of the stash that
    kv_commit_shared reads; with `rrb` (d f32) and `qr_out` (B, d) bf16 the same launch writes q + r_r_bias as kv_append does"""
    _req(qkv, torch.bfloat16, 'kv_stash qkv'); _req(stash, torch.bfloat16, 'kv_stash stash')
    B, d = stash.shape[0], stash.shape[-1] // 2
    if stash.dim() != 2 or tuple(qkv.shape) != (B, 3 * d) or not qkv.is_contiguous() or not stash.is_contiguous():
        raise MusicXLError('kv_stash: expected contiguous (B, 3d) qkv rows and a (B, 2d) stash')
    check(lib().mxl_kv_stash(_p(qkv), _p(stash), B, d, _p(rrb), _p(qr_out), _stream()), 'mxl_kv_stash')


def relattn_decode_shared_lds_bytes(K: int, dh: int, M: int, pieces: int = 1) -> int:
    """shared memory of one mxl_relattn_decode_shared workgroup (0: arguments outside its domain); the launch takes up to
    SHARED_LDS_MAX bytes"""
    return int(lib().mxl_relattn_decode_shared_lds_bytes(int(K), int(dh), int(M), int(pieces)))


SHARED_LDS_MAX = 160 * 1024


def relattn_decode_shared(qkv, kc, vc, rd, rwb, rrb, out, t_dev, K, H, dh, qr_buf, bd_buf, scale=None, qr_ready=False, split=None,
                          pieces=1, unfinished=None):
    """relattn_decode for the K candidate rows of every prompt over the prompt's one ring (mxl_relattn_decode_shared): kc / vc
    (B0, H, M, dh), everything per row -- qkv, qr_buf, bd_buf, out, unfinished and the split scratch -- sized for B0 * K rows.  The BD
    launch is relattn_decode's; slot t mod M of every row comes from its own qkv row."""
    B0, _, M, _ = kc.shape
    B, d = B0 * K, H * dh
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    if tuple(qkv.shape) != (B, 3 * d) or tuple(out.shape) != (B, d) or not qkv.is_contiguous() or not out.is_contiguous():
        raise MusicXLError(f'relattn_decode_shared: expected contiguous ({B}, {3 * d}) qkv and ({B}, {d}) out for {B0} rings x {K} rows')
    if not kc.is_contiguous() or not vc.is_contiguous() or vc.shape != kc.shape or bd_buf.numel() < B * H * M:
        raise MusicXLError('relattn_decode_shared: the rings must be contiguous (B0, H, M, dh) and bd_buf hold (B0 * K, H, M) f32')
    if not qr_ready:
        add_rowbias(qkv, 3 * d, 3 * d, rrb.reshape(-1), qr_buf, B, 1, d)
    if dh == 64 and B <= 64:
        check(lib().mxl_decode_bd(_p(qr_buf), _p(rd), _p(bd_buf), B, H, dh, M, d, rd.stride(0), _stream()), 'mxl_decode_bd')
    else:
        gemm_batched(qr_buf, rd, bd_buf, B, M, dh, lda=d, ldb=d, ldc=H * M, flags=GEMM_OUT_F32, batch=H, bdiv=1,
                     sA=(dh, 0), sB=(dh, 0), sC=(M, 0))
    if unfinished is not None:
        _req(unfinished, torch.int32, 'relattn_decode_shared unfinished')
        if unfinished.numel() != B:
            raise MusicXLError(f'relattn_decode_shared: unfinished must hold one word per row, {B}')
    n = pieces if (split is not None and pieces > 1) else 1
    check(lib().mxl_relattn_decode_shared(_p(qkv), _p(kc), _p(vc), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), B0, int(K), H, dh, M,
                                          float(scale), n, _p(split[0]) if n > 1 else 0, _p(split[1]) if n > 1 else 0,
                                          _p(unfinished), _stream()), 'mxl_relattn_decode_shared')


def kv_commit_shared(rings, stash, K, t_dev, sel, table=None):
    """see mxl_kv_commit_shared: rings = the K rings of every layer, then the V rings, contiguous (B0, H, M, dh) bf16 of one shape,
    with `table`, their addresses (beam_table); stash (layers, B0 * K, 2d) bf16 as kv_stash left it.  The stash of row b*K + sel[b]
    -> slot t mod M of ring b, one launch for all layers"""
    first = rings[0]
    _req(sel, torch.int32, 'kv_commit_shared sel'); _req(stash, torch.bfloat16, 'kv_commit_shared stash')
    if first.dim() != 4 or len(rings) % 2 or K < 2 or K > CONTRASTIVE_MAX or sel.numel() != first.shape[0] or not sel.is_contiguous():
        raise MusicXLError(f'kv_commit_shared: K then V rings (B0, H, M, dh), K = 2..{CONTRASTIVE_MAX} rows per ring and sel (B0,)')
    for t in rings:
        if not t.is_cuda or not t.is_contiguous() or t.shape != first.shape or t.dtype != torch.bfloat16 or t.data_ptr() % 16:
            raise MusicXLError('kv_commit_shared: the rings must be contiguous bf16 device tensors of one shape, 16-byte aligned')
    B0, H, M, dh = first.shape
    L = len(rings) // 2
    if tuple(stash.shape) != (L, B0 * K, 2 * H * dh) or not stash.is_contiguous():
        raise MusicXLError(f'kv_commit_shared: the stash must be contiguous ({L}, {B0 * K}, {2 * H * dh}) bf16')
    if table is None:
        table = beam_table(rings)
    if table.dtype != torch.int64 or table.numel() != len(rings) or not table.is_cuda:
        raise MusicXLError('kv_commit_shared: the table must hold one device address per ring (beam_table)')
    check(lib().mxl_kv_commit_shared(_p(table), L, _p(stash), B0, int(K), H, M, dh, _p(t_dev), _p(sel), _stream()),
          'mxl_kv_commit_shared')


def _req_tail_rings(kt, vt, B, H, dh, what):
    """tail rings: contiguous (B, H, Mt, dh) bf16 pairs"""
    _req(kt, torch.bfloat16, what); _req(vt, torch.bfloat16, what)
    if kt.dim() != 4 or vt.shape != kt.shape or (kt.shape[0], kt.shape[1], kt.shape[3]) != (B, H, dh) or not kt.is_contiguous() \
            or not vt.is_contiguous():
        raise MusicXLError(f'{what}: the tail rings must be contiguous ({B}, {H}, Mt, {dh}) bf16, one row per sequence')


def kv_append_tail(qkv, kt, vt, t_dev, t0_dev, rrb=None, qr_out=None):
    """see mxl_kv_append_tail: kt / vt head-major tail rings (B, H, Mt, dh); the k / v of the (B, 3d) qkv rows -> tail slot
    (t - t0) mod Mt, t and t0 (the prompt length) read on the device; with `rrb` (H*dh f32) and `qr_out` (B, H*dh) bf16 the same launch
    writes q + r_r_bias as kv_append does"""
    _req(qkv, torch.bfloat16, 'kv_append_tail qkv'); _req(t0_dev, torch.int32, 'kv_append_tail t0_dev')
    if kt.dim() != 4:
        raise MusicXLError('kv_append_tail: the tail rings must be (B, H, Mt, dh)')
    B, H, Mt, dh = kt.shape
    _req_tail_rings(kt, vt, B, H, dh, 'kv_append_tail')
    if tuple(qkv.shape) != (B, 3 * H * dh) or not qkv.is_contiguous():
        raise MusicXLError(f'kv_append_tail: expected contiguous ({B}, {3 * H * dh}) qkv rows')
    check(lib().mxl_kv_append_tail(_p(qkv), _p(kt), _p(vt), _p(t_dev), _p(t0_dev), B, Mt, H * dh, dh, _p(rrb), _p(qr_out), _stream()),
          'mxl_kv_append_tail')


def relattn_decode_prefix_lds_bytes(n: int, dh: int, M: int, pieces: int = 1) -> int:
    """shared memory of one mxl_relattn_decode_prefix workgroup (0: arguments outside its domain); the launch takes up to
    SHARED_LDS_MAX bytes"""
    return int(lib().mxl_relattn_decode_prefix_lds_bytes(int(n), int(dh), int(M), int(pieces)))


def prefix_attn_groups(n: int) -> int:
    """workgroups per (prompt, head, ring piece) of mxl_relattn_decode_prefix: groups of 8 rows, one group of 4 for n <= 4"""
    return 1 if n <= 4 else (n + 7) // 8


def relattn_decode_prefix(qkv, kp, vp, kt, vt, rd, rwb, rrb, out, t_dev, t0_dev, n, H, dh, qr_buf, bd_buf, scale=None, qr_ready=False,
                          split=None, pieces=1, unfinished=None):
    """relattn_decode for the n rows of every prompt over the prompt's rings kp / vp (B0, H, M, dh) and every row's own tail rings
    kt / vt (B0 * n, H, Mt, dh) (mxl_relattn_decode_prefix): a slot whose position is t0 or later comes from the row's tail.
    Everything per row -- qkv, qr_buf, bd_buf, out, unfinished and the split scratch -- is sized for B0 * n rows.  The BD launch is
    relattn_decode's."""
    B0, _, M, _ = kp.shape
    B, d = B0 * n, H * dh
    scale = scale if scale is not None else 1.0 / math.sqrt(dh)
    if tuple(qkv.shape) != (B, 3 * d) or tuple(out.shape) != (B, d) or not qkv.is_contiguous() or not out.is_contiguous():
        raise MusicXLError(f'relattn_decode_prefix: expected contiguous ({B}, {3 * d}) qkv and ({B}, {d}) out for {B0} prompts x {n} rows')
    if tuple(kp.shape) != (B0, H, M, dh) or not kp.is_contiguous() or not vp.is_contiguous() or vp.shape != kp.shape \
            or bd_buf.numel() < B * H * M:
        raise MusicXLError('relattn_decode_prefix: the prompt rings must be contiguous (B0, H, M, dh) and bd_buf hold (B0 * n, H, M) f32')
    _req_tail_rings(kt, vt, B, H, dh, 'relattn_decode_prefix')
    _req(t0_dev, torch.int32, 'relattn_decode_prefix t0_dev')
    if not qr_ready:
        add_rowbias(qkv, 3 * d, 3 * d, rrb.reshape(-1), qr_buf, B, 1, d)
    if dh == 64 and B <= 64:
        check(lib().mxl_decode_bd(_p(qr_buf), _p(rd), _p(bd_buf), B, H, dh, M, d, rd.stride(0), _stream()), 'mxl_decode_bd')
    else:
        gemm_batched(qr_buf, rd, bd_buf, B, M, dh, lda=d, ldb=d, ldc=H * M, flags=GEMM_OUT_F32, batch=H, bdiv=1,
                     sA=(dh, 0), sB=(dh, 0), sC=(M, 0))
    if unfinished is not None:
        _req(unfinished, torch.int32, 'relattn_decode_prefix unfinished')
        if unfinished.numel() != B:
            raise MusicXLError(f'relattn_decode_prefix: unfinished must hold one word per row, {B}')
    np_ = pieces if (split is not None and pieces > 1) else 1
    check(lib().mxl_relattn_decode_prefix(_p(qkv), _p(kp), _p(vp), _p(kt), _p(vt), _p(bd_buf), _p(rwb), _p(out), _p(t_dev), _p(t0_dev),
                                          B0, int(n), H, dh, M, kt.shape[2], float(scale), np_, _p(split[0]) if np_ > 1 else 0,
                                          _p(split[1]) if np_ > 1 else 0, _p(unfinished), _stream()), 'mxl_relattn_decode_prefix')


# ------------------------------------------------------------------ reformer
def axial_embed_fwd(ids, E, W0, W1, out, A0, A1, drop_p=0.0, seed=0, site_emb=0, site_pos=1):
    B, T = ids.shape
    d, d0 = E.shape[1], W0.shape[-1]
    check(lib().mxl_axial_embed_fwd(_p(ids), _p(E), _p(W0), _p(W1), _p(out), B, T, d, E.shape[0], A0, A1, d0, float(drop_p),
                                    seed, site_emb, site_pos, _stream()), 'mxl_axial_embed_fwd')
    return out


def axial_embed_bwd(ids, dout, dE, dW0, dW1, A0, A1, drop_p=0.0, seed=0, site_emb=0, site_pos=1, dout2=None):
    B, T = ids.shape
    d, d0 = dE.shape[1], dW0.shape[-1]
    check(lib().mxl_axial_embed_bwd(_p(ids), _p(dout), _p(dout2), _p(dE), _p(dW0), _p(dW1), B, T, d, dE.shape[0], A0, A1, d0,
                                    float(drop_p), seed, site_emb, site_pos, _stream()), 'mxl_axial_embed_bwd')


def lsh_hash(qk, bs, rs, rotations, buckets, B, T, H, dh, n_h, factors):
    arr = (C.c_int * len(factors))(*factors)
    check(lib().mxl_lsh_hash(_p(qk), bs, rs, _p(rotations), _p(buckets), B, T, H, dh, n_h, len(factors),
                             C.cast(arr, C.c_void_p), _stream()), 'mxl_lsh_hash')
    return buckets


def lsh_sort(buckets, sorted_idx, sorted_pos, BH, S, T, n_buckets_total):
    check(lib().mxl_lsh_sort(_p(buckets), _p(sorted_idx), _p(sorted_pos), BH, S, T, n_buckets_total, _stream()), 'mxl_lsh_sort')


def chunk_attn_fwd(q, k, v, spos, out, lse, B, T, H, dh, n_h, lsh, bs, rs, drop_p=0.0, seed=0, site=0):
    check(lib().mxl_chunk_attn_fwd(_p(q), _p(k), _p(v), _p(spos), _p(out), _p(lse), B, T, H, dh, n_h, int(lsh), bs, rs,
                                   float(drop_p), seed, site, _stream()), 'mxl_chunk_attn_fwd')


def chunk_attn_bwd(q, k, v, spos, out, lse, dout, dlse, dq, dk, dv, B, T, H, dh, n_h, lsh, bs, rs, drop_p=0.0, seed=0, site=0,
                   dq16=None, dk16=None, dv16=None, ld16=0):
    """dq / dk / dv: f32 (B, n_h, T, d), one slab per hash round, every element written once (may be None when the matching bf16
    destination is given; n_h == 1 only)"""
    check(lib().mxl_chunk_attn_bwd(_p(q), _p(k), _p(v), _p(spos), _p(out), _p(lse), _p(dout), _p(dlse), _p(dq), _p(dk), _p(dv),
                                   _p(dq16), _p(dk16), _p(dv16), int(ld16),
                                   B, T, H, dh, n_h, int(lsh), bs, rs, float(drop_p), seed, site, _stream()),
          'mxl_chunk_attn_bwd')


def lsh_keynorm_bwd(qk, bs, rs, dq, dk_eff, dqk, B, T, H, dh, ld_dqk=None):
    check(lib().mxl_lsh_keynorm_bwd(_p(qk), bs, rs, _p(dq), _p(dk_eff), _p(dqk), int(ld_dqk or H * dh), B, T, H, dh, _stream()),
          'mxl_lsh_keynorm_bwd')


def lsh_keynorm_bwd_rounds(qk, bs, rs, dq, dk_eff, dv, dqk, dv16, B, T, H, dh, n_h, ld_dqk=None, ld_dv=None):
    """lsh_keynorm_bwd over per-round slabs (B, n_h, T, d) f32; dv (optional) summed over the rounds into dv16 (bf16)"""
    check(lib().mxl_lsh_keynorm_bwd_rounds(_p(qk), bs, rs, _p(dq), _p(dk_eff), _p(dv), _p(dqk), int(ld_dqk or H * dh), _p(dv16),
                                           int(ld_dv or H * dh), B, T, H, dh, n_h, _stream()), 'mxl_lsh_keynorm_bwd_rounds')


def lsh_combine(out_r, lse, out, B, T, H, dh, n_h):
    check(lib().mxl_lsh_combine(_p(out_r), _p(lse), _p(out), B, T, H, dh, n_h, _stream()), 'mxl_lsh_combine')


def lsh_combine_bwd(out_r, lse, out, dout, dout_r, dlse, B, T, H, dh, n_h):
    check(lib().mxl_lsh_combine_bwd(_p(out_r), _p(lse), _p(out), _p(dout), _p(dout_r), _p(dlse), B, T, H, dh, n_h, _stream()),
          'mxl_lsh_combine_bwd')


# ------------------------------------------------------------------ Reformer cached decoding
def rf_decode_embed(ids, t, E, W0, W1, out, A1):
    B, d = out.shape
    check(lib().mxl_rf_decode_embed(_p(ids), ids.stride(0), t, _p(E), _p(W0), _p(W1), _p(out), B, d, E.shape[0], A1, W0.shape[-1],
                                    _stream()), 'mxl_rf_decode_embed')
    return out


def lsh_fix_buckets(buckets, rows, n_h, T, T_real, NB):
    check(lib().mxl_lsh_fix_buckets(_p(buckets), rows, n_h, T, T_real, NB, _stream()), 'mxl_lsh_fix_buckets')


def rf_query_bucket(raw, cache, bkmax, rows, n_h, NB, Tmax, t):
    check(lib().mxl_rf_query_bucket(_p(raw), _p(cache), _p(bkmax), rows, n_h, NB, Tmax, t, _stream()), 'mxl_rf_query_bucket')


def rf_decode_attn(q, kcache, vcache, sorted_idx, out, B, H, dh, n_h, Tmax, n, t, start=0, count=0, lsh=False):
    check(lib().mxl_rf_decode_attn(_p(q), q.stride(0), _p(kcache), _p(vcache), _p(sorted_idx), _p(out), B, H, dh, n_h, Tmax, n, t,
                                   start, count, int(lsh), _stream()), 'mxl_rf_decode_attn')
    return out
