"""`generate.contrastive_search(..., allowed=)` on the CPU, over the oracle decoder of tests/test_beam_cpu.py.  The routine calls two
kernels itself (the context norms and the candidate re-ranking), which have no CPU form: fp32 torch restatements stand in for them
here, so what is tested is the host logic -- the mask before the top-k, dead candidates, the stop rule -- not the kernels
(tests/test_contrastive_ops_gpu.py).  Then the C ABI of the device path: the header, the library and what ops.py binds agree, and the
entries refuse bad arguments before any launch."""
import re
from types import SimpleNamespace

import pytest
import torch

from oracle.transfoxl_ref import RefTransfoXLLMHeadModel, RefXLConfig
from symbolic_music_generation_amd import _lib, generate, ops
from tests.test_beam_cpu import _OracleDecoder

V, TP, L, K = 64, 5, 14, 4


class _OracleContrastiveDecoder(_OracleDecoder):
    """the beam hooks of the oracle decoder plus what contrastive_search reads of an XLDecoder: the last-layer hidden states of the
    prompt pass (eng._last.h) and of the last step (h)"""

    def __init__(self, model, rows, max_total_len):
        super().__init__(model, rows, max_total_len)
        self.eng.cfg.n_layer = model.config.n_layer
        self.eng.cfg.d_model = model.config.d_model

    def _forward(self, x, mems):
        hid, self.mems = self.model.transformer(x, mems=mems)
        self.logp = self.model.crit(hid[:, -1:], None).view(x.shape[0], -1)
        self.h = [hid[:, -1].contiguous()] * 2
        self.eng._last = SimpleNamespace(h=[hid.reshape(-1, hid.shape[-1])] * 2)


def _row_inv_norm(x, out, n):
    out.copy_(1.0 / x.float().norm(dim=-1))
    return out


def _contrastive_select(ctx, ctx_inv, S, hid, probs, alpha, score, sel):
    B, Kc = probs.shape
    h = hid.float().view(B, Kc, -1)
    cos = torch.einsum('bsd,bkd->bks', ctx[:, :S].float() * ctx_inv[:, :S, None], h / h.norm(dim=-1, keepdim=True))
    sc = (1.0 - alpha) * probs - alpha * cos.max(-1).values
    score.copy_(sc.reshape(-1))
    sel.copy_(sc.argmax(-1))
    return sel


@pytest.fixture
def host_kernels(monkeypatch):
    monkeypatch.setattr(ops, 'row_inv_norm', _row_inv_norm)
    monkeypatch.setattr(ops, 'contrastive_select', _contrastive_select)


def _model_and_prompt(seed):
    torch.manual_seed(seed)
    cfg = RefXLConfig.from_preset('debug', vocab_size=V, max_length=32)
    model = RefTransfoXLLMHeadModel(cfg).eval()
    prompt = torch.randint(0, V, (2, TP), generator=torch.Generator().manual_seed(seed + 1))
    return model, prompt


def _search(model, prompt, **kw):
    dec = _OracleContrastiveDecoder(model, prompt.shape[0] * K, L)
    return generate.contrastive_search(dec, prompt, L, top_k=K, penalty_alpha=0.6, pad_token_id=0, **kw)


@torch.no_grad()
@pytest.mark.parametrize('eos', [-1, None])
def test_without_a_mask_nothing_changes(host_kernels, eos):
    model, prompt = _model_and_prompt(1)
    plain = _search(model, prompt, eos_token_id=eos)
    assert plain.shape == (2, L) and torch.equal(plain[:, :TP], prompt)
    # a mask that bars nothing takes the masked branches (fill, dead candidates, the first maximum again) to the same tokens
    calls = []

    def everything(ids):
        calls.append(tuple(ids.shape))
        return torch.ones(ids.shape[0], V, dtype=torch.bool)
    assert torch.equal(_search(model, prompt, eos_token_id=eos, allowed=everything), plain)
    assert calls == [(2 * K, t) for t in range(TP, L)]               # every row's history up to the step, once per step
    trace = []
    assert torch.equal(_search(model, prompt, eos_token_id=eos, trace=trace), plain)
    assert len(trace) == L - TP and all(live.all() and sg.shape == (2,) and (lg >= 0).all() for live, sg, lg in trace)


@torch.no_grad()
def test_barred_tokens_never_appear_and_dead_candidates_are_never_picked(host_kernels):
    model, prompt = _model_and_prompt(1)
    free = _search(model, prompt, eos_token_id=-1)
    # bar what the free run emits, and leave sequence 1 fewer tokens than candidates: two of its four are dead at every step
    barred = sorted(set(free[:, TP:].flatten().tolist()))
    few = [t for t in range(V) if t not in barred][:2]

    def allowed(ids):
        ok = torch.ones(ids.shape[0], V, dtype=torch.bool)
        ok[:, barred] = False
        ok[K:] = False
        ok[K:, few] = True
        return ok
    got = _search(model, prompt, eos_token_id=-1, allowed=allowed)
    assert got.shape == (2, L) and torch.equal(got[:, :TP], prompt)
    assert not set(got[0, TP:].tolist()) & set(barred)
    assert set(got[1, TP:].tolist()) <= set(few)
    # an eos among the allowed tokens still ends a sequence, which then emits pad
    end = _search(model, prompt, eos_token_id=int(got[1, TP + 2]), allowed=allowed)
    first = got[1, TP:].tolist().index(int(got[1, TP + 2]))
    assert end[1, TP:TP + first + 1].tolist() == got[1, TP:TP + first + 1].tolist() and (end[1, TP + first + 1:] == 0).all()


def test_header_library_and_ops_agree_on_the_contrastive_entries():
    decl = _lib.declared_functions()
    L_ = _lib.lib()
    src = open(ops.__file__).read()
    bound = set(re.findall(r'lib\(\)\.(mxl_\w+)', src))
    assert bound <= set(decl), sorted(bound - set(decl))             # ops.py binds nothing the header does not declare
    for name, n_args in (('mxl_contrastive_topk', 14), ('mxl_contrastive_step', 23), ('mxl_ring_slot_broadcast', 10)):
        assert name in decl and name in bound and len(decl[name][1]) == n_args and hasattr(L_, name)
    Pt = 4096                                                        # stands for a device pointer: nothing is followed before a launch
    topk = dict(logp=Pt, ldl=64, V=64, B=2, K=4, sel=Pt, ids=Pt, ld_ids=16, t_dev=Pt, probs=Pt, dead=Pt, unfinished=None, pad=0)
    for bad in (dict(K=1), dict(K=33), dict(ldl=63), dict(B=0), dict(sel=None), dict(dead=None), dict(ld_ids=0)):
        assert L_.mxl_contrastive_topk(*{**topk, **bad}.values(), None) == -1, bad
    step = dict(ctx=Pt, ctx_bs=16 * 8, inv=Pt, inv_bs=16, Smax=16, t_dev=Pt, hid=Pt, probs=Pt, dead=Pt, alpha=0.6, B=2, K=4, d=8, score=Pt,
                sel=Pt, ids=Pt, ld_ids=16, unfinished=None, n_done=None, eos=-1, pad=0, later=0)
    for bad in (dict(K=1), dict(K=33), dict(d=12), dict(ctx_bs=16 * 8 - 8), dict(inv_bs=15), dict(ctx=Pt + 2), dict(sel=None),
                dict(Smax=0)):
        assert L_.mxl_contrastive_step(*{**step, **bad}.values(), None) == -1, bad
    ring = dict(table=Pt, n=4, B=2, K=3, H=2, M=4, dh=8, t_dev=Pt, sel=Pt)
    for bad in (dict(table=None), dict(n=0), dict(K=1), dict(K=33), dict(dh=12), dict(M=0), dict(B=70000), dict(sel=None)):
        assert L_.mxl_ring_slot_broadcast(*{**ring, **bad}.values(), None) == -1, bad
