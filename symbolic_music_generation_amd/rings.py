"""The K/V ring layouts of generate.XLDecoder, one class per mode, each owning what is specific to it: checks, tensors, a layer's
projection, append and attention launches, how the rings follow a beam reorder and how a contrastive step settles its slot.
XLDecoder picks one from its arguments (`_layout`), builds it and asks it.  A further mode is a class here and an arm in `_layout`."""
from typing import Optional

import torch

from . import ops
from ._lib import MusicXLError

HEAD_WIDTHS = (16, 32, 64)          # what the byte rings and the kernels that serve several rows per ring take


def prompt_tail_len(mem_len: int, generated: int) -> int:
    """slots of a row's tail ring for `generated` positions after the prompt: that many rounded up to a multiple of 16, mem_len at most"""
    return min(mem_len, max(16, (int(generated) + 15) // 16 * 16))


def _project(dec, l: int, h_in):
    """the qkv projection of layer l as a launch of its own, where the append is not fused with it: h_in -> dec.qkv"""
    d = dec.eng.cfg.d_model
    (ops.gemm_skinny if dec.B <= 64 else ops.gemm)(h_in, dec.eng._lw(l, 'dec_attn.qkv_net.weight'), dec.qkv, dec.B, 3 * d, d)


class RingLayout:
    """Plain bf16 rings, and the base of the others: per layer one head-major pair kc / vc (B, H, M, dh), one ring per decoder row,
    for every entry point.  Below 65 rows projection, append and q + r_r_bias are one launch (mxl_decode_qkv); above, a GEMM and
    mxl_kv_append.  The attention reads through the decoder's owner table under beam_rings='indexed'."""
    SHOWN = ('kc', 'vc', 'ke', 've', 'kt', 'vt', 'stash', 't0_dev', 'Mt', 'shared_K', 'prompt_n', 'kv_dtype', 'pieces')   # XLDecoder's aliases
    kv_dtype = stash = t0_dev = Mt = None
    shared_K = prompt_n = 0
    unit = 1                        # decoder rows per ring: the prompt pass runs on every unit-th row, and lanes are cut between units
    serves = alone = None           # the one entry point the layout serves ('sample' / 'contrastive'; None: all), its word to the others
    movable = True                  # mxl_beam_reorder / mxl_ring_slot_broadcast / index_select over kc + vc move its rings

    def check(self, cfg, batch: int):
        """raises for arguments or a model the layout cannot serve"""

    def build(self, cfg, batch: int, dev):
        """checks; `pieces` per (ring, head) of the attention launch -- one workgroup per (head, ring, group of 8 rows of the ring, 4 up
        to 4 rows) and piece -- so that every CU streams the same bytes; the tensors, zeroed; `key`, the layout's part of a graph key"""
        self.check(cfg, batch)
        self.rows = batch // self.unit
        self.pieces = ops.decode_ring_pieces(self.rows * ops.prefix_attn_groups(self.unit), cfg.n_head, cfg.mem_len)
        self.ke = self.ve = self.kt = self.vt = []
        self.allocate(cfg, batch, dev)
        self.key = (type(self).__name__, self.unit, self.Mt)

    def allocate(self, cfg, batch: int, dev):
        self.kc, self.vc = self._pairs(cfg, self.rows, cfg.mem_len, dev)

    @staticmethod
    def _pairs(cfg, rows: int, slots: int, dev, dtype=torch.bfloat16, per_slot=True) -> tuple:
        shape = (rows, cfg.n_head, slots) + ((cfg.d_head,) if per_slot else ())
        return tuple([torch.zeros(shape, device=dev, dtype=dtype) for _ in range(cfg.n_layer)] for _ in range(2))

    def tensors(self) -> list:
        """every tensor a step may write and a prompt pass zeroes: what a capture snapshots"""
        return [*self.kc, *self.vc, *self.ke, *self.ve, *self.kt, *self.vt]

    def rings(self) -> list:
        """the K rings of every layer, then the V rings: what the ring movers and their address table take"""
        return [*self.kc, *self.vc]

    def kv_sink(self, l: int, qkv, Tp: int):
        """layer l's qkv rows of the prompt pass -> the rings"""
        ops.kv_fill(qkv, self.kc[l], self.vc[l], Tp)

    def check_prompt(self, x):
        """raises for prompts (B, Tp) whose every unit-th row does not stand for the rows after it"""

    def spread(self, src, dst):
        """a (B / unit, ...) result of the prompt pass -> the B decoder rows"""
        dst.copy_(src)

    def layer(self, dec, l: int, h_in, live, owned: dict):
        """projection, append at slot t mod M and ring attention of layer l for the token in h_in: dec.qkv, dec.qr -> dec.av"""
        q = self.query(dec, l, live)
        if dec.B <= 64:      # projection, ring append and q + r_r_bias in one launch
            ops.decode_qkv(h_in, dec.eng._lw(l, 'dec_attn.qkv_net.weight'), dec.qkv, self.kc[l], self.vc[l], dec.t_dev,
                           q['rrb'].reshape(-1), dec.qr, q['dh'])
        else:
            _project(dec, l, h_in)
            ops.kv_append(dec.qkv, self.kc[l], self.vc[l], dec.t_dev, rrb=q['rrb'].reshape(-1), qr_out=dec.qr)
        ops.relattn_decode(dec.qkv, self.kc[l], self.vc[l], **q, **owned)

    def query(self, dec, l: int, live) -> dict:
        """what every ring attention launch takes after its rings"""
        e, c = dec.eng, dec.eng.cfg
        return dict(rd=dec.rd[l], rwb=e._lw(l, 'dec_attn.r_w_bias', e.P), rrb=e._lw(l, 'dec_attn.r_r_bias', e.P), out=dec.av,
                    t_dev=dec.t_dev, H=c.n_head, dh=c.d_head, qr_buf=dec.qr, bd_buf=dec.bd, qr_ready=True, split=dec.split,
                    pieces=self.pieces, unfinished=live)

    def follow_beams(self, dec):
        """beam_rings='copied': whole ring rows follow their beams, one launch over the table of the rings"""
        ops.beam_reorder(self.rings(), dec._beam_args[0], dec.beam.beam_idx, dec.beam.moved, table=dec.ring_table)

    def admit_candidates(self, K: int):
        """raises for a contrastive search of K candidates the layout was not built for"""

    def settle(self, dec, K: int):
        """after the pick of a contrastive step of K candidates: the one slot the step wrote follows the pick in every ring"""
        ops.ring_slot_broadcast(self.rings(), K, dec.t_dev, dec.cs.sel, table=dec.ring_table)


class FP8Rings(RingLayout):
    """uint8 rings kc / vc (B, H, M, dh) of e4m3fn bytes with one int8 exponent per slot and head, ke / ve (B, H, M) ("FP8
    rings"): (dh + 1) / (2 dh) of the bf16 bytes; zero bytes with e = 0 are the zero memories.  Projection, then the quantising
    append (one launch more per layer than the fused bf16 form), then the fp8 reader, through the owner table under
    beam_rings='indexed'.  The ring movers know the bf16 layout alone: the searches that move rings refuse this one."""
    kv_dtype, movable = 'fp8', False

    def check(self, cfg, batch: int):
        if cfg.d_head not in HEAD_WIDTHS:
            raise MusicXLError(f'fp8 K/V rings need a head width of 16, 32 or 64, not {cfg.d_head}')

    def allocate(self, cfg, batch: int, dev):
        self.kc, self.vc = self._pairs(cfg, batch, cfg.mem_len, dev, torch.uint8)
        self.ke, self.ve = self._pairs(cfg, batch, cfg.mem_len, dev, torch.int8, per_slot=False)

    def kv_sink(self, l: int, qkv, Tp: int):
        ops.kv_fill_fp8(qkv, self.kc[l], self.ke[l], self.vc[l], self.ve[l], Tp)

    def layer(self, dec, l: int, h_in, live, owned: dict):
        q, four = self.query(dec, l, live), (self.kc[l], self.ke[l], self.vc[l], self.ve[l])
        _project(dec, l, h_in)
        ops.kv_append_fp8(dec.qkv, *four, dec.t_dev, rrb=q['rrb'].reshape(-1), qr_out=dec.qr)
        ops.relattn_decode_fp8(dec.qkv, *four, **q, **owned)

    def follow_beams(self, dec):
        """the tests' reference for indexed fp8 rings (XLDecoder.beam_begin), eager only: bytes and exponents follow their beams by
        index_select; the rows of an item with moved == 0 stay (its beam_idx is not valid)"""
        nb, rows = dec._beam_args[0], torch.arange(dec.B, device=dec.eng.dev)
        src = torch.where(dec.beam.moved.repeat_interleave(nb) != 0, dec.beam.beam_idx.to(torch.int64), rows)
        for ring in self.tensors():
            ring.copy_(ring.index_select(0, src))


class PerPromptRings(RingLayout):
    """What SharedRings and PromptRings share: one bf16 ring pair per prompt, kc / vc (B0, H, M, dh), filled by a prompt pass of the B0
    prompts and read by the prompt's `unit` rows, whose own k / v of a step go elsewhere (one launch more per layer than the fused form)"""
    what, takes, most, lds_bytes, mem16 = 'rings', '', 1 << 30, None, False

    def __init__(self, k: int):
        self.unit = k

    @classmethod
    def misfit(cls, cfg, k: int, rows: int) -> Optional[str]:
        """why a model cannot keep one ring per k rows in a decoder of `rows` rows (None: it can): the head width, mem_len % 16 where
        the kernel needs it, and the shared memory of the attention workgroup at the decoder's ring pieces"""
        M, dh = cfg.mem_len, cfg.d_head
        if dh not in HEAD_WIDTHS:
            return f'{cls.what} need a head width of 16, 32 or 64, not {dh}'
        if cls.mem16 and (M % 16 or M < 16):
            return f'{cls.what} take a mem_len that is a multiple of 16, not {M}'
        pieces = ops.decode_ring_pieces((rows // k) * ops.prefix_attn_groups(k), cfg.n_head, M)
        if not 0 < getattr(ops, cls.lds_bytes)(k, dh, M, pieces) <= ops.SHARED_LDS_MAX:
            return (f'{cls.what}: mem_len {M} in {pieces} piece(s) needs more than the {ops.SHARED_LDS_MAX >> 10} KiB of shared memory a '
                    f'workgroup of {8 if k > 4 else 4} queries has for its scores')
        return None

    def check(self, cfg, batch: int):
        if self.unit < 2 or self.unit > self.most or batch % self.unit:
            raise MusicXLError(self.takes)
        misfit = self.misfit(cfg, self.unit, batch)
        if misfit:
            raise MusicXLError(misfit)


class SharedRings(PerPromptRings):
    """shared_rings = K, for contrastive search alone: the K candidate rows of a prompt read its rings, and no ring is written before
    the pick -- the k / v of a step wait in a stash (L, B, 2d) and the picked row's become slot t mod M of the prompt's rings
    (csrc/decode_shared.hip).  The prompt's log-probabilities go to rows b * K, where mxl_contrastive_topk reads them (sel starts at 0)."""
    what, most, lds_bytes = 'shared rings', ops.CONTRASTIVE_MAX, 'relattn_decode_shared_lds_bytes'
    takes = f'shared rings take 2..{ops.CONTRASTIVE_MAX} candidates per prompt and one decoder row per candidate'
    serves, alone = 'contrastive', 'a decoder with shared rings serves contrastive search alone (contrastive_begin)'
    shared_K = property(lambda self: self.unit)

    def allocate(self, cfg, batch: int, dev):
        super().allocate(cfg, batch, dev)
        self.stash = torch.empty(cfg.n_layer, batch, 2 * cfg.d_model, device=dev, dtype=torch.bfloat16)

    def spread(self, src, dst):
        dst.zero_()
        dst[::self.unit].copy_(src)

    def layer(self, dec, l: int, h_in, live, owned: dict):
        q = self.query(dec, l, live)
        _project(dec, l, h_in)
        ops.kv_stash(dec.qkv, self.stash[l], rrb=q['rrb'].reshape(-1), qr_out=dec.qr)
        ops.relattn_decode_shared(dec.qkv, self.kc[l], self.vc[l], K=self.unit, **q)

    def admit_candidates(self, K: int):
        if K != self.unit:
            raise MusicXLError(f'the decoder shares a ring among {self.unit} candidates, the search has {K}')

    def settle(self, dec, K: int):
        ops.kv_commit_shared(self.rings(), self.stash, K, dec.t_dev, dec.cs.sel, table=dec.ring_table)


class PromptRings(PerPromptRings):
    """prompt_rings = n with tail_len, for sampling alone: the n rows of a prompt are variations of it.  The prompt rings are written
    by the prompt pass and never again; every row has a pair of tail rings kt / vt (B, H, Mt, dh) for the positions generated after
    the prompt (csrc/decode_prefix.hip), Mt = prompt_tail_len(M, tail_len), tail_len = the most positions a generation adds (None: a
    full ring); t0_dev holds the prompt length.  Every prompt comes n times in a row, and its log-probabilities go to all n rows."""
    what, lds_bytes, mem16 = 'prompt rings', 'relattn_decode_prefix_lds_bytes', True
    takes = 'prompt rings take 2 or more rows per prompt and one decoder row per variation'
    serves, alone = 'sample', 'a decoder with prompt rings serves sampling alone (begin / run), not a search'
    prompt_n = property(lambda self: self.unit)

    def __init__(self, n: int, tail_len: Optional[int] = None):
        self.unit, self.tail_len = n, tail_len

    def allocate(self, cfg, batch: int, dev):
        super().allocate(cfg, batch, dev)
        self.Mt = prompt_tail_len(cfg.mem_len, cfg.mem_len if self.tail_len is None else self.tail_len)
        self.kt, self.vt = self._pairs(cfg, batch, self.Mt, dev)
        self.t0_dev = torch.zeros(1, device=dev, dtype=torch.int32)

    def check_prompt(self, x):
        if not bool((x.view(-1, self.unit, x.shape[1]) == x[::self.unit, None]).all()):
            raise MusicXLError(f'a decoder with prompt rings takes every prompt {self.unit} times in a row (repeat_interleave)')

    def spread(self, src, dst):
        dst.copy_(src.repeat_interleave(self.unit, 0))

    def layer(self, dec, l: int, h_in, live, owned: dict):
        q = self.query(dec, l, live)
        _project(dec, l, h_in)
        ops.kv_append_tail(dec.qkv, self.kt[l], self.vt[l], dec.t_dev, self.t0_dev, rrb=q['rrb'].reshape(-1), qr_out=dec.qr)
        ops.relattn_decode_prefix(dec.qkv, self.kc[l], self.vc[l], self.kt[l], self.vt[l], t0_dev=self.t0_dev, n=self.unit, **q)
