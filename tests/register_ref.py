"""The register rule beside the composed rules of tests/rules_ref.py: `keep` and `move` of a row under every group AND
grammar.RegisterRule, composed from rules_ref's and the rule's own primitives -- nothing of either is restated here.  A row its guide
feeds keeps that token alone, whatever the register says; otherwise the register's `allowed` comes on top of rules_ref.keep.  The move
is rules_ref.move followed by RegisterRule.move under the same condition: a row that was finished before the step keeps its words, an
id beyond the vocabulary moves nothing.  tests/test_register_rule_cpu.py ties both to the primitives token by token."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from symbolic_music_generation_amd.grammar import ANY_RANGE, NO_FLOOR, RegisterRule, pack_bounds
from tests import rules_ref
from tests.rules_ref import Rules, Words


class RegWords(NamedTuple):
    """the three register words of a row, with the values of an unconstrained row that has no open part"""
    bounds: tuple = ANY_RANGE
    gpart: int = 0
    gfloor: int = NO_FLOOR

    @property
    def grange(self) -> int:
        return pack_bounds(self.bounds)


# The rows of the device tests, whose words differ: an unconstrained row, gpart 0 / 1 / 2, floor 128, a floor below lo_bass (no
# pitched token is left), lo == hi, and the bounds 0 and 127.
EDGE_ROWS = [
    RegWords(ANY_RANGE, 2, 60),                       # unconstrained bounds: only the gap can bar
    RegWords((60, 72, 36, 55), 0, 50),                # no open part: untouched
    RegWords((60, 72, 36, 55), 1, NO_FLOOR),          # melody, no floor yet
    RegWords((60, 72, 36, 55), 2, 30),                # bass, the floor under lo_bass: no pitched token is left
    RegWords((64, 64, 40, 40), 2, NO_FLOOR),          # lo == hi, no floor
    RegWords((0, 127, 0, 127), 2, 0),                 # the bounds 0 and 127, the floor at 0
]


def keep(rules: Rules, words: Words, reg: RegisterRule, rw: RegWords, gap: int, V: int, guide_row=None, cur_len: Optional[int] = None):
    """(V,) bool: the tokens a row may emit under `rules` and the register rule"""
    if rules.grammar is not None or rules.key_rule is not None:
        out = rules_ref.keep(rules, words, V, guide_row, cur_len)
    else:                  # the register group alone: rules_ref.keep sizes the vocabulary by a table of the others; min_length is left
        out = np.ones(V, dtype=bool)
        if rules.stop is not None and cur_len is not None and cur_len < rules.stop[2] and 0 <= rules.stop[0] < V:
            out[rules.stop[0]] = False
    if rules.guide and rules.grammar.guide.forced(words.gpos, words.gforce, () if guide_row is None else guide_row) >= 0:
        return out
    return out & reg.allowed(rw.gpart, rw.gfloor, rw.bounds, gap)


def keep_rows(rules: Rules, rows_of_words, reg: RegisterRule, rows_of_reg, gap: int, V: int, guides=None, cur_len=None) -> torch.Tensor:
    guides = [None] * len(rows_of_words) if guides is None else guides
    return torch.from_numpy(np.stack([keep(rules, w, reg, rw, gap, V, g, cur_len) for w, rw, g in zip(rows_of_words, rows_of_reg, guides)]))


def move(rules: Rules, words: Words, reg: RegisterRule, rw: RegWords, tok: int, glen: int = 0):
    """(token written, Words, RegWords) after the row kept `tok`"""
    tok, stop = int(tok), rules.stop
    live = stop is None or bool(words.unfinished)
    if rules.grammar is not None or rules.key_rule is not None:
        out, w = rules_ref.move(rules, words, tok, glen)
    else:                                                            # the register group alone: only the stop rule beside it
        out, w = (tok, words) if live else (stop[1], words)
        if live and stop is not None and tok == stop[0]:
            w = w._replace(unfinished=0)
    if live and 0 <= tok < reg.vocab_size:
        part, floor = reg.move(rw.gpart, rw.gfloor, tok)
        rw = rw._replace(gpart=part, gfloor=floor)
    return out, w, rw


def host_allowed(grammar, reg: RegisterRule, bounds, gap: int, Tp=0, n_bars=None, rule=None, keys=None):
    """rules_ref.host_allowed with the register rule on top: every row of ids[:, :cur_len] is walked by RegisterRule.walk (nothing
    judged: the search only ever extends rows it allowed) and the words it ends in admit what `allowed` admits.  bounds: one
    (lo_melody, hi_melody, lo_bass, hi_bass) per row of ids"""
    base = rules_ref.host_allowed(grammar, Tp, n_bars, rule, keys) if (grammar is not None or rule is not None) else None

    def allowed(ids):
        out = base(ids) if base is not None else torch.ones(ids.shape[0], reg.vocab_size, dtype=torch.bool)
        for r, row in enumerate(ids.tolist()):
            part, floor, _ = reg.walk(row, bounds[r], gap, check_from=len(row))
            out[r] &= torch.from_numpy(reg.allowed(part, floor, bounds[r], gap))
        return out
    return allowed


def device_words(rows_of_reg, dev):
    """(grange, gpart, gfloor) int32 device tensors of the rows"""
    return (rules_ref.i32([rw.grange for rw in rows_of_reg], dev), rules_ref.i32([rw.gpart for rw in rows_of_reg], dev),
            rules_ref.i32([rw.gfloor for rw in rows_of_reg], dev))
