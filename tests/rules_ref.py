"""The host reference of the COMPOSED rules of a generation, and the one-step sampler tail the rule tests drive: what the device's
rules_load / token_allowed / rules_move make of the groups together (include/musicxl.h, "Rules of a generation"), written once.  The
groups themselves are product code, tested on the CPU beside their features: TokenGrammar's tables, BarBudget, BarCount, KeyRule and
MelodyGuide of grammar.py, each with `allows` / `move` / `walk`.  Only their composition lives here -- `keep` (which tokens a row may
emit) and `move` (the row's words after a token) -- and tests/test_rules_ref_cpu.py ties both to those primitives token by token and
to the walkers on real streams.  Nothing here restates a rule's arithmetic: a primitive that judges a token by its class is evaluated
once per class (the budget once per distinct (class, slots) pair) and spread over the vocabulary through the `cls` table, the
automaton and the key rule are read from the tables they expose (`allow`, `KeyRule.allowed`).  A further rule adds a field to `Rules`
and `Words` and a line to each of `keep` and `move`."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from symbolic_music_generation_amd.grammar import KeyRule, TokenGrammar


class Rules(NamedTuple):
    """which groups are on.  grammar: the TokenGrammar whose tables the class-based groups read (its budget, bar_count and guide
    are taken from it); automaton / budget / count / guide: that group of the grammar is on (the device turns a group on by the
    words it is handed); key_rule: a KeyRule or None; stop: (eos, pad, min_length) or None"""
    grammar: Optional[TokenGrammar] = None
    automaton: bool = True
    budget: bool = False
    count: bool = False
    key_rule: Optional[KeyRule] = None
    guide: bool = False
    stop: Optional[tuple] = None

    @property
    def vocab_size(self) -> int:
        return self.grammar.vocab_size if self.grammar is not None else self.key_rule.vocab_size


class Words(NamedTuple):
    """the per-row words in RowRules.WORDS order, with the values RowRules.__init__ gives a rule that is off"""
    unfinished: int = 1
    gstate: int = 0
    gbar: int = 0
    grem: int = 0
    gleft: int = -1
    gkey: int = -1
    gpos: int = 0
    gforce: int = 0


def keep(rules: Rules, words: Words, V: int, guide_row=None, cur_len: Optional[int] = None) -> np.ndarray:
    """(V,) bool: the tokens a row at `words` may emit.  A row its guide feeds may emit that token alone, whatever the other groups
    say; otherwise the automaton, the budget, the count and the key must all admit the token, and min_length bars eos while cur_len
    (the row's length before the step) is below it.  A finished row is judged like a live one: the stop rule acts in `move`."""
    g = rules.grammar
    assert V == rules.vocab_size
    if rules.guide:
        f = g.guide.forced(words.gpos, words.gforce, () if guide_row is None else guide_row)
        if f >= 0:
            return np.arange(V) == f
    out = np.ones(V, dtype=bool)
    if g is not None:
        cls = g.cls.astype(np.int64)
        if rules.automaton:
            out &= ((int(g.allow[words.gstate]) >> cls) & 1) == 1
        if rules.budget:
            kinds, of = np.unique((cls << 16) | g.budget.slots.astype(np.int64), return_inverse=True)
            out &= np.array([g.budget.allows(words.gbar, words.grem, int(x) >> 16, int(x) & 0xFFFF) for x in kinds])[of.reshape(-1)]
        if rules.count:
            out &= np.array([g.bar_count.allows(words.gleft, c) for c in range(g.n_classes)])[cls]
    if rules.key_rule is not None:
        out &= rules.key_rule.allowed(words.gkey)
    if rules.stop is not None and cur_len is not None and cur_len < rules.stop[2] and 0 <= rules.stop[0] < V:
        out[rules.stop[0]] = False
    return out


def keep_rows(rules: Rules, rows_of_words, V: int, guides=None, cur_len: Optional[int] = None) -> torch.Tensor:
    """(B, V) bool: `keep` of every row; guides: one guide per row (None or empty = none)"""
    guides = [None] * len(rows_of_words) if guides is None else guides
    return torch.from_numpy(np.stack([keep(rules, w, V, g, cur_len) for w, g in zip(rows_of_words, guides)]))


def move(rules: Rules, words: Words, tok: int, glen: int = 0):
    """(token written, Words) after a row at `words` kept `tok`; glen: the length of the row's guide.  Under a stop rule a row that
    was finished before the step writes pad and keeps every word.  A live row moves every group that is on along the token -- an
    id beyond the vocabulary moves nothing -- and then the stop rule looks at the token: eos finishes the row."""
    tok, g, stop = int(tok), rules.grammar, rules.stop
    if stop is not None and not words.unfinished:
        return stop[1], words
    w = words
    if 0 <= tok < rules.vocab_size:
        if g is not None:
            c = int(g.cls[tok])
            if rules.automaton:
                w = w._replace(gstate=int(g.next[w.gstate, c]))
            if rules.budget:
                bar, rem = g.budget.move(w.gbar, w.grem, c, int(g.budget.slots[tok]), int(g.budget.bars[tok]))
                w = w._replace(gbar=bar, grem=rem)
            if rules.count:
                w = w._replace(gleft=g.bar_count.move(w.gleft, c))
            if rules.guide:
                pos, force = g.guide.move(w.gpos, w.gforce, glen, c)
                w = w._replace(gpos=pos, gforce=force)
        if rules.key_rule is not None:
            w = w._replace(gkey=rules.key_rule.move(w.gkey, tok))
    if stop is not None and tok == stop[0]:
        w = w._replace(unfinished=0)
    return tok, w


def host_allowed(grammar, Tp=0, n_bars=None, rule=None, keys=None, seen=None):
    """the `allowed` callable of generate.beam_search / group_beam_search / contrastive_search for these rules, from the host
    walkers: every row of ids[:, :cur_len] is walked from its start by TokenGrammar.walk, walk_budget, walk_bars (the generated
    part, from n_bars) and KeyRule.walk, and the words they end in admit what `keep` admits.  A row that a walk itself rejects (the
    kept -inf continuation of a dead row, the pads after a finished sequence's eos) is barred whole: it is dead, or emits pad, on
    either side.  seen: a list that receives the number of allowed tokens of every row of every step."""
    rules = Rules(grammar, budget=grammar is not None and grammar.budget is not None, count=grammar is not None and n_bars is not None,
                  key_rule=rule)
    V = rules.vocab_size

    def words_after(r, row):
        """the words the walkers leave row r in, or None where one of them rejects it"""
        w = Words()
        if grammar is not None:
            s, bad = grammar.walk(row)
            if bad >= 0:
                return None
            w = w._replace(gstate=s)
            if rules.budget:
                bar, rem, bad = grammar.walk_budget(row)
                if bad >= 0:
                    return None
                w = w._replace(gbar=bar, grem=rem)
            if rules.count:
                left, bad = grammar.walk_bars(row[Tp:], n_bars)
                if bad >= 0:
                    return None
                w = w._replace(gleft=left)
        if rule is not None:
            w = w._replace(gkey=rule.walk(row, -1 if keys is None else keys[r], len(row))[0])
        return w

    def allowed(ids):
        out = np.zeros((ids.shape[0], V), dtype=bool)
        for r, row in enumerate(ids.tolist()):
            w = words_after(r, row)
            if w is not None:
                out[r] = keep(rules, w, V)
        if seen is not None:
            seen.extend(out.sum(1).tolist())
        return torch.from_numpy(out)
    return allowed


# ---------------------------------------------------------------------------------------------------------------- device side
def i32(x, dev):
    return torch.tensor(x, device=dev, dtype=torch.int32)


def token_ids(vocab, text):
    return [vocab.t2i(t) for t in text.split()]


def fresh_generate(m, ids, **kw):
    """m.generate on a new decoder"""
    m._decoder = None
    return m.generate(input_ids=ids, **kw)


def tail(dev, fused, scores, sampling, t0, *, width, seed, gen_seed, fill, stop=None, unfinished=None, alive=None, **rules):
    """one sampler tail over `scores` (B, V) at position t0; fused: the one launch (ops.sample_step), else mask / sample / advance.
    Returns (tokens = ids[:, t0 + 1] and out_probs, both on the host, emb, ids, (t, rng, ctr), E).  The embedding table E (V, width)
    is drawn from a generator seeded gen_seed, ids (B, 8) starts filled with `fill`, `seed` is the sampler's, and `rules` are the
    rule keywords of ops.sample_step as they are -- or rules=, an ops.RuleState that holds them all, the stop group included.  The
    mask writes into `scores`, and the words given move in place."""
    from symbolic_music_generation_amd import ops
    if 'rules' not in rules:
        rules = dict(rules, stop=stop, unfinished=unfinished, alive=alive)
    assert 'rules' not in rules or (len(rules) == 1 and stop is None and unfinished is None and alive is None), 'rules= holds every group'
    mask = {k: v for k, v in rules.items() if k not in ('unfinished', 'alive')}
    n, vocab = scores.shape
    gen = torch.Generator(device=dev).manual_seed(gen_seed)
    E = torch.randn(vocab, width, device=dev, generator=gen).to(torch.bfloat16)
    emb = torch.zeros(n, width, device=dev, dtype=torch.bfloat16)
    ids = torch.full((n, 8), fill, device=dev, dtype=torch.int64)
    t, rng, ctr = i32([t0], dev), torch.zeros(1, device=dev, dtype=torch.int64), i32([0], dev)
    probs = torch.full((n, vocab), -1.0, device=dev)
    if fused:
        ops.sample_step(scores, vocab, ids, t, rng, seed, E, emb, 1.0, ctr, out_probs=probs, **rules, **sampling)
    else:
        ops.rules_mask(scores, vocab, t, **mask)
        ops.sample(scores, ids, t, rng, seed, out_probs=probs, **sampling)
        ops.decode_advance(t, rng)
        ops.rules_advance(ids, t, **rules)
    assert t.tolist() == [t0 + 1] and rng.tolist() == [1]
    return ids[:, t0 + 1].cpu(), probs.cpu(), emb, ids, (t, rng, ctr), E
