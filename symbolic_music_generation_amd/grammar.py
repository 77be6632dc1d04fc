"""Token grammars for constrained generation: a deterministic finite automaton over token CLASSES, small enough to sit in the
sampler launch (`model.generate(..., grammar=g)`; DESIGN.md, "Grammar-constrained decoding").

    cls    (V,)   uint8    token id -> class, C <= 32 classes
    allow  (S,)   uint32   bit c set <=> class c may be emitted in state s, S <= 256 states
    next   (S, C) uint8    successor state; entries of classes a state bars hold the state itself and are never followed

The host side (this module) builds and validates the tables and walks id sequences (`walk`, the reference the device kernels
are tested against); `to(device)` uploads them once.  Building a grammar needs no GPU.

`music_grammar(vocab)` is the grammar of the music token stream (`MusicVocabulary.grammar()` / `MusicTokenizer.grammar()`):

    song   := TimeSig Tempo [Key] bar+ </s> [PAD]*
    bar    := <bar> <melody> note* <bass> note*         (the bass channel closes the bar)
    note   := pitch duration | <tup> pitch pitch+ duration </tup>

It is SYNTACTIC: what `MusicConverter.str2score` needs to parse a stream.  It does not make the durations of a bar add up to the
time signature -- a stream that is broken only in its durations passes -- and it bans no rare token.

`music_grammar(vocab, bar_budget=True)` attaches a `BarBudget` (`grammar.budget`) that does: two integers per row ride on the
automaton, `bar` (the bar length in slots of 4 / 2**precision quarters, set by the TimeSig token; 0 = unconstrained) and `rem` (the
slots still free in the open channel).  Its tables sit beside the grammar's:

    slots      (V,)   uint16   duration token -> slots, 0 = not a duration, RARE_SLOTS = a duration of unknown length (d_rare)
    bars       (V,)   uint16   time signature token -> bar length in slots (0 = unconstrained), NO_SIG = not a time signature
    opens      class bit mask  classes that open a channel (<melody>, <bass>): rem = bar
    need_free  class bit mask  classes that start a note (pitch, <tup>): allowed only while rem > 0
    need_full  class bit mask  classes that close a channel (<bass>, <bar>, </s>): allowed only at rem == 0

and a duration of k slots is allowed only if k <= rem.  The rule looks at the token's class and the two integers alone, never at the
automaton state, so it needs no state of its own and composes with any mask the grammar applies.

Format of a `slots` entry s other than RARE_SLOTS: bits 0..14 are the slots the token TAKES (`slots_take`), and bit 15 (`NEED_ONE_MORE`)
says that it NEEDS one more free than it takes (`slots_need` = (s & 0x7FFF) + (s >> 15)): the token is allowed only if its need
<= rem, and moves rem by its take.  No base vocabulary sets bit 15 -- a duration is far below 0x8000 slots -- so their tables read as
they always did.  The bit is for `subword_grammar(base, pieces)`, the grammar of a sub-word tokenizer (`PairMergeTokenizer.grammar()`,
`WordPieceMusicTokenizer.grammar()`): a sub-word id stands for a fixed sequence of base tokens, so it induces a partial function on
the base automaton's states -- ids with the same function share a token class -- takes the sum of its durations' slots, and, where it
ends on an open note start (`pitch duration pitch`), needs one more, because the pitch it leaves open still needs a duration.

Both forms of the music grammar also carry a `BarCount` (`grammar.bar_count`), the rule behind `generate(..., n_bars=k)`: one more
integer per row, `left` = the bars the row may still open (negative = no limit, the row is untouched), and two class bit masks

    count      class bit mask  classes that open a bar (<bar>): barred at left == 0, a kept one takes 1 from a positive left
    end        class bit mask  classes that end the stream (</s>): barred while left > 0

Under the bar budget a row whose last bar is full may emit only <bar> or </s>, so the count decides which: the row ends exactly when
its k-th bar is full.  Without a budget the rule still bars a further bar and an early end, but nothing forces the end.

`KeyRule` (`MusicVocabulary.key_rule()` / `MusicTokenizer.key_rule()`) is the harmonic rule behind `generate(..., in_key=rule)`.  It
stands beside the grammar, not on it: one more integer per row, `key` = the ordinal of the row's key in `vocab.KEY_NAMES` (negative =
no key, the row is untouched), and three tables

    keys       (V,)   uint8    Key_* token -> ordinal, NO_KEY = any other token
    pcs        (V,)   uint8    pitch token -> pitch class 0..11, NO_PITCH = no pitch (rests and the rare pitch included)
    inkey      (24,)  uint16   bit pc set <=> pitch class pc belongs to the key (metrics.in_key_table, the table of the IKR metric)

A pitch outside the row's key is barred, and a kept Key_* token sets the row's key.  It reads neither token classes nor the automaton
state, so it needs no grammar and composes with all of the above.

`MelodyGuide` (`grammar.guide`; both forms of the music grammar carry one) is the rule behind `generate(..., melody=m)`: part of a
row's output is given, not chosen.  A guide is the concatenation of `<bar> <melody> notes <bass>` spans, one per bar; the row is fed
each span token by token and writes the bass under it.  Two more integers per row, `pos` = the next index into the row's guide and
`force` = 1 while the row is being fed, and two class bit masks

    enter      class bit mask  classes that open a guided span (<bar>): a free row that keeps one while guide tokens are left is
                               fed from then on; the token is the guide's own
    leave      class bit mask  classes that close a guided span (<bass>): a fed row that keeps one chooses freely from then on

A fed row may emit the guide's next token alone, whatever the grammar, the budget, the count and the key say -- `generate` checks the
guide against the grammar and the budget on the host -- and the bar count, set to the number of bars in the guide, ends the row.

`RegisterRule` (`MusicVocabulary.register_rule()` / `MusicTokenizer.register_rule()`) is the rule behind `generate(..., register=rule)`:
every part stays in its register, and the bass under the melody.  Like the key rule it stands beside the grammar: it reads neither
token classes nor the automaton state.  One table

    reg        (V,)   uint8    pitch token -> MIDI number 0..127; REG_MELODY / REG_BASS / REG_BAR = the <melody> / <bass> / <bar> token;
                               NO_PITCH = any other token (rests and the rare pitch included: they are never barred)

three integers per row -- `range` (the bounds lo_melody, hi_melody, lo_bass, hi_bass, inclusive MIDI numbers, one byte each from the
lowest, fixed for the generation), `part` (0 = no part is open, 1 = melody, 2 = bass) and `floor` (the lowest melody pitch of the open
bar, NO_FLOOR = none yet) -- and one number for the generation, `gap` (-1 = the bass is not tied to the melody).  A pitch outside the
bounds of the open part is barred; in the bass, with gap >= 0 and a floor, the upper bound is min(hi_bass, floor - gap): gap 0 lets the
bass touch the bar's lowest melody note, gap 1 keeps it strictly below.  The bound is per bar, not aligned in time: it is sufficient to
keep the parts from crossing, not necessary.  A part token sets `part`, <bar> clears `part` and `floor`, a melody pitch lowers `floor`.
No dead end: the rest and the rare pitch are never barred and belong to the grammar's class `pitch`, so wherever a pitch may follow a
token is left even when the bounds leave no pitched one.

`BarRepeat` (`grammar.repeat`; both forms of the music grammar carry one) is the rule behind `generate(..., form='AABA')`: song form.
A row's generated bars are the bars it opens after its prompt, numbered from 0; a plan says of each whether it is free (-1) or
repeats an earlier generated bar j, and a repeating bar is copied token by token out of the row's own output.  Three more integers per
row, `bars` = the bars opened so far, `copy` = the column of the row's ids the next token is copied from (-1 = the row chooses) and
`stop` = the column where the copy ends, the table `barcol` (the column of every generated bar's `enter` token, written as the row
goes), the same two class bit masks as the guide's

    enter      class bit mask  classes that open a bar (<bar>): the row records the column and, if the plan names a source, copies
                               from behind the source's own `enter` token
    leave      class bit mask  classes that close the melody (<bass>): under span 1 the copy ends with it

and one number for the generation, `span` (0 = the whole bar is repeated, 1 = its melody, under which the row writes a new bass).  A
copying row may emit the one token of its history, whatever the other rules say, exactly as a guided row; the bar count, set to the
length of the plan, ends the row.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAX_CLASSES = 32
MAX_STATES = 256
RARE_SLOTS = 0xFFFF        # `slots` entry of a duration token of unknown length: barred in a constrained bar
NEED_ONE_MORE = 0x8000     # bit 15 of a `slots` entry other than RARE_SLOTS: the token needs one slot more free than it takes
NO_SIG = 0xFFFF            # `bars` entry of a token that is no time signature
NO_KEY = 0xFF              # `keys` entry of a token that is no key token
NO_PITCH = 0xFF            # `pcs` entry of a token that is no pitch
N_KEYS = 24
REG_MELODY, REG_BASS, REG_BAR = 0x80, 0x81, 0x82   # `reg` entries of the tokens that move a row's part
NO_FLOOR = 128             # `floor` of a row whose open bar holds no melody pitch yet
ANY_RANGE = (0, 127, 0, 127)                       # the bounds of an unconstrained row


class TokenGrammar:
    def __init__(self, cls, allow, next, start: int = 0, accepting: Optional[Iterable[int]] = None,
                 class_names: Optional[Sequence[str]] = None, state_names: Optional[Sequence[str]] = None):
        """cls (V,) token -> class; allow (S,) class bit masks; next (S, C) successor states; `accepting`: states in which a
        stream may end (informative: `accepts`).  Raises ValueError when the sizes are out of range or when a state that can be
        reached from `start` allows no class that has a token: the sampler must never face a row with every token barred."""
        cls_a = np.asarray(cls)
        next_a = np.asarray(next)
        allow_a = np.asarray(allow)
        if cls_a.ndim != 1 or cls_a.size == 0:
            raise ValueError('cls must be a non-empty 1-D array (token id -> class)')
        if next_a.ndim != 2 or allow_a.ndim != 1 or allow_a.shape[0] != next_a.shape[0]:
            raise ValueError('allow must be (S,) and next (S, C)')
        S, C = next_a.shape
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f'{C} token classes: a grammar has 1..{MAX_CLASSES} (one bit each in a 32-bit allow mask)')
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f'{S} states: a grammar has 1..{MAX_STATES} (a state is one byte of the next table)')
        if cls_a.min() < 0 or cls_a.max() >= C:
            raise ValueError(f'cls holds a class outside 0..{C - 1}')
        if next_a.min() < 0 or next_a.max() >= S:
            raise ValueError(f'next holds a state outside 0..{S - 1}')
        if int(allow_a.min()) < 0 or int(allow_a.max()) >> C:
            raise ValueError(f'allow has a bit set beyond class {C - 1}')
        if not 0 <= int(start) < S:
            raise ValueError(f'start state {start} outside 0..{S - 1}')
        self.cls = np.ascontiguousarray(cls_a, dtype=np.uint8)
        self.allow = np.ascontiguousarray(allow_a, dtype=np.uint32)
        self.next = np.ascontiguousarray(next_a, dtype=np.uint8)
        self.start = int(start)
        self.accepting = frozenset(int(s) for s in accepting) if accepting is not None else None
        if self.accepting is not None and any(not 0 <= s < S for s in self.accepting):
            raise ValueError('accepting holds a state outside the table')
        self.class_names = list(class_names) if class_names is not None else [str(c) for c in range(C)]
        self.state_names = list(state_names) if state_names is not None else [str(s) for s in range(S)]
        if len(self.class_names) != C or len(self.state_names) != S:
            raise ValueError('class_names / state_names do not match the tables')
        # entries of barred classes are never followed: make them self loops so that a look-up is always in range and harmless
        for s in range(S):
            for c in range(C):
                if not (int(self.allow[s]) >> c) & 1:
                    self.next[s, c] = s
        self.populated = 0                               # bit c set <=> class c has at least one token
        for c in np.unique(self.cls).tolist():
            self.populated |= 1 << int(c)
        for s in self.reachable():
            if not int(self.allow[s]) & self.populated:
                raise ValueError(f'state {self.state_names[s]} can be reached from the start state and allows no class that has '
                                 'a token: generation would face a row with every token barred')
        self._dev: Dict[str, tuple] = {}
        self.budget: Optional['BarBudget'] = None        # the duration budget riding on this grammar (BarBudget attaches itself)
        self.bar_count: Optional['BarCount'] = None      # the bar count rule of generate(n_bars=) (BarCount attaches itself)
        self.guide: Optional['MelodyGuide'] = None       # the guide rule of generate(melody=) (MelodyGuide attaches itself)
        self.repeat: Optional['BarRepeat'] = None        # the repeat rule of generate(form=) (BarRepeat attaches itself)

    # ---------------------------------------------------------------- shape
    @property
    def vocab_size(self) -> int:
        return int(self.cls.shape[0])

    @property
    def n_states(self) -> int:
        return int(self.next.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.next.shape[1])

    def state(self, name: str) -> int:
        return self.state_names.index(name)

    def reachable(self) -> List[int]:
        """states that can be reached from `start` through allowed classes that have tokens, in order of discovery"""
        seen, todo = [self.start], [self.start]
        while todo:
            s = todo.pop()
            for c in range(self.n_classes):
                if (int(self.allow[s]) & self.populated) >> c & 1:
                    n = int(self.next[s, c])
                    if n not in seen:
                        seen.append(n)
                        todo.append(n)
        return seen

    def only_token_states(self, token: int) -> List[int]:
        """reachable states in which `token` is the only token allowed (generate refuses min_length with such an eos)"""
        out = []
        if not 0 <= int(token) < self.vocab_size:
            return out
        counts = np.bincount(self.cls, minlength=self.n_classes)
        tc = int(self.cls[int(token)])
        for s in self.reachable():
            n = sum(int(counts[c]) for c in range(self.n_classes) if (int(self.allow[s]) >> c) & 1)
            if (int(self.allow[s]) >> tc) & 1 and n == 1:
                out.append(s)
        return out

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, start: Optional[int] = None) -> Tuple[int, int]:
        """(state, index of the first violation or -1) for a 1-D id sequence.  Ids < 0 are skipped (the decoder's marker of a left
        pad column); an id beyond the vocabulary is a violation.  The walk stops at a violation: the state returned is the one it
        happened in."""
        s = self.start if start is None else int(start)
        seq = ids.tolist() if hasattr(ids, 'tolist') else list(ids)
        V = self.vocab_size
        for i, tok in enumerate(seq):
            tok = int(tok)
            if tok < 0:
                continue
            if tok >= V:
                return s, i
            c = int(self.cls[tok])
            if not (int(self.allow[s]) >> c) & 1:
                return s, i
            s = int(self.next[s, c])
        return s, -1

    def walk_budget(self, ids, bar: int = 0, rem: int = 0) -> Tuple[int, int, int]:
        """(bar, rem, index of the first token the duration budget bars or -1) for a 1-D id sequence (BarBudget.walk): the host
        reference of mxl_budget_scan.  Ids < 0 are skipped, ids beyond the vocabulary are `walk`'s to report."""
        if self.budget is None:
            raise ValueError('this grammar carries no bar budget: build it with grammar(bar_budget=True)')
        return self.budget.walk(ids, bar, rem)

    def walk_bars(self, ids, left: int) -> Tuple[int, int]:
        """(left, index of the first token the bar count bars or -1) for a 1-D id sequence that starts with `left` bars to go
        (BarCount.walk): the host reference of the device rule.  Ids < 0 and ids beyond the vocabulary are skipped."""
        if self.bar_count is None:
            raise ValueError('this grammar carries no bar count: attach a grammar.BarCount (the music grammar has one)')
        return self.bar_count.walk(ids, left)

    def accepts(self, ids) -> bool:
        s, bad = self.walk(ids)
        return bad < 0 and (self.accepting is None or s in self.accepting)

    # ---------------------------------------------------------------- device tables
    def to(self, device):
        """the three tables on `device` (uploaded once per device): (cls uint8 (V,), allow int32 (S,), next uint8 (S * C,))"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.cls.copy()).to(device),
                              torch.from_numpy(self.allow.view(np.int32).copy()).to(device),
                              torch.from_numpy(self.next.reshape(-1).copy()).to(device))
        return self._dev[key]

    def __repr__(self):
        return f'TokenGrammar(V={self.vocab_size}, classes={self.n_classes}, states={self.n_states}, start={self.state_names[self.start]})'


class BarBudget:
    def __init__(self, grammar: TokenGrammar, slots, bars, opens, need_free, need_full):
        """The duration budget of `grammar` (module docstring) from explicit tables: slots / bars (V,) and three sets of classes,
        each a bit mask or an iterable of class names.  Attaches itself as `grammar.budget`.  Raises ValueError when the tables do
        not fit the grammar, or when some (state, bar, rem) that can be reached from the start state leaves no token allowed by
        grammar and budget together: the sampler must never face a row with every token barred."""
        V, C = grammar.vocab_size, grammar.n_classes
        slots_a, bars_a = np.asarray(slots), np.asarray(bars)
        if slots_a.shape != (V,) or bars_a.shape != (V,):
            raise ValueError(f'slots and bars must be ({V},): one entry per token of the grammar')
        if slots_a.min() < 0 or slots_a.max() > RARE_SLOTS or bars_a.min() < 0 or bars_a.max() > NO_SIG:
            raise ValueError('slots / bars entries must fit 16 bits')
        self.slots = np.ascontiguousarray(slots_a, dtype=np.uint16)
        self.bars = np.ascontiguousarray(bars_a, dtype=np.uint16)

        def mask(x):
            if isinstance(x, (int, np.integer)):
                m = int(x)
            else:
                m = 0
                for name in x:
                    if name not in grammar.class_names:
                        raise ValueError(f'unknown token class {name!r}')
                    m |= 1 << grammar.class_names.index(name)
            if m < 0 or m >> C:
                raise ValueError(f'a class mask has a bit set beyond class {C - 1}')
            return m

        self.opens, self.need_free, self.need_full = mask(opens), mask(need_free), mask(need_full)
        self.grammar = grammar
        # the distinct (slots, bars) pairs among the tokens of each class, with the number of tokens that share them
        self._kinds: List[Dict[Tuple[int, int], int]] = [dict() for _ in range(C)]
        for c, k, sig in zip(grammar.cls.tolist(), self.slots.tolist(), self.bars.tolist()):
            self._kinds[c][(k, sig)] = self._kinds[c].get((k, sig), 0) + 1
        self._reach = self._reachable()
        for (s, bar, rem), n in self._reach.items():
            if n == 0:
                raise ValueError(f'state {grammar.state_names[s]} with bar {bar} and {rem} slots free can be reached from the start '
                                 'state and allows no token under the bar budget: generation would face a row with every token barred')
        self._dev: Dict[str, tuple] = {}
        grammar.budget = self

    # ---------------------------------------------------------------- the rule
    @staticmethod
    def slots_take(k: int) -> int:
        """the slots a token with `slots` entry k takes from rem (module docstring; RARE_SLOTS takes nothing: it is never kept
        in a constrained row)"""
        return 0 if k == RARE_SLOTS else k & (NEED_ONE_MORE - 1)

    @staticmethod
    def slots_need(k: int) -> int:
        """the free slots a token with `slots` entry k needs: its take, one more with bit 15; RARE_SLOTS is beyond any rem"""
        return k if k == RARE_SLOTS else (k & (NEED_ONE_MORE - 1)) + (k >> 15)

    def allows(self, bar: int, rem: int, c: int, k: int) -> bool:
        """may a token of class c and `slots` entry k follow in a row at (bar, rem)?  (what the grammar state says comes on top)"""
        if bar <= 0:
            return True
        if self.slots_need(k) > rem:                     # a duration that overfills the channel; RARE_SLOTS is beyond any rem
            return False
        if (self.need_free >> c) & 1 and rem <= 0:
            return False
        if (self.need_full >> c) & 1 and rem != 0:
            return False
        return True

    def move(self, bar: int, rem: int, c: int, k: int, sig: int) -> Tuple[int, int]:
        """(bar, rem) after a token of class c with `slots` entry k and `bars` entry sig"""
        if sig != NO_SIG:
            bar, rem = sig, 0
        if (self.opens >> c) & 1:
            rem = bar
        if bar > 0 and k != RARE_SLOTS:
            rem = max(rem - self.slots_take(k), 0)
        return bar, rem

    def _reachable(self) -> Dict[Tuple[int, int, int], int]:
        """{(state, bar, rem): tokens allowed there by grammar and budget together} over everything the start state reaches"""
        g = self.grammar
        start = (g.start, 0, 0)
        seen, todo = {}, [start]
        while todo:
            node = todo.pop()
            if node in seen:
                continue
            s, bar, rem = node
            n = 0
            for c in range(g.n_classes):
                if not (int(g.allow[s]) >> c) & 1:
                    continue
                nxt = int(g.next[s, c])
                for (k, sig), count in self._kinds[c].items():
                    if self.allows(bar, rem, c, k):
                        n += count
                        succ = (nxt, *self.move(bar, rem, c, k, sig))
                        if succ not in seen:
                            todo.append(succ)
            seen[node] = n
        return seen

    def only_token_states(self, token: int) -> List[Tuple[int, int, int]]:
        """reachable (state, bar, rem) in which `token` is the only token allowed (TokenGrammar.only_token_states under the budget)"""
        g = self.grammar
        if not 0 <= int(token) < g.vocab_size:
            return []
        c, k = int(g.cls[int(token)]), int(self.slots[int(token)])
        return [node for node, n in self._reach.items()
                if n == 1 and (int(g.allow[node[0]]) >> c) & 1 and self.allows(node[1], node[2], c, k)]

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, bar: int = 0, rem: int = 0) -> Tuple[int, int, int]:
        """(bar, rem, index of the first token the budget bars or -1); the walk stops there.  Ids < 0 (left pads) and ids beyond
        the vocabulary are skipped: the latter are the grammar's to report."""
        seq = ids.tolist() if hasattr(ids, 'tolist') else list(ids)
        V = int(self.slots.shape[0])
        cls, slots, bars = self.grammar.cls, self.slots, self.bars
        bar, rem = int(bar), int(rem)
        for i, tok in enumerate(seq):
            tok = int(tok)
            if tok < 0 or tok >= V:
                continue
            c, k = int(cls[tok]), int(slots[tok])
            if not self.allows(bar, rem, c, k):
                return bar, rem, i
            bar, rem = self.move(bar, rem, c, k, int(bars[tok]))
        return bar, rem, -1

    # ---------------------------------------------------------------- device tables
    def to(self, device):
        """(slots, bars) on `device`, uploaded once per device: (V,) int16 each, holding the uint16 bit patterns"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.slots.view(np.int16).copy()).to(device),
                              torch.from_numpy(self.bars.view(np.int16).copy()).to(device))
        return self._dev[key]

    def __repr__(self):
        timed = (self.slots != RARE_SLOTS) & ((self.slots & (NEED_ONE_MORE - 1)) > 0)
        return f'BarBudget(bars={sorted(set(self.bars.tolist()) - {NO_SIG})}, durations={int(timed.sum())})'


def _class_mask(grammar: TokenGrammar, x) -> int:
    """a class bit mask of `grammar` from a mask or an iterable of class names"""
    if isinstance(x, (int, np.integer)):
        m = int(x)
    else:
        m = 0
        for name in ([x] if isinstance(x, str) else x):
            if name not in grammar.class_names:
                raise ValueError(f'unknown token class {name!r}')
            m |= 1 << grammar.class_names.index(name)
    if m < 0 or m >> grammar.n_classes:
        raise ValueError(f'a class mask has a bit set beyond class {grammar.n_classes - 1}')
    return m


class BarCount:
    def __init__(self, grammar: TokenGrammar, count, end):
        """The bar count rule of `grammar` (module docstring): `count` and `end`, each a class bit mask or an iterable of class
        names.  Attaches itself as `grammar.bar_count`; attach it after the grammar's BarBudget, if it gets one.
        The sampler must never face a row with every token barred, so the constructor looks at every state the start state reaches
        (under the budget: every (state, bar, rem)).  One that allows only `end` tokens would be stuck while left > 0: ValueError.
        One that allows only `count` tokens is stuck at left == 0 (the music grammar's S3: after the key only <bar> may follow, a
        song has a bar).  `needs_bar` holds the states from which such a state is reached without a `count` token: a row may not
        START there with n_bars = 0, which `generate` refuses per row.  A `count` token that leads into `needs_bar` could bring a
        row there with left == 0: ValueError."""
        self.count, self.end = _class_mask(grammar, count), _class_mask(grammar, end)
        if not self.count or not self.end:
            raise ValueError('count and end each need at least one class')
        if self.count & self.end:
            raise ValueError('a class cannot both open a bar and end the stream')
        self.grammar = grammar
        g, stuck = grammar, set()
        for s, name, classes in self._nodes():
            if classes and not classes & ~self.end:
                raise ValueError(f'{name} can be reached from the start state and allows only `end` classes: while bars are left '
                                 'to open that row would have every token barred')
            if classes and not classes & ~self.count:
                stuck.add(s)
        reach = g.reachable()
        needs, grew = set(stuck), True
        while grew:                                      # backwards from the stuck states over the transitions of other classes
            grew = False
            for s in reach:
                if s not in needs and any((int(g.allow[s]) & g.populated & ~self.count) >> c & 1 and int(g.next[s, c]) in needs
                                          for c in range(g.n_classes)):
                    needs.add(s)
                    grew = True
        self.needs_bar = frozenset(needs)
        for s in reach:
            for c in range(g.n_classes):
                if (int(g.allow[s]) & g.populated & self.count) >> c & 1 and int(g.next[s, c]) in needs:
                    raise ValueError(f'a `count` token in state {g.state_names[s]} leads to state {g.state_names[int(g.next[s, c])]}, '
                                     'from which only a further `count` token leads on: after its last bar that row would have '
                                     'every token barred')
        grammar.bar_count = self

    def _nodes(self):
        """(state, name, mask of the classes that have an allowed token) of everything the start state reaches"""
        g = self.grammar
        if g.budget is None:
            for s in g.reachable():
                yield s, f'state {g.state_names[s]}', int(g.allow[s]) & g.populated
            return
        bud = g.budget
        for s, bar, rem in bud._reach:
            m = 0
            for c in range(g.n_classes):
                if (int(g.allow[s]) >> c) & 1 and any(bud.allows(bar, rem, c, k) for k, _ in bud._kinds[c]):
                    m |= 1 << c
            yield s, f'state {g.state_names[s]} with bar {bar} and {rem} slots free', m

    # ---------------------------------------------------------------- the rule
    def allows(self, left: int, c: int) -> bool:
        """may a token of class c follow in a row with `left` bars to go?  (what the grammar and the budget say comes on top)"""
        if left < 0:
            return True
        if (self.count >> c) & 1 and left == 0:
            return False
        if (self.end >> c) & 1 and left > 0:
            return False
        return True

    def move(self, left: int, c: int) -> int:
        """`left` after a token of class c"""
        return left - 1 if left > 0 and (self.count >> c) & 1 else left

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, left: int) -> Tuple[int, int]:
        """(left, index of the first token the rule bars or -1); the walk stops there.  Ids < 0 (left pads) and ids beyond the
        vocabulary are skipped: the latter are the grammar's to report."""
        seq = ids.tolist() if hasattr(ids, 'tolist') else list(ids)
        cls, V, left = self.grammar.cls, self.grammar.vocab_size, int(left)
        for i, tok in enumerate(seq):
            tok = int(tok)
            if tok < 0 or tok >= V:
                continue
            c = int(cls[tok])
            if not self.allows(left, c):
                return left, i
            left = self.move(left, c)
        return left, -1

    def __repr__(self):
        names = lambda m: [n for i, n in enumerate(self.grammar.class_names) if (m >> i) & 1]
        return f'BarCount(count={names(self.count)}, end={names(self.end)})'


class MelodyGuide:
    def __init__(self, grammar: TokenGrammar, enter, leave):
        """The guide rule of `grammar` (module docstring): `enter` and `leave`, each a class bit mask or an iterable of class
        names.  Attaches itself as `grammar.guide`."""
        self.enter, self.leave = _class_mask(grammar, enter), _class_mask(grammar, leave)
        if not self.enter or not self.leave:
            raise ValueError('enter and leave each need at least one class')
        if self.enter & self.leave:
            raise ValueError('a class cannot both open and close a guided span')
        self.grammar = grammar
        grammar.guide = self

    # ---------------------------------------------------------------- the rule
    def forced(self, pos: int, force: int, guide) -> int:
        """the token a row at (pos, force) is fed from `guide` at this step, -1 = none: the row chooses"""
        return int(guide[pos]) if force and 0 <= pos < len(guide) else -1

    def allows(self, pos: int, force: int, guide, tok: int) -> bool:
        """may token `tok` follow in a row at (pos, force)?  A fed row may emit its guide token alone -- and that one whatever
        the other rules say; a free row is theirs to judge"""
        f = self.forced(pos, force, guide)
        return f < 0 or int(tok) == f

    def move(self, pos: int, force: int, glen: int, c: int) -> Tuple[int, int]:
        """(pos, force) after a kept token of class c in a row whose guide holds glen tokens"""
        if force:
            return pos + 1, 0 if (self.leave >> c) & 1 else 1
        if (self.enter >> c) & 1 and pos < glen:
            return pos + 1, 1
        return pos, 0

    def split(self, guide) -> List[List[int]]:
        """the bars of a guide: each starts with an `enter` token and ends at its first `leave` token, and nothing lies between
        them.  Raises ValueError naming the index where that fails, or for an empty guide or a token outside the vocabulary."""
        seq = [int(t) for t in (guide.tolist() if hasattr(guide, 'tolist') else list(guide))]
        cls, V = self.grammar.cls, self.grammar.vocab_size
        if not seq:
            raise ValueError('an empty guide holds no bar')
        bars, i = [], 0
        while i < len(seq):
            for j in range(i, len(seq)):
                if not 0 <= seq[j] < V:
                    raise ValueError(f'guide index {j}: token {seq[j]} is outside the vocabulary of {V} tokens')
            if not (self.enter >> int(cls[seq[i]])) & 1:
                raise ValueError(f'guide index {i}: token {seq[i]} opens no guided span (a bar starts with an `enter` token)')
            j = next((j for j in range(i + 1, len(seq)) if (self.leave >> int(cls[seq[j]])) & 1), None)
            if j is None:
                raise ValueError(f'guide index {i}: the bar that starts here never reaches a `leave` token')
            bars.append(seq[i:j + 1])
            i = j + 1
        return bars

    def extract(self, ids, first_bar: int = 0, n_bars: Optional[int] = None) -> List[int]:
        """the guide of a piece: over bars first_bar .. first_bar + n_bars - 1 of `ids` (default: to the last one), the tokens of
        each from its `enter` token up to and including its first `leave` token, concatenated.  Ids < 0 are skipped."""
        seq = [int(t) for t in (ids.tolist() if hasattr(ids, 'tolist') else list(ids)) if int(t) >= 0]
        cls = self.grammar.cls
        starts = [i for i, t in enumerate(seq) if (self.enter >> int(cls[t])) & 1]
        if first_bar < 0 or (n_bars is not None and n_bars < 0):
            raise ValueError('first_bar and n_bars must not be negative')
        chosen = starts[first_bar:] if n_bars is None else starts[first_bar:first_bar + n_bars]
        if n_bars is not None and len(chosen) != n_bars:
            raise ValueError(f'bars {first_bar}..{first_bar + n_bars - 1} asked of a piece with {len(starts)} bars')
        out = []
        for i in chosen:
            j = next((j for j in range(i + 1, len(seq)) if (self.leave >> int(cls[seq[j]])) & 1), None)
            if j is None or any((self.enter >> int(cls[t])) & 1 for t in seq[i + 1:j]):
                raise ValueError(f'the bar at index {i} never reaches a `leave` token')
            out += seq[i:j + 1]
        return out

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, guide, gpos: int = 0, gforce: int = 0) -> Tuple[int, int, int]:
        """(pos, force, index of the first token that departs from the guide or -1) for a 1-D id sequence in a row that starts at
        (gpos, gforce); the walk stops there.  A token departs if the row is fed another one, or if it opens a span (`enter`) in
        a free row whose guide is used up.  Ids < 0 (left pads) and ids beyond the vocabulary are skipped.  The host reference of
        the device rule."""
        seq = ids.tolist() if hasattr(ids, 'tolist') else list(ids)
        g = [int(t) for t in (guide.tolist() if hasattr(guide, 'tolist') else list(guide))]
        cls, V, pos, force = self.grammar.cls, self.grammar.vocab_size, int(gpos), int(gforce)
        for i, tok in enumerate(seq):
            tok = int(tok)
            if tok < 0 or tok >= V:
                continue
            c = int(cls[tok])
            if not self.allows(pos, force, g, tok) or (not force and (self.enter >> c) & 1 and pos >= len(g)):
                return pos, force, i
            pos, force = self.move(pos, force, len(g), c)
        return pos, force, -1

    def __repr__(self):
        names = lambda m: [n for i, n in enumerate(self.grammar.class_names) if (m >> i) & 1]
        return f'MelodyGuide(enter={names(self.enter)}, leave={names(self.leave)})'


class BarRepeat:
    SPANS = {'bar': 0, 'melody': 1}                      # generate's form_span -> the device's span

    def __init__(self, grammar: TokenGrammar, enter, leave):
        """The repeat rule of `grammar` (module docstring): `enter` and `leave`, each a class bit mask or an iterable of class
        names.  Attaches itself as `grammar.repeat`."""
        self.enter, self.leave = _class_mask(grammar, enter), _class_mask(grammar, leave)
        if not self.enter or not self.leave:
            raise ValueError('enter and leave each need at least one class')
        if self.enter & self.leave:
            raise ValueError('a class cannot both open a bar and close its melody')
        self.grammar = grammar
        grammar.repeat = self

    # ---------------------------------------------------------------- plans
    @staticmethod
    def plan_of(form, section_bars: int = 1) -> List[int]:
        """the plan of a form: plan[k] = -1, generated bar k is free, or j < k, it repeats generated bar j.  form: a string of
        sections, one character each, `section_bars` bars a section -- the first occurrence of a character is free, a later one
        copies the first bar by bar ('AABA', 2 -> [-1, -1, 0, 1, -1, -1, 0, 1]) -- or a sequence of ints, a plan itself, which is
        validated: -1 <= plan[k] < k.  ValueError for an empty form, section_bars < 1 or a bad entry."""
        if isinstance(section_bars, bool) or not hasattr(section_bars, '__index__') or int(section_bars) < 1:
            raise ValueError(f'section_bars must be an int >= 1, got {section_bars!r}')
        n = int(section_bars)
        if isinstance(form, str):
            if not form:
                raise ValueError('an empty form plans no bar')
            first, plan = {}, []
            for i, ch in enumerate(form):
                at = first.setdefault(ch, i)
                plan += [-1 if at == i else at * n + r for r in range(n)]
            return plan
        if isinstance(form, bytes) or not hasattr(form, '__iter__'):
            raise ValueError('a form is a string of sections or a plan, a sequence of ints')
        seq = form.tolist() if hasattr(form, 'tolist') else list(form)
        if any(isinstance(j, (bool, float, str)) or not hasattr(j, '__index__') for j in seq):
            raise ValueError('a plan is a sequence of ints')
        plan = [int(j) for j in seq]
        if not plan:
            raise ValueError('an empty form plans no bar')
        for k, j in enumerate(plan):
            if not -1 <= j < k:
                raise ValueError(f'plan entry {k} is {j}: a bar is free (-1) or repeats an earlier generated bar (0..{k - 1})')
        return plan

    # ---------------------------------------------------------------- the rule
    @staticmethod
    def start(n: int) -> dict:
        """the words of a row before its first generated token, with room for the columns of n bars"""
        return dict(bars=0, copy=-1, stop=0, barcol=[-1] * int(n))

    def forced(self, ids_row, gcopy: int) -> int:
        """the token a row with the word gcopy is fed from its own ids at this step, -1 = none: the row chooses"""
        return int(ids_row[gcopy]) if 0 <= gcopy < len(ids_row) and int(ids_row[gcopy]) >= 0 else -1

    def move(self, words: dict, plan_row, c: int, col: int, span: int) -> dict:
        """the words (bars, copy, stop, barcol) after a kept token of class c written at column col, under the row's plan"""
        w = dict(words, barcol=list(words['barcol']))
        if w['copy'] >= 0:
            w['copy'] += 1
            if w['copy'] >= w['stop'] or (span == 1 and (self.leave >> c) & 1):
                w['copy'] = -1
        elif (self.enter >> c) & 1 and w['bars'] < len(plan_row):
            k = w['bars']
            w['barcol'][k] = col
            w['bars'] = k + 1
            j = int(plan_row[k])
            if j >= 0:
                lo = w['barcol'][j] + 1
                hi = col if j + 1 == k else w['barcol'][j + 1]
                if lo < hi:
                    w['copy'], w['stop'] = lo, hi
        return w

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, plan_row, span: int = 0, start: int = 0) -> Tuple[dict, int]:
        """(words, index of the first token that departs from the plan or -1) for a 1-D id sequence whose generated part begins
        at index `start` (the tokens before it are the prompt: they move nothing); the walk stops at a departure.  A token departs
        if the row is copying and it is not the token of the row's own history at `copy`.  A sequence cut inside a copy is clean.
        Ids < 0 (left pads) and ids beyond the vocabulary are skipped.  The host reference of the device rule."""
        seq = [int(t) for t in (ids.tolist() if hasattr(ids, 'tolist') else list(ids))]
        plan = [int(j) for j in (plan_row.tolist() if hasattr(plan_row, 'tolist') else list(plan_row))]
        cls, V = self.grammar.cls, self.grammar.vocab_size
        w = self.start(len(plan))
        for i in range(int(start), len(seq)):
            tok = seq[i]
            if tok < 0 or tok >= V:
                continue
            f = self.forced(seq, w['copy']) if plan else -1
            if f >= 0 and tok != f:
                return w, i
            w = self.move(w, plan, int(cls[tok]), i, span)
        return w, -1

    def __repr__(self):
        names = lambda m: [n for i, n in enumerate(self.grammar.class_names) if (m >> i) & 1]
        return f'BarRepeat(enter={names(self.enter)}, leave={names(self.leave)})'


class KeyRule:
    def __init__(self, keys, pcs, inkey=None):
        """The key rule (module docstring) from explicit tables: keys / pcs (V,) with NO_KEY / NO_PITCH for "none", inkey (24,) bit
        masks over the 12 pitch classes (default: metrics.in_key_table()).  Raises ValueError when the tables are out of range, or
        when some key keeps no pitch token at all -- with pitch tokens in the vocabulary, a row in that key would have every pitch
        barred wherever only a pitch may follow."""
        keys_a, pcs_a = np.asarray(keys), np.asarray(pcs)
        if keys_a.ndim != 1 or keys_a.size == 0 or pcs_a.shape != keys_a.shape:
            raise ValueError('keys and pcs must be non-empty (V,) arrays: one entry per token')
        if inkey is None:
            from .metrics import in_key_table
            inkey = in_key_masks(in_key_table())
        inkey_a = np.asarray(inkey)
        if inkey_a.shape != (N_KEYS,) or int(inkey_a.min()) < 0 or int(inkey_a.max()) >> 12:
            raise ValueError(f'inkey must be ({N_KEYS},) bit masks over the 12 pitch classes')
        if ((keys_a < 0) | ((keys_a >= N_KEYS) & (keys_a != NO_KEY))).any():
            raise ValueError(f'keys holds an entry outside 0..{N_KEYS - 1} and NO_KEY')
        if ((pcs_a < 0) | ((pcs_a >= 12) & (pcs_a != NO_PITCH))).any():
            raise ValueError('pcs holds an entry outside 0..11 and NO_PITCH')
        self.keys = np.ascontiguousarray(keys_a, dtype=np.uint8)
        self.pcs = np.ascontiguousarray(pcs_a, dtype=np.uint8)
        self.inkey = np.ascontiguousarray(inkey_a, dtype=np.uint16)
        have = 0                                         # bit pc set <=> pitch class pc has a token
        for pc in np.unique(self.pcs[self.pcs != NO_PITCH]).tolist():
            have |= 1 << int(pc)
        for k in range(N_KEYS):
            if have and not int(self.inkey[k]) & have:
                raise ValueError(f'key {k} keeps no pitch token of this vocabulary: a row in that key would have every pitch barred')
        self._dev: Dict[str, tuple] = {}

    @property
    def vocab_size(self) -> int:
        return int(self.keys.shape[0])

    # ---------------------------------------------------------------- the rule
    def allows(self, key: int, tok: int) -> bool:
        """may token `tok` follow in a row in `key`?  (what the grammar, the budget and the count say comes on top)"""
        pc = int(self.pcs[int(tok)])
        return key < 0 or pc == NO_PITCH or bool((int(self.inkey[int(key)]) >> pc) & 1)

    def move(self, key: int, tok: int) -> int:
        """`key` after token `tok`: a key token sets it, nothing else changes it"""
        k = int(self.keys[int(tok)])
        return int(key) if k == NO_KEY else k

    def allowed(self, key: int) -> np.ndarray:
        """(V,) bool: `allows(key, v)` for every token v"""
        if key < 0:
            return np.ones(self.vocab_size, dtype=bool)
        return (self.pcs == NO_PITCH) | (((int(self.inkey[int(key)]) >> (self.pcs & 15).astype(np.int64)) & 1) == 1)

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, key: int = -1, check_from: int = 0) -> Tuple[int, int]:
        """(key, index of the first pitch outside the row's key or -1) for a 1-D id sequence that starts in `key`; the walk stops
        there.  Entries before `check_from` only move the key (a prompt supplies its key, its pitches are not judged).  Ids < 0
        (left pads) and ids beyond the vocabulary are skipped.  The host reference of mxl_key_scan."""
        seq = ids.tolist() if hasattr(ids, 'tolist') else list(ids)
        V, key = self.vocab_size, int(key)
        for i, tok in enumerate(seq):
            tok = int(tok)
            if tok < 0 or tok >= V:
                continue
            if i >= check_from and not self.allows(key, tok):
                return key, i
            key = self.move(key, tok)
        return key, -1

    # ---------------------------------------------------------------- device tables
    def to(self, device):
        """(keys, pcs, inkey) on `device`, uploaded once per device: uint8 (V,) twice and int16 (24,) holding the uint16 bit patterns"""
        import torch
        dk = str(torch.device(device))
        if dk not in self._dev:
            self._dev[dk] = (torch.from_numpy(self.keys.copy()).to(device), torch.from_numpy(self.pcs.copy()).to(device),
                             torch.from_numpy(self.inkey.view(np.int16).copy()).to(device))
        return self._dev[dk]

    def __repr__(self):
        return f'KeyRule(V={self.vocab_size}, key tokens={int((self.keys != NO_KEY).sum())}, pitches={int((self.pcs != NO_PITCH).sum())})'


def pack_bounds(bounds) -> int:
    """(lo_melody, hi_melody, lo_bass, hi_bass) -> the row's `range` word: one byte each from the lowest"""
    lm, hm, lb, hb = (int(x) for x in bounds)
    return lm | (hm << 8) | (lb << 16) | (hb << 24)


class RegisterRule:
    def __init__(self, reg):
        """The register rule (module docstring) from its table: reg (V,) with a MIDI number 0..127, REG_MELODY / REG_BASS / REG_BAR
        or NO_PITCH per token.  Raises ValueError for any other entry."""
        reg_a = np.asarray(reg)
        if reg_a.ndim != 1 or reg_a.size == 0:
            raise ValueError('reg must be a non-empty (V,) array: one entry per token')
        if ((reg_a < 0) | ((reg_a > 127) & ~np.isin(reg_a, (REG_MELODY, REG_BASS, REG_BAR, NO_PITCH)))).any():
            raise ValueError('reg holds an entry that is no MIDI number 0..127, part code or NO_PITCH')
        self.reg = np.ascontiguousarray(reg_a, dtype=np.uint8)
        self._dev: Dict[str, object] = {}

    @property
    def vocab_size(self) -> int:
        return int(self.reg.shape[0])

    # ---------------------------------------------------------------- the rule
    @staticmethod
    def bounds_of(part: int, floor: int, bounds, gap: int) -> Tuple[int, int]:
        """(lo, hi) a pitch of a row in `part` must lie in; hi < lo = no pitched token is left"""
        lm, hm, lb, hb = (int(x) for x in bounds)
        if part == 1:
            return lm, hm
        if part == 2:
            return lb, (min(hb, int(floor) - int(gap)) if gap >= 0 and floor < NO_FLOOR else hb)
        return 0, 127

    def allows(self, part: int, floor: int, bounds, gap: int, tok: int) -> bool:
        """may token `tok` follow in a row at (part, floor) under `bounds` and `gap`?  (the other rules come on top)"""
        p = int(self.reg[int(tok)])
        lo, hi = self.bounds_of(part, floor, bounds, gap)
        return p > 127 or lo <= p <= hi

    def allowed(self, part: int, floor: int, bounds, gap: int) -> np.ndarray:
        """(V,) bool: `allows(part, floor, bounds, gap, v)` for every token v"""
        lo, hi = self.bounds_of(part, floor, bounds, gap)
        return (self.reg > 127) | ((self.reg >= lo) & (self.reg <= hi))

    def move(self, part: int, floor: int, tok: int) -> Tuple[int, int]:
        """(part, floor) after token `tok`"""
        p = int(self.reg[int(tok)])
        if p == REG_MELODY:
            return 1, int(floor)
        if p == REG_BASS:
            return 2, int(floor)
        if p == REG_BAR:
            return 0, NO_FLOOR
        if p <= 127 and part == 1:
            return 1, min(int(floor), p)
        return int(part), int(floor)

    # ---------------------------------------------------------------- host reference
    def walk(self, ids, bounds=ANY_RANGE, gap: int = -1, part: int = 0, floor: int = NO_FLOOR, check_from: int = 0) -> Tuple[int, int, int]:
        """(part, floor, index of the first pitch outside its part's bounds or -1) for a 1-D id sequence that starts at (part,
        floor); the walk stops there.  Entries before `check_from` only move the words (the prompt's pitches are not judged).  Ids
        < 0 (left pads) and ids beyond the vocabulary are skipped.  The host reference of mxl_register_scan."""
        seq = ids.tolist() if hasattr(ids, 'tolist') else list(ids)
        V, part, floor = self.vocab_size, int(part), int(floor)
        for i, tok in enumerate(seq):
            tok = int(tok)
            if tok < 0 or tok >= V:
                continue
            if i >= check_from and not self.allows(part, floor, bounds, gap, tok):
                return part, floor, i
            part, floor = self.move(part, floor, tok)
        return part, floor, -1

    # ---------------------------------------------------------------- device table
    def to(self, device):
        """`reg` on `device`, uploaded once per device: uint8 (V,)"""
        import torch
        dk = str(torch.device(device))
        if dk not in self._dev:
            self._dev[dk] = torch.from_numpy(self.reg.copy()).to(device)
        return self._dev[dk]

    def __repr__(self):
        return f'RegisterRule(V={self.vocab_size}, pitches={int((self.reg <= 127).sum())})'


def music_register_rule(vocab) -> RegisterRule:
    """the register rule of a MusicVocabulary of any pitch kind.  A pitch token's entry is its MIDI number, the `i` its name was built
    from in `MusicVocabulary._pitches`: (octave + 1) * 12 + index - 1, where the `step` kind's B# (index 1, named an octave down) and
    C- (index 12, named an octave up) have their octave put back; the scale-degree suffix of the `degree` kind is ignored.  The rest
    and the rare pitch hold NO_PITCH."""
    reg = np.full(len(vocab), NO_PITCH, dtype=np.uint8)
    for tok, i in vocab.tok2id.items():
        m = vocab._re_pitch.match(tok)
        if m is None:
            continue
        idx, otv, name = int(m.group(1)), int(m.group(2)), m.group(3)
        if vocab.pitch_kind == 'step':
            if idx == 1 and name == 'B':
                otv += 1
            elif idx == 12 and name == 'C':
                otv -= 1
        midi = (otv + 1) * 12 + idx - 1
        if not 0 <= midi <= 127:
            raise ValueError(f'pitch token {tok!r} names MIDI number {midi}')
        reg[i] = midi
    for tok, code in ((vocab.start_of_melody, REG_MELODY), (vocab.start_of_bass, REG_BASS), (vocab.start_of_bar, REG_BAR)):
        reg[vocab.tok2id[tok]] = code
    return RegisterRule(reg)


def in_key_masks(table) -> np.ndarray:
    """(24,) uint16 from a (24, 12) 0/1 table (metrics.in_key_table): bit pc of entry k set <=> table[k, pc] == 1"""
    tab = np.asarray(table)
    return np.array([sum(1 << pc for pc in range(tab.shape[1]) if tab[k, pc] == 1) for k in range(tab.shape[0])], dtype=np.uint16)


def key_ordinal(key) -> int:
    """a key as `generate(key=)` takes it -> its ordinal in vocab.KEY_NAMES, -1 = none: None, an ordinal, or a name with or without
    the token prefix ('AMinor', 'Key_AMinor')"""
    from .vocab import KEY_NAMES
    if key is None:
        return -1
    if isinstance(key, str):
        name = key[len('Key_'):] if key.startswith('Key_') else key
        if name not in KEY_NAMES:
            raise ValueError(f'unknown key {key!r}')
        return KEY_NAMES.index(name)
    if isinstance(key, (bool, float)) or not -1 <= int(key) < N_KEYS:
        raise ValueError(f'a key is a name, None or an ordinal in -1..{N_KEYS - 1}, got {key!r}')
    return int(key)


def music_key_rule(vocab) -> KeyRule:
    """the key rule of a MusicVocabulary of any pitch kind, from the tables of the IKR metric (metrics.pitch_class_table,
    metrics.in_key_table): what the metric counts as an off-key pitch is what the rule bars.  For the `degree` pitch kind that is the
    token's pitch class alone; the scale-degree suffix is not checked against the key."""
    from .metrics import pitch_class_table
    from .vocab import KEY_NAMES
    pc = pitch_class_table(vocab).astype(np.int64)
    keys = np.full(len(vocab), NO_KEY, dtype=np.uint8)
    for o, name in enumerate(KEY_NAMES):
        if f'Key_{name}' in vocab:
            keys[vocab.tok2id[f'Key_{name}']] = o
    return KeyRule(keys, np.where(pc < 0, NO_PITCH, pc).astype(np.uint8))


def from_transitions(cls, class_names: Sequence[str], transitions: Sequence[Tuple[str, str, str]], start: str,
                     accepting: Optional[Iterable[str]] = None, budget: Optional[dict] = None,
                     bar_count: Optional[dict] = None, guide: Optional[dict] = None, repeat: Optional[dict] = None) -> TokenGrammar:
    """a TokenGrammar from (state, class, successor) triples by name; states are numbered in order of appearance, `start` first.
    budget: the explicit tables of a BarBudget to attach, as its keyword arguments (slots, bars, opens, need_free, need_full).
    bar_count: the classes of a BarCount to attach, as its keyword arguments (count, end).
    guide: the classes of a MelodyGuide to attach, as its keyword arguments (enter, leave)
    repeat: the classes of a BarRepeat to attach, as its keyword arguments (enter, leave)"""
    states = [start]
    for a, _, b in transitions:
        for s in (a, b):
            if s not in states:
                states.append(s)
    cid = {c: i for i, c in enumerate(class_names)}
    S, C = len(states), len(class_names)
    allow = np.zeros(S, dtype=np.uint32)
    nxt = np.zeros((max(S, 1), max(C, 1)), dtype=np.int64)
    for a, c, b in transitions:
        if c not in cid:
            raise ValueError(f'unknown token class {c!r}')
        i = states.index(a)
        if (int(allow[i]) >> cid[c]) & 1 and nxt[i, cid[c]] != states.index(b):
            raise ValueError(f'two successors for class {c!r} in state {a!r}: the automaton must be deterministic')
        allow[i] |= np.uint32(1 << cid[c])
        nxt[i, cid[c]] = states.index(b)
    acc = None if accepting is None else [states.index(s) for s in accepting]
    g = TokenGrammar(cls, allow, nxt, 0, acc, class_names, states)
    if budget is not None:
        BarBudget(g, **budget)
    if bar_count is not None:
        BarCount(g, **bar_count)
    if guide is not None:
        MelodyGuide(g, **guide)
    if repeat is not None:
        BarRepeat(g, **repeat)
    return g


# -------------------------------------------------------------------- the music token stream
MUSIC_CLASSES = ('time_sig', 'tempo', 'key', 'pitch', 'duration', '[OMIT]', '[PAD]', '<bar>', '</s>', '<melody>', '<bass>',
                 '<tup>', '</tup>')


def _channel(p: str, closes: Sequence[Tuple[str, str]]) -> List[Tuple[str, str, str]]:
    """one channel of a bar (melody M / bass B): notes and tuplets, `closes` = what may follow a completed note"""
    return [(f'{p}_OPEN', 'pitch', f'{p}_P'), (f'{p}_OPEN', '<tup>', f'{p}_T0'),
            (f'{p}_P', 'duration', f'{p}_D'),
            (f'{p}_D', 'pitch', f'{p}_P'), (f'{p}_D', '<tup>', f'{p}_T0'), *[(f'{p}_D', c, s) for c, s in closes],
            (f'{p}_T0', 'pitch', f'{p}_T1'),
            (f'{p}_T1', 'pitch', f'{p}_T1'), (f'{p}_T1', 'duration', f'{p}_T2'),
            (f'{p}_T2', '</tup>', f'{p}_D')]


MUSIC_TRANSITIONS = [
    ('S0', 'time_sig', 'S1'), ('S1', 'tempo', 'S2'), ('S2', 'key', 'S3'), ('S2', '<bar>', 'BAR'), ('S3', '<bar>', 'BAR'),
    ('BAR', '<melody>', 'M_OPEN'),
    *_channel('M', [('<bass>', 'B_OPEN')]),
    *_channel('B', [('<bar>', 'BAR'), ('</s>', 'END')]),
    ('END', '[PAD]', 'END'),
]


MUSIC_BAR_COUNT_CLASSES = dict(count=('<bar>',), end=('</s>',))
MUSIC_GUIDE_CLASSES = dict(enter=('<bar>',), leave=('<bass>',))
MUSIC_BUDGET_CLASSES = dict(opens=('<melody>', '<bass>'), need_free=('pitch', '<tup>'), need_full=('<bass>', '<bar>', '</s>'))


def music_budget_tables(vocab) -> dict:
    """slots and bars of a MusicVocabulary: a duration token d_x is x / (4 / 2**precision) slots (always whole: that is how the
    vocabulary lists its durations), d_rare is RARE_SLOTS; TimeSig_n/d is a bar of 2**precision * n / d slots, and TimeSig_rare or a
    bar that is no whole number of slots is 0 = unconstrained.  Every duration is below NEED_ONE_MORE (checked): bit 15 of a `slots`
    entry, "needs one more than it takes", is never set here -- only `subword_grammar` sets it"""
    from fractions import Fraction
    V = len(vocab)
    slot = Fraction(4, 2 ** vocab.precision)
    slots, bars = np.zeros(V, dtype=np.uint16), np.full(V, NO_SIG, dtype=np.uint16)
    for tok, i in vocab.tok2id.items():
        typ = vocab.type(tok)
        if typ == 'duration':
            n = None if tok == vocab.rare_duration else Fraction(tok[2:]) / slot
            if n is not None and (n.denominator != 1 or not 0 < n < NEED_ONE_MORE):
                raise ValueError(f'duration token {tok!r} is no whole number of slots')
            slots[i] = RARE_SLOTS if n is None else int(n)
        elif typ == 'time_sig':
            n = Fraction(0) if tok == vocab.rare_time_sig else Fraction(tok[len('TimeSig_'):]) * 2 ** vocab.precision
            bars[i] = int(n) if n.denominator == 1 and n < NO_SIG else 0
    return dict(slots=slots, bars=bars, **MUSIC_BUDGET_CLASSES)


def music_grammar(vocab, bar_budget: bool = False) -> TokenGrammar:
    """the grammar above for a MusicVocabulary of any pitch kind: the class of a token is its `vocab.type`, and every special
    token ([PAD] and [OMIT] included) is a class of its own.  bar_budget: attach the duration budget (`grammar.budget`), so that
    every channel of a bar generated under the grammar is exactly as long as the prompt's time signature says.  Either form
    carries the bar count rule of `generate(n_bars=)` (`grammar.bar_count`: count = <bar>, end = </s>) and the guide rule of
    `generate(melody=)` (`grammar.guide`: enter = <bar>, leave = <bass>) and the repeat rule of `generate(form=)` (`grammar.repeat`,
    over the same two classes)"""
    cid = {c: i for i, c in enumerate(MUSIC_CLASSES)}
    cls = np.zeros(len(vocab), dtype=np.uint8)
    for tok, i in vocab.tok2id.items():
        typ = vocab.type(tok)
        name = tok if typ == 'special' else typ
        if name not in cid:
            raise ValueError(f'token {tok!r} has no class in the music grammar')
        cls[i] = cid[name]
    return from_transitions(cls, MUSIC_CLASSES, MUSIC_TRANSITIONS, 'S0', accepting=['END'],
                            budget=music_budget_tables(vocab) if bar_budget else None, bar_count=MUSIC_BAR_COUNT_CLASSES,
                            guide=MUSIC_GUIDE_CLASSES, repeat=MUSIC_GUIDE_CLASSES)


# -------------------------------------------------------------------- sub-word vocabularies
def subword_grammar(base: TokenGrammar, pieces: Sequence[Sequence[int]]) -> TokenGrammar:
    """`base` composed with a sub-word vocabulary: pieces[v] = the base ids that id v stands for (`id2base_ids()` of a sub-word
    tokenizer).  The rule is defined on the DECODED stream: a row of ids is allowed iff the concatenation of its pieces is allowed
    under `base` -- and its budget and bar count, which the result carries if `base` does (never its guide or its repeat rule).

    States, start and accepting states are the base's.  A single-base id keeps the class (index and name) of its base token, so the
    class masks of the budget and the count carry over bit for bit.  A multi-base id gets the class of the partial function it
    induces on the states -- `base.allow` / `base.next` walked over its pieces, undefined where a step is barred; ids with the same
    function share a class, and one whose function is defined nowhere gets a class that no state allows.  More than MAX_CLASSES
    classes: NotImplementedError.

    Budget: a single keeps its `slots` and `bars` entries.  A multi has bars = NO_SIG and slots = the sum k of its durations' slots
    (RARE_SLOTS if one of them is rare), with NEED_ONE_MORE on top where walking its pieces through the base budget needs k + 1
    free -- which, for every sequence the base grammar admits anywhere, is: its last base token is of a `need_free` class (it ends
    on an open note start).  The table cannot say more: a multi that holds a token of an `opens` or `need_full` class or a time
    signature (under a bar count: of a `count` or `end` class) raises NotImplementedError naming the id and the token; a sum that
    does not fit 15 bits raises ValueError."""
    S, C0, V0 = base.n_states, base.n_classes, base.vocab_size
    bud, cnt = base.budget, base.bar_count
    cls = np.zeros(len(pieces), dtype=np.int64)
    slots = np.zeros(len(pieces), dtype=np.uint16)
    bars = np.full(len(pieces), NO_SIG, dtype=np.uint16)
    names, funcs = list(base.class_names), {}                         # funcs: the function as a tuple over the states -> class
    for v, seq in enumerate(pieces):
        seq = [int(p) for p in seq]
        if not seq or any(not 0 <= p < V0 for p in seq):
            raise ValueError(f'sub-word id {v}: its pieces {seq} are no non-empty list of base ids below {V0}')
        if len(seq) == 1:
            cls[v] = base.cls[seq[0]]
            if bud is not None:
                slots[v], bars[v] = bud.slots[seq[0]], bud.bars[seq[0]]
            continue
        cs = [int(base.cls[p]) for p in seq]
        fn = []
        for s in range(S):
            for c in cs:
                if s < 0 or not (int(base.allow[s]) >> c) & 1:
                    s = -1
                    break
                s = int(base.next[s, c])
            fn.append(s)
        fn = tuple(fn)
        if fn not in funcs:
            name = '+'.join(base.class_names[c] for c in cs)
            funcs[fn] = len(names)
            names.append(name if name not in names else f'{name}#{len(names)}')
        cls[v] = funcs[fn]
        fixed = 0 if bud is None else bud.opens | bud.need_full       # classes whose effect on (bar, rem) a slots entry cannot carry
        fixed |= 0 if cnt is None else cnt.count | cnt.end            # ... and those the bar count reads: it sees the multi's class
        for p, c in zip(seq, cs):
            if (fixed >> c) & 1 or (bud is not None and int(bud.bars[p]) != NO_SIG):
                raise NotImplementedError(f'sub-word id {v} holds base token {p} of class {base.class_names[c]!r} among its pieces '
                                          f'{seq}: a token that opens or closes a channel or a bar, ends the stream or sets the time '
                                          'signature must be a sub-word id of its own (a WordPiece tokenizer trained with '
                                          'punctuate=True and independent_global_token=True keeps them apart)')
        if bud is None:
            continue
        take, need, rare = 0, 0, False
        for p, c in zip(seq, cs):
            k = int(bud.slots[p])
            if k == RARE_SLOTS:
                rare = True
                break
            need = max(need, take + BarBudget.slots_need(k), take + ((bud.need_free >> c) & 1))
            take += BarBudget.slots_take(k)
        if rare:
            slots[v] = RARE_SLOTS
            continue
        assert need in (take, take + 1)                               # a step needs its own take at most, or one slot for a note start
        if take + (need - take) * NEED_ONE_MORE >= RARE_SLOTS or take >= NEED_ONE_MORE:
            raise ValueError(f'sub-word id {v} with pieces {seq} takes {take} slots: a `slots` entry holds 15 bits of them')
        slots[v] = take | (NEED_ONE_MORE if need > take else 0)
    if len(names) > MAX_CLASSES:
        raise NotImplementedError(f'{len(names)} token classes ({C0} of the base grammar and {len(names) - C0} distinct functions of '
                                  f'multi-token ids on its states): a grammar has at most {MAX_CLASSES}')
    allow = base.allow.astype(np.int64)
    nxt = np.tile(np.arange(S, dtype=np.int64)[:, None], (1, len(names)))
    nxt[:, :C0] = base.next
    for fn, c in funcs.items():
        for s, n in enumerate(fn):
            if n >= 0:
                allow[s] |= 1 << c
                nxt[s, c] = n
    g = TokenGrammar(cls, allow, nxt, base.start, base.accepting, names, base.state_names)
    if bud is not None:
        BarBudget(g, slots, bars, bud.opens, bud.need_free, bud.need_full)
    if cnt is not None:
        BarCount(g, cnt.count, cnt.end)
    return g
