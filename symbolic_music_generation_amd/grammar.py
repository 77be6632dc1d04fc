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
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAX_CLASSES = 32
MAX_STATES = 256


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


def from_transitions(cls, class_names: Sequence[str], transitions: Sequence[Tuple[str, str, str]], start: str,
                     accepting: Optional[Iterable[str]] = None) -> TokenGrammar:
    """a TokenGrammar from (state, class, successor) triples by name; states are numbered in order of appearance, `start` first"""
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
    return TokenGrammar(cls, allow, nxt, 0, acc, class_names, states)


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


def music_grammar(vocab) -> TokenGrammar:
    """the grammar above for a MusicVocabulary of any pitch kind: the class of a token is its `vocab.type`, and every special
    token ([PAD] and [OMIT] included) is a class of its own"""
    cid = {c: i for i, c in enumerate(MUSIC_CLASSES)}
    cls = np.zeros(len(vocab), dtype=np.uint8)
    for tok, i in vocab.tok2id.items():
        typ = vocab.type(tok)
        name = tok if typ == 'special' else typ
        if name not in cid:
            raise ValueError(f'token {tok!r} has no class in the music grammar')
        cls[i] = cid[name]
    return from_transitions(cls, MUSIC_CLASSES, MUSIC_TRANSITIONS, 'S0', accepting=['END'])
