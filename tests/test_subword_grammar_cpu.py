"""The grammar of the sub-word tokenizers on the host (grammar.subword_grammar; `PairMergeTokenizer.grammar()`,
`WordPieceMusicTokenizer.grammar()`): the composed tables against the BASE tables walked over every id's pieces, exhaustively, on
tokenizers trained on the fixture song (pair-merge: coverage 0.9; WordPiece: base + 400), three pitch kinds, and on a hand-made
vocabulary that keeps the flagged tokens covered where `tokenizers` is absent.  A flagged token ends on an open note start (`p d p`):
bit 15 of its `slots` entry says that it needs one slot more free than it takes."""
import numpy as np
import pytest

from symbolic_music_generation_amd import grammar as G
from symbolic_music_generation_amd.generate import check_bar_lengths, check_grammar, rules_config
from symbolic_music_generation_amd.grammar import NEED_ONE_MORE, NO_SIG, RARE_SLOTS, BarBudget, subword_grammar
from symbolic_music_generation_amd.vocab import MusicVocabulary
from tests import subword_rules as SR
from tests.rules_ref import Rules, Words, keep

CASES = [(s, k) for s in ('pairmerge', 'wordpiece') for k in SR.KINDS] + [('handmade', 'midi')]
BARS = (32, 24, 12)


@pytest.fixture(params=CASES, ids=lambda c: f'{c[0]}-{c[1]}')
def case(request):
    scheme, kind = request.param
    if scheme == 'wordpiece':
        pytest.importorskip('tokenizers')
    return (scheme, kind) + SR.grammars(scheme, kind)


def test_sizes_are_those_of_the_reference_settings(case):
    scheme, kind, tok, pieces, base, g = case
    assert g.vocab_size == tok.vocab_size == len(pieces) and g.n_states == base.n_states and g.start == base.start
    assert g.accepting == base.accepting and g.state_names == base.state_names
    assert base.n_classes < g.n_classes <= 32 and g.class_names[:base.n_classes] == base.class_names
    assert g.budget is not None and g.bar_count is not None and g.guide is None
    assert (g.bar_count.count, g.bar_count.end) == (base.bar_count.count, base.bar_count.end)
    assert (g.budget.opens, g.budget.need_free, g.budget.need_full) == (base.budget.opens, base.budget.need_free, base.budget.need_full)
    single = SR.single_of(pieces)
    assert sorted(single) == list(range(base.vocab_size))           # every base token keeps a single-token id
    assert len(SR.multis(pieces)) >= 40
    plain = tok.grammar()                                            # without the budget: the same automaton
    assert plain.budget is None and plain.bar_count is not None and np.array_equal(plain.cls, g.cls)
    assert np.array_equal(plain.allow, g.allow) and np.array_equal(plain.next, g.next)


def test_composition_exhaustively(case):
    """every id, every base state: the composed allow / next are the base tables walked over the id's pieces"""
    scheme, kind, tok, pieces, base, g = case
    seen_dead = 0
    for v, seq in enumerate(pieces):
        c = int(g.cls[v])
        if len(seq) == 1:
            assert c == int(base.cls[seq[0]]) and g.class_names[c] == base.class_names[c]
        else:
            assert c >= base.n_classes
        ends = [SR.base_state_walk(base, seq, s) for s in range(base.n_states)]
        seen_dead += all(e < 0 for e in ends)
        for s, e in enumerate(ends):
            assert bool((int(g.allow[s]) >> c) & 1) == (e >= 0), (v, seq, s)
            if e >= 0:
                assert int(g.next[s, c]) == e, (v, seq, s)
    if scheme == 'handmade':
        assert seen_dead > 0                                         # [p, p, d, p]: a class that no state allows


def test_budget_exhaustively(case):
    """every multi-base id, bars of 32, 24 and 12 slots, every rem in 0..bar+1: allows / move against the base budget over the pieces"""
    scheme, kind, tok, pieces, base, g = case
    bud, n = g.budget, 0
    for v in SR.multis(pieces):
        c, k, sig = int(g.cls[v]), int(bud.slots[v]), int(bud.bars[v])
        assert sig == NO_SIG
        for bar in BARS + (0,):
            for rem in range(0, bar + 2):
                ok, b1, r1 = SR.base_budget_walk(base, pieces[v], bar, rem)
                assert bud.allows(bar, rem, c, k) == ok, (v, pieces[v], bar, rem)
                if ok:
                    assert bud.move(bar, rem, c, k, sig) == (b1, r1), (v, pieces[v], bar, rem)
                n += 1
    assert n >= 40 * (32 + 24 + 12 + 6)
    for v, seq in enumerate(pieces):                                 # the singles: the base entries bit for bit
        if len(seq) == 1:
            assert (int(bud.slots[v]), int(bud.bars[v])) == (int(base.budget.slots[seq[0]]), int(base.budget.bars[seq[0]]))
    fl = SR.flagged(g)
    assert all(int(base.cls[pieces[v][-1]]) in _class_ids(base, base.budget.need_free) for v in fl)
    if scheme != 'pairmerge':
        assert fl
    else:
        assert not fl                                                # whole notes and whole tuplets never end on an open pitch


def _class_ids(g, mask):
    return {c for c in range(g.n_classes) if (mask >> c) & 1}


def test_real_streams(case):
    """the encoded fixtures: at every prefix the composed walks give what the base walks give on the expansion"""
    scheme, kind, tok, pieces, base, g = case
    ids = SR.encode(scheme, kind, SR.song_text(kind))
    full = SR.expand(pieces, ids)
    assert full == SR.fixture(f'sample_full_{kind}').tolist()
    off = SR.offsets(pieces, ids)
    s, bar, rem = g.start, 0, 0                                      # the composed words, moved a column at a time
    bs, bbar, brem = base.start, 0, 0                                # the base's, moved over that column's pieces
    for n, t in enumerate(ids):
        (s, bad), (bar, rem, over) = g.walk([t], s), g.walk_budget([t], bar, rem)
        assert bad == over == -1, n
        exp = full[off[n]:off[n + 1]]
        bs = SR.base_state_walk(base, exp, bs)
        ok, bbar, brem = SR.base_budget_walk(base, exp, bbar, brem)
        assert ok and (s, bar, rem) == (bs, bbar, brem), n
        if n % 97 == 0 or n == len(ids) - 1:                         # and both from the start of the row, now and then
            assert g.walk(ids[:n + 1]) == base.walk(full[:off[n + 1]]) == (s, -1)
            assert g.walk_budget(ids[:n + 1]) == base.walk_budget(full[:off[n + 1]]) == (bar, rem, -1)
    for start in (0, 7, 40, len(ids) // 2):
        for left in (-1, 0, 1, 3, 1000):
            got, want = g.walk_bars(ids[start:], left), base.walk_bars(full[off[start]:], left)
            assert got[0] == want[0] and got[1] == SR.column_of(pieces, ids[start:], want[1]), (start, left)
    assert g.accepts(ids) and g.state_names[g.walk(ids)[0]] == 'END' and g.walk_budget(ids)[1] == 0
    assert check_grammar(np.asarray(ids), g).tolist() == [-1] and check_bar_lengths(np.asarray(ids), g).tolist() == [-1]
    if kind == 'degree':                                             # gen_broken: grammatical, broken in its durations
        text = SR.song_text('degree', 'gen_broken')
        broken = SR.encode(scheme, kind, text)
        exp = SR.expand(pieces, broken)
        assert exp == SR.fixture('gen_broken').tolist()
        assert check_grammar(np.asarray(broken), g).tolist() == [-1]
        want = base.walk_budget(exp)[2]
        assert want >= 0
        assert check_bar_lengths(np.asarray(broken), g).tolist() == [SR.column_of(pieces, broken, want)]


def test_random_generation_on_the_host(case):
    """20 walks of 200 steps from a 4/4 header under the composed rules, favouring multi-base ids: the expansion breaks no base rule"""
    scheme, kind, tok, pieces, base, g = case
    v = SR.base_tokenizer(kind).vocab
    single = SR.single_of(pieces)
    header = [single[v.t2i(t)] for t in ('TimeSig_4/4', 'Tempo_120', '<bar>')]
    is_multi = np.array([len(p) > 1 for p in pieces])
    fl = set(SR.flagged(g))
    rules = Rules(g, budget=True, count=True)
    rng = np.random.default_rng(11)
    used, tight = 0, 0
    for _ in range(20):
        row = list(header)
        s, bad = g.walk(row)
        bar, rem, bad2 = g.walk_budget(row)
        assert bad == bad2 == -1
        left = 10 ** 6                                               # the count keeps </s> out: the walk never ends early
        for _ in range(200):
            ok = keep(rules, Words(gstate=s, gbar=bar, grem=rem, gleft=left), g.vocab_size)
            assert ok.any()
            pool = np.nonzero(ok & is_multi)[0]
            if not len(pool) or rng.random() >= 0.7:
                pool = np.nonzero(ok)[0]
            t = int(rng.choice(pool))
            c, k = int(g.cls[t]), int(g.budget.slots[t])
            used += bool(is_multi[t])
            tight += t in fl and rem == BarBudget.slots_need(k)
            s = int(g.next[s, c])
            bar, rem = g.budget.move(bar, rem, c, k, int(g.budget.bars[t]))
            left = g.bar_count.move(left, c)
            row.append(t)
        exp = SR.expand(pieces, row)
        assert base.walk(exp)[1] == -1 and base.walk_budget(exp)[2] == -1
        assert (g.walk(row), g.walk_budget(row)) == ((s, -1), (bar, rem, -1))
    assert used >= 100, used
    if scheme != 'pairmerge':
        assert tight >= 1                                            # a flagged id emitted with exactly its need free


@pytest.mark.parametrize('scheme,kind', [c for c in CASES if c[0] != 'pairmerge'])     # pair-merge tokens never end on an open pitch
def test_teeth_bit_15_is_needed_and_is_no_slot_count(scheme, kind):
    if scheme == 'wordpiece':
        pytest.importorskip('tokenizers')
    tok, pieces, base, g = SR.grammars(scheme, kind)
    bud = g.budget
    fl = SR.flagged(g)
    hit = None
    for (s, bar, rem) in bud._reach:                                 # every (state, bar, rem) the start state reaches
        for t in fl:
            c, k = int(g.cls[t]), int(bud.slots[t])
            if bar > 0 and (int(g.allow[s]) >> c) & 1 and bud.allows(bar, rem, c, k & ~NEED_ONE_MORE) and not bud.allows(bar, rem, c, k):
                assert not SR.base_budget_walk(base, pieces[t], bar, rem)[0]
                hit = (s, bar, rem, t)
                break
        if hit:
            break
    assert hit is not None                                           # with the bit cleared the tables admit what the base bars
    s, bar, rem, t = hit
    k = int(bud.slots[t])
    take = k & (NEED_ONE_MORE - 1)
    assert rem == take
    if take + 1 <= bar:                                              # read as a slot count, the entry bars the id where the base admits it
        assert SR.base_budget_walk(base, pieces[t], bar, take + 1)[0] and bud.allows(bar, take + 1, int(g.cls[t]), k)
        assert not k <= take + 1                                     # `k <= rem`: the rule of an entry that is a count alone
    # and the tables with the bit cleared hold a dead end, which the constructor finds
    g2 = G.TokenGrammar(g.cls, g.allow, g.next, g.start, g.accepting, g.class_names, g.state_names)
    cleared = np.where(bud.slots == RARE_SLOTS, bud.slots, bud.slots & (NEED_ONE_MORE - 1))
    with pytest.raises(ValueError, match='every token barred'):
        BarBudget(g2, cleared, bud.bars, bud.opens, bud.need_free, bud.need_full)


@pytest.mark.parametrize('kind', SR.KINDS)
def test_nothing_moved_in_the_base_tables(kind):
    vocab = MusicVocabulary(pitch_kind=kind)
    slots = vocab.grammar(bar_budget=True).budget.slots
    t = G.music_budget_tables(vocab)
    assert slots.dtype == np.uint16 and np.array_equal(slots, t['slots'])
    assert not ((slots != RARE_SLOTS) & ((slots & NEED_ONE_MORE) != 0)).any()
    assert int((slots == RARE_SLOTS).sum()) == 1
    for k in (0, 1, 48, 0x7FFF):
        assert BarBudget.slots_need(k) == BarBudget.slots_take(k) == k
    assert BarBudget.slots_need(0x8000 | 6) == 7 and BarBudget.slots_take(0x8000 | 6) == 6 and BarBudget.slots_need(RARE_SLOTS) == RARE_SLOTS


def test_refusals():
    hm = SR.tokenizer('handmade', 'midi')
    v = hm.vocab
    base = hm.base.grammar(bar_budget=True)
    marker = [v.t2i('<bar>'), v.t2i('<melody>')]
    with pytest.raises(NotImplementedError, match=rf'sub-word id {len(hm.pieces)} holds base token {marker[0]} of class \'<bar>\''):
        subword_grammar(base, hm.pieces + [marker])
    with pytest.raises(NotImplementedError, match='time_sig'):
        subword_grammar(base, hm.pieces + [[v.t2i('TimeSig_3/4'), v.t2i('Tempo_120')]])
    with pytest.raises(ValueError):
        subword_grammar(base, hm.pieces + [[]])
    # more than 32 classes: without budget the markers may merge, and sequences of two and three tokens over six of the classes
    # induce 36 different functions on the states
    import itertools
    reps = [v.t2i(t) for t in ('p_r', 'd_1', '<tup>', '</tup>', '<melody>', '<bass>')]
    many = [list(s) for n in (2, 3) for s in itertools.product(reps, repeat=n)]
    assert len({tuple(SR.base_state_walk(base, s, st) for st in range(base.n_states)) for s in many}) > 32 - base.n_classes
    with pytest.raises(NotImplementedError, match=r'\d+ token classes \(13 of the base grammar'):
        subword_grammar(hm.base.grammar(), hm.pieces + many)
    # a punctuate=False WordPiece tokenizer merges markers into its words
    if SR.have_tokenizers():
        from symbolic_music_generation_amd.subword import WordPieceMusicTokenizerTrainer
        tr = WordPieceMusicTokenizerTrainer(pitch_kind='midi', punctuate=False)
        wp = tr([SR.song_text('midi')] * 4, vocab_size=len(tr.vocab) + 200)
        with pytest.raises(NotImplementedError, match='sub-word id'):
            wp.grammar(bar_budget=True)
    from symbolic_music_generation_amd.subword import PairMergeTokenizer
    pm = SR.tokenizer('pairmerge', 'midi')
    assert isinstance(pm, PairMergeTokenizer)
    for call in (pm.key_rule, pm.register_rule, lambda: pm.melody_guide([0, 1])):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match='without merged tokens'):      # an untrained tokenizer has no sub-word id to compose
        PairMergeTokenizer({}, pitch_kind='midi').grammar(bar_budget=True)
    g = pm.grammar(bar_budget=True)
    with pytest.raises(ValueError, match='melody needs a grammar with a guide rule'):
        rules_config(batch=1, vocab_size=g.vocab_size, stop=(pm.eos_token_id, pm.pad_token_id, 0), grammar=g, melody=[[1, 2, 3]])
