"""The one-step reference of beam search that the kernel tests stand on, and the device state they compare it with: a plain-Python
restatement of one step of generate's host beam loop for every item -- HF 4.25.1 beam_search / group_beam_search +
HammingDiversityLogitsProcessor + BeamSearchScorer.process with one store per item -- over a slot store, with the candidate order
(score descending, flat index ascending) that mxl_beam_step and mxl_group_beam_step promise.  Plain beam search is ng = 1, pen = 0.
tests/test_group_beam_cpu.py ties it to generate.beam_search and generate.group_beam_search step for step, without a GPU.  The scores
are formed in f32 on both sides, product, difference and sum each rounded on its own (at ng = 1 the one sum), so indices, tokens,
ids, words, running scores, store contents and flags are compared exactly and only the length-normalised scores (powf against
Python's **) to rtol 1e-6."""
import torch

NEG = float('-inf')
MXL_EINVAL = -1


# ---------------------------------------------------------------------------------------------------------------- reference
class RefState:
    """the state one step reads and writes, on the host: ids (rows, ld) int64, scores (rows,) f32, the store as per item a list of
    [score, tokens] slots, done flags, words (n_words, rows) int"""

    def __init__(self, ids, scores, Bs, nb, words):
        self.ids, self.scores, self.Bs, self.nb = ids.clone(), scores.clone(), Bs, nb
        self.hyp = [[] for _ in range(Bs)]
        self.done = [False] * Bs
        self.n_done = 0
        self.words = words.clone()
        self.events = set()


def ref_step(st: RefState, logp: torch.Tensor, V: int, cur_len: int, eos: int, pad: int, lp: float, early: bool, ng: int = 1,
             pen: float = 0.0):
    """one mxl_beam_step (ng = 1) or mxl_group_beam_step on the host; returns (beam_idx, moved).  Events, into st.events: 'hamming1' / 'hamming2' (a token
    counted once / at least twice moved or left a group's 2 * gs best), 'added' / 'replaced' / 'rejected' / 'skipped' (an eos),
    'cut' (the item became done in a group that is not its last: the groups behind are not walked), 'frozen', 'dead', and
    'dead_uncounted' (a group scored under a penalty while an earlier group of the item holds a dead row)."""
    nb, gs = st.nb, st.nb // ng
    pen32 = torch.tensor(pen, dtype=torch.float32)
    beam_idx, moved = [], []
    new_ids, new_words, new_scores = st.ids.clone(), st.words.clone(), st.scores.clone()
    for b in range(st.Bs):
        r0 = b * nb
        if st.done[b]:
            st.events.add('frozen')
            beam_idx += list(range(r0, r0 + nb))
            moved.append(0)
            new_ids[r0:r0 + nb, cur_len] = pad
            new_words[0, r0:r0 + nb] = 0
            continue
        src, toks, dead = list(range(nb)), [pad] * nb, [False] * nb
        scs = st.scores[r0:r0 + nb].tolist()
        hyp, chosen, d = st.hyp[b], [], False
        for g in range(ng):
            if d:
                st.events.add('cut')
                break
            g0 = g * gs
            lo, hi = r0 + g0, r0 + g0 + gs
            cnt = torch.zeros(V, dtype=torch.float32)
            for t in chosen:
                cnt[t] += 1
            plain = logp[lo:hi, :V] + st.scores[lo:hi, None]
            sums = (logp[lo:hi, :V] - pen32 * cnt) + st.scores[lo:hi, None]      # f32: the three roundings the kernel makes
            flat = sums.reshape(-1).tolist()
            order = sorted(range(gs * V), key=lambda i: (-(flat[i] + 0.0), i))[:2 * gs]
            if chosen and pen > 0:
                if any(dead[:g0]):
                    st.events.add('dead_uncounted')
                pl = plain.reshape(-1).tolist()
                free = sorted(range(gs * V), key=lambda i: (-(pl[i] + 0.0), i))[:2 * gs]
                for k, i in enumerate(free):
                    if order[k] != i and cnt[i % V] > 0:
                        st.events.add('hamming1' if cnt[i % V] == 1 else 'hamming2')
            n_src, n_tok, n_sc, n_dead = [], [], [], []
            for rank, i in enumerate(order):
                j, v, s = i // V, i % V, flat[i]
                if v == eos:
                    if rank >= gs:
                        st.events.add('skipped')
                        continue
                    sc = s / cur_len ** lp
                    row = st.ids[lo + j, :cur_len].tolist()
                    if len(hyp) < nb:
                        hyp.append([sc, row])
                        st.events.add('added')
                    else:
                        worst = min(range(nb), key=lambda k: (hyp[k][0], k))
                        if sc > hyp[worst][0]:
                            hyp[worst] = [sc, row]
                            st.events.add('replaced')
                        else:
                            st.events.add('rejected')
                else:
                    n_src.append(g0 + j); n_sc.append(s); n_dead.append(s == NEG); n_tok.append(pad if s == NEG else v)
                if len(n_src) == gs:
                    break
            assert len(n_src) == gs
            src[g0:g0 + gs], toks[g0:g0 + gs], scs[g0:g0 + gs], dead[g0:g0 + gs] = n_src, n_tok, n_sc, n_dead
            chosen += [t for t, x in zip(n_tok, n_dead) if not x]
            if len(hyp) >= nb:
                d = True if early else min(h[0] for h in hyp) >= flat[order[0]] / cur_len ** lp
        for j in range(nb):
            new_ids[r0 + j, :cur_len] = st.ids[r0 + src[j], :cur_len]
            new_ids[r0 + j, cur_len] = toks[j]
            new_words[:, r0 + j] = st.words[:, r0 + src[j]]
            new_scores[r0 + j] = scs[j]
        for j in range(nb):
            if dead[j] or d:
                new_words[0, r0 + j] = 0
        if any(dead):
            st.events.add('dead')
        if d:
            st.done[b] = True
            st.n_done += 1
        beam_idx += [r0 + j for j in src]
        moved.append(int(src != list(range(nb))))
    st.ids, st.words, st.scores = new_ids, new_words, new_scores
    return beam_idx, moved


# ---------------------------------------------------------------------------------------------------------------- device side
class DevState:
    def __init__(self, ref: RefState, ld: int, dev):
        Bs, nb = ref.Bs, ref.nb
        rows = Bs * nb
        i32 = dict(device=dev, dtype=torch.int32)
        self.ids, self.scores, self.words = ref.ids.to(dev), ref.scores.to(dev), ref.words.to(dev, torch.int32).contiguous()
        self.hyp_ids = torch.full((Bs, nb, ld), -7, device=dev, dtype=torch.int64)
        self.hyp_len, self.hyp_score = torch.zeros(Bs, nb, **i32), torch.zeros(Bs, nb, device=dev)
        self.hyp_n, self.done, self.n_done = torch.zeros(Bs, **i32), torch.zeros(Bs, **i32), torch.zeros(1, **i32)
        self.beam_idx, self.moved = torch.full((rows,), -1, **i32), torch.full((Bs,), -1, **i32)
        self.t = torch.zeros(1, **i32)

    def step(self, logp, V, cur_len, eos, pad, lp, early, words=True, ng=1, pen=0.0):
        from symbolic_music_generation_amd import ops
        self.t.fill_(cur_len - 1)
        ops.beam_step(logp, V, self.scores, self.ids, self.t, self.hyp_len.shape[1], eos, pad, lp, early, self.hyp_ids, self.hyp_len,
                      self.hyp_score, self.hyp_n, self.done, self.n_done, self.beam_idx, self.moved,
                      words=self.words if words else None, n_words=self.words.shape[0] if words else 0, ng=ng, diversity_penalty=pen)


def compare(ref: RefState, d: DevState, beam_idx, moved, what):
    assert d.beam_idx.tolist() == beam_idx, what
    assert d.moved.tolist() == moved, what
    assert torch.equal(d.ids.cpu(), ref.ids), what
    assert torch.equal(d.words.cpu().to(torch.int64), ref.words), what
    got, want = d.scores.cpu(), ref.scores
    assert torch.equal(got == NEG, want == NEG), what
    fin = want != NEG
    assert torch.equal(got[fin], want[fin]), what                          # the same three f32 roundings
    assert d.done.tolist() == [int(x) for x in ref.done] and int(d.n_done) == ref.n_done, what
    assert d.hyp_n.tolist() == [len(h) for h in ref.hyp], what
    hyp_ids, hyp_len, hyp_score = d.hyp_ids.cpu(), d.hyp_len.tolist(), d.hyp_score.tolist()
    for b, hyp in enumerate(ref.hyp):
        for k, (sc, row) in enumerate(hyp):
            assert hyp_len[b][k] == len(row) and hyp_ids[b, k, :len(row)].tolist() == row, (what, b, k)
            if sc == NEG:
                assert hyp_score[b][k] == NEG, (what, b, k)
            else:
                assert abs(hyp_score[b][k] - sc) <= 1e-6 * abs(sc), (what, b, k, hyp_score[b][k], sc)


def distinct_logp(rows, ldl, g):
    """pairwise distinct values in (-6, -1), spaced 5 / (rows * ldl) apart"""
    n = rows * ldl
    return (-1.0 - 5.0 * torch.randperm(n, generator=g).to(torch.float64) / n).to(torch.float32).view(rows, ldl)
