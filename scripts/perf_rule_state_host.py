"""Host cost of an eager sampler tail through RowRules, as XLDecoder._sample_advance calls it: 300 steps x 7 rounds after a warm-up
round, 64 rows, the stop, grammar, budget, count, key and register groups on, top-k sampling, the host clock around the loop and a
synchronise after it.  Arms: `fused` (ops.sample_step), `unfused` (generate.sample_unfused) and `fused_flat` (ops.sample_step given
the 28 fields as flat keywords, as the kernel tests call it).  Every step copies the scores back from a fixed tensor, since the
unfused mask writes into them.  Prints one line per arm and, with an output path, writes the rounds as JSON; the digest of the ids
and the packed words after the last round tells whether two packages computed the same.

    python scripts/perf_rule_state_host.py [package root] [label] [out.json]

`package root`: a directory that holds another copy of the package (with its built library) and `include/`, to compare two commits
turn about on one card; default: this tree.  It runs with a package from before ops.RuleState as well.

    python scripts/perf_rule_state_host.py --construct

needs no GPU: what building the 28 fields costs as a frozen dataclass and as a NamedTuple (timeit, us per call)."""
import hashlib
import json
import os
import statistics
import sys
import time
import timeit

FIELDS = ('stop unfinished alive grammar gstate gbar grem gleft in_key gkey melody guide glen gpos gforce register grange gpart gfloor '
          'gap repeat plan nplan barcol span gbars gcopy gstop').split()


def construct():
    body = ''.join(f'    {n}: object = None\n' for n in FIELDS)
    ns = {}
    exec('from dataclasses import dataclass\nfrom typing import NamedTuple\n@dataclass(frozen=True)\nclass F:\n' + body
         + 'class T(NamedTuple):\n' + body, ns)
    F, T = ns['F'], ns['T']
    kw = {n: n for n in FIELDS}
    vals, f, t, n = list(kw.values()), F(**kw), T(**kw), 200000
    from dataclasses import replace
    for name, fn in (('frozen dataclass, by keyword', lambda: F(**kw)), ('frozen dataclass, by position', lambda: F(*vals)),
                     ('frozen dataclass, replace of 2 fields', lambda: replace(f, unfinished=None, alive=None)),
                     ('NamedTuple, by keyword', lambda: T(**kw)), ('NamedTuple, by position', lambda: T(*vals)),
                     ('NamedTuple, _replace of 2 fields', lambda: t._replace(unfinished=None, alive=None)),
                     ('a dict of the 28', lambda: dict(**kw))):
        print(f'{name:40s} {timeit.timeit(fn, number=n) / n * 1e6:6.2f} us')


if '--construct' in sys.argv:
    construct()
    sys.exit(0)

args = sys.argv[1:]
root = os.path.abspath(args[0]) if args else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
side, out_path = (args[1] if len(args) > 1 else 'this'), (args[2] if len(args) > 2 else None)
sys.path.insert(0, root)

import torch  # noqa: E402

from symbolic_music_generation_amd import ops  # noqa: E402
from symbolic_music_generation_amd.generate import RowRules, rules_config, sample_unfused, sampling_config, stop_config  # noqa: E402
from symbolic_music_generation_amd.vocab import MusicTokenizer  # noqa: E402

assert ops.__file__.startswith(root), (ops.__file__, root)
NEW = hasattr(ops, 'RuleState')
B, STEPS, ROUNDS, WARM, D = 64, 300, 7, 20, 64
dev = torch.device('cuda:0')
tok = MusicTokenizer(pitch_kind='degree')
voc = tok.vocab
V = len(voc)
g, key, reg = tok.grammar(bar_budget=True), tok.key_rule(), tok.register_rule()
prompt = [voc.t2i(t) for t in 'TimeSig_4/4 Tempo_120 Key_CMajor <bar> <melody>'.split()]
Tp = len(prompt)
W = Tp + STEPS + WARM + 8                      # every round restarts at column Tp - 1 and writes at most STEPS columns
stop = stop_config(voc.t2i('</s>'), voc.t2i('[PAD]'))
plan = rules_config(batch=B, vocab_size=V, stop=stop, grammar=g, n_bars=1000, in_key=key, register=reg, melody_range=(48, 84),
                    bass_range=(36, 60), bass_below=0)             # (n_bars 1000: no row ends inside a round)
sampling = sampling_config(do_sample=True, top_k=8)
gen = torch.Generator(device=dev).manual_seed(5)
base = 3.0 * torch.randn(B, V, device=dev, generator=gen)
scores = base.clone()
E = torch.randn(V, D, device=dev, generator=gen).to(torch.bfloat16)
emb = torch.zeros(B, D, device=dev, dtype=torch.bfloat16)
ids = torch.zeros(B, W, device=dev, dtype=torch.int64)
t = torch.zeros(1, device=dev, dtype=torch.int32)
ctr = torch.zeros(1, device=dev, dtype=torch.int32)
rng = torch.zeros(1, device=dev, dtype=torch.int64)
rules = RowRules(B, dev)
state = rules.state if NEW else rules.kwargs    # (before ops.RuleState: a dict of the keywords, built per call)
seed = 13


def restart():
    ids.zero_()
    ids[:, :Tp] = torch.tensor(prompt, device=dev)
    t.fill_(Tp - 1)
    rng.zero_()
    rules.start(ids, Tp, V, plan)
    rules.check_prompt(ids)


def fused():
    if NEW:
        ops.sample_step(scores, V, ids, t, rng, seed, E, emb, 1.0, ctr, state(), **sampling)
    else:
        ops.sample_step(scores, V, ids, t, rng, seed, E, emb, 1.0, ctr, **state(), **sampling)


def fused_flat():
    kw = state()
    ops.sample_step(scores, V, ids, t, rng, seed, E, emb, 1.0, ctr, **(kw._asdict() if NEW else kw), **sampling)


def unfused():
    if NEW:
        sample_unfused(scores, V, ids, t, rng, seed, sampling, state())
    else:
        sample_unfused(scores, V, ids, t, rng, seed, sampling, **state())


res = dict(side=side, package=root, new=NEW, arms={})
for name, step in (('fused', fused), ('unfused', unfused), ('fused_flat', fused_flat)):
    enq, drained, digest = [], [], None
    for r in range(ROUNDS + 1):                # round 0: warm-up, not kept
        restart()
        n = WARM if r == 0 else STEPS
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            scores.copy_(base)
            step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert int(t) == Tp - 1 + n
        if r:
            enq.append((t1 - t0) / n * 1e6)
            drained.append((t2 - t0) / n * 1e6)
            digest = hashlib.sha256(ids.cpu().numpy().tobytes() + rules.buf.cpu().numpy().tobytes()).hexdigest()[:16]
    res['arms'][name] = dict(enqueue_us=enq, drained_us=drained, ids_and_words=digest)
    print(f'{side} {name}: median {statistics.median(enq):.2f} us/step enqueue ({min(enq):.2f} .. {max(enq):.2f}), '
          f'drained {statistics.median(drained):.2f}, ids+words {digest}', flush=True)
if out_path:
    with open(out_path, 'w') as f:
        json.dump(res, f)
