"""What the bar budget costs per decode step on top of the grammar, at the C5 decode shape of `bench.py --mode decode` (12L/768d,
M = 2048, V = 1190, 64 rows, prompts of 256 tokens, top_k = 8, two decode lanes, hipGraph replay): the same window of replayed steps
under `tokenizer.grammar(bar_budget=True)` and under `tokenizer.grammar()`, alternating the two ROUNDS times in one process, as
scripts/perf_decode_grammar.py does for the grammar itself.  The spread is each variant's max - min over the rounds.

    python3 scripts/perf_decode_budget.py                      # env: ROUNDS (6), STEPS (400)
    python3 scripts/perf_decode_budget.py --only budget        # one variant, 50 steps: for rocprofv3 --kernel-trace --stats
    python3 scripts/perf_decode_budget.py --only grammar
"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd.generate import XLDecoderLanes, check_bar_lengths, check_grammar, rules_config
from symbolic_music_generation_amd.transformer_xl import MyTransfoXLConfig, MyTransfoXLLMHeadModel
from symbolic_music_generation_amd.vocab import MusicVocabulary

dev = torch.device('cuda:0')
V, M, B, Tp, L = 1190, 2048, 64, 256, 2048
ROUNDS, STEPS = int(os.environ.get('ROUNDS', 6)), int(os.environ.get('STEPS', 400))
ONLY = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None

vocab = MusicVocabulary(pitch_kind='degree')
assert len(vocab) == V
grammars = {'grammar': vocab.grammar(), 'budget': vocab.grammar(bar_budget=True)}
cfg = MyTransfoXLConfig('base', max_length=L, vocab_size=V, mem_len=M, cutoffs=[])
model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()


def prompts():
    """64 song openings of 256 tokens in 4/4 whose bars are full: four quarter notes in the melody, one whole note in the bass"""
    g = torch.Generator().manual_seed(77)
    t = vocab.t2i
    pitch = [i for tok, i in vocab.tok2id.items() if vocab.type(tok) == 'pitch']
    rows = []
    for _ in range(B):
        pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=g))]
        row = [t('TimeSig_4/4'), t('Tempo_120'), t('Key_CMajor')]
        while len(row) < Tp:
            row += [t('<bar>'), t('<melody>')]
            for _ in range(4):
                row += [pick(pitch), t('d_1')]
            row += [t('<bass>'), pick(pitch), t('d_4')]
        rows.append(row[:Tp])
    return torch.tensor(rows, dtype=torch.int64, device=dev)


ids = prompts()
samp = dict(do_sample=True, top_k=8, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0)


def window(dec, g, steps):
    """ms per replayed step over `steps` steps right after the prompt pass (ring slots Tp .. Tp + 20 + steps)"""
    n = dec.begin(ids, L, samp, use_graph=True, rules=rules_config(batch=B, vocab_size=V, grammar=g))
    assert n >= steps + 20
    for _ in range(20):
        dec.replay_once()
    dec.join()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dec.replay_once()
    dec.join()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


with torch.no_grad():
    assert check_grammar(ids, grammars['grammar']).tolist() == [-1] * B
    assert check_bar_lengths(ids, grammars['budget']).tolist() == [-1] * B
    if ONLY:
        dec = XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)
        print(f'{ONLY}: {window(dec, grammars[ONLY], 50):.3f} ms per step (50 steps)', flush=True)
        sys.exit(0)
    decs = {k: XLDecoderLanes(model.engine, B, L, seed=5, lanes=2) for k in grammars}
    for name, dec in decs.items():                                  # warm-up: library attributes, workspaces, graph capture
        window(dec, grammars[name], 20)
    ms = {k: [] for k in grammars}
    for r in range(ROUNDS):
        for name in (('grammar', 'budget') if r % 2 == 0 else ('budget', 'grammar')):
            ms[name].append(window(decs[name], grammars[name], STEPS))
        print(f'round {r}: grammar {ms["grammar"][-1]:.4f} ms/step, budget {ms["budget"][-1]:.4f} ms/step', flush=True)
    for k in grammars:
        out = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs[k].lanes], 0)
        print(f'{k:8s}: rows that obey the grammar {int((check_grammar(out, grammars["grammar"]) < 0).sum())} of {B}, '
              f'rows whose bars are all full {int((check_bar_lengths(out, grammars["budget"]) < 0).sum())} of {B}')
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(f'C5 decode step, {B} rows, 2 lanes, {STEPS} replayed steps x {ROUNDS} alternating rounds')
    for k in ('grammar', 'budget'):
        print(f'  {k:8s} median {med[k]:.4f} ms/step  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}  spread {spread[k]:.4f}')
    d = med['budget'] - med['grammar']
    print(f'  budget - grammar = {d:+.4f} ms/step ({100 * d / med["grammar"]:+.2f} %); run-to-run spread {max(spread.values()):.4f} ms')
