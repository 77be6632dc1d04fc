"""What `generate(grammar=...)` costs per decode step at the C5 decode shape of `bench.py --mode decode` (12L/768d, M = 2048,
V = 1190, 64 rows, prompts of 256 tokens, top_k = 8, two decode lanes, hipGraph replay): the same window of replayed steps with
and without the music grammar, alternating the two ROUNDS times in one process.  The baseline is the run without a grammar in
the same process on the same device; the spread is each variant's max - min over the rounds.

    python3 scripts/perf_decode_grammar.py                     # env: ROUNDS (6), STEPS (400)
    python3 scripts/perf_decode_grammar.py --only grammar      # one variant, 50 steps: for rocprofv3 --kernel-trace --stats
    python3 scripts/perf_decode_grammar.py --only plain

`--n-bars K`: what `generate(n_bars=)` costs on top of the bar budget, at the same shape.  Three arms alternate, all under
`tokenizer.grammar(bar_budget=True)` over prompts whose bars are full: `budget` (no eos rule: the arm of
scripts/perf_decode_budget.py), `budget+eos` (the eos rule that n_bars needs, no count; min_length = max_length keeps eos barred, as
the count does in the third arm, so that all 64 rows stay live) and `bars` (the eos rule and n_bars = K for every row; give a K no
row reaches inside the window, e.g. 1000).  `bars - budget+eos` is the cost of the count, `budget+eos - budget` that of the eos rule.

    python3 scripts/perf_decode_grammar.py --n-bars 1000
    python3 scripts/perf_decode_grammar.py --n-bars 1000 --only bars      # or budget, budget+eos: for rocprofv3 --kernel-trace --stats

`--in-key`: what `generate(in_key=)` costs, at the same shape, without a grammar: `plain` against `key` (the key rule over prompts
in C major, every row constrained), alternating as above; the tokens per second of each arm are printed beside the step times.

    python3 scripts/perf_decode_grammar.py --in-key
    python3 scripts/perf_decode_grammar.py --in-key --only key            # or plain

`--register`: what `generate(register=)` costs, at the same shape, without a grammar: `plain` against `register` (the register rule
with melody_range 55..84, bass_range 36..60 and bass_below 1 in every row), alternating as above; the rows that `check_register`
finds clean are printed for each arm.

    python3 scripts/perf_decode_grammar.py --register
    python3 scripts/perf_decode_grammar.py --register --only register     # or plain

`--form K`: what `generate(form=)` costs on top of the bar count, at the same shape, under `tokenizer.grammar(bar_budget=True)` over
prompts whose bars are full: `bars` (the eos rule and n_bars = K for every row, the third arm of --n-bars) against `form` (a plan of K
bars for every row in which every second bar repeats the bar before it, so that half of the bars a row writes are copies), alternating
as above; give a K no row reaches inside the window, e.g. 1000.  The rows that `check_form` finds clean are printed for each arm.

    python3 scripts/perf_decode_grammar.py --form 1000
    python3 scripts/perf_decode_grammar.py --form 1000 --only form        # or bars: for rocprofv3 --kernel-trace --stats
"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from symbolic_music_generation_amd.generate import XLDecoderLanes, check_grammar, rules_config
from symbolic_music_generation_amd.transformer_xl import MyTransfoXLConfig, MyTransfoXLLMHeadModel
from symbolic_music_generation_amd.vocab import MusicVocabulary

dev = torch.device('cuda:0')
V, M, B, Tp, L = 1190, 2048, 64, 256, 2048
ROUNDS, STEPS = int(os.environ.get('ROUNDS', 6)), int(os.environ.get('STEPS', 400))
ONLY = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
N_BARS = int(sys.argv[sys.argv.index('--n-bars') + 1]) if '--n-bars' in sys.argv else None
IN_KEY = '--in-key' in sys.argv
REGISTER = '--register' in sys.argv
FORM = int(sys.argv[sys.argv.index('--form') + 1]) if '--form' in sys.argv else None
FULL_BARS = N_BARS is not None or FORM is not None

vocab = MusicVocabulary(pitch_kind='degree')
assert len(vocab) == V
grammar = vocab.grammar()
cfg = MyTransfoXLConfig('base', max_length=L, vocab_size=V, mem_len=M, cutoffs=[])
model = MyTransfoXLLMHeadModel(cfg, device=dev, seed=77).eval()


def prompts():
    """64 well-formed song openings of 256 tokens: header, then bars of random notes in both channels"""
    g = torch.Generator().manual_seed(77)
    t = vocab.t2i
    pitch = [i for tok, i in vocab.tok2id.items() if vocab.type(tok) == 'pitch']
    dur = [i for tok, i in vocab.tok2id.items() if vocab.type(tok) == 'duration']
    rows = []
    for _ in range(B):
        pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=g))]
        row = [t('TimeSig_4/4'), t('Tempo_120'), t('Key_CMajor')]
        while len(row) < Tp:
            row += [t('<bar>'), t('<melody>')]
            for _ in range(4):                                     # (--n-bars, --form: full bars, four quarter notes over one whole note)
                row += [pick(pitch), pick(dur) if not FULL_BARS else t('d_1')]
            row += [t('<bass>'), pick(pitch), pick(dur) if not FULL_BARS else t('d_4')]
        rows.append(row[:Tp])
    return torch.tensor(rows, dtype=torch.int64, device=dev)


ids = prompts()
samp = dict(do_sample=True, top_k=8, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_p=1.0)


def window(dec, g, steps, **rules):
    """ms per replayed step over `steps` steps right after the prompt pass (ring slots Tp .. Tp + 20 + steps); rules: the arm's
    keywords of generate.rules_config beside the grammar"""
    n = dec.begin(ids, L, samp, use_graph=True, rules=rules_config(batch=B, vocab_size=V, grammar=g, **rules))
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


def bars_arms():
    """the --n-bars comparison (module docstring)"""
    from symbolic_music_generation_amd.generate import bars_after_prompt, check_bar_lengths, stop_config
    g = vocab.grammar(bar_budget=True)
    stop = stop_config(vocab.t2i('</s>'), vocab.t2i('[PAD]'))
    arms = {'budget': {}, 'budget+eos': dict(stop=stop[:2] + (L,)), 'bars': dict(stop=stop, n_bars=N_BARS)}
    assert check_bar_lengths(ids, g).tolist() == [-1] * B
    if ONLY:
        dec = XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)
        print(f'{ONLY}: {window(dec, g, 50, **arms[ONLY]):.3f} ms per step (50 steps)', flush=True)
        return
    decs = {k: XLDecoderLanes(model.engine, B, L, seed=5, lanes=2) for k in arms}
    for name, dec in decs.items():                                  # warm-up: library attributes, workspaces, graph capture
        window(dec, g, 20, **arms[name])
    ms = {k: [] for k in arms}
    names = list(arms)
    for r in range(ROUNDS):
        for name in names[r % 3:] + names[:r % 3]:
            ms[name].append(window(decs[name], g, STEPS, **arms[name]))
        print(f'round {r}: ' + ', '.join(f'{k} {ms[k][-1]:.4f}' for k in names) + ' ms/step', flush=True)
    for k in names:
        out = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs[k].lanes], 0)
        live = sum(int(d.alive) for d in decs[k].lanes) if k != 'budget' else B
        print(f'{k:10s}: rows whose bars are all full {int((check_bar_lengths(out, g) < 0).sum())} of {B}, live rows {live}, '
              f'bars opened per row {bars_after_prompt(out, g, prompt_len=Tp).float().mean():.1f}')
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(f'C5 decode step, {B} rows, 2 lanes, {STEPS} replayed steps x {ROUNDS} alternating rounds, n_bars = {N_BARS}')
    for k in names:
        print(f'  {k:10s} median {med[k]:.4f} ms/step  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}  spread {spread[k]:.4f}')
    for a, b in (('bars', 'budget+eos'), ('budget+eos', 'budget'), ('bars', 'budget')):
        d = med[a] - med[b]
        print(f'  {a} - {b} = {d:+.4f} ms/step ({100 * d / med[b]:+.2f} %); run-to-run spread {max(spread.values()):.4f} ms')


def key_arms():
    """the --in-key comparison (module docstring)"""
    from symbolic_music_generation_amd.generate import check_in_key
    rule = vocab.key_rule()
    arms = {'plain': {}, 'key': dict(in_key=rule)}
    if ONLY:
        dec = XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)
        print(f'{ONLY}: {window(dec, None, 50, **arms[ONLY]):.3f} ms per step (50 steps)', flush=True)
        return
    decs = {k: XLDecoderLanes(model.engine, B, L, seed=5, lanes=2) for k in arms}
    for name, dec in decs.items():                                  # warm-up: library attributes, workspaces, graph capture
        window(dec, None, 20, **arms[name])
    ms = {k: [] for k in arms}
    for r in range(ROUNDS):
        for name in (('plain', 'key') if r % 2 == 0 else ('key', 'plain')):
            ms[name].append(window(decs[name], None, STEPS, **arms[name]))
        print(f'round {r}: plain {ms["plain"][-1]:.4f} ms/step, key {ms["key"][-1]:.4f} ms/step', flush=True)
    for k in arms:
        out = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs[k].lanes], 0)
        print(f'{k:6s}: rows that stay in key {int((check_in_key(out, rule, prompt_len=Tp) < 0).sum())} of {B}')
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(f'C5 decode step, {B} rows, 2 lanes, {STEPS} replayed steps x {ROUNDS} alternating rounds')
    for k in arms:
        print(f'  {k:6s} median {med[k]:.4f} ms/step = {1e3 * B / med[k]:.0f} tok/s  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}  '
              f'spread {spread[k]:.4f}')
    d = med['key'] - med['plain']
    print(f'  key - plain = {d:+.4f} ms/step ({100 * d / med["plain"]:+.2f} %); run-to-run spread {max(spread.values()):.4f} ms')


def register_arms():
    """the --register comparison (module docstring)"""
    from symbolic_music_generation_amd.generate import check_register
    rule = vocab.register_rule()
    bounds = dict(melody_range=(55, 84), bass_range=(36, 60), bass_below=1)
    arms = {'plain': {}, 'register': dict(register=rule, **bounds)}
    if ONLY:
        dec = XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)
        print(f'{ONLY}: {window(dec, None, 50, **arms[ONLY]):.3f} ms per step (50 steps)', flush=True)
        return
    decs = {k: XLDecoderLanes(model.engine, B, L, seed=5, lanes=2) for k in arms}
    for name, dec in decs.items():                                  # warm-up: library attributes, workspaces, graph capture
        window(dec, None, 20, **arms[name])
    ms = {k: [] for k in arms}
    for r in range(ROUNDS):
        for name in (('plain', 'register') if r % 2 == 0 else ('register', 'plain')):
            ms[name].append(window(decs[name], None, STEPS, **arms[name]))
        print(f'round {r}: plain {ms["plain"][-1]:.4f} ms/step, register {ms["register"][-1]:.4f} ms/step', flush=True)
    for k in arms:
        out = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs[k].lanes], 0)
        print(f'{k:8s}: rows clean under check_register {int((check_register(out, rule, **bounds, prompt_len=Tp) < 0).sum())} of {B}')
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(f'C5 decode step, {B} rows, 2 lanes, {STEPS} replayed steps x {ROUNDS} alternating rounds')
    for k in arms:
        print(f'  {k:8s} median {med[k]:.4f} ms/step = {1e3 * B / med[k]:.0f} tok/s  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}  '
              f'spread {spread[k]:.4f}')
    d = med['register'] - med['plain']
    print(f'  register - plain = {d:+.4f} ms/step ({100 * d / med["plain"]:+.2f} %); run-to-run spread {max(spread.values()):.4f} ms')


def form_arms():
    """the --form comparison (module docstring)"""
    from symbolic_music_generation_amd.generate import bars_after_prompt, check_bar_lengths, check_form, form_config, stop_config
    g = vocab.grammar(bar_budget=True)
    stop = stop_config(vocab.t2i('</s>'), vocab.t2i('[PAD]'))
    plan = [-1 if k % 2 == 0 else k - 1 for k in range(FORM)]
    arms = {'bars': dict(stop=stop, n_bars=FORM), 'form': dict(stop=stop, melody=form_config(plan, None, None, B, g, stop))}
    assert check_bar_lengths(ids, g).tolist() == [-1] * B
    if ONLY:
        dec = XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)
        print(f'{ONLY}: {window(dec, g, 50, **arms[ONLY]):.3f} ms per step (50 steps)', flush=True)
        return
    decs = {k: XLDecoderLanes(model.engine, B, L, seed=5, lanes=2) for k in arms}
    for name, dec in decs.items():                                  # warm-up: library attributes, workspaces, graph capture
        window(dec, g, 20, **arms[name])
    ms = {k: [] for k in arms}
    for r in range(ROUNDS):
        for name in (('bars', 'form') if r % 2 == 0 else ('form', 'bars')):
            ms[name].append(window(decs[name], g, STEPS, **arms[name]))
        print(f'round {r}: bars {ms["bars"][-1]:.4f} ms/step, form {ms["form"][-1]:.4f} ms/step', flush=True)
    for k in arms:
        out = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs[k].lanes], 0)
        print(f'{k:5s}: rows whose bars are all full {int((check_bar_lengths(out, g) < 0).sum())} of {B}, rows clean under check_form '
              f'{int((check_form(out, g, plan, prompt_len=Tp) < 0).sum())} of {B}, live rows {sum(int(d.alive) for d in decs[k].lanes)}, '
              f'bars opened per row {bars_after_prompt(out, g, prompt_len=Tp).float().mean():.1f}')
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(f'C5 decode step, {B} rows, 2 lanes, {STEPS} replayed steps x {ROUNDS} alternating rounds, a plan of {FORM} bars')
    for k in arms:
        print(f'  {k:5s} median {med[k]:.4f} ms/step = {1e3 * B / med[k]:.0f} tok/s  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}  '
              f'spread {spread[k]:.4f}')
    d = med['form'] - med['bars']
    print(f'  form - bars = {d:+.4f} ms/step ({100 * d / med["bars"]:+.2f} %); run-to-run spread {max(spread.values()):.4f} ms')


with torch.no_grad():
    assert check_grammar(ids, grammar).tolist() == [-1] * B
    if FORM is not None:
        form_arms()
        sys.exit(0)
    if REGISTER:
        register_arms()
        sys.exit(0)
    if IN_KEY:
        key_arms()
        sys.exit(0)
    if N_BARS is not None:
        bars_arms()
        sys.exit(0)
    if ONLY:
        dec = XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)
        print(f'{ONLY}: {window(dec, grammar if ONLY == "grammar" else None, 50):.3f} ms per step (50 steps)', flush=True)
        sys.exit(0)
    decs = {'plain': XLDecoderLanes(model.engine, B, L, seed=5, lanes=2), 'grammar': XLDecoderLanes(model.engine, B, L, seed=5, lanes=2)}
    for name, dec in decs.items():                                  # warm-up: library attributes, workspaces, graph capture
        window(dec, grammar if name == 'grammar' else None, 20)
    ms = {'plain': [], 'grammar': []}
    for r in range(ROUNDS):
        for name in (('plain', 'grammar') if r % 2 == 0 else ('grammar', 'plain')):
            ms[name].append(window(decs[name], grammar if name == 'grammar' else None, STEPS))
        print(f'round {r}: plain {ms["plain"][-1]:.4f} ms/step, grammar {ms["grammar"][-1]:.4f} ms/step', flush=True)
    out = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs['grammar'].lanes], 0)
    free = torch.cat([d.ids[:, :Tp + 20 + STEPS] for d in decs['plain'].lanes], 0)
    print(f'rows that obey the grammar: with grammar {int((check_grammar(out, grammar) < 0).sum())} of {B}, '
          f'without {int((check_grammar(free, grammar) < 0).sum())} of {B}')
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(f'C5 decode step, {B} rows, 2 lanes, {STEPS} replayed steps x {ROUNDS} alternating rounds')
    for k in ('plain', 'grammar'):
        print(f'  {k:8s} median {med[k]:.4f} ms/step  min {min(ms[k]):.4f}  max {max(ms[k]):.4f}  spread {spread[k]:.4f}')
    d = med['grammar'] - med['plain']
    print(f'  grammar - plain = {d:+.4f} ms/step ({100 * d / med["plain"]:+.2f} %); run-to-run spread {max(spread.values()):.4f} ms')
