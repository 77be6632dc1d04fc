"""bench.py's plain run on the GPU (the tiny workload through the real training leg): the result line, and `--dump-outputs`
writing what the last timed step computed, the same from one run to the next."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--workload', 'tiny',
           '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_last_step(dev, tmp_path):
    out, dumps = _bench(tmp_path / 'a')
    assert out['steps'] == 3 and out['warmup'] == 1 and out['ms_per_step'] > 0 and out['value'] > 0
    assert out['unit'] == 'tokens/s' and out['higher_is_better'] is True and out['dtype'] == 'bf16'
    assert not {'roofline', 'cpu_baseline', 'decode', 'reformer', 'context'} & set(out), 'a plain run measures the headline only'
    assert set(dumps) == {'loss', 'losses', 'grad_norm'}
    assert dumps['losses'].shape == (8, 255) and dumps['loss'].shape == dumps['grad_norm'].shape == ()
    for name, a in dumps.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert 0.0 < float(dumps['loss']) < 2 * np.log(1190) and float(dumps['grad_norm']) > 0
    # same arguments, same inputs: a second process computes the same outputs, element for element, to within one bf16
    # rounding step (2^-7 relative).  Not bit for bit: the weight gradients' fp32 atomics may add in another order.
    _, again = _bench(tmp_path / 'b')
    assert set(again) == set(dumps)
    for name in dumps:
        np.testing.assert_allclose(again[name], dumps[name], rtol=2.0 ** -7, atol=0, err_msg=name)
