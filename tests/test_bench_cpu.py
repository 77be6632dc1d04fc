"""bench.py's options on CPU: a plain run measures the headline only (`--full` brings back every other measurement), and
`--dump-outputs` writes float32 arrays as DIR/<name>.npy."""
import os

import numpy as np

import bench


def test_plain_run_implies_no_extras_and_full_keeps_them():
    a = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_roofline and a.no_context_legs
    f = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2', '--full', '--dump-outputs', 'out'])
    assert f.full and f.dump_outputs == 'out'
    assert not (f.no_cpu_baseline or f.no_roofline or f.no_context_legs)
    assert bench.parse_args(['--full', '--no-cpu-baseline']).no_cpu_baseline


def test_dump_outputs_writes_float32_npy(tmp_path):
    losses = np.linspace(6.5, 7.5, 24, dtype=np.float32).reshape(4, 6)
    bench.dump_outputs(str(tmp_path / 'd'), {'losses': losses, 'loss': np.float32(7.0)})
    assert sorted(os.listdir(tmp_path / 'd')) == ['loss.npy', 'losses.npy']
    got = np.load(tmp_path / 'd' / 'losses.npy')
    assert got.dtype == np.float32 and np.array_equal(got, losses)
    assert np.load(tmp_path / 'd' / 'loss.npy').dtype == np.float32
