"""-m gpu: the one-GPU bench line.  A plain run measures the headline only and, with --dump-outputs, writes what its last timed step
computed; --full adds the side measurements (loss-fetching loops, roofline, CPU baseline) to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(args):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + args, env=env, capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(dev, tmp_path):
    d = _line(['--steps', '4', '--warmup', '2', '--dump-outputs', str(tmp_path)])
    assert d['steps'] == 4 and d['warmup'] == 2 and d['n_gpus'] == 1
    assert d['value'] > 0 and d['ms_per_step'] > 0 and abs(d['value'] * d['ms_per_step'] / 1e3 - 64) < 1e-6
    assert d['unit'] == 'images/sec' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    for k in ('roofline', 'cpu_baseline', 'with_loss_fetch_every_step', 'with_loss_read_one_step_behind'):
        assert k not in d, k
    assert d['dropped_steps']['timed'] == 0 and d['lstm_timeouts']['timed'] == 0
    loss = np.load(str(tmp_path / 'loss.npy'))
    assert loss.dtype == np.float64 and loss.shape == (4,) and np.isfinite(loss).all() and loss[0] == d['final_loss']
    params, grads = np.load(str(tmp_path / 'params.npy')), np.load(str(tmp_path / 'grads.npy'))
    assert params.dtype == grads.dtype == np.float32 and params.shape == grads.shape and params.size >= 7158592
    assert np.isfinite(params).all() and np.isfinite(grads).all() and np.abs(grads).max() > 0
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 * 10 ** 6 + 1024


def test_full_line_keeps_the_side_measurements(dev):
    d = _line(['--steps', '4', '--warmup', '2', '--full'])
    assert d['steps'] == 4 and d['value'] > 0 and d['ms_per_step'] > 0
    assert d['with_loss_fetch_every_step']['ms_per_step'] > 0 and d['with_loss_read_one_step_behind']['ms_per_step'] > 0
    assert d['dropped_steps']['side_loops'] == 0 and d['lstm_timeouts']['side_loops'] == 0
    assert 'error' not in d['roofline'] and d['roofline']['achieved'] > 0 and d['roofline']['wgrad']['achieved'] > 0
    cb = d['cpu_baseline']
    assert 'error' not in cb and cb['value'] > 0 and cb['c1_train_images_per_sec'] > 0 and cb['c1_forward_greedy_images_per_sec'] > 0


def test_two_runs_dump_the_same_bits(dev, tmp_path):
    """The same arguments give the same inputs AND the same trained state: two runs of the timed path (forward, CTC, backward, clip,
    Adam, many steps) dump bit-identical parameters, gradients and loss terms."""
    for r in ('a', 'b'):
        _line(['--steps', '30', '--warmup', '5', '--dump-outputs', str(tmp_path / r)])
    for name in ('loss', 'params', 'grads'):
        a, b = np.load(str(tmp_path / 'a' / (name + '.npy'))), np.load(str(tmp_path / 'b' / (name + '.npy')))
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b), '%s: %d elements differ, max %g' % (name, int((a != b).sum()), float(np.abs(a.astype(np.float64) - b).max()))
