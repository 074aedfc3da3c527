"""`python bench.py --gpus 1 --steps K --warmup W` (no --full): sets up, warms up, times the K steps, writes
--dump-outputs and prints the contract's line, and nothing that only `--full` measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ('hip_event_ms_per_step', 'steady_state', 'roofline', 'raster_roofline', 'kernel_us', 'entry_us', 'dist',
             'step_hbm', 'cpu_baseline', 'c2', 'kinds_variants', 'emd', 'c5')


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5', '--warmup', '2',
           '--dump-outputs', str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d['metric'] == 'render+Chamfer fwd+bwd images/sec' and d['unit'] == 'images/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert (d['n_gpus'], d['steps'], d['warmup']) == (1, 5, 2)
    assert d['value'] > 0 and d['ms_per_step'] > 0
    # value = images over the timed region / its time; ms_per_step = that time / steps (B = 64 images per step)
    assert abs(d['value'] - 64 / d['ms_per_step'] * 1e3) <= 1e-3 * d['value']
    assert d['config']['workload'].startswith('C3: B=64/GPU')
    # the device step counter: 3 eager steps before the graph capture, then the W + K replays, and no step after them
    assert '10 steps drawn' in d['config']['sampling']
    assert not [k for k in FULL_ONLY if k in d]
    for name, shape in (('grad_params', (64, 32, 10)), ('loss_total', ()), ('loss_silhouette', ()), ('loss_depth', ())):
        a = np.load(os.path.join(tmp_path, name + '.npy'))
        assert a.shape == shape and np.isfinite(a).all(), name
