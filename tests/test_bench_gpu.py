"""GPU: bench.py end to end at a small batch, as a fresh process: the result line and the --dump-outputs files of the real
call site (the engine's logits, the model's flat state, the optimizer's first moment)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs(tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '8',
                        '--dump-outputs', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 2 and line['ms_per_step'] > 0 and 'roofline' not in line and 'cpu_baseline' not in line
    z = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert sorted(z) == ['buffers', 'logits', 'loss', 'moment', 'params']
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in z.values())
    assert abs(float(z['loss'][0]) - line['loss']) <= 1e-4 * max(1.0, abs(line['loss']))
    assert z['logits'].shape[1:] == (8, 1000) and np.abs(z['logits']).max() > 0
    # the backward's result: every step's gradients averaged into the first moment, nonzero after three steps
    assert (z['moment'] != 0).mean() > 0.5
