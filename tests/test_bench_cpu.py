"""bench.py's command line and its --dump-outputs writer, on the host (the timed path itself needs the GPU)."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *args):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *args])
    return bench.parse()


def test_plain_run_has_no_extras_and_kernel_table_implies_full(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs, a.lr) == (1, 7, 2, False, '', 0.0)
    assert _parse(monkeypatch, '--full').full
    assert _parse(monkeypatch, '--kernel-table', 'kt.json').full


def test_dump_outputs_are_float32_bounded_and_repeatable(tmp_path):
    flat = dict(params=torch.arange(10_000_000, dtype=torch.float32), buffers=torch.ones(5))
    logits = torch.randn(2, 8, 10)
    moment = torch.arange(10_000_000, dtype=torch.float32) * -1e-7           # the optimizer's first moment (backward)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), torch.tensor([0.5]), logits, flat, moment)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['buffers.npy', 'logits.npy', 'loss.npy', 'moment.npy', 'params.npy']
    total = 0
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / 'a' / 'logits.npy'), logits.numpy())
    p = np.load(tmp_path / 'a' / 'params.npy')
    assert p.size == 1 << 22 and np.all(np.diff(p) >= 0) and p[-1] - p[0] > 9e6     # a sample of all 10 M, in order
    m = np.load(tmp_path / 'a' / 'moment.npy')
    assert m.size == 1 << 22 and np.all(np.diff(m) <= 0) and m.min() < -0.9
