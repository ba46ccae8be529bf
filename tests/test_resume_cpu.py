"""Host side of exact resuming (imagenet_models_amd.checkpoint, DESIGN.md "Resuming exactly"): the generator states as plain data,
the file under weights_only=True, CheckpointSaver's files / retention / atomic writes / write-behind errors, the loader's start
position, the per-rank packing, the schedule after a resume and train.py's refusal of a bad --resume path.  No device."""
import argparse
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from imagenet_models_amd import checkpoint as C
from imagenet_models_amd.dataset import FolderLoader
from imagenet_models_amd.optim import CosineLRScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _draws(n=100):
    out = []
    for _ in range(n):
        out.append((random.random(), random.gauss(0.0, 1.0), random.randint(0, 1 << 40),
                    float(np.random.beta(0.8, 1.3)), int(np.random.choice(15)), float(np.random.rand()), float(torch.rand(1))))
    return out


def test_host_generator_states_round_trip_through_plain_data(tmp_path):
    random.seed(11)
    np.random.seed(12)
    torch.manual_seed(13)
    random.gauss(0.0, 1.0)                   # leaves the cached second value in the state
    np.random.randn()                        # numpy's cached gaussian likewise
    torch.rand(3)
    packed = C.pack_host_generators()
    assert packed['python']['has_gauss'] == 1 and packed['numpy']['has_gauss'] == 1
    want = _draws()
    path = os.path.join(tmp_path, 'g.pt')
    torch.save(packed, path)
    random.seed(1)
    np.random.seed(2)
    torch.manual_seed(3)
    assert _draws() != want
    C.unpack_host_generators(torch.load(path, weights_only=True))
    assert _draws() == want


def test_own_generators_are_saved_instead_of_the_global_ones():
    class Piece:
        pass

    class Step:
        crop = auto_augment = collate_mixup = mixup_fn = None
    re, aa = Piece(), Piece()
    re.rng = random.Random(5)
    aa.rng, aa.np_rng = random, np.random.RandomState(6)
    step = Step()
    step.random_erasing, step.auto_augment = re, aa
    d = C.capture_rank_state(step)
    assert sorted(d['own']) == ['auto_augment.np_rng', 'random_erasing.rng']
    want = [re.rng.random() for _ in range(5)], aa.np_rng.rand(5).tolist()
    re.rng.seed(99)
    aa.np_rng.seed(99)
    assert C.restore_rank_state(d, step) == []
    assert ([re.rng.random() for _ in range(5)], aa.np_rng.rand(5).tolist()) == want
    del d['own']['random_erasing.rng']
    assert C.restore_rank_state(d, step) == ['generator of random_erasing.rng']


class _FakeSource:
    """what DeviceSnapshot is to the saver, from host tensors: snapshot() clones now, the returned function hands the clones over"""

    def __init__(self):
        self.w = torch.arange(6, dtype=torch.float32).view(2, 3)
        self.m = torch.zeros(6)
        self.steps = 0
        self.fail = None

    def advance(self):
        self.w += 1
        self.m += 0.5
        self.steps += 1

    def snapshot(self):
        w, m, steps = self.w.clone(), self.m.clone(), self.steps

        def materialise():
            if self.fail is not None:
                raise self.fail
            return {'state_dict': {'fc.weight': w, 'bn.num_batches_tracked': torch.tensor(steps)},
                    'optimizer': dict(kind='adamw', steps=steps, m=m, v=m * 2, param_groups=[dict(lr=0.1, weight_decay=0.0, initial_lr=0.1)]),
                    'state_dict_ema': {'fc.weight': w * 0.5}, 'counters': {'dp_counter': torch.tensor([steps])}}
        return materialise


def _train_state(epoch=0, batch=0):
    ts = {'opt_steps': 3, 'micro': 3, 're_offset': 3, 'loader': {'epoch': epoch, 'batch': batch}}
    ts.update(C.pack_ranks([C.capture_rank_state()], 1))
    return ts


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_checkpoint_is_plain_data_under_weights_only(tmp_path):
    src = _FakeSource()
    ts = _train_state(2, 5)
    saver = C.CheckpointSaver(str(tmp_path), src, arch='net')
    saver.take(2, metric=51.5, train_state=ts)
    saver.join()
    with torch.serialization.safe_globals([argparse.Namespace]):          # nothing else is allow-listed
        ck = torch.load(os.path.join(tmp_path, 'last.pth.tar'), weights_only=True)
    assert list(ck)[:6] == ['epoch', 'arch', 'state_dict', 'optimizer', 'version', 'metric']
    assert ck['epoch'] == 2 and ck['arch'] == 'net' and ck['version'] == 2 and ck['metric'] == 51.5
    assert torch.equal(ck['state_dict']['fc.weight'], src.w) and torch.equal(ck['state_dict_ema']['fc.weight'], src.w * 0.5)
    assert ck['optimizer']['steps'] == 0
    got = ck['train_state']
    assert _same({k: v for k, v in got.items() if k not in ('recovery', 'dp_counter')}, ts)
    assert got['recovery'] == 0 and torch.equal(got['dp_counter'], torch.tensor([0]))
    # the file the reader of this package opens is the same data
    assert _same(C.read_checkpoint(os.path.join(tmp_path, 'checkpoint-2.pth.tar'))['train_state'], got)


def _names(d):
    return sorted(os.listdir(d))


def test_retention_keeps_the_n_best_and_last_and_best_follows_the_metric(tmp_path):
    up, down = os.path.join(tmp_path, 'up'), os.path.join(tmp_path, 'down')
    src = _FakeSource()
    saver = C.CheckpointSaver(up, src, eval_metric='top1', checkpoint_hist=2)
    for epoch, metric in enumerate([10.0, 30.0, 20.0, 5.0, 25.0]):
        src.advance()
        best = saver.take(epoch, metric=metric, train_state=_train_state(epoch))
    saver.join()
    assert best == (30.0, 1)
    assert _names(up) == ['checkpoint-1.pth.tar', 'checkpoint-4.pth.tar', 'last.pth.tar', 'model_best.pth.tar']
    assert C.read_checkpoint(os.path.join(up, 'model_best.pth.tar'))['epoch'] == 1
    assert C.read_checkpoint(os.path.join(up, 'last.pth.tar'))['epoch'] == 4
    assert C.read_checkpoint(os.path.join(up, 'checkpoint-4.pth.tar'))['metric'] == 25.0
    src = _FakeSource()
    saver = C.CheckpointSaver(down, src, eval_metric='loss', checkpoint_hist=2)
    for epoch, metric in enumerate([3.0, 1.0, 2.0, 4.0]):
        src.advance()
        best = saver.take(epoch, metric=metric)
    saver.join()
    assert best == (1.0, 1)
    assert _names(down) == ['checkpoint-1.pth.tar', 'checkpoint-2.pth.tar', 'last.pth.tar', 'model_best.pth.tar']
    assert C.read_checkpoint(os.path.join(down, 'model_best.pth.tar'))['metric'] == 1.0
    # the default keeps every epoch file
    keep = os.path.join(tmp_path, 'all')
    saver = C.CheckpointSaver(keep, _FakeSource())
    for epoch in range(4):
        saver.take(epoch, metric=float(epoch))
    saver.join()
    assert _names(keep) == [f'checkpoint-{e}.pth.tar' for e in range(4)] + ['last.pth.tar', 'model_best.pth.tar']


def test_only_the_newest_recovery_file_remains(tmp_path):
    src = _FakeSource()
    saver = C.CheckpointSaver(str(tmp_path), src)
    for epoch, batch in ((0, 1), (0, 3), (1, 1)):
        src.advance()
        saver.take(epoch, train_state=_train_state(epoch, batch + 1), recovery_batch=batch)
    saver.join()
    assert _names(tmp_path) == ['recovery-1-1.pth.tar']
    ck = C.read_checkpoint(os.path.join(tmp_path, 'recovery-1-1.pth.tar'))
    assert ck['train_state']['recovery'] == 1 and ck['train_state']['loader'] == {'epoch': 1, 'batch': 2}
    assert torch.equal(ck['state_dict']['fc.weight'], src.w)


def test_interrupted_write_leaves_the_previous_last_loadable_and_no_temporary_file(tmp_path, monkeypatch):
    src = _FakeSource()
    saver = C.CheckpointSaver(str(tmp_path), src)
    saver.take(0, metric=1.0)
    saver.join()
    before = _names(tmp_path)
    real = C.CheckpointSaver._serialise

    def half_way(ck, path):
        real(ck, path)
        with open(path, 'r+b') as f:             # the file exists and is cut short when the write dies
            f.truncate(os.path.getsize(path) // 2)
        raise OSError('disk full')
    monkeypatch.setattr(C.CheckpointSaver, '_serialise', staticmethod(half_way))
    src.advance()
    saver.take(1, metric=2.0)
    with pytest.raises(OSError, match='disk full'):
        saver.join()
    assert _names(tmp_path) == before
    ck = C.read_checkpoint(os.path.join(tmp_path, 'last.pth.tar'))
    assert ck['epoch'] == 0 and torch.equal(ck['state_dict']['fc.weight'], torch.arange(6, dtype=torch.float32).view(2, 3))
    saver.join()                                 # raised once, then clear


def test_writer_exception_surfaces_at_the_next_take_and_at_join(tmp_path):
    src = _FakeSource()
    saver = C.CheckpointSaver(str(tmp_path), src)
    src.fail = RuntimeError('copy to host failed')
    saver.take(0, metric=1.0)
    with pytest.raises(RuntimeError, match='copy to host failed'):
        saver.take(1, metric=2.0)
    src.fail = None
    saver.take(1, metric=2.0)
    saver.join()
    src.fail = RuntimeError('again')
    saver.take(2, metric=3.0)
    with pytest.raises(RuntimeError, match='again'):
        saver.join()
    src.fail = ValueError('inside with')
    with pytest.raises(ValueError, match='inside with'):
        with saver:
            saver.take(3, metric=4.0)
    assert C.read_checkpoint(os.path.join(tmp_path, 'last.pth.tar'))['epoch'] == 1


class _Set:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize('rank,world', [(0, 1), (1, 2)])
def test_loader_start_position_lists_the_rest_of_the_epoch(rank, world):
    ld = FolderLoader(_Set(103), 8, None, train=True, seed=5, rank=rank, world=world)
    for epoch in (0, 3):
        full = ld.batches(epoch)
        assert len(full) == len(ld) > 2
        for k in (0, len(full) // 2, len(full)):
            ld.set_epoch(epoch, start_batch=k)
            plan = ld.plan()
            assert len(plan) == len(full) - k
            assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(plan, full[k:]))
        ld.set_epoch(epoch)                      # the position belongs to one epoch
        assert len(ld.plan()) == len(full)
    with pytest.raises(ValueError):
        ld.set_epoch(0, start_batch=len(ld) + 1)


def test_per_rank_packing_hands_each_rank_its_own_state_and_refuses_another_world_size():
    states = []
    for r in range(2):
        random.seed(100 + r)
        np.random.seed(200 + r)
        torch.manual_seed(300 + r)
        states.append(C.capture_rank_state())
    want = []
    for r in range(2):
        C.restore_rank_state(states[r])
        want.append(_draws(10))
    assert want[0] != want[1]
    ts = C.pack_ranks(states, 2)
    assert ts['world_size'] == 2 and C.saved_initial_seed(ts, 1) == 301
    for r in (1, 0):
        random.seed(0)
        C.restore_rank_state(C.select_rank(ts, r, 2))
        assert _draws(10) == want[r]
    with pytest.raises(ValueError, match='2 rank'):
        C.select_rank(ts, 0, 1)
    with pytest.raises(ValueError):
        C.pack_ranks(states, 3)


class _Opt:
    def __init__(self, lr):
        self.param_groups = [dict(lr=lr, weight_decay=0.0, initial_lr=lr)]


@pytest.mark.parametrize('e', [0, 1, 2, 3, 7, 19])
def test_schedule_after_a_resume_is_the_uninterrupted_one(e):
    kw = dict(t_initial=20, lr_min=1e-6, warmup_t=3, warmup_lr_init=1e-4)
    a = _Opt(0.05)
    sa = CosineLRScheduler(a, **kw)
    for epoch in range(e + 1):
        sa.step(epoch)
    b = _Opt(0.05)
    sb = CosineLRScheduler(b, **kw)
    b.param_groups[0].update(dict(lr=123.0, weight_decay=0.0, initial_lr=0.05))     # what load_state_dict brings back
    sb.step(e)
    assert b.param_groups[0]['lr'] == a.param_groups[0]['lr']
    want = 1e-4 + e * (0.05 - 1e-4) / 3 if e < 3 else 1e-6 + 0.5 * (0.05 - 1e-6) * (1 + math.cos(math.pi * e / 20))
    assert b.param_groups[0]['lr'] == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize('flag', ['--resume', '--initial-checkpoint'])
def test_train_cli_refuses_a_missing_checkpoint_before_the_device(flag, tmp_path):
    r = subprocess.run([sys.executable, 'train.py', '--synthetic', flag, '/nonexistent/last.pth.tar'], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert f"{flag} '/nonexistent/last.pth.tar': no such file" in r.stderr
    bad = os.path.join(tmp_path, 'bad.pth.tar')
    with open(bad, 'wb') as f:
        f.write(b'not a checkpoint')
    r = subprocess.run([sys.executable, 'train.py', '--synthetic', flag, bad], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'does not load' in r.stderr
