"""GPU: resuming exactly (imagenet_models_amd.checkpoint, train.py --resume; DESIGN.md "Resuming exactly").

A run that is stopped after step k, torn down and rebuilt from its checkpoint is fed byte for byte what the uninterrupted run is fed
(the input stage's output, the dense target, the DropPath table, the head-dropout masks: none depends on the trunk's arithmetic, so
the comparison is exact), holds bit for bit the state it saved, and lands where uninterrupted runs land, within their own run-to-run
spread.  The write-behind snapshot is of the moment take() was called, and ModelEma.swapped() evaluates the EMA in the model's place.

Small models built directly: a narrow GA-ConvNeXt (dims 16..128, depths (1, 1, 6, 1, 1), 40 classes, B = 4, fp32 mode, DropPath 0.2)
and a narrow MAP-ConvNeXt with head dropout, so that both device samplers exist."""
import gc
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _spread

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GA = dict(dims=(16, 32, 64, 128, 128), depths=(1, 1, 6, 1, 1), gram_dim=32, dim_embed=64, num_classes=40, naggre=2)
MAP = dict(dims=(16, 32, 64, 128), depths=(1, 1, 2, 1), last_dim=64, n_groups=2, n_tokens=2, gram_group=8, bp_dim=64, ca_dim=64,
           num_heads=8, num_classes=40)
B, NC = 4, 40


def _model(kind):
    """weights by the oracles' name-hashed fill: the same in every build, whatever the generators hold"""
    import imagenet_models_amd as A
    if kind == 'ga':
        from oracle import ga_convnext_oracle as O
        cfg = O.make_cfg(**GA)
        m = A.GA_ConvNeXt(num_classes=NC, depths=cfg['depths'], dims=cfg['dims'], gram_embedding_gropus=cfg['gram_groups'],
                          dim_embed=cfg['dim_embed'], stage3_naggre=cfg['naggre'], gram_dim=cfg['gram_dim'], drop_path_rate=0.2,
                          math_mode='fp32')
    else:
        from oracle import map_oracle as O
        cfg = O.make_cfg(**MAP)
        m = A.MAP_ConvNeXt(num_classes=NC, depths=cfg['depths'], dims=cfg['dims'], drop_path_rate=0.2, last_dim=cfg['last_dim'],
                           n_groups=cfg['n_groups'], n_tokens=cfg['n_tokens'], gram_group=cfg['gram_group'], bp_dim=cfg['bp_dim'],
                           ca_dim=cfg['ca_dim'], num_heads=cfg['num_heads'], head_drop=0.05, head_attn_drop=0.05, math_mode='fp32')
    m.load_state_dict(O.fill_state(cfg))
    return m.cuda().train()


def _seed(s):
    torch.manual_seed(s)
    random.seed(s + 1)
    np.random.seed(s + 2)


def _build(kind='ga', opt='adamw', ema=False, stage=False, lr=1e-3):
    """(model, optimizer, TrainStep, ModelEma | None); stage: everything random the input stage has, on the global generators as
    train.py builds it"""
    import imagenet_models_amd as A
    m = _model(kind)
    o = A.create_optimizer_v2(m, opt=opt, lr=lr, weight_decay=0.05, momentum=0.9)
    kw = {}
    if stage:
        kw = dict(auto_augment=A.RandAugment('rand-m9-mstd0.5-inc1'),
                  collate_mixup=A.FastCollateMixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode='elem', label_smoothing=0.1, num_classes=NC),
                  random_erasing=A.RandomErasing(probability=0.75, mode='pixel', max_count=2, seed=42))
    step = A.TrainStep(m, o, B, lam=-0.8, **kw)
    return m, o, step, (A.ModelEma(m, 0.5) if ema else None)


def _batch(i, uint8=False):
    """the batch of step i: a pure function of i"""
    g = torch.Generator().manual_seed(1000 + i)
    if uint8:
        x = torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8)
    else:
        x = torch.randn(B, 3, 224, 224, generator=g)
    return x.cuda(), torch.randint(0, NC, (B,), generator=g).cuda()


def _fed(step):
    """what the engine was fed in the step just run"""
    eng = step.eng
    out = {'x': eng.x_ref.clone(), 'target': eng.target_buf.clone(), 'drop_path': eng.dp_all.clone()}
    if getattr(eng, 'drop', None):
        out['dropout'] = eng.drop['buf'].clone()
    return out


def _teardown():
    gc.collect()
    torch.cuda.empty_cache()


def _save_sync(path, m, o, step, ema=None, epoch=0):
    import imagenet_models_amd as A
    A.save_checkpoint(m, o, epoch, path, arch='narrow', model_ema=ema, train_state=A.capture_train_state(step))


def _rebuild(path, wrong_seed, **kw):
    """the resume order: read the file, seed torch with the saved initial seed, build, restore.  Every host generator is reseeded
    with other values first, so only the file can bring the streams back"""
    import imagenet_models_amd as A
    _seed(wrong_seed)
    ck = A.read_checkpoint(path)
    torch.manual_seed(A.saved_initial_seed(ck['train_state']))
    m, o, step, ema = _build(**kw)
    A.resume_checkpoint(ck, m, o, ema, step)
    return m, o, step, ema


@pytest.mark.parametrize('kind', ['ga', 'map'])
def test_fed_data_continues_byte_for_byte(kind, tmp_path):
    _seed(7)
    m, o, step, _ = _build(kind, stage=True)
    assert (kind == 'map') == bool(getattr(step.eng, 'drop', None)) and step.eng.dp_scale
    want = []
    for i in range(6):
        step(*_batch(i, uint8=True))
        if i >= 3:
            want.append(_fed(step))
    assert not torch.equal(want[0]['x'], want[1]['x']) and not torch.equal(want[0]['target'], want[1]['target'])
    del m, o, step
    _teardown()
    _seed(7)
    m, o, step, _ = _build(kind, stage=True)
    for i in range(3):
        step(*_batch(i, uint8=True))
    path = os.path.join(tmp_path, 'k3.pth.tar')
    _save_sync(path, m, o, step)
    del m, o, step
    _teardown()
    m, o, step, _ = _rebuild(path, 12345, kind=kind, stage=True)
    assert o.steps == 3 and step.micro == 3 and step.random_erasing.offset == 3
    for i in range(3, 6):
        step(*_batch(i, uint8=True))
        got = _fed(step)
        for k, v in want[i - 3].items():
            assert torch.equal(got[k], v), (kind, i, k, int((got[k] != v).sum()))
    # and without the state the same build is fed something else: the comparison above is not vacuous
    del m, o, step
    _teardown()
    _seed(12345)
    m, o, step, _ = _build(kind, stage=True)
    step(*_batch(3, uint8=True))
    other = _fed(step)
    assert not torch.equal(other['x'], want[0]['x']) and not torch.equal(other['target'], want[0]['target'])


def _clone_sd(sd):
    return {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in sd.items()}


def _assert_same(got, want, what):
    assert list(got) == list(want), what
    for k, v in want.items():
        g = got[k]
        if torch.is_tensor(v):
            assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g.cpu(), v.cpu()), (what, k)
        else:
            assert g == v, (what, k, g, v)


@pytest.mark.parametrize('opt', ['nesterov', 'adamw', 'lamb'])
def test_state_round_trip_is_bitwise(opt, tmp_path):
    import imagenet_models_amd as A
    _seed(3)
    m, o, step, ema = _build('ga', opt=opt, ema=True)
    for i in range(2):
        step(*_batch(i))
        ema.update()
    o.param_groups[0]['lr'] = 3.3e-4                     # what a schedule left there
    saver = A.CheckpointSaver(str(tmp_path), A.DeviceSnapshot(m, o, ema, step), arch='narrow')
    saver.take(0, metric=1.0, train_state=A.capture_train_state(step, device_counters=False))
    saver.join()
    want = dict(model=_clone_sd(m.state_dict()), opt=_clone_sd(o.state_dict()), ema=_clone_sd(ema.state_dict()))
    nbt = [k for k in want['model'] if k.endswith('num_batches_tracked')]
    assert nbt and all(int(want['model'][k]) == 2 for k in nbt)
    assert want['opt']['steps'] == 2 and not torch.equal(want['ema'][next(iter(want['ema']))], want['model'][next(iter(want['model']))])
    del m, o, step, ema, saver
    _teardown()
    path = os.path.join(tmp_path, 'last.pth.tar')
    ck = A.read_checkpoint(path)
    assert list(ck)[:6] == ['epoch', 'arch', 'state_dict', 'optimizer', 'version', 'metric'] and 'state_dict_ema' in ck
    _assert_same(ck['optimizer'], want['opt'], 'optimizer dict of the file')
    m, o, step, ema = _rebuild(path, 999, kind='ga', opt=opt, ema=True)
    _assert_same(_clone_sd(m.state_dict()), want['model'], 'model')
    _assert_same(_clone_sd(o.state_dict()), want['opt'], 'optimizer')
    _assert_same(_clone_sd(ema.state_dict()), want['ema'], 'ema')
    assert o.param_groups[0]['lr'] == 3.3e-4 and o.steps == 2
    # the first resumed step pushes the hyper-parameter row of step steps + 1
    step(*_batch(2))
    g = o.param_groups[0]
    t = 3
    if opt == 'nesterov':
        row = [g['lr'], g['weight_decay'], 0.9, 0.0, 0.0, 0.0, 0.0, 0.0]             # not the first step: the flag is down
    else:
        b1, b2 = o.betas
        row = [g['lr'], g['weight_decay'], b1, b2, o.eps, 1 - b1 ** t, 1 - b2 ** t] + ([0.0] if opt == 'adamw' else [1 - b1, 1.0])
    assert torch.equal(o.hp.cpu(), torch.tensor(row, dtype=torch.float32)), (o.hp.cpu().tolist(), row)
    assert o.steps == 3


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_resumed_trajectory_lies_within_the_run_to_run_spread(monkeypatch, tmp_path):
    """Baseline: three uninterrupted 6-step runs from one seed (AdamW, lr 1e-3, fp32 mode, the serial launch schedule); d_cc is the
    largest pairwise relative L2 distance of their final flat parameters -- the spread the existing code has.  The interrupted run
    (3 steps, save, rebuild, restore, 3 steps) must lie within max(10 d_cc, 2^-23) of every baseline run: it is one more sample of the
    same order-dependent arithmetic, whereas an error in the state moves the parameters by about lr per step, orders of magnitude
    more; 2^-23 is one fp32 rounding, for baselines that agree bit for bit.  Negative control: the same resume with the moments
    zeroed and steps = 0 (what --no-resume-opt leaves) must fail that gate, or the gate measures nothing.
    Measured on one MI355X, six repeats: d_cc 9.4e-4 .. 1.04e-3, resumed 9.7e-4 .. 1.03e-3, control 1.27e-2 every time."""
    _spread.set_schedule(monkeypatch, True)

    def run(first, last, built=None):
        m, o, step, _ = built or _build('ga')
        for i in range(first, last):
            step(*_batch(i))
        return m, o, step

    base = []
    for _ in range(3):
        _seed(5)
        m, o, step = run(0, 6)
        base.append(m.flat_state()['params'].clone())
        del m, o, step
        _teardown()
    d_cc = max(_rel(base[i], base[j]) for i in range(3) for j in range(3) if i != j)
    gate = max(10 * d_cc, 2.0 ** -23)
    _seed(5)
    m, o, step = run(0, 3)
    path = os.path.join(tmp_path, 'k3.pth.tar')
    _save_sync(path, m, o, step)
    del m, o, step
    _teardown()
    m, o, step = run(3, 6, _rebuild(path, 777, kind='ga'))
    resumed = max(_rel(m.flat_state()['params'], b) for b in base)
    del m, o, step
    _teardown()
    built = _rebuild(path, 777, kind='ga')
    built[1].m.zero_()
    built[1].v.zero_()
    built[1].steps = 0
    m, o, step = run(3, 6, built)
    control = min(_rel(m.flat_state()['params'], b) for b in base)
    print(f'[resume trajectory] d_cc {d_cc:.3e}  gate {gate:.3e}  resumed {resumed:.3e}  control (moments zeroed, steps 0) {control:.3e}')
    assert control > gate, 'the negative control passes the gate: the test measures nothing'
    assert resumed <= gate


def test_snapshot_is_of_its_moment(tmp_path):
    import imagenet_models_amd as A
    _seed(9)
    m, o, step, ema = _build('ga', ema=True)
    saver = A.CheckpointSaver(str(tmp_path), A.DeviceSnapshot(m, o, ema, step), arch='narrow')
    for i in range(2):
        step(*_batch(i))
        ema.update()
    saver.take(0, train_state=A.capture_train_state(step, None, 0, 2, device_counters=False), recovery_batch=1)
    at_k = dict(model=_clone_sd(m.state_dict()), opt=_clone_sd(o.state_dict()), ema=_clone_sd(ema.state_dict()),
                dp=step.eng.dp_counter.clone())
    for i in range(2, 4):                                # two more steps at once, the write still in flight or not: no join
        step(*_batch(i))
        ema.update()
    saver.join()
    ck = A.read_checkpoint(os.path.join(tmp_path, 'recovery-0-1.pth.tar'))
    _assert_same(ck['state_dict'], at_k['model'], 'model at k')
    _assert_same(ck['optimizer'], at_k['opt'], 'optimizer at k')
    _assert_same(ck['state_dict_ema'], at_k['ema'], 'ema at k')
    ts = ck['train_state']
    assert torch.equal(ts['dp_counter'], at_k['dp'].cpu()) and int(ts['dp_counter']) == 2
    assert ts['opt_steps'] == 2 and ts['micro'] == 2 and ts['recovery'] == 1 and ts['loader'] == {'epoch': 0, 'batch': 2}
    flat_k = torch.cat([at_k['model'][n].reshape(-1) for n, _ in m.named_parameters()])
    flat_later = torch.cat([p.detach().reshape(-1) for _, p in m.named_parameters()])
    assert not torch.equal(flat_k, flat_later) and o.steps == 4


def test_ema_swap_evaluates_the_ema_and_restores_bitwise():
    import imagenet_models_amd as A
    _seed(4)
    m, o, step, ema = _build('ga', ema=True)
    for i in range(2):
        step(*_batch(i))
        ema.update()
    before = _clone_sd(m.state_dict()), _clone_sd(ema.state_dict())
    assert not torch.equal(m.flat_state()['params'], ema.flat)
    x, _ = _batch(50)
    m.eval()
    with torch.no_grad():
        own = torch.stack(m(x)).clone()
        with ema.swapped():
            got = torch.stack(m(x)).clone()
        again = torch.stack(m(x)).clone()
    m.train()
    _assert_same(_clone_sd(m.state_dict()), before[0], 'model after the swap')
    _assert_same(_clone_sd(ema.state_dict()), before[1], 'ema after the swap')
    assert torch.equal(own, again) and not torch.equal(own, got)
    ref = _model('ga')
    ref.load_state_dict({k: v.cpu() for k, v in before[1].items()})
    ref.eval()
    with torch.no_grad():
        want = torch.stack(ref(x)).clone()
    assert torch.equal(got, want), float((got - want).abs().max())


def test_file_without_train_state_resumes_weights_optimizer_and_epoch(tmp_path, caplog):
    """the layout before train_state existed (and a reference checkpoint's): its keys only"""
    import imagenet_models_amd as A
    _seed(6)
    m, o, step, _ = _build('ga')
    for i in range(2):
        step(*_batch(i))
    path = os.path.join(tmp_path, 'checkpoint-4.pth.tar')
    A.save_checkpoint(m, o, 4, path, metric=12.5, arch='narrow')
    want = _clone_sd(m.state_dict()), _clone_sd(o.state_dict())
    del m, o, step
    _teardown()
    ck = A.read_checkpoint(path)
    assert list(ck) == ['epoch', 'arch', 'state_dict', 'optimizer', 'version', 'metric']
    _seed(60)
    m, o, step, _ = _build('ga')
    with caplog.at_level('INFO', logger='train'):
        assert A.resume_checkpoint(ck, m, o, None, step) == (5, 0)
    assert 'no train_state' in caplog.text
    _assert_same(_clone_sd(m.state_dict()), want[0], 'model')
    _assert_same(_clone_sd(o.state_dict()), want[1], 'optimizer')
    # --no-resume-opt: the weights and the epoch only
    m2, o2, step2, _ = _build('ga')
    assert A.resume_checkpoint(ck, m2, o2, None, step2, resume_opt=False) == (5, 0)
    _assert_same(_clone_sd(m2.state_dict()), want[0], 'model')
    assert o2.steps == 0 and not o2.m.any()


def _cli(args, timeout=600):
    r = subprocess.run([sys.executable, 'train.py', '--synthetic', '--model', 'convnext_tiny', '-b', '8', '--steps-per-epoch', '3',
                        '--opt', 'adamw', '--lr', '1e-3', '--warmup-epochs', '1', '--log-interval', '1', '--model-ema'] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout + r.stderr


def test_command_line_resumes_from_last_and_from_a_recovery_file(tmp_path):
    import imagenet_models_amd as A
    D = os.path.join(tmp_path, 'out')
    out = _cli(['--epochs', '2', '--output', D, '--recovery-interval', '2', '--checkpoint-hist', '1'])
    assert '*** epoch 1: train loss' in out
    names = sorted(os.listdir(D))
    assert [n for n in names if n.startswith('checkpoint-')] in (['checkpoint-0.pth.tar'], ['checkpoint-1.pth.tar'])
    assert [n for n in names if n.startswith('recovery-')] == ['recovery-1-2.pth.tar']
    assert len(names) == 4 and 'last.pth.tar' in names and 'model_best.pth.tar' in names
    ck = A.read_checkpoint(os.path.join(D, 'last.pth.tar'))
    assert ck['epoch'] == 1 and ck['train_state']['opt_steps'] == 6 and ck['train_state']['loader'] == {'epoch': 1, 'batch': 3}
    out = _cli(['--epochs', '3', '--resume', os.path.join(D, 'last.pth.tar')])
    mt = re.search(r'Resumed \S+: starting at epoch (\d+), batch (\d+) of 3, lr (\S+)', out)
    assert mt and (int(mt.group(1)), int(mt.group(2))) == (2, 0), out[-1500:]
    lr2 = 1e-6 + 0.5 * (1e-3 - 1e-6) * (1 + math.cos(math.pi * 2 / 3))              # the 3-epoch cosine at epoch 2
    assert float(mt.group(3)) == pytest.approx(lr2, rel=1e-6)
    assert 'Train: 2 [   0/3' in out and 'Train: 1 [' not in out and '*** epoch 2: train loss' in out
    out = _cli(['--epochs', '2', '--resume', os.path.join(D, 'recovery-1-2.pth.tar')])
    mt = re.search(r'Resumed \S+: starting at epoch (\d+), batch (\d+) of 3', out)
    assert mt and (int(mt.group(1)), int(mt.group(2))) == (1, 3), out[-1500:]           # inside epoch 1, at the recorded batch + 1
    assert 'Train: 1 [' not in out and '*** epoch 1: train loss' in out
