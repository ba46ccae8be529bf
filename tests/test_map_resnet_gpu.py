"""GPU: MAP-ResNet50 (imagenet_models_amd.map_resnet, engine_resnet) against tests/golden/map_rn50_*.npz, written by
tools/gen_golden_map_resnet.py from the REAL reference classes with the repaired head composition (head([stem, layer1..4])):

  * fp32: eval logits at B = 2 (running statistics from the fixture) and top-5; one train step at B = 4: loss, logits, every parameter
    gradient (norm and first elements per tensor), the BatchNorm running statistics after the step;
  * the run-to-run spread of two identical fp32 steps (BatchNorm-sum atomics over 80 BatchNorms) is measured and printed, and the
    gradient gate is set above it; bf16 against fp32: errors printed, the loss gated;
  * the bucketed world-1 TrainStep equals the plain step (every gradient group final at its mark: tests/test_grad_marks_gpu.py);
  * two steps at drop_path_rate 0.2 and an eval through create_model; train.py / validate.py on synthetic data."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _gradcheck import norm_errors
from _mnv1_state import fill_state
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
NAME = 'map_resnet50'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen_input(batch, seed):
    from oracle.ga_convnext_oracle import gen_input
    return gen_input(batch, seed=seed)


def _build(mode, running=None):
    import imagenet_models_amd as A
    m = A.create_model(NAME, math_mode=mode, head_drop=0.0, head_attn_drop=0.0)
    sd = fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()})
    if running is not None:
        names, vals = running
        off = 0
        for n in names:
            k = sd[n].numel()
            sd[n] = torch.from_numpy(vals[off:off + k].astype(np.float32)).view_as(sd[n])
            off += k
        assert off == vals.size
    m.load_state_dict(sd)
    return m.cuda()


def _logits(out):
    if isinstance(out[0], (list, tuple)):
        return torch.stack([o[0] for o in out] + [o[1] for o in out])
    return torch.stack(out)


def rel(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _train_step(mode):
    import imagenet_models_amd as A
    z = np.load(os.path.join(GOLDEN, 'map_rn50_train_b4.npz'))
    B = int(z['batch'])
    m = _build(mode).train()
    target = torch.from_numpy(z['target']).cuda()
    m.zero_grad()
    out = m(_gen_input(B, seed=1).cuda())
    loss = A.map_loss(out, target, float(z['dec_lam']))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    return z, m, out, loss, grads


def _grad_errors(z, grads):
    gnames = z['grad_names'].tolist()
    assert sorted(gnames) == sorted(grads)
    gmax = float(z['grad_norm'].max())
    e_n, e_h = {}, {}
    for n, w, h in zip(gnames, z['grad_norm'].tolist(), z['grad_head']):
        g = grads[n]
        den = max(w, 1e-3 * gmax)
        e_n[n] = abs(float(g.double().norm()) - w) / den
        k = min(16, g.numel())
        e_h[n] = float((g.reshape(-1)[:k] - torch.from_numpy(h[:k])).abs().max()) / den
    return max(e_n.items(), key=lambda kv: kv[1]), max(e_h.items(), key=lambda kv: kv[1])


def test_eval_fp32_vs_reference_fixture():
    import imagenet_models_amd as A
    z = np.load(os.path.join(GOLDEN, 'map_rn50_eval.npz'))
    m = _build('fp32', (z['running_names'].tolist(), z['running'])).eval()
    with torch.no_grad():
        out = m(_gen_input(int(z['batch']), seed=0).cuda())
    lg = _logits(out)
    e = rel(lg[:, :, :z['logits'].shape[2]], z['logits'])
    print(f'[{NAME} fp32] eval logits vs reference fixture {e:.2e}')
    assert e <= 1e-3
    _, idx = A.heads_mean_topk(list(lg), 5)
    assert np.array_equal(idx.cpu().numpy(), z['top5'])


# gradient gate: two identical fp32 steps on MI355X differ per tensor by the spread test_fp32_run_to_run_spread prints (the
# BatchNorm-sum atomics, amplified by 80 train-mode BatchNorms at B = 4): measured ||g1 - g2|| / ||g2|| up to 2.0e-2 (median 5.5e-3),
# and against the fixture norm errors up to 5.6e-3, first-element errors up to 8.1e-3; the gates sit above both
GRAD_GATE_NORM, GRAD_GATE_HEAD = 3e-2, 5e-2


def test_train_step_fp32_vs_reference_fixture():
    z, m, out, loss, grads = _train_step('fp32')
    e_out = rel(_logits(out)[:, :, :z['logits'].shape[2]], z['logits'])
    e_loss = abs(float(loss.detach()) - float(z['loss'])) / abs(float(z['loss']))
    worst_n, worst_h = _grad_errors(z, grads)
    sd = m.state_dict()
    e_r = {}
    for n, w, h in zip(z['running_names'].tolist(), z['running_norm'], z['running_head']):
        v = sd[n].detach().cpu().double().reshape(-1)
        k = min(16, v.numel())
        e_r[n] = max(abs(float(v.norm()) - w) / w, float((v[:k] - torch.from_numpy(h[:k]).double()).abs().max()) / (w / np.sqrt(v.numel())))
    worst_r = max(e_r.items(), key=lambda kv: kv[1])
    print(f'[{NAME} fp32] train: logits {e_out:.2e} loss {e_loss:.2e} grad norm {worst_n} grad head {worst_h} running {worst_r}')
    assert e_out <= 1e-3 and e_loss <= 1e-3
    assert worst_n[1] <= GRAD_GATE_NORM and worst_h[1] <= GRAD_GATE_HEAD
    assert worst_r[1] <= 1e-3
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith('num_batches_tracked'))


def test_fp32_run_to_run_spread():
    """the measurement the gradient gate is set from: two identical fp32 steps, per-tensor norm-relative difference"""
    _, _, _, l1, g1 = _train_step('fp32')
    _, _, _, l2, g2 = _train_step('fp32')
    # measured like the fixture gate: relative to max(tensor norm, 1e-3 x the largest norm) -- analytically zero gradients (the
    # biases before a softmax or a train-mode BatchNorm) hold round-off noise only
    gmax = max(float(g.double().norm()) for g in g2.values())
    errs = {n: float((g1[n] - g2[n]).double().norm()) / max(float(g2[n].double().norm()), 1e-3 * gmax) for n in g1}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f'[{NAME} fp32] run-to-run: loss {abs(float(l1.detach()) - float(l2.detach())):.2e}, worst gradient tensor {worst}, '
          f'median {float(np.median(list(errs.values()))):.2e}')
    assert worst[1] <= GRAD_GATE_HEAD


def test_bf16_vs_fp32():
    _, _, out32, loss32, g32 = _train_step('fp32')
    _, _, out16, loss16, g16 = _train_step('bf16')
    e_out = rel(_logits(out16), _logits(out32).detach().cpu())
    e_loss = abs(float(loss16.detach()) - float(loss32.detach())) / abs(float(loss32.detach()))
    errs = norm_errors(g16, g32)
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    print(f'[{NAME} bf16] vs fp32: train step B=4: logits {e_out:.2e} loss {e_loss:.2e} worst gradient (rel, cos) {worst}')
    assert e_loss <= 0.15
    assert all(torch.isfinite(g).all() for g in g16.values())


def test_bucketed_trainstep_equals_plain_step():
    import imagenet_models_amd as A
    B = 4
    x = _gen_input(B, seed=3).cuda()
    y = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(3)).cuda()
    res = {}
    for tag in ('plain', 'buckets'):
        m = _build('fp32').train()
        opt = A.create_optimizer_v2(m, opt='sgd', lr=1e-2, momentum=0.9, weight_decay=0.05)
        comm = None
        if tag == 'buckets':
            comm = A.NativeComm(wire='fp32')
            step = A.TrainStep(m, opt, B, lam=-0.8, comm=comm, force_buckets=True, bucket_elems=2_000_000)
            assert {b[0] for b in step.buckets} >= {'heads', 'layer4', 'layer3', 'layer2', 'layer1', 'end'}
        else:
            step = A.TrainStep(m, opt, B, lam=-0.8, overlap_optimizer=False)
        p0 = m.flat_state()['params'].clone()
        loss = step(x, y)
        torch.cuda.synchronize()
        res[tag] = (float(loss), m.flat_state()['params'].clone() - p0, m.flat_state()['slices'])
        if comm is not None:
            comm.close()
    assert abs(res['plain'][0] - res['buckets'][0]) <= 1e-5 * abs(res['plain'][0])
    ua, ub, slices = res['plain'][1], res['buckets'][1], res['plain'][2]
    umax = float(ua.abs().max())
    for n, (off, k) in slices.items():
        a, b = ua[off:off + k], ub[off:off + k]
        if float(a.abs().max()) < 1e-4 * umax:
            continue
        e = float((a - b).norm() / a.norm())
        assert e <= 0.3, f'{n}: updates differ by {e:.3e} of their norm'


def test_two_steps_with_drop_path_and_eval_through_create_model():
    import imagenet_models_amd as A
    B = 4
    torch.manual_seed(0)
    m = A.create_model(NAME, drop_path_rate=0.2).cuda().train()
    opt = A.create_optimizer_v2(m, opt='adamw', lr=1e-3, weight_decay=0.05)
    step = A.TrainStep(m, opt, B, lam=-0.8)
    g = torch.Generator().manual_seed(5)
    losses = []
    for _ in range(2):
        x = torch.randn(B, 3, 224, 224, generator=g).cuda()
        y = torch.randint(0, 1000, (B,), generator=g).cuda()
        losses.append(float(step(x, y)))
    assert all(np.isfinite(losses)), losses
    assert torch.isfinite(m.flat_state()['params']).all()
    m.eval()
    with torch.no_grad():
        out = m(torch.randn(B, 3, 224, 224, generator=g).cuda())
    lg = _logits(out)
    assert lg.shape == (4, B, 1000) and torch.isfinite(lg).all()


def _run(cmd):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout + r.stderr


def test_train_and_validate_cli(tmp_path):
    out = _run([sys.executable, 'train.py', '--synthetic', '--model', NAME, '-b', '8', '--epochs', '1', '--steps-per-epoch', '3',
                '--drop-path', '0.1', '--log-interval', '1', '--dec-lam', '-0.8', '--opt', 'adamw', '--lr', '1e-3'])
    assert '*** epoch 0: train loss' in out and 'nan' not in out.lower()
    res = os.path.join(tmp_path, 'r.json')
    out = _run([sys.executable, 'validate.py', '--synthetic', '--model', NAME, '-b', '8', '--batches', '2', '--results-file', res])
    assert 'Acc@1' in out
    r = json.load(open(res))
    assert r['model'] == NAME and r['param_count'] == 42.71
