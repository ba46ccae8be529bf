"""GPU parity of the plain PiT (pit_s; MAP/models/map_pit.py, PoolingTransformer with pool_type='gap') through the
C ABI, against tests/golden/pit_gap_*.npz written by tools/gen_golden_pit_gap.py from the REAL reference class:
  * eval logits and top-5 of the registered pit_s;
  * one train step of the narrow V8 configuration (cross entropy, no DropPath) against the fp32 and the float64 run of the reference;
  * the bf16 mode against the fp32-mode step;
  * one fused TrainStep (adamw) and an eval pass of the full pit_s.
Metrics and gate values are those tests/test_map_pit_gpu.py applies to the pit_v8 fixtures -- logits max|a - b| / max|b| and relative
loss 1e-3 (bf16: 6e-2 / 2e-2), gradient norms |n - n*| / max(n*, 1e-3 max n*) 2e-2 -- the float64 file additionally under the per-tensor
5e-3 of tests/test_fp64_truth_gpu.py (norm, and 16-value head relative to the tensor's max), the bf16 gradients under tests/_gradcheck.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _gradcheck import assert_grads_close, BF16_REL, BF16_COS
from _mnv1_state import fill_state
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _gen_input(batch, seed, size):
    from oracle.map_pit_oracle import gen_input
    return gen_input(batch, seed=seed, size=size)


def _fill(m):
    m.load_state_dict(fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    return m


def rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@functools.lru_cache(maxsize=None)
def _narrow_step(mode):
    """one train step of the narrow configuration in `mode`: (logits, loss, {name: gradient}) on the CPU, computed once"""
    import imagenet_models_amd as A
    z = np.load(os.path.join(GOLDEN, 'pit_gap_v8_train_b4.npz'))
    cfg = json.loads(str(z['cfg']))
    m = _fill(A.PiT(pool_type='gap', drop_path_rate=0.0, math_mode=mode, **cfg)).cuda().train()
    x = _gen_input(int(z['batch']), 1, cfg['image_size'])
    m.zero_grad()
    out = m(x.cuda())
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (int(z['batch']), cfg['num_classes'])      # one tensor in train mode
    loss = F.cross_entropy(out, torch.from_numpy(z['target']).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().float().cpu(), float(loss.detach()), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}


@pytest.mark.parametrize('mode,tol', [('fp32', 1e-3), ('bf16', 6e-2)])
def test_eval_against_reference_fixture(mode, tol):
    import imagenet_models_amd as A
    z = np.load(os.path.join(GOLDEN, 'pit_gap_eval.npz'))
    m = _fill(A.create_model('pit_s', math_mode=mode)).cuda().eval()
    assert sum(p.numel() for p in m.parameters()) == int(z['param_count'])
    x = _gen_input(int(z['batch']), int(z['input_seed']), 224)
    assert np.array_equal(x.reshape(-1)[:16].numpy(), z['input_head']) and float(x.double().sum()) == float(z['input_sum'])
    with torch.no_grad():
        out = m(x.cuda())
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (int(z['batch']), 1000)
    got = out.float().cpu()
    e = rel(got[:, :z['logits'].shape[1]], z['logits'])
    print(f'[pit_gap {mode}] eval logits vs reference fixture: {e:.3e}')
    assert e < tol
    if mode == 'fp32':
        assert np.array_equal(got.topk(5, 1, True, True)[1].numpy(), z['top5'])


def _norm_errors(grads, z):
    names = [str(n) for n in z['grad_names']]
    assert set(names) == set(grads), sorted(set(names) ^ set(grads))[:6]
    gmax = float(z['grad_norm'].max())
    e = {n: abs(float(grads[n].norm()) - w) / max(w, 1e-3 * gmax) for n, w in zip(names, z['grad_norm'].tolist())}
    return sorted(e.items(), key=lambda kv: -kv[1])


@pytest.mark.parametrize('tag', ['pit_gap_v8_train_b4', 'pit_gap_v8_train_b4_fp64'])
def test_train_step_against_reference_fixture(tag):
    z = np.load(os.path.join(GOLDEN, tag + '.npz'))
    out, loss, grads = _narrow_step('fp32')
    e_out = rel(out, z['logits'])
    e_loss = abs(loss - float(z['loss'])) / abs(float(z['loss']))
    worst = _norm_errors(grads, z)
    print(f'[{tag} fp32 mode] vs reference fixture: logits {e_out:.2e} loss {e_loss:.2e} worst grad norms {worst[:4]}')
    assert e_out < 1e-3 and e_loss < 1e-3 and worst[0][1] < 2e-2, worst[:8]
    if tag.endswith('_fp64'):
        gmax = float(z['grad_absmax'].max())
        per = []
        for i, n in enumerate(str(n) for n in z['grad_names']):
            amax, nref = float(z['grad_absmax'][i]), float(z['grad_norm'][i])
            head = grads[n].reshape(-1)[:16].numpy()
            dh = float(np.abs(head - z['grad_head'][i][:head.size]).max())
            if amax >= 1e-4 * gmax:
                per.append((max(abs(float(grads[n].norm()) - nref) / nref, dh / amax), n))
            else:
                per.append((dh / (1e-4 * gmax) * 5e-3, n))      # analytically-zero gradients: |.| < 1e-4 of the global max
        per.sort(reverse=True)
        print(f'[{tag} fp32 mode] per-tensor norm / head errors against float64: worst {per[:5]}')
        assert per[0][0] < 5e-3, per[:10]


def test_bf16_mode_against_fp32_mode_step():
    out32, loss32, g32 = _narrow_step('fp32')
    out16, loss16, g16 = _narrow_step('bf16')
    e_out = rel(out16, out32)
    e_loss = abs(loss16 - loss32) / abs(loss32)
    print(f'[pit_gap_v8 bf16 vs fp32 mode] logits {e_out:.2e} loss {e_loss:.2e}')
    assert e_out < 6e-2 and e_loss < 2e-2
    assert_grads_close(g16, g32, BF16_REL, BF16_COS, 'pit_gap_v8 bf16 vs fp32 mode')


def test_fused_train_step_and_eval_of_the_full_model():
    import imagenet_models_amd as A
    B = 4
    m = _fill(A.create_model('pit_s', drop_path_rate=0.1)).cuda().train()
    opt = A.create_optimizer_v2(m, opt='adamw', lr=1e-3, weight_decay=0.05)
    step = A.TrainStep(m, opt, B)
    x = _gen_input(B, 2, 224).cuda()
    target = torch.tensor([1, 10, 100, 999], device='cuda')
    before = m.head.weight.detach().clone()
    loss = step(x, target)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and 0.0 < float(loss) < 50.0
    assert not torch.equal(before, m.head.weight.detach()), 'the optimizer did not move the classifier'
    assert all(torch.isfinite(p).all() for p in m.parameters())
    m.eval()
    with torch.no_grad():
        out = m(x)
    assert tuple(out.shape) == (B, 1000) and torch.isfinite(out).all()
    s, idx = A.heads_topk(out, 5)
    assert tuple(idx.shape) == (B, 5)
