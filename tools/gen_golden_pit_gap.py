"""Fixtures of the plain PiT (pool_type='gap') from the REAL reference class (MAP/models/map_pit.py, PoolingTransformer; timm's
Block comes from oracle/timm_stub, reused by import only):

  tests/golden/pit_gap_eval.npz               the registered pit_s, B = 2, eval, fp32: state names / shapes / count, parameter count,
                                              the input (its seed, first 16 values and sum: the tests regenerate it with
                                              gen_input and check these; the array itself is 600 KB), 256 logits per row, top-5
  tests/golden/pit_gap_v8_train_b4.npz        the narrow configuration of the pit_v8 fixtures (oracle/gen_golden_pit.py: V8) with
                                              pool_type='gap': one train step's forward + backward at B = 4, CrossEntropyLoss
                                              (smoothing 0), drop_path_rate 0: loss, logits, and per parameter gradient its norm /
                                              sum / max |.| / first 16 values
  tests/golden/pit_gap_v8_train_b4_fp64.npz   the same step with the reference class in float64 (m.double()), same fields

The state is the name-hashed fill of tests/_mnv1_state.py over the reference module's own state_dict, so that the tests fill this
package's container identically without shipping the weights; the input is oracle.map_pit_oracle.gen_input.  Everything is seeded:
two runs write equal arrays.

Run (needs the reference tree; not part of the test suite):
    python tools/gen_golden_pit_gap.py /path/to/reference/MAP/models"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'timm_stub'))

from _mnv1_state import fill_state  # noqa: E402
from oracle.map_pit_oracle import gen_input  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
NLOG = 256      # logits kept per row of the 1000-class eval fixture
V8 = dict(image_size=64, patch_size=16, stride=8, base_dims=(48, 48, 48), depth=(1, 2, 1), heads=(1, 2, 4), num_classes=40)


def load_reference(models_dir):
    sys.path.insert(0, models_dir)
    import map_pit
    return map_pit


def fill(m):
    sd = fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(sd)
    return sd


def run_eval(ref):
    m = ref.pit_s(False)
    assert m.pool_type == 'gap' and isinstance(m.head, nn.Linear)
    sd = fill(m)
    m.eval()
    x = gen_input(2, seed=0, size=224)
    with torch.no_grad():
        lg = m(x)
    assert lg.shape == (2, 1000)
    amax = float(lg.abs().max())
    print(f'[pit_gap] eval logits max |.| {amax:.3f}')
    assert 0.05 < amax < 50, 'eval logits are not O(1)'
    names = list(sd)
    np.savez_compressed(os.path.join(OUT, 'pit_gap_eval.npz'), batch=2, n_state=len(sd), param_count=sum(p.numel() for p in m.parameters()),
                        state_names=np.array(names), state_shapes=np.array([str(tuple(sd[n].shape)) for n in names]),
                        input_seed=0, input_head=x.reshape(-1)[:16].numpy(), input_sum=float(x.double().sum()),
                        logits=lg[:, :NLOG].numpy().astype(np.float32),
                        top5=lg.topk(5, 1, True, True)[1].numpy())


def run_train(ref, fp64):
    cfg = dict(V8)
    m = ref.PoolingTransformer(image_size=cfg['image_size'], patch_size=cfg['patch_size'], stride=cfg['stride'],
                               base_dims=list(cfg['base_dims']), depth=list(cfg['depth']), heads=list(cfg['heads']), mlp_ratio=4,
                               num_classes=cfg['num_classes'], pool_type='gap', drop_path_rate=0.0)
    fill(m)                                     # filled in fp32, widened below for the float64 run
    B = 4
    x = gen_input(B, seed=1, size=cfg['image_size'])
    if fp64:
        m.double()
        x = x.double()
    m.train()
    target = torch.randint(0, cfg['num_classes'], (B,), generator=torch.Generator().manual_seed(99))
    lg = m(x)
    assert lg.shape == (B, cfg['num_classes'])           # one tensor in train mode too
    loss = nn.CrossEntropyLoss()(lg, target)
    loss.backward()
    grads = {n: p.grad.detach() for n, p in m.named_parameters()}
    want = torch.float64 if fp64 else torch.float32
    assert loss.dtype == want and lg.dtype == want and all(g.dtype == want for g in grads.values())
    names = list(grads)
    head = np.zeros((len(names), 16), dtype=np.float64 if fp64 else np.float32)
    for i, n in enumerate(names):
        f = grads[n].reshape(-1)[:16]
        head[i, :f.numel()] = f.numpy()
    tag = 'pit_gap_v8_train_b4' + ('_fp64' if fp64 else '')
    print(f'[{tag}] loss {float(loss.detach()):.12f}, logits max |.| {float(lg.detach().abs().max()):.3f}, {len(names)} gradient tensors')
    np.savez_compressed(os.path.join(OUT, tag + '.npz'), cfg=json.dumps(cfg), batch=B, target=target.numpy(), loss=float(loss.detach()),
                        logits=lg.detach().numpy(), grad_names=np.array(names),
                        grad_norm=np.array([float(grads[n].double().norm()) for n in names]),
                        grad_sum=np.array([float(grads[n].double().sum()) for n in names]),
                        grad_absmax=np.array([float(grads[n].abs().max()) for n in names]), grad_head=head)


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)                    # one thread: the same summation order on every run
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('MAP_MODELS_DIR', ''))
    run_eval(ref)
    run_train(ref, fp64=False)
    run_train(ref, fp64=True)
    print('golden vectors written to', OUT)
