"""Fixtures of MobileNetV1 / MAP-MobileNetV1 from the REAL reference classes (MAP/models/map_mobilenet.py, MAPHead of MAP/models/map.py):

  tests/golden/{mnv1,map_mnv1}_eval.npz      state names / shapes / parameter count, the running statistics the eval pass uses, logits
                                             and top-5 of a B = 2 eval forward
  tests/golden/{mnv1,map_mnv1}_train_b4.npz  one train step at B = 4, 224 x 224, fp32: loss, logits, per-tensor gradient norm / sum /
                                             first 16 elements, and the running statistics after the step

State: the name-hashed fill of tests/_mnv1_state.py over the reference module's own state_dict.  Every nn.Dropout is set to p = 0
(MAPHead's attention dropout defaults to 0.05).  The eval state's running statistics come from one train-mode reference forward
with momentum 1 (a B = 4 batch of its own), so that the logits of the 27-layer ReLU trunk stay O(1); the hashed running
statistics would not.  The reference always builds 1000 classes; the fixtures keep them all.

Run (needs the reference tree and its timm stub; not part of the test suite):
    python tools/gen_golden_mobilenet.py /path/to/reference/MAP/models"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'timm_stub'))

from _mnv1_state import fill_state, running_names  # noqa: E402
from oracle.ga_convnext_oracle import gen_input  # noqa: E402
from oracle.gen_golden import grad_stats  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')


def load_reference(models_dir):
    sys.path.insert(0, models_dir)
    stub = types.ModuleType('torchsummary')      # map_mobilenet.py imports torchsummary.summary at module level and never calls it
    stub.summary = lambda *a, **k: None
    sys.modules.setdefault('torchsummary', stub)
    import map_mobilenet
    return map_mobilenet


def build(ref, use_map):
    m = ref.MobileNetV1(ch_in=3, n_classes=1000, use_map=use_map)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    sd = fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(sd)
    return m, sd


def logits_of(out):
    return torch.stack(out) if isinstance(out, (list, tuple)) else out[None]


NLOG = 256      # logits kept per row (of 1000 classes): enough for the parity gate, small fixtures


def running(m):
    sd = m.state_dict()
    names = running_names(list(sd))
    return names, [sd[n].reshape(-1) for n in names]


def run(ref, tag, use_map):
    # ---- eval: running statistics from one train-mode pass (momentum 1), then a B = 2 eval forward
    m, sd = build(ref, use_map)
    bns = [mod for mod in m.modules() if isinstance(mod, nn.BatchNorm2d)]
    for bn in bns:
        bn.momentum = 1.0
    m.train()
    with torch.no_grad():
        m(gen_input(4, seed=7))
    for bn in bns:
        bn.momentum = 0.1
        bn.num_batches_tracked.zero_()
        # stored as float16: round them here so that the reference logits below are those of the state the tests rebuild
        bn.running_mean.copy_(bn.running_mean.half().float())
        bn.running_var.copy_(bn.running_var.half().float())
    m.eval()
    with torch.no_grad():
        lg = logits_of(m(gen_input(2, seed=0)))
    amax = float(lg.abs().max())
    print(f'[{tag}] eval logits max |.| {amax:.3f}')
    assert 0.05 < amax < 50, 'eval logits are not O(1)'
    rnames, rvals = running(m)
    names = list(sd)
    np.savez_compressed(os.path.join(OUT, f'{tag}_eval.npz'), batch=2, use_map=use_map, n_state=len(sd),
                        param_count=sum(p.numel() for p in m.parameters()), state_names=np.array(names),
                        state_shapes=np.array([str(tuple(sd[n].shape)) for n in names]), running_names=np.array(rnames),
                        running=torch.cat(rvals).half().numpy(), logits=lg[:, :, :NLOG].numpy().astype(np.float32),
                        top5=lg.mean(0).topk(5, 1, True, True)[1].numpy())
    # ---- train: one step at B = 4 from the filled state
    m, sd = build(ref, use_map)
    m.train()
    B = 4
    x = gen_input(B, seed=1)
    target = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(99))
    lg = logits_of(m(x))
    loss = F.cross_entropy(lg[0], target)        # one output: map_loss (MAP/train.py:792-839) reduces to the cross-entropy
    loss.backward()
    grads = {n: p.grad.detach() for n, p in m.named_parameters()}
    gnames, norm, ssum, head = grad_stats(grads)
    rnames, rvals = running(m)     # after the step: per tensor norm, sum and first 16 elements
    rhead = np.zeros((len(rvals), 16), dtype=np.float32)
    for i, v in enumerate(rvals):
        rhead[i, :min(16, v.numel())] = v[:16].numpy()
    print(f'[{tag}] train B={B}: loss {float(loss.detach()):.5f}, logits max |.| {float(lg.detach().abs().max()):.3f}, {len(grads)} gradients')
    np.savez_compressed(os.path.join(OUT, f'{tag}_train_b4.npz'), batch=B, use_map=use_map, target=target.numpy(), loss=float(loss.detach()),
                        logits=lg.detach()[:, :, :NLOG].numpy().astype(np.float32), grad_names=np.array(gnames), grad_norm=norm,
                        grad_sum=ssum, grad_head=head, running_names=np.array(rnames),
                        running_norm=np.array([float(v.double().norm()) for v in rvals]),
                        running_sum=np.array([float(v.double().sum()) for v in rvals]), running_head=rhead)


if __name__ == '__main__':
    torch.manual_seed(0)
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('MAP_MODELS_DIR', ''))
    run(ref, 'mnv1', False)
    run(ref, 'map_mnv1', True)
