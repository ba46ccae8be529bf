"""Fixtures of MAP-ResNet50 from the REAL reference classes (MAP/models/map_resnet.py, MAPHead of MAP/models/map.py):

  tests/golden/map_rn50_eval.npz      state names / shapes / parameter count, the running statistics the eval pass uses, logits and
                                      top-5 of a B = 2 eval forward
  tests/golden/map_rn50_train_b4.npz  one train step at B = 4, 224 x 224, fp32: loss, logits, per-tensor gradient norm / sum / first 16
                                      elements, and the running statistics after the step
  tests/golden/map_rn50_train_b4_fp64.npz  (--fp64) the same train step with the reference classes in float64 (m.double()): the
                                      fields of oracle/gen_golden_fp64.py -- loss, 40 logits per row, per-tensor gradient norm / sum /
                                      max |.| / first 16 values -- the ground truth tests/test_map_resnet_gpu.py gates the fp32 engine on

Same recipe as tools/gen_golden_mobilenet.py: the name-hashed fill of tests/_mnv1_state.py over the reference module's own state_dict,
every nn.Dropout at p = 0, eval running statistics from one train-mode reference forward with momentum 1 (a B = 4 batch of its own),
256 logits per row, and the MAP loss of the other MAP fixtures (MAP/train.py:792-839 with dec_lam = -0.8).

The ONE deviation from the reference's forward: MAP_ResNet.forward (map_resnet.py:268-282) only hands the feature list to the head
for pool_type in ['mmcap', 'multi_gap']; map_resnet50 passes pool_type='map', so the reference calls self.head(x.mean([-2, -1]))
and raises IndexError.  The fixtures use the composition the checkpoint was trained with, built from the real modules:
    stem = m.stem(x); x = m.max_pool(stem); features = [stem, layer1(x), layer2(.), layer3(.), layer4(.)]; m.head(features)

Run (needs the reference tree and its timm stub; not part of the test suite):
    python tools/gen_golden_map_resnet.py /path/to/reference/MAP/models
    python tools/gen_golden_map_resnet.py --fp64 /path/to/reference/MAP/models"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'timm_stub'))

from _mnv1_state import fill_state, running_names  # noqa: E402
from oracle.ga_convnext_oracle import gen_input  # noqa: E402
from oracle.gen_golden import grad_stats  # noqa: E402
from oracle.gen_golden_map_variants import ref_loss  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
NLOG = 256      # logits kept per row (of 1000 classes)
TAG = 'map_rn50'


def load_reference(models_dir):
    sys.path.insert(0, models_dir)
    import map_resnet
    return map_resnet


def build(ref):
    m = ref.map_resnet50()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    sd = fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(sd)
    return m, sd


def forward_f10(m, x):
    """map_resnet.py:268-282 with the head on the feature list (see the module docstring)"""
    stem = m.stem(x)
    y = m.max_pool(stem)
    feats = [stem]
    for layer in m.layers:
        y = layer(y)
        feats.append(y)
    return m.head(feats)


def logits_of(out):
    """eval: [G][B][NC]; train: the org heads, then the avg heads ([2G][B][NC], the engine's layout)"""
    if isinstance(out[0], (list, tuple)):
        return torch.stack([o[0] for o in out] + [o[1] for o in out])
    return torch.stack(out)


def running(m):
    sd = m.state_dict()
    names = running_names(list(sd))
    return names, [sd[n].reshape(-1) for n in names]


def run(ref):
    # ---- eval: running statistics from one train-mode pass (momentum 1), then a B = 2 eval forward
    m, sd = build(ref)
    bns = [mod for mod in m.modules() if isinstance(mod, nn.BatchNorm2d)]
    for bn in bns:
        bn.momentum = 1.0
    m.train()
    with torch.no_grad():
        forward_f10(m, gen_input(4, seed=7))
    for bn in bns:
        bn.momentum = 0.1
        bn.num_batches_tracked.zero_()
        bn.running_mean.copy_(bn.running_mean.half().float())      # stored as float16
        bn.running_var.copy_(bn.running_var.half().float())
    m.eval()
    with torch.no_grad():
        lg = logits_of(forward_f10(m, gen_input(2, seed=0)))
    amax = float(lg.abs().max())
    print(f'[{TAG}] eval logits max |.| {amax:.3f}')
    assert 0.05 < amax < 50, 'eval logits are not O(1)'
    rnames, rvals = running(m)
    names = list(sd)
    np.savez_compressed(os.path.join(OUT, f'{TAG}_eval.npz'), batch=2, n_state=len(sd), param_count=sum(p.numel() for p in m.parameters()),
                        state_names=np.array(names), state_shapes=np.array([str(tuple(sd[n].shape)) for n in names]),
                        running_names=np.array(rnames), running=torch.cat(rvals).half().numpy(),
                        logits=lg[:, :, :NLOG].numpy().astype(np.float32), top5=lg.mean(0).topk(5, 1, True, True)[1].numpy())
    # ---- train: one step at B = 4 from the filled state
    m, sd = build(ref)
    m.train()
    B = 4
    x = gen_input(B, seed=1)
    target = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(99))
    out = forward_f10(m, x)
    lg = logits_of(out)
    loss = ref_loss(out, target, -0.8)
    loss.backward()
    grads = {n: p.grad.detach() for n, p in m.named_parameters()}
    gnames, norm, ssum, head = grad_stats(grads)
    rnames, rvals = running(m)
    rhead = np.zeros((len(rvals), 16), dtype=np.float32)
    for i, v in enumerate(rvals):
        rhead[i, :min(16, v.numel())] = v[:16].numpy()
    print(f'[{TAG}] train B={B}: loss {float(loss.detach()):.5f}, logits max |.| {float(lg.detach().abs().max()):.3f}, {len(grads)} gradients')
    np.savez_compressed(os.path.join(OUT, f'{TAG}_train_b4.npz'), batch=B, dec_lam=-0.8, target=target.numpy(), loss=float(loss.detach()),
                        logits=lg.detach()[:, :, :NLOG].numpy().astype(np.float32), grad_names=np.array(gnames), grad_norm=norm,
                        grad_sum=ssum, grad_head=head, running_names=np.array(rnames),
                        running_norm=np.array([float(v.double().norm()) for v in rvals]),
                        running_sum=np.array([float(v.double().sum()) for v in rvals]), running_head=rhead)


def run_fp64(ref):
    """the train step of run() in float64: same fill, input, target and loss; the state is filled in fp32 and widened"""
    m, _ = build(ref)
    m.double().train()
    B, nlog = 4, 40
    x = gen_input(B, seed=1).double()
    target = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(99))
    out = forward_f10(m, x)
    lg = logits_of(out).detach()
    loss = ref_loss(out, target, -0.8)
    loss.backward()
    grads = {n: p.grad.detach() for n, p in m.named_parameters()}
    assert loss.dtype == torch.float64 and lg.dtype == torch.float64 and all(g.dtype == torch.float64 for g in grads.values())
    names = list(grads)
    head = np.zeros((len(names), 16))
    for i, n in enumerate(names):
        f = grads[n].reshape(-1)[:16]
        head[i, :f.numel()] = f.numpy()
    print(f'[{TAG}] fp64 train B={B}: loss {float(loss.detach()):.12f}, {len(names)} gradient tensors')
    np.savez_compressed(os.path.join(OUT, f'{TAG}_train_b4_fp64.npz'), batch=B, dec_lam=-0.8, target=target.numpy(), loss=float(loss.detach()),
                        logits=lg[:, :, :nlog].numpy(), grad_names=np.array(names),
                        grad_norm=np.array([float(grads[n].norm()) for n in names]),
                        grad_sum=np.array([float(grads[n].sum()) for n in names]),
                        grad_absmax=np.array([float(grads[n].abs().max()) for n in names]), grad_head=head)


if __name__ == '__main__':
    torch.manual_seed(0)
    args = [a for a in sys.argv[1:] if a != '--fp64']
    ref = load_reference(args[0] if args else os.environ.get('MAP_MODELS_DIR', ''))
    if '--fp64' in sys.argv[1:]:
        run_fp64(ref)
    else:
        run(ref)
