#!/usr/bin/env python3
"""ga_input_erase beside ga_u8_normalize on the same box: device time per launch (HIP events around a batch of launches, median
over rounds, the variants alternating inside every round) and algorithmic GB/s (input read once, fp32 output written once).

  python tools/input_erase_bench.py                       # every variant, B = 256 at 224 x 224
  rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 tools/input_erase_bench.py --variants u8norm,erase25
                                                          # per-kernel durations of the two from one trace

Variants: u8norm = ga_u8_normalize; erase0 = ga_input_erase, uint8, no boxes; erase25 = uint8, the recipe (probability 0.25, one
box, 'pixel'); erase100 = uint8, every sample one box; erase25x3 = probability 0.25, up to 3 boxes; const25 / const100 = as erase25 / erase100 in mode 'const' (the box tests without
the generator); copy25 = fp32 input, the recipe."""
import argparse
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagenet_models_amd as A  # noqa: E402
from imagenet_models_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('-b', '--batch', type=int, default=256)
ap.add_argument('--img', type=int, default=224)
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--launches', type=int, default=20, help='launches between the two events of one timing')
ap.add_argument('--variants', default='u8norm,erase0,erase25,erase100,erase25x3,const25,const100,copy25')
args = ap.parse_args()
B, S = args.batch, args.img
MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)

x8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device='cuda')
xf = torch.randn(B, 3, S, S, device='cuda')
out = torch.empty(B, 3, S, S, device='cuda')


def table(prob, max_count):
    era = A.RandomErasing(probability=prob, mode='pixel', max_count=max_count, rng=random.Random(0))
    tab = torch.zeros(B, max_count, 4, dtype=torch.int32)
    used = [0] * B
    for i, top, left, h, w in era.sample(B, S, S):
        tab[i, used[i]] = torch.tensor([top, left, h, w], dtype=torch.int32)
        used[i] += 1
    frac = float((tab[:, :, 2] * tab[:, :, 3]).sum()) / (B * S * S)
    return tab.cuda(), frac


def plan(name):
    p = ops.Plan()
    if name == 'u8norm':
        p.u8_normalize(x8, out, MEAN, STD)
        return p, x8, 0.0
    prob, mc = {'erase0': (0.0, 1), 'erase25': (0.25, 1), 'erase100': (1.0, 1), 'erase25x3': (0.25, 3), 'const25': (0.25, 1),
                'const100': (1.0, 1), 'copy25': (0.25, 1)}[name]
    tab, frac = table(prob, mc)
    x = xf if name.startswith('copy') else x8
    p.input_erase(x, out, tab, mc, 0 if name.startswith('const') else 2, 1, 0, MEAN, STD)
    return p, x, frac


names = args.variants.split(',')
plans = {n: plan(n) for n in names}
for n in names:
    for _ in range(3):
        plans[n][0].run()
torch.cuda.synchronize()
times = {n: [] for n in names}
for _ in range(args.rounds):
    for n in names:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            plans[n][0].run()
        e1.record()
        times[n].append((e0, e1))
torch.cuda.synchronize()
print(f'B = {B}, {S} x {S}; {args.rounds} rounds of {args.launches} launches; us per launch: median (min .. max of the rounds)')
for n in names:
    t = sorted(a.elapsed_time(b) * 1e3 / args.launches for a, b in times[n])
    _, x, frac = plans[n]
    nbytes = x.numel() * x.element_size() + out.numel() * 4
    med = t[len(t) // 2]
    print(f'{n:10s} {med:8.1f} us  ({t[0]:.1f} .. {t[-1]:.1f})  {nbytes / med / 1e3:7.0f} GB/s   erased fraction {frac:.3f}', flush=True)
