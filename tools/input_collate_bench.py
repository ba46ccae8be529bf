#!/usr/bin/env python3
"""ga_input_collate (mix in uint8 -> normalise -> erase, one pass) beside the two launches it replaces in the default order,
ga_input_erase (normalise + erase) followed by ga_mixup_batch (fp32 mixup / cutmix), on the same box: device time per call (HIP
events around a batch of calls, median over rounds, the variants alternating inside every round) and the bytes each variant
must move at the least (its algorithmic bytes; partner reads counted once, as HBM traffic they are cache hits at best).

  python tools/input_collate_bench.py                     # every variant, B = 256 uint8 at 224 x 224, the recipe's settings
  rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 tools/input_collate_bench.py --variants fused_elem,two_mixup

The recipe: RandomErasing probability 0.25, one box, 'pixel'; mixup 0.8 / cutmix 1.0.  Variants:
  u8norm       ga_u8_normalize alone (the floor of any input stage: 1 B read, 4 B written per element)
  erase        ga_input_erase alone (the default order's first launch)
  two_mixup    ga_input_erase + ga_mixup_batch, a mixup batch        two_cutmix    ... a cutmix batch
  fused_mixup  ga_input_collate, every row 'mixup' (mode 'batch')    fused_cutmix  every row 'cutmix', one box
  fused_elem   ga_input_collate, the rows FastCollateMixup(mode='elem') draws (mixup and cutmix rows side by side)
  fused_none   ga_input_collate, every row 'none' (mixup switched off: must cost what `erase` costs)
The two orders do not compute the same thing (that is the point of the fused pass); the timing compares what each costs."""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagenet_models_amd as A  # noqa: E402
from imagenet_models_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('-b', '--batch', type=int, default=256)
ap.add_argument('--img', type=int, default=224)
ap.add_argument('--rounds', type=int, default=21)
ap.add_argument('--launches', type=int, default=200, help='calls between the two events of one timing')
ap.add_argument('--variants', default='u8norm,erase,two_mixup,two_cutmix,fused_mixup,fused_cutmix,fused_elem,fused_none')
args = ap.parse_args()
B, S = args.batch, args.img
MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)
LAM, BOX = 0.6, (40, 180, 30, 170)          # a cutmix box of 140 x 140: lam = 0.61

x8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device='cuda')
mid = torch.empty(B, 3, S, S, device='cuda')
out = torch.empty(B, 3, S, S, device='cuda')
n = x8.numel()

era = A.RandomErasing(probability=0.25, mode='pixel', max_count=1, rng=random.Random(0))
etab = torch.zeros(B, 1, 4, dtype=torch.int32)
for i, top, left, h, w in era.sample(B, S, S):
    etab[i, 0] = torch.tensor([top, left, h, w], dtype=torch.int32)
erased = float((etab[:, :, 2] * etab[:, :, 3]).sum()) / (B * S * S)
etab = etab.cuda()


def rows(kind):
    t = np.zeros((B, 8), dtype=np.int32)
    t[:, 0] = kind
    t[:, 1:5] = BOX if kind == 2 else 0
    t[:, 5] = np.full(B, LAM, dtype=np.float32).view(np.int32)
    t[:, 6] = np.full(B, 1.0 - LAM, dtype=np.float32).view(np.int32)
    return t


def plan(name):
    """-> (plan, algorithmic bytes, fraction of the elements whose partner is read)"""
    p = ops.Plan()
    if name == 'u8norm':
        p.u8_normalize(x8, out, MEAN, STD)
        return p, 5 * n, 0.0
    if name == 'erase':
        p.input_erase(x8, out, etab, 1, 2, 1, 0, MEAN, STD)
        return p, 5 * n, 0.0
    if name.startswith('two_'):
        cut = name == 'two_cutmix'
        p.input_erase(x8, mid, etab, 1, 2, 1, 0, MEAN, STD)
        p.mixup_batch(mid, out, LAM, cut, BOX)
        # 1 B + 4 B, then 4 B read + 4 B written; the partner's 4 B are a second read of a buffer the pass reads anyway
        return p, 13 * n, 1.0 if not cut else (BOX[1] - BOX[0]) * (BOX[3] - BOX[2]) / (S * S)
    if name == 'fused_elem':
        fm = A.FastCollateMixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode='elem', rng=np.random.RandomState(0))
        t = fm.sample(B, S, S)
        part = float(np.where(t[:, 0] == 1, 1.0, np.where(t[:, 0] == 2, (t[:, 2] - t[:, 1]) * (t[:, 4] - t[:, 3]) / (S * S), 0.0)).mean())
    else:
        kind = {'fused_none': 0, 'fused_mixup': 1, 'fused_cutmix': 2}[name]
        t = rows(kind)
        part = (0.0, 1.0, (BOX[1] - BOX[0]) * (BOX[3] - BOX[2]) / (S * S))[kind]
    mix = torch.from_numpy(t).cuda()
    p.input_collate(x8, out, mix, etab, 1, 2, 1, 0, MEAN, STD)
    return p, 5 * n, part


names = args.variants.split(',')
plans = {k: plan(k) for k in names}
for k in names:
    for _ in range(5):
        plans[k][0].run()
torch.cuda.synchronize()
times = {k: [] for k in names}
for _ in range(args.rounds):
    for k in names:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            plans[k][0].run()
        e1.record()
        times[k].append((e0, e1))
torch.cuda.synchronize()
print(f'B = {B}, uint8 {S} x {S}, erased fraction {erased:.3f}; {args.rounds} rounds of {args.launches} calls, variants alternating in '
      f'every round; us per call: median (min .. max of the rounds)')
med = {}
for k in names:
    t = sorted(a.elapsed_time(b) * 1e3 / args.launches for a, b in times[k])
    _, nbytes, part = plans[k]
    med[k] = t[len(t) // 2]
    print(f'{k:13s} {med[k]:8.1f} us  ({t[0]:.1f} .. {t[-1]:.1f})  {nbytes / 1e6:7.1f} MB  {nbytes / med[k] / 1e3:7.0f} GB/s   '
          f'partner read for {part:.2f} of the elements', flush=True)
for f, t in (('fused_mixup', 'two_mixup'), ('fused_cutmix', 'two_cutmix'), ('fused_elem', 'two_mixup'), ('fused_none', 'erase')):
    if f in med and t in med:
        print(f'{f} / {t}: {med[f] / med[t]:.3f}  ({med[t] - med[f]:+.1f} us saved)')
