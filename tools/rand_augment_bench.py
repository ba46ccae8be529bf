#!/usr/bin/env python3
"""ga_rand_augment (timm's --aa rand-m9-mstd0.5-inc1 on the uint8 batch) beside ga_u8_normalize, the floor of any input stage, on
the same box: device time per call (HIP events around a batch of calls, median over rounds, the variants alternating inside every
round) and the bytes each variant must move at the least (every layer reads and writes the uint8 batch once).

  python tools/rand_augment_bench.py                      # B = 256 uint8 at 224 x 224
  rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 tools/rand_augment_bench.py --variants recipe

Variants:
  u8norm    ga_u8_normalize alone (1 B read, 4 B written per element)
  recipe    the table RandAugment('rand-m9-mstd0.5-inc1') draws: two layers, each applied with p = 0.5, 15 ops drawn uniformly
  none      two layers, every row 'none' (p = 0): what the two copies of the batch cost
  <kind>    ONE layer with every row that kind: where the time of `recipe` goes (color, contrast, sharpness, autocontrast, equalize,
            posterize, rotate_bilinear, rotate_bicubic, shear_bicubic, translate_nearest)"""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagenet_models_amd as A  # noqa: E402
from imagenet_models_amd import ops, rand_augment as RA  # noqa: E402

KINDS = ('color', 'contrast', 'sharpness', 'autocontrast', 'equalize', 'posterize', 'rotate_bilinear', 'rotate_bicubic', 'shear_bicubic',
         'translate_nearest')
ap = argparse.ArgumentParser()
ap.add_argument('-b', '--batch', type=int, default=256)
ap.add_argument('--img', type=int, default=224)
ap.add_argument('--rounds', type=int, default=11)
ap.add_argument('--launches', type=int, default=20, help='calls between the two events of one timing')
ap.add_argument('--variants', default='u8norm,recipe,none,' + ','.join(KINDS))
args = ap.parse_args()
B, S = args.batch, args.img
MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)

x8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device='cuda')
out8 = torch.empty_like(x8)
outf = torch.empty(B, 3, S, S, device='cuda')
n = x8.numel()
keep = []


def one_kind(name):
    t = np.zeros((B, 1), dtype=RA.ROW)
    t['m'] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if name in ('color', 'contrast', 'sharpness'):
        t['kind'], t['farg'] = {'color': RA.COLOR, 'contrast': RA.CONTRAST, 'sharpness': RA.SHARPNESS}[name], 1.45
    elif name in ('autocontrast', 'equalize'):
        t['kind'] = RA.AUTOCONTRAST if name == 'autocontrast' else RA.EQUALIZE
    elif name == 'posterize':
        t['kind'], t['iarg'] = RA.POSTERIZE, 2
    else:
        form, interp = name.split('_')
        t['kind'], t['interp'] = RA.AFFINE, {'nearest': RA.NEAREST, 'bilinear': RA.BILINEAR, 'bicubic': RA.BICUBIC}[interp]
        t['m'] = {'rotate': RA.rotate_matrix(27.0, S, S), 'shear': (1.0, 0.27, 0.0, 0.0, 1.0, 0.0),
                  'translate': (1.0, 0.0, 0.405 * S, 0.0, 1.0, 0.0)}[form]
    return t


def plan(name):
    """-> (plan, algorithmic bytes, note)"""
    p = ops.Plan()
    if name == 'u8norm':
        p.u8_normalize(x8, outf, MEAN, STD)
        return p, 5 * n, ''
    if name == 'recipe':
        t = A.RandAugment('rand-m9-mstd0.5-inc1', rng=random.Random(0), np_rng=np.random.RandomState(0)).sample(B, S, S)
    elif name == 'none':
        t = A.RandAugment('rand-m9-mstd0.5-inc1-p0', rng=random.Random(0), np_rng=np.random.RandomState(0)).sample(B, S, S)
    else:
        t = one_kind(name)
    layers = t.shape[1]
    k = t['kind'].reshape(-1)
    geo = k == RA.AFFINE
    note = (f'{int((k != 0).sum())} of {k.size} rows applied; affine {int(geo.sum())} (bicubic {int((t["interp"].reshape(-1)[geo] == 3).sum())}), '
            f'sharpness {int((k == RA.SHARPNESS).sum())}, histogram / mean {int(np.isin(k, (1, 2, 8)).sum())}')
    dev = torch.from_numpy(t.reshape(-1).view(np.uint8).copy()).cuda()
    work = torch.empty(p.rand_augment_work_bytes(B, 3, S, S, layers), dtype=torch.uint8, device='cuda')
    keep.extend((dev, work))
    p.rand_augment(x8, out8, work, dev, layers, (124, 116, 104))
    return p, 2 * n * layers, note


names = args.variants.split(',')
plans = {k: plan(k) for k in names}
for k in names:
    for _ in range(3):
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
print(f'B = {B}, uint8 {S} x {S}; {args.rounds} rounds of {args.launches} calls, variants alternating in every round; us per call: median '
      f'(min .. max of the rounds)')
med = {}
for k in names:
    t = sorted(a.elapsed_time(b) * 1e3 / args.launches for a, b in times[k])
    _, nbytes, note = plans[k]
    med[k] = t[len(t) // 2]
    print(f'{k:18s} {med[k]:9.1f} us  ({t[0]:.1f} .. {t[-1]:.1f})  {nbytes / 1e6:7.1f} MB  {nbytes / med[k] / 1e3:7.0f} GB/s   {note}', flush=True)
if 'u8norm' in med:
    rate = plans['u8norm'][1] / med['u8norm']
    for k in names:
        if k != 'u8norm':
            print(f'{k}: its {plans[k][1] / 1e6:.1f} MB at the rate of ga_u8_normalize in this run ({rate / 1e3:.0f} GB/s) would take '
                  f'{plans[k][1] / rate:.1f} us; it takes {med[k]:.1f} us = {med[k] / (plans[k][1] / rate):.1f} x; {B / med[k] * 1e6:.0f} img/s')
