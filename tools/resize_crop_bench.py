#!/usr/bin/env python3
"""ga_resize_crop (timm's RandomResizedCrop + flip / Resize + CenterCrop of DECODED images) beside ga_u8_normalize, the floor of any
input stage, on the same box: device time per call (HIP events around a batch of calls, median over rounds, the variants
alternating inside every round), the host-to-device copy of the sources that comes with the stage, and PIL's time per image on one
host core for the same boxes, as context.

  python tools/resize_crop_bench.py                      # B = 256 sources of 375 x 500 -> 224 x 224
  rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 tools/resize_crop_bench.py --variants train --pil 0

Variants:
  u8norm    ga_u8_normalize alone on the (B, 3, S, S) batch (1 B read, 4 B written per element)
  train     the rows RandomResizedCrop(S) draws at its defaults (scale 0.08 .. 1, ratio 3/4 .. 4/3, 'random' interpolation, flips)
  bilinear  the same boxes, every row bilinear
  bicubic   the same boxes, every row bicubic
  eval      ResizeCenterCrop(S, 0.875, 'bicubic'): the whole image to short side floor(S / 0.875), the centre window
  h2d       the non_blocking copy of the packed sources from pinned memory (what shipping decoded sources costs)
  h2d_box   the same for the boxes of `train` only: crop-then-resize sees nothing else"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagenet_models_amd as A  # noqa: E402
from imagenet_models_amd import _lib, ops, resize_crop as RC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('-b', '--batch', type=int, default=256)
ap.add_argument('--img', type=int, default=224)
ap.add_argument('--source', default='375x500')
ap.add_argument('--rounds', type=int, default=11)
ap.add_argument('--launches', type=int, default=20, help='calls between the two events of one timing')
ap.add_argument('--variants', default='u8norm,train,bilinear,bicubic,eval,h2d,h2d_box')
ap.add_argument('--pil', type=int, default=16, help='images PIL resizes on one host core for the context line (0: none)')
args = ap.parse_args()
B, S = args.batch, args.img
SH, SW = (int(v) for v in args.source.lower().split('x'))
MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)

heights, widths = [SH] * B, [SW] * B
offsets, total = RC.pack_offsets(heights, widths)
src = torch.randint(0, 256, (total,), dtype=torch.uint8, device='cuda')
host_src = torch.empty(total, dtype=torch.uint8).pin_memory()
host_src.copy_(src)
x8 = torch.empty(B, 3, S, S, dtype=torch.uint8, device='cuda')
outf = torch.empty(B, 3, S, S, device='cuda')
lib = _lib.load()
keep = []

train = A.RandomResizedCrop(S, rng=random.Random(0), torch_gen=torch.Generator().manual_seed(0)).sample(heights, widths, offsets)
tables = {'train': train, 'bilinear': train.copy(), 'bicubic': train.copy(),
          'eval': A.ResizeCenterCrop(S, 0.875, 'bicubic').rows(heights, widths, offsets)}
tables['bilinear']['interp'] = RC.BILINEAR
tables['bicubic']['interp'] = RC.BICUBIC
box_bytes = int((3 * train['h'].astype(np.int64) * train['w']).sum())
host_box = torch.empty(box_bytes, dtype=torch.uint8).pin_memory()
dev_box = torch.empty(box_bytes, dtype=torch.uint8, device='cuda')


class Copy:
    def __init__(self, dst, host):
        self.dst, self.host = dst, host

    def run(self):
        self.dst.copy_(self.host, non_blocking=True)


def plan(name):
    """-> (runnable, algorithmic bytes, note)"""
    if name == 'u8norm':
        p = ops.Plan()
        p.u8_normalize(x8, outf, MEAN, STD)
        return p, 5 * x8.numel(), ''
    if name == 'h2d':
        return Copy(src, host_src), total, 'pinned host -> device, the whole sources'
    if name == 'h2d_box':
        return Copy(dev_box, host_box), box_bytes, 'pinned host -> device, the boxes of `train` only'
    t = tables[name]
    _lib.check(lib.ga_resize_crop_check_table(t.ctypes.data, B, S, S, total), 'ga_resize_crop_check_table')
    need = int(lib.ga_resize_crop_work_bytes(t.ctypes.data, B, S, S))
    dev = torch.from_numpy(t.view(np.uint8).copy()).cuda()
    work = torch.empty(need, dtype=torch.uint8, device='cuda')
    keep.extend((dev, work))
    p = ops.Plan()
    p.resize_crop(src, dev, x8, work, B, S, S)
    read = int((3 * t['h'].astype(np.int64) * t['w']).sum())
    mid = int((3 * t['h'].astype(np.int64) * S).sum())
    note = (f'boxes {read / 1e6:.1f} MB read, {mid / 1e6:.1f} MB between the passes (written and read), {x8.numel() / 1e6:.1f} MB out; '
            f'bicubic rows {int((t["interp"] == 3).sum())}, flips {int(t["flip"].sum())}, workspace {need / 1e6:.1f} MB')
    return p, read + 2 * mid + x8.numel(), note


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
print(f'B = {B}, sources {SH} x {SW} -> uint8 {S} x {S}; {args.rounds} rounds of {args.launches} calls, variants alternating in every '
      f'round; us per call: median (min .. max of the rounds)')
med = {}
for k in names:
    t = sorted(a.elapsed_time(b) * 1e3 / args.launches for a, b in times[k])
    _, nbytes, note = plans[k]
    med[k] = t[len(t) // 2]
    print(f'{k:10s} {med[k]:9.1f} us  ({t[0]:.1f} .. {t[-1]:.1f})  {nbytes / 1e6:7.1f} MB  {nbytes / med[k] / 1e3:7.0f} GB/s  '
          f'{B / med[k] * 1e6:9.0f} img/s   {note}', flush=True)
if 'u8norm' in med:
    rate = plans['u8norm'][1] / med['u8norm']
    for k in names:
        if k in tables:
            print(f'{k}: its {plans[k][1] / 1e6:.1f} MB at the rate of ga_u8_normalize in this run ({rate / 1e3:.0f} GB/s) would take '
                  f'{plans[k][1] / rate:.1f} us; it takes {med[k]:.1f} us = {med[k] / (plans[k][1] / rate):.1f} x')

if args.pil:
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is None:
        print('PIL is not installed: no host context line')
    else:
        torch.set_num_threads(1)
        n = min(args.pil, B)
        imgs = [Image.fromarray(host_src[o:o + 3 * SH * SW].numpy().reshape(SH, SW, 3), 'RGB') for o in offsets[:n]]
        for name in ('train', 'eval'):
            t0 = time.perf_counter()
            for im, r in zip(imgs, tables[name][:n]):
                top, left, h, w = int(r['top']), int(r['left']), int(r['h']), int(r['w'])
                o = im.crop((left, top, left + w, top + h)).resize((int(r['vw']), int(r['vh'])), int(r['interp']))
                if r['flip']:
                    o = o.transpose(Image.FLIP_LEFT_RIGHT)
                o = o.crop((int(r['ox']), int(r['oy']), int(r['ox']) + S, int(r['oy']) + S))
                np.asarray(o)
            dt = (time.perf_counter() - t0) / n
            print(f'PIL on one host core, the rows of `{name}`: {dt * 1e3:.2f} ms per image, {1 / dt:.0f} img/s ({n} images)')
