#!/usr/bin/env python3
"""Repeated augmentation through the folder loader, measured on one box in alternating rounds: FolderLoader(aug_repeats=3) on one
rank, batches of 256 entries of 375 x 500, 4:2:0, quality 90 files,

  (a) decode-once: each distinct file of a batch (85 or 86 of 256) is read, entropy-decoded, uploaded and rebuilt once, the copies
      are RaggedBatch entries that share its bytes (what the loader does)
  (b) per-entry: the same order, every one of the 256 entries read and decoded on its own (FolderLoader(decode_once=False): what a
      loader without the sharing does, and what timm's host pipeline does per copy)

as end-to-end loader throughput in FED images per second: the files' bytes on disk (page cache) -> RaggedBatch on the device, one
epoch per arm and round, the consumer only waiting.  Before any timing the two arms' batches of one epoch are compared entry by
entry, byte for byte.

The files are made with PIL where it is importable (--pictures distinct pictures, written under --files names); otherwise the
largest file of tests/golden/jpeg_pil.npz is used for every name, and the report says so."""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import imagenet_models_amd as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('-b', '--batch', type=int, default=256)
ap.add_argument('--files', type=int, default=16384, help='files in the folder: an epoch feeds files // 256 * 256 samples')
ap.add_argument('--pictures', type=int, default=128, help='distinct pictures among the files')
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--threads', type=int, default=16)
ap.add_argument('--rounds', type=int, default=7)
args = ap.parse_args()
B = args.batch


def make_pictures():
    try:
        from PIL import Image
    except ImportError:
        import _jpeg_ref as J
        cases = [c for c in J.load_golden(os.path.join(ROOT, 'tests', 'golden', 'jpeg_pil.npz'))[0] if c['kind'] == 'ok']
        big = max(cases, key=lambda c: len(c['data']))
        return [big['data']], f"PIL is not importable here: the fixture's largest file ({big['name']}, {len(big['data'])} bytes) under every name"
    out = []
    yy, xx = np.mgrid[0:375, 0:500].astype(np.float64)
    for k in range(args.pictures):
        rng = np.random.RandomState(k)
        chans = []
        for _ in range(3):
            a, b, c, d = rng.uniform(0.01, 0.06, 4)
            chans.append(128 + 70 * np.sin(a * xx + b * yy + rng.uniform(0, 6)) + 40 * np.cos(c * xx - d * yy) + rng.normal(0, 6, xx.shape))
        buf = io.BytesIO()
        Image.fromarray(np.clip(np.stack(chans, axis=-1), 0, 255).astype(np.uint8), 'RGB').save(buf, 'JPEG', quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out, (f'{args.pictures} pictures of 375 x 500, 4:2:0, quality 90, written by PIL (smooth picture + noise of sigma 6) under '
                 f'{args.files} names')


def entry_bytes(rb, k):
    o, n = int(rb.offsets[k]), 3 * int(rb.heights[k]) * int(rb.widths[k])
    return rb.data[o:o + n]


def epoch_rate(ld, epoch):
    """one epoch through the loader, the consumer only waiting -> fed images per second"""
    ld.set_epoch(epoch)
    torch.cuda.synchronize()
    t = time.perf_counter()
    n = 0
    for rb, y in ld:
        n += len(rb)
    torch.cuda.synchronize()
    assert n == len(ld) * B
    return n / (time.perf_counter() - t)


with tempfile.TemporaryDirectory() as root:
    pictures, what = make_pictures()
    for k in range(args.files):
        d = os.path.join(root, f'class{k % 8}')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f'{k:05d}.jpg'), 'wb') as f:
            f.write(pictures[k % len(pictures)])
    ds = A.ImageFolder(root)
    arms = {}
    for name, once in (('once', True), ('each', False)):
        dec = A.JpegDecoder(threads=args.threads, fallback=None)
        arms[name] = (A.FolderLoader(ds, B, dec, train=True, seed=0, aug_repeats=args.repeats, decode_once=once), dec)
    ld = arms['once'][0]
    distinct = [len(set(part.tolist())) for part, _ in ld.batches(0)]

    # the two arms feed the same bytes: one epoch of both, entry by entry
    for (ra, ya), (rb, yb) in zip(arms['once'][0], arms['each'][0]):
        torch.cuda.synchronize()
        assert len(ra) == len(rb) == B and torch.equal(ya, yb)
        assert np.array_equal(ra.heights, rb.heights) and np.array_equal(ra.widths, rb.widths)
        assert len(set(rb.offsets.tolist())) == B > len(set(ra.offsets.tolist()))
        for k in range(B):
            assert torch.equal(entry_bytes(ra, k), entry_bytes(rb, k)), f'entry {k} differs between the arms'
    counted = {name: (dec.decoded, len(l) * B) for name, (l, dec) in arms.items()}

    res = {'once': [], 'each': []}
    for r in range(args.rounds + 1):
        order = ('once', 'each') if r % 2 == 0 else ('each', 'once')
        row = {name: epoch_rate(arms[name][0], r) for name in order}
        if r:                                    # round 0 warms both arms up
            for name, v in row.items():
                res[name].append(v)

print(f'# aug-repeats A/B: {what}')
print(f'repeats {args.repeats}, one rank, batch {B}, {len(ld)} batches per epoch ({len(ld) * B} fed images), {min(distinct)} .. {max(distinct)} '
      f'distinct files per batch; {args.threads} decoder threads; {args.rounds} rounds after one warm-up, arms alternating, '
      'median (min .. max)')
print(f'checked first: every entry of every batch of one epoch is byte-equal between the arms; files decoded for that epoch: '
      f'{counted["once"][0]} (decode-once) against {counted["each"][0]} (per-entry) for {counted["once"][1]} fed images')
for name, label in (('once', '(a) decode-once'), ('each', '(b) per-entry  ')):
    v = res[name]
    print(f'{label}: {statistics.median(v):.0f} fed img/s ({min(v):.0f} .. {max(v):.0f})')
print(f'decode-once / per-entry, medians: {statistics.median(res["once"]) / statistics.median(res["each"]):.2f} x')
