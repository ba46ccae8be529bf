#!/usr/bin/env python3
"""The JPEG decoder of the input stage (imagenet_models_amd.JpegDecoder: host entropy stage + ga_jpeg_reconstruct) measured on one
box, in alternating rounds, on B files of 375 x 500, 4:2:0, quality 90:

  (i)   the reconstruct launch alone (HIP events around --launches calls) against its byte floor: 2 B per coefficient read + 3 B per
        pixel written at the stream rate DESIGN.md 5 quotes.  The per-kernel split comes from ONE profiler run of --mode kernels:
          rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 tools/jpeg_decode_ab.py --mode kernels
  (ii)  the host entropy stage: images per second on one thread and on 16
  (iii) end to end, files' bytes -> RaggedBatch on the device: JpegDecoder(threads=16) against the same files decoded wholly by PIL on
        16 threads and packed by pack_images (the way to feed the seam without this decoder)

The files are made with PIL where it is importable (a smooth picture plus mild noise: pure noise would make every coefficient
non-zero, which no photograph does); otherwise the largest file of tests/golden/jpeg_pil.npz is used B times, and the report says so."""
import argparse
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import imagenet_models_amd as A  # noqa: E402
from imagenet_models_amd import _lib, jpeg as JP, ops  # noqa: E402

STREAM_TBS = 4.83          # the streaming pass at 1 GiB

ap = argparse.ArgumentParser()
ap.add_argument('-b', '--batch', type=int, default=256)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--launches', type=int, default=10)
ap.add_argument('--mode', default='ab', choices=['ab', 'kernels'])
args = ap.parse_args()
B = args.batch


def make_files():
    try:
        from PIL import Image
    except ImportError:
        import _jpeg_ref as J
        cases = [c for c in J.load_golden(os.path.join(ROOT, 'tests', 'golden', 'jpeg_pil.npz'))[0] if c['kind'] == 'ok']
        big = max(cases, key=lambda c: len(c['data']))
        return [big['data']] * B, f"PIL is not importable here: the fixture's largest file ({big['name']}, {len(big['data'])} bytes) {B} times", None
    files = []
    yy, xx = np.mgrid[0:375, 0:500].astype(np.float64)
    for k in range(B):
        rng = np.random.RandomState(k)
        chans = []
        for _ in range(3):
            a, b, c, d = rng.uniform(0.01, 0.06, 4)
            chans.append(128 + 70 * np.sin(a * xx + b * yy + rng.uniform(0, 6)) + 40 * np.cos(c * xx - d * yy) + rng.normal(0, 6, xx.shape))
        buf = io.BytesIO()
        Image.fromarray(np.clip(np.stack(chans, axis=-1), 0, 255).astype(np.uint8), 'RGB').save(buf, 'JPEG', quality=90, subsampling=2)
        files.append(buf.getvalue())
    return files, f'{B} files of 375 x 500, 4:2:0, quality 90, written by PIL (smooth picture + noise of sigma 6)', Image


files, what, Image = make_files()
lib = _lib.load()
infos = [JP.probe(f)[1] for f in files]
ncoef = int(sum(i[5] for i in infos))
npix = int(sum(i[0] * i[1] for i in infos))
file_bytes = sum(len(f) for f in files)
floor_us = (2 * ncoef + 3 * npix) / (STREAM_TBS * 1e12) * 1e6

# the staged operands of one batch, for (i): what JpegDecoder.decode uploads
dec = A.JpegDecoder(threads=16, fallback=None)
rb = dec.decode(files)
torch.cuda.synchronize()
tab = dec.last
coef_h = np.zeros(ncoef, dtype=np.int16)
qt_h = np.zeros(192 * B, dtype=np.uint16)
for j, f in enumerate(files):
    assert lib.ga_jpeg_entropy_decode(f, len(f), coef_h.ctypes.data + 2 * int(tab[j]['coef_off']), int(infos[j][5]), qt_h.ctypes.data + 384 * j) == 0
d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
d_coef = torch.from_numpy(coef_h).cuda()
d_qt = torch.from_numpy(qt_h.view(np.int16)).cuda()
d_work = torch.empty(ncoef, dtype=torch.uint8, device='cuda')
d_dst = torch.empty(rb.data.numel(), dtype=torch.uint8, device='cuda')
plan = ops.Plan(eager=False)
plan.jpeg_reconstruct(d_tab, B, d_coef, d_qt, d_work, d_dst)


def same_images(a, b):
    """two byte buffers of the batch's layout hold the same images (the alignment padding between them is nobody's)"""
    return all(torch.equal(a[o:o + 3 * h * w], b[o:o + 3 * h * w]) for o, h, w in zip(rb.offsets.tolist(), rb.heights.tolist(), rb.widths.tolist()))


def reconstruct_us():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.launches):
        plan.run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.launches


plan.run()
torch.cuda.synchronize()
assert same_images(d_dst, rb.data)
if args.mode == 'kernels':
    for _ in range(args.launches):
        plan.run()
    torch.cuda.synchronize()
    print(f'{args.launches + 1} reconstruct launches over {what}; byte floor {floor_us:.1f} us per launch')
    sys.exit(0)

scratch_c = np.zeros(max(int(i[5]) for i in infos), dtype=np.int16)
scratch_q = np.zeros(192, dtype=np.uint16)


def entropy_one(f):
    c = np.empty(scratch_c.size, dtype=np.int16) if pool_mode else scratch_c
    q = np.empty(192, dtype=np.uint16) if pool_mode else scratch_q
    return lib.ga_jpeg_entropy_decode(f, len(f), c.ctypes.data, c.size, q.ctypes.data)


def pil_one(f):
    return np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))


pool = ThreadPoolExecutor(16)
res = {k: [] for k in ('recon_us', 'entropy_1', 'entropy_16', 'e2e_device', 'e2e_pil', 'pil_decode_16')}
for r in range(args.rounds + 1):
    row = {}
    row['recon_us'] = reconstruct_us()
    pool_mode = False
    t = time.perf_counter()
    assert all(entropy_one(f) == 0 for f in files)
    row['entropy_1'] = B / (time.perf_counter() - t)
    pool_mode = True
    t = time.perf_counter()
    assert all(s == 0 for s in pool.map(entropy_one, files))
    row['entropy_16'] = B / (time.perf_counter() - t)
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = dec.decode(files)
    torch.cuda.synchronize()
    row['e2e_device'] = B / (time.perf_counter() - t)
    if Image is not None:
        t = time.perf_counter()
        arrs = list(pool.map(pil_one, files))
        row['pil_decode_16'] = B / (time.perf_counter() - t)
        ref = A.pack_images(arrs)
        torch.cuda.synchronize()
        row['e2e_pil'] = B / (time.perf_counter() - t)
        if r == 0:
            assert same_images(out.data, ref.data), 'the two paths disagree'
    if r:                                    # round 0 warms both paths up
        for k, v in row.items():
            res[k].append(v)


def med(k):
    v = res[k]
    return (statistics.median(v), min(v), max(v)) if v else None


print(f'# JPEG decode A/B: {what}')
print(f'{ncoef} coefficients ({2 * ncoef / 1e6:.1f} MB staged), {npix} pixels ({3 * npix / 1e6:.1f} MB written), files {file_bytes / 1e6:.1f} MB; '
      f'{args.rounds} rounds after one warm-up, median (min .. max)')
m = med('recon_us')
print(f'(i)   ga_jpeg_reconstruct: {m[0]:.1f} us ({m[1]:.1f} .. {m[2]:.1f}) per launch of {B} images; byte floor {floor_us:.1f} us at {STREAM_TBS} TB/s '
      f'-> {floor_us / m[0] * 100:.0f} % of the floor rate; {B / m[0] * 1e6 / 1e3:.0f} k img/s')
for k, label in (('entropy_1', '(ii)  host entropy stage, 1 thread'), ('entropy_16', '(ii)  host entropy stage, 16 threads'),
                 ('e2e_device', '(iii) end to end, JpegDecoder(threads=16)'), ('pil_decode_16', '      PIL decode alone, 16 threads'),
                 ('e2e_pil', '(iii) end to end, PIL on 16 threads + pack_images')):
    m = med(k)
    print(f'{label}: ' + (f'{m[0]:.0f} img/s ({m[1]:.0f} .. {m[2]:.0f})' if m else 'NOT MEASURED (PIL is not importable here)'))
if med('e2e_pil'):
    print(f'device path / PIL path, end to end: {med("e2e_device")[0] / med("e2e_pil")[0]:.2f} x')
