#!/usr/bin/env python3
"""Writes tests/golden/resize_crop_pil.npz: small decoded sources, table rows and PIL's own outputs for ga_resize_crop, by the calls
timm and torchvision make: img.crop(box).resize((w, h), code) and transpose(FLIP_LEFT_RIGHT) for training, img.resize((w, h), code)
and the centre img.crop(...) for evaluation.  The restatement (tests/_resize_crop_ref.py) and, through it, the HIP kernels are gated
on equality with these bytes.

  python tools/gen_golden_resize_crop.py            (needs Pillow; the fixture was written with the version stored in it)
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _resize_crop_ref as R  # noqa: E402

SOURCES = ((37, 53), (64, 48), (9, 130), (300, 17), (16, 700), (96, 96))      # H x W
OUTPUTS = ((32, 32), (24, 40))                                                # OH x OW
KINDS = ('tl', 'tr', 'bl', 'br', 'full', '1x1', 'w=OW', 'h=OH')
EVAL_SIZE = 32


def box_of(kind, H, W, OH, OW):
    """(top, left, h, w) or None where the source is too small for the kind"""
    bh, bw = max(1, H * 2 // 3), max(1, W * 3 // 5)
    if kind == 'tl':
        return 0, 0, bh, bw
    if kind == 'tr':
        return 0, W - bw, bh, bw
    if kind == 'bl':
        return H - bh, 0, bh, bw
    if kind == 'br':
        return H - bh, W - bw, bh, bw
    if kind == 'full':
        return 0, 0, H, W
    if kind == '1x1':
        return H // 2, W // 3, 1, 1
    if kind == 'w=OW':
        return (H - bh) // 2, (W - OW) // 2, bh, OW if W >= OW else None
    if kind == 'h=OH':
        return (H - OH) // 2, (W - bw) // 2, OH if H >= OH else None, bw
    raise ValueError(kind)


def pil_row(img, r, OH, OW):
    """what PIL gives for one table row: crop (unless the box is the image), resize, flip, window"""
    im = Image.fromarray(img, 'RGB')
    top, left, h, w = int(r['top']), int(r['left']), int(r['h']), int(r['w'])
    if (top, left, h, w) != (0, 0, img.shape[0], img.shape[1]):
        im = im.crop((left, top, left + w, top + h))
    im = im.resize((int(r['vw']), int(r['vh'])), int(r['interp']))
    if int(r['flip']):
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    oy, ox = int(r['oy']), int(r['ox'])
    if (oy, ox, OH, OW) != (0, 0, int(r['vh']), int(r['vw'])):
        im = im.crop((ox, oy, ox + OW, oy + OH))
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def cases():
    """(source index, OH, OW, row, label)"""
    out, n = [], 0
    full = SOURCES.index((96, 96))
    for si, (H, W) in enumerate(SOURCES):
        for OH, OW in OUTPUTS:
            for interp in (R.BILINEAR, R.BICUBIC):
                if si == full:
                    kinds = KINDS                                        # every box kind, both filters, both output sizes
                else:
                    rot = [k for k in KINDS if k != 'full']
                    kinds = ('full', rot[n % len(rot)], rot[(n + 3) % len(rot)])
                for kind in kinds:
                    box = box_of(kind, H, W, OH, OW)
                    if None in box:
                        continue
                    flip = n % 2
                    n += 1
                    out.append((si, OH, OW, R.row(H, W, *box, OH, OW, 0, 0, interp, flip), f'{H}x{W}:{kind}:{OH}x{OW}:{interp}:flip{flip}'))
    for si, (H, W) in enumerate(SOURCES):                                # evaluation: non-zero oy / ox from the centre crop
        for pct in (0.875, 0.95):
            for interp in (R.BILINEAR, R.BICUBIC):
                r = R.eval_row(H, W, EVAL_SIZE, pct, interp)
                out.append((si, EVAL_SIZE, EVAL_SIZE, r, f'{H}x{W}:eval{pct}:{interp}'))
    return out


def main():
    srcs = [R.source(H, W, 20240930 + k) for k, (H, W) in enumerate(SOURCES)]
    cs = cases()
    rows = np.zeros(len(cs), dtype=R.ROW)
    which = np.zeros(len(cs), dtype=np.int32)
    shapes = np.zeros((len(cs), 2), dtype=np.int32)
    outs, labels, bad = [], [], 0
    for k, (si, OH, OW, r, label) in enumerate(cs):
        rows[k], which[k], shapes[k] = r, si, (OH, OW)
        want = pil_row(srcs[si], r, OH, OW)
        assert want.shape == (3, OH, OW), (label, want.shape)
        outs.append(want.reshape(-1))
        labels.append(label)
        got = R.apply_row(srcs[si], r, OH, OW)
        d = int((got != want).sum())
        if d:
            bad += 1
            print(f'restatement differs from PIL at {label}: {d} bytes')
    path = os.path.join(ROOT, 'tests', 'golden', 'resize_crop_pil.npz')
    arrays = {f'source_{k}': s for k, s in enumerate(srcs)}
    np.savez_compressed(path, rows=rows.view(np.uint8), which=which, shapes=shapes, outputs=np.concatenate(outs), labels=np.array(labels),
                        pil_version=np.array(PIL.__version__), **arrays)
    print(f'{path}: {len(cs)} cases, {os.path.getsize(path)} bytes, PIL {PIL.__version__}, {bad} cases differ from the restatement')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
