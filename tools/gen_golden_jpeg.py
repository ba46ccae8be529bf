#!/usr/bin/env python3
"""Writes tests/golden/jpeg_pil.npz: small JPEG files as PIL writes them and PIL's own decode of each, Image.open(f).convert('RGB') --
the bytes ga_jpeg_entropy_decode + ga_jpeg_reconstruct (and tests/_jpeg_ref.py) are gated on.  Data only: the byte strings and the
pixels.  Images are a smooth ramp plus noise, so that small and saturating coefficients both occur.

  python tools/gen_golden_jpeg.py               (needs Pillow with libjpeg-turbo; the fixture was written with the version stored in it)
  python tools/gen_golden_jpeg.py --dump DIR    write the fixture's files into DIR instead (input of csrc/jpeg_host_fuzz)
"""
import argparse
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'jpeg_pil.npz')

SIZES = ((8, 8), (16, 16), (17, 33), (9, 17), (48, 31), (37, 53), (64, 80), (1, 1), (2, 3), (1, 40),      # H x W
         (40, 1), (5, 4), (3, 6))                                                                      # chroma planes <= 2 wide
SUBSAMPLING = {0: '444', 1: '422', 2: '420'}


def picture(h, w, seed, grey=False):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 255 * (xx + yy) / max(h + w - 2, 1)], axis=-1)
    img = np.clip(ramp + rng.normal(0, 48, (h, w, 3)), 0, 255).astype(np.uint8)
    return img[:, :, 0] if grey else img


def encode(arr, mode='RGB', **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def cases():
    """(name, kind, bytes): kind 'ok' the device path decodes it, 'fallback' a valid file it hands on, 'refuse' one with no RGB meaning
    here (no pixels stored)"""
    out = []
    seed = 0
    for (h, w) in SIZES:
        for sub, tag in SUBSAMPLING.items():
            for q in (10, 95):
                seed += 1
                out.append((f'{h}x{w}_{tag}_q{q}', 'ok', encode(picture(h, w, seed), quality=q, subsampling=sub)))
    out.append(('37x53_420_q1', 'ok', encode(picture(37, 53, 901), quality=1, subsampling=2)))
    out.append(('48x31_422_q100', 'ok', encode(picture(48, 31, 902), quality=100, subsampling=1)))
    out.append(('64x80_420_q75_optimize', 'ok', encode(picture(64, 80, 903), quality=75, subsampling=2, optimize=True)))
    out.append(('37x53_420_q75_restart3', 'ok', encode(picture(37, 53, 904), quality=75, subsampling=2, restart_marker_blocks=3)))
    for k, ((h, w), q) in enumerate((((17, 33), 50), ((64, 80), 90), ((1, 1), 75))):
        out.append((f'{h}x{w}_grey_q{q}', 'ok', encode(picture(h, w, 910 + k, grey=True), 'L', quality=q)))
    out.append(('37x53_420_q75_progressive', 'fallback', encode(picture(37, 53, 920), quality=75, subsampling=2, progressive=True)))
    cmyk = np.concatenate([picture(16, 16, 921), picture(16, 16, 922)[:, :, :1]], axis=2)
    out.append(('16x16_cmyk_q75', 'refuse', encode(cmyk, 'CMYK', quality=75)))
    return out


def main():
    import PIL
    ap = argparse.ArgumentParser()
    ap.add_argument('--dump', default='', metavar='DIR')
    args = ap.parse_args()
    cs = cases()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for name, _, data in cs:
            open(os.path.join(args.dump, name + '.jpg'), 'wb').write(data)
        print(f'{len(cs)} files -> {args.dump}')
        return
    arrays = dict(names=np.array([c[0] for c in cs]), kinds=np.array([c[1] for c in cs]), pil_version=np.array(PIL.__version__))
    for i, (name, kind, data) in enumerate(cs):
        arrays[f'jpg_{i}'] = np.frombuffer(data, dtype=np.uint8)
        if kind != 'refuse':
            arrays[f'pix_{i}'] = decode(data)
    np.savez_compressed(PATH, **arrays)
    print(f'{len(cs)} files, {os.path.getsize(PATH)} bytes -> {PATH} (PIL {PIL.__version__})')


if __name__ == '__main__':
    main()
