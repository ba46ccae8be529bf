#!/usr/bin/env python3
"""Writes tests/golden/randaug_pil.npz: inputs, arguments and PIL's own outputs for every RandAugment op of ga_rand_augment, by the
calls timm's auto_augment.py makes (Image.transform / Image.rotate, ImageOps.*, Image.point, ImageEnhance.*).  The restatement
(tests/_rand_augment_ref.py) and, through it, the HIP kernels are gated on equality with these bytes.

  python tools/gen_golden_randaug.py            (needs Pillow; the fixture was written with the version stored in it)
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _rand_augment_ref as R  # noqa: E402

H, W = 48, 64
_PIL_INTERP = {R.NEAREST: Image.NEAREST, R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC}


def images():
    rng = np.random.RandomState(20240611)
    rand = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
    low = (rand // 3 + 40).astype(np.uint8)                      # low contrast: bins 40..125
    const = rand.copy()
    const[1] = 77                                                # a constant channel: one occupied bin
    step0 = np.full((3, H, W), 200, dtype=np.uint8)              # equalize: sum(h) - h[last] < 255 -> step == 0
    idx = rng.choice(H * W, 150, replace=False)
    for c in range(3):
        step0[c].reshape(-1)[idx] = rng.randint(0, 200, 150)
    return {'rand': rand, 'low': low, 'const': const, 'step0': step0}


def to_pil(a):
    return Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)), 'RGB')


def from_pil(im):
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def pil_op(img, name, arg, interp):
    """the PIL call timm makes for op `name`"""
    kw = dict(resample=_PIL_INTERP[interp], fillcolor=R.FILL)
    if name == 'none':
        return img.copy()
    if name == 'autocontrast':
        return ImageOps.autocontrast(img)
    if name == 'equalize':
        return ImageOps.equalize(img)
    if name == 'invert':
        return ImageOps.invert(img)
    if name == 'posterize':
        return img if arg >= 8 else ImageOps.posterize(img, arg)
    if name == 'solarize':
        return ImageOps.solarize(img, arg)
    if name == 'solarize_add':
        lut = [min(255, i + arg) if i < 128 else i for i in range(256)]
        return img.point(lut + lut + lut)
    if name == 'color':
        return ImageEnhance.Color(img).enhance(arg)
    if name == 'contrast':
        return ImageEnhance.Contrast(img).enhance(arg)
    if name == 'brightness':
        return ImageEnhance.Brightness(img).enhance(arg)
    if name == 'sharpness':
        return ImageEnhance.Sharpness(img).enhance(arg)
    if name == 'rotate':
        return img.rotate(arg, **kw)
    if name == 'affine':
        return img.transform(img.size, Image.AFFINE, arg, **kw)
    raise ValueError(name)


def row_of(name, arg, interp):
    """the table row that asks ga_rand_augment for the same thing"""
    if name in ('none', 'autocontrast', 'equalize', 'invert'):
        return R.row(getattr(R, name.upper()))
    if name in ('posterize', 'solarize', 'solarize_add'):
        return R.row(getattr(R, name.upper()), iarg=arg)
    if name in ('color', 'contrast', 'brightness', 'sharpness'):
        return R.row(getattr(R, name.upper()), farg=arg)
    if name == 'rotate':
        return R.row(R.AFFINE, interp=interp, m=R.rotate_matrix(arg, W, H))
    return R.row(R.AFFINE, interp=interp, m=arg)


def cases():
    out = [('rand', 'none', 0, 0)]
    for img in ('rand', 'low', 'const', 'step0'):
        out += [(img, 'autocontrast', 0, 0), (img, 'equalize', 0, 0)]
    out.append(('rand', 'invert', 0, 0))
    out += [('rand', 'posterize', b, 0) for b in (0, 2, 4, 8)]
    out += [('rand', 'solarize', t, 0) for t in (0, 128, 256)]
    out += [('rand', 'solarize_add', a, 0) for a in (0, 55, 110)]
    for name in ('color', 'contrast', 'brightness', 'sharpness'):
        out += [('rand', name, f, 0) for f in (0.1, 0.55, 1.9)]
    out.append(('low', 'contrast', 1.45, 0))
    geo = [('affine', R.shear_x(0.3)), ('affine', R.shear_x(-0.3)), ('affine', R.shear_x(0.135)),
           ('affine', R.shear_y(0.3)), ('affine', R.shear_y(-0.21)),
           ('affine', (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)),                         # the identity
           ('affine', R.translate_x_rel(0.125, W)),                            # an integer translation: 8 pixels
           ('affine', R.translate_x_rel(1.5, W)),                              # leaves only fill
           ('affine', R.translate_x_rel(-0.45, W)), ('affine', R.translate_y_rel(0.45, H)), ('affine', R.translate_y_rel(-0.2025, H)),
           ('affine', (1.0, 1.0, -1.0, 0.0, 1.0, 0.0)),                        # xin = x + y: exactly 0 and exactly W
           ('rotate', 0.0), ('rotate', 27.0), ('rotate', -13.5), ('rotate', 30.0)]
    for name, arg in geo:
        out += [('rand', name, arg, interp) for interp in (R.NEAREST, R.BILINEAR, R.BICUBIC)]
    return out


def main():
    imgs = images()
    names = sorted(imgs)
    cs = cases()
    rows = np.zeros(len(cs), dtype=R.ROW)
    which = np.zeros(len(cs), dtype=np.int32)
    outs = np.zeros((len(cs), 3, H, W), dtype=np.uint8)
    labels = []
    for k, (img, name, arg, interp) in enumerate(cs):
        rows[k] = row_of(name, arg, interp)
        which[k] = names.index(img)
        outs[k] = from_pil(pil_op(to_pil(imgs[img]), name, arg, interp))
        labels.append(f'{img}:{name}:{arg}:{interp}')
    path = os.path.join(ROOT, 'tests', 'golden', 'randaug_pil.npz')
    np.savez_compressed(path, images=np.stack([imgs[n] for n in names]), image_names=np.array(names), rows=rows.view(np.uint8),
                        which=which, outputs=outs, labels=np.array(labels), fill=np.array(R.FILL, dtype=np.uint8),
                        pil_version=np.array(PIL.__version__))
    bad = 0
    for k in range(len(cs)):
        got = R.apply_op(imgs[names[which[k]]], rows[k])
        d = int((got != outs[k]).sum())
        if d:
            bad += 1
            print(f'restatement differs from PIL at {labels[k]}: {d} bytes')
    print(f'{path}: {len(cs)} cases, {os.path.getsize(path)} bytes, PIL {PIL.__version__}, {bad} cases differ from the restatement')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
