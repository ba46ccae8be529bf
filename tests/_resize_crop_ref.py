"""numpy restatement of ga_resize_crop (include/gaext.h): PIL's ImagingResample for 8-bit channels -- coefficients in Python doubles,
22-bit fixed point, the horizontal pass rounded to uint8 ahead of the vertical one -- on a crop box, then the window and the flip;
plus, in plain Python, the two draw algorithms of imagenet_models_amd.resize_crop (timm's RandomResizedCropAndInterpolation.get_params
followed by the interpolation choice and torchvision's flip; torchvision's Resize + CenterCrop as timm's eval transform builds them).
Sources are uint8 [H][W][3] as a decoder hands them over; outputs are uint8 [3][OH][OW].  tests/golden/resize_crop_pil.npz
(tools/gen_golden_resize_crop.py) holds PIL's own outputs: the gate is equality."""
import math

import numpy as np

BILINEAR, BICUBIC = 2, 3
PRECISION_BITS = 22

ROW = np.dtype([('src_off', '<i8'), ('src_h', '<i4'), ('src_w', '<i4'), ('top', '<i4'), ('left', '<i4'), ('h', '<i4'), ('w', '<i4'),
                ('vh', '<i4'), ('vw', '<i4'), ('oy', '<i4'), ('ox', '<i4'), ('interp', '<i4'), ('flip', '<i4'), ('pad', '<i4', (2,))])
assert ROW.itemsize == 64


def row(src_h, src_w, top, left, h, w, vh, vw, oy=0, ox=0, interp=BICUBIC, flip=0, src_off=0):
    r = np.zeros((), dtype=ROW)
    for k, v in dict(src_off=src_off, src_h=src_h, src_w=src_w, top=top, left=left, h=h, w=w, vh=vh, vw=vw, oy=oy, ox=ox, interp=interp,
                     flip=flip).items():
        r[k] = v
    return r


# ---- coefficients ----------------------------------------------------------------------------------
def _bilinear(t):
    t = -t if t < 0.0 else t
    return 1.0 - t if t < 1.0 else 0.0


def _bicubic(t):
    a = -0.5
    t = -t if t < 0.0 else t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def ksize(in_size, out_size, interp):
    """PIL's row pitch of the coefficient table: the most taps an output index can have"""
    fs = max(in_size / out_size, 1.0)
    return int(math.ceil((1.0 if interp == BILINEAR else 2.0) * fs)) * 2 + 1


def coeffs(in_size, out_size, interp):
    """one axis -> bounds int32 [out][2] (xmin, count), integer coefficients int32 [out][ksize], zero past count"""
    f, S = (_bilinear, 1.0) if interp == BILINEAR else (_bicubic, 2.0)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = S * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ks), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5))
        w = [f((x - center + 0.5) * ss) for x in range(xmin, xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for k, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, k] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = xmin, xmax - xmin
    return bounds, kk


def _pass(img, out_size, interp):
    """resample axis 0 of uint8 [n][...] to out_size: int32 accumulation from 2^21, arithmetic shift, clamp"""
    bounds, kk = coeffs(img.shape[0], out_size, interp)
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    wide = img.astype(np.int32)
    for xx in range(out_size):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.tensordot(kk[xx, :n], wide[x0:x0 + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, vh, vw, interp):
    """uint8 [h][w][3] -> [vh][vw][3]: the horizontal pass, rounded to uint8, then the vertical pass"""
    t = _pass(np.ascontiguousarray(img.transpose(1, 0, 2)), vw, interp).transpose(1, 0, 2)
    return _pass(np.ascontiguousarray(t), vh, interp)


def apply_row(img, r, OH, OW):
    """one table row on its source image uint8 [H][W][3] -> uint8 [3][OH][OW]"""
    top, left, h, w = int(r['top']), int(r['left']), int(r['h']), int(r['w'])
    v = resize(img[top:top + h, left:left + w], int(r['vh']), int(r['vw']), int(r['interp']))
    if int(r['flip']):
        v = v[:, ::-1]
    oy, ox = int(r['oy']), int(r['ox'])
    return np.ascontiguousarray(v[oy:oy + OH, ox:ox + OW].transpose(2, 0, 1))


def resize_crop(images, table, OH, OW):
    """a list of sources and its table -> uint8 [B][3][OH][OW]"""
    return np.stack([apply_row(img, r, OH, OW) for img, r in zip(images, table)])


# ---- the draws, in plain Python --------------------------------------------------------------------
def sample_train_row(H, W, size, scale, ratio, interpolation, hflip, rng, torch_rand):
    """timm's RandomResizedCropAndInterpolation.get_params, then the interpolation, then the flip -> (top, left, h, w, interp, flip).
    rng: a random.Random; torch_rand: a callable returning the next torch.rand(1) as a float"""
    area = H * W
    box = None
    for _ in range(10):
        target_area = rng.uniform(*scale) * area
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        aspect = math.exp(rng.uniform(*log_ratio))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if w <= W and h <= H and w >= 1 and h >= 1:
            i = rng.randint(0, H - h)
            j = rng.randint(0, W - w)
            box = (i, j, h, w)
            break
    if box is None:
        in_ratio = W / H
        if in_ratio < min(ratio):
            w = W
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = H
            w = int(round(h * max(ratio)))
        else:
            w, h = W, H
        box = ((H - h) // 2, (W - w) // 2, h, w)
    if interpolation == 'random':
        interp = rng.choice((BILINEAR, BICUBIC))
    else:
        interp = {'bilinear': BILINEAR, 'bicubic': BICUBIC}[interpolation]
    flip = 1 if torch_rand() < hflip else 0
    return box + (interp, flip)


def train_table(heights, widths, size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), interpolation='random', hflip=0.5, rng=None,
                torch_rand=None, offsets=None):
    tab = np.zeros(len(heights), dtype=ROW)
    for b, (H, W) in enumerate(zip(heights, widths)):
        top, left, h, w, interp, flip = sample_train_row(int(H), int(W), size, scale, ratio, interpolation, hflip, rng, torch_rand)
        tab[b] = row(H, W, top, left, h, w, size, size, 0, 0, interp, flip, 0 if offsets is None else offsets[b])
    return tab


def eval_row(H, W, size, crop_pct, interp):
    """torchvision Resize(floor(size / crop_pct)) (the short side; the long one truncated) + CenterCrop(size)"""
    s = int(math.floor(size / crop_pct))
    if W <= H:
        vw, vh = s, int(s * H / W)
    else:
        vh, vw = s, int(s * W / H)
    oy = int(round((vh - size) / 2.))
    ox = int(round((vw - size) / 2.))
    return row(H, W, 0, 0, H, W, vh, vw, oy, ox, interp, 0)


def eval_table(heights, widths, size, crop_pct=0.875, interpolation='bicubic', offsets=None):
    tab = np.zeros(len(heights), dtype=ROW)
    for b, (H, W) in enumerate(zip(heights, widths)):
        tab[b] = eval_row(int(H), int(W), size, crop_pct, {'bilinear': BILINEAR, 'bicubic': BICUBIC}[interpolation])
        tab[b]['src_off'] = 0 if offsets is None else offsets[b]
    return tab


# ---- the fixture and sources for tests -----------------------------------------------------------------------------
def source(H, W, seed):
    """uint8 [H][W][3]: a smooth ramp, uniform noise and hard 0 / 255 blocks, so that bicubic overshoot reaches both clamps"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.empty((H, W, 3), dtype=np.uint8)
    ramp = (yy * 255.0 / max(H - 1, 1) * 0.5 + xx * 255.0 / max(W - 1, 1) * 0.5)
    for c in range(3):
        img[..., c] = np.clip(ramp * (0.6 + 0.2 * c) + 10 * c, 0, 255).astype(np.uint8)
    noise = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    third = (xx * 3 // max(W, 1)) + (yy * 3 // max(H, 1))
    img = np.where((third % 3 == 1)[..., None], noise, img)
    by, bx = max(1, H // 7), max(1, W // 7)
    blocks = (((yy // by) + (xx // bx)) % 2 * 255).astype(np.uint8)
    img = np.where((third % 3 == 2)[..., None], blocks[..., None], img)
    return np.ascontiguousarray(img.astype(np.uint8))


def load_golden(path):
    """tests/golden/resize_crop_pil.npz -> dict(sources, rows, which, shapes, outputs (one array per case), labels)"""
    z = np.load(path)
    rows = z['rows'].view(ROW).reshape(-1)
    shapes = z['shapes']
    ends = np.cumsum(3 * shapes[:, 0].astype(np.int64) * shapes[:, 1])
    outs = [z['outputs'][e - 3 * h * w:e].reshape(3, h, w) for e, (h, w) in zip(ends, shapes)]
    n_src = len([k for k in z.files if k.startswith('source_')])
    return dict(sources=[z[f'source_{k}'] for k in range(n_src)], rows=rows, which=z['which'], shapes=shapes, outputs=outs,
                labels=[str(s) for s in z['labels']])
