"""numpy restatement of the RandAugment ops of ga_rand_augment (include/gaext.h), written from the semantics PIL's C code has for
the calls timm's auto_augment.py makes (Image.transform / Image.rotate, ImageOps.autocontrast / equalize / invert / posterize /
solarize, Image.point, ImageEnhance.Color / Contrast / Brightness / Sharpness).  Images are uint8 [3][H][W]; every op returns a
new array.  tests/golden/randaug_pil.npz (tools/gen_golden_randaug.py) holds PIL's own outputs: the gate is equality."""
import math

import numpy as np

NONE, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE = range(12)
NEAREST, BILINEAR, BICUBIC = 0, 2, 3
FILL = (124, 116, 104)

ROW = np.dtype([('kind', '<i4'), ('interp', '<i4'), ('iarg', '<i4'), ('farg', '<f4'), ('m', '<f8', (6,))])
assert ROW.itemsize == 64


def row(kind=NONE, interp=0, iarg=0, farg=0.0, m=(1, 0, 0, 0, 1, 0)):
    r = np.zeros((), dtype=ROW)
    r['kind'], r['interp'], r['iarg'], r['farg'], r['m'] = kind, interp, iarg, farg, m
    return r


# ---- matrices, formed on the host ------------------------------------------------------------------
def shear_x(f):
    return (1.0, float(f), 0.0, 0.0, 1.0, 0.0)


def shear_y(f):
    return (1.0, 0.0, 0.0, float(f), 1.0, 0.0)


def translate_x_rel(pct, W):
    return (1.0, 0.0, pct * W, 0.0, 1.0, 0.0)


def translate_y_rel(pct, H):
    return (1.0, 0.0, 0.0, 0.0, 1.0, pct * H)


def rotate_matrix(deg, W, H):
    """Image.rotate's matrix about the image centre (no expand, no translate)"""
    ang = -math.radians(deg % 360.0)
    m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    a, b, c, d, e, f = m
    m[2] = a * -cx + b * -cy + c
    m[5] = d * -cx + e * -cy + f
    m[2] += cx
    m[5] += cy
    return tuple(m)


# ---- pixel ops ---------------------------------------------------------------------------------------
def gray(a):
    r, g, b = (a[c].astype(np.int64) for c in range(3))
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def blend(d, a, f):
    """d + f * (a - d): the product and the sum separately rounded in fp32; <= 0 -> 0, >= 255 -> 255, else truncated"""
    f = np.float32(f)
    d = np.asarray(d).astype(np.float32)
    a = np.asarray(a).astype(np.float32)
    t = (f * (a - d)).astype(np.float32)
    v = (d + t).astype(np.float32)
    out = np.where(v <= 0, np.float32(0), np.where(v >= 255, np.float32(255), np.trunc(v)))
    return out.astype(np.uint8)


def smooth(a):
    """ImageFilter.SMOOTH: 3x3 (1,1,1,1,5,1,1,1,1) / 13, the border row and column copied"""
    out = a.copy()
    H, W = a.shape[-2:]
    if H < 3 or W < 3:
        return out
    f = a.astype(np.float32)
    s = np.zeros(a.shape[:-2] + (H - 2, W - 2), dtype=np.float32)
    for dy in range(3):
        for dx in range(3):
            s += f[..., dy:dy + H - 2, dx:dx + W - 2] * np.float32(5 if (dy, dx) == (1, 1) else 1)
    v = (s / np.float32(13)).astype(np.float32) + np.float32(0.5)
    v = np.where(v <= 0, np.float32(0), np.where(v >= 255, np.float32(255), np.trunc(v)))
    out[..., 1:-1, 1:-1] = v.astype(np.uint8)
    return out


def _hist(ch):
    return np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    lut = [min(255, max(0, int(i * scale + offset))) for i in range(256)]
    return np.array(lut, dtype=np.uint8)


def equalize_lut(h):
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def _floor(v):
    return np.floor(v).astype(np.int64)


def _fix(v):
    """PIL's 16.16 fixed point: floor(v * 65536 + 0.5)"""
    return int(math.floor(float(v) * 65536.0 + 0.5))


def _nearest_index(m, H, W):
    """source (y, x) of every output pixel under PIL's NEAREST affine, -1 outside.  PIL does not take the double path here:
    an axis-aligned matrix (m1 == m3 == 0) steps the coordinate by REPEATED double additions and truncates; every other
    matrix runs in 16.16 fixed point"""
    m0, m1, m2, m3, m4, m5 = (float(v) for v in m)
    if m1 == 0 and m3 == 0:
        xs, ys = np.empty(W, dtype=np.int64), np.empty(H, dtype=np.int64)
        for tab, n, o, step, size in ((xs, W, m2 + m0 * 0.5, m0, W), (ys, H, m5 + m4 * 0.5, m4, H)):
            for k in range(n):
                i = -1 if o < 0.0 else int(o)
                tab[k] = i if 0 <= i < size else -1
                o += step
        return np.broadcast_to(ys[:, None], (H, W)), np.broadcast_to(xs[None, :], (H, W))
    a0, a1, a3, a4 = _fix(m0), _fix(m1), _fix(m3), _fix(m4)
    a2, a5 = _fix(m2 + m0 * 0.5 + m1 * 0.5), _fix(m5 + m3 * 0.5 + m4 * 0.5)
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    xx = (a2 + a1 * y + a0 * x) >> 16
    yy = (a5 + a4 * y + a3 * x) >> 16
    return np.where((yy >= 0) & (yy < H), yy, -1), np.where((xx >= 0) & (xx < W), xx, -1)


def affine(a, m, interp, fill=FILL):
    C, H, W = a.shape
    if interp == NEAREST:
        yy, xx = _nearest_index(m, H, W)
        inside = (yy >= 0) & (xx >= 0)
        out = np.empty_like(a)
        for c in range(C):
            out[c] = np.where(inside, a[c][np.maximum(yy, 0), np.maximum(xx, 0)], np.uint8(fill[c]))
        return out
    m0, m1, m2, m3, m4, m5 = (np.float64(v) for v in m)
    xs = np.arange(W, dtype=np.float64)[None, :] + 0.5
    ys = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = (m0 * xs + m1 * ys) + m2
    yin = (m3 * xs + m4 * ys) + m5
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.empty_like(a)
    xi = np.where(inside, xin, 0.0)
    yi = np.where(inside, yin, 0.0)
    xp, yp = xi - 0.5, yi - 0.5
    x0, y0 = _floor(xp), _floor(yp)
    dx, dy = xp - x0, yp - y0

    def cx(i):
        return np.clip(i, 0, W - 1)

    def cy(i):
        return np.clip(i, 0, H - 1)

    for c in range(C):
        f = a[c].astype(np.float64)
        if interp == BILINEAR:
            rows = []
            for j in (0, 1):
                v1, v2 = f[cy(y0 + j), cx(x0)], f[cy(y0 + j), cx(x0 + 1)]
                rows.append(v1 + (v2 - v1) * dx)
            v = rows[0] + (rows[1] - rows[0]) * dy
        elif interp == BICUBIC:
            def cubic(v1, v2, v3, v4, d):
                p1 = v2
                p2 = -v1 + v3
                p3 = 2 * (v1 - v2) + v3 - v4
                p4 = -v1 + v2 - v3 + v4
                return p1 + d * (p2 + d * (p3 + d * p4))
            rows = [cubic(*(f[cy(y0 + j), cx(x0 + i)] for i in (-1, 0, 1, 2)), dx) for j in (-1, 0, 1, 2)]
            v = cubic(*rows, dy)
        else:
            raise ValueError(f'interpolation code {interp}')
        v = np.where(v <= 0, 0.0, np.where(v >= 255, 255.0, np.trunc(v)))
        out[c] = np.where(inside, v.astype(np.uint8), np.uint8(fill[c]))
    return out


def apply_op(a, r, fill=FILL):
    """one table row on one uint8 [3][H][W] image"""
    kind, interp, iarg, farg = int(r['kind']), int(r['interp']), int(r['iarg']), np.float32(r['farg'])
    if kind == AUTOCONTRAST:
        return np.stack([autocontrast_lut(_hist(a[c]))[a[c]] for c in range(3)])
    if kind == EQUALIZE:
        return np.stack([equalize_lut(_hist(a[c]))[a[c]] for c in range(3)])
    if kind == INVERT:
        return 255 - a
    if kind == POSTERIZE:
        if iarg >= 8:
            return a.copy()
        mask = ~((1 << (8 - max(iarg, 0))) - 1) & 255
        return a & np.uint8(mask)
    if kind == SOLARIZE:
        return np.where(a.astype(np.int32) < iarg, a, 255 - a).astype(np.uint8)
    if kind == SOLARIZE_ADD:
        return np.where(a < 128, np.minimum(255, a.astype(np.int32) + iarg), a).astype(np.uint8)
    if kind == COLOR:
        return blend(gray(a)[None], a, farg)
    if kind == CONTRAST:
        g = gray(a)
        mean = int(int(g.sum()) / float(g.size) + 0.5)
        return blend(mean, a, farg)
    if kind == BRIGHTNESS:
        return blend(0, a, farg)
    if kind == SHARPNESS:
        return blend(smooth(a), a, farg)
    if kind == AFFINE:
        return affine(a, r['m'], interp, fill)
    return a.copy()                      # none, and every unknown kind


def rand_augment(x, table, fill=FILL):
    """x uint8 [B][3][H][W], table ROW [B][n_layers] -> the augmented batch: layer l+1 reads the whole output of layer l"""
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        a = x[b]
        for r in table[b]:
            a = apply_op(a, r, fill)
        out[b] = a
    return out


def check_table(table):
    t = np.asarray(table)
    return bool(((t['kind'] >= 0) & (t['kind'] <= AFFINE)).all() and np.isin(t['interp'], (NEAREST, BILINEAR, BICUBIC)).all())
