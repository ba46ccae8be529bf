"""numpy int64 restatement of ga_jpeg_reconstruct (include/gaext.h): libjpeg-turbo's default decode path from QUANTISED coefficients to
RGB bytes -- dequantise, the "islow" IDCT (columns, then rows), the crop of the chroma planes, the fancy 2 x 1 / 2 x 2 upsamplers with
libjpeg's replicating ones for planes of at most two columns, YCbCr -> RGB.  The coefficients come from the library's host entropy
stage (ga_jpeg_entropy_decode): tests/test_jpeg_ref_cpu.py holds the two together to PIL's own bytes (tests/golden/jpeg_pil.npz,
tools/gen_golden_jpeg.py); the GPU tests hold the kernels to this file and to the same bytes."""
import ctypes as C

import numpy as np

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
INFO_LEN = 24
ROW = np.dtype([('coef_off', '<i8'), ('dst_off', '<i8'), ('work_off', '<i8'), ('qt_off', '<i4'), ('width', '<i4'), ('height', '<i4'),
                ('ncomp', '<i4'), ('hs', '<i4'), ('vs', '<i4'), ('mcus_w', '<i4'), ('mcus_h', '<i4'), ('pad', '<i4', (2,))])
assert ROW.itemsize == 64


def _pass(v, s):
    """one 1-D pass over the LAST axis of an int64 (..., 8) array"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    h = 1 << (s - 1)
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([(o + h) >> s for o in out], axis=-1)


def idct_blocks(coef, qt):
    """coef: int16 (n, 64) natural order, qt: uint16 (64,) -> uint8 (n, 8, 8)"""
    x = (coef.astype(np.int64) * qt.astype(np.int64)[None, :]).reshape(-1, 8, 8)
    ws = _pass(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # columns first
    out = _pass(ws, 18)                                              # then rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def plane(coef, qt, bh, bw):
    """one component: coef int16 (bh * bw * 64,) -> uint8 (8 bh, 8 bw) over the MCU-padded grid"""
    b = idct_blocks(coef.reshape(bh * bw, 64), qt).reshape(bh, bw, 8, 8)
    return b.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p):
    """p: the CROPPED plane (ch, cw) -> (ch, 2 cw)"""
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(p, 2, axis=1)
    q = p.astype(np.int64)
    left = np.concatenate([q[:, :1], q[:, :-1]], axis=1)
    right = np.concatenate([q[:, 1:], q[:, -1:]], axis=1)
    out = np.empty((ch, 2 * cw), dtype=np.int64)
    out[:, 0::2] = (3 * q + left + 1) >> 2
    out[:, 1::2] = (3 * q + right + 2) >> 2
    return out.astype(np.uint8)


def upsample_h2v2(p):
    """p: the CROPPED plane (ch, cw) -> (2 ch, 2 cw)"""
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    q = p.astype(np.int64)
    up = np.concatenate([q[:1], q[:-1]], axis=0)
    down = np.concatenate([q[1:], q[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for v, other in ((0, up), (1, down)):
        cs = 3 * q + other
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        out[v::2, 0::2] = (3 * cs + left + 8) >> 4
        out[v::2, 1::2] = (3 * cs + right + 7) >> 4
    return out.astype(np.uint8)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def reconstruct(info, coef, qt):
    """info: int64 (24,) of ga_jpeg_probe, coef: the image's int16 coefficients, qt: uint16 (3, 64) -> uint8 (H, W, 3)"""
    W, H, ncomp, hs, vs = (int(info[k]) for k in range(5))
    planes = []
    for c in range(ncomp):
        bw, bh, at = int(info[11 + 4 * c]), int(info[12 + 4 * c]), int(info[21 + c])
        planes.append(plane(coef[at:at + bw * bh * 64], qt[c], bh, bw))
    y = planes[0][:H, :W]
    if ncomp == 1:
        return np.repeat(y[:, :, None], 3, axis=2)
    cw, ch = -(-W // hs), -(-H // vs)
    chroma = [p[:ch, :cw] for p in planes[1:]]
    if (hs, vs) == (2, 1):
        chroma = [upsample_h2v1(p) for p in chroma]
    elif (hs, vs) == (2, 2):
        chroma = [upsample_h2v2(p) for p in chroma]
    return ycc_to_rgb(y, chroma[0][:H, :W], chroma[1][:H, :W])


# ---- the library's host stage ------------------------------------------------------------------------------------------------------
def probe(lib, data):
    """-> (status, info int64 (24,))"""
    info = np.zeros(INFO_LEN, dtype=np.int64)
    return int(lib.ga_jpeg_probe(data, len(data), info.ctypes.data)), info


def entropy_decode(lib, data, guard=0, fill=0x5A5A):
    """probe + ga_jpeg_entropy_decode into buffers with `guard` BYTES of a known pattern on both sides -> (status, info, coef, qt,
    guards intact).  For a file that is not OK the buffers are sized for nothing"""
    st, info = probe(lib, data)
    n = int(info[5]) if st == OK else 0
    g2 = guard // 2
    cbuf = np.full(n + 2 * g2, fill, dtype=np.int16)
    qbuf = np.full(192 + 2 * g2, fill, dtype=np.uint16)
    st2 = int(lib.ga_jpeg_entropy_decode(data, len(data), cbuf.ctypes.data + 2 * g2, C.c_size_t(n), qbuf.ctypes.data + 2 * g2))
    intact = bool((cbuf[:g2] == fill).all() and (cbuf[g2 + n:] == fill).all() and (qbuf[:g2] == fill).all() and (qbuf[g2 + 192:] == fill).all())
    return st2 if st == OK else st, info, cbuf[g2:g2 + n], qbuf[g2:g2 + 192].reshape(3, 64), intact


def table_row(info, coef_off=0, dst_off=0, work_off=0, qt_off=0):
    r = np.zeros((), dtype=ROW)
    r['coef_off'], r['dst_off'], r['work_off'], r['qt_off'] = coef_off, dst_off, work_off, qt_off
    r['width'], r['height'], r['ncomp'], r['hs'], r['vs'], r['mcus_w'], r['mcus_h'] = (int(info[k]) for k in (0, 1, 2, 3, 4, 7, 8))
    return r


def load_golden(path):
    """tests/golden/jpeg_pil.npz -> list of dict(name, kind ('ok' | 'fallback' | 'refuse'), data (bytes), pixels (H, W, 3) or None)"""
    z = np.load(path)
    out = []
    for i, (name, kind) in enumerate(zip(z['names'].tolist(), z['kinds'].tolist())):
        pix = z[f'pix_{i}'] if f'pix_{i}' in z.files else None
        out.append(dict(name=name, kind=kind, data=z[f'jpg_{i}'].tobytes(), pixels=pix))
    return out, str(z['pil_version'])
