"""TEST INFRASTRUCTURE (CPU): independent restatements the RandomErasing tests compare the product against.

  * sample_boxes: timm.data.random_erasing.RandomErasing's box sampler in plain Python, written from its published algorithm
    (per sample: random() > probability skips; count; up to 10 attempts of uniform area / log-uniform aspect / rounded h, w /
    randint top, left).  timm is a third-party dependency that is NOT vendored in the reference and not installed here: parity
    of this restatement with timm itself is UNPINNED, as for oracle/mixup_oracle.py; the tests pin the product sampler against
    THIS restatement and against the closed-form properties of the boxes.
  * philox4x32_10 / normals: numpy Philox4x32-10 (checked against the Random123 known-answer vectors in the CPU tests) and
    Box-Muller in float64, in the counter layout documented in include/gaext.h (ga_input_erase).
  * erase: the whole pass on the CPU -- boxes applied in order (the later box wins), fills in float64.

Nothing here imports the product module."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MODES = {'const': 0, 'rand': 1, 'pixel': 2}


def sample_boxes(rng, B, H, W, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1,
                 max_count=None, num_splits=0):
    """-> ([(sample, top, left, h, w)] in erase order, [count drawn for the sample of each box])"""
    max_aspect = max_aspect or 1 / min_aspect
    max_count = max_count or min_count
    lo, hi = math.log(min_aspect), math.log(max_aspect)
    boxes, counts = [], []
    start = B // num_splits if num_splits > 1 else 0
    for i in range(start, B):
        if rng.random() > probability:
            continue
        count = min_count if min_count == max_count else rng.randint(min_count, max_count)
        for _ in range(count):
            for _ in range(10):
                target = rng.uniform(min_area, max_area) * (H * W) / count
                aspect = math.exp(rng.uniform(lo, hi))
                h = int(round(math.sqrt(target * aspect)))
                w = int(round(math.sqrt(target / aspect)))
                if w < W and h < H:
                    top = rng.randint(0, H - h)
                    left = rng.randint(0, W - w)
                    boxes.append((i, top, left, h, w))
                    counts.append(count)
                    break
    return boxes, counts


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words / key words: uint64 arrays (or ints) holding 32-bit values -> the four 32-bit outputs, uint64 arrays"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(v, dtype=np.uint64)) & np.uint64(MASK) for v in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def normals(q, offset, stream, seed):
    """float64 (4, len(q)): the four normals of counter (q, offset, stream) under key seed
    counter = (q[31:0], q[63:32], offset[31:0], offset[62:32] | stream << 31), key = (seed[31:0], seed[63:32]);
    u_k = ((r_k >> 9) + 0.5) * 2^-23;  n0, n1 = R(u0) cos / sin(2 pi u1);  n2, n3 = R(u2) cos / sin(2 pi u3);  R = sqrt(-2 ln u)"""
    q = np.atleast_1d(np.asarray(q, dtype=np.uint64))
    offset, seed = int(offset), int(seed) & 0xFFFFFFFFFFFFFFFF
    assert 0 <= offset < 1 << 63
    r = philox4x32_10(q & np.uint64(MASK), q >> np.uint64(32), offset & MASK, ((offset >> 32) & 0x7FFFFFFF) | (int(stream) << 31),
                      seed & MASK, seed >> 32)
    u = [((v >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for v in r]
    out = np.empty((4, q.size), dtype=np.float64)
    for k in range(2):
        rad = np.sqrt(-2.0 * np.log(u[2 * k]))
        out[2 * k] = rad * np.cos(2.0 * np.pi * u[2 * k + 1])
        out[2 * k + 1] = rad * np.sin(2.0 * np.pi * u[2 * k + 1])
    return out


def pixel_noise(idx, offset, seed):
    """float64 normals of 'pixel' mode at the flat element indices idx: call q = idx >> 2, output lane idx & 3"""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    n = normals(idx >> np.uint64(2), offset, 0, seed)
    return n[(idx & np.uint64(3)).astype(np.int64), np.arange(idx.size)]


def box_colour(b, j, c, max_count, CH, offset, seed):
    """float64 colour of 'rand' mode for box slot j of sample b, channel c: call q = (b*max_count + j)*CH + c, output lane 0"""
    return float(normals([(b * max_count + j) * CH + c], offset, 1, seed)[0, 0])


def normalize_u8(x8, mean, std):
    """what timm's PrefetchLoader does (fp32): x.float().sub_(mean).div_(std), mean / std in 0..255 units per channel"""
    m = np.asarray(mean, dtype=np.float32).reshape(1, -1, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(1, -1, 1, 1)
    return (x8.astype(np.float32) - m) / s


def erase(x, boxes, max_count, mode, seed, offset):
    """x: float32 (B, C, H, W) numpy (already normalised) -> (float64 erased copy, bool mask of the erased elements).
    boxes: [(sample, top, left, h, w)] in erase order; the slot of a box is its position among its sample's boxes."""
    B, C, H, W = x.shape
    out = x.astype(np.float64)
    mask = np.zeros(x.shape, dtype=bool)
    mode = MODES[mode] if isinstance(mode, str) else mode
    flat = np.arange(x.size, dtype=np.uint64).reshape(x.shape)
    used = {}
    for b, top, left, h, w in boxes:
        j = used.get(b, 0)
        used[b] = j + 1
        assert j < max_count
        sl = (b, slice(None), slice(top, top + h), slice(left, left + w))
        mask[sl] = True
        if mode == 0:
            out[sl] = 0.0
        elif mode == 1:
            for c in range(C):
                out[b, c, top:top + h, left:left + w] = box_colour(b, j, c, max_count, C, offset, seed)
        else:
            out[sl] = pixel_noise(flat[sl], offset, seed).reshape(out[sl].shape)
    return out, mask
