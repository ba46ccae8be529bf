"""TEST INFRASTRUCTURE (CPU): independent restatement of the collate-time mixup order the fused input pass implements
(timm FastCollateMixup on the uint8 batch -> PrefetchLoader's normalisation -> RandomErasing last), in numpy / torch on the
CPU, written from the semantics stated in include/gaext.h (ga_input_collate) and imagenet_models_amd/mixup.py.

timm is a third-party dependency that is NOT vendored in the reference and not installed here: parity of this restatement with
timm itself is UNPINNED, as for oracle/mixup_oracle.py; the tests pin the product against THIS restatement.

  * sample_table: the per-sample table {kind, yl, yh, xl, xh, bits(l), bits(m), 0} of modes 'batch', 'elem', 'pair', drawn from a
    numpy RandomState in timm's order;
  * mix_u8 / mix_f32: the pixels -- the partner of sample i is B-1-i, everything reads the original batch; the uint8 blend is
    u8(rint(fl(fl(a*l) + fl(b*m)))) with three separately rounded fp32 operations;
  * dense_target: the smoothed dense target of a scalar lam (complement in double) or of a float32 lam vector (in fp32);
  * contraction_sensitive_lam: a lam at which a blend contracted into an FMA rounds some byte pair differently.

Nothing here imports the product module."""
import functools

import numpy as np
import torch

NONE, MIXUP, CUTMIX = 0, 1, 2


def _box(rng, H, W, lam, minmax, correct_lam):
    if minmax is not None:
        cut_h = rng.randint(int(H * minmax[0]), int(H * minmax[1]))
        cut_w = rng.randint(int(W * minmax[0]), int(W * minmax[1]))
        yl = rng.randint(0, H - cut_h)
        xl = rng.randint(0, W - cut_w)
        box = (yl, yl + cut_h, xl, xl + cut_w)
    else:
        ratio = np.sqrt(1 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy = rng.randint(0, H)
        cx = rng.randint(0, W)
        box = (int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H)),
               int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W)))
    if correct_lam or minmax is not None:
        lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
    return box, lam


def sample_table(rng, B, H, W, mode='batch', mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5,
                 correct_lam=True, enabled=True):
    """-> (int32 (B, 8) table, lam): lam is a python float in 'batch' mode, a float32 (B,) vector in 'elem' / 'pair'"""
    assert B % 2 == 0 and mode in ('batch', 'elem', 'pair')
    if cutmix_minmax is not None:
        cutmix_alpha = 1.0
    tab = np.zeros((B, 8), dtype=np.int32)
    both = mixup_alpha > 0.0 and cutmix_alpha > 0.0
    assert both or mixup_alpha > 0.0 or cutmix_alpha > 0.0
    if mode == 'batch':
        lam, cut = 1.0, False
        if enabled and rng.rand() < prob:
            if both:
                cut = rng.rand() < switch_prob
                lam = rng.beta(cutmix_alpha, cutmix_alpha) if cut else rng.beta(mixup_alpha, mixup_alpha)
            elif mixup_alpha > 0.0:
                lam = rng.beta(mixup_alpha, mixup_alpha)
            else:
                cut = True
                lam = rng.beta(cutmix_alpha, cutmix_alpha)
            lam = float(lam)
        if lam != 1.0:
            if cut:
                box, lam = _box(rng, H, W, lam, cutmix_minmax, correct_lam)
                tab[:, 0] = CUTMIX
                tab[:, 1:5] = box
            else:
                tab[:, 0] = MIXUP
        l = np.full(B, lam, dtype=np.float32)
        m = np.full(B, 1.0 - lam, dtype=np.float32)           # the complement in double, rounded to fp32 once
    else:
        n = B if mode == 'elem' else B // 2
        lam = np.ones(n, dtype=np.float32)
        cut = np.zeros(n, dtype=bool)
        if enabled:
            if both:
                cut = rng.rand(n) < switch_prob
                first = rng.beta(cutmix_alpha, cutmix_alpha, size=n)
                second = rng.beta(mixup_alpha, mixup_alpha, size=n)
                lam_mix = np.where(cut, first, second)
            elif mixup_alpha > 0.0:
                lam_mix = rng.beta(mixup_alpha, mixup_alpha, size=n)
            else:
                cut = np.ones(n, dtype=bool)
                lam_mix = rng.beta(cutmix_alpha, cutmix_alpha, size=n)
            lam = np.where(rng.rand(n) < prob, lam_mix.astype(np.float32), lam)
        for i in range(n):
            mixed = lam[i] < 1 if mode == 'pair' else lam[i] != 1
            if not mixed:
                continue
            rows = [i] if mode == 'elem' else [i, B - 1 - i]
            if cut[i]:
                box, lam[i] = _box(rng, H, W, lam[i], cutmix_minmax, correct_lam)
                tab[rows, 0] = CUTMIX
                tab[rows, 1:5] = box
            else:
                tab[rows, 0] = MIXUP
        if mode == 'pair':
            lam = np.concatenate((lam, lam[::-1]))
        l = lam.astype(np.float32)
        m = np.float32(1) - l                                  # subtracted in fp32
    tab[:, 5] = l.view(np.int32)
    tab[:, 6] = m.view(np.int32)
    return tab, lam


def table_lm(tab):
    """the float32 l and m columns of a table"""
    return np.ascontiguousarray(tab[:, 5]).view(np.float32), np.ascontiguousarray(tab[:, 6]).view(np.float32)


def blend_u8(a, b, l, m):
    """uint8 arrays a (own), b (partner) -> u8(rint(fl(fl(a*l) + fl(b*m)))): numpy rounds each float32 operation separately;
    np.rint is round-half-to-even"""
    p = a.astype(np.float32) * np.float32(l)
    q = b.astype(np.float32) * np.float32(m)
    return np.rint(p + q).astype(np.uint8)


def blend_u8_contracted(a, b, l, m):
    """the same blend with a*l + fl(b*m) contracted into one FMA: the exact product (8 x 24 bits, exact in float64) added to the
    rounded one in float64 and rounded ONCE to fp32"""
    q = (b.astype(np.float32) * np.float32(m)).astype(np.float64)
    s = a.astype(np.float64) * np.float64(np.float32(l)) + q
    return np.rint(s.astype(np.float32)).astype(np.uint8)


def _mix(x, tab, blend):
    B = x.shape[0]
    l, m = table_lm(tab)
    out = x.copy()
    for b in range(B):
        pb = B - 1 - b
        kind, yl, yh, xl, xh = (int(v) for v in tab[b, :5])
        if kind == MIXUP:
            out[b] = blend(x[b], x[pb], l[b], m[b])
        elif kind == CUTMIX:
            out[b, :, yl:yh, xl:xh] = x[pb, :, yl:yh, xl:xh]
        else:
            assert kind == NONE
    return out


def mix_u8(x8, tab):
    """x8: uint8 numpy (B, C, H, W) -> the mixed uint8 batch"""
    assert x8.dtype == np.uint8
    return _mix(x8, tab, blend_u8)


def mix_f32(x, tab):
    """x: float32 numpy (B, C, H, W) -> the mixed float32 batch: fl(fl(x_i*l) + fl(x_j*m)), no rounding to integers"""
    assert x.dtype == np.float32
    return _mix(x, tab, lambda a, b, l, m: a * np.float32(l) + b * np.float32(m))


def dense_target(target, num_classes, lam, smoothing):
    """target: int64 torch (B,); lam: python float (complement in double) or float32 numpy (B,) (complement in fp32)"""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    t = target.long().view(-1, 1)
    y1 = torch.full((t.size(0), num_classes), off, dtype=torch.float32).scatter_(1, t, on)
    y2 = torch.full((t.size(0), num_classes), off, dtype=torch.float32).scatter_(1, t.flip(0), on)
    if isinstance(lam, np.ndarray):
        lt = torch.from_numpy(np.ascontiguousarray(lam, dtype=np.float32)).view(-1, 1)
        return y1 * lt + y2 * (1 - lt)
    return y1 * lam + y2 * (1.0 - lam)


def all_byte_pairs():
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    return a, b


def contraction_count(l, m=None):
    """the number of the 65 536 byte pairs that a contracted blend rounds differently at (l, m = 1 - l in fp32)"""
    l = np.float32(l)
    m = np.float32(1) - l if m is None else np.float32(m)
    a, b = all_byte_pairs()
    return int((blend_u8(a, b, l, m) != blend_u8_contracted(a, b, l, m)).sum())


@functools.lru_cache(maxsize=None)
def contraction_sensitive_lam(seed=0, alpha=0.8, tries=4000):
    """the first float32 lam among seeded Beta(alpha, alpha) draws at which contraction changes at least one byte pair
    -> (lam, count); (None, 0) if none is found"""
    rng = np.random.RandomState(seed)
    for _ in range(tries):
        l = np.float32(rng.beta(alpha, alpha))
        n = contraction_count(l)
        if n:
            return float(l), n
    return None, 0
