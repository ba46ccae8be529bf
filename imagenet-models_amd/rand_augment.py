"""RandAugment on the device for the training step (timm.data.auto_augment.rand_augment_transform as every recipe of the reference
asks for it: `--aa rand-mN-mstd0.5-inc1`, MAP/train_with_script.py:13-19).  timm runs it on the host, per image, with PIL, on the
cropped uint8 image ahead of fast_collate; here the ops and their arguments are drawn on the host in that order -- the op indices
from numpy's global generator, everything else from Python's `random` -- into one 64-byte row per (sample, layer), and
ga_rand_augment applies the table to the uint8 (B, 3, H, W) batch with PIL's own arithmetic, byte for byte (include/gaext.h).

timm is not vendored in the reference and not installed: the op list, the level functions and the draw order are a restatement of
its published algorithm (parity with timm itself is unpinned, as for mixup.py and random_erasing.py); the pixels are pinned to PIL
by tests/golden/randaug_pil.npz."""
import math
import random
import re

import numpy as np
import torch

from . import _lib, ops, staging

NONE, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE = range(12)
NEAREST, BILINEAR, BICUBIC = 0, 2, 3          # PIL's resampling codes
_INTERP = {'nearest': NEAREST, 'bilinear': BILINEAR, 'bicubic': BICUBIC}
_LEVEL_DENOM = 10.0

ROW = np.dtype([('kind', '<i4'), ('interp', '<i4'), ('iarg', '<i4'), ('farg', '<f4'), ('m', '<f8', (6,))])      # 64 bytes

# timm's _RAND_TRANSFORMS / _RAND_INCREASING_TRANSFORMS: the index np.random.choice draws
OPS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness',
       'Sharpness', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
_INCREASING = ('Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness', 'Sharpness')
_ENHANCE = {'Color': COLOR, 'Contrast': CONTRAST, 'Brightness': BRIGHTNESS, 'Sharpness': SHARPNESS}
_GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')


def parse_config(config_str):
    """'rand-m9-mstd0.5-inc1' -> dict(m, mstd, mmax, inc, n, p); anything this engine does not build is refused with a reason"""
    parts = config_str.split('-')
    if parts[0] != 'rand':
        raise ValueError(f"auto-augment config {config_str!r}: only timm's 'rand-...' (RandAugment) is built; 'augmix-...', "
                         "'original' and 'v0' policies are not")
    cfg = dict(m=10, mstd=0.0, mmax=10, inc=False, n=2, p=0.5)
    for c in parts[1:]:
        cs = re.split(r'(\d.*)', c)
        if len(cs) < 2:
            raise ValueError(f'auto-augment config {config_str!r}: section {c!r} has no value')
        key, val = cs[:2]
        if key == 'mstd':
            v = float(val)
            cfg['mstd'] = float('inf') if v > 100 else v          # > 100: the magnitude is uniform in [0, m]
        elif key == 'mmax':
            cfg['mmax'] = int(val)
        elif key == 'inc':
            cfg['inc'] = bool(int(val))
        elif key == 'm':
            cfg['m'] = int(val)
        elif key == 'n':
            cfg['n'] = int(val)
            if cfg['n'] < 1:
                raise ValueError(f'auto-augment config {config_str!r}: n (layers) must be at least 1')
        elif key == 'p':
            cfg['p'] = float(val)
        elif key == 'w':
            if int(val) != 0:
                raise ValueError(f'auto-augment config {config_str!r}: op weights (w{val}) are not built: the ops are drawn uniformly')
        elif key == 't':
            raise ValueError(f'auto-augment config {config_str!r}: a transform subset (t...) is not built: the 15 ops of rand-... are')
        else:
            raise ValueError(f'auto-augment config {config_str!r}: unknown section {c!r} (m, mstd, mmax, inc, n, p)')
    return cfg


def rotate_matrix(deg, W, H):
    """PIL Image.rotate's matrix about the centre (W/2, H/2): cos / sin rounded to 15 decimals, as PIL rounds them"""
    ang = -math.radians(deg % 360.0)
    a, b = round(math.cos(ang), 15), round(math.sin(ang), 15)
    d, e = round(-math.sin(ang), 15), round(math.cos(ang), 15)
    cx, cy = W / 2.0, H / 2.0
    return (a, b, (a * -cx + b * -cy + 0.0) + cx, d, e, (d * -cx + e * -cy + 0.0) + cy)


class RandAugment:
    def __init__(self, config_str, img_mean=(0.485, 0.456, 0.406), interpolation='random', rng=None, np_rng=None):
        self.config_str = config_str
        cfg = parse_config(config_str)
        self.magnitude, self.magnitude_std, self.magnitude_max = cfg['m'], cfg['mstd'], cfg['mmax']
        self.increasing, self.num_layers, self.prob = cfg['inc'], cfg['n'], cfg['p']
        if interpolation != 'random' and interpolation not in _INTERP:
            raise ValueError(f"RandAugment interpolation {interpolation!r}: 'random', 'bilinear', 'bicubic' or 'nearest'")
        self.interpolation = interpolation
        self.fill = tuple(min(255, round(255 * v)) for v in img_mean)          # timm's fillcolor
        self.rng = rng if rng is not None else random             # timm draws from Python's global generator ...
        self.np_rng = np_rng if np_rng is not None else np.random     # ... and the op indices from numpy's
        self.last = None                     # the table of the last call, for logging / tests
        self._ring, self._dev, self._work, self._out = staging.Ring(), None, None, None

    # -- level functions of a magnitude v in [0, mmax] (timm's _LEVEL_DENOM = 10) ----------------------
    def _negate(self, v):
        return -v if self.rng.random() > 0.5 else v

    def _level(self, name, v):
        """the argument of op `name` at magnitude v; draws the sign where the level is signed"""
        s = v / _LEVEL_DENOM
        if name == 'Rotate':
            return self._negate(s * 30.)
        if name in ('ShearX', 'ShearY'):
            return self._negate(s * 0.3)
        if name in ('TranslateXRel', 'TranslateYRel'):
            return self._negate(s * 0.45)
        if name in _ENHANCE:
            if self.increasing:
                return max(0.1, 1.0 + self._negate(s * 0.9))
            return s * 1.8 + 0.1
        if name == 'Posterize':
            return 4 - int(s * 4) if self.increasing else int(s * 4)
        if name == 'Solarize':
            return 256 - int(s * 256) if self.increasing else min(256, int(s * 256))
        if name == 'SolarizeAdd':
            return min(128, int(s * 110))
        return None                          # AutoContrast, Equalize, Invert

    def _row(self, row, name, H, W):
        """one applied op: magnitude, level (sign), interpolation -- drawn in that order"""
        v = self.magnitude
        if self.magnitude_std > 0:
            if self.magnitude_std == float('inf'):
                v = self.rng.uniform(0, v)
            else:
                v = self.rng.gauss(v, self.magnitude_std)
        v = max(0., min(v, self.magnitude_max))
        level = self._level(name, v)
        if name in _GEOMETRIC:
            interp = self.rng.choice((BILINEAR, BICUBIC)) if self.interpolation == 'random' else _INTERP[self.interpolation]
            m = {'Rotate': lambda: rotate_matrix(level, W, H),
                 'ShearX': lambda: (1.0, level, 0.0, 0.0, 1.0, 0.0), 'ShearY': lambda: (1.0, 0.0, 0.0, level, 1.0, 0.0),
                 'TranslateXRel': lambda: (1.0, 0.0, level * W, 0.0, 1.0, 0.0),
                 'TranslateYRel': lambda: (1.0, 0.0, 0.0, 0.0, 1.0, level * H)}[name]()
            row['kind'], row['interp'], row['m'] = AFFINE, interp, m
        elif name in _ENHANCE:
            row['kind'], row['farg'] = _ENHANCE[name], level
        elif name in ('Posterize', 'Solarize', 'SolarizeAdd'):
            row['kind'], row['iarg'] = {'Posterize': POSTERIZE, 'Solarize': SOLARIZE, 'SolarizeAdd': SOLARIZE_ADD}[name], level
        else:
            row['kind'] = {'AutoContrast': AUTOCONTRAST, 'Equalize': EQUALIZE, 'Invert': INVERT}[name]

    def sample(self, B, H, W):
        """the table of one batch (host only): ROW (B, n) -- per sample the n op indices from numpy, then per layer from `random`:
        the gate (random() > p: none, nothing more is drawn), the magnitude, the sign, the interpolation"""
        tab = np.zeros((B, self.num_layers), dtype=ROW)
        tab['m'] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        for b in range(B):
            idx = self.np_rng.choice(len(OPS), self.num_layers)
            for l in range(self.num_layers):
                if self.rng.random() > self.prob:
                    continue
                self._row(tab[b, l], OPS[int(idx[l])], H, W)
        return tab

    def stage(self, x, table=None):
        """draw the table of one batch (or take `table`), check it on the host and stage it on the device -> device uint8 table"""
        B, _, H, W = x.shape
        tab = self.sample(B, H, W) if table is None else np.ascontiguousarray(table, dtype=ROW)
        if tab.shape != (B, self.num_layers):
            raise ValueError(f'RandAugment table of shape {tab.shape}, expected {(B, self.num_layers)}')
        _lib.check(_lib.load().ga_rand_augment_check_table(tab.ctypes.data, tab.size), 'ga_rand_augment_check_table')
        self._dev = staging.buffer(self._dev, (tab.nbytes,), torch.uint8, x.device)
        self._ring.upload(tab, self._dev)
        self.last = tab
        return self._dev

    def __call__(self, x, table=None):
        """x: (B, 3, H, W) uint8 on the device -> the augmented uint8 batch, in a buffer this object owns and reuses; x itself is
        not modified.  table: a ROW (B, n) table to apply instead of a drawn one (tests, replay)"""
        x = staging.check_batch(x, 'RandAugment', dtypes=(torch.uint8,), channels=3)
        dev = self.stage(x, table)
        p = ops.Plan(eager=True)
        out = staging.buffer(self._out, x.shape, torch.uint8, x.device)
        if out is not self._out:             # another batch shape or device: the scratch follows it
            work = p.rand_augment_work_bytes(*x.shape, self.num_layers)
            self._out, self._work = out, torch.empty(work, dtype=torch.uint8, device=x.device)
        p.rand_augment(x, self._out, self._work, dev, self.num_layers, self.fill)
        return self._out
