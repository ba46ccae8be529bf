"""Resize and crop of DECODED images on the device: the first step of every recipe's input stage, which timm runs on the host, per
image, with PIL -- RandomResizedCropAndInterpolation + RandomHorizontalFlip for training (GA/train.py:195-217 and MAP/train.py reach
them through create_loader), Resize(floor(img / crop_pct)) + CenterCrop for evaluation.  A loader's remaining job is to decode a JPEG
and hand over its bytes: pack_images() puts a list of decoded H x W x 3 arrays of any sizes into one device byte buffer (a
RaggedBatch), the boxes, the interpolation and the flips are drawn on the host into one 64-byte row per sample, and ga_resize_crop
applies the table with PIL's own integer arithmetic, byte for byte (include/gaext.h), writing the uint8 (B, 3, size, size) batch
that RandAugment, FastCollateMixup, RandomErasing and the normalisation take.

timm is not vendored in the reference and not installed: the draw algorithms are a restatement of its published code (parity with
timm itself is unpinned, as for mixup.py, random_erasing.py and rand_augment.py); the pixels are pinned to PIL by
tests/golden/resize_crop_pil.npz.  What is pinned of the draws is the order PER SAMPLE -- the crop attempts (each: the area, the
aspect ratio, and on acceptance the top and the left) from Python's `random`, then the interpolation under 'random', then the flip
from torch's generator as torchvision's RandomHorizontalFlip draws it.  The order ACROSS the samples of a batch is unpinned, as
timm's split of a batch over loader workers makes it: here sample 0 draws first."""
import math
import random

import numpy as np
import torch

from . import _lib, ops, staging

BILINEAR, BICUBIC = 2, 3          # PIL's resampling codes
_INTERP = {'bilinear': BILINEAR, 'bicubic': BICUBIC}

ROW = np.dtype([('src_off', '<i8'), ('src_h', '<i4'), ('src_w', '<i4'), ('top', '<i4'), ('left', '<i4'), ('h', '<i4'), ('w', '<i4'),
                ('vh', '<i4'), ('vw', '<i4'), ('oy', '<i4'), ('ox', '<i4'), ('interp', '<i4'), ('flip', '<i4'), ('pad', '<i4', (2,))])
assert ROW.itemsize == 64


def _interp_code(name, allow_random):
    if name == 'random' and allow_random:
        return None
    if name in _INTERP:
        return _INTERP[name]
    if name in ('lanczos', 'box', 'hamming', 'nearest'):
        raise ValueError(f"interpolation {name!r} is not built: ga_resize_crop restates PIL's bilinear and bicubic filters only "
                         "(the two every recipe of the reference uses)")
    raise ValueError(f"interpolation {name!r}: 'bilinear', 'bicubic'" + (" or 'random'" if allow_random else ''))


class RaggedBatch:
    """decoded images of any sizes in ONE device byte buffer: image b is uint8 [heights[b]][widths[b]][3] at data[offsets[b]:],
    rows without padding.  offsets / heights / widths are host arrays (the tables are drawn on the host)"""

    def __init__(self, data, offsets, heights, widths):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError('RaggedBatch: data is a 1-d uint8 tensor')
        self.data = data
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.heights = np.ascontiguousarray(heights, dtype=np.int32)
        self.widths = np.ascontiguousarray(widths, dtype=np.int32)
        if not (self.offsets.shape == self.heights.shape == self.widths.shape and self.offsets.ndim == 1):
            raise ValueError('RaggedBatch: offsets, heights and widths are 1-d arrays of one length')

    def __len__(self):
        return len(self.offsets)

    def size(self, dim=0):
        if dim != 0:
            raise IndexError('a RaggedBatch has a batch dimension only')
        return len(self)

    def take(self, index):
        """entry k of the result is entry index[k] of this one, over the SAME data: entries may repeat, and those that do share one
        region of the buffer (a file decoded once under several table rows)"""
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        return RaggedBatch(self.data, self.offsets[index], self.heights[index], self.widths[index])


_PACK = staging.Ring()


def pack_offsets(heights, widths):
    """every image starts on a 16-byte boundary -> (offsets int64, total bytes)"""
    sizes = (3 * np.asarray(heights, dtype=np.int64) * np.asarray(widths, dtype=np.int64) + 15) & ~np.int64(15)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(sizes) else np.zeros(0, dtype=np.int64)
    return offsets, int(sizes.sum())


def parse_hw(text):
    """'375x500' -> (375, 500): the nominal size of synthetic decoded images (--synthetic-source)"""
    try:
        h, w = (int(v) for v in text.lower().split('x'))
    except ValueError:
        raise ValueError(f'--synthetic-source {text!r}: HxW, two positive integers') from None
    if h < 2 or w < 2 or h * 1.5 >= 32768 or w * 1.5 >= 32768:
        raise ValueError(f'--synthetic-source {text!r}: H and W from 2 up to 21844')
    return h, w


def synthetic_ragged(batch, source, seed, device):
    """B random decoded images in one device buffer: heights and widths drawn once, within [0.5, 1.5] of the nominal size"""
    g = torch.Generator().manual_seed(seed)
    hs = torch.randint(max(1, source[0] // 2), source[0] * 3 // 2 + 1, (batch,), generator=g).tolist()
    ws = torch.randint(max(1, source[1] // 2), source[1] * 3 // 2 + 1, (batch,), generator=g).tolist()
    offsets, total = pack_offsets(hs, ws)
    data = torch.randint(0, 256, (total,), device=device, dtype=torch.uint8, generator=torch.Generator(device=device).manual_seed(seed))
    return RaggedBatch(data, offsets, hs, ws)


def pack_images(images, device='cuda'):
    """a list of decoded H x W x 3 uint8 arrays -> RaggedBatch on `device`, through pinned staging with a non_blocking copy.  This
    is the seam where a decoder plugs in: it may as well write its output straight into the pinned buffer"""
    arrs = []
    for k, a in enumerate(images):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise TypeError(f'pack_images: image {k} is {a.dtype} {a.shape}, expected uint8 (H, W, 3)')
        arrs.append(a)
    if not arrs:
        raise ValueError('pack_images: an empty list')
    heights, widths = [a.shape[0] for a in arrs], [a.shape[1] for a in arrs]
    offsets, total = pack_offsets(heights, widths)
    i, host = _PACK.slot(total)
    h = host.numpy()
    for a, o in zip(arrs, offsets):
        h[o:o + a.size] = a.reshape(-1)
    data = torch.empty(total, dtype=torch.uint8, device=device)
    data.copy_(host[:total], non_blocking=True)
    _PACK.sent(i)
    return RaggedBatch(data, offsets, heights, widths)


class _ResizeCrop:
    """what both transforms share: the host check of a table, its staging, the workspace and the launch"""

    def __init__(self, size):
        self.OH, self.OW = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if self.OH < 1 or self.OW < 1 or self.OW % 4:
            raise ValueError(f'output size {self.OH} x {self.OW}: the width must be a multiple of 4 (ga_resize_crop)')
        self.last = None                     # the table of the last call, for logging / tests
        self._ring, self._dev, self._out, self._work = staging.Ring(), None, None, None

    def check(self, table, src_bytes):
        _lib.check(_lib.load().ga_resize_crop_check_table(table.ctypes.data, len(table), self.OH, self.OW, int(src_bytes)),
                   'ga_resize_crop_check_table')

    def _apply(self, ragged, table):
        if not isinstance(ragged, RaggedBatch):
            raise TypeError(f'{type(self).__name__} takes a RaggedBatch of decoded images (pack_images), got {type(ragged).__name__}')
        if not ragged.data.is_cuda:
            raise RuntimeError(f'{type(self).__name__} runs on the HIP kernels only (no CPU fallback)')
        B, dev = len(ragged), ragged.data.device
        tab = np.ascontiguousarray(table, dtype=ROW)
        if tab.shape != (B,):
            raise ValueError(f'table of shape {tab.shape}, expected {(B,)}')
        self.check(tab, ragged.data.numel())
        need = int(_lib.load().ga_resize_crop_work_bytes(tab.ctypes.data, B, self.OH, self.OW))
        self._dev = staging.buffer(self._dev, (tab.nbytes,), torch.uint8, dev)
        self._out = staging.buffer(self._out, (B, 3, self.OH, self.OW), torch.uint8, dev)
        self._work = staging.workspace(self._work, need, dev)          # grows with the largest boxes seen
        self._ring.upload(tab, self._dev)
        self.last = tab
        ops.Plan(eager=True).resize_crop(ragged.data, self._dev, self._out, self._work, B, self.OH, self.OW)
        return self._out


class RandomResizedCrop(_ResizeCrop):
    """timm's RandomResizedCropAndInterpolation followed by RandomHorizontalFlip"""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), interpolation='random', hflip=0.5, rng=None, torch_gen=None):
        super().__init__(size)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        if not (0 < self.scale[0] <= self.scale[1] and 0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError(f'RandomResizedCrop: scale {scale} and ratio {ratio} are (low, high) pairs of positive numbers')
        self._interp = _interp_code(interpolation, allow_random=True)
        self.interpolation = interpolation
        self.hflip = float(hflip)
        self.rng = rng if rng is not None else random          # timm draws from Python's global generator ...
        self.torch_gen = torch_gen                              # ... torchvision's flip from torch's (None: the global one)

    def _box(self, H, W):
        """timm's get_params: (top, left, h, w)"""
        area = H * W
        for _ in range(10):
            target_area = self.rng.uniform(*self.scale) * area
            log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
            aspect_ratio = math.exp(self.rng.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if 1 <= w <= W and 1 <= h <= H:
                i = self.rng.randint(0, H - h)
                j = self.rng.randint(0, W - w)
                return i, j, h, w
        in_ratio = W / H                                        # fallback: the central crop, the ratio clamped
        if in_ratio < min(self.ratio):
            w = W
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = H
            w = int(round(h * max(self.ratio)))
        else:
            w, h = W, H
        return (H - h) // 2, (W - w) // 2, h, w

    def sample(self, heights, widths, offsets=None):
        """the table of one batch (host only): per sample the box, then the interpolation, then the flip"""
        tab = np.zeros(len(heights), dtype=ROW)
        for b, (H, W) in enumerate(zip(heights, widths)):
            r = tab[b]
            r['src_h'], r['src_w'] = H, W
            r['top'], r['left'], r['h'], r['w'] = self._box(int(H), int(W))
            r['vh'], r['vw'] = self.OH, self.OW
            r['interp'] = self.rng.choice((BILINEAR, BICUBIC)) if self._interp is None else self._interp
            r['flip'] = int(bool(torch.rand(1, generator=self.torch_gen) < self.hflip))
            if offsets is not None:
                r['src_off'] = offsets[b]
        return tab

    def __call__(self, ragged, table=None):
        """ragged: a RaggedBatch -> the uint8 (B, 3, size, size) batch, in a buffer this object owns and reuses.  table: a ROW (B,)
        table to apply instead of a drawn one (tests, replay)"""
        if table is None and isinstance(ragged, RaggedBatch):
            table = self.sample(ragged.heights, ragged.widths, ragged.offsets)
        return self._apply(ragged, table)


class ResizeCenterCrop(_ResizeCrop):
    """timm's evaluation transform: torchvision Resize(floor(size / crop_pct)) -- the short side; the long one int(s * long / short)
    -- and CenterCrop(size)"""

    def __init__(self, size, crop_pct=0.875, interpolation='bicubic'):
        super().__init__(size)
        if self.OH != self.OW:
            raise ValueError('ResizeCenterCrop: a square output (timm scales the short side to floor(size / crop_pct))')
        if not 0 < crop_pct <= 1:
            raise ValueError(f'ResizeCenterCrop: crop_pct {crop_pct} must be in (0, 1]: above 1 the centre crop would need padding, '
                             'which is not built')
        self.crop_pct = float(crop_pct)
        self._interp = _interp_code(interpolation, allow_random=False)
        self.interpolation = interpolation

    def rows(self, heights, widths, offsets=None):
        s = int(math.floor(self.OH / self.crop_pct))
        tab = np.zeros(len(heights), dtype=ROW)
        for b, (H, W) in enumerate(zip(heights, widths)):
            H, W = int(H), int(W)
            vh, vw = (int(s * H / W), s) if W <= H else (s, int(s * W / H))
            r = tab[b]
            r['src_h'], r['src_w'], r['h'], r['w'], r['vh'], r['vw'] = H, W, H, W, vh, vw
            r['oy'], r['ox'] = int(round((vh - self.OH) / 2.)), int(round((vw - self.OW) / 2.))
            r['interp'] = self._interp
            if offsets is not None:
                r['src_off'] = offsets[b]
        return tab

    def __call__(self, ragged, table=None):
        if table is None and isinstance(ragged, RaggedBatch):
            table = self.rows(ragged.heights, ragged.widths, ragged.offsets)
        return self._apply(ragged, table)
