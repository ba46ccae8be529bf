"""RandomErasing on the device for the training step (timm.data.random_erasing.RandomErasing as timm's PrefetchLoader runs it:
on the GPU, on the normalised batch, ahead of mixup_fn -- every MAP recipe ends its input pipeline with
`--remode pixel --reprob 0.25`, MAP/train_with_script.py; MAP/train.py:214-220,643-646).  The boxes are drawn on the host from
Python's `random` exactly in timm's order; the fill is one HIP pass fused with the uint8 normalisation (ga_input_erase), its
noise from the counter-based Philox4x32-10 / Box-Muller generator laid out in include/gaext.h.

timm draws the noise from torch's CUDA generator; this engine draws it from its own documented one, so runs are reproducible
from (seed, call number) alone and a test can restate every value.  timm is not vendored in the reference and not installed:
the sampler is a restatement of its published algorithm (parity with timm itself is unpinned, as for mixup.py)."""
import math
import random

import numpy as np
import torch

from . import ops, staging

_MODES = {'const': 0, 'rand': 1, 'pixel': 2}


class RandomErasing:
    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode='const', min_count=1,
                 max_count=None, num_splits=0, seed=0, rng=None):
        if mode not in _MODES:
            raise ValueError(f"RandomErasing mode {mode!r}: 'const', 'rand' or 'pixel'")
        self.probability, self.min_area, self.max_area = probability, min_area, max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.mode = mode
        self.min_count, self.max_count = min_count, max_count or min_count
        self.num_splits = num_splits
        self.seed = int(seed)
        self.offset = 0                      # Philox offset: one per call, fresh noise every step from one seed
        self.rng = rng if rng is not None else random      # timm draws from Python's global generator
        self.last_boxes = None               # [(sample, top, left, h, w)] of the last call, in drawing order, for logging / tests
        self._ring, self._dev, self._out = staging.Ring(), None, None

    def sample(self, B, H, W):
        """the erase boxes of one batch, drawn as timm draws them: [(sample, top, left, h, w)] in erase order"""
        boxes = []
        area = H * W
        batch_start = B // self.num_splits if self.num_splits > 1 else 0     # the first (clean) augmentation split is kept
        for i in range(batch_start, B):
            if self.rng.random() > self.probability:
                continue
            count = self.min_count if self.min_count == self.max_count else self.rng.randint(self.min_count, self.max_count)
            for _ in range(count):
                for _attempt in range(10):
                    target_area = self.rng.uniform(self.min_area, self.max_area) * area / count
                    aspect_ratio = math.exp(self.rng.uniform(*self.log_aspect_ratio))
                    h = int(round(math.sqrt(target_area * aspect_ratio)))
                    w = int(round(math.sqrt(target_area / aspect_ratio)))
                    if w < W and h < H:
                        top = self.rng.randint(0, H - h)
                        left = self.rng.randint(0, W - w)
                        boxes.append((i, top, left, h, w))
                        break
        return boxes

    def stage(self, x):
        """draw the boxes of one batch and stage their table on the device, for a launch the caller makes (the fused collate
        pass, mixup.FastCollateMixup) -> (device int32 (B, max_count, 4) table, max_count, mode code, seed, offset of THIS call);
        the offset is advanced: one per call, whoever launches"""
        B, _, H, W = x.shape
        boxes = self.sample(B, H, W)
        tab = np.zeros((B, self.max_count, 4), dtype=np.int32)
        used = [0] * B
        for i, top, left, h, w in boxes:
            tab[i, used[i]] = (top, left, h, w)
            used[i] += 1
        self._dev = staging.buffer(self._dev, tab.shape, torch.int32, x.device)
        self._ring.upload(tab, self._dev)
        offset = self.offset
        self.offset += 1
        self.last_boxes = boxes
        return self._dev, self.max_count, _MODES[self.mode], self.seed, offset

    def __call__(self, x, mean=None, std=None):
        """x: (B, C, H, W) uint8 (normalised with mean / std, 0..255 units, in the same pass) or fp32 (copied) on the device
        -> the erased fp32 batch, in a buffer this object owns and reuses; x itself is not modified"""
        x = staging.check_batch(x, 'RandomErasing', stats=(mean, std))
        dev, max_count, mode, seed, offset = self.stage(x)
        self._out = staging.buffer(self._out, x.shape, torch.float32, x.device)
        ops.Plan(eager=True).input_erase(x, self._out, dev, max_count, mode, seed, offset, mean, std)
        return self._out
