"""Augmentation splits of the training batch (timm's `--aug-splits S`: AugMixDataset + fast_collate, GA/train.py:559-561): every base
sample gets the primary transform (random-resized crop + flip) ONCE; split 0 is that crop unchanged (the "clean" split), each of the
splits 1 .. S - 1 the `--aa` transform applied to the same crop with draws of its own.  The S b images are laid out split-major, as
fast_collate lays them out: row i + j b is split j of base sample i, and target[i + j b] = y_i.  The model runs on S b rows; with
`--jsd-loss` the loss is timm's JsdCrossEntropy over the splits (ga_loss_jsd_fwd_bwd), without it the ordinary loss over all rows.

No kernel of its own: the batch is replicated into a buffer this object owns and RandAugment runs once on the S b batch with a table
whose split-0 rows are `none`.  Draw order: this piece owns no random stream.  The crop's draws come first, as RandomResizedCrop
makes them; then RandAugment.sample's draws for b (S - 1) samples, base sample by base sample and split 1, 2, ... within each: draw
d = i (S - 1) + (j - 1) lands in table row j b + i.  Nothing is drawn for split 0.  The order ACROSS samples is unpinned, as for
every other restatement of timm's host-side augmentation; so is parity with timm itself (timm is not vendored in the reference)."""
import numpy as np
import torch

from . import staging
from .rand_augment import ROW


class AugSplits:
    def __init__(self, num_splits):
        num_splits = int(num_splits)
        if num_splits < 2:
            raise ValueError(f'AugSplits: num_splits must be at least 2 (the clean split and one augmented), got {num_splits}')
        self.num_splits = num_splits
        self.last = None                     # the RandAugment table of the last call (None without auto_augment)
        self._rep, self._tgt = None, None

    def sample_table(self, rand_augment, b, H, W):
        """the RandAugment table of one batch of b base samples (host only): ROW (S b, n).  Consumes exactly the draws of
        rand_augment.sample(b (S - 1), H, W); draw i (S - 1) + (j - 1) is row j b + i; the split-0 rows are the all-`none` rows
        RandAugment.sample initialises"""
        S, n = self.num_splits, rand_augment.num_layers
        draws = rand_augment.sample(b * (S - 1), H, W)
        tab = np.zeros((S * b, n), dtype=ROW)
        tab['m'] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        tab[b:] = draws.reshape(b, S - 1, n).transpose(1, 0, 2).reshape((S - 1) * b, n)
        return tab

    def __call__(self, x, target, rand_augment=None):
        """x: uint8 (b, 3, H, W) on the device (the crop's batch or a loader's), target: int64 (b,) -> (the uint8 (S b, 3, H, W)
        split-major batch, the int64 (S b,) targets), both in buffers that are reused from step to step: the replicated batch
        and the targets in this object's, the augmented batch in rand_augment's.  rand_augment None: the splits are plain
        copies (the reference with --aa '')."""
        x = staging.check_batch(x, 'AugSplits', dtypes=(torch.uint8,), channels=3)
        S, (b, _, H, W) = self.num_splits, x.shape
        if target.dim() != 1 or target.shape[0] != b:
            raise ValueError(f'AugSplits: {tuple(target.shape)} targets for a batch of {b} base samples')
        self._rep = staging.buffer(self._rep, (S * b,) + tuple(x.shape[1:]), torch.uint8, x.device)
        self._rep.view(S, b, *x.shape[1:]).copy_(x.unsqueeze(0).expand(S, *x.shape))
        self._tgt = staging.buffer(self._tgt, (S * b,), torch.int64, x.device)
        self._tgt.view(S, b).copy_(target.to(x.device, non_blocking=True).unsqueeze(0).expand(S, b))
        if rand_augment is None:
            self.last = None
            return self._rep, self._tgt
        self.last = self.sample_table(rand_augment, b, H, W)
        return rand_augment(self._rep, table=self.last), self._tgt
