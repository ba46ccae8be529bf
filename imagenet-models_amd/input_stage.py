"""The order of the training input stage: what happens to a loader's batch between the loader and the engine, in one place.

    crop -> (aug_splits with auto_augment inside | auto_augment) -> (collate_mixup with random_erasing | random_erasing)
         -> normalise + mixup_fn -> engine

Every piece is optional; an InputStage without any hands the batch through (the engine normalises a uint8 batch itself).

Default order (mixup_fn / random_erasing): normalise -> erase -> mixup -> engine, all in fp32.  random_erasing is an
imagenet_models_amd.RandomErasing (for a uint8 batch the erase pass IS the normalisation, ga_input_erase, so the batch is passed over
once), mixup_fn an imagenet_models_amd.Mixup (or a FastCollateMixup, which on an fp32 batch is timm's Mixup in modes 'elem' / 'pair'
as well).  This is timm's PrefetchLoader erase followed by the --no-prefetcher mixup_fn (MAP/train.py:614-626,643-646): a
combination timm itself never runs -- the erase boxes of both partners are blended into each other and the mixture is never
quantised.  It stays the default because every committed number was taken with it.
collate_mixup (opt-in): an imagenet_models_amd.FastCollateMixup -- the order every reference recipe runs (prefetcher on,
MAP/train.py:383): mixup / cutmix on the uint8 batch at collate time, each blended value rounded back to uint8, then the
normalisation, then random_erasing LAST on the mixed image -- one HIP pass (ga_input_collate).  It needs a uint8 batch, takes the
stage's random_erasing into the fused pass, and excludes mixup_fn.
auto_augment (opt-in): an imagenet_models_amd.RandAugment -- timm's --aa rand-..., which timm applies to the cropped uint8 image
ahead of fast_collate: it runs FIRST, on the uint8 batch (ga_rand_augment), and hands its uint8 result to whichever of the above is
configured.  It needs a uint8 batch.
crop (opt-in): an imagenet_models_amd.RandomResizedCrop -- the stage then takes a RaggedBatch of DECODED images
(imagenet_models_amd.pack_images, JpegDecoder) instead of a tensor: the crop, the resize and the flip run first (ga_resize_crop) and
their uint8 batch goes on exactly as a loader's uint8 batch does.
aug_splits (opt-in): an imagenet_models_amd.AugSplits -- timm's --aug-splits S: the b cropped uint8 samples become the split-major
S b batch (split 0 the crop itself, the others auto_augment applied to it with draws of their own; auto_augment then runs INSIDE
this piece, once, on the S b batch) and the labels are repeated S times; a random_erasing with num_splits = S then leaves split 0
alone.  It needs a uint8 batch and excludes mixup_fn / collate_mixup, as the reference does."""
import torch

from .resize_crop import RaggedBatch


class InputStage:
    def __init__(self, crop=None, auto_augment=None, collate_mixup=None, random_erasing=None, mixup_fn=None, aug_splits=None):
        if mixup_fn is not None and collate_mixup is not None:
            raise ValueError('TrainStep: mixup_fn (mix the normalised fp32 batch) and collate_mixup (mix the uint8 batch at collate '
                             'time) are two orders of the same augmentation: pass one of them')
        if aug_splits is not None:
            if mixup_fn is not None or collate_mixup is not None:
                raise ValueError('TrainStep: aug_splits cannot be combined with mixup_fn / collate_mixup (the reference asserts the '
                                 'same under its prefetcher, and the JSD loss needs class indices)')
            ns = getattr(random_erasing, 'num_splits', 0) if random_erasing is not None else 0
            if ns not in (0, aug_splits.num_splits):
                raise ValueError(f'TrainStep: random_erasing.num_splits = {ns} does not match aug_splits ({aug_splits.num_splits} splits): '
                                 f'0 (erase every split) or {aug_splits.num_splits} (keep the clean split)')
        self.aug_splits = aug_splits
        self.crop, self.auto_augment, self.collate_mixup = crop, auto_augment, collate_mixup
        self.random_erasing, self.mixup_fn = random_erasing, mixup_fn
        # what a loader has to yield: 'ragged' (a RaggedBatch: the crop makes the uint8 batch), 'uint8' (the first piece works on
        # bytes) or 'any' (a uint8 batch, normalised on the way, or a normalised fp32 one)
        bytes_first = auto_augment is not None or collate_mixup is not None or aug_splits is not None
        self.takes = 'ragged' if crop is not None else 'uint8' if bytes_first else 'any'

    def check(self, x):
        """the batch is what `takes` says; needs no device"""
        if isinstance(x, RaggedBatch) != (self.takes == 'ragged'):
            raise TypeError('TrainStep(crop=...) takes a RaggedBatch of decoded images, and a RaggedBatch needs TrainStep(crop=...): '
                            f'got {type(x).__name__} with crop {"set" if self.crop is not None else "None"}')
        if self.takes == 'uint8' and x.dtype != torch.uint8:
            if self.aug_splits is not None:
                raise TypeError(f'TrainStep(aug_splits=...) replicates the uint8 batch of the loader, got {x.dtype}')
            if self.auto_augment is not None:
                raise TypeError(f'TrainStep(auto_augment=...) augments the uint8 batch of the loader, got {x.dtype}')
            raise TypeError(f'TrainStep(collate_mixup=...) mixes the uint8 batch of the loader, got {x.dtype}')

    def __call__(self, x, target, engine):
        """(a loader's batch, its int64 labels, the training engine) -> (the engine's input, the target of the loss)"""
        self.check(x)
        if self.crop is not None:
            x = self.crop(x)
        if self.aug_splits is not None:
            x, target = self.aug_splits(x, target, self.auto_augment)
        elif self.auto_augment is not None:
            x = self.auto_augment(x)
        if self.collate_mixup is not None:
            x, target = self.collate_mixup(x, target, self.random_erasing, *engine.input_stats())
        elif self.random_erasing is not None:
            x = self.random_erasing(x, *engine.input_stats())
        if self.mixup_fn is not None:
            # a uint8 batch (PrefetchLoader layout) is normalised on the device FIRST: Mixup blends normalised pixels, and a
            # float tensor coming back from it would make the engine skip the normalisation
            x, target = self.mixup_fn(engine.normalize_u8(x), target)
        return x, target
