"""MI355X-native engine for the GA-ConvNeXt / GA / MAP ImageNet training hot path.

Python host code (timm-style registry, model containers, train/validate glue) over hand-written HIP kernels for
gfx950 reached through the C ABI in include/gaext.h.  There is no CPU or eager-PyTorch fallback: compute entry
points raise if csrc/libgaext.so is missing.
"""
from . import _lib  # noqa: F401
from . import ops  # noqa: F401

__version__ = '0.1.0'

from .registry import create_model, is_model, list_models, model_img_size, register_model  # noqa: E402,F401
from . import ga_convnext  # noqa: E402,F401  (registers the ga_convnext_* entry points)
from .ga_convnext import GA_ConvNeXt  # noqa: E402,F401
from . import ga_cswin  # noqa: E402,F401  (registers the ga_CSWin_* entry points)
from .ga_cswin import GA_CSWinTransformer  # noqa: E402,F401
from . import map_convnext  # noqa: E402,F401  (registers the map_convnext_* entry points)
from .map_convnext import MAP_ConvNeXt  # noqa: E402,F401
from . import map_vit  # noqa: E402,F401  (registers the map_vit_* entry points)
from .map_vit import MAP_ViT  # noqa: E402,F401
from . import map_pit  # noqa: E402,F401  (registers map_pit_s)
from . import convnext  # noqa: E402,F401  (registers the plain convnext_tiny / convnext_small of map_convnext.py)
from .convnext import ConvNeXt  # noqa: E402,F401
from .map_pit import MAP_PiT  # noqa: E402,F401
from . import pit  # noqa: E402,F401  (registers the baseline name pit_s)
from .pit import PiT  # noqa: E402,F401
from . import mobilenet  # noqa: E402,F401  (registers the extra names mobilenet_v1 / map_mobilenet_v1)
from .mobilenet import MobileNetV1  # noqa: E402,F401
from . import map_resnet  # noqa: E402,F401  (registers the repaired name map_resnet50)
from .map_resnet import MAP_ResNet  # noqa: E402,F401
from .loss import ga_loss, heads_topk, accuracy_from_topk, map_loss, heads_mean_topk  # noqa: E402,F401
from .optim import create_optimizer_v2, FusedSGD, FusedAdamW, FusedLamb, CosineLRScheduler  # noqa: E402,F401
from .optim import FusedAdam, FusedRMSprop, FusedLion, FusedLars, StepLRScheduler, optimizer_config  # noqa: E402,F401
from .mixup import FastCollateMixup, Mixup  # noqa: E402,F401
from .random_erasing import RandomErasing  # noqa: E402,F401
from .rand_augment import RandAugment  # noqa: E402,F401
from .aug_splits import AugSplits  # noqa: E402,F401
from .resize_crop import RaggedBatch, pack_images, parse_hw, synthetic_ragged, RandomResizedCrop, ResizeCenterCrop  # noqa: E402,F401
from .jpeg import JpegDecoder  # noqa: E402,F401
from .dataset import ImageFolder, FolderLoader, split_dir, evaluate_folder, repeat_aug_indices  # noqa: E402,F401
from .input_stage import InputStage  # noqa: E402,F401
from .trainer import TrainStep, distribute_bn, make_buckets  # noqa: E402,F401
from .comm import NativeComm  # noqa: E402,F401
from .checkpoint import save_checkpoint, load_checkpoint, ModelEma  # noqa: E402,F401
from .checkpoint import (read_checkpoint, resume_checkpoint, capture_train_state, restore_train_state,  # noqa: E402,F401
                         saved_initial_seed, CheckpointSaver, DeviceSnapshot)
