#!/usr/bin/env python3
"""ImageNet training script for the GA models on the MI355X-native engine -- the timm-style surface of the
reference's GA/train.py (argument names, loss, step, logging line), with the hot path on libgaext HIP kernels.

Differences from the reference, all deliberate: bf16 instead of fp16+GradScaler (`--amp`), a
`--synthetic` loader (metric runs use synthetic 3x224x224) beside the folder loader, gradients reduced once per
optimizer step, and `--device cpu` is refused: the product path has no CPU implementation (the CPU baseline is the
oracle timed by bench.py).

  python train.py --synthetic --model ga_convnext_tiny_768 -b 256 --epochs 1 --steps-per-epoch 50 --GA_lam -0.8
  python train.py /data/imagenet --model map_resnet50 -b 256 -j 8 --aa rand-m9-mstd0.5-inc1 --collate-mixup --reprob 0.25
      an image folder (DIR/train/<class>/*.jpg, DIR/validation/...): baseline JPEGs are entropy-decoded on -j host threads and
      rebuilt, cropped, resized and augmented on the device
  python train.py /data/imagenet ... --aug-repeats 3 -tb 1024 --cooldown-epochs 10    timm's repeated-augmentation order, each distinct
      file of a batch decoded once; --print-config prints what the flags resolve to and exits before a model is created
  python train.py /data/imagenet ... -b 64 --aug-splits 3 --jsd-loss --aa rand-m9-mstd0.5-inc1 --reprob 0.25 --resplit    every image
      cropped once and run as a clean and two RandAugment splits (192 rows per step), timm's JsdCrossEntropy per head
  python train.py /data/imagenet ... --output out --recovery-interval 500      out/last.pth.tar, checkpoint-N, model_best, and a recovery
      file every 500 optimizer steps, written behind the step
  python train.py /data/imagenet ... --output out --resume out/last.pth.tar    continue exactly: weights, optimizer, EMA, every random
      stream and the loader position (a recovery file resumes inside its epoch; the reference restarts at the next one)
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py --synthetic ...
"""
import argparse
import contextlib
import json
import logging
import os
import random
import sys
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imagenet_models_amd as A  # noqa: E402
from imagenet_models_amd import parse_hw, split_dir, synthetic_ragged  # noqa: E402,F401

_logger = logging.getLogger('train')

parser = argparse.ArgumentParser(description='GA ImageNet training (MI355X-native)')
parser.add_argument('data_dir', nargs='?', default='', help='dataset root: an image folder with one directory per class under the '
                    'split directories (unused with --synthetic)')
parser.add_argument('--train-split', default='train', metavar='NAME', help='dataset train split: a directory of the root (default: '
                    'train; the root itself where it has no such directory)')
parser.add_argument('--val-split', default='validation', metavar='NAME', help='dataset validation split (default: validation)')
parser.add_argument('-j', '--workers', type=int, default=8, metavar='N', help='host threads of the JPEG entropy stage, at most 16 '
                    '(default: 8)')
parser.add_argument('--model', default='ga_convnext_tiny_768')
parser.add_argument('--num-classes', type=int, default=None)
parser.add_argument('-b', '--batch-size', type=int, default=128)
parser.add_argument('--epochs', type=int, default=300)
parser.add_argument('--steps-per-epoch', type=int, default=100, help='synthetic epoch length (batches)')
parser.add_argument('--opt', default='sgd')
parser.add_argument('--opt-eps', type=float, default=None)
parser.add_argument('--opt-betas', type=float, nargs='+', default=None)
parser.add_argument('--momentum', type=float, default=0.9)
parser.add_argument('--weight-decay', type=float, default=2e-5)
parser.add_argument('--lr', type=float, default=0.05)
parser.add_argument('--sched', default='cosine', help='LR scheduler: "cosine" or "step" (default: "cosine"; any other name runs at a '
                    'constant --lr)')
parser.add_argument('--decay-epochs', type=float, default=100, metavar='N', help='--sched step: epochs between two decays, may be '
                    'fractional (default: 100)')
parser.add_argument('--decay-rate', '--dr', type=float, default=0.1, metavar='RATE', help='--sched step: the factor of one decay '
                    '(default: 0.1)')
parser.add_argument('--warmup-lr', type=float, default=1e-4)
parser.add_argument('--min-lr', type=float, default=1e-6)
parser.add_argument('--warmup-epochs', type=int, default=3)
parser.add_argument('--smoothing', type=float, default=0.1)
parser.add_argument('--bce-loss', action='store_true')
parser.add_argument('--bce-target-thresh', type=float, default=None, help='threshold for binarizing softened BCE targets')
# mixup / cutmix: the defaults are the reference's (GA/train.py:215-228: both ON); 0 / 0 turns them off
parser.add_argument('--mixup', type=float, default=0.2, help='mixup alpha, mixup enabled if > 0')
parser.add_argument('--cutmix', type=float, default=1.0, help='cutmix alpha, cutmix enabled if > 0')
parser.add_argument('--cutmix-minmax', type=float, nargs='+', default=None)
parser.add_argument('--mixup-prob', type=float, default=1.0)
parser.add_argument('--mixup-switch-prob', type=float, default=0.5)
parser.add_argument('--mixup-mode', default='batch', help='"batch", "pair" or "elem"; "half" is refused: it halves the batch the '
                    'engine is planned for')
parser.add_argument('--collate-mixup', action='store_true', help='the prefetcher order every reference recipe runs: mixup / cutmix on '
                    'the uint8 batch at collate time (rounded back to uint8), then normalise, then RandomErasing last on the mixed '
                    'image, as one device pass (timm FastCollateMixup + PrefetchLoader); opt-in, the default order is normalise -> '
                    'erase -> mixup in fp32')
parser.add_argument('--mixup-off-epoch', type=int, default=0)
# RandomErasing on the device (MAP/train.py:214-221; every MAP recipe runs --remode pixel --reprob 0.25)
parser.add_argument('--reprob', type=float, default=0., metavar='PCT', help='Random erase prob (default: 0.)')
parser.add_argument('--remode', type=str, default='pixel', help='Random erase mode (default: "pixel")')
parser.add_argument('--recount', type=int, default=1, help='Random erase count (default: 1)')
parser.add_argument('--resplit', action='store_true', default=False, help='Do not random erase first (clean) augmentation split: '
                    'with --aug-splits N the eraser gets num_splits = N and leaves split 0 alone (inert without --aug-splits, where '
                    'the batch has no splits)')
# augmentation splits + the JSD consistency loss (GA/train.py:195-196,559-561,613-615: AugMixDataset + JsdCrossEntropy)
parser.add_argument('--aug-splits', type=int, default=0, metavar='N', help='Number of augmentation splits (default: 0, valid: 0 or >=2): '
                    '-b counts base samples, each is cropped once and run N times -- split 0 as cropped, the others through --aa with '
                    'draws of their own -- so the model runs on N x b rows.  Excludes mixup / cutmix: their DEFAULTS (on) are switched '
                    'off by this flag, explicit --mixup / --cutmix > 0 end the run')
parser.add_argument('--jsd-loss', action='store_true', default=False, help='Enable Jensen-Shannon Divergence + CE loss (timm '
                    'JsdCrossEntropy, alpha 12, per head); needs --aug-splits; takes precedence over --bce-loss')
parser.add_argument('--split-bn', action='store_true', help='refused: separate BatchNorm layers per augmentation split are not built')
# RandAugment on the device (MAP/train.py --aa; every recipe of MAP/train_with_script.py runs rand-mN-mstd0.5-inc1)
parser.add_argument('--aa', type=str, default=None, metavar='NAME', help='Use AutoAugment policy, timm\'s "rand-m9-mstd0.5-inc1" form '
                    '(RandAugment only; applied on the device to the uint8 batch, ahead of every other input stage). (default: None)')
parser.add_argument('--train-interpolation', type=str, default='random', help='Training interpolation of the geometric RandAugment ops '
                    '(random, bilinear, bicubic, nearest; default: "random") and of the random-resized crop (random, bilinear, bicubic)')
# random-resized crop + flip on the device (timm create_loader's scale / ratio / hflip); runs on the decoded images of --synthetic-source
parser.add_argument('--scale', type=float, nargs=2, default=[0.08, 1.0], metavar=('LO', 'HI'), help='Random resize scale '
                    '(default: 0.08 1.0)')
parser.add_argument('--ratio', type=float, nargs=2, default=[3. / 4., 4. / 3.], metavar=('LO', 'HI'), help='Random resize aspect '
                    'ratio (default: 0.75 1.33)')
parser.add_argument('--hflip', type=float, default=0.5, help='Horizontal flip training aug probability (default: 0.5)')
parser.add_argument('--synthetic-source', type=str, default=None, metavar='HxW', help='the synthetic loader yields DECODED images '
                    '(uint8 HWC, heights and widths within [0.5, 1.5] of H and W) and the step starts with the random-resized crop + '
                    'flip on the device (default: None, the loader yields cropped batches)')
parser.add_argument('--drop-path', type=float, default=None)
parser.add_argument('--drop', type=float, default=None, metavar='PCT', help='Dropout rate, forwarded to the model factory as drop_rate '
                    '(MAP/train.py:446) when given; a factory that has no such argument ends the run (default: not forwarded)')
# repeated augmentation (timm RepeatAugSampler; GA/train.py:197 defaults to 3, MAP/train.py to 0, six of the seven MAP recipes pass 3)
parser.add_argument('--aug-repeats', type=int, default=0, metavar='N', help='Number of augmentation repetitions: every image of the '
                    'epoch\'s permutation N times in a row, the epoch cut back to the dataset\'s length; each distinct file of a batch '
                    'is decoded once (folder loader only; default: 0 -- the reference defaults to 3 in GA/train.py and 0 in MAP/train.py)')
parser.add_argument('--selected-round', type=int, default=256, metavar='N', help='with --aug-repeats: the epoch is rounded down to a '
                    'multiple of N samples before it is split over the ranks, 0: not rounded (default: 256, timm\'s)')
parser.add_argument('--grad-accumulation', type=int, default=1)
parser.add_argument('-tb', '--total-batch-size', type=int, default=None, metavar='N', help='total batch size per optimizer step: sets '
                    '--grad-accumulation to N // (batch size * ranks) and overrides it (MAP/train.py:406; default: not set)')
parser.add_argument('--cooldown-epochs', type=int, default=0, metavar='N', help='epochs to run at --min-lr after the cosine schedule '
                    'ends: the run has --epochs + N epochs (default: 0 -- the reference\'s is 10, so its 300-epoch recipes run 310)')
# the per-epoch evaluation of a folder run (validate.py has the same two)
parser.add_argument('--crop-pct', type=float, default=None, metavar='N', help='centre-crop fraction of the evaluation transform: the '
                    'short side is resized to floor(img / crop_pct) (default: 0.875; the recipes pass 0.95 or 0.875)')
parser.add_argument('--interpolation', type=str, default='bicubic', help='resize interpolation of the evaluation transform, bilinear or '
                    'bicubic (default: bicubic)')
parser.add_argument('--input-size', type=int, nargs=3, default=None, metavar=('C', 'H', 'W'), help='accepted when it is the size the '
                    'model is built for (3 224 224 for most); other sizes are not built')
parser.add_argument('--test-input-size', type=int, nargs=3, default=None, metavar=('C', 'H', 'W'), help='as --input-size, for the '
                    'evaluation')
parser.add_argument('--pin-mem', action='store_true', help='accepted for CLI compatibility (the staging ring is always pinned)')
parser.add_argument('--log-wandb', action='store_true', help='accepted with a warning: wandb logging is not built')
parser.add_argument('--project-name', default=None, help='accepted for CLI compatibility (the wandb project of a recipe)')
parser.add_argument('--print-config', action='store_true', help='print the resolved settings as one JSON line and exit, before the '
                    'model is created or a device touched')
parser.add_argument('--GA_lam', type=float, default=0)
parser.add_argument('--dec-lam', type=float, default=None, help='MAP: weight of the group-decorrelation KL term '
                    '(MAP/train_with_script.py:39, multi_group_loss); alias of --GA_lam for the map_* models')
parser.add_argument('--no-ddp-bb', action='store_true', help='no per-forward broadcast of the BatchNorm buffers from rank 0 '
                    '(GA/train.py:283,514)')
parser.add_argument('--sync-bn', action='store_true', help='BatchNorm statistics over the global batch (GA/train.py:247,449-455): the '
                    'per-channel sums go through the native RCCL communicator; implies --comm native')
parser.add_argument('--comm', default='torch', choices=['torch', 'native', 'native-bf16'], help='transport of the gradient buckets: '
                    'torch.distributed, or libgaext\'s own RCCL communicator (ga_allreduce_bucket) with an fp32 / bf16 wire')
parser.add_argument('--dist-bn', default='reduce', help='"reduce" | "broadcast" | "": distribute the BatchNorm running '
                    'statistics between ranks after every epoch (timm distribute_bn, GA/train.py:665-674)')
parser.add_argument('--model-ema', action='store_true', help='track an EMA of the weights (timm ModelEmaV2)')
parser.add_argument('--model-ema-decay', type=float, default=0.9998)
parser.add_argument('--clip-grad', type=float, default=None, help='clip gradients (GA/train.py --clip-grad)')
parser.add_argument('--clip-mode', default='norm', help='"norm", "value" or "agc"')
parser.add_argument('--amp', action='store_true', help='bf16 math mode (default)')
parser.add_argument('--fp32', action='store_true', help='fp32 parity math mode')
parser.add_argument('--gram-fp64', action='store_true', help='GA-ConvNeXt only: get_gram in float64 while training with a per-step '
                    'batch below 128, as the reference does (ga_convnext.py:456-457); off by default')
parser.add_argument('--channels-last', action='store_true', help='accepted for CLI compatibility (activations are always NHWC)')
parser.add_argument('--synthetic', action='store_true')
parser.add_argument('--device', default='cuda')
parser.add_argument('--seed', type=int, default=42)
parser.add_argument('--log-interval', type=int, default=50)
parser.add_argument('--output', default='')
# checkpoints and resuming (GA/train.py:96-99,269,485-526,633-693,810-812; MAP/train.py has the same flags)
parser.add_argument('--resume', default='', type=str, metavar='PATH', help='Resume full model and optimizer state from checkpoint; with the '
                    "file's train_state every random stream and the loader position too (default: none)")
parser.add_argument('--no-resume-opt', action='store_true', default=False, help='prevent resume of optimizer state when resuming model: '
                    'weights (and EMA) and epoch only')
parser.add_argument('--start-epoch', default=None, type=int, metavar='N', help='manual epoch number (useful on restarts); overrides the '
                    'epoch of --resume')
parser.add_argument('--initial-checkpoint', default='', type=str, metavar='PATH', help='Initialize model from this checkpoint (weights '
                    'only; default: none)')
parser.add_argument('--recovery-interval', type=int, default=0, metavar='N', help='write a recovery checkpoint every N optimizer steps '
                    'and at the last batch of an epoch, behind the step; only the newest is kept (default: 0, none)')
parser.add_argument('--checkpoint-hist', type=int, default=None, metavar='N', help='number of best epoch checkpoints to keep (default: '
                    'all of them -- the reference keeps 10; every epoch file stays, as it did before this flag existed)')
parser.add_argument('--eval-metric', default='top1', type=str, metavar='EVAL_METRIC', help='Best metric: "top1", "top5" or "loss" (the '
                    'epoch\'s training loss, lower is better: the evaluation loops compute none) (default: "top1")')
parser.add_argument('--local_rank', default=0, type=int)


class SyntheticLoader:
    """fixed-shape random batches generated on the device (seed = args.seed + rank, like timm random_seed); with `source` (H, W)
    one RaggedBatch of decoded images of varying sizes, built once and yielded every step"""

    def __init__(self, batch, steps, num_classes, seed, device, img=224, uint8=False, source=None):
        self.batch, self.steps, self.nc, self.img, self.uint8 = batch, steps, num_classes, img, uint8
        self.g = torch.Generator(device=device).manual_seed(seed)
        self.device = device
        self.ragged = synthetic_ragged(batch, source, seed, device) if source is not None else None
        self.start_batch = 0

    def __len__(self):
        return self.steps

    def set_epoch(self, epoch, start_batch=0):
        """the next iteration yields the batches from `start_batch` on (a run resumed inside an epoch: the generator `g` continues
        from its restored state, the epoch number plays no part)"""
        self.start_batch = int(start_batch)

    def __iter__(self):
        for _ in range(self.start_batch, self.steps):
            if self.ragged is not None:
                yield self.ragged, torch.randint(0, self.nc, (self.batch,), device=self.device, generator=self.g)
                continue
            if self.uint8:       # the layout of timm's fast_collate: PrefetchLoader / the collate-time mixup take it from here
                x = torch.randint(0, 256, (self.batch, 3, self.img, self.img), device=self.device, generator=self.g, dtype=torch.uint8)
            else:
                x = torch.randn(self.batch, 3, self.img, self.img, device=self.device, generator=self.g)
            y = torch.randint(0, self.nc, (self.batch,), device=self.device, generator=self.g)
            yield x, y


class AverageMeter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def train_one_epoch(epoch, step_fn, loader, args, world, rank, model_ema=None, saver=None, start_batch=0):
    batch_time_m, losses_m = AverageMeter(), AverageMeter()
    end = time.time()
    last_idx = len(loader) - 1
    loss = None
    for batch_idx, (x, y) in enumerate(loader, start_batch):
        loss = step_fn(x, y)
        boundary = step_fn.micro % step_fn.accum == 0
        if model_ema is not None and boundary:   # after every optimizer step (GA/train.py:774)
            model_ema.update()
        # recovery points at optimizer-step boundaries only (no partial gradient to save): a device snapshot, written behind
        if args.recovery_interval and args.output and boundary and (step_fn.opt.steps % args.recovery_interval == 0 or batch_idx == last_idx):
            state = A.capture_train_state(step_fn, loader, epoch, batch_idx + 1, rank, world, device_counters=False)
            if saver is not None:
                saver.take(epoch, train_state=state, recovery_batch=batch_idx)
        if batch_idx % args.log_interval == 0 or batch_idx == last_idx:
            torch.cuda.synchronize()
            lv = loss.detach().clone()
            if world > 1:
                dist.all_reduce(lv)
                lv /= world
            losses_m.update(float(lv), x.size(0))
            batch_time_m.update((time.time() - end) / (args.log_interval if batch_idx else 1))
            if rank == 0:
                _logger.info('Train: {} [{:>4d}/{} ({:>3.0f}%)]  Loss: {:#.4g} ({:#.3g})  Time: {:.3f}s, {:>7.2f}/s  LR: {:.3e}'.format(
                    epoch, batch_idx, len(loader), 100. * batch_idx / max(last_idx, 1), losses_m.val, losses_m.avg,
                    batch_time_m.val, x.size(0) * world / batch_time_m.val, step_fn.opt.param_groups[0]['lr']))
            end = time.time()
    return OrderedDict([('loss', losses_m.avg)])


def validate_folder(model, loader, crop, world):
    """top-1 / top-5 over exactly the real samples of an evaluation FolderLoader, summed over the ranks"""
    model.eval()
    counts = A.evaluate_folder(model, loader, crop)
    if world > 1:
        dist.all_reduce(counts)
    model.train()
    c1, c5, n = (int(v) for v in counts.tolist())
    return OrderedDict([('top1', 100. * c1 / max(n, 1)), ('top5', 100. * c5 / max(n, 1)), ('samples', n)])


def validate(model, loader, args, world):
    model.eval()
    top1_m, top5_m = AverageMeter(), AverageMeter()
    with torch.no_grad():
        for x, y in loader:
            outs = model(x)
            _, idx = A.heads_topk(outs, 5)                       # output = sum_k out_k.float() (train.py:848-851)
            acc1, acc5 = A.accuracy_from_topk(idx, y, (1, 5))
            if world > 1:
                t = torch.stack([acc1, acc5])
                dist.all_reduce(t)
                acc1, acc5 = t / world
            top1_m.update(float(acc1), x.size(0))
            top5_m.update(float(acc5), x.size(0))
    model.train()
    return OrderedDict([('top1', top1_m.avg), ('top5', top5_m.avg)])


def check_input_sizes(args, img):
    """--input-size / --test-input-size name the size the model is built for, or end the run"""
    for flag, size in (('--input-size', args.input_size), ('--test-input-size', args.test_input_size)):
        if size is not None and tuple(size) != (3, img, img):
            raise SystemExit(f"train.py: {flag} {' '.join(str(v) for v in size)}: {args.model} is built for 3 {img} {img}; other "
                             'sizes are not built')


def schedule_config(args):
    """the learning-rate schedule --sched resolves to: cosine, step, or none (a constant --lr) for every name that is not built"""
    warm = dict(warmup_epochs=args.warmup_epochs, warmup_lr=args.warmup_lr)
    if args.sched == 'cosine':
        return dict(kind='cosine', t_initial=args.epochs, min_lr=args.min_lr, **warm)
    if args.sched == 'step':
        return dict(kind='step', decay_epochs=args.decay_epochs, decay_rate=args.decay_rate, **warm)
    return dict(kind='none')


def create_scheduler(args, opt):
    cfg = schedule_config(args)
    if cfg['kind'] == 'cosine':         # --cooldown-epochs run past t_initial, where the schedule holds lr_min
        return A.CosineLRScheduler(opt, t_initial=args.epochs, lr_min=args.min_lr, warmup_t=args.warmup_epochs, warmup_lr_init=args.warmup_lr)
    if cfg['kind'] == 'step':
        return A.StepLRScheduler(opt, decay_t=args.decay_epochs, decay_rate=args.decay_rate, warmup_t=args.warmup_epochs,
                                 warmup_lr_init=args.warmup_lr)
    return None


def _flag_given(argv, *flags):
    return any(a.split('=', 1)[0] in flags for a in argv)


def resolve_aug_splits(args, argv=None):
    """--aug-splits / --jsd-loss / --split-bn as GA/train.py:533-561,613-615 checks them.  The reference asserts that mixup is off
    under aug splits; here mixup and cutmix default to ON, so the defaults yield to --aug-splits and only explicit ones end the run"""
    argv = sys.argv[1:] if argv is None else argv
    if args.split_bn:
        raise SystemExit('train.py: --split-bn (separate BatchNorm layers per augmentation split) is not built')
    if args.aug_splits == 1 or args.aug_splits < 0:
        raise SystemExit(f'train.py: --aug-splits {args.aug_splits}: a split count of 1 makes no sense (0, or at least 2)')
    if args.aug_splits > 8:
        raise SystemExit(f'train.py: --aug-splits {args.aug_splits}: at most 8 splits are built')
    if args.jsd_loss and args.aug_splits < 2:
        raise SystemExit('train.py: --jsd-loss is only valid with --aug-splits >= 2 (it compares the augmentation splits)')
    if args.aug_splits:
        if _flag_given(argv, '--mixup', '--cutmix', '--cutmix-minmax', '--collate-mixup') and (
                args.mixup > 0 or args.cutmix > 0. or args.cutmix_minmax is not None or args.collate_mixup):
            raise SystemExit(f'train.py: --aug-splits {args.aug_splits} cannot be combined with mixup / cutmix (--mixup {args.mixup} '
                             f'--cutmix {args.cutmix}): the split-major batch has no mixing partner order and the JSD loss needs '
                             'class indices; pass --mixup 0 --cutmix 0 or leave them out')
        args.mixup, args.cutmix = 0.0, 0.0


def resolve_config(args, world, rank, train_loader=None):
    """the settings the flags resolve to, checked on the host before the model is created (what --print-config prints).  Sets
    args.grad_accumulation from -tb and args.crop_pct to its default."""
    if args.aug_repeats < 0 or args.selected_round < 0 or args.cooldown_epochs < 0:
        raise SystemExit(f'train.py: --aug-repeats {args.aug_repeats}, --selected-round {args.selected_round} and --cooldown-epochs '
                         f'{args.cooldown_epochs} are whole numbers of at least 0')
    if args.total_batch_size is not None:
        args.grad_accumulation = args.total_batch_size // (args.batch_size * world)
        if args.grad_accumulation < 1:
            raise SystemExit(f'train.py: -tb {args.total_batch_size} is less than one batch of every rank ({args.batch_size} x {world} '
                             'rank(s)): no whole number of batches per optimizer step')
    if args.crop_pct is None:
        args.crop_pct = 0.875                  # timm's evaluation default
    resolve_aug_splits(args)
    try:
        optimizer = A.optimizer_config(args.opt, momentum=args.momentum, eps=args.opt_eps, betas=args.opt_betas)
    except ValueError as e:
        raise SystemExit(f'train.py: --opt: {e}')
    if args.sched == 'step' and not args.decay_epochs > 0:
        raise SystemExit(f'train.py: --decay-epochs {args.decay_epochs}: more than 0')
    cfg = OrderedDict([('model', args.model), ('batch_size', args.batch_size), ('world_size', world),
                       ('grad_accumulation', args.grad_accumulation), ('epochs', args.epochs + args.cooldown_epochs),
                       ('cooldown_epochs', args.cooldown_epochs), ('aug_repeats', args.aug_repeats),
                       ('selected_round', args.selected_round), ('crop_pct', args.crop_pct), ('interpolation', args.interpolation),
                       ('drop', args.drop), ('opt', args.opt.lower()), ('optimizer', optimizer), ('schedule', schedule_config(args)),
                       ('aug_splits', args.aug_splits), ('jsd_loss', bool(args.jsd_loss)),
                       ('model_batch', args.batch_size * max(1, args.aug_splits))])
    if train_loader is not None:
        cfg.update(train_images=len(train_loader.dataset), batches_per_epoch=len(train_loader),
                   distinct_files_per_epoch=train_loader.distinct_files(0))
    return cfg


def main():
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    args = parser.parse_args()
    if args.device != 'cuda':
        raise SystemExit('train.py: --device cpu is not available: the product path runs on the libgaext HIP kernels only '
                         '(the CPU baseline is the oracle timed by `bench.py`, kind "port")')
    if not args.synthetic and not args.data_dir:
        raise SystemExit('train.py: only --synthetic data is shipped (no dataset / network in this environment)')
    folder = None if args.synthetic else args.data_dir
    if args.mixup_mode == 'half':
        raise SystemExit("train.py: --mixup-mode half returns half of every batch; the engine is planned for the full batch size, so "
                         "it is not built ('batch', 'pair' or 'elem')")
    if args.mixup_mode not in ('batch', 'pair', 'elem'):
        raise SystemExit(f"train.py: --mixup-mode {args.mixup_mode!r}: 'batch', 'pair' or 'elem'")
    try:
        source = parse_hw(args.synthetic_source) if args.synthetic_source else None
    except ValueError as e:
        raise SystemExit(str(e))
    if folder is not None:
        try:
            train_set = A.ImageFolder(split_dir(folder, args.train_split))
            val_set = A.ImageFolder(split_dir(folder, args.val_split))
        except (OSError, RuntimeError) as e:
            raise SystemExit(f'train.py: {e}')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', str(args.local_rank)))
    if args.eval_metric not in ('top1', 'top5', 'loss'):
        raise SystemExit(f"train.py: --eval-metric {args.eval_metric!r}: 'top1', 'top5' or 'loss'")
    if args.checkpoint_hist is not None and args.checkpoint_hist < 1:
        raise SystemExit(f'train.py: --checkpoint-hist {args.checkpoint_hist}: at least 1')
    if not A.is_model(args.model):
        raise SystemExit(f'train.py: --model {args.model!r} is not a registered model')
    check_input_sizes(args, A.model_img_size(args.model))
    # the training order is planned on the host (the decoder joins the loader once it exists): a folder too small for its batch or
    # for --selected-round ends the run here
    loader = None
    if folder is not None:
        try:
            loader = A.FolderLoader(train_set, args.batch_size, None, train=True, seed=args.seed, rank=rank, world=world,
                                    aug_repeats=args.aug_repeats, selected_round=args.selected_round)
        except ValueError as e:
            raise SystemExit(f'train.py: {e}')
    config = resolve_config(args, world, rank, loader)
    if args.print_config:
        print(json.dumps(config))
        return
    if args.log_wandb and rank == 0:
        _logger.warning('--log-wandb: wandb logging is not built; the run logs to the console (and --output) only')
    if args.aug_repeats and folder is None and rank == 0:
        _logger.info('--aug-repeats %d has no effect with --synthetic: there are no files to repeat', args.aug_repeats)
    # the files are read here, on the host: one that is missing or does not load ends the run before the device is touched
    resume_ck = None
    for flag, path in (('--resume', args.resume), ('--initial-checkpoint', args.initial_checkpoint)):
        if not path:
            continue
        if not os.path.isfile(path):
            raise SystemExit(f'train.py: {flag} {path!r}: no such file')
        try:
            ck = A.read_checkpoint(path)
        except Exception as e:
            raise SystemExit(f'train.py: {flag} {path!r} does not load: {e}')
        if flag == '--resume':
            if not isinstance(ck, dict) or 'state_dict' not in ck:
                raise SystemExit(f"train.py: --resume {path!r} is not a training checkpoint (no 'state_dict' key)")
            resume_ck = ck
        del ck
    resume_state = resume_ck.get('train_state') if (resume_ck is not None and not args.no_resume_opt) else None
    if resume_state is not None and resume_state['world_size'] != world:
        raise SystemExit(f"train.py: --resume {args.resume!r} was written by {resume_state['world_size']} rank(s), this run has {world}: "
                         'the per-rank generator states and the loader position do not carry over (--no-resume-opt takes the weights '
                         'and the epoch only)')
    torch.manual_seed(args.seed + rank)
    if resume_state is not None:             # the DropPath / dropout samplers are keyed by torch.initial_seed() when the engine is built
        torch.manual_seed(A.saved_initial_seed(resume_state, rank))
    np.random.seed(args.seed + rank)          # timm random_seed(): mixup draws lam / boxes from numpy's global generator
    random.seed(args.seed + rank)             # ... and RandomErasing draws its boxes from Python's
    try:
        model = A.create_model(args.model, pretrained=False, num_classes=args.num_classes, drop_rate=args.drop,
                               drop_path_rate=args.drop_path, math_mode='fp32' if args.fp32 else 'bf16',
                               gram_fp64=True if args.gram_fp64 else None)
    except (TypeError, AssertionError) as e:
        if args.drop is None:
            raise
        raise SystemExit(f'train.py: --drop {args.drop}: {args.model} does not take drop_rate: {e}')
    img = getattr(model, 'cfg', {}).get('img_size', 224)
    check_input_sizes(args, img)
    try:
        eval_crop = A.ResizeCenterCrop(img, args.crop_pct, args.interpolation) if folder is not None else None
    except ValueError as e:
        raise SystemExit(f'train.py: --crop-pct / --interpolation: {e}')
    # the flag-dependent transforms, each built once, on the host: a flag they refuse ends the run before the device is touched
    # RandAugment as timm's create_transform builds it: fill = the rounded dataset mean, the interpolation of the geometric ops
    try:
        auto_augment = A.RandAugment(args.aa, interpolation=args.train_interpolation) if args.aa else None
    except ValueError as e:
        raise SystemExit(f'train.py: --aa / --train-interpolation: {e}')
    # the random-resized crop + flip as timm's create_transform builds them, ahead of everything else: only on decoded sources
    crop = None
    if source is not None or folder is not None:
        try:
            crop = A.RandomResizedCrop(img, scale=args.scale, ratio=args.ratio, interpolation=args.train_interpolation, hflip=args.hflip)
        except ValueError as e:
            raise SystemExit(f"train.py: --scale / --ratio / --train-interpolation with {'--synthetic-source' if folder is None else 'an image folder'}: {e}")
    backend = os.environ.get('GA_DIST_BACKEND', 'nccl')          # gloo: rehearsal with ranks sharing a device
    ndev = max(1, torch.cuda.device_count())
    if local >= ndev:
        if world > 1 and backend == 'nccl':
            raise SystemExit(f'train.py: LOCAL_RANK {local} but only {ndev} GPU(s) are visible: RCCL needs one device per rank '
                             '(GA_DIST_BACKEND=gloo rehearses several ranks on one device)')
        local %= ndev
    torch.cuda.set_device(local)
    if world > 1:
        if backend == 'nccl':
            dist.init_process_group('nccl', init_method='env://', device_id=torch.device('cuda', local))
        else:
            dist.init_process_group(backend, init_method='env://')
    model = model.cuda()
    if args.initial_checkpoint:
        A.load_checkpoint(model, args.initial_checkpoint)
    if world > 1:
        dist.broadcast(model.flat_state()['params'], 0)
        dist.broadcast(model.flat_state()['buffers'], 0)
    comm = None
    if world > 1 and (args.sync_bn or args.comm != 'torch'):
        if backend != 'nccl':
            raise SystemExit('train.py: --comm native / --sync-bn need one GPU per rank (the RCCL communicator of libgaext)')
        comm = A.NativeComm(wire='bf16' if args.comm == 'native-bf16' else 'fp32')
        if args.sync_bn:
            model.convert_sync_batchnorm(comm)
    if rank == 0:
        _logger.info('Model %s created, param count: %d', args.model, sum(p.numel() for p in model.parameters()))
    opt = A.create_optimizer_v2(model, opt=args.opt, lr=args.lr, weight_decay=args.weight_decay, momentum=args.momentum,
                                eps=args.opt_eps, betas=tuple(args.opt_betas) if args.opt_betas else None)
    sched = create_scheduler(args, opt)
    lam = args.dec_lam if args.dec_lam is not None else args.GA_lam
    # mixup / cutmix (GA/train.py:544-557): smoothing then lives in the dense target and the loss is SoftTargetCrossEntropy /
    # BinaryCrossEntropy on it (:616-621)
    # --collate-mixup: the same augmentation in the prefetcher order (FastCollateMixup on the uint8 batch -> normalise -> erase)
    mixup_fn = collate_mixup = None
    if args.mixup > 0 or args.cutmix > 0. or args.cutmix_minmax is not None:
        mkw = dict(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax, prob=args.mixup_prob,
                   switch_prob=args.mixup_switch_prob, mode=args.mixup_mode, label_smoothing=args.smoothing,
                   num_classes=model.num_classes)
        if args.collate_mixup:
            collate_mixup = A.FastCollateMixup(**mkw)
        elif args.mixup_mode != 'batch':       # the default order in modes pair / elem: the same pass on the normalised fp32 batch
            mixup_fn = A.FastCollateMixup(**mkw)
        else:
            mixup_fn = A.Mixup(**mkw)
    elif args.collate_mixup:
        raise SystemExit('train.py: --collate-mixup needs --mixup > 0, --cutmix > 0 or --cutmix-minmax')
    # RandomErasing as timm's create_loader builds it (re_prob / re_mode / re_count: the MAX count; num_splits 0 without aug-splits)
    random_erasing = None
    # --aug-splits N: the eraser keeps the clean split only with --resplit (timm create_loader: re_num_splits)
    aug_splits = A.AugSplits(args.aug_splits) if args.aug_splits else None
    if args.reprob > 0.:
        random_erasing = A.RandomErasing(probability=args.reprob, mode=args.remode, max_count=args.recount,
                                         num_splits=args.aug_splits if (args.resplit and args.aug_splits) else 0, seed=args.seed + rank)
    if aug_splits is not None and rank == 0:
        _logger.info('--aug-splits %d: %d base samples per batch, the model runs on %d rows; mixup / cutmix are off; loss: %s',
                     args.aug_splits, args.batch_size, args.batch_size * args.aug_splits,
                     'JSD (alpha 12) + CE on the clean split' if args.jsd_loss else 'the ordinary loss over all rows')
    step_fn = A.TrainStep(model, opt, args.batch_size * max(1, args.aug_splits), lam=lam,
                          loss='jsd' if args.jsd_loss else 'bce' if args.bce_loss else 'ce', aug_splits=aug_splits,
                          smoothing=args.smoothing, grad_accumulation=args.grad_accumulation,
                          clip_grad=args.clip_grad, clip_mode=args.clip_mode, broadcast_buffers=not args.no_ddp_bb,
                          mixup_fn=mixup_fn, bce_target_thresh=args.bce_target_thresh, comm=comm, random_erasing=random_erasing,
                          collate_mixup=collate_mixup, auto_augment=auto_augment, crop=crop)
    model_ema = A.ModelEma(model, args.model_ema_decay) if args.model_ema else None
    decoder = None
    if folder is not None:
        # the folder: the files' bytes -> JpegDecoder (host entropy stage on -j threads, reconstruction on the device) -> the crop
        if len(train_set.classes) > model.num_classes:
            raise SystemExit(f'train.py: {len(train_set.classes)} class directories, the model has {model.num_classes} classes '
                             '(--num-classes)')
        loader.decoder = decoder = A.JpegDecoder(threads=args.workers)
        eval_loader = A.FolderLoader(val_set, args.batch_size, decoder, train=False, rank=rank, world=world)
        if rank == 0:
            _logger.info('Folder %s: %d training images in %d classes, %d validation images; %d decoder threads', folder,
                         len(train_set), len(train_set.classes), len(val_set), decoder.threads)
            if args.aug_repeats:
                _logger.info('    --aug-repeats %d (selected_round %d): %d batches per epoch from %d distinct files on this rank, each '
                             'distinct file of a batch decoded once', args.aug_repeats, args.selected_round,
                             config['batches_per_epoch'], config['distinct_files_per_epoch'])
    else:
        loader = SyntheticLoader(args.batch_size, args.steps_per_epoch, model.num_classes, args.seed + rank, 'cuda', img,
                                 uint8=step_fn.input_stage.takes == 'uint8', source=source)
        eval_loader = SyntheticLoader(args.batch_size, max(1, args.steps_per_epoch // 10), model.num_classes, 7 + rank, 'cuda', img)
    start_epoch = start_batch = 0
    if resume_ck is not None:
        try:
            start_epoch, start_batch = A.resume_checkpoint(resume_ck, model, opt, model_ema, step_fn, loader, rank, world,
                                                           resume_opt=not args.no_resume_opt)
        except ValueError as e:
            raise SystemExit(f'train.py: --resume {args.resume!r}: {e}')
        resume_ck = resume_state = None
    if args.start_epoch is not None:
        start_epoch, start_batch = args.start_epoch, 0
    if sched is not None:
        sched.step(start_epoch)
    if args.resume and rank == 0:
        _logger.info('Resumed %s: starting at epoch %d, batch %d of %d, lr %.6e', args.resume, start_epoch, start_batch, len(loader),
                     opt.param_groups[0]['lr'])
    saver = None
    if args.output and rank == 0:
        saver = A.CheckpointSaver(args.output, A.DeviceSnapshot(model, opt, model_ema, step_fn), arch=args.model,
                                  eval_metric=args.eval_metric, checkpoint_hist=args.checkpoint_hist)
    model.train()
    # leaving this block -- the normal end or an exception -- waits for the write in flight; the writer's own exception is raised here
    with saver if saver is not None else contextlib.nullcontext():
        train_loop(args, model, opt, sched, step_fn, model_ema, loader, eval_loader, eval_crop, decoder, folder, mixup_fn or collate_mixup,
                   saver, start_epoch, start_batch, world, rank)
    if world > 1:
        dist.destroy_process_group()


def evaluate(model, eval_loader, eval_crop, args, world, folder):
    return validate_folder(model, eval_loader, eval_crop, world) if folder is not None else validate(model, eval_loader, args, world)


def train_loop(args, model, opt, sched, step_fn, model_ema, loader, eval_loader, eval_crop, decoder, folder, mixup, saver, start_epoch,
               start_batch, world, rank):
    for epoch in range(start_epoch, args.epochs + args.cooldown_epochs):
        if sched is not None:
            sched.step(epoch)
        if mixup is not None and args.mixup_off_epoch and epoch >= args.mixup_off_epoch:
            mixup.mixup_enabled = False      # GA/train.py:705-709, MAP/train.py:846-850
        first = start_batch if epoch == start_epoch else 0       # a recovery file resumes inside its epoch
        loader.set_epoch(epoch, first)
        train_metrics = train_one_epoch(epoch, step_fn, loader, args, world, rank, model_ema, saver, first)
        if world > 1 and args.dist_bn in ('broadcast', 'reduce'):
            A.distribute_bn(model, world, args.dist_bn == 'reduce')
        eval_metrics = evaluate(model, eval_loader, eval_crop, args, world, folder)
        if folder is not None and rank == 0:
            _logger.info('    evaluated %d images; %d of %d files so far went through the PIL fallback', eval_metrics['samples'],
                         decoder.fallbacks, decoder.decoded)
        if rank == 0:
            _logger.info('*** epoch %d: train loss %.4f  top1 %.3f  top5 %.3f', epoch, train_metrics['loss'],
                         eval_metrics['top1'], eval_metrics['top5'])
        if model_ema is not None:
            # the EMA weights evaluated in the model's place; the checkpoint is selected by their metric (GA/train.py:675-679)
            with model_ema.swapped():
                if world > 1 and args.dist_bn in ('broadcast', 'reduce'):      # distribute_bn of the EMA's statistics (:672-674)
                    A.distribute_bn(model, world, args.dist_bn == 'reduce')
                eval_metrics = evaluate(model, eval_loader, eval_crop, args, world, folder)
            if rank == 0:
                _logger.info('*** epoch %d (EMA): top1 %.3f  top5 %.3f', epoch, eval_metrics['top1'], eval_metrics['top5'])
        if args.output:
            state = A.capture_train_state(step_fn, loader, epoch, len(loader), rank, world, device_counters=False)
            if saver is not None:
                metric = train_metrics['loss'] if args.eval_metric == 'loss' else eval_metrics[args.eval_metric]
                best, best_epoch = saver.take(epoch, metric=metric, train_state=state)
                _logger.info('    checkpoint of epoch %d queued; best %s so far %.4f (epoch %d)', epoch, args.eval_metric, best, best_epoch)


if __name__ == '__main__':
    main()
