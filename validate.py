#!/usr/bin/env python3
"""Validation script (timm-style surface of MAP/validate.py / GA/train.py:validate): sums the head logits in fp32,
top-1/top-5 with bit-exact lowest-index tie-break, on the libgaext HIP kernels.  Synthetic data, or an image folder.

  python validate.py --synthetic --model ga_convnext_tiny_768 -b 256 --batches 10 [--checkpoint x.pth.tar] [--results-file r.json]
  python validate.py --synthetic --synthetic-source 375x500 --crop-pct 0.875 ...   decoded images: Resize + CenterCrop on the device
  python validate.py /data/imagenet --split validation --model map_resnet50 -b 256 -j 8    accuracy over exactly the folder's images
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

parser = argparse.ArgumentParser()
parser.add_argument('data', nargs='?', default='')
parser.add_argument('--model', '-m', default='ga_convnext_tiny_768')
parser.add_argument('-b', '--batch-size', type=int, default=256)
parser.add_argument('--batches', type=int, default=10)
parser.add_argument('--num-classes', type=int, default=None)
parser.add_argument('--checkpoint', default='')
parser.add_argument('--fp32', action='store_true')
parser.add_argument('--synthetic', action='store_true')
parser.add_argument('--split', default='validation', metavar='NAME', help='dataset split: a directory of the root (default: validation; '
                    'the root itself where it has no such directory)')
parser.add_argument('-j', '--workers', type=int, default=8, metavar='N', help='host threads of the JPEG entropy stage, at most 16')
parser.add_argument('--results-file', default='')
parser.add_argument('--crop-pct', type=float, default=0.875, help='centre-crop fraction of the evaluation transform: the short side '
                    'is resized to floor(img / crop_pct) (default: 0.875; used with --synthetic-source)')
parser.add_argument('--interpolation', type=str, default='bicubic', help='resize interpolation, bilinear or bicubic '
                    '(default: bicubic; used with --synthetic-source)')
parser.add_argument('--synthetic-source', type=str, default=None, metavar='HxW', help='evaluate on DECODED synthetic images (uint8 HWC, '
                    'heights and widths within [0.5, 1.5] of H and W): Resize + CenterCrop and the normalisation run on the device')


def validate_folder(args, A, model, img):
    """DIR[/split]/<class>/*: JpegDecoder -> ResizeCenterCrop -> the model, accuracy over exactly the folder's images"""
    try:
        crop = A.ResizeCenterCrop(img, args.crop_pct, args.interpolation)
        dataset = A.ImageFolder(A.split_dir(args.data, args.split))
    except (ValueError, OSError, RuntimeError) as e:
        raise SystemExit(f'validate.py: {e}')
    model = model.cuda().eval()
    if len(dataset.classes) > model.num_classes:
        raise SystemExit(f'validate.py: {len(dataset.classes)} class directories, the model has {model.num_classes} classes')
    decoder = A.JpegDecoder(threads=args.workers)
    loader = A.FolderLoader(dataset, args.batch_size, decoder, train=False)
    with torch.no_grad():
        model(torch.zeros(args.batch_size, 3, img, img, device='cuda'))       # warm-up (MAP/validate.py:240)
    torch.cuda.synchronize()
    t0 = time.time()
    counts = A.evaluate_folder(model, loader, crop)
    torch.cuda.synchronize()
    dt = time.time() - t0
    c1, c5, n = (int(v) for v in counts.tolist())
    res = dict(model=args.model, top1=round(100 * c1 / n, 4), top5=round(100 * c5 / n, 4),
               param_count=round(sum(p.numel() for p in model.parameters()) / 1e6, 2), img_per_sec=round(n / dt, 1), samples=n,
               classes=len(dataset.classes), pil_fallbacks=decoder.fallbacks)
    print(f' * Acc@1 {res["top1"]:.3f} Acc@5 {res["top5"]:.3f}  over {n} images ({res["img_per_sec"]:.1f} img/s)')
    print('--result\n' + json.dumps(res, indent=4))
    if args.results_file:
        json.dump(res, open(args.results_file, 'w'), indent=4)


def main():
    args = parser.parse_args()
    if not args.synthetic and not args.data:
        raise SystemExit('validate.py: only --synthetic data is shipped')
    import imagenet_models_amd as A
    # the model stays on the host until the crop is built from its input size: a flag the crop refuses ends the run before the device
    model = A.create_model(args.model, num_classes=args.num_classes, checkpoint_path=args.checkpoint,
                           math_mode='fp32' if args.fp32 else 'bf16')
    img = getattr(model, 'cfg', {}).get('img_size', 224)
    if not args.synthetic:
        return validate_folder(args, A, model, img)
    crop = source = None
    if args.synthetic_source:
        # decoded sources -> Resize + CenterCrop (ga_resize_crop) -> the uint8 batch, which the engine normalises with the model's
        # input statistics (ga_u8_normalize) as it does a loader's
        try:
            source = A.parse_hw(args.synthetic_source)
        except ValueError as e:
            raise SystemExit(str(e))
        try:
            crop = A.ResizeCenterCrop(img, args.crop_pct, args.interpolation)
        except ValueError as e:
            raise SystemExit(f'validate.py: --crop-pct / --interpolation: {e}')
    model = model.cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(0)
    n = c1 = c5 = 0
    with torch.no_grad():
        if source is not None:
            ragged = A.synthetic_ragged(args.batch_size, source, 0, 'cuda')
        model(torch.randn(args.batch_size, 3, img, img, device='cuda', generator=g))  # warm-up (MAP/validate.py:240)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.batches):
            x = crop(ragged) if source is not None else torch.randn(args.batch_size, 3, img, img, device='cuda', generator=g)
            y = torch.randint(0, model.num_classes, (args.batch_size,), device='cuda', generator=g)
            _, idx = A.heads_topk(model(x), 5)
            a1, a5 = A.accuracy_from_topk(idx, y, (1, 5))
            c1 += float(a1) * x.size(0) / 100
            c5 += float(a5) * x.size(0) / 100
            n += x.size(0)
        torch.cuda.synchronize()
        dt = time.time() - t0
    res = dict(model=args.model, top1=round(100 * c1 / n, 4), top5=round(100 * c5 / n, 4),
               param_count=round(sum(p.numel() for p in model.parameters()) / 1e6, 2), img_per_sec=round(n / dt, 1))
    print(f' * Acc@1 {res["top1"]:.3f} Acc@5 {res["top5"]:.3f}  ({res["img_per_sec"]:.1f} img/s)')
    print('--result\n' + json.dumps(res, indent=4))
    if args.results_file:
        json.dump(res, open(args.results_file, 'w'), indent=4)


if __name__ == '__main__':
    main()
