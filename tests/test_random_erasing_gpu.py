"""GPU: RandomErasing on the device (ga_input_erase, imagenet_models_amd.RandomErasing, TrainStep(random_erasing=...), train.py
--reprob) against the independent restatements of tests/_random_erasing_ref.py: a plain-Python sampler and a numpy
Philox4x32-10 + Box-Muller evaluated in float64 in the counter layout include/gaext.h documents.  timm is not installed and the
reference does not vendor it: parity with timm itself is unpinned (as for oracle/mixup_oracle.py); what is pinned is the kernel
against the documented generator, the untouched elements bit for bit against ga_u8_normalize, and the order of the step.

The cap on the noise is 1e-4 absolute: a wrong counter word, key word or output lane gives errors of order 1, fp32 logf / sqrtf /
sincospif rounding gives ~1e-6 (|n| <= 5.77, a few ulp of 4.8e-7 each)."""
import math
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _random_erasing_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)
CAP = 1e-4
SHAPES = [(8, 224, 224), (8, 160, 160), (8, 32, 48), (8, 6, 10)]       # 6 x 10: four-element spans that cross a row end


def _boxes(B, H, W):
    """boxes at the image border, overlapping ones (the later wins), widths / lefts that are not multiples of 4, a single pixel,
    three boxes on one sample, and seeded random ones; samples 4 and B-1.. stay clean"""
    bx = [(0, 0, 0, max(1, H // 3), W // 2 + 1),                                   # top-left corner
          (1, H - 5, W - 7, 5, 7),                                                 # bottom-right corner
          (2, 1, 2, H // 2, 5), (2, 1 + H // 4, 1, H // 3 + 1, W - 3),             # overlap
          (3, 1, 1, 1, 1),                                                         # one pixel
          (5, 0, 1, H - 1, W - 2), (5, 2, 3, 3, 5), (5, H // 2, 0, 2, W - 1)]      # three, nested and crossing
    rng = random.Random(H * 1000 + W)
    for _ in range(3):
        top, left = rng.randint(0, H - 1), rng.randint(0, W - 1)
        bx.append((6, top, left, rng.randint(1, H - top), rng.randint(1, W - left)))
    for _, top, left, h, w in bx:
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W and h > 0 and w > 0
    return bx


def _table(boxes, B, max_count):
    tab = torch.zeros(B, max(max_count, 1), 4, dtype=torch.int32)
    used = [0] * B
    for i, top, left, h, w in boxes:
        tab[i, used[i]] = torch.tensor([top, left, h, w], dtype=torch.int32)
        used[i] += 1
    return tab


def _launch(x, boxes, max_count, mode, seed, offset, mean=MEAN, std=STD):
    from imagenet_models_amd import ops
    xd = x.cuda()
    out = torch.empty(x.shape, dtype=torch.float32, device='cuda')
    tab = _table(boxes, x.shape[0], max_count).cuda() if max_count else None
    ops.Plan(eager=True).input_erase(xd, out, tab, max_count, R.MODES[mode], seed, offset, mean, std)
    assert torch.equal(xd.cpu(), x)                  # out of place: the caller's tensor is not modified
    return out.cpu()


def _inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8), torch.randn(B, 3, H, W, generator=g)


@pytest.mark.parametrize('shape', SHAPES)
def test_no_boxes_is_the_plain_normalisation_or_copy(shape):
    from imagenet_models_amd import ops
    B, H, W = shape
    x8, xf = _inputs(B, H, W)
    want = torch.empty(B, 3, H, W, device='cuda')
    ops.Plan(eager=True).u8_normalize(x8.cuda(), want, MEAN, STD)
    want = want.cpu()
    assert torch.equal(want, torch.from_numpy(R.normalize_u8(x8.numpy(), MEAN, STD)))
    for mode in ('const', 'rand', 'pixel'):
        for max_count in (0, 3):                     # no table at all / a table of unused slots (h == 0)
            assert torch.equal(_launch(x8, [], max_count, mode, 7, 0), want), (mode, max_count)
            assert torch.equal(_launch(xf, [], max_count, mode, 7, 0), xf), (mode, max_count)
    other = ((127.5, 100.0, 3.0), (64.0, 255.0, 1.5))
    assert torch.equal(_launch(x8, [], 3, 'pixel', 7, 0, *other), torch.from_numpy(R.normalize_u8(x8.numpy(), *other)))


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('mode', ['const', 'rand', 'pixel'])
@pytest.mark.parametrize('shape', SHAPES)
def test_fill_matches_the_restatement_and_the_rest_is_untouched(shape, mode, u8):
    """Measured on an MI355X, max |kernel - float64 restatement| inside the boxes: 'pixel' 5.7e-7 (224 x 224), 6.4e-7 (160 x 160),
    3.7e-7 (32 x 48), 2.1e-7 (6 x 10), the same for uint8 and fp32 input; 'rand' 1.1e-7; 'const' 0 -- two orders under the cap, what
    fp32 logf / sqrtf / sincospif rounding explains."""
    B, H, W = shape
    x8, xf = _inputs(B, H, W, seed=1)
    x = x8 if u8 else xf
    boxes, seed, offset = _boxes(B, H, W), 0x123456789ABCDEF, 3 + (5 << 32)      # 64-bit seed and offset words in use
    base = _launch(x, [], 3, mode, seed, offset)
    got = _launch(x, boxes, 3, mode, seed, offset)
    ref, mask = R.erase(base.numpy(), boxes, 3, mode, seed, offset)
    mask_t = torch.from_numpy(mask)
    assert mask.any() and not mask[4].any() and not mask[7].any()
    assert torch.equal(got[~mask_t], base[~mask_t])                              # bit-identical outside the boxes
    err = float(np.abs(got.numpy().astype(np.float64) - ref)[mask].max())
    print(f'input_erase {mode} {"u8" if u8 else "f32"} {shape}: max |err| inside the boxes {err:.3e}')
    assert err <= (0.0 if mode == 'const' else CAP), err
    if mode == 'const':
        assert (got[mask_t] == 0).all()
    if mode == 'rand':
        # one colour per (box, channel), bit-constant over what later boxes leave visible of it
        owner = np.full((B, H, W), -1)
        for k, (b, top, left, h, w) in enumerate(boxes):
            owner[b, top:top + h, left:left + w] = k
        for k, (b, *_r) in enumerate(boxes):
            vis = owner[b] == k
            if vis.any():
                for c in range(3):
                    assert np.unique(got[b, c].numpy()[vis]).size == 1, (k, c)
        assert np.unique(got.numpy()[mask]).size > len(boxes)                    # ... and different between boxes / channels
    if mode == 'pixel':
        # a different offset / seed is different noise; the same one reproduces bit for bit
        assert torch.equal(got, _launch(x, boxes, 3, mode, seed, offset))
        assert not torch.equal(got, _launch(x, boxes, 3, mode, seed, offset + 1))
        assert not torch.equal(got, _launch(x, boxes, 3, mode, seed + 1, offset))


def test_pixel_noise_statistics_and_fresh_noise_every_call():
    """B = 32 at 224 x 224, probability 1, 'pixel'.  min_area is raised to 0.15: with timm's default range [0.02, 1/3] the
    expected number of erased elements is 32 * 3 * 224^2 * 0.177 = 0.85e6, short of the 1e6 the bounds below are sized for
    (0.01 = 10 standard errors at N = 1e6); [0.15, 1/3] gives 1.16e6 expected."""
    import imagenet_models_amd as A
    B, H, W = 32, 224, 224
    kw = dict(probability=1.0, mode='pixel', min_area=0.15, seed=2024)
    era = A.RandomErasing(rng=random.Random(0), **kw)
    x = torch.zeros(B, 3, H, W, device='cuda')
    first = era(x).cpu()
    boxes = era.last_boxes
    assert boxes == R.sample_boxes(random.Random(0), B, H, W, probability=1.0, min_area=0.15)[0] and len(boxes) == B
    assert era.offset == 1
    mask = torch.zeros(B, 3, H, W, dtype=torch.bool)
    for b, top, left, h, w in boxes:
        mask[b, :, top:top + h, left:left + w] = True
    n = int(mask.sum())
    assert n > 1_000_000, n
    assert (first[~mask] == 0).all()
    a = first[mask].double()
    print(f'pixel noise over {n} elements: mean {float(a.mean()):+.2e}, std - 1 {float(a.std()) - 1:+.2e}, max |n| {float(a.abs().max()):.3f}')
    assert abs(float(a.mean())) < 0.01 and abs(float(a.std()) - 1) < 0.01
    assert float(a.abs().max()) <= math.sqrt(48 * math.log(2)) + 1e-5
    # the next call of the object on the same boxes: offset 1 -- uncorrelated with the first
    second = _launch(x.cpu(), boxes, 1, 'pixel', 2024, 1)
    b = second[mask].double()
    corr = float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))
    print(f'correlation of the noise of two consecutive calls: {corr:+.2e}')
    assert abs(corr) < 0.01
    # what the object itself launches on its second call is that offset (with the boxes it then draws)
    again = era(x).cpu()
    assert era.offset == 2 and torch.equal(again, _launch(x.cpu(), era.last_boxes, 1, 'pixel', 2024, 1))
    # the same (seed, offset) reproduces bit-identically across launches; the output buffer is reused, not re-allocated
    assert torch.equal(_launch(x.cpu(), boxes, 1, 'pixel', 2024, 0), first)
    assert torch.equal(_launch(x.cpu(), boxes, 1, 'pixel', 2024, 0), first)
    p0 = era(x).data_ptr()
    assert era(x).data_ptr() == p0


def test_object_on_uint8_and_fp32_batches():
    import imagenet_models_amd as A
    x8, xf = _inputs(8, 160, 160, seed=3)
    for mode in ('const', 'rand', 'pixel'):
        kw = dict(probability=0.6, mode=mode, min_count=1, max_count=3, seed=5)
        era = A.RandomErasing(rng=random.Random(9), **kw)
        ref_rng = random.Random(9)
        for step, x in enumerate((x8, xf, x8)):
            keep = x.clone()
            xd = x.cuda()
            got = (era(xd, MEAN, STD) if x.dtype == torch.uint8 else era(xd)).cpu()
            assert torch.equal(xd.cpu(), keep)
            boxes, _ = R.sample_boxes(ref_rng, 8, 160, 160, probability=0.6, min_count=1, max_count=3)
            assert era.last_boxes == boxes and era.offset == step + 1
            base = torch.from_numpy(R.normalize_u8(x.numpy(), MEAN, STD)) if x.dtype == torch.uint8 else x
            ref, mask = R.erase(base.numpy(), boxes, 3, mode, 5, step)
            mask_t = torch.from_numpy(mask)
            assert torch.equal(got[~mask_t], base[~mask_t])
            assert mask.any() and float(np.abs(got.numpy().astype(np.float64) - ref)[mask].max()) <= CAP
    with pytest.raises(ValueError, match='mean / std'):
        era(x8.cuda())
    with pytest.raises(TypeError):
        era(xf.cuda().half())


def _small_step(random_erasing=None, mixup_fn=None, stats=None):
    import imagenet_models_amd as A
    torch.manual_seed(0)
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    if stats is not None:
        m.input_mean, m.input_std = stats
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    return A.TrainStep(m, opt, 4, lam=0.0, random_erasing=random_erasing, mixup_fn=mixup_fn)


@pytest.mark.parametrize('stats', [None, ((120.0, 110.0, 100.0), (60.0, 64.0, 70.0))])
def test_train_step_erases_the_normalised_uint8_batch(stats):
    """TrainStep(random_erasing=...), uint8 input, B = 4: the engine's input is normalise -> erase of the restatement with the
    same boxes and generator, bit-exact outside the boxes and within the cap inside; the model's input_mean / input_std count"""
    import imagenet_models_amd as A
    mean, std = stats or (MEAN, STD)
    x8, _ = _inputs(4, 224, 224, seed=4)
    t = torch.tensor([3, 17, 5, 39])
    kw = dict(probability=1.0, mode='pixel', max_count=2, seed=11)
    era = A.RandomErasing(rng=random.Random(5), **kw)
    step = _small_step(random_erasing=era, stats=stats)
    ref_rng = random.Random(5)
    for k in range(2):                                   # the second step: the next boxes, offset 1
        loss = step(x8.cuda(), t.cuda())
        assert math.isfinite(float(loss))
        boxes, _ = R.sample_boxes(ref_rng, 4, 224, 224, probability=1.0, min_count=1, max_count=2)
        assert era.last_boxes == boxes and era.offset == k + 1
        base = R.normalize_u8(x8.numpy(), mean, std)
        ref, mask = R.erase(base, boxes, 2, 'pixel', 11, k)
        got = step.eng.x_ref.cpu().numpy()
        assert mask.any() and np.array_equal(got[~mask], base[~mask])
        err = float(np.abs(got.astype(np.float64) - ref)[mask].max())
        assert err <= CAP, err


def test_train_step_order_is_normalise_erase_mixup():
    """with a mixup_fn as well, the engine's input is oracle.mixup_oracle.Mixup (same numpy seed) of the erased batch; without
    random_erasing the step's input is what it was: the normalised batch, or Mixup of it"""
    import imagenet_models_amd as A
    from oracle import mixup_oracle as MO
    x8, _ = _inputs(4, 224, 224, seed=6)
    t = torch.tensor([3, 17, 5, 39])
    norm = torch.from_numpy(R.normalize_u8(x8.numpy(), MEAN, STD))
    mkw = dict(mixup_alpha=0.2, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=40)
    ekw = dict(probability=1.0, mode='pixel', max_count=2, seed=11)
    erased = A.RandomErasing(rng=random.Random(5), **ekw)(x8.cuda(), MEAN, STD).cpu().clone()
    assert not torch.equal(erased, norm)
    # erase + mixup
    step = _small_step(random_erasing=A.RandomErasing(rng=random.Random(5), **ekw), mixup_fn=A.Mixup(rng=np.random.RandomState(7), **mkw))
    assert math.isfinite(float(step(x8.cuda(), t.cuda())))
    rx, _ = MO.Mixup(rng=np.random.RandomState(7), **mkw)(erased, t)
    assert torch.equal(step.eng.x_ref.cpu(), rx) and not torch.equal(rx, erased)
    # erase alone: the erased batch reaches the engine as it is
    step = _small_step(random_erasing=A.RandomErasing(rng=random.Random(5), **ekw))
    step(x8.cuda(), t.cuda())
    assert torch.equal(step.eng.x_ref.cpu(), erased)
    # no random_erasing: unchanged paths
    step = _small_step()
    step(x8.cuda(), t.cuda())
    assert torch.equal(step.eng.x_ref.cpu(), norm)
    step = _small_step(mixup_fn=A.Mixup(rng=np.random.RandomState(7), **mkw))
    step(x8.cuda(), t.cuda())
    rx, _ = MO.Mixup(rng=np.random.RandomState(7), **mkw)(norm, t)
    assert torch.equal(step.eng.x_ref.cpu(), rx)


def test_train_cli_runs_with_random_erasing():
    cmd = [sys.executable, 'train.py', '--synthetic', '--model', 'map_convnext_tiny', '-b', '8', '--epochs', '1', '--steps-per-epoch', '2',
           '--reprob', '1.0', '--remode', 'pixel', '--recount', '2']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)       # a child process under its own time limit
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    m = re.search(r'\*\*\* epoch 0: train loss (\S+)', out)
    assert m and math.isfinite(float(m.group(1))), out[-2000:]
