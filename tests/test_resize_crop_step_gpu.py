"""GPU: the Python surface of the on-device resize and crop (imagenet_models_amd.pack_images / RandomResizedCrop / ResizeCenterCrop,
TrainStep(crop=...)) against the numpy restatement of tests/_resize_crop_ref.py applied to the objects' own tables, alone and ahead
of the existing input stages.  Every pixel gate is equality."""
import math
import random

import numpy as np
import pytest
import torch

import _rand_augment_ref as RA
import _resize_crop_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(120, 96), (75, 131), (224, 224), (301, 97)]


def _sources(seed=0):
    return [R.source(H, W, seed + k) for k, (H, W) in enumerate(SHAPES)]


def _small_step(**kw):
    import imagenet_models_amd as A
    torch.manual_seed(0)
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    return A.TrainStep(m, opt, 4, lam=0.0, **kw)


def test_pack_images_lays_the_sources_out_on_16_byte_starts():
    import imagenet_models_amd as A
    images = _sources()
    for _ in range(6):                                           # more calls than staging buffers: a slot is reused
        rb = A.pack_images(images)
    assert isinstance(rb, A.RaggedBatch) and len(rb) == 4 and rb.data.is_cuda and rb.data.dtype == torch.uint8
    assert (rb.offsets % 16 == 0).all() and rb.heights.tolist() == [s[0] for s in SHAPES] and rb.widths.tolist() == [s[1] for s in SHAPES]
    host = rb.data.cpu().numpy()
    for im, o in zip(images, rb.offsets):
        assert np.array_equal(host[o:o + im.size].reshape(im.shape), im)
    with pytest.raises(TypeError):
        A.pack_images([images[0].astype(np.float32)])
    with pytest.raises(TypeError):
        A.pack_images([images[0][:, :, 0]])


def test_transforms_equal_the_restatement_of_their_own_tables():
    import imagenet_models_amd as A
    images = _sources(3)
    rb = A.pack_images(images)
    rrc = A.RandomResizedCrop(64, rng=random.Random(1), torch_gen=torch.Generator().manual_seed(1))
    for _ in range(6):                                           # the table staging rotates; the generators go on
        out = rrc(rb)
        tab = rrc.last
        assert out.shape == (4, 3, 64, 64) and out.dtype == torch.uint8 and tab.shape == (4,) and (tab['src_off'] == rb.offsets).all()
        assert np.array_equal(out.cpu().numpy(), R.resize_crop(images, tab, 64, 64)), tab.tolist()
    seen = rrc.sample(rb.heights, rb.widths, rb.offsets)
    assert np.array_equal(rrc(rb, table=seen).cpu().numpy(), R.resize_crop(images, seen, 64, 64))
    for pct, interpolation in ((0.875, 'bicubic'), (0.95, 'bilinear'), (1.0, 'bicubic')):
        rcc = A.ResizeCenterCrop(64, pct, interpolation)
        out = rcc(rb)
        assert rcc.last.tobytes() == R.eval_table(rb.heights, rb.widths, 64, pct, interpolation, rb.offsets).tobytes()
        assert np.array_equal(out.cpu().numpy(), R.resize_crop(images, rcc.last, 64, 64)), (pct, interpolation)
    bad = seen.copy()
    bad[2]['left'] = 200
    with pytest.raises(RuntimeError, match='box outside its image'):
        rrc(rb, table=bad)
    with pytest.raises(TypeError, match='RaggedBatch'):
        rrc(rb.data)


def test_crop_then_rand_augment_then_collate_mixup():
    """crop -> RandAugment -> FastCollateMixup in sequence equals the two existing stages fed the restatement's uint8 batch: seeds and
    tables from the objects, the normalised fp32 input compared bit for bit"""
    import imagenet_models_amd as A
    from imagenet_models_amd import ops
    images = _sources(7)
    rb = A.pack_images(images)
    t = torch.tensor([3, 17, 5, 39])
    rrc = A.RandomResizedCrop(224, rng=random.Random(4), torch_gen=torch.Generator().manual_seed(4))
    ra = A.RandAugment('rand-m9-mstd0.5-inc1-p1.0', rng=random.Random(8), np_rng=np.random.RandomState(8))
    fm = A.FastCollateMixup(mode='elem', label_smoothing=0.1, num_classes=40, rng=np.random.RandomState(7), mixup_alpha=0.8, cutmix_alpha=1.0)
    step = _small_step(crop=rrc, auto_augment=ra, collate_mixup=fm)
    loss = step(rb, t.cuda())
    assert math.isfinite(float(loss))
    got = step.eng.x_ref.clone()
    cropped = R.resize_crop(images, rrc.last, 224, 224)
    aug = RA.rand_augment(cropped, ra.last)
    assert (aug != cropped).any()
    want = torch.empty(4, 3, 224, 224, device='cuda')
    mean, std = step.eng.input_stats()
    ops.Plan(eager=True).input_collate(torch.from_numpy(aug).cuda(), want, torch.from_numpy(fm.last).cuda(), None, 0, 0, 0, 0, mean, std)
    torch.cuda.synchronize()
    assert torch.equal(got, want), int((got != want).sum())


def test_train_step_with_and_without_crop():
    import imagenet_models_amd as A
    images = _sources(9)
    rb = A.pack_images(images)
    t = torch.tensor([3, 17, 5, 39]).cuda()
    rrc = A.RandomResizedCrop(224, rng=random.Random(5), torch_gen=torch.Generator().manual_seed(5))
    step = _small_step(crop=rrc)
    loss = step(rb, t)
    assert math.isfinite(float(loss))
    cropped = torch.from_numpy(R.resize_crop(images, rrc.last, 224, 224)).cuda()
    # crop=None on the same uint8 batch: the step is what it was, and its engine input is the same
    ref = _small_step()
    assert ref.crop is None
    ref_loss = ref(cropped, t)
    assert torch.equal(step.eng.x_ref, ref.eng.x_ref) and math.isfinite(float(ref_loss))
    with pytest.raises(TypeError, match='takes a RaggedBatch'):
        step(cropped, t)
    with pytest.raises(TypeError, match='RaggedBatch needs TrainStep'):
        ref(rb, t)
