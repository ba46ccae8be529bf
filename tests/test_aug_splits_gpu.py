"""GPU: augmentation splits (imagenet_models_amd.AugSplits, TrainStep(aug_splits=...)) and the JSD step (TrainStep(loss='jsd')).
The pixels of every split are gated by equality: split 0 against the input, split j against RandAugment applied to the input with
the rows of split j of AugSplits' own table; the erased batch against ga_u8_normalize on the clean split.  The step's loss and
d(logits) are gated by tests/_loss_jsd_ref.py's closed form evaluated on the engine's own logits, with the kernel test's gate."""
import math
import random

import numpy as np
import pytest
import torch

import _loss_jsd_ref as J
import _resize_crop_ref as R

pytestmark = pytest.mark.gpu

MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)
AA = 'rand-m9-mstd0.5-inc1-p1.0'


def _ra(seed):
    import imagenet_models_amd as A
    return A.RandAugment(AA, rng=random.Random(seed), np_rng=np.random.RandomState(seed))


def test_splits_are_the_clean_batch_and_rand_augment_of_it():
    import imagenet_models_amd as A
    from imagenet_models_amd import ops, rand_augment as RA
    b, S = 4, 3
    x = torch.randint(0, 256, (b, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    y = torch.tensor([3, 17, 5, 39]).cuda()
    keep = x.clone()
    sp, ra = A.AugSplits(S), _ra(8)
    out, tgt = sp(x, y, ra)
    assert out.shape == (S * b, 3, 32, 32) and out.dtype == torch.uint8 and torch.equal(x, keep)
    assert torch.equal(tgt, y.repeat(S)) and tgt.dtype == torch.int64
    out = out.clone()
    tab = sp.last
    assert tab.shape == (S * b, ra.num_layers) and (tab[:b]['kind'] == RA.NONE).all() and (tab[b:]['kind'] != RA.NONE).any()
    assert torch.equal(out[:b], x)                                         # the clean split: the bytes of the input
    other = _ra(0)
    for j in range(1, S):
        want = other(x, table=tab[j * b:(j + 1) * b])
        assert torch.equal(out[j * b:(j + 1) * b], want), j
        assert not torch.equal(want, x)
    assert not torch.equal(out[b:2 * b], out[2 * b:])                      # independent draws per split
    p0 = (sp(x, y, ra)[0].data_ptr(), tgt.data_ptr())                      # the buffers are reused from call to call
    o2, t2 = sp(x, y, ra)
    assert (o2.data_ptr(), t2.data_ptr()) == p0
    # RandomErasing(num_splits = S) leaves the clean split alone: there the pass is the plain normalisation, bit for bit
    era = A.RandomErasing(probability=1.0, mode='pixel', num_splits=S, seed=5, rng=random.Random(2))
    got = era(out, MEAN, STD)
    plain = torch.empty(S * b, 3, 32, 32, device='cuda')
    ops.Plan(eager=True).u8_normalize(out, plain, MEAN, STD)
    torch.cuda.synchronize()
    assert torch.equal(got[:b], plain[:b])
    assert sorted({bx[0] for bx in era.last_boxes}) == list(range(b, S * b))
    for i in range(b, S * b):
        assert not torch.equal(got[i], plain[i]), i
    # without auto_augment the splits are plain copies (the reference with --aa '')
    out3, tgt3 = A.AugSplits(2)(x, y)
    assert torch.equal(out3, torch.cat([x, x])) and torch.equal(tgt3, y.repeat(2))
    with pytest.raises(TypeError, match='AugSplits expects a uint8'):
        sp(x.float(), y, ra)
    with pytest.raises(ValueError, match='targets for a batch'):
        sp(x, y[:3], ra)


def test_all_splits_come_from_one_crop_of_a_ragged_batch():
    import imagenet_models_amd as A
    images = [R.source(H, W, 20 + k) for k, (H, W) in enumerate([(60, 48), (37, 66), (64, 64), (90, 41)])]
    rb = A.pack_images(images)
    y = torch.tensor([1, 2, 3, 4]).cuda()
    rrc = A.RandomResizedCrop(48, rng=random.Random(4), torch_gen=torch.Generator().manual_seed(4))
    sp, ra = A.AugSplits(3), _ra(6)
    stage = A.InputStage(crop=rrc, auto_augment=ra, aug_splits=sp)
    assert stage.takes == 'ragged'
    x, t = stage(rb, y, None)
    assert rrc.last.shape == (4,) and x.shape == (12, 3, 48, 48) and torch.equal(t, y.repeat(3))
    x = x.clone()
    cropped = torch.from_numpy(R.resize_crop(images, rrc.last, 48, 48)).cuda()
    assert torch.equal(x[:4], cropped)
    other = _ra(0)
    for j in (1, 2):
        assert torch.equal(x[4 * j:4 * j + 4], other(cropped, table=sp.last[4 * j:4 * j + 4])), j
    with pytest.raises(TypeError, match='takes a RaggedBatch'):
        stage(cropped, y, None)


@pytest.mark.parametrize('name', ['map_convnext_tiny', 'ga_convnext_tiny_768'])
def test_jsd_train_step_meets_the_kernel_gate_on_the_engines_logits(name):
    import imagenet_models_amd as A
    torch.manual_seed(0)
    S, b, NC, lam, smooth = 3, 2, 16, -0.8, 0.1       # 16 classes: both engines take a num_classes that is a multiple of 8 only
    m = A.create_model(name, num_classes=NC, math_mode='fp32').cuda().train()
    opt = A.create_optimizer_v2(m, opt='adamw', lr=1e-3, weight_decay=0.05)
    sp, ra = A.AugSplits(S), _ra(9)
    era = A.RandomErasing(probability=1.0, mode='pixel', num_splits=S, seed=3, rng=random.Random(3))
    step = A.TrainStep(m, opt, S * b, lam=lam, loss='jsd', smoothing=smooth, aug_splits=sp, auto_augment=ra, random_erasing=era)
    assert step.input_stage.takes == 'uint8' and step.num_splits == S
    x = torch.randint(0, 256, (b, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    y = torch.tensor([15, 2]).cuda()
    loss = step(x, y)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss))
    assert step.eng.x_ref.shape[0] == S * b
    org, avg, dorg, davg, K = step.eng._loss_operands()
    assert org.shape == (K, S * b, NC) and (avg is not None) == name.startswith('map_')
    c = J.JsdCase(K, b, S, NC, smooth, avg is not None, 1.0, 'engine', 0)
    c.lam = lam
    i = dict(org=org.double().cpu(), avg=None if avg is None else avg.double().cpu(), target=y.cpu(), initial=0.0)
    ref = J.JsdRef(i, c)
    assert int(ref.near_clamp().sum()) == 0
    dt = dorg.dtype
    got = dict(loss=float(loss), dorg=dorg.double().cpu().view(K, S * b, NC), davg=None if davg is None else davg.double().cpu().view(K, S * b, NC))
    ratios = J.jsd_ratios(got, ref.out, dt, 1.0)
    print(f'[{name}] K {K} loss {float(loss):.6f} (closed form {float(ref.out["loss"][0]):.6f}: jsd {float(ref.parts["jsd"]):.4f} ce '
          f'{float(ref.parts["ce"]):.4f} decor + avg {float(ref.parts["decor"]):.4f})  err / allowed ' + '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    assert max(ratios.values()) < 1.0, ratios
    assert float(ref.parts['jsd']) > 0                 # the splits differ: the consistency term is live
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_train_step_refusals_say_why():
    import imagenet_models_amd as A
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    sp = A.AugSplits(3)
    mkw = dict(mixup_alpha=0.2, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=40)
    with pytest.raises(ValueError, match="loss='jsd' is the consistency loss over augmentation splits"):
        A.TrainStep(m, opt, 6, loss='jsd')
    with pytest.raises(ValueError, match='aug_splits cannot be combined with mixup_fn / collate_mixup'):
        A.TrainStep(m, opt, 6, loss='jsd', aug_splits=sp, mixup_fn=A.Mixup(**mkw))
    with pytest.raises(ValueError, match='aug_splits cannot be combined with mixup_fn / collate_mixup'):
        A.TrainStep(m, opt, 6, aug_splits=sp, collate_mixup=A.FastCollateMixup(**mkw))
    with pytest.raises(ValueError, match='num_splits = 2 does not match aug_splits'):
        A.TrainStep(m, opt, 6, loss='jsd', aug_splits=sp, random_erasing=A.RandomErasing(probability=1.0, num_splits=2))
    with pytest.raises(ValueError, match='not a multiple of the 3'):
        A.TrainStep(m, opt, 8, loss='jsd', aug_splits=sp)
    # --aug-splits without --jsd-loss: the ordinary loss over all rows with the repeated targets
    step = A.TrainStep(m, opt, 6, lam=0.0, aug_splits=sp, auto_augment=_ra(1))
    x = torch.randint(0, 256, (2, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    assert math.isfinite(float(step(x, torch.tensor([3, 17]).cuda())))
    with pytest.raises(ValueError, match="kind='jsd' needs num_splits >= 2"):
        A.ga_loss([torch.zeros(6, 10, device='cuda')], torch.zeros(6, dtype=torch.int64, device='cuda'), kind='jsd')


def test_python_losses_equal_the_closed_form():
    """ga_loss / map_loss(kind='jsd') through their autograd wrappers: value and gradient against the closed form"""
    import imagenet_models_amd as A
    c = J.JSD_CASES[9]                                   # K5 Bs3 S3 NC1000 avg randn8
    i = J.jsd_inputs(c)
    ref = J.JsdRef(i, c)
    c1 = J.JsdCase(c.K, c.Bs, c.S, c.NC, c.smooth, c.avg, 1.0, c.regime, c.seed)
    ref1 = J.JsdRef(dict(i, initial=0.0), c1)
    org = [i['org'][k].float().cuda().requires_grad_(True) for k in range(c.K)]
    avg = [i['avg'][k].float().cuda().requires_grad_(True) for k in range(c.K)]
    tgt = i['target'].repeat(c.S).cuda()
    loss = A.map_loss([[o, a] for o, a in zip(org, avg)], tgt, c.lam, kind='jsd', smoothing=c.smooth, num_splits=c.S)
    loss.backward()
    got = dict(loss=float(loss), dorg=torch.stack([o.grad for o in org]).double().cpu(), davg=torch.stack([a.grad for a in avg]).double().cpu())
    ratios = J.jsd_ratios(got, ref1.out, J.F32, 1.0)
    assert max(ratios.values()) < 1.0, ratios
    # the GA loss is the same call without the avg logits
    c2 = J.JsdCase(c.K, c.Bs, c.S, c.NC, c.smooth, False, 1.0, c.regime, c.seed)
    ref2 = J.JsdRef(dict(i, avg=None, initial=0.0), c2)
    org2 = [i['org'][k].float().cuda().requires_grad_(True) for k in range(c.K)]
    l2 = A.ga_loss(org2, i['target'].cuda(), c.lam, kind='jsd', smoothing=c.smooth, num_splits=c.S, jsd_alpha=12.0)
    l2.backward()
    got2 = dict(loss=float(l2), dorg=torch.stack([o.grad for o in org2]).double().cpu(), davg=None)
    ratios2 = J.jsd_ratios(got2, ref2.out, J.F32, 1.0)
    assert max(ratios2.values()) < 1.0, ratios2
    with pytest.raises(TypeError, match='no dense-target'):
        A.ga_loss(org2, torch.zeros(c.B, c.NC, device='cuda'), kind='jsd', num_splits=c.S)
    del ref
