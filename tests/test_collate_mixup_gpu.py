"""GPU: the collate-time mixup order as one fused pass (ga_input_collate, ga_mixup_target_elem, imagenet_models_amd.FastCollateMixup,
TrainStep(collate_mixup=...), train.py --collate-mixup) against the independent restatement of tests/_collate_mixup_ref.py.

Every gate on the mixed pixels and on the targets is EQUALITY: a mixed value is an integer 0..255 pushed through the arithmetic
ga_u8_normalize already reproduces bit for bit, or a three-rounding fp32 expression; the fused erase is compared bit for bit
with ga_input_erase run on the restatement's mixed uint8 batch.  Only the TrainStep test measures the noise inside the erase
boxes against the float64 generator, under the 1e-4 cap of tests/test_random_erasing_gpu.py.  timm is not installed: parity with
timm itself is unpinned."""
import math
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _collate_mixup_ref as CM
import _random_erasing_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)
CAP = 1e-4
GA_ERR_BAD_ARG = -1                                      # include/gaext.h


def _f32bits(v):
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


def _row(kind, box=(0, 0, 0, 0), l=1.0, m=0.0):
    return [kind, *box, _f32bits(l), _f32bits(m), 0]


def _erase_table(boxes, B, max_count):
    tab = torch.zeros(B, max(max_count, 1), 4, dtype=torch.int32)
    used = [0] * B
    for i, top, left, h, w in boxes:
        tab[i, used[i]] = torch.tensor([top, left, h, w], dtype=torch.int32)
        used[i] += 1
    return tab


def _collate(x, tab, boxes=None, max_count=0, mode='const', seed=0, offset=0, mean=MEAN, std=STD):
    """launch ga_input_collate on the CPU tensor x (uint8 or fp32) with the numpy mix table; the input must come back unchanged"""
    from imagenet_models_amd import ops
    xd = x.cuda()
    out = torch.full(x.shape, float('nan'), dtype=torch.float32, device='cuda')
    mix = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.int32)).cuda()
    bt = _erase_table(boxes, x.shape[0], max_count).cuda() if max_count else None
    ops.Plan(eager=True).input_collate(xd, out, mix, bt, max_count, R.MODES[mode], seed, offset, mean, std)
    assert torch.equal(xd.cpu(), x)                  # out of place: the caller's tensor is not modified
    return out.cpu()


def _erase(x, boxes, max_count, mode, seed, offset):
    from imagenet_models_amd import ops
    out = torch.empty(x.shape, dtype=torch.float32, device='cuda')
    bt = _erase_table(boxes, x.shape[0], max_count).cuda() if max_count else None
    ops.Plan(eager=True).input_erase(x.cuda(), out, bt, max_count, R.MODES[mode], seed, offset, MEAN, STD)
    return out.cpu()


def _inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8), torch.randn(B, 3, H, W, generator=g)


def _norm(x8):
    return torch.from_numpy(R.normalize_u8(x8, MEAN, STD))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. every byte pair
# ---------------------------------------------------------------------------------------------------------------------------
def _pair_lams():
    sens, count = CM.contraction_sensitive_lam()
    assert sens is not None and count >= 1
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    beta = float(np.random.RandomState(11).beta(0.8, 0.8))
    return [0.5, sens, below_one, 1e-8, beta]


@pytest.mark.parametrize('form', ['batch', 'elem'])
@pytest.mark.parametrize('which', range(5))
def test_mixup_of_all_byte_pairs(which, form):
    """B = 4 at 256 x 256: sample 0 holds a = y, its partner (sample 3) b = x, so the two of them run every (a, b) and every (b, a);
    samples 1 and 2 are random.  The complement is formed as numpy forms it for a scalar lam ('batch': in double) and for a lam
    vector ('elem': in fp32).  A contracted blend fails this at the contraction-sensitive lam."""
    lam = _pair_lams()[which]
    x8, _ = _inputs(4, 256, 256, seed=2)
    ys, xs = torch.meshgrid(torch.arange(256), torch.arange(256), indexing='ij')
    x8[0] = ys.to(torch.uint8)
    x8[3] = xs.to(torch.uint8)
    l = np.float32(lam)
    m = np.float32(1.0 - lam) if form == 'batch' else np.float32(1) - l
    tab = np.array([_row(CM.MIXUP, l=l, m=m)] * 4, dtype=np.int32)
    ref = CM.mix_u8(x8.numpy(), tab)
    a, b = CM.all_byte_pairs()
    assert np.array_equal(ref[0, 0], CM.blend_u8(a, b, l, m)) and np.array_equal(ref[3, 1], CM.blend_u8(b, a, l, m))
    got = _collate(x8, tab)
    assert torch.equal(got, _norm(ref)), (lam, form, int((got != _norm(ref)).sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. cutmix geometry, mixed kinds in one launch
# ---------------------------------------------------------------------------------------------------------------------------
def _geometry_table(B, H, W):
    rows = [_row(CM.CUTMIX, (0, max(1, H // 3), 0, W // 2 + 1)),               # top-left corner
            _row(CM.CUTMIX, (H - 5, H, W - 7, W)),                             # bottom-right corner
            _row(CM.CUTMIX, (1, H - 1, 3, 8)),                                 # left and width no multiples of 4
            _row(CM.CUTMIX, (1, 2, 1, 2)),                                     # one pixel
            _row(CM.CUTMIX, (2, 2, 3, 3)),                                     # empty
            _row(CM.CUTMIX, (0, H, 0, W)),                                     # the whole image
            _row(CM.NONE),
            _row(CM.MIXUP, l=0.3, m=np.float32(1) - np.float32(0.3))]
    if B == 2:
        rows = [rows[2], rows[7]]
    return np.array(rows, dtype=np.int32)


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('shape', [(8, 6, 10), (8, 32, 48), (8, 160, 160), (2, 6, 10), (2, 32, 48)])
def test_cutmix_geometry_and_mixed_kinds(shape, u8):
    """6 x 10: four-element spans that cross a row end.  Neighbouring samples run 'none', 'mixup' and 'cutmix' in one launch."""
    B, H, W = shape
    x8, xf = _inputs(B, H, W, seed=3)
    tab = _geometry_table(B, H, W)
    if u8:
        ref = CM.mix_u8(x8.numpy(), tab)
        assert B == 2 or (np.array_equal(ref[5], x8.numpy()[2]) and np.array_equal(ref[4], x8.numpy()[4]))
        assert torch.equal(_collate(x8, tab), _norm(ref))
    else:
        ref = CM.mix_f32(xf.numpy(), tab)
        assert torch.equal(_collate(xf, tab), torch.from_numpy(ref))
    # the swapped roles: every box on the partner's side of the batch as well
    tab = tab[::-1].copy()
    if u8:
        assert torch.equal(_collate(x8, tab), _norm(CM.mix_u8(x8.numpy(), tab)))
    else:
        assert torch.equal(_collate(xf, tab), torch.from_numpy(CM.mix_f32(xf.numpy(), tab)))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. 'pair' (and 'elem', 'batch') through the object
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['pair', 'elem', 'batch'])
def test_object_on_uint8_batches(mode):
    """FastCollateMixup on a uint8 batch: table, pixels and dense target equal the restatement's for the same numpy seed.  In
    'pair' mode sample j = B-1-i blends with the SAME l on its own bytes and swaps the same box; rows with lam = 1 are
    bit-identical to ga_u8_normalize."""
    import imagenet_models_amd as A
    from imagenet_models_amd import ops
    B, H, W, NC = 8, 32, 48, 37
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.6)
    fm = A.FastCollateMixup(mode=mode, label_smoothing=0.1, num_classes=NC, rng=np.random.RandomState(5), **kw)
    ref_rng = np.random.RandomState(5)
    kinds = set()
    for step in range(6):
        x8, _ = _inputs(B, H, W, seed=10 + step)
        t = torch.randint(0, NC, (B,), generator=torch.Generator().manual_seed(step))
        gx, gt = fm(x8.cuda(), t.cuda(), None, MEAN, STD)
        tab, lam = CM.sample_table(ref_rng, B, H, W, mode=mode, **kw)
        assert np.array_equal(fm.last, tab)
        ref = CM.mix_u8(x8.numpy(), tab)
        assert torch.equal(gx.cpu(), _norm(ref)), (mode, step)
        assert torch.equal(gt.cpu(), CM.dense_target(t, NC, lam, 0.1)), (mode, step)
        assert torch.allclose(gt.sum(1).cpu(), torch.ones(B), atol=1e-6)
        plain = torch.empty(B, 3, H, W, device='cuda')
        ops.Plan(eager=True).u8_normalize(x8.cuda(), plain, MEAN, STD)
        l, m = CM.table_lm(tab)
        for i in range(B):
            j = B - 1 - i
            if l[i] == 1:
                assert torch.equal(gx[i], plain[i])
            if mode == 'pair':
                assert np.array_equal(tab[i], tab[j])
                if tab[i, 0] == CM.MIXUP:                    # mixed_j: l on ITS OWN bytes, m on sample i's
                    assert np.array_equal(ref[j], CM.blend_u8(x8.numpy()[j], x8.numpy()[i], l[i], m[i]))
        kinds.update(int(k) for k in tab[:, 0])
    assert kinds == {CM.NONE, CM.MIXUP, CM.CUTMIX}, kinds
    fm.mixup_enabled = False                             # --mixup-off-epoch: all 'none' rows, one-hot-smoothed targets
    gx, gt = fm(x8.cuda(), t.cuda(), None, MEAN, STD)
    assert (fm.last[:, 0] == CM.NONE).all() and torch.equal(gx, plain)
    assert torch.equal(gt.cpu(), CM.dense_target(t, NC, 1.0, 0.1))
    with pytest.raises(ValueError, match='mean / std'):
        fm(x8.cuda(), t.cuda())
    with pytest.raises(TypeError):
        fm(x8.cuda().half(), t.cuda())


# ---------------------------------------------------------------------------------------------------------------------------
# 4. fused erase
# ---------------------------------------------------------------------------------------------------------------------------
def _erase_boxes(B, H, W, max_count):
    """sample b carries b % (max_count + 1) boxes (so 0 .. max_count of them), seeded; sample 1's first box overlaps its cutmix box"""
    rng = random.Random(H * 100 + W + max_count)
    bx = []
    for b in range(B):
        for k in range(b % (max_count + 1)):
            top, left = rng.randint(0, H - 2), rng.randint(0, W - 2)
            bx.append((b, top, left, rng.randint(1, H - 1 - top), rng.randint(1, W - 1 - left)))
    return bx


@pytest.mark.parametrize('max_count', [1, 3, 6])
@pytest.mark.parametrize('mode', ['const', 'rand', 'pixel'])
@pytest.mark.parametrize('shape', [(8, 32, 48), (8, 6, 10)])
def test_fused_erase_is_input_erase_of_the_mixed_batch(shape, mode, max_count):
    """normalise and erase of the fused pass are ga_input_erase's, bit for bit, on the separately mixed uint8 batch: same boxes,
    seed, offset (64-bit words in use).  max_count 6 is the generic (looped) box path."""
    B, H, W = shape
    x8, _ = _inputs(B, H, W, seed=4)
    tab = _geometry_table(B, H, W)
    tab[6] = _row(CM.MIXUP, l=0.6899998188018799, m=np.float32(1) - np.float32(0.6899998188018799))
    boxes = _erase_boxes(B, H, W, max_count)
    boxes[0] = (1, H - 4, W - 6, 3, 4)                   # sample 1: over the corner of its cutmix box (H-5.., W-7..)
    assert boxes[0][0] == 1 or max_count == 0
    seed, offset = 0x123456789ABCDEF, 3 + (5 << 32)
    mixed = torch.from_numpy(CM.mix_u8(x8.numpy(), tab))
    want = _erase(mixed, boxes, max_count, mode, seed, offset)
    got = _collate(x8, tab, boxes, max_count, mode, seed, offset)
    assert torch.equal(got, want), (shape, mode, max_count, int((got != want).sum()))
    base = _norm(mixed.numpy())
    mask = torch.zeros(B, 3, H, W, dtype=torch.bool)
    for b, top, left, h, w in boxes:
        mask[b, :, top:top + h, left:left + w] = True
    assert mask.any() and torch.equal(got[~mask], base[~mask])
    if mode == 'const':                                  # the erase wins over the cutmix box it overlaps
        assert (got[mask] == 0).all() and mask[1, :, H - 4:H - 1, W - 6:W - 2].all()
    else:
        assert not torch.equal(got, _collate(x8, tab, boxes, max_count, mode, seed, offset + 1))
    # a table of unused slots, and no table: the mixed batch, normalised
    assert torch.equal(_collate(x8, tab, [], max_count, mode, seed, offset), base)
    assert torch.equal(_collate(x8, tab, None, 0, mode, seed, offset), base)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. arguments
# ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C
    from imagenet_models_amd import _lib
    lib = _lib.load()
    B, CH, H, W = 4, 3, 8, 8
    x8 = torch.zeros(B * CH * H * W + 64, dtype=torch.uint8, device='cuda')
    xf = torch.zeros(B * CH * H * W + 64, dtype=torch.float32, device='cuda')
    out = torch.full((B * CH * H * W + 64,), 7.0, dtype=torch.float32, device='cuda')
    mix = torch.zeros(B * 8 + 8, dtype=torch.int32, device='cuda')
    box = torch.zeros(B * 4 + 8, dtype=torch.int32, device='cuda')
    mean, std = (C.c_float * 4)(1, 2, 3, 4), (C.c_float * 4)(1, 1, 1, 1)
    X8, XF, O, M, BX = x8.data_ptr(), xf.data_ptr(), out.data_ptr(), mix.data_ptr(), box.data_ptr()

    def call(x=X8, u8=1, o=O, B=B, CH=CH, H=H, W=W, mean=mean, std=std, mix=M, boxes=BX, max_count=1, mode=0, seed=0, offset=0):
        return lib.ga_input_collate(x, u8, o, B, CH, H, W, mean, std, mix, boxes, max_count, mode, seed, offset, None)

    assert call() == 0 and call(x=XF, u8=0) == 0 and call(boxes=None, max_count=0) == 0      # the good calls these cases vary
    torch.cuda.synchronize()
    out.fill_(7.0)
    bad = dict(odd_B=dict(B=3), in_place=dict(x=O, u8=0), hw_not_x4=dict(H=3, W=3), x_u8_misaligned=dict(x=X8 + 1),
               x_f32_misaligned=dict(x=XF + 4, u8=0), out_misaligned=dict(o=O + 4), mix_misaligned=dict(mix=M + 4),
               boxes_misaligned=dict(boxes=BX + 4), no_mix=dict(mix=None), null_x=dict(x=None), null_out=dict(o=None),
               five_channels=dict(CH=5), big_B=dict(B=65536), zero_B=dict(B=0), bad_mode=dict(mode=3), offset_2_63=dict(offset=1 << 63),
               boxes_null_with_count=dict(boxes=None, max_count=1), negative_count=dict(max_count=-1),
               u8_without_stats=dict(mean=None, std=None), sample_2_30=dict(CH=1, H=32768, W=32768))
    for name, kw in bad.items():
        assert call(**kw) == GA_ERR_BAD_ARG, name
        assert 'ga_input_collate' in _lib.last_error(), name
    torch.cuda.synchronize()
    assert (out == 7.0).all()                            # nothing was launched
    tgt = torch.zeros(4, dtype=torch.int64, device='cuda')
    lam = torch.ones(4, device='cuda')
    dense = torch.full((4, 10), 7.0, device='cuda')
    T, D, L = tgt.data_ptr(), dense.data_ptr(), lam.data_ptr()
    for args in ((None, D, 4, 10, L), (T, None, 4, 10, L), (T, D, 4, 10, None), (T, D, 0, 10, L), (T, D, 4, 0, L)):
        assert lib.ga_mixup_target_elem(*args, 0.1, None) == GA_ERR_BAD_ARG and 'ga_mixup_target_elem' in _lib.last_error()
    torch.cuda.synchronize()
    assert (dense == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. targets
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('smoothing', [0.0, 0.1])
@pytest.mark.parametrize('NC', [1000, 10, 7])
def test_target_of_a_lam_vector(NC, smoothing):
    from imagenet_models_amd import ops
    B = 8
    t = torch.randint(0, NC, (B,), generator=torch.Generator().manual_seed(NC))
    t[1] = t[6]                                          # a pair of the same class: the two terms land on one column
    lam = np.array([1.0, 0.0, 0.6899998188018799, 0.5, 1e-8, float(np.nextafter(np.float32(1), np.float32(0))), 0.3, 0.123456],
                   dtype=np.float32)
    dense = torch.empty(B, NC, device='cuda')
    ops.Plan(eager=True).mixup_target_elem(t.cuda(), dense, NC, torch.from_numpy(lam).cuda(), smoothing)
    want = CM.dense_target(t, NC, lam, smoothing)
    assert torch.equal(dense.cpu(), want), int((dense.cpu() != want).sum())
    assert torch.allclose(dense.sum(1).cpu(), torch.ones(B), atol=1e-6)
    if smoothing == 0.0:
        assert torch.equal(dense[0].cpu(), torch.nn.functional.one_hot(t[0], NC).float())
        assert torch.equal(dense[1].cpu(), torch.nn.functional.one_hot(t[6], NC).float())


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the fp32 instantiation: timm's Mixup modes 'elem' / 'pair' on a normalised batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['elem', 'pair', 'batch'])
def test_fp32_batches_take_the_same_pass(mode):
    import imagenet_models_amd as A
    B, H, W, NC = 8, 32, 48, 37
    for kw in (dict(mixup_alpha=0.8, cutmix_alpha=1.0), dict(mixup_alpha=0.8, cutmix_alpha=0.0), dict(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.5)):
        fm = A.FastCollateMixup(mode=mode, label_smoothing=0.1, num_classes=NC, rng=np.random.RandomState(3), **kw)
        ref_rng = np.random.RandomState(3)
        for step in range(3):
            _, xf = _inputs(B, H, W, seed=20 + step)
            t = torch.randint(0, NC, (B,), generator=torch.Generator().manual_seed(step))
            xd = xf.cuda()
            gx, gt = fm(xd, t.cuda())
            assert torch.equal(xd.cpu(), xf)
            tab, lam = CM.sample_table(ref_rng, B, H, W, mode=mode, **kw)
            assert np.array_equal(fm.last, tab)
            assert torch.equal(gx.cpu(), torch.from_numpy(CM.mix_f32(xf.numpy(), tab))), (mode, kw, step)
            assert torch.equal(gt.cpu(), CM.dense_target(t, NC, lam, 0.1)), (mode, kw, step)


def test_mixup_batch_mode_still_equals_the_oracle():
    """Mixup(mode='batch') keeps its own kernels (ga_mixup_batch / ga_mixup_target) and its results; FastCollateMixup(mode='batch')
    on the same fp32 batch and seed gives the same bits through the new pass"""
    import imagenet_models_amd as A
    from oracle import mixup_oracle as MO
    NC = 37
    for kw in (dict(mixup_alpha=0.8, cutmix_alpha=0.0), dict(mixup_alpha=0.2, cutmix_alpha=1.0)):
        for seed in range(3):
            x = torch.randn(8, 3, 32, 48, generator=torch.Generator().manual_seed(seed))
            t = torch.randint(0, NC, (8,), generator=torch.Generator().manual_seed(100 + seed))
            rx, rt = MO.Mixup(num_classes=NC, label_smoothing=0.1, rng=np.random.RandomState(seed), **kw)(x, t)
            gx, gt = A.Mixup(num_classes=NC, label_smoothing=0.1, rng=np.random.RandomState(seed), **kw)(x.cuda(), t.cuda())
            assert torch.equal(gx.cpu(), rx) and torch.equal(gt.cpu(), rt)
            fx, ft = A.FastCollateMixup(num_classes=NC, label_smoothing=0.1, rng=np.random.RandomState(seed), **kw)(x.cuda(), t.cuda())
            assert torch.equal(fx.cpu(), rx) and torch.equal(ft.cpu(), rt)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. TrainStep
# ---------------------------------------------------------------------------------------------------------------------------
def _small_step(**kw):
    import imagenet_models_amd as A
    torch.manual_seed(0)
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    return A.TrainStep(m, opt, 4, lam=0.0, **kw)


def test_train_step_mixes_normalises_then_erases():
    """TrainStep(collate_mixup=..., random_erasing=...), uint8 input, B = 4, two steps: the engine's input is the restatement's
    mix -> normalise, bit-exact outside the erase boxes and within the noise cap inside (one clean box over the MIXTURE); the
    dense target is the restatement's"""
    import imagenet_models_amd as A
    x8, _ = _inputs(4, 224, 224, seed=4)
    t = torch.tensor([3, 17, 5, 39])
    mkw = dict(mixup_alpha=0.8, cutmix_alpha=1.0)
    ekw = dict(probability=1.0, mode='pixel', max_count=2, seed=11)
    era = A.RandomErasing(rng=random.Random(5), **ekw)
    fm = A.FastCollateMixup(mode='elem', label_smoothing=0.1, num_classes=40, rng=np.random.RandomState(7), **mkw)
    step = _small_step(collate_mixup=fm, random_erasing=era)
    ref_rng, ref_np = random.Random(5), np.random.RandomState(7)
    kinds = set()
    for k in range(2):
        loss = step(x8.cuda(), t.cuda())
        assert math.isfinite(float(loss))
        boxes, _ = R.sample_boxes(ref_rng, 4, 224, 224, probability=1.0, min_count=1, max_count=2)
        tab, lam = CM.sample_table(ref_np, 4, 224, 224, mode='elem', **mkw)
        assert era.last_boxes == boxes and era.offset == k + 1 and np.array_equal(fm.last, tab)
        base = R.normalize_u8(CM.mix_u8(x8.numpy(), tab), MEAN, STD)
        ref, mask = R.erase(base, boxes, 2, 'pixel', 11, k)
        got = step.eng.x_ref.cpu().numpy()
        assert mask.any() and np.array_equal(got[~mask], base[~mask])
        err = float(np.abs(got.astype(np.float64) - ref)[mask].max())
        print(f'step {k}: kinds {tab[:, 0].tolist()}, max |err| inside the erase boxes {err:.3e}')
        assert err <= CAP, err
        assert torch.equal(step.eng.target_buf.cpu(), CM.dense_target(t, 40, lam, 0.1))
        kinds.update(int(v) for v in tab[:, 0])
    assert kinds - {CM.NONE}                             # something was mixed
    with pytest.raises(ValueError, match='mixup_fn'):
        _small_step(collate_mixup=fm, mixup_fn=A.Mixup(num_classes=40))
    with pytest.raises(TypeError, match='uint8'):
        step(torch.randn(4, 3, 224, 224, device='cuda'), t.cuda())
    # a step built without collate_mixup gets the input it got before: the normalised batch
    plain = _small_step()
    plain(x8.cuda(), t.cuda())
    assert torch.equal(plain.eng.x_ref.cpu(), _norm(x8.numpy()))
    # ... and as a mixup_fn the object mixes the NORMALISED fp32 batch (timm's Mixup in mode 'pair'), no rounding to uint8
    fp = A.FastCollateMixup(mode='pair', label_smoothing=0.1, num_classes=40, rng=np.random.RandomState(7), **mkw)
    late = _small_step(mixup_fn=fp)
    late(x8.cuda(), t.cuda())
    tab, lam = CM.sample_table(np.random.RandomState(7), 4, 224, 224, mode='pair', **mkw)
    assert np.array_equal(fp.last, tab) and (tab[:, 0] != CM.NONE).any()
    assert torch.equal(late.eng.x_ref.cpu(), torch.from_numpy(CM.mix_f32(R.normalize_u8(x8.numpy(), MEAN, STD), tab)))
    assert torch.equal(late.eng.target_buf.cpu(), CM.dense_target(t, 40, lam, 0.1))


# ---------------------------------------------------------------------------------------------------------------------------
# 9. CLI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [['--collate-mixup', '--mixup-mode', 'elem'],
                                   ['--mixup-mode', 'pair'],                  # the default order, modes beyond 'batch': the fp32 pass
                                   ['--collate-mixup', '--epochs', '2', '--mixup-off-epoch', '1']])
def test_train_cli_runs_with_collate_mixup(flags):
    cmd = [sys.executable, 'train.py', '--synthetic', '--model', 'map_convnext_tiny', '-b', '8', '--epochs', '1', '--steps-per-epoch', '2',
           '--reprob', '1.0', '--remode', 'pixel'] + flags
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)       # a child process under its own time limit
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    m = re.search(r'\*\*\* epoch 0: train loss (\S+)', out)
    assert m and math.isfinite(float(m.group(1))), out[-2000:]
