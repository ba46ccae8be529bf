"""GPU: ga_rand_augment (csrc/randaug.hip, imagenet_models_amd.RandAugment, TrainStep(auto_augment=...)) against the numpy
restatement of tests/_rand_augment_ref.py -- itself held to PIL's own bytes by tests/test_rand_augment_ref_cpu.py -- and against the
PIL fixture directly.  Every pixel gate is equality."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

import _rand_augment_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GA_ERR_BAD_ARG = -1
ID = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _images(B, H, W, seed):
    x = np.random.RandomState(seed).randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    return x


def _run(x, table):
    """the table through imagenet_models_amd.RandAugment (host check, staging, workspace, launch) -> numpy"""
    import imagenet_models_amd as A
    table = np.ascontiguousarray(table, dtype=R.ROW)
    ra = A.RandAugment(f'rand-n{table.shape[1]}')
    xd = torch.from_numpy(x).cuda()
    out = ra(xd, table=table)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), torch.from_numpy(x))        # out of place: the input is untouched
    return out.cpu().numpy()


def _same(got, want, what):
    diff = int((got != want).sum())
    per = [int((got[b] != want[b]).sum()) for b in range(got.shape[0])]
    assert diff == 0, (what, 'differing bytes per sample', per)


def _single_layer_rows(which, H, W):
    """row b has kind b; three sets of arguments (both extremes and a middle) and the three interpolations"""
    post, sol, add, fac, interp, m = [(0, 0, 0, 0.1, R.NEAREST, R.rotate_matrix(27.0, W, H)),
                                      (8, 256, 110, 1.9, R.BILINEAR, R.shear_x(-0.3)),
                                      (2, 128, 55, 0.55, R.BICUBIC, R.rotate_matrix(-13.5, W, H))][which]
    rows = [R.row(R.NONE), R.row(R.AUTOCONTRAST), R.row(R.EQUALIZE), R.row(R.INVERT), R.row(R.POSTERIZE, iarg=post), R.row(R.SOLARIZE, iarg=sol),
            R.row(R.SOLARIZE_ADD, iarg=add), R.row(R.COLOR, farg=fac), R.row(R.CONTRAST, farg=fac), R.row(R.BRIGHTNESS, farg=fac),
            R.row(R.SHARPNESS, farg=fac), R.row(R.AFFINE, interp=interp, m=m)]
    assert [int(r['kind']) for r in rows] == list(range(12))
    return np.array(rows).reshape(12, 1)


@pytest.mark.parametrize('shape', [(48, 64), (36, 50)])       # 36 x 50: H*W % 4 == 0 with W % 4 != 0 -- groups of four run across rows
@pytest.mark.parametrize('which', [0, 1, 2])
def test_single_layer_every_kind(which, shape):
    H, W = shape
    x = _images(12, H, W, seed=10 + which)
    for b in (1, 2, 8):                                       # the histogram ops and contrast on an image that is not full-range
        x[b] = x[b] // 3 + 40
    tab = _single_layer_rows(which, H, W)
    want = R.rand_augment(x, tab)
    identities = {0: (6,), 1: (4, 5), 2: ()}[which]           # solarize_add 0; posterize 8 and solarize 256
    assert all((want[b] != x[b]).any() != (b in identities) for b in range(1, 12))
    _same(_run(x, tab), want, f'set {which}')


def test_fixture_cases_equal_pil_itself():
    """every case of tests/golden/randaug_pil.npz as one batch: the kernel's bytes against PIL's, no restatement in between --
    every kind, the degenerate images (low contrast, a constant channel, equalize's step == 0) through autocontrast and equalize,
    every geometric form at the three interpolations"""
    z = np.load(os.path.join(GOLDEN, 'randaug_pil.npz'))
    rows = z['rows'].view(R.ROW).reshape(-1, 1)
    x = z['images'][z['which']]
    names = [str(n) for n in z['image_names']]
    deg = [k for k in range(len(rows)) if names[z['which'][k]] != 'rand' and int(rows[k, 0]['kind']) in (R.AUTOCONTRAST, R.EQUALIZE)]
    assert len(deg) == 6
    got = _run(np.ascontiguousarray(x), rows)
    _same(got, z['outputs'], [str(s) for s in z['labels']])
    _same(got, R.rand_augment(x, rows), 'restatement')


def test_two_layers_in_order():
    H, W = 48, 64
    aff = R.row(R.AFFINE, interp=R.BILINEAR, m=R.rotate_matrix(27.0, W, H))
    cub = R.row(R.AFFINE, interp=R.BICUBIC, m=R.shear_y(0.3))
    pairs = [(aff, R.row(R.EQUALIZE)), (R.row(R.EQUALIZE), aff), (cub, R.row(R.SHARPNESS, farg=1.9)), (R.row(R.CONTRAST, farg=0.55), R.row(R.AUTOCONTRAST)),
             (R.row(R.NONE), R.row(R.COLOR, farg=1.45)), (R.row(R.COLOR, farg=1.45), R.row(R.NONE)), (R.row(R.NONE), R.row(R.NONE)),
             (R.row(R.SHARPNESS, farg=0.1), cub)]
    tab = np.array(pairs)
    x = _images(len(pairs), H, W, seed=20)
    x[1], x[5] = x[0], x[4]
    x[3] = x[3] // 3 + 40
    want = R.rand_augment(x, tab)
    assert (want[0] != want[1]).any()                         # affine -> equalize is not equalize -> affine: the order matters
    assert np.array_equal(want[4], want[5]) and np.array_equal(want[6], x[6])
    _same(_run(x, tab), want, 'two layers')
    # three layers: both ping-pong images of the workspace
    tab3 = np.array([(aff, R.row(R.EQUALIZE), R.row(R.SHARPNESS, farg=1.9)), (R.row(R.CONTRAST, farg=1.9), cub, R.row(R.AUTOCONTRAST)),
                     (R.row(R.NONE), R.row(R.INVERT), R.row(R.NONE)), (R.row(R.POSTERIZE, iarg=3), R.row(R.NONE), aff)])
    _same(_run(x[:4], tab3), R.rand_augment(x[:4], tab3), 'three layers')


def test_affine_edge_cases():
    H, W = 48, 64
    forms = [ID, R.translate_x_rel(0.125, W), R.translate_y_rel(-0.25, H), R.translate_x_rel(1.5, W), R.translate_y_rel(-1.0, H),
             (1.0, 1.0, -1.0, 0.0, 1.0, 0.0),                # xin = x + y: exactly 0 at (0, 0) and exactly W on a diagonal
             (1.0, -1.0, 0.0, 0.0, 1.0, 0.0)]                # xin = x - y: exactly 0 on a diagonal
    rows = [R.row(R.AFFINE, interp=i, m=m) for m in forms for i in (R.NEAREST, R.BILINEAR, R.BICUBIC)]
    tab = np.array(rows).reshape(-1, 1)
    x = np.repeat(_images(1, H, W, seed=30), len(rows), axis=0)
    got = _run(x, tab)
    _same(got, R.rand_augment(x, tab), 'edges')
    fill = np.array(R.FILL, dtype=np.uint8)[:, None, None]
    for i in range(3):
        assert np.array_equal(got[i], x[0])                                               # the identity returns the input
        assert np.array_equal(got[3 + i][:, :, :56], x[0][:, :, 8:]) and (got[3 + i][:, :, 56:] == fill).all()      # 8 pixels to the left
        assert np.array_equal(got[6 + i][:, 12:, :], x[0][:, :36, :]) and (got[6 + i][:, :12, :] == fill).all()     # 12 pixels down
        assert (got[9 + i] == fill).all() and (got[12 + i] == fill).all()                # only fill is left
        assert (got[15 + i][:, 47, 17:] == fill[:, 0]).all() and (got[15 + i][:, 47, :17] != fill[:, 0]).any()     # x + 47 >= 64: outside


def test_full_size_with_a_drawn_table():
    import imagenet_models_amd as A
    ra = A.RandAugment('rand-m9-mstd0.5-inc1', rng=random.Random(4), np_rng=np.random.RandomState(4))
    x = _images(3, 224, 224, seed=40)
    xd = torch.from_numpy(x).cuda()
    out = ra(xd)
    tab = ra.last
    assert tab.shape == (3, 2) and (tab['kind'] != R.NONE).sum() >= 2, tab['kind']
    _same(out.cpu().numpy(), R.rand_augment(x, tab), tab['kind'].tolist())
    # a second batch from the same object: the streams go on, the buffers are reused
    tab2 = ra.sample(3, 224, 224)
    _same(ra(xd, table=tab2).cpu().numpy(), R.rand_augment(x, tab2), tab2['kind'].tolist())


def _small_step(**kw):
    import imagenet_models_amd as A
    torch.manual_seed(0)
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    return A.TrainStep(m, opt, 4, lam=0.0, **kw)


def test_train_step_augments_first_then_collates():
    """TrainStep(auto_augment, collate_mixup, random_erasing): the engine's input equals ga_input_collate run on the separately
    augmented batch (the restatement's) with the same mix rows, boxes, seed and offset -- bit for bit, the erase noise included"""
    import imagenet_models_amd as A
    from imagenet_models_amd import ops
    x = _images(4, 224, 224, seed=50)
    t = torch.tensor([3, 17, 5, 39])
    ra = A.RandAugment('rand-m9-mstd0.5-inc1-p1.0', rng=random.Random(8), np_rng=np.random.RandomState(8))
    era = A.RandomErasing(probability=1.0, mode='pixel', max_count=2, seed=11, rng=random.Random(5))
    fm = A.FastCollateMixup(mode='elem', label_smoothing=0.1, num_classes=40, rng=np.random.RandomState(7), mixup_alpha=0.8, cutmix_alpha=1.0)
    step = _small_step(auto_augment=ra, collate_mixup=fm, random_erasing=era)
    loss = step(torch.from_numpy(x).cuda(), t.cuda())
    assert math.isfinite(float(loss))
    got = step.eng.x_ref.clone()
    assert (ra.last['kind'] != R.NONE).all() and len(era.last_boxes) >= 4
    aug = R.rand_augment(x, ra.last)
    assert (aug != x).any()
    boxes = torch.zeros(4, 2, 4, dtype=torch.int32)
    used = [0] * 4
    for i, top, left, h, w in era.last_boxes:
        boxes[i, used[i]] = torch.tensor([top, left, h, w], dtype=torch.int32)
        used[i] += 1
    want = torch.empty(4, 3, 224, 224, device='cuda')
    mean, std = step.eng.input_stats()
    ops.Plan(eager=True).input_collate(torch.from_numpy(aug).cuda(), want, torch.from_numpy(fm.last).cuda(), boxes.cuda(), 2, 2, 11, 0, mean, std)
    torch.cuda.synchronize()
    assert torch.equal(got, want), int((got != want).sum())
    # the other input stages take the augmented uint8 batch as well: erase alone, and the plain normalisation
    inv = np.array([[R.row(R.INVERT), R.row(R.NONE)]] * 4)
    plain = _small_step(auto_augment=A.RandAugment('rand-n2'))
    plain.auto_augment.sample = lambda B, H, W: inv
    plain(torch.from_numpy(x).cuda(), t.cuda())
    ref = _small_step()
    ref(torch.from_numpy(255 - x).cuda(), t.cuda())
    assert torch.equal(plain.eng.x_ref, ref.eng.x_ref)
    # p0: all rows none -- the batch comes back unchanged, and the step's input is what it is without auto_augment
    p0 = A.RandAugment('rand-m9-mstd0.5-inc1-p0')
    xd = torch.from_numpy(x).cuda()
    assert torch.equal(p0(xd), xd) and (p0.last['kind'] == R.NONE).all()
    same = _small_step(auto_augment=p0)
    same(xd, t.cuda())
    ref(xd, t.cuda())
    assert torch.equal(same.eng.x_ref, ref.eng.x_ref) and _small_step().auto_augment is None
    with pytest.raises(TypeError, match='uint8'):
        step(torch.randn(4, 3, 224, 224, device='cuda'), t.cuda())
    with pytest.raises(TypeError, match='uint8'):
        p0(torch.randn(4, 3, 224, 224, device='cuda'))
    with pytest.raises(RuntimeError, match='unknown kind 12'):
        p0(xd, table=np.array([[R.row(12), R.row(R.NONE)]] * 4))


def test_bad_arguments_are_refused_before_any_launch():
    from imagenet_models_amd import _lib
    lib = _lib.load()
    B, CH, H, W, n = 4, 3, 8, 8, 2
    need = lib.ga_rand_augment_work_bytes(B, CH, H, W, n)
    x = torch.zeros(B * CH * H * W + 64, dtype=torch.uint8, device='cuda')
    out = torch.full((B * CH * H * W + 64,), 7, dtype=torch.uint8, device='cuda')
    work = torch.full((need + 64,), 7, dtype=torch.uint8, device='cuda')
    tab = torch.zeros(B * n * 64 + 64, dtype=torch.uint8, device='cuda')
    fill = (C.c_ubyte * 3)(*R.FILL)
    X, O, WK, T = x.data_ptr(), out.data_ptr(), work.data_ptr(), tab.data_ptr()
    assert X % 16 == 0 and O % 16 == 0 and WK % 16 == 0 and T % 16 == 0

    def call(x=X, o=O, work=WK, work_bytes=need, B=B, CH=CH, H=H, W=W, ops=T, n=n, fill=fill):
        return lib.ga_rand_augment(x, o, work, work_bytes, B, CH, H, W, ops, n, fill, None)

    assert call() == 0 and call(n=0, ops=None, work=None, work_bytes=0, fill=None) == 0 and call(n=1, work_bytes=B * 1024) == 0    # the good calls
    torch.cuda.synchronize()
    assert not out[:B * CH * H * W].any()                    # all-none rows: a copy of the zero batch
    out.fill_(7)
    work.fill_(7)
    bad = dict(in_place=dict(o=X), one_channel=dict(CH=1), four_channels=dict(CH=4), hw_not_x4=dict(H=3, W=3), x_misaligned=dict(x=X + 1),
               out_misaligned=dict(o=O + 2), table_misaligned=dict(ops=T + 8), work_misaligned=dict(work=WK + 4),
               work_too_small=dict(work_bytes=need - 1), no_work=dict(work=None), negative_layers=dict(n=-1), no_table=dict(ops=None),
               no_fill=dict(fill=None), null_x=dict(x=None), null_out=dict(o=None), zero_B=dict(B=0), big_B=dict(B=65536),
               wide=dict(H=4, W=32768), sample_2_30=dict(H=20000, W=20000))
    for name, kw in bad.items():
        assert call(**kw) == GA_ERR_BAD_ARG, name
        assert 'ga_rand_augment' in _lib.last_error(), name
    torch.cuda.synchronize()
    assert (out == 7).all() and (work == 7).all()            # nothing was launched


def test_train_cli_runs_with_aa():
    """train.py --aa: RandAugment first, then the recipes' collate order, on the uint8 batches of the synthetic loader"""
    import subprocess
    import sys
    from conftest import ROOT
    cmd = [sys.executable, 'train.py', '--synthetic', '--model', 'mobilenet_v1', '--num-classes', '40', '-b', '8', '--epochs', '1',
           '--steps-per-epoch', '2', '--aa', 'rand-m9-mstd0.5-inc1', '--reprob', '0.25', '--remode', 'pixel', '--mixup', '0.8', '--cutmix', '1.0',
           '--collate-mixup']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)       # a child process under its own time limit
    assert r.returncode == 0, r.stderr[-3000:]
    assert '*** epoch 0: train loss' in r.stderr + r.stdout
