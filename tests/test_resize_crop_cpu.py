"""CPU: the host side of the on-device resize and crop (imagenet_models_amd.resize_crop: the draws of RandomResizedCrop.sample, the
rows of ResizeCenterCrop, the packing offsets; the C ABI of ga_resize_crop and its host checks; TrainStep's input types; the flags
of train.py / validate.py).  The draw algorithms are restated in plain Python in tests/_resize_crop_ref.py from the specification
(timm's transforms as written down in resize_crop.py; timm is not installed: parity with timm itself is unpinned)."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _resize_crop_ref as R
from conftest import ROOT

HEIGHTS = [375, 500, 64, 300, 17, 9, 224, 1, 33]
WIDTHS = [500, 375, 48, 17, 300, 130, 224, 1, 1200]


class Script:
    """a `random` that records the order of its calls and answers from a real generator"""

    def __init__(self, seed=0):
        self.rng, self.calls = random.Random(seed), []

    def uniform(self, a, b):
        self.calls.append('uniform')
        return self.rng.uniform(a, b)

    def randint(self, a, b):
        self.calls.append('randint')
        return self.rng.randint(a, b)

    def choice(self, seq):
        self.calls.append('choice')
        return self.rng.choice(seq)


def _torch_rand(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda: float(torch.rand(1, generator=g))


@pytest.mark.parametrize('interpolation,hflip,scale,ratio', [('random', 0.5, (0.08, 1.0), (3. / 4., 4. / 3.)),
                                                             ('bicubic', 0.5, (0.08, 1.0), (3. / 4., 4. / 3.)),
                                                             ('bilinear', 0.3, (0.35, 0.9), (0.5, 2.0))])
def test_sample_draws_what_the_restated_algorithm_draws(interpolation, hflip, scale, ratio):
    import imagenet_models_amd as A
    offsets, _ = A.resize_crop.pack_offsets(HEIGHTS, WIDTHS)
    for seed in (0, 1, 2):
        rrc = A.RandomResizedCrop(32, scale=scale, ratio=ratio, interpolation=interpolation, hflip=hflip, rng=random.Random(seed),
                                  torch_gen=torch.Generator().manual_seed(seed + 10))
        got = rrc.sample(HEIGHTS, WIDTHS, offsets)
        want = R.train_table(HEIGHTS, WIDTHS, 32, scale, ratio, interpolation, hflip, random.Random(seed), _torch_rand(seed + 10), offsets)
        assert got.dtype == R.ROW and got.tobytes() == want.tobytes()
        assert (got['vh'] == 32).all() and (got['vw'] == 32).all() and (got['oy'] == 0).all() and (got['ox'] == 0).all()
        assert (got['top'] + got['h'] <= got['src_h']).all() and (got['left'] + got['w'] <= got['src_w']).all() and (got['h'] >= 1).all()


def test_sample_draws_from_the_global_generators_by_default():
    import imagenet_models_amd as A
    random.seed(5)
    torch.manual_seed(6)
    got = A.RandomResizedCrop(32).sample(HEIGHTS, WIDTHS)
    g = torch.Generator().manual_seed(6)
    want = R.train_table(HEIGHTS, WIDTHS, 32, rng=random.Random(5), torch_rand=lambda: float(torch.rand(1, generator=g)))
    assert got.tobytes() == want.tobytes()


def test_fallback_branch_known_answers():
    """no attempt fits at scale >= 0.5: 300 x 17 is narrower than ratio 3/4 allows -> the full width, h = round(17 / 0.75) = 23,
    centred; 17 x 300 is wider than 4/3 -> the full height, w = round(17 * 4 / 3) = 23; a ratio inside the range -> the whole image"""
    import imagenet_models_amd as A
    rng = Script()
    rrc = A.RandomResizedCrop(32, scale=(0.5, 1.0), interpolation='bicubic', hflip=0.0, rng=rng)
    t = rrc.sample([300, 17], [17, 300])
    assert [int(t[0][k]) for k in ('top', 'left', 'h', 'w')] == [138, 0, 23, 17]
    assert [int(t[1][k]) for k in ('top', 'left', 'h', 'w')] == [0, 138, 17, 23]
    assert rng.calls == ['uniform', 'uniform'] * 20            # ten failed attempts each, no randint, no choice
    t = A.RandomResizedCrop(32, scale=(4.0, 5.0), interpolation='bilinear', hflip=0.0).sample([40], [50])
    assert [int(t[0][k]) for k in ('top', 'left', 'h', 'w', 'interp', 'flip')] == [0, 0, 40, 50, R.BILINEAR, 0]


def test_draw_order_interpolation_after_the_box_flip_last():
    import imagenet_models_amd as A
    rng = Script(3)
    rrc = A.RandomResizedCrop(32, scale=(1.0, 1.0), ratio=(1.0, 1.0), interpolation='random', hflip=0.5, rng=rng,
                              torch_gen=torch.Generator().manual_seed(9))
    t = rrc.sample([50, 50, 50, 50], [50, 50, 50, 50])
    # area 2500, ratio 1: the first attempt gives the whole image; randint(0, 0) twice; then the choice
    assert rng.calls == ['uniform', 'uniform', 'randint', 'randint', 'choice'] * 4
    assert (t['h'] == 50).all() and (t['w'] == 50).all() and (t['top'] == 0).all()
    ref = random.Random(3)
    want = []
    for _ in range(4):
        ref.uniform(1.0, 1.0), ref.uniform(0.0, 0.0), ref.randint(0, 0), ref.randint(0, 0)
        want.append(ref.choice((R.BILINEAR, R.BICUBIC)))
    assert t['interp'].tolist() == want
    g = torch.Generator().manual_seed(9)
    assert t['flip'].tolist() == [int(float(torch.rand(1, generator=g)) < 0.5) for _ in range(4)]
    fixed = Script(3)
    A.RandomResizedCrop(32, interpolation='bicubic', rng=fixed).sample([50], [50])
    assert 'choice' not in fixed.calls                          # a fixed interpolation draws nothing


def test_hflip_zero_and_one():
    import imagenet_models_amd as A
    assert not A.RandomResizedCrop(32, hflip=0.0, rng=random.Random(0)).sample(HEIGHTS, WIDTHS)['flip'].any()
    assert A.RandomResizedCrop(32, hflip=1.0, rng=random.Random(0)).sample(HEIGHTS, WIDTHS)['flip'].all()


def test_eval_rows_are_resize_short_side_and_centre_crop():
    import imagenet_models_amd as A
    for pct, interpolation in ((0.875, 'bicubic'), (0.95, 'bilinear'), (1.0, 'bicubic')):
        got = A.ResizeCenterCrop(32, pct, interpolation).rows(HEIGHTS, WIDTHS)
        assert got.tobytes() == R.eval_table(HEIGHTS, WIDTHS, 32, pct, interpolation).tobytes()
    # by hand: size 224 at 0.875 -> the short side to 256; 375 x 500 -> 256 x int(256 * 500 / 375) = 341; window at (16, round(58.5))
    r = A.ResizeCenterCrop(224).rows([375], [500])[0]
    assert [int(r[k]) for k in ('top', 'left', 'h', 'w', 'vh', 'vw', 'oy', 'ox', 'interp', 'flip')] == [0, 0, 375, 500, 256, 341, 16, 58, 3, 0]
    with pytest.raises(ValueError, match='crop_pct'):
        A.ResizeCenterCrop(224, crop_pct=1.1)


def test_refused_interpolations_say_why():
    import imagenet_models_amd as A
    for name in ('lanczos', 'box', 'hamming'):
        with pytest.raises(ValueError, match='bilinear and bicubic'):
            A.RandomResizedCrop(224, interpolation=name)
        with pytest.raises(ValueError, match='bilinear and bicubic'):
            A.ResizeCenterCrop(224, interpolation=name)
    with pytest.raises(ValueError):
        A.ResizeCenterCrop(224, interpolation='random')
    with pytest.raises(ValueError, match='multiple of 4'):
        A.RandomResizedCrop(30)


def test_pack_offsets_are_16_byte_aligned_and_disjoint():
    import imagenet_models_amd as A
    offsets, total = A.resize_crop.pack_offsets(HEIGHTS, WIDTHS)
    assert offsets.dtype == np.int64 and offsets[0] == 0 and (offsets % 16 == 0).all() and total % 16 == 0
    ends = offsets + 3 * np.array(HEIGHTS, dtype=np.int64) * np.array(WIDTHS)
    assert (ends[:-1] <= offsets[1:]).all() and (offsets[1:] - ends[:-1] < 16).all() and ends[-1] <= total < ends[-1] + 16


def test_entry_points_are_declared_bound_and_exported():
    import imagenet_models_amd as A
    from imagenet_models_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    for name in ('ga_resize_crop', 'ga_resize_crop_check_table', 'ga_resample_coeffs'):
        assert f'int {name}(' in hdr and name in _lib.exported_symbols()
    assert 'size_t ga_resize_crop_work_bytes(' in hdr and 'ga_resize_crop_work_bytes' in _lib.exported_symbols()
    assert hasattr(ops.Plan, 'resize_crop') and hasattr(ops.Plan, 'resample_coeffs')
    for cls in (A.RaggedBatch, A.RandomResizedCrop, A.ResizeCenterCrop):
        assert cls.__module__ == 'imagenet_models_amd.resize_crop'
    assert A.pack_images.__module__ == 'imagenet_models_amd.resize_crop' and A.resize_crop.ROW == R.ROW
    lib = _lib.load()
    # the workspace: B + 1 offsets, then per sample coefficients [k][OW], bounds, coefficients [k][OH], bounds, [3][h][OW] bytes
    tab = np.stack([R.row(64, 48, 0, 0, 64, 48, 32, 32, interp=R.BICUBIC), R.row(9, 130, 2, 3, 5, 100, 32, 32, interp=R.BILINEAR)])

    def region(h, w, interp):
        kh, kv = min(w, R.ksize(w, 32, interp)), min(h, R.ksize(h, 32, interp))
        return 4 * kh * 32 + 8 * 32 + 4 * kv * 32 + 8 * 32 + ((3 * h * 32 + 15) & ~15)
    assert lib.ga_resize_crop_work_bytes(tab.ctypes.data, 2, 32, 32) == 32 + region(64, 48, R.BICUBIC) + region(5, 100, R.BILINEAR)
    assert lib.ga_resize_crop_work_bytes(None, 2, 32, 32) == 0
    assert C.sizeof(C.c_int64) + 14 * C.sizeof(C.c_int32) == R.ROW.itemsize == 64


GOOD = dict(src_h=64, src_w=48, top=4, left=5, h=40, w=30, vh=32, vw=32, oy=0, ox=0, interp=R.BICUBIC, flip=0, src_off=16)
SRC_BYTES = 16 + 3 * 64 * 48


@pytest.mark.parametrize('change,why', [
    (dict(top=30), 'box outside its image'), (dict(left=20), 'box outside its image'), (dict(top=-1), 'box outside its image'),
    (dict(left=-2), 'box outside its image'),
    (dict(h=0), 'empty box'), (dict(w=0), 'empty box'), (dict(w=-3), 'empty box'),
    (dict(src_off=32), 'outside the source buffer'), (dict(src_off=-16), 'outside the source buffer'),
    (dict(vh=31), 'window outside'), (dict(ox=1), 'window outside'), (dict(oy=-1), 'window outside'), (dict(vw=40, ox=9), 'window outside'),
    (dict(interp=0), 'unknown interpolation'), (dict(interp=1), 'unknown interpolation'), (dict(interp=4), 'unknown interpolation'),
    (dict(flip=2), 'flip'), (dict(flip=-1), 'flip'),
    (dict(src_h=32768, src_off=0), 'extent'), (dict(src_w=40000), 'extent'), (dict(vh=32768), 'extent'), (dict(vw=32768), 'extent'),
    (dict(src_h=0), 'extent'), (dict(vw=0), 'extent'),
])
def test_check_table_refuses_each_bad_row(change, why):
    from imagenet_models_amd import _lib
    lib = _lib.load()
    good = np.stack([R.row(**GOOD)] * 3)
    assert lib.ga_resize_crop_check_table(good.ctypes.data, 3, 32, 32, SRC_BYTES) == 0
    bad = good.copy()
    for k, v in change.items():
        bad[1][k] = v
    src_bytes = 1 << 40 if 'src_h' in change or 'src_w' in change else SRC_BYTES        # the extent itself is what is refused
    assert lib.ga_resize_crop_check_table(bad.ctypes.data, 3, 32, 32, src_bytes) == -1
    err = _lib.last_error()
    assert 'ga_resize_crop_check_table: row 1' in err and why in err, err


def test_check_table_and_entry_refuse_bad_scalars():
    from imagenet_models_amd import _lib
    lib = _lib.load()
    good = np.stack([R.row(**dict(GOOD, vw=40, vh=40))] * 2)
    for B, OH, OW, why in ((2, 32, 30, 'multiple of 4'), (2, 32, 0, 'bad args'), (0, 32, 32, 'bad args'), (2, 32768, 32, 'bad args'),
                           (2, 32, 32768, 'bad args'), (70000, 32, 32, 'bad args')):
        assert lib.ga_resize_crop_check_table(good.ctypes.data, B, OH, OW, SRC_BYTES) == -1 and why in _lib.last_error(), (B, OH, OW)
    assert lib.ga_resize_crop_check_table(None, 2, 32, 32, SRC_BYTES) == -1
    # the launch entry validates before anything is enqueued: no device is needed to be refused
    fake = 1 << 20
    for args, why in (((None, 64, fake, fake, fake, 1 << 30, 2, 32, 32), 'device pointers'),
                      ((fake, 64, fake, fake, fake, 1 << 30, 2, 32, 30), 'multiple of 4'),
                      ((fake, 64, fake, fake + 8, fake, 1 << 30, 2, 32, 32), '16-byte aligned'),
                      ((fake, 64, fake + 4, fake, fake, 1 << 30, 2, 32, 32), '16-byte aligned'),
                      ((fake, 64, fake, fake, fake + 1, 1 << 30, 2, 32, 32), '16-byte aligned'),
                      ((fake, 64, fake, fake, fake, 64, 2, 32, 32), 'workspace'),
                      ((fake, 64, fake, fake, fake, 1 << 30, 2, 32768, 32), 'bad args')):
        assert lib.ga_resize_crop(*args, None) == -1 and 'ga_resize_crop' in _lib.last_error() and why in _lib.last_error(), args
    for args, why in (((0, 8, R.BICUBIC, fake, fake, 64), 'bad args'), ((8, 32768, R.BICUBIC, fake, fake, 64), 'bad args'),
                      ((8, 8, 0, fake, fake, 64), 'unknown interpolation'), ((700, 16, R.BICUBIC, fake, fake, 100), 'ksize'),
                      ((8, 8, R.BICUBIC, None, fake, 64), 'bad args'), ((8, 8, R.BICUBIC, fake, fake + 2, 64), '4-byte aligned')):
        assert lib.ga_resample_coeffs(*args, None) == -1 and why in _lib.last_error(), args


def test_train_step_input_types():
    import imagenet_models_amd as A
    ragged = A.RaggedBatch(torch.zeros(48, dtype=torch.uint8), [0], [4], [4])
    assert len(ragged) == 1 and ragged.size(0) == 1
    crop = A.RandomResizedCrop(32)
    with pytest.raises(TypeError, match='RaggedBatch needs TrainStep'):
        A.InputStage(crop=None).check(ragged)
    with pytest.raises(TypeError, match='takes a RaggedBatch'):
        A.InputStage(crop=crop).check(torch.zeros(1, 3, 32, 32, dtype=torch.uint8))
    A.InputStage(crop=crop).check(ragged)
    A.InputStage(crop=None).check(torch.zeros(1, 3, 32, 32))
    with pytest.raises(TypeError, match='takes a RaggedBatch'):
        crop(torch.zeros(1, 3, 32, 32, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        crop(ragged)
    with pytest.raises(TypeError):
        A.RaggedBatch(torch.zeros(48), [0], [4], [4])


def test_clis_list_the_new_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    text = ' '.join(r.stdout.split())
    for flag in ('--scale LO HI', '--ratio LO HI', '--hflip HFLIP', '--synthetic-source HxW', '--train-interpolation'):
        assert flag in text, flag
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'validate.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    text = ' '.join(r.stdout.split())
    for flag in ('--crop-pct CROP_PCT', '--interpolation INTERPOLATION', '--synthetic-source HxW'):
        assert flag in text, flag
    sys.path.insert(0, ROOT)
    import train
    import validate
    a = train.parser.parse_args(['--synthetic', '--synthetic-source', '120x96', '--scale', '0.1', '1.0', '--ratio', '0.5', '2', '--hflip', '0.3'])
    assert (a.scale, a.ratio, a.hflip, train.parse_hw(a.synthetic_source)) == ([0.1, 1.0], [0.5, 2.0], 0.3, (120, 96))
    d = train.parser.parse_args(['--synthetic'])
    assert (d.scale, d.ratio, d.hflip, d.synthetic_source) == ([0.08, 1.0], [3. / 4., 4. / 3.], 0.5, None)       # timm's defaults
    v = validate.parser.parse_args(['--synthetic', '--synthetic-source', '120x96', '--crop-pct', '0.95', '--interpolation', 'bilinear'])
    assert (v.crop_pct, v.interpolation, v.synthetic_source) == (0.95, 'bilinear', '120x96')
    assert validate.parser.parse_args([]).crop_pct == 0.875
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--synthetic', '--synthetic-source', '120x96', '--train-interpolation',
                        'lanczos'], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'bilinear and bicubic' in r.stderr


def test_documents_state_the_feature():
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'ga_resize_crop' in design and 'ga_resize_crop' in readme and '--synthetic-source' in readme
    assert 'The random-resized crop and the flip stay with the loader' not in design
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'resize_crop_trace.md'))
