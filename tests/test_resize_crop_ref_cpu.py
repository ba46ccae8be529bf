"""CPU: the numpy restatement of ga_resize_crop (tests/_resize_crop_ref.py -- what the GPU tests hold the kernels to) against PIL's
own outputs: the committed fixture tests/golden/resize_crop_pil.npz (tools/gen_golden_resize_crop.py, PIL 12.2.0) and, where PIL
imports, live PIL on seeded random (source, box, size, filter) draws.  Every gate is equality: 0 differing bytes."""
import os
import random

import numpy as np
import pytest

import _resize_crop_ref as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return R.load_golden(os.path.join(GOLDEN, 'resize_crop_pil.npz'))


def test_fixture_holds_what_the_gates_need(golden):
    g = golden
    assert os.path.getsize(os.path.join(GOLDEN, 'resize_crop_pil.npz')) < 500 * 1000
    assert sorted(s.shape for s in g['sources']) == sorted([(37, 53, 3), (64, 48, 3), (9, 130, 3), (300, 17, 3), (16, 700, 3), (96, 96, 3)])
    for s in g['sources']:                                       # hard blocks beside noise: bicubic overshoot reaches both clamps
        assert s.dtype == np.uint8 and s.min() == 0 and s.max() == 255
    r, shapes = g['rows'], g['shapes']
    assert {tuple(s) for s in shapes} == {(32, 32), (24, 40)}
    assert set(r['interp']) == {R.BILINEAR, R.BICUBIC} and set(r['flip']) == {0, 1}
    train = (r['oy'] == 0) & (r['ox'] == 0) & (r['vh'] == shapes[:, 0]) & (r['vw'] == shapes[:, 1])
    full = (r['h'] == r['src_h']) & (r['w'] == r['src_w'])
    for interp in (R.BILINEAR, R.BICUBIC):
        f = train & (r['interp'] == interp)
        assert (f & full).any() and (f & (r['h'] == 1) & (r['w'] == 1)).any()
        assert (f & (r['w'] == r['vw']) & ~full).any() and (f & (r['h'] == r['vh']) & ~full).any()      # one pass is the identity
        for top, left in ((0, 0), (0, 1), (1, 0), (1, 1)):                                                  # each corner
            t = r['top'] == 0 if top == 0 else r['top'] + r['h'] == r['src_h']
            l = r['left'] == 0 if left == 0 else r['left'] + r['w'] == r['src_w']
            assert (f & ~full & t & l).any()
        assert (f & (r['vh'] > r['h']) & (r['vw'] > r['w'])).any()                                           # upscale on both axes
        assert (f & (r['vh'] > r['h']) & (r['vw'] < r['w'])).any()                                           # up and down
        ev = ~train & (r['interp'] == interp)
        assert (ev & (r['oy'] > 0)).any() and (ev & (r['ox'] > 0)).any() and (ev & (r['oy'] > 0) & (r['ox'] > 0)).any()
    # tap counts no register array holds: the 700-wide source to 32 columns in the fixture, 700 -> 16 in the coefficient sweep
    assert (full & (r['src_w'] == 700) & (r['interp'] == R.BICUBIC) & (r['vw'] == 32)).any()
    assert R.coeffs(700, 32, R.BICUBIC)[0][:, 1].max() == 88
    assert R.ksize(700, 16, R.BICUBIC) == 177 and R.coeffs(700, 16, R.BICUBIC)[0][:, 1].max() == 175      # PIL's row pitch, the taps used


def test_restatement_equals_every_fixture_output(golden):
    g = golden
    for k, label in enumerate(g['labels']):
        OH, OW = (int(v) for v in g['shapes'][k])
        got = R.apply_row(g['sources'][g['which'][k]], g['rows'][k], OH, OW)
        assert got.dtype == np.uint8 and np.array_equal(got, g['outputs'][k]), (label, int((got != g['outputs'][k]).sum()))


def test_coefficients_are_identity_when_the_size_does_not_change():
    for interp in (R.BILINEAR, R.BICUBIC):
        for n in (1, 2, 17, 224):
            b, k = R.coeffs(n, n, interp)
            assert (b[:, 1] >= 1).all()
            for xx in range(n):
                taps = k[xx, :b[xx, 1]]
                assert taps.sum() == 1 << 22 and taps[xx - b[xx, 0]] == 1 << 22, (interp, n, xx)


def _pil(img, top, left, h, w, OH, OW, interp, flip):
    from PIL import Image
    im = Image.fromarray(img, 'RGB').crop((left, top, left + w, top + h)).resize((OW, OH), interp)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im).transpose(2, 0, 1)


def test_restatement_equals_live_pil():
    pytest.importorskip('PIL')
    rng = random.Random(7)
    shapes = [(375, 500, 224, 224)] + [(rng.randint(1, 110), rng.randint(1, 150), rng.choice((8, 17, 24, 32, 40)), rng.choice((8, 16, 32, 40)))
                                       for _ in range(149)]
    n = 0
    for k, (H, W, OH, OW) in enumerate(shapes):
        img = R.source(H, W, k)
        if k == 0:
            boxes = [(0, 0, H, W), (40, 61, 289, 377)]
        else:
            h, w = rng.randint(1, H), rng.randint(1, W)
            boxes = [(rng.randint(0, H - h), rng.randint(0, W - w), h, w)]
        for top, left, h, w in boxes:
            for interp in (R.BILINEAR, R.BICUBIC):
                flip = rng.randint(0, 1)
                got = R.apply_row(img, R.row(H, W, top, left, h, w, OH, OW, 0, 0, interp, flip), OH, OW)
                want = _pil(img, top, left, h, w, OH, OW, interp, flip)
                assert np.array_equal(got, want), ((H, W), (top, left, h, w), (OH, OW), interp, flip, int((got != want).sum()))
                n += 1
    assert n >= 300


def test_eval_rows_equal_live_pil_resize_and_centre_crop():
    pytest.importorskip('PIL')
    from PIL import Image
    for k, (H, W) in enumerate(((64, 48), (37, 53), (50, 50), (9, 130))):
        img = R.source(H, W, 100 + k)
        for pct in (0.875, 0.95, 1.0):
            for interp in (R.BILINEAR, R.BICUBIC):
                r = R.eval_row(H, W, 32, pct, interp)
                im = Image.fromarray(img, 'RGB').resize((int(r['vw']), int(r['vh'])), interp)
                oy, ox = int(r['oy']), int(r['ox'])
                want = np.asarray(im.crop((ox, oy, ox + 32, oy + 32))).transpose(2, 0, 1)
                assert np.array_equal(R.apply_row(img, r, 32, 32), want), ((H, W), pct, interp)
