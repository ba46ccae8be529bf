"""CPU: the numpy restatement of the RandAugment ops (tests/_rand_augment_ref.py -- what the GPU tests hold ga_rand_augment to)
against PIL's own outputs: the committed fixture tests/golden/randaug_pil.npz (tools/gen_golden_randaug.py, PIL 12.2.0) and, where
PIL imports, live PIL on the same and on further arguments.  Every gate is equality: 0 differing bytes."""
import os

import numpy as np
import pytest

import _rand_augment_ref as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'randaug_pil.npz'))
    return dict(images=z['images'], names=[str(n) for n in z['image_names']], rows=z['rows'].view(R.ROW).reshape(-1), which=z['which'],
                outputs=z['outputs'], labels=[str(s) for s in z['labels']], fill=tuple(int(v) for v in z['fill']))


def test_fixture_holds_what_the_gates_need(golden):
    g = golden
    assert g['images'].shape == (4, 3, 48, 64) and g['images'].dtype == np.uint8 and g['fill'] == R.FILL == (124, 116, 104)
    assert sorted(g['names']) == ['const', 'low', 'rand', 'step0']
    assert os.path.getsize(os.path.join(GOLDEN, 'randaug_pil.npz')) < 768 * 1024
    const, low, step0 = (g['images'][g['names'].index(n)] for n in ('const', 'low', 'step0'))
    assert (const[1] == const[1, 0, 0]).all() and low.min() >= 40 and low.max() <= 125
    h = np.bincount(step0[0].reshape(-1), minlength=256)
    assert 0 < h.sum() - h[np.nonzero(h)[0][-1]] < 255                       # equalize: step == 0
    kinds = g['rows']['kind']
    for k in range(1, 11):
        assert (kinds == k).sum() >= (1 if k in (R.INVERT,) else 3), k       # >= 3 arguments / images per kind
    geo = g['rows'][kinds == R.AFFINE]
    for interp in (R.NEAREST, R.BILINEAR, R.BICUBIC):
        assert (geo['interp'] == interp).sum() == len(geo) // 3 >= 12
    ident = (geo['m'] == np.array([1, 0, 0, 0, 1, 0.0])).all(1)
    assert ident.sum() >= 3                                                   # the identity (and rotate 0), every interpolation
    assert (g['rows']['iarg'][kinds == R.POSTERIZE].tolist() == [0, 2, 4, 8] and g['rows']['iarg'][kinds == R.SOLARIZE].tolist() == [0, 128, 256])
    assert g['rows']['iarg'][kinds == R.SOLARIZE_ADD].tolist() == [0, 55, 110]
    allfill = [k for k, s in enumerate(g['labels']) if ':affine:' in s and (g['outputs'][k] == np.array(R.FILL, dtype=np.uint8)[:, None, None]).all()]
    assert len(allfill) == 3                                                  # a translation that leaves only fill


def test_restatement_equals_every_fixture_output(golden):
    g = golden
    assert len(g['labels']) >= 70
    for k, label in enumerate(g['labels']):
        got = R.apply_op(g['images'][g['which'][k]], g['rows'][k], g['fill'])
        assert got.dtype == np.uint8 and got.shape == g['outputs'][k].shape
        assert int((got != g['outputs'][k]).sum()) == 0, label


def test_degenerate_and_identity_cases_are_what_they_should_be(golden):
    g = golden
    img = {n: g['images'][i] for i, n in enumerate(g['names'])}
    assert np.array_equal(R.apply_op(img['step0'], R.row(R.EQUALIZE)), img['step0'])                  # step == 0: identity
    assert np.array_equal(R.apply_op(img['const'], R.row(R.AUTOCONTRAST))[1], img['const'][1])        # hi <= lo: identity
    assert np.array_equal(R.apply_op(img['const'], R.row(R.EQUALIZE))[1], img['const'][1])            # one occupied bin
    ac = R.apply_op(img['low'], R.row(R.AUTOCONTRAST))
    assert ac.min() == 0 and ac.max() == 255
    for interp in (R.NEAREST, R.BILINEAR, R.BICUBIC):
        assert np.array_equal(R.apply_op(img['rand'], R.row(R.AFFINE, interp=interp)), img['rand'])
        t = R.apply_op(img['rand'], R.row(R.AFFINE, interp=interp, m=R.translate_x_rel(0.125, 64)))  # 8 pixels, an integer
        assert np.array_equal(t[:, :, :56], img['rand'][:, :, 8:]) and (t[:, :, 56:] == np.array(R.FILL, dtype=np.uint8)[:, None, None]).all()
    assert np.array_equal(R.apply_op(img['rand'], R.row(R.POSTERIZE, iarg=8)), img['rand'])
    assert not R.apply_op(img['rand'], R.row(R.POSTERIZE, iarg=0)).any()
    assert np.array_equal(R.apply_op(img['rand'], R.row(R.SOLARIZE, iarg=256)), img['rand'])
    assert np.array_equal(R.apply_op(img['rand'], R.row(R.SOLARIZE, iarg=0)), 255 - img['rand'])
    assert np.array_equal(R.apply_op(img['rand'], R.row(99)), img['rand']) and not R.check_table(np.array([R.row(99)]))
    assert not R.check_table(np.array([R.row(R.AFFINE, interp=1)])) and R.check_table(g['rows'])


def test_blend_truncates_and_saturates():
    a = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.blend(0, a, 1.0), a)
    assert np.array_equal(R.blend(0, a, 0.5), a // 2)                         # truncation: 0.5 -> 0, 1.5 -> 1
    assert R.blend(0, a, 1.9)[-1] == 255 and R.blend(255, a, 1.9)[0] == 0
    assert R.blend(100, np.array([101], dtype=np.uint8), 0.1)[0] == 100


def test_restatement_equals_live_pil(golden):
    """the fixture's cases again, and arguments beyond them, against the PIL that is installed"""
    PIL = pytest.importorskip('PIL')
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_golden_randaug as G
    finally:
        sys.path.pop(0)
    g = golden
    imgs = G.images()
    assert np.array_equal(np.stack([imgs[n] for n in sorted(imgs)]), g['images'])       # the generator still makes the fixture's inputs
    cases = G.cases()
    assert len(cases) == len(g['labels'])
    for k, (img, name, arg, interp) in enumerate(cases):
        want = G.from_pil(G.pil_op(G.to_pil(imgs[img]), name, arg, interp))
        row = G.row_of(name, arg, interp)
        assert row.tobytes() == g['rows'][k].tobytes(), g['labels'][k]
        assert int((R.apply_op(imgs[img], row) != want).sum()) == 0, (PIL.__version__, g['labels'][k])
    rng = np.random.RandomState(5)
    for t in range(20):                                                       # other sizes (odd ones too), random arguments
        H, W = [(48, 64), (37, 52), (5, 7), (224, 224)][t % 4]
        a = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
        todo = [(n, float(rng.uniform(0.1, 1.9)), 0) for n in ('color', 'contrast', 'brightness', 'sharpness')]
        todo += [('autocontrast', 0, 0), ('equalize', 0, 0), ('posterize', int(rng.randint(0, 5)), 0), ('solarize', int(rng.randint(0, 257)), 0),
                 ('solarize_add', int(rng.randint(0, 111)), 0)]
        for interp in (R.NEAREST, R.BILINEAR, R.BICUBIC):
            todo += [('affine', R.shear_x(rng.uniform(-0.3, 0.3)), interp), ('affine', R.shear_y(rng.uniform(-0.3, 0.3)), interp),
                     ('affine', R.translate_x_rel(rng.uniform(-0.45, 0.45), W), interp),
                     ('affine', R.translate_y_rel(rng.uniform(-0.45, 0.45), H), interp)]
        for name, arg, interp in todo:
            want = G.from_pil(G.pil_op(G.to_pil(a), name, arg, interp))
            assert int((R.apply_op(a, G.row_of(name, arg, interp)) != want).sum()) == 0, (name, arg, interp, H, W)
        for interp in (R.NEAREST, R.BILINEAR, R.BICUBIC):                     # Image.rotate == Image.transform with the restated matrix
            deg = float(rng.uniform(-30, 30))
            want = G.from_pil(G.to_pil(a).rotate(deg, resample=G._PIL_INTERP[interp], fillcolor=R.FILL))
            assert int((R.affine(a, R.rotate_matrix(deg, W, H), interp) != want).sum()) == 0, (deg, interp, H, W)
