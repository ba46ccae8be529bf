"""CPU: the host side of the on-device RandAugment (imagenet_models_amd.RandAugment: config parsing, level functions, the draw
order of sample(); the C ABI of ga_rand_augment; train.py's flags).  The draw order and the level functions are restated here by
hand from the specification (timm's auto_augment.py as written down in include/gaext.h / rand_augment.py; timm is not installed:
parity with timm itself is unpinned)."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _rand_augment_ref as R
from conftest import ROOT

RECIPES = ['rand-m7-mstd0.5-inc1', 'rand-m9-mstd0.5-inc1', 'rand-m15-mstd0.5-inc1', 'rand-m20-mstd0.5-inc1']
OPS = ['AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness', 'Sharpness',
       'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel']


class Fixed:
    """a `random` whose draws are scripted"""

    def __init__(self, value):
        self.value, self.calls = value, 0

    def random(self):
        self.calls += 1
        return self.value


def _restated_table(B, H, W, m, mstd, mmax, inc, n, p, interpolation):
    """the table by the specified draw order, from the GLOBAL generators: per sample np.random.choice(15, n), then per layer from
    `random`: the gate, the magnitude, the sign, the interpolation"""
    tab = np.zeros((B, n), dtype=R.ROW)
    tab['m'] = (1, 0, 0, 0, 1, 0)

    def neg(v):
        return -v if random.random() > 0.5 else v

    for b in range(B):
        idx = np.random.choice(15, n)
        for l in range(n):
            if random.random() > p:
                continue
            v = m
            if mstd == float('inf'):
                v = random.uniform(0, m)
            elif mstd > 0:
                v = random.gauss(m, mstd)
            v = max(0.0, min(v, mmax))
            s = v / 10.0
            name = OPS[idx[l]]
            if name in ('AutoContrast', 'Equalize', 'Invert'):
                tab[b, l] = R.row({'AutoContrast': R.AUTOCONTRAST, 'Equalize': R.EQUALIZE, 'Invert': R.INVERT}[name])
            elif name == 'Posterize':
                tab[b, l] = R.row(R.POSTERIZE, iarg=4 - int(s * 4) if inc else int(s * 4))
            elif name == 'Solarize':
                tab[b, l] = R.row(R.SOLARIZE, iarg=256 - int(s * 256) if inc else min(256, int(s * 256)))
            elif name == 'SolarizeAdd':
                tab[b, l] = R.row(R.SOLARIZE_ADD, iarg=min(128, int(s * 110)))
            elif name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
                f = max(0.1, 1.0 + neg(s * 0.9)) if inc else s * 1.8 + 0.1
                tab[b, l] = R.row({'Color': R.COLOR, 'Contrast': R.CONTRAST, 'Brightness': R.BRIGHTNESS, 'Sharpness': R.SHARPNESS}[name], farg=f)
            else:
                level = neg(s * {'Rotate': 30.0, 'ShearX': 0.3, 'ShearY': 0.3, 'TranslateXRel': 0.45, 'TranslateYRel': 0.45}[name])
                interp = random.choice((R.BILINEAR, R.BICUBIC)) if interpolation == 'random' else {'bilinear': 2, 'bicubic': 3, 'nearest': 0}[interpolation]
                mat = {'Rotate': lambda: R.rotate_matrix(level, W, H), 'ShearX': lambda: R.shear_x(level), 'ShearY': lambda: R.shear_y(level),
                       'TranslateXRel': lambda: R.translate_x_rel(level, W), 'TranslateYRel': lambda: R.translate_y_rel(level, H)}[name]()
                tab[b, l] = R.row(R.AFFINE, interp=interp, m=mat)
    return tab


@pytest.mark.parametrize('interpolation', ['random', 'bicubic'])
@pytest.mark.parametrize('config', RECIPES + ['rand-m9-mstd101-n3-p0.8', 'rand-m6-n1-p1.0-mmax8'])
def test_sample_equals_the_draw_order_restated_by_hand(config, interpolation):
    import imagenet_models_amd as A
    ra = A.RandAugment(config, interpolation=interpolation)
    kw = dict(m=ra.magnitude, mstd=ra.magnitude_std, mmax=ra.magnitude_max, inc=ra.increasing, n=ra.num_layers, p=ra.prob)
    kinds = set()
    for seed in range(4):
        random.seed(seed)
        np.random.seed(seed)
        got = [ra.sample(B, H, W) for B, H, W in ((8, 224, 224), (3, 48, 64))]           # consecutive batches continue the streams
        after = (random.random(), np.random.rand())
        random.seed(seed)
        np.random.seed(seed)
        want = [_restated_table(B, H, W, interpolation=interpolation, **kw) for B, H, W in ((8, 224, 224), (3, 48, 64))]
        assert after == (random.random(), np.random.rand())                              # the same number of draws from both generators
        for g, w in zip(got, want):
            assert g.dtype == R.ROW and g.shape == w.shape and g.tobytes() == w.tobytes(), (config, seed)
            assert R.check_table(g)
            kinds.update(int(k) for k in g['kind'].reshape(-1))
    assert len(kinds) >= 8 and R.AFFINE in kinds


def test_config_parsing_of_the_recipes_and_refusals():
    import imagenet_models_amd as A
    for config, m in zip(RECIPES, (7, 9, 15, 20)):
        ra = A.RandAugment(config)
        assert (ra.magnitude, ra.magnitude_std, ra.magnitude_max, ra.increasing, ra.num_layers, ra.prob) == (m, 0.5, 10, True, 2, 0.5)
        assert ra.fill == (124, 116, 104) and ra.interpolation == 'random'
    # m15 / m20: every drawn magnitude is clamped to mmax = 10 -- the increasing posterize of a geometric-free draw keeps 4 - 4 bits
    ra = A.RandAugment('rand-m20-mstd0.5-inc1', rng=random.Random(0))
    assert ra._level('Posterize', max(0.0, min(20, ra.magnitude_max))) == 0
    random.seed(1)
    np.random.seed(1)
    tab = A.RandAugment('rand-m20-mstd0.5-inc1-p1.0').sample(64, 224, 224).reshape(-1)
    assert (tab['iarg'][tab['kind'] == R.POSTERIZE] == 0).all() and (tab['iarg'][tab['kind'] == R.SOLARIZE] == 0).all()    # v == 10 exactly
    assert (tab['iarg'][tab['kind'] == R.SOLARIZE_ADD] == 110).all()
    f = tab['farg'][np.isin(tab['kind'], (R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS))]
    assert len(f) and np.isin(f, (np.float32(1.9), np.float32(0.1))).all()
    d = A.RandAugment('rand')
    assert (d.magnitude, d.magnitude_std, d.magnitude_max, d.increasing, d.num_layers, d.prob) == (10, 0.0, 10, False, 2, 0.5)
    assert A.RandAugment('rand-mstd101').magnitude_std == float('inf') and A.RandAugment('rand-mmax20-m15').magnitude_max == 20
    assert A.RandAugment('rand-w0').num_layers == 2
    for config, why in (('rand-m9-w1', 'weights'), ('rand-m9-t1', 'subset'), ('augmix-m5-w4-d2', "'rand-...'"), ('original', "'rand-...'"),
                        ('v0', "'rand-...'"), ('rand-m9-zz3', 'unknown section'), ('rand-m9-inc', 'no value'), ('rand-n0', 'at least 1')):
        with pytest.raises(ValueError, match=why):
            A.RandAugment(config)
    with pytest.raises(ValueError, match='interpolation'):
        A.RandAugment('rand-m9', interpolation='lanczos')


def test_every_level_function_at_0_5_10():
    import imagenet_models_amd as A
    plain = {v: A.RandAugment('rand-m9', rng=Fixed(0.1)) for v in (0, 5, 10)}           # random() = 0.1: the sign is kept
    for signed, scale in (('Rotate', 30.0), ('ShearX', 0.3), ('ShearY', 0.3), ('TranslateXRel', 0.45), ('TranslateYRel', 0.45)):
        for inc in ('', '-inc1'):
            pos, neg = A.RandAugment('rand-m9' + inc, rng=Fixed(0.1)), A.RandAugment('rand-m9' + inc, rng=Fixed(0.9))
            assert [pos._level(signed, v) for v in (0, 5, 10)] == [0.0, 0.5 * scale, scale]
            assert [neg._level(signed, v) for v in (0, 5, 10)] == [-0.0, -0.5 * scale, -scale]
            assert pos.rng.calls == 3 and neg.rng.calls == 3                            # one sign draw per level
    for name in ('Color', 'Contrast', 'Brightness', 'Sharpness'):
        assert [plain[v]._level(name, v) for v in (0, 5, 10)] == [0.1, 0.5 * 1.8 + 0.1, 1.8 + 0.1]
        up, down = A.RandAugment('rand-m9-inc1', rng=Fixed(0.1)), A.RandAugment('rand-m9-inc1', rng=Fixed(0.9))
        assert [up._level(name, v) for v in (0, 5, 10)] == [1.0, 1.45, 1.9]
        assert [down._level(name, v) for v in (0, 5, 10)] == [1.0, 0.55, 0.1]            # max(0.1, 1 - 0.9)
    assert all(p.rng.calls == 0 for p in plain.values())                                 # the plain enhance level is unsigned
    inc = A.RandAugment('rand-m9-inc1', rng=Fixed(0.1))
    assert [plain[0]._level('Posterize', v) for v in (0, 5, 10)] == [0, 2, 4] and [inc._level('Posterize', v) for v in (0, 5, 10)] == [4, 2, 0]
    assert [plain[0]._level('Solarize', v) for v in (0, 5, 10)] == [0, 128, 256] and [inc._level('Solarize', v) for v in (0, 5, 10)] == [256, 128, 0]
    for ra in (plain[0], inc):
        assert [ra._level('SolarizeAdd', v) for v in (0, 5, 10)] == [0, 55, 110]
        assert [ra._level(n, 5) for n in ('AutoContrast', 'Equalize', 'Invert')] == [None] * 3
    # Image.rotate's matrix: 0 degrees is the identity; the restatement and the package form the same doubles
    from imagenet_models_amd import rand_augment as RA
    assert RA.rotate_matrix(0.0, 64, 48) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    for deg in (27.0, -13.5, 30.0, -0.0):
        assert RA.rotate_matrix(deg, 224, 224) == R.rotate_matrix(deg, 224, 224) and RA.rotate_matrix(deg, 64, 48) == R.rotate_matrix(deg, 64, 48)
    c, s = round(math.cos(-math.radians(27.0)), 15), round(math.sin(-math.radians(27.0)), 15)
    assert RA.rotate_matrix(27.0, 64, 48)[:2] == (c, s) and RA.ROW == R.ROW and RA.OPS == tuple(OPS)


def test_p0_draws_one_random_per_layer_and_gives_all_none():
    import imagenet_models_amd as A
    rng = Fixed(0.25)
    ra = A.RandAugment('rand-m9-mstd0.5-inc1-p0', rng=rng, np_rng=np.random.RandomState(0))
    tab = ra.sample(5, 48, 64)
    assert rng.calls == 5 * 2 and (tab['kind'] == R.NONE).all() and tab.shape == (5, 2)
    assert (tab['m'] == np.array([1, 0, 0, 0, 1, 0.0])).all() and not tab['iarg'].any() and not tab['farg'].any()


def test_rand_augment_entry_points_are_declared_bound_and_exported():
    import ctypes as C
    from imagenet_models_amd import _lib, ops
    import imagenet_models_amd as A
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    lib = _lib.load()
    for name in ('ga_rand_augment', 'ga_rand_augment_check_table'):
        assert f'int {name}(' in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert 'size_t ga_rand_augment_work_bytes(' in hdr and 'ga_rand_augment_work_bytes' in _lib.exported_symbols()
    assert '{ int32 kind, int32 interp, int32 iarg, fp32 farg, double m[6] }' in hdr       # the row is documented beside the entry point
    assert hasattr(ops.Plan, 'rand_augment') and A.RandAugment.__module__ == 'imagenet_models_amd.rand_augment'
    # the workspace: 1 KiB of statistics per sample, no image for one layer, one for two, two beyond
    img = (4 * 3 * 48 * 64 + 255) // 256 * 256
    assert [lib.ga_rand_augment_work_bytes(4, 3, 48, 64, n) for n in (0, 1, 2, 3, 5)] == [4096, 4096, 4096 + img, 4096 + 2 * img, 4096 + 2 * img]
    assert lib.ga_rand_augment_work_bytes(4, 3, 48, 64, -1) == 0
    # bad arguments are refused on the host, before any launch
    assert lib.ga_rand_augment(None, None, None, 0, 2, 3, 8, 8, None, 1, None, None) != 0
    assert 'ga_rand_augment' in _lib.last_error()
    # the host-side check of a table: unknown kinds and interpolation codes
    good = np.array([R.row(k, interp=i) for k in range(12) for i in (0, 2, 3)])
    assert lib.ga_rand_augment_check_table(good.ctypes.data, good.size) == 0
    for bad, why in ((R.row(12), 'unknown kind 12'), (R.row(-1), 'unknown kind -1'), (R.row(R.AFFINE, interp=1), 'unknown interpolation 1'),
                     (R.row(R.NONE, interp=4), 'unknown interpolation 4')):
        tab = np.concatenate([good, np.array([bad])])
        assert lib.ga_rand_augment_check_table(tab.ctypes.data, tab.size) == -1 and why in _lib.last_error(), why
    assert lib.ga_rand_augment_check_table(None, 1) == -1
    assert C.sizeof(C.c_double) * 6 + 16 == R.ROW.itemsize == 64


def test_train_cli_lists_the_aa_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    text = ' '.join(r.stdout.split())
    assert '--aa NAME' in text and 'rand-m9-mstd0.5-inc1' in text and '--train-interpolation' in text
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--synthetic', '--aa', 'augmix-m5'], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "only timm's 'rand-...'" in r.stderr


def test_documents_state_the_feature():
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'ga_rand_augment' in design and 'ga_rand_augment' in readme and '--aa rand-m9-mstd0.5-inc1' in readme
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'rand_augment_trace.md'))
