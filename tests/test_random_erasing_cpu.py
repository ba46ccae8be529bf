"""CPU: the host side of RandomErasing (imagenet_models_amd.random_erasing) -- the box sampler draws in timm's order (against the
plain-Python restatement of tests/_random_erasing_ref.py; timm itself is not installed: parity with it is unpinned), every box
has the properties the algorithm guarantees, the numpy Philox4x32-10 the GPU tests hold the kernel against reproduces the
Random123 known-answer vectors, train.py carries the reference's four flags, and the new C entry point is declared, bound and
exported."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _random_erasing_ref as R
from conftest import ROOT

SETTINGS = [dict(probability=0.5), dict(probability=1.0), dict(probability=0.25, min_count=1, max_count=3),
            dict(probability=1.0, min_count=1, max_count=3), dict(probability=1.0, min_count=2, max_count=2),
            dict(probability=1.0, num_splits=2), dict(probability=0.7, min_count=1, max_count=3, num_splits=2),
            dict(probability=1.0, num_splits=3, min_area=0.1, max_area=0.2, min_aspect=0.5, max_aspect=4.0)]


@pytest.mark.parametrize('kw', SETTINGS)
@pytest.mark.parametrize('shape', [(8, 224, 224), (8, 160, 160), (8, 32, 48)])
def test_sampler_draws_in_the_restatements_order(kw, shape):
    import imagenet_models_amd as A
    B, H, W = shape
    for seed in range(6):
        mine = A.RandomErasing(mode='pixel', rng=random.Random(seed), **kw)
        a, b = random.Random(seed), mine.rng
        for _ in range(3):                                  # consecutive batches continue one stream
            want, _ = R.sample_boxes(a, B, H, W, **kw)
            assert mine.sample(B, H, W) == want, (kw, seed)
        assert a.random() == b.random()                     # ... and both consumed the same number of draws
    assert mine.max_count == (kw.get('max_count') or kw.get('min_count', 1))


@pytest.mark.parametrize('kw', SETTINGS)
@pytest.mark.parametrize('shape', [(8, 224, 224), (8, 160, 160), (9, 32, 48)])
def test_every_box_has_the_properties_of_the_algorithm(kw, shape):
    """h = round(sqrt(A r)), w = round(sqrt(A / r)) with A in [min_area, max_area] H W / count and r in [min_aspect, max_aspect]:
    each side is within 0.5 of its real value, so  A - (h + w + 1) / 2 + 1/4 <= h w <= A + (h + w + 1) / 2 + 1/4  at the ends of
    the area range, and  (h - 0.5) / (w + 0.5) <= r <= (h + 0.5) / (w - 0.5)  at the ends of the aspect range"""
    import imagenet_models_amd as A
    B, H, W = shape
    min_area, max_area = kw.get('min_area', 0.02), kw.get('max_area', 1 / 3)
    min_aspect = kw.get('min_aspect', 0.3)
    max_aspect = kw.get('max_aspect') or 1 / min_aspect
    nbox = 0
    for seed in range(20):
        mine = A.RandomErasing(mode='const', rng=random.Random(1000 + seed), **kw)
        boxes = mine.sample(B, H, W)
        ref, counts = R.sample_boxes(random.Random(1000 + seed), B, H, W, **kw)
        assert boxes == ref
        per_sample = {}
        for (i, top, left, h, w), count in zip(boxes, counts):
            nbox += 1
            per_sample[i] = per_sample.get(i, 0) + 1
            assert 0 < h < H and 0 < w < W
            assert 0 <= top and top + h <= H and 0 <= left and left + w <= W
            slack = (h + w + 1) / 2 + 0.25
            assert min_area * H * W / count - slack <= h * w <= max_area * H * W / count + slack, (h, w, count)
            assert (h + 0.5) / (w - 0.5) >= min_aspect * (1 - 1e-12) and (h - 0.5) / (w + 0.5) <= max_aspect * (1 + 1e-12), (h, w)
            assert kw.get('min_count', 1) <= count <= mine.max_count
            if kw.get('num_splits', 0) > 1:
                assert i >= B // kw['num_splits']           # the first (clean) split is never erased
            else:
                assert 0 <= i < B
        assert all(n <= mine.max_count for n in per_sample.values())
        if kw['probability'] == 1.0:
            start = B // kw['num_splits'] if kw.get('num_splits', 0) > 1 else 0
            assert sorted(per_sample) == list(range(start, B))
    assert nbox > 0


class _CountingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def random(self):
        self.calls.append('random')
        return super().random()

    def randint(self, a, b):
        self.calls.append('randint')
        return super().randint(a, b)


def test_zero_probability_draws_once_per_sample_and_erases_nothing():
    import imagenet_models_amd as A
    rng = _CountingRandom(3)
    mine = A.RandomErasing(probability=0.0, mode='pixel', max_count=3, rng=rng)
    assert mine.sample(16, 224, 224) == []
    assert rng.calls == ['random'] * 16
    rng = _CountingRandom(3)
    assert A.RandomErasing(probability=0.0, num_splits=2, rng=rng).sample(16, 224, 224) == [] and rng.calls == ['random'] * 8


def test_constructor_defaults_and_errors():
    import imagenet_models_amd as A
    re = A.RandomErasing()
    assert (re.probability, re.min_area, re.max_area, re.mode, re.min_count, re.max_count, re.num_splits, re.seed, re.offset) == \
        (0.5, 0.02, 1 / 3, 'const', 1, 1, 0, 0, 0)
    assert re.log_aspect_ratio == (math.log(0.3), math.log(1 / 0.3)) and re.rng is random
    assert A.RandomErasing(min_count=2).max_count == 2 and A.RandomErasing(max_count=3).min_count == 1
    with pytest.raises(ValueError):
        A.RandomErasing(mode='noise')
    with pytest.raises(RuntimeError, match='no CPU'):       # no CPU fallback, as Mixup
        re(torch.zeros(2, 3, 8, 8))


def test_philox4x32_10_known_answers():
    """the Random123 known-answer vectors of Philox4x32-10 (kat_vectors of the Random123 distribution; Salmon et al., SC'11):
    zero counter and key, all-ones counter and key, and the digits-of-pi counter and key"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v[0]) for v in R.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, [hex(g) for g in got])
    # vectorised over counters: the same values element by element
    c0 = np.arange(5, dtype=np.uint64)
    many = R.philox4x32_10(c0, 7, 9, 11, 123, 456)
    for k in range(5):
        one = R.philox4x32_10(k, 7, 9, 11, 123, 456)
        assert [int(v[k]) for v in many] == [int(v[0]) for v in one]


def test_restated_normals_use_the_documented_layout():
    """lane i & 3 of call i >> 2; a different offset, stream or seed is a different call; the uniforms never reach 0 or 1"""
    idx = np.arange(64)
    n = R.pixel_noise(idx, offset=5, seed=99)
    four = R.normals(np.arange(16), 5, 0, 99)
    assert np.array_equal(n.reshape(16, 4), four.T)
    assert not np.allclose(n, R.pixel_noise(idx, offset=6, seed=99)) and not np.allclose(n, R.pixel_noise(idx, offset=5, seed=98))
    assert R.box_colour(0, 0, 0, 1, 3, 5, 99) == R.normals([0], 5, 1, 99)[0, 0] != four[0, 0]
    big = R.pixel_noise(np.arange(400000), offset=0, seed=1)
    assert np.isfinite(big).all() and abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01 and np.abs(big).max() <= math.sqrt(48 * math.log(2))
    # 64-bit words: offset bits 32..62 and seed bits 32..63 reach the counter / key
    assert not np.allclose(n, R.pixel_noise(idx, offset=5 + (1 << 32), seed=99))
    assert not np.allclose(n, R.pixel_noise(idx, offset=5, seed=99 + (1 << 32)))


def test_restated_erase_applies_boxes_in_order():
    x = np.ones((2, 3, 8, 8), dtype=np.float32)
    boxes = [(1, 0, 0, 4, 4), (1, 2, 2, 4, 4)]
    out, mask = R.erase(x, boxes, 2, 'rand', seed=4, offset=0)
    assert mask.sum() == 3 * (16 + 16 - 4) and (out[0] == 1).all() and (out[~mask] == 1).all()
    for c in range(3):
        first, second = R.box_colour(1, 0, c, 2, 3, 0, 4), R.box_colour(1, 1, c, 2, 3, 0, 4)
        assert out[1, c, 0, 0] == first and out[1, c, 3, 3] == second and out[1, c, 5, 5] == second    # the later box wins
    out, _ = R.erase(x, boxes, 2, 'const', seed=4, offset=0)
    assert (out[mask] == 0).all()


def test_train_cli_lists_the_random_erasing_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ('--reprob', '--remode', '--recount', '--resplit'):
        assert flag in r.stdout, flag
    assert 'Random erase prob (default: 0.)' in r.stdout and 'Random erase mode (default: "pixel")' in r.stdout


def test_input_erase_is_declared_bound_and_exported():
    from imagenet_models_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    assert 'int ga_input_erase(' in hdr and 'ga_input_erase' in _lib.exported_symbols()
    assert hasattr(_lib.load(), 'ga_input_erase')
    # the documents state the size of the C ABI: they follow the table
    n = len(_lib.exported_symbols())
    for doc, phrase in (('README.md', f'{n} entry points'), ('DESIGN.md', f'{n} `extern "C"` entry points'),
                        ('INTEGRATION.md', f'all {n} entry points')):
        assert phrase in open(os.path.join(ROOT, doc)).read(), (doc, phrase)
    # bad arguments are refused on the host, before any launch
    lib = _lib.load()
    assert lib.ga_input_erase(None, 1, None, 1, 3, 8, 8, None, None, None, 0, 0, 0, 0, None) != 0
    assert 'ga_input_erase' in _lib.last_error()
