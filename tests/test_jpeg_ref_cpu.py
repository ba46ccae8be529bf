"""CPU: the host entropy stage of the JPEG decoder (csrc/jpeg_host.h through ga_jpeg_probe / ga_jpeg_entropy_decode) and the numpy
restatement of the device reconstruction (tests/_jpeg_ref.py) against PIL's own bytes: the committed fixture tests/golden/jpeg_pil.npz
(tools/gen_golden_jpeg.py, PIL 12.2.0 with libjpeg-turbo) and, where PIL is importable, a live decode of the same files.  Equality,
every file.  Then the host stage alone against damaged input: every prefix and 2,000 seeded single-byte mutations of two files into
guarded buffers."""
import io
import os
import random
import time

import numpy as np
import pytest

import _jpeg_ref as J
from conftest import GOLDEN


@pytest.fixture(scope='module')
def lib():
    from imagenet_models_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def golden():
    return J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]


def test_fixture_is_small_and_complete(golden):
    assert os.path.getsize(os.path.join(GOLDEN, 'jpeg_pil.npz')) <= os.path.getsize(os.path.join(GOLDEN, 'randaug_pil.npz'))
    names = [c['name'] for c in golden]
    sizes = ('8x8', '16x16', '17x33', '9x17', '48x31', '37x53', '64x80', '1x1', '2x3', '1x40', '40x1', '5x4', '3x6')
    for s in sizes:
        for sub in ('444', '422', '420'):
            for q in (10, 95):
                assert f'{s}_{sub}_q{q}' in names
    assert sum('_grey_' in n for n in names) == 3 and sum(c['kind'] == 'ok' for c in golden) == len(sizes) * 6 + 7
    assert any(n.endswith('_q1') for n in names) and any(n.endswith('_q100') for n in names)
    assert any('optimize' in n for n in names) and any('restart' in n for n in names)
    assert [c['kind'] for c in golden if 'progressive' in c['name']] == ['fallback']
    assert [(c['kind'], c['pixels']) for c in golden if 'cmyk' in c['name']] == [('refuse', None)]


def test_host_stage_and_restatement_equal_pil_on_every_file(lib, golden):
    checked = 0
    for c in golden:
        if c['kind'] != 'ok':
            continue
        st, info, coef, qt, intact = J.entropy_decode(lib, c['data'], guard=64)
        assert st == J.OK and intact, c['name']
        got = J.reconstruct(info, coef, qt)
        assert got.shape == c['pixels'].shape, c['name']
        diff = int((got != c['pixels']).sum())
        assert diff == 0, (c['name'], diff, int(np.abs(got.astype(int) - c['pixels'].astype(int)).max()))
        checked += 1
    assert checked == 85


def test_probe_classes_sizes_and_coefficient_counts(lib, golden):
    for c in golden:
        st, info = J.probe(lib, c['data'])
        if c['kind'] != 'ok':
            assert st == J.UNSUPPORTED, c['name']
            assert not info.any()
            continue
        assert st == J.OK, c['name']
        h, w = (int(v) for v in c['name'].split('_')[0].split('x'))
        sub = c['name'].split('_')[1]
        hs, vs = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'grey': (1, 1)}[sub]
        ncomp = 1 if sub == 'grey' else 3
        mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
        assert info[:5].tolist() == [w, h, ncomp, hs, vs] and info[7:9].tolist() == [mw, mh], c['name']
        assert info[9:13].tolist() == [hs, vs, mw * hs, mh * vs]
        want = 64 * mw * mh * (hs * vs + (2 if ncomp == 3 else 0))
        assert info[5] == want, c['name']
        if ncomp == 3:
            assert info[13:21].tolist() == [1, 1, mw, mh] * 2
            assert info[21:24].tolist() == [0, 64 * mw * mh * hs * vs, 64 * mw * mh * (hs * vs + 1)]
        assert info[6] == (3 if 'restart' in c['name'] else 0)
    # no JPEG at all (a PNG signature), nothing, and a bare SOI
    assert J.probe(lib, b'\x89PNG\r\n\x1a\n' + bytes(40))[0] == J.UNSUPPORTED
    assert J.probe(lib, b'')[0] == J.UNSUPPORTED
    assert J.probe(lib, b'\xff\xd8')[0] == J.CORRUPT
    # a buffer sized for another file is refused, not overrun
    big = next(c for c in golden if c['name'] == '64x80_444_q95')
    coef, qt = np.zeros(64, dtype=np.int16), np.zeros(192, dtype=np.uint16)
    assert lib.ga_jpeg_entropy_decode(big['data'], len(big['data']), coef.ctypes.data, 64, qt.ctypes.data) == J.CORRUPT
    assert lib.ga_jpeg_entropy_decode(None, 0, coef.ctypes.data, 64, qt.ctypes.data) == -1


def test_live_pil_decodes_the_fixture_bytes_to_the_stored_pixels(golden):
    Image = pytest.importorskip('PIL.Image')
    for c in golden:
        if c['pixels'] is not None:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(c['data'])).convert('RGB')), c['pixels']), c['name']


@pytest.mark.parametrize('name', ['37x53_420_q75_restart3', '64x80_grey_q90'])
def test_host_stage_survives_prefixes_and_mutations(lib, golden, name):
    """each call returns one of the three classes and leaves the 64 guard bytes on both sides of both buffers alone"""
    data = next(c for c in golden if c['name'] == name)['data']
    t0 = time.time()
    seen = {J.OK: 0, J.UNSUPPORTED: 0, J.CORRUPT: 0}
    for n in range(len(data) + 1):
        st, _, _, _, intact = J.entropy_decode(lib, data[:n], guard=64)
        assert st in seen and intact, (n, st)
        seen[st] += 1
        if n < len(data) - 2:
            assert st != J.OK, n                 # all of these files' bytes but the EOI marker are needed
    rnd = random.Random(20261020)
    for _ in range(2000):
        b = bytearray(data)
        at = rnd.randrange(len(b))
        b[at] = rnd.randrange(256)
        st, _, _, _, intact = J.entropy_decode(lib, bytes(b), guard=64)
        assert st in seen and intact, (at, b[at], st)
        seen[st] += 1
    assert seen[J.OK] and seen[J.CORRUPT]
    assert time.time() - t0 < 30
