"""GPU: ga_jpeg_reconstruct (csrc/jpeg.hip) byte for byte against (a) the numpy int64 restatement of tests/_jpeg_ref.py on coefficients
and tables handed in directly -- small random ones and the extremes the 64-bit intermediates are there for -- and (b) PIL's own bytes
of tests/golden/jpeg_pil.npz, every OK file alone and all of them as one batch in fixture order and shuffled, into a buffer whose
padding and tail must come back untouched.  No PIL here: the fixture holds its bytes."""
import os

import numpy as np
import pytest
import torch

import _jpeg_ref as J
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return [c for c in J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0] if c['kind'] == 'ok']


def _reconstruct(tab, coef, qt, dst_bytes, fill=0xA5):
    """stage a HOST table + coefficients + tables and launch -> (dst bytes, work bytes) as numpy"""
    from imagenet_models_amd import _lib, ops
    lib = _lib.load()
    tab = np.ascontiguousarray(tab, dtype=J.ROW).reshape(-1)
    work = int(lib.ga_jpeg_work_bytes(tab.ctypes.data, len(tab)))
    assert work == coef.size
    _lib.check(lib.ga_jpeg_check_table(tab.ctypes.data, len(tab), coef.size, qt.size, work, dst_bytes), 'ga_jpeg_check_table')
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    d_coef = torch.from_numpy(coef.copy()).cuda()
    d_qt = torch.from_numpy(qt.astype(np.uint16).view(np.int16).copy()).cuda()
    d_work = torch.full((work,), 0x3C, dtype=torch.uint8, device='cuda')
    d_dst = torch.full((dst_bytes,), fill, dtype=torch.uint8, device='cuda')
    ops.Plan(eager=True).jpeg_reconstruct(d_tab, len(tab), d_coef, d_qt, d_work, d_dst)
    torch.cuda.synchronize()
    return d_dst.cpu().numpy(), d_work.cpu().numpy()


def _block_sets(nb, kind, rng):
    """(coef int16 (nb, 64), qt uint16 (64,))"""
    if kind == 'small':
        return rng.randint(-40, 41, (nb, 64)).astype(np.int16), rng.randint(1, 64, 64).astype(np.uint16)
    if kind == 'single2047':        # one coefficient of +-2047 per block, every position in turn, table entries up to 255
        coef = np.zeros((nb, 64), dtype=np.int16)
        coef[np.arange(nb), np.arange(nb) % 64] = np.where(np.arange(nb) % 2, -2047, 2047)
        qt = rng.randint(1, 256, 64).astype(np.uint16)
        qt[::7] = 255
        return coef, qt
    if kind == 'dense2047':         # +-2047 everywhere with table entries up to 255: 2^19 per term, past int32 in both passes
        return rng.choice(np.array([-2047, 2047], dtype=np.int16), (nb, 64)), np.full(64, 255, dtype=np.uint16)
    if kind == 'int16':             # the int16 extremes with a table of ones
        return rng.choice(np.array([-32768, 32767, 0, -1, 1], dtype=np.int16), (nb, 64)), np.ones(64, dtype=np.uint16)
    raise ValueError(kind)


@pytest.mark.parametrize('kind', ['small', 'single2047', 'dense2047', 'int16'])
@pytest.mark.parametrize('nb', [1, 7, 65, 1030])
def test_idct_kernel_equals_the_restatement(nb, kind):
    """one grey image of nb blocks side by side: the IDCT kernel's plane is read back from the workspace, the image from dst"""
    rng = np.random.RandomState(nb * 31 + len(kind))
    coef, qt = _block_sets(nb, kind, rng)
    want = J.idct_blocks(coef, qt)                                   # (nb, 8, 8)
    info = np.zeros(J.INFO_LEN, dtype=np.int64)
    info[[0, 1, 2, 3, 4, 7, 8]] = [8 * nb, 8, 1, 1, 1, nb, 1]
    qt3 = np.zeros(192, dtype=np.uint16)
    qt3[:64] = qt
    dst, work = _reconstruct(J.table_row(info), coef.reshape(-1), qt3, 3 * 64 * nb + 256)
    plane = want.transpose(1, 0, 2).reshape(8, 8 * nb)
    assert np.array_equal(work.reshape(8, 8 * nb), plane), (nb, kind, int((work.reshape(8, 8 * nb) != plane).sum()))
    assert np.array_equal(dst[:3 * 64 * nb].reshape(8, 8 * nb, 3), np.repeat(plane[:, :, None], 3, axis=2))
    assert (dst[3 * 64 * nb:] == 0xA5).all()
    if kind != 'small':
        assert (want == 0).any() or (want == 255).any()              # the set does saturate


def _decode_host(golden):
    from imagenet_models_amd import _lib
    lib = _lib.load()
    out = []
    for c in golden:
        st, info, coef, qt, intact = J.entropy_decode(lib, c['data'])
        assert st == J.OK, c['name']
        out.append((info, coef, qt.reshape(-1)))
    return out


@pytest.fixture(scope='module')
def host(golden):
    return _decode_host(golden)


def _batch(golden, host, order):
    """the fixture files `order` as ONE launch -> list of (name, got, want), plus the untouched-bytes check"""
    from imagenet_models_amd.resize_crop import pack_offsets
    hs = [golden[k]['pixels'].shape[0] for k in order]
    ws = [golden[k]['pixels'].shape[1] for k in order]
    offsets, total = pack_offsets(hs, ws)
    tab = np.zeros(len(order), dtype=J.ROW)
    at = 0
    for j, k in enumerate(order):
        info = host[k][0]
        tab[j] = J.table_row(info, coef_off=at, dst_off=offsets[j], work_off=at, qt_off=192 * j)
        at += int(info[5])
    coef = np.concatenate([host[k][1] for k in order])
    qt = np.concatenate([host[k][2] for k in order])
    dst, _ = _reconstruct(tab, coef, qt, total + 256)
    written = np.zeros(total + 256, dtype=bool)
    res = []
    for j, k in enumerate(order):
        n = 3 * hs[j] * ws[j]
        written[offsets[j]:offsets[j] + n] = True
        res.append((golden[k]['name'], dst[offsets[j]:offsets[j] + n].reshape(hs[j], ws[j], 3), golden[k]['pixels']))
    assert (dst[~written] == 0xA5).all(), 'a byte of the alignment padding or of the 256-byte tail was written'
    assert (~written).sum() >= 256
    return res


def test_every_fixture_file_alone_equals_pil(golden, host):
    assert len(golden) == 85
    for k in range(len(golden)):
        for name, got, want in _batch(golden, host, [k]):
            assert np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize('shuffled', [False, True])
def test_all_fixture_files_as_one_batch_equal_pil(golden, host, shuffled):
    order = list(range(len(golden)))
    if shuffled:
        order = np.random.RandomState(7).permutation(len(golden)).tolist()
    for name, got, want in _batch(golden, host, order):
        assert np.array_equal(got, want), (name, shuffled, int((got != want).sum()))


def test_reconstruct_and_check_table_refuse_bad_calls(golden, host):
    from imagenet_models_amd import _lib
    lib = _lib.load()
    info = host[0][0]
    good = np.array([J.table_row(info)], dtype=J.ROW)
    n = int(info[5])
    dstb = 3 * int(info[0]) * int(info[1])
    assert lib.ga_jpeg_check_table(good.ctypes.data, 1, n, 192, n, dstb) == 0
    for field, value, why in (('width', 0, 'not a baseline image'), ('hs', 3, 'not a baseline image'), ('mcus_w', 9, 'not a baseline image'),
                              ('coef_off', 64, 'coefficients outside'), ('coef_off', 4, 'coefficients outside'), ('qt_off', 8, 'tables outside'),
                              ('work_off', 16, 'planes outside'), ('dst_off', 16, 'image outside'), ('dst_off', 8, 'image outside')):
        bad = good.copy()
        bad[0][field] = value
        assert lib.ga_jpeg_check_table(bad.ctypes.data, 1, n, 192, n, dstb) == -1 and why in _lib.last_error(), (field, _lib.last_error())
    assert lib.ga_jpeg_check_table(None, 1, n, 192, n, dstb) == -1 and lib.ga_jpeg_check_table(good.ctypes.data, 0, n, 192, n, dstb) == -1
    assert lib.ga_jpeg_work_bytes(good.ctypes.data, 1) == n and lib.ga_jpeg_work_bytes(None, 1) == 0
    t = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    p = t.data_ptr()
    assert lib.ga_jpeg_reconstruct(p, 1, p, p, p, None, None) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ga_jpeg_reconstruct(p, 1, p + 2, p, p, p, None) == -1 and '16-byte aligned' in _lib.last_error()
    assert lib.ga_jpeg_reconstruct(p, 0, p, p, p, p, None) == -1
