"""GPU: ga_resample_coeffs and ga_resize_crop (csrc/resample.hip) against the numpy restatement of tests/_resize_crop_ref.py --
itself held to PIL's own bytes by tests/test_resize_crop_ref_cpu.py -- and against the PIL fixture directly.  Every coefficient and
pixel gate is equality."""
import os

import numpy as np
import pytest
import torch

import _resize_crop_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GA_ERR_BAD_ARG = -1


def _pack(images):
    """sources back to back on 16-byte starts -> (device bytes, offsets)"""
    import imagenet_models_amd as A
    rb = A.pack_images(images)
    return rb.data, rb.offsets


def _run(images, table, OH, OW):
    """the table through the C ABI: host check, workspace from the host table, one launch -> numpy (B, 3, OH, OW)"""
    from imagenet_models_amd import _lib, ops
    lib = _lib.load()
    data, offsets = _pack(images)
    tab = np.ascontiguousarray(table, dtype=R.ROW).copy()
    tab['src_off'] = offsets
    B = len(tab)
    _lib.check(lib.ga_resize_crop_check_table(tab.ctypes.data, B, OH, OW, data.numel()), 'ga_resize_crop_check_table')
    need = lib.ga_resize_crop_work_bytes(tab.ctypes.data, B, OH, OW)
    work = torch.empty(need, dtype=torch.uint8, device='cuda')
    dev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    out = torch.full((B, 3, OH, OW), 7, dtype=torch.uint8, device='cuda')
    before = data.clone()
    ops.Plan(eager=True).resize_crop(data, dev, out, work, B, OH, OW)
    torch.cuda.synchronize()
    assert torch.equal(data, before)                          # the sources are untouched
    return out.cpu().numpy()


def _same(got, want, what):
    per = [int((got[b] != want[b]).sum()) for b in range(got.shape[0])]
    assert sum(per) == 0, (what, 'differing bytes per sample', per)


def _pairs():
    """(in, out): in = 1, in < out, in = out, in = out +- 1, primes, the heavy downscales, the real shapes"""
    pairs = [(1, 1), (1, 7), (1, 224), (2, 1), (2, 3), (3, 2), (700, 16), (500, 224), (375, 224), (32767, 8), (8, 32767 // 64), (224, 224),
             (256, 224), (341, 224), (224, 256), (100, 1), (1200, 224), (1600, 224), (9, 32), (130, 32), (17, 40), (300, 24)]
    for n in (2, 3, 5, 8, 13, 31, 32, 33, 64, 97, 127, 128, 223, 225, 251):
        pairs += [(n, n), (n, n + 1), (n + 1, n), (n, n - 1) if n > 1 else (n, n), (n - 1, n) if n > 1 else (n, n)]
    primes = (7, 11, 13, 17, 19, 23, 29, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 101, 103, 107, 109, 113, 131, 211, 223, 227, 229)
    pairs += [(a, b) for a, b in zip(primes, primes[::-1])]
    pairs += [(a, 32) for a in primes[::2]] + [(32, a) for a in primes[1::2]]
    rng = np.random.RandomState(3)
    pairs += [(int(a), int(b)) for a, b in zip(rng.randint(1, 1500, 60), rng.randint(1, 300, 60))]
    return sorted(set(pairs))


@pytest.mark.parametrize('interp', [R.BILINEAR, R.BICUBIC])
def test_coefficients_equal_the_restatement(interp):
    from imagenet_models_amd import ops
    pairs = _pairs()
    assert len(pairs) >= 190 and {(700, 16), (500, 224), (375, 224), (32767, 8), (1, 224)} <= set(pairs)
    p = ops.Plan(eager=True)
    got = []
    for n_in, n_out in pairs:
        ks = R.ksize(n_in, n_out, interp)
        bounds = torch.full((n_out, 2), -1, dtype=torch.int32, device='cuda')
        coeffs = torch.full((n_out, ks), -1, dtype=torch.int32, device='cuda')
        p.resample_coeffs(n_in, n_out, interp, bounds, coeffs, ks)
        got.append((bounds, coeffs))
    torch.cuda.synchronize()
    for (n_in, n_out), (bounds, coeffs) in zip(pairs, got):
        wb, wk = R.coeffs(n_in, n_out, interp)
        b, k = bounds.cpu().numpy(), coeffs.cpu().numpy()
        assert np.array_equal(b, wb), (n_in, n_out, 'bounds')
        assert np.array_equal(k, wk), (n_in, n_out, 'coefficients', int((k != wk).sum()), int(np.abs(k.astype(np.int64) - wk).max()))


def test_every_fixture_case_equals_pil():
    g = R.load_golden(os.path.join(GOLDEN, 'resize_crop_pil.npz'))
    for shape in ((32, 32), (24, 40)):
        idx = [k for k in range(len(g['labels'])) if tuple(g['shapes'][k]) == shape]
        assert len(idx) >= 30
        images = [g['sources'][g['which'][k]] for k in idx]
        got = _run(images, g['rows'][idx], *shape)
        want = np.stack([g['outputs'][k] for k in idx])
        _same(got, want, [g['labels'][k] for k in idx])
    assert sorted(k for s in ((32, 32), (24, 40)) for k in range(len(g['labels'])) if tuple(g['shapes'][k]) == s) == list(range(len(g['labels'])))


def test_one_batch_mixes_every_kind_of_sample():
    """upscale, heavy downscale, identity, a flipped sample and an eval-window sample in ONE launch: no state leaks between rows.
    Odd source widths: row starts are unaligned"""
    images = [R.source(11, 13, 1), R.source(16, 701, 2), R.source(32, 41, 3), R.source(75, 97, 4), R.source(61, 47, 5)]
    tab = np.stack([R.row(11, 13, 1, 2, 9, 11, 32, 32, interp=R.BICUBIC),                     # upscale on both axes
                    R.row(16, 701, 0, 0, 16, 701, 32, 32, interp=R.BICUBIC),                  # 701 -> 32 columns, 16 -> 32 rows
                    R.row(32, 41, 0, 5, 32, 32, 32, 32, interp=R.BILINEAR),                   # both passes are the identity
                    R.row(75, 97, 7, 9, 60, 71, 32, 32, interp=R.BILINEAR, flip=1),           # flipped
                    R.eval_row(61, 47, 32, 0.875, R.BICUBIC)])                                # 61 x 47 -> 46 x 36, window at (7, 2)
    assert (int(tab[4]['oy']), int(tab[4]['ox'])) == (7, 2)
    got = _run(images, tab, 32, 32)
    _same(got, R.resize_crop(images, tab, 32, 32), 'mixed batch')
    assert np.array_equal(got[2], images[2][:, 5:37].transpose(2, 0, 1))          # the identity is a copy of the box
    # each row alone gives the same bytes as in the batch
    for b in (1, 3, 4):
        _same(_run([images[b]], tab[b:b + 1], 32, 32), got[b:b + 1], f'row {b} alone')
    # the flip mirrors the resized image: the same row without it, mirrored
    plain = tab[3:4].copy()
    plain['flip'] = 0
    _same(_run([images[3]], plain, 32, 32)[:, :, :, ::-1], got[3:4], 'flip')


def test_real_shapes_375x500_to_224():
    import random
    import imagenet_models_amd as A
    images = [R.source(375, 500, 10), R.source(375, 499, 11), R.source(500, 375, 12)]
    rrc = A.RandomResizedCrop(224, rng=random.Random(2), torch_gen=torch.Generator().manual_seed(2))
    tab = rrc.sample([im.shape[0] for im in images], [im.shape[1] for im in images])
    tab[0]['interp'], tab[1]['interp'] = R.BICUBIC, R.BILINEAR
    got = _run(images, tab, 224, 224)
    _same(got, R.resize_crop(images, tab, 224, 224), tab.tolist())
    ev = R.eval_table([375, 375, 500], [500, 499, 375], 224, 0.875, 'bicubic')
    _same(_run(images, ev, 224, 224), R.resize_crop(images, ev, 224, 224), 'eval')


def test_bad_arguments_are_refused_before_any_launch():
    from imagenet_models_amd import _lib
    lib = _lib.load()
    B, OH, OW = 2, 32, 32
    images = [R.source(40, 50, 1), R.source(33, 47, 2)]
    data, offsets = _pack(images)
    tab = np.stack([R.row(40, 50, 1, 2, 30, 40, OH, OW), R.row(33, 47, 0, 0, 33, 47, OH, OW, interp=R.BILINEAR, flip=1)])
    tab['src_off'] = offsets
    need = lib.ga_resize_crop_work_bytes(tab.ctypes.data, B, OH, OW)
    dev = torch.zeros(B * 64 + 64, dtype=torch.uint8, device='cuda')
    dev[:B * 64] = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    out = torch.full((B * 3 * OH * OW + 64,), 7, dtype=torch.uint8, device='cuda')
    work = torch.full((need + 64,), 7, dtype=torch.uint8, device='cuda')
    S, T, O, WK = data.data_ptr(), dev.data_ptr(), out.data_ptr(), work.data_ptr()
    assert T % 16 == 0 and O % 16 == 0 and WK % 16 == 0

    def call(src=S, src_bytes=data.numel(), rows=T, o=O, work=WK, work_bytes=need, B=B, OH=OH, OW=OW):
        return lib.ga_resize_crop(src, src_bytes, rows, o, work, work_bytes, B, OH, OW, None)

    bad = dict(null_src=dict(src=None), null_rows=dict(rows=None), null_out=dict(o=None), null_work=dict(work=None), no_bytes=dict(src_bytes=0),
               zero_B=dict(B=0), big_B=dict(B=65536), ow_not_x4=dict(OW=30), zero_OH=dict(OH=0), tall=dict(OH=32768), wide=dict(OW=32768),
               out_misaligned=dict(o=O + 4), rows_misaligned=dict(rows=T + 8), work_misaligned=dict(work=WK + 2), work_too_small=dict(work_bytes=64))
    for name, kw in bad.items():
        assert call(**kw) == GA_ERR_BAD_ARG, name
        assert 'ga_resize_crop' in _lib.last_error(), name
    torch.cuda.synchronize()
    assert (out == 7).all() and (work == 7).all()            # nothing was launched
    # a workspace the host cannot see to be too small for the DEVICE table: only the region offsets are written, no pixel
    small = need - 16
    assert call(work_bytes=small) == 0
    torch.cuda.synchronize()
    assert (out == 7).all() and (work[32:] == 7).all()
    assert work[:24].view(torch.int64).tolist()[2] == need
    assert call() == 0                                        # the good call
    torch.cuda.synchronize()
    got = out[:B * 3 * OH * OW].view(B, 3, OH, OW).cpu().numpy()
    _same(got, R.resize_crop(images, tab, OH, OW), 'good call')
    assert (out[B * 3 * OH * OW:] == 7).all() and (work[need:] == 7).all()          # nothing behind the buffers is written
