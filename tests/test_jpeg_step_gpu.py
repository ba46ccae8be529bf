"""GPU: imagenet_models_amd.JpegDecoder in front of the existing input stage: decoding the fixture's files gives the crops the same
uint8 batch, bit for bit, as packing the fixture's PIL pixels does; a TrainStep(crop=...) trains from a folder of those files through
FolderLoader; what the device path does not rebuild goes through the PIL fallback or raises."""
import math
import os
import random

import numpy as np
import pytest
import torch

import _jpeg_ref as J
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]


def test_decoder_output_is_the_packed_pil_pixels(golden):
    import imagenet_models_amd as A
    ok = [c for c in golden if c['kind'] == 'ok']
    dec = A.JpegDecoder(threads=4, fallback=None)
    for _ in range(6):                                           # more calls than staging buffers: a slot is reused
        rb = dec.decode([c['data'] for c in ok])
    ref = A.pack_images([c['pixels'] for c in ok])
    assert isinstance(rb, A.RaggedBatch) and len(rb) == len(ok) and dec.fallbacks == 0 and dec.decoded == 6 * len(ok)
    assert np.array_equal(rb.offsets, ref.offsets) and np.array_equal(rb.heights, ref.heights) and np.array_equal(rb.widths, ref.widths)
    got, want = rb.data.cpu().numpy(), ref.data.cpu().numpy()
    for c, o, h, w in zip(ok, rb.offsets, rb.heights, rb.widths):
        assert np.array_equal(got[o:o + 3 * h * w], want[o:o + 3 * h * w]), c['name']
    one = A.JpegDecoder(threads=1, fallback=None).decode([c['data'] for c in ok]).data.cpu().numpy()      # one thread: the same bytes
    for c, o, h, w in zip(ok, rb.offsets, rb.heights, rb.widths):
        assert np.array_equal(one[o:o + 3 * h * w], want[o:o + 3 * h * w]), c['name']
    assert A.JpegDecoder(threads=99).threads == 16
    with pytest.raises(ValueError, match='empty'):
        dec.decode([])
    with pytest.raises(TypeError, match='sample 0'):
        dec.decode(['a path is not bytes'])


def test_crops_give_the_same_batch_from_decoded_files_and_from_packed_pixels(golden):
    import imagenet_models_amd as A
    ok = [c for c in golden if c['kind'] == 'ok']
    files, pixels = [c['data'] for c in ok], [c['pixels'] for c in ok]
    dec = A.JpegDecoder(threads=4)
    for size, pct in ((32, 0.875), (16, 1.0)):
        a = A.ResizeCenterCrop(size, pct, 'bicubic')(dec.decode(files)).clone()
        b = A.ResizeCenterCrop(size, pct, 'bicubic')(A.pack_images(pixels))
        assert a.shape == (len(ok), 3, size, size) and torch.equal(a, b), (size, pct, int((a != b).sum()))
    rrc = A.RandomResizedCrop(32, rng=random.Random(3), torch_gen=torch.Generator().manual_seed(3))
    table = rrc.sample([p.shape[0] for p in pixels], [p.shape[1] for p in pixels], A.pack_images(pixels).offsets)
    assert table['flip'].any() and not table['flip'].all()
    a = A.RandomResizedCrop(32)(dec.decode(files), table=table).clone()
    b = A.RandomResizedCrop(32)(A.pack_images(pixels), table=table)
    assert torch.equal(a, b), int((a != b).sum())


def _folder(root, cases, per_class):
    """cases -> root/c0/*.jpg, root/c1/*.jpg ...; returns the labels in the loader's file order"""
    for k, c in enumerate(cases):
        d = os.path.join(root, f'c{k // per_class}')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f'img{k}.jpg'), 'wb') as f:
            f.write(c['data'])


def test_train_step_runs_from_a_folder_of_fixture_files(golden, tmp_path):
    import imagenet_models_amd as A
    big = [c for c in golden if c['kind'] == 'ok' and c['name'].startswith(('64x80', '37x53', '48x31'))][:10]
    _folder(str(tmp_path), big, 5)
    ds = A.ImageFolder(str(tmp_path))
    assert len(ds) == 10 and ds.classes == ['c0', 'c1']
    dec = A.JpegDecoder(threads=2)
    torch.manual_seed(0)
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    rrc = A.RandomResizedCrop(224, rng=random.Random(5), torch_gen=torch.Generator().manual_seed(5))
    step = A.TrainStep(m, opt, 4, lam=0.0, crop=rrc)
    loader = A.FolderLoader(ds, 4, dec, train=True, seed=1)
    losses = []
    for ragged, y in loader:
        assert isinstance(ragged, A.RaggedBatch) and len(ragged) == 4 and y.shape == (4,) and y.dtype == torch.int64 and y.is_cuda
        losses.append(float(step(ragged, y)))
    assert len(losses) == len(loader) == 2 and all(math.isfinite(v) for v in losses), losses
    # evaluation: file order, the tail padded, the real count reported; the decoded bytes are the fixture's
    ev = list(A.FolderLoader(ds, 4, dec, train=False))
    assert [real for _, _, real in ev] == [4, 4, 2] and all(len(r) == 4 for r, _, _ in ev)
    assert torch.cat([y[:real] for _, y, real in ev]).tolist() == [0] * 5 + [1] * 5
    order = [int(os.path.basename(p)[3:-4]) for p, _ in ds.samples]
    first = ev[0][0]
    host = first.data.cpu().numpy()
    for j in range(4):
        want = big[order[j]]['pixels']
        o = first.offsets[j]
        assert np.array_equal(host[o:o + want.size].reshape(want.shape), want)
    last = ev[2][0]
    assert last.heights[1:].tolist() == [last.heights[1]] * 3 and last.widths[1:].tolist() == [last.widths[1]] * 3


def test_unsupported_files_raise_without_a_fallback_and_corrupt_ones_always(golden):
    import imagenet_models_amd as A
    prog = next(c for c in golden if c['kind'] == 'fallback')
    ok = next(c for c in golden if c['name'] == '17x33_420_q95')
    dec = A.JpegDecoder(threads=2, fallback=None)
    with pytest.raises(ValueError, match='sample 1 is not a baseline JPEG'):
        dec.decode([ok['data'], prog['data']])
    with pytest.raises(ValueError, match='sample 0 is a corrupt JPEG'):
        dec.decode([ok['data'][:len(ok['data']) // 2], ok['data']])
    with pytest.raises(ValueError, match='sample 1 is a corrupt JPEG'):
        A.JpegDecoder(threads=2).decode([ok['data'], ok['data'][:40]])
    with pytest.raises(ValueError, match='fallback'):
        A.JpegDecoder(fallback='opencv')


def test_progressive_and_png_files_go_through_the_pil_fallback(golden):
    Image = pytest.importorskip('PIL.Image')
    import io
    import imagenet_models_amd as A
    prog = next(c for c in golden if c['kind'] == 'fallback')
    ok = next(c for c in golden if c['name'] == '17x33_420_q95')
    buf = io.BytesIO()
    Image.fromarray(ok['pixels'], 'RGB').save(buf, 'PNG')
    dec = A.JpegDecoder(threads=2)
    rb = dec.decode([prog['data'], ok['data'], buf.getvalue()])
    assert dec.fallbacks == 2 and dec.decoded == 3
    host = rb.data.cpu().numpy()
    for o, want in zip(rb.offsets, (prog['pixels'], ok['pixels'], ok['pixels'])):
        assert np.array_equal(host[o:o + want.size].reshape(want.shape), want)
    cmyk = next(c for c in golden if c['kind'] == 'refuse')
    assert J.probe(__import__('imagenet_models_amd')._lib.load(), cmyk['data'])[0] == J.UNSUPPORTED
