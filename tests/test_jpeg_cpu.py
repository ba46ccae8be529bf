"""CPU: the host side of the JPEG path that needs no device -- the C ABI of the five ga_jpeg_* entry points and the host check of a
table (one message per reason), the table row layout shared by jpeg.py, the kernels and the restatement, JpegDecoder's refusals
(they come from the probe, ahead of any device call), and the flags / refusals of train.py and validate.py."""
import os
import sys

import numpy as np
import pytest

import _jpeg_ref as J
from conftest import GOLDEN, ROOT


@pytest.fixture(scope='module')
def golden():
    return J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]


def test_abi_surface_and_row_layout():
    import imagenet_models_amd as A
    from imagenet_models_amd import _lib, jpeg, ops
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    for name in ('ga_jpeg_probe', 'ga_jpeg_entropy_decode', 'ga_jpeg_check_table', 'ga_jpeg_reconstruct'):
        assert f'int {name}(' in hdr and name in _lib.exported_symbols()
    assert 'size_t ga_jpeg_work_bytes(' in hdr and 'ga_jpeg_work_bytes' in _lib.exported_symbols()
    assert hasattr(ops.Plan, 'jpeg_reconstruct')
    assert A.JpegDecoder.__module__ == 'imagenet_models_amd.jpeg' and A.FolderLoader.__module__ == 'imagenet_models_amd.dataset'
    assert jpeg.ROW == J.ROW and jpeg.ROW.itemsize == 64 and jpeg.INFO_LEN == J.INFO_LEN
    assert (jpeg.OK, jpeg.UNSUPPORTED, jpeg.CORRUPT) == (J.OK, J.UNSUPPORTED, J.CORRUPT) == (0, 1, 2)
    # the host stage is a header of its own, free of HIP, that a stand-alone program compiles
    host = open(os.path.join(ROOT, 'imagenet-models_amd', 'csrc', 'jpeg_host.h')).read()
    assert '#include <hip' not in host and 'common.h' not in host and 'malloc' not in host
    assert '#include "jpeg_host.h"' in open(os.path.join(ROOT, 'imagenet-models_amd', 'csrc', 'jpeg.hip')).read()
    assert 'jpeg_host.h' in open(os.path.join(ROOT, 'tools', 'jpeg_host_fuzz.cpp')).read()


def test_check_table_names_every_reason(golden):
    from imagenet_models_amd import _lib
    lib = _lib.load()
    c = next(c for c in golden if c['name'] == '37x53_420_q95')
    st, info = J.probe(lib, c['data'])
    assert st == J.OK
    good = np.array([J.table_row(info)], dtype=J.ROW)
    n, dstb = int(info[5]), 3 * 37 * 53
    assert n == 64 * 4 * 3 * 6 and lib.ga_jpeg_check_table(good.ctypes.data, 1, n, 192, n, dstb) == 0
    assert lib.ga_jpeg_work_bytes(good.ctypes.data, 1) == n and lib.ga_jpeg_work_bytes(None, 1) == 0
    for field, value, why in (('width', 0, 'not a baseline image'), ('height', 32768, 'not a baseline image'), ('ncomp', 2, 'not a baseline image'),
                              ('hs', 3, 'not a baseline image'), ('vs', 1, 'not a baseline image'), ('mcus_w', 5, 'not a baseline image'),
                              ('coef_off', 64, 'coefficients outside'), ('coef_off', 4, 'coefficients outside'), ('coef_off', -8, 'coefficients outside'),
                              ('qt_off', 8, 'tables outside'), ('qt_off', 4, 'tables outside'), ('work_off', 16, 'planes outside'),
                              ('work_off', 8, 'planes outside'), ('dst_off', 16, 'image outside'), ('dst_off', 8, 'image outside')):
        bad = good.copy()
        bad[0][field] = value
        assert lib.ga_jpeg_check_table(bad.ctypes.data, 1, n, 192, n, dstb) == -1, (field, value)
        assert 'ga_jpeg_check_table: row 0' in _lib.last_error() and why in _lib.last_error(), (field, _lib.last_error())
        if why == 'not a baseline image':
            assert lib.ga_jpeg_work_bytes(bad.ctypes.data, 1) == 0
    grey2 = good.copy()
    grey2[0]['ncomp'] = 1                                       # a grey image is sampled 1 x 1
    assert lib.ga_jpeg_check_table(grey2.ctypes.data, 1, n, 192, n, dstb) == -1
    assert lib.ga_jpeg_check_table(None, 1, n, 192, n, dstb) == -1 and lib.ga_jpeg_check_table(good.ctypes.data, 0, n, 192, n, dstb) == -1
    assert lib.ga_jpeg_check_table(good.ctypes.data, 65536, n, 192, n, dstb) == -1
    assert lib.ga_jpeg_reconstruct(None, 1, None, None, None, None, None) == -1 and 'device pointers' in _lib.last_error()


def test_decoder_refuses_from_the_probe_ahead_of_any_device_call(golden):
    import imagenet_models_amd as A
    prog = next(c for c in golden if c['kind'] == 'fallback')['data']
    cmyk = next(c for c in golden if c['kind'] == 'refuse')['data']
    dec = A.JpegDecoder(threads=2, fallback=None)
    assert dec.threads == 2 and A.JpegDecoder(threads=0).threads == 1 and A.JpegDecoder(threads=64).threads == 16
    for k, data in ((0, prog), (0, cmyk), (0, b'\x89PNG\r\n\x1a\n' + bytes(32))):
        with pytest.raises(ValueError, match=f'sample {k} is not a baseline JPEG.*fallback=None'):
            dec.decode([data])
    with pytest.raises(ValueError, match='sample 0 is a corrupt JPEG'):
        dec.decode([b'\xff\xd8\xff'])
    with pytest.raises(ValueError, match='empty'):
        dec.decode([])
    with pytest.raises(TypeError, match='sample 0 is str'):
        dec.decode(['n01440764_10026.JPEG'])
    with pytest.raises(ValueError, match="'pil' or None"):
        A.JpegDecoder(fallback='turbo')
    assert dec.fallbacks == 0 and dec.decoded == 0


def _main(monkeypatch, script, *args):
    """the script's main() in this process -> the SystemExit message (every refusal here comes ahead of any device call)"""
    import importlib
    mod = importlib.import_module(script)
    monkeypatch.setattr(sys, 'argv', [script + '.py', *args])
    with pytest.raises(SystemExit) as e:
        mod.main()
    return mod, str(e.value)


def test_cli_flags_and_refusals(tmp_path, monkeypatch):
    train, msg = _main(monkeypatch, 'train')
    assert msg == 'train.py: only --synthetic data is shipped (no dataset / network in this environment)'
    validate, msg = _main(monkeypatch, 'validate')
    assert msg == 'validate.py: only --synthetic data is shipped'
    assert all(f in train.parser.format_help() for f in ('--train-split', '--val-split', '-j N', '--workers'))
    assert all(f in validate.parser.format_help() for f in ('--split', '-j N', '--workers'))
    a = train.parser.parse_args(['/data'])
    assert (a.data_dir, a.train_split, a.val_split, a.workers, a.synthetic) == ('/data', 'train', 'validation', 8, False)
    assert 'is not a directory' in _main(monkeypatch, 'train', os.path.join(tmp_path, 'absent'))[1]
    assert 'is not a directory' in _main(monkeypatch, 'validate', os.path.join(tmp_path, 'absent'))[1]
    os.makedirs(os.path.join(tmp_path, 'train', 'c0'))
    assert _main(monkeypatch, 'train', str(tmp_path))[1].startswith('train.py: ImageFolder: no .jpg')
    assert _main(monkeypatch, 'validate', str(tmp_path))[1].startswith('validate.py: ImageFolder: no .jpg')
    assert train.split_dir(str(tmp_path), 'train') == os.path.join(tmp_path, 'train') and train.split_dir(str(tmp_path), 'val') == str(tmp_path)


def test_docs_name_the_decoder():
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'ga_jpeg_reconstruct' in design and 'ga_jpeg_reconstruct' in readme and 'validate.py /data/imagenet' in readme
    assert 'Huffman decoding on the device' in design and 'DCT-domain' in design and '--aug-repeats' in design
    assert os.path.exists(os.path.join(ROOT, 'profiles', 'jpeg_decode_trace.md'))
