"""GPU: train.py / validate.py on an image folder of the fixture's JPEG files (tests/golden/jpeg_pil.npz): the folder loader, the
JPEG decoder and the crops in front of the engines, and the refusal both CLIs keep when they are given neither a directory nor
--synthetic."""
import json
import os
import subprocess
import sys

import pytest

import _jpeg_ref as J
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, timeout=600, ok=True):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)       # a child process under its own time limit
    if ok:
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r, r.stdout + r.stderr


def _folder(root, n=10, per_class=5):
    files = [c for c in J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]
             if c['kind'] == 'ok' and c['name'].startswith(('64x80', '37x53', '48x31', '17x33'))][:n]
    assert len(files) == n
    for k, c in enumerate(files):
        d = os.path.join(root, f'class{k // per_class}')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f'{c["name"]}.jpg'), 'wb') as f:
            f.write(c['data'])


def test_validate_cli_counts_exactly_the_folders_images(tmp_path):
    _folder(os.path.join(tmp_path, 'validation'))
    res = os.path.join(tmp_path, 'r.json')
    _, out = _run([sys.executable, 'validate.py', str(tmp_path), '--model', 'mobilenet_v1', '-b', '4', '-j', '2',
                   '--results-file', res])
    r = json.load(open(res))
    assert r['samples'] == 10 and r['classes'] == 2 and r['pil_fallbacks'] == 0 and r['model'] == 'mobilenet_v1'
    assert 0.0 <= r['top1'] <= r['top5'] <= 100.0 and round(r['top1'] * 10) % 100 == 0       # a multiple of 1 / 10
    assert 'over 10 images' in out
    # the root itself where it has no split directory, under another split name
    _, out = _run([sys.executable, 'validate.py', os.path.join(tmp_path, 'validation'), '--split', 'val', '--model', 'mobilenet_v1',
                   '--num-classes', '40', '-b', '4'])
    assert 'over 10 images' in out


def test_train_cli_trains_and_evaluates_from_a_folder(tmp_path):
    _folder(os.path.join(tmp_path, 'train'))
    _folder(os.path.join(tmp_path, 'validation'), n=6, per_class=3)
    _, out = _run([sys.executable, 'train.py', str(tmp_path), '--model', 'mobilenet_v1', '-b', '4', '--epochs', '1',
                   '--log-interval', '1', '-j', '2'])
    assert '*** epoch 0: train loss' in out and 'nan' not in out.lower()
    assert '10 training images in 2 classes, 6 validation images' in out and 'evaluated 6 images' in out


def test_both_clis_still_refuse_without_a_directory_or_synthetic():
    r, out = _run([sys.executable, 'train.py', '--model', 'mobilenet_v1'], ok=False)
    assert r.returncode != 0 and 'train.py: only --synthetic data is shipped (no dataset / network in this environment)' in out
    r, out = _run([sys.executable, 'validate.py', '--model', 'mobilenet_v1'], ok=False)
    assert r.returncode != 0 and 'validate.py: only --synthetic data is shipped' in out
