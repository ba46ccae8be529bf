"""GPU: train.py / validate.py on decoded synthetic sources (--synthetic-source): the random-resized crop + flip, RandAugment and the
collate-time mixup on the device for training; Resize + CenterCrop and the normalisation for evaluation."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, timeout=600):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)       # a child process under its own time limit
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout + r.stderr


def test_train_cli_crops_decoded_sources():
    out = _run([sys.executable, 'train.py', '--synthetic', '--synthetic-source', '120x96', '--model', 'mobilenet_v1', '--num-classes', '40',
                '-b', '8', '--epochs', '1', '--steps-per-epoch', '2', '--log-interval', '1', '--aa', 'rand-m9-mstd0.5-inc1', '--mixup', '0.8',
                '--cutmix', '1.0', '--collate-mixup', '--scale', '0.08', '1.0', '--ratio', '0.75', '1.3333', '--hflip', '0.5'])
    assert '*** epoch 0: train loss' in out and 'nan' not in out.lower()


def test_validate_cli_resizes_and_centre_crops(tmp_path):
    res = os.path.join(tmp_path, 'r.json')
    out = _run([sys.executable, 'validate.py', '--synthetic', '--synthetic-source', '120x96', '--crop-pct', '0.875', '--model', 'mobilenet_v1',
                '--num-classes', '40', '-b', '8', '--batches', '2', '--results-file', res])
    assert 'Acc@1' in out
    assert json.load(open(res))['model'] == 'mobilenet_v1'
