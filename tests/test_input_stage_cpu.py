"""CPU: the one object that holds the order of the training input stage (imagenet_models_amd.InputStage) -- what it takes, what it
refuses, without a device -- and the helpers the two scripts share from the package."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_refuses_two_mixup_orders():
    import imagenet_models_amd as A
    with pytest.raises(ValueError, match='two orders of the same augmentation: pass one of them'):
        A.InputStage(mixup_fn=A.Mixup(num_classes=10), collate_mixup=A.FastCollateMixup(num_classes=10))


def test_stage_says_what_it_takes():
    import imagenet_models_amd as A
    erase, aa, crop = A.RandomErasing(0.25, mode='pixel'), A.RandAugment('rand-m9-mstd0.5-inc1'), A.RandomResizedCrop(32)
    assert A.InputStage().takes == 'any'
    assert A.InputStage(auto_augment=aa).takes == 'uint8'
    assert A.InputStage(crop=crop).takes == 'ragged' and A.InputStage(crop=crop, auto_augment=aa).takes == 'ragged'
    assert A.InputStage(random_erasing=erase).takes == 'any'
    assert A.InputStage(collate_mixup=A.FastCollateMixup(num_classes=10), random_erasing=erase).takes == 'uint8'
    assert A.InputStage(mixup_fn=A.Mixup(num_classes=10)).takes == 'any'
    s = A.InputStage(crop, aa, None, erase, None)
    assert (s.crop, s.auto_augment, s.collate_mixup, s.random_erasing, s.mixup_fn) == (crop, aa, None, erase, None)


def test_stage_type_errors_need_no_device():
    import imagenet_models_amd as A
    ragged = A.RaggedBatch(torch.zeros(48, dtype=torch.uint8), [0], [4], [4])
    u8, f32 = torch.zeros(2, 3, 32, 32, dtype=torch.uint8), torch.zeros(2, 3, 32, 32)
    aa, crop = A.RandAugment('rand-m9-mstd0.5-inc1'), A.RandomResizedCrop(32)
    y = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match='RaggedBatch needs TrainStep'):
        A.InputStage()(ragged, y, None)
    with pytest.raises(TypeError, match='takes a RaggedBatch'):
        A.InputStage(crop=crop)(u8, y, None)
    with pytest.raises(TypeError, match='augments the uint8 batch'):
        A.InputStage(auto_augment=aa)(f32, y, None)
    with pytest.raises(TypeError, match='augments the uint8 batch'):
        A.InputStage(auto_augment=aa, collate_mixup=A.FastCollateMixup(num_classes=10))(f32, y, None)
    with pytest.raises(TypeError, match='mixes the uint8 batch'):
        A.InputStage(collate_mixup=A.FastCollateMixup(num_classes=10))(f32, y, None)
    A.InputStage(crop=crop).check(ragged)
    A.InputStage(auto_augment=aa).check(u8)
    for x in (u8, f32):
        A.InputStage().check(x)
        got_x, got_y = A.InputStage()(x, y, None)          # nothing configured: the batch goes through as it is
        assert got_x is x and got_y is y


def test_helpers_are_in_the_package_and_in_train(tmp_path):
    import imagenet_models_amd as A
    sys.path.insert(0, ROOT)
    import train
    assert train.split_dir is A.split_dir and train.parse_hw is A.parse_hw and train.synthetic_ragged is A.synthetic_ragged
    assert A.split_dir.__module__ == 'imagenet_models_amd.dataset' and A.evaluate_folder.__module__ == 'imagenet_models_amd.dataset'
    assert A.parse_hw.__module__ == A.synthetic_ragged.__module__ == 'imagenet_models_amd.resize_crop'
    os.mkdir(tmp_path / 'train')
    assert A.split_dir(str(tmp_path), 'train') == os.path.join(tmp_path, 'train') and A.split_dir(str(tmp_path), 'val') == str(tmp_path)
    with pytest.raises(NotADirectoryError):
        A.split_dir(str(tmp_path / 'nothing'), 'train')
    assert A.parse_hw('375x500') == (375, 500) and A.parse_hw('2X3') == (2, 3)
    for text, why in (('375', 'HxW, two positive integers'), ('ax5', 'HxW, two positive integers'), ('1x5', 'from 2 up to 21844'),
                      ('5x21846', 'from 2 up to 21844')):
        with pytest.raises(ValueError, match=why):
            A.parse_hw(text)
    # what synthetic_ragged builds: sizes within [0.5, 1.5] of the nominal one, every image on a 16-byte boundary, no gaps beyond that
    r = A.synthetic_ragged(5, (120, 96), 3, 'cpu')
    assert len(r) == 5 and all(60 <= h <= 180 for h in r.heights) and all(48 <= w <= 144 for w in r.widths)
    sizes = [(3 * int(h) * int(w) + 15) // 16 * 16 for h, w in zip(r.heights, r.widths)]
    assert r.offsets.tolist() == [sum(sizes[:k]) for k in range(5)] and r.data.numel() == sum(sizes) and r.data.dtype == torch.uint8
    again = train.synthetic_ragged(5, (120, 96), 3, 'cpu')
    assert again.offsets.tolist() == r.offsets.tolist() and torch.equal(again.data, r.data)


def test_validate_does_not_import_train():
    code = "import sys; sys.path.insert(0, %r); import validate; assert 'train' not in sys.modules, 'validate imports train'" % ROOT
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
