"""GPU: repeated augmentation through the folder loader -- FolderLoader(aug_repeats=3) on a 12-file folder of the fixture's JPEGs
(4:4:4, 4:2:2, 4:2:0, odd sizes, grey, 1 x 1, a restart-marker file and the progressive one that goes through the PIL fallback), batch
8, selected_round 0: each distinct file of a batch is decoded once and the copies are entries that share its bytes; the crop, and the
whole input stage behind it, give bit for bit what they give on the same batch decoded entry by entry; train.py --aug-repeats 3 trains.
Every comparison is exact."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _jpeg_ref as J
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

NAMES = ['64x80_444_q95', '64x80_422_q95', '64x80_420_q95', '37x53_444_q95', '37x53_420_q1', '48x31_422_q100', '17x33_grey_q50',
         '64x80_grey_q90', '1x1_420_q95', '1x1_grey_q75', '37x53_420_q75_progressive', '37x53_420_q75_restart3']
BATCH = 8


def _write(root, names, per_class):
    cases = {c['name']: c for c in J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]}
    for k, name in enumerate(names):
        assert cases[name]['kind'] in ('ok', 'fallback')
        d = os.path.join(root, f'class{k // per_class}')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f'{k:02d}_{name}.jpg'), 'wb') as f:
            f.write(cases[name]['data'])


@pytest.fixture(scope='module')
def fed(tmp_path_factory):
    """the loader's batches of the fewest epochs whose batches hold all 12 files: [(index list, RaggedBatch, labels, files decoded
    for it, of them by PIL)], with the dataset and the decoder"""
    import imagenet_models_amd as A
    root = str(tmp_path_factory.mktemp('repeats'))
    _write(root, NAMES, per_class=4)
    ds = A.ImageFolder(root)
    assert len(ds) == 12 and len(ds.classes) == 3
    dec = A.JpegDecoder(threads=2)
    ld = A.FolderLoader(ds, BATCH, dec, train=True, seed=0, aug_repeats=3, selected_round=0)
    assert len(ld) == 1
    epochs, missing = [], set(range(12))
    for e in range(200):                                # the order is a pure function of (seed, epoch): chosen on the host
        new = set(ld.batches(e)[0][0].tolist()) & missing
        if new:
            epochs.append(e)
            missing -= new
        if not missing:
            break
    assert not missing and len(epochs) <= 12
    out = []
    for e in epochs:
        ld.set_epoch(e)
        before = (dec.decoded, dec.fallbacks)
        got = list(ld)
        torch.cuda.synchronize()
        assert len(got) == 1
        out.append((ld.batches(e)[0][0], got[0][0], got[0][1], dec.decoded - before[0], dec.fallbacks - before[1]))
    return ds, dec, out


def _bytes(rb, k):
    o, n = int(rb.offsets[k]), 3 * int(rb.heights[k]) * int(rb.widths[k])
    return rb.data[o:o + n]


def test_each_distinct_file_of_a_batch_is_decoded_once(fed):
    import imagenet_models_amd as A
    ds, dec, batches = fed
    alone = A.JpegDecoder(threads=1)
    single = {}
    prog = NAMES.index('37x53_420_q75_progressive')
    seen_prog = 0
    for part, rb, y, decoded, fallbacks in batches:
        assert isinstance(rb, A.RaggedBatch) and len(rb) == BATCH == len(part)
        distinct = list(dict.fromkeys(part.tolist()))
        assert 3 <= len(distinct) <= 4                                   # 8 entries of an order that writes every file 3 times
        assert decoded == len(distinct) and fallbacks == int(prog in distinct)
        seen_prog += int(prog in distinct)
        assert y.tolist() == [ds.samples[i][1] for i in part]
        for k, i in enumerate(part.tolist()):
            for j, other in enumerate(part.tolist()):                    # entries of one file share its bytes, others do not
                assert (rb.offsets[k] == rb.offsets[j]) == (i == other)
            if i not in single:
                single[i] = alone.decode([ds.read(i)[0]])
            one = single[i]
            assert (rb.heights[k], rb.widths[k]) == (one.heights[0], one.widths[0])
            assert torch.equal(_bytes(rb, k), _bytes(one, 0))
        # the buffer holds the distinct files only
        offs, total = A.resize_crop.pack_offsets([single[i].heights[0] for i in distinct], [single[i].widths[0] for i in distinct])
        assert rb.data.numel() == total and sorted(set(rb.offsets.tolist())) == offs.tolist()
    assert seen_prog >= 1 and len(single) == 12                          # the PIL fallback was among the shared sources


def _entry_by_entry(ds, part):
    """the batch decoded as the loader does without aug_repeats: every entry on its own"""
    import imagenet_models_amd as A
    return A.JpegDecoder(threads=2).decode([ds.read(int(i))[0] for i in part])


def test_crop_of_shared_sources_equals_the_crop_of_the_batch_decoded_entry_by_entry(fed):
    import imagenet_models_amd as A
    ds, dec, batches = fed
    rrc = A.RandomResizedCrop(64, rng=random.Random(3), torch_gen=torch.Generator().manual_seed(3))
    differed = 0
    for part, rb, y, _, _ in batches:
        per = _entry_by_entry(ds, part)
        assert np.array_equal(per.heights, rb.heights) and np.array_equal(per.widths, rb.widths)
        assert len(set(per.offsets.tolist())) == BATCH > len(set(rb.offsets.tolist()))
        table = rrc.sample(rb.heights, rb.widths)                       # ONE table; its src_off rebased per batch
        big = [k for k in range(BATCH - 1) if part[k] == part[k + 1] and rb.heights[k] * rb.widths[k] >= 37 * 53]
        if big:                                                         # two copies of one file under different rows: the mirror image
            k = big[0]
            table[k + 1] = table[k]
            table[k + 1]['flip'] = 1 - table[k]['flip']
        shared, each = table.copy(), table.copy()
        shared['src_off'], each['src_off'] = rb.offsets, per.offsets
        got = rrc(rb, table=shared).clone()
        want = rrc(per, table=each).clone()
        assert got.shape == (BATCH, 3, 64, 64) and got.dtype == torch.uint8
        assert torch.equal(got, want), int((got != want).sum())
        if big:
            assert not torch.equal(got[k], got[k + 1])
            differed += 1
        # drawn from the loader's own batch, the table points at the shared sources
        rrc(rb)
        assert np.array_equal(rrc.last['src_off'], rb.offsets)
    assert differed >= 1


def test_full_input_stage_is_the_same_on_both_batches(fed):
    import imagenet_models_amd as A
    ds, dec, batches = fed
    py, npr, tg, py_re = random.Random(), np.random.RandomState(), torch.Generator(), random.Random()
    torch.manual_seed(0)
    m = A.create_model('mobilenet_v1', num_classes=40).cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    era = A.RandomErasing(probability=1.0, mode='pixel', max_count=1, num_splits=0, seed=11, rng=py_re)
    step = A.TrainStep(m, opt, BATCH, lam=0.0,
                       crop=A.RandomResizedCrop(64, rng=py, torch_gen=tg),
                       auto_augment=A.RandAugment('rand-m9-mstd0.5-inc1', rng=py, np_rng=npr),
                       collate_mixup=A.FastCollateMixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=40, rng=npr),
                       random_erasing=era)

    def stage(rb, y, seed):
        py.seed(seed), npr.seed(seed), tg.manual_seed(seed), py_re.seed(seed)
        random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)           # the global generators too: nothing may drift
        era.offset = 0
        x, target = step.input_stage(rb, y, step.eng)
        torch.cuda.synchronize()
        return x.clone(), target.clone(), step.input_stage.crop.last.copy()

    for n, (part, rb, y, _, _) in enumerate(batches[:3]):
        per = _entry_by_entry(ds, part)
        x1, t1, tab1 = stage(rb, y, 20 + n)
        x2, t2, tab2 = stage(per, y, 20 + n)
        for f in tab1.dtype.names:                                      # no draw moved: the tables differ in src_off only
            assert np.array_equal(tab1[f], tab2[f]) == (f != 'src_off'), f
        assert x1.shape == (BATCH, 3, 64, 64) and x1.dtype == torch.float32 and t1.shape == (BATCH, 40)
        assert torch.equal(x1, x2) and torch.equal(t1, t2)
        assert torch.isfinite(x1).all()


def test_train_cli_trains_with_repeats_from_a_folder(tmp_path):
    # the 10-file folder of tests/test_jpeg_cli_gpu.py
    names = [c['name'] for c in J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]
             if c['kind'] == 'ok' and c['name'].startswith(('64x80', '37x53', '48x31', '17x33'))][:10]
    _write(os.path.join(tmp_path, 'train'), names, per_class=5)
    _write(os.path.join(tmp_path, 'validation'), names[:6], per_class=3)
    r = subprocess.run([sys.executable, 'train.py', str(tmp_path), '--model', 'mobilenet_v1', '-b', '4', '--epochs', '1', '--log-interval',
                        '1', '-j', '2', '--aug-repeats', '3', '--selected-round', '0'], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert '*** epoch 0: train loss' in out and 'nan' not in out.lower()
    assert '10 training images in 2 classes, 6 validation images' in out and 'evaluated 6 images' in out
    # 10 samples in 2 batches of 4: [a a a b] [b b c c] -- 3 distinct files, 2 decoded per batch; the evaluation decodes 2 x 4
    assert '--aug-repeats 3 (selected_round 0): 2 batches per epoch from 3 distinct files' in out
    assert '0 of 12 files so far went through the PIL fallback' in out
