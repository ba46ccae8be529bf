"""CPU: the host side of the folder loader (imagenet_models_amd.dataset): ImageFolder's order and class indices on a tmp_path tree --
timm's folder parser: classes sorted, files in natural order -- and FolderLoader's index plan: per-epoch permutations, rank slices
that are disjoint and cover every kept sample once, the dropped training tail, the padded evaluation tail and its real count.  No
file is decoded here."""
import os

import numpy as np
import pytest

from imagenet_models_amd.dataset import FolderLoader, ImageFolder, natural_key


def _tree(root, spec):
    for cls, files in spec.items():
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for f in files:
            with open(os.path.join(root, cls, f), 'wb') as h:
                h.write(f.encode())


def test_image_folder_orders_classes_and_files_as_timm_does(tmp_path):
    root = str(tmp_path)
    _tree(root, {'n02': ['img10.jpg', 'img2.JPEG', 'img1.png', 'notes.txt'], 'n01': ['b.jpg', 'a.jpeg'], 'n10': ['x.jpg'],
                 'empty': ['readme.md']})
    open(os.path.join(root, 'stray.jpg'), 'wb').close()              # a file outside every class directory is no sample
    ds = ImageFolder(root)
    assert ds.classes == ['n01', 'n02', 'n10'] and ds.class_to_idx == {'n01': 0, 'n02': 1, 'n10': 2}
    rel = [(os.path.relpath(p, root), t) for p, t in ds.samples]
    assert rel == [('n01/a.jpeg', 0), ('n01/b.jpg', 0), ('n02/img1.png', 1), ('n02/img2.JPEG', 1), ('n02/img10.jpg', 1), ('n10/x.jpg', 2)]
    assert len(ds) == 6 and ds.read(4) == (b'img10.jpg', 1)
    assert natural_key('img10.jpg') > natural_key('IMG2.jpg')
    with pytest.raises(FileNotFoundError):
        ImageFolder(os.path.join(root, 'absent'))
    os.makedirs(os.path.join(root, 'hollow', 'c'))
    with pytest.raises(RuntimeError, match='no .jpg'):
        ImageFolder(os.path.join(root, 'hollow'))


class _Set:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize('n,batch,world', [(103, 8, 1), (103, 8, 3), (64, 8, 2), (17, 4, 4)])
def test_training_rank_slices_are_disjoint_and_cover_every_kept_sample_once(n, batch, world):
    loaders = [FolderLoader(_Set(n), batch, None, train=True, seed=5, rank=r, world=world) for r in range(world)]
    kept = n // (world * batch) * world * batch
    for epoch in (0, 1, 7):
        parts = [ld.indices(epoch) for ld in loaders]
        assert all(len(p) == kept // world == len(ld) * batch for p, ld in zip(parts, loaders))
        allidx = np.concatenate(parts)
        assert len(set(allidx.tolist())) == kept == len(allidx) and allidx.min() >= 0 and allidx.max() < n
        plan = loaders[0].batches(epoch)
        assert len(plan) == len(loaders[0]) and all(real == batch and len(part) == batch for part, real in plan)
    a, b = loaders[0].indices(0), loaders[0].indices(1)
    assert not np.array_equal(a, b)                                    # another epoch, another permutation ...
    assert np.array_equal(a, FolderLoader(_Set(n), batch, None, train=True, seed=5, rank=0, world=world).indices(0))   # ... from the seed
    assert not np.array_equal(a, FolderLoader(_Set(n), batch, None, train=True, seed=6, rank=0, world=world).indices(0))
    loaders[0].set_epoch(7)
    assert np.array_equal(loaders[0].indices(), loaders[0].indices(7))


def test_training_needs_one_full_batch():
    with pytest.raises(ValueError, match='no full batch'):
        FolderLoader(_Set(7), 4, None, train=True, world=2, rank=1)
    with pytest.raises(ValueError):
        FolderLoader(_Set(7), 4, None, rank=2, world=2)


@pytest.mark.parametrize('n,batch,world', [(10, 4, 1), (8, 4, 1), (10, 4, 3), (3, 4, 2)])
def test_evaluation_keeps_order_pads_the_tail_and_reports_the_real_count(n, batch, world):
    seen = []
    for r in range(world):
        ld = FolderLoader(_Set(n), batch, None, train=False, rank=r, world=world)
        mine = list(range(r, n, world))
        plan = ld.batches()
        assert len(plan) == len(ld) == -(-len(mine) // batch)
        flat = []
        for part, real in plan:
            assert len(part) == batch and 1 <= real <= batch
            assert (part[real:] == part[real - 1]).all()               # the tail repeats the last sample
            flat += part[:real].tolist()
        assert flat == mine                                            # order kept, nothing twice
        assert sum(real for _, real in plan) == len(mine)
        seen += flat
    assert sorted(seen) == list(range(n))
