"""CPU: repeated augmentation on the host -- the order of timm's RepeatAugSampler (dataset.repeat_aug_indices) against the step-by-step
restatement of tests/_repeat_aug_ref.py and a pinned small case, FolderLoader's epoch lengths and refusals with aug_repeats on, its
unchanged plan with aug_repeats off, the resume position, RaggedBatch.take, the table check on rows that share a source, and the
two values the train state records beside the loader position.  No file is decoded here."""
import numpy as np
import pytest
import torch

import _repeat_aug_ref as REF
import _resize_crop_ref as R
from imagenet_models_amd import checkpoint as C
from imagenet_models_amd.dataset import FolderLoader, first_occurrences, repeat_aug_indices
from imagenet_models_amd.resize_crop import RaggedBatch, pack_offsets


class _Set:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize('selected_round', [0, 256])
@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('repeats', [1, 2, 3])
@pytest.mark.parametrize('n', [10, 257, 1000])
def test_order_equals_the_step_by_step_restatement(n, repeats, world, selected_round):
    for seed in (0, 5):
        for rank in range(world):
            got = repeat_aug_indices(n, seed, repeats, rank, world, selected_round)
            assert got.dtype == np.int64 and got.tolist() == REF.repeat_aug_ref(n, seed, repeats, rank, world, selected_round)


def test_pinned_small_case():
    assert repeat_aug_indices(10, 5, 3, 0, 1, 0).tolist() == [1, 1, 1, 4, 4, 4, 9, 9, 9, 6]
    ld = FolderLoader(_Set(10), 4, None, train=True, seed=5, aug_repeats=3, selected_round=0)
    plan = ld.batches(0)
    assert [p.tolist() for p, _ in plan] == [[1, 1, 1, 4], [4, 4, 9, 9]] and all(real == 4 for _, real in plan)
    assert len(ld) == 2 and [len(first_occurrences(p)[0]) for p, _ in plan] == [2, 2] and ld.distinct_files(0) == 3
    assert ld.indices(0).tolist() == [1, 1, 1, 4, 4, 4, 9, 9] == REF.repeat_aug_ref(10, 5, 3, 0, 1, 0)[:8]
    # world a multiple of repeats: the copies go to different ranks, no rank sees a file twice
    assert [repeat_aug_indices(10, 5, 3, r, 3, 0).tolist() for r in range(3)] == [[1, 4, 9, 6]] * 3
    assert [repeat_aug_indices(10, 5, 3, r, 2, 0).tolist() for r in range(2)] == [[1, 1, 4, 9, 9], [1, 4, 4, 9, 6]]
    # the loader seeds with seed + epoch: seed 0 is timm's own order (timm seeds with the epoch alone)
    assert FolderLoader(_Set(10), 4, None, seed=2, aug_repeats=3, selected_round=0).indices(3).tolist() == ld.indices(0).tolist()


def test_first_occurrences_keeps_the_order_of_first_sight():
    distinct, inverse = first_occurrences(np.array([4, 4, 9, 9, 1, 4]))
    assert distinct.tolist() == [4, 9, 1] and inverse.tolist() == [0, 0, 1, 1, 2, 0]
    distinct, inverse = first_occurrences(np.array([7, 3, 5]))
    assert distinct.tolist() == [7, 3, 5] and inverse.tolist() == [0, 1, 2]


def test_epoch_lengths_and_the_selected_round_refusal():
    assert len(FolderLoader(_Set(1000), 1, None, aug_repeats=3).indices(0)) == 768
    for rank in range(8):
        assert len(FolderLoader(_Set(1000), 1, None, aug_repeats=3, rank=rank, world=8).indices(0)) == 96
    ld = FolderLoader(_Set(1000), 100, None, aug_repeats=3)
    assert len(ld) == 7 == len(ld.batches(0)) and len(ld.indices(0)) == 700                  # the ragged tail of 68 is dropped
    assert 700 // 3 <= ld.distinct_files(0) <= 700 // 3 + 1
    assert len(FolderLoader(_Set(1000), 100, None, aug_repeats=3, selected_round=0)) == 10
    with pytest.raises(ValueError, match='selected_round 256'):
        FolderLoader(_Set(200), 4, None, aug_repeats=3)
    assert len(FolderLoader(_Set(200), 4, None, aug_repeats=3, selected_round=0)) == 50
    with pytest.raises(ValueError, match='no full batch'):
        FolderLoader(_Set(3), 4, None, aug_repeats=3, selected_round=0)


@pytest.mark.parametrize('n,batch,world', [(103, 8, 1), (103, 8, 3), (64, 8, 2), (17, 4, 4)])
def test_without_repeats_the_plan_is_the_one_it_was(n, batch, world):
    for rank in range(world):
        ld = FolderLoader(_Set(n), batch, None, train=True, seed=5, rank=rank, world=world, aug_repeats=0)
        assert ld.aug_repeats == 0 and ld.selected_round == 256 and len(ld) == n // (world * batch)
        for epoch in (0, 3):
            order = torch.randperm(n, generator=torch.Generator().manual_seed(5 + epoch)).numpy()
            want = order[:n // (world * batch) * (world * batch)][rank::world]
            assert np.array_equal(ld.indices(epoch), want)
            plan = ld.batches(epoch)
            assert len(plan) == len(ld) and all(real == batch for _, real in plan)
            assert np.array_equal(np.concatenate([p for p, _ in plan]), want)
    ev = FolderLoader(_Set(n), batch, None, train=False, rank=world - 1, world=world)
    assert np.array_equal(ev.indices(), np.arange(n)[world - 1::world]) and len(ev) == -(-len(range(world - 1, n, world)) // batch)


@pytest.mark.parametrize('rank,world', [(0, 1), (1, 2), (2, 3)])
def test_start_position_lists_the_rest_of_the_epoch_with_repeats_on(rank, world):
    ld = FolderLoader(_Set(300), 8, None, train=True, seed=5, rank=rank, world=world, aug_repeats=3)
    for epoch in (0, 3):
        full = ld.batches(epoch)
        assert len(full) == len(ld) == 256 // world // 8
        for k in (0, 1, len(full) // 2, len(full)):
            ld.set_epoch(epoch, start_batch=k)
            plan = ld.plan()
            assert len(plan) == len(full) - k and all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(plan, full[k:]))
    assert not np.array_equal(ld.indices(0), ld.indices(1))


def test_refusals():
    for bad in (1.5, 0.5, -1, '3'):
        with pytest.raises((ValueError, TypeError)):
            FolderLoader(_Set(1000), 4, None, aug_repeats=bad)
    with pytest.raises(ValueError, match='fractional'):
        FolderLoader(_Set(1000), 4, None, aug_repeats=2.5)
    with pytest.raises(ValueError, match='fractional'):
        repeat_aug_indices(1000, 0, 1.5)
    with pytest.raises(ValueError, match='evaluation'):
        FolderLoader(_Set(1000), 4, None, train=False, aug_repeats=3)
    with pytest.raises(ValueError, match='selected_round'):
        FolderLoader(_Set(1000), 4, None, aug_repeats=3, selected_round=-256)


def test_ragged_take_gathers_the_arrays_over_the_same_data():
    hs, ws = [5, 1, 7], [4, 1, 3]
    offsets, total = pack_offsets(hs, ws)
    rb = RaggedBatch(torch.arange(total, dtype=torch.int32).to(torch.uint8), offsets, hs, ws)
    t = rb.take([2, 0, 0, 1, 2])
    assert isinstance(t, RaggedBatch) and len(t) == 5 and t.data is rb.data
    assert t.offsets.tolist() == [offsets[2], 0, 0, offsets[1], offsets[2]] and t.offsets.dtype == np.int64
    assert t.heights.tolist() == [7, 5, 5, 1, 7] and t.widths.tolist() == [3, 4, 4, 1, 3] and t.heights.dtype == np.int32
    assert rb.offsets.tolist() == offsets.tolist() and len(rb) == 3                       # the source is left as it was
    same = rb.take(np.arange(3))
    assert same.offsets.tolist() == rb.offsets.tolist() and same.heights.tolist() == hs
    with pytest.raises(IndexError):
        rb.take([3])


def test_check_table_accepts_rows_that_share_a_source():
    from imagenet_models_amd import _lib
    lib = _lib.load()
    src_bytes = 16 + 3 * 64 * 48
    base = dict(src_h=64, src_w=48, vh=32, vw=32, oy=0, ox=0, src_off=16)
    rows = np.stack([R.row(top=4, left=5, h=40, w=30, interp=R.BICUBIC, flip=0, **base),
                     R.row(top=0, left=0, h=64, w=48, interp=R.BILINEAR, flip=1, **base),
                     R.row(top=63, left=47, h=1, w=1, interp=R.BICUBIC, flip=1, **base)])
    assert lib.ga_resize_crop_check_table(rows.ctypes.data, 3, 32, 32, src_bytes) == 0
    rows[2]['src_off'] = 32                                                               # each row is still bounded on its own
    assert lib.ga_resize_crop_check_table(rows.ctypes.data, 3, 32, 32, src_bytes) == -1
    assert 'row 2' in _lib.last_error() and 'outside the source buffer' in _lib.last_error()


class _Opt:
    steps = 11


class _Step:
    opt, micro, random_erasing = _Opt(), 3, None


class _Model:
    def load_state_dict(self, sd):
        self.sd = sd


def test_train_state_records_the_order_the_position_counts_in():
    on = FolderLoader(_Set(1000), 8, None, aug_repeats=3, selected_round=128)
    off = FolderLoader(_Set(1000), 8, None)
    ts = C.capture_train_state(_Step(), on, epoch=2, batch=5, device_counters=False)
    assert ts['loader'] == {'epoch': 2, 'batch': 5} and ts['opt_steps'] == 11           # the position keeps its two keys ...
    assert (ts['aug_repeats'], ts['selected_round']) == (3, 128)                        # ... the order's settings stand beside it
    plain = C.capture_train_state(_Step(), off, 1, 0, device_counters=False)
    assert plain['loader'] == {'epoch': 1, 'batch': 0} and (plain['aug_repeats'], plain['selected_round']) == (0, 256)
    assert C.loader_order(None) == {'aug_repeats': 0, 'selected_round': 256}
    ck = {'epoch': 2, 'version': 2, 'state_dict': {}, 'train_state': dict(ts, recovery=1)}
    assert C.resume_checkpoint(ck, _Model(), loader=on) == (2, 5)
    for other in (off, FolderLoader(_Set(1000), 8, None, aug_repeats=2, selected_round=128),
                  FolderLoader(_Set(1000), 8, None, aug_repeats=3, selected_round=256)):
        with pytest.raises(ValueError, match='aug_repeats 3, selected_round 128'):
            C.resume_checkpoint(ck, _Model(), loader=other)
        assert C.resume_checkpoint(ck, _Model(), loader=other, resume_opt=False) == (3, 0)     # --no-resume-opt: weights and the next epoch
    # a file written before the two keys existed: 0 / 256
    old = {'epoch': 2, 'version': 2, 'state_dict': {},
           'train_state': {k: v for k, v in dict(ts, recovery=1).items() if k not in ('aug_repeats', 'selected_round')}}
    assert C.resume_checkpoint(old, _Model(), loader=off) == (2, 5)
    assert C.resume_checkpoint(old, _Model(), loader=FolderLoader(_Set(1000), 8, None, selected_round=0)) == (2, 5)
    with pytest.raises(ValueError, match='aug_repeats 0, selected_round 256'):
        C.resume_checkpoint(old, _Model(), loader=on)
