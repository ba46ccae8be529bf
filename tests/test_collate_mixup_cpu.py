"""CPU: the host side of the collate-time mixup order (imagenet_models_amd.FastCollateMixup.sample, the C ABI of ga_input_collate /
ga_mixup_target_elem, train.py's flags) against the independent restatement of tests/_collate_mixup_ref.py, and the restatement's
own blend against plain numpy.  timm is not installed: parity with timm itself is unpinned."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _collate_mixup_ref as CM
from conftest import ROOT

CONFIGS = {
    'mixup': dict(mixup_alpha=0.8, cutmix_alpha=0.0),
    'cutmix': dict(mixup_alpha=0.0, cutmix_alpha=1.0),
    'both': dict(mixup_alpha=0.8, cutmix_alpha=1.0),
    'minmax': dict(mixup_alpha=0.0, cutmix_alpha=0.0, cutmix_minmax=(0.2, 0.6)),
    'prob': dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5, switch_prob=0.3),
}
SIZES = [(224, 224), (160, 160), (6, 10)]


@pytest.mark.parametrize('mode', ['batch', 'elem', 'pair'])
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_sample_equals_the_restatement_draw_for_draw(cfg, mode):
    import imagenet_models_amd as A
    kw = CONFIGS[cfg]
    kinds = set()
    for H, W in SIZES:
        for seed in range(6):
            mine_rng, ref_rng = np.random.RandomState(seed), np.random.RandomState(seed)
            fm = A.FastCollateMixup(mode=mode, rng=mine_rng, **kw)
            for call in range(3):                            # consecutive batches continue the same stream
                B = (8, 2, 16)[call]
                got = fm.sample(B, H, W)
                want, lam = CM.sample_table(ref_rng, B, H, W, mode=mode, **kw)
                assert got.dtype == np.int32 and got.shape == (B, 8)
                assert np.array_equal(got, want), (cfg, mode, H, W, seed, call)          # l, m compared as their bit patterns
                assert mine_rng.rand() == ref_rng.rand()     # the same number of draws
                l, m = CM.table_lm(got)
                assert (got[:, 7] == 0).all() and ((l >= 0) & (l <= 1)).all()
                yl, yh, xl, xh = got[:, 1], got[:, 2], got[:, 3], got[:, 4]
                assert ((0 <= yl) & (yl <= yh) & (yh <= H) & (0 <= xl) & (xl <= xh) & (xh <= W)).all()
                if mode == 'batch':
                    assert (got == got[0]).all() and m[0] == np.float32(1.0 - lam)
                else:
                    assert np.array_equal(m, np.float32(1) - l) and np.array_equal(l, lam)
                if mode == 'pair':                           # mirror-symmetric: i and B-1-i share lam, kind and box
                    assert np.array_equal(got, got[::-1])
                cut = got[:, 0] == CM.CUTMIX
                area = 1.0 - (yh - yl) * (xh - xl) / float(H * W)
                assert np.array_equal(l[cut], area[cut].astype(np.float32))               # corrected lam of a cut box
                assert (l[got[:, 0] == CM.NONE] == 1).all()
                kinds.update(int(k) for k in got[:, 0])
    expect = {'mixup': {CM.MIXUP}, 'cutmix': {CM.CUTMIX}, 'both': {CM.MIXUP, CM.CUTMIX}, 'minmax': {CM.CUTMIX},
              'prob': {CM.NONE, CM.MIXUP, CM.CUTMIX}}[cfg]
    assert kinds >= expect and (cfg == 'prob' or kinds == expect), kinds


@pytest.mark.parametrize('mode', ['batch', 'elem', 'pair'])
def test_disabled_mixup_gives_all_none_rows(mode):
    import imagenet_models_amd as A
    mine_rng, ref_rng = np.random.RandomState(3), np.random.RandomState(3)
    fm = A.FastCollateMixup(mode=mode, rng=mine_rng, **CONFIGS['both'])
    fm.mixup_enabled = False
    got = fm.sample(8, 224, 224)
    want, _ = CM.sample_table(ref_rng, 8, 224, 224, mode=mode, enabled=False, **CONFIGS['both'])
    assert np.array_equal(got, want) and (got[:, :5] == 0).all()
    l, m = CM.table_lm(got)
    assert (l == 1).all() and (m == 0).all()
    assert mine_rng.rand() == ref_rng.rand()


def test_half_and_unknown_modes_raise():
    import imagenet_models_amd as A
    with pytest.raises(ValueError, match='half of the batch'):
        A.FastCollateMixup(mode='half')
    with pytest.raises(ValueError, match="'batch', 'elem' or 'pair'"):
        A.FastCollateMixup(mode='rows')
    with pytest.raises(AssertionError):
        A.FastCollateMixup(mode='elem').sample(7, 8, 8)      # an odd batch has no partner for its middle sample


def test_restatement_blend_is_plain_numpy_rint():
    a, b = CM.all_byte_pairs()
    lam = 0.5
    plain = np.rint(a.astype(np.float32) * lam + b.astype(np.float32) * (1 - lam))
    got = CM.blend_u8(a, b, np.float32(0.5), np.float32(0.5))
    assert got.dtype == np.uint8 and np.array_equal(got, plain)
    assert got[1, 2] == 2 and got[1, 4] == 2 and got[3, 4] == 4 and got[255, 255] == 255 and got[0, 1] == 0       # ties to even
    # a float32 image round trip and a general lam
    for lam in (0.3, 0.6899998188018799):
        l = np.float32(lam)
        m = np.float32(1) - l
        plain = np.rint(a.astype(np.float32) * l + b.astype(np.float32) * m)
        assert np.array_equal(CM.blend_u8(a, b, l, m), plain)
    x = np.random.RandomState(0).randint(0, 256, (4, 3, 6, 10)).astype(np.uint8)
    tab = np.zeros((4, 8), dtype=np.int32)
    tab[:, 0] = (CM.MIXUP, CM.CUTMIX, CM.NONE, CM.CUTMIX)
    tab[1, 1:5] = (1, 4, 3, 9)
    tab[3, 1:5] = (2, 2, 0, 10)                              # empty
    tab[:, 5] = np.full(4, 0.25, dtype=np.float32).view(np.int32)
    tab[:, 6] = np.full(4, 0.75, dtype=np.float32).view(np.int32)
    out = CM.mix_u8(x, tab)
    assert np.array_equal(out[0], np.rint(x[0].astype(np.float32) * np.float32(0.25) + x[3].astype(np.float32) * np.float32(0.75)).astype(np.uint8))
    assert np.array_equal(out[1, :, 1:4, 3:9], x[2, :, 1:4, 3:9]) and (out[1] != x[1]).sum() <= 3 * 3 * 6
    assert np.array_equal(out[1, :, 0], x[1, :, 0]) and np.array_equal(out[2], x[2]) and np.array_equal(out[3], x[3])


def test_a_contracted_blend_rounds_differently():
    """the lam the GPU test uses: found among seeded Beta draws, at least one byte pair where fma(a, l, fl(b*m)) rounds to another
    integer than fl(fl(a*l) + fl(b*m)); the known case l = 0.6899998188018799, (113, 163): 128 separately, 129 fused"""
    l = np.float32(0.6899998188018799)
    m = np.float32(1) - l
    a, b = np.array([113], dtype=np.uint8), np.array([163], dtype=np.uint8)
    assert CM.blend_u8(a, b, l, m)[0] == 128 and CM.blend_u8_contracted(a, b, l, m)[0] == 129
    assert CM.contraction_count(l) >= 1
    assert CM.contraction_count(0.5) == 0                    # both products exact: nothing to contract
    lam, count = CM.contraction_sensitive_lam()
    print(f'contraction-sensitive lam {lam!r}: {count} of 65536 byte pairs differ')
    assert lam is not None and count >= 1 and 0 < lam < 1 and np.float32(lam) == lam


def test_dense_target_restatement():
    import torch
    t = torch.tensor([3, 1, 0, 2])
    d = CM.dense_target(t, 4, 0.25, 0.0)
    assert torch.equal(d[0], torch.tensor([0.0, 0.0, 0.75, 0.25])) and torch.equal(d[1], torch.tensor([0.75, 0.25, 0.0, 0.0]))
    lam = np.array([1.0, 0.0, 0.5, 0.25], dtype=np.float32)
    d = CM.dense_target(t, 4, lam, 0.0)
    assert torch.equal(d, torch.tensor([[0, 0, 0, 1.0], [1.0, 0, 0, 0], [0.5, 0.5, 0, 0], [0, 0, 0.25, 0.75]]))
    d = CM.dense_target(t, 4, lam, 0.1)
    assert torch.allclose(d.sum(1), torch.ones(4), atol=1e-6)


def test_collate_entry_points_are_declared_bound_and_exported():
    from imagenet_models_amd import _lib, ops
    import imagenet_models_amd as A
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    lib = _lib.load()
    for name in ('ga_input_collate', 'ga_mixup_target_elem'):
        assert f'int {name}(' in hdr and name in _lib.exported_symbols() and hasattr(lib, name)
    assert 'kind, yl, yh, xl, xh, bits(l), bits(m), 0' in hdr                # the mix row is documented beside the entry point
    assert hasattr(ops.Plan, 'input_collate') and hasattr(ops.Plan, 'mixup_target_elem')
    assert A.FastCollateMixup.__module__ == 'imagenet_models_amd.mixup'
    # bad arguments are refused on the host, before any launch
    assert lib.ga_input_collate(None, 1, None, 2, 3, 8, 8, None, None, None, None, 0, 0, 0, 0, None) != 0
    assert 'ga_input_collate' in _lib.last_error()
    assert lib.ga_mixup_target_elem(None, None, 2, 10, None, 0.1, None) != 0
    assert 'ga_mixup_target_elem' in _lib.last_error()


def test_train_cli_lists_the_collate_flag_and_refuses_half():
    train = os.path.join(ROOT, 'train.py')
    r = subprocess.run([sys.executable, train, '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    text = ' '.join(r.stdout.split())
    assert '--collate-mixup' in text and 'prefetcher order every reference recipe runs' in text
    assert '"batch", "pair" or "elem"' in text
    for extra, why in ((['--mixup-mode', 'half'], 'half of every batch'), (['--mixup-mode', 'half', '--collate-mixup'], 'half of every batch'),
                       (['--mixup-mode', 'rows', '--collate-mixup'], "'batch', 'pair' or 'elem'")):
        r = subprocess.run([sys.executable, train, '--synthetic'] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and why in r.stderr, (extra, r.stderr[-500:])
