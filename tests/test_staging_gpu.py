"""GPU: the pinned staging ring of the input stage (imagenet_models_amd.staging.Ring) on its own: more uploads than it has slots,
with no host synchronisation in between, then the growth of a used slot.  Every gate is equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _table(rows, seed):
    return np.random.RandomState(seed).randint(0, 256, (rows, 64)).astype(np.uint8)


def test_ring_reuses_and_grows_its_slots():
    from imagenet_models_amd import staging
    ring = staging.Ring()
    uploads = staging.DEPTH + 3
    assert uploads == 7
    dev = torch.zeros(4, 64, dtype=torch.uint8, device='cuda')
    tables = [_table(4, k) for k in range(uploads)]          # 4 x 64 bytes each: at least two slots are written a second time
    clones = []
    for t in tables:
        assert ring.upload(t, dev) is dev
        clones.append(dev.clone())                              # on the device, behind the copy: no host synchronisation
    # a used slot grows (the eighth upload goes to slot 3, which has held 256 bytes), then a small table follows in the next one
    big, small = _table(64, 100), _table(4, 101)
    big_dev = torch.zeros(64, 64, dtype=torch.uint8, device='cuda')
    ring.upload(big, big_dev)
    big_clone = big_dev.clone()
    ring.upload(small, dev)
    clones.append(dev.clone())
    torch.cuda.synchronize()
    for k, (t, c) in enumerate(zip(tables + [small], clones)):
        assert np.array_equal(c.cpu().numpy(), t), f'upload {k}'
    assert np.array_equal(big_clone.cpu().numpy(), big)
    # the two-phase form hands out the next slot in rotation, large enough, and never a buffer whose copy may still be running
    i, host = ring.slot(48 * 64)
    assert i == (uploads + 2) % staging.DEPTH and host.is_pinned() and host.dtype == torch.uint8 and host.numel() >= 48 * 64
    ring.sent(i)
    with pytest.raises(ValueError, match='does not fill'):
        ring.upload(_table(8, 0), dev)
    torch.cuda.synchronize()
