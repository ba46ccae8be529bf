"""The order of timm 0.9.2's RepeatAugSampler, restated step by step with torch ops and Python lists -- independent of
imagenet_models_amd.dataset.repeat_aug_indices, which the tests compare with it.  timm is not installed: parity with timm itself is
unpinned, as for every other timm restatement of this project."""
import math

import torch


def num_selected(n, world, selected_round):
    if selected_round:
        return int(math.floor(n // selected_round * selected_round / world))
    return int(math.ceil(n / world))


def repeat_aug_ref(n, seed, repeats, rank, world, selected_round):
    """-> this rank's list of sample indices of one epoch"""
    g = torch.Generator()
    g.manual_seed(seed)
    perm = torch.randperm(n, generator=g).tolist()                  # 1. the epoch's permutation
    rep = []
    for a in perm:                                                  # 2. every entry `repeats` times in a row
        rep += [a] * repeats
    total = int(math.ceil(n * repeats / world)) * world
    rep += rep[:total - len(rep)]                                   # 3. padded with its own head
    assert len(rep) == total
    mine = [rep[k] for k in range(rank, total, world)]              # 4. every world-th entry from rank
    return mine[:num_selected(n, world, selected_round)]            # 5. the first num_selected


def full_batches(indices, batch):
    """6. the epoch's full batches; the remainder is dropped"""
    return [indices[at:at + batch] for at in range(0, len(indices) // batch * batch, batch)]
