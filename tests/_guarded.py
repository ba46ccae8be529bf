"""NaN-filled guarded device buffers for the kernel edge tests (tests/test_attn_edges_gpu.py,
tests/test_class_attn_mt_edges_gpu.py, tests/test_gemm_forms_edges_gpu.py): a kernel that leaves an in-range element unwritten, or writes a pad column or a
guard row, is caught by comparing bit patterns before and after."""
import torch


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded:
    """[rows][ld] device buffer of which columns [0, width) are in range, inside a NaN-filled allocation with `guard`
    elements (default: one row) in front and behind; `off` shifts the view by that many elements.  check() verifies
    that everything outside the range kept its bits and (written=True) that no in-range element is NaN."""

    def __init__(self, rows, width, ld, dt, data=None, off=0, guard=None):
        guard = ld if guard is None else guard
        self.rows, self.width, self.ld = rows, width, ld
        self.flat = torch.full((2 * guard + rows * ld + 8,), float('nan'), dtype=dt, device='cuda')
        self.start = guard + off
        self.view = self.flat[self.start:self.start + rows * ld].view(rows, ld)
        if data is not None:
            self.view[:, :width] = data.to(dt).cuda()
        self.before = _bits(self.flat).clone()

    def inner(self):
        return self.view[:, :self.width]

    def check(self, name, written=True):
        same = _bits(self.flat) == self.before
        inside = torch.zeros_like(same)
        inside[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width] = True
        assert bool(same[~inside].all()), f'{name}: {int((~same[~inside]).sum())} guard / pad elements were written'
        if written:
            nan = torch.isnan(self.inner())
            assert not bool(nan.any()), f'{name}: {int(nan.any(1).sum())} of {self.rows} rows hold elements that were never written'
        else:
            assert bool(same.all()), f'{name}: written although the call was refused'
