"""Host -> device staging of the input stage: the one pinned ring every table and every packed batch travels through, the workspace
growth rule and the batch check that its users share.

A Ring is DEPTH pinned host buffers in rotation, each guarded by the event of its last non_blocking copy: a slot is rewritten (or,
when it is too small, replaced) only after that copy has completed, which in a running loop it has long ago, so a step never
synchronises with the device.  A change of batch shape or of device needs nothing more: the slot is waited for, then grown."""
import numpy as np
import torch

DEPTH = 4          # copies in flight per ring: a slot is rewritten only after its copy of DEPTH calls ago has completed


class Ring:
    def __init__(self):
        self._host, self._copied, self._calls = [None] * DEPTH, [None] * DEPTH, 0

    def slot(self, nbytes):
        """-> (index, pinned uint8 buffer of at least nbytes) whose previous copy has completed.  The caller fills it -- through raw
        pointers from other threads if it likes --, copies it with non_blocking=True and calls sent(index)"""
        i = self._calls % DEPTH
        self._calls += 1
        if self._copied[i] is not None:
            self._copied[i].synchronize()          # complete long ago in a running loop: no stall
        if self._host[i] is None or self._host[i].numel() < nbytes:
            self._host[i] = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        return i, self._host[i]

    def sent(self, i):
        """the copy out of slot i has been enqueued on the current stream"""
        ev = self._copied[i] or torch.cuda.Event()
        ev.record()
        self._copied[i] = ev

    def upload(self, table, dev):
        """a host table (a numpy array of any dtype) -> the device tensor `dev` of the same number of bytes: one slot, one
        non_blocking copy, one event"""
        src = np.ascontiguousarray(table).reshape(-1).view(np.uint8)
        dst = dev.view(-1).view(torch.uint8)
        if dst.numel() != src.nbytes:
            raise ValueError(f'a table of {src.nbytes} bytes does not fill a device tensor of {dst.numel()}')
        i, host = self.slot(src.nbytes)
        host.numpy()[:src.nbytes] = src
        dst.copy_(host[:src.nbytes], non_blocking=True)
        self.sent(i)
        return dev


def buffer(buf, shape, dtype, device):
    """a device buffer an object owns and reuses: `buf` while it has this shape, dtype and device, otherwise a new one"""
    if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype or buf.device != device:
        buf = torch.empty(tuple(shape), dtype=dtype, device=device)
    return buf


def workspace(buf, nbytes, device):
    """device uint8 scratch of at least nbytes: `buf` while it is large enough and on `device`, otherwise a new one a quarter
    larger than asked for -- it grows with the largest request seen, not at every new maximum"""
    if buf is None or buf.numel() < nbytes or buf.device != device:
        buf = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=device)
    return buf


def check_batch(x, who, dtypes=(torch.uint8, torch.float32), channels=None, stats=None):
    """x is on the device, of one of `dtypes`, (B, C, H, W) [with C == channels] -> x contiguous; `who` names the caller.  stats:
    the (mean, std) of a pass that normalises a uint8 batch -- then both must be there"""
    if not x.is_cuda:
        raise RuntimeError(f'{who} runs on the HIP kernels only (no CPU fallback)')
    if x.dtype not in dtypes or x.dim() != 4 or (channels is not None and x.shape[1] != channels):
        names = ' or '.join(str(d).replace('torch.', '') for d in dtypes)
        raise TypeError(f"{who} expects a {names} (B, {channels or 'C'}, H, W) batch, got {x.dtype} {tuple(x.shape)}")
    if stats is not None and x.dtype == torch.uint8 and any(s is None for s in stats):
        raise ValueError(f'{who} on a uint8 batch normalises it in the same pass: pass mean / std (0..255 units)')
    return x.contiguous()
