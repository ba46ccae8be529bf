"""JPEG files into the device input stage: the decoder at the seam resize_crop.pack_images() left open.  A baseline JPEG is split where
the work changes kind: the entropy stage -- markers and Huffman codes, bit-serial, branchy -- runs on the host, one file per call of
ga_jpeg_entropy_decode on a small thread pool (ctypes releases the GIL), straight into slices of ONE slot of the pinned staging.Ring; the pixel
reconstruction -- dequantise, IDCT, chroma upsampling, YCbCr -> RGB, regular and wide -- runs on the device in one
ga_jpeg_reconstruct launch over a 64-byte row per image, into the RaggedBatch byte buffer RandomResizedCrop / ResizeCenterCrop read.
The result equals PIL's Image.open(f).convert('RGB') byte for byte (tests/golden/jpeg_pil.npz).

What the device path does not rebuild (include/gaext.h: progressive, arithmetic, CMYK, other samplings, PNG ...) the probe reports as
UNSUPPORTED: with fallback='pil' those files are decoded by PIL on the host and their pixels travel in the same staging buffer into
their slot of the same RaggedBatch; without PIL, or with fallback=None, they raise.  A CORRUPT file always raises."""
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, ops, staging
from .resize_crop import RaggedBatch, pack_offsets

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
MAX_THREADS = 16
INFO_LEN = 24

ROW = np.dtype([('coef_off', '<i8'), ('dst_off', '<i8'), ('work_off', '<i8'), ('qt_off', '<i4'), ('width', '<i4'), ('height', '<i4'),
                ('ncomp', '<i4'), ('hs', '<i4'), ('vs', '<i4'), ('mcus_w', '<i4'), ('mcus_h', '<i4'), ('pad', '<i4', (2,))])
assert ROW.itemsize == 64


def _align16(v):
    return (int(v) + 15) & ~15


def _pil_image():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def probe(data):
    """-> (status, info int64 (24,)) of one file's bytes (include/gaext.h: ga_jpeg_probe)"""
    info = np.zeros(INFO_LEN, dtype=np.int64)
    st = _lib.load().ga_jpeg_probe(data, len(data), info.ctypes.data)
    if st < 0:
        _lib.check(st, 'ga_jpeg_probe')
    return int(st), info


class JpegDecoder:
    """decode(list of bytes) -> RaggedBatch.  threads: the entropy stage's pool (capped at 16: a loader shares the host with the
    step's own launch thread); fallback: 'pil' or None.  `fallbacks` counts the files PIL decoded, `decoded` all of them"""

    def __init__(self, threads=8, fallback='pil'):
        if fallback not in ('pil', None):
            raise ValueError(f"JpegDecoder: fallback {fallback!r}: 'pil' or None")
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.fallback = fallback
        self.fallbacks = self.decoded = 0
        self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix='jpeg')
        self._ring, self._work = staging.Ring(), None
        self.last = None                     # the table of the last call, for logging / tests

    def _entropy(self, job):
        data, coef_ptr, ncoef, qt_ptr = job
        return _lib.load().ga_jpeg_entropy_decode(data, len(data), coef_ptr, ncoef, qt_ptr)

    def _fallback_pixels(self, k, data, why):
        Image = _pil_image() if self.fallback == 'pil' else None
        if Image is None:
            raise ValueError(f'JpegDecoder: sample {k} is {why} and there is no fallback decoder '
                             f"({'PIL is not importable' if self.fallback == 'pil' else 'fallback=None'})")
        try:
            with Image.open(io.BytesIO(data)) as im:
                a = np.asarray(im.convert('RGB'))
        except Exception as e:
            raise ValueError(f'JpegDecoder: sample {k} is {why} and PIL refuses it too: {e}') from None
        if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1 or max(a.shape[:2]) >= 32768:
            raise ValueError(f'JpegDecoder: sample {k}: PIL decoded it to shape {a.shape}')
        return np.ascontiguousarray(a)

    def decode(self, files, device='cuda'):
        """files: a list of bytes objects, one encoded image each -> RaggedBatch on `device`"""
        files = list(files)
        if not files:
            raise ValueError('JpegDecoder.decode: an empty list')
        lib = _lib.load()
        n = len(files)
        infos, pixels = [None] * n, {}
        for k, data in enumerate(files):
            if not isinstance(data, (bytes, bytearray, memoryview)):
                raise TypeError(f'JpegDecoder.decode: sample {k} is {type(data).__name__}, expected the bytes of a file')
            if not isinstance(data, bytes):
                files[k] = data = bytes(data)
            st, info = probe(data)
            if st == CORRUPT:
                raise ValueError(f'JpegDecoder: sample {k} is a corrupt JPEG file (its header ends early or contradicts itself)')
            if st == UNSUPPORTED:
                pixels[k] = self._fallback_pixels(k, data, 'not a baseline JPEG the device path rebuilds (progressive, arithmetic, '
                                                  'CMYK, another sampling, or no JPEG at all)')
            else:
                infos[k] = info
        heights = [pixels[k].shape[0] if k in pixels else int(infos[k][1]) for k in range(n)]
        widths = [pixels[k].shape[1] if k in pixels else int(infos[k][0]) for k in range(n)]
        offsets, total = pack_offsets(heights, widths)
        dev_n = [k for k in range(n) if k not in pixels]
        # one staging buffer: [table rows][3 x 64 uint16 per image][coefficients][the fallback images' pixels]
        tab = np.zeros(len(dev_n), dtype=ROW)
        qt_at = _align16(tab.nbytes)
        coef_at = _align16(qt_at + 384 * len(dev_n))
        ncoef = work = 0
        for j, k in enumerate(dev_n):
            info, r = infos[k], tab[j]
            r['coef_off'], r['dst_off'], r['work_off'], r['qt_off'] = ncoef, offsets[k], work, 192 * j
            r['width'], r['height'], r['ncomp'], r['hs'], r['vs'], r['mcus_w'], r['mcus_h'] = (int(info[i]) for i in (0, 1, 2, 3, 4, 7, 8))
            ncoef += int(info[5])
            work += int(info[5])
        pix_at = _align16(coef_at + 2 * ncoef)
        staged = pix_at
        pix_off = {}
        for k, a in pixels.items():
            pix_off[k] = staged
            staged = _align16(staged + a.size)
        out = torch.empty(total, dtype=torch.uint8, device=device)
        if dev_n:
            _lib.check(lib.ga_jpeg_check_table(tab.ctypes.data, len(tab), ncoef, 192 * len(tab), work, out.numel()), 'ga_jpeg_check_table')
        i, host = self._ring.slot(staged)
        h = host.numpy()
        base = host.data_ptr()
        h[:tab.nbytes] = tab.view(np.uint8).reshape(-1)
        jobs = [(files[k], base + coef_at + 2 * int(tab[j]['coef_off']), int(infos[k][5]), base + qt_at + 384 * j)
                for j, k in enumerate(dev_n)]
        results = list(self._pool.map(self._entropy, jobs))
        for k, st in zip(dev_n, results):
            if st != OK:
                raise ValueError(f'JpegDecoder: sample {k} is a corrupt JPEG file (its scan ends early, holds a code no symbol has, a '
                                 f'run past coefficient 63 or a wrong restart marker; status {st})')
        for k, a in pixels.items():
            h[pix_off[k]:pix_off[k] + a.size] = a.reshape(-1)
        dev = torch.empty(staged, dtype=torch.uint8, device=out.device)
        dev.copy_(host[:staged], non_blocking=True)
        self._ring.sent(i)
        if dev_n:
            self._work = staging.workspace(self._work, work, out.device)      # grows with the largest batch seen
            ops.Plan(eager=True).jpeg_reconstruct(dev[:tab.nbytes], len(tab), dev[coef_at:coef_at + 2 * ncoef].view(torch.int16),
                                                  dev[qt_at:qt_at + 384 * len(tab)].view(torch.int16), self._work, out)
        for k, a in pixels.items():
            out[int(offsets[k]):int(offsets[k]) + a.size].copy_(dev[pix_off[k]:pix_off[k] + a.size])
        self.fallbacks += len(pixels)
        self.decoded += n
        self.last = tab
        return RaggedBatch(out, offsets, heights, widths)
