"""An ImageNet-style folder as the loader of the device input stage: ImageFolder lists root/<class>/<file> as timm's folder parser
does (class directories sorted, files in natural order, labels by class index), FolderLoader reads the encoded bytes of one batch
at a time, hands them to a decoder (imagenet_models_amd.JpegDecoder) and yields (RaggedBatch, labels) -- what
TrainStep(crop=RandomResizedCrop(...)) and ResizeCenterCrop take.  No pixel is touched on the host.

Training: a permutation per epoch from seed + epoch (set_epoch), strided by rank, the ragged tail dropped -- the engines are planned
for one batch size.  Evaluation: file order, strided by rank, the last batch padded by repeating the last sample; the third element
of what it yields is the number of real entries.  One producer thread keeps `prefetch` batches ahead of the consumer.
evaluate_folder is the accuracy loop over such a loader that both scripts run."""
import os
import queue
import re
import threading

import numpy as np
import torch

from .loss import heads_topk

IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png')


def natural_key(s):
    """timm.utils.misc.natural_key: digit runs compare as numbers, the rest case-insensitively"""
    return [int(t) if t.isdigit() else t for t in re.split(r'(\d+)', s.lower())]


def split_dir(root, name):
    """timm's _search_split: root/name where that is a directory, else the root itself"""
    if not os.path.isdir(root):
        raise NotADirectoryError(f'{root!r} is not a directory')
    cand = os.path.join(root, name)
    return cand if name and os.path.isdir(cand) else root


class ImageFolder:
    """samples: (path, class index) of every image file under root/<class>/..., classes: the sorted directory names"""

    def __init__(self, root):
        if not os.path.isdir(root):
            raise FileNotFoundError(f'ImageFolder: {root!r} is not a directory')
        found = []
        for base, _, files in os.walk(root, topdown=False, followlinks=True):
            rel = os.path.relpath(base, root) if base != root else ''
            label = os.path.basename(rel)                    # timm's find_images_and_targets, leaf_name_only=True
            for f in files:
                if os.path.splitext(f)[1].lower() in IMG_EXTENSIONS and label:
                    found.append((os.path.join(base, f), label))
        if not found:
            raise RuntimeError(f'ImageFolder: no {" / ".join(IMG_EXTENSIONS)} file under a class directory of {root!r}')
        self.root = root
        self.classes = sorted({label for _, label in found}, key=natural_key)
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        found.sort(key=lambda s: natural_key(s[0]))
        self.samples = [(path, self.class_to_idx[label]) for path, label in found]

    def __len__(self):
        return len(self.samples)

    def read(self, index):
        """-> (the file's bytes, class index)"""
        path, target = self.samples[index]
        with open(path, 'rb') as f:
            return f.read(), target


class FolderLoader:
    """iterating yields (RaggedBatch, int64 labels on the device) while training and (RaggedBatch, labels, real) for evaluation,
    `real` of the `batch` entries being samples of the dataset (the rest repeat the last one)"""

    def __init__(self, dataset, batch, decoder, train=True, seed=0, rank=0, world=1, prefetch=2, device='cuda'):
        if batch < 1 or world < 1 or not 0 <= rank < world or prefetch < 1:
            raise ValueError(f'FolderLoader: batch {batch}, rank {rank} of {world}, prefetch {prefetch}')
        self.dataset, self.batch, self.decoder, self.train = dataset, int(batch), decoder, bool(train)
        self.seed, self.rank, self.world, self.prefetch, self.device = int(seed), int(rank), int(world), int(prefetch), device
        self.epoch = self.start_batch = 0
        if self.train and len(self) == 0:
            raise ValueError(f'FolderLoader: {len(dataset)} samples over {world} rank(s) give no full batch of {batch}')

    def set_epoch(self, epoch, start_batch=0):
        """start_batch: the next iteration yields batches(epoch)[start_batch:] -- a run resumed inside an epoch; the skipped
        batches' files are neither read nor decoded"""
        if not 0 <= int(start_batch) <= len(self):
            raise ValueError(f'FolderLoader: start_batch {start_batch} of an epoch of {len(self)} batches')
        self.epoch, self.start_batch = int(epoch), int(start_batch)

    def plan(self):
        """what the next iteration reads, decodes and yields: batches() of the epoch from the start position on"""
        return self.batches()[self.start_batch:]

    def indices(self, epoch=None):
        """this rank's sample indices of an epoch, in order.  Training: the epoch's permutation cut to a multiple of world * batch
        (every rank runs the same number of full batches), then every world-th entry from rank"""
        n = len(self.dataset)
        if self.train:
            g = torch.Generator().manual_seed(self.seed + (self.epoch if epoch is None else int(epoch)))
            order = torch.randperm(n, generator=g).numpy()
            keep = n // (self.world * self.batch) * (self.world * self.batch)
            return order[:keep][self.rank::self.world]
        return np.arange(n, dtype=np.int64)[self.rank::self.world]

    def __len__(self):
        n = len(self.dataset)
        if self.train:
            return n // (self.world * self.batch)
        return -(-len(range(self.rank, n, self.world)) // self.batch)

    def batches(self, epoch=None):
        """-> list of (index array of `batch` entries, real count)"""
        idx = self.indices(epoch)
        out = []
        for at in range(0, len(idx), self.batch):
            part = idx[at:at + self.batch]
            real = len(part)
            if real < self.batch:
                part = np.concatenate([part, np.full(self.batch - real, part[-1], dtype=part.dtype)])
            out.append((part, real))
        return out

    def _produce(self, plan, q, stop, stream):
        try:
            torch.cuda.set_device(stream.device)             # the current device is per thread
            for part, real in plan:
                if stop.is_set():
                    return
                files, labels = zip(*(self.dataset.read(int(i)) for i in part))
                with torch.cuda.stream(stream):
                    ragged = self.decoder.decode(list(files), device=stream.device)
                    y = torch.tensor(labels, dtype=torch.int64).pin_memory().to(stream.device, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(stream)
                q.put((ragged, y, real, done))
            q.put(None)
        except BaseException as e:          # handed to the consumer: a corrupt file must stop the epoch, not hang it
            q.put(e)

    def __iter__(self):
        plan = self.plan()
        q, stop = queue.Queue(maxsize=self.prefetch), threading.Event()
        stream = torch.cuda.Stream(device=torch.device(self.device))       # the producer's copies and launches: the step's stream waits per batch
        t = threading.Thread(target=self._produce, args=(plan, q, stop, stream), name='folder-loader', daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                ragged, y, real, done = item
                torch.cuda.current_stream().wait_event(done)
                ragged.data.record_stream(torch.cuda.current_stream())
                y.record_stream(torch.cuda.current_stream())
                yield (ragged, y) if self.train else (ragged, y, real)
        finally:
            stop.set()
            while t.is_alive():              # unblock a producer waiting on a full queue
                try:
                    q.get_nowait()
                except queue.Empty:
                    t.join(0.01)


def evaluate_folder(model, loader, crop):
    """an eval-mode model over an evaluation FolderLoader, crop: a ResizeCenterCrop -> int64 device tensor (top-1 hits, top-5 hits,
    samples) over exactly the real samples (the last batch is padded to the engine's size)"""
    counts = torch.zeros(3, dtype=torch.int64, device=loader.device)
    with torch.no_grad():
        for ragged, y, real in loader:
            _, idx = heads_topk(model(crop(ragged)), 5)
            hit = idx[:real].to(torch.int64) == y[:real, None]
            counts += torch.stack([hit[:, 0].sum(), hit.any(dim=1).sum(), torch.tensor(real, device=loader.device)])
    return counts
