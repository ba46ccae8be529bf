"""An ImageNet-style folder as the loader of the device input stage: ImageFolder lists root/<class>/<file> as timm's folder parser
does (class directories sorted, files in natural order, labels by class index), FolderLoader reads the encoded bytes of one batch
at a time, hands them to a decoder (imagenet_models_amd.JpegDecoder) and yields (RaggedBatch, labels) -- what
TrainStep(crop=RandomResizedCrop(...)) and ResizeCenterCrop take.  No pixel is touched on the host.

Training: a permutation per epoch from seed + epoch (set_epoch), strided by rank, the ragged tail dropped -- the engines are planned
for one batch size.  Evaluation: file order, strided by rank, the last batch padded by repeating the last sample; the third element
of what it yields is the number of real entries.  One producer thread keeps `prefetch` batches ahead of the consumer.
aug_repeats > 0: the training order is timm's RepeatAugSampler (repeat_aug_indices) and each distinct file of a batch is read and
decoded once -- the copies are entries of the RaggedBatch that share one region of its buffer.
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


def num_selected(n, world, selected_round):
    """timm's num_selected_samples: what a rank feeds per epoch under repeated augmentation"""
    return n // selected_round * selected_round // world if selected_round else -(-n // world)


def repeat_aug_indices(n, seed, repeats, rank=0, world=1, selected_round=256):
    """timm 0.9.2's RepeatAugSampler for one epoch -> this rank's int64 index array.  The permutation of `n` under torch's generator
    seeded with `seed` (timm seeds with the epoch alone), every entry written `repeats` times in a row, padded with its own head
    to a multiple of `world`, every world-th entry from `rank`, cut to num_selected: floor(n // selected_round * selected_round /
    world), or ceil(n / world) with selected_round 0.  A rank reads about n / repeats distinct files and feeds n / world samples."""
    if int(repeats) != repeats or repeats < 1:
        raise ValueError(f'repeat_aug_indices: repeats {repeats!r}: a whole number of at least 1 (fractional repeats are not built)')
    if n < 1 or world < 1 or not 0 <= rank < world or selected_round < 0:
        raise ValueError(f'repeat_aug_indices: n {n}, rank {rank} of {world}, selected_round {selected_round}')
    g = torch.Generator().manual_seed(int(seed))
    order = torch.repeat_interleave(torch.randperm(n, generator=g), int(repeats))
    total = -(-n * int(repeats) // world) * world
    order = torch.cat([order, order[:total - len(order)]])
    return order[rank:total:world][:num_selected(n, world, selected_round)].numpy()


def first_occurrences(part):
    """an index list -> (its distinct entries in the order they first occur, inverse) with distinct[inverse] == part"""
    part = np.asarray(part)
    uniq, first, inverse = np.unique(part, return_index=True, return_inverse=True)
    by_first = np.argsort(first, kind='stable')
    place = np.empty(len(uniq), dtype=np.int64)
    place[by_first] = np.arange(len(uniq))
    return uniq[by_first], place[inverse.reshape(-1)]


class FolderLoader:
    """iterating yields (RaggedBatch, int64 labels on the device) while training and (RaggedBatch, labels, real) for evaluation,
    `real` of the `batch` entries being samples of the dataset (the rest repeat the last one).
    aug_repeats N > 0 (training only): the order of repeat_aug_indices(n, seed + epoch, N, rank, world, selected_round), cut to full
    batches; a batch's distinct files are decoded once and its RaggedBatch entries gathered from them (RaggedBatch.take).
    decode_once=False decodes every entry on its own instead -- the same bytes at the cost of a loader without the sharing, the
    other arm of tools/aug_repeats_ab.py"""

    def __init__(self, dataset, batch, decoder, train=True, seed=0, rank=0, world=1, prefetch=2, device='cuda', aug_repeats=0,
                 selected_round=256, decode_once=True):
        if batch < 1 or world < 1 or not 0 <= rank < world or prefetch < 1:
            raise ValueError(f'FolderLoader: batch {batch}, rank {rank} of {world}, prefetch {prefetch}')
        if isinstance(aug_repeats, bool) or int(aug_repeats) != aug_repeats or aug_repeats < 0:
            raise ValueError(f'FolderLoader: aug_repeats {aug_repeats!r}: a whole number of at least 0 (timm\'s fractional repeats are '
                             'not built)')
        if isinstance(selected_round, bool) or int(selected_round) != selected_round or selected_round < 0:
            raise ValueError(f'FolderLoader: selected_round {selected_round!r}: a whole number of at least 0')
        if aug_repeats and not train:
            raise ValueError(f'FolderLoader: aug_repeats {aug_repeats} on an evaluation loader: repeated augmentation is a training order')
        self.aug_repeats, self.selected_round, self.decode_once = int(aug_repeats), int(selected_round), bool(decode_once)
        self.dataset, self.batch, self.decoder, self.train = dataset, int(batch), decoder, bool(train)
        self.seed, self.rank, self.world, self.prefetch, self.device = int(seed), int(rank), int(world), int(prefetch), device
        self.epoch = self.start_batch = 0
        if self.aug_repeats and self._selected() == 0:
            raise ValueError(f'FolderLoader: {len(dataset)} samples under selected_round {self.selected_round} over {world} rank(s) '
                             f'give an epoch of no sample with aug_repeats {self.aug_repeats} (timm rounds the epoch down to a multiple '
                             'of selected_round; 0 turns the rounding off)')
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
        (every rank runs the same number of full batches), then every world-th entry from rank.  With aug_repeats: the full batches
        of repeat_aug_indices"""
        n = len(self.dataset)
        if self.aug_repeats:
            order = repeat_aug_indices(n, self.seed + (self.epoch if epoch is None else int(epoch)), self.aug_repeats, self.rank,
                                       self.world, self.selected_round)
            return order[:len(order) // self.batch * self.batch]
        if self.train:
            g = torch.Generator().manual_seed(self.seed + (self.epoch if epoch is None else int(epoch)))
            order = torch.randperm(n, generator=g).numpy()
            keep = n // (self.world * self.batch) * (self.world * self.batch)
            return order[:keep][self.rank::self.world]
        return np.arange(n, dtype=np.int64)[self.rank::self.world]

    def _selected(self):
        """what this rank feeds per epoch under aug_repeats, before the ragged tail is dropped"""
        return num_selected(len(self.dataset), self.world, self.selected_round)

    def __len__(self):
        n = len(self.dataset)
        if self.aug_repeats:
            return self._selected() // self.batch
        if self.train:
            return n // (self.world * self.batch)
        return -(-len(range(self.rank, n, self.world)) // self.batch)

    def distinct_files(self, epoch=None):
        """how many different files this rank reads in an epoch"""
        return len(np.unique(self.indices(epoch)))

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
                # under aug_repeats the copies of a file differ in their table rows only: read and decode it once
                distinct, inverse = first_occurrences(part) if self.aug_repeats and self.decode_once else (part, None)
                files, labels = zip(*(self.dataset.read(int(i)) for i in distinct))
                with torch.cuda.stream(stream):
                    ragged = self.decoder.decode(list(files), device=stream.device)
                    if inverse is not None:
                        ragged, labels = ragged.take(inverse), [labels[j] for j in inverse]
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
