"""Checkpoint I/O in timm's CheckpointSaver layout ({'epoch','arch','state_dict','optimizer','version':2,'metric'},
GA/train.py:649-651,693) so reference `.pth.tar` files load by key.  Loading uses weights_only=True.

Beside those keys a file carries `train_state`: everything else that decides step k+1 (DESIGN.md "Resuming exactly"), as tensors,
ints, floats, strings and lists only.  capture_train_state / restore_train_state collect it and put it back; CheckpointSaver writes
the files (last / checkpoint-N / model_best / recovery-N-B) atomically, from a device snapshot, behind the training thread."""
import argparse
import contextlib
import logging
import os
import random
import shutil
import threading

import numpy as np
import torch
import torch.distributed as dist

_logger = logging.getLogger('train')


class ModelEma:
    """timm ModelEmaV2 (GA/train.py:497-502, 774-775): ema = decay * ema + (1 - decay) * model over every state_dict
    value, on the device.  The parameters live in ONE flat fp32 buffer, so their update is a single kernel launch
    (ga_lerp_f32); BatchNorm running statistics are few small tensors, num_batches_tracked is copied."""

    def __init__(self, model, decay=0.9998):
        from .ops import Plan
        self.model, self.decay = model, decay
        st = model.flat_state()
        self.gen = st['gen']
        self.flat = st['params'].clone()
        self.slices = st['slices']
        self.buffers = {n: b.detach().clone() for n, b in model.named_buffers()}
        self.plan = Plan(name='ema')
        self.plan.lerp_f32(self.flat, st['params'], 1.0 - decay, st['total'])
        for n, b in model.named_buffers():
            if b.dtype == torch.float32 and b.numel() > 0:
                self.plan.lerp_f32(self.buffers[n], b, 1.0 - decay, b.numel())

    def update(self, model=None):
        self.model.check_flat_generation(self.gen, 'ModelEma')
        self.plan.run()
        for n, b in self.model.named_buffers():
            if b.dtype != torch.float32:
                self.buffers[n].copy_(b)

    def state_dict(self):
        ref = self.model.state_dict()
        out = {}
        for k, v in ref.items():
            if k in self.slices:
                off, n = self.slices[k]
                out[k] = self.flat[off:off + n].view(v.shape)
            else:
                out[k] = self.buffers[k]
        return out

    def load_state_dict(self, sd):
        """write a `state_dict_ema` into the flat buffer and the buffers (every key of state_dict() must be there, shapes equal)"""
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        if missing:
            raise RuntimeError(f'ModelEma.load_state_dict: missing {missing[:5]}')
        with torch.no_grad():
            for k, v in own.items():
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise RuntimeError(f'ModelEma.load_state_dict: {k} has shape {tuple(sd[k].shape)}, the model {tuple(v.shape)}')
                v.copy_(sd[k].to(v.device))

    def _exchange(self):
        self.model.check_flat_generation(self.gen, 'ModelEma')
        self.model.flush_counters()
        st = self.model.flat_state()
        pairs = [(st['params'], self.flat)] + [(b, self.buffers[n]) for n, b in self.model.named_buffers()]
        with torch.no_grad():
            for a, b in pairs:
                if a.numel():
                    keep = a.clone()
                    a.copy_(b)
                    b.copy_(keep)
        for e in self.model._engines.values():
            e.weights_dirty = True

    @contextlib.contextmanager
    def swapped(self):
        """inside the block the model holds the EMA's parameters and buffers (and the EMA the model's): evaluate, then leave;
        both are bitwise what they were afterwards.  The engines' effective weights are marked stale on entry and on exit."""
        self._exchange()
        try:
            yield self.model
        finally:
            self._exchange()


def save_checkpoint(model, optimizer, epoch, path, metric=None, arch='', model_ema=None, train_state=None):
    ck = {'epoch': epoch, 'arch': arch, 'state_dict': {k: v.detach().cpu() for k, v in model.state_dict().items()},
          'optimizer': {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in optimizer.state_dict().items()}
          if optimizer is not None else None, 'version': 2, 'metric': metric}
    if model_ema is not None:      # timm CheckpointSaver key
        ck['state_dict_ema'] = {k: v.detach().cpu() for k, v in model_ema.state_dict().items()}
    if train_state is not None:
        ck['train_state'] = train_state
    torch.save(ck, path)


def read_checkpoint(path):
    """the file as a dict, nothing from it executed: timm-layout checkpoints (`CheckpointSaver` passes args=args, GA/train.py:649-651)
    carry an argparse.Namespace under 'args', allow-listed as plain data; everything else stays under weights_only=True"""
    with torch.serialization.safe_globals([argparse.Namespace]):
        return torch.load(path, map_location='cpu', weights_only=True)


def _model_state(ck, use_ema=False):
    if use_ema and isinstance(ck, dict) and 'state_dict_ema' in ck:
        ck = {'state_dict': ck['state_dict_ema']}
    sd = ck.get('state_dict', ck.get('model', ck)) if isinstance(ck, dict) else ck
    return {k[7:] if k.startswith('module.') else k: v for k, v in sd.items()}


def load_checkpoint(model, path, strict=True, use_ema=False):
    return model.load_state_dict(_model_state(read_checkpoint(path), use_ema), strict=strict)


# ----------------------------------------------------------------------------------------------------------------------------
# the training state as plain data
# ----------------------------------------------------------------------------------------------------------------------------
def pack_python_random(rng=random):
    """random.getstate() = (version, 624 words + position, the cached second gauss value or None) as {int, int64 tensor, ...}"""
    version, words, gauss = rng.getstate()
    return {'version': int(version), 'words': torch.tensor(words, dtype=torch.int64), 'has_gauss': int(gauss is not None),
            'gauss': float(gauss) if gauss is not None else 0.0}


def unpack_python_random(d, rng=random):
    rng.setstate((d['version'], tuple(int(w) for w in d['words'].tolist()), d['gauss'] if d['has_gauss'] else None))


def pack_numpy_random(rng=np.random):
    """np.random.get_state() (legacy MT19937 layout; the module or a RandomState)"""
    kind, keys, pos, has_gauss, cached = rng.get_state()
    if kind != 'MT19937':
        raise ValueError(f'numpy generator of kind {kind!r}: only the MT19937 RandomState layout is saved')
    return {'kind': str(kind), 'keys': torch.from_numpy(np.asarray(keys).astype(np.int64)), 'pos': int(pos),
            'has_gauss': int(has_gauss), 'cached_gaussian': float(cached)}


def unpack_numpy_random(d, rng=np.random):
    rng.set_state((d['kind'], d['keys'].numpy().astype(np.uint32), d['pos'], d['has_gauss'], d['cached_gaussian']))


def pack_torch_generator(gen=None):
    return (torch.get_rng_state() if gen is None else gen.get_state()).clone()


def unpack_torch_generator(state, gen=None):
    if gen is None:
        torch.set_rng_state(state)
    else:
        gen.set_state(state)


def pack_host_generators(py=random, np_=np.random, torch_gen=None):
    """the three host generators the input stage draws from -> {'python', 'numpy', 'torch'} of plain data"""
    return {'python': pack_python_random(py), 'numpy': pack_numpy_random(np_), 'torch': pack_torch_generator(torch_gen)}


def unpack_host_generators(d, py=random, np_=np.random, torch_gen=None):
    unpack_python_random(d['python'], py)
    unpack_numpy_random(d['numpy'], np_)
    unpack_torch_generator(d['torch'], torch_gen)


# which attribute of which input-stage piece draws from which kind of host generator (and what "the global one" is)
_PIECE_GENERATORS = (('crop', 'rng', 'python'), ('crop', 'torch_gen', 'torch'), ('auto_augment', 'rng', 'python'),
                     ('auto_augment', 'np_rng', 'numpy'), ('collate_mixup', 'rng', 'numpy'), ('mixup_fn', 'rng', 'numpy'),
                     ('random_erasing', 'rng', 'python'))
_GLOBAL = {'python': random, 'numpy': np.random, 'torch': None}
_PACK = {'python': pack_python_random, 'numpy': pack_numpy_random, 'torch': pack_torch_generator}
_UNPACK = {'python': unpack_python_random, 'numpy': unpack_numpy_random, 'torch': unpack_torch_generator}


def _own_generators(step_fn):
    """{'piece.attr': (kind, generator)} of the pieces that were built with a generator of their own"""
    out = {}
    for piece, attr, kind in _PIECE_GENERATORS:
        obj = getattr(step_fn, piece, None)
        if obj is not None and hasattr(obj, attr) and getattr(obj, attr) is not _GLOBAL[kind]:
            out[f'{piece}.{attr}'] = (kind, getattr(obj, attr))
    return out


def capture_rank_state(step_fn=None, loader=None):
    """this rank's host-side state: the global generators, the pieces' own ones, the seed the engine's samplers were keyed by and
    the synthetic loader's device generator"""
    d = pack_host_generators()
    d['own'] = {k: _PACK[kind](g) for k, (kind, g) in (_own_generators(step_fn) if step_fn is not None else {}).items()}
    d['initial_seed'] = int(torch.initial_seed())
    g = getattr(loader, 'g', None)
    if isinstance(g, torch.Generator):
        d['loader_generator'] = g.get_state().clone()
    return d


def restore_rank_state(d, step_fn=None, loader=None):
    """-> names of what the file holds no state for"""
    missing = []
    unpack_host_generators(d)
    own = _own_generators(step_fn) if step_fn is not None else {}
    for k, (kind, g) in own.items():
        if k in d.get('own', {}):
            _UNPACK[kind](d['own'][k], g)
        else:
            missing.append(f'generator of {k}')
    g = getattr(loader, 'g', None)
    if isinstance(g, torch.Generator):
        if 'loader_generator' in d:
            g.set_state(d['loader_generator'])
        else:
            missing.append('loader generator')
    return missing


def pack_ranks(states, world):
    """the ranks' host states (rank order) -> the per-rank part of train_state"""
    if len(states) != world:
        raise ValueError(f'{len(states)} rank states for a world of {world}')
    return {'world_size': int(world), 'ranks': list(states)}


def select_rank(train_state, rank, world):
    """this rank's own host state out of a train_state; a run of another world size is refused"""
    saved = train_state['world_size']
    if saved != world:
        raise ValueError(f'the checkpoint was written by {saved} rank(s), this run has {world}: the per-rank generator states and '
                         'the loader position do not carry over (--no-resume-opt takes the weights and the epoch only)')
    return train_state['ranks'][rank]


def _gather(obj, rank, world, group=None):
    if world <= 1:
        return [obj]
    out = [None] * world if rank == 0 else None
    dist.gather_object(obj, out, dst=0, group=group)
    return out if rank == 0 else [None] * world


def _device_counters(step_fn):
    """{'dp_counter' / 'drop_counter': the int64 [1] device tensor} of the samplers the training engine has"""
    eng, out = step_fn.eng, {}
    if getattr(eng, 'dp_scale', None) and getattr(eng, 'dp_counter', None) is not None:
        out['dp_counter'] = eng.dp_counter
    if getattr(eng, 'drop', None):
        out['drop_counter'] = eng.drop['counter']
    return out


def loader_order(loader):
    """what the order a loader position counts in depends on beside (seed, epoch): the folder loader's repeated-augmentation
    settings (0 / 256 for every loader that has none)"""
    return {'aug_repeats': int(getattr(loader, 'aug_repeats', 0)), 'selected_round': int(getattr(loader, 'selected_round', 256))}


def check_loader_order(ts, loader):
    """a saved position is a position in the order it was saved under: a run with other repeated-augmentation settings is refused.
    A train_state without the two keys was written by a loader without them: 0 / 256"""
    saved = (int(ts.get('aug_repeats', 0)), int(ts.get('selected_round', 256)))
    mine = (int(getattr(loader, 'aug_repeats', 0)), int(getattr(loader, 'selected_round', 256)))
    if saved[0] != mine[0] or (saved[0] and saved[1] != mine[1]):
        raise ValueError(f'the checkpoint was written with aug_repeats {saved[0]}, selected_round {saved[1]}, this run has aug_repeats '
                         f'{mine[0]}, selected_round {mine[1]}: the loader position counts batches of another order '
                         '(--no-resume-opt takes the weights and the epoch only)')


def capture_train_state(step_fn, loader=None, epoch=0, batch=0, rank=0, world=1, group=None, device_counters=True):
    """everything beside weights, optimizer moments and EMA that decides the next step (module docstring), as plain data.
    epoch / batch: the loader position -- `batch` batches of `epoch` are consumed.  Every rank calls it (the host generator states
    are gathered to rank 0 with torch.distributed's object collective); rank 0's result is complete.
    device_counters=False leaves the samplers' device counters out: CheckpointSaver adds them from its snapshot without a
    host read on the training thread."""
    ts = {'opt_steps': int(step_fn.opt.steps), 'micro': int(step_fn.micro),
          'loader': {'epoch': int(epoch), 'batch': int(batch)}, **loader_order(loader)}
    if step_fn.random_erasing is not None:
        ts['re_offset'] = int(step_fn.random_erasing.offset)
    if device_counters:
        for k, t in _device_counters(step_fn).items():
            ts[k] = t.detach().cpu()
    ts.update(pack_ranks(_gather(capture_rank_state(step_fn, loader), rank, world, group), world))
    return ts


def restore_train_state(ts, step_fn, loader=None, rank=0, world=1):
    """put a train_state back into freshly built objects (built AFTER torch.manual_seed(saved_initial_seed(...)): the samplers are
    keyed when the engine is built).  Restores what is there -> names of what the file did not hold."""
    missing = restore_rank_state(select_rank(ts, rank, world), step_fn, loader)
    if int(torch.initial_seed()) != ts['ranks'][rank]['initial_seed']:
        raise RuntimeError(f"the samplers of this run are keyed by torch.initial_seed() = {torch.initial_seed()}, the checkpoint's by "
                           f"{ts['ranks'][rank]['initial_seed']}: call torch.manual_seed(saved_initial_seed(...)) before building")
    step_fn.opt.steps = ts['opt_steps']
    step_fn.opt._hp_host = None
    step_fn.micro = ts['micro']
    if step_fn.random_erasing is not None:
        if 're_offset' in ts:
            step_fn.random_erasing.offset = ts['re_offset']
        else:
            missing.append('RandomErasing offset')
    for k, t in _device_counters(step_fn).items():
        if k in ts:
            t.copy_(ts[k].to(t.device))
        else:
            missing.append(k)
    return missing


def saved_initial_seed(ts, rank=0):
    """the torch.initial_seed() this rank's DropPath / dropout samplers were built with, or None"""
    ranks = ts.get('ranks', []) if ts else []
    return ranks[rank]['initial_seed'] if rank < len(ranks) else None


def resume_checkpoint(ck, model, optimizer=None, model_ema=None, step_fn=None, loader=None, rank=0, world=1, resume_opt=True):
    """a checkpoint dict (read_checkpoint) into built objects -> (epoch to start at, batch to start at).
    An epoch-end file resumes at epoch + 1 (timm: version > 1), a recovery file inside its epoch at the batch after the one recorded.
    resume_opt=False (--no-resume-opt): weights (and EMA) and epoch only.  A file without train_state -- a reference checkpoint or
    an older file -- resumes weights, optimizer and epoch."""
    model.load_state_dict(_model_state(ck))
    if model_ema is not None:
        if 'state_dict_ema' in ck:
            model_ema.load_state_dict(_model_state({'state_dict': ck['state_dict_ema']}))
        else:
            model_ema.load_state_dict(model.state_dict())
    epoch = ck.get('epoch')
    start_epoch = 0 if epoch is None else epoch + 1 if ck.get('version', 1) > 1 else epoch
    start_batch = 0
    if not resume_opt:
        return start_epoch, 0
    if optimizer is not None and ck.get('optimizer') is not None:
        optimizer.load_state_dict(ck['optimizer'])
    ts = ck.get('train_state')
    if ts is None:
        _logger.info('the checkpoint has no train_state: weights, optimizer and epoch are resumed; generators, sampler counters and '
                     'the loader position start afresh')
        return start_epoch, 0
    check_loader_order(ts, loader)
    if step_fn is not None:
        missing = restore_train_state(ts, step_fn, loader, rank, world)
        if missing:
            _logger.info('train_state holds nothing for: %s', ', '.join(missing))
    pos = ts['loader']
    if ts.get('recovery'):
        start_epoch, start_batch = pos['epoch'], pos['batch']
    return start_epoch, start_batch


# ----------------------------------------------------------------------------------------------------------------------------
# snapshot on the device, write behind
# ----------------------------------------------------------------------------------------------------------------------------
class DeviceSnapshot:
    """Pre-allocated device mirrors of the flat buffers (parameters, BatchNorm buffers, optimizer moments, EMA, sampler counters).
    snapshot() enqueues the device-to-device copies on the current stream -- the step's: they read the state exactly as the steps
    enqueued so far leave it, and later steps are ordered behind them -- records an event and returns a function.  Called on
    another thread, that function waits for the event on a stream of its own, moves the mirrors into pinned host memory and
    builds the file's dicts.  The training thread reads nothing back and waits for nothing."""

    def __init__(self, model, optimizer=None, model_ema=None, step_fn=None):
        self.model, self.opt, self.ema, self.step_fn = model, optimizer, model_ema, step_fn
        st = model.flat_state()
        self.gen = st['gen']
        self.device = st['params'].device
        src = {'params': st['params'], 'buffers': st['buffers'], 'ibuffers': st['ibuffers']}
        if optimizer is not None:
            for n in optimizer.moment_names:
                src['opt.' + n] = getattr(optimizer, n)
        if model_ema is not None:
            src['ema.flat'] = model_ema.flat
            for n, b in model_ema.buffers.items():
                src['ema.buf.' + n] = b
        if step_fn is not None:
            for k, t in _device_counters(step_fn).items():
                src['counter.' + k] = t
        self.src = {k: v for k, v in src.items() if v.numel()}
        self.mirror = {k: torch.empty_like(v) for k, v in self.src.items()}
        self.host = None                         # pinned, allocated by the first write
        self.stream = torch.cuda.Stream(device=self.device)
        # where every state_dict entry lies: (mirror name, element offset, shape), or a constant captured once (e.g. bp_index)
        self.layout = self._layout(model.state_dict(), {'params': st['params'], 'buffers': st['buffers'], 'ibuffers': st['ibuffers']})
        self.ema_layout = None
        if model_ema is not None:
            flats = {'ema.flat': model_ema.flat}
            flats.update({'ema.buf.' + n: b for n, b in model_ema.buffers.items()})
            self.ema_layout = self._layout(model_ema.state_dict(), flats)

    @staticmethod
    def _layout(sd, flats):
        out = {}
        for k, v in sd.items():
            for name, f in flats.items():
                lo = f.data_ptr()
                if f.numel() and f.dtype == v.dtype and lo <= v.data_ptr() < lo + f.numel() * f.element_size():
                    out[k] = (name, (v.data_ptr() - lo) // f.element_size(), tuple(v.shape))
                    break
            else:
                out[k] = v.detach().cpu().clone() if v.numel() else torch.empty(v.shape, dtype=v.dtype)
        return out

    def snapshot(self):
        self.model.check_flat_generation(self.gen, 'DeviceSnapshot')
        self.model.flush_counters()
        with torch.no_grad():
            for k, v in self.src.items():
                self.mirror[k].copy_(v, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record()
        opt_host = None
        if self.opt is not None:
            opt_host = dict(kind=self.opt.kind, steps=int(self.opt.steps), param_groups=[dict(g) for g in self.opt.param_groups])

        def materialise():
            torch.cuda.set_device(self.device)               # the current device is per thread
            if self.host is None:
                self.host = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in self.mirror.items()}
            with torch.cuda.stream(self.stream):
                self.stream.wait_event(ready)
                for k, v in self.mirror.items():
                    self.host[k].copy_(v, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self.stream)
            done.synchronize()                               # this thread waits for its own stream, nobody else does

            def build(layout):
                sd = {}
                for k, where in layout.items():
                    if torch.is_tensor(where):
                        sd[k] = where
                    else:
                        name, off, shape = where
                        n = int(np.prod(shape)) if shape else 1
                        sd[k] = self.host[name].reshape(-1)[off:off + n].view(shape)
                return sd
            out = {'state_dict': build(self.layout), 'optimizer': None, 'counters': {}}
            if opt_host is not None:
                out['optimizer'] = dict(kind=opt_host['kind'], steps=opt_host['steps'],
                                        **{n: self.host['opt.' + n] for n in self.opt.moment_names},
                                        param_groups=opt_host['param_groups'])
            if self.ema_layout is not None:
                out['state_dict_ema'] = build(self.ema_layout)
            for k in self.host:
                if k.startswith('counter.'):
                    out['counters'][k[len('counter.'):]] = self.host[k].clone()
            return out
        return materialise


def _better(a, b, decreasing):
    return a < b if decreasing else a > b


class CheckpointSaver:
    """last.pth.tar, checkpoint-{epoch}.pth.tar, model_best.pth.tar (by `eval_metric`; 'loss' is decreasing) and
    recovery-{epoch}-{batch}.pth.tar (only the newest is kept) under `output`, each written to a temporary name in the same
    directory and moved into place with os.replace.

    source: an object whose snapshot() -- called on the training thread by take() -- returns a function that, on the writer
    thread, returns {'state_dict', 'optimizer', ['state_dict_ema'], ['counters']} of host tensors (DeviceSnapshot).
    take() returns once the snapshot is enqueued; the file is written behind.  The next take() and join() wait for the
    previous write first and re-raise what it raised; so does leaving a `with saver:` block.
    checkpoint_hist: keep that many best epoch files (None: all of them; timm's default is 10)."""

    def __init__(self, output, source, arch='', eval_metric='top1', checkpoint_hist=None):
        if checkpoint_hist is not None and checkpoint_hist < 1:
            raise ValueError(f'checkpoint_hist {checkpoint_hist}: at least 1, or None to keep every epoch file')
        self.output, self.source, self.arch = output, source, arch
        self.eval_metric = eval_metric
        self.decreasing = eval_metric == 'loss'
        self.hist = checkpoint_hist
        self.files = []                  # [(path, metric)] of the epoch files kept, best first
        self.best_metric = self.best_epoch = None
        self.recovery = None             # path of the newest recovery file
        self._thread = self._error = None
        os.makedirs(output, exist_ok=True)

    # -- waiting ---------------------------------------------------------------------------------------
    def join(self):
        """wait for the write in flight; an exception of the writer is raised here"""
        t, self._thread = self._thread, None
        if t is not None:
            t.join()
        e, self._error = self._error, None
        if e is not None:
            raise e

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.join()
        else:                            # an exception is on its way: finish the write, keep the first error
            try:
                self.join()
            except BaseException:
                pass

    # -- files -----------------------------------------------------------------------------------------
    @staticmethod
    def _serialise(ck, path):
        torch.save(ck, path)

    def _atomic_save(self, ck, path):
        tmp = f'{path}.tmp.{os.getpid()}'
        try:
            self._serialise(ck, tmp)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)

    def _atomic_copy(self, src, path):
        tmp = f'{path}.tmp.{os.getpid()}'
        try:
            try:
                os.link(src, tmp)
            except OSError:
                shutil.copyfile(src, tmp)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)

    def _write(self, materialise, ck, jobs):
        try:
            got = materialise()
            counters = got.pop('counters', None) or {}
            ck.update(got)
            if ck.get('train_state') is not None:
                ck['train_state'].update(counters)
            first = None
            for op, path in jobs:
                if op == 'save':
                    self._atomic_save(ck, path)
                    first = path
                elif op == 'copy':
                    self._atomic_copy(first, path)
                elif os.path.exists(path):
                    os.unlink(path)
        except BaseException as e:
            self._error = e

    def take(self, epoch, metric=None, train_state=None, recovery_batch=None):
        """snapshot now, write behind.  recovery_batch None: an epoch-end save (last, checkpoint-{epoch}, model_best by `metric`,
        retention); else the recovery file of (epoch, recovery_batch) -- call it at optimizer-step boundaries only."""
        self.join()
        materialise = self.source.snapshot()
        ck = {'epoch': epoch, 'arch': self.arch, 'state_dict': None, 'optimizer': None, 'version': 2, 'metric': metric}
        if train_state is not None:
            ck['train_state'] = dict(train_state, recovery=int(recovery_batch is not None))
        jobs = []
        if recovery_batch is not None:
            path = os.path.join(self.output, f'recovery-{epoch}-{recovery_batch}.pth.tar')
            jobs.append(('save', path))
            if self.recovery is not None and self.recovery != path:
                jobs.append(('remove', self.recovery))
            self.recovery = path
        else:
            jobs.append(('save', os.path.join(self.output, 'last.pth.tar')))
            path = os.path.join(self.output, f'checkpoint-{epoch}.pth.tar')
            jobs.append(('copy', path))
            self.files = [f for f in self.files if f[0] != path] + [(path, metric)]
            if metric is not None:       # best first; a file without a metric ranks last, newest first among equals
                ranked = sorted((f for f in self.files if f[1] is not None), key=lambda f: f[1], reverse=not self.decreasing)
                self.files = ranked + [f for f in self.files if f[1] is None]
            if metric is not None and (self.best_metric is None or _better(metric, self.best_metric, self.decreasing)):
                self.best_metric, self.best_epoch = metric, epoch
                jobs.append(('copy', os.path.join(self.output, 'model_best.pth.tar')))
            if self.hist is not None:
                for old, _ in self.files[self.hist:]:
                    jobs.append(('remove', old))
                self.files = self.files[:self.hist]
        self._thread = threading.Thread(target=self._write, args=(materialise, ck, jobs), name='checkpoint-writer', daemon=True)
        self._thread.start()
        return self.best_metric, self.best_epoch
