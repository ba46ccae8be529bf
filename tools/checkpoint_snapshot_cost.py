#!/usr/bin/env python3
"""What a checkpoint costs the training thread: ga_convnext_tiny_768, B = 256, bf16, AdamW, EMA on, synthetic batches, alternating
rounds in ONE process.  Three figures, written as markdown (profiles/checkpoint_snapshot.md):

  take      wall time the training thread spends inside one CheckpointSaver.take() (device snapshot enqueued, host state captured;
            the previous write has been joined beforehand, so this is the snapshot alone, not a wait for the disk)
  sync      the same state through the synchronous save_checkpoint (.cpu() on every tensor + torch.save on the training thread)
  step      ms per step over windows of CS_STEPS steps, a recovery point every CS_INTERVAL steps against none; a window ends in a
            device synchronise and, for the recovery arm, in the saver's join (the write that is still in flight is paid for)

    python tools/checkpoint_snapshot_cost.py [out.md]        CS_ROUNDS=5  CS_STEPS=40  CS_INTERVAL=20  CS_DIR=<where the files go>

Nothing is asserted: the figures are a record, not a gate."""
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import imagenet_models_amd as A  # noqa: E402

ROUNDS = int(os.environ.get('CS_ROUNDS', '5'))
STEPS = int(os.environ.get('CS_STEPS', '40'))
INTERVAL = int(os.environ.get('CS_INTERVAL', '20'))
MODEL, BATCH = os.environ.get('CS_MODEL', 'ga_convnext_tiny_768'), int(os.environ.get('CS_BATCH', '256'))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('checkpoint_snapshot_cost.py needs the GPU: a host timing says nothing about it')
    out_md = sys.argv[1] if len(sys.argv) > 1 else None
    torch.manual_seed(0)
    m = A.create_model(MODEL).cuda().train()
    opt = A.create_optimizer_v2(m, opt='adamw', lr=1e-3, weight_decay=0.05)
    step = A.TrainStep(m, opt, BATCH, lam=-0.8)
    ema = A.ModelEma(m, 0.9998)
    x = torch.randn(BATCH, 3, 224, 224, device='cuda')
    y = torch.randint(0, m.num_classes, (BATCH,), device='cuda')
    work = tempfile.mkdtemp(prefix='ckpt_cost_', dir=os.environ.get('CS_DIR') or None)
    saver = A.CheckpointSaver(work, A.DeviceSnapshot(m, opt, ema, step), arch=MODEL)

    def run(n, recover):
        for i in range(n):
            step(x, y)
            ema.update()
            if recover and (i + 1) % INTERVAL == 0:
                saver.take(0, train_state=A.capture_train_state(step, None, 0, i + 1, device_counters=False), recovery_batch=i)

    def window(recover):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(STEPS, recover)
        torch.cuda.synchronize()
        saver.join()
        return (time.perf_counter() - t0) * 1e3 / STEPS

    try:
        run(10, False)                                   # warm every plan; the first take allocates the pinned host mirror
        saver.take(0, train_state=A.capture_train_state(step, None, 0, 0, device_counters=False), recovery_batch=0)
        saver.join()
        torch.cuda.synchronize()
        take, sync, plain, rec = [], [], [], []
        for _ in range(ROUNDS):
            run(3, False)
            t0 = time.perf_counter()
            saver.take(0, train_state=A.capture_train_state(step, None, 0, 3, device_counters=False), recovery_batch=2)
            take.append((time.perf_counter() - t0) * 1e3)
            saver.join()
            run(3, False)
            t0 = time.perf_counter()
            A.save_checkpoint(m, opt, 0, os.path.join(work, 'sync.pth.tar'), arch=MODEL, model_ema=ema,
                              train_state=A.capture_train_state(step, None, 0, 3))
            sync.append((time.perf_counter() - t0) * 1e3)
            plain.append(window(False))
            rec.append(window(True))
        size = os.path.getsize(os.path.join(work, 'sync.pth.tar')) / 2 ** 20
    finally:
        try:
            saver.join()
        finally:
            shutil.rmtree(work, ignore_errors=True)

    def fmt(v):
        return f'{statistics.median(v):.2f} (min {min(v):.2f}, max {max(v):.2f})'
    lines = [
        '# Cost of a checkpoint on the training thread', '',
        f'Box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; files under `{os.path.dirname(work)}`.',
        f'Workload: `{MODEL}`, B = {BATCH}, bf16, AdamW, EMA on, synthetic batch; {ROUNDS} alternating rounds in one process '
        f'(`tools/checkpoint_snapshot_cost.py`), median (min, max).  File size {size:.0f} MiB.', '',
        '| figure | ms |', '|---|---|',
        f'| training thread inside one `CheckpointSaver.take()` | {fmt(take)} |',
        f'| the same state through the synchronous `save_checkpoint` | {fmt(sync)} |',
        f'| step, no recovery points ({STEPS}-step windows) | {fmt(plain)} |',
        f'| step, a recovery point every {INTERVAL} steps (windows end in the join of the last write) | {fmt(rec)} |', '',
        'The step figures include the write that is still in flight when a window ends; with a write that takes longer than '
        f'{INTERVAL} steps the next `take()` waits for it, and that wait is in the figure.']
    text = '\n'.join(lines) + '\n'
    print(text)
    if out_md:
        os.makedirs(os.path.dirname(os.path.abspath(out_md)), exist_ok=True)
        with open(out_md, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
