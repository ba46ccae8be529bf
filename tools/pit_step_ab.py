"""Step time of the plain pit_s against map_pit_s, back to back on one device: alternating rounds of fused train steps (TrainStep,
adamw, synthetic input) in the bf16 mode, each round timed with a host clock around work that ends in a device synchronise.
Prints one line per round and a JSON summary (median and min .. max per model).

    python tools/pit_step_ab.py [--batch 256] [--rounds 5] [--steps 10] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagenet_models_amd as A  # noqa: E402


def make(name, batch, drop_path):
    m = A.create_model(name, drop_path_rate=drop_path).cuda().train()
    opt = A.create_optimizer_v2(m, opt='adamw', lr=1e-3, weight_decay=0.05)
    return A.TrainStep(m, opt, batch, lam=-0.8 if name.startswith('map_') else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--drop-path', type=float, default=0.1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: there is no CPU path to time'
    names = ('pit_s', 'map_pit_s')
    steps = {n: make(n, args.batch, args.drop_path) for n in names}
    x = torch.randn(args.batch, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (args.batch,), device='cuda')
    for n in names:
        for _ in range(args.warmup):
            steps[n](x, y)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for r in range(args.rounds):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                steps[n](x, y)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) * 1e3 / args.steps)
            print(f'round {r} {n}: {ms[n][-1]:.3f} ms/step', flush=True)
    print(json.dumps({'batch': args.batch, 'mode': 'bf16', 'steps_per_round': args.steps,
                      **{n: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)}
                         for n, v in ms.items()}}))


if __name__ == '__main__':
    main()
