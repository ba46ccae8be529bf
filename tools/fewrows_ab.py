#!/usr/bin/env python3
"""A/B of the few-row forms (csrc/gemm_fewrows.hip, knob FEWROWS) against ga_gemm / ga_wgrad, interleaved rounds in ONE process:
median device time per launch of each arm, back-to-back launches on one stream.

    python tools/fewrows_ab.py [out.json]        FR_ROUNDS=9  FR_ITERS=20

  sweep   M = 64 .. 1024 at N x K = 192 x 768 and 768 x 192, NT (bias) and TN (accumulate + dbias): where the row bound belongs
          (FEWROWS_MAXM is lifted for the new arm)
  corpus  the few-row descriptors of ga_convnext_tiny_768 in tests/golden/gemm_forms.json (M <= 512, batch <= 64) under the default
          knobs: what each launch of the step gains, with the bytes of its operands; a descriptor the predicate leaves alone has
          few = none and the same kernel in both arms"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
from imagenet_models_amd import ops, _lib as L  # noqa: E402
import gemm_forms as T  # noqa: E402

ROUNDS = int(os.environ.get('FR_ROUNDS', '9'))
ITERS = int(os.environ.get('FR_ITERS', '20'))
BF = torch.bfloat16


def time_once(fn, d):
    s = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        L.check(fn(C.byref(d), s), 'launch')
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def ab(d, old, new, knobs):
    """median ms per launch: (old entry point, new entry point under `knobs`)"""
    lib = L.load()
    arms = {'old': (getattr(lib, old), {}), 'new': (getattr(lib, new), knobs)}
    t = {k: [] for k in arms}
    for k, (fn, kv) in arms.items():
        with L.knobs(**kv):
            time_once(fn, d)
    for _ in range(ROUNDS):
        for k, (fn, kv) in arms.items():
            with L.knobs(**kv):
                t[k].append(time_once(fn, d))
    return tuple(sorted(t[k])[len(t[k]) // 2] for k in ('old', 'new'))


def buf(n, dt=BF):
    return (torch.randn(int(n), device='cuda') * 0.5).to(dt)


def sweep(rows):
    lift = dict(FEWROWS_MAXM=1 << 20)
    for N, K in ((192, 768), (768, 192)):
        for M in (64, 128, 256, 512, 1024):
            d = ops._set(L.GemmDesc(), M=M, N=N, K=K, batch=1, dtype=L.GA_BF16, A=buf(M * K), lda=K, B=buf(N * K), ldb=K,
                         C=buf(M * N), ldc=N, alpha=1.0, bias=buf(N, torch.float32), rows_per_scale=1)
            w = ops._set(L.WgradDesc(), M=M, N=N, K=K, batch=1, dtype=L.GA_BF16, Y=buf(M * N), ldy=N, X=buf(M * K), ldx=K,
                         dW=buf(N * K, torch.float32), ldw=K, dbias=buf(N, torch.float32), alpha=1.0, split_m=1, accumulate=1)
            for kind, desc, old, new in (('nt', d, 'ga_gemm', 'ga_gemm_fewrows'), ('tn', w, 'ga_wgrad', 'ga_wgrad_fewrows')):
                with L.knobs(**lift):
                    few = T.FEWROWS[old](desc)
                o, n = ab(desc, old, new, lift)
                rows.append(dict(part='sweep', kind=kind, M=M, N=N, K=K, old_ms=round(o, 5), new_ms=round(n, 5), speedup=round(o / n, 3), few=few))
                print(f'sweep {kind} M={M:5d} N={N} K={K}: old {o * 1e3:7.2f} us  new {n * 1e3:7.2f} us  x{o / n:.2f}  ({few})', flush=True)


def corpus(rows):
    cases = [c for c in json.load(open(T.GOLDEN)) if c['src'] == 'ga_convnext_tiny_768' and c['desc']['M'] <= 512 and c['desc']['batch'] <= 64]
    for c in cases:
        f, fn = dict(c['desc']), c['fn']
        Z, M, N, K = f['batch'], f['M'], f['N'], f['K']

        def mat(rows_, ld, stride, dt=BF):
            return buf(Z * f.get(stride, 0) + rows_ * f[ld] + 64, dt)
        if fn == 'ga_gemm':
            ptr = dict(A=mat(M, 'lda', 'strideA'), B=mat(N, 'ldb', 'strideB'),
                       C=mat(M, 'ldc', 'strideC', torch.float32 if f.get('c_f32') else BF))
            if f.get('C2'):
                ptr['C2'] = mat(M, 'ldc', 'strideC')
            if f.get('R'):
                ptr['R'] = mat(M, 'ldr', 'strideR')
            if f.get('H'):
                ptr['H'] = mat(M, 'ldh', 'strideH')
            for name, stride in (('bias', 'strideBias'), ('colsum', 'strideCol'), ('colsumsq', 'strideCol')):
                if f.get(name):
                    ptr[name] = buf(Z * f.get(stride, 0) + N + 64, torch.float32)
            nbytes = 2 * Z * (M * K + N * K) + (4 if f.get('c_f32') else 2) * Z * M * N * (1 + bool(f.get('C2')) + bool(f.get('R')) + bool(f.get('H')))
            d = ops._set(L.GemmDesc(), **{**f, **ptr})
        else:
            ptr = dict(Y=mat(M, 'ldy', 'strideY'), X=mat(M, 'ldx', 'strideX'), dW=mat(N, 'ldw', 'strideW', torch.float32))
            if f.get('dbias'):
                ptr['dbias'] = buf(Z * f.get('strideDbias', 0) + N + 64, torch.float32)
            nbytes = 2 * Z * (M * N + M * K) + 4 * Z * N * K * (1 + bool(f.get('accumulate')))
            d = ops._set(L.WgradDesc(), **{**f, **ptr})
        few = T.FEWROWS[fn](d)
        o, n = ab(d, fn, fn + '_fewrows', {})
        rows.append(dict(part='corpus', fn=fn, M=M, N=N, K=K, batch=Z, form=c['form'][0], few=few, operand_bytes=nbytes,
                         old_ms=round(o, 5), new_ms=round(n, 5), speedup=round(o / n, 3)))
        print(f"corpus {fn:8s} {M}x{N}x{K} b{Z:<2d} {c['form'][0]:18s} {few:22s} old {o * 1e3:7.2f} us  new {n * 1e3:7.2f} us  x{o / n:.2f}  "
              f'{nbytes / 1e6:.2f} MB', flush=True)


def main():
    rows = []
    print(L.config_string(), flush=True)
    sweep(rows)
    corpus(rows)
    if len(sys.argv) > 1:
        json.dump(dict(config=L.config_string(), rounds=ROUNDS, iters=ITERS, rows=rows), open(sys.argv[1], 'w'), indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
