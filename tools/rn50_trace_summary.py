#!/usr/bin/env python3
"""MAP-ResNet50 kernel times of one training run against the HBM byte floor of the new csrc/resnet.hip kernels:
    rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 bench.py --model map_resnet50 --steps 5 --warmup 2
    python tools/rn50_trace_summary.py <dir>/<name>_results.db [batch] [GB/s]
Steps are counted from the max-pool forward launches (one per step).  Per new kernel: launches and device time per step and the least
time its bytes take at the given bandwidth (default 6300 GB/s): one read of every big input and one write of every big output (bf16,
uint8 window indices); the SE kernels move a few MB and are listed without a floor.  Then the step's kernel time split into GEMM /
weight-gradient kernels and the rest."""
import sqlite3
import sys

NBLOCK, WIDTH, STRIDE = (3, 4, 6, 3), (64, 128, 256, 256), (1, 2, 2, 2)


def blocks():
    H, cin = 56, 64
    for n, w, s in zip(NBLOCK, WIDTH, STRIDE):
        for j in range(n):
            st = s if j == 0 else 1
            Ho = H // st
            yield H, cin, w, st, Ho, 4 * w, j == 0
            H, cin = Ho, 4 * w


def floors(B, e=2):
    f = dict.fromkeys(['maxpool_fwd', 'maxpool_bwd', 'bn_gelu_fwd', 'bn_gelu_bwd_reduce', 'bn_gelu_bwd_apply', 'se_res_fwd', 'se_res_bwd_a',
                       'se_res_bwd_b', 'subsample2_fwd', 'subsample2_bwd'], 0)
    mc = [3 * 112 * 112 * 64]          # stem: three BN + GELU at 112 x 112 x 64
    for H, cin, w, s, Ho, cout, ds in blocks():
        mc += [H * H * w, Ho * Ho * w]
        f['se_res_fwd'] += 3 * Ho * Ho * cout
        f['se_res_bwd_a'] += 4 * Ho * Ho * cout
        f['se_res_bwd_b'] += 3 * Ho * Ho * cout
        if ds and s == 2:
            f['subsample2_fwd'] += 2 * Ho * Ho * cin
            f['subsample2_bwd'] += 3 * Ho * Ho * cin
    tot = sum(mc)
    f['bn_gelu_fwd'], f['bn_gelu_bwd_reduce'], f['bn_gelu_bwd_apply'] = 2 * tot, 2 * tot, 3 * tot
    f = {k: v * B * e for k, v in f.items()}
    f['maxpool_fwd'] = B * (112 * 112 * 64 * e + 56 * 56 * 64 * (e + 1))
    f['maxpool_bwd'] = B * (56 * 56 * 64 * (e + 1) + 112 * 112 * 64 * 2 * e)
    return f


def main():
    db = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    bw = float(sys.argv[3]) if len(sys.argv) > 3 else 6300.0
    cur = sqlite3.connect(db).cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    sfx = [t for t in tabs if t.startswith('rocpd_kernel_dispatch_')][0][len('rocpd_kernel_dispatch_'):]
    rows = list(cur.execute(f"""select s.kernel_name, count(*), sum(d.end - d.start) from rocpd_kernel_dispatch_{sfx} d
                                join rocpd_info_kernel_symbol_{sfx} s on s.id = d.kernel_id group by s.kernel_name"""))
    steps = sum(n for name, n, _ in rows if 'maxpool_fwd_kernel' in name)
    fl = floors(B)
    print(f'{steps} steps; floor bandwidth {bw:.0f} GB/s, B = {B}, bf16')
    print(f'{"kernel":24s} {"launches/step":>13s} {"ms/step":>8s} {"floor ms":>8s} {"x floor":>7s}')
    new_ms = new_floor = 0.0
    for k in list(fl) + ['se_fwd1', 'se_fwd2', 'se_bwd1', 'se_bwd2', 'se_bwd3', 'se_bwd4', 'partial_sum']:
        hit = [(n, t) for name, n, t in rows if f'{k}_kernel' in name]
        if not hit:
            continue
        n, t = sum(h[0] for h in hit), sum(h[1] for h in hit)
        ms = t / steps / 1e6
        f = fl.get(k, 0) / bw / 1e6
        new_ms += ms
        new_floor += f
        print(f'{k:24s} {n / steps:13.1f} {ms:8.3f} {f:8.3f} {ms / f if f else float("nan"):7.1f}')
    print(f'{"new kernels":24s} {"":13s} {new_ms:8.3f} {new_floor:8.3f} {new_ms / new_floor:7.1f}')
    tot = sum(t for _, _, t in rows) / steps / 1e6
    gemm = sum(t for name, _, t in rows if any(s in name for s in ('gemm_', 'conv3_c64', 'tn2_reduce'))) / steps / 1e6
    print(f'step kernel time {tot:.2f} ms: GEMM / weight-gradient kernels {gemm:.2f} ms ({100 * gemm / tot:.1f} %), '
          f'new resnet.hip kernels {new_ms:.2f} ms ({100 * new_ms / tot:.1f} %), everything else {tot - gemm - new_ms:.2f} ms')


if __name__ == '__main__':
    main()
