#!/usr/bin/env python3
"""Depthwise 3 x 3 kernel times of a MobileNetV1 training run against their HBM byte floor:
    rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python3 bench.py --model mobilenet_v1 ...
    python tools/dwconv3_trace_summary.py <dir>/<name>_results.db [batch] [GB/s]
Per kernel form (forward / data gradient / weight gradient, stride 1 / 2): launches per step, device time per step and per launch,
and the least time the bytes the form must move take at the given bandwidth (default 6300 GB/s, the measured copy rate): one read of
the input and one write of the output (forward, data gradient), one read of each operand (weight gradient), bf16.  Steps are
counted from the forward launches (13 per step)."""
import sqlite3
import sys

# (H, C, stride) of the 13 conv_dw layers at 224 x 224 (map_mobilenet.py:39-63)
LAYERS = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2)] + [(14, 512, 1)] * 5 + \
         [(14, 512, 2), (7, 1024, 1)]


def floor_bytes(B, stride, elt=2):
    tot = 0
    for H, C, s in LAYERS:
        if s != stride:
            continue
        Ho = (H - 1) // s + 1
        tot += B * (H * H + Ho * Ho) * C * elt
    return tot


def main():
    db = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    bw = float(sys.argv[3]) if len(sys.argv) > 3 else 6300.0
    cur = sqlite3.connect(db).cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    sfx = [t for t in tabs if t.startswith('rocpd_kernel_dispatch_')][0][len('rocpd_kernel_dispatch_'):]
    rows = list(cur.execute(f"""select s.kernel_name, count(*), sum(d.end - d.start) from rocpd_kernel_dispatch_{sfx} d
                                join rocpd_info_kernel_symbol_{sfx} s on s.id = d.kernel_id where s.kernel_name like '%dw3_%'
                                group by s.kernel_name"""))
    n_fwd = sum(c for k, c, _ in rows if 'dw3_fwd' in k)
    steps = n_fwd / len(LAYERS)
    print(f'{steps:g} steps traced, batch {B}, floor at {bw:g} GB/s\n')
    print('| kernel | stride | launches / step | ms / step | us / launch | byte floor ms / step | floor / time |')
    print('|---|---|---|---|---|---|---|')
    tot_t = tot_f = 0.0
    for form in ('dw3_fwd', 'dw3_bwd_data', 'dw3_bwd_weight', 'dw3_wgrad_reduce'):
        for s in (1, 2):
            sel = [(c, t) for k, c, t in rows if form in k and (form == 'dw3_wgrad_reduce' or f'Li{s}E' in k)]
            if not sel or (form == 'dw3_wgrad_reduce' and s == 2):
                continue
            c, t = sum(a for a, _ in sel), sum(b for _, b in sel)
            ms = t / 1e6 / steps
            fl = 0.0 if form == 'dw3_wgrad_reduce' else floor_bytes(B, s) / (bw * 1e9) * 1e3
            tot_t += ms
            tot_f += fl
            ratio = f'{fl / ms:.2f}' if fl else '-'
            print(f'| {form} | {s if form != "dw3_wgrad_reduce" else "-"} | {c / steps:g} | {ms:.3f} | {t / 1e3 / c:.1f} | {fl:.3f} | {ratio} |')
    print(f'| all | | | {tot_t:.3f} | | {tot_f:.3f} | {tot_f / tot_t:.2f} |')


if __name__ == '__main__':
    main()
