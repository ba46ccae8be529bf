"""Where a tile of the persistent fused MLP backward spends its cycles (development aid).

Needs the diagnostic twin of the library: `make -C imagenet-models_amd/csrc libgaext_stamps.so`, then
    GAEXT_LIB=imagenet-models_amd/csrc/libgaext_stamps.so python tools/mlp_phases.py [--out FILE]
One launch per knob value at the bench shape (C = 96, M = 256 * 56 * 56, bf16, A stored, DH not, dW1 / db1 given).  The kernel sums
clock differences between its phase boundaries per workgroup (wave 0) and leaves the sums behind the partials; the stamps fence
the schedule, so the table is shares of a tile, not times."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagenet_models_amd import _lib, ops  # noqa: E402

PHASES = ('rows staged (loads, LDS writes, barrier)', 'P1: h, t products, GELU, a / dh to LDS, barrier',
          'P2: dx, dW1 products, a / dh rows out, weights staged', 'dx store tail', 'tile-end barrier')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rows', type=int, default=256 * 56 * 56)
    args = ap.parse_args()
    assert 'stamps' in os.environ.get('GAEXT_LIB', ''), 'run with GAEXT_LIB=<libgaext_stamps.so>'
    C, M = 96, args.rows
    H = 4 * C
    gd, bf = ops.GA_BF16, torch.bfloat16
    g = torch.Generator(device='cuda').manual_seed(1)
    X = torch.randn(M, C, device='cuda', generator=g).to(bf)
    DY = torch.randn(M, C, device='cuda', generator=g).to(bf)
    W1 = (torch.randn(H, C, device='cuda', generator=g) * C ** -0.5).to(bf)
    W2 = (torch.randn(C, H, device='cuda', generator=g) * H ** -0.5).to(bf)
    b1 = torch.randn(H, device='cuda', generator=g) * 0.1
    W1T, W2T = W1.T.contiguous(), W2.T.contiguous()
    A = torch.empty(M, H, device='cuda', dtype=bf)
    DX = torch.empty(M, C, device='cuda', dtype=bf)
    dW1, db1 = torch.zeros(H, C, device='cuda'), torch.zeros(H, device='cuda')
    need = ops.mlp_bwd_partials(M, C, gd)
    grid = need // (4 * (H * C + H))
    tiles = (M + 127) // 128
    lines = [f'{_lib.config_string()}', f'C = {C}, M = {M}: {tiles} tiles of 128 rows over {grid} workgroups; clock sums of wave 0 per '
             'workgroup, summed over the workgroups; shares of the stamped kernel, not times']
    for knob in (0, 1):
        part = torch.zeros(need // 4 + grid * 5 * 2, device='cuda')      # 5 64-bit sums per workgroup behind the partials
        with _lib.knobs(MLP_PREFETCH=knob):
            for _ in range(2):                                           # the second launch is the one read
                part[need // 4:].zero_()
                ops.Plan(eager=True).mlp_bwd(X, DY, W1, b1, W2T, W1T, A, None, DX, M, C, gd, dW1=dW1, db1=db1, partials=part)
                torch.cuda.synchronize()
        st = part[need // 4:].view(torch.int64).view(grid, 5).double().cpu()
        tot = st.sum()
        assert tot > 0, 'no stamps: is this the stamps build?'
        lines.append(f'MLP_PREFETCH={knob}: {float(tot) / tiles:.0f} clocks per tile')
        for name, v in zip(PHASES, st.sum(0)):
            lines.append(f'    {100 * float(v) / float(tot):5.1f} %   {float(v) / tiles:8.0f} clocks per tile   {name}')
        lines.append(f'    per workgroup total: min {float(st.sum(1).min()):.0f}  max {float(st.sum(1).max()):.0f} clocks')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
