"""The depthwise 3 x 3 kernels of csrc/dwconv3.hip (MobileNetV1's conv_dw, MAP/models/map_mobilenet.py:25-37) through the C ABI:

  * forward / data gradient / weight gradient against CPU fp32 F.conv2d(groups=C) and its autograd at every MobileNetV1 shape, in
    both dtypes (bf16: inputs rounded to bf16 first, the reference in fp32 on the rounded values);
  * the BatchNorm sums fused into the forward against the sums of the reference output;
  * the stride-2 forms against ga_dwpool_* (PiT's pooling conv, mult = 1, zero bias): two independent code paths;
  * odd map sizes computed correctly, and unsupported shapes refused with GA_ERR_UNSUPPORTED."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (H, C, stride) of the 13 conv_dw layers of MobileNetV1 at 224 x 224
SHAPES = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 2),
          (7, 1024, 1)]
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}


def _ops():
    from imagenet_models_amd import ops
    return ops


def err(a, b):
    return float((a.float().cpu() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def case(B, H, C, s, dt, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + H + C + s)
    x = torch.randn(B, C, H, H, generator=g).to(dt).float()
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).contiguous()
    Ho = (H - 1) // s + 1
    dy = torch.randn(B, C, Ho, Ho, generator=g).to(dt).float()
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=s, padding=1, groups=C)
    y.backward(dy)
    return x, w, dy, y.detach(), xr.grad, wr.grad, Ho


def run_fwd(x, w, B, H, C, s, Ho, dt, stats=True):
    ops = _ops()
    y = torch.empty(B, Ho, Ho, C, dtype=dt, device='cuda')
    cs = torch.zeros(C, device='cuda') if stats else None
    cq = torch.zeros(C, device='cuda') if stats else None
    p = ops.Plan(eager=True)
    p.dwconv3_fwd(nhwc(x).to(dt).cuda(), w.cuda(), y, B, H, H, C, s, ops.ga_dtype(dt), colsum=cs, colsumsq=cq)
    torch.cuda.synchronize()
    return y, cs, cq


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('H,C,s', SHAPES)
def test_fwd_bwd_vs_conv2d(dt, H, C, s):
    ops = _ops()
    B = 2
    x, w, dy, yref, dxref, dwref, Ho = case(B, H, C, s, dt)
    tol = TOL[dt]
    y, cs, cq = run_fwd(x, w, B, H, C, s, Ho, dt)
    e = err(y, nhwc(yref))
    # fused BatchNorm sums: of the fp32 outputs before rounding
    es = float((cs.cpu() - yref.sum((0, 2, 3))).abs().max() / (yref.abs().sum((0, 2, 3)).max()))
    eq = float((cq.cpu() - (yref * yref).sum((0, 2, 3))).abs().max() / ((yref * yref).sum((0, 2, 3)).max()))
    dx = torch.empty(B, H, H, C, dtype=dt, device='cuda')
    dw = torch.full((C, 1, 3, 3), 0.25, device='cuda')            # bwd_weight accumulates
    p = ops.Plan(eager=True)
    dyd = nhwc(dy).to(dt).cuda()
    p.dwconv3_bwd_data(dyd, w.cuda(), dx, B, H, H, C, s, ops.ga_dtype(dt))
    p.dwconv3_bwd_weight(dyd, nhwc(x).to(dt).cuda(), dw, B, H, H, C, s, ops.ga_dtype(dt))
    torch.cuda.synchronize()
    edx = err(dx, nhwc(dxref))
    edw = err(dw - 0.25, dwref)
    print(f'[dwconv3 {H}x{C}/s{s} {dt}] y {e:.2e} sums {es:.2e} / {eq:.2e} dx {edx:.2e} dw {edw:.2e}')
    assert e <= tol and edx <= tol
    assert es <= 1e-5 and eq <= 1e-5
    assert edw <= (1e-5 if dt == torch.float32 else 1e-4)       # (fp32 sums of products of exactly representable values)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('H,C', [(112, 64), (56, 128), (28, 256), (14, 512), (15, 64)])
def test_stride2_vs_dwpool(dt, H, C):
    """ga_dwpool_* (mult 1, zero bias) is an independent implementation of the same stride-2 convolution"""
    ops = _ops()
    B = 2
    x, w, dy, _, _, _, Ho = case(B, H, C, 2, dt, seed=1)
    gd = ops.ga_dtype(dt)
    xd, dyd, wd = nhwc(x).to(dt).cuda(), nhwc(dy).to(dt).cuda(), w.cuda()
    zero = torch.zeros(C, device='cuda')
    y3, _, _ = run_fwd(x, w, B, H, C, 2, Ho, dt, stats=False)
    yp = torch.empty_like(y3)
    dx3, dxp = torch.empty(B, H, H, C, dtype=dt, device='cuda'), torch.empty(B, H, H, C, dtype=dt, device='cuda')
    dw3, dwp, dbp = torch.zeros(C, 9, device='cuda'), torch.zeros(C, 9, device='cuda'), torch.zeros(C, device='cuda')
    p = ops.Plan(eager=True)
    p.dwpool_fwd(xd, wd, zero, yp, B, H, H, C, 1, gd)
    p.dwconv3_bwd_data(dyd, wd, dx3, B, H, H, C, 2, gd)
    p.dwpool_bwd_data(dyd, wd, dxp, B, H, H, C, 1, gd)
    p.dwconv3_bwd_weight(dyd, xd, dw3, B, H, H, C, 2, gd)
    p.dwpool_bwd_weight(dyd, xd, dwp, dbp, B, H, H, C, 1, gd)
    torch.cuda.synchronize()
    tol = TOL[dt]
    assert err(y3, yp.float().cpu()) <= tol and err(dx3, dxp.float().cpu()) <= tol
    assert err(dw3, dwp.cpu()) <= 1e-5


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('H', [15, 9])
def test_odd_sizes(H, s):
    ops = _ops()
    B, C = 3, 40
    x, w, dy, yref, dxref, dwref, Ho = case(B, H, C, s, torch.float32, seed=2)
    y, cs, _ = run_fwd(x, w, B, H, C, s, Ho, torch.float32)
    dx = torch.empty(B, H, H, C, device='cuda')
    dw = torch.zeros(C, 1, 3, 3, device='cuda')
    p = ops.Plan(eager=True)
    p.dwconv3_bwd_data(nhwc(dy).cuda(), w.cuda(), dx, B, H, H, C, s, ops.GA_F32)
    p.dwconv3_bwd_weight(nhwc(dy).cuda(), nhwc(x).cuda(), dw, B, H, H, C, s, ops.GA_F32)
    torch.cuda.synchronize()
    assert err(y, nhwc(yref)) <= 1e-5 and err(dx, nhwc(dxref)) <= 1e-5 and err(dw, dwref) <= 1e-5
    assert err(cs, yref.sum((0, 2, 3))) <= 1e-5


def test_unsupported_shapes_are_refused():
    from imagenet_models_amd import _lib
    ops = _ops()
    lib = _lib.load()
    x = torch.zeros(2 * 8 * 8 * 16, device='cuda')
    w = torch.zeros(16 * 9, device='cuda')
    y = torch.zeros_like(x)
    GA_ERR_UNSUPPORTED = -2
    for C, s in ((12, 1), (16, 3), (16, 0)):
        rc = lib.ga_dwconv3_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 2, 8, 8, C, s, None, None, ops.GA_F32, None)
        assert rc == GA_ERR_UNSUPPORTED, (C, s, rc)
        rc = lib.ga_dwconv3_bwd_data(x.data_ptr(), w.data_ptr(), y.data_ptr(), 2, 8, 8, C, s, ops.GA_F32, None)
        assert rc == GA_ERR_UNSUPPORTED, (C, s, rc)
        rc = lib.ga_dwconv3_bwd_weight(x.data_ptr(), x.data_ptr(), w.data_ptr(), 2, 8, 8, C, s, ops.GA_F32, y.data_ptr(),
                                       ctypes.c_size_t(y.numel() * 4), None)
        assert rc == GA_ERR_UNSUPPORTED, (C, s, rc)
        assert lib.ga_dwconv3_bwd_weight_workspace(2, 8, 8, C, s, ops.GA_F32) == 0
    torch.cuda.synchronize()
    assert float(y.abs().sum()) == 0.0       # nothing was written
