"""GPU: the MAP-ResNet50 kernels of csrc/resnet.hip against PyTorch CPU fp32 (autograd of the reference's layers), bf16 and fp32:
max pool (incl. ties, odd sizes, NaN), BatchNorm-apply + GELU, the SE unit with BatchNorm over the batch, the SE-scale / DropPath /
residual / ReLU tail and the stride-2 subsample; GA_ERR_UNSUPPORTED for C % 8 != 0; bitwise-repeatable backward launches."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
TOL = {'fp32': 2e-5, 'bf16': 2e-2}


def _plan():
    from imagenet_models_amd.ops import Plan
    return Plan(eager=True)


def _ga(dt):
    from imagenet_models_amd.ops import ga_dtype
    return ga_dtype(DT[dt])


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(DT[dt]).cuda()


def nchw(t, B, H, W):
    return t.float().cpu().view(B, H, W, -1).permute(0, 3, 1, 2)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,H,C', [(2, 112, 64), (3, 7, 16), (2, 15, 24)])
def test_maxpool(dt, B, H, C):
    g = torch.Generator().manual_seed(H)
    x = (torch.randn(B, C, H, H, generator=g) * 2).round() / 2          # quantised: many ties inside the windows
    x = x.to(DT[dt]).float()
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    dy = torch.randn(y.shape, generator=g).to(DT[dt]).float()
    y.backward(dy)
    Ho = y.shape[2]
    xg, yg = nhwc(x, dt), torch.empty(B * Ho * Ho, C, dtype=DT[dt], device='cuda')
    idx = torch.empty(B * Ho * Ho, C, dtype=torch.uint8, device='cuda')
    p = _plan()
    p.maxpool3s2_fwd(xg, yg, idx, B, H, H, C, _ga(dt))
    assert torch.equal(nchw(yg, B, Ho, Ho), y.detach())
    dx = torch.full((B * H * H, C), 0.5, dtype=DT[dt], device='cuda')
    p.maxpool3s2_bwd(nhwc(dy, dt), idx, dx, B, H, H, C, _ga(dt), accumulate=True)
    assert rel(nchw(dx, B, H, H), xr.grad + 0.5) <= TOL[dt]
    dx1, dx2 = torch.empty_like(dx), torch.empty_like(dx)
    for d in (dx1, dx2):
        p.maxpool3s2_bwd(nhwc(dy, dt), idx, d, B, H, H, C, _ga(dt))
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx2) and rel(nchw(dx1, B, H, H), xr.grad) <= TOL[dt]


def test_maxpool_nan_propagates():
    x = torch.randn(1, 8, 9, 9)
    x[0, 3, 4, 4] = float('nan')          # inside one window
    x[0, 3, 3, 3] = float('nan')          # inside four
    y = F.max_pool2d(x, 3, 2, 1)
    yg = torch.empty(25, 8, device='cuda')
    idx = torch.empty(25, 8, dtype=torch.uint8, device='cuda')
    _plan().maxpool3s2_fwd(nhwc(x, 'fp32'), yg, idx, 1, 9, 9, 8, _ga('fp32'))
    out = nchw(yg, 1, 5, 5)
    assert torch.equal(torch.isnan(out), torch.isnan(y)) and int(torch.isnan(y).sum()) == 4
    m = ~torch.isnan(y)
    assert torch.equal(out[m], y[m])


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('train', [True, False])
def test_bn_gelu(dt, train):
    g = torch.Generator().manual_seed(1)
    B, C, H = 4, 24, 9
    x = (torch.randn(B, C, H, H, generator=g) * 1.5 + 0.3).to(DT[dt]).float()
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.uniform_(-0.5, 0.5, generator=g)
        bn.running_mean.uniform_(-0.2, 0.2, generator=g)
        bn.running_var.uniform_(0.5, 1.5, generator=g)
    bn.train(train)
    xr = x.clone().requires_grad_(True)
    y = F.gelu(bn(xr))
    dy = torch.randn(y.shape, generator=g).to(DT[dt]).float()
    y.backward(dy)
    M = B * H * H
    if train:
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    else:
        mean, var = bn.running_mean, bn.running_var
    rstd = (var + 1e-5).rsqrt()
    scale = bn.weight.detach() * rstd
    shift = bn.bias.detach() - mean * scale
    cu = lambda t: t.detach().float().contiguous().cuda()
    xg, yg = nhwc(x, dt).view(M, C), torch.empty(M, C, dtype=DT[dt], device='cuda')
    p = _plan()
    p.bn_gelu_fwd(xg, cu(scale), cu(shift), yg, M, C, _ga(dt))
    assert rel(nchw(yg, B, H, H), y.detach()) <= TOL[dt]
    if not train:
        return
    s1, s2 = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    dyg, dx = nhwc(dy, dt).view(M, C), torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.bn_gelu_bwd_reduce(dyg, xg, cu(scale), cu(shift), cu(mean), cu(rstd), s1, s2, M, C, _ga(dt))
    p.bn_gelu_bwd_apply(dyg, xg, cu(scale), cu(shift), cu(mean), cu(rstd), cu(bn.weight), s1, s2, M, dx, M, C, _ga(dt))
    assert rel(s2, bn.weight.grad) <= 1e-4 and rel(s1, bn.bias.grad) <= 1e-4
    assert rel(nchw(dx, B, H, H), xr.grad) <= (1e-4 if dt == 'fp32' else 3e-2)
    a1, a2 = torch.empty_like(s1), torch.empty_like(s2)
    p.bn_gelu_bwd_reduce(dyg, xg, cu(scale), cu(shift), cu(mean), cu(rstd), a1, a2, M, C, _ga(dt))
    torch.cuda.synchronize()
    assert torch.equal(a1, s1) and torch.equal(a2, s2)


def _se_ref(C, g):
    r = C // 16
    se = nn.Sequential(nn.Conv2d(C, r, 1, bias=False), nn.BatchNorm2d(r), nn.GELU(), nn.Conv2d(r, C, 1, bias=True), nn.Sigmoid())
    with torch.no_grad():
        for prm in se.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
        se[1].running_mean.uniform_(-0.2, 0.2, generator=g)
        se[1].running_var.uniform_(0.5, 1.5, generator=g)
    return se


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('rs', [False, True])
@pytest.mark.parametrize('ds', [False, True])
def test_se_residual_block_tail(dt, train, rs, ds):
    """relu(res' + r * se(bn3(x3)) * bn3(x3)) with BN-3 (and the downsample BN: res' = bn_d(res)) in train mode, against autograd"""
    g = torch.Generator().manual_seed(7)
    B, C, H = 4, 64, 6
    HW, M = H * H, B * H * H
    x3 = (torch.randn(B, C, H, H, generator=g) + 0.2).to(DT[dt]).float()
    res = torch.randn(B, C, H, H, generator=g).to(DT[dt]).float()
    bn3, bnd = nn.BatchNorm2d(C), nn.BatchNorm2d(C)
    with torch.no_grad():
        for b in (bn3, bnd):
            b.weight.uniform_(0.5, 1.5, generator=g)
            b.bias.uniform_(-0.5, 0.5, generator=g)
    se = _se_ref(C, g)
    se.train(train)
    run0 = (se[1].running_mean.clone(), se[1].running_var.clone())        # before the reference forward updates them
    r = torch.tensor([1.0, 0.0, 1.25, 2.0]) if rs else torch.ones(B)
    x3r, resr = x3.clone().requires_grad_(True), res.clone().requires_grad_(True)
    u = bn3(x3r)
    gate = se(u.mean((2, 3), keepdim=True))
    y = F.relu((bnd(resr) if ds else resr) + r.view(B, 1, 1, 1) * gate * u)
    dy = torch.randn(y.shape, generator=g).to(DT[dt]).float()
    y.backward(dy)
    cu = lambda t: t.detach().float().contiguous().cuda()
    mean3, var3 = x3.mean((0, 2, 3)), x3.var((0, 2, 3), unbiased=False)
    rstd3 = (var3 + 1e-5).rsqrt()
    sc3 = bn3.weight.detach() * rstd3
    sh3 = bn3.bias.detach() - mean3 * sc3
    R = C // 16
    x3g, resg = nhwc(x3, dt).view(M, C), nhwc(res, dt).view(M, C)
    S = torch.empty(B, C, device='cuda')
    p = _plan()
    p.spatial_sum(x3g, None, S, B, HW, C, 1.0, _ga(dt))
    rm, rv = cu(run0[0]), cu(run0[1])
    rm0, rv0 = rm.clone(), rv.clone()
    hpre, h = torch.empty(B, R, device='cuda'), torch.empty(B, R, device='cuda')
    mean, rstd, gt = torch.empty(R, device='cuda'), torch.empty(R, device='cuda'), torch.empty(B, C, device='cuda')
    W1, W2 = cu(se[0].weight).view(R, C), cu(se[3].weight).view(C, R)
    p.se_bn_fwd(S, HW, cu(sc3), cu(sh3), W1, cu(se[1].weight), cu(se[1].bias), rm, rv, W2, cu(se[3].bias), hpre, mean, rstd, h, gt, B, C, R,
                train)
    assert rel(gt, gate.detach().view(B, C)) <= (1e-5 if dt == 'fp32' else 1e-3)
    if train:
        assert rel(rm, se[1].running_mean) <= 1e-5 and rel(rv, se[1].running_var) <= 1e-5
        assert not torch.equal(rm, rm0)
    else:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    rdev = cu(r) if rs else None
    if ds:
        md, vd = res.mean((0, 2, 3)), res.var((0, 2, 3), unbiased=False)
        scd = bnd.weight.detach() * (vd + 1e-5).rsqrt()
        rsc, rsh = cu(scd), cu(bnd.bias.detach() - md * scd)
    else:
        rsc = rsh = None
    yg = torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.se_residual_fwd(x3g, cu(sc3), cu(sh3), gt, rdev, resg, rsc, rsh, yg, B, HW, C, _ga(dt))
    assert rel(nchw(yg, B, H, H), y.detach()) <= TOL[dt]
    if not train:
        return
    dyg = nhwc(dy, dt).view(M, C)
    dm = torch.empty(M, C, dtype=DT[dt], device='cuda')
    P1, P2 = torch.empty(B, C, device='cuda'), torch.empty(B, C, device='cuda')
    p.se_residual_bwd_a(dyg, yg, x3g, cu(mean3), cu(rstd3), dm, P1, P2, B, HW, C, _ga(dt))
    dz, dh, dsp = torch.empty(B, C, device='cuda'), torch.empty(B, R, device='cuda'), torch.empty(B, C, device='cuda')
    s1, s2 = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    gW1, gg1, gb1, gW2, gb2 = (torch.zeros_like(t) for t in (W1, cu(se[1].weight), cu(se[1].bias), W2, cu(se[3].bias)))
    p.se_bn_bwd(P1, P2, rdev, cu(bn3.weight), cu(bn3.bias), cu(mean3), cu(rstd3), S, HW, cu(sc3), cu(sh3), W1, cu(se[1].weight),
                cu(se[1].bias), W2, hpre, mean, rstd, h, gt, dz, dh, dsp, s1, s2, gW1, gg1, gb1, gW2, gb2, B, C, R)
    dx3 = torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.se_residual_bwd_b(dm, x3g, cu(mean3), cu(rstd3), cu(bn3.weight), gt, rdev, dsp, s1, s2, dx3, B, HW, C, _ga(dt))
    tol = 2e-4 if dt == 'fp32' else 5e-2
    assert rel(gW1, se[0].weight.grad.view(R, C)) <= tol and rel(gW2, se[3].weight.grad.view(C, R)) <= tol
    assert rel(gg1, se[1].weight.grad) <= tol and rel(gb1, se[1].bias.grad) <= tol and rel(gb2, se[3].bias.grad) <= tol
    assert rel(s2, bn3.weight.grad) <= tol and rel(s1, bn3.bias.grad) <= tol
    assert rel(nchw(dx3, B, H, H), x3r.grad) <= tol
    if not ds:
        assert rel(nchw(dm, B, H, H), resr.grad) <= TOL[dt]
    # two launches of the tail's backward on the same input: bitwise equal
    dmb, Q1, Q2 = torch.empty_like(dm), torch.empty_like(P1), torch.empty_like(P2)
    p.se_residual_bwd_a(dyg, yg, x3g, cu(mean3), cu(rstd3), dmb, Q1, Q2, B, HW, C, _ga(dt))
    dx3b = torch.empty_like(dx3)
    p.se_residual_bwd_b(dmb, x3g, cu(mean3), cu(rstd3), cu(bn3.weight), gt, rdev, dsp, s1, s2, dx3b, B, HW, C, _ga(dt))
    torch.cuda.synchronize()
    assert torch.equal(dm, dmb) and torch.equal(P1, Q1) and torch.equal(P2, Q2) and torch.equal(dx3, dx3b)


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
def test_subsample_downsample(dt):
    """1 x 1 / 2 conv == subsample + 1 x 1 conv; the transpose scatters to the even pixels (zero elsewhere, or added)"""
    g = torch.Generator().manual_seed(3)
    B, C, H = 2, 16, 14
    x = torch.randn(B, C, H, H, generator=g).to(DT[dt]).float()
    Ho = 7
    xs = torch.empty(B * Ho * Ho, C, dtype=DT[dt], device='cuda')
    p = _plan()
    p.subsample2_fwd(nhwc(x, dt), xs, B, H, H, C, _ga(dt))
    assert torch.equal(nchw(xs, B, Ho, Ho), x[:, :, ::2, ::2])
    w = torch.randn(32, C, 1, 1, generator=g)
    assert rel(F.conv2d(nchw(xs, B, Ho, Ho), w), F.conv2d(x, w, stride=2)) <= 1e-5
    dy = torch.randn(B, C, Ho, Ho, generator=g).to(DT[dt]).float()
    dx = torch.full((B * H * H, C), 7.0, dtype=DT[dt], device='cuda')
    p.subsample2_bwd(nhwc(dy, dt), dx, B, H, H, C, _ga(dt))
    ref = torch.zeros(B, C, H, H)
    ref[:, :, ::2, ::2] = dy
    assert torch.equal(nchw(dx, B, H, H), ref)
    p.subsample2_bwd(nhwc(dy, dt), dx, B, H, H, C, _ga(dt), accumulate=True)
    assert torch.equal(nchw(dx, B, H, H), 2 * ref)


def test_unsupported_channel_count():
    from imagenet_models_amd import _lib as L
    lib = L.load()
    x = torch.zeros(4 * 9 * 9 * 12, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    assert lib.ga_maxpool3s2_fwd(x.data_ptr(), x.data_ptr(), None, 4, 9, 9, 12, L.GA_F32, s) == -2
    assert lib.ga_bn_gelu_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 4 * 81, 12, L.GA_F32, s) == -2
    assert lib.ga_subsample2_fwd(x.data_ptr(), x.data_ptr(), 4, 9, 9, 12, L.GA_F32, s) == -2
    assert lib.ga_se_residual_bwd_a(*([x.data_ptr()] * 8), 4, 81, 12, L.GA_F32, s) == -2
    assert lib.ga_se_bn_fwd(x.data_ptr(), 81, *([x.data_ptr()] * 14), 4, 12, 1, 1, s) == -2
