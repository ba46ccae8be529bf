"""GPU: the csrc/resnet.hip kernels at the shapes the MAP-ResNet50 engine launches them with, against plain float64 PyTorch on the CPU.

test_resnet_kernels_gpu.py runs every kernel at toy sizes (B <= 4, C <= 64, SE hidden width 4, <= 324 rows): one pass of every
grid-stride loop, one channel block, one batch block.  This file runs the paths those sizes never reach:

  * a second grid-stride pass of every elementwise launch (blocks_for caps the grid at 4096 x 256 threads = 1,048,576 items of
    8 channels), asserted from the shape before the launch;
  * bn_gelu_bwd_reduce with several channel blocks, gy at its 256 cap and at its 2048 / gx cap, and many rows per lane;
  * se_bn_fwd / _bwd at B = 256 and the engine's (C, R): several sample rows per wave, se_bwd2's channel loop more than once,
    several channel and 8-row batch blocks of se_fwd2 / se_bwd3 and a batch tail, every se_check limit at once (B = 1024, C = 2048,
    R = 128: a full hp[kSeMaxB] LDS array);
  * se_residual_bwd_a with C / 64 > 1 channel blocks; the stride-2 subsample at the three downsample shapes;
  * edges: zero-variance channels (BN-GELU and the SE hidden BatchNorm), DropPath rows with r = 0, the GA_ERR_UNSUPPORTED refusals of
    se_check with nothing written, a too-small bn_gelu_bwd_reduce workspace.

References: float64 on the CPU (bf16 cases: the inputs rounded to bf16 first, the reference run on the rounded values), autograd for
every backward.  Gates (max |error| / max |reference|) come from the dtype's rounding: fp32 outputs 1e-5 (a few ulp of fp32 through
erf / exp), fp32 reductions 1e-4 (fp32 sums of up to 150k terms), running statistics 1e-5, bf16 stored outputs 1e-2 (bf16 has an 8-bit
significand: 2^-8 = 3.9e-3 relative per element, one rounding of the output plus one of an input), bf16-input fp32 reductions 1e-3;
max pool and subsample only move values, so they are exact.  Every reduction is also launched twice and compared bitwise."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DT = {'fp32': torch.float32, 'bf16': torch.bfloat16}
OUT_GATE = {'fp32': 1e-5, 'bf16': 1e-2}
RED_GATE = {'fp32': 1e-4, 'bf16': 1e-3}
STAT_GATE = 1e-5
GRID_ITEMS = 4096 * 256          # blocks_for(): beyond this many 8-channel items a launch makes a second grid-stride pass
EPS = 1e-5
GA_OK, GA_ERR_BAD_ARG, GA_ERR_UNSUPPORTED = 0, -1, -2     # include/gaext.h


def _plan():
    from imagenet_models_amd.ops import Plan
    return Plan(eager=True)


def _ga(dt):
    from imagenet_models_amd.ops import ga_dtype
    return ga_dtype(DT[dt])


def _lib():
    from imagenet_models_amd import _lib as L
    return L, L.load()


def err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def check(tag, got, ref, gate):
    e = err(got, ref)
    print(f'  {tag:<44s} {e:.2e}  (gate {gate:.0e})')
    assert e <= gate, f'{tag}: {e:.3e} > {gate:.0e}'


def q(t, dt):
    """round to the tested dtype, back in float64: the values the kernel sees"""
    return t.to(DT[dt]).double()


def dev(t, dt=None):
    return t.to(DT[dt] if dt else torch.float32).contiguous().cuda()


def f32(t):
    return t.float().contiguous().cuda()


def _rand(shape, g, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm-apply + GELU: rows x C (NHWC rows), batch statistics of the raw conv output x
# ---------------------------------------------------------------------------------------------------------------------------
def _red_grid(rows, C):
    """(gx, gy) of ga_bn_gelu_bwd_reduce (resnet.hip red_gy)"""
    gx = (C // 8 + 7) // 8
    return gx, max(1, min(256, (rows + 31) // 32, max(1, 2048 // gx)))


BN_GELU_SHAPES = [
    (12, 112, 64),      # stem: rows 150,528, n8 1,204,224 > 1,048,576 (two grid-stride passes); reduce gy = 256 cap, 18 rows per lane
    (16, 56, 64),       # layer1 conv1 / conv2
    (16, 56, 128),      # layer2 conv1 (gx = 2)
    (16, 28, 128),      # layer2 conv2
    (16, 14, 256),      # layer3 conv2 (gx = 4)
    (16, 7, 256),       # layer4 conv2
    (32, 14, 1024),     # gx = 16: gy at the 2048 / gx = 128 cap
    (4, 28, 72),        # a partial channel block (9 chunks: one full workgroup of 8, one with a single active chunk)
]


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,H,C', BN_GELU_SHAPES)
def test_bn_gelu_real_shapes(dt, B, H, C):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C)
    M = B * H * H
    x = q(_rand((M, C), g, 1.5, 0.3), dt)
    x[:, 3] = 0.75                                            # zero-variance channel: every sample equal
    dy = q(_rand((M, C), g), dt)
    w = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    b = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    # reference: BatchNorm (batch statistics) written out, exact-erf GELU, autograd
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    mean = xr.mean(0)
    var = ((xr - mean) ** 2).mean(0)
    rstd = (var + EPS).rsqrt()
    y = F.gelu((xr - mean) * rstd * wr + br)
    y.backward(dy)
    m64, r64 = mean.detach(), rstd.detach()
    assert float(var.detach()[3]) == 0.0
    sc, sh = w * r64, b - m64 * w * r64
    print(f'\n[bn_gelu {dt}] B={B} {H}x{H} C={C}: rows {M}, n8 {M * C // 8}, reduce grid {_red_grid(M, C)}')
    if (B, H, C) == (12, 112, 64):
        assert M * C // 8 > GRID_ITEMS and _red_grid(M, C)[1] == 256 and M > 256 * 32 * 16
    if C == 1024:
        assert _red_grid(M, C) == (16, 128) and (M + 31) // 32 > 128
    p = _plan()
    xg, dyg = dev(x, dt), dev(dy, dt)
    yg = torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.bn_gelu_fwd(xg, f32(sc), f32(sh), yg, M, C, _ga(dt))
    check('y', yg, y.detach(), OUT_GATE[dt])
    s1, s2 = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    args = (dyg, xg, f32(sc), f32(sh), f32(m64), f32(r64))
    p.bn_gelu_bwd_reduce(*args, s1, s2, M, C, _ga(dt))
    check('s1 = dbias', s1, br.grad, RED_GATE[dt])
    check('s2 = dweight', s2, wr.grad, RED_GATE[dt])
    dx = torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.bn_gelu_bwd_apply(*args, f32(w), s1, s2, M, dx, M, C, _ga(dt))
    # fp32: dx = w rstd (g - s1 / n - xhat s2 / n) carries the error of the two fp32 reductions (measured 1.5e-5 .. 2.7e-5 at
    # 784 .. 50,176 rows), so it takes the reduction gate; bf16: the rounding of the stored output dominates
    check('dx', dx, xr.grad, OUT_GATE[dt] if dt == 'bf16' else RED_GATE[dt])
    a1, a2 = torch.empty_like(s1), torch.empty_like(s2)
    p.bn_gelu_bwd_reduce(*args, a1, a2, M, C, _ga(dt))
    torch.cuda.synchronize()
    assert torch.equal(a1, s1) and torch.equal(a2, s2), 'bn_gelu_bwd_reduce is not bitwise repeatable'


def test_bn_gelu_bwd_reduce_refuses_a_short_workspace():
    L, lib = _lib()
    M, C = 16 * 56 * 56, 128
    need = int(lib.ga_bn_gelu_bwd_workspace(M, C))
    assert need == 2 * _red_grid(M, C)[1] * C * 4
    x = torch.zeros(M, C, device='cuda')
    vec = torch.ones(C, device='cuda')
    s1, s2 = torch.full((C,), 7.0, device='cuda'), torch.full((C,), 7.0, device='cuda')
    ws = torch.full((need // 4,), 5.0, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    ptr = [x.data_ptr(), x.data_ptr()] + [vec.data_ptr()] * 4 + [s1.data_ptr(), s2.data_ptr()]
    for short in (need - 4, need // 2, 0):
        assert lib.ga_bn_gelu_bwd_reduce(*ptr, M, C, L.GA_F32, ws.data_ptr(), short, s) == GA_ERR_BAD_ARG
    assert lib.ga_bn_gelu_bwd_reduce(*ptr, M, C, L.GA_F32, None, need, s) == GA_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((s1 == 7).all()) and bool((s2 == 7).all()) and bool((ws == 5).all())
    assert lib.ga_bn_gelu_bwd_reduce(*ptr, M, C, L.GA_F32, ws.data_ptr(), need, s) == GA_OK
    torch.cuda.synchronize()
    assert bool((s1 == 0).all()) and bool((s2 == 0).all())          # dy = 0


# ---------------------------------------------------------------------------------------------------------------------------
# max pool 3 x 3 / 2, pad 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,H,C', [(44, 112, 64), (4, 57, 64)])
def test_maxpool_real_shapes(dt, B, H, C):
    """B = 44 at 112 -> 56: the forward counts OUTPUT items (44 x 56 x 56 x 8 = 1,103,872), so it makes a second grid-stride pass;
    odd H = 57 -> 29: the last window row / column is clipped.  Continuous values (no ties), so the gradient is a gather."""
    g = torch.Generator().manual_seed(H + B)
    x = torch.randn(B, C, H, H, generator=g).to(DT[dt]).float()
    Ho = (H - 1) // 2 + 1
    if H == 112:
        assert B * Ho * Ho * C // 8 > GRID_ITEMS
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)        # max is exact in any precision: an fp32 reference
    dy = torch.randn(y.shape, generator=g).to(DT[dt]).float()
    y.backward(dy)
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    p = _plan()
    yg = torch.empty(B * Ho * Ho, C, dtype=DT[dt], device='cuda')
    idx = torch.empty(B * Ho * Ho, C, dtype=torch.uint8, device='cuda')
    p.maxpool3s2_fwd(dev(to_nhwc(x), dt), yg, idx, B, H, H, C, _ga(dt))
    assert torch.equal(yg.float().cpu(), to_nhwc(y.detach())), 'max pool forward is not exact'
    dx = torch.empty(B * H * H, C, dtype=DT[dt], device='cuda')
    p.maxpool3s2_bwd(dev(to_nhwc(dy), dt), idx, dx, B, H, H, C, _ga(dt))
    print(f'\n[maxpool {dt}] B={B} {H}->{Ho} C={C}')
    check('dx', dx, to_nhwc(xr.grad), OUT_GATE[dt])
    dx2 = torch.empty_like(dx)
    p.maxpool3s2_bwd(dev(to_nhwc(dy), dt), idx, dx2, B, H, H, C, _ga(dt))
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)


# ---------------------------------------------------------------------------------------------------------------------------
# SE unit with BatchNorm over the batch
# ---------------------------------------------------------------------------------------------------------------------------
def _se_case(B, C, R, HW, seed, rowscale=True):
    """inputs of ga_se_bn_fwd / _bwd as float64 CPU tensors; W1 row 0 is zero, so hidden unit 0 has zero batch variance"""
    g = torch.Generator().manual_seed(seed)
    d = dict(B=B, C=C, R=R, HW=HW)
    d['S'] = _rand((B, C), g, 1.0, 0.2) * HW                  # per-sample spatial sums of the raw conv3 output
    d['scale3'] = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    d['shift3'] = _rand(C, g, 0.3)
    d['W1'] = _rand((R, C), g, C ** -0.5)
    d['W1'][0] = 0.0
    d['g1'] = torch.rand(R, generator=g, dtype=torch.float64) + 0.5
    d['b1'] = _rand(R, g, 0.3)
    d['W2'] = _rand((C, R), g, R ** -0.5)
    d['b2'] = _rand(C, g, 0.3)
    d['rmean'] = _rand(R, g, 0.2)
    d['rvar'] = torch.rand(R, generator=g, dtype=torch.float64) + 0.5
    d['P1'] = _rand((B, C), g, HW ** 0.5)
    d['P2'] = _rand((B, C), g, HW ** 0.5)
    d['g3'] = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    d['b3'] = _rand(C, g, 0.3)
    d['mean3'] = _rand(C, g, 0.2)
    d['rstd3'] = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    r = torch.ones(B, dtype=torch.float64)
    if rowscale:
        r = (torch.rand(B, generator=g) < 0.75).double() / 0.75  # DropPath rows: r = 0 or 1 / keep
        r[0], r[-1] = 0.0, 1.0 / 0.75
    d['r'] = r if rowscale else None
    d['dW1_0'], d['dg1_0'], d['db1_0'] = _rand((R, C), g), _rand(R, g), _rand(R, g)      # the gradients accumulate (+=)
    d['dW2_0'], d['db2_0'] = _rand((C, R), g), _rand(C, g)
    for k, v in list(d.items()):                               # everything the kernel reads is fp32: round it here
        if isinstance(v, torch.Tensor):
            d[k] = v.float().double()
    return d


def _se_ref(d, training):
    B, HW = d['B'], d['HW']
    p = (d['scale3'] * d['S'] / HW + d['shift3']).requires_grad_(True)      # pooled BatchNorm-3 output
    prm = {k: d[k].clone().requires_grad_(True) for k in ('W1', 'g1', 'b1', 'W2', 'b2')}
    hpre = p @ prm['W1'].t()
    hpre.retain_grad()
    if training:
        mu = hpre.mean(0)
        var = ((hpre - mu) ** 2).mean(0)
    else:
        mu, var = d['rmean'], d['rvar']
    rstd = (var + EPS).rsqrt()
    h = F.gelu((hpre - mu) * rstd * prm['g1'] + prm['b1'])
    z = h @ prm['W2'].t() + prm['b2']
    z.retain_grad()
    gate = torch.sigmoid(z)
    out = dict(hpre=hpre.detach(), mean=mu.detach(), rstd=rstd.detach(), h=h.detach(), gate=gate.detach())
    if training:
        out['rmean'] = 0.9 * d['rmean'] + 0.1 * mu.detach()
        out['rvar'] = 0.9 * d['rvar'] + 0.1 * var.detach() * B / (B - 1)
        r = d['r'] if d['r'] is not None else torch.ones(B, dtype=torch.float64)
        dgate = r[:, None] * (d['g3'] * d['P2'] + d['b3'] * d['P1'])       # the tail's gradient of the gate
        (gate * dgate).sum().backward()
        ds = p.grad
        gr = gate.detach() * r[:, None]
        sx = d['rstd3'] * (d['S'] - HW * d['mean3'])                        # sum_hw xhat3
        out.update(dz=z.grad, dhpre=hpre.grad, ds=ds, s1=(gr * d['P1'] + ds).sum(0), s2=(gr * d['P2'] + ds / HW * sx).sum(0),
                   dW1=prm['W1'].grad, dg1=prm['g1'].grad, db1=prm['b1'].grad, dW2=prm['W2'].grad, db2=prm['b2'].grad)
    return out


def _se_run(d, training, ref=None):
    """ga_se_bn_fwd (+ ga_se_bn_bwd in train mode) on the GPU; returns the outputs as CUDA tensors"""
    B, C, R, HW = d['B'], d['C'], d['R'], d['HW']
    p = _plan()
    o = {k: torch.empty(B, R, device='cuda') for k in ('hpre', 'h')}
    o.update(mean=torch.empty(R, device='cuda'), rstd=torch.empty(R, device='cuda'), gate=torch.empty(B, C, device='cuda'),
             rmean=f32(d['rmean']), rvar=f32(d['rvar']))
    i = {k: f32(d[k]) for k in ('S', 'scale3', 'shift3', 'W1', 'g1', 'b1', 'W2', 'b2', 'P1', 'P2', 'g3', 'b3', 'mean3', 'rstd3')}
    p.se_bn_fwd(i['S'], HW, i['scale3'], i['shift3'], i['W1'], i['g1'], i['b1'], o['rmean'], o['rvar'], i['W2'], i['b2'], o['hpre'],
                o['mean'], o['rstd'], o['h'], o['gate'], B, C, R, training)
    if not training:
        return o
    o.update(dz=torch.empty(B, C, device='cuda'), dhpre=torch.empty(B, R, device='cuda'), ds=torch.empty(B, C, device='cuda'),
             s1=torch.empty(C, device='cuda'), s2=torch.empty(C, device='cuda'))
    for k in ('dW1', 'dg1', 'db1', 'dW2', 'db2'):
        o[k] = f32(d[k + '_0'])
    rs = f32(d['r']) if d['r'] is not None else None
    p.se_bn_bwd(i['P1'], i['P2'], rs, i['g3'], i['b3'], i['mean3'], i['rstd3'], i['S'], HW, i['scale3'], i['shift3'], i['W1'], i['g1'],
                i['b1'], i['W2'], o['hpre'], o['mean'], o['rstd'], o['h'], o['gate'], o['dz'], o['dhpre'], o['ds'], o['s1'], o['s2'],
                o['dW1'], o['dg1'], o['db1'], o['dW2'], o['db2'], B, C, R)
    return o


SE_SHAPES = [
    (256, 256, 16, 3136),      # layer1: 64 sample rows per wave, se_bwd2's channel loop once, 32 batch blocks
    (256, 512, 32, 784),       # layer2: 2 channel blocks, the channel loop twice
    (256, 1024, 64, 196),      # layer3: 4 channel blocks, 4 passes
    (256, 1024, 64, 49),       # layer4
    (2, 64, 4, 49),            # the train-mode minimum
    (9, 256, 16, 196),         # an 8-row batch block plus a 1-row tail
    (1024, 2048, 128, 49),     # every se_check limit at once: hp[kSeMaxB] full, hs[8][kSeMaxR] full, 8 channel blocks
    (24, 264, 16, 196),        # a channel-block tail (264 = 256 + 8)
]


@pytest.mark.parametrize('B,C,R,HW', SE_SHAPES)
def test_se_bn_real_shapes(B, C, R, HW):
    d = _se_case(B, C, R, HW, seed=B + C + R)
    ref = _se_ref(d, True)
    o = _se_run(d, True)
    print(f'\n[se_bn train] B={B} C={C} R={R} HW={HW}: se_fwd2 / se_bwd3 grid ({(C + 255) // 256}, {(B + 7) // 8})')
    assert float(ref['rstd'][0]) == pytest.approx(EPS ** -0.5)          # hidden unit 0: zero batch variance
    for k in ('hpre', 'h', 'gate'):
        check(k, o[k], ref[k], OUT_GATE['fp32'])
    check('mean', o['mean'], ref['mean'], RED_GATE['fp32'])
    check('rstd', o['rstd'], ref['rstd'], RED_GATE['fp32'])
    check('running_mean', o['rmean'], ref['rmean'], STAT_GATE)
    check('running_var', o['rvar'], ref['rvar'], STAT_GATE)
    for k in ('dz', 'dhpre', 's1', 's2'):
        check(k, o[k], ref[k], RED_GATE['fp32'])
    if B == 2:
        # two samples: xhat = +-1 and the BatchNorm backward of every unit with nonzero variance is exactly zero, and unit 0 (zero
        # variance) meets the zero row of W1 -- ds = dhpre W1 is zero; measured against the size of its terms
        e = float(o['ds'].abs().max()) / float(ref['dhpre'].abs().max() * d['W1'].abs().sum(0).max())
        print(f'  {"ds (analytically zero)":<44s} {e:.2e}  (gate {RED_GATE["fp32"]:.0e})')
        assert e <= RED_GATE['fp32']
    else:
        check('ds', o['ds'], ref['ds'], RED_GATE['fp32'])
    for k in ('dW1', 'dg1', 'db1', 'dW2', 'db2'):
        check(k + ' (+= onto a nonzero gradient)', o[k] - f32(d[k + '_0']), ref[k], RED_GATE['fp32'])
    o2 = _se_run(d, True)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert torch.equal(v, o2[k]), f'{k} differs between two identical launches'


@pytest.mark.parametrize('B,C,R', [(1, 256, 16), (256, 1024, 64)])
def test_se_bn_eval(B, C, R):
    """eval: the running statistics normalise (B = 1 is allowed) and are left untouched"""
    d = _se_case(B, C, R, 49, seed=3 * B + C, rowscale=False)
    ref = _se_ref(d, False)
    o = _se_run(d, False)
    print(f'\n[se_bn eval] B={B} C={C} R={R}')
    for k in ('hpre', 'h', 'gate', 'mean', 'rstd'):
        check(k, o[k], ref[k], OUT_GATE['fp32'])
    torch.cuda.synchronize()
    assert torch.equal(o['rmean'], f32(d['rmean'])) and torch.equal(o['rvar'], f32(d['rvar']))


@pytest.mark.parametrize('B,C,R,training', [(1025, 64, 4, 1), (4, 2056, 16, 1), (4, 256, 129, 1), (1, 256, 16, 1),
                                            (1025, 64, 4, 0), (4, 2056, 16, 0), (4, 256, 129, 0), (0, 256, 16, 0)])
def test_se_check_refuses_and_writes_nothing(B, C, R, training):
    L, lib = _lib()
    n = max(B, 1) * max(C, R) * 2
    buf = torch.full((30, n), 3.0, device='cuda')
    ptr = [buf[k].data_ptr() for k in range(30)]
    s = torch.cuda.current_stream().cuda_stream
    assert lib.ga_se_bn_fwd(ptr[0], 49, *ptr[1:15], B, C, R, training, s) == GA_ERR_UNSUPPORTED
    if training:
        assert lib.ga_se_bn_bwd(*ptr[:8], 49, *ptr[8:29], B, C, R, s) == GA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((buf == 3.0).all()), 'a refused SE call wrote to its buffers'


# ---------------------------------------------------------------------------------------------------------------------------
# SE-scale + DropPath + residual + ReLU tail and its two backward passes
# ---------------------------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(16, 3136, 256), (16, 784, 512), (16, 196, 1024), (256, 49, 1024)]


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('extras', [False, True], ids=['plain', 'rowscale+dsbn'])
@pytest.mark.parametrize('B,HW,C', TAIL_SHAPES)
def test_se_residual_real_shapes(dt, extras, B, HW, C):
    """y = relu(res' + r gate bn3(x3)), res' = bn_d(res) with extras; backward pass A (dm, P1, P2) and pass B (dx3) against autograd
    through BN-3 with batch statistics, given the gradient ds of the pooled BN-3 output as the SE backward hands it over"""
    g = torch.Generator().manual_seed(HW + C + int(extras))
    M = B * HW
    n8 = M * C // 8
    print(f'\n[se_residual {dt} {"rowscale+dsbn" if extras else "plain"}] B={B} HW={HW} C={C}: n8 {n8}, pass A grid ({C // 64}, {B})')
    assert C // 64 > 1
    if HW == 3136:
        assert n8 > GRID_ITEMS
    x3 = q(_rand((B, HW, C), g, 1.0, 0.2), dt)
    res = q(_rand((B, HW, C), g), dt)
    dy = q(_rand((B, HW, C), g), dt)
    gate = torch.rand(B, C, generator=g, dtype=torch.float64).float().double()
    ds = _rand((B, C), g).float().double()
    g3 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    b3 = _rand(C, g, 0.3).float().double()
    mean3 = x3.mean((0, 1))
    rstd3 = (((x3 - mean3) ** 2).mean((0, 1)) + EPS).rsqrt()
    sc3, sh3 = (g3 * rstd3).float().double(), (b3 - mean3 * g3 * rstd3).float().double()
    r = torch.ones(B, dtype=torch.float64)
    rsc = rsh = None
    if extras:
        r = (torch.rand(B, generator=g) < 0.75).double() / 0.75
        r[0], r[-1] = 0.0, 1.0 / 0.75                                    # a dropped row and a kept one, whatever the draw
        md = res.mean((0, 1))
        scd = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * (((res - md) ** 2).mean((0, 1)) + EPS).rsqrt()
        rsc, rsh = scd.float().double(), (_rand(C, g, 0.3) - md * scd).float().double()
    # forward on the GPU first: the backward reference takes the kernel's ReLU mask (y > 0), as pass A does -- an fp64 y and an fp32 y
    # can disagree on the sign of values within an ulp of zero
    p = _plan()
    x3g, resg, dyg = dev(x3.view(M, C), dt), dev(res.view(M, C), dt), dev(dy.view(M, C), dt)
    rg = f32(r) if extras else None
    yg = torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.se_residual_fwd(x3g, f32(sc3), f32(sh3), f32(gate), rg, resg, f32(rsc) if extras else None, f32(rsh) if extras else None, yg, B, HW,
                      C, _ga(dt))
    resp = res * rsc + rsh if extras else res
    y_ref = torch.relu(resp + r[:, None, None] * gate[:, None, :] * (x3 * sc3 + sh3))
    check('y', yg, y_ref.view(M, C), OUT_GATE[dt])
    mask = (yg.cpu().view(B, HW, C) > 0).double()
    x3r = x3.clone().requires_grad_(True)
    mu = x3r.mean((0, 1))
    rstd = (((x3r - mu) ** 2).mean((0, 1)) + EPS).rsqrt()
    u = (x3r - mu) * rstd * g3 + b3
    u.retain_grad()
    ylin = resp + r[:, None, None] * gate[:, None, :] * u
    ylin.retain_grad()
    ((ylin * mask * dy).sum() + (u.mean(1) * ds).sum()).backward()
    dm_ref, du = ylin.grad, u.grad
    xh = (x3 - mean3) * rstd3
    P1_ref, P2_ref = dm_ref.sum(1), (dm_ref * xh).sum(1)
    s1, s2 = du.sum((0, 1)), (du * xh).sum((0, 1))
    dm = torch.empty(M, C, dtype=DT[dt], device='cuda')
    P1, P2 = torch.empty(B, C, device='cuda'), torch.empty(B, C, device='cuda')
    p.se_residual_bwd_a(dyg, yg, x3g, f32(mean3), f32(rstd3), dm, P1, P2, B, HW, C, _ga(dt))
    assert torch.equal(dm.double().cpu(), dm_ref.view(M, C)), 'dm = dy * (y > 0) is exact'
    check('P1', P1, P1_ref, RED_GATE[dt])
    check('P2', P2, P2_ref, RED_GATE[dt])
    dx3 = torch.empty(M, C, dtype=DT[dt], device='cuda')
    p.se_residual_bwd_b(dm, x3g, f32(mean3), f32(rstd3), f32(g3), f32(gate), rg, f32(ds), f32(s1), f32(s2), dx3, B, HW, C, _ga(dt))
    check('dx3', dx3, x3r.grad.view(M, C), OUT_GATE[dt])
    dmb, Q1, Q2 = torch.empty_like(dm), torch.empty_like(P1), torch.empty_like(P2)
    p.se_residual_bwd_a(dyg, yg, x3g, f32(mean3), f32(rstd3), dmb, Q1, Q2, B, HW, C, _ga(dt))
    torch.cuda.synchronize()
    assert torch.equal(dm, dmb) and torch.equal(P1, Q1) and torch.equal(P2, Q2), 'pass A is not bitwise repeatable'


# ---------------------------------------------------------------------------------------------------------------------------
# stride-2 subsample and its transpose
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,H,C', [(16, 56, 256), (16, 28, 512), (16, 14, 1024), (4, 15, 64)])
def test_subsample_real_shapes(dt, B, H, C):
    """the downsample inputs of layer2..4 (the backward counts input items: 16 x 56 x 56 x 256 / 8 > 1,048,576); odd H = 15"""
    g = torch.Generator().manual_seed(H * C)
    Ho = (H - 1) // 2 + 1
    if H == 56:
        assert B * H * H * C // 8 > GRID_ITEMS
    x = torch.randn(B, H, H, C, generator=g).to(DT[dt])
    p = _plan()
    ys = torch.empty(B * Ho * Ho, C, dtype=DT[dt], device='cuda')
    p.subsample2_fwd(x.cuda(), ys, B, H, H, C, _ga(dt))
    assert torch.equal(ys.cpu(), x[:, ::2, ::2].reshape(-1, C))
    dy = torch.randn(B, Ho, Ho, C, generator=g).to(DT[dt])
    base = torch.randn(B, H, H, C, generator=g).to(DT[dt])
    ref = torch.zeros(B, H, H, C, dtype=DT[dt])
    ref[:, ::2, ::2] = dy
    dx = base.cuda()
    p.subsample2_bwd(dy.cuda(), dx, B, H, H, C, _ga(dt))
    assert torch.equal(dx.cpu().view(B, H, H, C), ref)
    dx = base.cuda()
    p.subsample2_bwd(dy.cuda(), dx, B, H, H, C, _ga(dt), accumulate=True)
    acc = base.clone()
    acc[:, ::2, ::2] = (base[:, ::2, ::2].float() + dy.float()).to(DT[dt])      # one rounding of the fp32 sum
    assert torch.equal(dx.cpu().view(B, H, H, C), acc)
