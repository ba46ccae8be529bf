"""GPU: the two weight-gradient forms of ConvNeXt's patchify convolutions behind ga_wgrad --
  * GA_A_PATCH2 operands on the wide TN kernel (gemm_tn2_kernel<true>, knob TN2_PATCH2), the 2 x 2 / stride-2 downsample convs;
  * the direct stem kernel (stem4_wgrad_kernel + stem4_wgrad_reduce, knob STEM4_WGRAD_DIRECT), Conv2d(3, C, 4, 4) on the fp32 image.

Every case computes dW and dbias three times from the same bf16-rounded inputs: (a) in float64 with torch, (b) by the old form
(knob = 0: gemm_tn_kernel, register-staged gather, split-M atomics), (c) by the new form.  Gate, per tensor, on the relative norm
error against (a):    err(new) <= 2 * err(old) + 2^-23.
Both forms add the same bf16 x bf16 products in fp32 and differ in the ORDER only, so the old form's own error is the scale; the
factor 2 covers order effects.  2^-23 (one fp32 epsilon, relative to the tensor's norm) is the floor: a result held in fp32 cannot
be expected closer than that to float64, and without it a tensor the old form happens to hit almost exactly would gate on noise.
Every figure is printed before it is asserted.

The new forms combine per-workgroup partial tiles with a reduce launch in a fixed order, so two runs must give the same bits: that
is asserted for dW wherever the partial path runs, and for dbias of the stem kernel.  The bias gradient of the wide TN kernel is
still added with fp32 atomics (unchanged by this form) and is gated against float64 only.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def _imp():
    from imagenet_models_amd import ops
    return ops


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _gate(name, new, old, ref):
    e_new, e_old = _rel(new, ref), _rel(old, ref)
    print(f'{name}: new {e_new:.3e}  old {e_old:.3e}  bound {2 * e_old + EPS32:.3e}  |ref| {float(ref.norm()):.3e}')
    return e_new, e_old


def _check(errs):
    bad = [(n, en, eo) for n, en, eo in errs if not en <= 2 * eo + EPS32]
    assert not bad, f'new form above 2 x old + 2^-23: {bad}'


def _wants_workspace(ops, *a, **kw):
    p = ops.Plan()
    p.wgrad(*a, **kw)
    return bool(p._ws_req)


# ----------------------------------------------------------------------------------------------------------
# GA_A_PATCH2 on the wide TN kernel
# ----------------------------------------------------------------------------------------------------------
# (B, H, W, C, N, non-zero dW, new form expected (None: eligible but small output -> atomics, no workspace))
PATCH2 = [
    pytest.param(256, 56, 56, 96, 192, False, True, id='stages.1.downsample-B256'),
    pytest.param(256, 28, 28, 192, 384, False, True, id='stages.2.downsample-B256'),
    pytest.param(256, 14, 14, 384, 768, False, True, id='stages.3.downsample-B256-ragged-split'),   # 392 stages in 10 splits of 40: last 32
    pytest.param(1, 56, 56, 96, 192, False, False, id='B1-engine-map-old-dispatch'),                # M = 784 < 8192: stays on the old form
    pytest.param(1, 256, 256, 96, 192, False, True, id='B1-large-map'),                             # one image, 512 stages
    pytest.param(12, 56, 56, 96, 192, False, True, id='B12-ragged-split'),                          # 294 stages in 33 splits of 9: last 6
    pytest.param(80, 12, 40, 24, 40, False, None, id='nonsquare-C24-atomics'),                      # 2C = 48: run boundary inside a 128-column piece
    pytest.param(64, 28, 28, 192, 384, True, True, id='accumulate-nonzero'),
    pytest.param(256, 28, 28, 128, 256, False, True, id='base-stages.1.downsample'),
]


@pytest.mark.parametrize('B,H,W,C,N,nonzero,expect_new', PATCH2)
def test_patch2_wgrad_forms(knobs, B, H, W, C, N, nonzero, expect_new):
    ops = _imp()
    g = torch.Generator(device='cuda').manual_seed(1234 + B + H + C)
    M, K = B * (H // 2) * (W // 2), 4 * C
    X = torch.randn(B, H, W, C, generator=g, device='cuda').bfloat16()
    DY = (torch.randn(M, N, generator=g, device='cuda') * 0.5).bfloat16()
    init = torch.randn(N, K, generator=g, device='cuda') * 3.0 if nonzero else torch.zeros(N, K, device='cuda')
    binit = torch.randn(N, generator=g, device='cuda') if nonzero else torch.zeros(N, device='cuda')
    # (a) float64: row m of the operand = the 2 x 2 patch of output pixel m, k = (ky, kx, c)
    xp = X.double().reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(M, K)
    dy64 = DY.double()
    ref_w = init.double() + dy64.t() @ xp
    ref_b = binit.double() + dy64.sum(0)
    del xp, dy64

    kw = dict(x_kind=ops.A_PATCH2, x_dims=(H, W, C))

    def run(flag):
        knobs(TN2_PATCH2=flag)
        dW, db = init.clone(), binit.clone()
        ops.Plan(eager=True).wgrad(DY, X, dW, M, N, K, ops.GA_BF16, dbias=db, **kw)
        torch.cuda.synchronize()
        return dW, db

    old_w, old_b = run(0)
    new_w, new_b = run(1)
    new_w2, _ = run(1)
    if expect_new is not None:
        assert _wants_workspace(ops, DY, X, init.clone(), M, N, K, ops.GA_BF16, dbias=binit.clone(), **kw) == expect_new, 'dispatch'
    errs = [('dW',) + _gate('patch2 dW', new_w, old_w, ref_w), ('dbias',) + _gate('patch2 dbias', new_b, old_b, ref_b)]
    _check(errs)
    if expect_new:
        assert torch.equal(new_w, new_w2), 'two runs of the partial-tile path differ'


# ----------------------------------------------------------------------------------------------------------
# direct stem kernel
# ----------------------------------------------------------------------------------------------------------
STEM = [
    pytest.param(256, 224, 224, 96, False, id='stem-B256'),              # 6272 pixel tiles over 512 workgroups
    pytest.param(1, 224, 224, 96, False, id='stem-B1-ragged-tile'),      # 3136 pixels = 24.5 tiles
    pytest.param(64, 224, 224, 128, False, id='stem-base-C128'),
    pytest.param(3, 36, 52, 96, False, id='stem-small-nonsquare'),       # 351 pixels: fewer tiles than workgroups, ragged, rows of 13
    pytest.param(32, 224, 224, 96, True, id='stem-accumulate-nonzero'),
    pytest.param(16, 224, 224, 128, True, id='stem-C128-accumulate-nonzero'),
]


@pytest.mark.parametrize('B,H,W,N,nonzero', STEM)
def test_stem_wgrad_forms(knobs, B, H, W, N, nonzero):
    ops = _imp()
    g = torch.Generator(device='cuda').manual_seed(4321 + B + H + N)
    M = B * (H // 4) * (W // 4)
    X = torch.randn(B, 3, H, W, generator=g, device='cuda')                       # fp32 NCHW image, rounded to bf16 by both forms
    DY = (torch.randn(M, N, generator=g, device='cuda') * 0.5).bfloat16()
    init = torch.randn(N, 48, generator=g, device='cuda') * 3.0 if nonzero else torch.zeros(N, 48, device='cuda')
    binit = torch.randn(N, generator=g, device='cuda') if nonzero else torch.zeros(N, device='cuda')
    xp = X.bfloat16().double().reshape(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(M, 48)   # k = (c, ky, kx)
    dy64 = DY.double()
    ref_w = init.double() + dy64.t() @ xp
    ref_b = binit.double() + dy64.sum(0)
    del xp, dy64
    kw = dict(x_kind=ops.A_STEM4_NCHW, x_dims=(H, W, 3))

    def run(flag):
        knobs(STEM4_WGRAD_DIRECT=flag)
        dW, db = init.clone(), binit.clone()
        ops.Plan(eager=True).wgrad(DY, X, dW, M, N, 48, ops.GA_BF16, dbias=db, **kw)
        torch.cuda.synchronize()
        return dW, db

    old_w, old_b = run(0)
    new_w, new_b = run(1)
    new_w2, new_b2 = run(1)
    assert _wants_workspace(ops, DY, X, init.clone(), M, N, 48, ops.GA_BF16, dbias=binit.clone(), **kw), 'dispatch'
    errs = [('dW',) + _gate('stem dW', new_w, old_w, ref_w), ('dbias',) + _gate('stem dbias', new_b, old_b, ref_b)]
    _check(errs)
    assert torch.equal(new_w, new_w2) and torch.equal(new_b, new_b2), 'two runs of the direct stem form differ'


def test_stem_wgrad_without_bias(knobs):
    """dbias = None: the column sums are not formed and nothing but dW is written"""
    ops = _imp()
    g = torch.Generator(device='cuda').manual_seed(7)
    B, H, W, N = 8, 64, 64, 96
    M = B * (H // 4) * (W // 4)
    X = torch.randn(B, 3, H, W, generator=g, device='cuda')
    DY = torch.randn(M, N, generator=g, device='cuda').bfloat16()
    xp = X.bfloat16().double().reshape(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(M, 48)
    ref = DY.double().t() @ xp
    out = {}
    for flag in (0, 1):
        knobs(STEM4_WGRAD_DIRECT=flag)
        dW = torch.zeros(N, 48, device='cuda')
        ops.Plan(eager=True).wgrad(DY, X, dW, M, N, 48, ops.GA_BF16, x_kind=ops.A_STEM4_NCHW, x_dims=(H, W, 3))
        torch.cuda.synchronize()
        out[flag] = dW
    _check([('dW',) + _gate('stem dW (no bias)', out[1], out[0], ref)])
