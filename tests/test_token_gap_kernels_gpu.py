"""ga_token_gap_fwd / ga_token_gap_bwd (csrc/pit.hip: the global average pool over the tokens of the plain PiT head and its backward)
against float64 on the CPU, through the C ABI, in fp32 and bf16.

Gates follow rounding (u = 2^-24 for fp32, 2^-8 for bf16, the unit roundoffs of the two formats):
  forward   |y - ref| <= (N + 2) * 2^-24 * max_n |x[b, n, c]|  per output: N - 1 fp32 additions of partial sums bounded by N * max|x|,
            the rounding of 1/N and of the product with it; bf16 adds the rounding of the stored value, 2^-8 * |ref|
  backward  |dx - dy/N| <= u * |dy/N|: one rounding of the exact quotient in the output dtype (for bf16 the fp32 quotient is rounded
            once more by the store; the second rounding moves the result by at most 2^-24 |q|, which a bound that is only reached at
            the bottom of a binade, where the bf16 value is exact, still covers)
Each test prints the worst ratio to its gate and runs the kernel twice: the results must be bitwise equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, N, C): the model's shape; a short row on the vector path of both dtypes; C = 20 (no multiple of 8: the bf16 one-element path,
# N = 5 a non-power-of-two reduction); N = 1 (identity); more samples than rows of a wave; and more columns than one pass of the
# capped grid covers (2048 workgroups x 64 columns), so that the grid-stride loop runs more than once in both dtypes
SHAPES = [(3, 49, 576), (2, 9, 40), (2, 5, 20), (1, 1, 8), (257, 4, 8), (2048 * 64 + 1, 4, 8)]
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}


def _ops():
    from imagenet_models_amd import ops
    return ops


def _scaled(shape, dt, seed):
    """random values stored in dt; sample 0 scaled by 1e3, the last sample (when there is a second one) by 1e-3"""
    v = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    v[0] *= 1e3
    if shape[0] > 1:
        v[-1] *= 1e-3
    return v.to(dt)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,N,C', SHAPES)
def test_token_gap_fwd(dt, B, N, C):
    ops = _ops()
    x = _scaled((B, N, C), dt, seed=N * 1000 + C)
    xd = x.cuda()
    ys = []
    for _ in range(2):
        y = torch.full((B, C), float('nan'), dtype=dt, device='cuda')
        ops.Plan(eager=True).token_gap_fwd(xd, y, B, N, C, ops.ga_dtype(dt))
        torch.cuda.synchronize()
        ys.append(y.cpu())
    assert torch.equal(ys[0].view(torch.uint8), ys[1].view(torch.uint8)), 'the forward does not repeat bitwise'
    x64 = x.double()
    ref = x64.mean(1)
    gate = (N + 2) * 2.0 ** -24 * x64.abs().amax(1)
    if dt == torch.bfloat16:
        gate = gate + 2.0 ** -8 * ref.abs()
    diff = (ys[0].double() - ref).abs()
    assert torch.isfinite(ys[0].float()).all()
    ratio = float((diff / gate.clamp_min(1e-300)).max())
    print(f'[token_gap_fwd {B}x{N}x{C} {dt}] worst |y - ref| / gate = {ratio:.3f}')
    assert bool((diff <= gate).all()), ratio
    if N == 1:
        assert torch.equal(ys[0].view(torch.uint8), x[:, 0].contiguous().view(torch.uint8)), 'N = 1 is the identity'


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,N,C', SHAPES)
def test_token_gap_bwd(dt, B, N, C):
    ops = _ops()
    dy = _scaled((B, C), dt, seed=N * 1000 + C + 1)
    dyd = dy.cuda()
    outs = []
    for _ in range(2):
        dx = torch.full((B, N, C), float('nan'), dtype=dt, device='cuda')
        ops.Plan(eager=True).token_gap_bwd(dyd, dx, B, N, C, ops.ga_dtype(dt))
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)), 'the backward does not repeat bitwise'
    q = (dy.double() / N)[:, None, :].expand(B, N, C)
    gate = U[dt] * q.abs()
    diff = (outs[0].double() - q).abs()
    assert torch.isfinite(outs[0].float()).all()
    ratio = float((diff / gate.clamp_min(1e-300)).max())
    print(f'[token_gap_bwd {B}x{N}x{C} {dt}] worst |dx - dy/N| / gate = {ratio:.3f}')
    assert bool((diff <= gate).all()), ratio
    assert torch.equal(outs[0][:, :1].expand(B, N, C).contiguous().view(torch.uint8), outs[0].view(torch.uint8)), 'rows of a sample differ'


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_pointers_off_the_16_byte_grid_take_the_one_element_path(dt):
    """C = 8 allows 16-byte pieces, but an x or dx that starts one element into its allocation does not: same results, no fault"""
    ops = _ops()
    B, N, C = 3, 7, 8
    x = _scaled((B, N, C), dt, seed=11)
    raw = torch.zeros(B * N * C + 1, dtype=dt, device='cuda')
    raw[1:].copy_(x.reshape(-1))
    y, y0 = torch.empty(B, C, dtype=dt, device='cuda'), torch.empty(B, C, dtype=dt, device='cuda')
    p = ops.Plan(eager=True)
    p.token_gap_fwd(raw[1:], y, B, N, C, ops.ga_dtype(dt))
    p.token_gap_fwd(x.cuda(), y0, B, N, C, ops.ga_dtype(dt))
    draw = torch.zeros(B * N * C + 1, dtype=dt, device='cuda')
    dx0 = torch.empty(B, N, C, dtype=dt, device='cuda')
    p.token_gap_bwd(y0, draw[1:], B, N, C, ops.ga_dtype(dt))
    p.token_gap_bwd(y0, dx0, B, N, C, ops.ga_dtype(dt))
    torch.cuda.synchronize()
    x64 = x.double()
    gate = (N + 2) * 2.0 ** -24 * x64.abs().amax(1) + (2.0 ** -8 * x64.mean(1).abs() if dt == torch.bfloat16 else 0)
    assert bool(((y.cpu().double() - x64.mean(1)).abs() <= gate).all())
    assert torch.equal(draw[1:].view(B, N, C).cpu().view(torch.uint8), dx0.cpu().view(torch.uint8)) and float(draw[0]) == 0.0
