"""fc1 weight gradient accumulated inside the fused MLP backward (ga_mlp_bwd with dW1 / db1, csrc/mlp.hip; C = 96).

Kernel level: the persistent tile walk (automatic grid, 3 workgroups over 8 tiles with a partial last one, ONE workgroup over 22
tiles) against the fp64 product of the kernel's OWN operands -- the DH it stores and X -- within 2e-4 of the reference's max
magnitude: the bound test_wgrad_wide_tile_bf16 applies to a bf16 weight gradient with fp32 accumulation against the same kind of
reference.  dW1 / db1 are pre-filled with 0.5 (they are accumulated into).  A / DH / DX keep the 2e-2 checks of test_mlp_bwd;
a second launch that stores neither A nor DH gives the same bits (fixed reduction order).  C = 192 with dW1 is refused.

Engine level: one train step with GAEXT_MLP_WG1=0 (mlp_bwd + the wg1 launch) and one with =1, same seed: the stage-0 fc1 and norm
gradients differ by fp32 summation order only (2e-4 of max)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

C, H = 96, 384
FILL = 0.5


def _ops():
    from imagenet_models_amd import ops
    return ops


def gelu_tanh(x):
    return torch.nn.functional.gelu(x, approximate='tanh')


def close(got, ref, tol, what):
    err = float((got.double().cpu() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-12))
    print(f'{what}: {err:.3e} (bound {tol:g})')
    assert err < tol, (what, err)
    return err


def _operands(M):
    """the seeded bf16 operands and fp32 references of test_mlp_bwd"""
    g = torch.Generator().manual_seed(7 * C + M)
    bf = lambda t: t.to(torch.bfloat16)
    X, DY = bf(torch.randn(M, C, generator=g)), bf(torch.randn(M, C, generator=g))
    W1, W2 = bf(torch.randn(H, C, generator=g) * C ** -0.5), bf(torch.randn(C, H, generator=g) * H ** -0.5)
    b1 = torch.randn(H, generator=g) * 0.1
    pre = (X.float() @ W1.float().T + b1).requires_grad_(True)
    a = gelu_tanh(pre)
    a.backward(DY.float() @ W2.float())
    dh = bf(pre.grad).float()
    return dict(X=X, DY=DY, W1=W1, W2=W2, b1=b1, a=a.detach(), dh=dh, dx=dh @ W1.float())


def _launch(o, M, max_blocks, store):
    ops = _ops()
    A = torch.empty(M, H, dtype=torch.bfloat16, device='cuda') if store else None
    DH = torch.empty(M, H, dtype=torch.bfloat16, device='cuda') if store else None
    DX = torch.empty(M, C, dtype=torch.bfloat16, device='cuda')
    dW1 = torch.full((H, C), FILL, device='cuda')
    db1 = torch.full((H,), FILL, device='cuda')
    nbytes = ops.mlp_bwd_partials(M, C, ops.GA_BF16, max_blocks)
    tiles = (M + 127) // 128
    assert nbytes % (4 * (H * C + H)) == 0 and 1 <= nbytes // (4 * (H * C + H)) <= (max_blocks or tiles)
    part = torch.full((nbytes // 4,), float('nan'), device='cuda')       # stale partials must not leak into the sums
    ops.Plan(eager=True).mlp_bwd(o['X'].cuda(), o['DY'].cuda(), o['W1'].cuda(), o['b1'].cuda(), o['W2'].T.contiguous().cuda(),
                                 o['W1'].T.contiguous().cuda(), A, DH, DX, M, C, ops.GA_BF16, dW1=dW1, db1=db1, partials=part,
                                 max_blocks=max_blocks)
    torch.cuda.synchronize()
    return A, DH, DX, dW1, db1


@pytest.mark.parametrize('M,max_blocks', [(256, 0),                  # two tiles, automatic grid
                                          (128 * 7 + 5, 3),          # workgroups walk 3, 3 and 2 tiles; the last tile is partial
                                          (128 * 21 + 77, 1)])       # one accumulator set through 22 tiles
def test_mlp_bwd_fused_fc1_wgrad(M, max_blocks):
    ops = _ops()
    assert ops.mlp_bwd_wgrad_supported(C, H, ops.GA_BF16)
    assert not ops.mlp_bwd_wgrad_supported(192, 768, ops.GA_BF16) and not ops.mlp_bwd_wgrad_supported(C, H, ops.GA_F32)
    o = _operands(M)
    A, DH, DX, dW1, db1 = _launch(o, M, max_blocks, store=True)
    # 1. against the fp64 product of the kernel's own operands
    dh64 = DH.double().cpu()
    close(dW1.cpu() - FILL, dh64.T @ o['X'].double(), 2e-4, 'dW1')
    close(db1.cpu() - FILL, dh64.sum(0), 2e-4, 'db1')
    # 2. the stored tensors are what test_mlp_bwd asks of them
    close(A, o['a'], 2e-2, 'a')
    close(DH, o['dh'], 2e-2, 'dh')
    close(DX, o['dx'], 2e-2, 'dx')
    # 3. nothing stored: the same bits
    _, _, DX2, dW1b, db1b = _launch(o, M, max_blocks, store=False)
    assert torch.equal(dW1, dW1b) and torch.equal(db1, db1b) and torch.equal(DX, DX2)


def test_mlp_bwd_fused_fc1_wgrad_refused_at_192():
    """C = 192: the accumulators alone would take 288 registers -- the library's error, and nothing is launched"""
    from imagenet_models_amd import _lib
    ops = _ops()
    lib = _lib.load()
    M, Cw = 256, 192
    Hw = 4 * Cw
    assert ops.mlp_bwd_partials(M, Cw, ops.GA_BF16) == 0
    bf = dict(dtype=torch.bfloat16, device='cuda')
    X, DY, DX = torch.zeros(M, Cw, **bf), torch.zeros(M, Cw, **bf), torch.full((M, Cw), 7.0, **bf)
    W1, W2T, W1T = torch.zeros(Hw, Cw, **bf), torch.zeros(Hw, Cw, **bf), torch.zeros(Cw, Hw, **bf)
    b1 = torch.zeros(Hw, device='cuda')
    A, DH = torch.full((M, Hw), 7.0, **bf), torch.full((M, Hw), 7.0, **bf)
    dW1, db1 = torch.full((Hw, Cw), 7.0, device='cuda'), torch.full((Hw,), 7.0, device='cuda')
    part = torch.full((4 * (Hw * Cw + Hw),), 7.0, device='cuda')
    d = _lib.MlpBwdDesc()
    d.X, d.ldx, d.DY, d.lddy = X.data_ptr(), Cw, DY.data_ptr(), Cw
    d.W1, d.ldw1, d.b1 = W1.data_ptr(), Cw, b1.data_ptr()
    d.W2T, d.ldw2t, d.W1T, d.ldw1t = W2T.data_ptr(), Cw, W1T.data_ptr(), Hw
    d.A, d.lda, d.DH, d.lddh, d.DX, d.lddx = A.data_ptr(), Hw, DH.data_ptr(), Hw, DX.data_ptr(), Cw
    d.M, d.C, d.H, d.dtype = M, Cw, Hw, ops.GA_BF16
    d.dW1, d.ldw, d.db1 = dW1.data_ptr(), Cw, db1.data_ptr()
    d.partials, d.partials_bytes, d.max_blocks = part.data_ptr(), part.numel() * 4, 0
    lib.ga_last_error(ctypes.create_string_buffer(8), 8)
    rc = lib.ga_mlp_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    assert 'ga_mlp_bwd' in _lib.last_error() and 'ga_mlp_bwd_wgrad_supported' in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    for t in (A, DH, DX, dW1, db1, part):        # nothing ran: the outputs still hold what the test put there
        assert bool((t == 7.0).all())
    d.dW1 = None                                 # the same descriptor without dW1 is the plain launch
    assert lib.ga_mlp_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert not bool((DX == 7.0).all()) and bool((dW1 == 7.0).all())


# the small ConvNeXt and the batch of the parity tests (tests/test_convnext_gpu.py) with a 96-wide stage 0: the width at which the
# engine takes the fused MLP branch (bf16 mode)
CNX_96 = dict(dims=(96, 32, 64, 128), depths=(1, 1, 2, 1), num_classes=40)
BLK = 'stages.0.0.'


def _stage0_grads(monkeypatch, knob):
    import imagenet_models_amd as A
    from oracle import convnext_oracle as O
    monkeypatch.setenv('GAEXT_MLP_WG1', knob)          # read when the engine is built
    cfg = O.make_cfg(**CNX_96)
    m = A.ConvNeXt(num_classes=cfg['num_classes'], depths=cfg['depths'], dims=cfg['dims'], drop_path_rate=0.0, math_mode='bf16')
    m.load_state_dict(O.fill_state(cfg))
    m = m.cuda().train()
    opt = A.create_optimizer_v2(m, opt='sgd', lr=0.0, weight_decay=0.0, momentum=0.0)
    # two micro-batches per update and ONE call: the step stops before the optimizer and leaves the gradients in the flat buffer
    step = A.TrainStep(m, opt, 4, lam=-0.8, grad_accumulation=2)
    x = O.gen_input(4, seed=1)
    target = torch.randint(0, 40, (4,), generator=torch.Generator().manual_seed(5))
    step(x.cuda(), target.cuda())
    torch.cuda.synchronize()
    labels = [call[2] for call in step.eng.bwd.calls]
    st = m.flat_state()
    grads = {n: st['grads'][off:off + k].detach().double().cpu() for n, (off, k) in st['slices'].items()
             if n.startswith(BLK) and ('.pwconv1.' in n or '.norm.' in n)}
    return grads, labels


def test_engine_fused_fc1_wgrad_matches_the_wg1_launch(monkeypatch):
    old, lab_old = _stage0_grads(monkeypatch, '0')
    new, lab_new = _stage0_grads(monkeypatch, '1')
    assert any(l and l.endswith(BLK + 'wg1') for l in lab_old), 'the GAEXT_MLP_WG1=0 engine took no fused C = 96 branch'
    assert any(l and l.endswith(BLK + 'mlpb') for l in lab_new)
    assert not any(l and l.startswith('stages.0.') and l.endswith('wg1') for l in lab_new)
    assert sorted(old) == sorted(new) and len(old) == 4, sorted(old)
    for n in sorted(old):
        assert float(old[n].abs().max()) > 0
        close(new[n], old[n], 2e-4, n)
