"""tests/_attn_ref.py checked without a GPU: the closed-form float64 attention reference against torch.autograd, the
error metric on hand-made errors, and the validity condition of the gate that tests/test_attn_edges_gpu.py applies
to the bf16 kernels (block_err(kernel, exact) <= 2 * block_err(rounding_model, exact)): for every case gated that
way the rounding model itself stays within the project's bf16 attention tolerance of 2e-2, so twice its error is a
tight bound and not a loose one.  Measured here: at most 1.46e-2 over all cases (dq of (1, 129, 2, 48) offset; then
1.42e-2, dk of (1, 65, 1, 16) ramp)."""
import math

import pytest
import torch

import _attn_ref as R


@pytest.mark.parametrize('B,N,H,hd,kind', [(2, 37, 3, 16, 'plain'), (1, 70, 2, 64, 'ramp')])
def test_exact_matches_autograd(B, N, H, hd, kind):
    qkv, dout = R.make_inputs(B, N, H, hd, kind, seed=5)
    C = H * hd
    x = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)      # (3, B, H, N, hd)
    S = x[0] @ x[1].transpose(-1, -2) * hd ** -0.5
    out = torch.softmax(S, dim=-1) @ x[2]
    out.backward(R.split_heads(dout, B, N, H, hd))
    ref = dict(out=out.detach(), lse=torch.logsumexp(S, -1).detach(), dq=x.grad[0], dk=x.grad[1], dv=x.grad[2])
    got = dict(zip(('out', 'lse', 'dq', 'dk', 'dv'), R.exact(qkv, dout, B, N, H, hd)))
    assert got['out'].shape == (B, H, N, hd) and got['lse'].shape == (B, H, N) and qkv.shape == (B * N, 3 * C)
    for n in ('out', 'dq', 'dk', 'dv'):
        assert R.block_err(got[n], ref[n], N) <= 1e-12, n
    assert float((got['lse'] - ref['lse']).abs().max()) <= 1e-12


def test_inputs_are_representable_and_of_the_stated_kind():
    B, N, H, hd = 2, 257, 1, 64
    rowmax = {}
    for kind in R.KINDS:
        qkv, dout = R.make_inputs(B, N, H, hd, kind, seed=3)
        assert torch.equal(qkv, R.rnd(qkv, torch.bfloat16)) and torch.equal(dout, R.rnd(dout, torch.bfloat16))
        out, lse, *_ = R.exact(qkv, dout, B, N, H, hd)
        q, k = (R.split_heads(qkv[:, j * hd:(j + 1) * hd], B, N, H, hd) for j in range(2))
        P = torch.exp(q @ k.transpose(-1, -2) * hd ** -0.5 - lse[..., None])
        rowmax[kind] = float(P.max(-1).values.mean())
        if kind == 'offset':
            assert float(lse.min()) > 30.0               # the common +32 is there
        if kind == 'ramp':                               # the maximum over keys [0, 64 j) keeps rising: alpha < 1 in a full block
            S = q @ k.transpose(-1, -2)                  # (the ramp is 9 per block against a noise maximum of ~14 +- 3: nearly every row)
            m = torch.stack([S[..., :64 * j].max(-1).values for j in range(1, 5)], -1)      # the four full blocks
            assert float((m[..., 1:] > m[..., :-1]).double().mean()) > 0.95
    assert rowmax['plain'] < 0.1 and rowmax['sharp'] > 0.6, rowmax


def test_block_err_localises_and_normalises():
    N = 40
    ref = torch.ones(2, 3, N, 8, dtype=torch.float64)
    assert R.block_err(ref.clone(), ref, N) == 0.0
    got = ref.clone()
    got[1, 2, 32:40] += 0.5                              # the short last block (8 rows) of one head: every element off by 0.5
    assert abs(R.block_err(got, ref, N) - 0.5) < 1e-12
    got = ref.clone()
    got[0, 0, 16] += 0.5                                 # one row of a full block: 0.5 * sqrt(8) over sqrt(16 * 8)
    assert abs(R.block_err(got, ref, N) - 0.5 / 4.0) < 1e-12
    got = ref.clone()
    got[0, 1, 3, 2] = float('nan')
    assert R.block_err(got, ref, N) == math.inf
    z = torch.zeros(1, 1, N, 8, dtype=torch.float64)
    assert R.block_err(z.clone(), z, N) == 0.0
    z2 = z.clone()
    z2[0, 0, 0, 0] = 1e-30
    assert R.block_err(z2, z, N) == math.inf


@pytest.mark.parametrize('B,N,H,hd,kind', R.bf16_gated_cases())
def test_rounding_model_validity(B, N, H, hd, kind):
    """the validity condition of the GPU gate: the model of the declared bf16 arithmetic is itself within 2e-2"""
    e = R.reference(B, N, H, hd, kind)['model_err']
    print(f'B{B} N{N} H{H} hd{hd} {kind}: ' + ' '.join(f'{n} {v:.2e}' for n, v in e.items()))
    for n, v in e.items():
        assert v <= 2e-2, (n, v)
