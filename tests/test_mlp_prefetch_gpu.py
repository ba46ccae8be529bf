"""Next-tile prefetch in the persistent fused MLP backward (knob MLP_PREFETCH, csrc/mlp.hip: mlp_bwd_kernel<96, 64, true, true>).

The prefetch moves rows, not arithmetic: with the knob on, A, DH, DX and the reduced dW1 / db1 must carry the BITS of the knob-off
launch (every tile through stage_rows).  C = 96, H = 384, bf16, dW1 / db1 given, automatic grid; G = the workgroups of that grid.
Row counts: 1 (no next tile), 127 and 129 (a ragged only tile; a second tile for one workgroup only), 128 G - 1 and 128 G + 1 (every
workgroup one tile, the last ragged; one workgroup with a ragged second tile that arrives by prefetch), 2 * 128 G + 129 (third
tiles: the two X images swap twice).  Per row count: knob 1 against knob 0 bit for bit; knob 1 against the fp64 closed form with the
gates of test_mlp_bwd_wgrad_gpu; X and DY with 256 NaN rows behind row M -- the buffer window of the row DMA must end at M -- give
finite results with the same bits; a second knob-1 launch gives the same bits."""
import functools

import pytest
import torch

from test_mlp_bwd_wgrad_gpu import C, FILL, H, _operands, close

N_PART = H * C + H
GUARD = 256


def _ops():
    from imagenet_models_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _grid():
    """workgroups of the automatic persistent grid when there are tiles enough (one per CU)"""
    ops = _ops()
    return ops.mlp_bwd_partials(1 << 24, C, ops.GA_BF16) // (4 * N_PART)


@functools.lru_cache(maxsize=None)
def _case(M):
    """operands and fp32 references (read only), on the host"""
    return _operands(M)


def _launch(o, M, prefetch, guard=False):
    from imagenet_models_amd import _lib
    ops = _ops()
    dev = dict(device='cuda')

    def rows(t):
        if not guard:
            return t.cuda()
        g = torch.full((M + GUARD, C), float('nan'), dtype=torch.bfloat16, **dev)
        g[:M] = t.cuda()
        return g

    X, DY = rows(o['X']), rows(o['DY'])
    A = torch.empty(M, H, dtype=torch.bfloat16, **dev)
    DH = torch.empty(M, H, dtype=torch.bfloat16, **dev)
    DX = torch.empty(M, C, dtype=torch.bfloat16, **dev)
    dW1, db1 = torch.full((H, C), FILL, **dev), torch.full((H,), FILL, **dev)
    part = torch.full((ops.mlp_bwd_partials(M, C, ops.GA_BF16) // 4,), float('nan'), **dev)
    with _lib.knobs(MLP_PREFETCH=prefetch):
        ops.Plan(eager=True).mlp_bwd(X, DY, o['W1'].cuda(), o['b1'].cuda(), o['W2'].T.contiguous().cuda(),
                                     o['W1'].T.contiguous().cuda(), A, DH, DX, M, C, ops.GA_BF16, dW1=dW1, db1=db1, partials=part)
        torch.cuda.synchronize()
    return dict(A=A, DH=DH, DX=DX, dW1=dW1, db1=db1)


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs ({int((a[k] != b[k]).sum())} elements)'


ROWS = ['1', '127', '129', '128*G-1', '128*G+1', '2*128*G+129']


@pytest.mark.gpu
@pytest.mark.parametrize('rows', ROWS)
def test_mlp_prefetch_same_bits(rows):
    G = _grid()
    assert G >= 2
    M = eval(rows, {'G': G})
    o = _case(M)
    on = _launch(o, M, 1)
    off = _launch(o, M, 0)
    _same_bits(on, off, f'M={M}: MLP_PREFETCH=1 against 0')
    # the fp64 closed form of the kernel's own operands, and the stored tensors (gates of test_mlp_bwd_wgrad_gpu)
    dh64 = on['DH'].double().cpu()
    close(on['dW1'].cpu() - FILL, dh64.T @ o['X'].double(), 2e-4, 'dW1')
    close(on['db1'].cpu() - FILL, dh64.sum(0), 2e-4, 'db1')
    close(on['A'], o['a'], 2e-2, 'a')
    close(on['DH'], o['dh'], 2e-2, 'dh')
    close(on['DX'], o['dx'], 2e-2, 'dx')
    # rows >= M never enter: NaN behind row M changes nothing
    guarded = _launch(o, M, 1, guard=True)
    for k, t in guarded.items():
        assert bool(torch.isfinite(t.float()).all()), f'M={M}: {k} is not finite with NaN rows behind row M'
    _same_bits(guarded, on, f'M={M}: NaN guard rows')
    _same_bits(_launch(o, M, 1), on, f'M={M}: second MLP_PREFETCH=1 launch')


def test_config_string_reports_mlp_prefetch(monkeypatch):
    """no GPU: the knob shows in the configuration record when it is set through the API or the environment"""
    from imagenet_models_amd import _lib
    assert 'MLP_PREFETCH' not in _lib.config_string()
    with _lib.knobs(MLP_PREFETCH=0):
        assert ' MLP_PREFETCH=0(api)' in _lib.config_string()
    assert 'MLP_PREFETCH' not in _lib.config_string()
    monkeypatch.setenv('GAEXT_MLP_PREFETCH', '0')
    assert ' host:GAEXT_MLP_PREFETCH=0' in _lib.config_string()
