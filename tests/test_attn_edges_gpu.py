"""Global attention kernels (csrc/attn.hip) at block edges, forced tile forms, padded leading dimensions, misaligned
operands and every delta / generic dispatch branch, against the float64 closed form of tests/_attn_ref.py; and the ViT
stem helpers (patchify, vit_embed_fwd / _bwd) against float64.

Gates.  bf16: every one of out, dq, dk, dv satisfies
    block_err(kernel, exact) <= F * block_err(rounding_model, exact),    F = 2,
both sides computed here (block_err: worst 16-row block, normalised per head).  The rounding model is the arithmetic the
kernel header declares; the kernel adds a different summation order, the exp2 / __expf approximations and the rounding
of the un-normalised P, each well below one bf16 ulp of a result, hence F = 2.  tests/test_attn_ref_cpu.py proves
block_err(rounding_model, exact) <= 2e-2 for every case gated here.  lse: |lse - lse64| <= 1e-3 * max(1, |lse64|) per
element.  fp32 generic kernels: block_err <= 2e-4 and 1e-5 for lse.  Where the exact result is identically zero (dq and
dk at N = 1, where dS = P (dP - delta) = 0) the kernel is held to the rounding noise of that cancellation instead, see
_zero_ref_bound.

Every case runs on buffers filled with NaN, pad columns and guard rows included: no in-range element may stay NaN (so
dqkv is overwritten, not accumulated into), everything else must keep its bits.

Every case prints block_err(kernel) / block_err(rounding_model) per tensor, and the module prints the worst ratio per
input kind when it is done (run with -s).  F = 2 rests on the argument above, not on those figures: a ratio above 2 is
a finding to be explained from the arithmetic, never a reason to adopt what was observed.

Worst kernel / model ratio seen on an MI355X, all 114 cases passing (kind: MFMA forms by input kind; generic: the simple
bf16 kernels, which round less than the model):
              out    dq     dk     dv
    plain     1.07   1.16   1.05   1.00
    sharp     0.87   0.99   1.16   1.00
    ramp      0.89   0.98   1.24   1.00
    offset    0.96   1.03   1.74   1.00
    generic   0.71   0.80   0.79   0.78
Closest to the limit: dk of (1, 129, 2, 48) offset, 5.91e-3 against the model's 3.40e-3.  There every q carries the
common component 2 sqrt(hd) u, so dk = dS^T q multiplies the rounding of dS and of delta by that component (the
amplification make_inputs describes), and the kernel's delta and dP come from differently ordered fp32 sums.
"""
import math

import pytest
import torch

import _attn_ref as R
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu

F = 2.0
BF, F32 = torch.bfloat16, torch.float32
WORST = {}       # (kind, tensor) -> worst kernel / model ratio of this run, printed when the module is done


def _ops():
    from imagenet_models_amd import ops
    return ops


def _aligned16(t):
    return t.data_ptr() % 16 == 0


def _vec(n, data=None):
    return Guarded(1, n, n, F32, data=data, guard=64)


class Run:
    pass


def run_attn(B, N, H, hd, kind='plain', dt=BF, padq=0, pado=0, dout_off=0, dqkv_off=0, parts=1, backward=True):
    """forward (+ backward) of one case on guarded NaN-filled buffers, as `parts` descriptors over equal sub-batches;
    checks the buffers and returns the results per head in float64 together with the dispatch the operands select"""
    ops = _ops()
    ref = R.reference(B, N, H, hd, kind, dt)
    C, M, n = H * hd, B * N, B * H * N
    ldq, ldo = 3 * C + padq, C + pado
    r = Run()
    r.ref, r.shape, r.dt, r.kind = ref, (B, N, H, hd), dt, kind
    r.qkv = Guarded(M, 3 * C, ldq, dt, data=ref['qkv'])
    r.out = Guarded(M, C, ldo, dt)
    r.dout = Guarded(M, C, ldo, dt, data=ref['dout'], off=dout_off)
    r.dqkv = Guarded(M, 3 * C, ldq, dt, off=dqkv_off)
    r.lse, r.ws = _vec(n), _vec(n)
    # mfma_eligible, mfma_bwd_eligible and delta_form below restate the dispatch conditions of ga_attn_fwd / ga_attn_bwd for these
    # operands.  The library does not report which kernel it launched, so the tests' assertions on them say which branch a case
    # is MEANT to reach (and fail when a case is edited so that it no longer would); they are no proof that the branch ran, and
    # a change of the thresholds in attn.hip has to be made here as well.
    vec_ld = ldq % 8 == 0 and ldo % 8 == 0
    if vec_ld:                 # whole rows with ld % 8 == 0 keep the interior 16-byte aligned
        assert _aligned16(r.qkv.view) and _aligned16(r.out.view)
        assert _aligned16(r.dout.view) == (dout_off % (16 // r.dout.flat.element_size()) == 0)
        assert _aligned16(r.dqkv.view) == (dqkv_off % (16 // r.dqkv.flat.element_size()) == 0)
    r.mfma_eligible = dt == BF and hd % 16 == 0 and hd <= 64 and vec_ld and _aligned16(r.qkv.view) and _aligned16(r.out.view)
    r.mfma_bwd_eligible = r.mfma_eligible and _aligned16(r.dout.view) and _aligned16(r.dqkv.view)
    L8 = hd // 8
    if hd % 8 == 0 and L8 & (L8 - 1) == 0 and _aligned16(r.out.view) and _aligned16(r.dout.view) and ldo % (8 if dt == BF else 4) == 0:
        r.delta_form = 'rows'
    elif hd % 8 == 0 and _aligned16(r.out.view) and _aligned16(r.dout.view) and ldo % 8 == 0:
        r.delta_form = 'heads'
    else:
        r.delta_form = 'generic'
    p = ops.Plan(eager=True)
    Bp = B // parts
    assert Bp * parts == B
    for i in range(parts):
        rows = slice(i * Bp * N, (i + 1) * Bp * N)
        st = slice(i * Bp * H * N, (i + 1) * Bp * H * N)
        d = p.attn_desc(r.qkv.view[rows], r.out.view[rows], r.lse.view[:, st], Bp, N, H, hd, hd ** -0.5, ops.ga_dtype(dt), ldq=ldq, ldo=ldo)
        p.attn_fwd(d)
        if backward:
            p.attn_bwd(d, r.dout.view[rows], r.dqkv.view[rows], r.ws.view[:, st])
    torch.cuda.synchronize()
    r.qkv.check('qkv', written=False)
    r.dout.check('dout', written=False)
    r.out.check('out')
    r.lse.check('lse')
    r.dqkv.check('dqkv', written=backward)
    r.ws.check('workspace', written=backward)
    heads = lambda x: R.split_heads(x.double().cpu(), B, N, H, hd)
    dq = r.dqkv.inner()
    r.got = dict(out=heads(r.out.inner()), lse=r.lse.inner().double().cpu().view(B, H, N),
                 dq=heads(dq[:, :C]), dk=heads(dq[:, C:2 * C]), dv=heads(dq[:, 2 * C:]))
    return r


def _zero_ref_bound(r, name):
    """N = 1: P = 1, so dP = dO . v = delta and dq = dk = 0 exactly.  The kernel forms dP and delta as two fp32 dot
    products of the same hd terms in different orders, each within hd * u * sum|dO v| of the exact value (u = 2^-23 allows
    for accumulators that truncate), so |dS| <= 2 hd u sum|dO v| and |dq_c| <= scale |dS| |k_c| (dk: |q_c|); 1 % covers
    P, the dS and the result rounding."""
    B, N, H, hd = r.shape
    assert N == 1
    C = H * hd
    q, k, v = (R.split_heads(r.ref['qkv'][:, j * C:(j + 1) * C], B, N, H, hd) for j in range(3))
    g = R.split_heads(r.ref['dout'], B, N, H, hd)
    ds = 2 * hd * 2.0 ** -23 * (g * v).abs().sum(-1, keepdim=True)
    return 1.01 * hd ** -0.5 * ds * (k if name == 'dq' else q).abs()


def gate(r, label, tensors=('out', 'dq', 'dk', 'dv'), row=None):
    """row: the line of the worst-ratio report this case counts under (default: its input kind on the MFMA forms, 'generic' else)"""
    B, N, H, hd = r.shape
    ex, got, bad, line = r.ref['exact'], r.got, [], []
    tol = 1e-3 if r.dt == BF else 1e-5
    e_l = float(((got['lse'] - ex['lse']).abs() / ex['lse'].abs().clamp(min=1.0)).max())
    line.append(f'lse {e_l:.1e}')
    if not e_l <= tol:
        bad.append(f'lse {e_l:.2e} > {tol}')
    for n in tensors:
        if N == 1 and n in ('dq', 'dk'):          # zero in exact arithmetic (float64 leaves a residue of ~1e-16)
            assert float(ex[n].abs().max()) < 1e-12
            over = float((got[n].abs() - _zero_ref_bound(r, n)).max())
            line.append(f'{n} zero-ref max|x| {float(got[n].abs().max()):.1e}')
            if not over <= 0:
                bad.append(f'{n}: exact result is zero, kernel exceeds the cancellation bound by {over:.2e}')
            continue
        e = R.block_err(got[n], ex[n], N)
        if r.dt == BF:
            m = r.ref['model_err'][n]
            ratio = e / m if m > 0 else (0.0 if e == 0 else math.inf)
            line.append(f'{n} {e:.2e}/{m:.2e}={ratio:.2f}')
            key = (row or (r.kind if r.mfma_eligible else 'generic'), n)
            WORST[key] = max(WORST.get(key, 0.0), ratio)
            if not e <= F * m:
                bad.append(f'{n}: block_err {e:.3e} > {F} * model {m:.3e} (ratio {ratio:.2f})')
        else:
            line.append(f'{n} {e:.2e}')
            if not e <= 2e-4:
                bad.append(f'{n}: block_err {e:.3e} > 2e-4')
    print(f'[{label} B{B} N{N} H{H} hd{hd} {r.kind} {str(r.dt)[6:]}] ' + '  '.join(line))
    assert not bad, bad


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for kind in sorted({k for k, _ in WORST}):
        print(f'\nworst kernel/model ratio, {kind}: ' + '  '.join(f'{n} {WORST[(kind, n)]:.2f}' for n in ('out', 'dq', 'dk', 'dv') if (kind, n) in WORST))


# ---------------------------------------------------------------------------------------------------------------------
# bf16 MFMA forms
# ---------------------------------------------------------------------------------------------------------------------
def fwd_workgroups(B, N, H, qt=0):
    """dispatch rule of ga_attn_fwd: 64 * QT query rows per workgroup, QT = 2 from N = 128"""
    qt = qt or (2 if N >= 128 else 1)
    return -(-N // (64 * qt)) * B * H


@pytest.mark.parametrize('N', R.THRESH_N)
def test_thresholds_and_tails(N):
    r = run_attn(2, N, 2, 64)
    assert r.mfma_bwd_eligible and r.delta_form == 'rows'
    gate(r, 'edge')


@pytest.mark.parametrize('N', R.FORCED_N)
@pytest.mark.parametrize('kt', [1, 2])
@pytest.mark.parametrize('qt', [1, 2])
def test_forced_tile_forms(qt, kt, N, knobs):
    knobs(ATTN_QT=qt, ATTN_KT=kt)
    r = run_attn(2, N, 2, 64)
    assert r.mfma_bwd_eligible
    gate(r, f'QT{qt} KT{kt}')


@pytest.mark.parametrize('B,H,N', sorted(R.WALK))
def test_workgroup_walk(B, H, N):
    nwg = fwd_workgroups(B, N, H)
    assert nwg == R.WALK[(B, H, N)]          # 18 and 9: more than 8 and no multiple of 8; 7 and 1: fewer workgroups than XCDs
    r = run_attn(B, N, H, 64)
    assert r.mfma_bwd_eligible
    gate(r, f'walk nwg{nwg}')


@pytest.mark.parametrize('B,N,H,hd', R.HEAD_WIDTHS)
def test_head_widths_on_mfma(B, N, H, hd):
    r = run_attn(B, N, H, hd)
    assert r.mfma_bwd_eligible and r.delta_form == ('heads' if hd == 48 else 'rows')
    gate(r, 'width')


@pytest.mark.parametrize('padq,pado', R.LD_PADS)
@pytest.mark.parametrize('B,N,H,hd', R.LD_SHAPES)
def test_leading_dimensions(B, N, H, hd, padq, pado):
    r = run_attn(B, N, H, hd, padq=padq, pado=pado)
    assert r.mfma_bwd_eligible
    gate(r, f'ld+{padq}+{pado}')


@pytest.mark.parametrize('kind', ['sharp', 'ramp', 'offset'])
@pytest.mark.parametrize('B,N,H,hd', R.KIND_SHAPES)
def test_input_kinds(B, N, H, hd, kind):
    r = run_attn(B, N, H, hd, kind=kind)
    assert r.mfma_bwd_eligible
    if kind == 'offset':
        assert bool(torch.isfinite(r.got['out']).all()) and bool(torch.isfinite(r.got['lse']).all())
    gate(r, 'kind')


@pytest.mark.parametrize('which', ['dout', 'dqkv'])
def test_mfma_forward_then_simple_backward(which):
    """an operand 8 bytes off a 16-byte boundary: the forward is the MFMA form, the backward the simple kernels reading its
    lse; a misaligned dout also sends delta to the per-(b, h, q) kernel"""
    r = run_attn(*R.MISALIGNED, dout_off=4 if which == 'dout' else 0, dqkv_off=4 if which == 'dqkv' else 0)
    t = r.dout.view if which == 'dout' else r.dqkv.view
    assert t.data_ptr() % 16 == 8
    assert r.mfma_eligible and not r.mfma_bwd_eligible and r.delta_form == ('generic' if which == 'dout' else 'rows')
    gate(r, f'misaligned {which}')


def test_delta_heads_form_then_simple_backward(knobs):
    knobs(ATTN_MFMA=0)
    r = run_attn(*R.SIMPLE_HD48)
    assert r.delta_form == 'heads'
    gate(r, 'ATTN_MFMA=0', row='generic')


def test_sub_batch_descriptors_are_bit_identical():
    """one descriptor over B = 4 against two over the row slices [0, 2N) and [2N, 4N) (the engine's micro-batches): no
    atomics, one workgroup per output element in a fixed order, so only the workgroup-to-item map differs"""
    one = run_attn(*R.SUB_BATCH)
    two = run_attn(*R.SUB_BATCH, parts=2)
    gate(one, 'sub-batch')
    for name in ('out', 'lse', 'dqkv'):
        a, b = getattr(one, name), getattr(two, name)
        assert torch.equal(_bits(a.flat), _bits(b.flat)), name


# ---------------------------------------------------------------------------------------------------------------------
# generic kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,H,hd', R.GENERIC_F32)
def test_generic_fp32(B, N, H, hd):
    r = run_attn(B, N, H, hd, dt=F32)
    assert not r.mfma_eligible and r.delta_form == {12: 'generic', 20: 'generic', 40: 'heads', 96: 'heads', 64: 'rows', 128: 'rows'}[hd]
    gate(r, 'generic')


def test_generic_fp32_odd_leading_dimensions():
    shape, padq, pado = R.GENERIC_F32_ODD_LD
    r = run_attn(*shape, dt=F32, padq=padq, pado=pado)
    assert (shape[2] * shape[3] + pado) % 4 != 0 and r.delta_form == 'generic'
    gate(r, f'generic ld+{padq}+{pado}')


@pytest.mark.parametrize('B,N,H,hd', R.GENERIC_BF16)
def test_generic_bf16_wide_heads(B, N, H, hd):
    r = run_attn(B, N, H, hd)
    assert not r.mfma_eligible and r.delta_form == ('rows' if hd == 128 else 'heads')
    gate(r, 'generic')


# ---------------------------------------------------------------------------------------------------------------------
# ATTN_QT / ATTN_KT outside {0, 1, 2}
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('knob,call', [('ATTN_QT', 'fwd'), ('ATTN_QT', 'bwd'), ('ATTN_KT', 'bwd')])
def test_tile_knob_out_of_range_is_refused(knob, call, knobs):
    """only the <1> and <2> tile forms exist and the grid is sized from the knob: with 3 the launch would cover N in steps of 192
    rows with workgroups that handle 64, leaving the rest unwritten.  The call must fail before anything is launched."""
    ops = _ops()
    B, N, H, hd = 2, 257, 2, 64
    ref = R.reference(B, N, H, hd)
    C, M, n = H * hd, B * N, B * H * N
    qkv, dout = Guarded(M, 3 * C, 3 * C, BF, data=ref['qkv']), Guarded(M, C, C, BF, data=ref['dout'])
    out, dqkv, lse, ws = Guarded(M, C, C, BF), Guarded(M, 3 * C, 3 * C, BF), _vec(n), _vec(n)
    p = ops.Plan(eager=True)
    d = p.attn_desc(qkv.view, out.view, lse.view, B, N, H, hd, hd ** -0.5, ops.GA_BF16)
    if call == 'bwd':
        p.attn_fwd(d)
        torch.cuda.synchronize()
        out.check('out')
    knobs(**{knob: 3})
    err = None
    try:
        if call == 'fwd':
            p.attn_fwd(d)
        else:
            p.attn_bwd(d, dout.view, dqkv.view, ws.view)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    tgt = out.inner() if call == 'fwd' else dqkv.inner()[:, (0 if knob == 'ATTN_QT' else C):][:, :C]
    left = int(torch.isnan(tgt).any(1).sum())
    assert err is not None, f'{knob}=3 was accepted by ga_attn_{call}: {left} of {M} rows were never written'
    assert knob in err and '3' in err, err
    if call == 'fwd':
        out.check('out', written=False)
        lse.check('lse', written=False)
    else:
        dqkv.check('dqkv', written=False)
        ws.check('workspace', written=False)


# ---------------------------------------------------------------------------------------------------------------------
# ViT stem helpers
# ---------------------------------------------------------------------------------------------------------------------
def _randn(shape, seed, dt=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dt)


# the last shape: B (Np + 1) C / 8 = 2 107 400 items > 8192 blocks * 256, the grid-stride loop wraps
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('B,Np,C', [(1, 1, 8), (3, 9, 24), (2, 196, 200), (4, 2049, 2056)])
def test_vit_embed_fwd(B, Np, C, dt):
    ops = _ops()
    tok, cls, pos = _randn((B * Np, C), 1, dt), _randn((C,), 2), _randn((Np + 1, C), 3)
    x0 = Guarded(B * (Np + 1), C, C, dt)
    tok_d = Guarded(B * Np, C, C, dt, data=tok)
    ops.Plan(eager=True).vit_embed_fwd(tok_d.view, cls.cuda(), pos.cuda(), x0.view, B, Np, C, ops.ga_dtype(dt))
    torch.cuda.synchronize()
    x0.check('x0')
    tok_d.check('tok', written=False)
    ref = torch.cat([cls.double().expand(B, 1, C), tok.double().view(B, Np, C)], 1) + pos.double()
    got = x0.inner().cpu().view(B, Np + 1, C)
    if dt == F32:
        assert torch.equal(got, ref.float())
    else:       # one rounding to bf16 (8 significant bits: unit roundoff 2^-8) of the fp32 sum (2^-24)
        assert bool(((got.double() - ref).abs() <= 2.0 ** -8 * (1 + 2.0 ** -14) * ref.abs()).all())


# the last shape: (Np + 1) C / 8 = 1 052 929 items > 4096 blocks * 256
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('B,Np,C', [(1, 1, 8), (3, 9, 24), (2, 196, 200), (1, 4096, 2056)])
def test_vit_embed_bwd(B, Np, C, dt):
    ops = _ops()
    dx0 = _randn((B * (Np + 1), C), 4, dt)
    pre_cls, pre_pos = _randn((1, C), 5) + 3.0, _randn((Np + 1, C), 6) - 2.0
    dx_d = Guarded(B * (Np + 1), C, C, dt, data=dx0)
    dtok = Guarded(B * Np, C, C, dt)
    dcls, dpos = Guarded(1, C, C, F32, data=pre_cls, guard=64), Guarded(Np + 1, C, C, F32, data=pre_pos)
    ops.Plan(eager=True).vit_embed_bwd(dx_d.view, dtok.view, dcls.view, dpos.view, B, Np, C, ops.ga_dtype(dt))
    torch.cuda.synchronize()
    for name, b in (('dtok', dtok), ('dcls', dcls), ('dpos', dpos)):
        b.check(name)
    dx_d.check('dx0', written=False)
    x = dx0.view(B, Np + 1, C)
    assert torch.equal(_bits(dtok.inner().cpu().view(B, Np, C)), _bits(x[:, 1:].contiguous()))         # a copy
    s = x.double().sum(0)
    for name, got, ref in (('dpos', dpos.inner().cpu(), pre_pos.double() + s), ('dcls', dcls.inner().cpu(), pre_cls.double() + s[:1])):
        e = float(((got.double() - ref).abs().max(1).values / ref.abs().max(1).values).max())
        assert e <= 1e-6, (name, e)


# the last shape: B (H / P) (W / P) 3 P^2 / 8 = 2 359 296 items > 8192 blocks * 256
@pytest.mark.parametrize('dt', [F32, BF])
@pytest.mark.parametrize('B,H,W,P', [(2, 32, 48, 8), (2, 32, 48, 16), (6, 1024, 1024, 16)])
def test_patchify(B, H, W, P, dt):
    ops = _ops()
    x = _randn((B, 3, H, W), 7)
    K, L = 3 * P * P, (H // P) * (W // P)
    out = Guarded(B * L, K, K, dt)
    ops.Plan(eager=True).patchify(x.cuda(), out.view, P, ops.ga_dtype(dt))
    torch.cuda.synchronize()
    out.check('patches')
    ref = torch.nn.functional.unfold(x, P, stride=P).transpose(1, 2).reshape(B * L, K)                  # (c, ky, kx) order
    assert torch.equal(_bits(out.inner().cpu()), _bits(ref.to(dt).contiguous()))
