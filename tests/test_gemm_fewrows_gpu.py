"""GPU: the few-row forms (csrc/gemm_fewrows.hip) through their own entry points, ga_gemm_fewrows / ga_wgrad_fewrows, against float64
computed from the same bf16 inputs.

The yardstick is the existing path: on every output of every case the relative-norm error of the new form against float64 may not
exceed that of ga_gemm / ga_wgrad on the same descriptor by more than a factor of 2 (the allowance for another fp32 summation
order).  bf16 outputs are dominated by the output rounding in both forms; for fp32 outputs (c_f32, the column sums, dW, dbias) the
comparison is meaningful as it stands.  Every output buffer is wider than the matrix and pre-filled, so a store outside the tile
shows; the column sums are accumulated into, as the engines use them.

Measured pairs (MI355X; relative-norm error of the new form / of the existing form), printed by the tests before they assert:
  bf16 C, every NT case                                     1.38e-3 .. 2.02e-3 / the same to four digits (output rounding)
  fc1 C2 (GELU')           1x40x24 b3, 33x96x200            2.152e-3 / 2.152e-3, 2.110e-3 / 2.110e-3
  fp32 C                   31x1000x24 b3                    3.202e-8 / 3.202e-8
                           256x96x200                       4.834e-8 / 6.007e-8
                           1x8x8                            2.010e-8 / 2.010e-8
  colsum, colsumsq         31x40x2320                       4.673e-8 / 1.202e-7, 5.558e-8 / 1.139e-7
                           256x96x8 b3                      5.220e-8 / 6.819e-8, 5.274e-8 / 5.726e-8
  colsum (dgrad2)          1x1000x200 b3, 256x96x24, 31x8x8 6.446e-8 / 8.058e-8, 9.782e-8 / 1.162e-7, 4.579e-8 / 9.603e-8
  dW, dbias                256x1000x24 acc                  8.722e-8 / 8.722e-8, 2.762e-8 / 2.762e-8
                           49x88x2316 b3 store              3.720e-8 / 3.720e-8, 2.762e-8 / 2.762e-8
                           1x8x192 acc, 49x8x24 store       2.124e-8 / 2.124e-8, 3.513e-8 / 3.513e-8
                           256x88x192 b3 acc, alpha 0.5     8.894e-8 / 8.894e-8, 2.674e-8 / 2.674e-8
(the weight gradients agree to the digit: up to M = 256 both forms add the same 32-row MFMA steps in the same order)
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 777.0      # exactly representable in bf16


def _mods():
    from imagenet_models_amd import _lib as L, ops
    return L, ops


def _launch(fname, d):
    L, _ = _mods()
    L.check(getattr(L.load(), fname)(C.byref(d), torch.cuda.current_stream().cuda_stream), fname)


def _form(fname, d):
    L, _ = _mods()
    buf = C.create_string_buffer(64)
    L.check(getattr(L.load(), fname)(C.byref(d), buf, 64), fname)
    return buf.value.decode()


def _up8(n):
    return (n + 7) // 8 * 8


def _view(buf, Z, rows, cols, stride, ld):
    return torch.as_strided(buf, (Z, rows, cols), (stride, ld, 1))


def _relerr(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


def _gelu64(x):
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _compare(pairs, what):
    """pairs: name -> (new, old, float64 reference); the issue's bound on every output"""
    bad = []
    for name, (new, old, ref) in pairs.items():
        en, eo = _relerr(new, ref), _relerr(old, ref)
        print(f'{what} {name}: fewrows {en:.3e}  existing {eo:.3e}')
        if not en <= 2.0 * eo:
            bad.append((name, en, eo))
    assert not bad, (what, bad)


# ----------------------------------------------------------------------------------------------------------
# NT
# ----------------------------------------------------------------------------------------------------------
# (M, N, K, batch, epilogue): every epilogue once at a ragged and once at an aligned shape; M in {1, 31, 33, 256}, N in {8, 40, 96,
# 1000}, K in {8, 24, 200, 2320} all occur; batch 3 runs with a_batch_mod = 2; every leading dimension is wider than its matrix
NT_CASES = [
    (256, 1000, 200, 1, 'plain'), (33, 96, 2320, 3, 'plain'),
    (31, 1000, 24, 3, 'c_f32'), (256, 96, 200, 1, 'c_f32'), (1, 8, 8, 1, 'c_f32'),
    (33, 40, 200, 3, 'fc2'), (256, 96, 24, 1, 'fc2'),
    (31, 40, 2320, 1, 'colsum'), (256, 96, 8, 3, 'colsum'),
    (1, 40, 24, 3, 'fc1'), (33, 96, 200, 1, 'fc1'),
    (1, 1000, 200, 3, 'dg2'), (256, 96, 24, 1, 'dg2'), (31, 8, 8, 1, 'dg2'),
]


def _nt_case(M, N, K, Z, epi, seed):
    L, ops = _mods()
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16

    def rnd(n, scale=1.0, dt=bf):
        return (torch.randn(n, generator=g) * scale).to(dt).cuda()
    ZA = 2 if Z > 1 else 1
    lda, ldb, ldc = K + 8, K + 16, _up8(N) + 8
    sA, sB, sC = M * lda + 8, N * ldb + 16, M * ldc + 8
    A, B = rnd(ZA * sA), rnd(Z * sB, 1 / math.sqrt(K))
    a64 = _view(A, ZA, M, K, sA, lda).double().cpu()
    b64 = _view(B, Z, N, K, sB, ldb).double().cpu()
    sBias, sCol = N + 3, N + 5
    bias = rnd(Z * sBias, dt=torch.float32)
    f = dict(M=M, N=N, K=K, batch=Z, dtype=L.GA_BF16, A=A, lda=lda, strideA=sA, a_batch_mod=ZA if Z > 1 else 0, B=B, ldb=ldb,
             strideB=sB, ldc=ldc, strideC=sC, alpha=1.0, rows_per_scale=1)
    ref = torch.stack([a64[z % ZA] @ b64[z].t() for z in range(Z)])
    outs = ['C']
    if epi != 'dg2':
        f.update(bias=bias, strideBias=sBias)
        ref = ref + torch.as_strided(bias, (Z, 1, N), (sBias, 0, 1)).double().cpu()
    if epi == 'c_f32':
        f.update(c_f32=1)
    ref2 = None
    if epi == 'fc1':
        f.update(act=ops.ACT_GELU, c2_mode=2)
        ref, ref2 = _gelu64(ref)
        outs.append('C2')
    if epi == 'dg2':
        ldh, sH = _up8(N) + 16, M * (_up8(N) + 16) + 8
        H = rnd(Z * sH)
        f.update(H=H, ldh=ldh, strideH=sH, h_is_deriv=1)
        ref = ref * _view(H, Z, M, N, sH, ldh).double().cpu()
    if epi == 'fc2':
        rps = 7
        rs = (torch.rand((M + rps - 1) // rps, generator=g) + 0.5).cuda()
        ldr, sR = _up8(N) + 24, M * (_up8(N) + 24) + 4
        R = rnd(Z * sR)
        f.update(alpha=0.5, rowscale=rs, rows_per_scale=rps, R=R, ldr=ldr, strideR=sR)
        acc = torch.stack([a64[z % ZA] @ b64[z].t() for z in range(Z)])      # alpha scales the product, not the bias
        ref = 0.5 * acc + torch.as_strided(bias, (Z, 1, N), (sBias, 0, 1)).double().cpu()
        ref = ref * rs.double().cpu().repeat_interleave(rps)[:M][None, :, None] + _view(R, Z, M, N, sR, ldr).double().cpu()
    cols = epi in ('colsum', 'dg2')
    if cols:
        f.update(strideCol=sCol)
        outs.append('colsum')
        if epi == 'colsum':
            outs.append('colsumsq')
    cdt = torch.float32 if epi == 'c_f32' else bf

    def run(fname):
        Cb = torch.full((Z * sC,), SENT, dtype=cdt, device='cuda')
        C2b = torch.full((Z * sC,), SENT, dtype=bf, device='cuda') if epi == 'fc1' else None
        cs = torch.full((Z * sCol,), SENT, device='cuda') if cols else None
        cq = torch.full((Z * sCol,), SENT, device='cuda') if epi == 'colsum' else None
        for t in (cs, cq):
            if t is not None:
                torch.as_strided(t, (Z, N), (sCol, 1)).zero_()
        d = ops._set(L.GemmDesc(), C=Cb, C2=C2b, colsum=cs, colsumsq=cq, **f)
        if fname == 'ga_gemm_fewrows':
            assert _form('ga_gemm_fewrows_form', d).startswith('fewrows32x32:'), 'the case must reach the new kernel'
        _launch(fname, d)
        torch.cuda.synchronize()
        got = {'C': _view(Cb, Z, M, N, sC, ldc).clone()}
        if C2b is not None:
            got['C2'] = _view(C2b, Z, M, N, sC, ldc).clone()
        for name, t in (('colsum', cs), ('colsumsq', cq)):
            if t is not None:
                got[name] = torch.as_strided(t, (Z, N), (sCol, 1)).clone()
        if fname == 'ga_gemm_fewrows':      # canaries: nothing outside the matrices was written
            for name, t, v in (('C', Cb, _view(Cb, Z, M, N, sC, ldc)), ('C2', C2b, C2b is not None and _view(C2b, Z, M, N, sC, ldc)),
                               ('colsum', cs, cs is not None and torch.as_strided(cs, (Z, N), (sCol, 1))),
                               ('colsumsq', cq, cq is not None and torch.as_strided(cq, (Z, N), (sCol, 1)))):
                if t is not None:
                    v.fill_(SENT)
                    assert bool((t == SENT).all()), f'{name}: a store outside the matrix'
        return got
    new, old = run('ga_gemm_fewrows'), run('ga_gemm')
    refs = {'C': ref, 'C2': ref2, 'colsum': ref.sum(1), 'colsumsq': (ref * ref).sum(1)}
    return {name: (new[name], old[name], refs[name]) for name in outs}


@pytest.mark.parametrize('case', NT_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_nt_fewrows_against_fp64_and_the_existing_form(case):
    M, N, K, Z, epi = case
    _compare(_nt_case(M, N, K, Z, epi, seed=11), f'nt {M}x{N}x{K} b{Z} {epi}')


# ----------------------------------------------------------------------------------------------------------
# TN
# ----------------------------------------------------------------------------------------------------------
# (M, N, K, batch, accumulate, dbias, alpha): M in {1, 49, 256}, N in {8, 88, 1000}, K in {24, 192, 2316}; batch 3 runs with
# x_batch_mod = 2 and a strided dbias; ldx covers K rounded up to 8, ldw and the strides are wider than the matrices
TN_CASES = [
    (256, 1000, 24, 1, 1, True, 1.0), (49, 88, 2316, 3, 0, True, 1.0), (1, 8, 192, 1, 1, False, 1.0), (256, 88, 192, 3, 1, True, 0.5),
    (49, 8, 24, 1, 0, False, 1.0),
]


def _tn_case(M, N, K, Z, accumulate, dbias, alpha, seed):
    L, ops = _mods()
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16

    def rnd(n, dt=bf):
        return torch.randn(n, generator=g).to(dt).cuda()
    ZX = 2 if Z > 1 else 1
    ldy, ldx, ldw = N + 8, _up8(K) + 8, K + 3
    sY, sX, sW, sDb = M * ldy + 8, M * ldx + 16, N * ldw + 5, N + 3
    Y, X = rnd(Z * sY), rnd(ZX * sX)
    y64, x64 = _view(Y, Z, M, N, sY, ldy).double().cpu(), _view(X, ZX, M, K, sX, ldx).double().cpu()
    W0, db0 = rnd(Z * sW, torch.float32), rnd(Z * sDb, torch.float32)
    w0 = _view(W0, Z, N, K, sW, ldw).double().cpu()
    ref = alpha * torch.stack([y64[z].t() @ x64[z % ZX] for z in range(Z)]) + (w0 if accumulate else 0.0)
    refb = torch.as_strided(db0, (Z, N), (sDb, 1)).double().cpu() + alpha * y64.sum(1)
    f = dict(M=M, N=N, K=K, batch=Z, dtype=L.GA_BF16, Y=Y, ldy=ldy, strideY=sY, X=X, ldx=ldx, strideX=sX, x_batch_mod=ZX if Z > 1 else 0,
             ldw=ldw, strideW=sW, strideDbias=sDb, alpha=alpha, split_m=1, accumulate=accumulate)

    def run(fname):
        W, db = W0.clone(), db0.clone() if dbias else None
        d = ops._set(L.WgradDesc(), dW=W, dbias=db, **f)
        if fname == 'ga_wgrad_fewrows':
            assert _form('ga_wgrad_fewrows_form', d) == 'fewrows_tn64x64', 'the case must reach the new kernel'
        _launch(fname, d)
        torch.cuda.synchronize()
        return W, db
    Wn, dbn = run('ga_wgrad_fewrows')
    Wo, dbo = run('ga_wgrad')
    Wn2, dbn2 = run('ga_wgrad_fewrows')
    assert torch.equal(Wn, Wn2) and (not dbias or torch.equal(dbn, dbn2)), 'two runs give the same bits'
    pairs = {'dW': (_view(Wn, Z, N, K, sW, ldw), _view(Wo, Z, N, K, sW, ldw), ref)}
    if dbias:
        pairs['dbias'] = (torch.as_strided(dbn, (Z, N), (sDb, 1)), torch.as_strided(dbo, (Z, N), (sDb, 1)), refb)
    # canaries: the elements between the rows / batch elements keep their initial values
    for name, t, t0, v in (('dW', Wn.clone(), W0, (Z, N, K, sW, ldw)),):
        _view(t, *v).copy_(_view(t0, *v))
        assert torch.equal(t, t0), f'{name}: a store outside the matrix'
    if dbias:
        t = dbn.clone()
        torch.as_strided(t, (Z, N), (sDb, 1)).copy_(torch.as_strided(db0, (Z, N), (sDb, 1)))
        assert torch.equal(t, db0), 'dbias: a store outside the vector'
    return pairs


@pytest.mark.parametrize('case', TN_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_tn_fewrows_against_fp64_and_the_existing_form(case):
    M, N, K, Z, accumulate, dbias, alpha = case
    _compare(_tn_case(M, N, K, Z, accumulate, dbias, alpha, seed=13), f'tn {M}x{N}x{K} b{Z} acc{accumulate}')


# ----------------------------------------------------------------------------------------------------------
# what the new entry points do not take goes to the old ones unchanged
# ----------------------------------------------------------------------------------------------------------
def _fallback_pairs(dt, M, N, K):
    """the same product through both entry points of each kind: (new C, old C), (new dW, old dW), and the form names"""
    L, ops = _mods()
    g = torch.Generator().manual_seed(17)
    A = torch.randn(M, K, generator=g).to(dt).cuda()
    B = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt).cuda()
    Y = torch.randn(M, N, generator=g).to(dt).cuda()
    bias = torch.randn(N, generator=g).cuda()
    out = []
    forms = []
    for fname in ('ga_gemm_fewrows', 'ga_gemm'):
        Cb = torch.zeros(M, N, dtype=dt, device='cuda')
        d = ops._set(L.GemmDesc(), M=M, N=N, K=K, batch=1, dtype=ops.ga_dtype(dt), A=A, lda=K, B=B, ldb=K, C=Cb, ldc=N, alpha=1.0,
                     bias=bias, rows_per_scale=1)
        forms.append(_form('ga_gemm_fewrows_form', d))
        _launch(fname, d)
        out.append(Cb)
    for fname in ('ga_wgrad_fewrows', 'ga_wgrad'):
        W = torch.zeros(N, K, device='cuda')
        d = ops._set(L.WgradDesc(), M=M, N=N, K=K, batch=1, dtype=ops.ga_dtype(dt), Y=Y, ldy=N, X=A, ldx=K, dW=W, ldw=K, alpha=1.0,
                     split_m=1, accumulate=0)
        forms.append(_form('ga_wgrad_fewrows_form', d))
        _launch(fname, d)
        out.append(W)
    torch.cuda.synchronize()
    return out, forms


@pytest.mark.parametrize('what', ['fp32', 'tall', 'knob'])
def test_fewrows_entry_points_forward_what_they_do_not_take(what, knobs):
    if what == 'knob':
        knobs(FEWROWS=0)
    dt, M = (torch.float32, 256) if what == 'fp32' else (torch.bfloat16, 8192 if what == 'tall' else 256)
    (Cn, Co, Wn, Wo), forms = _fallback_pairs(dt, M, 192, 96)
    assert forms == ['none'] * 4, forms
    assert torch.equal(Cn, Co) and torch.equal(Wn, Wo)
    assert float(Cn.float().abs().max()) > 0 and float(Wn.abs().max()) > 0
