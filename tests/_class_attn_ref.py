"""Float64 closed forms, seeded inputs, the tolerance gate and the shared case tables for the multi-token class-attention
kernels of csrc/map.hip (ga_class_attn_mt_fwd / _bwd and the `interactive` pair ga_class_attn_mt_ia_fwd / _bwd).  Pure
torch on the CPU, written from the formulas in include/gaext.h and the kernel headers; tests/test_class_attn_ref_cpu.py
validates it and tests/test_class_attn_mt_edges_gpu.py gates the kernels with it.

Layouts, as in the header: q [B][T][E], kv_cls [B][T][2E] (k | v of the class rows), kv_tok [B][N-T][2E] (k | v of the
image tokens), dout / out / dq [B][T][E], mask and P [B][T][heads][N], E = heads * hd, key n < T is class row n.
A case is the tuple (B, T, Nt, heads, hd) with N = T + Nt.

With S[b][t][h][n] = scale * q[b][t][h] . k[b][n][h]:
  plain        A = softmax_n(S),  D = A * mask,  out[b][t][h] = sum_n D[b][t][h][n] v[b][n][h],  P = A
               dD = dout . v,  dA = dD * mask,  dS = A * (dA - sum_n dA A),
               dq = scale dS k,  dk = scale dS^T q,  dv = D^T dout
  interactive  U = S + W1 S + b1,  A = softmax_n(U),  Pm = A + W2 A + b2,  D = Pm * mask,  out = D v,  P = A
               (W S)[h][n] = sum_g W[h][g] S[g][n]: the linears mix the HEADS of one (b, t, n))
               dPm = dD * mask,  dW2[h][g] = sum dPm[h] A[g],  db2[h] = sum dPm[h],  dA = dPm + W2^T dPm,
               dU = A * (dA - sum_n dA A),  dW1[h][g] = sum dU[h] S[g],  db1[h] = sum dU[h],  dS = dU + W1^T dU,
               dq, dk, dv as above (the parameter gradients summed over b, t and n).
"""
import functools
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
KINDS = ('plain', 'sharp', 'masked')
PLAIN_OUT = ('out', 'P', 'dq', 'dkv_cls', 'dkv_tok')
IA_OUT = PLAIN_OUT + ('dW1', 'db1', 'dW2', 'db2')
FP32_STORED = ('P', 'dW1', 'db1', 'dW2', 'db2')          # stored as fp32 in both modes


def rnd(x, dt):
    """x (float64) rounded to dt, held as float64"""
    return x.to(F32).to(dt).to(F64)


def case_seed(case, kind):
    B, T, Nt, heads, hd = case
    return 1000003 * B + 100003 * T + 1009 * Nt + 101 * heads + hd + 7919 * KINDS.index(kind)


def make_inputs(case, dt, kind='plain'):
    """Seeded operands of one case, rounded to dt (W1, b1, W2, b2: fp32) and held as float64, so the kernels and the
    reference see identical numbers.
    plain:  randn everywhere (scores with std ~1: a broad softmax).
    sharp:  q times 16 (scores with std ~16): most softmax rows are close to one-hot.
    masked: randn and an attention-dropout mask with keep probability 0.5, already divided by keep (entries 0 or 2);
            row (b, t, h) = (0, 0, 0) and the last row of the mask are entirely zero (all attention of a query dropped).
    W1, W2 = 0.3 / sqrt(heads) * randn, b1, b2 = 0.3 / sqrt(heads) * (1 + |randn|) with alternating signs: every entry of
    b2 is well away from zero, so (A + W2 A + b2) * mask differs from A * mask + W2 (A ...) + b2 and its other orderings
    wherever the mask is 0 or 2."""
    assert kind in KINDS, kind
    B, T, Nt, heads, hd = case
    E, N = heads * hd, T + Nt
    g = torch.Generator().manual_seed(case_seed(case, kind))
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    i = dict(q=r(B, T, E), kv_cls=r(B, T, 2 * E), kv_tok=r(B, Nt, 2 * E), dout=r(B, T, E), mask=None)
    if kind == 'sharp':
        i['q'] *= 16.0
    a = 0.3 / math.sqrt(heads)
    sign = torch.tensor([1.0, -1.0], dtype=F64).repeat(heads)[:heads]
    i['W1'], i['W2'] = a * r(heads, heads), a * r(heads, heads)
    i['b1'], i['b2'] = a * (1 + r(heads).abs()) * sign, -a * (1 + r(heads).abs()) * sign
    if kind == 'masked':
        m = (torch.rand(B, T, heads, N, generator=g, dtype=F64) < 0.5).to(F64) / 0.5
        m[0, 0, 0] = 0.0
        m[-1, -1, -1] = 0.0
        i['mask'] = m
    for n in ('q', 'kv_cls', 'kv_tok', 'dout'):
        i[n] = rnd(i[n], dt)
    for n in ('W1', 'b1', 'W2', 'b2'):
        i[n] = rnd(i[n], F32)
    i['case'], i['scale'] = case, hd ** -0.5
    return i


# ---------------------------------------------------------------------------------------------------------------------
# closed forms (no autograd).  `dtype` lets tests/test_class_attn_ref_cpu.py evaluate the same formulas in fp32.
# ---------------------------------------------------------------------------------------------------------------------
def _qkv(i, dtype):
    B, T, Nt, heads, hd = i['case']
    kv = torch.cat([i['kv_cls'], i['kv_tok']], 1).to(dtype)                     # [B][N][2E]
    E = heads * hd
    q = i['q'].to(dtype).reshape(B, T, heads, hd)
    k, v = kv[..., :E].reshape(B, T + Nt, heads, hd), kv[..., E:].reshape(B, T + Nt, heads, hd)
    return q, k, v


def _scores(i, dtype):
    q, k, v = _qkv(i, dtype)
    return q, k, v, torch.einsum('bthd,bnhd->bthn', q, k) * i['scale']


def _mix(W, X):
    """(W X)[b][t][h][n] = sum_g W[h][g] X[b][t][g][n]"""
    return torch.einsum('hg,btgn->bthn', W, X)


def _apply_mask(X, i):
    return X if i['mask'] is None else X * i['mask'].to(X.dtype)


def _out(D, v, i):
    B, T, Nt, heads, hd = i['case']
    return torch.einsum('bthn,bnhd->bthd', D, v).reshape(B, T, heads * hd)


def _dqkv(dS, D, q, k, g, i):
    """dq [B][T][E], dkv_cls [B][T][2E], dkv_tok [B][Nt][2E] from the score gradient and the dv weights"""
    B, T, Nt, heads, hd = i['case']
    E = heads * hd
    dq = torch.einsum('bthn,bnhd->bthd', dS, k).reshape(B, T, E) * i['scale']
    dk = torch.einsum('bthn,bthd->bnhd', dS, q).reshape(B, T + Nt, E) * i['scale']
    dv = torch.einsum('bthn,bthd->bnhd', D, g).reshape(B, T + Nt, E)
    dkv = torch.cat([dk, dv], -1)
    return dq, dkv[:, :T], dkv[:, T:]


def _softmax_bwd(A, dA):
    return A * (dA - (dA * A).sum(-1, keepdim=True))


def plain_fwd(i, dtype=F64):
    """out [B][T][E], P [B][T][heads][N]"""
    q, k, v, S = _scores(i, dtype)
    A = torch.softmax(S, -1)
    return _out(_apply_mask(A, i), v, i), A


def plain_bwd(i, dtype=F64):
    """dq, dkv_cls, dkv_tok"""
    q, k, v, S = _scores(i, dtype)
    B, T, Nt, heads, hd = i['case']
    g = i['dout'].to(dtype).reshape(B, T, heads, hd)
    A = torch.softmax(S, -1)
    dA = _apply_mask(torch.einsum('bthd,bnhd->bthn', g, v), i)
    return _dqkv(_softmax_bwd(A, dA), _apply_mask(A, i), q, k, g, i)


def ia_fwd(i, dtype=F64):
    """out, P (= A, the softmax output)"""
    q, k, v, S = _scores(i, dtype)
    W1, b1, W2, b2 = (i[n].to(dtype) for n in ('W1', 'b1', 'W2', 'b2'))
    A = torch.softmax(S + _mix(W1, S) + b1[:, None], -1)
    Pm = A + _mix(W2, A) + b2[:, None]
    return _out(_apply_mask(Pm, i), v, i), A


def ia_bwd(i, dtype=F64):
    """dq, dkv_cls, dkv_tok, dW1, db1, dW2, db2"""
    q, k, v, S = _scores(i, dtype)
    B, T, Nt, heads, hd = i['case']
    W1, b1, W2, b2 = (i[n].to(dtype) for n in ('W1', 'b1', 'W2', 'b2'))
    g = i['dout'].to(dtype).reshape(B, T, heads, hd)
    A = torch.softmax(S + _mix(W1, S) + b1[:, None], -1)
    D = _apply_mask(A + _mix(W2, A) + b2[:, None], i)
    dPm = _apply_mask(torch.einsum('bthd,bnhd->bthn', g, v), i)
    dW2, db2 = torch.einsum('bthn,btgn->hg', dPm, A), dPm.sum((0, 1, 3))
    dU = _softmax_bwd(A, dPm + _mix(W2.t(), dPm))
    dW1, db1 = torch.einsum('bthn,btgn->hg', dU, S), dU.sum((0, 1, 3))
    dS = dU + _mix(W1.t(), dU)
    return _dqkv(dS, D, q, k, g, i) + (dW1, db1, dW2, db2)


def evaluate(family, i, dtype=F64):
    """every result of one family as a dict name -> tensor"""
    if family == 'plain':
        return dict(zip(PLAIN_OUT, plain_fwd(i, dtype) + plain_bwd(i, dtype)))
    return dict(zip(IA_OUT, ia_fwd(i, dtype) + ia_bwd(i, dtype)))


@functools.lru_cache(maxsize=None)
def reference(family, case, dt, kind='plain'):
    """inputs and the float64 results of one case; computed once and shared: callers must not modify what it returns"""
    i = make_inputs(case, dt, kind)
    return dict(family=family, dt=dt, inputs=i, exact=evaluate(family, i))


# ---------------------------------------------------------------------------------------------------------------------
# the gate: the single place where the tolerance lives
# ---------------------------------------------------------------------------------------------------------------------
R_BF16 = 2.0 ** -8
FLOOR = 2e-4
ROW_SUM_TOL = 1e-5


def stored_dtype(name, dt):
    return F32 if name in FP32_STORED else dt


def gate(got, ref, out_dt, zero_scale=0.0):
    """Worst over the elements of |got - ref| / allowed, allowed = r |ref| + 2e-4 max|ref|; the caller asserts <= 1.

    r = 2^-8 for a tensor stored as bf16: the kernels compute in fp32 from the stored operands and round ONCE, so no
    intermediate rounding is modelled.  Half a bf16 ulp is between 2^-9 (just below a power of two) and 2^-8 (just
    above one) of the value; r is the lower figure times F = 2, the factor tests/test_attn_edges_gpu.py argues for,
    which is also the upper figure: r |ref| admits exactly the one rounding, and everything else (summation order,
    __expf) has to fit into the floor.  The fp32 evaluation in tests/test_class_attn_ref_cpu.py reaches 0.9 this way.
    r = 0 for a tensor stored as fp32 (P, dW1, db1, dW2, db2, and everything in fp32 mode).
    2e-4 max|ref| is the project's fp32 tolerance (tests/test_kernels_gpu.py): it covers the fp32 summation error of
    elements that are small next to the tensor's largest because their terms cancel.

    Where the exact result is identically zero the floor would vanish with it, and the bound falls back to
    2e-4 * zero_scale, zero_scale = the largest magnitude of the operand product that cancels (see zero_scale() below;
    the counterpart of _zero_ref_bound in tests/test_attn_edges_gpu.py).  Two such cases exist.  A fully masked
    (b, t, h) row contributes nothing to dk | dv, and where every row that feeds a tensor is masked the tensor is zero.
    And db1 = sum_n dU is zero for ANY input, because the softmax backward dU = A (dA - sum_n dA A) sums to zero over n:
    the kernel's db1 is the fp32 rounding noise of that cancellation.  float64 leaves a residue of ~1e-16 of the scale
    there, so "identically zero" is max|ref| <= 1e-9 * zero_scale.  With zero_scale = 0 a zero reference demands got == 0.

    NaN or inf in got gives inf."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if top <= 1e-9 * float(zero_scale):
        top = float(zero_scale)
    allowed = (R_BF16 if out_dt == BF else 0.0) * ref.abs() + FLOOR * top
    err = (got - ref).abs()
    inf = torch.full_like(err, math.inf)
    ratio = torch.where(allowed > 0, err / allowed.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf).max()) if ratio.numel() else 0.0


def zero_scale(family, i, name):
    """The fallback scale of gate() for a gradient whose exact value is identically zero.  The softmax backward
    dU = A (dA - sum_n dA A) is where a zero arises from fp32 terms that cancel: with sum_n A = 1 each side of the
    difference is at most max|dA| (dA = dout . v * mask, interactive: that plus W2^T of it).
      db1 = sum over (b, t, n) of dU: B T rows, each a cancellation of terms that sum to at most max|dA|; fp32 sums of
          N terms err by far less than 2e-4 / (B T) of that for the B T <= 16 and N <= 200 of the tables -> max|dA|.
      dq, dk multiply dS (at most max|dA| per entry) by scale and by an entry of k / q -> scale max|dA| max(max|q|, max|k|);
          dv has no cancellation, the bound of dk is used for the k | v rows as a whole.
    out, P, dW1, dW2 and db2 are never identically zero on the tabled cases: they get 0, an exact comparison."""
    if name not in ('dq', 'dkv_cls', 'dkv_tok', 'db1'):
        return 0.0
    B, T, Nt, heads, hd = i['case']
    q, k, v = _qkv(i, F64)
    dA = _apply_mask(torch.einsum('bthd,bnhd->bthn', i['dout'].reshape(B, T, heads, hd), v), i)
    if family == 'ia':
        dA = dA + _mix(i['W2'].t(), dA)
    top = float(dA.abs().max())
    return top if name == 'db1' else i['scale'] * top * max(float(q.abs().max()), float(k.abs().max()))


def row_sum_err(P):
    """max |sum_n P - 1| over the rows of P, summed in float64"""
    return float((P.to(F64).sum(-1) - 1.0).abs().max())


def gate_all(got, ref):
    """name -> worst ratio for every tensor of reference()'s result `ref` that is present in `got`"""
    return {n: gate(got[n], x, stored_dtype(n, ref['dt']), zero_scale(ref['family'], ref['inputs'], n))
            for n, x in ref['exact'].items() if n in got}


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_class_attn_mt_edges_gpu.py, (B, T, Nt, heads, hd); tests/test_class_attn_ref_cpu.py proves the
# closed forms and the reachability of the gate on every one of them
# ---------------------------------------------------------------------------------------------------------------------
def mt_lds(T, N, heads, hd, bwd):
    """restates mt_lds of csrc/map.hip: scores of one query [N][E / 8], one (forward) or two (backward) planes
    [T][heads][N] and the 16 x E reduction buffer, fp32"""
    E = heads * hd
    return 4 * (N * (E // 8) + (2 if bwd else 1) * T * heads * N + 16 * E)


def ia_lds(T, N, heads, bwd):
    """restates the wrappers of the interactive pair: two planes [heads][N] forward, 2T + 4 backward, fp32"""
    return 4 * ((2 * T + 4) if bwd else 2) * heads * N


LDS_LIMIT = 160 * 1024


def largest_n(lds):
    """largest N with lds(N) <= LDS_LIMIT (lds is increasing in N)"""
    n = 1
    while lds(n + 1) <= LDS_LIMIT:
        n += 1
    return n


PLAIN_T = tuple((2, T, 49, 4, 16) for T in (1, 4, 5, 6, 7, 8))                            # MT = 4, 6 and 8
PLAIN_N = tuple((2, T, N - T, 4, 16) for T in (3, 5) for N in (T + 1, 9, 17, 63, 64, 65, 129, 200))
PLAIN_HEADS = tuple((2, 4, 49, h, 8) for h in (1, 8, 9, 16, 17, 64))                      # 64: E = 512, every lane live
PLAIN_HD = ((2, 4, 49, 4, 8), (2, 4, 49, 4, 24), (2, 4, 49, 4, 64), (2, 4, 49, 1, 8), (2, 4, 49, 16, 32))
PLAIN_STRIDE = (2, 5, 49, 4, 24)
PLAIN_KIND_SHAPES = ((2, 5, 49, 4, 16), (2, 3, 62, 4, 16), (2, 4, 49, 16, 32))
PLAIN_LDS_HEADS, PLAIN_LDS_HD, PLAIN_LDS_T = 64, 8, 8
PLAIN_LDS_N = {bwd: largest_n(lambda n: mt_lds(PLAIN_LDS_T, n, PLAIN_LDS_HEADS, PLAIN_LDS_HD, bwd)) for bwd in (False, True)}
PLAIN_LDS = {bwd: (1, PLAIN_LDS_T, n - PLAIN_LDS_T, PLAIN_LDS_HEADS, PLAIN_LDS_HD) for bwd, n in PLAIN_LDS_N.items()}
PLAIN_TWICE = (2, 5, 60, 8, 16)

# map_resnet50: n_tokens = 4 and the self-distillation token -> T = 5, 12 heads of 32 (map_resnet.py);
# map_mobilenet_v1: n_tokens = 4, no self-distillation token -> T = 4 (mobilenet.py; its 192-wide head has 6 heads of 32,
# the 12-head T = 4 shape is the same head at map_resnet50's width); 49 = the 7 x 7 map at 224 x 224
IA_MODEL = ((2, 4, 49, 12, 32), (2, 5, 49, 12, 32), (2, 4, 49, 6, 32))
IA_HEADS = tuple((2, 3, 20, h, 8) for h in (1, 4, 5, 13))
IA_N = tuple((2, 3, N - 3, 3, 8) for N in (4, 63, 64, 65, 130))                          # heads * N: 12 .. 390 around 256
IA_T = ((2, 1, 20, 3, 8), (2, 8, 20, 3, 8))
IA_HD12 = (2, 3, 20, 3, 12)
IA_LDS_T, IA_LDS_HEADS, IA_LDS_HD = 8, 12, 8
IA_LDS_N = largest_n(lambda n: ia_lds(IA_LDS_T, n, IA_LDS_HEADS, True))
IA_LDS = (1, IA_LDS_T, IA_LDS_N - IA_LDS_T, IA_LDS_HEADS, IA_LDS_HD)
IA_TWICE = (2, 5, 49, 12, 32)


def plain_gated():
    """every (case, kind) the GPU module gates on the plain kernels"""
    s = list(PLAIN_T) + list(PLAIN_N) + list(PLAIN_HEADS) + list(PLAIN_HD) + [PLAIN_STRIDE, PLAIN_TWICE] + list(PLAIN_LDS.values())
    c = {(x, 'plain') for x in s}
    c |= {(x, k) for x in PLAIN_KIND_SHAPES for k in ('sharp', 'masked')}
    return sorted(c)


def ia_gated():
    s = list(IA_MODEL) + list(IA_HEADS) + list(IA_N) + list(IA_T) + [IA_HD12, IA_LDS, IA_TWICE]
    c = {(x, 'plain') for x in s}
    c |= {(x, k) for x in IA_MODEL[:2] for k in ('sharp', 'masked')}
    return sorted(c)
