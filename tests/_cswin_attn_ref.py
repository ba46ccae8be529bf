"""Float64 closed forms, seeded inputs, the tolerance gate and the shared case tables for the CSWin stripe-attention
kernels of csrc/cswin.hip (ga_cswin_attn_fwd / _bwd, ga_cswin_lepe_wgrad, ga_cswin_lepe_wgrad_reduce).  Pure torch on the
CPU, written from the formulas in include/gaext.h and the kernel header comments; tests/test_cswin_attn_ref_cpu.py
validates it and tests/test_cswin_attn_edges_gpu.py gates the kernels with it.

Layouts, as in the header: qkv [B*L][3C] = q | k | v column blocks of width C, tokens in image raster order, L = reso^2;
dout / out [B*L][C]; dqkv as qkv.  Branch i owns channels [i*cb, (i+1)*cb), cb = C / nbranch, of every block, hpb =
heads / nbranch heads of hd = C / heads channels, and the stripe shape Hs[i] x Ws[i]; lepe_w[i] [cb][9] (tap = 3 (dy+1) +
dx+1), lepe_b[i] [cb].  A case is the tuple (B, reso, C, heads, stripes), stripes = ((Hs, Ws),) per branch.

Per (image, window, head), over the N = Hs Ws tokens of the window, scale = hd^-0.5:
  S[t][j] = (q_t scale) . k_j,  P = softmax_j(S),
  out[t][c] = sum_j P[t][j] v[j][c] + sum_tap w[c][tap] v[t + tap][c] + b[c]      (t + tap inside the WINDOW, else 0)
  dP[t][j] = dout_t . v_j,  delta_t = sum_j P dP,  dS = P (dP - delta)
  dq_t = scale sum_j dS[t][j] k_j,   dk_j = scale sum_t dS[t][j] q_t,
  dv_j = sum_t P[t][j] dout_t + sum_tap w[c][tap] dout[j - tap][c]                (the LePE transpose)
  dw[c][tap] = sum over all windows and tokens of dout[t][c] v[t + tap][c],   db[c] = sum of dout[t][c].

The gate (gate(), the single place where the tolerance lives), per element:
    |got - ref| <= r |ref| + 2^-8 A + 2e-4 max|ref|.
Generic form (A = 0): the kernels compute in fp32 from the stored operands and round once -- the project's class-attention
gate (tests/_class_attn_ref.py): r = 2^-8 for a tensor stored as bf16 (half a bf16 ulp is at most 2^-8 of the value), r = 0
for fp32 (everything in fp32 mode, and dw / db always); 2e-4 max|ref| is the project's fp32 tolerance and has to hold the
summation order and __expf.
MFMA form (bf16, head_dim 32, N <= 112): it rounds more than once BY DESIGN, at exactly these points:
  * P and dS are packed to bf16 (acc_pair_frag) before they enter the second product: P -> P (1 + e), |e| <= 2^-8, so
    sum_j P v changes by at most 2^-8 sum_j |P[t][j]| |v[j][c]|, and likewise for dS in dq / dk and P in dv;
  * the LePE weights are rounded to bf16 (lepe_wfrags): at most 2^-8 sum_tap |w[c][tap]| |x[t +- tap][c]|;
  * the operands read transposed (V, K, dO, Q) are the stored bf16 values: exact; the first products (S, dP), the softmax,
    delta and lse are fp32 of exact bf16 products; the fused dw / db partials are fp32 sums of exact products: A = 0.
So A (returned by evaluate() as abs_out / abs_dqkv next to the values) is
  out: sum_j P |v| + sum_tap |w| |v_shift|          dq: scale sum_j |dS| |k|
  dk:  scale sum_t |dS| |q|                         dv: sum_t P |dout| + sum_tap |w| |dout_shift|
and the element's own final rounding is r |ref| as above.  Every term is the worst case of one documented rounding; nothing
is fitted to what the kernels produce.  tests/test_cswin_attn_ref_cpu.py proves that an fp32 emulation with (without) these
roundings meets the MFMA (generic) gate on every case and kind, and that eleven wrong restatements do not.

Where the exact result is identically zero (N = 1: P = 1, dS = P (dP - delta) = 0, so dq = dk = 0) the floor falls back to
2e-4 * zero_scale, zero_scale = scale max|dP| max(|q|, |k|): the size of the terms that cancel.
"""
import functools
import math

import torch
import torch.nn.functional as Fn

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
KINDS = ('plain', 'sharp', 'negative')
WRONG = ('pad_unmasked', 'lepe_across_border', 'dv_not_flipped', 'tap_swapped', 'branch1_shape0', 'lepe_row_global',
         'dk_scale_twice', 'dk_scale_none', 'delta_dropped', 'bias_dropped', 'db_per_window')
R_BF16 = 2.0 ** -8
FLOOR = 2e-4
LDS_LIMIT = 160 * 1024


def rnd(x, dt):
    """x (float64) rounded to dt, held as float64"""
    return x.to(F32).to(dt).to(F64)


def geom(case):
    B, reso, C, heads, stripes = case
    nb = len(stripes)
    return B, reso, C, heads, nb, C // nb, heads // nb, C // heads


def n_tokens(case):
    return max(hs * ws for hs, ws in case[4])


def n_items(case):
    B, reso, C, heads, stripes = case
    return B * (reso // stripes[0][0]) * (reso // stripes[0][1]) * heads


def form(case, dt, knob=1):
    """'mfma' or 'generic': restates use_mfma of csrc/cswin.hip"""
    return 'mfma' if knob and dt == BF and case[2] // case[3] == 32 and n_tokens(case) <= 112 else 'generic'


def bwd_lds(case, dt, knob=1):
    """restates attn_lds of csrc/cswin.hip for the backward: (bytes, one-plane form?)"""
    hd, n = case[2] // case[3], n_tokens(case)
    if form(case, dt, knob) == 'mfma':
        kp = 64 if n <= 64 else 128
        return 4 * kp * 64 + 4096 + 2 * kp * 4 + 16, False
    two = 4 * (4 * 128 * (hd + 1) + 2 * n * (n + 1))
    return (two, False) if two <= LDS_LIMIT else (4 * (4 * 128 * (hd + 1) + n * (n + 1) + 128), True)


def case_seed(case, kind):
    B, reso, C, heads, stripes = case
    return 1000003 * B + 10007 * reso + 101 * C + 13 * heads + sum(7 * h + 3 * w for h, w in stripes) + 7919 * KINDS.index(kind)


def make_inputs(case, dt, kind='plain', only_wgrad=False):
    """Seeded operands of one case, rounded to dt (lepe_w, lepe_b: fp32) and held as float64, so the kernels and the
    reference see identical numbers.
    plain:    randn everywhere.
    sharp:    q times 16: near one-hot softmax rows (pins the max subtraction).
    negative: q = 1 + |randn|, k = -(1 + |randn|): every real score is far below 0, so a pad key left unmasked at score 0
              takes nearly all of the softmax mass and the result is wrong by O(1).
    only_wgrad: q and k stay zero (the weight-gradient kernel does not read them; spares the large case their randn)."""
    assert kind in KINDS, kind
    B, reso, C, heads, nb, cb, hpb, hd = geom(case)
    rows = B * reso * reso
    g = torch.Generator().manual_seed(case_seed(case, kind))
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    qkv = torch.zeros(rows, 3 * C, dtype=F64)
    if only_wgrad:
        qkv[:, 2 * C:] = r(rows, C)
    else:
        qkv = r(rows, 3 * C)
        if kind == 'sharp':
            qkv[:, :C] *= 16.0
        if kind == 'negative':
            qkv[:, :C] = 1.0 + qkv[:, :C].abs()
            qkv[:, C:2 * C] = -(1.0 + qkv[:, C:2 * C].abs())
    i = dict(qkv=rnd(qkv, dt), dout=rnd(r(rows, C), dt))
    i['lepe_w'] = [rnd(r(cb, 9) / 3, F32) for _ in range(nb)]
    i['lepe_b'] = [rnd(0.5 * (1 + r(cb).abs()) * (-1.0) ** k, F32) for k in range(nb)]     # every entry well away from zero
    i['case'], i['scale'] = case, hd ** -0.5
    return i


# ---------------------------------------------------------------------------------------------------------------------
# closed forms (no autograd).  dtype / mfma / flip give the fp32 emulations of tests/test_cswin_attn_ref_cpu.py, `wrong`
# its deliberately wrong restatements.
# ---------------------------------------------------------------------------------------------------------------------
def _win(x, B, reso, hs, ws, hpb):
    """[B*L][cb] -> [windows][hpb][N][hd]"""
    hd = x.shape[1] // hpb
    t = x.reshape(B, reso // hs, hs, reso // ws, ws, hpb, hd).permute(0, 1, 3, 5, 2, 4, 6)
    return t.reshape(-1, hpb, hs * ws, hd)


def _unwin(t, B, reso, hs, ws):
    """[windows][hpb][N][hd] -> [B*L][cb]"""
    hpb, hd = t.shape[1], t.shape[3]
    t = t.reshape(B, reso // hs, reso // ws, hpb, hs, ws, hd).permute(0, 1, 4, 2, 5, 3, 6)
    return t.reshape(B * reso * reso, hpb * hd)


def _shift(x, dy, dx, B, reso, hs, ws, across=False):
    """y[t] = x[t + (dy, dx)] in window layout [windows][hpb][N][hd], zero where the neighbour is outside the window
    (across: outside the IMAGE -- the wrong restatement that reads through the stripe border)"""
    W, hpb, N, hd = x.shape
    if across:
        img = _unwin(x, B, reso, hs, ws).reshape(B, reso, reso, hpb * hd)
        p = Fn.pad(img, (0, 0, 1, 1, 1, 1))[:, 1 + dy:1 + dy + reso, 1 + dx:1 + dx + reso]
        return _win(p.reshape(B * reso * reso, hpb * hd), B, reso, hs, ws, hpb)
    grid = Fn.pad(x.reshape(W, hpb, hs, ws, hd), (0, 0, 1, 1, 1, 1))
    return grid[:, :, 1 + dy:1 + dy + hs, 1 + dx:1 + dx + ws].reshape(W, hpb, N, hd)


def _bf(x):
    return x.to(BF).to(x.dtype)


def evaluate(i, dtype=F64, mfma=False, flip=False, wrong=None, only_wgrad=False):
    """out [B*L][C], dqkv [B*L][3C], dw [nb][cb][9], db [nb][cb], and the absolute sums abs_out / abs_dqkv of the gate.
    mfma: P, dS and the LePE weights rounded to bf16 where the MFMA kernels round them; flip: the token sums run in
    reversed order (another summation order than the default)."""
    assert wrong is None or wrong in WRONG, wrong
    case = i['case']
    B, reso, C, heads, nb, cb, hpb, hd = geom(case)
    scale = i['scale']
    rows = B * reso * reso
    qkv, dout = i['qkv'].to(dtype), i['dout'].to(dtype)
    out, abs_out = torch.zeros(rows, C, dtype=dtype), torch.zeros(rows, C, dtype=dtype)
    dqkv, abs_dqkv = torch.zeros(rows, 3 * C, dtype=dtype), torch.zeros(rows, 3 * C, dtype=dtype)
    dws, dbs = [], []
    mm = (lambda a, b: (a.flip(-1) @ b.flip(-2))) if flip else (lambda a, b: a @ b)
    for br in range(nb):
        hs, ws = case[4][0] if (wrong == 'branch1_shape0' and br == 1) else case[4][br]
        N = hs * ws
        sl = slice(br * cb, (br + 1) * cb)
        w_ = lambda x: _win(x, B, reso, hs, ws, hpb)
        q, k, v = w_(qkv[:, sl]), w_(qkv[:, C + br * cb:C + (br + 1) * cb]), w_(qkv[:, 2 * C + br * cb:2 * C + (br + 1) * cb])
        g = w_(dout[:, sl])
        src = (1 - br) if (wrong == 'lepe_row_global' and br == 1) else br    # [w1 | w0] back to back, row at the global channel
        w = i['lepe_w'][src].to(dtype).reshape(hpb, 1, hd, 9)
        bias = i['lepe_b'][src].to(dtype).reshape(hpb, 1, hd)
        wk = _bf(w) if mfma else w
        across = wrong == 'lepe_across_border'
        taps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        tapi = lambda dy, dx: (dx + 1) * 3 + dy + 1 if wrong == 'tap_swapped' else (dy + 1) * 3 + dx + 1
        sh = lambda x, dy, dx: _shift(x, dy, dx, B, reso, hs, ws, across)
        # ---- weight gradient
        dw = torch.stack([(g * sh(v, dy, dx)).sum((0, 2)) for dy, dx in taps], -1)           # [hpb][hd][9]
        db = (g[0] if wrong == 'db_per_window' else g).sum((-2) if wrong == 'db_per_window' else (0, 2))
        if wrong == 'tap_swapped':
            dw = dw.reshape(hpb, hd, 3, 3).transpose(2, 3).reshape(hpb, hd, 9)
        dws.append(dw.reshape(cb, 9))
        dbs.append(db.reshape(cb))
        if only_wgrad:
            continue
        # ---- forward
        S = mm(q * scale, k.transpose(-1, -2))
        if wrong == 'pad_unmasked' and N % 16:
            P = torch.softmax(torch.cat([S, S.new_zeros(S.shape[:-1] + (16 - N % 16,))], -1), -1)[..., :N]
        else:
            P = torch.softmax(S, -1)
        Pk = _bf(P) if mfma else P
        o = mm(Pk, v)
        ao = mm(P, v.abs())
        for dy, dx in taps:
            x = sh(v, dy, dx)
            o = o + wk[..., tapi(dy, dx)] * x
            ao = ao + w[..., tapi(dy, dx)].abs() * x.abs()
        if wrong != 'bias_dropped':
            o = o + bias
        # ---- backward
        dP = mm(g, v.transpose(-1, -2))
        delta = 0.0 if wrong == 'delta_dropped' else (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        dSk = _bf(dS) if mfma else dS
        dq = mm(dSk, k) * scale
        adq = mm(dS.abs(), k.abs()) * scale
        kscale = dict(dk_scale_twice=scale * scale, dk_scale_none=1.0).get(wrong, scale)
        dk = mm(dSk.transpose(-1, -2), q) * kscale
        adk = mm(dS.abs().transpose(-1, -2), q.abs()) * scale
        dv = mm(Pk.transpose(-1, -2), g)
        adv = mm(P.transpose(-1, -2), g.abs())
        for dy, dx in taps:
            x = sh(g, dy, dx) if wrong == 'dv_not_flipped' else sh(g, -dy, -dx)
            dv = dv + wk[..., tapi(dy, dx)] * x
            adv = adv + w[..., tapi(dy, dx)].abs() * x.abs()
        u_ = lambda x: _unwin(x, B, reso, hs, ws)
        out[:, sl], abs_out[:, sl] = u_(o), u_(ao)
        for j, (x, a) in enumerate(((dq, adq), (dk, adk), (dv, adv))):
            c = slice(j * C + br * cb, j * C + (br + 1) * cb)
            dqkv[:, c], abs_dqkv[:, c] = u_(x), u_(a)
    res = dict(dw=torch.stack(dws), db=torch.stack(dbs))
    if not only_wgrad:
        res.update(out=out, dqkv=dqkv, abs_out=abs_out, abs_dqkv=abs_dqkv)
    return res


def zero_scale(i):
    """fallback scale of gate() for dq / dk where they are identically zero (N = 1): scale max|dP| max(|q|, |k|)"""
    case = i['case']
    B, reso, C, heads, nb, cb, hpb, hd = geom(case)
    top = 0.0
    for br in range(nb):
        hs, ws = case[4][br]
        g = _win(i['dout'][:, br * cb:(br + 1) * cb], B, reso, hs, ws, hpb)
        v = _win(i['qkv'][:, 2 * C + br * cb:2 * C + (br + 1) * cb], B, reso, hs, ws, hpb)
        top = max(top, float((g @ v.transpose(-1, -2)).abs().max()))
    return i['scale'] * top * float(i['qkv'][:, :2 * C].abs().max())


def _reference(case, dt, kind, only_wgrad):
    i = make_inputs(case, dt, kind, only_wgrad)
    return dict(dt=dt, inputs=i, exact=evaluate(i, only_wgrad=only_wgrad), zero_scale=0.0 if only_wgrad else zero_scale(i))


_cached = functools.lru_cache(maxsize=None)(_reference)


def reference(case, dt, kind='plain', only_wgrad=False):
    """inputs and the float64 results of one case; computed once and shared: callers must not modify what it returns
    (only_wgrad, the one large case: not kept)"""
    return (_reference if only_wgrad else _cached)(case, dt, kind, only_wgrad)


# ---------------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------------
def gate(got, ref, out_dt, abs_sum=None, zs=0.0):
    """Worst over the elements of |got - ref| / allowed, allowed = r |ref| + 2^-8 abs_sum + 2e-4 max|ref| (module docstring);
    the caller asserts <= 1.  abs_sum = None: the generic form.  Where max|ref| <= 1e-9 zs the floor is 2e-4 zs.  NaN or inf
    in got gives inf."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if top <= 1e-9 * float(zs):
        top = float(zs)
    allowed = (R_BF16 if out_dt == BF else 0.0) * ref.abs() + FLOOR * top
    if abs_sum is not None:
        allowed = allowed + R_BF16 * abs_sum.to(F64)
    err = (got - ref).abs()
    inf = torch.full_like(err, math.inf)
    ratio = torch.where(allowed > 0, err / allowed.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf).max()) if ratio.numel() else 0.0


def gate_all(got, ref, frm):
    """name -> worst ratio for out, dq, dk, dv, dw, db as far as present in `got` (out, dqkv, dw, db); frm 'mfma' / 'generic'"""
    ex, dt = ref['exact'], ref['dt']
    C = ref['inputs']['case'][2]
    res = {}
    if 'out' in got:
        res['out'] = gate(got['out'], ex['out'], dt, ex['abs_out'] if frm == 'mfma' else None)
    if 'dqkv' in got:
        for j, n in enumerate(('dq', 'dk', 'dv')):
            c = slice(j * C, (j + 1) * C)
            res[n] = gate(got['dqkv'][:, c], ex['dqkv'][:, c], dt, ex['abs_dqkv'][:, c] if frm == 'mfma' else None,
                          ref['zero_scale'] if j < 2 else 0.0)
    for n in ('dw', 'db'):
        if n in got:
            res[n] = gate(got[n], ex[n], F32)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_cswin_attn_edges_gpu.py, (B, reso, C, heads, stripes); tests/test_cswin_attn_ref_cpu.py proves
# the closed forms and the reachability of the gate on every one of them
# ---------------------------------------------------------------------------------------------------------------------
def col(p, C=64, heads=2, B=1):
    """column / row stripes of a p x p image: N = p for any p"""
    return (B, p, C, heads, ((p, 1), (1, p)))


def two(reso, hs, ws, C=64, heads=2, B=1):
    return (B, reso, C, heads, ((hs, ws), (ws, hs)))


def one(reso, C=64, heads=2, B=1):
    return (B, reso, C, heads, ((reso, reso),))


# head_dim 32 around the tile counts: NT = 4 up to 64, NT = 7 up to 112, generic above (bf16); 109 / 110: the last N with two
# score planes in the generic backward at head_dim 32 and the first with one
N_HD32 = (one(1, B=2), col(2, B=2), col(15), one(4, B=2), col(17), two(12, 12, 4), one(7), two(21, 21, 3), one(8), two(16, 16, 4),
          col(65), two(12, 12, 6), one(9), col(97), col(109), col(110), two(28, 28, 4), col(113), one(11), two(16, 16, 8))
# generic form at head_dim 8 (C = 16) and 16 (C = 32); head_dim 16: 126 is the last N with two planes, 127 the first with one
N_HD8 = (one(1, 16, B=2), col(17, 16), two(16, 16, 4, 16), two(16, 16, 8, 16))
N_HD16 = (one(1, 32, B=2), col(17, 32), two(16, 16, 4, 32), two(42, 42, 3, 32), col(127, 32), two(16, 16, 8, 32))
KIND_SHAPES = (col(17), one(7), col(65), col(97), col(113))
# work items B * nwin * heads = 9 .. 15 and 20: xcd_walk with a remainder
ITEMS = tuple(one(4, 32, 1, B=b) for b in (9, 10, 11, 12, 13, 14, 15)) + (two(8, 8, 4, B=5),)
HEADS = (two(8, 8, 4, 128, 4), two(8, 8, 4, 192, 6))                    # 2 and 3 heads per branch; C / 8 = 24
STRIDE = two(6, 6, 3, B=2)                                               # N = 18: a ragged tile
BORDERS = (col(17), two(10, 10, 2))                                      # stripes of width 1 and 2
PARTIAL_T = (1, 31, 32, 63, 64, 67, 97, 2049)                            # T = B * nwin of the fused partials' reduce
PARTIALS = tuple(one(4, 32, 1, B=t) for t in PARTIAL_T)
WGRAD_TRIP = (65, 16, 512, 16, ((16, 8), (8, 16)))                       # 16 640 rows > 4 * 4 * 1024: a second grid-stride trip
TWICE = two(14, 14, 7, B=2)


def gated():
    """every (case, kind) the GPU module gates on the attention kernels"""
    s = list(N_HD32) + list(N_HD8) + list(N_HD16) + list(ITEMS) + list(HEADS) + [STRIDE, TWICE] + list(BORDERS) + list(PARTIALS)
    c = {(x, 'plain') for x in s}
    c |= {(x, k) for x in KIND_SHAPES for k in KINDS}
    return sorted(c)
