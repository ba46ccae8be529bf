"""Float64 closed forms of the LayerNorm, LayerNorm+GELU and BatchNorm kernels (csrc/norm.hip, ga_layernorm_gelu_* of csrc/cswin.hip),
the ONE gate the kernel tests hold them to, fp32 restatements of every kernel form in its documented order and roundings, wrong
restatements that the gate has to reject, a pure Python mirror of the form selection, and the case tables shared by
tests/test_norm_ref_cpu.py and tests/test_norm_edges_gpu.py.

The references are explicit sums (no F.layer_norm / F.batch_norm); tensors are [rows][C] float64 (CPU, or the device for the walks),
every input value is exactly representable in the dtype the kernel reads it in; eps is the fp32 value the kernel receives.
    LayerNorm fwd   mean = sum_c x / C, var = sum_c (x - mean)^2 / C, rstd = (var + eps)^-1/2, xhat = (x - mean) rstd, y = xhat w + b
    LayerNorm bwd   xhat from the STORED fp32 mean / rstd (or x itself: x_is_normalized), gw = g w
                    dx = rstd (gw - mean_c gw - xhat mean_c(gw xhat)) + dres;  dw += sum_rows g xhat;  db += sum_rows g
                    dx2 = (dx as stored) * scale2[row // rows_per_scale], rounded to the dtype
    LN+GELU         y = gelu(xhat w + b), erf GELU;  bwd: gz = g gelu'(xhat w + b), then the LayerNorm backward on gz (dw / db from gz)
    bn_finalize     mean = sum / n, var = max(sumsq / n - mean^2, 0), rstd = (var + eps)^-1/2, scale = w rstd, shift = b - mean scale,
                    running = (1 - m) running + m (mean | var n / max(n - 1, 1));  eval: mean / var are the running ones
    affine_act      y = relu?((x scale + shift) rowscale[row // rps] + res)          (the kernel's order: scale, rowscale, residual)
    bn_bwd_reduce   g = dy (y_relu > 0) rowscale;  s1 += sum_rows g;  s2 += sum_rows g xhat,  xhat = (x - mean) rstd
    bn_bwd_apply    dx = w rstd (g - s1 / n - xhat s2 / n),  n given apart from rows
Each function returns, per output element, the absolute sum A of the terms that reach it.

gate(): per element |got - ref| <= r |ref| + u L A, nothing relative to the tensor's maximum.
    r = 2^-8 for an output stored as bf16 (ONE round-to-nearest; a second rounding is not covered), 0 for fp32 outputs.
    u = 2^-24, L = the longest chain of fp32 roundings a term passes through, read from the kernel source:
      LayerNorm forward, K = kMaxCh E values per lane (E = 8 bf16 / 4 fp32), G lanes:
        mean   K in-lane adds + log2 G shuffle adds + the multiply by 1/C                                   K + log2 G + 1
        rstd   (x - mu), its square, the same sum, 1/C, + eps, rsqrt (2 ulp): all relative, halved by the root; below the mean's
        y      (x - mu), rstd, the fma                                                                       3
        An error dmu of the mean reaches y as rstd |w| dmu, a relative error of rstd as |xhat w|: with
            A_y = rstd |w| mean_c|x| + |xhat w| + |b|       L_fwd = K + log2 G + 4
        covers both (A carries the amplification by rstd: on a `flat` row, rstd = eps^-1/2 = 1000, y = b exactly in float64 and the
        kernel's y - b is the rounding of 1/C times 1000 |w|).  A_mean = mean_c|x|.  A_rstd = rstd (1 + rstd^2 u L mean_c|x|^2 / 2):
        the second term is the mean's error squared, which the variance of a flat row consists of.
      LayerNorm backward (mean / rstd are inputs, the stored ones): xhat 2 roundings, gw 1, the fma chains K + log2 G + 1/C,
        xhat s2, two subtractions, rstd, + dres:                                                             L_bwd = K + log2 G + 10
            A_dx = rstd (|gw| + mean_c|gw| + |xhat| mean_c|gw xhat|) + |dres|
        dw / db: a thread adds T = ceil(rows / (grid rpb)) terms, the workgroup's rpb slots meet in LDS, `grid` atomics land on the
        initial value:                                                                                       L_dw = T + rpb + grid + 3
            A_dw = sum_rows |g xhat| + |initial|,  A_db = sum_rows |g| + |initial|
      LayerNorm+GELU (K = 8): gelu through Abramowitz-Stegun 7.1.26, |cdf error| <= 1.5e-7 = 2.6 u, v_rcp, __expf and 8 more
        operations: 12 u |z| on top of |gelu'| <= 1.13 times the error of z:   A_y = 1.13 A_z + |z|,      L = L_fwd + 12
        backward: gelu' is off by 12 u absolutely and by |gelu''| <= 0.8 times the 3 u (|xhat w| + |b|) of z:
            A_gz = |g| (|gelu'| + 1 + |xhat w| + |b|)   and A_dx, A_dw, A_db as above with A_gz for |g|,     L = L_bwd + 12 | L_dw + 12
      bn_finalize: mean 1; var = sumsq / n - mu mu: division, product, subtraction on A_var = sumsq / n + mean^2 (the cancellation of
        the one-pass form is IN this A: at |mean| = 32 std it allows 1024 u of the variance); rstd: A = rstd + rstd^3 A_var / 2;
        scale, shift and the running statistics 3 more:                                                       L = 6
      affine_act: fma, rowscale, residual: A = (|x scale| + |shift|) |rowscale| + |res|,                      L = 3
      bn_bwd_reduce: g 1, (x - mean) rstd g 3, T = ceil(rows / (16 gx)) adds, 16 slots, gx atomics:          L = T + 16 + gx + 5
      bn_bwd_apply: A = w rstd, B = -A rstd s2 / n (1 / n rounded), D = -A s1 / n, g rowscale, two fmas:     L = 9
            A_dx = |w rstd| (|g| + |s1 / n| + |xhat s2 / n|)

Input kinds:
    plain   |values| in [0.5, 2] with random signs: every row, column and sample differs, a read from a neighbour is wrong by O(1)
    offset  rows (LayerNorm) / columns (BatchNorm) around +-32 with a spread of about 1 in steps of 1/4: bf16 values
    flat    constant rows / columns: the variance is 0 (or rounds below it: the clamp), rstd = eps^-1/2
    y_relu holds +0, -0 and negative values on a known mask; scale2 / rowscale are distinct per sample, 0 and 1 among them
"""
import math

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
R_BF16, U = 2.0 ** -8, 2.0 ** -24
EPS6, EPS5 = float(torch.tensor(1e-6, dtype=F32)), float(torch.tensor(1e-5, dtype=F32))


def rnd_to(t, dt):
    return t.to(F32).to(dt).to(F64)


def r_of(dt):
    return R_BF16 if dt == BF else 0.0


def gate(got, ref, A, r, uL):
    """worst err / allowed over the elements of one tensor; inf if an element is off where nothing is allowed (or is NaN)"""
    got, ref, A = got.to(F64), ref.to(F64), A.to(F64)
    err = (got - ref).abs()
    allowed = r * ref.abs() + uL * A
    ratio = torch.where(err > 0, err / allowed, torch.zeros_like(err))
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the form selection of csrc/norm.hip, mirrored (pick_group, nch3 / LN_DISPATCH, grid_blocks, the backward's workgroup cap)
# ------------------------------------------------------------------------------------------------------------------------------
def epc(dt):
    return 8 if dt == BF else 4


def pick_group(C, e, g12=16):
    nch = C // e
    if nch == 12:
        return g12 if g12 in (4, 8, 16, 32, 64) else 16
    g = 4
    while g <= 64:
        if 4 * g >= nch:
            return g
        g <<= 1
    return 64 if nch <= 512 else 0


class Form:
    """the instantiation ln_*_kernel<T, G, AFF, K> that serves (C, dtype) and its launch geometry"""

    def __init__(self, C, dt, g12=16):
        self.C, self.dt, self.E = C, dt, epc(dt)
        self.nch = C // self.E
        self.G = pick_group(C, self.E, g12)
        G, nch = self.G, self.nch
        nch3 = 1 if nch <= G else 2 if nch <= 3 * G else 0 if nch <= 4 * G else 8
        self.K = 1 if (nch3 == 1 and G == 16) else 8 if nch3 == 8 else 3 if nch3 else 4       # chunks per lane (kMaxCh)
        if nch3 == 8:
            assert G == 64
        self.rpb = 256 // G
        self.ragged = nch % G != 0            # lanes hold different numbers of chunks
        self.padded = self.K * G > nch        # zero-filled chunk slots exist

    def key(self):
        return (self.G, self.K)

    def grid_fwd(self, rows):
        return max(1, min(4096, -(-rows // self.rpb)))

    def bwd_cap(self, dw, wgs_knob=0):
        if not dw:
            return 4096
        return max(64, wgs_knob) if wgs_knob > 0 else (1024 if self.C <= 128 else 512)

    def grid_bwd(self, rows, dw, wgs_knob=0):
        return max(1, min(self.bwd_cap(dw, wgs_knob), -(-rows // self.rpb)))

    def trips(self, rows, grid):
        return -(-rows // (grid * self.rpb))

    def lds_bwd(self):
        return 2 * self.rpb * self.C * 4

    def L_fwd(self):
        return self.K * self.E + int(math.log2(self.G)) + 4

    def L_bwd(self):
        return self.K * self.E + int(math.log2(self.G)) + 10

    def L_dw(self, rows, grid):
        return self.trips(rows, grid) + self.rpb + grid + 3

    def __repr__(self):
        return f'G{self.G}xK{self.K}'


def all_forms():
    """every (G, K) LN_DISPATCH can reach over the accepted chunk counts and LN_G12 values (the same for both dtypes)"""
    out = set()
    for nch in range(1, 513):
        for g12 in (4, 8, 16, 32, 64):
            out.add(Form(nch * 8, BF, g12).key())
    return out


def lng_form(C):
    """LayerNorm+GELU: one 8-channel chunk per lane, G = C / 8 lanes, RPB rows per workgroup"""
    G = C // 8
    return G, 256 // G


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _mag(shape, lo, hi, g):
    return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)) * (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1)


SCALES = [0.0, 1.25, 1.0, 0.5, 2.0, 1.5, 0.75, 1.75]


def scales(nsamp):
    """distinct neighbours, 0 and 1 among them"""
    return torch.tensor([SCALES[i % 8] + (i // 8) * 0.125 for i in range(nsamp)], dtype=F64)


def field(rows, C, dt, kind, g, axis):
    """[rows][C] values of dtype dt; axis = 1: the kind applies along a row (LayerNorm), 0: along a column (BatchNorm)"""
    if kind == 'plain':
        return rnd_to(_mag((rows, C), 0.5, 2.0, g), dt)
    shape = (rows, 1) if axis == 1 else (1, C)
    if kind == 'offset':
        base = (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1) * 32
        return base + torch.randint(-4, 5, (rows, C), generator=g).to(F64) / 4          # 30.x .. 34: multiples of 1/4, bf16 values
    assert kind == 'flat'
    return rnd_to(_mag(shape, 0.5, 2.0, g), dt).expand(rows, C).clone()


def ln_inputs(rows, C, dt, kind='plain', seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    i = dict(x=field(rows, C, dt, kind, g, 1), g=rnd_to(_mag((rows, C), 0.5, 2.0, g), dt), dres=rnd_to(_mag((rows, C), 0.5, 2.0, g), dt))
    i['w'] = _mag((C,), 0.5, 1.5, g).to(F32).to(F64)
    i['b'] = _mag((C,), 0.25, 1.0, g).to(F32).to(F64)
    return i


def initial(n, k):
    """known nonzero start of an accumulated gradient (fp32 values)"""
    return (torch.linspace(0.5, 1.5, n, dtype=F64) * (-1.0) ** k).to(F32).to(F64)


def relu_mask_field(rows, C, dt, g):
    """y_relu: positive on a known mask, else exact +0, -0 or a negative value (one third each)"""
    pos = torch.randint(0, 2, (rows, C), generator=g).bool()
    which = torch.randint(0, 3, (rows, C), generator=g)
    mag = rnd_to(0.5 + torch.rand((rows, C), generator=g, dtype=F64), dt)
    y = torch.where(pos, mag, torch.where(which == 2, -mag, torch.zeros_like(mag)))
    y = torch.where(~pos & (which == 1), -torch.zeros_like(mag), y)                   # -0
    return y, pos


def bn_inputs(rows, C, dt, kind='plain', seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    i = dict(x=field(rows, C, dt, kind, g, 0), dy=rnd_to(_mag((rows, C), 0.5, 2.0, g), dt), res=rnd_to(_mag((rows, C), 0.5, 2.0, g), dt))
    i['y_relu'], i['mask'] = relu_mask_field(rows, C, dt, g)
    for n, lo, hi in (('w', 0.5, 1.5), ('b', 0.25, 1.0), ('scale', 0.5, 1.5), ('shift', 0.25, 1.0), ('s1', 0.5, 2.0), ('s2', 0.5, 2.0)):
        i[n] = _mag((C,), lo, hi, g).to(F32).to(F64)
    # per-channel statistics of x as a GEMM epilogue would hand them over (fp32 values): any fp32 value is a valid input
    i['sum'] = i['x'].sum(0).to(F32).to(F64)
    i['sumsq'] = (i['x'] * i['x']).sum(0).to(F32).to(F64)
    i['rmean'] = _mag((C,), 0.25, 1.0, g).to(F32).to(F64)
    i['rvar'] = (0.5 + torch.rand((C,), generator=g, dtype=F64)).to(F32).to(F64)
    return i


# ------------------------------------------------------------------------------------------------------------------------------
# float64 closed forms
# ------------------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, w=None, b=None, eps=EPS6, uL=0.0):
    """dict of (ref, A) for mean, rstd, xhat, y"""
    C = x.shape[1]
    mean = x.sum(1) / C
    d = x - mean[:, None]
    var = (d * d).sum(1) / C
    rstd = (var + eps) ** -0.5
    xhat = d * rstd[:, None]
    ax = x.abs().sum(1) / C
    z = xhat if w is None else xhat * w
    A = rstd[:, None] * ax[:, None] * (1.0 if w is None else w.abs()) + z.abs() + (0.0 if b is None else b.abs())
    y = z if b is None else z + b
    return dict(mean=(mean, ax), rstd=(rstd, rstd * (1 + 0.5 * rstd * rstd * uL * ax * ax)), xhat=(xhat, None), y=(y, A))


def _xhat(x, mean, rstd, xnorm):
    return x if xnorm else (x - mean[:, None]) * rstd[:, None]


def ln_bwd(g, x, mean, rstd, w=None, dres=None, xnorm=False, Ag=None):
    """dx, A_dx, dw, A_dw, db, A_db (the sums only, without an initial value).  Ag: the magnitude standing in for |g| (LN+GELU)"""
    C = x.shape[1]
    xh = _xhat(x, mean, rstd, xnorm)
    gw = g if w is None else g * w
    Ag = g.abs() if Ag is None else Ag
    agw = Ag if w is None else Ag * w.abs()
    s1 = gw.sum(1, keepdim=True) / C
    s2 = (gw * xh).sum(1, keepdim=True) / C
    rs = rstd[:, None]
    dx = rs * (gw - s1 - xh * s2)
    A = rs * (agw + agw.sum(1, keepdim=True) / C + xh.abs() * (agw * xh.abs()).sum(1, keepdim=True) / C)
    if dres is not None:
        dx, A = dx + dres, A + dres.abs()
    return dx, A, (g * xh).sum(0), (Ag * xh.abs()).sum(0), g.sum(0), Ag.sum(0)


def second_output(dx_stored, scale2, rps, dt):
    """dx2 = (dx as stored) * scale2[row // rps]: ONE fp32 product, rounded to dt; torch reproduces it bit for bit"""
    rows = dx_stored.shape[0]
    idx = torch.arange(rows, device=dx_stored.device) // rps
    return (dx_stored.to(F32) * scale2.to(F32).to(dx_stored.device)[idx][:, None]).to(dt)


def gelu64(z):
    return z * 0.5 * (1 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad64(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def lng_fwd(x, w, b, eps=EPS6, uL=0.0):
    f = ln_fwd(x, w, b, eps, uL)
    z, Az = f['y']
    f['y'] = (gelu64(z), 1.13 * Az + z.abs())
    return f


def lng_bwd(g, x, mean, rstd, w, b):
    xh = _xhat(x, mean, rstd, False)
    z = xh * w + b
    gp = gelu_grad64(z)
    Agz = g.abs() * (gp.abs() + 1 + (xh * w).abs() + b.abs())
    return ln_bwd(g * gp, x, mean, rstd, w, None, False, Ag=Agz)


def bn_finalize(s, ssq, n, w, b, eps, momentum, rmean, rvar, training=True):
    """dict of (ref, A): mean, rstd, scale, shift, rmean, rvar (the running ones None when not given or in eval)"""
    out = {}
    if training:
        mean = s / n
        raw = ssq / n - mean * mean
        var = raw.clamp(min=0)
        Avar = ssq / n + mean * mean
        if rmean is not None:
            unb = n / max(n - 1.0, 1.0)
            out['rmean'] = ((1 - momentum) * rmean + momentum * mean, ((1 - momentum) * rmean).abs() + (momentum * mean).abs())
            out['rvar'] = ((1 - momentum) * rvar + momentum * var * unb, ((1 - momentum) * rvar).abs() + momentum * unb * Avar)
    else:
        mean, var, Avar = rmean, rvar, rvar.abs()
    rstd = (var + eps) ** -0.5
    Ars = rstd + 0.5 * rstd ** 3 * Avar
    ww = torch.ones_like(mean) if w is None else w
    bb = torch.zeros_like(mean) if b is None else b
    scale = ww * rstd
    out.update(mean=(mean, mean.abs()), rstd=(rstd, Ars), scale=(scale, ww.abs() * Ars),
               shift=(bb - mean * scale, bb.abs() + mean.abs() * ww.abs() * Ars))
    return out


def _rowscale(rows, rowscale, rps, like):
    if rowscale is None:
        return torch.ones(rows, 1, dtype=F64, device=like.device)
    return rowscale.to(like.device)[torch.arange(rows, device=like.device) // rps][:, None]


def affine_act(x, scale=None, shift=None, res=None, rowscale=None, rps=1, relu=False):
    rsc = _rowscale(x.shape[0], rowscale, rps, x)
    t = x if scale is None else x * scale + shift
    A = (x.abs() if scale is None else (x * scale).abs() + shift.abs()) * rsc.abs()
    t = t * rsc
    if res is not None:
        t, A = t + res, A + res.abs()
    return (t.clamp(min=0) if relu else t), A


def _bn_g(dy, y_relu, rowscale, rps, ge=False):
    g = dy if y_relu is None else dy * ((y_relu >= 0) if ge else (y_relu > 0)).to(F64)
    return g * _rowscale(dy.shape[0], rowscale, rps, dy)


def bn_bwd_reduce(dy, x, mean, rstd, y_relu=None, rowscale=None, rps=1):
    """s1, A1, s2, A2 (the sums only)"""
    g = _bn_g(dy, y_relu, rowscale, rps)
    xh = (x - mean) * rstd
    return g.sum(0), g.abs().sum(0), (g * xh).sum(0), (g * xh).abs().sum(0)


def bn_bwd_apply(dy, x, mean, rstd, w, s1, s2, n, y_relu=None, rowscale=None, rps=1):
    g = _bn_g(dy, y_relu, rowscale, rps)
    xh = (x - mean) * rstd
    a = rstd if w is None else w * rstd
    return a * (g - s1 / n - xh * s2 / n), a.abs() * (g.abs() + (s1 / n).abs() + (xh * s2 / n).abs())


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 restatements in kernel order (CPU), right and wrong
# ------------------------------------------------------------------------------------------------------------------------------
def f32(t):
    return t.to(F32)


def fma(a, b, c):
    """fp32 a * b + c with one rounding (the product of two fp32 values is exact in float64)"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _lanes(t, fm):
    """[rows][C] -> [rows][K][G][E]: chunk ci = lg + G j sits in lane lg, slot j; the slots past nch are zero-filled"""
    rows = t.shape[0]
    pad = fm.K * fm.G * fm.E - fm.C
    return torch.nn.functional.pad(f32(t), (0, pad)).view(rows, fm.K, fm.G, fm.E)


def _unlanes(t, fm):
    return t.reshape(t.shape[0], -1)[:, :fm.C]


def _live(fm):
    """[K][G][1] mask of the chunk slots with ci < nch"""
    ci = torch.arange(fm.K)[:, None] * fm.G + torch.arange(fm.G)[None, :]
    return (ci < fm.nch)[:, :, None]


def _lane_sum(v, fm):
    """in-lane sum over (j, e) in order, then the xor butterfly over the G lanes: [rows][K][G][E] -> [rows][G] (all lanes equal)"""
    s = torch.zeros(v.shape[0], fm.G, dtype=F32)
    for j in range(fm.K):
        for e in range(fm.E):
            s = s + v[:, j, :, e]
    return _butterfly(s, fm.G)


def _butterfly(s, G):
    o = G // 2
    idx = torch.arange(G)
    while o > 0:
        s = s + s[:, idx ^ o]
        o >>= 1
    return s


def _rsqrt(t):
    return (t.to(F64) ** -0.5).to(F32)


def ln_fwd_as(x, w, b, eps, fm, dt, wrong=None):
    """mean, rstd (fp32 as float64) and y (values of dt) as ln_fwd_kernel<T, G, AFF, K> computes them"""
    v = _lanes(x, fm)
    live = _live(fm)
    invC = f32(torch.tensor(1.0 / (fm.K * fm.G * fm.E if wrong == 'padded_mean' else fm.C)))
    invV = f32(torch.tensor(1.0 / (fm.C - 1))) if wrong == 'c_minus_1' else invC
    epsf = f32(torch.tensor(1e-5 if wrong == 'eps_1e5' else eps))
    mu = _lane_sum(v, fm) * invC                                 # [rows][G]
    if wrong == 'one_pass':
        q2 = torch.zeros(v.shape[0], fm.G, dtype=F32)
        for j in range(fm.K):
            for e in range(fm.E):
                q2 = fma(v[:, j, :, e], v[:, j, :, e], q2)
        var = _butterfly(q2, fm.G) * invC - mu * mu
    else:
        dlt = v - mu[:, None, :, None]
        sq = dlt * dlt
        if wrong != 'no_guard':
            sq = torch.where(live, sq, torch.zeros_like(sq))
        q = torch.zeros(v.shape[0], fm.G, dtype=F32)
        for j in range(fm.K):
            for e in range(fm.E):
                q = q + sq[:, j, :, e]
        var = _butterfly(q, fm.G) * invV
    rs = f32(1.0 / (var.to(F64).clamp(min=0).sqrt() + float(epsf))) if wrong == 'eps_outside' else _rsqrt(var + epsf)
    o = (v - mu[:, None, :, None]) * rs[:, None, :, None]
    if w is not None:
        o = fma(o, _lanes(w[None], fm), _lanes(b[None], fm))
    return mu[:, 0].to(F64), rs[:, 0].to(F64), _unlanes(o, fm).to(dt).to(F64)


def _scale2_index(rows, rps, wrong):
    r = torch.arange(rows)
    if wrong == 'scale2_mod':
        return r % rps
    idx = r // rps
    if wrong == 'scale2_neighbour':                          # the last row of a sample takes the next sample's factor
        nxt = torch.clamp(idx + 1, max=int(idx.max()))
        idx = torch.where(r % rps == rps - 1, nxt, idx)
    return idx


def ln_bwd_as(g, x, mean, rstd, w, dres, xnorm, fm, dt, dw0=None, db0=None, grid=None, scale2=None, rps=1, wrong=None):
    """dx (values of dt), dx2 (or None), dw, db (fp32 as float64, or None) as ln_bwd_kernel<T, G, AFF, K> computes them"""
    rows = x.shape[0]
    live = _live(fm)
    gv, xv = _lanes(g, fm), _lanes(x, fm)
    rs = f32(rstd)[:, None, None, None]
    mu = torch.zeros_like(rs) if xnorm else f32(mean)[:, None, None, None]
    sc = torch.ones_like(rs) if xnorm else rs
    xh = torch.where(live, (xv - mu) * sc, torch.zeros_like(xv))
    graw = gv
    wl = _lanes(w[None], fm) if w is not None else None
    gwv = gv * wl if w is not None else gv
    invC = f32(torch.tensor(1.0 / fm.C))
    s1 = torch.zeros(rows, fm.G, dtype=F32)
    s2 = torch.zeros(rows, fm.G, dtype=F32)
    s1src = graw if wrong == 's1_from_g' else gwv
    for j in range(fm.K):
        for e in range(fm.E):
            s1 = s1 + s1src[:, j, :, e]
            s2 = fma(gwv[:, j, :, e], xh[:, j, :, e], s2)
    s1 = (_butterfly(s1, fm.G) * invC)[:, None, :, None]
    s2 = (_butterfly(s2, fm.G) * invC)[:, None, :, None]
    if wrong == 'no_s2':
        s2 = torch.zeros_like(s2)
    o = _lanes(dres, fm) if dres is not None else torch.zeros_like(gv)
    if wrong == 'dres_before_rstd':
        o = rs * (o + (gwv - s1 - xh * s2))
    else:
        o = o + rs * (gwv - s1 - xh * s2)
    dx32 = _unlanes(o, fm)
    dx = dx32.to(dt)
    dx2 = None
    if scale2 is not None:
        src = dx32 if wrong == 'dx2_unrounded' else dx.to(F32)
        dx2 = (src * f32(scale2)[_scale2_index(rows, rps, wrong)][:, None]).to(dt).to(F64)
    dw = db = None
    if dw0 is not None:
        grid = grid or fm.grid_bwd(rows, True)
        T = fm.trips(rows, grid)
        per = grid * fm.rpb
        gx = _unlanes(graw, fm)
        xs = f32(x) if wrong == 'dw_from_x' else _unlanes(xh, fm)
        pad = T * per - rows
        gx = torch.nn.functional.pad(gx, (0, 0, 0, pad)).view(T, grid, fm.rpb, fm.C)
        xs = torch.nn.functional.pad(xs, (0, 0, 0, pad)).view(T, grid, fm.rpb, fm.C)
        if wrong == 'drop_last_row':
            gx = gx.clone()
            gx.view(-1, fm.C)[rows - 1] = 0
        aw = torch.zeros(grid, fm.rpb, fm.C, dtype=F32)
        ab = torch.zeros(grid, fm.rpb, fm.C, dtype=F32)
        for k in range(T):
            aw = fma(gx[k], xs[k], aw)
            ab = ab + gx[k]
        pw = torch.zeros(grid, fm.C, dtype=F32)
        pb = torch.zeros(grid, fm.C, dtype=F32)
        for r in range(fm.rpb):
            pw, pb = pw + aw[:, r], pb + ab[:, r]
        dwv, dbv = f32(dw0).clone(), f32(db0).clone()
        for k in range(grid):                                    # the atomics, in some order
            dwv, dbv = dwv + pw[k], dbv + pb[k]
        dw, db = dwv.to(F64), dbv.to(F64)
    return dx.to(F64), dx2, dw, db


def _gelu_cdf32(x):
    """gelu_cdf_f of csrc/common.h in fp32 (v_rcp and __expf stood in for by correctly rounded ones)"""
    c = lambda v: f32(torch.tensor(v))
    z = x.abs() * c(0.70710678118654752)
    t = f32(1.0 / fma(c(0.3275911), z, c(1.0)).to(F64))
    p = fma(t, c(1.061405429), c(-1.453152027))
    for k in (1.421413741, -0.284496736, 0.254829592):
        p = fma(p, t, c(k))
    e = f32(torch.exp((-z * z).to(F64)))
    half = c(0.5) * p * t * e
    return torch.where(x >= 0, 1.0 - half, half), e


def lng_fwd_as(x, w, b, eps, dt):
    C = x.shape[1]
    fm = Form(C, BF)              # (only its lane layout is used: one 8-channel chunk per lane)
    fm.G, fm.K, fm.E, fm.nch, fm.rpb = C // 8, 1, 8, C // 8, 256 // (C // 8)
    v = _lanes(x, fm)
    invC = f32(torch.tensor(1.0 / C))
    mu = _lane_sum(v, fm) * invC
    dlt = v - mu[:, None, :, None]
    rs = _rsqrt(_lane_sum(dlt * dlt, fm) * invC + f32(torch.tensor(eps)))
    z = fma(dlt * rs[:, None, :, None], _lanes(w[None], fm), _lanes(b[None], fm))
    y = z * _gelu_cdf32(z)[0]
    return mu[:, 0].to(F64), rs[:, 0].to(F64), _unlanes(y, fm).to(dt).to(F64)


def lng_bwd_as(g, x, mean, rstd, w, b, dt, dw0, db0, grid):
    C = x.shape[1]
    fm = Form(C, BF)
    fm.G, fm.K, fm.E, fm.nch, fm.rpb = C // 8, 1, 8, C // 8, 256 // (C // 8)
    xh = (f32(x) - f32(mean)[:, None]) * f32(rstd)[:, None]
    z = fma(xh, f32(w)[None], f32(b)[None])
    cdf, e = _gelu_cdf32(z)
    gp = fma(z * f32(torch.tensor(0.3989422804014327)), e, cdf)
    gz = f32(g) * gp
    return ln_bwd_as(gz.to(F64), x, mean, rstd, w, None, False, fm, dt, dw0, db0, grid)


def bn_finalize_as(s, ssq, n, w, b, eps, momentum, rmean, rvar, training=True, wrong=None):
    """bn_finalize_kernel in fp32; also returns the variance BEFORE the clamp (to show that a case reaches it)"""
    c = lambda v: f32(torch.tensor(float(v)))
    out = {}
    raw = None
    if training:
        mu = f32(s) / c(n)
        raw = f32(ssq) / c(n) - mu * mu
        var = raw.clamp(min=0)
        if rmean is not None:
            unb = c(1.0) if wrong == 'biased_running' else c(n) / torch.maximum(c(n) - 1.0, c(1.0))
            out['rmean'] = (c(1.0) - c(momentum)) * f32(rmean) + c(momentum) * mu
            out['rvar'] = (c(1.0) - c(momentum)) * f32(rvar) + c(momentum) * var * unb
        if wrong == 'unbiased_rstd':
            var = var * (c(n) / torch.maximum(c(n) - 1.0, c(1.0)))
    else:
        mu, var = f32(rmean), f32(rvar)
    rs = _rsqrt(var + c(eps))
    a = (f32(w) if w is not None else 1.0) * rs
    out.update(mean=mu, rstd=rs, scale=a, shift=(f32(b) if b is not None else 0.0) - mu * a)
    return {k: v.to(F64) for k, v in out.items()}, raw


def affine_act_as(x, scale, shift, res, rowscale, rps, relu, dt, wrong=None):
    rsc = f32(_rowscale(x.shape[0], rowscale, rps, x))
    t = f32(x)
    if scale is not None:
        t = fma(t, f32(scale), f32(shift))
    if wrong == 'res_scaled':
        t = (t + f32(res)) * rsc
    else:
        t = t * rsc
        if res is not None:
            t = t + f32(res)
    if relu:
        t = t.clamp(min=0)
    return t.to(dt).to(F64)


def bn_reduce_grid(rows, C):
    slices = -(-C // 64)
    return max(1, min((rows + 15) // 16, max(1, 1024 // slices))), slices


def bn_bwd_reduce_as(dy, x, mean, rstd, y_relu, rowscale, rps, s10, s20, wrong=None):
    rows, C = x.shape
    gx, _ = bn_reduce_grid(rows, C)
    g = f32(dy)
    if y_relu is not None:
        g = torch.where((y_relu >= 0) if wrong == 'ge_mask' else (y_relu > 0), g, torch.zeros_like(g))
    if rowscale is not None:
        g = g * f32(_rowscale(rows, rowscale, rps, x))
    t2 = g * (f32(x) - f32(mean)) * f32(rstd)
    T = -(-rows // (gx * 16))
    pad = T * gx * 16 - rows
    g = torch.nn.functional.pad(g, (0, 0, 0, pad)).view(T, gx, 16, C)
    t2 = torch.nn.functional.pad(t2, (0, 0, 0, pad)).view(T, gx, 16, C)
    a1 = torch.zeros(gx, 16, C, dtype=F32)
    a2 = torch.zeros(gx, 16, C, dtype=F32)
    for k in range(T):
        a1, a2 = a1 + g[k], a2 + t2[k]
    p1 = torch.zeros(gx, C, dtype=F32)
    p2 = torch.zeros(gx, C, dtype=F32)
    for r in range(16):
        p1, p2 = p1 + a1[:, r], p2 + a2[:, r]
    s1, s2 = f32(s10).clone(), f32(s20).clone()
    for k in range(gx):
        s1, s2 = s1 + p1[k], s2 + p2[k]
    return s1.to(F64), s2.to(F64)


def bn_bwd_apply_as(dy, x, mean, rstd, w, s1, s2, n, y_relu, rowscale, rps, dt, wrong=None):
    rows = x.shape[0]
    inv_n = f32(torch.tensor(1.0)) / f32(torch.tensor(float(rows if wrong == 'rows_for_n' else n)))
    rs = f32(rstd)
    A = (f32(w) if w is not None else 1.0) * rs
    Bc = -A * rs * f32(s2) * inv_n
    D = -A * f32(s1) * inv_n
    gg = f32(dy) * f32(_rowscale(rows, rowscale, rps, x))
    if y_relu is not None:
        gg = torch.where((y_relu >= 0) if wrong == 'ge_mask' else (y_relu > 0), gg, torch.zeros_like(gg))
    xc = f32(x) if wrong == 'B_x' else f32(x) - f32(mean)
    return fma(A.expand_as(gg), gg, fma(Bc.expand_as(gg), xc, D.expand_as(gg))).to(dt).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------
# the case tables
# ------------------------------------------------------------------------------------------------------------------------------
class LnCase:
    """(dtype, C, LN_G12) with the form the mirror expects; `reaches` names what the case is in the table for"""

    def __init__(self, dt, C, g12=16, reaches=''):
        self.dt, self.C, self.g12, self.reaches = dt, C, g12, reaches
        self.form = Form(C, dt, g12)

    def rows(self):
        r = self.form.rpb
        return sorted({1, r - 1, r, r + 1} - {0})

    def __repr__(self):
        return f'{"bf16" if self.dt == BF else "fp32"}-C{self.C}' + (f'-g12_{self.g12}' if self.g12 != 16 else '')


LN_CASES = [
    LnCase(BF, 8, reaches='nch = 1, G = 4'), LnCase(BF, 16), LnCase(BF, 96, reaches='G = 16, one chunk'),
    LnCase(BF, 96, 4, reaches='G = 4, three chunks'), LnCase(BF, 104, reaches='nch = 13, ragged 4-chunk'), LnCase(BF, 128),
    LnCase(BF, 192), LnCase(BF, 200, reaches='nch = 25, ragged G = 8 x 4'), LnCase(BF, 384), LnCase(BF, 392, reaches='nch = 49, ragged G = 16 x 4'),
    LnCase(BF, 768), LnCase(BF, 1024, reaches='G = 32, 4 chunks; 65,536 B of LDS with dw'), LnCase(BF, 1536), LnCase(BF, 2048),
    LnCase(BF, 2056, reaches='nch = 257, ragged 8-chunk'), LnCase(BF, 4096, reaches='full 8-chunk'),
    LnCase(F32, 4), LnCase(F32, 48, reaches='one-chunk G = 16'), LnCase(F32, 48, 4), LnCase(F32, 52), LnCase(F32, 68), LnCase(F32, 100),
    LnCase(F32, 132), LnCase(F32, 196), LnCase(F32, 260), LnCase(F32, 388), LnCase(F32, 516), LnCase(F32, 1024),
    LnCase(F32, 1536, reaches='the map_pit_s NormHead'), LnCase(F32, 2048, reaches='65,536 B of LDS with dw'),
]
LN_SMALL = [c for c in LN_CASES if c.C <= 392]            # the cases the CPU restatements run on
AFF_VARIANTS = ('none', 'w', 'all', 'dwdb')              # (w, dw, db): none | w only | all three | dw + db without w
RPS = (1, 3, 49, 197)
LDS_PLAIN = 65536


def dw_served(form):
    """parameter gradients are served up to 64 KB of LDS for the reduce (bf16 C in (2048, 4096] is refused)"""
    return form.lds_bwd() <= LDS_PLAIN


LNG_C = (8, 32, 512)
BN_FINALIZE_C = (1, 127, 128, 129, 2048)
BN_APPLY_C = (8, 72, 2048)
BN_REDUCE_C = (4, 64, 68, 200, 2048)
