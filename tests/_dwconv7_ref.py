"""Float64 closed forms of the depthwise 7x7 convolution (pad 3, stride 1, NHWC) and of its two gradients, the ONE gate the kernel
tests hold csrc/dwconv.hip to, fp32 restatements of every kernel form in its documented order and roundings, wrong restatements that
the gate has to reject, and the case tables shared by tests/test_dwconv7_ref_cpu.py and tests/test_dwconv7_edges_gpu.py.

The reference is written as explicit shifted sums over the 49 taps (no conv2d: it cannot share a padding or flipping convention
with a library).  Tensors are [B][H][W][C] float64 on the CPU, w49 is [49][C] (tap = ky * 7 + kx), every input value is exactly
representable in the dtype the kernel reads it in.
    fwd         y[b,oy,ox,c]  = bias[c] + sum_{ky,kx} w[ky,kx,c] x[b,oy+ky-3,ox+kx-3,c]          (zero outside the image)
    bwd_data    dx[b,iy,ix,c] = res[b,iy,ix,c] + sum_{ky,kx} w[ky,kx,c] dy[b,iy-(ky-3),ix-(kx-3),c]
                dx2           = (dx as stored) * scale2[b], rounded to the dtype
    bwd_weight  dw49[ky*7+kx,c] += sum_{b,oy,ox} dy[b,oy,ox,c] x[b,oy+ky-3,ox+kx-3,c];   dbias[c] += sum dy[b,oy,ox,c]
Each function also returns, per output element, the absolute sum A of its terms (|bias|, |res| and every |w x| or |dy x|).

gate(): per element  |got - ref| <= r |ref| + (u + w) A,  nothing relative to the tensor's maximum.
    r = 2^-8 for an output stored as bf16: ONE round-to-nearest, whose half ulp is 2^-8 of a value just above a power of two (an
        element whose fp32 value falls to the other side of a rounding boundary than the exact one stays inside r |ref| + u A);
        0 for fp32 outputs (dw49 / dbias always).  A second rounding of any part of the sum is not covered.
    w = 2^-9 for the forms that round the taps to bf16 (dot2 forward / backward-data, MFMA) on taps that are not bf16 values
        (kind `rough` only): every product is off by at most 2^-9 of itself; 0 otherwise
    u = 2^-24 L, L = the number of fp32 roundings a term can pass through on its way to the result in the form that ran, i.e. the
        longest accumulation chain.  From the kernel source:
        forward / backward-data
          scalar, rs    acc = bias, 49 fused multiply-adds in (ky, kx) order (rs: the input rows arrive in ky order), + res: L = 50
          dot2          28 v_dot2_f32_bf16 per element (four per tap row, the last with a zero tap), at most two roundings each,
                        + res: L = 57
          mfma          7 chained 16x16x32 MFMAs, 7 nonzero products each (zeros add nothing), + the accumulate: L = 7 * 8 + 1 = 57
        backward-weight: t = terms one lane adds into one accumulator, then the partials
          rs            t = 4 R ceil(units / (4 nbw)) (4 columns of the strip, R rows of the unit, the units the wave walks), + 2
                        (the four waves meet in LDS), + nstrips * ceil(nbw / 16) (a reduce group's chain), + 16 groups, + 1 (+=)
          dot2          t = 2 * 7 * NP * ceil(tiles / gx) (NP = 4 | 7 pixel pairs per row, 7 rows of the wave's row group),
                        + 1 (14x14: the two row groups meet in LDS), + ceil(parts / 16) + 16 + 1
          scalar        t = 7 * TW * ceil(tiles / gx) (7 rows, TW = 7 | 14 columns), + ceil(parts / 16) + 16 + 1
        (chain_fwd / chain_wgrad below parse the form name the library reports.)

Input kinds:
    plain    |x|, |dy|, |res| in [0.5, 2] with random signs, taps with |w| in [0.25, 1] that are bf16 values: a single missing, doubled
             or misplaced term moves its element by at least 0.125, far beyond the gate; w = 0 for every form
    rough    the same tensors with fp32 randn taps (not bf16 values): the only kind with w > 0; pins which forms round the taps
    impulse  (the GPU module) one hot pixel per channel, results bit-exact
Every image, row, column and channel carries its own random values, so a read from a neighbour is wrong by O(1).
"""
import re

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
R_BF16, W_TAPS, U = 2.0 ** -8, 2.0 ** -9, 2.0 ** -24


def rnd_to(t, dt):
    """the values of float64 `t` rounded to dtype dt, as float64"""
    return t.to(F32).to(dt).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _mag(shape, lo, hi, g):
    return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)) * (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1)


def make_inputs(geom, dt, kind='plain', seed=0):
    B, H, W, C = geom
    g = torch.Generator().manual_seed(1000 + seed)
    i = {n: rnd_to(_mag((B, H, W, C), 0.5, 2.0, g), dt) for n in ('x', 'dy', 'res')}
    if kind == 'rough':
        i['w49'] = torch.randn(49, C, generator=g, dtype=F32).to(F64)
        assert not torch.equal(rnd_to(i['w49'], BF), i['w49'])
    else:
        i['w49'] = rnd_to(_mag((49, C), 0.25, 1.0, g), BF)
    i['bias'] = _mag((C,), 0.25, 1.0, g).to(F32).to(F64)
    i['scale2'] = torch.tensor(([0.0, 1.25, 2.0, 1.0, 0.5, 1.5] * (B // 6 + 1))[:B], dtype=F64)
    return i


def initial(n, k):
    """known nonzero start of an accumulated gradient (fp32 values)"""
    return (torch.linspace(0.5, 1.5, n, dtype=F64) * (-1.0) ** k).to(F32).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------
# float64 closed forms
# ------------------------------------------------------------------------------------------------------------------------------
def _ranges(n, d):
    """output range [a, b) whose source index o + d lies in [0, n)"""
    return max(0, -d), min(n, n - d)


def fwd(x, w49, bias=None):
    """y, A"""
    B, H, W, C = x.shape
    y = torch.zeros_like(x) if bias is None else bias.expand(B, H, W, C).clone()
    A = y.abs()
    ax, aw = x.abs(), w49.abs()
    for ky in range(7):
        y0, y1 = _ranges(H, ky - 3)
        for kx in range(7):
            x0, x1 = _ranges(W, kx - 3)
            if y0 >= y1 or x0 >= x1:
                continue
            t = ky * 7 + kx
            src = (slice(None), slice(y0 + ky - 3, y1 + ky - 3), slice(x0 + kx - 3, x1 + kx - 3))
            y[:, y0:y1, x0:x1] += w49[t] * x[src]
            A[:, y0:y1, x0:x1] += aw[t] * ax[src]
    return y, A


def bwd_data(dy, w49, res=None):
    """dx, A:  dx[i] = res[i] + sum_k w[k] dy[i - (k - 3)]"""
    B, H, W, C = dy.shape
    dx = torch.zeros_like(dy) if res is None else res.clone()
    A = dx.abs()
    ad, aw = dy.abs(), w49.abs()
    for ky in range(7):
        y0, y1 = _ranges(H, 3 - ky)
        for kx in range(7):
            x0, x1 = _ranges(W, 3 - kx)
            if y0 >= y1 or x0 >= x1:
                continue
            t = ky * 7 + kx
            src = (slice(None), slice(y0 + 3 - ky, y1 + 3 - ky), slice(x0 + 3 - kx, x1 + 3 - kx))
            dx[:, y0:y1, x0:x1] += w49[t] * dy[src]
            A[:, y0:y1, x0:x1] += aw[t] * ad[src]
    return dx, A


def second_output(dx_stored, scale2, dt):
    """dx2 = (dx as stored) * scale2[img] in fp32, rounded to dt: the product of an fp32 multiply, which torch reproduces bit for bit"""
    return (dx_stored.to(F32) * scale2.to(F32).view(-1, 1, 1, 1)).to(dt)


def bwd_weight(dy, x, rows=None):
    """dw49 [49][C], A_w, dbias [C], A_b of the images (all) and the output rows `rows` = (lo, hi) (all)"""
    B, H, W, C = x.shape
    lo, hi = rows or (0, H)
    dw, Aw = torch.zeros(49, C, dtype=x.dtype, device=x.device), torch.zeros(49, C, dtype=x.dtype, device=x.device)
    for ky in range(7):
        y0, y1 = _ranges(H, ky - 3)
        y0, y1 = max(y0, lo), min(y1, hi)
        for kx in range(7):
            x0, x1 = _ranges(W, kx - 3)
            if y0 >= y1 or x0 >= x1:
                continue
            p = dy[:, y0:y1, x0:x1] * x[:, y0 + ky - 3:y1 + ky - 3, x0 + kx - 3:x1 + kx - 3]
            dw[ky * 7 + kx] = p.sum((0, 1, 2))
            Aw[ky * 7 + kx] = p.abs().sum((0, 1, 2))
    return dw, Aw, dy[:, lo:hi].sum((0, 1, 2)), dy[:, lo:hi].abs().sum((0, 1, 2))


# ------------------------------------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------------------------------------
def chain_fwd(form):
    fam = form.split(':')[0].split('+')[0]
    return {'rs': 50, 'scalar_7x7': 50, 'scalar_14x14': 50, 'dot2_7x7': 57, 'dot2_14x14': 57, 'mfma': 57}[fam]


def rounds_taps(form):
    return form.startswith(('dot2', 'mfma'))


def _cdiv(a, b):
    return -(-a // b)


def chain_wgrad(form, B, H, W):
    fam = form.split(':')[0]
    num = {k: int(v) for k, v in re.findall(r'([A-Za-z]+)(\d+)', form.split(':', 1)[1].split('+')[0])}
    if fam == 'rs':
        units = B * num['seg']
        return 4 * num['R'] * _cdiv(units, 4 * num['nbw']) + 2 + _cdiv(W, 4) * _cdiv(num['nbw'], 16) + 16 + 1
    big = fam.endswith('14x14')
    tiles = B * (H // 14) * (W // 14) if big else B * _cdiv(H, 7) * _cdiv(W, 7)
    parts = num['parts']
    if fam.startswith('dot2'):
        return 2 * 7 * (7 if big else 4) * _cdiv(tiles, parts) + (1 if big else 0) + _cdiv(parts, 16) + 16 + 1
    gx = parts // 2 if big else parts
    return 7 * (14 if big else 7) * _cdiv(tiles, gx) + _cdiv(parts, 16) + 16 + 1


def gate(got, ref, A, r, u, w=0.0):
    """worst err / allowed over the elements of one tensor (float64 CPU tensors); inf if an element is off where nothing is allowed"""
    err = (got - ref).abs()
    allowed = r * ref.abs() + (u + w) * A
    ratio = torch.where(err > 0, err / allowed, torch.zeros_like(err))      # 0 / 0 = 0, x / 0 = inf
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    return float(ratio.max()) if ratio.numel() else 0.0


def gate_conv(got, ref, A, dt, form, kind):
    return gate(got, ref, A, R_BF16 if dt == BF else 0.0, U * chain_fwd(form), W_TAPS if kind == 'rough' and rounds_taps(form) else 0.0)


def gate_wgrad(got, ref, A, form, geom):
    return gate(got, ref, A, 0.0, U * chain_wgrad(form, geom[0], geom[1], geom[2]))


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the forms (the documented order and roundings), for tests/test_dwconv7_ref_cpu.py
# ------------------------------------------------------------------------------------------------------------------------------
def _fma(acc, p):
    """fp32 acc + exact products p (float64), rounded once"""
    return (acc.to(F64) + p).to(F32)


def _gather(x, dy, dx, mode='zero'):
    """x[b, y + dy, x + dx] for every output pixel; outside the image: zero | clamp | the flat neighbour (wrap_row: the column
    overflows into the next / previous row of the image; wrap_img: the row overflows into the next / previous image)"""
    B, H, W, C = x.shape
    yy, xx = torch.arange(H) + dy, torch.arange(W) + dx
    if mode == 'zero':
        return torch.nn.functional.pad(x, (0, 0, 3, 3, 3, 3))[:, 3 + dy:3 + dy + H, 3 + dx:3 + dx + W]
    if mode == 'clamp':
        return x[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]
    if mode == 'wrap_row':
        p = (yy[:, None] * W + xx[None, :]).reshape(-1)
        ok = ((p >= 0) & (p < H * W)).to(x.dtype)
        return (x.reshape(B, H * W, C)[:, p.clamp(0, H * W - 1)] * ok[None, :, None]).reshape(B, H, W, C)
    assert mode == 'wrap_img'
    okx = ((xx >= 0) & (xx < W)).to(x.dtype)
    g = (torch.arange(B)[:, None] * H + yy[None, :]).reshape(-1)
    ok = ((g >= 0) & (g < B * H)).to(x.dtype)
    z = x.reshape(B * H, W, C)[g.clamp(0, B * H - 1)] * ok[:, None, None]
    return (z[:, xx.clamp(0, W - 1)] * okx[None, :, None]).reshape(B, H, W, C)


def conv_as(form, x, w49, bias, res, dt, flip, pad='zero', drop_tap=None, bias_times=1, flipped=None, twice=False):
    """the convolution as the form `form` evaluates it in fp32: taps rounded to bf16 where the form does, accumulation in (ky, kx)
    order in groups of 1 (scalar, rs), 2 (dot2) or 7 (MFMA) exact products per fp32 rounding, the residual added in fp32, ONE rounding
    to dt.  pad / drop_tap / bias_times / flipped / twice=True (the rounding to dt BEFORE the residual as well) state it wrongly."""
    grp = {50: 1}.get(chain_fwd(form), 7 if form.startswith('mfma') else 2)
    w = rnd_to(w49, BF) if rounds_taps(form) else w49
    flipped = flip if flipped is None else flipped
    B, H, W, C = x.shape
    acc = torch.zeros(B, H, W, C, dtype=F32)
    if bias is not None:
        for _ in range(bias_times):
            acc = acc + bias.to(F32)
    for ky in range(7):
        for k0 in range(0, 7, grp):
            p = torch.zeros(B, H, W, C, dtype=F64)
            for kx in range(k0, min(7, k0 + grp)):
                t = ky * 7 + kx
                if t == drop_tap:
                    p = p + w[48 - t if flipped else t] * _gather(x, ky - 3, kx - 3, 'zero') * _interior(H, W, ky - 3, kx - 3)
                    continue
                p = p + w[48 - t if flipped else t] * _gather(x, ky - 3, kx - 3, pad)
            acc = _fma(acc, p)
    if twice:
        acc = acc.to(dt).to(F32)
    if res is not None:
        acc = _fma(acc, res)
    return acc.to(dt).to(F64)


def _interior(H, W, dy, dx):
    """1 where the tap's source pixel lies at least one pixel inside the image, 0 on its border ring: a tap dropped at the border"""
    yy, xx = torch.arange(H) + dy, torch.arange(W) + dx
    oky = ((yy > 0) & (yy < H - 1)).to(F64)
    okx = ((xx > 0) & (xx < W - 1)).to(F64)
    return oky[None, :, None, None] * okx[None, None, :, None]


def wgrad_plan(form, B, H, W):
    """how the form splits the reduction: a list of partials, each a list of chains (what one wave or workgroup accumulates before it
    meets the others), each a list of units (image, row_lo, row_hi) in the order they are walked"""
    fam = form.split(':')[0]
    num = {k: int(v) for k, v in re.findall(r'([A-Za-z]+)(\d+)', form.split(':', 1)[1].split('+')[0])}
    if fam == 'rs':
        R, nseg, nbw = num['R'], num['seg'], num['nbw']
        units = [(u // nseg, (u % nseg) * R, (u % nseg + 1) * R) for u in range(B * nseg)]
        return [[units[kb * 4 + wv::4 * nbw] for wv in range(4)] for kb in range(nbw)]
    # LDS forms: workgroup g walks the tiles g, g + gx, ..; whole images when the map is one tile, else approximated by image
    big = fam.endswith('14x14')
    parts = num['parts']
    gx = parts // 2 if (big and fam.startswith('scalar')) else parts
    th = 14 if big else 7
    tiles = [(b, ty * th, min(H, (ty + 1) * th)) for b in range(B) for ty in range(_cdiv(H, th))]
    if big and fam.startswith('scalar'):      # a partial per (workgroup, group of 7 rows)
        return [[[(b, lo + 7 * rg, lo + 7 * rg + 7) for b, lo, hi in tiles[g::gx]]] for g in range(gx) for rg in range(2)]
    return [[tiles[g::gx]] for g in range(gx)]


def wgrad_as(form, dy, x, init_w, init_b, seam=0, second='add', store=False, skip_part=None):
    """dw49, dbias (float64 values of fp32 results) as the form accumulates them: fp32 sums per unit, chain, partial, 16 reduce groups
    and the += into the initial values.  seam = -1 | +1 drops | doubles the last row of every unit that ends inside the image;
    second='overwrite': a chain's second unit replaces its first; store: dw49 = sum instead of +=; skip_part: that partial is left out"""
    B, H, W, C = x.shape
    dyf, xf = dy, x
    parts = []
    for chains in wgrad_plan(form, B, H, W):
        pw, pb = torch.zeros(49, C, dtype=F32), torch.zeros(C, dtype=F32)
        for units in chains:
            cw, cb = torch.zeros(49, C, dtype=F32), torch.zeros(C, dtype=F32)
            for n, (b, lo, hi) in enumerate(units):
                uw, _, ub, _ = bwd_weight(dyf[b:b + 1], xf[b:b + 1], (lo, hi))
                if seam and hi < H:
                    sw, _, sb, _ = bwd_weight(dyf[b:b + 1], xf[b:b + 1], (hi - 1, hi))
                    uw, ub = uw + seam * sw, ub + seam * sb
                if second == 'overwrite' and n == 1:
                    cw, cb = uw.to(F32), ub.to(F32)
                else:
                    cw, cb = cw + uw.to(F32), cb + ub.to(F32)
            pw, pb = pw + cw, pb + cb
        parts.append((pw, pb))
    if skip_part is not None:
        parts.pop(skip_part % len(parts))
    per = _cdiv(len(parts), 16)
    sw, sb = torch.zeros(49, C, dtype=F32), torch.zeros(C, dtype=F32)
    for g0 in range(0, len(parts), per):
        gw, gb = torch.zeros(49, C, dtype=F32), torch.zeros(C, dtype=F32)
        for pw, pb in parts[g0:g0 + per]:
            gw, gb = gw + pw, gb + pb
        sw, sb = sw + gw, sb + gb
    if store:
        return sw.to(F64), sb.to(F64)
    return (init_w.to(F32) + sw).to(F64), (init_b.to(F32) + sb).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases: (label, family, dtype, geometry or a function of the CU count, knobs, kinds, which of fwd / bwd / wgrad run)
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, label, fam, dt, geom, knobs=None, kinds=('plain',), ops=('fwd', 'bwd', 'wgrad'), fwd=None, wgrad=None):
        self.label, self.fam, self.dt, self._geom, self.knobs = label, fam, dt, geom, dict(knobs or {})
        self.kinds, self.ops = kinds, ops
        self._fwd, self._wgrad = fwd, wgrad          # expected form names: str or a function of (geometry, CU count); None: the family

    def geom(self, cus):
        return self._geom(cus) if callable(self._geom) else self._geom

    def want(self, which, cus):
        w = self._fwd if which == 'fwd' else self._wgrad
        return w(self.geom(cus), cus) if callable(w) else w

    def __repr__(self):
        return self.label


RS = dict(DWW_RS=2)
LDS7 = dict(DW_RS=0, DWW_RS=0)
LDS14 = dict(DW_RS=0, DW_MFMA=0, DWW_RS=0)
MFMA = dict(DW_RS=0, DW_MFMA=2, DWW_RS=0)


def _rs(label, geom, R, **kw):
    B, H, W, C = geom
    wpu = _cdiv(_cdiv(W, 4) * (C // 2), 64)
    return Case(label, 'rs', BF, geom, dict(RS, DW_RS_ROWS=R, DWW_RS_ROWS=R), fwd=f'rs:R{R}:seg{H // R}:wpu{wpu}',
                wgrad=lambda g, cus: f'rs:R{R}:seg{H // R}:wpu{wpu}:nbw{max(1, 2 * cus // wpu)}', **kw)


def _wpu_for_nbw(cus, nbw):
    """waves per unit that give max(1, 2 cus / wpu) == nbw"""
    for wpu in range(1, 2 * cus + 1):
        if max(1, 2 * cus // wpu) == nbw:
            return wpu
    raise AssertionError((cus, nbw))


def _two_unit_geom(cus):
    """C = 768, W = 28: wpu = 42; 4 nbw waves per lane map and 4 nbw + 4 units: four waves walk two units, the others one"""
    return (4 * max(1, 2 * cus // 42) + 4, 7, 28, 768)


def _nbw_geom(nbw):
    """W = 4, H = 7: one strip, wpu = C / 128"""
    return lambda cus: (2, 7, 4, 128 * _wpu_for_nbw(cus, nbw))


CASES = [_rs(f'rs W{W}', (2, 7, W, 16), 7) for W in (1, 2, 3, 4, 5, 7, 8, 9, 13)] + [
    _rs('rs H14 R14', (2, 14, 8, 16), 14, kinds=('plain', 'rough')),
    _rs('rs H21 R21', (2, 21, 8, 16), 21),
    _rs('rs H21 R7', (2, 21, 8, 16), 7),
    _rs('rs H35 R35', (1, 35, 5, 16), 35),
    _rs('rs C8', (2, 14, 5, 8), 14),
    _rs('rs C24 W12', (2, 14, 12, 24), 14),
    _rs('rs C136 W8', (2, 21, 8, 136), 21),
    _rs('rs B3 R7', (3, 14, 9, 16), 7),
    _rs('rs one unit', (1, 14, 5, 16), 14, ops=('wgrad',)),
    Case('rs two-unit wave', 'rs', BF, _two_unit_geom, dict(RS, DWW_RS_ROWS=7), ops=('wgrad',),
         wgrad=lambda g, cus: f'rs:R7:seg1:wpu42:nbw{max(1, 2 * cus // 42)}'),
] + [Case(f'rs nbw{n}', 'rs', BF, _nbw_geom(n), dict(RS, DWW_RS_ROWS=7), ops=('wgrad',),
          wgrad=(lambda n: lambda g, cus: f'rs:R7:seg1:wpu{g[3] // 128}:nbw{n}')(n)) for n in (15, 16, 17)] + [
    Case(f'dot2_7 {H}x{W} C{C}', 'dot2_7x7', BF, (B, H, W, C), LDS7, kinds=kinds)
    for B, H, W, C, kinds in ((2, 1, 1, 16, ('plain',)), (2, 6, 13, 16, ('plain',)), (2, 7, 7, 16, ('plain',)), (2, 8, 15, 72, ('plain', 'rough')),
                              (2, 13, 8, 8, ('plain',)), (1, 15, 6, 128, ('plain',)))] + [
    Case('dot2_7 walk', 'dot2_7x7', BF, lambda cus: (4 * cus // 8 * 3 // 2, 3, 5, 512), LDS7, ops=('fwd', 'bwd'),
         fwd=lambda g, cus: f'dot2_7x7:gx{4 * cus // 8}:tiles{g[0]}'),
] + [Case(f'dot2_7 parts{n}', 'dot2_7x7', BF, (n, 5, 6, 16), LDS7, ops=('wgrad',), wgrad=f'dot2_7x7:parts{n}') for n in (1, 15, 16, 17, 33)] + [
    Case(f'dot2_14 {H}x{W} C{C}', 'dot2_14x14', BF, (B, H, W, C), LDS14, kinds=kinds)
    for B, H, W, C, kinds in ((2, 14, 14, 8, ('plain',)), (2, 14, 42, 72, ('plain', 'rough')), (1, 28, 14, 128, ('plain',)))] + [
    Case('dot2_14 walk', 'dot2_14x14', BF, lambda cus: (2 * cus // 8 + 8, 14, 14, 512), LDS14,
         fwd=lambda g, cus: f'dot2_14x14:gx{2 * cus // 8}:tiles{g[0]}', wgrad=lambda g, cus: f'dot2_14x14:parts{cus // 8}'),
] + [Case(f'mfma {H}x{W} C{C} B{B} xcd{x}', 'mfma', BF, (B, H, W, C), dict(MFMA, DW_XCD8=x), kinds=kinds, ops=('fwd', 'bwd'), fwd=name)
     for B, H, W, C, x, kinds, name in (
         (1, 14, 14, 8, 1, ('plain',), 'mfma:gx1:tiles1'), (2, 28, 14, 40, 1, ('plain', 'rough'), 'mfma:gx4:tiles4'),
         (15, 14, 14, 32, 1, ('plain',), 'mfma:gx15:tiles15'), (16, 14, 14, 32, 1, ('plain',), 'mfma:gx16:tiles16'),
         (17, 14, 14, 32, 1, ('plain',), 'mfma:gx16:tiles17'), (17, 14, 14, 32, 0, ('plain',), 'mfma:gx17:tiles17'),
         (20, 14, 14, 32, 1, ('plain',), 'mfma:gx16:tiles20'))] + [
    Case('mfma many slices', 'mfma', BF, lambda cus: (cus // 16 + 4, 14, 14, 512), MFMA, ops=('fwd', 'bwd'),
         fwd=lambda g, cus: f'mfma:gx{cus // 16 // 8 * 8 if cus // 16 >= 16 else cus // 16}:tiles{g[0]}'),
] + [Case(f'scalar {"bf16" if dt == BF else "f32"} {H}x{W} C{C}', f'scalar_{til}', dt, (B, H, W, C), {}, kinds=kinds)
     for dt, B, H, W, C, til, kinds in (
         (F32, 2, 9, 10, 4, '7x7', ('plain',)), (F32, 2, 9, 10, 36, '7x7', ('plain', 'rough')), (F32, 2, 1, 1, 68, '7x7', ('plain',)),
         (F32, 2, 14, 14, 4, '14x14', ('plain',)), (F32, 1, 14, 28, 36, '14x14', ('plain',)), (F32, 1, 28, 14, 68, '14x14', ('plain',)),
         (BF, 2, 9, 10, 4, '7x7', ('plain',)), (BF, 2, 9, 10, 12, '7x7', ('plain', 'rough')), (BF, 2, 1, 1, 68, '7x7', ('plain',)),
         (BF, 2, 14, 14, 4, '14x14', ('plain',)), (BF, 1, 14, 28, 12, '14x14', ('plain',)), (BF, 1, 28, 14, 68, '14x14', ('plain',)))]


def family_of(form):
    return form.split(':')[0].split('+')[0]
