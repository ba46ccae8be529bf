"""Float64 references of the Adam, RMSprop / RMSpropTF, Lion and LARS steps of csrc/loss_optim.hip (include/gaext.h states their
operation order), fp32 restatements in the kernels' order, the wrong restatements the gate has to reject, and the inputs shared
by tests/test_optim_more_cpu.py and tests/test_optim_more_gpu.py.  gate(), U, FlatStub and the LAMB tensor sizes are those of
tests/_loss_optim_ref.py: |got - ref| <= a0 + 2^-126 per element, a0 = U x (every magnitude that enters the element x the fp32
roundings it can pass through), U = 2^-24, one step from the state the kernel itself left.  A fused multiply-add has fewer
roundings than the product and the sum it replaces, so the counts hold whether or not the compiler contracts.

Common: w = wd x wd_mult.  g' = g + w p: the product 1, the sum 1 -> e_g = U (2 w |p| + |g|); w = 0 gives g' = g exactly, e_g = 0.
An error e of g' reaches a square average (1 - b) g'^2 as (1 - b)(2 |g'| e + e^2), a root sqrt(x) as half x's relative error.
    Adam   m = b1 m + (1 - b1) g': 1 - b1, the product, the fused sum = 3 of A_m = b1 |m| + (1 - b1) |g'|, + (1 - b1) e_g
           v = b2 v + (1 - b2) g' g': 4 of v (AdamW's count) + the error of g'
           p -= (lr / bc1) m / (sqrt(v) rsqrt(bc2) + eps): |p| 1 (the difference); the update: half of v's relative error, sqrt 1,
           rsqrt 2 (its argument's rounding is in the hp row; the hardware rsqrt is within 1 ulp), the product 1, + eps 1, lr / bc1
           1, the product with m 1, the quotient 1, the difference 1 = 9 -> 11 of |update| (AdamW's bound keeps the same two spare),
           + m's error through the same quotient
    RMSprop (torch)  sq = alpha sq + (1 - alpha) g' g': 4 of sq + the error of g';  avg = sqrt(sq) + eps: half of sq's, sqrt 1, the sum 1
           q = g' / avg: e_g / avg + |q| (avg's relative error + 1)
           no momentum: p -= lr q: the product 1 and the difference 1 of |update|, |p| 1
           momentum:    buf = mu buf + q: 2 of (mu |buf| + |q|) + q's error;  p -= lr buf: 2 of lr |buf|, |p| 1, + lr x buf's error
    RMSpropTF        sq += (1 - alpha)(g' g' - sq): g' g' 1, the difference 1 of (g'^2 + sq), 1 - alpha and the product 2 of the same,
           the sum 1 of the new sq, + the error of g';  avg = sqrt(sq + eps): the sum 1, half of the radicand's, sqrt 1
           q as above;  no momentum: as above;  momentum: t = lr q (1), buf = mu buf + t: 2 of (mu |buf| + |t|);  p -= buf: 1 of |p| + |buf|
    Lion   p (1 - lr w) : lr w 1, 1 - x 1, the product 1, the difference 1 = 4 of |p| (1 where w = 0: the factor is exactly 1), 1 of
           lr.  The update itself is exactly lr, 0 or -lr: c = b1 m + (1 - b1) g carries 3 of A_c = b1 |m| + (1 - b1) |g|, and where
           the float64 |c| is within that of zero its sign is not determined by the inputs to fp32 precision -- there, and only
           there, either sign is right and 2 lr is allowed.  m += (1 - b2)(g - m): the difference 1, 1 - b2 and the product 2 of
           (1 - b2)(|g| + |m|), the sum 1 of the new |m|
    LARS   norms: ceil(chunk / 256) + 10 + chunks roundings of a positive sum (LAMB's count: the thread's chain, six wave steps, four
           partials, one atomic per chunk);  w = sqrt(sp), q = sqrt(sg): half of the sums' + 1 each
           den = q + w wd + eps: the product 1, two sums;  trust = tc w / den: the product 1, the quotient 1;  trust_clip: / lr 1
           d = (g + wd p) trust: e_g trust + |d| (trust's relative error + 1);  where nothing is adapted d = g exactly
           buf = mu buf + d: 2 of (mu |buf| + |d|) + d's (the first step copies d);  nesterov: d + mu buf: 2 more of (|d| + mu |buf|)
           p -= lr d: the product 1 and the difference 1 of lr |d|, |p| 1
"""
import math

import torch

import _loss_optim_ref as R
from _loss_optim_ref import F32, F64, U, gate, FlatStub, LAMB_CHUNK, _s          # noqa: F401  (re-exported for the test modules)

STRIDE = dict(adam=8192 * 256, rmsprop=8192 * 256, lion=8192 * 256)     # a flat kernel loops above this many elements
LR, WD, BETAS, LION_BETAS = 5e-3, 0.05, (0.9, 0.999), (0.9, 0.99)
RMS_ALPHA, RMS_EPS, RMSTF_EPS = 0.9, 1e-8, 1e-3         # 1e-3: the MobileNet recipes' --opt-eps; at timm's 1e-10 the place of eps is invisible in fp32
LARS_TC, LARS_EPS = 0.001, 1e-8


def hp_row(kind, lr, wd, b1=0.9, b2=0.999, eps=0.0, t=1, mu=0.0, alpha=0.9, trust_coeff=0.001, first=False):
    """the fp32 hyper-parameter row optim.py pushes to the device, as float64 values of fp32 numbers"""
    if kind == 'adam':
        row = [lr, wd, b1, b2, eps, 1 - b1 ** t, 1 - b2 ** t, 0.0]
    elif kind == 'rmsprop':
        row = [lr, wd, mu, alpha, eps, 0.0, 0.0, 0.0]
    elif kind == 'lion':
        row = [lr, wd, b1, b2, 0.0, 0.0, 0.0, 0.0]
    elif kind == 'lars':
        row = [lr, wd, mu, trust_coeff, eps, 1.0 if first else 0.0, 0.0, 0.0]
    else:
        raise ValueError(kind)
    return torch.tensor(row, dtype=F64).to(F32)


def _coupled(p, g, w):
    """g' and its error bound e_g"""
    if w == 0:
        return g.clone(), torch.zeros_like(g)
    return g + w * p, U * (2 * w * p.abs() + g.abs())


def _half_rel(a, x):
    """half the relative error a / x of a non-negative x, 0 where x is 0 (there a is 0 too)"""
    return torch.where(x > 0, a / (2 * x.clamp(min=1e-300)), torch.zeros_like(x))


# ------------------------------------------------------------------------------------------------------------------------------
# float64 steps over lists of tensors with a decay flag each; the bound of every output stands beside it
# ------------------------------------------------------------------------------------------------------------------------------
def adam_step(ps, gs, ms, vs, decay, lr, wd, b1, b2, eps, t=None, bc1=None, bc2=None):
    """torch.optim.Adam (coupled L2).  -> new ps, ms, vs, allowed {p, m, v} per tensor"""
    bc1 = 1 - b1 ** t if bc1 is None else bc1
    bc2 = 1 - b2 ** t if bc2 is None else bc2
    P, M, V, Al = [], [], [], []
    for p, g, m, v, d in zip(ps, gs, ms, vs, decay):
        g1, e_g = _coupled(p, g, wd if d else 0.0)
        m1 = b1 * m + (1 - b1) * g1
        v1 = b2 * v + (1 - b2) * g1 * g1
        den = v1.sqrt() / math.sqrt(bc2) + eps
        step = lr / bc1
        upd = step * m1 / den
        a_m = 3 * U * (b1 * m.abs() + (1 - b1) * g1.abs()) + (1 - b1) * e_g
        a_v = 4 * U * v1 + (1 - b2) * (2 * g1.abs() * e_g + e_g * e_g)
        a_p = U * p.abs() + step / den * a_m + upd.abs() * (_half_rel(a_v, v1) + 11 * U)
        P.append(p - upd)
        M.append(m1)
        V.append(v1)
        Al.append(dict(p=a_p, m=a_m, v=a_v))
    return P, M, V, Al


def rmsprop_step(ps, gs, sqs, bufs, decay, lr, wd, mu, alpha, eps, tf=False):
    """tf False: torch.optim.RMSprop (not centered); tf True: timm RMSpropTF (not centered, coupled decay, lr_in_momentum).
    bufs None: the form without momentum.  -> new ps, sqs, bufs (or None), allowed {p, sq, buf} per tensor"""
    P, S, Bf, Al = [], [], [], []
    for i, (p, g, sq, d) in enumerate(zip(ps, gs, sqs, decay)):
        g1, e_g = _coupled(p, g, wd if d else 0.0)
        e_g2 = (1 - alpha) * (2 * g1.abs() * e_g + e_g * e_g)
        if tf:
            sq1 = sq + (1 - alpha) * (g1 * g1 - sq)
            a_sq = U * ((1 - alpha) * (g1 * g1 + 3 * (g1 * g1 + sq.abs())) + sq1.abs()) + e_g2
            rad = sq1 + eps
            avg = rad.sqrt()
            a_avg = (a_sq + U * rad) / (2 * avg) + U * avg
        else:
            sq1 = alpha * sq + (1 - alpha) * g1 * g1
            a_sq = 4 * U * sq1 + e_g2
            r = sq1.sqrt()
            avg = r + eps
            a_avg = r * (_half_rel(a_sq, sq1) + U) + U * avg
        q = g1 / avg
        a_q = e_g / avg + q.abs() * (a_avg / avg + U)
        al = dict(sq=a_sq)
        if bufs is None:
            upd = lr * q
            p1 = p - upd
            al['p'] = U * (p.abs() + upd.abs()) + lr * a_q + U * upd.abs()
        elif tf:
            tt = lr * q
            b1_ = mu * bufs[i] + tt
            al['buf'] = lr * a_q + U * tt.abs() + 2 * U * (mu * bufs[i].abs() + tt.abs())
            p1 = p - b1_
            al['p'] = U * (p.abs() + b1_.abs()) + al['buf']
            Bf.append(b1_)
        else:
            b1_ = mu * bufs[i] + q
            al['buf'] = a_q + 2 * U * (mu * bufs[i].abs() + q.abs())
            upd = lr * b1_
            p1 = p - upd
            al['p'] = U * (p.abs() + upd.abs()) + U * upd.abs() + lr * al['buf']
            Bf.append(b1_)
        P.append(p1)
        S.append(sq1)
        Al.append(al)
    return P, S, (None if bufs is None else Bf), Al


def lion_step(ps, gs, ms, decay, lr, wd, b1, b2):
    """timm Lion.  -> new ps, ms, allowed {p, m} per tensor, and per tensor the mask of elements whose sign is not determined"""
    P, M, Al, Und = [], [], [], []
    for p, g, m, d in zip(ps, gs, ms, decay):
        w = wd if d else 0.0
        c = b1 * m + (1 - b1) * g
        a_c = 3 * U * (b1 * m.abs() + (1 - b1) * g.abs())
        und = (c.abs() <= a_c) & (a_c > 0)
        m1 = m + (1 - b2) * (g - m)
        P.append(p * (1 - lr * w) - lr * torch.sign(c))
        M.append(m1)
        Al.append(dict(p=U * ((4 if w else 1) * p.abs() + lr) + 2 * lr * und.to(F64),
                       m=U * (3 * (1 - b2) * (g.abs() + m.abs()) + m1.abs())))
        Und.append(und)
    return P, M, Al, Und


def lars_step(ps, gs, bufs, decay, lr, wd, mu, tc, eps, nesterov=False, trust_clip=False, first=False, chunk=LAMB_CHUNK):
    """timm Lars (always_adapt off) with SGD momentum, dampening 0; bufs None: no momentum.
    -> dict of per-tensor lists p, buf, norms [(sum p^2, sum g^2)], trust, allowed [{p, buf, norms}]"""
    out = dict(p=[], buf=[], norms=[], trust=[], allowed=[])
    for i, (p, g, d) in enumerate(zip(ps, gs, decay)):
        sp, sg = float((p * p).sum()), float((g * g).sum())
        cn = math.ceil(min(p.numel(), chunk) / 256) + 10 + math.ceil(p.numel() / chunk)
        a_sp, a_sg = U * cn * sp, U * cn * sg
        trust, e_tr = 1.0, 0.0
        if d and wd != 0:
            wn, qn = math.sqrt(sp), math.sqrt(sg)
            if wn > 0 and qn > 0:
                den = qn + wn * wd + eps
                trust = tc * wn / den
                e_w, e_q = a_sp / (2 * sp) + U, a_sg / (2 * sg) + U
                e_tr = e_w + U + (qn * e_q + wn * wd * (e_w + U)) / den + 2 * U + U
            if trust_clip:
                trust, e_tr = min(trust / lr, 1.0), e_tr + U
            g1, e_g = _coupled(p, g, wd)
            dd = g1 * trust
            a_d = dd.abs() * (e_tr + U) + trust * e_g
        else:
            dd, a_d = g.clone(), torch.zeros_like(g)
        al = dict(norms=(a_sp, a_sg))
        if bufs is None:
            fin, a_fin = dd, a_d
        else:
            b = bufs[i]
            nb = dd.clone() if first else mu * b + dd
            al['buf'] = a_d if first else a_d + 2 * U * (mu * b.abs() + dd.abs())
            if nesterov:
                fin = dd + mu * nb
                a_fin = a_d + mu * al['buf'] + 2 * U * (dd.abs() + mu * nb.abs())
            else:
                fin, a_fin = nb, al['buf']
            out['buf'].append(nb)
        al['p'] = U * p.abs() + 2 * U * lr * fin.abs() + lr * a_fin
        out['p'].append(p - lr * fin)
        out['norms'].append((sp, sg))
        out['trust'].append(trust)
        out['allowed'].append(al)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# restatements in the kernels' order, in dtype dt, with the wrong variants the gate must reject
# ------------------------------------------------------------------------------------------------------------------------------
ADAM_WRONG = ['decoupled_decay', 'eps_inside_root']
RMSPROP_WRONG = ['eps_outside_root', 'sq_from_zero', 'decoupled_decay']          # of the tf form
RMSPROP_TORCH_WRONG = ['eps_inside_root', 'decoupled_decay']
LION_WRONG = ['m_before_sign', 'sign_of_g']
LARS_WRONG = ['trust_no_decay', 'no_w_wd_in_den', 'clip_without_lr']


def adam_restate(p, g, m, v, hp, wd_mult, dt=F32, wrong=None):
    lr, wd, b1, b2, eps, bc1, bc2 = (hp[k].to(dt) for k in range(7))
    wd = wd * wd_mult
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    step, rbc2 = lr / bc1, torch.rsqrt(bc2)
    gi = g if wrong == 'decoupled_decay' else g + wd * p
    mi = b1 * m + (1 - b1) * gi
    vi = b2 * v + (1 - b2) * gi * gi
    den = (vi * rbc2 * rbc2 + eps).sqrt() if wrong == 'eps_inside_root' else vi.sqrt() * rbc2 + eps
    pi = p * (1 - lr * wd) if wrong == 'decoupled_decay' else p
    return (pi - step * mi / den).to(F64), mi.to(F64), vi.to(F64)


def rmsprop_restate(p, g, sq, buf, hp, tf, wd_mult, dt=F32, wrong=None):
    """buf None: the form without momentum.  -> p, sq, buf (or None)"""
    lr, wd, mu, alpha, eps = (hp[k].to(dt) for k in range(5))
    wd = wd * wd_mult
    oma = 1 - alpha
    p, g, si = p.to(dt), g.to(dt), sq.to(dt)
    gi = g if wrong == 'decoupled_decay' else g + wd * p
    pi = p * (1 - lr * wd) if wrong == 'decoupled_decay' else p
    inside = tf != (wrong in ('eps_outside_root', 'eps_inside_root'))
    si = si + oma * (gi * gi - si) if tf else alpha * si + oma * gi * gi
    avg = (si + eps).sqrt() if inside else si.sqrt() + eps
    if buf is None:
        return (pi - lr * gi / avg).to(F64), si.to(F64), None
    bi = mu * buf.to(dt) + (lr * gi / avg if tf else gi / avg)
    return (pi - (bi if tf else lr * bi)).to(F64), si.to(F64), bi.to(F64)


def lion_restate(p, g, m, hp, wd_mult, dt=F32, wrong=None):
    lr, wd, b1, b2 = (hp[k].to(dt) for k in range(4))
    wd = wd * wd_mult
    p, g, m = p.to(dt), g.to(dt), m.to(dt)
    m1 = m + (1 - b2) * (g - m)
    c = b1 * (m1 if wrong == 'm_before_sign' else m) + (1 - b1) * g
    if wrong == 'sign_of_g':
        c = g
    return (p * (1 - lr * wd) - lr * torch.sign(c)).to(F64), m1.to(F64)


def lars_restate(ps, gs, bufs, decay, hp, nesterov, trust_clip, dt=F32, wrong=None, chunk=LAMB_CHUNK):
    """ga_lars_stage1 + ga_lars_stage2 over the chunk table (zeroed norms).  -> dict like lars_step"""
    lr, wd, mu, tc, eps = (hp[k].to(dt) for k in range(5))
    first = float(hp[5]) != 0.0
    out = dict(p=[], buf=[], norms=[])
    for i, (p, g, d) in enumerate(zip(ps, gs, decay)):
        p, g = p.to(dt), g.to(dt)
        sp, sg = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt)
        for c0 in range(0, p.numel(), chunk):
            sp = sp + (p[c0:c0 + chunk] ** 2).sum()
            sg = sg + (g[c0:c0 + chunk] ** 2).sum()
        if (d or wrong == 'trust_no_decay') and float(wd) != 0.0:
            wn, gn = sp.sqrt(), sg.sqrt()
            trust = _s(1.0, dt)
            if wn > 0 and gn > 0:
                trust = tc * wn / ((gn + eps) if wrong == 'no_w_wd_in_den' else (gn + wn * wd + eps))
            if trust_clip:
                trust = torch.minimum(trust if wrong == 'clip_without_lr' else trust / lr, _s(1.0, dt))
            dd = (g + wd * p) * trust
        else:
            dd = g
        if bufs is not None:
            bi = dd if first else mu * bufs[i].to(dt) + dd
            dd = dd + mu * bi if nesterov else bi
            out['buf'].append(bi.to(F64))
        out['p'].append((p - lr * dd).to(F64))
        out['norms'].append((float(sp), float(sg)))
    return out


def lars_ratios(got, ref):
    """got: dict of per-tensor lists (float64) -> name -> worst ratio over the tensors"""
    out = {}
    for n in ('p', 'buf'):
        if got.get(n):
            out[n] = max(gate(x, r, al[n]) for x, r, al in zip(got[n], ref[n], ref['allowed']))
    out['norms'] = max(max(gate(x[k], r[k], al['norms'][k]) for k in (0, 1)) for x, r, al in zip(got['norms'], ref['norms'], ref['allowed']))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
STEPS = 3


def flat_inputs(n, seed, device='cpu'):
    """p0 and the gradients of STEPS steps (float64 values of fp32 numbers) with the edge elements the steps must hold at: p = 0 at
    3 mod 7, g = 0 in every step at 5 mod 11 (both at 38 mod 77), the whole gradient of the second step zero"""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda sc: (torch.randn(n, generator=gen, device=device, dtype=F32) * sc).to(F64)
    p0, grads = rn(0.05), [rn(0.01) for _ in range(STEPS)]
    p0[3::7] = 0
    for g in grads:
        g[5::11] = 0
    grads[1].zero_()
    return p0, grads


LARS_SIZES, LARS_NDECAY = R.LAMB_SIZES, R.LAMB_NDECAY
LARS_ZERO_P, LARS_ZERO_G = 2, 3          # decayed tensors: the one whose parameters are all zero, the one whose gradient is zero
LARS_FORMS = [(False, False), (True, False), (False, True), (True, True)]          # (nesterov, trust_clip): lars, nlars, larc, nlarc
LARS_CASES = {'decay': dict(wd=0.05, zero_g=False), 'wd0': dict(wd=0.0, zero_g=False), 'zero_grads': dict(wd=0.05, zero_g=True)}


def lars_inputs(label):
    """p0 per tensor and the gradients of STEPS steps.  |p| / |g| is 4, 8, 12 by tensor, so with trust_coeff 1e-3, wd 0.05 and lr
    5e-3 the clipped ratio trust / lr (0.67, 1.14, 1.5) lies on both sides of 1"""
    c = LARS_CASES[label]
    gen = torch.Generator().manual_seed(700 + sorted(LARS_CASES).index(label))
    p0 = [(torch.randn(n, generator=gen, dtype=F32) * (0.02 * (1 + (i + 1) % 3))).to(F64) for i, n in enumerate(LARS_SIZES)]
    p0[LARS_ZERO_P].zero_()
    grads = []
    for s in range(STEPS):
        gs = [(torch.randn(n, generator=gen, dtype=F32) * (0.0 if c['zero_g'] else 0.005)).to(F64) for n in LARS_SIZES]
        gs[LARS_ZERO_G].zero_()
        grads.append(gs)
    return p0, grads
