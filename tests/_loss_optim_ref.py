"""Float64 references of what csrc/loss_optim.hip computes at the end of a training step, the ONE gate its kernel tests use, fp32
restatements in the kernels' order, wrong restatements that the gate has to reject, and the case tables shared by
tests/test_loss_optim_ref_cpu.py and tests/test_loss_optim_edges_gpu.py.

gate(): per element  |got - ref| <= r |ref| + a0 + eps_fast ce + floor,  nothing relative to the tensor's maximum.
    r     = 2^-8 where the output is stored as bf16 (ONE round-to-nearest; half an ulp is 2^-8 of a value just above a power of
            two), 0 for fp32 outputs (their store is exact; the last operation's rounding is counted in a0)
    a0    = U sum_i n_i A_i, U = 2^-24: every magnitude A_i that enters the element times the number n_i of fp32 roundings it can
            pass through in the kernel.  The counts stand next to each formula below.  An argument x of exp() counts as a
            magnitude too: an absolute error d of x is a relative error d of exp(x), so |x| large costs precision -- this is
            what the large-logit cases measure the kernel against
    ce    = the same sum for the ONE allowance that cannot be derived: the error of the hardware's v_exp_f32 / v_log_f32 behind
            __expf / __logf (documented as about 1 ulp, not as correctly rounded).  ce counts how many of them enter the element,
            weighted like a0; EPS_FAST is measured on the MI355X (tests/test_loss_optim_edges_gpu.py) and set to 4 x the worst need.
            The products inside the intrinsics (x * log2 e, log2 s * ln 2) are ordinary roundings and counted in a0
    floor = 2^-126 (x grad_scale): __expf and the stores may flush subnormals to zero

Loss (csrc/loss_optim.hip ga_loss_kernel), out [K][B][NC], optional avg [K][B][NC], t the class-index target (smoothed one-hot:
off = s / NC, on = 1 - s + off) or the dense one, binarised t > thr under BCE with thr >= 0:
    logp_k = log_softmax(out_k), p_k = exp(logp_k);  logr = log_softmax(mean_k out_k), r = exp(logr)  (r is a constant: detached)
    loss  = sum_k [ L(out_k, t) + lam sum_bc r (logr - logp_k) / (B NC) + (avg) sum_bc p_k (logp_k - loga_k) / (B NC) ]
    CE:   L = -sum_bc t logp / B                                   dL/dout = (p sum_c t - t) / B
    BCE:  L = sum_bc [max(x,0) - x t + log1p(exp(-|x|))] / (B NC)  dL/dout = (sigmoid(x) - t) / (B NC)
    dorg  = grad_scale [ dL/dout + lam (p_k - r) / (B NC) ]        davg = grad_scale (softmax(avg_k) - p_k) / (B NC)
    (the loss VALUE is not scaled by grad_scale.)
  log_softmax of a row x in the kernel: m = max x (exact); z = x - m (1 rounding of |z|); __expf(z) (1 rounding of |z| in the
  product with log2 e, 1 v_exp); s = sum: ceil(NC / 256) + 10 additions of positive terms (the thread's chain, six wave steps, four
  wave partials); __logf(s) (1 v_log, 1 rounding of |log s| in the product with ln 2); lse = m + log s (1 rounding of |lse|);
  logp = x - lse (1 rounding of |logp|); p = __expf(logp) (1 rounding of |logp|, 1 v_exp):
    d(logp) = U [ sum_c p_c 2 |z_c| + ceil(NC/256) + 10 + 2 |log s| + |lse| + |logp| ],  ce(logp) = 1 + |log s|
    d(p) / p = d(logp) + U |logp|,  ce(p) = ce(logp) + 1
  the mean row adds d(mean_c) = U sum_k |out_kc| (K - 1 additions and the division, each at most U of the partial sum, over K) at
  its own column and, through lse, at most its maximum over the row.
  dorg: (p - r) 1, lam / (B NC) 1, the product 1, the sum with dL/dout 1, grad_scale 1: 5 roundings of every magnitude, written
  as 4 U (p + r) |lam| / (B NC) + the terms of dL/dout + U A; CE: p sum_t (d(p) + (ceil(NC/256) + 10 + 3) U) + 3 U |t| (the
  smoothed values on, off are computed in fp32); BCE: sigmoid = 1 / (1 + exp(-x)): U (|x| (1 - sigmoid) + 3) + 2 U (sigmoid + |t|).
  loss: every term's own error (same building blocks) + n_acc U (sum of |terms| + |initial|), n_acc = 3 K ceil(NC/256) per
  target term (x 2 with avg) + 10 + B + 1: the thread's chain, the block sum, B atomic additions onto the initial value.

Optimizers (one step from the state the kernel itself left, so that the bound is one step's): see sgd_step / adamw_step /
lamb_step; the hyper-parameters are the fp32 values of the hp row (hp_row()), exact in float64.
    SGD    g' = g + wd p (2); buf = first ? g' : mu buf + g' (2); d = nesterov ? g' + mu buf : buf (2); p -= lr d (2)
           buf: 4 U A_buf;  p: U (2 |p| + 8 lr A_d)
    AdamW  m = b1 m + (1 - b1) g (3: 1 - b1, product, fma); v = b2 v + (1 - b2) g g (4);
           p = p (1 - lr wd) - (lr / bc1) m / (sqrt(v) rsqrt(bc2) + eps): p 4; the step: v's 4 / 2, sqrt 1, rsqrt 2, product 1,
           + eps 1, lr / bc1 1, product 1, quotient 1, difference 1 = 11 -> 13 of |step| + 3 of A_m through the same quotient
    LAMB   gsumsq: n_ss(total) roundings of a positive sum (sumsq_kernel: four products and three additions per float4 trip, six
           wave steps, four partials, one atomic per workgroup); gn = sqrt (1): e_gn = U (n_ss / 2 + 1); clipped g: e_g = e_gn + 2 U
           m (3: two products and the sum, + e_g), v (4, + 2 e_g), u = (m / bc1) / (sqrt(v) rsqrt(bc2) + eps) + wd p: m's error through the quotient,
           |adam part| (v's / 2 + 10 U), wd p 2, the sum 1;  norms: ceil(chunk / 256) + 10 + chunks of the positive sums (+ 2 |u| d(u));
           trust = sqrt(sp) / sqrt(su): halves of both + 3;  p -= (lr trust) u: |p| 1, the step 3 + e_trust + d(u)
"""
import math

import numpy as np
import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
R_BF16 = 2.0 ** -8
TINY = 2.0 ** -126
# the v_exp_f32 / v_log_f32 allowance: measured on an MI355X by tests/test_loss_optim_edges_gpu.py (see its docstring), 4 x the worst need
EPS_FAST = 4 * 1.68e-7

# the launch constants of csrc/loss_optim.hip the cases are sized by: a flat kernel loops above STRIDE[name] elements
STRIDE = dict(sgd=8192 * 256, adamw=8192 * 256, clip=4096 * 256, sumsq=2048 * 256 * 4, mixup_batch=8192 * 256, u8_normalize=8192 * 1024,
              dropout_mask=2048 * 256)
LDS_OPT_IN = 65536          # dynamic LDS above this needs hipFuncSetAttribute: (NC + 8) * 4 in the loss, NC * 4 in heads_topk
NC_MAX = 36000
LAMB_CHUNK = 16384


def r_of(dt):
    return R_BF16 if dt == BF else 0.0


def gate(got, ref, a0, r=0.0, ce=None, eps=None, floor=TINY):
    """worst |got - ref| / (r |ref| + a0 + eps ce + floor) over the elements (float64 tensors or numbers)"""
    got, ref, a0 = (torch.as_tensor(x, dtype=F64) for x in (got, ref, a0))
    allowed = r * ref.abs() + a0 + floor
    if ce is not None:
        allowed = allowed + (EPS_FAST if eps is None else eps) * torch.as_tensor(ce, dtype=F64)
    err = (got - ref).abs()
    ratio = torch.where(err.isnan(), torch.full_like(err, float('inf')), err / allowed)
    return float(ratio.max())


def need_eps(got, ref, a0, ce, r=0.0, floor=TINY):
    """the smallest eps_fast with which every element meets the gate (0 where a0 alone is enough)"""
    got, ref, a0, ce = (torch.as_tensor(x, dtype=F64) for x in (got, ref, a0, ce))
    excess = (got - ref).abs() - (r * ref.abs() + a0 + floor)
    need = torch.where(excess > 0, excess / ce.clamp(min=1e-300), torch.zeros_like(excess))
    return float(need.max())


# ------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------
class LossCase:
    def __init__(self, label, K, B, NC, kind, smooth, tgt, thr, avg, gs, regime, grad=True, seed=0):
        self.label, self.K, self.B, self.NC, self.kind, self.smooth, self.tgt, self.thr = label, K, B, NC, kind, smooth, tgt, thr
        self.avg, self.gs, self.regime, self.grad, self.seed, self.lam = avg, gs, regime, grad, seed, -0.8

    def __repr__(self):
        return self.label

    def entry(self):
        """the C entry point the case goes through: the two wrappers where their argument lists suffice"""
        if self.tgt == 'idx' and self.thr < 0:
            return 'ga_map_loss_fwd_bwd' if self.avg else 'ga_loss_fwd_bwd'
        return 'ga_loss_dense_fwd_bwd'


def _lc(K, B, NC, kind, smooth, tgt, thr, avg, gs, regime, grad=True):
    label = f'K{K}-B{B}-NC{NC}-{"bce" if kind else "ce"}-s{smooth}-{tgt}-thr{thr}-{"avg" if avg else "noavg"}-gs{gs}-{regime}' + ('' if grad else '-lossonly')
    return LossCase(label, K, B, NC, kind, smooth, tgt, thr, avg, gs, regime, grad, seed=len(LOSS_CASES))


LOSS_CASES = []
for _a in [
    (1, 1, 1, 0, 0.0, 'idx', -1.0, False, 1.0, 'randn2'),
    (2, 3, 1, 1, 0.1, 'dense_uneven', -1.0, True, 0.25, 'randn2'),
    (2, 3, 2, 1, 0.1, 'idx', 0.2, True, 0.25, 'randn2'),
    (5, 1, 2, 0, 0.0, 'idx', -1.0, False, 1.0, 'const'),
    (5, 3, 63, 0, 0.1, 'dense1', -1.0, False, 65536.0, 'randn30'),
    (7, 1, 64, 1, 0.0, 'dense_uneven', -1.0, True, 1.0, 'randn2'),
    (2, 3, 64, 1, 0.0, 'dense1', 0.2, False, 1.0, 'spike'),
    (2, 3, 65, 0, 0.0, 'dense_uneven', -1.0, False, 0.25, 'same'),
    (1, 3, 255, 1, 0.1, 'dense1', 0.2, True, 1.0, 'const'),
    (5, 1, 256, 0, 0.1, 'idx', -1.0, True, 65536.0, 'spike'),
    (7, 3, 257, 0, 0.0, 'dense_uneven', 0.2, True, 1.0, 'randn2'),
    (5, 3, 257, 0, 0.1, 'idx', -1.0, False, 1.0, 'randn2', False),
    (5, 3, 1000, 0, 0.1, 'idx', -1.0, False, 1.0, 'randn2'),
    (5, 3, 1000, 0, 0.0, 'idx', -1.0, False, 0.25, 'randn30'),
    (5, 3, 1000, 1, 0.1, 'idx', -1.0, False, 1.0, 'randn30'),
    (2, 3, 1000, 0, 0.0, 'dense1', -1.0, True, 0.25, 'same'),
    (2, 3, 1000, 1, 0.1, 'idx', -1.0, True, 1.0, 'randn2', False),
    (2, 3, 16376, 0, 0.1, 'idx', -1.0, True, 1.0, 'randn2'),
    (2, 3, 16377, 1, 0.0, 'dense1', 0.2, False, 0.25, 'randn30'),
    (2, 1, 16377, 0, 0.1, 'idx', -1.0, False, 1.0, 'randn2'),
    (7, 3, 36000, 0, 0.1, 'dense_uneven', -1.0, True, 65536.0, 'randn2'),
    (1, 1, 36000, 1, 0.1, 'idx', -1.0, False, 1.0, 'spike'),
]:
    LOSS_CASES.append(_lc(*_a))


def loss_inputs(c):
    """float64 tensors whose values are fp32 values: org, avg (or None), target (int64) or dense, initial loss"""
    g = torch.Generator().manual_seed(500 + c.seed)
    K, B, NC = c.K, c.B, c.NC
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F32).to(F64)
    if c.regime == 'randn2':
        org = rn(K, B, NC) * 2
    elif c.regime == 'randn30':
        org = (rn(K, B, NC) * 30).to(F32).to(F64)
    elif c.regime == 'same':
        org = (rn(1, B, NC) * 2).expand(K, B, NC).clone()
    elif c.regime == 'const':
        org = rn(K, B, NC) * 2
        org[:, 0, :] = 1.5
    elif c.regime == 'spike':
        org = torch.zeros(K, B, NC, dtype=F64)
        for k in range(K):
            for b in range(B):
                org[k, b, (7 * k + 3 * b) % NC] = 80.0
    else:
        raise ValueError(c.regime)
    i = dict(org=org, avg=(rn(K, B, NC) * 2) if c.avg else None, target=None, dense=None, initial=3.25)
    t = torch.randint(0, NC, (B,), generator=g)
    t[0] = NC - 1
    if B > 1:
        t[1] = 0
    if c.tgt == 'idx':
        i['target'] = t
    else:
        t2 = t.flip(0) if B > 1 else (t + 1) % NC
        off = 0.1 / NC
        d = torch.full((B, NC), 2 * off * 0.5, dtype=F64)
        for b in range(B):      # the mixed smoothed one-hot of ga_mixup_target, lam = 0.37: every row sums to 1
            d[b, t[b]] += 0.37 * 0.9
            d[b, t2[b]] += 0.63 * 0.9
        if c.tgt == 'dense_uneven':
            d = d * torch.tensor(([0.6, 1.7, 1.0] * B)[:B], dtype=F64)[:, None]
        i['dense'] = d.to(F32).to(F64)
    return i


def _targets(i, c, NC):
    """t [B][NC] float64 and the CE row sum"""
    if i['dense'] is not None:
        t = i['dense']
    else:
        off = c.smooth / NC
        t = torch.full((i['org'].shape[1], NC), off, dtype=F64)
        t[torch.arange(t.shape[0]), i['target']] = 1.0 - c.smooth + off
    if c.kind == 1 and c.thr >= 0:
        t = (t > c.thr).to(F64)
    tsum = t.sum(-1, keepdim=True) if (i['dense'] is not None and c.kind == 0) else torch.ones(t.shape[0], 1, dtype=F64)
    return t, tsum


def _chain(NC):
    return math.ceil(NC / 256) + 10


def _lsm(x):
    """logp, p, d(logp), ce(logp) of the rows of x (see the module docstring)"""
    NC = x.shape[-1]
    m = x.max(-1, keepdim=True).values
    z = x - m
    e = torch.exp(z)
    s = e.sum(-1, keepdim=True)
    ls = torch.log(s)
    lse = m + ls
    logp = x - lse
    row = (e / s * 2 * z.abs()).sum(-1, keepdim=True) + _chain(NC) + 2 * ls.abs() + lse.abs()
    return logp, torch.exp(logp), U * (row + logp.abs()), (1 + ls.abs()).expand_as(logp)


def loss_ref(i, c):
    """the closed forms written by hand.  Returns dict name -> (ref, a0, ce) for 'loss' (the increment), 'dorg', 'davg'"""
    org, avg = i['org'], i['avg']
    K, B, NC = org.shape
    BN, lam, gs = B * NC, c.lam, c.gs
    t, tsum = _targets(i, c, NC)
    logp, p, d_lp, ce_lp = _lsm(org)
    d_p, ce_p = d_lp + U * logp.abs(), ce_lp + 1
    d_mean = U * org.abs().sum(0)
    logr, rr, d_lr, ce_lr = _lsm(org.sum(0) / K)
    d_lr = d_lr + d_mean + d_mean.max(-1, keepdim=True).values
    d_r, ce_r = d_lr + U * logr.abs(), ce_lr + 1
    al = abs(lam)
    # ---- gradient
    gkl = lam / BN * (p - rr)
    a_kl = al / BN * (p * d_p + rr * d_r + 4 * U * (p + rr))
    c_kl = al / BN * (p * ce_p + rr * ce_r)
    if c.kind == 0:
        gh = (p * tsum - t) / B
        a_h = (p * tsum * (d_p + (_chain(NC) + 3) * U) + 3 * U * t.abs()) / B
        c_h = p * tsum * ce_p / B
        A_h = (p * tsum + t.abs()) / B
    else:
        sg = torch.sigmoid(org)
        gh = (sg - t) / BN
        a_h = (sg * U * (org.abs() * (1 - sg) + 3) + 2 * U * (sg + t.abs())) / BN
        c_h = sg * (1 - sg) / BN
        A_h = (sg + t.abs()) / BN
    A = al / BN * (p + rr) + A_h
    out = {'dorg': (gs * (gkl + gh), gs * (a_kl + a_h + U * A), gs * (c_kl + c_h))}
    # ---- loss value: every term with its own error, then the accumulation
    D = logr - logp
    T = [lam * rr * D / BN]
    aT = [al / BN * rr * (d_r * D.abs() + d_lr + d_lp + 4 * U * D.abs())]
    cT = [al / BN * rr * (ce_r * D.abs() + ce_lr + ce_lp)]
    if c.kind == 0:
        T.append(-t * logp / B)
        aT.append(t.abs() / B * (d_lp + 3 * U * logp.abs()))
        cT.append(t.abs() / B * ce_lp)
    else:
        x = org
        l1p = torch.log1p(torch.exp(-x.abs()))
        e = torch.exp(-x.abs())
        T.append((x.clamp(min=0) - x * t + l1p) / BN)
        aT.append((4 * U * (x.clamp(min=0) + (x * t).abs() + l1p) + e / (1 + e) * U * x.abs() + 2 * U * l1p) / BN)
        cT.append((e / (1 + e) + l1p) / BN)
    if avg is not None:
        loga, pa, d_la, ce_la = _lsm(avg)
        d_pa, ce_pa = d_la + U * loga.abs(), ce_la + 1
        Da = logp - loga
        T.append(p * Da / BN)
        aT.append(p / BN * (d_p * Da.abs() + d_lp + d_la + 4 * U * Da.abs()))
        cT.append(p / BN * (ce_p * Da.abs() + ce_lp + ce_la))
        out['davg'] = (gs * (pa - p) / BN, gs / BN * (pa * d_pa + p * d_p + 4 * U * (pa + p)), gs / BN * (pa * ce_pa + p * ce_p))
    n_acc = 3 * K * math.ceil(NC / 256) * (2 if avg is not None else 1) + 10 + B + 1
    mag = sum(float(x.abs().sum()) for x in T) + abs(i['initial'])
    out['loss'] = (sum(x.sum() for x in T), sum(float(x.sum()) for x in aT) + n_acc * U * mag, sum(float(x.sum()) for x in cT))
    return out


def loss_autograd(i, c):
    """loss, dorg, davg from the project's oracles on float64 leaves (oracle.ga_convnext_oracle.ga_loss, oracle.map_oracle.
    multi_group_loss; the MAP oracle takes no BCE threshold, there the GA oracle's loss carries the same self-distillation term)"""
    from oracle import ga_convnext_oracle as O, map_oracle as MP
    import torch.nn.functional as Fn
    K = i['org'].shape[0]
    o = [i['org'][k].clone().requires_grad_(True) for k in range(K)]
    a = None if i['avg'] is None else [i['avg'][k].clone().requires_grad_(True) for k in range(K)]
    kind = 'bce' if c.kind else 'ce'
    tgt = i['target'] if i['dense'] is None else i['dense']
    thr = c.thr if (c.thr >= 0 and c.kind == 1) else None
    if a is not None and thr is None and K > 1:
        loss = MP.multi_group_loss([[x, y] for x, y in zip(o, a)], tgt, c.lam, kind, c.smooth)
    else:
        loss = O.ga_loss(o, tgt, c.lam, kind, c.smooth, thr)
        if a is not None:
            for x, y in zip(o, a):
                loss = loss + Fn.kl_div(Fn.log_softmax(y, dim=1), Fn.log_softmax(x, dim=1).detach(), reduction='sum', log_target=True) / x.numel()
    loss.backward()
    return dict(loss=loss.detach(), dorg=c.gs * torch.stack([x.grad for x in o]),
                davg=None if a is None else c.gs * torch.stack([y.grad for y in a]))


LOSS_WRONG = ['kl_over_B', 'undetached', 'smooth_nc_minus_1', 'bce_over_B', 'ce_p_minus_t', 'thr_under_ce', 'gs_on_loss']


def loss_restate(i, c, dt=F32, wrong=None):
    """the kernel's formulas in its order, evaluated by torch in dtype dt; `wrong` names one of LOSS_WRONG"""
    org = i['org'].to(dt)
    K, B, NC = org.shape
    lam, gs = c.lam, c.gs
    invB, invBN = 1.0 / B, 1.0 / (float(B) * float(NC))
    inv_kl = invB if wrong == 'kl_over_B' else invBN
    inv_bce = invB if wrong == 'bce_over_B' else invBN

    def lsm(x):
        m = x.max(-1, keepdim=True).values
        return x - (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True)))
    if i['dense'] is not None:
        t = i['dense'].to(dt)
    else:
        off = c.smooth / NC
        on = 1.0 - c.smooth + off
        if wrong == 'smooth_nc_minus_1' and NC > 1:
            off, on = c.smooth / (NC - 1), 1.0 - c.smooth
        t = torch.full((B, NC), off, dtype=dt)
        t[torch.arange(B), i['target']] = on
    if c.thr >= 0 and (c.kind == 1 or wrong == 'thr_under_ce'):
        t = (t > c.thr).to(dt)
    tsum = t.sum(-1, keepdim=True) if (i['dense'] is not None and c.kind == 0 and wrong != 'ce_p_minus_t') else torch.ones(B, 1, dtype=dt)
    mean = torch.zeros(B, NC, dtype=dt)
    for k in range(K):
        mean = mean + org[k]
    mean = mean / K
    logr = lsm(mean)
    rr = torch.exp(logr)
    logp = lsm(org)
    p = torch.exp(logp)
    D = logr - logp
    total = (lam * rr * D * inv_kl).sum()
    g = lam * inv_kl * (p - rr)
    if wrong == 'undetached':        # the gradient that flows through r when the mean is not detached
        klj = (rr * D).sum(-1, keepdim=True)
        g = g + (lam * inv_kl / K) * (rr * (D - klj)).sum(0, keepdim=True)
    if c.kind == 0:
        total = total + (-t * logp * invB).sum()
        g = g + (p * tsum - t) * invB
    else:
        total = total + ((org.clamp(min=0) - org * t + torch.log1p(torch.exp(-org.abs()))) * inv_bce).sum()
        g = g + (1.0 / (1.0 + torch.exp(-org)) - t) * inv_bce
    out = dict(dorg=(g * gs).to(F64), davg=None)
    if i['avg'] is not None:
        loga = lsm(i['avg'].to(dt))
        total = total + (p * (logp - loga) * invBN).sum()
        out['davg'] = ((torch.exp(loga) - p) * invBN * gs).to(F64)
    out['loss'] = (total * gs if wrong == 'gs_on_loss' else total).to(F64)
    return out


def loss_ratios(got, ref, dt, gs=1.0, eps=None):
    """got: dict of float64 tensors (loss = the increment); ref: loss_ref(); -> name -> worst ratio"""
    out = {}
    for n, (r, a0, ce) in ref.items():
        if got.get(n) is None:
            continue
        out[n] = gate(got[n], r, a0, 0.0 if n == 'loss' else r_of(dt), ce, eps, floor=TINY * max(1.0, gs))
    return out


def loss_need_eps(got, ref, dt, gs=1.0):
    return max(need_eps(got[n], r, a0, ce, 0.0 if n == 'loss' else r_of(dt), TINY * max(1.0, gs)) for n, (r, a0, ce) in ref.items()
               if got.get(n) is not None)


# ------------------------------------------------------------------------------------------------------------------------------
# heads_topk
# ------------------------------------------------------------------------------------------------------------------------------
def topk_ref(logits, topk):
    """logits fp32 [K][B][NC] -> (the k-ordered fp32 sum from 0, indices): NaN ranks largest, then by value, ties by lowest index"""
    s = torch.zeros_like(logits[0])
    for k in range(logits.shape[0]):
        s = s + logits[k]
    key = torch.where(s == 0, torch.zeros_like(s), s)
    return s, torch.sort(key, dim=1, descending=True, stable=True).indices[:, :topk]


def topk_restate(logits, topk, wrong=None):
    """the kernel's selection: topk passes, each takes the largest value not yet taken, NaN above everything, lowest index first.
    wrong = 'nan_as_inf' is the order heads_topk_kernel had before these tests: NaN stored as +inf, so that a +inf in front of a
    NaN was ranked above it"""
    s, _ = topk_ref(logits, topk)
    v = torch.where(s == 0, torch.zeros_like(s), s)
    nan, ninf = torch.isnan(v), torch.full_like(v, float('-inf'))
    taken, out = torch.zeros_like(nan), []
    for _ in range(topk):
        if wrong == 'nan_as_inf':
            k, free = torch.where(nan, -ninf, v), ~taken
        else:
            has = (nan & ~taken).any(1, keepdim=True)
            k, free = torch.where(nan, torch.zeros_like(v), v), torch.where(has, nan & ~taken, ~taken & ~nan)
        kk = torch.where(free, k, ninf)
        i = (free & (kk == kk.max(1, keepdim=True).values)).float().argmax(1)
        taken[torch.arange(v.shape[0]), i] = True
        out.append(i)
    return torch.stack(out, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# optimizers: float64 step functions over lists of tensors with a decay flag each
# ------------------------------------------------------------------------------------------------------------------------------
def hp_row(kind, lr, wd, b1=0.9, b2=0.999, eps=0.0, t=1, first=False, grad_averaging=True, max_grad_norm=1.0):
    """the fp32 hyper-parameter row optim.py pushes to the device, as float64 values of fp32 numbers"""
    if kind == 'sgd':
        row = [lr, wd, b1, 0.0, 0.0, 0.0, 0.0, 1.0 if first else 0.0]
    elif kind == 'adamw':
        row = [lr, wd, b1, b2, eps, 1 - b1 ** t, 1 - b2 ** t, 0.0]
    else:
        row = [lr, wd, b1, b2, eps, 1 - b1 ** t, 1 - b2 ** t, (1 - b1) if grad_averaging else 1.0, max_grad_norm]
    return torch.tensor(row, dtype=F64).to(F32)


def sgd_step(ps, gs, bufs, decay, lr, wd, mu, nesterov=True, first=False):
    """torch.optim.SGD (dampening 0).  -> new ps, new bufs, allowed {p, buf} per tensor"""
    P, Bf, Al = [], [], []
    for p, g, b, d in zip(ps, gs, bufs, decay):
        w = wd if d else 0.0
        g1 = g + w * p
        nb = g1.clone() if first else mu * b + g1
        dd = g1 + mu * nb if nesterov else nb
        Ag = g.abs() + w * p.abs()
        Ab = Ag if first else mu * b.abs() + Ag
        Ad = Ag + mu * Ab if nesterov else Ab
        P.append(p - lr * dd)
        Bf.append(nb)
        Al.append(dict(p=U * (2 * p.abs() + 8 * lr * Ad), buf=4 * U * Ab))
    return P, Bf, Al


def adamw_step(ps, gs, ms, vs, decay, lr, wd, b1, b2, eps, t=None, bc1=None, bc2=None):
    """torch.optim.AdamW.  -> new ps, ms, vs, allowed {p, m, v} per tensor"""
    bc1 = 1 - b1 ** t if bc1 is None else bc1
    bc2 = 1 - b2 ** t if bc2 is None else bc2
    P, M, V, Al = [], [], [], []
    for p, g, m, v, d in zip(ps, gs, ms, vs, decay):
        w = wd if d else 0.0
        m1 = b1 * m + (1 - b1) * g
        v1 = b2 * v + (1 - b2) * g * g
        den = v1.sqrt() / math.sqrt(bc2) + eps
        step = lr / bc1 / den
        Am = b1 * m.abs() + (1 - b1) * g.abs()
        P.append(p * (1 - lr * w) - step * m1)
        M.append(m1)
        V.append(v1)
        Al.append(dict(m=3 * U * Am, v=4 * U * v1, p=U * (4 * p.abs() + step * (3 * Am + 13 * m1.abs()))))
    return P, M, V, Al


def n_sumsq(n):
    """roundings a term of ga_sumsq_f32's positive sum passes through"""
    n4 = max(1, n // 4)
    blocks = max(1, min(2048, (n4 + 255) // 256))
    return 7 * math.ceil(n4 / (256 * blocks)) + 1 + 10 + blocks


def lamb_step(ps, gs, ms, vs, decay, lr, wd, b1, b2, eps, t=None, max_grad_norm=1.0, grad_averaging=True, bc1=None, bc2=None, b3=None,
              chunk=LAMB_CHUNK):
    """LAMB as published (You et al. 2020) in timm's arrangement, the eight steps of the module docstring.
    -> dict of per-tensor lists p, m, v, u, norms [(sum p^2, sum u^2)], trust, and `allowed` with the same keys"""
    bc1 = 1 - b1 ** t if bc1 is None else bc1
    bc2 = 1 - b2 ** t if bc2 is None else bc2
    b3 = ((1 - b1) if grad_averaging else 1.0) if b3 is None else b3
    total = sum(g.numel() for g in gs)
    gn = math.sqrt(sum(float((g * g).sum()) for g in gs))                     # 1
    clip = max_grad_norm / gn if gn > max_grad_norm else 1.0                  # 2:  g / (gn / max)
    e_g = U * (n_sumsq(total) / 2 + 1) + 2 * U if gn > max_grad_norm else 0.0
    out = dict(p=[], m=[], v=[], u=[], norms=[], trust=[], allowed=[], gn=gn)
    for p, g, m, v, d in zip(ps, gs, ms, vs, decay):
        gi = g * clip
        m1 = b1 * m + b3 * gi                                                 # 3
        v1 = b2 * v + (1 - b2) * gi * gi                                      # 4
        den = v1.sqrt() / math.sqrt(bc2) + eps
        a = (m1 / bc1) / den                                                  # 5
        w = wd if d else 0.0
        u = a + w * p                                                         # 6
        sp, su = float((p * p).sum()), float((u * u).sum())
        trust = math.sqrt(sp) / math.sqrt(su) if (d and wd != 0 and sp > 0 and su > 0) else 1.0       # 7
        p1 = p - lr * trust * u                                               # 8
        a_m = 3 * U * (b1 * m.abs() + b3 * gi.abs()) + e_g * b3 * gi.abs()
        a_v = 4 * U * v1 + 2 * e_g * (1 - b2) * gi * gi
        relv = torch.where(v1 > 0, a_v / (2 * v1.clamp(min=1e-300)), torch.zeros_like(v1))
        a_u = a_m / (bc1 * den) + a.abs() * (relv + 10 * U) + U * (3 * w * p.abs() + a.abs())
        cn = math.ceil(min(p.numel(), chunk) / 256) + 10 + math.ceil(p.numel() / chunk)
        a_sp = U * cn * sp
        a_su = U * (cn + 1) * su + 2 * float((u.abs() * a_u).sum())
        e_tr = (a_sp / (2 * sp) + a_su / (2 * su) + 3 * U) if trust != 1.0 else 0.0
        a_p = U * (p.abs() + 3 * lr * trust * u.abs()) + lr * trust * (u.abs() * e_tr + a_u)
        for k, x in (('p', p1), ('m', m1), ('v', v1), ('u', u), ('norms', (sp, su)), ('trust', trust)):
            out[k].append(x)
        out['allowed'].append(dict(p=a_p, m=a_m, v=a_v, u=a_u, norms=(a_sp, a_su)))
    return out


# ---- restatements in the kernels' order, in dtype dt, with the wrong variants the gate must reject
SGD_WRONG = ['stale_buf_first', 'no_nesterov']
ADAMW_WRONG = ['coupled_decay', 'no_bc1']
LAMB_WRONG = ['trust_per_chunk', 'trust_no_decay', 'trust_from_g', 'l2_decay', 'eps_before_bc2', 'bc2_no_sqrt', 'beta3_one',
              'clip_scales_up', 'stale_norms']
CLIP_WRONG = ['no_1e-6', 'agc_eps_on_gnorm']


def _s(x, dt):
    return torch.tensor(float(x), dtype=dt)


def sgd_restate(p, g, buf, hp, nesterov, wd_mult, dt=F32, wrong=None):
    lr, wd, mu, first = hp[0].to(dt), hp[1].to(dt) * wd_mult, hp[2].to(dt), float(hp[7]) != 0.0
    p, g, buf = p.to(dt), g.to(dt), buf.to(dt)
    gi = g + wd * p
    bi = gi if (first and wrong != 'stale_buf_first') else mu * buf + gi
    gi = gi + mu * bi if (nesterov and wrong != 'no_nesterov') else bi
    return (p - lr * gi).to(F64), bi.to(F64)


def adamw_restate(p, g, m, v, hp, wd_mult, dt=F32, wrong=None):
    lr, wd, b1, b2, eps, bc1, bc2 = (hp[k].to(dt) for k in range(7))
    wd = wd * wd_mult
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    if wrong == 'coupled_decay':
        g = g + wd * p
    step = lr if wrong == 'no_bc1' else lr / bc1
    mi = b1 * m + (1 - b1) * g
    vi = b2 * v + (1 - b2) * g * g
    pi = p if wrong == 'coupled_decay' else p * (1 - lr * wd)
    return (pi - step * mi / (vi.sqrt() * torch.rsqrt(bc2) + eps)).to(F64), mi.to(F64), vi.to(F64)


def lamb_restate(ps, gs, ms, vs, decay, hp, norms, dt=F32, wrong=None, chunk=LAMB_CHUNK):
    """ga_sumsq_f32 + ga_lamb_stage1 + ga_lamb_stage2 over the chunk table; `norms` [ntensors][2] (dt) is the device buffer the plan
    re-zeroes: it is passed in so that `stale_norms` can leave the previous step's sums in place.  -> dict like lamb_step"""
    lr, wd, b1, b2, eps, bc1, bc2, b3, mx = (hp[k].to(dt) for k in range(9))
    ps, gs, ms, vs = ([x.to(dt) for x in l] for l in (ps, gs, ms, vs))
    gsum = torch.zeros((), dtype=dt)
    for g in gs:
        gsum = gsum + (g * g).sum()
    gn = gsum.sqrt()
    iclip = mx / gn if gn > mx else _s(1.0, dt)
    if wrong == 'clip_scales_up' and gn > 0:
        iclip = mx / gn
    if wrong == 'beta3_one':
        b3 = _s(1.0, dt)
    if wrong != 'stale_norms':
        norms.zero_()
    out = dict(p=[], m=[], v=[], u=[], norms=[])
    per_chunk = []
    for ti, (p, g, m, v, d) in enumerate(zip(ps, gs, ms, vs, decay)):
        w = wd if d else _s(0.0, dt)
        gi = g * iclip
        if wrong == 'l2_decay':
            gi = gi + w * p
        mi = b1 * m + b3 * gi
        vi = b2 * v + (1 - b2) * gi * gi
        if wrong == 'eps_before_bc2':
            den = (vi.sqrt() + eps) * torch.rsqrt(bc2)
        elif wrong == 'bc2_no_sqrt':
            den = vi.sqrt() / bc2 + eps
        else:
            den = vi.sqrt() * torch.rsqrt(bc2) + eps
        up = (mi * (1 / bc1)) / den
        if wrong != 'l2_decay':
            up = up + w * p
        nrm_u = gi if wrong == 'trust_from_g' else up
        pc = []
        for c0 in range(0, p.numel(), chunk):
            sp, su = (p[c0:c0 + chunk] ** 2).sum(), (nrm_u[c0:c0 + chunk] ** 2).sum()
            norms[ti, 0] += sp
            norms[ti, 1] += su
            pc.append((sp, su))
        per_chunk.append(pc)
        out['m'].append(mi.to(F64))
        out['v'].append(vi.to(F64))
        out['u'].append(up.to(F64))
    for ti, (p, d) in enumerate(zip(ps, decay)):
        up = out['u'][ti].to(dt)
        p1 = p.clone()
        for ci, c0 in enumerate(range(0, p.numel(), chunk)):
            trust = _s(1.0, dt)
            if (d or wrong == 'trust_no_decay') and float(wd) != 0.0:
                sp, su = per_chunk[ti][ci] if wrong == 'trust_per_chunk' else (norms[ti, 0], norms[ti, 1])
                wn, un = sp.sqrt(), su.sqrt()
                if wn > 0 and un > 0:
                    trust = wn / un
            p1[c0:c0 + chunk] = p[c0:c0 + chunk] - (lr * trust) * up[c0:c0 + chunk]
        out['p'].append(p1.to(F64))
        out['norms'].append((float(norms[ti, 0]), float(norms[ti, 1])))
    return out


def lamb_ratios(got, ref):
    """got: dict of per-tensor lists (float64) -> name -> worst ratio over the tensors"""
    out = {}
    for n in ('p', 'm', 'v', 'u'):
        if n in got:
            out[n] = max(gate(x, r, al[n]) for x, r, al in zip(got[n], ref[n], ref['allowed']))
    if 'norms' in got:
        out['norms'] = max(max(gate(x[k], r[k], al['norms'][k]) for k in (0, 1)) for x, r, al in zip(got['norms'], ref['norms'], ref['allowed']))
    return out


LAMB_SIZES = [1, 63, 64, 257, 16384, 16385, 40000, 7, 300]
LAMB_NDECAY = 6
LAMB_STEPS = 3
# label -> wd, eps, grad_averaging, gradient scale (global norm ~ 240 x scale against max_grad_norm 1), all gradients zero
LAMB_CASES = {
    'clipped': dict(wd=0.05, eps=1e-6, avg=True, gscale=1.0, zero_g=False),
    'unclipped': dict(wd=0.05, eps=1e-8, avg=False, gscale=1e-3, zero_g=False),
    'wd0': dict(wd=0.0, eps=1e-6, avg=True, gscale=1e-3, zero_g=False),
    'zero_grads': dict(wd=0.05, eps=1e-8, avg=True, gscale=0.0, zero_g=True),
}
LAMB_ZERO_P, LAMB_ZERO_G = 2, 3     # decay tensors: the one whose parameters are all zero, the one whose gradient is zero
LAMB_LR, BETAS = 5e-3, (0.9, 0.999)


def lamb_inputs(label):
    """p0 per tensor and the gradients of LAMB_STEPS steps, float64 values of fp32 numbers"""
    c = LAMB_CASES[label]
    g = torch.Generator().manual_seed(900 + sorted(LAMB_CASES).index(label))
    p0 = [(torch.randn(n, generator=g, dtype=F32) * (0.02 * (1 + i % 3))).to(F64) for i, n in enumerate(LAMB_SIZES)]
    p0[LAMB_ZERO_P].zero_()
    grads = []
    for s in range(LAMB_STEPS):
        gs = [(torch.randn(n, generator=g, dtype=F32) * c['gscale']).to(F64) for n in LAMB_SIZES]
        gs[LAMB_ZERO_G].zero_()
        grads.append(gs)
    return p0, grads


def decay_flags(sizes=LAMB_SIZES, n_decay=LAMB_NDECAY):
    return [i < n_decay for i in range(len(sizes))]


# ------------------------------------------------------------------------------------------------------------------------------
# clipping
# ------------------------------------------------------------------------------------------------------------------------------
def sumsq_ref(x):
    s = float((x * x).sum())
    return s, U * n_sumsq(x.numel()) * s


def clip_norm_ref(g, limit):
    """torch.nn.utils.clip_grad_norm_: g *= min(1, limit / (|g| + 1e-6)).  -> ref, a0"""
    n = math.sqrt(float((g * g).sum()))
    coef = min(1.0, limit / (n + 1e-6))
    ref = g * coef
    return ref, ref.abs() * U * (n_sumsq(g.numel()) / 2 + 4), coef


def clip_norm_restate(g, limit, dt=F32, wrong=None):
    g = g.to(dt)
    coef = _s(limit, dt) / ((g * g).sum().sqrt() + (0.0 if wrong == 'no_1e-6' else _s(1e-6, dt)))
    return (g if coef >= 1 else g * coef).to(F64)


def agc_ref(p, g, units, clip_factor, eps=1e-3):
    """timm adaptive_clip_grad per unit (offset, length) of the flat buffers.  -> ref, a0, clipped flag per unit"""
    ref, a0, flags = g.clone(), torch.zeros_like(g), []
    for off, ln in units:
        pp, gg = p[off:off + ln], g[off:off + ln]
        mx = max(math.sqrt(float((pp * pp).sum())), eps) * clip_factor
        gn = math.sqrt(float((gg * gg).sum()))
        n = math.ceil(ln / 64) + 6
        if gn >= mx:
            ref[off:off + ln] = gg * (mx / max(gn, 1e-6))
        # the two norms (n roundings each, halved by the square roots), sqrt 2, max_norm 1, quotient 1, product 1; a unit at the
        # threshold may go either way: the factor is 1 within the same bound
        a0[off:off + ln] = ref[off:off + ln].abs() * U * (n + 5)
        flags.append(0 if gn < mx * (1 - 1e-3) else (2 if gn > mx * (1 + 1e-3) else 1))
    return ref, a0, flags


def agc_restate(p, g, units, clip_factor, eps=1e-3, dt=F32, wrong=None):
    p, out = p.to(dt), g.to(dt).clone()
    for off, ln in units:
        pp, gg = p[off:off + ln], out[off:off + ln].clone()
        mx = torch.maximum((pp * pp).sum().sqrt(), _s(eps, dt)) * _s(clip_factor, dt)
        gn = (gg * gg).sum().sqrt()
        if gn >= mx:
            out[off:off + ln] = gg * (mx / torch.maximum(gn, _s(eps if wrong == 'agc_eps_on_gnorm' else 1e-6, dt)))
    return out.to(F64)


def agc_inputs(lengths, nunits):
    """units of the given lengths (cycled) laid end to end with gaps, |p| ~ 0.1 per element; unit 0 clearly unclipped, unit 1
    clearly clipped, unit 2 exactly at the threshold (|g| = clip_factor |p| by construction), unit 3: |p| < eps and
    eps * clip_factor < |g| < eps, where the 1e-6 floor and the eps floor differ"""
    g = torch.Generator().manual_seed(77 + nunits + sum(lengths))
    units, off = [], 3
    for u in range(nunits):
        ln = lengths[u % len(lengths)]
        units.append((off, ln))
        off += ln + 5
    p = (torch.randn(off, generator=g, dtype=F32) * 0.1).to(F64)
    gr = torch.randn(off, generator=g, dtype=F32).to(F64)
    for u, (o, ln) in enumerate(units):
        if u % 4 == 0:
            gr[o:o + ln] *= 1e-4
        elif u % 4 == 2:
            gr[o:o + ln] = p[o:o + ln] * 0.02
        elif u % 4 == 3:
            p[o:o + ln] *= 1e-4 / math.sqrt(ln)
            gr[o:o + ln] *= 1e-4 / math.sqrt(ln)
    return p, gr.to(F32).to(F64), units


# ------------------------------------------------------------------------------------------------------------------------------
# samplers: the documented generator in integers
# ------------------------------------------------------------------------------------------------------------------------------
_M = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def random24(seed, call, n):
    """the top 24 bits of splitmix64(splitmix64(seed ^ call * 0xD1342543DE82EF95) + i), i < n"""
    with np.errstate(over='ignore'):
        base = splitmix64(np.uint64(seed) ^ (np.uint64(call) * np.uint64(0xD1342543DE82EF95)))
        h = splitmix64(base + np.arange(n, dtype=np.uint64))
    return (h >> np.uint64(40)).astype(np.int64)


def _mask(u24, keep32):
    """u24 2^-24 < keep in fp32 (both sides exact there) ? 1 / keep (one fp32 division) : 0"""
    keep32 = np.asarray(keep32, dtype=np.float32)
    return np.where(u24.astype(np.float64) < keep32.astype(np.float64) * 16777216.0, np.float32(1.0) / keep32, np.float32(0.0)).astype(np.float32)


def dropout_mask_ref(n, keep, seed, call):
    return _mask(random24(seed, call, n), np.float32(keep))


def drop_path_ref(keep, sites, B, seed, call):
    """keep: fp32 per site -> [sites][B]"""
    k = np.repeat(np.asarray(keep, dtype=np.float32), B)
    return _mask(random24(seed, call, sites * B), k).reshape(sites, B)


# ------------------------------------------------------------------------------------------------------------------------------
# FlatStub: what the fused optimizers need of a model, on arbitrary tensor sizes
# ------------------------------------------------------------------------------------------------------------------------------
class FlatStub:
    """flat fp32 parameter / gradient buffers of tensors of the given sizes laid end to end, the first n_decay_tensors of them
    in the weight-decay segment: enough to construct FusedSGD / FusedAdamW / FusedLamb.  params / grads may be given (views of
    guarded allocations)"""

    def __init__(self, sizes, n_decay_tensors, device='cuda', params=None, grads=None):
        from collections import OrderedDict
        self.sizes = list(sizes)
        total = sum(self.sizes)
        self.slices, off = OrderedDict(), 0
        for i, n in enumerate(self.sizes):
            self.slices[f't{i}'] = (off, n)
            off += n
        self._flat = dict(params=torch.zeros(total, device=device) if params is None else params,
                          grads=torch.zeros(total, device=device) if grads is None else grads,
                          n_decay=sum(self.sizes[:n_decay_tensors]), total=total, slices=self.slices, gen=1)
        self._engines = {}

    def flat_state(self):
        return self._flat

    def check_flat_generation(self, gen, who):
        assert gen == self._flat['gen'], who

    def split(self, flat):
        return [flat[o:o + n] for o, n in self.slices.values()]
