"""Float64 closed form of what csrc/loss_jsd.hip computes (ga_loss_jsd_fwd_bwd: timm's JsdCrossEntropy per head over S augmentation
splits, plus the head-decorrelation and self-distillation terms of the ordinary loss), its rounding-count allowance for the gate of
tests/_loss_optim_ref.py, an fp32 restatement in the kernel's order, three wrong restatements the gate has to reject, and the case
table shared by tests/test_loss_jsd_ref_cpu.py and tests/test_loss_jsd_edges_gpu.py.

Layout: org / avg [K][B][NC], B = S Bs, split-major: row i + s Bs is split s of base sample i; target [Bs].  With logp = x - lse(x)
(never log(p)), p = exp(logp), per head and base sample:
    q_c  = mean_s p_sc,   m_c = clamp(q_c, 1e-7, 1),   u_c = 1 where 1e-7 <= q_c <= 1 (the clamp passes its gradient at equality)
    loss = CE_smooth(x_0, y) / Bs + A sum_sc p_sc (logp_sc - log m_c),                 A = alpha / (S Bs) = alpha / B
    g_sc = A [ (logp_sc - log m_c) + 1 - u_c q_c / m_c ]  =  A [ (logp_sc - log m_c) + (1 - u_c) ]     (m = q where u = 1)
    dx_sc = p_sc (g_sc - sum_c' p_sc' g_sc')  ( + (p_0c - t_c) / Bs on split 0 )
This is the reference, NOT autograd: where p underflows to 0 torch's xlogy derivative is 0 / 0 = NaN, the closed form in log space
(and the kernel) gives the limit 0.  tests/test_loss_jsd_ref_cpu.py holds it to float64 autograd wherever nothing underflows.
The decorrelation term lam KL_mean(logp_k || log_softmax(mean_j out_j)) and the `avg` term run over all B rows unchanged: their
values, gradients and allowances are R.loss_ref's own, evaluated with an all-zero dense target (which makes its CE part exactly 0).

Allowance (a0 in units of U = 2^-24 per fp32 rounding of the magnitude it rounds, ce per hardware exp / log, as in R's docstring;
d(logp), d(p) / p = d(logp) + U |logp|, ce(logp) = 1 + |log s|, ce(p) = ce(logp) + 1 are R._lsm's):
    q      S - 1 additions and the division, each at most U of the partial sum <= S q: d(q) = sum_s p_s d(p_s)/p_s / S + S U q;
           ce(q) = sum_s p_s ce(p_s) / S
    log m  __logf: 1 v_log (relative to |log m|), 1 rounding of |log m| in the product with ln 2, the fp32 constant 1e-7f (2^-26
           relative): d(log m) = u d(q) / q + 2 U |log m| + U,  ce(log m) = u ce(q) / q + |log m|
    D      = logp - log m, 1 rounding: d(D) = d(logp) + d(log m) + U |D|,  ce(D) = ce(logp) + ce(log m)
    value  A (p D): A = alpha / B 1, p D 1, A . 1: d = A p (d(D) + |D| (d(p)/p + 3 U)),  ce = A p (ce(D) + |D| ce(p))
    g      A (D + (1 - u)): the sum 1, A 1, the product 1: d(g) = A d(D) + 3 U |g|,  ce(g) = A ce(D)
    dot_s  sum_c p g: per term p d(g) + p |g| (d(p)/p + U), then ceil(NC / 256) + 10 additions (R._chain) of sum_c p |g|
    dx     p (g - dot): the difference 1, the product 1: d = p (d(g) + d(dot) + U |g - dot|) + |dx| (d(p)/p + U)
    CE     (p - t) / Bs on split 0: p's error, the difference, 1 / Bs and the product 3 U, on / off 3 U |t| (R's CE count
           without the row sum of a dense target); value -t logp / Bs: |t| (d(logp) + 3 U |logp|) / Bs
    dorg   the three parts are added (2 roundings) and scaled by grad_scale (1): 3 U (|kl| + |dx| + |ce|) on top of the parts
    loss   a thread adds (3 S + 1) terms per column and head ((2 S + 1) without avg), then six wave steps, four partials and one
           atomic per workgroup: n_acc = (3 S + 1) K ceil(NC / 256) + 10 + Bs + 1 roundings of (sum of |terms| + |initial|)
    flush  v_exp_f32 returns 0 for a result below 2^-126 (no subnormal results), so p carries an ABSOLUTE error of up to TINY =
           2^-126 besides its relative one.  R's floor covers that where p enters with a factor <= 1 (the decorrelation, avg and
           CE gradients); in the JSD terms it is multiplied by |g - dot|, A |D| and |g|, which are not: TINY |g - dot| on dx, TINY
           sum_c |g| on dot, TINY A |D| on the value.  This is the same underflow the kernel answers with the limit 0
The clamp makes the gradient discontinuous at q = 1e-7: a column whose float64 q lies within the derived relative error of the fp32
q, band_rel = d(q) / q + eps ce(q) / q, of 1e-7 can fall on either side and is named by JsdRef.near_clamp; the tests assert that no
column of their seeds does (change the seed, not the band)."""
import math

import torch

import _loss_optim_ref as R
from _loss_optim_ref import BF, F32, F64, R_BF16, TINY, U, gate, need_eps      # noqa: F401  (re-exported for the tests)

CLAMP_LO = 1e-7
LDS_OPT_IN = 65536            # dynamic LDS above this takes the hipFuncSetAttribute opt-in
LDS_MAX = 160 * 1024          # refused above


def lds_bytes(S, NC):
    """include/gaext.h: the S log r rows + 8 floats of reduction scratch"""
    return 4 * (S * NC + 8)


class JsdCase:
    def __init__(self, K, Bs, S, NC, smooth, avg, gs, regime, seed):
        self.K, self.Bs, self.S, self.NC, self.smooth, self.avg, self.gs, self.regime, self.seed = K, Bs, S, NC, smooth, avg, gs, regime, seed
        self.B, self.lam, self.alpha = S * Bs, -0.8, 12.0
        self.label = f'K{K}-Bs{Bs}-S{S}-NC{NC}-s{smooth}-{"avg" if avg else "noavg"}-gs{gs}-{regime}'

    def __repr__(self):
        return self.label


JSD_CASES = [JsdCase(*a, seed=n) for n, a in enumerate([
    (1, 1, 2, 1, 0.0, False, 1.0, 'randn2'),
    (5, 3, 2, 2, 0.1, True, 0.25, 'randn2'),
    (1, 1, 3, 63, 0.1, False, 65536.0, 'randn8'),
    (5, 3, 4, 64, 0.0, True, 1.0, 'same'),
    (5, 1, 8, 65, 0.1, False, 1.0, 'randn2'),
    (1, 3, 2, 255, 0.0, True, 0.25, 'spike'),
    (5, 3, 3, 256, 0.1, False, 1.0, 'const'),
    (5, 1, 4, 257, 0.1, True, 65536.0, 'randn30'),
    (5, 3, 3, 1000, 0.1, False, 1.0, 'randn2'),
    (5, 3, 3, 1000, 0.1, True, 1.0, 'randn8'),
    (5, 3, 3, 1000, 0.0, False, 0.25, 'randn30'),
    (1, 1, 8, 1000, 0.1, True, 1.0, 'randn8'),
    (5, 1, 2, 1000, 0.1, False, 1.0, 'spike'),
    (1, 3, 4, 1000, 0.0, False, 1.0, 'same'),
    (1, 1, 2, 8188, 0.1, True, 1.0, 'randn2'),           # 4 (2 * 8188 + 8) = 65536: the last size without the opt-in
    (1, 1, 2, 8189, 0.0, False, 0.25, 'randn8'),         # the first with it
    (1, 1, 8, 2047, 0.1, False, 1.0, 'randn2'),          # the same edge at S = 8
    (5, 1, 8, 2048, 0.1, True, 1.0, 'randn30'),
    (1, 1, 2, 20476, 0.1, False, 1.0, 'randn8'),         # 4 (2 * 20476 + 8) = 163840: the largest the entry point takes
    (1, 3, 8, 5119, 0.0, True, 65536.0, 'randn8'),       # the same bound at S = 8
    (5, 3, 4, 257, 0.1, False, 1.0, 'randn8'),
    (1, 3, 3, 64, 0.1, True, 1.0, 'spike'),
    (5, 1, 3, 65, 0.0, False, 1.0, 'const'),
    (1, 3, 2, 2, 0.0, False, 1.0, 'same'),
    (5, 3, 8, 63, 0.1, True, 0.25, 'randn30'),
])]


def jsd_inputs(c):
    """float64 tensors whose values are fp32 values: org, avg (or None) [K][B][NC], target int64 [Bs], the initial loss"""
    g = torch.Generator().manual_seed(7100 + c.seed)
    K, B, Bs, S, NC = c.K, c.B, c.Bs, c.S, c.NC
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F32).to(F64)
    if c.regime in ('randn2', 'randn8', 'randn30'):
        org = (rn(K, B, NC) * float(c.regime[5:])).to(F32).to(F64)
    elif c.regime == 'same':                   # every split holds the same rows: the JSD term and its gradient vanish
        org = (rn(K, 1, Bs, NC) * 2).expand(K, S, Bs, NC).reshape(K, B, NC).clone()
    elif c.regime == 'spike':                  # one logit 120 above the rest, in split 1 only: p underflows in fp32, not in float64
        org = rn(K, B, NC) * 2
        for k in range(K):
            for i in range(Bs):
                col = (7 * k + 3 * i) % NC
                org[k, Bs + i, :] = org[k, Bs + i, :].clamp(-4, 4)
                org[k, Bs + i, col] = 124.0
    elif c.regime == 'const':
        org = rn(K, B, NC) * 2
        org[:, 0, :] = 1.5
        org[:, B - 1, :] = -2.25
    else:
        raise ValueError(c.regime)
    t = torch.randint(0, NC, (Bs,), generator=g)
    t[0] = NC - 1
    if Bs > 1:
        t[1] = 0
    return dict(org=org, avg=(rn(K, B, NC) * 2) if c.avg else None, target=t, initial=3.25)


def _zero_dense_case(c):
    """R.loss_ref with a dense all-zero target under CE: exactly the decorrelation and avg terms, with their allowances"""
    return R.LossCase('decor', c.K, c.B, c.NC, 0, 0.0, 'dense', -1.0, c.avg, c.gs, c.regime)


class JsdRef:
    """closed form + allowance of one case: .out = name -> (ref, a0, ce) for 'loss' (the increment), 'dorg', 'davg';
    .clamped [K][Bs][NC] bool, .near_clamp(eps) -> bool mask of the columns the gradient comparison cannot decide"""

    def __init__(self, i, c):
        org = i['org']
        K, B, NC = org.shape
        S, Bs, gs, A = c.S, c.Bs, c.gs, c.alpha / B
        base = R.loss_ref(dict(org=org, avg=i['avg'], target=None, dense=torch.zeros(B, NC, dtype=F64), initial=i['initial']),
                          _zero_dense_case(c))
        logp, p, d_lp, ce_lp = R._lsm(org)
        v = lambda x: x.reshape(K, S, Bs, NC)
        logp, p, d_lp, ce_lp = v(logp), v(p), v(d_lp), v(ce_lp)
        rel_p, ce_p = d_lp + U * logp.abs(), ce_lp + 1
        q = p.mean(1, keepdim=True)
        u = ((q >= CLAMP_LO) & (q <= 1.0)).to(F64)
        m = q.clamp(CLAMP_LO, 1.0)
        logm = torch.log(m)
        d_q = (p * rel_p).sum(1, keepdim=True) / S + S * U * q
        ce_q = (p * ce_p).sum(1, keepdim=True) / S
        qs = q.clamp(min=1e-300)
        d_lm = u * d_q / qs + 2 * U * logm.abs() + U
        ce_lm = u * ce_q / qs + logm.abs()
        D = logp - logm
        d_D, ce_D = d_lp + d_lm + U * D.abs(), ce_lp + ce_lm
        # ---- value
        T_j = A * p * D
        a_j = A * p * (d_D + D.abs() * (rel_p + 3 * U)) + TINY * A * D.abs()
        c_j = A * p * (ce_D + D.abs() * ce_p)
        # ---- gradient of the JSD term
        gg = A * (D + (1 - u))
        d_g, ce_g = A * d_D + 3 * U * gg.abs(), A * ce_D
        pg = p * gg.abs()
        dot = (p * gg).sum(-1, keepdim=True)
        d_dot = (p * d_g + pg * (rel_p + U) + TINY * gg.abs()).sum(-1, keepdim=True) + R._chain(NC) * U * pg.sum(-1, keepdim=True)
        ce_dot = (p * (ce_g + gg.abs() * ce_p)).sum(-1, keepdim=True)
        dx = p * (gg - dot)
        a_dx = p * (d_g + d_dot + U * (gg - dot).abs()) + dx.abs() * (rel_p + U) + TINY * (gg - dot).abs()
        c_dx = p * (ce_g + ce_dot) + dx.abs() * ce_p
        # ---- smoothed CE on split 0, mean over Bs
        off = c.smooth / NC
        t = torch.full((Bs, NC), off, dtype=F64)
        t[torch.arange(Bs), i['target']] = 1.0 - c.smooth + off
        gh, a_h, c_h = torch.zeros_like(dx), torch.zeros_like(dx), torch.zeros_like(dx)
        gh[:, 0] = (p[:, 0] - t) / Bs
        a_h[:, 0] = (p[:, 0] * (rel_p[:, 0] + 3 * U) + 3 * U * t) / Bs
        c_h[:, 0] = p[:, 0] * ce_p[:, 0] / Bs
        T_c = -t * logp[:, 0] / Bs
        a_c = t / Bs * (d_lp[:, 0] + 3 * U * logp[:, 0].abs())
        c_c = t / Bs * ce_lp[:, 0]
        # ---- together with the imported terms
        kl, a_kl, c_kl = base['dorg']
        f = lambda x: x.reshape(K, B, NC)
        new = gs * f(dx + gh)
        self.out = {'dorg': (kl + new, a_kl + gs * f(a_dx + a_h) + 3 * U * (kl.abs() + gs * f(dx.abs() + gh.abs())), c_kl + gs * f(c_dx + c_h))}
        if 'davg' in base:
            self.out['davg'] = base['davg']
        l0, a_l0, c_l0 = base['loss']
        nchunk = math.ceil(NC / 256)
        n_acc = ((3 if i['avg'] is not None else 2) * S + 1) * K * nchunk + 10 + Bs + 1
        n_imp = 3 * K * nchunk * (2 if i['avg'] is not None else 1) + 10 + B + 1
        mag_new = float(T_j.abs().sum() + T_c.abs().sum())
        mag_imp = float(l0.abs()) + abs(i['initial'])          # at least |sum|; the imported bound holds the sum of |terms| itself
        self.out['loss'] = (l0 + T_j.sum() + T_c.sum(),
                            a_l0 + float(a_j.sum() + a_c.sum()) + n_acc * U * mag_new + max(0, n_acc - n_imp) * U * mag_imp,
                            c_l0 + float(c_j.sum() + c_c.sum()))
        self.clamped = (u == 0).squeeze(1)
        self.q, self.band_a, self.band_c = q.squeeze(1), (d_q / qs).squeeze(1), (ce_q / qs).squeeze(1)
        self.parts = dict(jsd=T_j.sum(), ce=T_c.sum(), decor=l0, dx=f(dx), gh=f(gh))

    def near_clamp(self, eps=R.EPS_FAST):
        """[K][Bs][NC]: float64 q within the fp32 q's derived relative error of the clamp's lower end"""
        return (self.q / CLAMP_LO - 1).abs() <= self.band_a + eps * self.band_c


JSD_WRONG = ['clamp_ignored', 'ce_all_rows', 'batchmean_over_B']


def jsd_restate(i, c, dt=F32, wrong=None):
    """the kernel's formulas in its order, evaluated by torch in dtype dt; `wrong` names one of JSD_WRONG"""
    org = i['org'].to(dt)
    K, B, NC = org.shape
    S, Bs, lam, gs = c.S, c.Bs, c.lam, c.gs
    invBs, invBN = 1.0 / Bs, 1.0 / (float(B) * float(NC))
    A = c.alpha / B
    if wrong == 'batchmean_over_B':
        A = c.alpha / (S * B)
    if wrong == 'ce_all_rows':
        invBs = 1.0 / B
    lo = torch.tensor(CLAMP_LO, dtype=dt)

    def lsm(x):
        mx = x.max(-1, keepdim=True).values
        return x - (mx + torch.log(torch.exp(x - mx).sum(-1, keepdim=True)))
    mean = torch.zeros(B, NC, dtype=dt)
    for k in range(K):
        mean = mean + org[k]
    logr = lsm(mean / K)
    rr = torch.exp(logr)
    logp = lsm(org)
    p = torch.exp(logp)
    total = (lam * rr * (logr - logp) * invBN).sum()
    g = lam * invBN * (p - rr)
    lp4, p4 = logp.view(K, S, Bs, NC), p.view(K, S, Bs, NC)
    q = torch.zeros(K, 1, Bs, NC, dtype=dt)
    for s in range(S):
        q = q + p4[:, s:s + 1]
    q = q / S
    logm = torch.log(q.clamp(lo, 1.0))
    extra = torch.zeros_like(q) if wrong == 'clamp_ignored' else ((q < lo) | (q > 1.0)).to(dt)
    D = lp4 - logm
    total = total + (A * (p4 * D)).sum()
    gj = A * (D + extra)
    dot = (p4 * gj).sum(-1, keepdim=True)
    g = g + (p4 * (gj - dot)).reshape(K, B, NC)
    off = c.smooth / NC
    on = 1.0 - c.smooth + off
    t = torch.full((Bs, NC), off, dtype=dt)
    t[torch.arange(Bs), i['target']] = on
    rows = range(S) if wrong == 'ce_all_rows' else (0,)
    g = g.view(K, S, Bs, NC).clone()
    for s in rows:
        total = total + (-t * lp4[:, s] * invBs).sum()
        g[:, s] += (p4[:, s] - t) * invBs
    out = dict(dorg=(g.reshape(K, B, NC) * gs).to(F64), davg=None)
    if i['avg'] is not None:
        loga = lsm(i['avg'].to(dt))
        total = total + (p * (logp - loga) * invBN).sum()
        out['davg'] = ((torch.exp(loga) - p) * invBN * gs).to(F64)
    out['loss'] = total.to(F64)
    return out


def jsd_autograd(i, c):
    """float64 autograd of the reference's own formulation: timm JsdCrossEntropy per head (GA/train.py:737-739), the decorrelation
    term on the detached head mean and MAP's avg term.  NaN where a probability underflows (the xlogy derivative)"""
    import torch.nn.functional as Fn
    K, S = c.K, c.S
    o = [i['org'][k].clone().requires_grad_(True) for k in range(K)]
    a = None if i['avg'] is None else [i['avg'][k].clone().requires_grad_(True) for k in range(K)]
    tgt = i['target']
    loss = 0.0
    mean_log = Fn.log_softmax(torch.stack([x.detach() for x in o]).mean(0), dim=-1)
    for k in range(K):
        split = torch.split(o[k], c.Bs)
        logp0 = Fn.log_softmax(split[0], dim=-1)
        nll = -logp0.gather(-1, tgt[:, None]).squeeze(1)
        ce = ((1 - c.smooth) * nll + c.smooth * (-logp0.mean(-1))).mean()       # timm LabelSmoothingCrossEntropy / CrossEntropyLoss
        probs = [Fn.softmax(x, dim=1) for x in split]
        logm = torch.clamp(torch.stack(probs).mean(0), 1e-7, 1).log()
        loss = loss + ce + c.alpha * sum(Fn.kl_div(logm, ps, reduction='batchmean') for ps in probs) / len(probs)
        loss = loss + c.lam * Fn.kl_div(Fn.log_softmax(o[k], dim=-1), mean_log, reduction='mean', log_target=True)
        if a is not None:
            loss = loss + Fn.kl_div(Fn.log_softmax(a[k], dim=1), Fn.log_softmax(o[k], dim=1).detach(), reduction='sum', log_target=True) / o[k].numel()
    loss.backward()
    return dict(loss=loss.detach(), dorg=c.gs * torch.stack([x.grad for x in o]),
                davg=None if a is None else c.gs * torch.stack([y.grad for y in a]))


def jsd_ratios(got, ref, dt, gs=1.0, eps=None):
    """got: dict of float64 tensors (loss = the increment); ref: JsdRef.out -> name -> worst err / allowed"""
    return {n: gate(got[n], r, a0, 0.0 if n == 'loss' else R.r_of(dt), ce, eps, floor=TINY * max(1.0, gs))
            for n, (r, a0, ce) in ref.items() if got.get(n) is not None}


def jsd_need_eps(got, ref, dt, gs=1.0):
    return max(need_eps(got[n], r, a0, ce, 0.0 if n == 'loss' else R.r_of(dt), TINY * max(1.0, gs)) for n, (r, a0, ce) in ref.items()
               if got.get(n) is not None)
