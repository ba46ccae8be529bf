"""tests/_loss_optim_ref.py checked without a GPU: the hand-written float64 closed forms equal autograd through the project's
oracles; the float64 optimizer steps equal torch's own optimizers where torch has them; an fp32 evaluation of every formula in the
kernel's order meets the gate on every case (the worst ratio is printed: it has to leave room); and every named wrong restatement
is rejected on at least one case -- if one slips through, the cases are too tame or the gate too loose.  The samplers' integer
restatement is checked for its statistics and against the published first output of splitmix64."""
import math

import numpy as np
import pytest
import torch

import _loss_optim_ref as R
from _loss_optim_ref import BF, F32, F64

SMALL = [c for c in R.LOSS_CASES if c.K * c.B * c.NC <= 60000]      # autograd and the wrong restatements: the small cases suffice
_REF = {}


def _ref(c):
    if c.label not in _REF:
        i = R.loss_inputs(c)
        _REF[c.label] = (i, R.loss_ref(i, c))
    return _REF[c.label]


def _got(out, dt):
    return {n: (None if v is None else (v if n == 'loss' else v.to(F32).to(dt).to(F64))) for n, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', SMALL, ids=repr)
def test_loss_closed_form_equals_autograd(c):
    i, ref = _ref(c)
    ag = R.loss_autograd(i, c)
    # the oracle builds the smoothed BCE target of class indices in fp32 (as timm does): each t is off by at most U t there
    t32 = c.kind == 1 and c.tgt == 'idx'
    t, _ = R._targets(i, c, c.NC)
    slack = R.U * float((i['org'] * t).abs().sum()) / (c.B * c.NC) if t32 else 0.0
    assert abs(float(ag['loss']) - float(ref['loss'][0])) <= 1e-12 * (abs(float(ref['loss'][0])) + 1) + slack
    for n in ('dorg', 'davg'):
        if n in ref:
            assert float((ag[n] - ref[n][0]).abs().max()) <= (1e-12 + (R.U / (c.B * c.NC) if t32 else 0.0)) * c.gs, n


def test_cases_cover_the_settings():
    cs = R.LOSS_CASES
    assert {c.NC for c in cs} >= {1, 2, 63, 64, 65, 255, 256, 257, 1000, 16376, 16377, 36000}
    assert {c.K for c in cs} >= {1, 2, 5, 7} and {c.B for c in cs} == {1, 3}
    assert {c.kind for c in cs} == {0, 1} and {c.smooth for c in cs} == {0.0, 0.1} and {c.thr for c in cs} == {-1.0, 0.2}
    assert {c.tgt for c in cs} == {'idx', 'dense1', 'dense_uneven'} and {c.gs for c in cs} == {1.0, 0.25, 65536.0}
    assert {c.regime for c in cs} == {'randn2', 'randn30', 'same', 'const', 'spike'} and {c.avg for c in cs} == {True, False}
    assert any(not c.grad for c in cs) and {c.entry() for c in cs} == {'ga_loss_fwd_bwd', 'ga_map_loss_fwd_bwd', 'ga_loss_dense_fwd_bwd'}
    assert (16376 + 8) * 4 <= R.LDS_OPT_IN < (16377 + 8) * 4
    d = R.loss_inputs(next(c for c in cs if c.tgt == 'dense_uneven' and c.B == 3))['dense'].sum(1)
    assert torch.allclose(d, torch.tensor([0.6, 1.7, 1.0], dtype=F64), atol=1e-6)


def test_loss_fp32_restatement_meets_the_gate():
    worst = {}
    for c in R.LOSS_CASES:
        i, ref = _ref(c)
        out = R.loss_restate(i, c)
        for dt in (F32, BF):
            for n, v in R.loss_ratios(_got(out, dt), ref, dt, c.gs).items():
                key = (n, 'bf16' if dt == BF else 'fp32')
                if v > worst.get(key, (0, ''))[0]:
                    worst[key] = (v, c.label)
    for k in sorted(worst):
        print(f'loss fp32 restatement {k[0]:5s} {k[1]:5s} worst err / allowed {worst[k][0]:.3f}   {worst[k][1]}')
    assert max(v for v, _ in worst.values()) < 1.0, worst


def test_identical_heads_have_no_kl_term():
    c = next(c for c in R.LOSS_CASES if c.regime == 'same' and c.kind == 0 and c.tgt == 'dense_uneven')
    i, ref = _ref(c)
    t, tsum = R._targets(i, c, c.NC)
    p = torch.softmax(i['org'], -1)
    assert float((ref['dorg'][0] - c.gs * (p * tsum - t) / c.B).abs().max()) < 1e-15      # lam (p - r) / (B NC) vanishes


@pytest.mark.parametrize('wrong', R.LOSS_WRONG)
def test_wrong_loss_restatement_fails(wrong):
    """... by a margin: the eps_fast it would take to let it pass is at least 4 x EPS_FAST, on the case that shows it best"""
    best, need, where = 0.0, 0.0, None
    for c in SMALL:
        i, ref = _ref(c)
        got = _got(R.loss_restate(i, c, wrong=wrong), F32)
        v = max(R.loss_ratios(got, ref, F32, c.gs).values())
        if v > best:
            best, where = v, c.label
        need = max(need, R.loss_need_eps(got, ref, F32, c.gs))
    print(f'{wrong}: err / allowed {best:.3g} on {where}; would pass with eps_fast = {need:.3g} = {need / R.EPS_FAST:.3g} x EPS_FAST')
    assert best > 1.0, f'{wrong} meets the gate on every case'
    assert need >= 4 * R.EPS_FAST, f'{wrong}: EPS_FAST {R.EPS_FAST:.3g} is not below a quarter of its excess {need:.3g}'


# ------------------------------------------------------------------------------------------------------------------------------
# optimizers
# ------------------------------------------------------------------------------------------------------------------------------
def _flat_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g, dtype=F32) * 0.05).to(F64)
    grads = [(torch.randn(n, generator=g, dtype=F32) * 0.01).to(F64) for _ in range(3)]
    poison = torch.randn(n, generator=g, dtype=F32).to(F64) * 3
    return p, grads, poison


def _sgd_run(n, nesterov, wd_mult, wrong=None):
    p, grads, buf = _flat_inputs(n, 11)
    worst = 0.0
    for s, g in enumerate(grads):
        hp = R.hp_row('sgd', 5e-3, 0.05, 0.9, first=s == 0)
        h = [float(x) for x in hp]
        (rp,), (rb,), (al,) = R.sgd_step([p], [g], [buf], [wd_mult != 0], h[0], h[1], h[2], nesterov, s == 0)
        gp, gb = R.sgd_restate(p, g, buf, hp, nesterov, wd_mult, wrong=wrong)
        worst = max(worst, R.gate(gp, rp, al['p']), R.gate(gb, rb, al['buf']))
        p, buf = gp, gb
    return worst


def _adamw_run(n, wd_mult, wrong=None):
    p, grads, _ = _flat_inputs(n, 12)
    m, v, worst = torch.zeros_like(p), torch.zeros_like(p), 0.0
    for s, g in enumerate(grads):
        hp = R.hp_row('adamw', 5e-3, 0.05, *R.BETAS, 1e-8, s + 1)
        h = [float(x) for x in hp]
        (rp,), (rm,), (rv,), (al,) = R.adamw_step([p], [g], [m], [v], [wd_mult != 0], h[0], h[1], h[2], h[3], h[4], bc1=h[5], bc2=h[6])
        gp, gm, gv = R.adamw_restate(p, g, m, v, hp, wd_mult, wrong=wrong)
        worst = max(worst, R.gate(gp, rp, al['p']), R.gate(gm, rm, al['m']), R.gate(gv, rv, al['v']))
        p, m, v = gp, gm, gv
    return worst


def _lamb_run(label, wrong=None):
    c = R.LAMB_CASES[label]
    ps, grads = R.lamb_inputs(label)
    decay = R.decay_flags()
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    norms, worst = torch.zeros(len(ps), 2, dtype=F32), {}
    for s in range(R.LAMB_STEPS):
        hp = R.hp_row('lamb', R.LAMB_LR, c['wd'], *R.BETAS, c['eps'], s + 1, grad_averaging=c['avg'])
        h = [float(x) for x in hp]
        ref = R.lamb_step(ps, grads[s], ms, vs, decay, h[0], h[1], h[2], h[3], h[4], max_grad_norm=h[8], bc1=h[5], bc2=h[6], b3=h[7])
        got = R.lamb_restate(ps, grads[s], ms, vs, decay, hp, norms, wrong=wrong)
        for n, v in R.lamb_ratios(got, ref).items():
            worst[n] = max(worst.get(n, 0.0), v)
        ps, ms, vs = got['p'], got['m'], got['v']
    return worst


def test_optimizer_fp32_restatements_meet_the_gate():
    w = max(_sgd_run(n, nes, mult) for n in (1, 257, 4099) for nes in (True, False) for mult in (0.0, 1.0))
    print(f'sgd fp32 restatement worst err / allowed {w:.3f}')
    assert w < 1.0
    w = max(_adamw_run(n, mult) for n in (1, 257, 4099) for mult in (0.0, 1.0))
    print(f'adamw fp32 restatement worst err / allowed {w:.3f}')
    assert w < 1.0
    for label in R.LAMB_CASES:
        w = _lamb_run(label)
        print(f'lamb {label} fp32 restatement worst err / allowed ' + '  '.join(f'{n} {v:.3f}' for n, v in w.items()))
        assert max(w.values()) < 1.0, (label, w)


def test_lamb_cases_cover_the_regimes():
    for label, c in R.LAMB_CASES.items():
        _, grads = R.lamb_inputs(label)
        gn = math.sqrt(sum(float((g * g).sum()) for g in grads[0]))
        assert (gn > 2.0) == (label == 'clipped') and (gn == 0.0) == c['zero_g'], (label, gn)
    chunks = [math.ceil(n / R.LAMB_CHUNK) for n in R.LAMB_SIZES]
    assert set(chunks) == {1, 2, 3} and R.LAMB_SIZES[4] == R.LAMB_CHUNK and sum(R.LAMB_SIZES[:R.LAMB_NDECAY]) % 4 != 0


@pytest.mark.parametrize('wrong', R.SGD_WRONG)
def test_wrong_sgd_restatement_fails(wrong):
    assert max(_sgd_run(257, True, 1.0, wrong), _sgd_run(257, True, 0.0, wrong)) > 1.0


@pytest.mark.parametrize('wrong', R.ADAMW_WRONG)
def test_wrong_adamw_restatement_fails(wrong):
    assert max(_adamw_run(257, 1.0, wrong), _adamw_run(257, 0.0, wrong)) > 1.0


@pytest.mark.parametrize('wrong', R.LAMB_WRONG)
def test_wrong_lamb_restatement_fails(wrong):
    worst = {label: max(_lamb_run(label, wrong).values()) for label in R.LAMB_CASES}
    print(f'{wrong}: ' + '  '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) > 1.0, f'{wrong} meets the gate on every case'


# ---- anchors: the float64 steps against torch's own optimizers
def _torch_run(make, p0, grads):
    pt = p0.clone().requires_grad_(True)
    opt = make([pt])
    for g in grads:
        pt.grad = g.clone()
        opt.step()
    return pt.detach()


def _anchor_inputs():
    g = torch.Generator().manual_seed(3)
    return torch.randn(301, generator=g, dtype=F64), [torch.randn(301, generator=g, dtype=F64) for _ in range(5)]


@pytest.mark.parametrize('nesterov', [True, False])
def test_sgd_step_equals_torch(nesterov):
    p0, grads = _anchor_inputs()
    want = _torch_run(lambda ps: torch.optim.SGD(ps, lr=5e-3, momentum=0.9, nesterov=nesterov, weight_decay=0.05), p0, grads)
    p, buf = p0, torch.zeros_like(p0)
    for s, g in enumerate(grads):
        (p,), (buf,), _ = R.sgd_step([p], [g], [buf], [True], 5e-3, 0.05, 0.9, nesterov, s == 0)
    assert float((p - want).abs().max()) < 1e-14


def test_adamw_step_equals_torch():
    p0, grads = _anchor_inputs()
    want = _torch_run(lambda ps: torch.optim.AdamW(ps, lr=5e-3, betas=R.BETAS, eps=1e-8, weight_decay=0.05), p0, grads)
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for s, g in enumerate(grads):
        (p,), (m,), (v,), _ = R.adamw_step([p], [g], [m], [v], [True], 5e-3, 0.05, *R.BETAS, 1e-8, s + 1)
    assert float((p - want).abs().max()) < 1e-14


def test_lamb_without_decay_and_clip_is_adam():
    """wd = 0 (no trust ratio), max_grad_norm = inf, grad averaging: LAMB is torch.optim.Adam(lr, betas, eps, weight_decay=0), whose
    denominator is sqrt(v) / sqrt(1 - beta2^t) + eps -- eps outside the bias-corrected square root -- and whose step is lr / (1 - beta1^t)"""
    p0, grads = _anchor_inputs()
    want = _torch_run(lambda ps: torch.optim.Adam(ps, lr=5e-3, betas=R.BETAS, eps=1e-6), p0, grads)
    ps, ms, vs = [p0[:100], p0[100:]], [torch.zeros(100, dtype=F64), torch.zeros(201, dtype=F64)], [torch.zeros(100, dtype=F64), torch.zeros(201, dtype=F64)]
    for s, g in enumerate(grads):
        o = R.lamb_step(ps, [g[:100], g[100:]], ms, vs, [True, False], 5e-3, 0.0, *R.BETAS, 1e-6, s + 1, max_grad_norm=float('inf'))
        ps, ms, vs = o['p'], o['m'], o['v']
        assert o['trust'] == [1.0, 1.0]
    assert float((torch.cat(ps) - want).abs().max()) < 1e-14


def test_lamb_direction_is_adamw_direction_plus_decay():
    p0, grads = _anchor_inputs()
    g = grads[0] * 1e-3                        # below max_grad_norm
    o = R.lamb_step([p0], [g], [torch.zeros_like(p0)], [torch.zeros_like(p0)], [True], 5e-3, 0.05, *R.BETAS, 1e-6, 1)
    (pa,), _, _, _ = R.adamw_step([p0], [g], [torch.zeros_like(p0)], [torch.zeros_like(p0)], [True], 1.0, 0.0, *R.BETAS, 1e-6, 1)
    assert float((o['u'][0] - ((p0 - pa) + 0.05 * p0)).abs().max()) < 1e-12
    trust = float(p0.norm() / o['u'][0].norm())
    assert abs(o['trust'][0] - trust) < 1e-12 and float((o['p'][0] - (p0 - 5e-3 * trust * o['u'][0])).abs().max()) < 1e-15


# ------------------------------------------------------------------------------------------------------------------------------
# clipping
# ------------------------------------------------------------------------------------------------------------------------------
def _clip_cases():
    g = torch.Generator().manual_seed(8)
    for n, scale in ((7, 1e-4), (7, 1.0), (1000, 1.0)):
        x = (torch.randn(n, generator=g, dtype=F32) * scale).to(F64)
        nrm = float(x.norm())
        for limit in (0.5 * nrm, 10 * nrm, float(torch.tensor(nrm, dtype=F32))):
            yield x, limit


def _agc_cases():
    for nunits in (1, 4, 5, 9):
        yield R.agc_inputs([1, 63, 64, 65, 4097], nunits)


def _clip_worst(wrong=None):
    w = 0.0
    for x, limit in _clip_cases():
        ref, a0, _ = R.clip_norm_ref(x, limit)
        w = max(w, R.gate(R.clip_norm_restate(x, limit, wrong=wrong), ref, a0))
    return w


def _agc_worst(wrong=None):
    w = 0.0
    for p, g, units in _agc_cases():
        ref, a0, _ = R.agc_ref(p, g, units, 0.02)
        w = max(w, R.gate(R.agc_restate(p, g, units, 0.02, wrong=wrong), ref, a0))
    return w


def test_clip_restatements_meet_the_gate():
    a, b = _clip_worst(), _agc_worst()
    print(f'clip norm fp32 restatement worst err / allowed {a:.3f}, agc {b:.3f}')
    assert a < 1.0 and b < 1.0
    assert _clip_worst('no_1e-6') > 1.0 and _agc_worst('agc_eps_on_gnorm') > 1.0


def test_agc_ref_equals_the_oracle():
    from oracle import mixup_oracle as MO
    p, g, units = R.agc_inputs([1, 63, 64, 65, 4097], 9)
    ref, _, flags = R.agc_ref(p, g, units, 0.02)
    assert set(flags) == {0, 1, 2}
    for (off, ln), f in zip(units, flags):
        want = MO.adaptive_clip_grad([p[off:off + ln].clone()], [g[off:off + ln].clone()], clip_factor=0.02)[0]
        assert float((ref[off:off + ln] - want).abs().max()) <= 1e-12 * float(want.abs().max()), (off, ln, f)


# ------------------------------------------------------------------------------------------------------------------------------
# top-k and the samplers
# ------------------------------------------------------------------------------------------------------------------------------
def test_topk_ref_orders_nan_inf_and_ties():
    x = torch.tensor([[[1.0, float('inf'), 5.0, float('nan'), 5.0, float('-inf'), -0.0, 0.0]]])
    s, idx = R.topk_ref(x, 8)
    assert idx.tolist() == [[3, 1, 2, 4, 0, 6, 7, 5]]
    clean = torch.randn(1, 4, 50, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.topk_ref(clean, 5)[1], clean[0].topk(5, 1, True, True)[1])


def test_topk_restatement_and_the_order_it_replaced():
    """the kernel's selection loop equals the reference; the order it had before (NaN stored as +inf) does not, on a row with a +inf
    in front of a NaN -- and only there"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 6, 70, generator=g)
    x[:, 0, 5] = x[:, 0, 69] = 4.0
    x[0, 1, 7] = float('nan')
    x[1, 1, 9] = float('inf')
    x[0, 2, 3] = float('inf')
    x[1, 2, 40] = float('nan')
    x[:, 3, :] = float('-inf')
    x[0, 4, 8] = float('-inf')
    for topk in (1, 5, 70):
        want = R.topk_ref(x, topk)[1]
        assert torch.equal(R.topk_restate(x, topk), want)
        old = R.topk_restate(x, topk, wrong='nan_as_inf')
        rows = (old != want).any(1).nonzero().flatten().tolist()
        assert rows == [2], rows
    assert R.topk_restate(x, 2, wrong='nan_as_inf')[2].tolist() == [3, 40] and R.topk_ref(x, 2)[1][2].tolist() == [40, 3]


def test_sampler_restatement():
    assert int(R.splitmix64(0)) == 0xE220A8397B1DCDAF            # the published first output of splitmix64 seeded with 0
    n = 1 << 16
    for keep in (0.9, 0.5):
        a, b = R.dropout_mask_ref(n, keep, 1234, 0), R.dropout_mask_ref(n, keep, 1234, 1)
        assert set(np.unique(a).tolist()) == {0.0, float(np.float32(1) / np.float32(keep))}
        for m in (a, b):
            assert abs(float((m > 0).mean()) - keep) <= 4 * math.sqrt(keep * (1 - keep) / n)
        assert not np.array_equal(a, b)
        assert abs(float(((a > 0) == (b > 0)).mean()) - (keep * keep + (1 - keep) ** 2)) < 0.01       # consecutive counters: independent
    assert np.array_equal(R.dropout_mask_ref(100, 1.0, 5, 3), np.ones(100, dtype=np.float32))
    keep = np.linspace(0.5, 1.0, 7).astype(np.float32)
    d = R.drop_path_ref(keep, 7, 4096, 99, 2)
    for s in range(7):
        k = float(keep[s])
        assert abs(float((d[s] > 0).mean()) - k) <= 4 * math.sqrt(k * (1 - k) / 4096) + 1e-9
    assert np.array_equal(d.reshape(-1)[:4096], R.dropout_mask_ref(4096, 0.5, 99, 2))       # one generator behind both samplers
    assert not np.array_equal(d, R.drop_path_ref(keep, 7, 4096, 99, 3))


def test_flat_stub_layout():
    st = R.FlatStub(R.LAMB_SIZES, R.LAMB_NDECAY, device='cpu')
    f = st.flat_state()
    assert f['total'] == sum(R.LAMB_SIZES) and f['n_decay'] == sum(R.LAMB_SIZES[:6]) and list(f['slices'].values())[6] == (f['n_decay'], 40000)
    assert [t.numel() for t in st.split(f['params'])] == R.LAMB_SIZES and st._engines == {}
    st.check_flat_generation(f['gen'], 'x')
