"""tests/_optim_more_ref.py checked without a GPU, and the host side of the Adam / RMSprop / RMSpropTF / Lion / LARS steps: the
float64 steps equal torch's own optimizers where torch has them (RMSpropTF and LARS where they reduce to one); an fp32 evaluation
in the kernels' order meets the derived bounds (the worst ratio is printed) and every named wrong restatement does not; the factory
builds every name with timm's defaults and refuses the rest; state round trips; the entry points are declared, bound and exported;
StepLRScheduler's values; and train.py --print-config resolves the optimizer and the schedule before a model exists."""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _optim_more_ref as M
from _optim_more_ref import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 257, 300]
NEW_SYMBOLS = ['ga_adam_step', 'ga_rmsprop_step', 'ga_lion_step', 'ga_lars_stage1', 'ga_lars_stage2']


# ---- (a) anchors: the float64 steps against torch.optim in float64, 3 steps, to 1e-12 of max |p|
def _anchor_inputs():
    g = torch.Generator().manual_seed(31)
    return ([torch.randn(n, generator=g, dtype=F64) for n in SIZES],
            [[torch.randn(n, generator=g, dtype=F64) for n in SIZES] for _ in range(3)])


def _torch_run(make, p0, grads, preset=None):
    pt = [p.clone().requires_grad_(True) for p in p0]
    opt = make(pt)
    if preset is not None:
        for p in pt:
            opt.state[p].update(preset(p))
    for gs in grads:
        for p, g in zip(pt, gs):
            p.grad = g.clone()
        opt.step()
    return [p.detach() for p in pt]


def _close(got, want):
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), float((a - b).abs().max())


def test_adam_step_equals_torch():
    p0, grads = _anchor_inputs()
    want = _torch_run(lambda ps: torch.optim.Adam(ps, lr=5e-3, betas=M.BETAS, eps=1e-8, weight_decay=0.05), p0, grads)
    p, m, v = p0, [torch.zeros_like(x) for x in p0], [torch.zeros_like(x) for x in p0]
    for s, gs in enumerate(grads):
        p, m, v, _ = M.adam_step(p, gs, m, v, [True] * 4, 5e-3, 0.05, *M.BETAS, 1e-8, s + 1)
    _close(p, want)


@pytest.mark.parametrize('mu', [0.0, 0.9])
def test_rmsprop_step_equals_torch(mu):
    p0, grads = _anchor_inputs()
    want = _torch_run(lambda ps: torch.optim.RMSprop(ps, lr=5e-3, alpha=0.9, eps=1e-8, weight_decay=0.05, momentum=mu), p0, grads)
    p, sq, buf = p0, [torch.zeros_like(x) for x in p0], ([torch.zeros_like(x) for x in p0] if mu else None)
    for gs in grads:
        p, sq, buf, _ = M.rmsprop_step(p, gs, sq, buf, [True] * 4, 5e-3, 0.05, mu, 0.9, 1e-8, tf=False)
    _close(p, want)


@pytest.mark.parametrize('mu', [0.0, 0.9])
def test_rmsproptf_step_equals_torch_where_they_coincide(mu):
    """square average preset to ones, eps 0 (its place no longer matters) and a constant lr (lr inside or outside the buffer)"""
    p0, grads = _anchor_inputs()

    def preset(p):
        st = dict(step=torch.tensor(0.0), square_avg=torch.ones_like(p))
        if mu:
            st['momentum_buffer'] = torch.zeros_like(p)
        return st
    want = _torch_run(lambda ps: torch.optim.RMSprop(ps, lr=5e-3, alpha=0.9, eps=0.0, weight_decay=0.05, momentum=mu), p0, grads, preset)
    p, sq, buf = p0, [torch.ones_like(x) for x in p0], ([torch.zeros_like(x) for x in p0] if mu else None)
    for gs in grads:
        p, sq, buf, _ = M.rmsprop_step(p, gs, sq, buf, [True] * 4, 5e-3, 0.05, mu, 0.9, 0.0, tf=True)
    _close(p, want)
    assert float((p[2] - p0[2]).abs().max()) > 1e-3


@pytest.mark.parametrize('nesterov', [True, False])
def test_lars_step_with_every_decay_flag_clear_is_sgd(nesterov):
    p0, grads = _anchor_inputs()
    want = _torch_run(lambda ps: torch.optim.SGD(ps, lr=5e-3, momentum=0.9, nesterov=nesterov), p0, grads)
    p, buf = p0, [torch.zeros_like(x) for x in p0]
    for s, gs in enumerate(grads):
        o = M.lars_step(p, gs, buf, [False] * 4, 5e-3, 0.05, 0.9, 0.001, 1e-8, nesterov=nesterov, first=s == 0)
        p, buf = o['p'], o['buf']
        assert o['trust'] == [1.0] * 4
    _close(p, want)


def test_lion_step_by_hand():
    """no torch twin: three elements by hand.  c = 0.9 m + 0.1 g is 0.1, -0.08, 0 -> the update is -lr, +lr, 0"""
    p, g, m = (torch.tensor(x, dtype=F64) for x in ([1.0, 1.0, 1.0], [1.0, 1.0, 0.0], [0.0, -0.2, 0.0]))
    (p1,), (m1,), _, (und,) = M.lion_step([p], [g], [m], [True], 0.1, 0.5, 0.9, 0.99)
    assert torch.allclose(p1, torch.tensor([0.95 - 0.1, 0.95 + 0.1, 0.95], dtype=F64), atol=1e-15)
    assert torch.allclose(m1, torch.tensor([0.01, -0.2 + 0.01 * 1.2, 0.0], dtype=F64), atol=1e-15) and not und.any()
    (p2,), _, _, _ = M.lion_step([p], [g], [m], [False], 0.1, 0.5, 0.9, 0.99)
    assert torch.allclose(p2, torch.tensor([0.9, 1.1, 1.0], dtype=F64), atol=1e-15)


# ---- (b) fp32 restatements against the float64 steps
def _adam_run(n, mult, wrong=None):
    p, grads = M.flat_inputs(n, 41)
    m, v, worst = torch.zeros_like(p), torch.zeros_like(p), 0.0
    for s, g in enumerate(grads):
        hp = M.hp_row('adam', M.LR, M.WD, *M.BETAS, eps=1e-8, t=s + 1)
        h = [float(x) for x in hp]
        (rp,), (rm,), (rv,), (al,) = M.adam_step([p], [g], [m], [v], [mult != 0], h[0], h[1], h[2], h[3], h[4], bc1=h[5], bc2=h[6])
        gp, gm, gv = M.adam_restate(p, g, m, v, hp, mult, wrong=wrong)
        worst = max(worst, M.gate(gp, rp, al['p']), M.gate(gm, rm, al['m']), M.gate(gv, rv, al['v']))
        p, m, v = gp, gm, gv
    return worst


def _rmsprop_run(n, tf, mu, mult, wrong=None):
    p, grads = M.flat_inputs(n, 42)
    sq = torch.full_like(p, 1.0 if (tf and wrong != 'sq_from_zero') else 0.0)
    ref_sq = torch.full_like(p, 1.0 if tf else 0.0)
    buf, worst = (torch.zeros_like(p) if mu else None), 0.0
    for s, g in enumerate(grads):
        hp = M.hp_row('rmsprop', M.LR, M.WD, mu=mu, alpha=M.RMS_ALPHA, eps=M.RMSTF_EPS if tf else M.RMS_EPS)
        h = [float(x) for x in hp]
        (rp,), (rs,), rb, (al,) = M.rmsprop_step([p], [g], [ref_sq], None if buf is None else [buf], [mult != 0], h[0], h[1], h[2], h[3], h[4], tf=tf)
        gp, gs_, gb = M.rmsprop_restate(p, g, sq, buf, hp, tf, mult, wrong=wrong)
        worst = max(worst, M.gate(gp, rp, al['p']), M.gate(gs_, rs, al['sq']))
        if buf is not None:
            worst = max(worst, M.gate(gb, rb[0], al['buf']))
        p, sq, ref_sq, buf = gp, gs_, gs_, gb
    return worst


def _lion_run(n, mult, wrong=None):
    p, grads = M.flat_inputs(n, 43)
    m = grads[2].clone() * 0.5          # a momentum that is not zero: the sign of c is not the sign of g
    worst, undetermined = 0.0, 0
    for g in grads:
        hp = M.hp_row('lion', M.LR, M.WD, *M.LION_BETAS)
        h = [float(x) for x in hp]
        (rp,), (rm,), (al,), (und,) = M.lion_step([p], [g], [m], [mult != 0], h[0], h[1], h[2], h[3])
        gp, gm = M.lion_restate(p, g, m, hp, mult, wrong=wrong)
        worst = max(worst, M.gate(gp, rp, al['p']), M.gate(gm, rm, al['m']))
        undetermined += int(und.sum())
        p, m = gp, gm
    return worst, undetermined


def _lars_run(label, nesterov, trust_clip, mu=0.9, wrong=None):
    c = M.LARS_CASES[label]
    ps, grads = M.lars_inputs(label)
    decay = M.R.decay_flags(M.LARS_SIZES, M.LARS_NDECAY)
    bufs, worst = ([torch.zeros_like(p) for p in ps] if mu else None), {}
    for s in range(M.STEPS):
        hp = M.hp_row('lars', M.LR, c['wd'], mu=mu, trust_coeff=M.LARS_TC, eps=M.LARS_EPS, first=s == 0)
        h = [float(x) for x in hp]
        ref = M.lars_step(ps, grads[s], bufs, decay, h[0], h[1], h[2], h[3], h[4], nesterov, trust_clip, first=s == 0)
        got = M.lars_restate(ps, grads[s], bufs, decay, hp, nesterov, trust_clip, wrong=wrong)
        for n, v in M.lars_ratios(got, ref).items():
            worst[n] = max(worst.get(n, 0.0), v)
        ps, bufs = got['p'], (got['buf'] if mu else None)
    return worst, ref


def test_fp32_restatements_meet_the_bounds():
    w = max(_adam_run(n, mult) for n in (1, 257, 4099) for mult in (0.0, 1.0))
    print(f'adam fp32 restatement worst err / allowed {w:.3f}')
    assert w <= 1.0
    for tf in (False, True):
        w = max(_rmsprop_run(n, tf, mu, mult) for n in (1, 257, 4099) for mu in (0.0, 0.9) for mult in (0.0, 1.0))
        print(f'rmsprop tf={int(tf)} fp32 restatement worst err / allowed {w:.3f}')
        assert w <= 1.0
    runs = [_lion_run(n, mult) for n in (1, 257, 4099) for mult in (0.0, 1.0)]
    print(f'lion fp32 restatement worst err / allowed {max(r[0] for r in runs):.3f}, {sum(r[1] for r in runs)} elements with an undetermined sign')
    assert max(r[0] for r in runs) <= 1.0 and sum(r[1] for r in runs) <= 2          # the 2 lr allowance is not what lets Lion pass
    for label in M.LARS_CASES:
        for nesterov, clip in M.LARS_FORMS:
            for mu in (0.9, 0.0):
                w, _ = _lars_run(label, nesterov, clip, mu)
                print(f'lars {label} nesterov={int(nesterov)} clip={int(clip)} mu={mu} worst err / allowed ' + '  '.join(f'{n} {v:.3f}' for n, v in w.items()))
                assert max(w.values()) <= 1.0, (label, nesterov, clip, mu, w)


def test_lars_cases_cover_the_regimes():
    _, ref = _lars_run('decay', False, False)
    t = ref['trust']
    assert all(x == 1.0 for x in t[M.LARS_NDECAY:]) and t[M.LARS_ZERO_G] == 1.0 and sum(abs(x - 1.0) > 0.5 for x in t[:M.LARS_NDECAY]) >= 4
    _, ref = _lars_run('decay', False, True)
    t = [x for i, x in enumerate(ref['trust'][:M.LARS_NDECAY]) if i not in (M.LARS_ZERO_P, M.LARS_ZERO_G)]
    assert any(x == 1.0 for x in t) and any(x < 0.9 for x in t), t          # trust / lr on both sides of 1
    assert _lars_run('wd0', True, True)[1]['trust'] == [1.0] * len(M.LARS_SIZES)
    p0, _ = M.lars_inputs('decay')
    assert not p0[M.LARS_ZERO_P].any() and {math.ceil(n / M.LAMB_CHUNK) for n in M.LARS_SIZES} == {1, 2, 3}


@pytest.mark.parametrize('wrong', M.ADAM_WRONG)
def test_wrong_adam_restatement_fails(wrong):
    assert max(_adam_run(257, 1.0, wrong), _adam_run(257, 0.0, wrong)) > 1.0


@pytest.mark.parametrize('wrong', M.RMSPROP_WRONG)
@pytest.mark.parametrize('mu', [0.0, 0.9])
def test_wrong_rmsproptf_restatement_fails(wrong, mu):
    assert max(_rmsprop_run(257, True, mu, 1.0, wrong), _rmsprop_run(257, True, mu, 0.0, wrong)) > 1.0


@pytest.mark.parametrize('wrong', M.RMSPROP_TORCH_WRONG)
@pytest.mark.parametrize('mu', [0.0, 0.9])
def test_wrong_rmsprop_restatement_fails(wrong, mu):
    assert max(_rmsprop_run(257, False, mu, 1.0, wrong), _rmsprop_run(257, False, mu, 0.0, wrong)) > 1.0


@pytest.mark.parametrize('wrong', M.LION_WRONG)
def test_wrong_lion_restatement_fails(wrong):
    assert max(_lion_run(257, 1.0, wrong)[0], _lion_run(257, 0.0, wrong)[0]) > 1.0


@pytest.mark.parametrize('wrong', M.LARS_WRONG)
def test_wrong_lars_restatement_fails(wrong):
    worst = {(label, f): max(_lars_run(label, *f, wrong=wrong)[0].values()) for label in M.LARS_CASES for f in M.LARS_FORMS}
    print(f'{wrong}: ' + '  '.join(f'{k[0]}{k[1]} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) > 1.0, f'{wrong} meets the bounds on every case'


# ---- (c) the host side
def _stub():
    return M.FlatStub([5, 300, 1000, 7, 64], 3, device='cpu')


class _RecordedPlan:
    """stands in for ops.Plan where there is no device: keeps the name and the arguments of every launch an optimizer records"""

    def __init__(self, name='', **_):
        self.name, self.calls = name, []

    def __getattr__(self, fn):
        return lambda *a, **k: self.calls.append((fn, a))


@pytest.fixture(autouse=True)
def _no_device_plans(monkeypatch):
    from imagenet_models_amd import optim
    monkeypatch.setattr(optim, 'Plan', _RecordedPlan)


def test_launches_follow_the_decay_segments():
    import imagenet_models_amd as A
    mk = lambda name, **kw: A.create_optimizer_v2(_stub(), opt=name, lr=0.1, weight_decay=0.05, **kw)
    for name, fn, tail in (('adam', 'adam_step', lambda n, mult: (n, mult)), ('lion', 'lion_step', lambda n, mult: (n, mult)),
                           ('rmsprop', 'rmsprop_step', lambda n, mult: (n, False, mult)), ('rmsproptf', 'rmsprop_step', lambda n, mult: (n, True, mult))):
        o = mk(name)
        assert [(f, a[-len(tail(0, 0)):]) for f, a in o.plan.calls] == [(fn, tail(1305, 1.0)), (fn, tail(71, 0.0))], name
        assert all(a[0].data_ptr() == o.p[off:].data_ptr() and a[1].data_ptr() == o.g[off:].data_ptr() for (_, a), off in zip(o.plan.calls, (0, 1305)))
        pl = o.range_plan(1300, 1310)          # a range that straddles the boundary: one launch per segment, then the gradients' zeroing
        assert [(f, a[-1]) for f, a in pl.calls[:2]] == [(fn, 1.0), (fn, 0.0)] and pl.calls[2][0] == 'zero' and pl.calls[2][1][0].numel() == 10
    assert mk('rmsprop', momentum=0.0).plan.calls[0][1][3] is None and mk('rmsprop').plan.calls[0][1][3] is not None
    o = mk('nlarc')
    assert [f for f, _ in o.plan.calls] == ['zero', 'lars_stage1', 'lars_stage2'] and o.plan.calls[2][1][-2:] == (True, True)
    assert o.plan.calls[2][1][5] == 5 and mk('lars', momentum=0.0).plan.calls[2][1][2] is None


def test_factory_builds_every_name_with_timms_defaults():
    import imagenet_models_amd as A
    mk = lambda name, **kw: A.create_optimizer_v2(_stub(), opt=name, lr=0.1, weight_decay=0.05, momentum=0.8, **kw)
    o = mk('adam')
    assert type(o) is A.FusedAdam and o.kind == 'adam' and o.moment_names == ('m', 'v') and (o.betas, o.eps) == ((0.9, 0.999), 1e-8)
    assert mk('Adam', eps=1e-6, betas=(0.8, 0.9)).eps == 1e-6 and mk('adam', betas=(0.8, 0.9)).betas == (0.8, 0.9)
    o = mk('rmsprop')
    assert type(o) is A.FusedRMSprop and o.kind == 'rmsprop' and not o.tf and (o.alpha, o.momentum, o.eps) == (0.9, 0.8, 1e-8)
    assert o.moment_names == ('sq', 'buf') and not o.sq.any()
    o = mk('rmsproptf')
    assert type(o) is A.FusedRMSprop and o.kind == 'rmsproptf' and o.tf and (o.alpha, o.momentum, o.eps) == (0.9, 0.8, 1e-10)
    assert bool((o.sq == 1).all()) and not o.buf.any() and mk('rmsproptf', eps=1e-3).eps == 1e-3
    o = A.create_optimizer_v2(_stub(), opt='rmsproptf', lr=0.1, momentum=0.0)
    assert o.moment_names == ('sq',) and o.buf is None
    o = mk('lion', eps=1e-3)
    assert type(o) is A.FusedLion and o.kind == 'lion' and o.moment_names == ('m',) and o.betas == (0.9, 0.99) and not hasattr(o, 'eps')
    for name, nesterov, clip in (('lars', False, False), ('nlars', True, False), ('larc', False, True), ('nlarc', True, True)):
        o = mk(name)
        assert type(o) is A.FusedLars and o.kind == 'lars' and (o.nesterov, o.trust_clip) == (nesterov, clip)
        assert (o.momentum, o.trust_coeff, o.eps) == (0.8, 0.001, 1e-8) and o.moment_names == ('buf',) and not o.supports_ranges
        assert o.chunks.tolist() == [[0, 5, 0, 1], [5, 300, 1, 1], [305, 1000, 2, 1], [1305, 7, 3, 0], [1312, 64, 4, 0]]
    for name in ('adam', 'rmsprop', 'rmsproptf', 'lion'):
        assert mk(name).supports_ranges
    for o in (mk('adam'), mk('lars')):
        assert o.param_groups == [dict(lr=0.1, weight_decay=0.05, initial_lr=0.1)] and o.steps == 0
    # the names that existed keep their classes
    assert type(mk('sgd')) is A.FusedSGD and type(mk('adamw')) is A.FusedAdamW and type(mk('lamb')) is A.FusedLamb


@pytest.mark.parametrize('name', ['adagrad', 'novograd', 'lookahead_adam', 'rmsprop_tf', 'sgdp', ''])
def test_factory_refuses_the_rest_and_lists_what_it_has(name):
    import imagenet_models_amd as A
    with pytest.raises(ValueError, match='is not implemented on the HIP path yet') as e:
        A.create_optimizer_v2(_stub(), opt=name, lr=0.1)
    for have in ('sgd', 'momentum', 'nesterov', 'adamw', 'lamb', 'adam', 'rmsprop', 'rmsproptf', 'lion', 'lars', 'nlars', 'larc', 'nlarc'):
        assert re.search(rf'[ (]{have}[,)]', str(e.value)), have
    with pytest.raises(ValueError, match='is not implemented'):
        A.optimizer_config(name)


@pytest.mark.parametrize('name', ['adam', 'rmsprop', 'rmsproptf', 'lion', 'nlarc'])
def test_state_dict_round_trip(name):
    import imagenet_models_amd as A
    a = A.create_optimizer_v2(_stub(), opt=name, lr=0.1, weight_decay=0.05)
    g = torch.Generator().manual_seed(5)
    for n in a.moment_names:
        getattr(a, n).copy_(torch.randn(a.total, generator=g))
    a.steps, a.param_groups[0]['lr'] = 7, 3.3e-4
    a._hp_host = [0.0]
    sd = a.state_dict()
    assert list(sd) == ['kind', 'steps', *a.moment_names, 'param_groups'] and sd['kind'] == a.kind and sd['steps'] == 7
    getattr(a, a.moment_names[0]).zero_()          # the dict holds copies
    assert sd[a.moment_names[0]].any()
    b = A.create_optimizer_v2(_stub(), opt=name, lr=0.1, weight_decay=0.05)
    b._hp_host = [0.0]
    b.load_state_dict(sd)
    assert b.steps == 7 and b.param_groups[0] == dict(lr=3.3e-4, weight_decay=0.05, initial_lr=0.1) and b._hp_host is None
    for n in b.moment_names:
        assert torch.equal(getattr(b, n), sd[n])


def test_symbols_are_declared_bound_and_exported():
    from imagenet_models_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    declared = set(re.findall(r'^\s*(?:int|size_t)\s+(ga_\w+)\s*\(', hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
        assert hasattr(ops.Plan, name[3:]), name
    for phrase in ('avg = sqrt(sq + eps) -- eps INSIDE the root', 'sq starts at ONE', 'sign(0) = 0', 'trust = min(trust / lr, 1)',
                   'ONE atomic'):
        assert phrase in hdr, phrase
    # bad arguments are refused on the host, before any launch
    for name, args in (('ga_adam_step', (None, None, None, None, None, 8, 1.0, None)), ('ga_rmsprop_step', (None, None, None, None, None, 8, 0, 1.0, None)),
                       ('ga_lion_step', (None, None, None, None, 8, 1.0, None)), ('ga_lars_stage1', (None, None, None, 1, None, None)),
                       ('ga_lars_stage2', (None, None, None, None, None, 1, None, 0, 0, None))):
        assert getattr(lib, name)(*args) != 0 and name in _lib.last_error(), name


def test_step_lr_scheduler_values():
    import imagenet_models_amd as A
    opt = A.create_optimizer_v2(_stub(), opt='rmsproptf', lr=0.064)
    s = A.StepLRScheduler(opt, decay_t=10, decay_rate=0.5, warmup_t=3, warmup_lr_init=1e-4)
    assert opt.param_groups[0]['lr'] == 1e-4          # the warm-up start, before the first step()
    lr = lambda t: (s.step(t), opt.param_groups[0]['lr'])[1]
    assert lr(0) == 1e-4 and lr(2) == pytest.approx(1e-4 + 2 * (0.064 - 1e-4) / 3, rel=1e-15) and lr(3) == 0.064
    assert lr(9) == 0.064 and lr(10) == 0.032 and lr(20) == 0.016 and lr(19) == 0.032
    s.step_update(5)
    assert opt.param_groups[0]['lr'] == 0.032 and opt.param_groups[0]['initial_lr'] == 0.064
    # a fractional interval, timm's form: decay_rate ** (t // decay_t)
    s = A.StepLRScheduler(opt, decay_t=2.4, decay_rate=0.97)
    assert [lr(t) for t in (0, 2, 3, 5)] == [0.064, 0.064, 0.064 * 0.97, 0.064 * 0.97 ** 2]
    # the surface the resume path uses is the cosine schedule's
    assert {'step', 'step_update'} <= set(dir(A.CosineLRScheduler)) & set(dir(A.StepLRScheduler))
    with pytest.raises(ValueError):
        A.StepLRScheduler(opt, decay_t=0, decay_rate=0.5)


def _print_config(argv):
    r = subprocess.run([sys.executable, 'train.py', '--synthetic', '--print-config'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    return r, [ln for ln in r.stdout.splitlines() if ln.startswith('{')]


def test_print_config_resolves_optimizer_and_schedule():
    r, lines = _print_config(['--model', 'mobilenet_v1', '--opt', 'rmsproptf', '--sched', 'step', '--decay-epochs', '2.4', '--decay-rate', '0.97',
                              '--opt-eps', '0.001', '--momentum', '0.9', '--warmup-epochs', '5', '--warmup-lr', '1e-6'])
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    cfg = json.loads(lines[0])
    assert cfg['opt'] == 'rmsproptf' and cfg['optimizer'] == dict(kind='rmsproptf', alpha=0.9, momentum=0.9, eps=0.001)
    assert cfg['schedule'] == dict(kind='step', decay_epochs=2.4, decay_rate=0.97, warmup_epochs=5, warmup_lr=1e-6)
    r, lines = _print_config(['--model', 'mobilenet_v1', '--opt', 'nlarc', '--dr', '0.5', '--sched', 'step'])
    cfg = json.loads(lines[0])
    assert cfg['optimizer'] == dict(kind='lars', momentum=0.9, nesterov=True, trust_clip=True, trust_coeff=0.001, eps=1e-8)
    assert cfg['schedule']['decay_epochs'] == 100 and cfg['schedule']['decay_rate'] == 0.5          # the reference's defaults; --dr
    r, lines = _print_config(['--model', 'mobilenet_v1'])          # today's defaults
    cfg = json.loads(lines[0])
    assert cfg['optimizer'] == dict(kind='sgd', momentum=0.9, nesterov=True) and cfg['schedule']['kind'] == 'cosine'
    assert json.loads(_print_config(['--model', 'mobilenet_v1', '--sched', 'plateau'])[1][0])['schedule'] == dict(kind='none')
    r, lines = _print_config(['--model', 'mobilenet_v1', '--opt', 'adagrad'])
    assert r.returncode != 0 and not lines and "optimizer 'adagrad' is not implemented on the HIP path yet" in r.stderr
