"""tests/_norm_ref.py against itself and against torch (CPU, float64 / fp32): the float64 closed forms agree with torch's own float64
layer_norm / batch_norm / autograd; fp32 arithmetic in each kernel form's order and roundings meets the gate on every small case in both
dtypes; every wrong restatement fails it on the case meant for it; the Python mirror of the form selection covers every instantiation
LN_DISPATCH can reach.  The kernels themselves are held to the same gate by tests/test_norm_edges_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import _norm_ref as R
from _norm_ref import BF, F32, F64, U

DTS = [BF, F32]
ids_dt = lambda dt: 'bf16' if dt == BF else 'fp32'


def _close(a, b, tol=1e-11):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# the closed forms against a second source
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'offset', 'flat'])
@pytest.mark.parametrize('eps', [R.EPS6, R.EPS5])
def test_layernorm_closed_forms_agree_with_torch(kind, eps):
    i = R.ln_inputs(7, 24, BF, kind)
    f = R.ln_fwd(i['x'], i['w'], i['b'], eps)
    _close(f['y'][0], F.layer_norm(i['x'], (24,), i['w'], i['b'], eps), 1e-9)
    _close(R.ln_fwd(i['x'], None, None, eps)['y'][0], F.layer_norm(i['x'], (24,), None, None, eps), 1e-9)
    x = i['x'].clone().requires_grad_()
    w = i['w'].clone().requires_grad_()
    b = i['b'].clone().requires_grad_()
    F.layer_norm(x, (24,), w, b, eps).backward(i['g'])
    dx, _, dw, _, db, _ = R.ln_bwd(i['g'], i['x'], f['mean'][0], f['rstd'][0], i['w'], i['dres'])
    _close(dx - i['dres'], x.grad, 1e-7)
    _close(dw, w.grad, 1e-9)
    _close(db, b.grad, 1e-9)
    # x_is_normalized: the same gradient from xhat
    dxn = R.ln_bwd(i['g'], f['xhat'][0], None, f['rstd'][0], i['w'], i['dres'], xnorm=True)[0]
    _close(dxn, dx, 1e-9)


def test_layernorm_gelu_closed_forms_agree_with_torch():
    i = R.ln_inputs(9, 32, BF)
    f = R.lng_fwd(i['x'], i['w'], i['b'])
    x = i['x'].clone().requires_grad_()
    w = i['w'].clone().requires_grad_()
    b = i['b'].clone().requires_grad_()
    y = F.gelu(F.layer_norm(x, (32,), w, b, R.EPS6))
    _close(f['y'][0], y.detach(), 1e-12)
    y.backward(i['g'])
    dx, _, dw, _, db, _ = R.lng_bwd(i['g'], i['x'], f['mean'][0], f['rstd'][0], i['w'], i['b'])
    _close(dx, x.grad, 1e-9)
    _close(dw, w.grad, 1e-9)
    _close(db, b.grad, 1e-9)


@pytest.mark.parametrize('kind', ['plain', 'offset'])
def test_batchnorm_closed_forms_agree_with_torch(kind):
    rows, C = 40, 12
    i = R.bn_inputs(rows, C, BF, kind)
    s, ssq = i['x'].sum(0), (i['x'] ** 2).sum(0)            # float64 statistics here: the identity, not the fp32 hand-over
    fin = R.bn_finalize(s, ssq, rows, i['w'], i['b'], R.EPS5, 0.125, i['rmean'], i['rvar'])
    rm, rv = i['rmean'].clone(), i['rvar'].clone()
    x = i['x'].clone().requires_grad_()
    w = i['w'].clone().requires_grad_()
    y = F.batch_norm(x, rm, rv, w, i['b'], True, 0.125, R.EPS5)
    _close(fin['rmean'][0], rm, 1e-9)
    _close(fin['rvar'][0], rv, 1e-7)
    ya, _ = R.affine_act(i['x'], fin['scale'][0], fin['shift'][0], i['res'], relu=True)
    _close(ya, F.relu(y.detach() + i['res']), 1e-7)
    F.relu(y).backward(i['dy'])
    mean, rstd = fin['mean'][0], fin['rstd'][0]
    yr = y.detach()
    s1, _, s2, _ = R.bn_bwd_reduce(i['dy'], i['x'], mean, rstd, yr)
    _close(s2, w.grad, 1e-6)
    dx, _ = R.bn_bwd_apply(i['dy'], i['x'], mean, rstd, i['w'], s1, s2, rows, yr)
    _close(dx, x.grad, 1e-6)
    ev = R.bn_finalize(None, None, rows, i['w'], i['b'], R.EPS5, 0.125, i['rmean'], i['rvar'], training=False)
    ye, _ = R.affine_act(i['x'], ev['scale'][0], ev['shift'][0])
    _close(ye, F.batch_norm(i['x'], i['rmean'], i['rvar'], i['w'], i['b'], False, 0.125, R.EPS5), 1e-9)


# ------------------------------------------------------------------------------------------------------------------------------
# the mirror of the form selection
# ------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_dispatchable_instantiation():
    want = R.all_forms()
    assert want == {(4, 3), (4, 4), (8, 3), (8, 4), (16, 1), (16, 3), (16, 4), (32, 3), (32, 4), (64, 3), (64, 4), (64, 8)}
    for dt in DTS:
        have = {c.form.key() for c in R.LN_CASES if c.dt == dt}
        assert have == want, (ids_dt(dt), want - have)
    byname = {repr(c): c.form for c in R.LN_CASES}
    assert byname['bf16-C96'].key() == (16, 1) and byname['bf16-C96-g12_4'].key() == (4, 3) and byname['fp32-C48'].key() == (16, 1)
    assert byname['bf16-C104'].ragged and byname['bf16-C104'].key() == (4, 4) and byname['bf16-C2056'].ragged
    assert byname['bf16-C2056'].key() == byname['bf16-C4096'].key() == byname['fp32-C1536'].key() == (64, 8)
    assert byname['bf16-C1024'].lds_bwd() == byname['fp32-C2048'].lds_bwd() == 65536 and byname['bf16-C4096'].lds_bwd() == 131072
    assert R.Form(96, BF, 5).G == 16 and R.pick_group(4104, 8) == 0          # the knob is clamped; past the range
    assert R.Form(16, BF).grid_fwd(4096 * 64 + 65) == 4096 and R.Form(16, BF).trips(4096 * 64 + 65, 4096) == 2
    assert R.Form(1024, BF).grid_bwd(1027, True, 64) == 64 and R.Form(96, BF).grid_bwd(16401, True) == 1024


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 arithmetic in kernel order meets the gate
# ------------------------------------------------------------------------------------------------------------------------------
def _ln_ratios(case, rows, kind, eps, aff, wrong=None, dres=True, xnorm=False, rps=None, bwrong=None):
    fm, dt = case.form, case.dt
    i = R.ln_inputs(rows, case.C, dt, kind)
    w, b = (i['w'], i['b']) if aff != 'none' else (None, None)
    uLf = U * fm.L_fwd()
    ref = R.ln_fwd(i['x'], w, b, eps, uLf)
    mu, rs, y = R.ln_fwd_as(i['x'], w, b, eps, fm, dt, wrong)
    out = dict(mean=R.gate(mu, *ref['mean'], 0.0, uLf), rstd=R.gate(rs, *ref['rstd'], 0.0, uLf), y=R.gate(y, *ref['y'], R.r_of(dt), uLf))
    # backward on the STORED statistics
    wb = i['w'] if aff in ('w', 'all') else None
    grads = aff in ('all', 'dwdb')
    xin = R.ln_fwd_as(i['x'], None, None, eps, fm, dt)[2] if xnorm else i['x']
    dres = i['dres'] if dres else None
    dw0, db0 = (R.initial(case.C, 0), R.initial(case.C, 1)) if grads else (None, None)
    sc2 = R.scales(-(-rows // rps)) if rps else None
    dx, dx2, dw, db = R.ln_bwd_as(i['g'], xin, mu, rs, wb, dres, xnorm, fm, dt, dw0, db0, None, sc2, rps or 1, bwrong)
    rdx, Adx, rdw, Adw, rdb, Adb = R.ln_bwd(i['g'], xin, mu, rs, wb, dres, xnorm)
    out['dx'] = R.gate(dx, rdx, Adx, R.r_of(dt), U * fm.L_bwd())
    if grads:
        Ldw = U * fm.L_dw(rows, fm.grid_bwd(rows, True))
        out['dw'] = R.gate(dw - dw0, rdw, Adw + dw0.abs(), 0.0, Ldw)
        out['db'] = R.gate(db - db0, rdb, Adb + db0.abs(), 0.0, Ldw)
    if rps:
        out['dx2'] = 0.0 if torch.equal(dx2, R.second_output(dx, sc2, rps, dt).to(F64)) else float('inf')
    return out


@pytest.mark.parametrize('case', R.LN_SMALL, ids=repr)
def test_layernorm_fp32_restatement_meets_the_gate(case):
    n = 0
    for rows in case.rows():
        for kind in ('plain', 'offset', 'flat'):
            aff = R.AFF_VARIANTS[n % 4]
            r = _ln_ratios(case, rows, kind, (R.EPS6, R.EPS5)[n % 2], aff, dres=n % 3 != 0, xnorm=n % 5 == 0, rps=(None, 1, 3)[n % 3])
            n += 1
            assert all(v < 1.0 for v in r.values()), (case, rows, kind, aff, r)


def _case(name):
    return next(c for c in R.LN_CASES if repr(c) == name)


WRONG_FWD = [('padded_mean', 'bf16-C104', 'plain'), ('no_guard', 'bf16-C104', 'plain'), ('no_guard', 'fp32-C52', 'offset'),
             ('c_minus_1', 'bf16-C16', 'plain'), ('c_minus_1', 'fp32-C48', 'plain'), ('eps_outside', 'fp32-C48', 'flat'),
             ('eps_outside', 'bf16-C96', 'flat'), ('eps_1e5', 'fp32-C48', 'flat'), ('eps_1e5', 'bf16-C8', 'flat'),
             ('one_pass', 'fp32-C48', 'offset'), ('one_pass', 'bf16-C96', 'offset')]


@pytest.mark.parametrize('wrong,name,kind', WRONG_FWD)
def test_wrong_layernorm_forward_fails(wrong, name, kind):
    case = _case(name)
    r = _ln_ratios(case, case.form.rpb + 1, kind, R.EPS6, 'all', wrong)
    assert max(r['mean'], r['rstd'], r['y']) > 1.0, r
    ok = _ln_ratios(case, case.form.rpb + 1, kind, R.EPS6, 'all')
    assert all(v < 1.0 for v in ok.values()), ok


WRONG_BWD = [('no_s2', 'dx'), ('s1_from_g', 'dx'), ('dres_before_rstd', 'dx'), ('dw_from_x', 'dw'), ('drop_last_row', 'db'),
             ('scale2_mod', 'dx2'), ('scale2_neighbour', 'dx2'), ('dx2_unrounded', 'dx2')]


@pytest.mark.parametrize('name', ['bf16-C96', 'fp32-C48', 'bf16-C104'])
@pytest.mark.parametrize('wrong,tensor', WRONG_BWD)
def test_wrong_layernorm_backward_fails(wrong, tensor, name):
    case = _case(name)
    if wrong == 'dx2_unrounded' and case.dt == F32:
        return                                  # fp32 stores what it computed: there is no second rounding to get wrong
    r = _ln_ratios(case, 3 * 3 + 1, 'plain', R.EPS6, 'all', rps=3, bwrong=wrong)
    assert r[tensor] > 1.0, r
    assert all(v < 1.0 for k, v in r.items() if k != tensor and not (wrong == 'drop_last_row' and k == 'dw')), r


@pytest.mark.parametrize('dt', DTS, ids=ids_dt)
@pytest.mark.parametrize('C', R.LNG_C)
def test_layernorm_gelu_fp32_restatement_meets_the_gate(C, dt):
    G, rpb = R.lng_form(C)
    rows = min(rpb + 1, 33)
    i = R.ln_inputs(rows, C, dt)
    Lf = 8 + (G.bit_length() - 1) + 4
    ref = R.lng_fwd(i['x'], i['w'], i['b'], R.EPS6, U * Lf)
    mu, rs, y = R.lng_fwd_as(i['x'], i['w'], i['b'], R.EPS6, dt)
    grid = -(-rows // rpb)
    dw0, db0 = R.initial(C, 0), R.initial(C, 1)
    dx, _, dw, db = R.lng_bwd_as(i['g'], i['x'], mu, rs, i['w'], i['b'], dt, dw0, db0, grid)
    rdx, Adx, rdw, Adw, rdb, Adb = R.lng_bwd(i['g'], i['x'], mu, rs, i['w'], i['b'])
    Lb, Ld = 8 + (G.bit_length() - 1) + 10 + 12, 1 + rpb + grid + 3 + 12
    r = dict(mean=R.gate(mu, *ref['mean'], 0.0, U * Lf), rstd=R.gate(rs, *ref['rstd'], 0.0, U * Lf),
             y=R.gate(y, *ref['y'], R.r_of(dt), U * (Lf + 12)), dx=R.gate(dx, rdx, Adx, R.r_of(dt), U * Lb),
             dw=R.gate(dw - dw0, rdw, Adw + dw0.abs(), 0.0, U * Ld), db=R.gate(db - db0, rdb, Adb + db0.abs(), 0.0, U * Ld))
    assert all(v < 1.0 for v in r.values()), r


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ------------------------------------------------------------------------------------------------------------------------------
def _fin(kind, n=48, C=129, wrong=None, running=True, affine=True, training=True):
    i = R.bn_inputs(n, C, F32, kind)          # the statistics are fp32 whatever x is stored as; flat fp32 columns round below zero
    a = (i['sum'], i['sumsq'], n, i['w'] if affine else None, i['b'] if affine else None, R.EPS5, 0.125,
         i['rmean'] if running or not training else None, i['rvar'] if running or not training else None, training)
    ref = R.bn_finalize(*a)
    got, raw = R.bn_finalize_as(*a, wrong=wrong)
    return {k: R.gate(got[k], *ref[k], 0.0, U * 6) for k in ref}, raw


@pytest.mark.parametrize('kind', ['plain', 'offset', 'flat'])
def test_bn_finalize_fp32_restatement_meets_the_gate(kind):
    for n in (1, 48):
        for running, affine, training in ((True, True, True), (False, False, True), (True, True, False)):
            r, raw = _fin(kind, n, running=running, affine=affine, training=training)
            assert all(v < 1.0 for v in r.values()), (kind, n, r)
    if kind == 'flat':
        assert bool((_fin('flat')[1] < 0).any()), 'no flat column rounds below zero: the clamp is not reached'


@pytest.mark.parametrize('wrong,tensor', [('biased_running', 'rvar'), ('unbiased_rstd', 'rstd')])
def test_wrong_bn_finalize_fails(wrong, tensor):
    r, _ = _fin('plain', wrong=wrong)
    assert r[tensor] > 1.0 and all(v < 1.0 for k, v in r.items() if k in ('mean', 'rmean')), r


def _bn_apply_ratios(dt, rows, C, kind, wrong=None, rps=3, n=None):
    i = R.bn_inputs(rows, C, dt, kind)
    rsc = R.scales(-(-rows // rps))
    out = {}
    ref, A = R.affine_act(i['x'], i['scale'], i['shift'], i['res'], rsc, rps, True)
    out['affine_act'] = R.gate(R.affine_act_as(i['x'], i['scale'], i['shift'], i['res'], rsc, rps, True, dt, wrong), ref, A, R.r_of(dt), U * 3)
    ref, A = R.affine_act(i['x'], None, None, i['res'], rsc, rps, False)
    out['rowscale_res'] = R.gate(R.affine_act_as(i['x'], None, None, i['res'], rsc, rps, False, dt, wrong), ref, A, R.r_of(dt), U * 3)
    fin, _ = R.bn_finalize_as(i['sum'], i['sumsq'], rows, None, None, R.EPS5, 0.125, None, None)
    mean, rstd = fin['mean'], fin['rstd']
    s10, s20 = R.initial(C, 0), R.initial(C, 1)
    gx, _ = R.bn_reduce_grid(rows, C)
    L = U * (-(-rows // (16 * gx)) + 16 + gx + 5)
    s1, s2 = R.bn_bwd_reduce_as(i['dy'], i['x'], mean, rstd, i['y_relu'], rsc, rps, s10, s20, wrong)
    r1, A1, r2, A2 = R.bn_bwd_reduce(i['dy'], i['x'], mean, rstd, i['y_relu'], rsc, rps)
    out['s1'] = R.gate(s1 - s10, r1, A1 + s10.abs(), 0.0, L)
    out['s2'] = R.gate(s2 - s20, r2, A2 + s20.abs(), 0.0, L)
    n = n or rows
    ref, A = R.bn_bwd_apply(i['dy'], i['x'], mean, rstd, i['w'], i['s1'], i['s2'], n, i['y_relu'], rsc, rps)
    out['dx'] = R.gate(R.bn_bwd_apply_as(i['dy'], i['x'], mean, rstd, i['w'], i['s1'], i['s2'], n, i['y_relu'], rsc, rps, dt, wrong), ref, A,
                       R.r_of(dt), U * 9)
    return out


@pytest.mark.parametrize('dt', DTS, ids=ids_dt)
@pytest.mark.parametrize('kind', ['plain', 'offset', 'flat'])
def test_bn_apply_and_reduce_fp32_restatements_meet_the_gate(kind, dt):
    for rows, C, n in ((1, 8, None), (17, 72, None), (50, 200, 100)):
        r = _bn_apply_ratios(dt, rows, C, kind, n=n)
        assert all(v < 1.0 for v in r.values()), (rows, C, r)


@pytest.mark.parametrize('dt', DTS, ids=ids_dt)
@pytest.mark.parametrize('wrong,tensor,n', [('ge_mask', 's1', None), ('ge_mask', 'dx', None), ('rows_for_n', 'dx', 100), ('B_x', 'dx', None),
                                            ('res_scaled', 'affine_act', None), ('res_scaled', 'rowscale_res', None)])
def test_wrong_batchnorm_fails(wrong, tensor, n, dt):
    r = _bn_apply_ratios(dt, 50, 72, 'plain', wrong, n=n)
    assert r[tensor] > 1.0, r
    ok = _bn_apply_ratios(dt, 50, 72, 'plain', n=n)
    assert all(v < 1.0 for v in ok.values()), ok
