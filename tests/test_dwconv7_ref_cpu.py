"""The gate of tests/_dwconv7_ref.py against arithmetic: on every case of tests/test_dwconv7_edges_gpu.py (its shapes at 256 CUs),
fp32 evaluation in each kernel form's documented order and roundings (conv_as / wgrad_as: taps rounded to bf16 where the form does,
accumulation in the form's groups, the partition of the weight gradient into units, waves, partials and reduce groups) stays inside
gate(), and fourteen wrong restatements of the same formulas do not.  Needs no GPU; the form names come from the library's own
queries (ga_dwconv7_form / ga_dwconv7_bwd_weight_form), as in the GPU module.

The walk cases keep their full batch for the weight gradient (the reduction runs over it) and evaluate the convolution on the first
two and the last image (its elements do not depend on the batch).

Worst err / allowed of the fp32 evaluation per form (all cases, both kinds; python -m pytest tests/test_dwconv7_ref_cpu.py -s):
                     fwd     bwd     bwd+res  dw      dbias
    rs               0.991   0.993   0.989    0.022   0.007
    dot2_7x7         0.991   0.989   0.993    0.014   0.010
    dot2_14x14       0.992   0.993   0.993    0.002   0.001
    mfma             0.993   0.993   0.993
    scalar_7x7 bf16  0.978   0.986   0.993    0.020   0.013
    scalar_14x14 bf16 0.985  0.991   0.987    0.001   0.001
    scalar_7x7 fp32  0.054   0.061   0.063    0.032   0.027
    scalar_14x14 fp32 0.054  0.054   0.060    0.004   0.001
The bf16 rows are the ONE rounding of the stored value: half an ulp is 2^-8 of a value just above a power of two, all of r |ref|, and
with thousands of elements one lands there.  The fp32 rows and the gradients show what the accumulation itself uses of u A: 6 % and
less.  The restatement that rounds the sum to bf16 BEFORE the residual as well (what the dot2 and MFMA forms did until this suite)
reaches 28 (dot2 7x7), 58 (dot2 14x14) and 33 (MFMA) times the allowance on the cases aimed at it.
"""
import ctypes as C

import pytest
import torch

import _dwconv7_ref as R
from _dwconv7_ref import BF, F32, F64

CUS = 256
WORST = {}


def _L():
    from imagenet_models_amd import _lib
    return _lib


def names(case, geom, res=0, y2=0):
    """the forward / backward-data and the weight-gradient form names the library reports for the case under its knobs"""
    L = _L()
    lib = L.load()
    buf = C.create_string_buffer(64)
    dt = 1 if case.dt == BF else 0
    with L.knobs(**case.knobs):
        L.check(lib.ga_dwconv7_form(*geom, dt, res, y2, buf, 64), 'ga_dwconv7_form')
        f = buf.value.decode()
        L.check(lib.ga_dwconv7_bwd_weight_form(*geom, dt, buf, 64), 'ga_dwconv7_bwd_weight_form')
        return f, buf.value.decode()


def _cus():
    import test_dwconv7_forms_cpu as T
    return T._cus()


def _sub(i, n=2):
    """the first n and the last image of every [B]-leading input"""
    B = i['x'].shape[0]
    if B <= n + 1:
        return i
    pick = list(range(n)) + [B - 1]
    return {k: (v[pick] if k in ('x', 'dy', 'res', 'scale2') else v) for k, v in i.items()}


def _note(fam, dt, tensor, ratio):
    key = (fam + (' bf16' if dt == BF else ' fp32') if fam.startswith('scalar') else fam, tensor)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.mark.parametrize('case', R.CASES, ids=repr)
def test_fp32_in_the_forms_order_meets_the_gate(case):
    cus = _cus()
    geom = case.geom(cus)
    fname, wname = names(case, geom)
    assert R.family_of(fname) == case.fam or 'fwd' not in case.ops, fname
    for which, name in (('fwd', fname), ('wgrad', wname)):
        if which in case.ops and case.want(which, cus):
            assert name == case.want(which, cus), (which, name)
    for kind in case.kinds:
        full = R.make_inputs(geom, case.dt, kind)
        i = _sub(full) if geom[0] * geom[1] * geom[2] * geom[3] > 1 << 20 else full
        fam = R.family_of(fname)
        if 'fwd' in case.ops:
            ref, A = R.fwd(i['x'], i['w49'], i['bias'])
            got = R.conv_as(fname, i['x'], i['w49'], i['bias'], None, case.dt, False)
            _note(fam, case.dt, 'fwd', R.gate_conv(got, ref, A, case.dt, fname, kind))
        if 'bwd' in case.ops:
            for res, tag in ((None, 'bwd'), (i['res'], 'bwd+res')):
                ref, A = R.bwd_data(i['dy'], i['w49'], res)
                got = R.conv_as(fname, i['dy'], i['w49'], None, res, case.dt, True)
                _note(fam, case.dt, tag, R.gate_conv(got, ref, A, case.dt, fname, kind))
        if 'wgrad' in case.ops and kind == 'plain':
            dw, Aw, db, Ab = R.bwd_weight(full['dy'], full['x'])
            iw, ib = R.initial(49 * geom[3], 0).view(49, -1), R.initial(geom[3], 1)
            gw, gb = R.wgrad_as(wname, full['dy'], full['x'], iw, ib)
            wfam = R.family_of(wname)
            _note(wfam, case.dt, 'dw', R.gate_wgrad(gw - iw, dw, Aw, wname, geom))
            _note(wfam, case.dt, 'dbias', R.gate_wgrad(gb - ib, db, Ab, wname, geom))
    bad = {k: v for k, v in WORST.items() if not v < 1.0}
    assert not bad, bad


def test_zz_report():
    """prints the table of the module docstring (run with -s)"""
    for k in sorted(WORST):
        print(f'{k[0]:14s} {k[1]:8s} {WORST[k]:.3f}')


# ------------------------------------------------------------------------------------------------------------------------------
# wrong restatements: each has to fail the gate on the cases aimed at it
# ------------------------------------------------------------------------------------------------------------------------------
def _case(label):
    return next(c for c in R.CASES if c.label == label)


def _conv_ratio(label, op, **wrong):
    """ratio of a wrongly stated forward ('fwd') or backward-data ('bwd': with the residual) on the case; also checks the right one"""
    case = _case(label)
    geom = case.geom(CUS)
    fname, _ = names(case, geom)
    i = _sub(R.make_inputs(geom, case.dt))
    if op == 'fwd':
        ref, A = R.fwd(i['x'], i['w49'], i['bias'])
        args = (fname, i['x'], i['w49'], i['bias'], None, case.dt, False)
    else:
        ref, A = R.bwd_data(i['dy'], i['w49'], i['res'])
        args = (fname, i['dy'], i['w49'], None, i['res'], case.dt, True)
    assert R.gate_conv(R.conv_as(*args), ref, A, case.dt, fname, 'plain') < 1.0
    if 'res_dropped' in wrong:
        args = args[:4] + (None,) + args[5:]
        wrong = {}
    if 'zero_col' in wrong or 'zero_row' in wrong:
        x = args[1].clone()
        if 'zero_col' in wrong:
            x[:, :, wrong['zero_col']] = 0
        else:
            x[:, wrong['zero_row']] = 0
        args = (args[0], x) + args[2:]
        wrong = {}
    return R.gate_conv(R.conv_as(*args, **wrong), ref, A, case.dt, fname, 'plain')


CONV_TARGETS = ['rs W5', 'rs H21 R7', 'dot2_7 8x15 C72', 'dot2_14 14x42 C72', 'mfma 28x14 C40 B2 xcd1', 'scalar bf16 9x10 C12', 'scalar f32 9x10 C36']


@pytest.mark.parametrize('label', CONV_TARGETS)
def test_a_dropped_border_tap_fails(label):
    assert _conv_ratio(label, 'fwd', drop_tap=0) > 1 and _conv_ratio(label, 'bwd', drop_tap=27) > 1


@pytest.mark.parametrize('label', CONV_TARGETS)
@pytest.mark.parametrize('pad', ['clamp', 'wrap_row', 'wrap_img'])
def test_wrong_padding_fails(label, pad):
    assert _conv_ratio(label, 'fwd', pad=pad) > 1 and _conv_ratio(label, 'bwd', pad=pad) > 1


@pytest.mark.parametrize('label', CONV_TARGETS)
def test_unflipped_taps_bias_twice_and_a_dropped_residual_fail(label):
    assert _conv_ratio(label, 'bwd', flipped=False) > 1
    assert _conv_ratio(label, 'fwd', flipped=True) > 1
    assert _conv_ratio(label, 'fwd', bias_times=2) > 1
    assert _conv_ratio(label, 'bwd', res_dropped=True) > 1


@pytest.mark.parametrize('label', ['dot2_7 8x15 C72', 'dot2_14 14x42 C72', 'mfma 28x14 C40 B2 xcd1'])
def test_rounding_before_the_residual_fails(label):
    """what the dot2 and MFMA forms did before this suite: the sum rounded to bf16, the residual added, rounded again"""
    assert _conv_ratio(label, 'bwd', twice=True) > 1


def test_scale2_of_the_neighbouring_image_fails():
    case = _case('rs B3 R7')
    i = R.make_inputs(case.geom(CUS), BF)
    dx = R.conv_as('rs', i['dy'], i['w49'], None, i['res'], BF, True).to(BF)
    good = R.second_output(dx, i['scale2'], BF)
    assert len(set(i['scale2'].tolist())) == 3 and 0.0 in i['scale2'].tolist()
    for shift in (1, -1):
        assert not torch.equal(R.second_output(dx, i['scale2'].roll(shift), BF), good)


@pytest.mark.parametrize('label', ['rs W5', 'rs W9', 'rs W13', 'rs W1'])
def test_a_dropped_last_strip_column_fails(label):
    W = _case(label).geom(CUS)[2]
    assert W % 4 and _conv_ratio(label, 'fwd', zero_col=W - 1) > 1 and _conv_ratio(label, 'bwd', zero_col=W - 1) > 1


@pytest.mark.parametrize('label,R_', [('rs H21 R7', 7), ('rs B3 R7', 7)])
def test_a_dropped_halo_row_at_a_segment_boundary_fails(label, R_):
    for row in (R_ - 1, R_):       # the last row of segment 0 (the halo of segment 1) and the first of segment 1 (the halo of segment 0)
        assert _conv_ratio(label, 'fwd', zero_row=row) > 1 and _conv_ratio(label, 'bwd', zero_row=row) > 1


def _wgrad_ratio(label, **wrong):
    case = _case(label)
    geom = case.geom(CUS)
    _, wname = names(case, geom)
    i = R.make_inputs(geom, case.dt)
    dw, Aw, db, Ab = R.bwd_weight(i['dy'], i['x'])
    iw, ib = R.initial(49 * geom[3], 0).view(49, -1), R.initial(geom[3], 1)
    out = []
    for kw in ({}, wrong):
        gw, gb = R.wgrad_as(wname, i['dy'], i['x'], iw, ib, **kw)
        out.append((R.gate_wgrad(gw - iw, dw, Aw, wname, geom), R.gate_wgrad(gb - ib, db, Ab, wname, geom)))
    assert max(out[0]) < 1.0
    return out[1]


@pytest.mark.parametrize('label', ['rs H21 R7', 'rs B3 R7'])
@pytest.mark.parametrize('seam', [-1, 1])
def test_segment_seam_rows_dropped_or_doubled_fail(label, seam):
    w, b = _wgrad_ratio(label, seam=seam)
    assert w > 1 and b > 1


def test_a_second_unit_that_overwrites_the_first_fails():
    w, b = _wgrad_ratio('rs two-unit wave', second='overwrite')
    assert w > 1 and b > 1


@pytest.mark.parametrize('label', ['rs H14 R14', 'dot2_7 parts17', 'dot2_14 14x14 C8', 'scalar f32 28x14 C68', 'scalar bf16 9x10 C12'])
def test_stored_instead_of_accumulated_and_a_partial_left_out_fail(label):
    w, b = _wgrad_ratio(label, store=True)
    assert w > 1 and b > 1
    w, b = _wgrad_ratio(label, skip_part=0)
    assert w > 1 and b > 1
