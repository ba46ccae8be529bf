"""Multi-token class attention (csrc/map.hip: ga_class_attn_mt_fwd / _bwd and the `interactive` pair
ga_class_attn_mt_ia_fwd / _bwd) at the edges of its launch geometry, against the float64 closed forms of
tests/_class_attn_ref.py: T over the three instantiations MT = 4 / 6 / 8, N around the wave counts (16 forward, 8
backward; 4 interactive) and around 64 lanes, heads above the wave count, E = 8 (one live lane) and E = 512 (all 64),
hd / 8 in {1, 3, 8}, padded and unequal row strides, the column-slice operand of engine_map.py, the three input kinds,
the largest N the 160 KiB LDS bound admits and the refusal of N + 1, run-to-run bit identity, the accumulation of
dW1 / db1 / dW2 / db2, and the argument checks.

Gate (tests/_class_attn_ref.py gate(), the single place where it lives): per element
    |got - ref| <= r |ref| + 2e-4 max|ref|,
r = 2^-8 for a tensor stored as bf16, r = 0 for one stored as fp32 (P, dW1, db1, dW2, db2, everything in fp32 mode).
The kernels compute in fp32 from the stored operands and round once, so no intermediate rounding is modelled: r |ref|
admits that one rounding (half a bf16 ulp is at most 2^-8 of the value), 2e-4 max|ref| is the project's fp32 tolerance
(tests/test_kernels_gpu.py) and covers the summation order and __expf.  Every row of P sums to 1 within 1e-5.  db1 is
zero in exact arithmetic (the softmax backward sums to zero over the keys); it is held to 2e-4 of the largest dA, the
terms that cancel (zero_scale()).  tests/test_class_attn_ref_cpu.py proves that fp32 arithmetic in another summation
order meets this gate on every case here and that nine wrong restatements of the formulas do not.

Every output lives in a NaN-filled guarded allocation (tests/_guarded.py): no in-range element of out, P, dq, dkv_cls,
dkv_tok may stay NaN (they are overwritten, not accumulated into), pad columns and guards keep their bits, inputs are
not written.  dW1 / db1 / dW2 / db2 start from known nonzero values and `got - initial` is gated.

Every case prints its worst err / allowed ratio per tensor, the module prints the worst per family and dtype when it is
done (run with -s).  The gate rests on the argument above, not on those figures: a ratio above 1 is a finding to be
explained from the arithmetic, never a reason to widen gate().

Worst err / allowed seen on an MI355X, all 168 cases passing (the module takes 3.4 s):
                   out    P      dq     dkv_cls  dkv_tok  dW1    db1    dW2    db2
    plain bf16     0.928  0.006  0.879  0.872    0.933
    plain fp32     0.006  0.004  0.006  0.006    0.006
    interact. bf16 0.904  0.014  0.867  0.890    0.925    0.009  0.001  0.005  0.001
    interact. fp32 0.010  0.019  0.027  0.013    0.022    0.015  0.001  0.008  0.001
Closest to the limit: dkv_tok of plain (2, 6, 49, 4, 16) in bf16, 0.933, then out of plain (2, 3, 6, 4, 16), 0.928, and dkv_tok of
interactive (2, 4, 49, 6, 32), 0.925.  All bf16 figures near 0.9 are the one rounding of an element just above a power of two,
where half an ulp is 2^-8 of the value, i.e. all of r |ref| (the fp32 CPU evaluation of tests/test_class_attn_ref_cpu.py reaches
0.90 the same way); the fp32 rows show what the arithmetic itself uses of the floor: under 3 %, most on the sharp kind (dq of
interactive (2, 5, 49, 12, 32) sharp), where the scores reach +-60 and __expf and the fp32 score sums weigh most.
No kernel was found wrong.  The one library change these tests needed: ga_class_attn_mt_bwd accepted dout, q, kv_cls, kv_tok,
dkv_cls and dkv_tok off a 16-byte boundary and ran its 16-byte loads / stores on them; test_plain_misaligned_operand_is_refused
holds it to the GA_ERR_BAD_ARG that include/gaext.h promises.
"""
import pytest
import torch

import _class_attn_ref as R
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DT = [BF, F32]
OUTPUTS = ('out', 'P', 'dq', 'dkv_cls', 'dkv_tok')
PARAM_GRADS = ('dW1', 'db1', 'dW2', 'db2')
WORST = {}       # (family, dtype, tensor) -> (worst ratio, case label) of this run


def _ops():
    from imagenet_models_amd import ops
    return ops


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v).replace('torch.', '')


def _vec(data):
    return Guarded(1, data.numel(), data.numel(), F32, data=data.reshape(1, -1), guard=64)


def _initial(n, k):
    """known nonzero start of an accumulated parameter gradient"""
    return torch.linspace(0.5, 1.5, n, dtype=torch.float64).to(F32) * (-1.0) ** k


class Run:
    pass


def alloc(family, case, dt, kind='plain', tok_pad=0, dtok_pad=None, slice3=False, off=None):
    """the guarded operands of one case.  tok_pad / dtok_pad: pad columns of the kv_tok / dkv_tok rows; slice3: both are the
    column slice [2E, 4E) of a [rows][3 * 2E] matrix, as engine_map.py passes the k | v of one of three heads' groups;
    off: operand name -> elements its view is shifted by (misalignment)"""
    off = off or {}
    ref = R.reference(family, case, dt, kind)
    i = ref['inputs']
    B, T, Nt, heads, hd = case
    E, N = heads * hd, T + Nt
    r = Run()
    r.family, r.case, r.dt, r.kind, r.ref = family, case, dt, kind, ref
    r.tok_ld = 6 * E if slice3 else 2 * E + tok_pad
    r.dtok_ld = 6 * E if slice3 else 2 * E + (tok_pad if dtok_pad is None else dtok_pad)
    col = 2 * E if slice3 else 0
    g = lambda name, rows, width, ld, data=None, shift=0: Guarded(rows, width, ld, dt, data=data, off=shift + off.get(name, 0))
    r.q = g('q', B * T, E, E, i['q'].reshape(B * T, E))
    r.kv_cls = g('kv_cls', B * T, 2 * E, 2 * E, i['kv_cls'].reshape(B * T, 2 * E))
    r.kv_tok = g('kv_tok', B * Nt, 2 * E, r.tok_ld, i['kv_tok'].reshape(B * Nt, 2 * E), col)
    r.dout = g('dout', B * T, E, E, i['dout'].reshape(B * T, E))
    r.mask = None if i['mask'] is None else Guarded(B * T * heads, N, N, F32, data=i['mask'].reshape(-1, N))
    r.out, r.P = g('out', B * T, E, E), Guarded(B * T * heads, N, N, F32)
    r.dq, r.dkv_cls = g('dq', B * T, E, E), g('dkv_cls', B * T, 2 * E, 2 * E)
    r.dkv_tok = g('dkv_tok', B * Nt, 2 * E, r.dtok_ld, None, col)
    r.inputs = ['q', 'kv_cls', 'kv_tok', 'dout'] + (['mask'] if r.mask is not None else [])
    if family == 'ia':
        for k, n in enumerate(('W1', 'b1', 'W2', 'b2')):
            setattr(r, n, _vec(i[n]))
            setattr(r, 'd' + n, _vec(_initial(i[n].numel(), k)))
        r.inputs += ['W1', 'b1', 'W2', 'b2']
    return r


def _args(r, over):
    B, T, Nt, heads, hd = r.case
    a = dict(B=B, T=T, N=T + Nt, heads=heads, hd=hd, tok_ld=r.tok_ld, dtok_ld=r.dtok_ld)
    a.update(over)
    return a


def call_fwd(r, **over):
    ops, a = _ops(), _args(r, over)
    m = None if r.mask is None else r.mask.view
    p = ops.Plan(eager=True)
    tail = (a['B'], a['T'], a['N'], a['heads'], a['hd'], r.case[4] ** -0.5, ops.ga_dtype(r.dt))
    if r.family == 'plain':
        p.class_attn_mt_fwd(r.q.view, r.kv_cls.view, r.kv_tok.view, a['tok_ld'], r.out.view, r.P.view, m, *tail)
    else:
        p.class_attn_mt_ia_fwd(r.q.view, r.kv_cls.view, r.kv_tok.view, a['tok_ld'], r.out.view, r.P.view, m, r.W1.view, r.b1.view,
                               r.W2.view, r.b2.view, *tail)


def call_bwd(r, **over):
    ops, a = _ops(), _args(r, over)
    m = None if r.mask is None else r.mask.view
    p = ops.Plan(eager=True)
    tail = (a['B'], a['T'], a['N'], a['heads'], a['hd'], r.case[4] ** -0.5, ops.ga_dtype(r.dt))
    if r.family == 'plain':
        p.class_attn_mt_bwd(r.dout.view, r.q.view, r.kv_cls.view, r.kv_tok.view, a['tok_ld'], r.P.view, m, r.dq.view, r.dkv_cls.view,
                            r.dkv_tok.view, a['dtok_ld'], *tail)
    else:
        p.class_attn_mt_ia_bwd(r.dout.view, r.q.view, r.kv_cls.view, r.kv_tok.view, a['tok_ld'], r.P.view, m, r.W1.view, r.W2.view,
                               r.b2.view, r.dq.view, r.dkv_cls.view, r.dkv_tok.view, a['dtok_ld'], r.dW1.view, r.db1.view, r.dW2.view,
                               r.db2.view, *tail)


def check_buffers(r, fwd=True, bwd=True):
    """inputs kept their bits; out / P (fwd) and dq / dkv_cls / dkv_tok / the parameter gradients (bwd) are written in range and
    nowhere else, or (False) not touched at all"""
    torch.cuda.synchronize()
    for n in r.inputs:
        getattr(r, n).check(n, written=False)
    for n in ('out', 'P'):
        getattr(r, n).check(n, written=fwd)
    for n in ('dq', 'dkv_cls', 'dkv_tok') + (PARAM_GRADS if r.family == 'ia' else ()):
        getattr(r, n).check(n, written=bwd)


def results(r, names, calls=1):
    """the named results on the CPU in float64, shaped as the reference's; parameter gradients as (got - initial) / calls"""
    B, T, Nt, heads, hd = r.case
    E, N = heads * hd, T + Nt
    shape = dict(out=(B, T, E), P=(B, T, heads, N), dq=(B, T, E), dkv_cls=(B, T, 2 * E), dkv_tok=(B, Nt, 2 * E),
                 dW1=(heads, heads), db1=(heads,), dW2=(heads, heads), db2=(heads,))
    got = {}
    for n in names:
        x = getattr(r, n).inner().double().cpu()
        if n in PARAM_GRADS:
            x = (x - _initial(x.numel(), PARAM_GRADS.index(n)).double().reshape(1, -1)) / calls
        got[n] = x.reshape(shape[n])
    return got


def gate(r, label, names=None, calls=1):
    names = names or (OUTPUTS + (PARAM_GRADS if r.family == 'ia' else ()))
    got = results(r, names, calls)
    ratios = R.gate_all(got, r.ref)
    assert set(ratios) == set(names)
    line = [f'{n} {v:.3f}' for n, v in ratios.items()]
    bad = [f'{n}: err / allowed = {v:.3f}' for n, v in ratios.items() if not v <= 1.0]
    if 'P' in got:
        rs = R.row_sum_err(got['P'])
        line.append(f'rowsum {rs:.1e}')
        if not rs <= R.ROW_SUM_TOL:
            bad.append(f'P: a row sums to 1 +- {rs:.2e} > {R.ROW_SUM_TOL}')
    tag = f'{r.family} {label} {_id(r.case)} {r.kind} {_id(r.dt)}'
    print(f'[{tag}] ' + '  '.join(line))
    for n, v in ratios.items():
        key = (r.family, _id(r.dt), n)
        if v >= WORST.get(key, (-1.0, ''))[0]:
            WORST[key] = (v, tag)
    assert not bad, bad


def run(family, case, dt, kind='plain', label='', **kw):
    r = alloc(family, case, dt, kind, **kw)
    call_fwd(r)
    call_bwd(r)
    check_buffers(r)
    gate(r, label)
    return r


def refused(call, r, **over):
    """the library's error text if the call is refused, else None"""
    try:
        call(r, **over)
    except RuntimeError as e:
        return str(e)
    return None


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for fam, dt in sorted({k[:2] for k in WORST}):
        names = [n for n in OUTPUTS + PARAM_GRADS if (fam, dt, n) in WORST]
        print(f'\nworst err/allowed, {fam} {dt}: ' + '  '.join(f'{n} {WORST[(fam, dt, n)][0]:.3f}' for n in names))
        top = max(names, key=lambda n: WORST[(fam, dt, n)][0])
        print(f'    closest to the limit: {top} of [{WORST[(fam, dt, top)][1]}]')


# ---------------------------------------------------------------------------------------------------------------------
# plain kernels: 16 waves forward, 8 backward, a wave per k | v row, a lane per 8-channel chunk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.PLAIN_T, ids=_id)
def test_plain_token_counts(case, dt):
    """T = 1, 4 -> MT = 4; 5, 6 -> MT = 6; 7, 8 -> MT = 8"""
    run('plain', case, dt, label='T')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.PLAIN_N, ids=_id)
def test_plain_key_counts(case, dt):
    """N = T + 1 (fewer rows than waves), 9 and 17 (one more than the backward's / forward's waves), 63 / 64 / 65 and 129 (the
    64-lane softmax loop), 200"""
    run('plain', case, dt, label='N')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.PLAIN_HEADS, ids=_id)
def test_plain_head_counts(case, dt):
    """heads 8 / 9 and 16 / 17 straddle the backward's and the forward's wave count; 64 x 8 = E = 512: every lane live, the head
    loop wraps four (eight) times"""
    run('plain', case, dt, label='heads')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.PLAIN_HD, ids=_id)
def test_plain_head_widths(case, dt):
    """hd / 8 = 1, 3, 8 chunks per head; E = 8: one live lane; 16 x 32 = E = 512"""
    run('plain', case, dt, label='hd')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('form', ['pads', 'slice'])
def test_plain_strides(form, dt):
    E2 = 2 * R.PLAIN_STRIDE[3] * R.PLAIN_STRIDE[4]
    if form == 'pads':
        r = run('plain', R.PLAIN_STRIDE, dt, label='ld+16/+40', tok_pad=16, dtok_pad=40)
        assert (r.tok_ld, r.dtok_ld) == (E2 + 16, E2 + 40)
    else:
        r = run('plain', R.PLAIN_STRIDE, dt, label='slice', slice3=True)
        assert r.tok_ld == r.dtok_ld == 3 * E2 and r.kv_tok.start == r.kv_tok.ld + E2


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('kind', ['sharp', 'masked'])
@pytest.mark.parametrize('case', R.PLAIN_KIND_SHAPES, ids=_id)
def test_plain_input_kinds(case, kind, dt):
    run('plain', case, dt, kind, label='kind')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_plain_lds_bound(bwd, dt):
    """heads = 64, hd = 8, T = 8: the largest N that mt_lds (restated as R.mt_lds) keeps within 160 KiB runs and passes the
    gate; N + 1 is refused by the library before anything is launched"""
    T, heads, hd = R.PLAIN_LDS_T, R.PLAIN_LDS_HEADS, R.PLAIN_LDS_HD
    N = R.PLAIN_LDS_N[bwd]
    assert R.mt_lds(T, N, heads, hd, bwd) <= R.LDS_LIMIT < R.mt_lds(T, N + 1, heads, hd, bwd)
    r = alloc('plain', R.PLAIN_LDS[bwd], dt)
    call_fwd(r)
    if bwd:
        call_bwd(r)
    check_buffers(r, bwd=bwd)
    gate(r, f'lds N{N}', None if bwd else ('out', 'P'))
    over = alloc('plain', (1, T, N + 1 - T, heads, hd), dt)
    if bwd:
        call_fwd(over)                      # the forward still fits: P is real
        check_buffers(over, bwd=False)
    err = refused(call_bwd if bwd else call_fwd, over)
    assert err is not None and 'LDS' in err and 'code -1' in err, err
    check_buffers(over, fwd=bwd, bwd=False)


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_plain_is_bit_reproducible(dt):
    """no atomics, a fixed reduction order: two runs agree in every bit"""
    a = run('plain', R.PLAIN_TWICE, dt, label='twice')
    b = run('plain', R.PLAIN_TWICE, dt, label='twice')
    for n in OUTPUTS:
        assert torch.equal(_bits(getattr(a, n).flat), _bits(getattr(b, n).flat)), n


# ---------------------------------------------------------------------------------------------------------------------
# interactive kernels: 256 threads = 4 waves, a thread per (head, key), a wave per head / per (h, g) pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.IA_MODEL, ids=_id)
def test_ia_model_shapes(case, dt):
    run('ia', case, dt, label='model')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.IA_HEADS, ids=_id)
def test_ia_head_counts(case, dt):
    """heads 1, 4 / 5 (the 4 waves), 13 (169 (h, g) pairs)"""
    run('ia', case, dt, label='heads')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.IA_N, ids=_id)
def test_ia_key_counts(case, dt):
    """heads = 3: heads * N = 12, 189, 192, 195 (below 256 threads) and 390 (above); N around the 64 lanes"""
    run('ia', case, dt, label='N')


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.IA_T, ids=_id)
def test_ia_token_counts(case, dt):
    run('ia', case, dt, label='T')


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_ia_head_width_12_odd_strides(dt):
    """hd = 12, tok_ld = 2E + 3, dtok_ld = 2E + 5: the interactive pair reads and writes element by element, so it admits head
    widths that are no multiple of 8 and rows that are not 16-byte aligned (include/gaext.h), and computes them right"""
    r = run('ia', R.IA_HD12, dt, label='hd12 ld+3/+5', tok_pad=3, dtok_pad=5)
    assert r.tok_ld % 2 == 1 and r.dtok_ld % 2 == 1 and r.tok_ld != r.dtok_ld


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('kind', ['sharp', 'masked'])
@pytest.mark.parametrize('case', R.IA_MODEL[:2], ids=_id)
def test_ia_input_kinds(case, kind, dt):
    run('ia', case, dt, kind, label='kind')


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_ia_lds_bound(dt):
    """T = 8, heads = 12: the backward's (2T + 4) heads N fp32 planes fit 160 KiB up to N = 170; 171 is refused with nothing
    written and dW1 .. db2 unchanged"""
    T, heads, hd, N = R.IA_LDS_T, R.IA_LDS_HEADS, R.IA_LDS_HD, R.IA_LDS_N
    assert R.ia_lds(T, N, heads, True) <= R.LDS_LIMIT < R.ia_lds(T, N + 1, heads, True)
    run('ia', R.IA_LDS, dt, label=f'lds N{N}')
    over = alloc('ia', (1, T, N + 1 - T, heads, hd), dt)
    call_fwd(over)
    check_buffers(over, bwd=False)
    err = refused(call_bwd, over)
    assert err is not None and 'LDS' in err and 'code -1' in err, err
    check_buffers(over, bwd=False)


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_ia_backward_accumulates_parameter_gradients_only(dt):
    """two backward calls on the same buffers: dW1, db1, dW2, db2 hold initial + 2 * gradient (atomics: within twice the gate's
    allowance, i.e. (got - initial) / 2 within the allowance), dq / dkv_cls / dkv_tok equal the single call's"""
    one = run('ia', R.IA_TWICE, dt, label='once')
    two = alloc('ia', R.IA_TWICE, dt)
    call_fwd(two)
    call_bwd(two)
    call_bwd(two)
    check_buffers(two)
    gate(two, 'twice', PARAM_GRADS, calls=2)
    for n in ('dq', 'dkv_cls', 'dkv_tok'):
        assert torch.equal(_bits(getattr(one, n).flat), _bits(getattr(two, n).flat)), n


# ---------------------------------------------------------------------------------------------------------------------
# argument refusals.  Buffers are sized for the arguments passed, so a call that were accepted would stay in bounds.
# ---------------------------------------------------------------------------------------------------------------------
def _assert_refused(r, call, what, **over):
    err = refused(call, r, **over)
    assert err is not None, f'{what} was accepted by {r.family} {call.__name__[5:]}'
    assert 'code -1' in err and 'ga_class_attn_mt_' in err, err
    check_buffers(r, fwd=False, bwd=False)


BOTH = [
    ('T = 0', (2, 1, 20, 4, 8), dict(T=0, N=20)),
    ('T = 9', (2, 9, 20, 4, 8), {}),
    ('N = T', (2, 3, 1, 4, 8), dict(N=3)),
    ('tok_ld < 2E', (2, 3, 20, 4, 8), dict(tok_ld=2 * 32 - 8)),
]
PLAIN_ONLY = [('hd = 12', (2, 3, 20, 4, 12), {}), ('E = 520', (2, 3, 20, 65, 8), {})]


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('family', ['plain', 'ia'])
@pytest.mark.parametrize('what,case,over', BOTH, ids=[b[0].replace(' ', '') for b in BOTH])
def test_bad_arguments_are_refused(what, case, over, family, dt):
    for call in (call_fwd, call_bwd):
        _assert_refused(alloc(family, case, dt), call, what, **over)


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('what,case,over', PLAIN_ONLY, ids=[b[0].replace(' ', '') for b in PLAIN_ONLY])
def test_plain_refuses_what_its_vector_loads_cannot_do(what, case, over, dt):
    """hd % 8 != 0 and E > 512 (more 8-channel chunks than lanes); the interactive pair takes both (test_ia_head_width_12_odd_strides)"""
    for call in (call_fwd, call_bwd):
        _assert_refused(alloc('plain', case, dt), call, what, **over)


MISALIGNED = [(call_fwd, n) for n in ('q', 'kv_cls', 'kv_tok')] + [(call_bwd, n) for n in ('dout', 'q', 'kv_cls', 'kv_tok', 'dkv_cls', 'dkv_tok')]


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('call,name', MISALIGNED, ids=[f'{c.__name__[5:]}-{n}' for c, n in MISALIGNED])
def test_plain_misaligned_operand_is_refused(call, name, dt):
    """every operand the plain kernels touch with 16-byte loads / stores, one element off: GA_ERR_BAD_ARG before any launch"""
    case = (2, 3, 20, 4, 8)
    base = alloc('plain', case, dt)
    assert all(getattr(base, n).view.data_ptr() % 16 == 0 for _, n in MISALIGNED)
    r = alloc('plain', case, dt, off={name: 1})
    assert getattr(r, name).view.data_ptr() % 16 == torch.empty(0, dtype=dt).element_size()
    _assert_refused(r, call, f'{name} one element off a 16-byte boundary')
