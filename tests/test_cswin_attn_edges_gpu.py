"""CSWin stripe attention with LePE (csrc/cswin.hip: ga_cswin_attn_fwd / _bwd in the generic and the MFMA form,
ga_cswin_lepe_wgrad, the fused weight-gradient partials and ga_cswin_lepe_wgrad_reduce) at the edges of its launch geometry,
against the float64 closed forms of tests/_cswin_attn_ref.py: N = Hs Ws around the 16-token tiles and the tile counts NT = 4 /
7 (1, 2, 15 .. 17, 48, 49, 63 .. 65, 72, 81, 97, 112, 113, 121, 128), the generic form at head_dim 8 / 16 / 32 on both sides of
its two-plane / one-plane backward (109 / 110 at head_dim 32, 126 / 127 at 16), the three input kinds (`negative` makes an
unmasked pad key wrong by O(1)), work-item counts with a remainder for xcd_walk (9 .. 15, 20), 2 and 3 heads per branch, padded
and unequal row strides, column- and row-sliced operands, stripes of width 1 and 2, the partial reduce at T = 1 .. 2049 (one
split, ragged splits, an empty tail split), the unfused weight gradient's second grid-stride trip, run-to-run bit identity, the
accumulation into dw / db, and the host-side argument checks.

Gate (tests/_cswin_attn_ref.py gate(), the single place where it lives): per element
    |got - ref| <= r |ref| + 2^-8 A + 2e-4 max|ref|,
r = 2^-8 for a tensor stored as bf16, 0 for fp32 (dw / db always); A = 0 for the generic form, which rounds once, and for the
MFMA form the absolute sum of the terms that pass through one of its documented bf16 roundings (P, dS, the LePE weights); the
derivation is in that module's docstring.  tests/test_cswin_attn_ref_cpu.py proves that fp32 arithmetic with and without those
roundings meets the gate on every case here and that eleven wrong restatements do not.

Every output (out, dqkv, the partial workspace) lives in a NaN-filled guarded allocation (tests/_guarded.py): no in-range
element may stay NaN, pad columns and guards keep their bits, qkv / dout / lepe_w / lepe_b are not written.  dw / db start
from known nonzero values and `got - initial` is gated; in bf16 at head_dim 32 both forms run (knob CSWIN_MFMA), and on the
MFMA form the fused and the unfused weight gradient are each gated against float64.

Every case prints its worst err / allowed ratio per tensor, the module prints the worst per form and dtype when it is done
(run with -s).  The gate rests on the argument above, not on those figures: a ratio above 1 is a finding to be explained
from the arithmetic, never a reason to widen gate().

Worst err / allowed seen on an MI355X, all 150 tests passing (the module takes 8.0 s, its slowest test 1.0 s):
                    out    dq     dk     dv     dw     db     dw_unfused  db_unfused
    generic bf16    0.927  0.896  0.903  0.919  0.005  0.001
    generic fp32    0.017  0.022  0.019  0.007  0.005  0.003
    MFMA bf16       0.773  0.777  0.837  0.772  0.001  0.001  0.002       0.001
Closest to the limit.  Generic bf16: out of (1, 8, 192, 6, (8,4)/(4,8)), 0.927, then dv of N = 97 sharp, 0.919: the ONE rounding of
an element just above a power of two, where half an ulp is 2^-8 of the value, i.e. all of r |ref|; the fp32 CPU evaluation of
tests/test_cswin_attn_ref_cpu.py reaches the same 0.927 on the same case.  MFMA: dk and dq of N = 65 sharp, 0.837 / 0.777: near
one-hot rows put a whole element's absolute sum A into one or two terms, so the bf16 rounding of that one P / dS entry and the
element's own final rounding can both be near their worst case at once (the CPU emulation with the documented roundings gives
the same 0.837); on the plain kind the MFMA form stays near 0.6 - 0.7 because the roundings of many terms average out.  The fp32
rows show what the arithmetic itself uses of the floor: about 2 %, most on the sharp kind (dq at N = 97, dk at N = 113, the
one-plane backward), where the scores reach +-60 and __expf and the fp32 score sums weigh most.  The negative kind, which turns
an unmasked pad key into an O(1) error, passes on NT = 4 (N = 17, 49), NT = 7 (65, 97) and phase B at the same ratios as plain.

No kernel was found computing wrong.  Two library changes came with these tests:
  * the generic backward needed (4 * 128 (hd + 1) + 2 N (N + 1)) * 4 bytes of LDS -- 199 680 B at head_dim 32, N = 128 against the
    160 KiB there are -- so fp32 at head_dim 32 with N in [110, 128], bf16 at head_dim 32 with N in [113, 128] and head_dim 16 at
    N = 127 / 128 ran forward and were refused backward although include/gaext.h promises Hs Ws <= 128 for both.  Those shapes
    now run a one-plane form of the same kernel (dS and the row statistic lse in LDS, P = exp(s - lse) recomputed in the key
    phase; at most 134 144 B); every other shape runs the code it ran before.  The demand comes from one host function
    (attn_lds) that the forward and the backward launch and refuse from.  N = 109 | 110 (head_dim 32, fp32), 126 | 127 (head_dim
    16) and 113 / 121 / 128 in bf16 are gated here on both sides of each threshold.
  * ga_cswin_lepe_wgrad accepted a dout off a 16-byte boundary and an ldo that is no multiple of 8 (bf16) / 4 (fp32) elements
    and ran its 8-element loads on them; test_misaligned_operand_is_refused / test_bad_strides_are_refused hold it to the
    GA_ERR_BAD_ARG the attention entry points already gave.
"""
import pytest
import torch

import _cswin_attn_ref as R
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DT = [BF, F32]
NAMES = ('out', 'dq', 'dk', 'dv', 'dw', 'db', 'dw_unfused', 'db_unfused')
WORST = {}       # (form, dtype, tensor) -> (worst ratio, case label) of this run


def _ops():
    from imagenet_models_amd import ops
    return ops


def _id(v):
    if isinstance(v, tuple):
        return 'x'.join(_id(x) for x in v)
    return str(v).replace('torch.', '')


@pytest.fixture
def mfma_knob():
    """sets CSWIN_MFMA for one test and restores the default afterwards"""
    from imagenet_models_amd import _lib
    lib = _lib.load()
    yield lambda v: lib.ga_set_knob(b'CSWIN_MFMA', int(v))
    lib.ga_unset_knob(b'CSWIN_MFMA')


def _vec(data):
    return Guarded(1, data.numel(), data.numel(), F32, data=data.reshape(1, -1), guard=64)


def _initial(n, k):
    """known nonzero start of an accumulated parameter gradient"""
    return torch.linspace(0.5, 1.5, n, dtype=torch.float64).to(F32) * (-1.0) ** k


class Run:
    pass


def alloc(case, dt, kind='plain', ldq_pad=0, ldo_pad=0, qcol=0, ocol=0, off=None, only_wgrad=False):
    """the guarded operands of one case.  ldq_pad / ldo_pad: pad columns of the qkv | dqkv and the out | dout rows; qcol / ocol:
    the operands are the column slice starting there of a matrix that is ld wide; off: operand name -> elements its view is
    shifted by (misalignment)"""
    off = off or {}
    ref = R.reference(case, dt, kind, only_wgrad)
    i = ref['inputs']
    B, reso, C, heads, nb, cb, hpb, hd = R.geom(case)
    rows = B * reso * reso
    r = Run()
    r.case, r.dt, r.kind, r.ref, r.rows = case, dt, kind, ref, rows
    r.ldq, r.ldo = 3 * C + ldq_pad, C + ldo_pad
    g = lambda name, width, ld, col, data=None: Guarded(rows, width, ld, dt, data=data, off=col + off.get(name, 0))
    r.qkv, r.dout = g('qkv', 3 * C, r.ldq, qcol, i['qkv']), g('dout', C, r.ldo, ocol, i['dout'])
    r.out, r.dqkv = g('out', C, r.ldo, ocol), g('dqkv', 3 * C, r.ldq, qcol)
    r.lw, r.lb = [_vec(w) for w in i['lepe_w']], [_vec(b) for b in i['lepe_b']]
    grads = lambda: ([_vec(_initial(cb * 9, k)) for k in range(nb)], [_vec(_initial(cb, k + 1)) for k in range(nb)])
    (r.dw, r.db), (r.dw2, r.db2) = grads(), grads()
    r.ws = None
    return r


def desc(r, rows=None, **over):
    """the descriptor of the whole case, or of the images [rows[0], rows[1]) as engine_cswin.py slices them"""
    ops = _ops()
    B, reso, C, heads, stripes = r.case
    L = reso * reso
    b0, b1 = rows or (0, B)
    a = dict(B=b1 - b0, reso=reso, C=C, heads=heads, stripes=list(stripes), ldq=r.ldq, ldo=r.ldo)
    a.update(over)
    r.plan = ops.Plan(eager=True)
    d = r.plan.cswin_desc(r.qkv.view[b0 * L:b1 * L], r.out.view[b0 * L:b1 * L], a['B'], a['reso'], a['C'], a['heads'], a['stripes'],
                          [(w.view, b.view) for w, b in zip(r.lw, r.lb)], (C // heads) ** -0.5, ops.ga_dtype(r.dt),
                          ldq=a['ldq'], ldo=a['ldo'])
    if 'nbranch' in a:
        d.nbranch = a['nbranch']
    return d


def _pairs(dw, db):
    return [(w.view, b.view) for w, b in zip(dw, db)]


def call_all(r, rows=None):
    """forward, backward and the weight gradient(s) of the images `rows` (default: all)"""
    ops = _ops()
    L = r.case[1] ** 2
    b0, b1 = rows or (0, r.case[0])
    d = desc(r, rows)
    p = r.plan
    dout, dqkv = r.dout.view[b0 * L:b1 * L], r.dqkv.view[b0 * L:b1 * L]
    p.cswin_attn_fwd(d)
    need = ops.cswin_attn_bwd_workspace(d)
    r.fused = need > 0
    if need:
        r.ws = Guarded(1, need // 4, need // 4, F32, guard=64)
        p.cswin_attn_bwd(d, dout, dqkv, lepe_ws=r.ws.view)
        p.cswin_lepe_wgrad_reduce(d, r.ws.view, _pairs(r.dw, r.db))
        p.cswin_lepe_wgrad(d, dout, _pairs(r.dw2, r.db2))
    else:
        p.cswin_attn_bwd(d, dout, dqkv)
        p.cswin_lepe_wgrad(d, dout, _pairs(r.dw, r.db))


def check_buffers(r, written=True, grads=True):
    """inputs kept their bits; out, dqkv, the workspace and the parameter gradients are written in range and nowhere else, or
    (False) not touched at all"""
    torch.cuda.synchronize()
    for n in ('qkv', 'dout'):
        getattr(r, n).check(n, written=False)
    for n, x in [('lepe_w', r.lw), ('lepe_b', r.lb)]:
        for k, t in enumerate(x):
            t.check(f'{n}{k}', written=False)
    r.out.check('out', written=written)
    r.dqkv.check('dqkv', written=written)
    if r.ws is not None:
        r.ws.check('lepe_ws', written=written)
    for k in range(len(r.dw)):
        r.dw[k].check(f'dw{k}', written=written and grads)
        r.db[k].check(f'db{k}', written=written and grads)
        r.dw2[k].check(f'dw2_{k}', written=written and grads and r.ws is not None)
        r.db2[k].check(f'db2_{k}', written=written and grads and r.ws is not None)


def _grad(bufs, k0, calls=1):
    """(got - initial) / calls of the per-branch gradient buffers, [nb][...] in float64"""
    return torch.stack([(t.inner().double().cpu().reshape(-1) - _initial(t.width, k + k0).double()) / calls for k, t in enumerate(bufs)])


def gate(r, label, frm, calls=1, attn=True):
    nb, cb = len(r.dw), r.dw[0].width // 9
    got = dict(dw=_grad(r.dw, 0, calls).reshape(nb, cb, 9), db=_grad(r.db, 1, calls))
    if attn:
        got.update(out=r.out.inner().double().cpu(), dqkv=r.dqkv.inner().double().cpu())
    ratios = R.gate_all(got, r.ref, frm)
    if r.ws is not None:
        un = R.gate_all(dict(dw=_grad(r.dw2, 0, calls).reshape(nb, cb, 9), db=_grad(r.db2, 1, calls)), r.ref, frm)
        ratios.update(dw_unfused=un['dw'], db_unfused=un['db'])
    tag = f'{label} {_id(r.case)} {r.kind} {_id(r.dt)} {frm}'
    print(f'[{tag}] ' + '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    for n, v in ratios.items():
        key = (frm, _id(r.dt), n)
        if v >= WORST.get(key, (-1.0, ''))[0]:
            WORST[key] = (v, tag)
    bad = [f'{n}: err / allowed = {v:.3f}' for n, v in ratios.items() if not v <= 1.0]
    assert not bad, (tag, bad)


def run(case, dt, kind='plain', label='', knob=None, set_knob=None, **kw):
    """one case end to end on the form that `knob` (CSWIN_MFMA; None: the default, 1) selects"""
    if knob is not None:
        set_knob(knob)
    r = alloc(case, dt, kind, **kw)
    call_all(r)
    check_buffers(r)
    frm = R.form(case, dt, 1 if knob is None else knob)
    assert r.fused == (frm == 'mfma')
    gate(r, label, frm)
    return r


def forms(case, dt):
    """the CSWIN_MFMA settings to run: both where the MFMA form exists, else the default only"""
    return (1, 0) if R.form(case, dt) == 'mfma' else (1,)


def run_forms(case, dt, kind, label, set_knob, **kw):
    return [run(case, dt, kind, label, knob, set_knob, **kw) for knob in forms(case, dt)]


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for frm, dt in sorted({k[:2] for k in WORST}):
        names = [n for n in NAMES if (frm, dt, n) in WORST]
        print(f'\nworst err/allowed, {frm} {dt}: ' + '  '.join(f'{n} {WORST[(frm, dt, n)][0]:.3f}' for n in names))
        top = sorted(names, key=lambda n: -WORST[(frm, dt, n)][0])[:2]
        for n in top:
            print(f'    closest to the limit: {n} of [{WORST[(frm, dt, n)][1]}]')


# ---------------------------------------------------------------------------------------------------------------------
# token counts, head widths, kinds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.N_HD32, ids=_id)
def test_token_counts_head_dim_32(case, dt, mfma_knob):
    """N around the 16-token tiles and the tile counts: bf16 runs NT = 4 up to 64, NT = 7 up to 112 and the generic form above
    (and everywhere with CSWIN_MFMA = 0); the generic backward keeps two score planes up to N = 109 and one from 110 on"""
    run_forms(case, dt, 'plain', f'N{R.n_tokens(case)}', mfma_knob)


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.N_HD8 + R.N_HD16, ids=_id)
def test_token_counts_head_dim_8_and_16(case, dt):
    """the generic form at N = 1, 17, 64, 128; head_dim 16 also at 126 (two planes) and 127 (one)"""
    run(case, dt, label=f'hd{case[2] // case[3]} N{R.n_tokens(case)}')


def test_backward_serves_every_stripe_the_forward_serves():
    """include/gaext.h: Hs Ws <= 128 forward and backward.  The two-plane generic backward needs more than 160 KiB from N = 110
    (head_dim 32) and N = 127 (head_dim 16) on; those run the one-plane form.  The cases on both sides of each threshold and N =
    113 / 128 in bf16 are gated above; this pins that the table holds them and which form each takes."""
    table = set(R.N_HD32 + R.N_HD16)
    for case, dt, one_plane in ((R.col(109), F32, False), (R.col(110), F32, True), (R.two(42, 42, 3, 32), F32, False),
                                (R.col(127, 32), F32, True), (R.col(113), BF, True), (R.two(16, 16, 8), BF, True),
                                (R.two(16, 16, 8, 16), F32, False)):
        assert case in table or case in R.N_HD8
        nbytes, rc = R.bwd_lds(case, dt)
        assert rc == one_plane and nbytes <= R.LDS_LIMIT, (case, nbytes, rc)


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('case', R.KIND_SHAPES, ids=_id)
def test_input_kinds(case, kind, dt, mfma_knob):
    """N = 17, 49, 65, 97 (ragged last tile in NT = 4 and NT = 7) and 113 (generic): sharp pins the max subtraction, negative the
    pad-key masks of st_tiles and of phase B"""
    run_forms(case, dt, kind, f'kind N{R.n_tokens(case)}', mfma_knob)


# ---------------------------------------------------------------------------------------------------------------------
# work items, heads per branch, strides
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.ITEMS, ids=_id)
def test_item_counts_with_a_remainder(case, dt, mfma_knob):
    """9 .. 15 and 20 work items: xcd_walk with nwg >> 3 >= 1 and nwg & 7 != 0.  A remap that is not a bijection computes one
    window twice and leaves another NaN"""
    run_forms(case, dt, 'plain', f'items{R.n_items(case)}', mfma_knob)


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.HEADS, ids=_id)
def test_heads_per_branch(case, dt, mfma_knob):
    """2 and 3 heads per branch (the LePE weight row is the channel INSIDE the branch); C = 192: C / 8 = 24 does not divide the
    256 threads of lepe_wgrad_kernel"""
    run_forms(case, dt, 'plain', f'heads{case[3]}', mfma_knob)


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('layout', ['pads', 'slice', 'rows'])
def test_strides_and_slices(layout, dt, mfma_knob):
    C = R.STRIDE[2]
    for knob in forms(R.STRIDE, dt):
        if layout == 'pads':
            r = run(R.STRIDE, dt, label='ldq+16 ldo+40', knob=knob, set_knob=mfma_knob, ldq_pad=16, ldo_pad=40)
            assert (r.ldq, r.ldo) == (3 * C + 16, C + 40)
        elif layout == 'slice':          # qkv = columns [8, 8 + 3C) of a 3C + 24 wide matrix, out = columns [16, 16 + C) of a C + 32 wide one
            r = run(R.STRIDE, dt, label='column slice', knob=knob, set_knob=mfma_knob, ldq_pad=24, ldo_pad=32, qcol=8, ocol=16)
            assert r.qkv.start == r.qkv.ld + 8 and r.out.start == r.out.ld + 16
        else:                            # images [0, 1) and [1, 3) through two row-sliced descriptors; dw / db accumulate over both
            mfma_knob(knob)
            case = (3,) + R.STRIDE[1:]
            r = alloc(case, dt)
            call_all(r, (0, 1))
            torch.cuda.synchronize()
            L = case[1] ** 2
            assert bool(torch.isnan(r.out.inner()[L:]).all()) and bool(torch.isnan(r.dqkv.inner()[L:]).all())
            assert not bool(torch.isnan(r.out.inner()[:L]).any())
            r.ws = None                  # (the first call's partials are summed; the second call brings its own buffer)
            call_all(r, (1, 3))
            check_buffers(r)
            gate(r, 'row slices', R.form(case, dt, knob))


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('case', R.BORDERS, ids=_id)
def test_lepe_borders(case, dt, mfma_knob):
    """stripes of width 1 and 2.  With Ws = 1 (Hs = 1) the taps with dx != 0 (dy != 0) are never inside the window: their dw
    entries keep the initial value bit for bit (the kernels add an exact 0.0 or nothing)"""
    for r in run_forms(case, dt, 'plain', f'border w{min(min(s) for s in case[4])}', mfma_knob):
        for k, (hs, ws) in enumerate(case[4]):
            dead = [t for t in range(9) if (ws == 1 and t % 3 != 1) or (hs == 1 and t // 3 != 1)]
            if not dead:
                continue
            for bufs in (r.dw, r.dw2) if r.fused else (r.dw,):
                now = _bits(bufs[k].inner().reshape(-1, 9)[:, dead])
                was = _bits(_initial(bufs[k].width, k).cuda().reshape(-1, 9)[:, dead])
                assert torch.equal(now, was), f'dw{k}: a tap that is never inside the stripe changed'


# ---------------------------------------------------------------------------------------------------------------------
# LePE weight gradient: the fused partials and their reduce, the unfused kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.PARTIALS, ids=_id)
def test_fused_partials_and_their_reduce(case):
    """T = B nwin (window, head) partials: min(64, T / 32) splits of ceil(T / splits): one split up to 63, two at 64 and 67
    (34 + 33), three at 97 (33 + 33 + 31), 64 of 33 at 2049 with an empty tail split.  The fused and the unfused weight gradient
    are each gated against float64"""
    r = run(case, BF, label=f'T{case[0]}')
    assert r.fused and r.ws.width == case[0] * 320


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_unfused_weight_gradient_second_grid_stride_trip(dt):
    """C = 512: 4 rows per block and trip, the grid capped at 1024 blocks of 4 trips; 16 640 rows make the first blocks loop once
    more.  Called alone (q and k are not read and stay zero); the reference computes dw / db only"""
    case = R.WGRAD_TRIP
    B, reso, C, heads, nb, cb, hpb, hd = R.geom(case)
    rpb = 256 // (C // 8)
    assert B * reso * reso > 4 * rpb * 1024
    r = alloc(case, dt, only_wgrad=True)
    d = desc(r)
    r.plan.cswin_lepe_wgrad(d, r.dout.view, _pairs(r.dw, r.db))
    torch.cuda.synchronize()
    for t in r.dw + r.db:
        t.check('grad')
    r.qkv.check('qkv', written=False)
    r.dout.check('dout', written=False)
    gate(r, 'wgrad trip', 'generic', attn=False)


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_gradients_accumulate_and_outputs_are_bit_reproducible(dt, mfma_knob):
    """out, dqkv and the partial workspace are written with plain stores in a fixed order: two runs agree in every bit, and a
    second backward on the same buffers leaves dqkv as it was.  dw / db go through fp32 atomics and are held to bit identity only
    where ONE block adds to each element: the fused form here (T = 4 < 64: one split; one block per head and output).  The
    unfused kernel runs 4 blocks on this shape: its dw / db are gated, not compared bit for bit.  After two backward calls dw /
    db hold initial + 2 * gradient"""
    for knob in forms(R.TWICE, dt):
        a = run(R.TWICE, dt, label='once', knob=knob, set_knob=mfma_knob)
        b = run(R.TWICE, dt, label='again', knob=knob, set_knob=mfma_knob)
        for n in ('out', 'dqkv') + (('ws',) if a.fused else ()):
            assert torch.equal(_bits(getattr(a, n).flat), _bits(getattr(b, n).flat)), n
        if a.fused:
            for k in range(2):
                assert torch.equal(_bits(a.dw[k].flat), _bits(b.dw[k].flat)) and torch.equal(_bits(a.db[k].flat), _bits(b.db[k].flat))
        d = desc(b)
        if b.fused:
            b.plan.cswin_attn_bwd(d, b.dout.view, b.dqkv.view, lepe_ws=b.ws.view)
            b.plan.cswin_lepe_wgrad_reduce(d, b.ws.view, _pairs(b.dw, b.db))
            b.plan.cswin_lepe_wgrad(d, b.dout.view, _pairs(b.dw2, b.db2))
        else:
            b.plan.cswin_attn_bwd(d, b.dout.view, b.dqkv.view)
            b.plan.cswin_lepe_wgrad(d, b.dout.view, _pairs(b.dw, b.db))
        check_buffers(b)
        gate(b, 'twice', R.form(R.TWICE, dt, knob), calls=2)
        assert torch.equal(_bits(a.dqkv.flat), _bits(b.dqkv.flat))


# ---------------------------------------------------------------------------------------------------------------------
# argument refusals: host-side checks, nothing is launched.  Buffers are sized for the arguments passed.
# ---------------------------------------------------------------------------------------------------------------------
def _fwd(r, **over):
    d = desc(r, **over)
    r.plan.cswin_attn_fwd(d)


def _bwd(r, ws=None, **over):
    d = desc(r, **over)
    r.plan.cswin_attn_bwd(d, r.dout.view, r.dqkv.view, lepe_ws=ws)


def _wgrad(r, **over):
    d = desc(r, **over)
    r.plan.cswin_lepe_wgrad(d, r.dout.view, _pairs(r.dw, r.db))


def _assert_refused(r, call, fname, what, **kw):
    try:
        call(r, **kw)
        err = None
    except RuntimeError as e:
        err = str(e)
    assert err is not None, f'{what} was accepted by {fname}'
    assert 'code -1' in err and fname in err, err
    check_buffers(r, written=False)


SMALL = R.two(8, 8, 4)                      # N = 32, head_dim 32: the MFMA form in bf16
MISALIGNED = [(_fwd, 'ga_cswin_attn_fwd', 'qkv'), (_fwd, 'ga_cswin_attn_fwd', 'out'), (_bwd, 'ga_cswin_attn_bwd', 'qkv'),
              (_bwd, 'ga_cswin_attn_bwd', 'dout'), (_bwd, 'ga_cswin_attn_bwd', 'dqkv'), (_wgrad, 'ga_cswin_lepe_wgrad', 'dout')]


@pytest.mark.parametrize('dt', DT, ids=_id)
@pytest.mark.parametrize('call,fname,name', MISALIGNED, ids=[f'{f[9:]}-{n}' for _, f, n in MISALIGNED])
def test_misaligned_operand_is_refused(call, fname, name, dt):
    """every operand the kernels touch with 16-byte loads / stores, one element off"""
    base = alloc(SMALL, dt)
    assert all(getattr(base, n).view.data_ptr() % 16 == 0 for n in ('qkv', 'out', 'dout', 'dqkv'))
    r = alloc(SMALL, dt, off={name: 1})
    assert getattr(r, name).view.data_ptr() % 16 == torch.empty(0, dtype=dt).element_size()
    _assert_refused(r, call, fname, f'{name} off a 16-byte boundary')


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_bad_strides_are_refused(dt):
    C = SMALL[2]
    odd = 4 if dt == BF else 2               # a multiple of 8 bytes, not of 16; the views shifted so that row 0 stays aligned
    qoff, ooff = dict(qkv=odd, dqkv=odd), dict(out=odd, dout=odd)
    for n, o in (('qkv', alloc(SMALL, dt, ldq_pad=odd, off=qoff)), ('out', alloc(SMALL, dt, ldo_pad=odd, off=ooff))):
        assert getattr(o, n).view.data_ptr() % 16 == 0 and getattr(o, n).ld * getattr(o, n).view.element_size() % 16 == 8
    for call, fname in ((_fwd, 'ga_cswin_attn_fwd'), (_bwd, 'ga_cswin_attn_bwd')):
        _assert_refused(alloc(SMALL, dt, ldq_pad=odd, off=qoff), call, fname, 'ldq off the 16-byte element count')
        _assert_refused(alloc(SMALL, dt, ldo_pad=odd, off=ooff), call, fname, 'ldo off the 16-byte element count')
        _assert_refused(alloc(SMALL, dt), call, fname, 'ldq < 3C', ldq=3 * C - 8)
        _assert_refused(alloc(SMALL, dt), call, fname, 'ldo < C', ldo=C - 8)
    _assert_refused(alloc(SMALL, dt, ldo_pad=odd, off=ooff), _wgrad, 'ga_cswin_lepe_wgrad', 'ldo off the 16-byte element count')


@pytest.mark.parametrize('dt', DT, ids=_id)
def test_bad_shapes_are_refused(dt):
    calls = ((_fwd, 'ga_cswin_attn_fwd'), (_bwd, 'ga_cswin_attn_bwd'), (_wgrad, 'ga_cswin_lepe_wgrad'))
    for call, fname in calls:
        _assert_refused(alloc(R.col(129, B=1), dt), call, fname, 'a stripe of 129 tokens')
        _assert_refused(alloc(SMALL, dt), call, fname, 'branches with 2 and 4 windows', stripes=[(8, 4), (2, 8)])
        _assert_refused(alloc((1, 8, 48, 2, ((8, 4), (4, 8))), dt), call, fname, 'head_dim 24')
        _assert_refused(alloc(SMALL, dt), call, fname, 'nbranch = 3', nbranch=3)


def test_workspace_checks(mfma_knob):
    ops = _ops()
    r = alloc(SMALL, BF)
    need = ops.cswin_attn_bwd_workspace(desc(r)) // 4
    assert need == R.n_items(SMALL) * 320
    big = Guarded(1, need + 8, need + 8, F32, guard=64)
    _assert_refused(r, _bwd, 'ga_cswin_attn_bwd', 'a workspace one element short', ws=big.view[0, :need - 1])
    _assert_refused(r, _bwd, 'ga_cswin_attn_bwd', 'a workspace off a 16-byte boundary', ws=big.view[0, 1:need + 1])
    big.check('lepe_ws', written=False)
    # shapes on the generic form take no workspace: fp32, N > 112, and bf16 with the knob at 0
    for case, dt, knob in ((SMALL, F32, 1), (R.col(113), BF, 1), (SMALL, BF, 0)):
        mfma_knob(knob)
        g = alloc(case, dt)
        assert ops.cswin_attn_bwd_workspace(desc(g)) == 0
        _assert_refused(g, _bwd, 'ga_cswin_attn_bwd', 'a workspace for a generic-form shape', ws=big.view[0])
        try:
            g.plan.cswin_lepe_wgrad_reduce(desc(g), big.view[0], _pairs(g.dw, g.db))
            err = None
        except RuntimeError as e:
            err = str(e)
        assert err is not None and 'code -1' in err and 'ga_cswin_lepe_wgrad_reduce' in err, err
        check_buffers(g, written=False)
    big.check('lepe_ws', written=False)
