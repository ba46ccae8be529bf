"""The depthwise 7x7 kernels of csrc/dwconv.hip (ga_dwconv7_fwd / _bwd_data / _bwd_data2 / _bwd_weight: the scalar template, the
LDS-staged dot2 forms on 7x7 and 14x14 tiles, the MFMA Toeplitz form, the register-sliding LDS-DMA forms `rs` and the two reduce
kernels) at the edges of their launch geometry, against the float64 closed forms of tests/_dwconv7_ref.py.  The cases are that
module's CASES (shapes that depend on the CU count are derived from ga_device_info): the rs march with 0, 1, 2 and 4 steady trips
(R = 7 / 14 / 21 / 35, knobs DW_RS_ROWS / DWW_RS_ROWS), segments with halos inside the image, W = 1 .. 13 around the strips of 4,
C = 8 / 24 / 136, a persistent weight-gradient wave that walks two units, workgroups without a unit, nbw = 15 / 16 / 17 for the
reduce's group split; the dot2 forms at H, W = 1 .. 15, C = 8 / 72 / 128, walks longer than the grid, 1 .. 33 partials; the MFMA
form at C = 8 / 32 / 40, 15 / 16 / 17 / 20 tiles with and without the XCD rounding, many slices; the scalar template in fp32 and in
bf16 (C % 8 != 0) on both tilings with a last slice of 4 channels.

Every case asserts the form name the library reports (ga_dwconv7_form / ga_dwconv7_bwd_weight_form) and never skips: a regime that
is missed fails with the name obtained.  Gate: tests/_dwconv7_ref.py gate(), per element |got - ref| <= r |ref| + (u + w) A;
tests/test_dwconv7_ref_cpu.py proves that fp32 arithmetic in each form's order meets it and that fourteen wrong restatements do not.
y, dx, dx2 and the weight-gradient workspace (sized exactly to ga_dwconv7_bwd_weight_workspace, passed to the C ABI directly) live in
NaN-filled guarded allocations (tests/_guarded.py); inputs keep their bits; dw49 / dbias start from known nonzero values and
`got - initial` is gated; dx2 is bit-identical to ga_rowscale of dx and to the fp32 product; each weight gradient is run twice and
is bit-identical; the rs forward is bit-identical across R.  The `impulse` tests put one hot pixel per channel at the corners, edges,
strip, segment and tile boundaries and hold every form to the bit-exact placed taps.  (The <RES = false, Y2 = true> instantiation of
the rs kernel cannot be reached through the C ABI: ga_dwconv7_bwd_data2 requires the residual.)

Each case prints its worst err / allowed per tensor, the module prints the worst per form and dtype at the end (run with -s).

Worst err / allowed seen on an MI355X (256 CUs), all 76 tests passing.  The module takes 4.3 s (2.9 s inside the tests), its slowest
tests are `rs two-unit wave` (52 x 7 x 28 x 768, 0.57 s), `dot2_14 walk` (72 x 14 x 14 x 512, 0.49 s) and `dot2_7 walk` (0.31 s): the
sizes the CU count dictates, with the float64 reference of the cases above 2^19 elements evaluated by torch on the device;
tests/test_cswin_attn_edges_gpu.py takes 7.6 s for 150 tests in the same run.
                        fwd    fwd (no bias)  bwd    bwd+res  dw     dbias
    rs            bf16  0.991  0.992          0.993  0.989    0.022  0.007
    dot2_7x7      bf16  0.995  0.987          0.994  0.995    0.014  0.010
    dot2_14x14    bf16  0.994  0.992          0.994  0.994    0.002  0.001
    mfma          bf16  0.994  0.993          0.993  0.994
    scalar_7x7    bf16  0.978  0.988          0.986  0.993    0.020  0.013
    scalar_14x14  bf16  0.985  0.989          0.991  0.987    0.001  0.001
    scalar_7x7    fp32  0.054  0.052          0.061  0.063    0.032  0.027
    scalar_14x14  fp32  0.054  0.052          0.054  0.060    0.008  0.005
Closest to the limit: every bf16 output, at 0.98 - 0.995, and the most on the largest tensors (the walks, 1.5 M - 7 M elements): the ONE
rounding of a stored element just above a power of two, where half an ulp is 2^-8 of the value -- all of r |ref|; the fp32 CPU
evaluation of tests/test_dwconv7_ref_cpu.py reaches the same 0.993 on the small cases.  The fp32 rows show what the accumulation
itself uses of u A: 6 % (49 fused multiply-adds against the bound for 50 worst-case roundings); the weight gradients use 2 % and less,
most at nbw = 15 / 17 (4224 / 3712 channels, 2 units: 28 terms and the reduce, bounded as 48 roundings).  On the `rough` taps rs and scalar pass with
w = 0 at the same ratios (they multiply by the fp32 taps); dot2 and MFMA reach 0.73 - 0.83 of the allowance with w = 2^-9 (they round
the taps to bf16, as documented).  The names show R = 14 / 21 / 35 (1, 2 and 4 steady trips) for the forward and the weight-gradient rs
kernels, rs:R7:seg1:wpu42:nbw12 on 52 units (four waves walk two), dot2_7x7:gx128:tiles192, dot2_14x14:gx64:tiles72, mfma:gx16:tiles17 /
tiles20 and scalar_7x7+bf16 / scalar_14x14+bf16.

Found: one wrong kernel pair, no other.  The steady loops, the two-unit walk, the persistent tile walks, the ragged reduces, the bf16
scalar instantiation, the impulses (bit-exact on every form) and the refusals all hold.
  * dwconv7_dot2_kernel and dwconv7_mfma_kernel rounded the convolution to bf16 on its way through LDS (the strip / the out buffer)
    and added the residual of backward-data to THAT, rounding a second time: dx was off by up to half an ulp of the convolution, which
    is unbounded relative to dx where the residual cancels it -- 28 (dot2 7x7), 58 (dot2 14x14) and 33 (MFMA) times the allowance in the
    fp32 restatement of that order (test_rounding_before_the_residual_fails), against 0.99 for the rs and scalar forms, which add the
    residual in fp32.  The old gate (2e-2 of the tensor's maximum) could not see it.  Now the residual's 16-byte pieces pass through the
    same LDS piece first (dot2: the wave's strip, in order with the wave's own LDS operations; MFMA: the out buffer, fetched with the
    tile's prefetch and stored by commit()), and the lane that owns an element adds it to the fp32 sum before the ONE rounding; the
    second output is the stored value times the factor, as before.  The forward and the residual-free backward-data run the arithmetic
    they ran; the register-sliding forms that serve every ConvNeXt shape of the benchmark are untouched.
"""
import ctypes as C
import time

import pytest
import torch

import _dwconv7_ref as R
from _dwconv7_ref import BF, F32, F64
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu

WORST = {}       # (family, dtype, tensor) -> (worst ratio, case)
T0 = [None]
BAD_ARG = -1


def _L():
    from imagenet_models_amd import _lib
    return _lib


def _cus():
    n = C.c_int(0)
    _L().check(_L().load().ga_device_info(C.byref(n), None, None), 'ga_device_info')
    return n.value


def _gd(dt):
    return 1 if dt == BF else 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else C.c_void_p((t.view if isinstance(t, Guarded) else t).data_ptr())


def _names(geom, dt, res=0, y2=0):
    L = _L()
    lib = L.load()
    buf = C.create_string_buffer(64)
    L.check(lib.ga_dwconv7_form(*geom, _gd(dt), res, y2, buf, 64), 'ga_dwconv7_form')
    f = buf.value.decode()
    L.check(lib.ga_dwconv7_bwd_weight_form(*geom, _gd(dt), buf, 64), 'ga_dwconv7_bwd_weight_form')
    return f, buf.value.decode()


def _map(data, dt, geom):
    B, H, W, Cc = geom
    return Guarded(B * H * W, Cc, Cc, dt, data=None if data is None else data.reshape(-1, Cc), guard=(Cc + 7) // 8 * 8)   # 16-byte aligned


def _vec(data):
    return Guarded(1, data.numel(), data.numel(), F32, data=data.reshape(1, -1), guard=64)


def _note(fam, dt, tensor, ratio, label):
    key = (fam, 'bf16' if dt == BF else 'fp32', tensor)
    if ratio > WORST.get(key, (-1.0, ''))[0]:
        WORST[key] = (ratio, label)


class Run:
    """the guarded operands of one case on the device and the calls on them"""

    def __init__(self, geom, dt, i):
        self.geom, self.dt, self.i = geom, dt, i
        self.x, self.dy, self.res = (_map(i[n], dt, geom) for n in ('x', 'dy', 'res'))
        self.w49, self.bias, self.scale2 = _vec(i['w49']), _vec(i['bias']), _vec(i['scale2'])
        self.lib = _L().load()

    def out(self):
        return _map(None, self.dt, self.geom)

    def shaped(self, g):
        return g.inner().reshape(self.geom)

    def fwd(self, y, bias=True):
        return self.lib.ga_dwconv7_fwd(_ptr(self.x), _ptr(self.w49), _ptr(self.bias) if bias else None, _ptr(y), *self.geom, _gd(self.dt), _stream())

    def bwd(self, dx, res=True):
        return self.lib.ga_dwconv7_bwd_data(_ptr(self.dy), _ptr(self.w49), _ptr(self.res) if res else None, _ptr(dx), *self.geom, _gd(self.dt),
                                            _stream())

    def bwd2(self, dx, dx2):
        return self.lib.ga_dwconv7_bwd_data2(_ptr(self.dy), _ptr(self.w49), _ptr(self.res), _ptr(dx), _ptr(dx2), _ptr(self.scale2), *self.geom,
                                             _gd(self.dt), _stream())

    def workspace(self):
        need = int(self.lib.ga_dwconv7_bwd_weight_workspace(*self.geom, _gd(self.dt)))
        assert need > 0 and need % 4 == 0
        return Guarded(1, need // 4, need // 4, F32, guard=64), need

    def wgrad(self, dw, db, ws, need):
        return self.lib.ga_dwconv7_bwd_weight(_ptr(self.dy), _ptr(self.x), _ptr(dw), _ptr(db), *self.geom, _gd(self.dt), _ptr(ws), need, _stream())

    def grads(self):
        Cc = self.geom[3]
        return _vec(R.initial(49 * Cc, 0)), _vec(R.initial(Cc, 1))

    def inputs_unwritten(self):
        torch.cuda.synchronize()
        for n in ('x', 'dy', 'res', 'w49', 'bias', 'scale2'):
            getattr(self, n).check(n, written=False)


def _ok(rc, what):
    _L().check(rc, what)


def _dev(i, big):
    """the float64 operands of the reference: on the device for the large cases (the same shifted sums, run by torch)"""
    return {k: v.cuda() for k, v in i.items()} if big else i


def _f64(g, run, big):
    t = run.shaped(g).double()
    return t if big else t.cpu()


def run_case(case, kind, knobs):
    cus = _cus()
    geom = case.geom(cus)
    knobs(**case.knobs)
    label = f'{case.label} {kind} {geom}'
    fname, wname = _names(geom, case.dt)
    if 'fwd' in case.ops or 'bwd' in case.ops:
        assert R.family_of(fname) == case.fam, f'{label}: the case is meant for {case.fam}, the library runs {fname}'
        want = case.want('fwd', cus)
        assert want is None or fname == want, f'{label}: expected {want}, the library runs {fname}'
    if 'wgrad' in case.ops:
        assert R.family_of(wname) == case.fam, f'{label}: the case is meant for {case.fam}, the library runs {wname}'
        want = case.want('wgrad', cus)
        assert want is None or wname == want, f'{label}: expected {want}, the library runs {wname}'
    i = R.make_inputs(geom, case.dt, kind)
    big = geom[0] * geom[1] * geom[2] * geom[3] > 1 << 19
    d = _dev(i, big)
    r = Run(geom, case.dt, i)
    ratios = {}
    fam = R.family_of(fname)
    if 'fwd' in case.ops:
        y = r.out()
        _ok(r.fwd(y), 'fwd')
        torch.cuda.synchronize()
        y.check('y')
        ref, A = R.fwd(d['x'], d['w49'], d['bias'])
        ratios['fwd'] = R.gate_conv(_f64(y, r, big), ref, A, case.dt, fname, kind)
        if not big:                 # null bias
            y0 = r.out()
            _ok(r.fwd(y0, bias=False), 'fwd without bias')
            torch.cuda.synchronize()
            y0.check('y (no bias)')
            ref, A = R.fwd(d['x'], d['w49'], None)
            ratios['fwd_nobias'] = R.gate_conv(_f64(y0, r, big), ref, A, case.dt, fname, kind)
    if 'bwd' in case.ops:
        dx0, dx1, dx1b, dx2, rs2 = r.out(), r.out(), r.out(), r.out(), r.out()
        _ok(r.bwd(dx0, res=False), 'bwd_data without res')
        _ok(r.bwd(dx1), 'bwd_data')
        _ok(r.bwd2(dx1b, dx2), 'bwd_data2')
        n = dx1.inner().numel()
        rowscale = n // geom[0] % 8 == 0            # ga_rowscale takes images of a multiple of 8 elements (all but 1 x 1 x 68)
        if rowscale:
            _ok(r.lib.ga_rowscale(_ptr(dx1b), _ptr(r.scale2), _ptr(rs2), n, n // geom[0], _gd(case.dt), _stream()), 'rowscale')
        torch.cuda.synchronize()
        for name, g in (('dx (no res)', dx0), ('dx', dx1), ('dx of bwd_data2', dx1b), ('dx2', dx2)):
            g.check(name)
        for res, g, tag in ((None, dx0, 'bwd'), (d['res'], dx1, 'bwd+res')):
            ref, A = R.bwd_data(d['dy'], d['w49'], res)
            ratios[tag] = R.gate_conv(_f64(g, r, big), ref, A, case.dt, fname, kind)
        assert torch.equal(_bits(dx1.inner()), _bits(dx1b.inner())), f'{label}: dx of bwd_data2 differs from dx of bwd_data'
        assert not rowscale or torch.equal(_bits(dx2.inner()), _bits(rs2.inner())), f'{label}: dx2 is not ga_rowscale of dx'
        want2 = R.second_output(r.shaped(dx1b).cpu(), i['scale2'], case.dt)
        assert torch.equal(r.shaped(dx2).cpu().double(), want2.double()), f'{label}: dx2 is not dx * scale2[img]'
    if 'wgrad' in case.ops and kind == 'plain':
        ws, need = r.workspace()
        (dw, db), (dwb, dbb), (dwc, dbc) = r.grads(), r.grads(), r.grads()
        _ok(r.wgrad(dw, db, ws, need), 'bwd_weight')
        _ok(r.wgrad(dwb, dbb, ws, need), 'bwd_weight again')
        _ok(r.wgrad(dwc, None, ws, need), 'bwd_weight without dbias')
        torch.cuda.synchronize()
        # the workspace is the largest of the forms' demands: a form may leave part of it unwritten, none may write its guards
        same = _bits(ws.flat) == ws.before
        inside = torch.zeros_like(same)
        inside[ws.start:ws.start + ws.width] = True
        assert bool(same[~inside].all()), f'{label}: the workspace guards were written'
        for name, g in (('dw49', dw), ('dbias', db), ('dw49 (2)', dwb), ('dbias (2)', dbb), ('dw49 (no dbias)', dwc)):
            g.check(name)
        dbc.check('dbias of the call without dbias', written=False)
        assert torch.equal(_bits(dw.inner()), _bits(dwb.inner())) and torch.equal(_bits(db.inner()), _bits(dbb.inner())), \
            f'{label}: the weight gradient differs from run to run'
        assert torch.equal(_bits(dw.inner()), _bits(dwc.inner())), f'{label}: dw49 depends on dbias being given'
        rw, Aw, rb, Ab = R.bwd_weight(d['dy'], d['x'])
        gw = dw.inner().double().cpu().view(49, -1) - R.initial(49 * geom[3], 0).view(49, -1)
        gb = db.inner().double().cpu().view(-1) - R.initial(geom[3], 1)
        ratios['dw'] = R.gate_wgrad(gw, rw.cpu(), Aw.cpu(), wname, geom)
        ratios['dbias'] = R.gate_wgrad(gb, rb.cpu(), Ab.cpu(), wname, geom)
    r.inputs_unwritten()
    print(f'[{label} {fname} | {wname}] ' + '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    for n, v in ratios.items():
        _note(R.family_of(wname) if n in ('dw', 'dbias') else fam, case.dt, n, v, label)
    bad = {n: v for n, v in ratios.items() if not v < 1.0}
    assert not bad, f'{label}: err / allowed {bad}'
    return r


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a test that leaves the device in error ends the session: nothing more is launched on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


@pytest.fixture(scope='module', autouse=True)
def _report():
    T0[0] = time.time()
    yield
    print(f'\nworst err / allowed per form, dtype and tensor (module wall time {time.time() - T0[0]:.1f} s):')
    for k in sorted(WORST):
        print(f'    {k[0]:13s} {k[1]:5s} {k[2]:11s} {WORST[k][0]:.3f}   {WORST[k][1]}')


@pytest.mark.parametrize('case,kind', [(c, k) for c in R.CASES for k in c.kinds], ids=lambda v: str(v).replace(' ', '_'))
def test_edges(case, kind, knobs):
    run_case(case, kind, knobs)


def test_rs_forward_is_bit_identical_across_R(knobs):
    """H = 21 as one segment (R = 21: two steady trips) and as three (R = 7: halos inside the image) on the same data"""
    geom, outs = (2, 21, 8, 16), []
    i = R.make_inputs(geom, BF)
    r = Run(geom, BF, i)
    for rows in (21, 7):
        knobs(DW_RS_ROWS=rows)
        assert _names(geom, BF)[0] == f'rs:R{rows}:seg{21 // rows}:wpu1'
        y, dx, dxb, dx2 = r.out(), r.out(), r.out(), r.out()
        _ok(r.fwd(y), 'fwd')
        _ok(r.bwd(dx), 'bwd')
        _ok(r.bwd2(dxb, dx2), 'bwd2')
        torch.cuda.synchronize()
        for g in (y, dx, dxb, dx2):
            g.check(f'R{rows}')
        outs.append([_bits(g.inner()).clone() for g in (y, dx, dxb, dx2)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ----------------------------------------------------------------------------------------------------------------------------
# impulse: one hot pixel per channel, bit-exact
# ----------------------------------------------------------------------------------------------------------------------------
def _positions(B, H, W, Rr):
    ys = sorted({0, H // 2, H - 1, Rr - 1, Rr, 6, 7, 13, 14} & set(range(H)))
    xs = sorted({0, W // 2, W - 1, 3, 4, 5, 6, 7, 13, 14} & set(range(W)))
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    pos += [(H // 2, x) for x in xs] + [(y, W // 2) for y in ys] + [(v, v) for v in (6, 7, 13, 14) if v < min(H, W)]
    pos += [(a, b) for a, b in ((6, 13), (13, 6), (7, 14), (14, 7)) if a < H and b < W]
    seen, out = set(), []
    for p in pos:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


IMPULSE = [
    ('rs', BF, (3, 21, 16, 48), dict(DWW_RS=2, DW_RS_ROWS=7, DWW_RS_ROWS=7), 7),
    ('rs', BF, (3, 21, 16, 48), dict(DWW_RS=2, DW_RS_ROWS=21, DWW_RS_ROWS=21), 7),
    ('dot2_7x7', BF, (3, 15, 16, 48), R.LDS7, 7),
    ('dot2_14x14', BF, (3, 28, 28, 48), R.LDS14, 14),
    ('mfma', BF, (3, 28, 28, 48), R.MFMA, 14),
    ('scalar_7x7', BF, (3, 15, 16, 44), {}, 7),
    ('scalar_14x14', BF, (3, 28, 28, 44), {}, 14),
    ('scalar_7x7', F32, (3, 15, 16, 44), {}, 7),
    ('scalar_14x14', F32, (3, 28, 28, 44), {}, 14),
]


@pytest.mark.parametrize('fam,dt,geom,kn,Rr', IMPULSE, ids=lambda v: str(v).replace(' ', '').replace('torch.', ''))
def test_impulse_is_bit_exact(fam, dt, geom, kn, Rr, knobs):
    """channel c carries its one hot pixel (a power of two) at position c of _positions, in image c % B (the last image included);
    taps are multiples of 1/16 in [0.25, 1], bias and residual multiples of 1/8: every result is one exact product plus bias / res"""
    B, H, W, Cc = geom
    knobs(**kn)
    fname, wname = _names(geom, dt)
    assert R.family_of(fname) == fam and (fam == 'mfma' or R.family_of(wname) == fam), (fname, wname)
    pos = _positions(B, H, W, Rr)
    assert len(pos) <= Cc, (len(pos), Cc)
    g = torch.Generator().manual_seed(5)
    sgn = lambda shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    i = dict(w49=torch.randint(4, 17, (49, Cc), generator=g).double() / 16 * sgn((49, Cc)),
             bias=torch.randint(-8, 9, (Cc,), generator=g).double() / 8,
             res=torch.randint(-16, 17, geom, generator=g).double() / 8,
             dense=torch.randint(-16, 17, geom, generator=g).double() / 8,
             scale2=torch.tensor([0.0, 2.0, 0.5], dtype=F64))
    hot = torch.zeros(geom, dtype=F64)
    for c in range(Cc):
        y, x = pos[c % len(pos)]
        hot[c % B, y, x, c] = 2.0 ** ((c % 3) - 1)
    # forward / backward-data of the hot map
    r = Run(geom, dt, dict(i, x=hot, dy=hot))
    y, dx0, dx1, dxb, dx2 = (r.out() for _ in range(5))
    _ok(r.fwd(y), 'fwd')
    _ok(r.bwd(dx0, res=False), 'bwd')
    _ok(r.bwd(dx1), 'bwd res')
    _ok(r.bwd2(dxb, dx2), 'bwd2')
    torch.cuda.synchronize()
    for name, got, ref in (('fwd', y, R.fwd(hot, i['w49'], i['bias'])[0]), ('bwd', dx0, R.bwd_data(hot, i['w49'])[0]),
                           ('bwd+res', dx1, R.bwd_data(hot, i['w49'], i['res'])[0]), ('bwd2', dxb, R.bwd_data(hot, i['w49'], i['res'])[0])):
        got.check(name)
        assert torch.equal(R.rnd_to(ref, dt), ref), name                # the expectation is a value of the dtype
        bad = r.shaped(got).double().cpu() != ref
        assert not bool(bad.any()), f'{fname} {name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}'
    dx2.check('dx2')
    assert torch.equal(r.shaped(dx2).cpu().double(), R.second_output(r.shaped(dxb).cpu(), i['scale2'], dt).double())
    r.inputs_unwritten()
    # backward-weight: hot dy, dense x; initial values are multiples of 1/16
    r = Run(geom, dt, dict(i, x=i['dense'], dy=hot))
    iw = torch.randint(-32, 33, (49, Cc), generator=g).double() / 16
    ib = torch.randint(-32, 33, (Cc,), generator=g).double() / 16
    dw, db = _vec(iw), _vec(ib)
    ws, need = r.workspace()
    _ok(r.wgrad(dw, db, ws, need), 'bwd_weight')
    torch.cuda.synchronize()
    dw.check('dw49')
    db.check('dbias')
    rw, _, rb, _ = R.bwd_weight(hot, i['dense'])
    outside = rw == 0
    bad = dw.inner().double().cpu().view(49, Cc) != iw + rw
    assert not bool(bad.any()), f'{wname}: {int(bad.sum())} of dw49 differ, first at {bad.nonzero()[0].tolist()}'
    assert bool(outside.any()) and torch.equal(dw.inner().double().cpu().view(49, Cc)[outside], iw[outside])
    assert torch.equal(db.inner().double().cpu().view(-1), ib + rb)
    r.inputs_unwritten()


# ----------------------------------------------------------------------------------------------------------------------------
# refusals: GA_ERR_BAD_ARG with a message, nothing written
# ----------------------------------------------------------------------------------------------------------------------------
def _refused(rc, outs):
    assert rc == BAD_ARG and _L().last_error(), rc
    torch.cuda.synchronize()
    for g in outs:
        g.check('refused', written=False)


@pytest.mark.parametrize('dt', [BF, F32], ids=['bf16', 'fp32'])
def test_refusals(dt):
    geom = (2, 7, 5, 8)
    i = R.make_inputs(geom, dt)
    r = Run(geom, dt, i)
    lib, s, gd = r.lib, _stream(), _gd(dt)
    y, y2 = r.out(), r.out()
    dw, db = r.grads()
    ws, need = r.workspace()
    P = _ptr
    outs = (y, y2, dw, db, ws)
    bad_c = (2, 7, 5, 6)
    _refused(lib.ga_dwconv7_fwd(P(r.x), P(r.w49), P(r.bias), P(y), *bad_c, gd, s), outs)                          # C % 4 != 0
    _refused(lib.ga_dwconv7_bwd_data(P(r.dy), P(r.w49), P(r.res), P(y), *bad_c, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_data2(P(r.dy), P(r.w49), P(r.res), P(y), P(y2), P(r.scale2), *bad_c, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_weight(P(r.dy), P(r.x), P(dw), P(db), *bad_c, gd, P(ws), need, s), outs)
    _refused(lib.ga_dwconv7_fwd(None, P(r.w49), P(r.bias), P(y), *geom, gd, s), outs)                            # null required operands
    _refused(lib.ga_dwconv7_fwd(P(r.x), None, P(r.bias), P(y), *geom, gd, s), outs)
    _refused(lib.ga_dwconv7_fwd(P(r.x), P(r.w49), P(r.bias), None, *geom, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_data(None, P(r.w49), P(r.res), P(y), *geom, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_data(P(r.dy), P(r.w49), P(r.res), None, *geom, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_data2(P(r.dy), P(r.w49), None, P(y), P(y2), P(r.scale2), *geom, gd, s), outs)     # bwd_data2 without res
    _refused(lib.ga_dwconv7_bwd_data2(P(r.dy), P(r.w49), P(r.res), P(y), None, P(r.scale2), *geom, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_data2(P(r.dy), P(r.w49), P(r.res), P(y), P(y2), None, *geom, gd, s), outs)
    _refused(lib.ga_dwconv7_bwd_weight(None, P(r.x), P(dw), P(db), *geom, gd, P(ws), need, s), outs)
    _refused(lib.ga_dwconv7_bwd_weight(P(r.dy), P(r.x), None, P(db), *geom, gd, P(ws), need, s), outs)
    _refused(lib.ga_dwconv7_bwd_weight(P(r.dy), P(r.x), P(dw), P(db), *geom, gd, P(ws), need - 4, s), outs)       # one float short
    _refused(lib.ga_dwconv7_bwd_weight(P(r.dy), P(r.x), P(dw), P(db), *geom, gd, None, need, s), outs)            # null workspace
    _refused(lib.ga_dwconv7_bwd_weight(P(r.dy), P(r.x), P(dw), P(db), 0, 7, 5, 8, gd, P(ws), need, s), outs)
    r.inputs_unwritten()
    _ok(lib.ga_dwconv7_bwd_weight(P(r.dy), P(r.x), P(dw), P(db), *geom, gd, P(ws), need, s), 'the exact workspace is enough')
    torch.cuda.synchronize()
