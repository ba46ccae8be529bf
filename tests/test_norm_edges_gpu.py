"""The norm kernels of csrc/norm.hip (ga_layernorm_fwd / _bwd / _bwd_dp, ga_bn_finalize, ga_affine_act, ga_bn_bwd_reduce / _apply) and
ga_layernorm_gelu_fwd / _bwd of csrc/cswin.hip at the edges of their launch geometry, against the float64 closed forms of
tests/_norm_ref.py and its ONE gate (per element |got - ref| <= r |ref| + u L A; tests/test_norm_ref_cpu.py proves that fp32 arithmetic
in each form's order meets it and that twenty wrong restatements do not).  The cases are that module's tables: every
ln_*_kernel<T, G, AFF, K> instantiation LN_DISPATCH can reach in both dtypes (one chunk on 16 lanes, LN_G12 = 4 / 16, ragged 4- and
8-chunk rows, the 8-chunk forms up to C = 4096), rows 1 / rpb - 1 / rpb / rpb + 1, every (w, dw, db) x dres x x_is_normalized variant,
null and given statistics, eps 1e-6 and 1e-5, the `plain`, `offset` and `flat` kinds; the DropPath second output at rows_per_scale
1 / 3 / 49 / 197 over sample boundaries; persistent walks longer than every workgroup cap; LayerNorm+GELU at C = 8 / 32 / 512; the
BatchNorm kernels off the block sizes, with rowscale, column-sliced x / dx (the stacked-heads layout), n apart from rows, up to their
LDS limits, and a ChunkWalk second trip with a nonzero column step.  The kernels are called through ops.Plan(eager=True); the refusals
and the calls a plan cannot express go through the C ABI.

Outputs live in NaN-filled guarded allocations (tests/_guarded.py), inputs keep their bits, dw / db / s1 / s2 start from known nonzero
values and `got - initial` is gated, dx2 is bit-identical to the fp32 product of the stored dx and scale2 on every row, y / dx / mean /
rstd and the apply kernels are bit-identical between two runs.  The backward kernels run on the statistics the forward STORED, which
are gated against float64 on their own.  No case skips; every walk asserts, through the mirror of the form selection, the grid and
trip count it is meant to reach.  Each case prints its worst err / allowed per tensor, the module prints the worst per kernel, form
and dtype at the end (run with -s).

Worst err / allowed seen on an MI355X, all 162 tests passing, none skipped.  The module takes 5.8 s (8.4 s run alone, when it also pays for the
device context and the library load); tests/test_dwconv7_edges_gpu.py takes 1.9 s for its 76 tests in the same run.  Slowest: the two ChunkWalk second trips (120,000 x 72 in a [rows][216] matrix, 0.8 s
each, most of it the host drawing 8.6 M random values four times), the first case (0.55 s with the library load) and the fp32 C = 1536
second output at rows_per_scale = 197 (0.3 s); every reference above 2^19 elements is evaluated in float64 by torch on the device.
    LayerNorm, per form G x K (lanes per row x chunks per lane):
                      fwd y  y (no w)  mean   rstd   bwd dx  dw     db
    G4xK3    bf16     0.995  0.993     0.044  0.119  0.995   0.022  0.014
    G4xK4    bf16     0.988  0.990     0.040  0.117  0.994   0.050  0.014
    G8xK3    bf16     0.991  0.993     0.043  0.118  0.993   0.046  0.027
    G8xK4    bf16     0.994  0.993     0.035  0.083  0.993   0.054  0.027
    G16xK1   bf16     0.996  0.981     0.083  0.163  0.995   0.094  0.048
    G16xK3   bf16     0.991  0.989     0.042  0.069  0.994   0.093  0.047
    G16xK4   bf16     0.992  0.984     0.030  0.089  0.994   0.096  0.048
    G32xK3   bf16     0.986  0.994     0.040  0.072  0.995   0.189  0.077
    G32xK4   bf16     0.995  0.994     0.000  0.092  0.995   0.171  0.077
    G64xK3   bf16     0.987  0.994     0.039  0.096  0.993   0.265  0.121
    G64xK4   bf16     0.993  0.975     0.000  0.077  0.994   0.236  0.124
    G64xK8   bf16     0.993  0.992     0.007  0.079  0.993   (dw is refused: more than 64 KB of LDS)
    G4xK3    fp32     0.198  0.198     0.198  0.104  0.066   0.028  0.028
    G4xK4    fp32     0.162  0.162     0.162  0.109  0.058   0.033  0.018
    G8xK3    fp32     0.146  0.146     0.146  0.089  0.056   0.064  0.055
    G8xK4    fp32     0.178  0.178     0.178  0.084  0.057   0.071  0.039
    G16xK1   fp32     0.148  0.148     0.148  0.143  0.085   0.078  0.055
    G16xK3   fp32     0.120  0.120     0.120  0.085  0.056   0.096  0.082
    G16xK4   fp32     0.126  0.126     0.126  0.081  0.050   0.097  0.102
    G32xK3   fp32     0.078  0.078     0.078  0.073  0.052   0.147  0.150
    G32xK4   fp32     0.164  0.164     0.164  0.060  0.046   0.194  0.163
    G64xK3   fp32     0.109  0.109     0.109  0.051  0.048   0.223  0.203
    G64xK4   fp32     0.155  0.155     0.155  0.053  0.047   0.250  0.237
    G64xK8   fp32     0.144  0.144     0.144  0.077  0.035   0.238  0.219
    ga_layernorm_bwd_dp  bf16  dx 0.995  dw 0.066  db 0.045       fp32  dx 0.086  dw 0.231  db 0.216      dx2: bit-identical everywhere
    LayerNorm+GELU       bf16  y 0.995  dx 0.991  mean 0.000  rstd 0.190  dw 0.063  db 0.051
                         fp32  y 0.060  dx 0.028  mean 0.131  rstd 0.161  dw 0.056  db 0.050
    bn_finalize          mean 0.111  rstd 0.173  scale 0.253  shift 0.254  running_mean 0.270  running_var 0.284
    affine_act           bf16 0.996   fp32 0.604 (0.634 on the second trip)
    bn_bwd_apply         bf16 0.996   fp32 0.371
    bn_bwd_reduce        bf16 s1 0.043  s2 0.145    fp32 s1 0.114  s2 0.115
Closest to the limit: every bf16 output at 0.98 - 0.996, the ONE rounding of a stored value just above a power of two, all of
r |ref|.  The fp32 rows show what the arithmetic itself uses of u L A: a fifth and less for the LayerNorm outputs (the worst fp32 y are
the `flat` rows, where y - b is nothing but the mean's error times rstd = 1000 and equals the mean's own ratio), a quarter for the
parameter gradients at one to four rows, 0.6 for affine_act (three roundings against L = 3).  The one-pass BatchNorm variance stays inside
its derived allowance: rstd of the `offset` columns (|mean| = 32, std about 0.65: A_var is 2400 times the variance) reaches 0.167 of
it, of the `flat` fp32 columns whose sumsq / n - mean^2 rounds below zero and is clamped 0.151.
The walks ran, by the mirror the tests assert: bf16 C = 16, 262,209 rows: G4xK3, forward and dw-free backward 4096 workgroups x 2
trips; bf16 C = 96, 16,401 rows: G16xK1, backward with dw 1024 x 2; bf16 C = 1024 and fp32 C = 2048 with LN_BWD_WGS = 64 (65,536 B of LDS):
G32xK4 / G64xK8, 64 x 3; fp32 C = 1536, 2053 rows: G64xK8, 512 x 2; LayerNorm+GELU C = 512, 4101 rows: G64, 1024 x 2; bn_bwd_reduce 256 x 4
slices, 1024 x 1 and 32 x 32, two trips each; affine_act / bn_bwd_apply 2048 workgroups, 1,080,000 chunks, dcol = 2.

Found: no wrong arithmetic -- every form, ragged or full, every variant, the boundary rows of the second output, the column slices, the
walks and the clamp hold, and the kernels are unchanged.  What was wrong were missing refusals on the host, now in csrc/norm.hip and
csrc/cswin.hip and pinned by the refusal tests:
  * ga_layernorm_bwd / _bwd_dp returned success for a db without a dw and never wrote it (the kernel reduces both under `dw`): dw and
    db are now both or neither, which is what every engine passes; C = 0 was accepted and wrote nothing: refused like the forward.
  * with dw the backward asks for 2 rpb C 4 bytes of dynamic LDS: 65,536 B at bf16 C = 1024 / 2048 and fp32 C = 2048 (served, tested),
    65,792 - 131,072 B for bf16 C in (2048, 4096].  A launch gets at most 64 KB of the 160 KB unless its kernel is opted into more
    (hipFuncAttributeMaxDynamicSharedMemorySize), which these are not: that launch could only fail.  It is refused before the
    launch, with the byte counts; the same widths without dw (no LDS) are served and tested.
  * ga_affine_act, ga_bn_bwd_reduce, ga_bn_bwd_apply divided by rows_per_scale = 0 when given a rowscale, and div_small's float
    reciprocal is exact only for rows < 2^24: both are required now (without a rowscale rows_per_scale is not looked at).
  * no entry point looked at pointer alignment, and a column slice makes a base pointer off 16 bytes easy to pass: every tensor pointer is
    held to the width of its vector accesses (16 bytes; 8 for bn_bwd_reduce in bf16), fp32 vectors to 4.
  * LN_G12 outside {4, 8, 16, 32, 64} dispatched the 64-lane kernel with the rows per workgroup of another G: clamped to 16.
Mutation check by hand (not kept): with the `ci < nch` guard taken off the forward's variance all 18 cases whose form has zero-filled
chunk slots fail (rstd at 11 - 9400 times its allowance) and the 12 full forms pass; with scale2 indexed by the next sample on a
sample's last row all 26 second-output cases fail on exactly those rows.
"""
import ctypes as C
import time

import pytest
import torch

import _norm_ref as R
from _norm_ref import BF, F32, F64, U
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu

WORST = {}       # (kernel, form, dtype, tensor) -> (worst ratio, case)
T0 = [None]
BAD_ARG = -1
BIG = 1 << 19


def _L():
    from imagenet_models_amd import _lib
    return _lib


def _plan():
    from imagenet_models_amd import ops
    return ops.Plan(eager=True)


def _gd(dt):
    return 1 if dt == BF else 0


def _dn(dt):
    return 'bf16' if dt == BF else 'fp32'


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else C.c_void_p((t.view if isinstance(t, Guarded) else t).data_ptr())


def _v(g):
    return None if g is None else g.view


def _mat(data, dt, rows, Cc, ld=None, col0=0):
    """[rows][Cc] operand: columns [col0, col0 + Cc) of a [rows][ld] matrix inside a guarded allocation (16-byte aligned)"""
    ld = ld or Cc
    return Guarded(rows, Cc, ld, dt, data=data, off=col0, guard=(ld + 7) // 8 * 8)


def _vec(data=None, n=None):
    n = data.numel() if data is not None else n
    return Guarded(1, n, n, F32, data=None if data is None else data.reshape(1, -1), guard=64)


def _f64(g, dev):
    t = g.inner().double()
    return t if dev else t.cpu()


def _vf(g, dev=False):
    return _f64(g, dev).view(-1)


def _note(kernel, form, dt, ratios, label):
    for tensor, ratio in ratios.items():
        key = (kernel, str(form), _dn(dt), tensor)
        if ratio > WORST.get(key, (-1.0, ''))[0]:
            WORST[key] = (ratio, label)


def _finish(kernel, form, dt, ratios, label):
    print(f'[{kernel} {form} {label}] ' + '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    _note(kernel, form, dt, ratios, label)
    bad = {n: v for n, v in ratios.items() if not v < 1.0}
    assert not bad, f'{kernel} {form} {label}: err / allowed {bad}'


def _unwritten(guards):
    torch.cuda.synchronize()
    for n, g in guards.items():
        if g is not None:
            g.check(n, written=False)


def _freeze(*guards):
    """an output that was checked becomes an input of later calls: from here on it has to keep its bits"""
    for g in guards:
        if g is not None:
            g.before = _bits(g.flat).clone()


def _same(a, b, what):
    assert torch.equal(_bits(a.inner()), _bits(b.inner())), f'{what}: differs from run to run'


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
    print(f'\nworst err / allowed per kernel, form, dtype and tensor (module wall time {time.time() - T0[0]:.1f} s):')
    for k in sorted(WORST):
        print(f'    {k[0]:14s} {k[1]:9s} {k[2]:5s} {k[3]:12s} {WORST[k][0]:.3f}   {WORST[k][1]}')


# ----------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------------
class Ln:
    """the guarded operands of one LayerNorm case on the device and the calls on them"""

    def __init__(self, fm, rows, i):
        self.fm, self.rows, self.C, self.dt, self.i = fm, rows, fm.C, fm.dt, i
        self.dev = rows * fm.C > BIG
        self.d = {k: v.cuda() for k, v in i.items()} if self.dev else i            # the float64 operands of the reference
        self.x, self.g, self.dres = (_mat(i[n], self.dt, rows, self.C) for n in ('x', 'g', 'dres'))
        self.w, self.b = _vec(i['w']), _vec(i['b'])
        self.inputs = dict(x=self.x, g=self.g, dres=self.dres, w=self.w, b=self.b)
        self.p = _plan()

    def out(self):
        return _mat(None, self.dt, self.rows, self.C)

    def stat(self):
        return _vec(n=self.rows)

    def fwd(self, y, aff, mean, rstd, eps, x=None):
        self.p.layernorm_fwd(_v(x or self.x), _v(self.w) if aff else None, _v(self.b) if aff else None, _v(y), _v(mean), _v(rstd), self.rows,
                             self.C, eps, _gd(self.dt))

    def bwd(self, x, mean, rstd, w, dres, dx, dw, db, xnorm, dx2=None, scale2=None, rps=1):
        self.p.layernorm_bwd(_v(self.g), _v(x), _v(mean), _v(rstd), _v(self.w) if w else None, _v(self.dres) if dres else None, _v(dx), _v(dw),
                             _v(db), self.rows, self.C, int(xnorm), _gd(self.dt), dx2=_v(dx2), scale2=_v(scale2), rows_per_scale=rps)

    def forward_checked(self, aff, stats, eps, label, twice=False):
        """y (and mean, rstd) of one forward, gated; returns the guarded outputs and the ratios"""
        fm, d = self.fm, self.d
        y, mean, rstd = self.out(), self.stat() if stats else None, self.stat() if stats else None
        self.fwd(y, aff, mean, rstd, eps)
        if twice:
            yb, mb, rb = self.out(), self.stat(), self.stat()
            self.fwd(yb, aff, mb, rb, eps)
        torch.cuda.synchronize()
        y.check('y')
        uL = U * fm.L_fwd()
        ref = R.ln_fwd(d['x'], d['w'] if aff else None, d['b'] if aff else None, eps, uL)
        ratios = {'y': R.gate(_f64(y, self.dev), *ref['y'], R.r_of(self.dt), uL)}
        if stats:
            mean.check('mean')
            rstd.check('rstd')
            ratios['mean'] = R.gate(_vf(mean, self.dev), *ref['mean'], 0.0, uL)
            ratios['rstd'] = R.gate(_vf(rstd, self.dev), *ref['rstd'], 0.0, uL)
        if twice:
            for a, b2, n in ((y, yb, 'y'), (mean, mb, 'mean'), (rstd, rb, 'rstd')):
                b2.check(n)
                _same(a, b2, f'{label} {n}')
        _freeze(y, mean, rstd)
        return y, mean, rstd, ratios

    def backward_checked(self, xg, mean, rstd, aff, dres, xnorm, grid_knob=0, scale2=None, rps=1, twice=False, label=''):
        """one backward on stored statistics, gated; aff in R.AFF_VARIANTS"""
        fm, d, dev = self.fm, self.d, self.dev
        w, grads = aff in ('w', 'all'), aff in ('all', 'dwdb')
        dx = self.out()
        dx2 = self.out() if scale2 is not None else None
        dw0, db0 = R.initial(self.C, 0), R.initial(self.C, 1)
        dw, db = (_vec(dw0), _vec(db0)) if grads else (None, None)
        self.bwd(xg, None if xnorm else mean, rstd, w, dres, dx, dw, db, xnorm, dx2, scale2, rps)
        if twice:
            dxb = self.out()
            self.bwd(xg, None if xnorm else mean, rstd, w, dres, dxb, None, None, xnorm)
        torch.cuda.synchronize()
        dx.check('dx')
        xin = _f64(xg, dev)
        mu, rs = (None if xnorm else _vf(mean, dev)), _vf(rstd, dev)
        rdx, Adx, rdw, Adw, rdb, Adb = R.ln_bwd(d['g'], xin, mu, rs, d['w'] if w else None, d['dres'] if dres else None, xnorm)
        ratios = {'dx': R.gate(_f64(dx, dev), rdx, Adx, R.r_of(self.dt), U * fm.L_bwd())}
        if grads:
            dw.check('dw')
            db.check('db')
            grid = fm.grid_bwd(self.rows, True, grid_knob)
            uL = U * fm.L_dw(self.rows, grid)
            ratios['dw'] = R.gate(_vf(dw) - dw0, rdw.cpu(), Adw.cpu() + dw0.abs(), 0.0, uL)
            ratios['db'] = R.gate(_vf(db) - db0, rdb.cpu(), Adb.cpu() + db0.abs(), 0.0, uL)
        if dx2 is not None:
            dx2.check('dx2')
            want = R.second_output(dx.inner(), _vf(scale2), rps, self.dt)
            bad = _bits(dx2.inner()) != _bits(want)
            assert not bool(bad.any()), f'{label}: dx2 is not dx * scale2[row // {rps}] on rows {bad.any(1).nonzero().view(-1)[:8].tolist()}'
        if twice:
            dxb.check('dx (2)')
            if not grads:
                _same(dx, dxb, f'{label} dx')
        return dx, ratios

    def inputs_unwritten(self, more=None):
        _unwritten(dict(self.inputs, **(more or {})))


def _set_g12(case, knobs):
    if case.form.nch == 12:
        knobs(LN_G12=case.g12)


@pytest.mark.parametrize('case', R.LN_CASES, ids=repr)
def test_layernorm_edges(case, knobs):
    _set_g12(case, knobs)
    fm = case.form
    affs = [a for a in R.AFF_VARIANTS if R.dw_served(fm) or a in ('none', 'w')]
    for rows in case.rows():
        for kind in ('plain', 'offset', 'flat'):
            label = f'{case} rows {rows} {kind}'
            ln = Ln(fm, rows, R.ln_inputs(rows, case.C, case.dt, kind))
            y, mean, rstd, rf = ln.forward_checked(True, True, R.EPS6, label, twice=kind == 'plain')
            yn, _, _, rn = ln.forward_checked(False, False, R.EPS5, label)
            _finish('ln_fwd', fm, case.dt, rf, label + ' affine eps 1e-6')
            _finish('ln_fwd', fm, case.dt, {'y (plain)': rn['y']}, label + ' no affine, no statistics, eps 1e-5')
            full = kind == 'plain'
            for aff in affs if full else affs[-1:]:
                for dres in (False, True) if full else (True,):
                    for xnorm in (False, True) if full else (False,):
                        _, rb = ln.backward_checked(yn if xnorm else ln.x, mean, rstd, aff, dres, xnorm, twice=aff == 'w' and dres, label=label)
                        _finish('ln_bwd', fm, case.dt, rb, f'{label} {aff} dres={int(dres)} xnorm={int(xnorm)}')
            ln.inputs_unwritten(dict(mean=mean, rstd=rstd, y=yn))


DP_CASES = [(n, rps) for n in ('bf16-C96', 'bf16-C96-g12_4', 'bf16-C16', 'bf16-C104', 'fp32-C48', 'fp32-C1536') for rps in R.RPS] + \
           [('bf16-C2056', 3), ('bf16-C2056', 49)]


@pytest.mark.parametrize('name,rps', DP_CASES)
def test_layernorm_droppath_second_output(name, rps, knobs):
    """ga_layernorm_bwd_dp: three whole samples and one row of a fourth; the first and last row of each sample carry their own factor"""
    case = next(c for c in R.LN_CASES if repr(c) == name)
    _set_g12(case, knobs)
    fm, rows = case.form, 3 * rps + 1
    label = f'{case} rows {rows} rps {rps}'
    ln = Ln(fm, rows, R.ln_inputs(rows, case.C, case.dt))
    sc = R.scales(4)
    assert 0.0 in sc.tolist() and 1.0 in sc.tolist() and len(set(sc.tolist())) == 4
    scale2 = _vec(sc)
    _, mean, rstd, _ = ln.forward_checked(True, True, R.EPS6, label)
    for aff in ('all', 'none') if R.dw_served(fm) else ('w', 'none'):
        dx, rb = ln.backward_checked(ln.x, mean, rstd, aff, True, False, scale2=scale2, rps=rps, label=label)
        plain, _ = ln.backward_checked(ln.x, mean, rstd, aff, True, False)
        _same(dx, plain, f'{label}: dx of bwd_dp against dx of bwd')
        _finish('ln_bwd_dp', fm, case.dt, rb, f'{label} {aff}')
    ln.inputs_unwritten(dict(mean=mean, rstd=rstd, scale2=scale2))


WALKS = [
    # (case name, rows, LN_BWD_WGS knob, variant, expected (grid fwd, trips fwd, grid bwd, trips bwd))
    ('bf16-C16', 4096 * 64 + 65, 0, 'none', (4096, 2, 4096, 2)),        # forward and dw-free backward past 4096 workgroups (8 MB)
    ('bf16-C96', 1024 * 16 + 17, 0, 'all', (1026, 1, 1024, 2)),         # backward with dw past its 1024 workgroups (C <= 128)
    ('bf16-C1024', 64 * 8 * 2 + 3, 64, 'all', (129, 1, 64, 3)),         # backward with dw past LN_BWD_WGS = 64, 65,536 B of LDS
    ('fp32-C2048', 64 * 4 * 2 + 3, 64, 'all', (129, 1, 64, 3)),         # the 8-chunk fp32 form, 65,536 B of LDS
    ('fp32-C1536', 512 * 4 + 5, 0, 'all', (514, 1, 512, 2)),            # the map_pit_s NormHead past the default 512 workgroups
]


@pytest.mark.parametrize('name,rows,wgs,aff,want', WALKS, ids=[w[0] for w in WALKS])
def test_layernorm_walks(name, rows, wgs, aff, want, knobs):
    case = next(c for c in R.LN_CASES if repr(c) == name)
    fm = case.form
    if wgs:
        knobs(LN_BWD_WGS=wgs)
    gf, gb = fm.grid_fwd(rows), fm.grid_bwd(rows, aff == 'all', wgs)
    got = (gf, fm.trips(rows, gf), gb, fm.trips(rows, gb))
    assert got == want and got[3] >= 2, f'{name}: the shape reaches {got}, the case is meant for {want}'
    label = f'{case} rows {rows} walk fwd grid {gf} x {got[1]} trips, bwd grid {gb} x {got[3]} trips'
    ln = Ln(fm, rows, R.ln_inputs(rows, case.C, case.dt))
    _, mean, rstd, rf = ln.forward_checked(True, True, R.EPS6, label)
    _finish('ln_fwd', fm, case.dt, rf, label)
    _, rb = ln.backward_checked(ln.x, mean, rstd, aff, True, False, grid_knob=wgs, label=label)
    _finish('ln_bwd', fm, case.dt, rb, label)
    ln.inputs_unwritten(dict(mean=mean, rstd=rstd))


# ----------------------------------------------------------------------------------------------------------------------------
# LayerNorm + GELU
# ----------------------------------------------------------------------------------------------------------------------------
def _lng_rows(Cc):
    G, rpb = R.lng_form(Cc)
    return sorted({1, rpb - 1, rpb + 1} - {0})


LNG = [(Cc, dt, rows) for Cc in R.LNG_C for dt in (BF, F32) for rows in _lng_rows(Cc)] + [(512, BF, 1024 * 4 + 5)]


@pytest.mark.parametrize('Cc,dt,rows', LNG, ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_gelu_edges(Cc, dt, rows):
    G, rpb = R.lng_form(Cc)
    grid = max(1, min(1024, -(-rows // rpb)))
    T = -(-rows // (grid * rpb))
    if rows > 1024 * rpb:
        assert grid == 1024 and T == 2
    lg = G.bit_length() - 1
    label = f'C{Cc} {_dn(dt)} rows {rows} G{G} bwd grid {grid} x {T} trips'
    i = R.ln_inputs(rows, Cc, dt)
    dev = rows * Cc > BIG
    d = {k: v.cuda() for k, v in i.items()} if dev else i
    x, g, w, b = _mat(i['x'], dt, rows, Cc), _mat(i['g'], dt, rows, Cc), _vec(i['w']), _vec(i['b'])
    p = _plan()
    outs = []
    for _ in range(2):
        y, dx, mean, rstd = _mat(None, dt, rows, Cc), _mat(None, dt, rows, Cc), _vec(n=rows), _vec(n=rows)
        dw0, db0 = R.initial(Cc, 0), R.initial(Cc, 1)
        dw, db = _vec(dw0), _vec(db0)
        p.layernorm_gelu_fwd(x.view, w.view, b.view, y.view, mean.view, rstd.view, rows, Cc, R.EPS6, _gd(dt))
        p.layernorm_gelu_bwd(g.view, x.view, mean.view, rstd.view, w.view, b.view, dx.view, dw.view, db.view, rows, Cc, _gd(dt))
        torch.cuda.synchronize()
        for n, t in (('y', y), ('dx', dx), ('mean', mean), ('rstd', rstd), ('dw', dw), ('db', db)):
            t.check(n)
        outs.append((y, dx, mean, rstd))
    for a, b2, n in zip(outs[0], outs[1], ('y', 'dx', 'mean', 'rstd')):
        _same(a, b2, f'{label} {n}')
    Lf = 8 + lg + 4
    ref = R.lng_fwd(d['x'], d['w'], d['b'], R.EPS6, U * Lf)
    rdx, Adx, rdw, Adw, rdb, Adb = R.lng_bwd(d['g'], d['x'], _vf(mean, dev), _vf(rstd, dev), d['w'], d['b'])
    Lb, Ld = 8 + lg + 10 + 12, T + rpb + grid + 3 + 12
    ratios = dict(mean=R.gate(_vf(mean, dev), *ref['mean'], 0.0, U * Lf), rstd=R.gate(_vf(rstd, dev), *ref['rstd'], 0.0, U * Lf),
                  y=R.gate(_f64(y, dev), *ref['y'], R.r_of(dt), U * (Lf + 12)), dx=R.gate(_f64(dx, dev), rdx, Adx, R.r_of(dt), U * Lb),
                  dw=R.gate(_vf(dw) - dw0, rdw.cpu(), Adw.cpu() + dw0.abs(), 0.0, U * Ld),
                  db=R.gate(_vf(db) - db0, rdb.cpu(), Adb.cpu() + db0.abs(), 0.0, U * Ld))
    _unwritten(dict(x=x, g=g, w=w, b=b))
    _finish('ln_gelu', f'G{G}', dt, ratios, label)


# ----------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'offset', 'flat'])
@pytest.mark.parametrize('Cc', R.BN_FINALIZE_C)
def test_bn_finalize_edges(Cc, kind):
    p = _plan()
    for n in (1, 48):
        i = R.bn_inputs(n, Cc, F32, kind)
        for running, affine, training in ((True, True, True), (False, False, True), (False, True, True), (True, True, False)):
            label = f'C{Cc} n {n} {kind} running={int(running)} affine={int(affine)} training={int(training)}'
            ins = dict(sum=_vec(i['sum']), sumsq=_vec(i['sumsq']), w=_vec(i['w']) if affine else None, b=_vec(i['b']) if affine else None)
            res = []
            for _ in range(2):
                rm, rv = (_vec(i['rmean']), _vec(i['rvar'])) if running else (None, None)
                o = {k: _vec(n=Cc) for k in ('mean', 'rstd', 'scale', 'shift')}
                p.bn_finalize(_v(ins['sum']), _v(ins['sumsq']), n, _v(ins['w']), _v(ins['b']), R.EPS5, 0.125, _v(rm), _v(rv), o['mean'].view,
                              o['rstd'].view, o['scale'].view, o['shift'].view, Cc, int(training))
                torch.cuda.synchronize()
                for k, t in o.items():
                    t.check(k)
                res.append(o)
                if running and training:
                    o.update(rmean=rm, rvar=rv)
                    rm.check('running_mean')
                    rv.check('running_var')
                elif running:
                    _unwritten(dict(rmean=rm, rvar=rv))
            for k in ('mean', 'rstd', 'scale', 'shift'):
                _same(res[0][k], res[1][k], f'{label} {k}')
            ref = R.bn_finalize(i['sum'], i['sumsq'], n, i['w'] if affine else None, i['b'] if affine else None, R.EPS5, 0.125,
                                i['rmean'] if running else None, i['rvar'] if running else None, training)
            ratios = {k: R.gate(_vf(res[0][k]), *ref[k], 0.0, U * 6) for k in ref}
            _unwritten(ins)
            _finish('bn_finalize', 'train' if training else 'eval', F32, ratios, label)
    # null mean / rstd outputs: scale and shift alone, the same bits
    both = []
    for stats in (True, False):
        o = {k: _vec(n=Cc) for k in ('scale', 'shift') + (('mean', 'rstd') if stats else ())}
        p.bn_finalize(ins['sum'].view, ins['sumsq'].view, n, None, None, R.EPS5, 0.125, None, None, _v(o.get('mean')), _v(o.get('rstd')),
                      o['scale'].view, o['shift'].view, Cc, 1)
        torch.cuda.synchronize()
        for k in o:
            o[k].check(k)
        both.append(o)
    for k in ('scale', 'shift'):
        _same(both[0][k], both[1][k], f'C{Cc} {k} without mean / rstd outputs')


class Bn:
    def __init__(self, rows, Cc, dt, kind='plain', ld=None, col0=0):
        self.rows, self.C, self.dt = rows, Cc, dt
        self.ld, self.col0 = ld or Cc, col0
        self.i = i = R.bn_inputs(rows, Cc, dt, kind)
        self.dev = rows * Cc > BIG
        self.d = {k: v.cuda() for k, v in i.items()} if self.dev else i
        self.x = _mat(i['x'], dt, rows, Cc, self.ld, col0)                  # a column slice of a wider matrix when ld > C
        self.dy, self.res, self.y_relu = (_mat(i[n], dt, rows, Cc) for n in ('dy', 'res', 'y_relu'))
        self.v = {n: _vec(i[n]) for n in ('w', 'scale', 'shift', 's1', 's2')}
        # per-channel statistics as the forward hands them over: fp32 values of the float64 ones
        fin = R.bn_finalize(i['sum'], i['sumsq'], rows, None, None, R.EPS5, 0.125, None, None)
        i['mean'], i['rstd'] = fin['mean'][0].to(F32).to(F64), fin['rstd'][0].to(F32).to(F64)
        self.d['mean'], self.d['rstd'] = (i[k].cuda() if self.dev else i[k] for k in ('mean', 'rstd'))
        self.v['mean'], self.v['rstd'] = _vec(i['mean']), _vec(i['rstd'])
        self.p = _plan()

    def rowscale(self, rps):
        sc = R.scales(-(-self.rows // rps))
        return sc, _vec(sc)

    def inputs_unwritten(self, more=None):
        _unwritten(dict(dict(x=self.x, dy=self.dy, res=self.res, y_relu=self.y_relu, **self.v), **(more or {})))

    def ldarg(self):
        return 0 if self.ld == self.C else self.ld


def _apply_rows(Cc):
    """one row; a few; the last count under one workgroup of 256 chunks, and one and two rows more (C = 8: 255 / 256 / 257 chunks;
    C = 2048: one row is exactly one workgroup)"""
    r0 = 255 * 8 // Cc
    return sorted({1, 17} | ({r0, r0 + 1, r0 + 2} if r0 else set()))


APPLY_SHAPES = [(Cc, dt) for Cc in R.BN_APPLY_C for dt in (BF, F32)]


@pytest.mark.parametrize('Cc,dt', APPLY_SHAPES + [(8192, BF), (8192, F32)], ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else f'C{v}')
def test_affine_act_edges(Cc, dt):
    n = 0
    for rows in _apply_rows(Cc):
        for ld, col0 in ((Cc, 0), (3 * Cc, Cc)):
            bn = Bn(rows, Cc, dt, ('plain', 'offset', 'flat')[n % 3], ld, col0)
            d = bn.d
            for aff, res, relu, rps in ((1, 1, 1, 1), (0, 1, 0, 49), (1, 0, 1, None), (1, 1, 0, 196), (0, 0, 1, 1)):
                n += 1
                label = f'C{Cc} {_dn(dt)} rows {rows} ld {ld} affine={aff} res={res} relu={relu} rps={rps}'
                sc, scg = bn.rowscale(rps) if rps else (None, None)
                ys = []
                for _ in range(2):
                    y = _mat(None, dt, rows, Cc)
                    bn.p.affine_act(bn.x.view, _v(bn.v['scale']) if aff else None, _v(bn.v['shift']) if aff else None, bn.res.view if res else None,
                                    y.view, rows, Cc, relu, _gd(dt), rowscale=_v(scg), rows_per_scale=rps or 1, ldx=bn.ldarg())
                    torch.cuda.synchronize()
                    y.check('y')
                    ys.append(y)
                _same(ys[0], ys[1], label)
                ref, A = R.affine_act(d['x'], d['scale'] if aff else None, d['shift'] if aff else None, d['res'] if res else None, sc, rps or 1, relu)
                bn.inputs_unwritten(dict(rowscale=scg))
                _finish('affine_act', f'ld{ld // Cc}C', dt, {'y': R.gate(_f64(ys[0], bn.dev), ref, A, R.r_of(dt), U * 3)}, label)


@pytest.mark.parametrize('Cc,dt', APPLY_SHAPES + [(4096, BF), (4096, F32)], ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else f'C{v}')
def test_bn_bwd_apply_edges(Cc, dt):
    n = 0
    for rows in _apply_rows(Cc):
        for ld, col0 in ((Cc, 0), (3 * Cc, Cc)):
            bn = Bn(rows, Cc, dt, ('plain', 'offset', 'flat')[n % 3], ld, col0)
            d = bn.d
            for w, yr, rps, nn in ((1, 1, 1, rows), (0, 0, 49, 2 * rows), (1, 1, 196, 2 * rows), (1, 0, None, rows)):
                n += 1
                label = f'C{Cc} {_dn(dt)} rows {rows} ld {ld} w={w} y_relu={yr} rps={rps} n={nn}'
                sc, scg = bn.rowscale(rps) if rps else (None, None)
                dxs = []
                for _ in range(2):
                    dx = _mat(None, dt, rows, Cc, ld, col0)               # dx a column slice as well: lddx = ldx
                    bn.p.bn_bwd_apply(bn.dy.view, bn.y_relu.view if yr else None, bn.x.view, bn.v['mean'].view, bn.v['rstd'].view,
                                      _v(bn.v['w']) if w else None, bn.v['s1'].view, bn.v['s2'].view, nn, dx.view, rows, Cc, _gd(dt),
                                      rowscale=_v(scg), rows_per_scale=rps or 1, ldx=bn.ldarg(), lddx=bn.ldarg())
                    torch.cuda.synchronize()
                    dx.check('dx')                                         # the columns outside the slice keep their bits
                    dxs.append(dx)
                _same(dxs[0], dxs[1], label)
                ref, A = R.bn_bwd_apply(d['dy'], d['x'], d['mean'], d['rstd'], d['w'] if w else None, d['s1'], d['s2'], nn, d['y_relu'] if yr else None,
                                        sc, rps or 1)
                bn.inputs_unwritten(dict(rowscale=scg))
                _finish('bn_bwd_apply', f'ld{ld // Cc}C', dt, {'dx': R.gate(_f64(dxs[0], bn.dev), ref, A, R.r_of(dt), U * 9)}, label)


@pytest.mark.parametrize('dt', [BF, F32], ids=_dn)
def test_chunk_walk_second_trip(dt):
    """C = 72 (P = 9 chunks per row) with more than 2048 * 256 chunks: every thread takes a second trip, with dcol = 524288 % 9 = 2 and
    a wrap of the column; rowscale through div_small at rows_per_scale = 196; x and dx as slices of a [rows][216] matrix"""
    Cc, rows, rps = 72, 120000, 196
    n8, stride = rows * Cc // 8, 2048 * 256
    assert n8 > stride and stride % (Cc // 8) == 2 and rows < 1 << 24
    bn = Bn(rows, Cc, dt, 'plain', 3 * Cc, Cc)
    d = bn.d
    sc, scg = bn.rowscale(rps)
    y, dx = _mat(None, dt, rows, Cc), _mat(None, dt, rows, Cc, 3 * Cc, Cc)
    bn.p.affine_act(bn.x.view, bn.v['scale'].view, bn.v['shift'].view, bn.res.view, y.view, rows, Cc, 1, _gd(dt), rowscale=scg.view, rows_per_scale=rps,
                    ldx=3 * Cc)
    bn.p.bn_bwd_apply(bn.dy.view, bn.y_relu.view, bn.x.view, bn.v['mean'].view, bn.v['rstd'].view, bn.v['w'].view, bn.v['s1'].view, bn.v['s2'].view,
                      rows, dx.view, rows, Cc, _gd(dt), rowscale=scg.view, rows_per_scale=rps, ldx=3 * Cc, lddx=3 * Cc)
    torch.cuda.synchronize()
    y.check('y')
    dx.check('dx')
    ref, A = R.affine_act(d['x'], d['scale'], d['shift'], d['res'], sc, rps, True)
    ratios = {'y': R.gate(_f64(y, True), ref, A, R.r_of(dt), U * 3)}
    ref, A = R.bn_bwd_apply(d['dy'], d['x'], d['mean'], d['rstd'], d['w'], d['s1'], d['s2'], rows, d['y_relu'], sc, rps)
    ratios['dx'] = R.gate(_f64(dx, True), ref, A, R.r_of(dt), U * 9)
    bn.inputs_unwritten(dict(rowscale=scg))
    _finish('chunk_walk', 'trip2', dt, ratios, f'C72 rows {rows} {_dn(dt)} n8 {n8} stride {stride}')


REDUCE = [(Cc, dt, rows) for Cc in R.BN_REDUCE_C for dt in (BF, F32) for rows in (1, 15, 16, 17)] + \
         [(200, BF, 16 * 256 + 33), (4, F32, 16 * 1024 + 33), (2048, BF, 16 * 32 + 19)]


@pytest.mark.parametrize('Cc,dt,rows', REDUCE, ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else str(v))
def test_bn_bwd_reduce_edges(Cc, dt, rows):
    gx, slices = R.bn_reduce_grid(rows, Cc)
    T = -(-rows // (16 * gx))
    if rows > 17:
        assert gx == max(1, 1024 // slices) and T >= 2, (gx, T)
    uL = U * (T + 16 + gx + 5)
    n = 0
    for ld, col0 in ((Cc, 0), (3 * Cc, Cc)):
        bn = Bn(rows, Cc, dt, ('plain', 'offset', 'flat')[n % 3], ld, col0)
        d = bn.d
        for yr, rps in ((1, 1), (0, None), (1, 49), (0, 196)):
            n += 1
            label = f'C{Cc} {_dn(dt)} rows {rows} ld {ld} y_relu={yr} rps={rps} grid {gx} x {slices}, {T} trips'
            sc, scg = bn.rowscale(rps) if rps else (None, None)
            s10, s20 = R.initial(Cc, 0), R.initial(Cc, 1)
            s1, s2 = _vec(s10), _vec(s20)
            bn.p.bn_bwd_reduce(bn.dy.view, bn.y_relu.view if yr else None, bn.x.view, bn.v['mean'].view, bn.v['rstd'].view, s1.view, s2.view, rows, Cc,
                               _gd(dt), rowscale=_v(scg), rows_per_scale=rps or 1, ldx=bn.ldarg())
            torch.cuda.synchronize()
            s1.check('s1')
            s2.check('s2')
            r1, A1, r2, A2 = R.bn_bwd_reduce(d['dy'], d['x'], d['mean'], d['rstd'], d['y_relu'] if yr else None, sc, rps or 1)
            ratios = {'s1': R.gate(_vf(s1) - s10, r1.cpu(), A1.cpu() + s10.abs(), 0.0, uL), 's2': R.gate(_vf(s2) - s20, r2.cpu(), A2.cpu() + s20.abs(), 0.0, uL)}
            bn.inputs_unwritten(dict(rowscale=scg))
            _finish('bn_bwd_reduce', f'ld{ld // Cc}C', dt, ratios, label)


# ----------------------------------------------------------------------------------------------------------------------------
# refusals: GA_ERR_BAD_ARG with a message on the host, nothing launched, nothing written
# ----------------------------------------------------------------------------------------------------------------------------
def _refused(rc, outs, what):
    assert rc == BAD_ARG and _L().last_error(), f'{what}: returned {rc}'
    torch.cuda.synchronize()
    for g in outs:
        g.check(f'refused ({what})', written=False)


def _off(g, nbytes):
    """the operand's address moved by nbytes (never dereferenced: the call is refused on the host)"""
    return C.c_void_p(g.view.data_ptr() + nbytes)


@pytest.mark.parametrize('dt', [BF, F32], ids=_dn)
def test_layernorm_refusals(dt, knobs):
    e = R.epc(dt)
    rows, Cc = 5, 4 * e
    lib, s, gd, P = _L().load(), _stream(), _gd(dt), _ptr
    big = 4096 if dt == BF else 2048
    x, g, dres, y, dx, dx2 = (_mat(None, dt, rows, big) for _ in range(6))
    w, b, dw, db = (_vec(n=big) for _ in range(4))
    mean, rstd, sc2 = _vec(n=rows), _vec(n=rows), _vec(n=rows)
    outs = (x, g, dres, y, dx, dx2, w, b, dw, db, mean, rstd, sc2)

    def fwd(xx=None, ww=P(w), bb=P(b), yy=None, C_=Cc, rows_=rows):
        return lib.ga_layernorm_fwd(xx or P(x), ww, bb, yy or P(y), P(mean), P(rstd), rows_, C_, R.EPS6, gd, s)

    def bwd(C_=Cc, gg=None, xx=None, dd=None, dxx=None, dww=P(dw), dbb=P(db), mm=P(mean), rows_=rows):
        return lib.ga_layernorm_bwd(gg or P(g), xx or P(x), mm, P(rstd), P(w), dd or P(dres), dxx or P(dx), dww, dbb, rows_, C_, 0, gd, s)

    def bdp(C_=Cc, rps=1, d2=None, sc=P(sc2), dww=P(dw), dbb=P(db)):
        return lib.ga_layernorm_bwd_dp(P(g), P(x), P(mean), P(rstd), P(w), P(dres), P(dx), dww, dbb, rows, C_, 0, d2 or P(dx2), sc, rps, gd, s)

    for what, rc in (
            ('fwd C off the chunk', fwd(C_=Cc + e // 2)), ('fwd C = 0', fwd(C_=0)), ('fwd C past the range', fwd(C_=512 * e + e)),
            ('fwd w without b', fwd(bb=None)), ('fwd b without w', fwd(ww=None)), ('fwd rows = 0', fwd(rows_=0)),
            ('fwd x off 16 bytes', fwd(xx=_off(x, 8))), ('fwd y off 16 bytes', fwd(yy=_off(y, 4 if dt == F32 else 2))),
            ('bwd C off the chunk', bwd(C_=Cc + e // 2)), ('bwd C = 0', bwd(C_=0)), ('bwd C past the range', bwd(C_=512 * e + e)),
            ('bwd db without dw', bwd(dww=None)), ('bwd dw without db', bwd(dbb=None)), ('bwd without mean', bwd(mm=None)),
            ('bwd g off 16 bytes', bwd(gg=_off(g, 8))), ('bwd x off 16 bytes', bwd(xx=_off(x, 8))), ('bwd dres off 16 bytes', bwd(dd=_off(dres, 8))),
            ('bwd dx off 16 bytes', bwd(dxx=_off(dx, 8))), ('bwd dw off 4 bytes', bwd(dww=_off(dw, 2))),
            ('bwd_dp C = 0', bdp(C_=0)), ('bwd_dp rows_per_scale = 0', bdp(rps=0)), ('bwd_dp db without dw', bdp(dww=None)),
            ('bwd_dp dx2 off 16 bytes', bdp(d2=_off(dx2, 8))), ('bwd_dp without scale2', bdp(sc=None))):
        _refused(rc, outs, what)
    if dt == BF:            # 2 rpb C 4 bytes of LDS for the parameter-gradient reduce: 131,072 B at C = 4096, 65,792 B at C = 2056
        for Cw in (2056, 4096):
            _refused(bwd(C_=Cw), outs, f'bwd with dw at C = {Cw}')
            _refused(bdp(C_=Cw), outs, f'bwd_dp with dw at C = {Cw}')
            assert 'LDS' in _L().last_error()
    # LN_G12 outside the dispatched group sizes is clamped to 16: the call is served, by the one-chunk form, with the same bits
    C12 = 12 * e
    i = R.ln_inputs(17, C12, dt)
    ln = Ln(R.Form(C12, dt), 17, i)
    ya, yb = ln.out(), ln.out()
    ln.fwd(ya, True, None, None, R.EPS6)
    knobs(LN_G12=5)
    ln.fwd(yb, True, None, None, R.EPS6)
    torch.cuda.synchronize()
    ya.check('y')
    yb.check('y (LN_G12 = 5)')
    _same(ya, yb, 'LN_G12 = 5 against 16')


@pytest.mark.parametrize('dt', [BF, F32], ids=_dn)
def test_layernorm_gelu_refusals(dt):
    rows, Cc = 5, 32
    lib, s, gd, P = _L().load(), _stream(), _gd(dt), _ptr
    x, g, y, dx = (_mat(None, dt, rows, Cc) for _ in range(4))
    w, b, dw, db, mean, rstd = (_vec(n=Cc) for _ in range(6))
    outs = (x, g, y, dx, w, b, dw, db, mean, rstd)

    def fwd(xx=None, yy=None, C_=Cc):
        return lib.ga_layernorm_gelu_fwd(xx or P(x), P(w), P(b), yy or P(y), P(mean), P(rstd), rows, C_, R.EPS6, gd, s)

    def bwd(gg=None, xx=None, dxx=None, C_=Cc):
        return lib.ga_layernorm_gelu_bwd(gg or P(g), xx or P(x), P(mean), P(rstd), P(w), P(b), dxx or P(dx), P(dw), P(db), rows, C_, gd, s)

    for what, rc in (('fwd C = 24', fwd(C_=24)), ('fwd C = 1024', fwd(C_=1024)), ('fwd x off 16 bytes', fwd(xx=_off(x, 8))),
                     ('fwd y off 16 bytes', fwd(yy=_off(y, 8))), ('bwd C = 4', bwd(C_=4)), ('bwd g off 16 bytes', bwd(gg=_off(g, 8))),
                     ('bwd x off 16 bytes', bwd(xx=_off(x, 8))), ('bwd dx off 16 bytes', bwd(dxx=_off(dx, 8)))):
        _refused(rc, outs, what)


@pytest.mark.parametrize('dt', [BF, F32], ids=_dn)
def test_batchnorm_refusals(dt):
    rows, Cc = 6, 16
    lib, s, gd, P = _L().load(), _stream(), _gd(dt), _ptr
    x, dy, res, yr, y, dx = (_mat(None, dt, rows, Cc) for _ in range(6))
    v = {n: _vec(n=Cc) for n in ('scale', 'shift', 'mean', 'rstd', 'w', 's1', 's2', 'rsc', 'sum', 'sumsq')}
    outs = (x, dy, res, yr, y, dx) + tuple(v.values())
    V = lambda n: P(v[n])

    def act(xx=None, yy=None, rr=None, rsc=V('rsc'), rps=2, C_=Cc, rows_=rows, ldx=0, sh=V('shift')):
        return lib.ga_affine_act(xx or P(x), V('scale'), sh, rr or P(res), rsc, rps, yy or P(y), rows_, C_, 1, gd, ldx, s)

    def red(dd=None, xx=None, rsc=V('rsc'), rps=2, C_=Cc, ldx=0, s1=V('s1')):
        return lib.ga_bn_bwd_reduce(dd or P(dy), P(yr), xx or P(x), V('mean'), V('rstd'), rsc, rps, s1, V('s2'), rows, C_, gd, ldx, s)

    def app(dd=None, xx=None, dxx=None, rsc=V('rsc'), rps=2, C_=Cc, rows_=rows, n=rows, ldx=0, lddx=0):
        return lib.ga_bn_bwd_apply(dd or P(dy), P(yr), xx or P(x), V('mean'), V('rstd'), V('w'), V('s1'), V('s2'), rsc, rps, n, dxx or P(dx), rows_, C_,
                                   gd, ldx, lddx, s)

    def fin(sm=V('sum'), C_=Cc, n=rows, sc=V('scale')):
        return lib.ga_bn_finalize(sm, V('sumsq'), n, V('w'), V('w'), R.EPS5, 0.125, None, None, V('mean'), V('rstd'), sc, V('shift'), C_, 1, s)

    half = 8                               # half a 16-byte piece
    for what, rc in (
            ('affine_act rows_per_scale = 0', act(rps=0)), ('affine_act rows_per_scale < 0', act(rps=-3)), ('affine_act rows = 2^24', act(rows_=1 << 24)),
            ('affine_act C off 8', act(C_=12)), ('affine_act C past the LDS table', act(C_=8200)), ('affine_act scale without shift', act(sh=None)),
            ('affine_act ldx < C', act(ldx=8)), ('affine_act x off 16 bytes', act(xx=_off(x, half))), ('affine_act y off 16 bytes', act(yy=_off(y, half))),
            ('affine_act res off 16 bytes', act(rr=_off(res, half))), ('affine_act rowscale off 4 bytes', act(rsc=_off(v['rsc'], 2))),
            ('bn_bwd_reduce rows_per_scale = 0', red(rps=0)), ('bn_bwd_reduce C off 4', red(C_=6)), ('bn_bwd_reduce C = 0', red(C_=0)),
            ('bn_bwd_reduce ldx off 4', red(ldx=18)), ('bn_bwd_reduce dy misaligned', red(dd=_off(dy, 4))), ('bn_bwd_reduce x misaligned', red(xx=_off(x, 4))),
            ('bn_bwd_reduce s1 off 4 bytes', red(s1=_off(v['s1'], 2))),
            ('bn_bwd_apply rows_per_scale = 0', app(rps=0)), ('bn_bwd_apply rows = 2^24', app(rows_=1 << 24)), ('bn_bwd_apply n = 0', app(n=0)),
            ('bn_bwd_apply C past the LDS table', app(C_=4104)), ('bn_bwd_apply lddx off 8', app(lddx=20)), ('bn_bwd_apply dy off 16 bytes', app(dd=_off(dy, half))),
            ('bn_bwd_apply x off 16 bytes', app(xx=_off(x, half))), ('bn_bwd_apply dx off 16 bytes', app(dxx=_off(dx, half))),
            ('bn_finalize C = 0', fin(C_=0)), ('bn_finalize n = 0', fin(n=0)), ('bn_finalize without sum', fin(sm=None)),
            ('bn_finalize sum off 4 bytes', fin(sm=_off(v['sum'], 2))), ('bn_finalize scale off 4 bytes', fin(sc=_off(v['scale'], 1)))):
        _refused(rc, outs, what)
    # without a rowscale, rows_per_scale is not looked at: the call is served
    i = R.bn_inputs(rows, Cc, dt)
    xi, yo = _mat(i['x'], dt, rows, Cc), _mat(None, dt, rows, Cc)
    _L().check(lib.ga_affine_act(P(xi), None, None, None, None, 0, P(yo), rows, Cc, 0, gd, 0, s), 'affine_act without rowscale, rows_per_scale = 0')
    torch.cuda.synchronize()
    yo.check('y')
    assert torch.equal(_bits(yo.inner()), _bits(xi.inner()))
