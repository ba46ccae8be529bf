"""GPU: every NT form of ga_gemm (staged 128 / 96 / 64, big, dma128, dma256x128 / x96, t256, pp, r3) isolated by its knobs and held,
at its tile, slab and grid edges, to the float64 reference and the ONE per-element gate of tests/_gemm_ref.py (its docstring has the
reference, the gate, the chains L and the measured GELU constants; tests/test_gemm_ref_cpu.py proves on the CPU that the gate passes
honest fp32 restatements and rejects wrong ones).

Every launch goes through ops.Plan.gemm; before it runs, the descriptor the plan recorded must name the form the case table states
(ops.gemm_form) and no few-row form (ops.gemm_fewrows_form): a case that lands on another form fails.  The table is written for 256
compute units; on another device the module skips.

A, B, R and H sit at a nonzero 16-byte offset in allocations whose pad columns (leading dimensions wider than the matrices) and guard
rows hold NaN; bias starts one float into its allocation, with NaN between the batch elements' vectors; C, C2 and the column sums are
tests/_guarded.py Guarded buffers: every in-range element must be written, every pad and guard element keep its bits.  The rows of a
dropped sample (row scale 0.0) must equal R bit for bit, the impulse kind's output B[n, k_m] bit for bit.

The float64 reference of a case is computed once and shared by the families and epilogues that run on it; the comparison itself runs
in float64 on the device."""
import pytest
import torch

import _gemm_ref as G
from _guarded import Guarded

pytestmark = pytest.mark.gpu

WORST = {}        # form -> (worst gate ratio, where)
_CTX = {}         # the current case's inputs, device operands and references (one case at a time)


@pytest.fixture(scope='module', autouse=True)
def _needs_256_cus():
    from imagenet_models_amd import ops
    if ops.num_cus() != 256:
        pytest.skip(f'the case table is written for 256 compute units, this device has {ops.num_cus()}')
    yield
    _CTX.clear()


def _padded(data, ld, dt):
    """[Z][rows][width] float64 values -> the [Z * rows][ld] device view of them, 16 bytes into a NaN-filled allocation with two guard
    rows in front and behind; the pad columns hold NaN"""
    Z, rows, width = data.shape
    off = 16 // torch.empty((), dtype=dt).element_size()
    flat = torch.full((4 * ld + Z * rows * ld + 2 * off,), float('nan'), dtype=dt, device='cuda')
    v = flat[2 * ld + off:2 * ld + off + Z * rows * ld].view(Z * rows, ld)
    v[:, :width] = data.reshape(Z * rows, width).to(dt).cuda()
    assert v.data_ptr() % 16 == 0
    return v


class Ctx:
    def __init__(self, c):
        self.c, self.L = c, G.layout(c)
        self.inp = inp = G.make_inputs(c)
        L, dt = self.L, c.dt
        self.A = _padded(inp['a'], L['lda'], dt)
        self.Aact = _padded(inp['a_aact'], L['lda'], dt) if 'gen_aact' in c.epis else None
        self.B = _padded(inp['b'], L['ldb'], dt)
        self.R = _padded(inp['R'], L['ldr'], dt)
        self.H = _padded(inp['H'], L['ldh'], dt)
        sb = L['strideBias']
        buf = torch.full((1 + c.Z * sb + 8,), float('nan'), device='cuda')
        self.bias = buf[1:]                                   # 4-byte aligned only
        self.bias[:c.Z * sb].view(c.Z, sb)[:, :c.N] = inp['bias'].float().cuda()
        assert self.bias.data_ptr() % 16 == 4
        self.rowscale = torch.cat([inp['rowscale'].float(), torch.full((4,), float('nan'))]).cuda()
        self.base, self.refs, self.Aimp = {}, {}, None

    def ref(self, epi):
        """{name: Out} on the device"""
        if epi not in self.refs:
            aact = epi == 'gen_aact'
            if aact not in self.base:
                self.base[aact] = G.product(self.c, self.inp, aact)
            o = G.reference(self.c, self.inp, epi, self.base[aact])
            self.refs[epi] = {n: G.Out(v.ref.cuda(), v.A.cuda(), v.E.cuda(), v.r) for n, v in o.items()}
        return self.refs[epi]

    def impulse(self):
        """A of the impulse kind and the expected output [Z][M][N] (bf16, device)"""
        if self.Aimp is None:
            c = self.c
            self.Aimp = _padded(G.make_inputs(c, 'impulse')['a'], self.L['lda'], c.dt)
            km = (7 * torch.arange(c.M) + 3) % c.K
            self.want_imp = self.inp['b'][:, :, km].transpose(1, 2).to(c.dt).cuda()
        return self.Aimp, self.want_imp


def _ctx(c):
    if c.label not in _CTX:
        _CTX.clear()
        torch.cuda.empty_cache()
        _CTX[c.label] = Ctx(c)
    return _CTX[c.label]


def _cbuf(c, L, dt):
    off = 16 // torch.empty((), dtype=dt).element_size()
    if c.grouped:
        return Guarded(c.M, c.Z * c.N, L['ldc'], dt, off=off)
    return Guarded(c.Z * c.M, c.N, L['ldc'], dt, off=off)


def _read(c, g):
    """a Guarded C as [Z][M][N]"""
    if c.grouped:
        return g.inner().view(c.M, c.Z, c.N).permute(1, 0, 2)
    return g.inner().view(c.Z, c.M, c.N)


def _launch(ops, c, fam, epi, x, impulse=False):
    """one launch through a recorded plan, after the form check; returns its Guarded outputs"""
    kw = G.gemm_kwargs(c, epi, ops, impulse)
    L = x.L
    out = {'C': _cbuf(c, L, torch.float32 if kw.get('c_f32') else c.dt)}
    if 'C2' in kw:
        out['C2'] = _cbuf(c, L, c.dt)
    for n in ('colsum', 'colsumsq'):
        if n in kw:
            out[n] = Guarded(c.Z, c.N, L['strideCol'], torch.float32, data=torch.zeros(c.Z, c.N), off=1)
    named = dict(bias=x.bias, R=x.R, H=x.H, rowscale=x.rowscale, **{n: g.view for n, g in out.items()})
    kw = {k: (named[v] if isinstance(v, str) else v) for k, v in kw.items()}
    A = x.impulse()[0] if impulse else (x.Aact if epi == 'gen_aact' else x.A)
    P = ops.Plan()
    P.gemm(A, x.B, out['C'].view, c.M, c.N, c.K, ops.ga_dtype(c.dt), **kw)
    fn, args, _ = P.calls[-1]
    d = args[0]._obj
    assert fn.__name__ == 'ga_gemm', fn.__name__
    assert ops.gemm_form(d) == c.want(fam, epi), (epi, ops.gemm_form(d), c.want(fam, epi))
    assert ops.gemm_fewrows_form(d) == 'none'
    P.run()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('c,fam', G.PAIRS, ids=[f'{f}-{c.label}' for c, f in G.PAIRS])
def test_gemm_form_at_its_edges(c, fam, knobs):
    from imagenet_models_amd import ops
    knobs(**G.FAMILIES[fam])
    x = _ctx(c)
    worst = (0.0, '')
    for epi in c.epis_of(fam):
        out = _launch(ops, c, fam, epi, x)
        form = c.want(fam, epi)
        for name, o in x.ref(epi).items():
            g = out[name]
            g.check(f'{form} {name}')
            got = (_read(c, g) if name in ('C', 'C2') else g.inner()).double()
            assert bool(torch.isfinite(got).all()), (form, name, 'not finite')
            ratio = G.gate_out(c, name, got, o)
            print(f'{form} {c.label} {epi} {name}: gate ratio {ratio:.3f}')
            worst = max(worst, (ratio, f'{c.label} {epi} {name}'))
            assert ratio <= 1.0, (form, epi, name, ratio)
        if epi == 'fc2':        # the rows of a dropped sample equal R bit for bit
            rows = (x.inp['rowscale'][torch.arange(c.M) // c.rps] == 0).cuda()
            got = _read(c, out['C'])[:, rows].contiguous().view(torch.int16)
            want = x.R[:, :c.N].view(c.Z, c.M, c.N)[:, rows].contiguous().view(torch.int16)
            assert int(rows.sum()) > 0 or c.M <= c.rps
            assert torch.equal(got, want), (form, 'rows of a dropped sample differ from R')
    if c.dt == G.BF and c.epis is G.FUSED and fam != 'big':       # impulse kind (big has no plain epilogue)
        out = _launch(ops, c, fam, 'plain', x, impulse=True)
        out['C'].check(f'{c.want(fam, "plain")} impulse C')
        got, want = _read(c, out['C']).contiguous().view(torch.int16), x.impulse()[1].contiguous().view(torch.int16)
        assert torch.equal(got, want), (fam, f'{int((got != want).sum())} elements of the impulse output are not B[n, k_m]')
    key = c.fams[fam]
    WORST[key] = max(WORST.get(key, (0.0, '')), worst)


def test_report_worst_gate_ratio_per_form():
    """the figures for the record (run with -s); every one of them was asserted <= 1 where it arose"""
    for form, (ratio, where) in sorted(WORST.items()):
        print(f'worst gate ratio {form}: {ratio:.3f} ({where})')
        assert ratio <= 1.0
