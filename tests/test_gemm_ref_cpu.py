"""CPU: the float64 reference and the gate of tests/_gemm_ref.py, which tests/test_gemm_forms_edges_gpu.py holds the NT GEMM forms to.
The reference agrees with torch.nn.functional; fp32 restatements of the accumulation and epilogue in the kernels' documented order pass
the gate on every case of the table; each wrong restatement is rejected on every case it applies to; the measured GELU constants are
still below their allowance; the case table reaches the forms it names (256 compute units); Guarded.check() catches both faults.
The worst gate ratio of an honest restatement is 0.995 (7x256x8z128 and 257x128x8, the plain output: a value just above a power of
two, where bf16's half ulp is 2^-8 of it); run with -s for the figure of every case and for where each wrong restatement applies."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as G
from _gemm_ref import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}        # case label -> worst gate ratio of its honest restatements (printed by the last test)


def _small(c):
    return c.Z * c.M * c.N <= 200000


# ------------------------------------------------------------------------------------------------------------------------------
# reference vs torch
# ------------------------------------------------------------------------------------------------------------------------------
def _torch_gelu(x, approximate):
    x = x.clone().requires_grad_(True)
    y = F.gelu(x, approximate=approximate)
    y.sum().backward()
    return y.detach(), x.grad


def test_gelu_forms_match_torch():
    """the logistic form is torch's tanh GELU (its constant 1.5957691216 is 2 sqrt(2 / pi) to 4e-12: 1e-9 covers it), the erf form is
    torch's default, and both derivatives are what autograd gives"""
    x = torch.linspace(-13, 13, 20001, dtype=F64)
    for mine, approx, tol in ((G.gelu_tanh64, 'tanh', 1e-9), (G.gelu_erf64, 'none', 1e-14)):
        for got, ref in zip(mine(x), _torch_gelu(x, approx)):
            assert float((got - ref).abs().max()) <= tol, (approx, float((got - ref).abs().max()))


@pytest.mark.parametrize('c', [c for c in G.CASES if _small(c)], ids=repr)
def test_reference_matches_torch(c):
    """every epilogue of the reference against a composition of torch.nn.functional in float64"""
    inp = G.make_inputs(c)
    Z, tol = c.Z, 1e-11
    a = G._a_of(c, inp['a'])
    rs = inp['rowscale'].repeat_interleave(c.rps)[:c.M][None, :, None]
    for epi in c.epis:
        aa = a
        if epi == 'gen_aact':
            aa = F.gelu(G._a_of(c, inp['a_aact']))
            aa = G.rnd_to(aa, c.dt) if c.dt == G.BF else aa
        lin = torch.stack([F.linear(aa[z], inp['b'][z]) for z in range(Z)])
        pre = lin + inp['bias'][:, None, :]
        want = {}
        if epi in ('plain', 'gen_aact'):
            want['C'] = pre
        elif G.CLS[epi] == 'fc1':
            want['C'], want['C2'] = _torch_gelu(pre, 'tanh' if c.dt == G.BF else 'none')
            tol = 1e-8
        elif epi == 'fc2':
            want['C'] = pre * rs + inp['R']
        elif epi == 'fc2_nors':
            want['C'] = pre + inp['R']
        elif epi == 'dg2':
            want['C'] = lin * inp['H']
        else:
            v = G.ALPHA * lin + inp['bias'][:, None, :]
            want['C2'] = v
            want['C'] = F.relu(F.relu(v) * _torch_gelu(inp['H'], 'none')[1] * rs + inp['R'])
        if epi in ('plain', 'dg2', 'gen_full', 'gen_full_cf32'):
            want['colsum'], want['colsumsq'] = want['C'].sum(1), (want['C'] ** 2).sum(1)
        for name, o in G.reference(c, inp, epi).items():
            scale = float(o.A.abs().max())
            assert float((o.ref - want[name]).abs().max()) <= tol * scale, (epi, name)
            assert bool((o.A >= o.ref.abs() * (1 - 1e-12)).all()) or G.CLS[epi] == 'fc1', (epi, name, 'A is no absolute sum')


def test_measured_gelu_constants_are_below_their_allowance():
    """the fp32 restatements of gelu_both_fast and of the Abramowitz-Stegun erf form against float64 on the dense grid: what the module
    docstring records, and at most a quarter of what the gate allows (the cases' own pre-activations: test_restatements)"""
    k = G.gelu_constants()
    print('measured', k)
    allowed = dict(fast_act=G.G_FAST_ACT, fast_grad=G.G_FAST_GRAD, erf_act=G.G_ERF_ACT, erf_grad=G.G_ERF_GRAD)
    for n, v in k.items():
        assert v <= G.G_MEASURED[n] * 1.001, (n, v, 'the recorded measurement is stale')
        assert 4 * v <= allowed[n] * 1.02, (n, v, allowed[n])


# ------------------------------------------------------------------------------------------------------------------------------
# honest and wrong restatements on every case
# ------------------------------------------------------------------------------------------------------------------------------
def applicability():
    """[(wrong, case, family, reason or None)]: where each wrong restatement applies"""
    rows = []
    for w, (epi, _, applies) in G.WRONG.items():
        for c, fam in G.PAIRS:
            why = applies(c, fam) if epi in c.epis_of(fam) else f'no {epi} epilogue on this case and family'
            rows.append((w, c, fam, why))
    return rows


@pytest.mark.parametrize('c', G.CASES, ids=repr)
def test_restatements(c):
    """the kernels' arithmetic restated in fp32 (one rounding per MFMA of 32 products over the K slabs, the epilogue in fp32, ONE rounding
    to the storage type) stays inside the gate with ratio <= 1 for every epilogue; each wrong restatement leaves it"""
    inp = G.make_inputs(c)
    bases, accs = {}, {}
    worst = 0.0
    for epi in c.epis:
        aact = epi == 'gen_aact'
        if aact not in bases:
            bases[aact], accs[aact] = G.product(c, inp, aact), G.accumulate(c, inp, aact)
        ref = G.reference(c, inp, epi, bases[aact])
        got = G.restate(c, inp, epi, accs[aact])
        for name, o in ref.items():
            ratio = G.gate_out(c, name, got[name], o)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (epi, name, ratio)
        if G.CLS[epi] == 'fc1' and epi != 'fc1_noc2':       # the constants on this case's own pre-activations
            x = (accs[False][0].to(F64) + inp['bias'][:, None, :]).to(F32)
            den = x.to(F64).abs().clamp(min=1.0)
            f32, f64, al = (G.gelu_fast_f32, G.gelu_tanh64, (G.G_FAST_ACT, G.G_FAST_GRAD)) if c.dt == G.BF else \
                (G.gelu_erf_f32, G.gelu_erf64, (G.G_ERF_ACT, G.G_ERF_GRAD))
            for g, r, a in zip(f32(x), f64(x.to(F64)), al):
                assert 4 * float(((g.to(F64) - r).abs() / den).max()) <= a * 1.02
    WORST[c.label] = worst
    print(f'{c.label}: worst honest gate ratio {worst:.3f}')
    done = set()
    for w, (epi, names, applies) in G.WRONG.items():
        for fam in c.fams:
            if epi not in c.epis_of(fam) or applies(c, fam) is not None:
                continue
            key = (w, G.TILE_M[fam], fam in ('staged', 'dma256'), fam in ('pp', 't256'))
            if key in done:
                continue
            done.add(key)
            ref = G.reference(c, inp, epi, bases[False])
            got = G.restate(c, inp, epi, accs[False], wrong=w, fam=fam)
            ratio = max(G.gate_out(c, n, got[n], ref[n]) for n in names)
            assert ratio > 1.0, (w, fam, ratio, 'the gate accepts a wrong restatement')


def test_every_wrong_restatement_applies_somewhere_and_the_rest_is_listed():
    rows = applicability()
    for w in G.WRONG:
        on = [(c, f) for ww, c, f, why in rows if ww == w and why is None]
        off = {}
        for ww, c, f, why in rows:
            if ww == w and why is not None:
                off.setdefault(why, set()).add(c.label)
        print(f'{w}: applies to {len(on)} of {len(G.PAIRS)} case x family pairs; not where: ' +
              '; '.join(f'{why}: {", ".join(sorted(v))}' for why, v in off.items()))
        assert len(on) >= 5, w
        for fam in G.FAMILIES:        # ... and on every family, except where the family has no such epilogue or (gelu_swap) no K = 8
            if (fam == 'big' and G.WRONG[w][0] not in ('fc2', 'dg2')) or (w == 'gelu_swap' and fam in ('r3', 'pp', 't256')):
                continue
            assert any(f == fam for _, f in on), (w, fam)


def test_worst_honest_ratio_is_reported():
    if WORST:
        label = max(WORST, key=WORST.get)
        print(f'worst honest gate ratio over {len(WORST)} cases: {WORST[label]:.3f} ({label})')
        assert WORST[label] <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# the case table and the forms
# ------------------------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('gemm_forms_tool', os.path.join(ROOT, 'tools', 'gemm_forms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_case_table_reaches_the_forms_it_names():
    """under each family's knobs, with 256 compute units, ga_gemm_form names the form the table states for every launch of the GPU module
    and ga_gemm_fewrows_form names none: the descriptors are the ones tools/gemm_forms.py records from the same table"""
    T = _tool()
    from imagenet_models_amd import _lib as L
    T.prime()
    corpus = [k for k in T.test_cases() if k['src'].startswith(T.EDGES + '[')]
    want = [(f'{T.EDGES}[{fam}-{c.label}]', c.want(fam, epi)) for c, fam in G.PAIRS for epi in c.epis_of(fam)]
    assert len(corpus) == len(want)
    seen = set()
    for k, (src, form) in zip(corpus, want):
        assert k['src'] == src
        assert T.answer(k) == [form], (src, k['desc'])
        with L.knobs(**k['knobs']):
            assert T.FEWROWS['ga_gemm'](T.unpack('ga_gemm', k['desc'])) == 'none', src
        seen.add(form.split(':')[0])
    assert seen == {'staged128', 'staged96', 'staged64', 'big', 'dma128', 'dma256x128', 'dma256x96', 't256', 'pp', 'r3'}


def test_edge_list_of_the_issue_is_covered():
    """per family: M one short of / one over a tile and M < 8, a ragged and a whole last K slab, fewer slabs than ring slots, batch > 1,
    N % 8 != 0 where the family accepts it"""
    for fam, bm in G.TILE_M.items():
        cs = [c for c, f in G.PAIRS if f == fam and c.epis is G.FUSED and c.dt == G.BF]
        assert any(c.M % bm == bm - 1 for c in cs), (fam, 'one row short')
        assert any(c.M % bm == 1 for c in cs), (fam, 'one row over')
        assert any(c.M < 8 for c in cs), (fam, 'M < 8')
        assert any(c.K % 64 for c in cs) and any(c.K % 64 == 0 for c in cs), (fam, 'K slabs')
        assert any(c.Z > 1 for c in cs) and (fam == 't256' or any(c.grouped for c in cs)), (fam, 'batch')
        if fam in ('staged', 'big', 'dma128', 'dma256'):
            assert any(c.N % 8 for c in cs), (fam, 'N % 8')
        assert any(c.K % 64 > 8 for c in cs), (fam, 'a K tail of several chunks')
        if fam in G.PER_CU:      # the three grid edges: fewer tiles than workgroups, exactly one each, more (the stream crosses a tile)
            g = [G.grid(c, fam) for c in cs]
            assert any(t < w for t, w in g) and any(t == w for t, w in g) and any(t > w for t, w in g), (fam, g)
        ks = {c.K for c in cs}
        assert ks >= ({256, 264, 328, 520} if fam in ('pp', 't256') else {64, 72, 96, 104, 128, 264} if fam == 'r3' else {8, 64, 72, 128, 136, 200, 264}), (fam, ks)


# ------------------------------------------------------------------------------------------------------------------------------
# Guarded.check() on the CPU
# ------------------------------------------------------------------------------------------------------------------------------
def _guarded_cpu(rows, width, ld, dt, off=0):
    """a tests/_guarded.py Guarded whose allocation lives on the CPU (the class allocates on the device): same fields, its own check()"""
    from _guarded import Guarded, _bits
    g = object.__new__(Guarded)
    g.rows, g.width, g.ld = rows, width, ld
    g.flat = torch.full((2 * ld + rows * ld + 8,), float('nan'), dtype=dt)
    g.start = ld + off
    g.view = g.flat[g.start:g.start + rows * ld].view(rows, ld)
    g.before = _bits(g.flat).clone()
    return g


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32])
def test_guarded_check_catches_a_pad_write_and_an_unwritten_element(dt):
    g = _guarded_cpu(5, 12, 16, dt, off=8)
    g.inner().copy_(torch.ones(5, 12))
    g.check('clean')
    g.view[2, 12] = 1.0                       # a pad column
    with pytest.raises(AssertionError, match='guard / pad'):
        g.check('pad')
    g = _guarded_cpu(5, 12, 16, dt)
    g.inner().copy_(torch.ones(5, 12))
    g.flat[g.start - 1] = 0.0                 # the guard row in front
    with pytest.raises(AssertionError, match='guard / pad'):
        g.check('guard')
    g = _guarded_cpu(5, 12, 16, dt)
    g.inner().copy_(torch.ones(5, 12))
    g.view[4, 11] = float('nan')              # an in-range element the kernel never wrote
    with pytest.raises(AssertionError, match='never written'):
        g.check('unwritten')
