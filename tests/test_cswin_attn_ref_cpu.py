"""tests/_cswin_attn_ref.py checked without a GPU, for every case that tests/test_cswin_attn_edges_gpu.py gates:
  * the float64 closed forms equal oracle.ga_cswin_oracle.lepe_attention (the restatement of LePEAttention, itself pinned
    by tests/golden/cswin_modules.npz) evaluated in float64 with torch.autograd, within 1e-10 relative, and reproduce the real
    module's vectors of tests/golden/cswin_modules.npz at the fp32 tolerance of test_stripe_attention_vs_reference_vectors;
  * the gate is reachable: a float32 evaluation of the formulas in reversed token order, rounded where the kernels store,
    meets the generic gate, and one that also rounds P, dS and the LePE weights to bf16 where the MFMA kernels do meets the
    MFMA gate, on every case, kind and dtype of the GPU table;
  * the gate is sharp: each of the wrong restatements of R.WRONG is rejected under the generic fp32, the generic bf16 and the
    MFMA gate, on at least one case of every input kind."""
import os

import numpy as np
import pytest
import torch

import _cswin_attn_ref as R
from conftest import GOLDEN

F64, F32, BF = R.F64, R.F32, R.BF
CASES = R.gated()


def _id(v):
    if isinstance(v, tuple):
        return 'x'.join(_id(x) for x in v)
    return str(v).replace('torch.', '')


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _oracle(i):
    """out, dqkv, dw, db by autograd through the oracle's LePEAttention restatement, float64"""
    from oracle import ga_cswin_oracle as O
    case = i['case']
    B, reso, C, heads, nb, cb, hpb, hd = R.geom(case)
    L = reso * reso
    q3 = i['qkv'].reshape(B, L, 3, C).permute(2, 0, 1, 3).clone().requires_grad_(True)
    ws = [w.reshape(cb, 1, 3, 3).clone().requires_grad_(True) for w in i['lepe_w']]
    bs = [b.clone().requires_grad_(True) for b in i['lepe_b']]
    outs = []
    for br, (hs, wd) in enumerate(case[4]):
        sl = slice(br * cb, (br + 1) * cb)
        q, k, v = (q3[j][:, :, sl] for j in range(3))
        if (hs, wd) == (reso, reso):
            idx, split = -1, reso
        elif hs == reso:
            idx, split = 0, wd
        elif wd == reso:
            idx, split = 1, hs
        else:
            return None                                    # a stripe shape LePEAttention cannot express (neither side = reso)
        outs.append(O.lepe_attention(q, k, v, ws[br], bs[br], reso, idx, split, hpb))
    out = torch.cat(outs, 2).reshape(B * L, C)
    out.backward(i['dout'])
    return dict(out=out.detach(), dqkv=q3.grad.permute(1, 2, 0, 3).reshape(B * L, 3 * C),
                dw=torch.stack([w.grad.reshape(cb, 9) for w in ws]), db=torch.stack([b.grad for b in bs]))


@pytest.mark.parametrize('case,kind', CASES, ids=_id)
def test_closed_forms_match_the_oracle_in_float64(case, kind):
    ref = R.reference(case, BF, kind)
    want = _oracle(ref['inputs'])
    assert want is not None
    for n, w in want.items():
        x = ref['exact'][n]
        assert x.shape == w.shape, n
        if n == 'dqkv' and R.n_tokens(case) == 1:           # dq = dk = 0 identically
            C = case[2]
            assert float(x[:, :2 * C].abs().max()) <= 1e-10 * ref['zero_scale']
            assert float(w[:, :2 * C].abs().max()) <= 1e-10 * ref['zero_scale']
            x, w = x[:, 2 * C:], w[:, 2 * C:]
        assert _rel(x, w) <= 1e-10, (n, _rel(x, w))


def test_wgrad_only_case_matches_the_oracle_on_a_small_shape():
    """the only_wgrad path (q = k = 0) used for R.WGRAD_TRIP gives the dw / db of the full evaluation"""
    case = R.two(8, 8, 4, B=2)
    i = R.make_inputs(case, BF, 'plain', only_wgrad=True)
    a, b = R.evaluate(i, only_wgrad=True), _oracle(i)
    assert set(a) == {'dw', 'db'}
    assert _rel(a['dw'], b['dw']) <= 1e-10 and _rel(a['db'], b['db']) <= 1e-10


@pytest.mark.parametrize('name', ['lepe_v', 'lepe_h', 'lepe_full', 'lepe_s1', 'lepe_s2h'])
def test_closed_forms_reproduce_the_real_module(name):
    """inputs as test_stripe_attention_vs_reference_vectors (tests/test_cswin_kernels_gpu.py) seeds them; its fp32 tolerances"""
    z = np.load(os.path.join(GOLDEN, 'cswin_modules.npz'))
    reso, idx, split, dim, heads = [int(v) for v in z[f'{name}.cfg']]
    qkv = torch.randn(3, 2, reso * reso, dim, generator=torch.Generator().manual_seed(4321 + len(name)))
    gy = torch.randn(2, reso * reso, dim, generator=torch.Generator().manual_seed(4321 + 100 + len(name)))
    B, L = 2, reso * reso
    stripe = (reso, reso) if idx == -1 else ((reso, split) if idx == 0 else (split, reso))
    i = dict(case=(B, reso, dim, heads, (stripe,)), scale=(dim // heads) ** -0.5,
             qkv=qkv.permute(1, 2, 0, 3).reshape(B * L, 3 * dim).to(F64), dout=gy.reshape(B * L, dim).to(F64),
             lepe_w=[torch.from_numpy(z[f'{name}.w']).reshape(dim, 9).to(F64)], lepe_b=[torch.from_numpy(z[f'{name}.b']).to(F64)])
    ex = R.evaluate(i)
    want = dict(out=torch.from_numpy(z[f'{name}.y']).reshape(B * L, dim),
                dqkv=torch.from_numpy(z[f'{name}.dqkv']).permute(1, 2, 0, 3).reshape(B * L, 3 * dim),
                dw=torch.from_numpy(z[f'{name}.dw']).reshape(1, dim, 9), db=torch.from_numpy(z[f'{name}.db']).reshape(1, dim))
    for n, tol in (('out', 2e-4), ('dqkv', 3e-4), ('dw', 3e-4), ('db', 3e-4)):
        assert _rel(ex[n], want[n].to(F64)) <= tol, (n, _rel(ex[n], want[n].to(F64)))


def _stored(i, dt, mfma):
    """the formulas in float32, reversed summation order, each result rounded to the type the kernels store it in"""
    r = R.evaluate(i, F32, mfma=mfma, flip=True)
    return dict(out=R.rnd(r['out'].to(F64), dt), dqkv=R.rnd(r['dqkv'].to(F64), dt), dw=r['dw'].to(F64), db=r['db'].to(F64))


@pytest.mark.parametrize('dt', [BF, F32], ids=_id)
@pytest.mark.parametrize('case,kind', CASES, ids=_id)
def test_fp32_evaluation_passes_the_generic_gate(case, kind, dt):
    ref = R.reference(case, dt, kind)
    ratios = R.gate_all(_stored(ref['inputs'], dt, False), ref, 'generic')
    print(f'{_id(case)} {kind} {_id(dt)}: ' + ' '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    assert set(ratios) == {'out', 'dq', 'dk', 'dv', 'dw', 'db'}
    assert all(v <= 1.0 for v in ratios.values()), ratios


MFMA_CASES = [c for c in CASES if R.form(c[0], BF) == 'mfma']


@pytest.mark.parametrize('case,kind', MFMA_CASES, ids=_id)
def test_bf16_rounded_evaluation_passes_the_mfma_gate(case, kind):
    ref = R.reference(case, BF, kind)
    ratios = R.gate_all(_stored(ref['inputs'], BF, True), ref, 'mfma')
    print(f'{_id(case)} {kind} mfma: ' + ' '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_the_mfma_roundings_do_not_all_fit_the_generic_gate():
    """the MFMA gate is wider for a reason: the emulation with the documented roundings exceeds the generic gate somewhere"""
    worst = 0.0
    for case in R.KIND_SHAPES[:3]:
        ref = R.reference(case, BF, 'plain')
        worst = max(worst, max(R.gate_all(_stored(ref['inputs'], BF, True), ref, 'generic').values()))
    assert worst > 1.0, worst


def test_form_and_lds_restatements():
    assert R.form(R.two(28, 28, 4), BF) == 'mfma' and R.form(R.col(113), BF) == 'generic' and R.form(R.col(65), F32) == 'generic'
    assert R.form(R.col(65), BF, knob=0) == 'generic' and R.form(R.col(17, 32), BF) == 'generic'
    # the arithmetic of the two-plane generic backward against 160 KiB: head_dim 32 fits up to N = 109, head_dim 16 up to 126
    assert R.bwd_lds(R.col(109), F32) == (4 * (4 * 128 * 33 + 2 * 109 * 110), False) and R.bwd_lds(R.col(109), F32)[0] <= R.LDS_LIMIT
    assert 4 * (4 * 128 * 33 + 2 * 110 * 111) > R.LDS_LIMIT and R.bwd_lds(R.col(110), F32)[1]
    assert 4 * (4 * 128 * 33 + 2 * 128 * 129) == 199680
    assert not R.bwd_lds(R.two(42, 42, 3, 32), F32)[1] and R.bwd_lds(R.col(127, 32), F32)[1] and R.bwd_lds(R.two(16, 16, 8, 32), BF)[1]
    assert not R.bwd_lds(R.two(16, 16, 8, 16), F32)[1]                                # head_dim 8 fits two planes at 128
    assert R.bwd_lds(R.col(113), BF)[1] and not R.bwd_lds(R.two(28, 28, 4), BF)[1]
    for case, _ in CASES:
        for dt in (BF, F32):
            for knob in (0, 1):
                assert R.bwd_lds(case, dt, knob)[0] <= R.LDS_LIMIT
    assert [R.n_items(c) for c in R.ITEMS] == [9, 10, 11, 12, 13, 14, 15, 20]
    assert sorted({R.n_tokens(c) for c in R.N_HD32}) == [1, 2, 15, 16, 17, 48, 49, 63, 64, 65, 72, 81, 97, 109, 110, 112, 113, 121, 128]


def test_inputs_are_representable_and_of_the_stated_kind():
    case = R.col(17)
    C = case[2]
    peak = {}
    for kind in R.KINDS:
        for dt in (BF, F32):
            i = R.make_inputs(case, dt, kind)
            assert torch.equal(i['qkv'], R.rnd(i['qkv'], dt)) and torch.equal(i['dout'], R.rnd(i['dout'], dt))
            assert all(torch.equal(w, R.rnd(w, F32)) for w in i['lepe_w'] + i['lepe_b'])
            assert all(float(b.abs().min()) >= 0.5 * (1 - 1e-6) for b in i['lepe_b'])
        if kind == 'negative':
            assert float(i['qkv'][:, :C].min()) >= 1.0 and float(i['qkv'][:, C:2 * C].max()) <= -1.0
        ex = R.evaluate(i)
        q = R._win(i['qkv'][:, :32], 1, 17, 17, 1, 1)
        k = R._win(i['qkv'][:, C:C + 32], 1, 17, 17, 1, 1)
        S = (q * i['scale']) @ k.transpose(-1, -2)
        peak[kind] = float(torch.softmax(S, -1).max(-1).values.mean())
        if kind == 'negative':
            assert float(S.max()) < -5.0
    assert peak['plain'] < 0.5 and peak['sharp'] > 0.85, peak
    again = R.make_inputs(case, F32, 'negative')
    assert torch.equal(again['qkv'], i['qkv']) and torch.equal(again['lepe_w'][1], i['lepe_w'][1])         # seeded


def test_gate_arithmetic():
    ref = torch.tensor([1.0, -0.5, 0.0, 1e-3], dtype=F64)
    assert R.gate(ref.clone(), ref, BF) == 0.0
    d = torch.tensor([0.0, 0.0, 1e-4, 0.0], dtype=F64)                 # floor alone: 2e-4 * max|ref| = 2e-4
    assert abs(R.gate(ref + d, ref, F32) - 0.5) < 1e-12 and abs(R.gate(ref + d, ref, BF) - 0.5) < 1e-12
    d = torch.tensor([2.0 ** -8 + 2e-4, 0.0, 0.0, 0.0], dtype=F64)     # bf16: exactly at the limit of the largest element
    assert abs(R.gate(ref + d, ref, BF) - 1.0) < 1e-9 and R.gate(ref + d, ref, F32) > 20
    a = torch.tensor([2.0, 0.0, 0.0, 0.0], dtype=F64)                  # an absolute sum of 2 admits another 2^-7
    assert abs(R.gate(ref + d, ref, BF, a) - (2.0 ** -8 + 2e-4) / (3 * 2.0 ** -8 + 2e-4)) < 1e-9
    bad = ref.clone()
    bad[1] = float('nan')
    assert R.gate(bad, ref, BF) == float('inf')
    z = torch.zeros(3, dtype=F64)
    assert R.gate(z.clone(), z, BF) == 0.0 and R.gate(z + 1e-30, z, BF) == float('inf')
    assert abs(R.gate(z + 1e-4, z, F32, zs=1.0) - 0.5) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the gate is sharp.  A wrong restatement applies to a case if the defect can show there at all; it must then fail the gate of
# every form and dtype on at least one applicable case of every input kind (the cases of R.KIND_SHAPES carry all three kinds;
# the remaining cases are plain).
# ---------------------------------------------------------------------------------------------------------------------
def _applies(wrong, case):
    B, reso, C, heads, stripes = case
    nwin = (reso // stripes[0][0]) * (reso // stripes[0][1])
    if wrong == 'pad_unmasked':
        return any((h * w) % 16 for h, w in stripes)
    if wrong == 'lepe_across_border':
        return nwin > 1
    if wrong in ('dv_not_flipped', 'tap_swapped'):
        return R.n_tokens(case) > 1
    if wrong in ('branch1_shape0', 'lepe_row_global'):
        return len(stripes) == 2 and (wrong == 'lepe_row_global' or stripes[0] != stripes[1])
    if wrong in ('dk_scale_twice', 'dk_scale_none'):
        return R.n_tokens(case) > 1
    if wrong == 'db_per_window':
        return B * nwin > 1
    return True


SHARP_CASES = [(c, k) for c, k in CASES if c in R.KIND_SHAPES] + [(R.two(10, 10, 2), 'plain'), (R.two(8, 8, 4, 128, 4), 'plain')]
GATES = [('generic', F32), ('generic', BF), ('mfma', BF)]


@pytest.mark.parametrize('wrong', R.WRONG)
def test_wrong_restatement_is_rejected(wrong):
    hit = {}
    for case, kind in SHARP_CASES:
        if not _applies(wrong, case):
            continue
        for frm, dt in GATES:
            if frm == 'mfma' and R.form(case, BF) != 'mfma':
                continue
            ref = R.reference(case, dt, kind)
            r = R.evaluate(ref['inputs'], wrong=wrong)
            got = dict(out=R.rnd(r['out'], dt), dqkv=R.rnd(r['dqkv'], dt), dw=r['dw'], db=r['db'])
            worst = max(R.gate_all(got, ref, frm).values())
            key = (frm, _id(dt), kind)
            hit[key] = max(hit.get(key, 0.0), worst)
    print(wrong, {k: round(v, 2) for k, v in hit.items()})
    assert len(hit) == len(GATES) * len(R.KINDS), sorted(hit)
    assert all(v > 1.0 for v in hit.values()), {k: v for k, v in hit.items() if not v > 1.0}


@pytest.mark.parametrize('wrong', R.WRONG)
def test_wrong_restatement_is_the_right_form_where_it_cannot_show(wrong):
    """each flag changes nothing on a case it does not apply to: the rejection above is the defect's, not a side effect's"""
    for case in (R.one(4, B=1), R.one(1, B=1)):
        if _applies(wrong, case):
            continue
        i = R.reference(case, BF)['inputs']
        a, b = R.evaluate(i), R.evaluate(i, wrong=wrong)
        assert all(torch.equal(a[n], b[n]) for n in ('out', 'dqkv', 'dw', 'db')), wrong
