"""tests/_class_attn_ref.py checked without a GPU, for every case that tests/test_class_attn_mt_edges_gpu.py gates:
  * the four closed forms equal float64 torch.autograd of the literal formula (restated here with matmul and
    nn.functional.linear, not with the reference's einsums) within 1e-10 relative;
  * the gate is reachable: a float32 torch evaluation of the same formulas (another summation order than the kernels'),
    rounded to the storage type where the kernels store it, passes gate() on every case, kind and dtype;
  * the gate is sharp: nine deliberately wrong restatements are each rejected, on the tensors they must corrupt and on
    no tensor they cannot reach."""
import math

import pytest
import torch
import torch.nn.functional as Fn

import _class_attn_ref as R

F64, F32, BF = R.F64, R.F32, R.BF
CASES = [('plain',) + c for c in R.plain_gated()] + [('ia',) + c for c in R.ia_gated()]


def _id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v).replace('torch.', '')


def _literal(family, i, q, kvc, kvt, W1, b1, W2, b2):
    """out, P from leaves that autograd can differentiate: map.py's ClassAttention written down as it reads"""
    B, T, Nt, heads, hd = i['case']
    E, N = heads * hd, T + Nt
    kv = torch.cat([kvc, kvt], 1)
    qh = q.reshape(B, T, heads, hd).permute(0, 2, 1, 3)
    kh = kv[..., :E].reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    vh = kv[..., E:].reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    S = (qh @ kh.transpose(-1, -2) * i['scale']).permute(0, 2, 3, 1)            # [B][T][N][heads]
    if family == 'ia':
        S = S + Fn.linear(S, W1, b1)
    A = torch.softmax(S, dim=2)
    Pm = A + Fn.linear(A, W2, b2) if family == 'ia' else A
    D = Pm if i['mask'] is None else Pm * i['mask'].permute(0, 1, 3, 2)
    out = (D.permute(0, 3, 1, 2) @ vh).transpose(1, 2).reshape(B, T, E)
    return out, A.permute(0, 1, 3, 2)


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize('family,case,kind', CASES, ids=_id)
def test_closed_forms_match_autograd(family, case, kind):
    ref = R.reference(family, case, BF, kind)
    i, ex = ref['inputs'], ref['exact']
    names = ('q', 'kv_cls', 'kv_tok', 'W1', 'b1', 'W2', 'b2')
    leaves = [i[n].clone().requires_grad_(True) for n in names]
    out, P = _literal(family, i, *leaves)
    out.backward(i['dout'])
    want = dict(out=out.detach(), P=P.detach(), dq=leaves[0].grad, dkv_cls=leaves[1].grad, dkv_tok=leaves[2].grad)
    if family == 'ia':
        want.update(dW1=leaves[3].grad, db1=leaves[4].grad, dW2=leaves[5].grad, db2=leaves[6].grad)
    assert set(want) == set(ex)
    for n, w in want.items():
        assert ex[n].shape == w.shape, n
        if n == 'db1':         # identically zero (R.gate): both sides are float64 residue of the same cancellation
            zs = R.zero_scale(family, i, n)
            assert float(ex[n].abs().max()) <= 1e-10 * zs and float(w.abs().max()) <= 1e-10 * zs
            continue
        assert _rel(ex[n], w) <= 1e-10, (n, _rel(ex[n], w))


def _stored(family, i, dt, dtype=F32):
    """the formulas evaluated in `dtype`, each result rounded to the type the kernels store it in"""
    return {n: R.rnd(x.to(F64), R.stored_dtype(n, dt)) for n, x in R.evaluate(family, i, dtype).items()}


@pytest.mark.parametrize('dt', [BF, F32], ids=_id)
@pytest.mark.parametrize('family,case,kind', CASES, ids=_id)
def test_fp32_evaluation_passes_the_gate(family, case, kind, dt):
    ref = R.reference(family, case, dt, kind)
    got = _stored(family, ref['inputs'], dt)
    ratios = R.gate_all(got, ref)
    rs = R.row_sum_err(got['P'])
    print(f'{family} {case} {kind} {_id(dt)}: ' + ' '.join(f'{n} {v:.3f}' for n, v in ratios.items()) + f'  rowsum {rs:.1e}')
    assert set(ratios) == set(R.PLAIN_OUT if family == 'plain' else R.IA_OUT)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert rs <= R.ROW_SUM_TOL


def test_inputs_are_representable_and_of_the_stated_kind():
    case = (2, 5, 49, 12, 32)
    peak = {}
    for kind in R.KINDS:
        for dt in (BF, F32):
            i = R.make_inputs(case, dt, kind)
            for n in ('q', 'kv_cls', 'kv_tok', 'dout'):
                assert torch.equal(i[n], R.rnd(i[n], dt)), n
            for n in ('W1', 'b1', 'W2', 'b2'):
                assert torch.equal(i[n], R.rnd(i[n], F32)) and i[n].shape == ((12, 12) if n[0] == 'W' else (12,))
            assert float(i['b2'].abs().min()) >= 0.3 / math.sqrt(12) * (1 - 1e-6)
        peak[kind] = float(R.plain_fwd(i)[1].max(-1).values.mean())
        if kind == 'masked':
            m = i['mask']
            assert set(m.unique().tolist()) == {0.0, 2.0} and 0.4 < float((m > 0).double().mean()) < 0.6
            assert float(m[0, 0, 0].abs().max()) == 0.0 and float(m[-1, -1, -1].abs().max()) == 0.0
        else:
            assert i['mask'] is None
    assert peak['plain'] < 0.2 and peak['sharp'] > 0.85, peak
    again = R.make_inputs(case, F32, 'masked')
    assert all(torch.equal(again[n], i[n]) for n in ('q', 'kv_tok', 'mask', 'W2'))           # seeded


def test_gate_arithmetic():
    ref = torch.tensor([1.0, -0.5, 0.0, 1e-3], dtype=F64)
    assert R.gate(ref.clone(), ref, BF) == 0.0
    d = torch.tensor([0.0, 0.0, 1e-4, 0.0], dtype=F64)                 # floor alone: 2e-4 * max|ref| = 2e-4
    assert abs(R.gate(ref + d, ref, F32) - 0.5) < 1e-12 and abs(R.gate(ref + d, ref, BF) - 0.5) < 1e-12
    d = torch.tensor([2.0 ** -8 + 2e-4, 0.0, 0.0, 0.0], dtype=F64)     # bf16: exactly at the limit of the largest element
    assert abs(R.gate(ref + d, ref, BF) - 1.0) < 1e-9 and R.gate(ref + d, ref, F32) > 20
    bad = ref.clone()
    bad[1] = float('nan')
    assert R.gate(bad, ref, BF) == math.inf
    z = torch.zeros(3, dtype=F64)
    assert R.gate(z.clone(), z, BF) == 0.0 and R.gate(z + 1e-30, z, BF) == math.inf
    assert abs(R.gate(z + 1e-4, z, F32, zero_scale=1.0) - 0.5) < 1e-12
    assert abs(R.gate(z + 1e-4, z + 1e-17, F32, zero_scale=1.0) - 0.5) < 1e-9      # float64 residue counts as zero
    assert R.row_sum_err(torch.tensor([[0.25, 0.75], [0.5, 0.5 + 3e-5]], dtype=F64)) > R.ROW_SUM_TOL


def test_fully_masked_single_query_is_exactly_zero():
    """T = 1, B = heads = 1 and the only row masked: every gradient and out are identically zero, no cancellation is
    involved (dA = dD * 0), so zero_scale is 0 and the gate demands exact zeros"""
    i = R.make_inputs((1, 1, 7, 1, 8), BF, 'masked')
    assert float(i['mask'].abs().max()) == 0.0
    for family in ('plain', 'ia'):
        ex = R.evaluate(family, i)
        for n in ('out', 'dq', 'dkv_cls', 'dkv_tok'):
            assert float(ex[n].abs().max()) == 0.0 and R.zero_scale(family, i, n) == 0.0
            assert R.gate(ex[n].clone(), ex[n], BF) == 0.0 and R.gate(ex[n] + 1e-20, ex[n], BF) == math.inf


def test_lds_tables():
    """the largest key counts the 160 KiB bound admits at heads = 64, hd = 8, T = 8 (plain) and T = 8, heads = 12
    (interactive backward), from the restated formulas"""
    assert R.mt_lds(8, 56, 64, 8, False) == 4 * (56 * 64 + 8 * 64 * 56 + 16 * 512) == 161792 <= R.LDS_LIMIT < R.mt_lds(8, 57, 64, 8, False)
    assert R.mt_lds(8, 30, 64, 8, True) == 163328 <= R.LDS_LIMIT < R.mt_lds(8, 31, 64, 8, True)
    assert R.PLAIN_LDS_N == {False: 56, True: 30}
    assert R.ia_lds(8, 170, 12, True) == 163200 <= R.LDS_LIMIT < R.ia_lds(8, 171, 12, True) and R.IA_LDS_N == 170


# ---------------------------------------------------------------------------------------------------------------------
# the gate is sharp
# ---------------------------------------------------------------------------------------------------------------------
def _restated(family, i, wrong=None):
    """R.evaluate restated step by step in float64, with one deliberate mistake switched on by `wrong`"""
    B, T, Nt, heads, hd = i['case']
    q, k, v, S = R._scores(i, F64)
    g = i['dout'].reshape(B, T, heads, hd)
    mask = (lambda X: R._apply_mask(X, i))
    dD = torch.einsum('bthd,bnhd->bthn', g, v)
    if family == 'plain':
        A = torch.softmax(S, -1)
        D = mask(A)
        if wrong == 'mask after softmax backward':
            dS = mask(R._softmax_bwd(A, dD))
        else:
            dS = R._softmax_bwd(A, mask(dD))
        dq, dkc, dkt = R._dqkv(dS, A if wrong == 'no mask on dv weights' else D, q, k, g, i)
        if wrong == 'no scale on dk':
            E = heads * hd
            dkc, dkt = dkc.clone(), dkt.clone()
            dkc[..., :E] /= i['scale']
            dkt[..., :E] /= i['scale']
        return dict(zip(R.PLAIN_OUT, (R._out(D, v, i), A, dq, dkc, dkt)))
    W1, b1, W2, b2 = (i[n] for n in ('W1', 'b1', 'W2', 'b2'))
    A = torch.softmax(S + R._mix(W1, S) + b1[:, None], -1)
    Pm = A + R._mix(W2, A) + (0.0 if wrong == 'b2 omitted from D' else b2[:, None])
    D = mask(Pm)
    dPm = mask(dD)
    dW2 = torch.einsum('bthn,btgn->hg', dPm, A)
    db2 = (dD if wrong == 'db2 from unmasked dD' else dPm).sum((0, 1, 3))
    dU = R._softmax_bwd(A, dPm + R._mix(W2 if wrong == 'W2 untransposed in dA' else W2.t(), dPm))
    dW1 = torch.einsum('bthn,btgn->hg', dU, A if wrong == 'dW1 against A' else S)
    db1 = dU.sum((0, 1, 3))
    dS = dU + R._mix(W1 if wrong == 'W1 untransposed in dS' else W1.t(), dU)
    P = Pm if wrong == 'P saved as Pm' else A
    return dict(zip(R.IA_OUT, (R._out(D, v, i), P) + R._dqkv(dS, D, q, k, g, i) + (dW1, db1, dW2, db2)))


# (family, wrong restatement, tabled (case, kind), tensors that must trip, tensors the mistake cannot reach)
WRONG = [
    ('plain', 'no mask on dv weights', ((2, 5, 49, 4, 16), 'masked'), {'dkv_cls', 'dkv_tok'}, {'out', 'P', 'dq'}),
    ('plain', 'mask after softmax backward', ((2, 5, 49, 4, 16), 'masked'), {'dq', 'dkv_cls', 'dkv_tok'}, {'out', 'P'}),
    ('plain', 'no scale on dk', ((2, 5, 49, 4, 16), 'plain'), {'dkv_cls', 'dkv_tok'}, {'out', 'P', 'dq'}),
    ('ia', 'W2 untransposed in dA', ((2, 5, 49, 12, 32), 'plain'), {'dq', 'dkv_cls', 'dkv_tok', 'dW1'}, {'out', 'P', 'dW2', 'db2'}),
    ('ia', 'W1 untransposed in dS', ((2, 5, 49, 12, 32), 'plain'), {'dq', 'dkv_cls', 'dkv_tok'}, {'out', 'P', 'dW1', 'db1', 'dW2', 'db2'}),
    ('ia', 'b2 omitted from D', ((2, 5, 49, 12, 32), 'masked'), {'out', 'dkv_cls', 'dkv_tok'}, {'P', 'dq', 'dW1', 'db1', 'dW2', 'db2'}),
    ('ia', 'db2 from unmasked dD', ((2, 5, 49, 12, 32), 'masked'), {'db2'}, set(R.IA_OUT) - {'db2'}),
    ('ia', 'dW1 against A', ((2, 5, 49, 12, 32), 'plain'), {'dW1'}, set(R.IA_OUT) - {'dW1'}),
    ('ia', 'P saved as Pm', ((2, 5, 49, 12, 32), 'plain'), {'P'}, set(R.IA_OUT) - {'P'}),
]


@pytest.mark.parametrize('family', ['plain', 'ia'])
def test_restatement_is_faithful(family):
    for fam, case, kind in CASES:
        if fam == family and kind == 'masked':
            ref = R.reference(family, case, BF, kind)
            got = _restated(family, ref['inputs'])
            assert all(torch.equal(got[n], x) for n, x in ref['exact'].items())


@pytest.mark.parametrize('family,wrong,where,trips,clean', WRONG, ids=[w[1].replace(' ', '_') for w in WRONG])
def test_wrong_restatement_is_rejected(family, wrong, where, trips, clean):
    """judged by the WIDER of the two gates (bf16 storage, results rounded to bf16): what fails it fails the fp32 one too"""
    case, kind = where
    assert (case, kind) in (R.plain_gated() if family == 'plain' else R.ia_gated())
    ref = R.reference(family, case, BF, kind)
    got = {n: R.rnd(x, R.stored_dtype(n, BF)) for n, x in _restated(family, ref['inputs'], wrong).items()}
    ratios = R.gate_all(got, ref)
    print(f'{wrong}: ' + ' '.join(f'{n} {v:.2f}' for n, v in ratios.items()))
    tripped = {n for n, v in ratios.items() if v > 1.0}
    assert trips <= tripped, (wrong, 'not rejected on', trips - tripped, ratios)
    assert not (clean & tripped), (wrong, 'rejected on a tensor it cannot reach', clean & tripped)
    assert trips | clean | {'db1'} >= set(ratios)
