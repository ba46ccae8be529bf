"""The few-row forms' eligibility (csrc/gemm_select.h: nt_fewrows_wanted / tn_fewrows_wanted) over the model descriptors of
tests/golden/gemm_forms.json, through ga_gemm_fewrows_form / ga_wgrad_fewrows_form.  Needs no GPU: the selection assumes 256 CUs."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_M = 512           # gemm_select.h: the default of FEWROWS_MAXM
HALF_CUS = 128


def _tool():
    spec = importlib.util.spec_from_file_location('gemm_forms_tool', os.path.join(ROOT, 'tools', 'gemm_forms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _models(T):
    return [c for c in json.load(open(T.GOLDEN)) if not c['src'].startswith('test_')]


def _few(T, c):
    return T.FEWROWS[c['fn']](T.unpack(c['fn'], c['desc']))


def _cdiv(a, b):
    return -(-a // b)


def _expected(c):
    """the rule restated: bf16, plain layouts, M <= 512, the register-staged / 128 x 128 body with fewer tiles x batch than half the CUs"""
    d, form = c['desc'], c['form'][0]
    if d['dtype'] != 1 or d['M'] > MAX_M:
        return False
    if c['fn'] == 'ga_wgrad':
        if form != 'tn' or d.get('x_kind') or d.get('x_act') or (not d.get('accumulate') and d.get('split_m', 1) > 1):
            return False
        return _cdiv(d['N'], 128) * _cdiv(d['K'], 128) * d['split_m'] * d['batch'] < HALF_CUS
    if not form.startswith('staged') or '+gather' in form or d.get('a_kind') or d.get('c_kind') or d.get('a_act') or d.get('relu_after'):
        return False
    if d.get('act') and not form.endswith(':fc1'):
        return False
    if (not d.get('act') and d.get('C2')) or (d.get('H') and not d.get('h_is_deriv')):
        return False
    width = int(form[6:form.index(':')])
    return _cdiv(d['M'], 128) * _cdiv(d['N'], width) * d['batch'] < HALF_CUS


# the flagship's few-row launches (ga_convnext_tiny_768 at batch 256): (fn, M, N, K, batch) -> few-row form
FLAGSHIP = {
    ('ga_gemm', 256, 96, 2320, 8): 'fewrows32x32:plain',         # gram_embedding conv (+ column sums)
    ('ga_gemm', 256, 384, 768, 1): 'fewrows32x32:plain',         # kvc
    ('ga_gemm', 256, 192, 768, 1): 'fewrows32x32:plain',         # q (forward and a data gradient)
    ('ga_gemm', 256, 768, 192, 1): 'fewrows32x32:fc2',           # proj
    ('ga_gemm', 256, 192, 192, 16): 'fewrows32x32:fc1',          # mlp.fc1
    ('ga_gemm', 256, 192, 768, 4): 'fewrows32x32:fc2',           # mlp.fc2
    ('ga_gemm', 256, 1000, 768, 5): 'fewrows32x32:generic',      # fc.all (fp32 logits)
    ('ga_gemm', 256, 768, 1000, 5): 'fewrows32x32:plain',        # fc.all.dg
    ('ga_gemm', 256, 768, 192, 4): 'fewrows32x32:dg2',           # mlp.fc2.dg
    ('ga_gemm', 256, 192, 192, 4): {'fewrows32x32:plain', 'fewrows32x32:fc2'},      # mlp.fc1.dg0..3
    ('ga_gemm', 256, 768, 384, 1): 'fewrows32x32:plain',         # kvc.dg
    ('ga_wgrad', 256, 192, 768, 4): 'fewrows_tn64x64',           # mlp.fc2.wg
    ('ga_wgrad', 256, 192, 192, 16): 'fewrows_tn64x64',          # mlp.fc1.wg
    ('ga_wgrad', 256, 768, 192, 1): 'fewrows_tn64x64',           # proj.wg
    ('ga_wgrad', 256, 384, 768, 1): 'fewrows_tn64x64',           # kvc.wg
    ('ga_wgrad', 256, 192, 768, 1): 'fewrows_tn64x64',           # q.wg
    # where they are: the 128 x 128 form already spreads them over more than half the chip
    ('ga_wgrad', 256, 1000, 768, 5): 'none',                     # fc.all.wg: 240 tiles
    ('ga_wgrad', 256, 96, 2316, 8): 'none',                      # gram_embedding.wg: 152 tiles
    ('ga_gemm', 256, 2316, 96, 8): 'none',                       # gram_embedding.dg: 592 tiles
    ('ga_wgrad', 196, 192, 192, 256): 'none',                    # the per-sample Gram products
}


def test_fewrows_forms_over_the_model_corpus():
    T = _tool()
    T.prime()
    models = _models(T)
    named = 0
    for c in models:
        few = _few(T, c)
        assert (few != 'none') == _expected(c), (c, few)
        d = c['desc']
        if d['M'] > MAX_M or d['dtype'] != 1 or d.get('a_kind') or d.get('x_kind'):
            assert few == 'none', (c, few)
        named += few != 'none'
    assert named >= 60, named       # the heads of every family, not the flagship's alone


def test_fewrows_forms_of_the_flagship_and_its_pinned_forms():
    T = _tool()
    T.prime()
    seen = set()
    for c in _models(T):
        d = c['desc']
        key = (c['fn'], d['M'], d['N'], d['K'], d['batch'])
        if c['src'] != 'ga_convnext_tiny_768' or key not in FLAGSHIP:
            continue
        seen.add(key)
        want = FLAGSHIP[key]
        assert _few(T, c) in (want if isinstance(want, set) else {want}), (key, _few(T, c))
        assert T.answer(c) == c['form'], (key, T.answer(c), c['form'])      # ga_gemm_form / ga_wgrad_form: what the fixture records
    assert seen == set(FLAGSHIP), set(FLAGSHIP) - seen


def test_fewrows_knob_turns_the_forms_off():
    from imagenet_models_amd import _lib as L
    T = _tool()
    T.prime()
    few = [c for c in _models(T) if c['src'] == 'ga_convnext_tiny_768' and _few(T, c) != 'none']
    assert few
    with L.knobs(FEWROWS=0):
        assert all(_few(T, c) == 'none' for c in few)
        assert ' FEWROWS=0' in L.config_string()
    assert all(_few(T, c) != 'none' for c in few)
    assert 'FEWROWS' not in L.config_string()
