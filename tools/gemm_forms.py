#!/usr/bin/env python3
"""descriptor -> kernel form of ga_gemm / ga_wgrad (include/gaext.h: ga_gemm_form, ga_wgrad_form) over a corpus of descriptors.

    python tools/gemm_forms.py                  # print the corpus with the form each descriptor gets        (no GPU needed)
    python tools/gemm_forms.py --check          # compare against tests/golden/gemm_forms.json, exit 1 on a difference
    python tools/gemm_forms.py --write [--models FILE]   # record corpus and answers in that file (FILE: a new --dump-models)
    python tools/gemm_forms.py --coverage       # the forced-form GPU tests: how many launches reach the form the test names, and
                                                # tests/test_gemm_forms_edges_gpu.py: launches that reach a form of the named family
    python tools/gemm_forms.py --dump-models    # GPU machine: rebuild the model part of the corpus (plans only, no kernel runs)

The corpus is (a) the descriptors of the forced-form GPU tests under their knob settings, restated here call by call (those of
tests/test_gemm_forms_edges_gpu.py come from the case table it shares with this tool, tests/_gemm_ref.py), and (b) every
distinct ga_gemm / ga_wgrad descriptor of the engines of tools/plan_fingerprint.py's NAMED models (bf16 training step at the bench
batch, default knobs).  Pointers are reduced to null-or-not plus their low 4 bits.  The answers are this library's own; on a
machine without a GPU the selection assumes 256 compute units, the MI355X's count.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from imagenet_models_amd import _lib as L, ops  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'gemm_forms.json')
BENCH_BATCH = 256
FN = {'ga_gemm': (L.GemmDesc, ops.gemm_form), 'ga_wgrad': (L.WgradDesc, ops.wgrad_form)}
# the few-row entry points take the same descriptors (ops.Plan records them where their _form query names a form): the corpus keeps
# such a call under the name of the product, and the listing shows the few-row form beside the pinned one
FEWROWS = {'ga_gemm': ops.gemm_fewrows_form, 'ga_wgrad': ops.wgrad_fewrows_form}
BASE = {'ga_gemm_fewrows': 'ga_gemm', 'ga_wgrad_fewrows': 'ga_wgrad'}


def pack(d):
    """descriptor -> its non-zero fields; a pointer becomes 0x1000 + its low 4 bits"""
    out = {}
    for name, typ in d._fields_:
        v = getattr(d, name)
        if typ in (C.c_void_p, C.c_char_p) or (isinstance(typ, type) and issubclass(typ, C._Pointer)):
            v = C.cast(v, C.c_void_p).value
            v = 0x1000 + (v & 15) if v else 0
        if v:
            out[name] = v
    return out


def unpack(fn, fields):
    d = FN[fn][0]()
    for name, typ in d._fields_:
        if name in fields:
            v = fields[name]
            setattr(d, name, C.cast(C.c_void_p(v), typ) if isinstance(typ, type) and issubclass(typ, C._Pointer) else v)
    return d


def answer(case):
    """the form (and, for ga_wgrad, the workspace bytes) the library names for one corpus case, or the error it raises"""
    d = unpack(case['fn'], case['desc'])
    with L.knobs(**case.get('knobs', {})):
        try:
            form = FN[case['fn']][1](d)
        except RuntimeError as e:
            form = 'error: ' + str(e).split('): ', 1)[-1]
        return [form, int(L.load().ga_wgrad_workspace(C.byref(d)))] if case['fn'] == 'ga_wgrad' else [form]


def prime():
    """the first selection enters every knob it reads in the library's table; setting and unsetting a knob the table does not know
    yet uses up a slot each time"""
    L.load().ga_wgrad_workspace(C.byref(L.WgradDesc(M=1, N=1, K=1, batch=1)))


class Recorder(ops.Plan):
    """an ops.Plan that records descriptors for operands that do not exist: every operand is `OP`, a 16-byte aligned address;
    a weight gradient gets the workspace it asks for, as Plan.finalize() would give it"""

    def __init__(self, src, knobs, cases):
        super().__init__()
        self.src, self.kn, self.cases = src, knobs, cases

    def record(self, fname, d, label=None):
        self.cases.append(dict(src=self.src, knobs=self.kn, fn=BASE.get(fname, fname), desc=pack(d)))

    def _want_workspace(self, nbytes, patch):
        patch(0x1000, nbytes)


OP = object()
EDGES = 'test_gemm_form_at_its_edges'


def edge_table():
    """tests/_gemm_ref.py: the case table of tests/test_gemm_forms_edges_gpu.py"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('_gemm_ref', os.path.join(ROOT, 'tests', '_gemm_ref.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cases():
    """part (a): the ga_gemm / ga_wgrad calls of the forced-form GPU tests, in the tests' order"""
    cases = []
    bf = L.GA_BF16
    real_ptr, real_cus = ops._ptr, ops._NUM_CU
    ops._ptr, ops._NUM_CU = (lambda t: None if t is None else 0x1000), 256

    def rec(src, **knobs):
        L.load()
        for k, v in knobs.items():
            L.check(L.load().ga_set_knob(k.encode(), v), k)      # Plan.wgrad asks ga_wgrad_workspace while it records
        return Recorder(src, knobs, cases)

    def done(knobs):
        for k in knobs:
            L.load().ga_unset_knob(k.encode())

    try:
        forced = dict(dma256=dict(NT_DMA=2), t256=dict(NT_DMA=0, NT_T256=15), pp=dict(NT_PP=15), r3=dict(NT_R3=15),
                      dma128=dict(NT_DMA=0, NT_DMA2=15, NT_DMA2_MINK=8))
        for M, N, K in [(70000, 384, 96), (66000, 192, 200), (65600, 768, 384), (70000, 96, 384), (66000, 512, 328), (33000, 1536, 768),
                        (40100, 264, 520), (12500, 3072, 768), (50200, 384, 1536)]:
            for form in ('dma256', 'dma128', 't256', 'pp', 'r3'):
                P = rec(f'test_gemm_lds_dma_form_bf16[{form}]', **forced[form])
                P.gemm(OP, OP, OP, M, N, K, bf, bias=OP, colsum=OP, colsumsq=OP)
                P.gemm(OP, OP, OP, M, N, K, bf, bias=OP, act=ops.ACT_GELU, C2=OP, c2_mode=2)
                P.gemm(OP, OP, OP, M, N, K, bf, bias=OP, rowscale=OP, rows_per_scale=100, R=OP, ldr=N)
                P.gemm(OP, OP, OP, M, N, K, bf, H=OP, ldh=N, h_is_deriv=True, colsum=OP)
                done(forced[form])
        for M, N, K, Z in [(300, 136, 64, 1), (257, 96, 72, 1), (1000, 1000, 768, 1), (5, 40, 96, 1), (2600, 384, 200, 2),
                           (131072 + 40, 128, 96, 1), (70, 1000, 1536, 1)]:
            P = rec('test_gemm_ring3_form_small_and_batched', NT_R3=15)
            kw = dict(batch=Z, strideA=M * K, strideB=N * K, strideC=M * N, bias=OP, strideBias=N)
            P.gemm(OP, OP, OP, M, N, K, bf, colsum=OP, colsumsq=OP, strideCol=N, **kw)
            P.gemm(OP, OP, OP, M, N, K, bf, act=ops.ACT_GELU, C2=OP, c2_mode=2, **kw)
            P.gemm(OP, OP, OP, M, N, K, bf, rowscale=OP, rows_per_scale=7, R=OP, ldr=N, strideR=M * N, **kw)
            P.gemm(OP, OP, OP, M, N, K, bf, R=OP, ldr=N, strideR=M * N, **kw)
            del kw['bias'], kw['strideBias']
            P.gemm(OP, OP, OP, M, N, K, bf, H=OP, ldh=N, strideH=M * N, h_is_deriv=True, colsum=OP, strideCol=N, **kw)
            done(['NT_R3'])
        for Bn, H, W, Cc, N in [(2, 8, 12, 16, 24), (3, 28, 28, 96, 192), (5, 14, 14, 384, 768), (1, 10, 6, 48, 136), (40, 56, 56, 96, 192)]:
            P = rec('test_gemm_patch2_ring3_form_bf16', NT_R3=15)
            M = Bn * (H // 2) * (W // 2)
            P.gemm(OP, OP, OP, M, N, 4 * Cc, bf, a_kind=ops.A_PATCH2, a_dims=(H, W, Cc), bias=OP)
            if N % 8 == 0:
                P.gemm(OP, OP, OP, M, 4 * Cc, N, bf, c_kind=ops.C_UNPATCH2, c_dims=(H, W, Cc))
            done(['NT_R3'])
        # tests/test_cswin_kernels_gpu.py
        for B, H, W, Ci, Co in [(2, 28, 28, 32, 64), (1, 14, 14, 64, 128), (3, 56, 56, 64, 64), (8, 112, 112, 64, 64), (5, 14, 30, 96, 32)]:
            for r3 in (15, 0):
                P = rec('test_conv3x3_stride2_dgrad_on_the_ring_form', NT_R3=r3)
                P.gemm(OP, OP, OP, B * (H // 2) * (W // 2), 4 * Ci, 4 * Co, bf, a_kind=ops.A_NEIGH2, a_dims=(H // 2, W // 2, Co),
                       c_kind=ops.C_UNPATCH2, c_dims=(H, W, Ci))
                done(['NT_R3'])
        for B, H, W, Ci, Co in [(2, 28, 28, 32, 64), (1, 14, 14, 64, 128), (3, 56, 56, 64, 64), (8, 112, 112, 64, 64), (5, 14, 30, 96, 40),
                                (2, 4, 4, 32, 16)]:
            for r3 in (15, 0):
                P = rec('test_conv3x3_stride2_forward_on_the_ring_form', NT_R3=r3)
                P.gemm(OP, OP, OP, B * (H // 2) * (W // 2), Co, 9 * Ci, bf, a_kind=ops.A_CONV3S2, a_dims=(H, W, Ci), bias=OP)
                done(['NT_R3'])
        # tests/test_convnext_wgrad_forms_gpu.py
        for B, H, W, Cc, N in [(256, 56, 56, 96, 192), (256, 28, 28, 192, 384), (256, 14, 14, 384, 768), (1, 56, 56, 96, 192),
                               (1, 256, 256, 96, 192), (12, 56, 56, 96, 192), (80, 12, 40, 24, 40), (64, 28, 28, 192, 384),
                               (256, 28, 28, 128, 256)]:
            for flag in (0, 1):
                P = rec('test_patch2_wgrad_forms', TN2_PATCH2=flag)
                P.wgrad(OP, OP, OP, B * (H // 2) * (W // 2), N, 4 * Cc, bf, dbias=OP, x_kind=ops.A_PATCH2, x_dims=(H, W, Cc))
                done(['TN2_PATCH2'])
        for B, H, W, N, bias in [(256, 224, 224, 96, OP), (1, 224, 224, 96, OP), (64, 224, 224, 128, OP), (3, 36, 52, 96, OP),
                                 (32, 224, 224, 96, OP), (16, 224, 224, 128, OP), (8, 64, 64, 96, None)]:
            for flag in (0, 1):
                P = rec('test_stem_wgrad_forms' if bias else 'test_stem_wgrad_without_bias', STEM4_WGRAD_DIRECT=flag)
                P.wgrad(OP, OP, OP, B * (H // 4) * (W // 4), N, 48, bf, dbias=bias, x_kind=ops.A_STEM4_NCHW, x_dims=(H, W, 3))
                done(['STEM4_WGRAD_DIRECT'])
        # tests/test_gemm_forms_edges_gpu.py: one table feeds the test and this corpus (tests/_gemm_ref.py)
        G = edge_table()
        for c, fam in G.PAIRS:
            P = rec(f'{EDGES}[{fam}-{c.label}]', **G.FAMILIES[fam])
            for epi in c.epis_of(fam):
                kw = {k: (OP if isinstance(v, str) else v) for k, v in G.gemm_kwargs(c, epi, ops).items()}
                P.gemm(OP, OP, OP, c.M, c.N, c.K, ops.ga_dtype(c.dt), **kw)
            done(G.FAMILIES[fam])
    finally:
        ops._ptr, ops._NUM_CU = real_ptr, real_cus
    return cases


def dump_models():
    """part (b), on the GPU machine: the descriptors of every NAMED model's bf16 training engine at the bench batch"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from plan_fingerprint import NAMED
    import imagenet_models_amd as A
    seen, cases = set(), []
    for name, kw in NAMED:
        tag = name + ''.join(f'+{k}' for k in kw)
        torch.manual_seed(0)
        m = A.create_model(name, drop_path_rate=0.2, **kw).cuda()
        eng = m.make_engine(BENCH_BATCH, True, 'bf16')
        n0 = len(cases)
        for p in (eng.prep, eng.fwd, eng.bwd, vars(eng).get('dp_plan')):
            if p is None:
                continue
            p.finalize()
            for fn, args, _ in p.calls:
                fname = BASE.get(getattr(fn, '__name__', ''), getattr(fn, '__name__', ''))
                if fname in FN:
                    desc = pack(args[0]._obj)
                    key = json.dumps([fname, desc], sort_keys=True)
                    if key not in seen:
                        seen.add(key)
                        cases.append(dict(src=tag, fn=fname, desc=desc))
        print(f'{tag}: {len(cases) - n0} new descriptors', flush=True)
        del eng, m
        torch.cuda.empty_cache()
    return cases


def coverage(cases, forms):
    """per parameter of test_gemm_lds_dma_form_bf16: launches whose form is the one the parameter names; per family of
    test_gemm_form_at_its_edges: launches whose form belongs to that family"""
    rows = {}
    for c, f in zip(cases, forms):
        if c['src'].startswith('test_gemm_lds_dma_form_bf16['):
            want = c['src'][c['src'].index('[') + 1:-1]
            hit, n = rows.get(want, (0, 0))
            rows[want] = (hit + (f[0].split(':')[0].split('x')[0] == want), n + 1)
    for want, (hit, n) in rows.items():
        print(f'| `{want}` | {hit} of {n} |')
    # ... and per family of tests/test_gemm_forms_edges_gpu.py: launches that reach a form of that family
    rows = {}
    for c, f in zip(cases, forms):
        if c['src'].startswith(EDGES + '['):
            want = c['src'][c['src'].index('[') + 1:].split('-')[0]
            hit, n = rows.get(want, (0, 0))
            fam = f[0].split(':')[0].split('x')[0]
            rows[want] = (hit + ((fam[:6] if want == 'staged' else fam) == want), n + 1)
    print()
    for want, (hit, n) in rows.items():
        print(f'| `{want}` | {hit} of {n} |')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--coverage', action='store_true')
    ap.add_argument('--dump-models', default='', metavar='FILE', help='write part (b) of the corpus to FILE (needs the GPU)')
    ap.add_argument('--models', default='', metavar='FILE', help='--write: take part (b) from FILE instead of keeping the recorded one')
    a = ap.parse_args()
    if a.dump_models:
        json.dump(dump_models(), open(a.dump_models, 'w'), separators=(',', ':'))
        return 0
    recorded = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else []
    prime()
    if a.check:
        bad = [(c, answer(c)) for c in recorded if answer(c) != c['form']]
        for c, f in bad[:20]:
            print(f"{c['src']} {c.get('knobs', {})} {c['fn']} {c['desc']}: {f}, recorded {c['form']}")
        print(f'{len(recorded)} descriptors, {len(bad)} differences')
        return int(bool(bad) or not recorded)
    cases = test_cases() + (json.load(open(a.models)) if a.models else [c for c in recorded if not c['src'].startswith('test_')])
    forms = [answer(c) for c in cases]
    if a.coverage:
        coverage(cases, forms)
    elif a.write:
        with open(GOLDEN, 'w') as f:
            f.write('[\n' + ',\n'.join(json.dumps(dict(c, form=fm), separators=(',', ':')) for c, fm in zip(cases, forms)) + '\n]\n')
        print(f'{len(forms)} descriptors written to {GOLDEN}')
    else:
        for c, f in zip(cases, forms):
            with L.knobs(**c.get('knobs', {})):
                few = FEWROWS[c['fn']](unpack(c['fn'], c['desc']))
            print(c['src'], json.dumps(c.get('knobs', {})), c['fn'], json.dumps(c['desc']), '->', *f, f'fewrows={few}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
