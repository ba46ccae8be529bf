"""CPU: host logic of the product package -- the C-ABI library loads and exports every symbol include/gaext.h
declares (no compute without a GPU), registry / factories / state_dict surface, flat parameter layout, gradient
buckets + a world-size-2 gloo all-reduce over them, LR schedule, and the "no CPU fallback" contract."""
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


_C_CLASS = {'int': 'int', 'int64_t': 'i64', 'float': 'f32', 'double': 'f64', 'size_t': 'u64', 'uint64_t': 'u64'}


def _c_class(ctype):
    """class of a C type as the header spells it: every pointer and handle is 'ptr'"""
    ctype = re.sub(r'\bconst\b', '', ctype).strip()
    return 'ptr' if '*' in ctype or ctype in ('ga_stream_t', 'ga_comm_t') else _C_CLASS[ctype]


def _py_class(typ):
    """... and of a ctypes type of _lib"""
    import ctypes as C
    if typ in (C.c_void_p, C.c_char_p) or issubclass(typ, C._Pointer):
        return 'ptr'
    return {C.c_int: 'int', C.c_int64: 'i64', C.c_float: 'f32', C.c_double: 'f64', C.c_size_t: 'u64', C.c_uint64: 'u64'}[typ]


def test_library_exports_every_declared_symbol():
    from imagenet_models_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    declared = sorted(set(re.findall(r'^\s*(?:int|size_t)\s+(ga_\w+)\s*\(', hdr, flags=re.M)))
    assert len(declared) >= 38
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/gaext.h but not exported by libgaext.so'
    assert sorted(_lib.exported_symbols()) == declared, 'ctypes signature table out of sync with the header'
    assert lib.ga_version() >= 100
    # every prototype: argument count, the class of each argument (pointer / handle, int, int64_t, float, double, 64-bit unsigned)
    # and of the return value against _SIGS
    protos = re.findall(r'^\s*(int|size_t)\s+(ga_\w+)\s*\(([^)]*)\)\s*;', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S), flags=re.M)
    assert sorted(p[1] for p in protos) == declared
    for ret, name, params in protos:
        params = [] if params.strip() in ('', 'void') else [re.sub(r'\w+$', '', p.strip()) for p in params.split(',')]
        argtypes, restype = _lib._SIGS[name]
        assert [_c_class(p) for p in params] == [_py_class(t) for t in argtypes], name
        assert _c_class(ret) == _py_class(restype), name


def test_tuning_knobs_are_a_table_not_the_environment():
    """include/gaext.h ga_set_knob / ga_unset_knob / ga_config_string: no launch reads the environment; a non-default knob shows
    up in the configuration string (what a bench or parity record prints); result-changing debug switches are compiled out"""
    import subprocess
    from imagenet_models_amd import _lib
    lib = _lib.load()
    base = _lib.config_string()
    assert base.startswith('libgaext ') and 'gfx950' in base and 'DEBUG-BUILD' not in base
    assert 'NT_DMA' not in base
    with _lib.knobs(NT_DMA=2, TN2=0):
        s = _lib.config_string()
        assert 'NT_DMA=2(api)' in s and 'TN2=0(api)' in s, s
    assert _lib.config_string() == base
    assert lib.ga_set_knob(b'', 1) != 0 and lib.ga_set_knob(b'X' * 40, 1) != 0
    # getenv appears in the runtime's knob table only; the debug knob of the ping-pong GEMM body is not in a release build
    for f in os.listdir(os.path.join(ROOT, 'imagenet-models_amd', 'csrc')):
        if f.endswith('.hip') and f != 'runtime.hip':
            assert 'getenv' not in open(os.path.join(ROOT, 'imagenet-models_amd', 'csrc', f)).read(), f
    strs = subprocess.run(['strings', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert 'PP_DBG' not in strs


def test_library_never_allocates_device_memory():
    """include/gaext.h: every pointer is caller-owned; the two reducing entry points take a caller workspace"""
    import subprocess
    from imagenet_models_amd import _lib
    syms = subprocess.run(['nm', '-D', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for banned in ('hipMalloc', 'hipFree', 'hipMallocAsync', 'hipDeviceSynchronize', 'hipStreamSynchronize'):
        assert not re.search(r'\bU ' + banned + r'\b', syms), f'libgaext.so references {banned}'
    lib = _lib.load()
    assert lib.ga_dwconv7_bwd_weight_workspace(2, 14, 14, 64, _lib.GA_BF16) > 0


def test_descriptor_structs_match_header_field_order():
    import ctypes as C
    from imagenet_models_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()

    def fields(struct_name):
        """(name, class, array length or 0) of every field, in order"""
        end = hdr.index('} ' + struct_name + ';')
        body = hdr[hdr.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        out = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            base, stars, rest = re.match(r'^((?:const\s+)?\w+)\s*(\**)\s*(.*)$', decl, flags=re.S).groups()
            for part in rest.split(','):
                ptr, name, n = re.match(r'^\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*$', part).groups()
                out.append((name, _c_class(base + stars + ptr), int(n or 0)))
        return out

    def py_fields(cls):
        return [(name, _py_class(typ._type_), typ._length_) if issubclass(typ, C.Array) else (name, _py_class(typ), 0)
                for name, typ in cls._fields_]

    structs = (('ga_gemm_desc', _lib.GemmDesc), ('ga_wgrad_desc', _lib.WgradDesc), ('ga_wprep_desc', _lib.WprepDesc),
               ('ga_wunfold_desc', _lib.WunfoldDesc), ('ga_small_desc', _lib.SmallDesc), ('ga_cswin_attn_desc', _lib.CswinAttnDesc),
               ('ga_mlp_desc', _lib.MlpDesc), ('ga_mlp_bwd_desc', _lib.MlpBwdDesc), ('ga_small_linear_desc', _lib.SmallLinearDesc),
               ('ga_attn_desc', _lib.AttnDesc))
    assert len(structs) == hdr.count('typedef struct {') == len([c for c in vars(_lib).values()
                                                                  if isinstance(c, type) and issubclass(c, C.Structure)])
    for cname, cls in structs:
        assert fields(cname) == py_fields(cls), cname


def test_registry_and_factories():
    import imagenet_models_amd as A
    import warnings
    from imagenet_models_amd import registry
    names = A.list_models()
    for n in ('ga_convnext_tiny_688', 'ga_convnext_tiny_768', 'ga_convnext_small_688', 'ga_convnext_small_768',
              'ga_convnext_base_976', 'ga_convnext_base_1024'):      # all six registered variants (ga_convnext.py:572-613) run on the engine
        assert n in names and A.is_model(n) and registry.is_supported(n)
    # timm create_model drops None kwargs (GA/train.py:407-420 passes many that are None)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m = A.create_model('ga_convnext_tiny_688', pretrained=False, num_classes=10, drop_rate=None, drop_path_rate=0.1,
                           drop_block_rate=None, global_pool=None, bn_momentum=None, bn_eps=None, scriptable=None)
    assert m.num_classes == 10 and m.cfg['dims'][-1] == 688 and m.cfg['dim_embed'] == 168
    assert sum(p.numel() for p in A.create_model('ga_convnext_tiny_688').parameters()) == 47821324
    # an entry point the engine cannot run stays constructible but is hidden from list_models() and warns when created
    registry.register_model(lambda pretrained=False, **kw: A.create_model('ga_convnext_tiny_768', **kw), name='_test_unsupported_entry')
    registry.mark_unsupported('_test_unsupported_entry', 'refuses: test entry')
    try:
        assert '_test_unsupported_entry' not in A.list_models() and '_test_unsupported_entry' in A.list_models(include_unsupported=True)
        with pytest.warns(UserWarning, match='refuses'):
            A.create_model('_test_unsupported_entry')
    finally:
        registry._unregister('_test_unsupported_entry')
    with pytest.raises(RuntimeError):
        A.create_model('ga_convnext_tiny_768', pretrained=True)
    with pytest.raises(RuntimeError):
        A.create_model('not_a_model')


def test_no_cpu_fallback_is_loud():
    import imagenet_models_amd as A
    m = A.create_model('ga_convnext_tiny_768')
    with pytest.raises(RuntimeError, match='no CPU'):
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match='GPU'):
        m.flat_state()
    with pytest.raises(RuntimeError):
        A.ga_loss([torch.zeros(2, 10)] * 5, torch.zeros(2, dtype=torch.long), -0.8)
    from imagenet_models_amd import ops
    with pytest.raises(AssertionError):
        ops.Plan(eager=False).gemm(torch.zeros(8, 8), torch.zeros(8, 8), torch.zeros(8, 8), 8, 8, 8, ops.GA_F32)


def _small():
    import imagenet_models_amd as A
    return A.GA_ConvNeXt(num_classes=40, depths=(1, 1, 6, 1, 1), dims=(16, 32, 64, 128, 128), gram_dim=32, dim_embed=64)


# what _small()'s training engine seals (EngineBase.grad_groups(); there is no engine on the CPU): tests/test_grad_marks_gpu.py
# asserts that the engine reports exactly this
GA_CONVNEXT_GROUPS = [('heads', ('stages.4.', 'gram_contraction.', 'gram_layer.', 'gram_embedding.', 'ga.', 'fc.')),
                      ('stage3', ('stages.3.',)), ('stage2', ('stages.2.',)), ('stage1', ('stages.1.',))]


def test_flat_layout_and_buckets_partition_the_gradient_buffer():
    from imagenet_models_amd.trainer import TrainStep
    m = _small()
    m._flatten()   # CPU tensors are fine for the layout logic
    st = m.flat_state()
    total = sum(p.numel() for p in m.parameters())
    assert st['total'] == total
    # timm weight-decay rule: decay segment holds exactly the >=2-D non-bias parameters
    n_decay = sum(p.numel() for n, p in m.named_parameters() if not (p.ndim <= 1 or n.endswith('.bias')))
    assert st['n_decay'] == n_decay
    for n, p in m.named_parameters():
        off, k = st['slices'][n]
        assert p.data_ptr() == st['params'].data_ptr() + 4 * off and p.grad.data_ptr() == st['grads'].data_ptr() + 4 * off
        assert (off < n_decay) == (not m.no_weight_decay_param(n, p))
    from imagenet_models_amd.trainer import make_buckets
    for cap in (8 << 20, 50000):     # one bucket per run / runs cut into <= 50k-element all-reduces
        buckets = make_buckets(st, GA_CONVNEXT_GROUPS, cap)
        cover = sorted((a, b) for _, a, b in buckets)
        assert cover[0][0] == 0 and cover[-1][1] == total
        for (a0, b0), (a1, b1) in zip(cover, cover[1:]):
            assert b0 == a1                                   # exact partition
        assert all(b - a <= cap for a, b in cover)
        # backward-completion order: the heads' slices first (the end of the decay segment), marks never go backwards
        assert buckets[0][0] == 'heads' and any(mk == 'heads' and b == n_decay for mk, a, b in buckets)
        marks = [mk for mk, _, _ in buckets]
        order = [g for g, _ in GA_CONVNEXT_GROUPS] + ['end']
        assert [order.index(mk) for mk in marks] == sorted(order.index(mk) for mk in marks)
        owner = {n: next((g for g, pre in GA_CONVNEXT_GROUPS if n.startswith(tuple(pre))), 'end') for n in st['slices']}
        for n, (off, k) in st['slices'].items():
            assert all(mk == owner[n] for mk, a, b in buckets if a < off + k and off < b), n
    k_off = st['slices']['ga.0.attn.k.weight'][0]
    v_off = st['slices']['ga.0.attn.v.weight'][0]
    assert v_off == k_off + m.ga[0].attn.k.weight.numel()   # engine relies on k/v adjacency


def _gloo_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from imagenet_models_amd.trainer import make_buckets
    torch.manual_seed(0)
    m = _small()
    m._flatten()
    st = m.flat_state()
    buckets = make_buckets(st, GA_CONVNEXT_GROUPS, 60000)
    g = torch.Generator().manual_seed(100 + rank)
    local = torch.randn(st['total'], generator=g)
    st['grads'].copy_(local / world)          # TrainStep folds 1/world into the loss gradient scale
    works = [dist.all_reduce(st['grads'][a:b], async_op=True) for _, a, b in buckets]
    for w in works:
        w.wait()
    want = sum(torch.randn(st['total'], generator=torch.Generator().manual_seed(100 + r)) for r in range(world)) / world
    ok = torch.allclose(st['grads'], want, atol=1e-6)
    # parameter views see the reduced gradient
    p = dict(m.named_parameters())['fc.4.weight']
    off, k = st['slices']['fc.4.weight']
    ok = ok and torch.equal(p.grad.reshape(-1), st['grads'][off:off + k])
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_bucketed_allreduce_world2_gloo():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(res) == [(0, True), (1, True)]


def test_cosine_schedule_matches_timm_formula():
    import math
    from imagenet_models_amd.optim import CosineLRScheduler

    class _Opt:
        param_groups = [dict(lr=5e-3, initial_lr=5e-3)]
    opt = _Opt()
    sch = CosineLRScheduler(opt, t_initial=300, lr_min=1e-5, warmup_t=3, warmup_lr_init=1e-6)
    assert opt.param_groups[0]['lr'] == 1e-6
    sch.step(1)
    assert abs(opt.param_groups[0]['lr'] - (1e-6 + (5e-3 - 1e-6) / 3)) < 1e-12
    sch.step(150)
    assert abs(opt.param_groups[0]['lr'] - (1e-5 + 0.5 * (5e-3 - 1e-5) * (1 + math.cos(math.pi * 150 / 300)))) < 1e-12


def test_drop_path_schedule_matches_reference():
    # ga_convnext.py:362: linspace over sum(depths) INCLUDING the trailing 1; gram layers take the last point
    from oracle import ga_convnext_oracle as O
    import imagenet_models_amd as A
    from imagenet_models_amd.engine import GAEngine, tap_indices
    assert tap_indices(9, 2) == O.tap_indices(9, 2) == [2, 5]
    assert tap_indices(27, 4) == O.tap_indices(27, 4) == [4, 9, 14, 19]
    m = A.create_model('ga_convnext_tiny_768', drop_path_rate=0.2)
    eng = GAEngine.__new__(GAEngine)
    eng.cfg = m.cfg
    rates = GAEngine._drop_path_rates(eng)
    ref = O.drop_path_rates(O.make_cfg('ga_convnext_tiny_768', drop_path_rate=0.2))
    assert abs(rates['stages.2.blocks.4.'] - ref[2][4]) < 1e-7 and abs(rates['stages.3.blocks.2.'] - ref[3][2]) < 1e-7
    assert abs(rates['gram_layer.3.blocks.0.'] - ref[4][0]) < 1e-7 and rates['stages.4.'] == pytest.approx(0.2)


def test_engines_compose_builders_over_one_base():
    """every engine family is engine_base.EngineBase plus the builders it runs: no family carries another family's head, and no
    method name means two things inside one engine (same name in two classes of an MRO -> same parameter list; against the base
    only its declared hooks _build / _drop_path_rates are compared)"""
    import inspect
    from imagenet_models_amd.engine import GAEngine
    from imagenet_models_amd.engine_base import EngineBase
    from imagenet_models_amd.engine_convnext import ConvNeXtEngine
    from imagenet_models_amd.engine_cswin import CSWinEngine
    from imagenet_models_amd.engine_map import MAPEngine
    from imagenet_models_amd.engine_mobilenet import MobileNetEngine
    from imagenet_models_amd.engine_pit import MAPPiTEngine, PiTEngine
    from imagenet_models_amd.engine_resnet import ResNetEngine
    from imagenet_models_amd.engine_vit import MAPViTEngine
    families = [MAPEngine, MAPViTEngine, MAPPiTEngine, PiTEngine, ResNetEngine, MobileNetEngine, ConvNeXtEngine, CSWinEngine]
    for E in families:
        assert issubclass(E, EngineBase), E
        assert hasattr(E, '_build_heads') == (E is CSWinEngine), E
    assert not hasattr(PiTEngine, '_build_map_head') and not hasattr(ConvNeXtEngine, '_build_map_head')
    for E in families + [GAEngine]:
        assert E.__mro__[-2] is EngineBase, E       # the base comes last
        seen = {}
        for cls in E.__mro__[:-1]:
            for name, f in vars(cls).items():
                f = getattr(f, '__func__', f)       # staticmethod
                if not inspect.isfunction(f) or (cls is EngineBase and name not in ('_build', '_drop_path_rates')):
                    continue
                sig = str(inspect.signature(f))
                assert seen.setdefault(name, (cls, sig))[1] == sig, (E.__name__, name, seen[name], cls, sig)


def test_load_timm_layout_checkpoint_with_args_namespace(tmp_path):
    """timm CheckpointSaver files (GA/train.py:649-651: args=args) hold an argparse.Namespace, 'module.'-prefixed keys when
    saved from DDP, and state_dict_ema: load_checkpoint must read them under weights_only=True"""
    import argparse
    from imagenet_models_amd.checkpoint import load_checkpoint
    m = _small()
    sd = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}
    ema = {k: torch.full_like(v, 0.5) if v.is_floating_point() else v.clone() for k, v in m.state_dict().items()}
    path = os.path.join(tmp_path, 'checkpoint-3.pth.tar')
    torch.save({'epoch': 3, 'arch': 'ga_convnext_tiny_768', 'state_dict': {'module.' + k: v for k, v in sd.items()},
                'optimizer': {'state': {}, 'param_groups': [{'lr': 0.1}]}, 'version': 2,
                'args': argparse.Namespace(model='ga_convnext_tiny_768', lr=5e-3, opt='lamb'), 'amp_scaler': {'scale': 65536.0},
                'state_dict_ema': ema, 'metric': 81.2}, path)
    load_checkpoint(m, path)
    assert float(m.fc[0].weight.mean()) == 0.25
    load_checkpoint(m, path, use_ema=True)
    assert float(m.fc[0].weight.mean()) == 0.5
    with pytest.raises(RuntimeError, match='size mismatch'):      # a wrong-shaped tensor is rejected, not broadcast
        bad = dict(sd)
        bad['fc.0.bias'] = torch.zeros(1)
        m2 = _small()
        m2._flatten()
        m2.load_state_dict(bad)


def test_second_cuda_call_keeps_flat_buffers_and_stale_holders_raise():
    """model.cuda()/.to() after the optimizer exists must not silently re-create the flat buffers"""
    m = _small()
    m._flatten()
    st = m.flat_state()
    gen = st['gen']
    m.check_flat_generation(gen, 'test')
    m._flatten()                                  # what a parameter move does
    with pytest.raises(RuntimeError, match='re-created'):
        m.check_flat_generation(gen, 'test')


def test_asm_load_audit_flags_a_touched_destination(tmp_path):
    """tools/asm_load_audit.py (run by the Makefile on every rebuild of gemm.hip): an instruction that touches the destination
    registers of an inline-asm buffer load before the s_waitcnt that retires it is a finding; the same code with the wait first is not."""
    import subprocess
    import sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'asm_load_audit.py')
    bad = """_Z9my_kernelv:                           ; @_Z9my_kernelv
\tbuffer_load_dwordx4 v[4:7], v1, s[8:11], 0 offen
\tv_add_u32_e32 v5, v2, v3
\ts_waitcnt vmcnt(0)
\ts_endpgm
.Lfunc_end0:
"""
    good = bad.replace('\tv_add_u32_e32 v5, v2, v3\n\ts_waitcnt vmcnt(0)\n', '\ts_waitcnt vmcnt(0)\n\tv_add_u32_e32 v5, v2, v3\n')
    lds = bad.replace('buffer_load_dwordx4 v[4:7], v1, s[8:11], 0 offen', 'buffer_load_dwordx4 v1, s[8:11], 0 offen lds')
    for text, rc in ((bad, 1), (good, 0), (lds, 0)):
        f = tmp_path / 'k.s'
        f.write_text(text)
        r = subprocess.run([sys.executable, tool, str(f), 'my_kernel'], capture_output=True, text=True)
        assert r.returncode == rc, (text, r.stdout, r.stderr)


def test_asm_store_audit_flags_a_write_behind_a_16_byte_buffer_store(tmp_path):
    """tools/asm_load_audit.py --stores (run by the Makefile on every rebuild of dwconv.hip): a VALU write of a 16-byte buffer
    store's data registers inside the 2 wait states behind the store is a finding (hipcc does not pad this pair when
    the store has an SGPR offset); behind `s_nop 1`, or on other registers, it is not."""
    import subprocess
    import sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'asm_load_audit.py')
    bad = """_Z9my_kernelv:                           ; @_Z9my_kernelv
\tbuffer_store_dwordx4 v[4:7], v1, s[8:11], s2 offen
\tv_pk_mul_f32 v[6:7], s[34:35], v[16:17]
\ts_endpgm
.Lfunc_end0:
"""
    padded = bad.replace('\tv_pk_mul_f32', '\ts_nop 1\n\tv_pk_mul_f32')
    other = bad.replace('v_pk_mul_f32 v[6:7]', 'v_pk_mul_f32 v[8:9]')
    for text, rc in ((bad, 1), (padded, 0), (other, 0)):
        f = tmp_path / 'k.s'
        f.write_text(text)
        r = subprocess.run([sys.executable, tool, '--stores', str(f), 'my_kernel'], capture_output=True, text=True)
        assert r.returncode == rc, (text, r.stdout, r.stderr)


def _gemm_forms_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gemm_forms', os.path.join(ROOT, 'tools', 'gemm_forms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.prime()
    return mod


def test_kernel_form_selection_matches_the_recorded_corpus():
    """ga_gemm_form / ga_wgrad_form (and ga_wgrad_workspace) over tests/golden/gemm_forms.json -- the descriptors of the forced-form GPU
    tests under their knobs and of the model engines at the bench batch -- name the recorded forms; the test part of the corpus is the
    one tools/gemm_forms.py restates from the tests"""
    import json
    T = _gemm_forms_tool()
    recorded = json.load(open(T.GOLDEN))
    assert len(recorded) > 400 and any(not c['src'].startswith('test_') for c in recorded)
    bad = [(c['src'], c.get('knobs'), c['desc'], T.answer(c), c['form']) for c in recorded if T.answer(c) != c['form']]
    assert not bad, bad[:5]
    strip = lambda c: {k: c[k] for k in ('src', 'knobs', 'fn', 'desc')}
    assert [strip(c) for c in recorded if c['src'].startswith('test_')] == [strip(c) for c in T.test_cases()]


def test_kernel_form_selection_structural_properties():
    """seeded random descriptors: ga_*_form rejects exactly what the header's requirements reject (GA_ERR_BAD_ARG); under default knobs
    no form is named whose hard precondition is false (t256: N % 256 == 0 and K >= 256; pp: K >= NT_PP_MINK; LDS-DMA forms: operand
    offsets < 2^30; r3: K >= 64); the name of a weight-gradient form gives the bytes ga_wgrad_workspace reports"""
    import ctypes as C
    import random
    from imagenet_models_amd import _lib as L, ops
    T = _gemm_forms_tool()
    lib = L.load()
    rnd = random.Random(20261019)
    buf = C.create_string_buffer(64)
    PTR = lambda null=0.0, mis=0.0: 0 if rnd.random() < null else 0x10000 + (rnd.randrange(1, 16) if rnd.random() < mis else 0)
    dim = lambda: rnd.choice([rnd.randrange(1, 300), 256 * rnd.randrange(1, 64), 6272 << rnd.randrange(6), 65536 + rnd.randrange(140000),
                              rnd.randrange(1, 3000000), 50176, 73856, 8192, 200704])
    wid = lambda: rnd.choice([8, 24, 40, 64, 96, 128, 136, 192, 256, 264, 384, 512, 768, 1000, 1536, 2208, 3072, rnd.randrange(1, 3100)])
    dep = lambda: rnd.choice([8, 48, 64, 72, 96, 192, 200, 256, 328, 384, 512, 520, 768, 1024, 1536, 3072, 8 * rnd.randrange(1, 400),
                              rnd.randrange(1, 3100)])
    ld = lambda w: rnd.choice([w] * 8 + [w + 8 * rnd.randrange(9), w + rnd.randrange(1, 8), w + (1 << 20)])
    taps = {ops.A_PATCH2: 4, ops.A_NEIGH2: 4, ops.A_CONV3: 9, ops.A_CONV3S2: 9, ops.A_STEM4_NCHW: 16}

    def gather(kind):        # (H, W, C, rows per image) of a mostly valid map
        H, W, Cc = rnd.choice([2, 4, 8, 14, 16, 28, 32, 56, 112, 224, 7]), rnd.choice([2, 4, 8, 16, 28, 32, 48, 56, 112, 224, 5]), \
            rnd.choice([3, 8, 16, 32, 64, 96, 128, 384])
        if kind == ops.A_STEM4_NCHW and rnd.random() < 0.9:
            Cc = 3
        rows = {ops.A_PATCH2: (H // 2) * (W // 2), ops.A_STEM4_NCHW: (H // 4) * (W // 4), ops.A_CONV3S2: ((H + 1) // 2) * ((W + 1) // 2)}.get(kind, H * W)
        return H, W, Cc, max(rows, 1)

    seen = set()
    for i in range(30000):
        if i % 3:
            d = L.GemmDesc(M=dim(), N=wid(), K=dep(), batch=rnd.choice([1] * 8 + [2, 6, 0]), dtype=rnd.choice([L.GA_BF16] * 8 + [L.GA_F32, 7]),
                           a_kind=rnd.choice([ops.A_PLAIN] * 6 + [1, 2, 3, 4, 5, 6]), alpha=rnd.choice([1.0] * 9 + [0.5]),
                           A=PTR(.01, .01), B=PTR(.01, .01), C=PTR(.01, .01), c_f32=rnd.random() < .05, relu_after=rnd.random() < .04)
            if d.a_kind in taps:
                d.a_H, d.a_W, d.a_C, rows = gather(d.a_kind)
                if rnd.random() < .9:
                    d.M, d.K = rows * rnd.choice([1, 2, 8, 64, 256]), taps[d.a_kind] * d.a_C
            d.lda, d.ldb, d.ldc = ld(d.K), ld(d.K), ld(d.N)
            if rnd.random() < .1:
                d.c_kind, d.c_H, d.c_W, d.c_C = rnd.choice([ops.C_UNPATCH2] * 9 + [2]), 56, 56, rnd.choice([d.N // 4, 24])
            epi = rnd.randrange(6)
            d.bias = PTR(.4, .04)
            if epi == 1:
                d.act, d.C2, d.c2_mode = ops.ACT_GELU, PTR(.3, .03), rnd.choice([2, 2, 2, 1, 0])
            elif epi == 2:
                d.R, d.ldr, d.rowscale, d.rows_per_scale = PTR(0, .03), ld(d.N), PTR(.5), rnd.choice([49] * 9 + [0])
            elif epi == 3:
                d.H, d.ldh, d.h_is_deriv = PTR(0, .03), ld(d.N), rnd.random() < .85
            elif epi == 4:
                d.act, d.H, d.ldh, d.R, d.ldr = rnd.randrange(3), PTR(.5), d.N, PTR(.5), d.N
            d.colsum = PTR(.75)
            epc = 8 if d.dtype == L.GA_BF16 else 4
            H, W, Cc = d.a_H, d.a_W, d.a_C
            ok = bool(d.A and d.B and d.C) and d.batch >= 1 and d.dtype in (L.GA_BF16, L.GA_F32) and not ((d.A | d.B | d.C) & 15) and \
                d.ldb % epc == 0 and d.K % epc == 0 and \
                {ops.A_PLAIN: lambda: d.lda % epc == 0,
                 ops.A_PATCH2: lambda: Cc % epc == 0 and H % 2 == 0 and W % 2 == 0 and d.K == 4 * Cc and d.M % ((H // 2) * (W // 2)) == 0,
                 ops.A_CONV3: lambda: Cc % epc == 0 and d.K == 9 * Cc and d.M % (H * W) == 0,
                 ops.A_CONV3S2: lambda: Cc % epc == 0 and d.K == 9 * Cc and d.M % (((H + 1) // 2) * ((W + 1) // 2)) == 0,
                 ops.A_NEIGH2: lambda: Cc % epc == 0 and d.K == 4 * Cc and d.M % (H * W) == 0,
                 ops.A_STEM4_NCHW: lambda: Cc == 3 and d.K == 48 and H % 4 == 0 and W % 4 == 0}.get(d.a_kind, lambda: False)() and \
                ((d.c_C % 8 == 0 and d.N == 4 * d.c_C and not d.c_f32) if d.c_kind == ops.C_UNPATCH2 else d.c_kind == ops.C_PLAIN) and \
                (not d.H or (d.H & 15 == 0 and d.ldh % 8 == 0)) and (not d.R or (d.R & 15 == 0 and d.ldr % 8 == 0)) and \
                (not d.C2 or (d.C2 & 15 == 0 and d.c_kind == ops.C_PLAIN and not d.c_f32 and d.c2_mode in (1, 2))) and \
                (not d.rowscale or d.rows_per_scale > 0) and (d.c_kind != ops.C_PLAIN or d.ldc % 8 == 0)
            rc = lib.ga_gemm_form(C.byref(d), buf, 64)
            assert rc == (0 if ok else -1), (rc, ok, T.pack(d), L.last_error())
            if not ok:
                continue
            form = buf.value.decode()
            kind = form.split(':')[0]
            seen.add('staged' if kind.startswith('staged') else kind.split('x')[0])
            fits = d.M * d.lda < 1 << 30 and d.N * d.ldb < 1 << 30
            assert kind != 't256' or (d.N % 256 == 0 and d.K >= 256 and fits), (form, T.pack(d))
            assert kind != 'pp' or d.K >= 512, (form, T.pack(d))
            assert not kind.startswith('dma') or fits, (form, T.pack(d))
            assert kind not in ('r3', 'r3g') or d.K >= 64, (form, T.pack(d))
        else:
            d = L.WgradDesc(M=dim(), N=wid(), K=dep(), batch=rnd.choice([1] * 8 + [2, 0]), dtype=rnd.choice([L.GA_BF16] * 8 + [L.GA_F32, 5]),
                            x_kind=rnd.choice([ops.A_PLAIN] * 4 + [1, 2, 3, 4, 5, 6]), alpha=1.0, Y=PTR(.01, .01), X=PTR(.01, .01), dW=PTR(.01),
                            dbias=PTR(.6), split_m=rnd.choice([1, 1, 2, 16, 0]), accumulate=rnd.random() < .7, x_act=rnd.random() < .1)
            if d.x_kind in taps:
                d.x_H, d.x_W, d.x_C, rows = gather(d.x_kind)
                if d.x_kind == ops.A_CONV3S2:
                    rows = max((d.x_H // 2) * (d.x_W // 2), 1)
                if rnd.random() < .9:
                    d.M, d.K = rows * rnd.choice([1, 2, 8, 64, 256]), taps[d.x_kind] * d.x_C
                if rnd.random() < .7:
                    d.N = rnd.choice([96, 128]) if d.x_kind == ops.A_STEM4_NCHW else 64
            d.ldy, d.ldx, d.ldw = ld(d.N), ld(d.K), d.K
            have_ws = rnd.random() < .8
            if have_ws:
                d.workspace, d.ws_bytes = 0x20000, 1 << 50
            epc = 8 if d.dtype == L.GA_BF16 else 4
            ok = bool(d.Y and d.X and d.dW) and d.batch >= 1 and d.split_m >= 1 and d.dtype in (L.GA_BF16, L.GA_F32) and not ((d.Y | d.X) & 15) and \
                d.N % epc == 0 and d.ldy % epc == 0 and \
                (d.ldx % epc == 0 and d.ldx >= (d.K + epc - 1) // epc * epc if d.x_kind == ops.A_PLAIN else
                 d.x_C == 3 and d.K == 48 if d.x_kind == ops.A_STEM4_NCHW else
                 d.x_kind in taps and d.x_C % epc == 0 and d.K == taps[d.x_kind] * d.x_C)
            rc = lib.ga_wgrad_form(C.byref(d), buf, 64)
            assert rc == (0 if ok else -1), (rc, ok, T.pack(d), L.last_error())
            if not ok:
                continue
            form = buf.value.decode()
            part = form.split(':')
            seen.add(part[0])
            per_wg = {'conv3_wgrad_direct': 64 * 576, 'conv3s2_wgrad_direct': 64 * 576, 'conv0_wgrad_direct': 64 * 72, 'stem4_wgrad_direct': d.N * 49}
            need = lib.ga_wgrad_workspace(C.byref(d))
            if not have_ws:
                assert part[0] in ('tn', 'tn2', 'tn2p') and part[-1] != 'partials', form
            elif part[0] in per_wg:
                assert need == int(part[1][3:]) * per_wg[part[0]] * 4, (form, need)
            elif part[0] == 'tn':
                assert need == 0, (form, need)
            else:
                assert need == (d.batch * int(part[1][5:]) * d.N * d.K * 4 if part[2] == 'partials' else 0), (form, need)
    assert seen >= {'r3', 'r3g', 'dma256', 'pp', 't256', 'dma128', 'big', 'staged', 'tn', 'tn2', 'tn2p', 'stem4_wgrad_direct'}, seen
