"""ops.Plan keeps what it points to: a plan recorded from operands that then go out of scope holds every device address and
host array it will pass at replay.  Plans are built only, apart from one tiny replay over memory that a dropped operand would
have given back to the allocator."""
import ctypes as C
import gc
import json
import os

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

B, HH, CC = 2, 14, 16          # the three workspace calls: 2 x 14 x 14 x 16


def _inputs():
    """the operands of the replayed calls (rowscale; transpose / axpy), the same at every call"""
    g = torch.Generator().manual_seed(7)
    r = lambda *shape: torch.randn(*shape, generator=g).cuda()      # noqa: E731
    return dict(x=r(2, 196, 16), s=r(2), src=r(12, 49), ax=r(500), ay=r(500))


def _replayed(p, i, outs):
    """record the calls the test replays; their outputs are new zero / copied tensors listed in `outs`"""
    y, dst, ay = torch.zeros_like(i['x']), torch.zeros(49, 12, device='cuda'), i['ay'].clone()
    p.rowscale(i['x'], i['s'], y, y.numel(), 196 * 16, 0)
    p.transpose_f32(i['src'], dst, 12, 49)
    p.axpy_f32(ay, i['ax'], 2.0, 500)       # a power of two: the batched and the single kernel round alike
    outs += [y, dst, ay]


def _record():
    """one call of every kind over operands that exist in this function only"""
    from imagenet_models_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    t = lambda *shape, dt=f32: torch.zeros(*shape, dtype=dt, device='cuda')      # noqa: E731
    p = ops.Plan(name='keep', defer_small=True)
    _replayed(p, _inputs(), [])             # a plain wrapper; two deferred small jobs
    p.gemm(t(64, 8), t(16, 8), t(64, 16), 64, 16, 8, ops.GA_F32, bias=t(16), R=t(64, 16), ldr=16, colsum=t(16))
    d = p.attn_desc(t(8, 24, dt=bf), t(8, 8, dt=bf), t(8), 1, 8, 1, 8, 8 ** -0.5, ops.GA_BF16)      # a pre-built descriptor
    p.attn_fwd(d)
    d = p.cswin_desc(t(64, 48, dt=bf), t(64, 16, dt=bf), 1, 8, 16, 2, [(8, 2), (2, 8)], [(t(8, 1, 3, 3), t(8)), (t(8, 1, 3, 3), t(8))],
                     8 ** -0.5, ops.GA_BF16)
    p.cswin_attn_fwd(d)
    p.dwconv7_bwd_weight(t(B, HH, HH, CC, dt=bf), t(B, HH, HH, CC, dt=bf), t(CC, 49), t(CC), B, HH, HH, CC, ops.GA_BF16)
    p.lane = 1                              # another lane: another workspace
    p.dwconv3_bwd_weight(t(B, HH, HH, CC, dt=bf), t(B, HH, HH, CC, dt=bf), t(CC, 9), B, HH, HH, CC, 1, ops.GA_BF16)
    p.lane = 0
    p.bn_gelu_bwd_reduce(t(B * HH * HH, CC, dt=bf), t(B * HH * HH, CC, dt=bf), t(CC), t(CC), t(CC), t(CC), t(CC), t(CC), B * HH * HH, CC,
                         ops.GA_BF16)
    w = next(c['desc'] for c in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'gemm_forms.json')))
             if c['fn'] == 'ga_wgrad' and not c.get('knobs') and c['form'][1] and c['desc']['M'] == 12544)
    p.wgrad(t(w['M'], w['N'], dt=bf), t(w['M'], w['K'], dt=bf), t(w['N'], w['K']), w['M'], w['N'], w['K'], ops.GA_BF16, dbias=t(w['N']))
    p.flush()
    p.u8_normalize(t(2, 3, 8, 8, dt=torch.uint8), t(2, 3, 8, 8), [120.0, 115.0, 100.0], [58.0, 57.0, 57.5])
    return p


def _kept_tensors(p):
    """tensors reachable from plan.keep: the kept ones and those attached to a kept descriptor"""
    out = []
    for k in p.keep:
        for v in [k] + list(getattr(k, 'operands', ())):
            if isinstance(v, torch.Tensor):
                out.append(v)
    return out


def _struct_pointers(s):
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:
            yield name, v
        elif issubclass(typ, C.Array) and typ._type_ is C.c_void_p:
            for k, x in enumerate(v):
                yield f'{name}[{k}]', x


def test_plan_keeps_every_pointer_it_will_pass():
    p = _record()
    gc.collect()
    p.finalize()
    kept = _kept_tensors(p)
    spans = [(t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()) for t in kept + list(p._ws.values())]
    assert len(p._ws) == 2 and all(n > 0 for _, n in spans)

    def held(ptr):
        return any(lo <= ptr < lo + n for lo, n in spans)

    batches = {t.data_ptr(): arr for t, arr in zip(p.keep, p.keep[1:]) if isinstance(t, torch.Tensor) and isinstance(arr, C.Array)}
    names, checked = [], 0
    for fn, args, label in p.calls:
        names.append(fn.__name__)
        assert len(args) == len(fn.argtypes) - 1, label      # the stream is added at replay
        for a, typ in zip(args, fn.argtypes):
            if a is None:
                continue
            if typ is C.c_void_p:
                assert held(a), (label, hex(a))
                checked += 1
            elif issubclass(typ, C._Pointer) and issubclass(typ._type_, C.Structure):      # a descriptor passed by reference
                for name, v in _struct_pointers(a._obj):
                    assert v is None or held(v), (label, name)
                    checked += v is not None
            elif issubclass(typ, C._Pointer):                                              # a host array
                assert any(a is k for k in p.keep), label
                checked += 1
        if fn.__name__.endswith('_batch'):
            assert len(batches[args[0]]) == args[1] == 2
            for d in batches[args[0]]:
                for name, v in _struct_pointers(d):
                    assert v is None or held(v), (label, name)
                    checked += v is not None
    assert names == ['ga_rowscale', 'ga_gemm', 'ga_attn_fwd', 'ga_cswin_attn_fwd', 'ga_dwconv7_bwd_weight', 'ga_dwconv3_bwd_weight',
                     'ga_bn_gelu_bwd_reduce', 'ga_wgrad', 'ga_small_batch', 'ga_u8_normalize']
    # 3 rowscale, 6 gemm, 3 attn, 6 cswin, 5 + 4 + 9 workspace calls, 5 wgrad (4 + workspace), 1 + 4 batch, 2 + 2 u8_normalize
    assert checked == 50
    for i in (4, 5, 6):
        assert p.calls[i][1][-2] is not None and p.calls[i][1][-1] > 0      # finalize() gave each its lane's workspace
    assert p.calls[7][1][0]._obj.ws_bytes == p._ws[0].numel() > 0


def test_kept_operands_survive_new_allocations():
    """memory of a dropped operand would be handed out again: replay after fresh allocations of the same sizes, against eager"""
    from imagenet_models_amd import _lib, ops
    p = _record()
    gc.collect()
    p.finalize()
    fresh = [torch.full_like(v, 12345.0) for v in list(_inputs().values()) * 4]      # noqa: F841
    torch.cuda.synchronize()
    run = [i for i, (fn, _, _) in enumerate(p.calls) if fn.__name__ in ('ga_rowscale', 'ga_small_batch')]
    for i in run:
        p.run_range(i, i + 1)
    torch.cuda.synchronize()
    want = []
    _replayed(ops.Plan(eager=True), _inputs(), want)
    torch.cuda.synchronize()
    batch = next(arr for arr in p.keep if isinstance(arr, C.Array) and isinstance(arr[0], _lib.SmallDesc))
    got_at = [p.calls[run[0]][1][2], batch[0].y, batch[1].y]
    by_ptr = {t.data_ptr(): t for t in _kept_tensors(p)}
    for ptr, w in zip(got_at, want):
        assert w.abs().sum() > 0 and torch.equal(by_ptr[ptr], w)
