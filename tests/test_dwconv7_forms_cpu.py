"""ga_dwconv7_form / ga_dwconv7_bwd_weight_form (include/gaext.h; csrc/dwconv.hip: dw_select / dww_select) name the kernel form, the
grid and the rows per segment that the depthwise 7x7 launches run, and ga_dwconv7_bwd_weight_workspace still asks for what it asked
for before the selection was hoisted: tests/golden/dwconv7_workspace.json holds its answers over sweep() as recorded from the
library before that change.  Needs no GPU: without a device the selection assumes 256 CUs, the MI355X's count, and on a device
with another count the tests that depend on it return early (the GPU suite derives its shapes from the count instead)."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'dwconv7_workspace.json')
BF, F32 = 1, 0


def _L():
    from imagenet_models_amd import _lib
    assert (_lib.GA_BF16, _lib.GA_F32) == (BF, F32)
    return _lib


def _cus():
    """256 without a device; the device's count otherwise (the selection reads it once)"""
    import torch
    if not torch.cuda.is_available():
        return 256
    n = C.c_int(0)
    _L().check(_L().load().ga_device_info(C.byref(n), None, None), 'ga_device_info')
    return n.value


def fwd_form(B, H, W, Cc, dt, res=0, y2=0):
    L = _L()
    buf = C.create_string_buffer(64)
    L.check(L.load().ga_dwconv7_form(B, H, W, Cc, dt, res, y2, buf, 64), 'ga_dwconv7_form')
    return buf.value.decode()


def wgrad_form(B, H, W, Cc, dt):
    L = _L()
    buf = C.create_string_buffer(64)
    L.check(L.load().ga_dwconv7_bwd_weight_form(B, H, W, Cc, dt, buf, 64), 'ga_dwconv7_bwd_weight_form')
    return buf.value.decode()


def sweep():
    """(B, H, W, C, dtype): every tiling (7x7 ragged, 14x14), the register-sliding eligibility on both sides, channel counts around
    the slices of 32 / 64 and the wave of 64 channel pairs, batches from 1 to the training step's 256"""
    out = []
    for dt in (BF, F32):
        for B in (1, 2, 3, 8, 64, 256):
            for H, W in ((1, 1), (6, 13), (7, 7), (7, 1), (9, 10), (14, 14), (14, 42), (28, 14), (21, 5), (28, 28), (35, 8), (49, 28),
                         (56, 56), (30, 30), (112, 112)):
                for Cc in (4, 8, 12, 24, 36, 40, 64, 68, 72, 96, 128, 136, 192, 384, 512, 768):
                    out.append((B, H, W, Cc, dt))
    return out


def test_workspace_is_what_it_was():
    if _cus() != 256:
        return
    lib = _L().load()
    gold = json.load(open(GOLDEN))
    cases = sweep()
    assert gold['num_cus'] == 256 and len(gold['bytes']) == len(cases)
    bad = [(c, int(lib.ga_dwconv7_bwd_weight_workspace(*c)), g) for c, g in zip(cases, gold['bytes'])
           if int(lib.ga_dwconv7_bwd_weight_workspace(*c)) != g]
    assert not bad, bad[:5]
    # knobs that move the weight gradient between its forms do not move the demand: it is the largest of the forms that may serve
    with _L().knobs(DWW_RS=0, DWW_RS_ROWS=14):
        assert all(int(lib.ga_dwconv7_bwd_weight_workspace(*c)) == g for c, g in zip(cases, gold['bytes']))
    assert lib.ga_dwconv7_bwd_weight_workspace(0, 7, 7, 8, BF) == 0


# the names at 256 CUs.  rs forward: R is the longest divisor of H (a multiple of 7) with B * (H / R) * wpu >= 2048 waves.
FWD = [
    ((256, 56, 56, 96, BF), {}, 'rs:R56:seg1:wpu11'),              # the training step: 256 * 1 * 11 = 2816 waves
    ((5, 14, 14, 192, BF), {}, 'rs:R7:seg2:wpu6'),                 # far from 2048 waves: R falls through to 7
    ((5, 14, 14, 192, BF), dict(DW_RS_ROWS=14), 'rs:R14:seg1:wpu6'),
    ((5, 14, 14, 192, BF), dict(DW_RS_ROWS=21), 'rs:R7:seg2:wpu6'),  # a knob that does not divide H is ignored
    ((2, 21, 8, 136, BF), dict(DW_RS_ROWS=7), 'rs:R7:seg3:wpu3'),  # 2 strips x 68 pairs = 136 lanes: an incomplete third wave
    ((3, 7, 1, 8, BF), {}, 'rs:R7:seg1:wpu1'),
    ((2, 14, 14, 96, BF), dict(DW_RS=0), 'dot2_14x14:gx2:tiles2'),
    ((72, 14, 14, 512, BF), dict(DW_RS=0, DW_MFMA=0), 'dot2_14x14:gx64:tiles72'),     # 2 * 256 / 8 slices
    ((2, 10, 9, 16, BF), {}, 'dot2_7x7:gx8:tiles8'),               # H % 7 != 0: no rs
    ((48, 13, 13, 512, BF), {}, 'dot2_7x7:gx128:tiles192'),        # 4 * 256 / 8 slices
    ((2, 28, 28, 40, BF), dict(DW_RS=0, DW_MFMA=2), 'mfma:gx8:tiles8'),
    ((5, 28, 28, 512, BF), dict(DW_RS=0, DW_MFMA=2), 'mfma:gx16:tiles20'),            # 256 / 16 slices
    ((17, 14, 14, 32, BF), dict(DW_RS=0, DW_MFMA=2), 'mfma:gx16:tiles17'),            # 17 rounded down to a multiple of 8
    ((17, 14, 14, 32, BF), dict(DW_RS=0, DW_MFMA=2, DW_XCD8=0), 'mfma:gx17:tiles17'),
    ((1, 14, 14, 12, BF), {}, 'scalar_14x14+bf16'),                # bf16 with C % 8 != 0
    ((1, 9, 10, 68, BF), {}, 'scalar_7x7+bf16'),
    ((2, 14, 14, 96, F32), {}, 'scalar_14x14+f32'),
    ((1, 1, 1, 4, F32), {}, 'scalar_7x7+f32'),
]
WGRAD = [
    ((256, 56, 56, 96, BF), {}, 'rs:R28:seg2:wpu11:nbw46'),        # B * (H / R) >= 8 * nbw = 368 units first holds at two segments
    ((8, 49, 28, 768, BF), dict(DWW_RS_ROWS=7), 'rs:R7:seg7:wpu42:nbw12'),   # 56 units for 48 waves of a lane map: some walk two
    ((5, 14, 14, 192, BF), {}, 'dot2_14x14:parts5'),               # below 28 x 28 the default keeps the dot2 form
    ((5, 14, 14, 192, BF), dict(DWW_RS=2), 'rs:R7:seg2:wpu6:nbw85'),
    ((5, 14, 14, 192, BF), dict(DWW_RS=2, DWW_RS_ROWS=14), 'rs:R14:seg1:wpu6:nbw85'),
    ((33, 7, 7, 64, BF), dict(DWW_RS=0), 'dot2_7x7:parts33'),
    ((2, 28, 28, 40, BF), dict(DWW_RS=0), 'dot2_14x14:parts8'),
    ((2, 28, 28, 36, BF), {}, 'scalar_14x14:parts16+bf16'),        # two partials (row groups) per workgroup
    ((2, 28, 28, 96, F32), {}, 'scalar_14x14:parts16+f32'),
    ((1, 9, 10, 68, F32), {}, 'scalar_7x7:parts4+f32'),
]


@pytest.mark.parametrize('geom,kn,want', FWD, ids=lambda v: str(v).replace(' ', ''))
def test_forward_names(geom, kn, want):
    if _cus() != 256:
        return
    with _L().knobs(**kn):
        assert fwd_form(*geom) == want
        if want.startswith('rs:'):
            assert fwd_form(*geom, 1, 0) == want + '+res' and fwd_form(*geom, 1, 1) == want + '+res+y2'
        else:
            assert fwd_form(*geom, 1, 1) == want


def test_forward_heuristics():
    """the two choices that rest on the CU count, restated: R of the rs form and `many` of the MFMA form"""
    if _cus() != 256:
        return
    # 28 x 28 x 192: 7 strips x 96 pairs = 672 lanes = 11 waves (10.5); 256 * 11 = 2816 >= 2048 at one segment
    assert fwd_form(256, 28, 28, 192, BF) == 'rs:R28:seg1:wpu11'
    assert fwd_form(128, 28, 28, 192, BF) == 'rs:R14:seg2:wpu11'         # 1408 < 2048 <= 2816
    assert fwd_form(64, 28, 28, 192, BF) == 'rs:R7:seg4:wpu11'           # 64 * 2 * 11 = 1408 < 2048 <= 64 * 4 * 11
    with _L().knobs(DW_RS=0):
        # MFMA by default only from 56 x 56 and tiles x slices >= 16 * 256: 64 * 16 tiles * 3 slices = 3072 is too few
        assert fwd_form(64, 56, 56, 96, BF) == 'dot2_14x14:gx256:tiles1024'
        assert fwd_form(128, 56, 56, 96, BF) == 'mfma:gx80:tiles2048'    # 256 / 3 = 85 -> 80
        assert fwd_form(256, 28, 28, 192, BF) == 'dot2_14x14:gx170:tiles1024'
    with _L().knobs(DW_RS=0, DW_MFMA=0):
        assert fwd_form(128, 56, 56, 96, BF) == 'dot2_14x14:gx256:tiles2048'


@pytest.mark.parametrize('geom,kn,want', WGRAD, ids=lambda v: str(v).replace(' ', ''))
def test_weight_gradient_names(geom, kn, want):
    if _cus() != 256:
        return
    with _L().knobs(**kn):
        assert wgrad_form(*geom) == want


def test_queries_validate_like_the_launches():
    L = _L()
    lib = L.load()
    buf = C.create_string_buffer(64)
    for args in ((1, 7, 7, 6, BF, 0, 0), (0, 7, 7, 8, BF, 0, 0), (1, 7, 7, 8, BF, 0, 1)):      # C % 4, B = 0, a second output without res
        assert lib.ga_dwconv7_form(*args, buf, 64) == -1 and L.last_error()
    assert lib.ga_dwconv7_bwd_weight_form(1, 7, 7, 6, BF, buf, 64) == -1
    assert lib.ga_dwconv7_form(1, 7, 7, 8, BF, 0, 0, None, 0) == 0                              # no buffer: validation only
    small = C.create_string_buffer(6)
    assert lib.ga_dwconv7_form(1, 7, 7, 8, BF, 0, 0, small, 6) == 0 and small.value == b'rs:R7'  # truncated, NUL-terminated
