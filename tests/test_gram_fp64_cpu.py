"""CPU: the host side of the opt-in float64 Gram path (GA_ConvNeXt.get_gram's `training and B < 128` branch): the gram_fp64
kwarg through create_model, its refusal by the families whose reference has no such branch, the train.py flag, and the C ABI."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

NEW_SYMBOLS = ('ga_gram_f64_fwd', 'ga_gram_f64_bwd', 'ga_gram_f64_fwd_workspace', 'ga_gram_f64_bwd_workspace')


def test_kwarg_reaches_the_model_config():
    import imagenet_models_amd as A
    assert A.create_model('ga_convnext_tiny_768', gram_fp64=True).cfg['gram_fp64'] is True
    assert A.create_model('ga_convnext_tiny_768').cfg['gram_fp64'] is False          # off unless asked for
    assert A.create_model('ga_convnext_tiny_768', gram_fp64=None).cfg['gram_fp64'] is False
    assert A.create_model('ga_convnext_small_688', gram_fp64=True).cfg['gram_fp64'] is True


@pytest.mark.parametrize('name', ['ga_CSWin_64_12211_tiny_224', 'map_convnext_tiny', 'map_vit_small_patch16_224', 'map_pit_s',
                                  'map_resnet50', 'map_mobilenet_v1', 'convnext_tiny'])
def test_other_families_refuse_the_kwarg(name):
    import imagenet_models_amd as A
    from imagenet_models_amd import registry
    for value in (True, False):
        with pytest.raises(ValueError, match='gram_fp64 is only defined for the GA-ConvNeXt family'):
            A.create_model(name, gram_fp64=value)
    with pytest.raises(ValueError, match='gram_fp64'):
        registry.model_entrypoint(name)(gram_fp64=True)                                     # the factory itself, not only create_model


def test_train_cli_lists_the_flag():
    r = subprocess.run([sys.executable, 'train.py', '--help'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--gram-fp64' in r.stdout


def test_new_symbols_are_declared_bound_and_exported():
    from imagenet_models_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    declared = set(re.findall(r'^\s*(?:int|size_t)\s+(ga_\w+)\s*\(', hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    # the byte counts of the two caller-owned float64 buffers: packed upper triangle per sample, C x C per sample
    assert lib.ga_gram_f64_fwd_workspace(3, 192) == 3 * (192 * 193 // 2) * 8
    assert lib.ga_gram_f64_bwd_workspace(3, 192) == 3 * 192 * 192 * 8
    assert lib.ga_gram_f64_fwd_workspace(0, 192) == 0


def test_bad_arguments_fail_on_the_host():
    """argument checks run before anything touches the device: null pointers and bad geometry come back as an error code"""
    from imagenet_models_amd import _lib
    lib = _lib.load()
    assert lib.ga_gram_f64_fwd(None, None, None, None, 0, 2, 49, 32, 7, 8, 72, _lib.GA_F32, None) != 0
    assert 'ga_gram_f64_fwd' in _lib.last_error()
    assert lib.ga_gram_f64_bwd(None, None, None, None, None, None, 0, 2, 49, 32, 7, 5, 72, _lib.GA_F32, None) != 0
    assert 'ga_gram_f64_bwd' in _lib.last_error()
