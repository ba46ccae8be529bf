"""CPU: the plain PiT container (imagenet_models_amd.pit, registered as pit_s) against the reference's layout recorded in
tests/golden/pit_gap_eval.npz (tools/gen_golden_pit_gap.py, from the reference class): the registry's "baseline" tier, state_dict
names / shapes / order, parameter count, the weight-decay split, the classifier accessors, the gram_fp64 refusal, the factory's
kwargs, and the two token-pooling entry points of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

NAME = 'pit_s'
NEW_SYMBOLS = ('ga_token_gap_fwd', 'ga_token_gap_bwd')


def _z():
    return np.load(os.path.join(GOLDEN, 'pit_gap_eval.npz'))


def test_baseline_tier_is_created_but_not_listed():
    import imagenet_models_amd as A
    from imagenet_models_amd import registry
    base = A.list_models()
    extra = A.list_models(include_extra=True)
    repaired = A.list_models(include_extra=True, include_repaired=True)
    assert len(base) == 19 and set(extra) - set(base) == {'mobilenet_v1', 'map_mobilenet_v1'}       # the three pinned lists are unchanged
    assert set(repaired) - set(extra) == {'map_resnet50'}
    assert all(NAME not in names for names in (base, extra, repaired, A.list_models(include_repaired=True),
                                               A.list_models(include_unsupported=True)))
    assert A.list_models(include_baseline=True) == sorted(base + [NAME])
    assert set(A.list_models(include_extra=True, include_repaired=True, include_baseline=True)) - set(repaired) == {NAME}
    assert A.list_models(filter='pit', include_baseline=True) == ['map_pit_s', NAME]
    assert A.is_model(NAME) and registry.is_supported(NAME) and registry.is_baseline(NAME)
    assert not registry.is_extra(NAME) and not registry.is_repaired(NAME)
    assert not registry.is_baseline('map_pit_s') and not registry.is_baseline('convnext_tiny') and not registry.is_baseline('map_resnet50')
    assert callable(registry.model_entrypoint(NAME))


def test_state_dict_matches_reference_record():
    import imagenet_models_amd as A
    z = _z()
    m = A.create_model(NAME, drop_path_rate=0.1)
    sd = m.state_dict()
    assert list(sd) == z['state_names'].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == z['state_shapes'].tolist()
    assert len(sd) == int(z['n_state'])
    assert sum(p.numel() for p in m.parameters()) == int(z['param_count'])
    assert isinstance(m.head, torch.nn.Linear) and tuple(m.head.weight.shape) == (1000, 576)
    assert m.num_classes == 1000 and m.cfg['drop_path_rate'] == 0.1
    # the trunk is map_pit_s's: same names and shapes outside head.*
    t = {k: tuple(v.shape) for k, v in A.create_model('map_pit_s').state_dict().items() if not k.startswith('head.')}
    assert {k: tuple(v.shape) for k, v in sd.items() if not k.startswith('head.')} == t


def test_factory_kwargs():
    import imagenet_models_amd as A
    from imagenet_models_amd import registry
    m = A.create_model(NAME, num_classes=40, pretrained_cfg=dict(url=''), pretrained_cfg_overlay=dict(file=''))
    assert tuple(m.head.weight.shape) == (40, 576)
    # the MAP-only arguments are accepted and change nothing, as PoolingTransformer ignores them when pool_type != 'map'
    a = A.create_model(NAME, last_dim=64, n_groups=3, n_tokens=2, gram_group=4, multi_scale_level=1, gram=False, self_distill_token=False)
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in A.create_model(NAME).state_dict().items()]
    with pytest.raises(RuntimeError, match='pit_s: .*load a state_dict instead'):
        A.create_model(NAME, pretrained=True)
    with pytest.raises(AssertionError):
        A.PiT(pool_type='map')
    for value in (True, False):
        with pytest.raises(ValueError, match='gram_fp64 is only defined for the GA-ConvNeXt family'):
            A.create_model(NAME, gram_fp64=value)
    with pytest.raises(ValueError, match='gram_fp64'):
        registry.model_entrypoint(NAME)(gram_fp64=True)


def test_weight_decay_split():
    """map_pit.py:159-161 (pos_embed, cls_token) on top of timm's rule (no decay for ndim <= 1 and *.bias)"""
    import imagenet_models_amd as A
    m = A.create_model(NAME)
    params = list(m.named_parameters())
    decay = [n for n, p in params if not m.no_weight_decay_param(n, p)]
    assert decay == [n for n, p in params if p.ndim > 1 and not n.endswith('.bias') and n != 'pos_embed']
    assert 'pos_embed' not in decay and dict(params)['pos_embed'].ndim == 4
    assert m.no_weight_decay() == {'pos_embed', 'cls_token'}
    for n in ('patch_embed.conv.weight', 'transformers.1.blocks.5.attn.qkv.weight', 'pools.1.conv.weight', 'head.weight'):
        assert n in decay
    for n in ('head.bias', 'transformers.0.blocks.0.norm1.weight', 'pools.0.conv.bias'):
        assert n not in decay and n in dict(params)


def test_classifier_accessors():
    import imagenet_models_amd as A
    m = A.create_model(NAME)
    assert m.get_classifier() is m.head
    trunk = {k: v.clone() for k, v in m.state_dict().items() if not k.startswith('head.')}
    m.reset_classifier(24)
    assert m.num_classes == 24 and m.cfg['num_classes'] == 24 and m.get_classifier() is m.head
    assert tuple(m.head.weight.shape) == (24, 576) and tuple(m.head.bias.shape) == (24,)
    sd = m.state_dict()
    assert list(sd)[-2:] == ['head.weight', 'head.bias'] and all(torch.equal(sd[k], v) for k, v in trunk.items())
    m.reset_classifier(0)
    assert isinstance(m.head, torch.nn.Identity) and m.num_classes == 0 and not any(k.startswith('head.') for k in m.state_dict())


def test_forward_needs_the_gpu():
    import imagenet_models_amd as A
    with pytest.raises(RuntimeError):
        A.create_model(NAME)(torch.zeros(1, 3, 224, 224))


def test_new_symbols_are_declared_bound_and_exported():
    from imagenet_models_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'gaext.h')).read()
    declared = set(re.findall(r'^\s*(?:int|size_t)\s+(ga_\w+)\s*\(', hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert hasattr(ops.Plan, 'token_gap_fwd') and hasattr(ops.Plan, 'token_gap_bwd')
    # argument checks run on the host, before anything touches the device
    assert lib.ga_token_gap_fwd(None, None, 2, 49, 576, _lib.GA_F32, None) != 0
    assert 'ga_token_gap_fwd' in _lib.last_error()
    assert lib.ga_token_gap_bwd(None, None, 2, 49, 576, _lib.GA_BF16, None) != 0
    assert 'ga_token_gap_bwd' in _lib.last_error()
