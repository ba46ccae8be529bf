"""CPU: the MAP-ResNet50 container (imagenet_models_amd.map_resnet) against the reference's layout recorded in
tests/golden/map_rn50_eval.npz (tools/gen_golden_map_resnet.py, from the reference classes): state_dict names / shapes / order,
parameter count, the weight-decay split, reference-order loading, and the registry's "repaired" tier."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NAME = 'map_resnet50'


def _z():
    return np.load(os.path.join(GOLDEN, 'map_rn50_eval.npz'))


def test_repaired_tier_is_created_but_not_listed():
    import imagenet_models_amd as A
    from imagenet_models_amd import registry
    base = A.list_models()
    extra = A.list_models(include_extra=True)
    assert len(base) == 19 and NAME not in base and NAME not in extra
    assert set(extra) - set(base) == {'mobilenet_v1', 'map_mobilenet_v1'}          # the two pinned lists are unchanged
    full = A.list_models(include_extra=True, include_repaired=True)
    assert set(full) - set(extra) == {NAME}
    assert A.list_models(include_repaired=True) == sorted(base + [NAME])
    assert A.is_model(NAME) and registry.is_supported(NAME) and registry.is_repaired(NAME) and not registry.is_extra(NAME)
    assert not registry.is_repaired('map_mobilenet_v1') and not registry.is_repaired('map_convnext_tiny')
    assert callable(registry.model_entrypoint(NAME))


def test_state_dict_matches_reference_record():
    import imagenet_models_amd as A
    z = _z()
    m = A.create_model(NAME, drop_path_rate=0.2)
    sd = m.state_dict()
    assert list(sd) == z['state_names'].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == z['state_shapes'].tolist()
    assert len(sd) == int(z['n_state']) == 628
    assert sum(p.numel() for p in m.parameters()) == int(z['param_count']) == 42708288
    keys = list(sd)
    # stem.*, head.*, layer1.* ... layer4.* (the head is assigned before the layers are attached)
    firsts = [next(i for i, k in enumerate(keys) if k.startswith(p)) for p in ('stem.', 'head.', 'layer1.', 'layer2.', 'layer3.', 'layer4.')]
    assert firsts == sorted(firsts) and firsts[0] == 0
    trunk = sum(p.numel() for n, p in m.named_parameters() if not n.startswith('head.'))
    assert trunk == 14360608
    assert m.num_classes == 1000 and m.cfg['drop_path_rate'] == 0.2


def test_num_classes_drop_and_pretrained():
    import imagenet_models_amd as A
    m = A.create_model(NAME, num_classes=40, drop=0.0)
    assert dict(m.named_parameters())['head.heads.0.head.weight'].shape[0] == 40
    with pytest.raises(RuntimeError, match='network fetch'):
        A.create_model(NAME, pretrained=True)
    with pytest.raises(NotImplementedError):
        A.create_model(NAME, drop=0.1)


def test_weight_decay_split():
    """timm's rule (no decay for ndim <= 1 and *.bias) laid out in the flat buffer: decay part first"""
    import imagenet_models_amd as A
    m = A.create_model(NAME)
    params = list(m.named_parameters())
    decay = [n for n, p in params if p.ndim > 1 and not n.endswith('.bias')]
    assert [n for n, p in params if not m.no_weight_decay_param(n, p)] == decay
    assert all(n.endswith('.weight') for n in decay)
    for n in ('stem.0.0.weight', 'layer1.0.conv2.0.weight', 'layer2.0.downsample.0.weight', 'layer3.5.se.1.0.weight',
              'layer4.2.se.2.weight', 'head.mmcap.multi_scale.concat_conv.0.weight'):
        assert n in decay
    for n in ('stem.0.1.weight', 'layer3.5.conv3.1.weight', 'layer4.2.se.2.bias', 'layer4.2.se.1.1.weight', 'head.heads.0.norm.weight'):
        assert n not in decay and n in dict(params)


def test_reference_order_state_dict_loads():
    """a state_dict in the reference's key order (as a reference checkpoint holds it) loads into the model, values included"""
    import imagenet_models_amd as A
    from _mnv1_state import fill_state
    z = _z()
    shapes = OrderedDict((n, tuple(int(v) for v in s.strip('()').split(',') if v.strip())) for n, s in
                         zip(z['state_names'].tolist(), z['state_shapes'].tolist()))
    sd = fill_state(shapes, seed=3)
    m = A.create_model(NAME)
    m.load_state_dict(sd)
    own = m.state_dict()
    for n in ('stem.0.0.weight', 'layer2.0.downsample.1.running_var', 'layer4.2.se.2.bias', 'head.self_dt_heads.3.head.bias'):
        assert torch.equal(own[n], sd[n])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith('layer4.')})


def test_forward_needs_the_gpu():
    import imagenet_models_amd as A
    m = A.create_model(NAME)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 224, 224))
