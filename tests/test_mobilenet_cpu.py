"""CPU: MobileNetV1 / MAP-MobileNetV1 containers (imagenet_models_amd.mobilenet) against the reference's layout recorded in
tests/golden/{mnv1,map_mnv1}_eval.npz (tools/gen_golden_mobilenet.py, from the reference classes): names, parameter counts, state_dict
keys / shapes / order, the weight-decay split, and the registry's "extra" names."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

NAMES = {'mobilenet_v1': 'mnv1', 'map_mobilenet_v1': 'map_mnv1'}


def test_extra_names_are_created_but_not_listed_by_default():
    import imagenet_models_amd as A
    from imagenet_models_amd import registry
    base = A.list_models()
    assert len(base) == 19 and not any('mobilenet' in n for n in base)
    full = A.list_models(include_extra=True)
    assert set(full) - set(base) == set(NAMES)
    for n in NAMES:
        assert A.is_model(n) and registry.is_supported(n) and registry.is_extra(n)
        assert callable(registry.model_entrypoint(n))
        assert A.list_models(filter=n, include_extra=True)[-1] == n


@pytest.mark.parametrize('name', list(NAMES))
def test_state_dict_matches_reference_record(name):
    import imagenet_models_amd as A
    z = np.load(os.path.join(GOLDEN, f'{NAMES[name]}_eval.npz'))
    m = A.create_model(name, drop_path_rate=0.2)          # bench.py passes drop_path_rate: accepted and ignored
    sd = m.state_dict()
    assert list(sd) == z['state_names'].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == z['state_shapes'].tolist()
    assert len(sd) == int(z['n_state']) == {'mobilenet_v1': 164, 'map_mobilenet_v1': 203}[name]
    count = sum(p.numel() for p in m.parameters())
    assert count == int(z['param_count']) == {'mobilenet_v1': 4231976, 'map_mobilenet_v1': 4879612}[name]
    assert m.num_classes == 1000


@pytest.mark.parametrize('name', list(NAMES))
def test_num_classes_and_pretrained(name):
    import imagenet_models_amd as A
    m = A.create_model(name, num_classes=40)
    head = 'fc.2.weight' if name == 'mobilenet_v1' else 'fc.heads.0.weight'
    assert dict(m.named_parameters())[head].shape[0] == 40
    with pytest.raises(RuntimeError, match='network fetch'):
        A.create_model(name, pretrained=True)


@pytest.mark.parametrize('name', list(NAMES))
def test_weight_decay_split(name):
    """timm's rule (no decay for ndim <= 1 and *.bias) laid out in the flat buffer: decay part first"""
    import imagenet_models_amd as A
    m = A.create_model(name)
    params = list(m.named_parameters())
    decay = [n for n, p in params if p.ndim > 1 and not n.endswith('.bias')]
    nodecay = [n for n, p in params if n not in decay]
    assert [n for n, p in params if not m.no_weight_decay_param(n, p)] == decay
    # every conv / linear weight decays, every BatchNorm / bias parameter does not
    assert all(n.endswith('.weight') for n in decay)
    assert all(('.1.' in n or '.4.' in n or n.endswith('.bias') or 'norm' in n or p.ndim <= 1)
               for n, p in params if n in nodecay)
    assert 'layers.0.0.0.weight' in decay and 'layers.3.2.0.weight' in decay and 'layers.3.2.1.weight' in nodecay
    if name == 'mobilenet_v1':
        assert 'fc.2.weight' in decay and 'fc.2.bias' in nodecay
    else:
        assert 'fc.mmcap.channel_convertor.0.weight' in decay and 'fc.mmcap.channel_convertor.1.weight' in nodecay


def test_forward_needs_the_gpu():
    import torch
    import imagenet_models_amd as A
    m = A.create_model('mobilenet_v1')
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 224, 224))
