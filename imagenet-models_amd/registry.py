"""timm-style model registry (the reference's plugin boundary: `@register_model` factories looked up by
`create_model(name, pretrained, num_classes, drop_rate, drop_path_rate, ...)`, GA/train.py:407-420)."""
import sys

import warnings

_entrypoints = {}
_unsupported = {}   # name -> reason: registered for state_dict / checkpoint compatibility, refused by the HIP engine
# "extra" names: created, checked and run like any other name, but left out of list_models() unless include_extra=True, so that the
# default list (which the entry-point coverage test pins) stays as it was.  Moving them into the default list is a follow-up that
# updates that pin together with the list.
_extra = set()
# "repaired" names: the reference factory builds the model but the reference's own forward fails for it, and the engine runs the
# composition the reference clearly intends (map_resnet50: MAPHead on [stem, layer1..4] instead of head(x.mean(...))).
# Like the extra tier they are reachable through every lookup and left out of list_models() (include_extra=True too) unless
# include_repaired=True.
_repaired = set()
# "baseline" names: the plain counterpart the reference registers beside a MAP model whose family joined the engine after the default
# list was pinned (pit_s, the pool_type='gap' PoolingTransformer that map_pit_s is measured against).  Reachable through every lookup,
# left out of list_models() -- with include_extra / include_repaired too -- unless include_baseline=True.
_baseline = set()


def register_model(fn, name=None):
    name = name or fn.__name__
    _entrypoints[name] = fn
    mod = sys.modules.get(fn.__module__)
    if name == fn.__name__ and mod is not None and hasattr(mod, '__all__') and name not in mod.__all__:
        mod.__all__.append(name)
    return fn


def register_extra_model(fn, name=None):
    """register_model for an "extra" name (see _extra): reachable through every lookup, listed only with include_extra=True"""
    register_model(fn, name)
    _extra.add(name or fn.__name__)
    return fn


def is_extra(name):
    return name in _extra


def register_repaired_model(fn, name=None):
    """register_model for a "repaired" name (see _repaired): reachable through every lookup, listed only with include_repaired=True"""
    register_model(fn, name)
    _repaired.add(name or fn.__name__)
    return fn


def is_repaired(name):
    return name in _repaired


def register_baseline_model(fn, name=None):
    """register_model for a "baseline" name (see _baseline): reachable through every lookup, listed only with include_baseline=True"""
    register_model(fn, name)
    _baseline.add(name or fn.__name__)
    return fn


def is_baseline(name):
    return name in _baseline


def _unregister(name):
    _entrypoints.pop(name, None)
    _unsupported.pop(name, None)
    _extra.discard(name)
    _repaired.discard(name)
    _baseline.discard(name)


def is_model(name):
    return name in _entrypoints


def mark_unsupported(name, reason):
    _unsupported[name] = reason


def is_supported(name):
    return name in _entrypoints and name not in _unsupported


def list_models(filter='', include_unsupported=False, include_extra=False, include_repaired=False, include_baseline=False):
    """names the HIP engine can run; include_unsupported adds the ones that only construct (parameter layout, checkpoints),
    include_extra the "extra" names (mobilenet_v1, map_mobilenet_v1), include_repaired the "repaired" ones (map_resnet50),
    include_baseline the "baseline" ones (pit_s); every other lookup treats those like any name"""
    return sorted(n for n in _entrypoints if filter in n and (include_unsupported or n not in _unsupported)
                  and (include_extra or n not in _extra) and (include_repaired or n not in _repaired)
                  and (include_baseline or n not in _baseline))


def model_entrypoint(name):
    return _entrypoints[name]


_img_size = {}      # name -> input side, for the names not built for 224 (a factory's module says so beside the factory)


def set_img_size(name, size):
    _img_size[name] = int(size)


def model_img_size(name):
    """the input side a registered name is built for (its cfg['img_size'] once created), known without creating it: a command line
    is checked against it before any weight is allocated"""
    if not is_model(name):
        raise RuntimeError(f'Unknown model ({name}); known: {list_models()}')
    return _img_size.get(name, 224)


def reject_gram_fp64(variant, kwargs):
    """gram_fp64 is GA_ConvNeXt.get_gram's float64 branch (ga_convnext.py:456-457).  ga_cswin.get_gram and MAP's GramToken have no
    such branch in the reference, so every other family refuses the kwarg instead of swallowing it."""
    if 'gram_fp64' in kwargs:
        raise ValueError(f'{variant}: gram_fp64 is only defined for the GA-ConvNeXt family (the float64 branch of '
                         f'GA_ConvNeXt.get_gram); the reference has no such branch for this model')


def create_model(model_name, pretrained=False, checkpoint_path='', scriptable=None, **kwargs):
    """timm.create_model semantics: kwargs whose value is None are dropped before reaching the factory."""
    if not is_model(model_name):
        raise RuntimeError(f'Unknown model ({model_name}); known: {list_models()}')
    kwargs = {k: v for k, v in kwargs.items() if v is not None}
    if model_name in _unsupported:   # say so at creation time, not at the first training step
        warnings.warn(f'{model_name}: {_unsupported[model_name]}', stacklevel=2)
    model = _entrypoints[model_name](pretrained=pretrained, **kwargs)
    if checkpoint_path:
        from .checkpoint import load_checkpoint
        load_checkpoint(model, checkpoint_path)
    return model
