"""Plain PiT: the `pool_type != 'map'` branch of MAP/models/map_pit.py (PoolingTransformer :84-201; registered
baseline pit_s :202-218, the model map_pit_s's gain is measured against): the trunk of map_pit, `head` = Linear(dims[-1], num_classes)
on the global average pool of the last stage's tokens (:148, :194).  One (B, num_classes) output in train and eval, not a list.
Compute: engine_pit.PiTEngine."""
import math

import torch
import torch.nn as nn

from .flat_model import FlatModel
from .map_pit import _ConvEmbedding, _HeadPooling, _Transformer
from .registry import register_baseline_model, reject_gram_fp64

__all__ = ['PiT']


class PiT(FlatModel):
    def __init__(self, image_size=224, patch_size=16, stride=8, base_dims=(48, 48, 48), depth=(2, 6, 4), heads=(3, 6, 12), mlp_ratio=4,
                 num_classes=1000, in_chans=3, attn_drop_rate=0., drop_rate=0., drop_path_rate=0., pool_type='gap', last_dim=384,
                 n_groups=4, n_tokens=3, gram_group=24, self_distill_token=True, gram=True, multi_scale_level=2, math_mode=None, **kwargs):
        """last_dim ... multi_scale_level only configure the MAPHead: PoolingTransformer ignores them when pool_type != 'map' (:138-148)"""
        super().__init__()
        assert pool_type != 'map', "this class is the plain PoolingTransformer; pool_type='map' is MAP_PiT"
        assert in_chans == 3 and mlp_ratio == 4, 'only the trunk of the registered pit_s / map_pit_s models'
        assert attn_drop_rate == 0. and drop_rate == 0., 'the reference recipes run PiT without token / attention dropout'
        base_dims, depth, heads = tuple(base_dims), tuple(depth), tuple(heads)
        assert len(base_dims) == len(depth) == len(heads) == 3
        dims = tuple(b * h for b, h in zip(base_dims, heads))
        assert all(dims[i + 1] % dims[i] == 0 for i in range(2)), 'conv_head_pooling is depthwise: C[s+1] must be a multiple of C[s]'
        width = math.floor((image_size - patch_size) / stride + 1)
        self.num_classes = num_classes
        self.drop_path_rate = drop_path_rate
        self.pool_type = pool_type
        self.embed_dim = dims[-1]
        self.cfg = dict(family='pit', img_size=image_size, patch_size=patch_size, stride=stride, base_dims=base_dims, depth=depth,
                        heads=heads, dims=dims, width=width, num_classes=num_classes, drop_path_rate=drop_path_rate)
        self.pos_embed = nn.Parameter(torch.randn(1, dims[0], width, width))
        self.patch_embed = _ConvEmbedding(in_chans, dims[0], patch_size, stride)
        self.transformers = nn.ModuleList([_Transformer(dims[s], depth[s]) for s in range(3)])
        self.pools = nn.ModuleList([_HeadPooling(dims[s], dims[s + 1]) for s in range(2)])
        self.head = nn.Linear(dims[-1], num_classes)             # :148; PyTorch's default init (_init_weights :154-157 only sets LayerNorm)
        nn.init.trunc_normal_(self.pos_embed, std=.02)          # :151
        self.math_mode = math_mode

    @staticmethod
    def no_weight_decay_param(name, p):
        return p.ndim <= 1 or name.endswith('.bias') or name in ('pos_embed', 'cls_token')       # :159-161 + the usual 1-d rule

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        """:166-171: a fresh Linear(embed_dim, num_classes), or Identity for num_classes = 0 (the pooled features; that form has no
        engine).  On the GPU the flat parameter / gradient buffers are re-created, so optimizers and TrainStep objects built before
        the call must be rebuilt (FlatModel.check_flat_generation tells them)."""
        dev = self.pos_embed.device
        self.num_classes = self.cfg['num_classes'] = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes).to(dev) if num_classes > 0 else nn.Identity()
        self._engines = {}
        if self._flat is not None:
            self._flatten()

    def make_engine(self, batch, training, mode):
        if self.num_classes <= 0:
            raise RuntimeError('PiT without a classifier (reset_classifier(0)) returns pooled features in the reference; the engine '
                               'only runs the classifier form')
        from .engine_pit import PiTEngine
        return PiTEngine(self, batch, training, mode)

    def forward(self, x, pre_logits=False):
        assert not pre_logits
        return super().forward(x)[0]


@register_baseline_model
def pit_s(pretrained=False, **kwargs):
    reject_gram_fp64('pit_s', kwargs)
    kwargs.pop('pretrained_cfg', None)
    kwargs.pop('pretrained_cfg_overlay', None)
    if pretrained:
        raise RuntimeError('pit_s: the reference factory loads no weights for this name (map_pit.py:202-218) and a pretrained '
                           'checkpoint would be a network download; load a state_dict instead')
    return PiT(image_size=224, patch_size=16, stride=8, base_dims=[48, 48, 48], depth=[2, 6, 4], heads=[3, 6, 12], mlp_ratio=4,
               pool_type='gap', **kwargs)
