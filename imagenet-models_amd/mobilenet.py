"""MobileNetV1 and MAP-MobileNetV1 on the MI355X-native engine: registry names, constructor arguments and `state_dict` keys / shapes
of the reference's MobileNetV1 (MAP/models/map_mobilenet.py:12-113); every FLOP runs in the hand-written HIP kernels
of libgaext (engine_mobilenet.MobileNetEngine).  The nn.Modules below only HOLD parameters and buffers under the reference's names.

  layers.{i}.{j} ............ conv_bn (:18-23, the 3 -> 32 3 x 3 / 2 stem at layers.0.0) or conv_dw (:25-37): depthwise 3 x 3 conv
                              (no bias) .0, BN .1, pointwise 1 x 1 conv (no bias) .3, BN .4 (the ReLUs at .2 / .5 hold nothing)
  fc (plain) ................ AdaptiveAvgPool2d -> Flatten -> Linear(1024, n_classes) at fc.2
  fc (use_map=True) ......... MAPHead (:67-83): one group, four Gram tokens, no self-distillation token, interactive class
                              attention, mlp_ratio 1, nn.Linear heads; multi_scale_level = -1 -> channel_convertor = ConvNormAct(1024,
                              192, 1) with ReLU on the last map (map.py:356-364)

Outputs: plain -> one (B, n_classes) tensor; MAP -> a list of one (B, n_classes) tensor in both modes (MAPHead without the
self-distillation token, map.py:536-537).
"""
import torch.nn as nn

from .flat_model import FlatModel, Holder
from .map_convnext import _MAPHead
from .registry import register_extra_model, reject_gram_fp64

__all__ = ['MobileNetV1']

# (in, out, stride) of the 13 conv_dw layers per entry of `layers` (map_mobilenet.py:39-63); layers[0] starts with the stem
STAGES = (((32, 64, 1),),
          ((64, 128, 2), (128, 128, 1)),
          ((128, 256, 2), (256, 256, 1)),
          ((256, 512, 2),) + ((512, 512, 1),) * 5,
          ((512, 1024, 2), (1024, 1024, 1)))
STEM_CH = 32


def _conv_bn(inp, oup, stride):
    return nn.Sequential(nn.Conv2d(inp, oup, 3, stride, 1, bias=False), nn.BatchNorm2d(oup))


def _conv_dw(inp, oup, stride):
    # indices 2 / 5 (ReLU) hold no parameters; placeholders keep the reference's numbering
    return nn.Sequential(nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False), nn.BatchNorm2d(inp), nn.Identity(),
                         nn.Conv2d(inp, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup))


class MobileNetV1(FlatModel):
    def __init__(self, ch_in=3, n_classes=1000, use_map=False, math_mode=None, head_drop=0.05, head_attn_drop=0.05, drop_path_rate=0.,
                 **kwargs):
        """head_drop / head_attn_drop: the dropout probabilities of the MAP head (CABlock drop=0.05, MAPHead attn_drop=0.05) -- exposed so
        that parity tests can switch the masks off.  drop_path_rate is accepted and ignored: the reference has no stochastic depth."""
        super().__init__()
        assert ch_in == 3
        self.num_classes = n_classes
        self.use_map = bool(use_map)
        self.drop_path_rate = drop_path_rate
        self.cfg = dict(family='mobilenet_v1', use_map=self.use_map, num_classes=n_classes, drop_path_rate=0.0, stages=STAGES,
                        stem_ch=STEM_CH)
        layers = []
        for i, st in enumerate(STAGES):
            mods = [_conv_bn(ch_in, STEM_CH, 2)] if i == 0 else []
            mods += [_conv_dw(a, b, s) for a, b, s in st]
            layers.append(nn.Sequential(*mods))
        self.layers = nn.ModuleList(layers)
        channels = [st[-1][1] for st in STAGES]
        if self.use_map:
            dim = 192
            # map_mobilenet.py:67-83 (MAPHead arguments) + the MAPHead defaults it keeps (attn_drop 0.05, bp_groups 1)
            self.cfg.update(last_dim=dim, n_groups=1, n_tokens=4, gram_group=32, bp_dim=dim, bp_groups=1, gram_dim=dim, ca_dim=dim,
                            num_heads=dim // 32, mlp_ratio=1, mlp_groups=1, multi_scale_level=-1, channel_convertor=True,
                            head_drop=head_drop, head_attn_drop=head_attn_drop, self_distill_token=False, head_fn='linear',
                            interactive=True, channels=tuple(channels))
            self.norm = nn.Identity()
            self.fc = _MAPHead(self.cfg, channels)
        else:
            self.fc = nn.Sequential(Holder(), Holder(), nn.Linear(channels[-1], n_classes))
        self.math_mode = math_mode

    def make_engine(self, batch, training, mode):
        from .engine_mobilenet import MobileNetEngine
        return MobileNetEngine(self, batch, training, mode)

    def forward(self, x, pre_logits=False):
        """plain: (B, n_classes) logits; MAP: [logits] (one group, no self-distillation token)"""
        assert not pre_logits, 'pre_logits is not on the hot path'
        outs = super().forward(x)
        return outs if self.use_map else outs[0]


def _create(variant, pretrained, use_map, num_classes=1000, **kwargs):
    reject_gram_fp64(variant, kwargs)
    for k in ('pretrained_cfg', 'pretrained_cfg_overlay', 'in_22k', 'drop_rate'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError(f'{variant}: pretrained weights need a network fetch (map_mobilenet.py:104-108); load a local file with '
                           'checkpoint_path= instead')
    return MobileNetV1(ch_in=3, n_classes=num_classes, use_map=use_map, **kwargs)


@register_extra_model
def mobilenet_v1(pretrained=False, **kwargs):
    """map_mobilenet.py:96-98.  num_classes is honoured here (the reference always builds 1000 classes); drop_path_rate is accepted
    and ignored, as the reference ignores it"""
    return _create('mobilenet_v1', pretrained, False, **kwargs)


@register_extra_model
def map_mobilenet_v1(pretrained=False, **kwargs):
    """map_mobilenet.py:101-110 (pretrained=True there downloads a checkpoint: here it raises).  num_classes is honoured (the
    reference always builds 1000 classes); drop_path_rate is accepted and ignored"""
    return _create('map_mobilenet_v1', pretrained, True, **kwargs)
