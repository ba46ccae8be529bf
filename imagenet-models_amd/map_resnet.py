"""MAP-ResNet50 on the MI355X-native engine: registry name, constructor arguments and `state_dict` keys / shapes / order of the
reference's `map_resnet50` (MAP/models/map_resnet.py:200-340); every FLOP runs in the hand-written HIP kernels of libgaext
(engine_resnet.ResNetEngine).  The nn.Modules below only HOLD parameters and buffers under the reference's names.

  stem.{0,1,2} ......... deep stem (stem_type='deep'): ConvNormAct 3 x 3 / 2 3 -> 64, then 3 x 3 64 -> 64 twice (conv .0, BN .1, GELU)
  head.* ............... MAPHead(channels=[64, 256, 512, 1024, 1024], multi_scale_level=3): 4 groups x 4 tokens, gram_group 32,
                         last_dim = ca_dim = 384, 12 heads, interactive class attention, NormHead, self-distillation token,
                         mlp_ratio 4 / mlp_groups 2, GELU after the multi-scale concat conv.  Registered BEFORE the layers: the
                         reference assigns self.head before register_layer() attaches layer1..4 (:248-268)
  layer{1..4}.{j} ...... BottleNeck (:44-67) with SE (:31-41): conv1 1 x 1 / conv2 3 x 3 (stride on conv2) / conv3 1 x 1 (no act),
                         each conv .0 + BN .1; downsample (1 x 1 / stride, BN) in block 0 of every layer; se.1 = ConvNormAct(C, C/16)
                         (conv .0 without bias, BN .1), se.2 = Conv2d(C/16, C) with bias

Outputs: eval -> list of 4 (B, num_classes) logits; train -> list of 4 [org, avg] pairs.  The reference's own forward never reaches the
MAP head for pool_type='map' (it calls head(x.mean(...)) and raises IndexError); the engine runs head([stem, layer1..4]), the
composition its checkpoint was trained with (registry tier "repaired").
"""
import torch.nn as nn

from .flat_model import FlatModel
from .map_convnext import _MAPHead
from .registry import register_repaired_model, reject_gram_fp64

__all__ = ['MAP_ResNet']

NBLOCK = (3, 4, 6, 3)
CHANNELS = (64, 128, 256, 256)       # bottleneck widths; outputs are 4x
STRIDES = (1, 2, 2, 2)
STEM_CH = 64
SE_R = 16


def _cna(cin, cout, k, stride=1):
    """ConvNormAct (map_resnet.py:21-28): conv .0 (no bias), BatchNorm .1; the GELU at .2 holds nothing"""
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, k // 2, bias=False), nn.BatchNorm2d(cout))


class _SE(nn.Module):
    """SEUnit (:31-41): .0 AdaptiveAvgPool2d (no parameters), .1 ConvNormAct(C, C/16, 1), .2 Conv2d(C/16, C, 1, bias)"""

    def __init__(self, c):
        super().__init__()
        self.add_module('0', nn.Identity())
        self.add_module('1', _cna(c, c // SE_R, 1))
        self.add_module('2', nn.Conv2d(c // SE_R, c, 1, bias=True))


class _Bottleneck(nn.Module):
    """BottleNeck (:44-67): registration order conv1, conv2, conv3, downsample, se"""

    def __init__(self, cin, width, stride, downsample):
        super().__init__()
        cout = width * 4
        self.conv1 = _cna(cin, width, 1)
        self.conv2 = _cna(width, width, 3, stride)
        self.conv3 = _cna(width, cout, 1)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))
        self.se = _SE(cout)


class MAP_ResNet(FlatModel):
    def __init__(self, num_classes=1000, drop_path_rate=0., drop=0., head_drop=0.05, head_attn_drop=0.05, math_mode=None, **kwargs):
        """head_drop / head_attn_drop: the dropout probabilities CABlock hard-codes (map.py:149) -- exposed so that parity tests can switch
        the masks off.  drop: MAPHead's dropout on the pooled org tokens (map.py:523-524); only 0 is on the hot path"""
        super().__init__()
        if drop:
            raise NotImplementedError('map_resnet50: drop > 0 (MAPHead dropout on the org tokens) is not on the HIP path')
        for k in ('avg_down', 'stem_type', 'pool_type'):
            if k in kwargs and kwargs[k] not in (False, 'deep', 'map'):
                raise NotImplementedError(f'map_resnet50: {k}={kwargs[k]!r} is not on the HIP path (only avg_down=False, stem_type="deep", '
                                          'pool_type="map")')
        self.num_classes = num_classes
        self.drop_path_rate = drop_path_rate
        channels = [STEM_CH] + [c * 4 for c in CHANNELS]
        L = 384
        self.cfg = dict(family='map_resnet', num_classes=num_classes, drop_path_rate=drop_path_rate, nblock=NBLOCK, widths=CHANNELS,
                        strides=STRIDES, stem_ch=STEM_CH, se_r=SE_R,
                        # MAPHead arguments of MAP_ResNet (:247-256) + the MAPHead defaults it keeps (attn_drop 0.05, bp_groups 1)
                        last_dim=L, n_groups=4, n_tokens=4, gram_group=32, bp_dim=L, bp_groups=1, gram_dim=L, ca_dim=384, num_heads=12,
                        mlp_ratio=4, mlp_groups=2, multi_scale_level=3, head_drop=head_drop, head_attn_drop=head_attn_drop,
                        self_distill_token=True, head_fn='norm', interactive=True, channels=tuple(channels))
        self.stem = nn.Sequential(_cna(3, 64, 3, 2), _cna(64, 64, 3), _cna(64, STEM_CH, 3))
        self.head = _MAPHead(self.cfg, channels)
        cin = STEM_CH
        for i, (n, w, s) in enumerate(zip(NBLOCK, CHANNELS, STRIDES)):
            blocks = []
            for j in range(n):
                blocks.append(_Bottleneck(cin, w, s if j == 0 else 1, j == 0 and (cin != 4 * w or s != 1)))
                cin = 4 * w
            setattr(self, f'layer{i + 1}', nn.Sequential(*blocks))
        self.math_mode = math_mode

    def make_engine(self, batch, training, mode):
        from .engine_resnet import ResNetEngine
        return ResNetEngine(self, batch, training, mode)

    def forward(self, x, pre_logits=False):
        """eval: list of 4 logits; train: list of 4 [org_out, avg_out] (map.py:519-537)"""
        assert not pre_logits, 'pre_logits is not on the hot path'
        outs = super().forward(x)
        if not self.training:
            return outs
        K = self.cfg['n_groups']
        return [[outs[k], outs[K + k]] for k in range(K)]


@register_repaired_model
def map_resnet50(pretrained=False, **kwargs):
    """map_resnet.py:318-333 (pretrained=True there downloads a checkpoint: here it raises).  Repaired tier: the reference's forward
    fails for this name; the engine runs the MAP head on [stem, layer1..4]"""
    reject_gram_fp64('map_resnet50', kwargs)
    for k in ('pretrained_cfg', 'pretrained_cfg_overlay', 'in_22k', 'drop_rate', 'drop_block_rate', 'global_pool', 'bn_momentum', 'bn_eps'):
        kwargs.pop(k, None)
    if pretrained:
        raise RuntimeError('map_resnet50: pretrained weights need a network fetch (map_resnet.py:326-330); load a local file with '
                           'checkpoint_path= instead')
    return MAP_ResNet(**kwargs)
