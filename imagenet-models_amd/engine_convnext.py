"""ConvNeXtEngine: the map_convnext trunk (engine_map.FBConvNeXtTrunk: the ConvNeXt trunk under the FB parameter names) with the plain head of
/root/reference/MAP/models/map_convnext.py:111-115,134-140 -- global average pool (ga_spatial_sum), LayerNorm(1e-6), Linear
(ga_gemm, fp32 logits); backward: classifier weight gradient / dgrad, LayerNorm backward, ga_rows_bcast as the seed of stage 3."""
import torch

from .engine_base import EngineBase
from .engine_map import FBConvNeXtTrunk


class ConvNeXtEngine(FBConvNeXtTrunk, EngineBase):
    def _build(self):
        d = self.cfg['dims']
        B, F, dt, P = self.B, self.fwd, self.dt, self.P
        feats, taps, stage_in, x_stem = self._build_trunk()
        x3, res = feats[3]
        HW, C = res * res, d[3]
        hd = self.hd = dict(pool=self.act('head.pool', (B, C)), y=self.act('head.y', (B, C)), mean=self.act('head.mean', (B,), torch.float32),
                            rstd=self.act('head.rstd', (B,), torch.float32))
        pool32 = self.tmp('head.pool32', (B, C), torch.float32)            # ga_spatial_sum reduces into fp32
        F.spatial_sum(x3, None, pool32, B, HW, C, 1.0 / HW, dt, label='head.pool')
        F.cast_from_f32(pool32, hd['pool'], B * C, dt, label='head.pool.cast')
        F.layernorm_fwd(hd['pool'], P['norm.weight'], P['norm.bias'], hd['y'], hd['mean'], hd['rstd'], B, C, 1e-6, dt, label='head.ln')
        self._linear_head_fwd(hd['y'], 'head.', C, 'head.fc')
        if self.training:
            Bk = self.bwd
            dy = self._linear_head_bwd(hd['y'], 'head.', C, 'head.dy')
            dpool = self.tmp('head.dpool', (B, C))
            Bk.layernorm_bwd(dy, hd['pool'], hd['mean'], hd['rstd'], P['norm.weight'], None, dpool, self.grad('norm.weight'),
                             self.grad('norm.bias'), B, C, False, dt, label='head.lnb')
            seed3 = self.buf('head.seed3', (B * HW, C))
            Bk.rows_bcast(dpool, seed3, B, HW, C, 1.0 / HW, dt, label='head.poolb')
            self._seal('heads', 'head.', 'norm.', flush=None)       # nothing deferred, the classifier's weight gradient joined by the range's end
            self._build_trunk_backward({3: seed3, 2: None, 1: None, 0: None}, [], [], feats, stage_in)
