"""MobileNetEngine: launch plans of MobileNetV1 (MAP/models/map_mobilenet.py:12-93) with its plain head or the MAP head.

  conv_bn stem (:18-23) .............. ga_nchw3_to_nhwc8 + ONE ga_gemm (GA_A_CONV3S2 gather, K = 72) with the BatchNorm column sums
                                       in its epilogue -> ga_bn_finalize -> ga_affine_act(ReLU)
  conv_dw (:25-37), 13 x ............. ga_dwconv3_fwd (stride 1 / 2, BatchNorm sums fused) -> finalize -> affine + ReLU -> pointwise
                                       ga_gemm (+ sums) -> finalize -> affine + ReLU
  plain head (:89-93) ................ ga_spatial_sum (global average pool) -> Linear (ga_gemm, fp32 logits); backward ga_rows_bcast
  MAP head (:67-83) .................. channel_convertor (1 x 1 conv -> BN -> ReLU, map.py:356-364) on the 7 x 7 map, then
                                       MAPHead._build_map_head (one group, four tokens, interactive attention, mlp_ratio 1)

Backward mirrors it: ga_bn_bwd_reduce / _apply with the stored ReLU output as the mask, the pointwise data gradient through the
transposed weight copy of ga_weight_prep, ga_wgrad for the pointwise and stem weights and ga_dwconv3_bwd_data / _bwd_weight for the
depthwise ones (weight gradients on the asynchronous lane).  The stem needs no input gradient.  Train-mode BatchNorm uses the batch
statistics and updates the running ones (momentum 0.1, eps 1e-5); eval-mode BatchNorm uses the running statistics.
"""
import torch

from . import ops  # noqa: F401
from .engine_base import EngineBase, pad8
from .engine_map import MAPHead
from .ops import A_CONV3S2


class MobileNetEngine(MAPHead, EngineBase):
    HP = 'fc.'

    def _drop_path_rates(self):
        return {}      # MobileNetV1 has no stochastic depth

    def _build(self):
        cfg = self.cfg
        B, T, F, dt, P = self.B, self.training, self.fwd, self.dt, self.P
        img = self.img
        assert self.sync_bn is None, 'SyncBatchNorm is not on the MobileNetV1 path'
        if T:
            F.zero(self.bn_pool, label='zero.bn_sums')
        # ---------------- stem: conv_bn(3, 32, 2) ----------------
        sp, C0 = 'layers.0.0.', cfg['stem_ch']
        H = (img - 1) // 2 + 1
        M = B * H * H
        W0 = self._image_pack8_stem(sp + '0', C0)
        st = self.stem = dict(c=self.act(sp + 'c', (M, C0)), bn=self._bn_bufs(sp + '1.', C0), a=self.act(sp + 'a', (M, C0)), M=M, C=C0)
        F.gemm(self.x8, W0, st['c'], M, C0, 72, dt, a_kind=A_CONV3S2, a_dims=(img, img, 8), colsum=st['bn']['s'] if T else None,
               colsumsq=st['bn']['q'] if T else None, label=sp + 'conv')
        self._bn_finalize(sp + '1.', st['bn'], M, C0)
        F.affine_act(st['c'], st['bn']['scale'], st['bn']['shift'], None, st['a'], M, C0, True, dt, label=sp + 'bn')
        # ---------------- the 13 conv_dw layers ----------------
        x, C = st['a'], C0
        self.units = []          # per stage: the conv_dw layers' saved tensors
        feats = []
        for i, stage in enumerate(cfg['stages']):
            us = []
            for j, (cin, cout, s) in enumerate(stage):
                assert cin == C
                u = self._conv_dw_fwd(f'layers.{i}.{j + (1 if i == 0 else 0)}.', x, H, cin, cout, s)
                us.append(u)
                x, H, C = u['a'], u['Ho'], cout
            self.units.append(us)
            feats.append((x, H, C))
        x4, H4, C4 = feats[-1]
        M4 = B * H4 * H4
        # ---------------- head ----------------
        if cfg['use_map']:
            self.xh = self._conv1x1_bn_act_fwd(x4, M4, C4, self.HP + 'mmcap.channel_convertor.', 'relu')
            self._build_map_head(self.xh, M4, H4)
        else:
            self.drop, self.G, self.sdt = None, 1, False         # the plain Linear: one group of logits, no dropout, no mean token
            pool32 = self.tmp('head.pool32', (B, C4), torch.float32)         # ga_spatial_sum reduces into fp32
            self.pool = self.act('head.pool', (B, C4))
            F.spatial_sum(x4, None, pool32, B, H4 * H4, C4, 1.0 / (H4 * H4), dt, label='fc.pool')
            F.cast_from_f32(pool32, self.pool, B * C4, dt, label='fc.pool.cast')
            self._linear_head_fwd(self.pool, 'fc.2.', C4, 'fc.2')
        if T:
            self._build_mobilenet_backward(x4, M4, H4, C4)

    def _conv_dw_fwd(self, pre, x, H, cin, cout, s):
        """conv_dw (map_mobilenet.py:25-37): depthwise 3 x 3 / s -> BN -> ReLU -> 1 x 1 -> BN -> ReLU"""
        B, T, F, dt, P = self.B, self.training, self.fwd, self.dt, self.P
        Ho = (H - 1) // s + 1
        Mo = B * Ho * Ho
        w9 = P[pre + '0.weight']           # (cin, 1, 3, 3) fp32 = [cin][9], read by the kernel as it is
        assert w9.is_contiguous() and w9.data_ptr() % 16 == 0, 'the depthwise weight must be 16-byte aligned in the flat buffer'
        u = dict(pre=pre, x=x, H=H, Ho=Ho, Mo=Mo, cin=cin, cout=cout, s=s)
        u['d'], u['bn1'], u['da'] = self.act(pre + 'd', (Mo, cin)), self._bn_bufs(pre + '1.', cin), self.act(pre + 'da', (Mo, cin))
        F.dwconv3_fwd(x, w9, u['d'], B, H, H, cin, s, dt, colsum=u['bn1']['s'] if T else None, colsumsq=u['bn1']['q'] if T else None,
                      label=pre + 'dw')
        self._bn_finalize(pre + '1.', u['bn1'], Mo, cin)
        F.affine_act(u['d'], u['bn1']['scale'], u['bn1']['shift'], None, u['da'], Mo, cin, True, dt, label=pre + 'bn1')
        Wp = self._w_plain(pre + '3.weight', cout, cin, 1, 1)
        u['p'], u['bn2'], u['a'] = self.act(pre + 'p', (Mo, cout)), self._bn_bufs(pre + '4.', cout), self.act(pre + 'a', (Mo, cout))
        F.gemm(u['da'], Wp, u['p'], Mo, cout, cin, dt, ldb=pad8(cin), colsum=u['bn2']['s'] if T else None,
               colsumsq=u['bn2']['q'] if T else None, label=pre + 'pw')
        self._bn_finalize(pre + '4.', u['bn2'], Mo, cout)
        F.affine_act(u['p'], u['bn2']['scale'], u['bn2']['shift'], None, u['a'], Mo, cout, True, dt, label=pre + 'bn2')
        return u

    # ------------------------------------------------------------------------------------------
    def _build_mobilenet_backward(self, x4, M4, H4, C4):
        Bk, B, dt, P, cfg = self.bwd, self.B, self.dt, self.P, self.cfg
        if cfg['use_map']:
            dy = self._build_head_backward(self.xh, M4)      # zeroes the arena, marks 'heads'; the gradient wrt the last map
        else:
            Bk.zero(self.arena, label='zero.arena')
            dpool = self._linear_head_bwd(self.pool, 'fc.2.', C4, 'head.dpool')
            dy = self.buf('head.seed', (M4, C4))
            Bk.rows_bcast(dpool, dy, B, H4 * H4, C4, 1.0 / (H4 * H4), dt, label='fc.poolb')
            self._seal('heads', 'fc.', flush='heads.')
        # input gradients ping-pong between two buffers per shape; what the asynchronous weight gradients read (the gradients
        # behind the BatchNorms) is kept per layer, so no later launch of the main lane overwrites it
        flip = 0
        for i in range(len(self.units) - 1, -1, -1):
            for u in reversed(self.units[i]):
                flip ^= 1
                dy = self._conv_dw_bwd(u, dy, self.tmp(f'dx{flip}', (B * u['H'] * u['H'], u['cin'])))
            if i > 0:
                self._seal(f'stage{i}', f'layers.{i}.', flush=f'stage{i}.')
        # stem: weight gradient only
        st, sp = self.stem, 'layers.0.0.'
        dc = self.buf(sp + 'dc', (st['M'], st['C']))
        self._bn_bwd(sp + '1.', st['bn'], dy, st['a'], st['c'], dc, st['M'], st['C'])
        G0 = self.gbuf((st['C'], 72))
        with self._wlane():
            Bk.wgrad(dc, self.x8, G0, st['M'], st['C'], 72, dt, x_kind=A_CONV3S2, x_dims=(self.img, self.img, 8), label=sp + 'conv.wg')
            Bk.convw_unpack_grad(G0, self.grad(sp + '0.weight'), st['C'], 3, 9, 8, 72, label=sp + 'conv.unf')   # same lane: after the wgrad

    def _conv_dw_bwd(self, u, dy, dx):
        Bk, B, dt, P = self.bwd, self.B, self.dt, self.P
        pre, Mo, cin, cout, s, H = u['pre'], u['Mo'], u['cin'], u['cout'], u['s'], u['H']
        dp = self.buf(pre + 'dp', (Mo, cout))
        self._bn_bwd(pre + '4.', u['bn2'], dy, u['a'], u['p'], dp, Mo, cout)
        with self._wlane():
            Bk.wgrad(dp, u['da'], self.grad(pre + '3.weight'), Mo, cout, cin, dt, label=pre + 'pw.wg')
        dda = self.tmp('dda', (Mo, cin))
        Bk.gemm(dp, self.W[pre + '3.weight.T'], dda, Mo, cin, cout, dt, ldb=pad8(cout), label=pre + 'pw.dg')
        dd = self.buf(pre + 'dd', (Mo, cin))
        self._bn_bwd(pre + '1.', u['bn1'], dda, u['da'], u['d'], dd, Mo, cin)
        with self._wlane():
            Bk.dwconv3_bwd_weight(dd, u['x'], self.grad(pre + '0.weight'), B, H, H, cin, s, dt, label=pre + 'dw.wg')
        Bk.dwconv3_bwd_data(dd, P[pre + '0.weight'], dx, B, H, H, cin, s, dt, label=pre + 'dw.dg')
        return dx
