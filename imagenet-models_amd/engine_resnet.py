"""ResNetEngine: launch plans of MAP-ResNet50 (MAP/models/map_resnet.py:200-340, its MAPHead from map.py) for a fixed
(batch, train|eval, math mode).

  deep stem (:217-221) ................ ga_nchw3_to_nhwc8 + ga_gemm (GA_A_CONV3S2 gather, K = 72), then two GA_A_CONV3 GEMMs
                                        (K = 576); each with the BatchNorm column sums in its epilogue -> ga_bn_finalize ->
                                        ga_bn_gelu_fwd (BatchNorm-apply + GELU in one pass)
  max_pool (:225) ..................... ga_maxpool3s2_fwd (uint8 window index kept for the backward)
  BottleNeck + SEUnit (:31-67), 16 x .. conv1 1 x 1 GEMM -> BN + GELU; conv2 3 x 3 GEMM (GA_A_CONV3, or GA_A_CONV3S2 on the
                                        stride-2 blocks) -> BN + GELU; conv3 1 x 1 GEMM -> BN statistics only; ga_spatial_sum of the
                                        raw conv3 output -> ga_se_bn_fwd (pooled BN-3 output, conv, BatchNorm over the batch, GELU,
                                        conv + bias, sigmoid); downsample = ga_subsample2_fwd (stride 2) + 1 x 1 GEMM (+ sums);
                                        ga_se_residual_fwd: relu(res' + r * gate * bn3(conv3)) in one pass (BN-3 and the downsample
                                        BN applied inside it, r = the block's DropPath factors)
  MAPHead ............................. five maps resized to 14 x 14 (stem 112 mode 2 f = 8, layer1 f = 4, layer2 f = 2, layer3
                                        copy, layer4 mode 3) into one concat -> MAPHead._build_map_head

The reference's forward for pool_type='map' calls head(x.mean([-2, -1])) and raises; the engine runs
head([stem, layer1, layer2, layer3, layer4]), the composition the checkpoint was trained with.

Backward mirrors it: ga_se_residual_bwd_a (dm = dy * (y > 0) and the per-sample sums P1 / P2), ga_se_bn_bwd (SE parameter
gradients, the gradient of the pooled BN-3 output and BN-3's two sums), ga_se_residual_bwd_b (the conv3 output gradient),
ga_bn_gelu_bwd_reduce / _apply from the raw conv outputs, ga_wgrad for every conv weight on the asynchronous lane, the stride-2
data gradients through GA_A_NEIGH2 (conv2) and ga_subsample2_bwd (downsample), ga_maxpool3s2_bwd adding into the stem gradient of
the multi-scale branch.  DDP bucket marks after the head and after each layer.  SyncBatchNorm is not on this path.
"""
import torch

from . import ops  # noqa: F401
from .engine_base import EngineBase, pad8
from .engine_map import MAPHead
from .ops import A_CONV3, A_CONV3S2, A_NEIGH2, C_UNPATCH2


class ResNetEngine(MAPHead, EngineBase):
    def _drop_path_rates(self):
        """map_resnet.py:262-265: block k of 16 (in order) gets drop_path_rate * k / 16"""
        nb, rate = self.cfg['nblock'], self.cfg['drop_path_rate']
        n, k, out = sum(nb), 0, {}
        for i, cnt in enumerate(nb):
            for j in range(cnt):
                out[f'layer{i + 1}.{j}.'] = float(rate) * k / n
                k += 1
        return out

    # ------------------------------------------------------------------------------------------
    def _conv_bn_gelu(self, pre, c, M, C, gemm):
        """ConvNormAct with GELU: gemm(colsum, colsumsq) writes the raw conv output c; returns (bn buffers, activation)"""
        T, F, dt = self.training, self.fwd, self.dt
        bn = self._bn_bufs(pre + '1.', C)
        gemm(bn['s'] if T else None, bn['q'] if T else None)
        self._bn_finalize(pre + '1.', bn, M, C)
        a = self.act(pre + 'a', (M, C))
        F.bn_gelu_fwd(c, bn['scale'], bn['shift'], a, M, C, dt, label=pre + 'bngelu')
        return bn, a

    def _bn_gelu_bwd(self, pre, bn, da, c, dc, M, C):
        Bk = self.bwd
        s1, s2 = self.gbuf((C,)), self.gbuf((C,))
        Bk.bn_gelu_bwd_reduce(da, c, bn['scale'], bn['shift'], bn['mean'], bn['rstd'], s1, s2, M, C, self.dt, label=pre + 'bngr')
        Bk.bn_gelu_bwd_apply(da, c, bn['scale'], bn['shift'], bn['mean'], bn['rstd'], self.P[pre + '1.weight'], s1, s2, M, dc, M, C, self.dt,
                             label=pre + 'bnga')
        Bk.axpy_f32(self.grad(pre + '1.weight'), s2, 1.0, C)
        Bk.axpy_f32(self.grad(pre + '1.bias'), s1, 1.0, C)

    def _build(self):
        cfg = self.cfg
        B, T, F, dt, P = self.B, self.training, self.fwd, self.dt, self.P
        img = self.img
        NC = cfg['num_classes']
        assert NC % 8 == 0, 'num_classes must be a multiple of 8 (pad the classifier)'
        assert self.sync_bn is None, 'SyncBatchNorm is not on the MAP-ResNet50 path'
        if T:
            F.zero(self.bn_pool, label='zero.bn_sums')
        # ---------------- deep stem ----------------
        H1 = img // 2
        M1 = B * H1 * H1
        C0 = cfg['stem_ch']
        W0 = self._image_pack8_stem('stem.0.0', 64)
        S = self.stem = {}
        S['c0'] = self.act('stem.0.c', (M1, 64))
        S['bn0'], S['a0'] = self._conv_bn_gelu('stem.0.', S['c0'], M1, 64, lambda s, q: F.gemm(
            self.x8, W0, S['c0'], M1, 64, 72, dt, a_kind=A_CONV3S2, a_dims=(img, img, 8), colsum=s, colsumsq=q, label='stem.0.conv'))
        x = S['a0']
        for k, cout in ((1, 64), (2, C0)):
            sp = f'stem.{k}.'
            Wk = self._w_plain(sp + '0.weight', cout, 64, 3, 3, flip=True)
            c = S[f'c{k}'] = self.act(sp + 'c', (M1, cout))
            S[f'bn{k}'], S[f'a{k}'] = self._conv_bn_gelu(sp, c, M1, cout, lambda s, q, x=x, Wk=Wk, c=c, sp=sp: F.gemm(
                x, Wk, c, M1, cout, 9 * 64, dt, ldb=pad8(9 * 64), a_kind=A_CONV3, a_dims=(H1, H1, 64), colsum=s, colsumsq=q,
                label=sp + 'conv'))
            x = S[f'a{k}']
        x_stem = x
        # ---------------- max pool ----------------
        H = (H1 - 1) // 2 + 1
        xp = self.act('maxpool.y', (B * H * H, C0))
        S['idx'] = self.buf('maxpool.idx', (B * H * H, C0), torch.uint8) if T else None
        F.maxpool3s2_fwd(x_stem, xp, S['idx'], B, H1, H1, C0, dt, label='maxpool')
        S['Hp'] = H
        # ---------------- layers ----------------
        x, C = xp, C0
        self.layers, feats = [], []
        for i, (n, w, s) in enumerate(zip(cfg['nblock'], cfg['widths'], cfg['strides'])):
            us = []
            for j in range(n):
                u = self._bottleneck_fwd(f'layer{i + 1}.{j}.', x, H, C, w, s if j == 0 else 1, j == 0 and (C != 4 * w or s != 1))
                us.append(u)
                x, H, C = u['y'], u['Ho'], 4 * w
            self.layers.append(us)
            feats.append((x, H, C))
        # ---------------- MultiScale + MAP head ----------------
        Hc = 14
        M4 = B * Hc * Hc
        cat, ctot = self._ms_concat_fwd([(x_stem, H1, C0)] + feats, Hc)
        xh = self._multi_scale_conv_fwd(cat, M4, ctot)
        self._build_map_head(xh, M4, Hc)
        if T:
            self._build_resnet_backward(xh, M4)

    def _bottleneck_fwd(self, pre, x, H, cin, w, s, has_ds):
        B, T, F, dt, P, Bf = self.B, self.training, self.fwd, self.dt, self.P, self.Bf
        cout, R = 4 * w, 4 * w // self.cfg['se_r']
        Ho = (H - 1) // s + 1
        assert s == 1 or H % 2 == 0, 'stride-2 blocks need an even input size'
        Mi, Mo, HW = B * H * H, B * Ho * Ho, Ho * Ho
        u = dict(pre=pre, x=x, H=H, Ho=Ho, cin=cin, w=w, s=s, has_ds=has_ds, R=R)
        # conv1 1 x 1 -> BN -> GELU
        W1 = self._w_plain(pre + 'conv1.0.weight', w, cin, 1, 1)
        u['c1'] = self.act(pre + 'c1', (Mi, w))
        u['bn1'], u['a1'] = self._conv_bn_gelu(pre + 'conv1.', u['c1'], Mi, w, lambda a, b: F.gemm(
            x, W1, u['c1'], Mi, w, cin, dt, ldb=pad8(cin), colsum=a, colsumsq=b, label=pre + 'conv1'))
        # conv2 3 x 3 / s -> BN -> GELU
        u['c2'] = self.act(pre + 'c2', (Mo, w))
        if s == 1:
            W2 = self._w_plain(pre + 'conv2.0.weight', w, w, 3, 3, flip=True)
            kind = A_CONV3
        else:
            W2 = self._w_plain(pre + 'conv2.0.weight', w, w, 3, 3, need_T=False)
            kind = A_CONV3S2
            if T:
                u['Bt'] = self.buf('wD.' + pre + 'conv2', (4 * w, pad8(4 * w)))
                self.prep.conv3s2_dgrad_prep(P[pre + 'conv2.0.weight'], u['Bt'], w, w, pad8(4 * w), dt, label='prep.' + pre + 'conv2.dgrad')
        u['bn2'], u['a2'] = self._conv_bn_gelu(pre + 'conv2.', u['c2'], Mo, w, lambda a, b: F.gemm(
            u['a1'], W2, u['c2'], Mo, w, 9 * w, dt, ldb=pad8(9 * w), a_kind=kind, a_dims=(H, H, w), colsum=a, colsumsq=b,
            label=pre + 'conv2'))
        # conv3 1 x 1 -> BN statistics (applied inside the SE / residual kernels)
        W3 = self._w_plain(pre + 'conv3.0.weight', cout, w, 1, 1)
        u['c3'], u['bn3'] = self.act(pre + 'c3', (Mo, cout)), self._bn_bufs(pre + 'conv3.1.', cout)
        F.gemm(u['a2'], W3, u['c3'], Mo, cout, w, dt, ldb=pad8(w), colsum=u['bn3']['s'] if T else None,
               colsumsq=u['bn3']['q'] if T else None, label=pre + 'conv3')
        self._bn_finalize(pre + 'conv3.1.', u['bn3'], Mo, cout)
        # SE
        sp = pre + 'se.'
        u['S'] = self.act(sp + 'S', (B, cout), torch.float32)
        F.spatial_sum(u['c3'], None, u['S'], B, HW, cout, 1.0, dt, label=sp + 'sum')
        for k, shape in (('hpre', (B, R)), ('h', (B, R)), ('mean', (R,)), ('rstd', (R,)), ('gate', (B, cout))):
            u['se_' + k] = self.act(sp + k, shape, torch.float32)
        F.se_bn_fwd(u['S'], HW, u['bn3']['scale'], u['bn3']['shift'], P[sp + '1.0.weight'], P[sp + '1.1.weight'], P[sp + '1.1.bias'],
                    Bf[sp + '1.1.running_mean'], Bf[sp + '1.1.running_var'], P[sp + '2.weight'], P[sp + '2.bias'], u['se_hpre'], u['se_mean'],
                    u['se_rstd'], u['se_h'], u['se_gate'], B, cout, R, T, label=sp + 'mlp')
        # shortcut
        rsc = rsh = None
        res = x
        if has_ds:
            dp = pre + 'downsample.'
            xs = x
            if s == 2:
                xs = self.act(dp + 'xs', (Mo, cin))
                F.subsample2_fwd(x, xs, B, H, H, cin, dt, label=dp + 'sub')
            u['xs'] = xs
            Wd = self._w_plain(dp + '0.weight', cout, cin, 1, 1)
            u['cd'], u['bnd'] = self.act(dp + 'c', (Mo, cout)), self._bn_bufs(dp + '1.', cout)
            F.gemm(xs, Wd, u['cd'], Mo, cout, cin, dt, ldb=pad8(cin), colsum=u['bnd']['s'] if T else None,
                   colsumsq=u['bnd']['q'] if T else None, label=dp + 'conv')
            self._bn_finalize(dp + '1.', u['bnd'], Mo, cout)
            res, rsc, rsh = u['cd'], u['bnd']['scale'], u['bnd']['shift']
        else:
            assert cin == cout and s == 1
        u['r'] = self.dp_scale.get(pre) if T else None
        u['y'] = self.act(pre + 'y', (Mo, cout))
        F.se_residual_fwd(u['c3'], u['bn3']['scale'], u['bn3']['shift'], u['se_gate'], u['r'], res, rsc, rsh, u['y'], B, HW, cout, dt,
                          label=pre + 'tail')
        return u

    # ------------------------------------------------------------------------------------------
    def _build_resnet_backward(self, xh, M4):
        Bk, B, dt = self.bwd, self.B, self.dt
        seeds = self._ms_concat_bwd(self._build_head_backward(xh, M4))      # (the head backward zeroes the arena, marks 'heads')
        dy = seeds[4]
        for li in range(3, -1, -1):
            for u in reversed(self.layers[li]):
                dy = self._bottleneck_bwd(u, dy)
            if li > 0:
                M, C = dy.shape
                Bk.affine_act(dy, None, None, seeds[li], dy, M, C, False, dt, label=f'layer{li}.seed')
            self._seal(f'layer{li + 1}', f'layer{li + 1}.', flush=f'layer{li + 1}.')
        # max pool -> adds into the multi-scale gradient of the stem output
        S, C0, H1 = self.stem, self.cfg['stem_ch'], self.img // 2
        M1 = B * H1 * H1
        da = seeds[0]
        Bk.maxpool3s2_bwd(dy, S['idx'], da, B, H1, H1, C0, dt, accumulate=True, label='maxpool.b')
        # deep stem
        for k in (2, 1):
            sp = f'stem.{k}.'
            cin = 64
            dc = self.buf(sp + 'dc', (M1, S[f'c{k}'].shape[1]))
            self._bn_gelu_bwd(sp, S[f'bn{k}'], da, S[f'c{k}'], dc, M1, dc.shape[1])
            G = self.gbuf((dc.shape[1], 9 * cin))
            with self._wlane():
                Bk.wgrad(dc, S[f'a{k - 1}'], G, M1, dc.shape[1], 9 * cin, dt, x_kind=A_CONV3, x_dims=(H1, H1, cin), label=sp + 'wg')
            Bk.weight_unfold(G, 9 * cin, dc.shape[1], cin, 3, 3, dW=self.grad(sp + '0.weight'), label=sp + 'unf')
            dprev = self.tmp(f'stem.da{k}', (M1, cin))
            Bk.gemm(dc, self.W[sp + '0.weight.T'], dprev, M1, cin, 9 * dc.shape[1], dt, ldb=pad8(9 * dc.shape[1]), a_kind=A_CONV3,
                    a_dims=(H1, H1, dc.shape[1]), label=sp + 'dg')
            da = dprev
        dc0 = self.buf('stem.0.dc', (M1, 64))
        self._bn_gelu_bwd('stem.0.', S['bn0'], da, S['c0'], dc0, M1, 64)
        G0 = self.gbuf((64, 72))
        with self._wlane():
            Bk.wgrad(dc0, self.x8, G0, M1, 64, 72, dt, x_kind=A_CONV3S2, x_dims=(self.img, self.img, 8), label='stem.0.wg')
            Bk.convw_unpack_grad(G0, self.grad('stem.0.0.weight'), 64, 3, 9, 8, 72, label='stem.0.unf')   # same lane: after the wgrad

    def _bottleneck_bwd(self, u, dy):
        """dy: gradient of the block output; returns the gradient of its input"""
        Bk, B, dt, P, W = self.bwd, self.B, self.dt, self.P, self.W
        pre, H, Ho, cin, w, s, R = u['pre'], u['H'], u['Ho'], u['cin'], u['w'], u['s'], u['R']
        cout = 4 * w
        Mi, Mo, HW = B * H * H, B * Ho * Ho, Ho * Ho
        bn3, sp = u['bn3'], pre + 'se.'
        g3, b3 = P[pre + 'conv3.1.weight'], P[pre + 'conv3.1.bias']
        # tail pass A: dm = dy * (y > 0), P1 / P2
        dm = self.tmp('dm', (Mo, cout))
        P1, P2 = self.tmp('se.P1', (B, cout), torch.float32), self.tmp('se.P2', (B, cout), torch.float32)
        Bk.se_residual_bwd_a(dy, u['y'], u['c3'], bn3['mean'], bn3['rstd'], dm, P1, P2, B, HW, cout, dt, label=pre + 'tail.a')
        # SE backward + BN-3 sums
        dz, dh = self.tmp('se.dz', (B, cout), torch.float32), self.tmp('se.dh', (B, R), torch.float32)
        dsp = self.tmp('se.ds', (B, cout), torch.float32)
        s1, s2 = self.gbuf((cout,)), self.gbuf((cout,))
        Bk.se_bn_bwd(P1, P2, u['r'], g3, b3, bn3['mean'], bn3['rstd'], u['S'], HW, bn3['scale'], bn3['shift'], P[sp + '1.0.weight'],
                     P[sp + '1.1.weight'], P[sp + '1.1.bias'], P[sp + '2.weight'], u['se_hpre'], u['se_mean'], u['se_rstd'], u['se_h'],
                     u['se_gate'], dz, dh, dsp, s1, s2, self.grad(sp + '1.0.weight'), self.grad(sp + '1.1.weight'),
                     self.grad(sp + '1.1.bias'), self.grad(sp + '2.weight'), self.grad(sp + '2.bias'), B, cout, R, label=sp + 'mlpb')
        Bk.axpy_f32(self.grad(pre + 'conv3.1.weight'), s2, 1.0, cout)
        Bk.axpy_f32(self.grad(pre + 'conv3.1.bias'), s1, 1.0, cout)
        # tail pass B: gradient of the raw conv3 output
        dc3 = self.buf(pre + 'dc3', (Mo, cout))
        Bk.se_residual_bwd_b(dm, u['c3'], bn3['mean'], bn3['rstd'], g3, u['se_gate'], u['r'], dsp, s1, s2, dc3, B, HW, cout, dt,
                             label=pre + 'tail.b')
        # conv3
        with self._wlane():
            Bk.wgrad(dc3, u['a2'], self.grad(pre + 'conv3.0.weight'), Mo, cout, w, dt, label=pre + 'conv3.wg')
        da2 = self.tmp('da2', (Mo, w))
        Bk.gemm(dc3, W[pre + 'conv3.0.weight.T'], da2, Mo, w, cout, dt, ldb=pad8(cout), label=pre + 'conv3.dg')
        # conv2
        dc2 = self.buf(pre + 'dc2', (Mo, w))
        self._bn_gelu_bwd(pre + 'conv2.', u['bn2'], da2, u['c2'], dc2, Mo, w)
        G = self.gbuf((w, 9 * w))
        with self._wlane():
            Bk.wgrad(dc2, u['a1'], G, Mo, w, 9 * w, dt, x_kind=A_CONV3 if s == 1 else A_CONV3S2, x_dims=(H, H, w), label=pre + 'conv2.wg')
        Bk.weight_unfold(G, 9 * w, w, w, 3, 3, dW=self.grad(pre + 'conv2.0.weight'), label=pre + 'conv2.unf')
        da1 = self.tmp('da1', (Mi, w))
        if s == 1:
            Bk.gemm(dc2, W[pre + 'conv2.0.weight.T'], da1, Mi, w, 9 * w, dt, ldb=pad8(9 * w), a_kind=A_CONV3, a_dims=(H, H, w),
                    label=pre + 'conv2.dg')
        else:
            Bk.gemm(dc2, u['Bt'], da1, Mo, 4 * w, 4 * w, dt, ldb=pad8(4 * w), a_kind=A_NEIGH2, a_dims=(Ho, Ho, w), c_kind=C_UNPATCH2,
                    c_dims=(H, H, w), label=pre + 'conv2.dg')
        # conv1
        dc1 = self.buf(pre + 'dc1', (Mi, w))
        self._bn_gelu_bwd(pre + 'conv1.', u['bn1'], da1, u['c1'], dc1, Mi, w)
        with self._wlane():
            Bk.wgrad(dc1, u['x'], self.grad(pre + 'conv1.0.weight'), Mi, w, cin, dt, label=pre + 'conv1.wg')
        dx = self.tmp('dx', (Mi, cin))
        W1T = W[pre + 'conv1.0.weight.T']
        if not u['has_ds']:
            Bk.gemm(dc1, W1T, dx, Mi, cin, w, dt, ldb=pad8(w), R=dm, ldr=cin, label=pre + 'conv1.dg')
            return dx
        dp = pre + 'downsample.'
        dcd = self.buf(dp + 'dc', (Mo, cout))
        self._bn_bwd(dp + '1.', u['bnd'], dm, None, u['cd'], dcd, Mo, cout)
        with self._wlane():
            Bk.wgrad(dcd, u['xs'], self.grad(dp + '0.weight'), Mo, cout, cin, dt, label=dp + 'wg')
        dxs = self.tmp('dxs', (Mo, cin))
        Bk.gemm(dcd, W[dp + '0.weight.T'], dxs, Mo, cin, cout, dt, ldb=pad8(cout), label=dp + 'dg')
        if s == 1:
            Bk.gemm(dc1, W1T, dx, Mi, cin, w, dt, ldb=pad8(w), R=dxs, ldr=cin, label=pre + 'conv1.dg')
        else:
            Bk.gemm(dc1, W1T, dx, Mi, cin, w, dt, ldb=pad8(w), label=pre + 'conv1.dg')
            Bk.subsample2_bwd(dxs, dx, B, H, H, cin, dt, accumulate=True, label=dp + 'subb')
        return dx
