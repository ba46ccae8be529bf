"""GAEngine: the launch plans of one GA_ConvNeXt = engine_base.EngineBase + the builders of this module:

  ConvNeXtTrunk ... stem + the four ConvNeXt stages, forward and backward (GA-ConvNeXt, MAP-ConvNeXt and the plain ConvNeXt);
  GAHeads ......... aggregation into the concat buffer, SE-Bottleneck, the five GA heads (GA-ConvNeXt, GA-CSWin), on the stacked
                    products and the GroupConvMlp of engine_heads.HeadStacks.

What is saved for backward per ConvNeXt block: xhat (LN output, no affine), rstd, h (pre-GELU hidden) and the
block output of fc1 as a = gelu(h) and g = gelu'(h) (both written by the fc1 epilogue), and the block output.

Reference semantics restated here: /root/reference/GA/ga_convnext.py:98-112 (block), :139-150 (stage + taps),
:294-318 (Bottleneck), :452-467 (get_gram), :153-248 (class attention block), :469-505 (forward).
"""
import os

import torch

from . import ops
from .engine_base import EngineBase, GAFunction, pad8  # noqa: F401  (GAFunction, pad8: this module's long-standing exports)
from .engine_heads import HeadStacks, Stacked
from .ops import (A_CONV3, A_PATCH2, A_STEM4_NCHW, ACT_GELU, ASYNC_LANE, C_UNPATCH2, GA_BF16)


def tap_indices(nblocks, naggre):
    """ga_convnext.py:141-147"""
    taps = []
    if nblocks > 5:
        for i in range(nblocks):
            if (i + 1) % (nblocks // (naggre + 1)) == 0 and len(taps) < naggre:
                taps.append(i)
    return taps


class ConvNeXtTrunk:
    """builder: stem + the four ConvNeXt stages on EngineBase's buffers and plans"""

    # parameter names of the ConvNeXt trunk: GA-ConvNeXt follows timm's ConvNeXt (ga_convnext.py:86-137,356-359), MAP-ConvNeXt
    # the FB one (map_convnext.py:16-83) -- same arithmetic, different module names
    # `stage`: the prefixes of everything whose gradient is final once stage i's backward (blocks, then its downsample) is recorded
    NAMES = dict(stem_conv='stem.0.', stem_ln='stem.1.', ds_ln='stages.{i}.downsample.0.', ds_conv='stages.{i}.downsample.1.',
                 block='stages.{i}.blocks.{j}.', dw='conv_dw.', fc1='mlp.fc1.', fc2='mlp.fc2.', stage=('stages.{i}.',))

    def _build_trunk(self):
        """stem + the four ConvNeXt stages; returns (feats [(x, res)], taps, stage_in [(x, H)], stem output)"""
        cfg, nm = self.cfg, self.NAMES
        d, dep = cfg['dims'], cfg['depths']
        B, T, F = self.B, self.training, self.fwd
        dt = self.dt
        S0 = self.img // 4
        # ---------------- stem ----------------
        M0 = B * S0 * S0
        if T:
            F.zero(self.bn_pool, label='zero.bn_sums')
        sc, sl = nm['stem_conv'], nm['stem_ln']
        Wst = self._w_plain(sc + 'weight', d[0], 3, 4, 4, stem=True, need_T=False)
        stem_pre = self.act('stem.pre', (M0, d[0]))
        self.x_placeholder = torch.zeros(8, device=self.dev)  # patched by set_input
        mean = self.act('stem.mean', (M0,), torch.float32)
        rstd = self.act('stem.rstd', (M0,), torch.float32)
        x = self.buf('stem.out', (M0, d[0]))
        # GA_ConvNeXt-trunk switches, read when the engine is built
        self.mlp_wg1 = os.environ.get('GAEXT_MLP_WG1', '1') != '0'     # fc1 weight gradient inside the fused MLP backward (C = 96)
        fwd_skew = int(os.environ.get('GAEXT_FWD_SKEW', '-1'))         # chain k+1 starts when chain k has passed this stage
        if dt == GA_BF16 and d[0] in (96, 128) and self.img % 4 == 0 and os.environ.get('GAEXT_STEM_FUSED', '1') != '0':
            # conv + bias + LayerNorm in one pass over the image (ga_stem4_ln_fwd): the input pointer is argument 0 of this call
            self.input_call = len(F.calls)
            F.stem4_ln_fwd(self.x_placeholder, Wst, Wst.shape[1], self.P[sc + 'bias'], self.P[sl + 'weight'], self.P[sl + 'bias'],
                           stem_pre, x, mean, rstd, B, self.img, self.img, d[0], 1e-6, label='stem.conv+ln')
        else:
            F.gemm(self.x_placeholder, Wst, stem_pre, M0, d[0], 48, dt, a_kind=A_STEM4_NCHW, a_dims=(self.img, self.img, 3),
                   bias=self.P[sc + 'bias'], label='stem.conv')
            self.input_desc = self._last_desc(F)
            F.layernorm_fwd(stem_pre, self.P[sl + 'weight'], self.P[sl + 'bias'], x, mean, rstd, M0, d[0], 1e-6, dt,
                            label='stem.ln')
        # ---------------- stages 0..3 ----------------
        # one pass per chain (batch part): with GAEXT_FWD_SPLIT > 1 the chains run on side streams; every pass names
        # the same full-batch buffers and records its own rows only
        x_stem = x
        chains = self._chains()
        skew_ev = None
        for ci, chain in enumerate(chains):
            self._chain = chain if len(chains) > 1 else None
            if self._chain is not None and skew_ev is not None:
                F.lane_wait(chain[0], skew_ev)       # start this chain when the previous one has passed stage fwd_skew
                skew_ev = None
            feats, taps = [], []
            x = x_stem
            res = S0
            stage_in = []
            for i in range(4):
                if i > 0:
                    Hp = res
                    res //= 2
                    Mi = B * res * res
                    Mp = B * Hp * Hp
                    pre = f'stages.{i}.downsample.'          # buffer names only
                    pln, pcv = nm['ds_ln'].format(i=i), nm['ds_conv'].format(i=i)
                    ln = self.act(pre + 'ln', (Mp, d[i - 1]))
                    mean = self.act(pre + 'mean', (Mp,), torch.float32)
                    rstd = self.act(pre + 'rstd', (Mp,), torch.float32)
                    Wd = self._w_plain(pcv + 'weight', d[i], d[i - 1], 2, 2)
                    xo = self.buf(pre + 'out', (Mi, d[i]))
                    for lane, r0, r1, b0, b1 in self._fsplits(Hp * Hp):
                        F.lane = lane
                        F.layernorm_fwd(x[r0:r1], self.P[pln + 'weight'], self.P[pln + 'bias'], ln[r0:r1], mean[r0:r1],
                                        rstd[r0:r1], r1 - r0, d[i - 1], 1e-6, dt, label=pre + 'ln')
                        F.gemm(ln[r0:r1], Wd, xo[r0 // 4:r1 // 4], (r1 - r0) // 4, d[i], 4 * d[i - 1], dt, a_kind=A_PATCH2,
                               a_dims=(Hp, Hp, d[i - 1]), bias=self.P[pcv + 'bias'], label=pre + 'conv')
                    F.lane = 0
                    stage_in.append((x, Hp))
                    x = xo
                tap_at = tap_indices(dep[i], cfg['naggre']) if i == 2 else []
                for j in range(dep[i]):
                    x = self._block_fwd(nm['block'].format(i=i, j=j), x, res, d[i])
                    if j in tap_at:
                        taps.append(x)
                feats.append((x, res))
                if self._chain is not None and i == fwd_skew and ci + 1 < len(chains):
                    skew_ev = F.lane_signal(chain[0])
        self._chain = None
        return feats, taps, stage_in, x_stem

    def _block_weights(self, pre, C):
        if pre + 'w49' in self.W:
            return
        P = self.P
        w49 = self.buf('w.' + pre + 'w49', (49, C), torch.float32)
        self.prep.transpose_f32(P[pre + self.NAMES['dw'] + 'weight'], w49, C, 49, label='prep.' + pre + 'w49')
        self.W[pre + 'w49'] = w49
        self._w_plain(pre + self.NAMES['fc1'] + 'weight', 4 * C, C, 1, 1, cs=P[pre + 'norm.weight'])
        b1e = self.buf('w.' + pre + 'b1e', (4 * C,), torch.float32)
        self.prep.bias_fold(P[pre + self.NAMES['fc1'] + 'weight'], P[pre + self.NAMES['fc1'] + 'bias'], None, P[pre + 'norm.bias'], b1e, 4 * C, C)
        self.W[pre + 'b1e'] = b1e
        self._w_plain(pre + self.NAMES['fc2'] + 'weight', C, 4 * C, 1, 1, rs=P[pre + 'gamma'])
        b2e = self.buf('w.' + pre + 'b2e', (C,), torch.float32)
        self.prep.bias_fold(None, P[pre + self.NAMES['fc2'] + 'bias'], P[pre + 'gamma'], None, b2e, C, 4 * C)
        self.W[pre + 'b2e'] = b2e

    # ------------------------------------------------------------------------------------------
    # ConvNeXt block
    # ------------------------------------------------------------------------------------------
    def _block_fwd(self, pre, x, res, C):
        assert C % 8 == 0
        F, dt, B = self.fwd, self.dt, self.B
        M = B * res * res
        self._block_weights(pre, C)
        W = self.W
        u = self.tmp('u', (M, C))
        xn = self.blk_act(pre + 'xn', (M, C))
        rstd = self.blk_act(pre + 'rstd', (M,), torch.float32)
        # fc1 stores a = gelu(h) and, when training, g = gelu'(h): backward never re-evaluates erf, and neither the
        # fc2 operand loader nor the wgrad loader has to (they used to, once per N tile)
        fused = self._mlp_fused(C)
        a = None if fused else self.blk_act(pre + 'a', (M, 4 * C))
        g = self.buf(pre + 'g', (M, 4 * C)) if (self.training and not fused) else None
        y = self.buf(pre + 'y', (M, C))
        dp = self.dp_scale.get(pre)
        cur = F.lane      # inside a head's lane: one chain in that lane
        for lane, r0, r1, b0, b1 in (self._fsplits(res * res) if cur == 0 else [(cur, 0, M, 0, B)]):
            F.lane = lane
            F.dwconv7_fwd(x[r0:r1], W[pre + 'w49'], self.P[pre + self.NAMES['dw'] + 'bias'], u[r0:r1], b1 - b0, res, res, C, dt,
                          label=pre + 'dw')
            F.layernorm_fwd(u[r0:r1], None, None, xn[r0:r1], None, rstd[r0:r1], r1 - r0, C, 1e-6, dt, label=pre + 'ln')
            if fused:     # fc1 -> GELU -> fc2 in one kernel: the [M, 4C] hidden activation never reaches HBM (csrc/mlp.hip)
                F.mlp_fwd(xn[r0:r1], W[pre + self.NAMES['fc1'] + 'weight'], W[pre + 'b1e'], W[pre + self.NAMES['fc2'] + 'weight'],
                          W[pre + 'b2e'], y[r0:r1], r1 - r0, C, dt, R=x[r0:r1], rowscale=dp[b0:b1] if dp is not None else None,
                          rows_per_scale=res * res, label=pre + 'mlp')
                continue
            F.gemm(xn[r0:r1], W[pre + self.NAMES['fc1'] + 'weight'], a[r0:r1], r1 - r0, 4 * C, C, dt, bias=W[pre + 'b1e'], act=ACT_GELU,
                   C2=g[r0:r1] if g is not None else None, c2_mode=2 if g is not None else 0, label=pre + 'fc1')
            F.gemm(a[r0:r1], W[pre + self.NAMES['fc2'] + 'weight'], y[r0:r1], r1 - r0, C, 4 * C, dt, bias=W[pre + 'b2e'],
                   rowscale=dp[b0:b1] if dp is not None else None, rows_per_scale=res * res, R=x[r0:r1], ldr=C,
                   label=pre + 'fc2')
        F.lane = cur
        self.blocks[pre] = dict(x=x, xn=xn, rstd=rstd, a=a, g=g, y=y, res=res, C=C, fused=fused)
        return y

    def _mlp_fused(self, C):
        """the fused MLP bodies (ga_mlp_fwd / ga_mlp_bwd) replace the fc1 / fc2 / dgrad2 / dgrad1 launches where they win: bf16 and
        the channel counts in GA_FUSED_MLP (default 96: stage 0, where the unfused GEMMs run at the HBM rate; measured at
        B = 256: forward 0.66 -> 0.27 ms, backward pair 0.45 -> 0.54 ms per block; at C = 192 the backward loses more than the
        forward gains)"""
        allowed = [int(v) for v in os.environ.get('GA_FUSED_MLP', '96').split(',') if v.strip()]
        if not self.training and 'GA_FUSED_MLP' not in os.environ:
            allowed.append(192)          # forward only: the fused body wins at C = 192 too (0.36 -> 0.29 ms per block)
        return C in allowed and ops.mlp_supported(C, 4 * C, self.dt)

    def _block_bwd(self, pre, dy, dx, next_pre=None):
        """dy: grad wrt the block output; writes dx (a different buffer) = grad wrt the block input.  next_pre: the block
        whose backward follows and takes dx as its dy unchanged -- its DropPath-scaled copy is written here, by the
        depthwise backward-data kernel that produces dx, instead of by a separate pass"""
        Bk, dt, B, P, W = self.bwd, self.dt, self.B, self.P, self.W
        b = self.blocks[pre]
        res, C = b['res'], b['C']
        M = B * res * res
        dp = self.dp_scale.get(pre)
        dyz = dy
        par, dz_tag = '', 'dyz'
        # the weight-gradient launches read only what the dgrad chain has already produced and nothing on the chain
        # reads their results: on the trunk they go to the plan's asynchronous lane and fill the tails of the chain's
        # launches (the next block joins before it overwrites dyz / dh / du)
        side = self._wgrad_window()
        if side:
            # two sets of the transients the weight-gradient launches read (dh, du; three of dyz; the caller rotates
            # three dx buffers): this block only has to wait for the asynchronous launches of the block before the
            # previous one
            par = str(self._bwd_seq & 1)
            dz_tag = f'dyz{self._bwd_seq % 3}'
        if dp is not None:
            if pre in self._pre_dyz:
                dyz = self._pre_dyz.pop(pre)          # written by the previous block's depthwise backward
            else:
                dyz = self.tmp(dz_tag, (M, C))
                Bk.rowscale(dy, dp, dyz, M * C, res * res * C, dt, label=pre + 'dp')
        wl = ASYNC_LANE if side else Bk.lane
        ml = Bk.lane
        G2, gb2 = self.gbuf((C, 4 * C)), self.gbuf((C,))
        gb1 = self.gbuf((4 * C,))
        G1 = self.gbuf((4 * C, C))
        g = self.tmp('g', (M, C))
        if b['fused'] and self.mlp_wg1 and ops.mlp_bwd_wgrad_supported(C, 4 * C, dt):
            # as below, and the fc1 weight gradient (G1, gb1) is accumulated by the same kernel from the dh / xn tiles it holds in
            # LDS: dh is neither stored nor read back and the wg1 launch is gone (csrc/mlp.hip).  The workgroups' fp32 partials
            # are written by the kernel and summed into G1 / gb1 by the reduce launch that the same call puts right behind it on
            # this chain lane; the next block's mlp_bwd, later on the same lane, writes them again -- nothing on another lane
            # ever reads them (the parity suffix follows dh / du all the same)
            a = self.tmp('a' + par, (M, 4 * C))
            part = self.tmp('mlpwg' + par, (ops.mlp_bwd_partials(M, C, dt) // 4,), torch.float32)
            Bk.mlp_bwd(b['xn'], dyz, W[pre + self.NAMES['fc1'] + 'weight'], W[pre + 'b1e'], W[pre + self.NAMES['fc2'] + 'weight.T'],
                       W[pre + self.NAMES['fc1'] + 'weight.T'], a, None, g, M, C, dt, dW1=G1, db1=gb1, partials=part, label=pre + 'mlpb')
            Bk.lane = wl
            Bk.wgrad(dyz, a, G2, M, C, 4 * C, dt, dbias=gb2, label=pre + 'wg2')
            Bk.lane = ml
        elif b['fused']:
            # hidden pre-activation re-computed; a / dh written once for the two weight-gradient GEMMs, dh stays on chip for dgrad1
            a = self.tmp('a' + par, (M, 4 * C))
            dh = self.tmp('dh' + par, (M, 4 * C))
            Bk.mlp_bwd(b['xn'], dyz, W[pre + self.NAMES['fc1'] + 'weight'], W[pre + 'b1e'], W[pre + self.NAMES['fc2'] + 'weight.T'],
                       W[pre + self.NAMES['fc1'] + 'weight.T'], a, dh, g, M, C, dt, label=pre + 'mlpb')
            Bk.lane = wl
            Bk.wgrad(dyz, a, G2, M, C, 4 * C, dt, dbias=gb2, label=pre + 'wg2')
            Bk.wgrad(dh, b['xn'], G1, M, 4 * C, C, dt, dbias=gb1, label=pre + 'wg1')
            Bk.lane = ml
        else:
            dh = self.tmp('dh' + par, (M, 4 * C))
            Bk.lane = wl
            Bk.wgrad(dyz, b['a'], G2, M, C, 4 * C, dt, dbias=gb2, label=pre + 'wg2')
            Bk.lane = ml
            Bk.gemm(dyz, W[pre + self.NAMES['fc2'] + 'weight.T'], dh, M, 4 * C, C, dt, H=b['g'], ldh=4 * C, h_is_deriv=True, colsum=gb1,
                    label=pre + 'dg2')
            Bk.lane = wl
            Bk.wgrad(dh, b['xn'], G1, M, 4 * C, C, dt, label=pre + 'wg1')
            Bk.lane = ml
            Bk.gemm(dh, W[pre + self.NAMES['fc1'] + 'weight.T'], g, M, C, 4 * C, dt, label=pre + 'dg1')
        du = self.tmp('du' + par, (M, C))
        Bk.layernorm_bwd(g, b['xn'], None, b['rstd'], None, None, du, None, None, M, C, True, dt, label=pre + 'lnb')
        dw49 = self.gbuf((49, C))
        Bk.lane = wl
        Bk.dwconv7_bwd_weight(du, b['x'], dw49, self.grad(pre + self.NAMES['dw'] + 'bias'), B, res, res, C, dt, label=pre + 'dww')
        Bk.lane = ml
        self._wgrad_window_mark(side)
        dx2 = dp_next = None
        if next_pre is not None and self.fuse_dp:
            dp_next = self.dp_scale.get(next_pre)
            if dp_next is not None:
                nxt = f'dyz{(self._bwd_seq + 1) % 3}' if side else 'dyz'
                dx2 = self._pre_dyz[next_pre] = self.tmp(nxt, (M, C))
        Bk.dwconv7_bwd_data(du, W[pre + 'w49'], dy, dx, B, res, res, C, dt, dx2=dx2, scale2=dp_next, label=pre + 'dwd')
        Bk.weight_unfold(G2, 4 * C, C, 4 * C, gb=gb2, W=P[pre + self.NAMES['fc2'] + 'weight'], b=P[pre + self.NAMES['fc2'] + 'bias'],
                         rs=P[pre + 'gamma'], dW=self.grad(pre + self.NAMES['fc2'] + 'weight'), db=self.grad(pre + self.NAMES['fc2'] + 'bias'),
                         d_rs=self.grad(pre + 'gamma'), label=pre + 'unf2')
        Bk.weight_unfold(G1, C, 4 * C, C, gb=gb1, W=P[pre + self.NAMES['fc1'] + 'weight'], b=P[pre + self.NAMES['fc1'] + 'bias'],
                         cs=P[pre + 'norm.weight'], v=P[pre + 'norm.bias'], dW=self.grad(pre + self.NAMES['fc1'] + 'weight'),
                         db=self.grad(pre + self.NAMES['fc1'] + 'bias'), d_cs=self.grad(pre + 'norm.weight'),
                         d_v=self.grad(pre + 'norm.bias'), label=pre + 'unf1')
        Bk.transpose_f32(dw49, self.grad(pre + self.NAMES['dw'] + 'weight'), 49, C, accumulate=True, label=pre + 'unfdw')

    def _build_trunk_backward(self, seed, d_taps, tap_at, feats, stage_in, stem_seed=None):
        """backward of _build_trunk: seed[i] = gradient of stage i's output from the aggregation, d_taps those of the stage-2
        taps (after blocks tap_at), stem_seed that of the stem output (MAP: the stem output is a feature map itself)"""
        Bk, dt, B, P, W, cfg, nm = self.bwd, self.dt, self.B, self.P, self.W, self.cfg, self.NAMES
        d, dep = cfg['dims'], cfg['depths']
        dy = seed[3]
        for i in (3, 2, 1, 0):
            res = feats[i][1]
            Mi = B * res * res
            pp = [self.tmp(f'dxA{i}', (Mi, d[i])), self.tmp(f'dxB{i}', (Mi, d[i])), self.tmp(f'dxC{i}', (Mi, d[i]))]
            turn = 0
            for j in reversed(range(dep[i])):
                if i == 2 and j in tap_at:
                    dtap = d_taps[tap_at.index(j)]
                    Bk.affine_act(dy, None, None, dtap, dy, Mi, d[i], False, dt, label=f'tap.add.{j}')
                dx = pp[turn % 3]          # not this block's dy nor the previous block's (still read by its wgrad)
                turn += 1
                nxt = nm['block'].format(i=i, j=j - 1) if j > 0 and not (i == 2 and (j - 1) in tap_at) else None
                self._block_bwd(nm['block'].format(i=i, j=j), dy, dx, next_pre=nxt)
                dy = dx
            if i > 0:
                pre = f'stages.{i}.downsample.'          # buffer names only
                pln, pcv = nm['ds_ln'].format(i=i), nm['ds_conv'].format(i=i)
                x_prev, Hp = stage_in[i - 1]
                Mp = B * Hp * Hp
                G = self.gbuf((d[i], 4 * d[i - 1]))
                with self._wlane():
                    Bk.wgrad(dy, self.bufs[pre + 'ln'], G, Mi, d[i], 4 * d[i - 1], dt, x_kind=A_PATCH2,
                             x_dims=(Hp, Hp, d[i - 1]), dbias=self.grad(pcv + 'bias'), label=pre + 'wg')
                Bk.weight_unfold(G, 4 * d[i - 1], d[i], d[i - 1], 2, 2, dW=self.grad(pcv + 'weight'), label=pre + 'unf')
                dln = self.tmp('dln', (Mp, d[i - 1]))
                Bk.gemm(dy, W[pcv + 'weight.T'], dln, Mi, 4 * d[i - 1], d[i], dt, ldb=pad8(d[i]), c_kind=C_UNPATCH2,
                        c_dims=(Hp, Hp, d[i - 1]), label=pre + 'dg')
                dprev = self.tmp(f'dprev{i}', (Mp, d[i - 1]))
                Bk.layernorm_bwd(dln, x_prev, self.bufs[pre + 'mean'], self.bufs[pre + 'rstd'], P[pln + 'weight'],
                                 seed[i - 1], dprev, self.grad(pln + 'weight'), self.grad(pln + 'bias'), Mp, d[i - 1],
                                 False, dt, label=pre + 'lnb')
                dy = dprev
            # gradients of stage i (incl. its downsample) are final; stage 0's stay with the stem's, under the end of the plan
            self._seal(f'stage{i}', *([p.format(i=i) for p in nm['stage']] if i > 0 else ()), flush=f'stage{i}.')
        # stem
        M0 = dy.shape[0]
        sc, sl = nm['stem_conv'], nm['stem_ln']
        if stem_seed is not None:
            Bk.affine_act(dy, None, None, stem_seed, dy, M0, d[0], False, dt, label='stem.seed')
        dpre = self.tmp('dstem', (M0, d[0]))
        Bk.layernorm_bwd(dy, self.bufs['stem.pre'], self.bufs['stem.mean'], self.bufs['stem.rstd'], P[sl + 'weight'], None,
                         dpre, self.grad(sl + 'weight'), self.grad(sl + 'bias'), M0, d[0], False, dt, label='stem.lnb')
        with self._wlane():
            Bk.wgrad(dpre, self.x_placeholder, self.grad(sc + 'weight'), M0, d[0], 48, dt, x_kind=A_STEM4_NCHW,
                     x_dims=(self.img, self.img, 3), dbias=self.grad(sc + 'bias'), label='stem.wg')
        self.input_bwd_desc = self._last_desc(Bk)


class GAHeads(HeadStacks):
    """builder: what follows the trunk of a GA model -- the aggregation of the stage outputs and taps into one concat buffer, the
    SE-Bottleneck and the five GA heads.  The family supplies `_gram_layer_fwd` / `_gram_layer_bwd` (gram_layer[k] is a block of its
    own trunk) and sets `self.cout`, the width of the map the heads read."""

    def _aggregate_fwd(self, feats, taps, d, Hc):
        """ga_convnext.py:479-483, ga_cswin.py:666-669: stage outputs 0 / 1, the stage-2 taps and output (average pool) and the stage-3
        output (bilinear x 2) into the columns of one [B*Hc*Hc, ctot] buffer; returns (cat, ctot)"""
        B, F, dt = self.B, self.fwd, self.dt
        segs = [(feats[0][0], feats[0][1], d[0], 0), (feats[1][0], feats[1][1], d[1], 0)]
        segs += [(t, feats[2][1], d[2], 0) for t in taps]
        segs += [(feats[2][0], feats[2][1], d[2], 0), (feats[3][0], feats[3][1], d[3], 1)]
        ctot = sum(c for _, _, c, _ in segs)
        cat = self.act('agg.cat', (B * Hc * Hc, ctot))
        off = 0
        self.agg_segs = []
        for src, hw, c, mode in segs:
            F.pool_concat_fwd(src, cat, B, hw, hw, c, Hc, Hc, ctot, off, mode, dt, label=f'agg.{off}')
            self.agg_segs.append((src, hw, c, mode, off))
            off += c
        return cat, ctot

    def _aggregate_bwd(self, dcat, ctot, Hc):
        """gradient seeds of the aggregated maps, in the order of _aggregate_fwd's segments"""
        seeds = []
        for src, hw, c, mode, off in self.agg_segs:
            ds = self.buf(f'agg.d{off}', (self.B * hw * hw, c))
            self.bwd.pool_concat_bwd(dcat, None, ds, self.B, hw, hw, c, Hc, Hc, ctot, off, mode, self.dt, label=f'agg.b{off}')
            seeds.append(ds)
        return seeds

    # ------------------------------------------------------------------------------------------
    # Bottleneck (ga_convnext.py:294-318)
    # ------------------------------------------------------------------------------------------
    def _bott_pad(self, pre, w, wp, ctot, cout):
        """odd-width variants (688 / 976: the Bottleneck is 172 / 244 channels wide, rows of 344 / 488 bytes): the branch runs
        wp = pad8(w) channels wide on zero-padded COPIES of its parameters (ga_pad_copy_f32 in the weight-prep plan); the extra
        channels carry exact zeros through conv / BN / ReLU / SE, their gradients are zero, and the real part of every
        gradient is copied back after the backward pass.  Returns (params, pending gradient copies)."""
        P = self.P
        R = P[pre + 'se.fc1.weight'].shape[0]
        spec = {'conv1.weight': ((wp, ctot), w, ctot, ctot, ctot), 'conv2.weight': ((wp, wp, 3, 3), w, 9 * w, 9 * w, 9 * wp),
                'conv3.weight': ((cout, wp), cout, w, w, wp), 'se.fc1.weight': ((R, wp), R, w, w, wp),
                'se.fc2.weight': ((wp, R), w, R, R, R), 'se.fc2.bias': ((wp,), 1, w, w, wp)}
        for bn in ('bn1', 'bn2'):
            spec[bn + '.weight'] = ((wp,), 1, w, w, wp)
            spec[bn + '.bias'] = ((wp,), 1, w, w, wp)
        PB, back = {}, []
        for name, (shape, rows, cols, lds, ldd) in spec.items():
            # (conv2: a source row is [ci][9], contiguous; the padded row [wp][9] holds it at its head)
            buf = self.buf('pad.' + pre + name, shape, torch.float32, zero=True)
            self.prep.pad_copy_f32(P[pre + name], buf, rows, cols, lds, ldd, label='prep.pad.' + pre + name)
            PB[pre + name] = buf
            back.append((name, rows, cols, lds, ldd))
        return PB, back

    def _bottleneck_fwd(self, cat, M4, ctot, cout, pre='stages.4.'):
        """pre: the SE-Bottleneck's parameter prefix (GA-CSWin with stage5='bottleneck': 'stage5.')"""
        F, dt, B, P, T = self.fwd, self.dt, self.B, self.P, self.training
        par_branch = os.environ.get('GAEXT_PAR_BRANCH', '1') != '0'   # the shortcut branch beside the main branch (forward)
        w_real = cout // 4
        w = pad8(w_real)
        HW = M4 // B
        st = self.bott = dict(pre=pre, cat=cat, w=w, w_real=w_real, cout=cout, ctot=ctot, PB=None)
        if w != w_real:
            st['PB'], st['back'] = self._bott_pad(pre, w_real, w, ctot, cout)
            P = dict(P)                      # the padded copies shadow the Bottleneck's odd-width parameters
            P.update(st['PB'])
        st['P'] = P
        stats = T  # batch statistics only in train mode

        def conv_bn(name, bnname, A, Wt, N, Kdim, bias=None, n_real=None, **kw):
            c = self.act(pre + name + '.out', (M4, N))
            bn = self._bn_bufs(pre + bnname + '.', N, zero=bool(n_real) and n_real != N)
            F.gemm(A, Wt, c, M4, N, Kdim, dt, bias=bias, colsum=bn['s'] if stats else None,
                   colsumsq=bn['q'] if stats else None, label=pre + name, **kw)
            # (padded width: the statistics buffers are N wide, zero beyond the real channels -> scale = shift = 0 there)
            self._bn_finalize(pre + bnname + '.', bn, M4, n_real or N)
            return c, bn

        # the shortcut branch (conv 1x1 of the 2208-channel concat + BN) only needs `cat`: it runs on the plan's
        # asynchronous lane beside the main branch and is joined before the sum
        F.lane = ASYNC_LANE if par_branch else 0
        Wds = self._w_plain(pre + 'downsample.0.weight', cout, ctot, 1, 1)
        st['sc'], st['bnd'] = conv_bn('downsample.0', 'downsample.1', cat, Wds, cout, ctot, bias=P[pre + 'downsample.0.bias'])
        t = self.tmp('bott.t', (M4, cout))
        F.affine_act(st['sc'], st['bnd']['scale'], st['bnd']['shift'], None, t, M4, cout, False, dt, label=pre + 'bnd')
        F.lane = 0
        Wc1 = self._w_plain(pre + 'conv1.weight', w, ctot, 1, 1, src=P[pre + 'conv1.weight'])
        st['c1'], st['bn1'] = conv_bn('conv1', 'bn1', cat, Wc1, w, ctot, n_real=w_real)
        st['y1'] = self.act(pre + 'y1', (M4, w))
        F.affine_act(st['c1'], st['bn1']['scale'], st['bn1']['shift'], None, st['y1'], M4, w, True, dt, label=pre + 'bn1')
        Wc2 = self._w_plain(pre + 'conv2.weight', w, w, 3, 3, flip=True, src=P[pre + 'conv2.weight'])
        st['c2'], st['bn2'] = conv_bn('conv2', 'bn2', st['y1'], Wc2, w, 9 * w, n_real=w_real, a_kind=A_CONV3, a_dims=(14, 14, w))
        st['y2'] = self.act(pre + 'y2', (M4, w))
        F.affine_act(st['c2'], st['bn2']['scale'], st['bn2']['shift'], None, st['y2'], M4, w, True, dt, label=pre + 'bn2')
        # squeeze-excite
        R = P[pre + 'se.fc1.weight'].shape[0]
        st['R'] = R
        st['sp'] = self.act(pre + 'se.sp', (B, w), torch.float32)
        st['hid'] = self.act(pre + 'se.hid', (B, R), torch.float32)
        st['gate'] = self.act(pre + 'se.gate', (B, w), torch.float32)
        F.spatial_sum(st['y2'], None, st['sp'], B, HW, w, 1.0 / HW, dt, label=pre + 'se.pool')
        F.se_mlp_fwd(st['sp'], P[pre + 'se.fc1.weight'], P[pre + 'se.fc1.bias'], P[pre + 'se.fc2.weight'],
                     P[pre + 'se.fc2.bias'], st['hid'], st['gate'], B, w, R, label=pre + 'se.mlp')
        st['z'] = self.act(pre + 'se.z', (M4, w))
        F.chan_scale(st['y2'], st['gate'], None, st['z'], B, HW, w, dt, label=pre + 'se.scale')
        Wc3 = self._w_plain(pre + 'conv3.weight', cout, w, 1, 1, src=P[pre + 'conv3.weight'])
        st['c3'], st['bn3'] = conv_bn('conv3', 'bn3', st['z'], Wc3, cout, w)
        x4 = self.buf(pre + 'out', (M4, cout))
        if par_branch:
            F.join_async()
        F.affine_act(st['c3'], st['bn3']['scale'], st['bn3']['shift'], t, x4, M4, cout, True, dt,
                     rowscale=self.dp_scale.get(pre), rows_per_scale=HW, label=pre + 'bn3+add')
        st['x4'] = x4
        return x4

    def _bottleneck_bwd(self, dx4, dcat):
        Bk, dt, B, P, W = self.bwd, self.dt, self.B, self.bott['P'], self.W
        st = self.bott
        pre = st['pre']
        w, cout, ctot = st['w'], st['cout'], st['ctot']
        padded = st['PB'] is not None
        GB = {pre + name: self.gbuf(tuple(st['PB'][pre + name].shape)) for name, *_ in st['back']} if padded else {}

        def grad(name):          # gradient buffer of a Bottleneck parameter: the zeroed padded one where the branch is padded
            return GB[name] if name in GB else self.grad(name)

        M4 = dx4.shape[0]
        HW = M4 // B
        dp = self.dp_scale.get(pre)
        dc3 = self.tmp('bott.dc3', (M4, cout))
        self._bn_bwd(pre + 'bn3.', st['bn3'], dx4, st['x4'], st['c3'], dc3, M4, cout, rowscale=dp, rps=HW)
        # shortcut branch on the asynchronous lane: BN backward, weight gradient and the FIRST write of dcat
        dsc = self.tmp('bott.dsc', (M4, cout))
        with self._wlane():
            self._bn_bwd(pre + 'downsample.1.', st['bnd'], dx4, st['x4'], st['sc'], dsc, M4, cout)
            Bk.wgrad(dsc, st['cat'], self.grad(pre + 'downsample.0.weight'), M4, cout, ctot, dt,
                     dbias=self.grad(pre + 'downsample.0.bias'), label=pre + 'ds.wg')
            Bk.gemm(dsc, W[pre + 'downsample.0.weight.T'], dcat, M4, ctot, cout, dt, ldb=pad8(cout), label=pre + 'ds.dg')
        # conv3
        with self._wlane():
            Bk.wgrad(dc3, st['z'], grad(pre + 'conv3.weight'), M4, cout, w, dt, label=pre + 'conv3.wg')
        dz = self.tmp('bott.dz', (M4, w))
        Bk.gemm(dc3, W[pre + 'conv3.weight.T'], dz, M4, w, cout, dt, label=pre + 'conv3.dg')
        # squeeze-excite
        dgate = self.tmp('bott.dgate', (B, w), torch.float32)
        dsp = self.tmp('bott.dsp', (B, w), torch.float32)
        Bk.spatial_sum(dz, st['y2'], dgate, B, HW, w, 1.0, dt, label=pre + 'se.dgate')
        Bk.se_mlp_bwd(dgate, st['gate'], st['hid'], st['sp'], P[pre + 'se.fc1.weight'], P[pre + 'se.fc2.weight'], dsp,
                      grad(pre + 'se.fc1.weight'), grad(pre + 'se.fc1.bias'), grad(pre + 'se.fc2.weight'),
                      grad(pre + 'se.fc2.bias'), B, w, st['R'], ds_scale=1.0 / HW, label=pre + 'se.mlpb')
        dy2 = self.tmp('bott.dy2', (M4, w))
        Bk.chan_scale(dz, st['gate'], dsp, dy2, B, HW, w, dt, label=pre + 'se.back')
        dc2 = self.tmp('bott.dc2', (M4, w))
        self._bn_bwd(pre + 'bn2.', st['bn2'], dy2, st['y2'], st['c2'], dc2, M4, w, weight=P[pre + 'bn2.weight'] if padded else None,
                     c_real=st['w_real'])
        # conv2 3x3
        G = self.gbuf((w, 9 * w))
        with self._wlane():
            Bk.wgrad(dc2, st['y1'], G, M4, w, 9 * w, dt, x_kind=A_CONV3, x_dims=(14, 14, w), label=pre + 'conv2.wg')
        Bk.weight_unfold(G, 9 * w, w, w, 3, 3, dW=grad(pre + 'conv2.weight'), label=pre + 'conv2.unf')
        dy1 = self.tmp('bott.dy1', (M4, w))
        Bk.gemm(dc2, W[pre + 'conv2.weight.T'], dy1, M4, w, 9 * w, dt, a_kind=A_CONV3, a_dims=(14, 14, w),
                ldb=pad8(9 * w), label=pre + 'conv2.dg')
        dc1 = self.tmp('bott.dc1', (M4, w))
        self._bn_bwd(pre + 'bn1.', st['bn1'], dy1, st['y1'], st['c1'], dc1, M4, w, weight=P[pre + 'bn1.weight'] if padded else None,
                     c_real=st['w_real'])
        # conv1 and the shortcut conv both read `cat`; conv1's dgrad adds onto the shortcut's (already written) dcat
        with self._wlane():
            Bk.wgrad(dc1, st['cat'], grad(pre + 'conv1.weight'), M4, w, ctot, dt, label=pre + 'conv1.wg')
        if self.async_wgrad:
            Bk.join_async()
        Bk.gemm(dc1, W[pre + 'conv1.weight.T'], dcat, M4, ctot, w, dt, ldb=pad8(w), R=dcat, ldr=ctot, label=pre + 'conv1.dg')
        if padded:     # the real part of every padded gradient back into the parameter's gradient (the weight-gradient lane has joined)
            skip = ('bn1.weight', 'bn1.bias', 'bn2.weight', 'bn2.bias')       # accumulated by _bn_bwd at the real width
            Bk.flush(pre + 'pad.')      # the deferred weight-unfold job of conv2 writes the padded gradient: run it first
            for name, rows, cols, lds, ldd in st['back']:
                if name not in skip:
                    Bk.pad_copy_f32(GB[pre + name], self.grad(pre + name), rows, cols, ldd, lds, accumulate=True, label=pre + name + '.unpad')

    def _build_heads(self, x4, M4, Hc):
        """the five GA heads on the stage-4 / stage-5 map x4 [M4, cout] (ga_convnext.py:491-504, ga_cswin.py:677-692)"""
        cfg, B, F = self.cfg, self.B, self.fwd
        cout = self.cout
        NC, K = cfg['num_classes'], cfg['branches']
        assert NC % 8 == 0, 'num_classes must be a multiple of 8 (pad the classifier)'
        self.logits = self.buf('logits', (K, B, NC), torch.float32)
        self.heads = []
        E_, nh_ = cfg['dim_embed'], cfg['num_heads']
        # ga_class_attn_*2 wants head widths that are multiples of 8 and E <= 512.  Odd head widths (688 / 976 variants:
        # dim_embed 168 / 240 = 8 heads of 21 / 30) run hd_p = pad8(hd) wide on zero-padded COPIES of the q / k / v rows and the
        # proj columns (the Bottleneck's scheme, _bott_pad): the extra channels of q, k, v and of the attention output are exact
        # zeros, so are their gradients; the real part of each padded weight gradient is copied back after the backward pass.
        hd_ = E_ // max(nh_, 1)
        self.hd_p = pad8(hd_)
        self.Ea = nh_ * self.hd_p
        self.shared_tok = E_ % nh_ == 0 and self.Ea <= 512
        for k in range(K):      # k and v projections are one stacked [2E, cout] matrix
            self._kv_adjacent(f'ga.{k}.attn.k', f'ga.{k}.attn.v')
        if self.shared_tok and self.Ea != E_:
            for k in range(K):
                pre = f'ga.{k}.attn.'
                # (name, padded shape, rows, cols, source row pitch, padded row pitch)
                spec = (('k.weight', (2 * self.Ea, cout), 2 * nh_, hd_ * cout, hd_ * cout, self.hd_p * cout),
                        ('q.weight', (self.Ea, cout), nh_, hd_ * cout, hd_ * cout, self.hd_p * cout),
                        ('proj.weight', (cout, self.Ea), cout * nh_, hd_, hd_, self.hd_p))
                for name, shape, rows, cols, lds, ldd in spec:
                    buf = self.buf('pad.' + pre + name, shape, torch.float32, zero=True)
                    self.prep.pad_copy_f32(self.P[pre + name], buf, rows, cols, lds, ldd, label='prep.pad.' + pre + name)
                    self.ppad[pre + name] = (buf, 'copy', (rows, cols, lds, ldd))
        if self.shared_tok:
            # LayerScaleBlockClassAttn.norm1 on cat(x_cls, tokens) (ga_convnext.py:244-246) as the shared-token k|v stack: its affine
            # part is folded into each head's k | v (and q) weights
            self.tok = self._tok_stack_fwd('ga', x4, M4, cout, 2 * self.Ea, 1e-5,
                                           [Stacked(f'ga.{k}.attn.k.weight', norm=f'ga.{k}.norm1.', pre=f'ga.{k}.') for k in range(K)])
        self._contract_all_fwd(x4, M4)
        # classifiers: inputs of the five heads in one [K][B][cout] buffer, weights stacked -> one batched GEMM
        self.fc_all = self._fc_stack('all', K, cout, [Stacked(f'fc.{k}.weight', f'fc.{k}.bias', prep=f'prep.fc.{k}') for k in range(K)])
        # with GAEXT_HEAD_STREAMS=n > 1 head k runs on side stream k % n (between a fork / join of the plan)
        self.head_lanes = int(os.environ.get('GAEXT_HEAD_STREAMS', '5')) if self.shared_tok else 1
        for k in self._each_head(F, K):
            self.heads.append(self._head_fwd(k, x4, M4, cout, Hc))
        self._fc_stack_fwd(self.fc_all, self.logits)

    def _contraction_heads(self):
        """gram_contraction[k] = conv1x1 + BatchNorm, as the conv stack's data"""
        return [Stacked(f'gram_contraction.{k}.0.weight', f'gram_contraction.{k}.0.bias', norm=f'gram_contraction.{k}.1.',
                        pre=f'gram_contraction.{k}.', prep=f'prep.gram_contraction.{k}.w', bufs=f'gram_contraction.{k}.1.')
                for k in range(self.cfg['branches'])]

    def _contract_all_fwd(self, x4, M4):
        """gram_contraction (conv1x1 768 -> 192 + BN) of the five heads"""
        self.gcon = self._conv_stack_fwd('gram_contraction', x4, M4, self.cout, self.cfg['gram_dim'], self._contraction_heads())

    def _head_supported(self):
        cfg, cout = self.cfg, self.cout
        g, E, nh, mg, groups = cfg['gram_dim'], cfg['dim_embed'], cfg['num_heads'], cfg['mlp_groups'], cfg['gram_groups']
        # (cout / groups and cout / mg need NOT be multiples of 8: the 688 / 976 variants run those grouped one-token layers
        #  on the alignment-free ga_small_linear kernels)
        return E % nh == 0 and E % 8 == 0 and g % 8 == 0 and cout % 8 == 0 and cout % groups == 0 and cout % mg == 0

    def _gram_fp64(self):
        """get_gram's float64 branch (ga_convnext.py:456-457: `self.training and B < 128`, B the per-step micro-batch), taken only
        by a model built with gram_fp64=True"""
        return bool(self.cfg.get('gram_fp64')) and self.training and self.B < 128

    def _head_fwd(self, k, x4, M4, cout, Hc):
        cfg = self.cfg
        if not self._head_supported():
            # ga_convnext_{tiny,small}_688 / base_976: 688 / 8 = 86 and 688 / 4 = 172 channels per group are not multiples
            # of 8, so the grouped operands of gram_embedding / GroupConvMlp are not 16-byte aligned per group -- and the
            # stage-4 Bottleneck is 688 / 4 = 172 channels wide (rows of 344 bytes).  Tried in round 1: padded group
            # layouts around the head GEMMs work, the 172-wide Bottleneck activations need padded leading dimensions in
            # the BatchNorm / 3x3-gather / squeeze-excite kernels as well (not built)
            raise NotImplementedError(
                f"GA head with dims[4]={cout}, gram groups={cfg['gram_groups']}, mlp groups={cfg['mlp_groups']}, "
                f"dim_embed={cfg['dim_embed']}: the HIP engine needs dims[4] divisible by {8 * cfg['gram_groups']} and "
                f"{8 * cfg['mlp_groups']} (per-group channel counts that are multiples of 8); the *_768 / *_1024 variants "
                f"qualify, *_688 / *_976 need padded group layouts (not built)")
        h = dict(k=k)
        # gram_contraction[k]'s BatchNorm on this head's column slice of the stacked conv output -> h['g0'] [M4, gram_dim]
        gcn = self.gcon
        h['gc'] = gcn['out'][:, k * gcn['n']:]                      # [M4, g] view, row stride gcn['ld']
        h['bn_gc'], h['g0'] = self._conv_stack_bn_fwd(gcn, k, h['gc'], f'gram_contraction.{k}.g0')
        h['g1'] = self._gram_layer_fwd(h, k, Hc)
        self._head_tail_fwd(h, k, x4, M4, cout, Hc)
        return h

    def _head_tail_fwd(self, h, k, x4, M4, cout, Hc):
        """get_gram -> gram_embedding (+BN) -> LayerScaleBlockClassAttn -> this head's classifier input"""
        F, dt, B, P, T, cfg = self.fwd, self.dt, self.B, self.P, self.training, self.cfg
        g, E, nh, mg, NC = cfg['gram_dim'], cfg['dim_embed'], cfg['num_heads'], cfg['mlp_groups'], cfg['num_classes']
        groups = cfg['gram_groups']
        HW = Hc * Hc
        hd = E // nh
        h['scale'] = hd ** -0.5
        if self.shared_tok:       # padded head width (== the real one for the *_768 / *_1024 variants)
            E, hd = self.Ea, self.hd_p
        g1 = h['g1']
        ntri = g * (g + 1) // 2
        Kg = ntri // groups
        Kp = pad8(Kg)
        h['Kg'], h['Kp'] = Kg, Kp
        h['vec'] = self.act(f'gram.{k}.vec', (B, groups * Kp))
        h['gram64'] = self._gram_fp64()
        if h['gram64']:
            # --- Gram vector through get_gram's float64 branch (opt-in, gram_fp64=True): x / H in the activation dtype, everything
            # up to the normalised vector in double, one rounding on the way out; the packed double Gram entries and 1 / norm stay
            # for the backward
            h['Hc'] = Hc
            h['G64'] = self.act(f'gram.{k}.G64', (B, ntri), torch.float64)
            h['inv'] = self.act(f'gram.{k}.inv64', (B,), torch.float64)
            F.gram_f64_fwd(g1, h['vec'], h['inv'], h['G64'], B, HW, g, Hc, groups, Kp, dt, label=f'gram.{k}.f64')
        else:
            # --- Gram vector (fp32 accumulate; the reference's fp64 branch for train & B<128 is covered by the 1e-3 gate)
            alpha = 1.0 / (Hc * Hc * HW)
            h['alpha'] = alpha
            G = self.tmp('gramG', (B, g, g), torch.float32)
            F.wgrad(g1, g1, G, HW, g, g, dt, batch=B, strideY=HW * g, strideX=HW * g, strideW=g * g, split_m=1,
                    accumulate=False, alpha=alpha, label=f'gram.{k}')
            h['inv'] = self.act(f'gram.{k}.inv', (B,), torch.float32)
            F.gram_pack_fwd(G, h['vec'], h['inv'], B, g, groups, Kp, dt, label=f'gram.{k}.pack')
        # --- gram_embedding: grouped 1x1 + BN on (B, cout)
        pre = f'gram_embedding.{k}.'
        cg = cout // groups
        h['e'] = self.act(pre + 'out', (B, cout))
        h['bn_e'] = self._bn_bufs(pre + '1.', cout)
        h['emb_small'] = None
        if cg % 8:      # 688 / 8 = 86 (976 / 8 = 122) channels per group: off the 16-byte grid
            # backward: alignment-free form on the master weights.  Forward (the expensive product: K = 2316 per group): the
            # batched MFMA GEMM into a group-padded buffer [B][groups][pad8(cg)] -- aligned group bases, ragged N -- then compacted
            h['emb_small'] = F.small_linear_desc(h['vec'], P[pre + '0.weight'], h['e'], B, groups, cg, Kg, dt, lda=groups * Kp,
                                                 a_gstride=Kp, ldy=cout, bias=P[pre + '0.bias'])
            cgp = pad8(cg)
            ep = self.tmp('emb_pad', (B, groups * cgp))
            Wemb = self._w_plain(pre + '0.weight', cg, Kg, 1, 1, groups=groups, ldo=Kp, need_T=self.pad_gmlp)
            F.gemm(h['vec'], Wemb, ep, B, cg, Kp, dt, lda=groups * Kp, batch=groups, strideA=Kp, strideB=cg * Kp,
                   ldc=groups * cgp, strideC=cgp, bias=P[pre + '0.bias'], strideBias=cg, label=pre + 'conv')
            F.pad_copy(ep, h['e'], B * groups, cg, cgp, cg, dt, label=pre + 'compact')
            if T:
                F.colstats(h['e'], cout, B, cout, h['bn_e']['s'], h['bn_e']['q'], dt, label=pre + 'stats')
        else:
            Wemb = self._w_plain(pre + '0.weight', cg, Kg, 1, 1, groups=groups, ldo=Kp)
            F.gemm(h['vec'], Wemb, h['e'], B, cg, Kp, dt, lda=groups * Kp, batch=groups, strideA=Kp, strideB=cg * Kp,
                   ldc=cout, strideC=cg, bias=P[pre + '0.bias'], strideBias=cg, colsum=h['bn_e']['s'] if T else None,
                   colsumsq=h['bn_e']['q'] if T else None, strideCol=cg, label=pre + 'conv')
        self._bn_finalize(pre + '1.', h['bn_e'], B, cout)
        h['cls0'] = self.buf(pre + 'cls0', (B, cout))
        F.affine_act(h['e'], h['bn_e']['scale'], h['bn_e']['shift'], None, h['cls0'], B, cout, False, dt, label=pre + 'bn')
        # --- class-attention block
        pre = f'ga.{k}.'
        N = HW
        h['ao'] = self.act(pre + 'ao', (B, E))
        h['P'] = self.act(pre + 'P', (B, nh, N + 1), torch.float32)
        if self.shared_tok:
            # class-token row normalised on its own; norm1's affine part folded into the k | v and q operands
            g1, b1 = P[pre + 'norm1.weight'], P[pre + 'norm1.bias']
            h['cn'] = self.act(pre + 'cn', (B, cout))
            h['rc'] = self.act(pre + 'rc', (B,), torch.float32)
            F.layernorm_fwd(h['cls0'], None, None, h['cn'], None, h['rc'], B, cout, 1e-5, dt, label=pre + 'ln1c')
            tk = self.tok
            E2 = tk['E2']
            h['kvt'] = tk['kv'][:, k * E2:]                       # column slice, row stride tk['ld']
            h['kvc'] = self.act(pre + 'kvc', (B, E2))
            F.gemm(h['cn'], tk['W'][k * E2:], h['kvc'], B, E2, cout, dt, bias=tk['b'][k * E2:], label=pre + 'kvc')
            Wq = self._w_plain(pre + 'attn.q.weight', E, cout, 1, 1, cs=g1, src=self._pw(pre + 'attn.q.weight'))
            bq = self.buf('w.' + pre + 'bq', (E,), torch.float32)
            self.prep.bias_fold(self._pw(pre + 'attn.q.weight'), None, None, b1, bq, E, cout)
            h['q'] = self.act(pre + 'q', (B, E))
            F.gemm(h['cn'], Wq, h['q'], B, E, cout, dt, bias=bq, label=pre + 'q')
            F.class_attn_fwd2(h['q'], h['kvc'], h['kvt'], h['ao'], h['P'], B, N + 1, nh, hd, h['scale'], dt, tok_ld=tk['ld'],
                              label=pre + 'attn')
        else:
            h['u'] = self.act(pre + 'u', (B * (N + 1), cout))
            F.token_cat(h['cls0'], x4, h['u'], B, N, cout, dt, label=pre + 'cat')
            h['un'] = self.act(pre + 'un', (B * (N + 1), cout))
            h['m1'] = self.act(pre + 'm1', (B * (N + 1),), torch.float32)
            h['r1'] = self.act(pre + 'r1', (B * (N + 1),), torch.float32)
            F.layernorm_fwd(h['u'], P[pre + 'norm1.weight'], P[pre + 'norm1.bias'], h['un'], h['m1'], h['r1'], B * (N + 1),
                            cout, 1e-5, dt, label=pre + 'ln1')
            # k and v projections as one GEMM: attn.k.weight and attn.v.weight are adjacent in the flat parameter
            # buffer, so together they already are the stacked [2E, cout] matrix
            Wkv = self.buf('w.' + pre + 'kv', (2 * E, cout))
            WkvT = self.buf('wT.' + pre + 'kv', (cout, 2 * E)) if T else None
            self.prep.weight_prep(P[pre + 'attn.k.weight'], 1, 2 * E, cout, 1, 1, dt, out=Wkv, ldo=cout, outT=WkvT, ldt=2 * E if T else 0,
                                  label='prep.' + pre + 'kv')
            h['Wkv'], h['WkvT'] = Wkv, WkvT
            h['kv'] = self.act(pre + 'kv', (B * (N + 1), 2 * E))
            F.gemm(h['un'], Wkv, h['kv'], B * (N + 1), 2 * E, cout, dt, label=pre + 'kv')
            Wq = self._w_plain(pre + 'attn.q.weight', E, cout, 1, 1)
            h['q'] = self.act(pre + 'q', (B, E))
            F.gemm(h['un'], Wq, h['q'], B, E, cout, dt, lda=(N + 1) * cout, label=pre + 'q')
            F.class_attn_fwd(h['q'], h['kv'], h['ao'], h['P'], B, N + 1, nh, hd, h['scale'], dt, label=pre + 'attn')
        Wpr = self._w_plain(pre + 'attn.proj.weight', cout, E, 1, 1, rs=P[pre + 'gamma_1'], src=self._pw(pre + 'attn.proj.weight'))
        bpr = self.buf('w.' + pre + 'bproj', (cout,), torch.float32)
        self.prep.bias_fold(None, P[pre + 'attn.proj.bias'], P[pre + 'gamma_1'], None, bpr, cout, E)
        dp = self.dp_scale.get(pre)
        h['cls1'] = self.buf(pre + 'cls1', (B, cout))
        F.gemm(h['ao'], Wpr, h['cls1'], B, cout, E, dt, bias=bpr, rowscale=dp, rows_per_scale=1, R=h['cls0'], ldr=cout,
               label=pre + 'proj')
        h['t'] = self.act(pre + 't', (B, cout))
        h['m2'] = self.act(pre + 'm2', (B,), torch.float32)
        h['r2'] = self.act(pre + 'r2', (B,), torch.float32)
        F.layernorm_fwd(h['cls1'], P[pre + 'norm2.weight'], P[pre + 'norm2.bias'], h['t'], h['m2'], h['r2'], B, cout, 1e-5,
                        dt, label=pre + 'ln2')
        h['cls2'] = self.fc_all['x'][k]                          # slice of [K][B][cout]: the five classifiers run as one GEMM
        h['mlp'] = self._gmlp_fwd(pre + 'mlp.', h['t'], B, cout, mg, h['cls2'], h['cls1'], dp, 1, gamma_name=pre + 'gamma_2')

    def _head_bwd(self, h, dlog, dx4, first):
        Bk, dt, B, P, W, cfg = self.bwd, self.dt, self.B, self.P, self.W, self.cfg
        k = h['k']
        g, E, nh, mg, NC = cfg['gram_dim'], cfg['dim_embed'], cfg['num_heads'], cfg['mlp_groups'], cfg['num_classes']
        groups = cfg['gram_groups']
        cout = self.cout
        M4 = dx4.shape[0]
        HW = M4 // B
        N = HW
        hd = E // nh
        if self.shared_tok:
            E, hd = self.Ea, self.hd_p
        pre = f'ga.{k}.'
        dp = self.dp_scale.get(pre)
        # classifier: done for all heads at once in _build_backward
        dcls2 = self.fc_all['dx'][k]
        dmz = dcls2
        if dp is not None:
            dmz = self.tmp('dmz', (B, cout))
            Bk.rowscale(dcls2, dp, dmz, B * cout, cout, dt)
        dtk = self.tmp('dt', (B, cout))
        self._gmlp_bwd(pre + 'mlp.', h['mlp'], dmz, h['t'], B, cout, mg, dtk, gamma_name=pre + 'gamma_2')
        dcls1 = self.tmp('dcls1', (B, cout))
        Bk.layernorm_bwd(dtk, h['cls1'], h['m2'], h['r2'], P[pre + 'norm2.weight'], dcls2, dcls1,
                         self.grad(pre + 'norm2.weight'), self.grad(pre + 'norm2.bias'), B, cout, False, dt, label=pre + 'ln2b')
        dpz = dcls1
        if dp is not None:
            dpz = self.tmp('dpz', (B, cout))
            Bk.rowscale(dcls1, dp, dpz, B * cout, cout, dt)
        # attention projection
        Gp, gbp = self.gbuf((cout, E)), self.gbuf((cout,))
        Bk.wgrad(dpz, h['ao'], Gp, B, cout, E, dt, dbias=gbp, label=pre + 'proj.wg')
        Bk.weight_unfold(Gp, E, cout, E, gb=gbp, W=self._pw(pre + 'attn.proj.weight'), b=P[pre + 'attn.proj.bias'],
                         rs=P[pre + 'gamma_1'], dW=self._pg(pre + 'attn.proj.weight'), db=self.grad(pre + 'attn.proj.bias'),
                         d_rs=self.grad(pre + 'gamma_1'), label=pre + 'proj.unf')
        dao = self.tmp('dao', (B, E))
        Bk.gemm(dpz, W[pre + 'attn.proj.weight.T'], dao, B, E, cout, dt, ldb=pad8(cout), label=pre + 'proj.dg')
        dq = self.tmp('dq', (B, E))
        # k, v are adjacent parameters -> their gradients form one [2E, cout] matrix in the flat gradient buffer
        self._kv_adjacent(pre + 'attn.k', pre + 'attn.v', of=self.grad)
        if self.shared_tok:
            g1, b1 = P[pre + 'norm1.weight'], P[pre + 'norm1.bias']
            dg1, db1 = self.grad(pre + 'norm1.weight'), self.grad(pre + 'norm1.bias')
            tk = self.tok
            E2 = tk['E2']
            dkvc = self.tmp('dkvc', (B, E2))
            dkvt = tk['dkv'][:, k * E2:]
            Bk.class_attn_bwd2(dao, h['q'], h['kvc'], h['kvt'], h['P'], dq, dkvc, dkvt, B, N + 1, nh, hd, h['scale'], dt,
                               tok_ld=tk['ld'], label=pre + 'attnb')
            # class-token row's share of the effective k|v weight gradient (the token rows' share: one wgrad after the loop)
            Bk.wgrad(dkvc, h['cn'], tk['G'][k * E2:], B, E2, cout, dt, dbias=tk['gb'][k * E2:], label=pre + 'kvc.wg')
            Gq, gbq = self.gbuf((E, cout)), self.gbuf((E,))
            Bk.wgrad(dq, h['cn'], Gq, B, E, cout, dt, dbias=gbq, label=pre + 'q.wg')
            Bk.weight_unfold(Gq, cout, E, cout, gb=gbq, W=self._pw(pre + 'attn.q.weight'), cs=g1, v=b1,
                             dW=self._pg(pre + 'attn.q.weight'), d_cs=dg1, d_v=db1, label=pre + 'q.unf')
            # gradient wrt the normalised class-token row (the image-token rows: one GEMM over all heads after the loop)
            dcn = self.tmp('dcn', (B, cout))
            Bk.gemm(dkvc, tk['WT'][:, k * E2:], dcn, B, cout, E2, dt, ldb=tk['ld'], label=pre + 'kvc.dg')
            Bk.gemm(dq, W[pre + 'attn.q.weight.T'], dcn, B, cout, E, dt, ldb=pad8(E), R=dcn, ldr=cout, label=pre + 'q.dg')
            # dcls0 = dcls1 + LN'(dcn)
            Bk.layernorm_bwd(dcn, h['cn'], None, h['rc'], None, dcls1, dcls1, None, None, B, cout, True, dt, label=pre + 'ln1cb')
        else:
            dkv = self.tmp('dkv', (B * (N + 1), 2 * E))
            Bk.class_attn_bwd(dao, h['q'], h['kv'], h['P'], dq, dkv, B, N + 1, nh, hd, h['scale'], dt, label=pre + 'attnb')
            Bk.wgrad(dkv, h['un'], self.grad(pre + 'attn.k.weight'), B * (N + 1), 2 * E, cout, dt, label=pre + 'kv.wg')
            dun = self.tmp('dun', (B * (N + 1), cout))
            Bk.gemm(dkv, h['WkvT'], dun, B * (N + 1), cout, 2 * E, dt, label=pre + 'kv.dg')
            Bk.wgrad(dq, h['un'], self.grad(pre + 'attn.q.weight'), B, E, cout, dt, ldx=(N + 1) * cout, label=pre + 'q.wg')
            Bk.gemm(dq, W[pre + 'attn.q.weight.T'], dun, B, cout, E, dt, ldb=pad8(E), ldc=(N + 1) * cout, R=dun,
                    ldr=(N + 1) * cout, label=pre + 'q.dg')
            du = self.tmp('du_tok', (B * (N + 1), cout))
            Bk.layernorm_bwd(dun, h['u'], h['m1'], h['r1'], P[pre + 'norm1.weight'], None, du, self.grad(pre + 'norm1.weight'),
                             self.grad(pre + 'norm1.bias'), B * (N + 1), cout, False, dt, label=pre + 'ln1b')
            # dcls0 = dcls1 + du[:,0];  dx4 (+)= du[:,1:]
            Bk.token_split(du, dcls1, dx4, B, N, cout, True, not first, dt, label=pre + 'split')
        # gram_embedding BN + grouped conv
        pre = f'gram_embedding.{k}.'
        cg = cout // groups
        Kg, Kp = h['Kg'], h['Kp']
        de = self.tmp('de', (B, cout))
        self._bn_bwd(pre + '1.', h['bn_e'], dcls1, None, h['e'], de, B, cout)
        gW = self.grad(pre + '0.weight')
        dvec = self.buf(f'gram.{k}.dvec', (B, groups * Kp), zero=True)   # pad columns stay zero
        if h['emb_small'] is not None and self.pad_gmlp:
            # odd group width (86 / 122 output channels per group): the gradient in a group-padded copy [B][groups][pad8(cg)] (pad
            # columns zero) -> both products on the MFMA kernels; the weight gradient lands in a padded scratch [groups][pad8(cg)][Kg]
            # whose real rows are added to the parameter's gradient
            cgp = pad8(cg)
            dep = self.buf(pre + 'de.pad', (B, groups * cgp), zero=True)
            Bk.pad_copy(de, dep, B * groups, cg, cg, cgp, dt, label=pre + 'de.pad')
            Gp, gbp = self.gbuf((groups * cgp, Kg)), self.gbuf((groups * cgp,))
            Bk.wgrad(dep, h['vec'], Gp, B, cgp, Kg, dt, ldy=groups * cgp, ldx=groups * Kp, ldw=Kg, batch=groups, strideY=cgp,
                     strideX=Kp, strideW=cgp * Kg, dbias=gbp, strideDbias=cgp, label=pre + 'wg')
            Bk.pad_copy_f32(Gp, gW, groups, cg * Kg, cgp * Kg, cg * Kg, accumulate=True, label=pre + 'wg.unpad')
            Bk.pad_copy_f32(gbp, self.grad(pre + '0.bias'), groups, cg, cgp, cg, accumulate=True, label=pre + 'db.unpad')
            Bk.gemm(dep, W[pre + '0.weight.T'], dvec, B, Kg, cgp, dt, lda=groups * cgp, batch=groups, strideA=cgp,
                    strideB=Kg * cgp, ldb=cgp, ldc=groups * Kp, strideC=Kp, label=pre + 'dg')
        elif h['emb_small'] is not None:
            Bk.small_linear_bwd(h['emb_small'], de, dA=dvec, dW=gW, dbias=self.grad(pre + '0.bias'), label=pre + 'bwd')
        else:
            Bk.wgrad(de, h['vec'], gW, B, cg, Kg, dt, ldy=cout, ldx=groups * Kp, ldw=Kg, batch=groups, strideY=cg, strideX=Kp,
                     strideW=cg * Kg, dbias=self.grad(pre + '0.bias'), strideDbias=cg, label=pre + 'wg')
            Bk.gemm(de, W[pre + '0.weight.T'], dvec, B, Kg, cg, dt, lda=cout, batch=groups, strideA=cg, strideB=Kg * pad8(cg),
                    ldb=pad8(cg), ldc=groups * Kp, strideC=Kp, label=pre + 'dg')
        dg1 = self.tmp('dg1', (M4, g))
        if h['gram64']:
            S64 = self.tmp('gramS64', (B, g, g), torch.float64)
            Bk.gram_f64_bwd(dvec, h['g1'], h['G64'], h['inv'], dg1, S64, B, HW, g, h['Hc'], groups, Kp, dt, label=f'gram.{k}.f64b')
        else:
            S = self.tmp('gramS', (B, g, g))
            Bk.gram_pack_bwd(dvec, h['vec'], h['inv'], S, B, g, groups, Kp, dt, label=f'gram.{k}.packb')
            Bk.gemm(h['g1'], S, dg1, HW, g, g, dt, batch=B, strideA=HW * g, strideB=g * g, strideC=HW * g, alpha=h['alpha'],
                    label=f'gram.{k}.dx')
        dg0 = self.tmp('dg0', (M4, g))
        self._gram_layer_bwd(h, dg1, dg0)
        self._conv_stack_bn_bwd(self.gcon, k, h['bn_gc'], dg0, h['gc'])

    # ------------------------------------------------------------------------------------------
    # backward of the heads
    # ------------------------------------------------------------------------------------------
    def _build_heads_backward(self, x4, M4):
        """backward of _build_heads: classifiers, the heads, the shared parts; returns dx4 [M4, cout]"""
        Bk, cfg = self.bwd, self.cfg
        K, NC = cfg['branches'], cfg['num_classes']
        self.dlogits = self.buf('dlogits', (K, self.B, NC))
        Bk.zero(self.arena, label='zero.arena')
        dx4 = self.tmp('dx4', (M4, self.cout))
        self._fc_stack_bwd(self.fc_all, self.dlogits, 'all')
        if self.shared_tok:
            self._tok_stack_bwd_open(self.tok)
        self._conv_stack_bwd_open(self.gcon)
        for k in self._each_head(Bk, K):
            self._head_bwd(self.heads[k], self.dlogits[k], dx4, first=(k == 0))
        self._contract_all_bwd(x4, dx4, M4)
        if self.shared_tok:
            self._tok_stack_bwd_close(self.tok, dx4)
        return dx4

    def _contract_all_bwd(self, x4, dx4, M4):
        """weight / data gradients of the five gram_contraction convs; FIRST writer of dx4 on the shared-token path (the per-head
        token_split of the other path has written it)"""
        self._conv_stack_bwd_close(self.gcon, x4, dx4, R=None if self.shared_tok else dx4, ldr=self.cout)


class GAEngine(ConvNeXtTrunk, GAHeads, EngineBase):
    """GA_ConvNeXt: the ConvNeXt trunk, the aggregation, the SE-Bottleneck "stage 4" and the five GA heads"""

    def _drop_path_rates(self):
        dep = self.cfg['depths']
        rate = self.cfg['drop_path_rate']
        pts = torch.linspace(0, rate, sum(dep)).split(list(dep))
        out = {}
        for i in range(4):
            for j in range(dep[i]):
                out[f'stages.{i}.blocks.{j}.'] = float(pts[i][j])
        out['stages.4.'] = float(rate)
        for k in range(self.cfg['branches']):
            out[f'gram_layer.{k}.blocks.0.'] = float(pts[-1][0])   # dp_rates[-1] (ga_convnext.py:413)
            out[f'ga.{k}.'] = 0.0                                    # LayerScaleBlockClassAttn default drop_path=0
        return out

    def _arena_extra(self):
        """the padded gradient copies of the odd-width variants (688 / 976)"""
        cfg = self.cfg
        cout, g, groups = cfg['dims'][4], cfg['gram_dim'], cfg['gram_groups']
        if cout % (8 * groups) == 0 and cout % (8 * cfg['mlp_groups']) == 0 and (cfg['dim_embed'] // max(cfg['num_heads'], 1)) % 8 == 0:
            return 0
        cp = cout + 8 * max(groups, cfg['mlp_groups'])
        return cfg['branches'] * (cp * (g * (g + 1) // 2 // groups + 8) + 8 * cp * cp // cfg['mlp_groups'] + 4 * cp * 512) + (1 << 20)

    def _build(self):
        cfg = self.cfg
        d = cfg['dims']
        self._init_group_mlp()
        feats, taps, stage_in, _ = self._build_trunk()
        Hc = 14
        M4 = self.B * Hc * Hc
        cat, ctot = self._aggregate_fwd(feats, taps, d, Hc)
        assert ctot == sum(d[:-1]) + d[2] * cfg['naggre']
        # ---------------- Bottleneck "stage 4" ----------------
        x4 = self._bottleneck_fwd(cat, M4, ctot, d[4])
        self.cout = d[4]
        self._build_heads(x4, M4, Hc)
        if self.training:
            self._build_backward(feats, taps, stage_in, x4, M4, ctot)

    def _gram_layer_fwd(self, h, k, Hc):
        """gram_layer[k]: one ConvNeXt block at 14x14 (ga_convnext.py:411-415)"""
        h['blk'] = f'gram_layer.{k}.blocks.0.'
        return self._block_fwd(h['blk'], h['g0'], Hc, self.cfg['gram_dim'])

    def _gram_layer_bwd(self, h, dg1, dg0):
        self._block_bwd(h['blk'], dg1, dg0)

    def _build_backward(self, feats, taps, stage_in, x4, M4, ctot):
        cfg = self.cfg
        dx4 = self._build_heads_backward(x4, M4)
        dcat = self.tmp('dcat', (M4, ctot))
        self._bottleneck_bwd(dx4, dcat)
        self._seal('heads', 'stages.4.', 'gram_contraction.', 'gram_layer.', 'gram_embedding.', 'ga.', 'fc.', flush='heads.',
                   then=self._unpad_all)
        # aggregate backward -> gradient seeds of the stage outputs / taps
        seeds = self._aggregate_bwd(dcat, ctot, 14)
        ntap = len(taps)
        d_s0, d_s1 = seeds[0], seeds[1]
        d_taps = seeds[2:2 + ntap]
        d_s2, d_s3 = seeds[2 + ntap], seeds[3 + ntap]
        seed = {0: d_s0, 1: d_s1, 2: d_s2, 3: d_s3}
        tap_at = tap_indices(cfg['depths'][2], cfg['naggre'])
        self._build_trunk_backward(seed, d_taps, tap_at, feats, stage_in)
