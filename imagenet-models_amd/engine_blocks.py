"""TransformerBlocks: the builder of the pre-norm transformer block every attention family records -- timm's `Block` (ViT, PiT) and
the CSWinBlock of GA-CSWin, forward and backward:

  LayerNorm (no affine: folded into the next linear) -> qkv GEMM -> attention -> proj GEMM (+ DropPath + residual) -> LayerNorm
  (folded) -> fc1 + GELU (+ GELU' when training) -> fc2 (+ DropPath + residual);  GroupConvMlp behind an affine LayerNorm instead
  when mlp_groups > 1

What a family decides is in a BlockSpec; the attention between the qkv and the proj GEMM is the spec's recorder: GlobalAttention
(ga_attn_*) or StripeAttention (ga_cswin_*: both stripe branches and LePE in one kernel).

Saved for backward per block: xn1 (LN1 output without affine), rstd1, qkv, the attention output, xn2, rstd2, a = gelu(h),
g = gelu'(h), the block output.
"""
import dataclasses

import torch

from . import ops
from .engine_base import pad8
from .ops import ACT_GELU


@dataclasses.dataclass(frozen=True)
class BlockSpec:
    """the facts of one block that its family decides; made by the caller in the forward, kept in blocks[pre]['spec'] for the backward"""
    C: int
    heads: int
    ntok: int           # tokens per image = rows per DropPath scale
    eps: float          # of both LayerNorms
    qkv: str            # parameter-name prefixes under the block's, e.g. 'attn.qkv.'
    proj: str
    mlp_groups: int
    attn: object        # GlobalAttention / StripeAttention


class GlobalAttention:
    """timm's Attention over all tokens of an image (flash-style; the row log-sum-exp is saved for backward)"""

    def desc(self, eng, pre, st, sp, r0, r1, b0, b1):
        hd = sp.C // sp.heads
        st['lse'] = eng.blk_act(pre + 'lse', (eng.B, sp.heads, sp.ntok), torch.float32)
        return eng.fwd.attn_desc(st['qkv'][r0:r1], st['att'][r0:r1], st['lse'][b0:b1], b1 - b0, sp.ntok, sp.heads, hd, hd ** -0.5, eng.dt)

    def fwd(self, eng, pre, desc):
        eng.fwd.attn_fwd(desc, label=pre + 'attn')

    def bwd(self, eng, pre, st, datt, dqkv):
        ws = eng.tmp('attn_delta', (st['lse'].numel(),), torch.float32)
        eng.bwd.attn_bwd(st['desc'], datt, dqkv, ws, label=pre + 'attnb')


class StripeAttention:
    """CSWin's LePEAttention of both stripe branches, windows addressed in place; mod = the block's parameter holder (geometry)"""

    def __init__(self, mod):
        self.mod = mod

    def desc(self, eng, pre, st, sp, r0, r1, b0, b1):
        mod, P = self.mod, eng.P
        lepe = [(P[pre + f'attns.{i}.get_v.weight'], P[pre + f'attns.{i}.get_v.bias']) for i in range(mod.branch_num)]
        d = eng.fwd.cswin_desc(st['qkv'][r0:r1], st['att'][r0:r1], b1 - b0, mod.reso, sp.C, sp.heads, mod.stripes(), lepe,
                               (sp.C // sp.heads) ** -0.5, eng.dt)
        if b1 - b0 == eng.B:      # the backward's descriptor: its LePE weight-gradient partials count towards the shared buffer's size
            eng._lepe_ws_elems = max(eng._lepe_ws_elems, ops.cswin_attn_bwd_workspace(d) // 4)
        return d

    def fwd(self, eng, pre, desc):
        eng.fwd.cswin_attn_fwd(desc, label=pre + 'attn')

    def bwd(self, eng, pre, st, datt, dqkv):
        Bk = eng.bwd
        lepe_grads = [(eng.grad(pre + f'attns.{i}.get_v.weight'), eng.grad(pre + f'attns.{i}.get_v.bias'))
                      for i in range(self.mod.branch_num)]
        need = ops.cswin_attn_bwd_workspace(st['desc'])
        if need:    # the MFMA kernel leaves the LePE weight-gradient partials of its LDS tiles; the reduce follows in stream order
            lws = eng.tmp('lepe_ws', (eng._lepe_ws_elems,), torch.float32)
            assert need <= lws.numel() * 4
            Bk.cswin_attn_bwd(st['desc'], datt, dqkv, lepe_ws=lws, label=pre + 'attnb')
            Bk.cswin_lepe_wgrad_reduce(st['desc'], lws, lepe_grads, label=pre + 'lepe.red')
        else:
            Bk.cswin_attn_bwd(st['desc'], datt, dqkv, label=pre + 'attnb')
            with eng._wlane():
                Bk.cswin_lepe_wgrad(st['desc'], datt, lepe_grads, label=pre + 'lepe.wg')


def timm_block(C, heads, ntok):
    """the facts of timm's `Block` (ViT, PiT)"""
    return BlockSpec(C=C, heads=heads, ntok=ntok, eps=1e-6, qkv='attn.qkv.', proj='attn.proj.', mlp_groups=1, attn=GlobalAttention())


class TransformerBlocks:
    """builder: the pre-norm transformer block, forward and backward, on EngineBase's buffers and plans (the grouped-MLP form
    needs GroupMlp in the family as well)"""

    def _tblock_fwd(self, pre, x, sp):
        """x [B*ntok, C] -> block output (same shape).  Inside a forward chain (EngineBase._chains: the trunk recorded once per batch
        part, each part on its own lane) the launches cover the chain's rows of the same full-batch buffers; weight preparation and
        the backward's attention descriptor are recorded by the first pass only"""
        F, dt, B, P, T = self.fwd, self.dt, self.B, self.P, self.training
        C, mg, rps, eps, pq, pp = sp.C, sp.mlp_groups, sp.ntok, sp.eps, pre + sp.qkv, pre + sp.proj
        M = B * rps
        assert C % 8 == 0
        (lane, r0, r1, b0, b1), = self._fsplits(rps)
        n = r1 - r0
        first = pre not in self.blocks
        assert mg == 1 or n == M, 'grouped-MLP blocks are recorded for the whole batch'
        if self._chain is not None:      # (outside a chain the caller's lane stands: the heads' gram_layer blocks)
            F.lane = lane
        dp1, dp2 = self.dp_scale.get(pre + '#1'), self.dp_scale.get(pre + '#2')
        dp1c = dp1[b0:b1] if dp1 is not None else None
        dp2c = dp2[b0:b1] if dp2 is not None else None
        st = self.blocks.setdefault(pre, dict(x=x, spec=sp))
        # --- attention branch
        st['xn1'] = self.blk_act(pre + 'xn1', (M, C))
        st['r1'] = self.blk_act(pre + 'r1', (M,), torch.float32)
        F.layernorm_fwd(x[r0:r1], None, None, st['xn1'][r0:r1], None, st['r1'][r0:r1], n, C, eps, dt, label=pre + 'ln1')
        Wqkv = self._w_plain(pq + 'weight', 3 * C, C, 1, 1, cs=P[pre + 'norm1.weight'])
        bq = self.buf('w.' + pre + 'bqkv', (3 * C,), torch.float32)
        if first:
            self.prep.bias_fold(P[pq + 'weight'], P.get(pq + 'bias'), None, P[pre + 'norm1.bias'], bq, 3 * C, C)
        st['qkv'] = self.blk_act(pre + 'qkv', (M, 3 * C))
        F.gemm(st['xn1'][r0:r1], Wqkv, st['qkv'][r0:r1], n, 3 * C, C, dt, bias=bq, label=pre + 'qkv')
        st['att'] = self.blk_act(pre + 'att', (M, C))
        if first:      # the backward's descriptor: the whole batch
            st['desc'] = sp.attn.desc(self, pre, st, sp, 0, M, 0, B)
        sp.attn.fwd(self, pre, st['desc'] if n == M else sp.attn.desc(self, pre, st, sp, r0, r1, b0, b1))
        Wp = self._w_plain(pp + 'weight', C, C, 1, 1)
        # x1 is re-read by the affine LayerNorm backward of the grouped-MLP form only
        x1 = st['x1'] = self.buf(pre + 'x1', (M, C)) if (mg > 1 and T) else self.tmp('x1', (M, C))
        F.gemm(st['att'][r0:r1], Wp, x1[r0:r1], n, C, C, dt, bias=P[pp + 'bias'], rowscale=dp1c, rows_per_scale=rps, R=x[r0:r1], ldr=C,
               label=pre + 'proj')
        # --- MLP branch
        y = st['y'] = self.buf(pre + 'y', (M, C))
        if mg == 1:
            st['xn2'] = self.blk_act(pre + 'xn2', (M, C))
            st['r2'] = self.blk_act(pre + 'r2', (M,), torch.float32)
            F.layernorm_fwd(x1[r0:r1], None, None, st['xn2'][r0:r1], None, st['r2'][r0:r1], n, C, eps, dt, label=pre + 'ln2')
            W1 = self._w_plain(pre + 'mlp.fc1.weight', 4 * C, C, 1, 1, cs=P[pre + 'norm2.weight'])
            b1e = self.buf('w.' + pre + 'b1e', (4 * C,), torch.float32)
            if first:
                self.prep.bias_fold(P[pre + 'mlp.fc1.weight'], P[pre + 'mlp.fc1.bias'], None, P[pre + 'norm2.bias'], b1e, 4 * C, C)
            st['a'] = self.blk_act(pre + 'a', (M, 4 * C))
            st['g'] = self.buf(pre + 'g', (M, 4 * C)) if T else None
            F.gemm(st['xn2'][r0:r1], W1, st['a'][r0:r1], n, 4 * C, C, dt, bias=b1e, act=ACT_GELU, C2=st['g'][r0:r1] if T else None,
                   c2_mode=2 if T else 0, label=pre + 'fc1')
            W2 = self._w_plain(pre + 'mlp.fc2.weight', C, 4 * C, 1, 1)
            F.gemm(st['a'][r0:r1], W2, y[r0:r1], n, C, 4 * C, dt, bias=P[pre + 'mlp.fc2.bias'], rowscale=dp2c, rows_per_scale=rps,
                   R=x1[r0:r1], ldr=C, label=pre + 'fc2')
        else:
            st['t'] = self.blk_act(pre + 't', (M, C))
            st['m2'] = self.blk_act(pre + 'm2', (M,), torch.float32)
            st['r2'] = self.blk_act(pre + 'r2', (M,), torch.float32)
            F.layernorm_fwd(x1, P[pre + 'norm2.weight'], P[pre + 'norm2.bias'], st['t'], st['m2'], st['r2'], M, C, eps, dt,
                            label=pre + 'ln2')
            st['mlp'] = self._gmlp_fwd(pre + 'mlp.', st['t'], M, C, mg, y, x1, dp2, rps)
        return y

    def _tblock_bwd(self, pre, dy, dx, next_pre=None):
        """dy: gradient wrt the block output; writes dx (a different buffer) = gradient wrt the block input.  next_pre: the block
        that consumes dx unchanged as ITS dy (the next one of the backward chain, when no feature seed is added in between): this
        block's last LayerNorm backward then also writes that block's DropPath-scaled copy (self._pre_dyz), saving it a pass"""
        Bk, dt, B, P, W = self.bwd, self.dt, self.B, self.P, self.W
        st = self.blocks[pre]
        sp = st['spec']
        C, mg, rps, pq, pp = sp.C, sp.mlp_groups, sp.ntok, pre + sp.qkv, pre + sp.proj
        M = B * rps
        dp1, dp2 = self.dp_scale.get(pre + '#1'), self.dp_scale.get(pre + '#2')
        # trunk blocks: the weight-gradient launches go to the plan's asynchronous lane (nothing on the dgrad chain reads their
        # results); two sets of the transients they read + three rotating dx buffers (caller), so this block only waits for the
        # asynchronous launches of the block before the previous one (same scheme as ConvNeXtTrunk._block_bwd)
        side = self._wgrad_window()
        par = str(self._bwd_seq & 1) if side else ''
        dyz = dy
        if dp2 is not None:
            dyz = self._pre_dyz.pop(pre, None)           # written by the LayerNorm backward of the block before (backward order)
            if dyz is None:
                dyz = self.tmp('dyz' + par, (M, C))
                Bk.rowscale(dy, dp2, dyz, M * C, rps * C, dt, label=pre + 'dp2')
        dx1 = self.tmp('dx1' + par, (M, C))
        dx1z = dx1
        fuse1 = dp1 is not None and self.fuse_dp and mg == 1
        if fuse1:
            dx1z = self.tmp('dx1z' + par, (M, C))
        if mg == 1:
            with self._wlane():
                Bk.wgrad(dyz, st['a'], self.grad(pre + 'mlp.fc2.weight'), M, C, 4 * C, dt, dbias=self.grad(pre + 'mlp.fc2.bias'),
                         label=pre + 'wg2')
            dh = self.tmp('dh' + par, (M, 4 * C))
            gb1 = self.gbuf((4 * C,))
            Bk.gemm(dyz, W[pre + 'mlp.fc2.weight.T'], dh, M, 4 * C, C, dt, ldb=pad8(C), H=st['g'], ldh=4 * C, h_is_deriv=True,
                    colsum=gb1, label=pre + 'dg2')
            G1 = self.gbuf((4 * C, C))
            with self._wlane():
                Bk.wgrad(dh, st['xn2'], G1, M, 4 * C, C, dt, label=pre + 'wg1')
            gx = self.tmp('g', (M, C))
            Bk.gemm(dh, W[pre + 'mlp.fc1.weight.T'], gx, M, C, 4 * C, dt, ldb=pad8(4 * C), label=pre + 'dg1')
            if fuse1:       # the DropPath-scaled copy of dx1 rides on the LayerNorm backward that writes dx1
                Bk.layernorm_bwd(gx, st['xn2'], None, st['r2'], None, dy, dx1, None, None, M, C, True, dt, label=pre + 'ln2b', dx2=dx1z,
                                 scale2=dp1, rows_per_scale=rps)
            else:
                Bk.layernorm_bwd(gx, st['xn2'], None, st['r2'], None, dy, dx1, None, None, M, C, True, dt, label=pre + 'ln2b')
            Bk.weight_unfold(G1, C, 4 * C, C, gb=gb1, W=P[pre + 'mlp.fc1.weight'], b=P[pre + 'mlp.fc1.bias'],
                             cs=P[pre + 'norm2.weight'], v=P[pre + 'norm2.bias'], dW=self.grad(pre + 'mlp.fc1.weight'),
                             db=self.grad(pre + 'mlp.fc1.bias'), d_cs=self.grad(pre + 'norm2.weight'),
                             d_v=self.grad(pre + 'norm2.bias'), label=pre + 'unf1')
        else:
            dtk = self.tmp('dtk', (M, C))
            self._gmlp_bwd(pre + 'mlp.', st['mlp'], dyz, st['t'], M, C, mg, dtk)
            Bk.layernorm_bwd(dtk, st['x1'], st['m2'], st['r2'], P[pre + 'norm2.weight'], dy, dx1, self.grad(pre + 'norm2.weight'),
                             self.grad(pre + 'norm2.bias'), M, C, False, dt, label=pre + 'ln2b')
        # --- attention branch
        if dp1 is not None and not fuse1:
            dx1z = self.tmp('dx1z' + par, (M, C))
            Bk.rowscale(dx1, dp1, dx1z, M * C, rps * C, dt, label=pre + 'dp1')
        with self._wlane():
            Bk.wgrad(dx1z, st['att'], self.grad(pp + 'weight'), M, C, C, dt, dbias=self.grad(pp + 'bias'), label=pre + 'proj.wg')
        datt = self.tmp('datt' + par, (M, C))
        Bk.gemm(dx1z, W[pp + 'weight.T'], datt, M, C, C, dt, ldb=pad8(C), label=pre + 'proj.dg')
        dqkv = self.tmp('dqkv' + par, (M, 3 * C))
        sp.attn.bwd(self, pre, st, datt, dqkv)
        Gq, gbq = self.gbuf((3 * C, C)), self.gbuf((3 * C,))
        with self._wlane():
            Bk.wgrad(dqkv, st['xn1'], Gq, M, 3 * C, C, dt, dbias=gbq, label=pre + 'qkv.wg')
        has_b = (pq + 'bias') in P
        Bk.weight_unfold(Gq, C, 3 * C, C, gb=gbq, W=P[pq + 'weight'], b=P.get(pq + 'bias'), cs=P[pre + 'norm1.weight'],
                         v=P[pre + 'norm1.bias'], dW=self.grad(pq + 'weight'), db=self.grad(pq + 'bias') if has_b else None,
                         d_cs=self.grad(pre + 'norm1.weight'), d_v=self.grad(pre + 'norm1.bias'), label=pre + 'qkv.unf')
        gq = self.tmp('g', (M, C))
        Bk.gemm(dqkv, W[pq + 'weight.T'], gq, M, C, 3 * C, dt, ldb=pad8(3 * C), label=pre + 'qkv.dg')
        ndp = self.dp_scale.get(next_pre + '#2') if next_pre is not None else None
        if ndp is not None and self.fuse_dp:
            # the consumer's transients alternate with the block parity exactly like this block's (par of the next block = 1 - par)
            npar = str((self._bwd_seq + 1) & 1) if side else ''
            ndyz = self.tmp('dyz' + npar, (M, C))
            if side:           # that buffer was block t-1's: its asynchronous weight gradients must be done before it is rewritten
                Bk.join_async(f'blk{self._bwd_seq - 1}')
            Bk.layernorm_bwd(gq, st['xn1'], None, st['r1'], None, dx1, dx, None, None, M, C, True, dt, label=pre + 'ln1b', dx2=ndyz,
                             scale2=ndp, rows_per_scale=rps)
            self._pre_dyz[next_pre] = ndyz
        else:
            Bk.layernorm_bwd(gq, st['xn1'], None, st['r1'], None, dx1, dx, None, None, M, C, True, dt, label=pre + 'ln1b')
        self._wgrad_window_mark(side)
