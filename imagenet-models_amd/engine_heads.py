"""Builders shared by the GA heads (engine.GAHeads) and the MAP head (engine_map.MAPHead):

  GroupMlp ........ GroupConvMlp forward / backward and the zero-padded parameter copies of the odd-width variants;
  HeadStacks ...... the three products that run ONCE for all heads: the shared-token k|v stack, the stacked 1x1 contraction conv
                    with a BatchNorm per head on its column slice, and the stacked classifiers.
"""
import os
from collections import namedtuple

import torch

from . import ops
from .engine_base import pad8
from .ops import ACT_GELU


class GroupMlp:
    """builder: GroupConvMlp (the GA heads' and the MAP head's MLP) and the zero-padded copies of parameters that the odd-width
    variants run on.  `_init_group_mlp` comes first in the build of a family that uses it."""

    def _init_group_mlp(self):
        # zero-padded copies of parameters of the odd-width variants: name -> (padded buffer, how to copy); gradients: name -> arena buffer
        self.ppad, self.pgrad = {}, {}
        self.pad_gmlp = os.environ.get('GAEXT_PAD_GMLP', '1') != '0'    # odd-width grouped one-token layers on padded MFMA layouts

    def _pw(self, name):
        """master copy of a parameter: the zero-padded one where the layer runs on a padded layout"""
        return self.ppad[name][0] if name in self.ppad else self.P[name]

    def _pg(self, name):
        """gradient buffer of a parameter (padded: a zeroed arena buffer, copied back by _unpad_all)"""
        if name not in self.ppad:
            return self.grad(name)
        if name not in self.pgrad:
            self.pgrad[name] = self.gbuf(tuple(self.ppad[name][0].shape))
        return self.pgrad[name]

    def _pad_groups(self, name, R, Cdim, RG, RGp, CG, CGp):
        """register (once) the two-level group-padded copy of parameter `name` ([R][C] -> [R/RG*RGp][C/CG*CGp], ga_pad_groups_f32)"""
        if name not in self.ppad:
            buf = self.buf('pad.' + name, (R // RG * RGp, Cdim // CG * CGp), torch.float32, zero=True)
            self.prep.pad_groups_f32(self.P[name], buf, R, Cdim, RG, RGp, CG, CGp, label='prep.pad.' + name)
            self.ppad[name] = (buf, 'groups', (R, Cdim, RG, RGp, CG, CGp))
        return self.ppad[name][0]

    def _unpad_all(self):
        """real part of every padded parameter gradient back into the parameter's gradient; call AFTER the flush of the heads'
        deferred weight-unfold jobs (they write the padded gradients) and before the 'heads' mark (_seal(..., then=self._unpad_all))"""
        for name, g in self.pgrad.items():
            _, kind, a = self.ppad[name]
            if kind == 'copy':
                rows, cols, lds, ldd = a
                self.bwd.pad_copy_f32(g, self.grad(name), rows, cols, ldd, lds, accumulate=True, label=name + '.unpad')
            else:
                self.bwd.pad_groups_f32(g, self.grad(name), *a, unpad=True, accumulate=True, label=name + '.unpad')

    # ------------------------------------------------------------------------------------------
    # GroupConvMlp (ga_convnext.py:190-222, ga_cswin.py:321-349): grouped fc1 -> GELU -> channel_shuffle -> grouped fc2
    # on `rows` tokens.  The shuffle is folded into the ROW ORDER of fc1's effective weights: hidden index
    # n = gi*gc + ci  <-  fc1 output channel ci*mg + gi; with Nv = gc / mg rows per "virtual group" the fc1 input group is
    # constant inside one (= v % mg), so fc1 is a batched GEMM over mg*mg virtual groups and fc2 one over mg groups.
    # ------------------------------------------------------------------------------------------
    def _gmlp_fwd(self, pre, t, rows, C, mg, out, R, rowscale, rps, gamma_name=None, act='gelu', drop_mask=None, ratio=4):
        """out = R + rowscale * gamma * fc2(shuffle(drop(act(fc1(t)))));  pre = '<block>.mlp.';  act 'gelu' (GA) or 'relu'
        (MAP, map.py:467) with an optional dropout mask [rows, ratio * C] on the hidden layer (in the SHUFFLED channel order);
        ratio: the hidden width over C (mlp_ratio; with mg = 1 the channel shuffle is the identity)"""
        F, dt, P, T = self.fwd, self.dt, self.P, self.training
        gamma = self._pw(gamma_name) if gamma_name else None
        Hd = int(ratio * C)
        gc_ = Hd // mg
        Nv = gc_ // mg          # rows per virtual group (fc1 input group is constant inside one)
        cin = C // mg
        n_idx = torch.arange(Hd)
        perm = ((n_idx % gc_) * mg + n_idx // gc_).to(torch.int32).to(self.dev)
        if (Nv % 8 or cin % 8) and self.pad_gmlp and C % mg == 0:
            # odd widths (688 / 4 = 172 channels per group) on the MFMA kernels: the layer runs as a GroupConvMlp of mg groups of
            # cin_p = pad8(cin) channels on zero-padded copies of its five parameters (fc1 rows in groups of 4 cin -> 4 cin_p and
            # columns cin -> cin_p; fc2 rows and columns in groups of cin -> cin_p; ga_pad_groups_f32) and group-padded copies of
            # its input / residual; padded hidden and output channels are exact zeros (zero weights, zero biases), the real part
            # of the output is compacted back and the real part of every padded gradient copied back after the backward pass
            assert Hd == 4 * C, 'the padded odd-width layout is laid out for mlp_ratio 4'
            cin_p = pad8(cin)
            Cp = mg * cin_p
            self._pad_groups(pre + 'fc1.weight', Hd, cin, 4 * cin, 4 * cin_p, cin, cin_p)
            self._pad_groups(pre + 'fc1.bias', 1, Hd, 1, 1, 4 * cin, 4 * cin_p)
            self._pad_groups(pre + 'fc2.weight', C, gc_, cin, cin_p, cin, cin_p)
            self._pad_groups(pre + 'fc2.bias', 1, C, 1, 1, cin, cin_p)
            if gamma_name:
                self._pad_groups(gamma_name, 1, C, 1, 1, cin, cin_p)
            # (persistent zero-initialised buffers: the pad columns are never written)
            tp = self.buf(pre + 't.pad', (rows, Cp), zero=True)
            F.pad_copy(t, tp, rows * mg, cin, cin, cin_p, dt, label=pre + 't.pad')
            Rp = None
            if R is not None:
                Rp = self.buf(pre + 'R.pad', (rows, Cp), zero=True)
                F.pad_copy(R, Rp, rows * mg, cin, cin, cin_p, dt, label=pre + 'R.pad')
            outp = self.tmp('gmlp.out.pad', (rows, Cp))
            st = self._gmlp_fwd(pre, tp, rows, Cp, mg, outp, Rp, rowscale, rps, gamma_name=gamma_name, act=act, drop_mask=drop_mask)
            F.pad_copy(outp, out, rows * mg, cin, cin_p, cin, dt, label=pre + 'out.unpad')
            st['pad'] = dict(tp=tp, Cp=Cp, cin=cin, cin_p=cin_p)
            return st
        if Nv % 8 or cin % 8:
            # the same layers on the alignment-free kernels (GAEXT_PAD_GMLP=0), fp32 master weights,
            # the channel_shuffle as a column map of fc2's input (hidden kept in the ORIGINAL channel order, pre-activation saved)
            assert act == 'gelu' and drop_mask is None and rows <= 4096, (pre, C, mg, rows)
            st = dict(naive=True, Hd=Hd, hpre=self.act(pre + 'hpre', (rows, Hd)), am=self.act(pre + 'am', (rows, Hd)),
                      yraw=self.act(pre + 'yraw', (rows, C)) if T else None)
            st['d1'] = F.small_linear_desc(t, P[pre + 'fc1.weight'], st['hpre'], rows, mg, gc_, cin, dt, lda=C, a_gstride=cin, ldy=Hd,
                                           bias=P[pre + 'fc1.bias'])
            F.small_linear_fwd(st['d1'], label=pre + 'fc1')
            F.gelu_fwd(st['hpre'], st['am'], rows * Hd, dt, label=pre + 'gelu')
            kw = dict(bias=P[pre + 'fc2.bias'], a_perm=perm, col_scale=gamma, Yraw=st['yraw'])
            d2 = F.small_linear_desc(st['am'], P[pre + 'fc2.weight'], out, rows, mg, cin, gc_, dt, lda=Hd, a_gstride=gc_, ldy=C,
                                     rowscale=rowscale, rows_per_scale=rps, R=R, ldr=C, **kw)
            F.small_linear_fwd(d2, label=pre + 'fc2')
            # the backward sees a gradient that already carries the DropPath scale: same layer without the row scale
            st['d2b'] = F.small_linear_desc(st['am'], P[pre + 'fc2.weight'], out, rows, mg, cin, gc_, dt, lda=Hd, a_gstride=gc_, ldy=C, **kw)
            return st
        assert gc_ % mg == 0, (pre, C, mg)
        Wm1 = self._w_plain(pre + 'fc1.weight', Nv, cin, 1, 1, groups=mg * mg, row_perm=perm, src=self._pw(pre + 'fc1.weight'))
        bm1 = self.buf('w.' + pre + 'bm1', (Hd,), torch.float32)
        self.prep.bias_fold(None, self._pw(pre + 'fc1.bias'), None, None, bm1, Hd, cin, row_perm=perm)
        st = dict(perm=perm, Hd=Hd, gc=gc_, Nv=Nv, cin=cin)
        st['am'] = self.act(pre + 'am', (rows, Hd))                      # gelu(hidden), shuffled order
        st['gm'] = self.act(pre + 'gm', (rows, Hd)) if T else None       # gelu'(hidden)
        if act == 'gelu':
            assert drop_mask is None
            F.gemm(t, Wm1, st['am'], rows, Nv, cin, dt, lda=C, batch=mg * mg, strideA=cin, a_batch_mod=mg,
                   strideB=Nv * pad8(cin), ldb=pad8(cin), ldc=Hd, strideC=Nv, bias=bm1, strideBias=Nv, act=ACT_GELU,
                   C2=st['gm'], c2_mode=2 if T else 0, label=pre + 'fc1')
        else:   # ReLU: its derivative (times the dropout mask) is a small pass of its own; the GEMM epilogue stays generic
            two = T or drop_mask is not None
            raw = self.tmp('am_raw', (rows, Hd)) if two else st['am']
            F.gemm(t, Wm1, raw, rows, Nv, cin, dt, lda=C, batch=mg * mg, strideA=cin, a_batch_mod=mg,
                   strideB=Nv * pad8(cin), ldb=pad8(cin), ldc=Hd, strideC=Nv, bias=bm1, strideBias=Nv, act=ops.ACT_RELU,
                   label=pre + 'fc1')
            if two:
                F.relu_drop(raw, drop_mask, st['am'], st['gm'], rows * Hd, dt, label=pre + 'relu')
        Wm2 = self._w_plain(pre + 'fc2.weight', cin, gc_, 1, 1, groups=mg, rs=gamma, src=self._pw(pre + 'fc2.weight'))
        bm2 = self.buf('w.' + pre + 'bm2', (C,), torch.float32)
        self.prep.bias_fold(None, self._pw(pre + 'fc2.bias'), gamma, None, bm2, C, gc_)
        F.gemm(st['am'], Wm2, out, rows, cin, gc_, dt, lda=Hd, batch=mg, strideA=gc_, strideB=cin * pad8(gc_),
               ldb=pad8(gc_), ldc=C, strideC=cin, bias=bm2, strideBias=cin, rowscale=rowscale,
               rows_per_scale=rps, R=R, ldr=C, strideR=cin, label=pre + 'fc2')
        return st

    def _gmlp_bwd(self, pre, st, dmz, t, rows, C, mg, dtk, gamma_name=None):
        """dmz: gradient wrt the MLP branch output (DropPath scale already applied) -> dtk = gradient wrt the input t"""
        Bk, dt, P, W = self.bwd, self.dt, self.P, self.W
        gamma = self._pw(gamma_name) if gamma_name else None
        if 'pad' in st:       # the padded layer (see _gmlp_fwd): group-padded gradient in, real part of the input gradient out
            pd = st.pop('pad')
            cin, cin_p, Cp = pd['cin'], pd['cin_p'], pd['Cp']
            dmzp = self.buf(pre + 'dmz.pad', (rows, Cp), zero=True)
            Bk.pad_copy(dmz, dmzp, rows * mg, cin, cin, cin_p, dt, label=pre + 'dmz.pad')
            dtkp = self.tmp('gmlp.dt.pad', (rows, Cp))
            self._gmlp_bwd(pre, st, dmzp, pd['tp'], rows, Cp, mg, dtkp, gamma_name=gamma_name)
            Bk.pad_copy(dtkp, dtk, rows * mg, cin, cin_p, cin, dt, label=pre + 'dt.unpad')
            st['pad'] = pd
            return
        if st.get('naive'):
            Hd = st['Hd']
            dam, dh = self.tmp('dam', (rows, Hd)), self.tmp('dhm', (rows, Hd))
            Bk.small_linear_bwd(st['d2b'], dmz, dA=dam, dW=self.grad(pre + 'fc2.weight'), dbias=self.grad(pre + 'fc2.bias'),
                                dcol_scale=self.grad(gamma_name) if gamma_name else None, label=pre + 'fc2.bwd')
            Bk.gelu_bwd(dam, st['hpre'], dh, rows * Hd, dt, label=pre + 'geluB')
            Bk.small_linear_bwd(st['d1'], dh, dA=dtk, dW=self.grad(pre + 'fc1.weight'), dbias=self.grad(pre + 'fc1.bias'),
                                label=pre + 'fc1.bwd')
            return
        Hd, gc_, Nv, cin = st['Hd'], st['gc'], st['Nv'], st['cin']
        # fc2 (mg groups)
        Gm2, gbm2 = self.gbuf((C, gc_)), self.gbuf((C,))
        Bk.wgrad(dmz, st['am'], Gm2, rows, cin, gc_, dt, ldy=C, ldx=Hd, ldw=gc_, batch=mg, strideY=cin, strideX=gc_,
                 strideW=cin * gc_, dbias=gbm2, strideDbias=cin, label=pre + 'fc2.wg')
        Bk.weight_unfold(Gm2, gc_, C, gc_, gb=gbm2, W=self._pw(pre + 'fc2.weight'), b=self._pw(pre + 'fc2.bias'),
                         rs=gamma, dW=self._pg(pre + 'fc2.weight'), db=self._pg(pre + 'fc2.bias'),
                         d_rs=self._pg(gamma_name) if gamma_name else None, label=pre + 'fc2.unf')
        dhm = self.tmp('dhm', (rows, Hd))
        gbm1 = self.gbuf((Hd,))
        Bk.gemm(dmz, W[pre + 'fc2.weight.T'], dhm, rows, gc_, cin, dt, lda=C, batch=mg, strideA=cin,
                strideB=gc_ * pad8(cin), ldb=pad8(cin), ldc=Hd, strideC=gc_, H=st['gm'], ldh=Hd, strideH=gc_, h_is_deriv=True,
                colsum=gbm1, strideCol=gc_, label=pre + 'fc2.dg')
        # fc1 (mg*mg virtual groups)
        Gm1 = self.gbuf((Hd, cin))
        Bk.wgrad(dhm, t, Gm1, rows, Nv, cin, dt, ldy=Hd, ldx=C, ldw=cin, batch=mg * mg, strideY=Nv, strideX=cin,
                 x_batch_mod=mg, strideW=Nv * cin, label=pre + 'fc1.wg')
        Bk.weight_unfold(Gm1, cin, Hd, cin, gb=gbm1, W=self._pw(pre + 'fc1.weight'), b=self._pw(pre + 'fc1.bias'),
                         row_perm=st['perm'], dW=self._pg(pre + 'fc1.weight'), db=self._pg(pre + 'fc1.bias'),
                         label=pre + 'fc1.unf')
        Wm1T = W[pre + 'fc1.weight.T']            # [mg*mg][cin][pad8(Nv)]
        for gi in range(mg):
            Bk.gemm(dhm[:, gi * gc_:], Wm1T[gi * mg * cin:], dtk, rows, cin, Nv, dt, lda=Hd, batch=mg, strideA=Nv,
                    strideB=cin * pad8(Nv), ldb=pad8(Nv), ldc=C, strideC=cin, R=dtk if gi > 0 else None, ldr=C,
                    strideR=cin, label=pre + f'fc1.dg{gi}')


# one head's share of a stack, as parameter names: weight, bias (None: the layer has none), the prefix of the norm that goes with it
# (token stack: the LayerNorm whose affine part is folded into the weight; conv stack: the BatchNorm on the head's column slice), the
# prefix of the head's labels, the label of its weight-prep launch and the prefix of its BatchNorm buffers
Stacked = namedtuple('Stacked', 'w b norm pre prep bufs', defaults=(None, None, None, None, None))


class HeadStacks(GroupMlp):
    """builder: the products that run once for all heads of a GA or MAP head because every head reads the same map, each head's operands
    stacked along N (or along the batch), forward and backward.  Stateless: a stack is a dict that its forward returns and the family
    keeps (`self.tok`, `self.gcon`, `self.fc_*`); what differs between the families -- the tag the labels and buffer names are formed
    from, width, row count, LayerNorm eps, the heads' parameter names (`Stacked`) -- comes in as data.  Weights go through `_pw` and
    gradients through `_pg` where the layer may run on a padded copy.  What the heads do between the stacks (Gram vector, grouped
    embedding, class-attention block) stays in the family: the two class-attention bodies record their launches in different orders."""

    def _each_head(self, plan, n):
        """k = 0 .. n-1; what is recorded for head k goes to side lane 1 + k % head_lanes of `plan` with transients of its own
        (the heads are independent chains of mostly small launches), what follows the last head to the main lane again"""
        for k in range(n):
            if self.head_lanes > 1:
                plan.lane, self.tmp_prefix = 1 + k % self.head_lanes, f'h{k}.'
            yield k
        plan.lane, self.tmp_prefix = 0, ''

    def _kv_adjacent(self, kn, vn, bias=False, of=None):
        """parameters kn / vn ('<...>.k', '<...>.v') are neighbours in the flat buffer, so k | v is one stacked [2E, C] matrix;
        of: where the tensors come from (default the parameters; `self.grad` for their gradients)"""
        of = of or self.P.__getitem__
        for s in ('.weight', '.bias')[:1 + bias]:
            k, v = of(kn + s), of(vn + s)
            assert v.data_ptr() == k.data_ptr() + k.numel() * 4, f'{kn}{s} | {vn}{s} must be adjacent in the flat buffer'

    def _stack_scatter(self, G, gb, heads):
        """head k's part of a stacked weight gradient G (and bias gradient gb) added to its parameters' gradients"""
        K = len(heads)
        for k, hd in enumerate(heads):
            self.bwd.axpy_f32(self.grad(hd.w), G.view(K, -1)[k], 1.0, G.numel() // K)
            if hd.b:
                self.bwd.axpy_f32(self.grad(hd.b), gb.view(K, -1)[k], 1.0, gb.numel() // K)

    # ------------------------------------------------------------------------------------------
    # shared-token k|v stack.  norm1 of a class-attention block acts row-wise on cat(class rows, image tokens): the normalised image
    # tokens are the SAME for all heads (only the affine part differs, and that is folded into each head's k | v weights like the
    # ConvNeXt block's LayerNorm into fc1).  One LayerNorm over the tokens instead of one per head over the concatenation, no
    # concatenated copy, the k | v rows of ALL heads from one GEMM over the shared tokens, one backward LayerNorm over the summed
    # gradient.  Head k reads / writes the column slice [k*E2, (k+1)*E2) of tk['kv'] / tk['dkv'] and the rows of tk['W'] / tk['G'].
    # ------------------------------------------------------------------------------------------
    def _tok_stack_fwd(self, tag, x, rows, C, E2, eps, heads):
        F, dt, P, T = self.fwd, self.dt, self.P, self.training
        ld = len(heads) * E2
        tk = dict(tag=tag, heads=heads, rows=rows, C=C, E2=E2, ld=ld,
                  xn=self.act(tag + '.tok.xn', (rows, C)), rstd=self.act(tag + '.tok.rstd', (rows,), torch.float32))
        F.layernorm_fwd(x, None, None, tk['xn'], None, tk['rstd'], rows, C, eps, dt, label=tag + '.tok.ln')
        tk['W'] = self.buf(f'w.{tag}.kv_all', (ld, C))
        tk['WT'] = self.buf(f'wT.{tag}.kv_all', (C, ld)) if T else None
        tk['b'] = self.buf(f'w.{tag}.bkv_all', (ld,), torch.float32)
        for k, hd in enumerate(heads):
            pk = self._pw(hd.w)
            self.prep.weight_prep(pk, 1, E2, C, 1, 1, dt, out=tk['W'][k * E2:], ldo=C, outT=tk['WT'][:, k * E2:] if T else None,
                                  ldt=ld if T else 0, cs=P[hd.norm + 'weight'], t_cols=E2, label='prep.' + hd.pre + 'kv')
            self.prep.bias_fold(pk, self._pw(hd.b) if hd.b else None, None, P[hd.norm + 'bias'], tk['b'][k * E2:], E2, C)
        tk['kv'] = self.act(tag + '.kv_all', (rows, ld))
        F.gemm(tk['xn'], tk['W'], tk['kv'], rows, ld, C, dt, bias=tk['b'], label=tag + '.kv_all')
        return tk

    def _tok_stack_bwd_open(self, tk):
        """before the heads' backward: what they write slice-wise and the closing consumes"""
        tk['dkv'] = self.tmp('dkv_all', (tk['rows'], tk['ld']))
        tk['G'], tk['gb'] = self.gbuf((tk['ld'], tk['C'])), self.gbuf((tk['ld'],))

    def _tok_stack_bwd_close(self, tk, dx):
        """after the heads' backward: the token rows' share of the effective k|v weight gradients of all heads at once, each head's
        norm fold undone, and dx += LayerNorm'(gradient wrt the shared normalised tokens, summed over the heads by the K = ld GEMM)"""
        Bk, dt, P = self.bwd, self.dt, self.P
        tag, rows, C, E2, ld = tk['tag'], tk['rows'], tk['C'], tk['E2'], tk['ld']
        with self._wlane():
            Bk.wgrad(tk['dkv'], tk['xn'], tk['G'], rows, ld, C, dt, dbias=tk['gb'], label=tag + '.kv_all.wg')
        for k, hd in enumerate(tk['heads']):
            Bk.weight_unfold(tk['G'][k * E2:], C, E2, C, gb=tk['gb'][k * E2:], W=self._pw(hd.w), b=self._pw(hd.b) if hd.b else None,
                             cs=P[hd.norm + 'weight'], v=P[hd.norm + 'bias'], dW=self._pg(hd.w), db=self._pg(hd.b) if hd.b else None,
                             d_cs=self.grad(hd.norm + 'weight'), d_v=self.grad(hd.norm + 'bias'), label=hd.pre + 'kv.unf')
        dxt = self.tmp('dxn_tok', (rows, C))
        Bk.gemm(tk['dkv'], tk['WT'], dxt, rows, C, ld, dt, label=tag + '.kv_all.dg')
        Bk.layernorm_bwd(dxt, tk['xn'], None, tk['rstd'], None, dx, dx, None, None, rows, C, True, dt, label=tag + '.tok.lnb')

    # ------------------------------------------------------------------------------------------
    # stacked 1x1 contraction conv: the convs of all heads read the same map -> ONE GEMM with the weight matrices stacked along N;
    # head k owns the column slice [k*n, (k+1)*n) of its output / batch statistics / gradient, and its BatchNorm runs on that slice
    # ------------------------------------------------------------------------------------------
    def _conv_stack(self, tag, rows, C, n, heads):
        """the stack's dict before any buffer; a family with a product form of its own fills it itself"""
        return dict(tag=tag, heads=heads, rows=rows, C=C, n=n, ld=len(heads) * n)

    def _conv_stack_fwd(self, tag, x, rows, C, n, heads):
        """the dense form: conv1x1 C -> n of every head (with bias where the heads name one), batch sums for the BatchNorms"""
        F, dt, P, T = self.fwd, self.dt, self.P, self.training
        gc = self._conv_stack(tag, rows, C, n, heads)
        ld = gc['ld']
        gc['W'] = self.buf(f'w.{tag}.all', (ld, C))
        gc['WT'] = self.buf(f'wT.{tag}.all', (C, ld)) if T else None
        gc['b'] = self.buf(f'w.{tag}.ball', (ld,), torch.float32) if heads[0].b else None
        gc['s'], gc['q'] = self._bn_pool(ld), self._bn_pool(ld)
        for k, hd in enumerate(heads):
            self.prep.weight_prep(P[hd.w], 1, n, C, 1, 1, dt, out=gc['W'][k * n:], ldo=C, outT=gc['WT'][:, k * n:] if T else None,
                                  ldt=ld if T else 0, t_cols=n, label=hd.prep)
            if hd.b:
                self.prep.bias_fold(None, P[hd.b], None, None, gc['b'][k * n:], n, C)
        gc['out'] = self.act(tag + '.all.out', (rows, ld))
        F.gemm(x, gc['W'], gc['out'], rows, ld, C, dt, bias=gc['b'], colsum=gc['s'] if T else None, colsumsq=gc['q'] if T else None,
               label=tag + '.all')
        return gc

    def _conv_stack_bn_fwd(self, gc, k, x, out):
        """head k's BatchNorm on x, its column slice of the stacked conv output (a view, row stride gc['ld']) -> (the BatchNorm's
        state, the buffer named `out` [rows, n])"""
        hd, n, rows = gc['heads'][k], gc['n'], gc['rows']
        bn = dict(s=gc['s'][k * n:(k + 1) * n], q=gc['q'][k * n:(k + 1) * n],
                  mean=self.buf(hd.bufs + 'bmean', (n,), torch.float32), rstd=self.buf(hd.bufs + 'brstd', (n,), torch.float32),
                  scale=self.buf(hd.bufs + 'scale', (n,), torch.float32), shift=self.buf(hd.bufs + 'shift', (n,), torch.float32))
        self._bn_finalize(hd.norm, bn, rows, n)
        y = self.buf(out, (rows, n))
        self.fwd.affine_act(x, bn['scale'], bn['shift'], None, y, rows, n, False, self.dt, ldx=gc['ld'], label=hd.pre + 'bn')
        return bn, y

    def _conv_stack_bwd_open(self, gc):
        gc['dout'] = self.tmp('dgc_all', (gc['rows'], gc['ld']))

    def _conv_stack_bn_bwd(self, gc, k, bn, dy, x):
        """head k's BatchNorm backward into its column slice of the stacked gradient; the conv's wgrad / dgrad run once for all heads"""
        n = gc['n']
        self._bn_bwd(gc['heads'][k].norm, bn, dy, None, x, gc['dout'][:, k * n:], gc['rows'], n, ldx=gc['ld'], lddx=gc['ld'])

    def _conv_stack_bwd_close(self, gc, x, dx, cin=None, wgrad=None, dgrad=None, **dg_kw):
        """weight gradients of all heads (one launch on the weight-gradient lane, rows k*n.. -> head k's weight / bias gradient), then
        the data gradient into dx; dg_kw: the caller's own keywords of that GEMM.  A family with a product form of its own passes
        wgrad(G, gb, label) / dgrad(label) and cin, the columns of one head's weight matrix"""
        Bk, dt = self.bwd, self.dt
        rows, C, ld = gc['rows'], gc['C'], gc['ld']
        wg, dg = gc['tag'] + '.all.wg', gc['tag'] + '.all.dg'
        G, gb = self.gbuf((ld, cin or C)), self.gbuf((ld,)) if gc['heads'][0].b else None
        with self._wlane():
            if wgrad:
                wgrad(G, gb, wg)
            else:
                Bk.wgrad(gc['dout'], x, G, rows, ld, C, dt, dbias=gb, label=wg)
        self._stack_scatter(G, gb, gc['heads'])
        if dgrad:
            dgrad(dg)
        else:
            Bk.gemm(gc['dout'], gc['WT'], dx, rows, C, ld, dt, label=dg, **dg_kw)

    # ------------------------------------------------------------------------------------------
    # stacked classifiers: the inputs of the K heads in one [K][B][cin] buffer, weights stacked -> one batched GEMM into a slice
    # of the logits; backward one batched wgrad and one batched dgrad
    # ------------------------------------------------------------------------------------------
    def _fc_stack(self, name, K, cin, heads=None):
        """buffers of stack `name` and, for the heads given, their weights and biases into it (heads=None: the family fills them)"""
        B, NC, dt, P, T = self.B, self.cfg['num_classes'], self.dt, self.P, self.training
        ldn = pad8(NC)
        fc = dict(name=name, heads=heads, K=K, cin=cin, x=self.act(f'fc.{name}.x', (K, B, cin)))
        fc['W'] = self.buf(f'w.fc.{name}', (K, NC, cin))
        fc['WT'] = self.buf(f'wT.fc.{name}', (K, cin, ldn)) if T else None
        fc['b'] = self.buf(f'w.fc.{name}.b', (K, NC), torch.float32)
        for k, hd in enumerate(heads or ()):
            self.prep.weight_prep(P[hd.w], 1, NC, cin, 1, 1, dt, out=fc['W'][k], ldo=cin, outT=fc['WT'][k] if T else None,
                                  ldt=ldn if T else 0, label=hd.prep)
            self.prep.bias_fold(None, P[hd.b], None, None, fc['b'][k], NC, cin)
        return fc

    def _fc_stack_fwd(self, fc, logits):
        B, NC, K, cin = self.B, self.cfg['num_classes'], fc['K'], fc['cin']
        self.fwd.gemm(fc['x'], fc['W'], logits, B, NC, cin, self.dt, batch=K, strideA=B * cin, strideB=NC * cin, strideC=B * NC,
                      bias=fc['b'], strideBias=NC, c_f32=True, label='fc.' + fc['name'])

    def _fc_stack_bwd(self, fc, dlogits, name, scatter=None):
        """name: of the backward's labels and of the transient fc['dx'] [K][B][cin]; scatter(G, gb, heads): the family's own way from
        the stacked weight gradient to the parameters' gradients (default: added row block by row block)"""
        Bk, B, NC, K, cin = self.bwd, self.B, self.cfg['num_classes'], fc['K'], fc['cin']
        G, gb = self.gbuf((K, NC, cin)), self.gbuf((K, NC))
        Bk.wgrad(dlogits, fc['x'], G, B, NC, cin, self.dt, batch=K, strideY=B * NC, strideX=B * cin, strideW=NC * cin, dbias=gb,
                 strideDbias=NC, label=f'fc.{name}.wg')
        (scatter or self._stack_scatter)(G, gb, fc['heads'])
        fc['dx'] = self.tmp('dfc.' + name, (K, B, cin))
        Bk.gemm(dlogits, fc['WT'], fc['dx'], B, cin, NC, self.dt, batch=K, strideA=B * NC, strideB=cin * pad8(NC), ldb=pad8(NC),
                strideC=B * cin, label=f'fc.{name}.dg')
