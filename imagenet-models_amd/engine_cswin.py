"""CSWinEngine: the static launch plans (weight prep / forward / backward) of one GA_CSWinTransformer for a fixed
(batch, train|eval, math mode): engine_base.EngineBase (buffers, plans, BatchNorm helpers) + engine.GAHeads (aggregation,
SE-Bottleneck, GroupConvMlp, the whole GA head); the trunk is restated here from /root/reference/GA/ga_cswin.py:

  deep stem :463-477 ........ NCHW fp32 -> NHWC8 pack, three 3x3 convs as gather GEMMs (s2, s1, s2), LayerNorm+GELU fused
  CSWinBlock :191-212 ....... LN1 (affine folded into qkv) -> qkv GEMM -> stripe attention + LePE (one kernel for both
                              branches, windows addressed in place) -> proj GEMM (+DropPath, +residual) -> LN2 (folded)
                              -> fc1+GELU(+GELU') -> fc2 (+DropPath, +residual);  GroupConvMlp when mlp_groups > 1:
                              engine_blocks.TransformerBlocks with cswin_block's facts (StripeAttention)
  Merge_Block :253-268 ...... 3x3 s2 gather GEMM (+bias) -> LayerNorm; data gradient as a transposed-conv GEMM
  aggregation :666-669 ...... avg-pool / taps / bilinear x2 into one concat buffer (ga_pool_concat)
  stage5 :531-542 ........... Merge_Block_LCF (1x1) + CSWinBlock, or the SE-Bottleneck
  heads :677-692 ............ grouped (g=8) gram_contraction + BN -> CSWinBlock(192, 6 heads) -> Gram -> grouped embed + BN
                              -> class attention (q/k/v width C/4) -> fc
"""
import os

import torch

from . import ops
from .engine import GAHeads
from .engine_base import EngineBase, pad8
from .engine_blocks import BlockSpec, StripeAttention, TransformerBlocks
from .ops import A_CONV3, A_CONV3S2, A_NEIGH2, C_UNPATCH2


def tap_after(nblocks, naggre):
    """ga_cswin.py:659 -- 1-based block counts of stage3 after which a tap is taken"""
    step = nblocks // (naggre + 1)
    taps = []
    for b in range(1, nblocks + 1):
        if b % step == 0 and len(taps) < naggre:
            taps.append(b)
    return taps


def cswin_block(mod):
    """ga_cswin.py:191-212 -- the facts of CSWinBlock `mod` (its parameter holder: geometry) for TransformerBlocks"""
    return BlockSpec(C=mod.dim, heads=mod.num_heads, ntok=mod.reso * mod.reso, eps=1e-5, qkv='qkv.', proj='proj.',
                     mlp_groups=mod.mlp_groups, attn=StripeAttention(mod))


class CSWinEngine(TransformerBlocks, GAHeads, EngineBase):
    # ------------------------------------------------------------------------------------------
    def _drop_path_rates(self):
        """ga_cswin.py:486 (linspace over the 4 trunk stages), :538,571 (stage5 and gram layers: dpr[-1]), :541 (Bottleneck:
        drop_path_rate).  A CSWinBlock applies DropPath twice (attention branch, MLP branch: :209-210) -- two sites '#1', '#2'."""
        cfg = self.cfg
        dep, rate = cfg['depth'], cfg['drop_path_rate']
        dpr = torch.linspace(0, rate, sum(dep)).tolist()
        out, i = {}, 0
        for si in range(4):
            for j in range(dep[si]):
                out[f'stage{si + 1}.{j}.#1'] = out[f'stage{si + 1}.{j}.#2'] = dpr[i]
                i += 1
        if cfg['stage5'] == 'CSWin':
            out['stage5.2.#1'] = out['stage5.2.#2'] = dpr[-1]
        else:
            out['stage5.'] = float(rate)
        for k in range(cfg['branches']):
            out[f'gram_layer.{k}.1.#1'] = out[f'gram_layer.{k}.1.#2'] = dpr[-1]
            out[f'ga.{k}.'] = 0.0
        return out

    # ------------------------------------------------------------------------------------------
    # 3x3 / stride-2 conv (+bias) -> LayerNorm   (Merge_Block; the last stem conv without bias)
    # ------------------------------------------------------------------------------------------
    def _conv3s2_ln_fwd(self, cname, nname, x, Hin, Cin, Cout, bias):
        F, dt, B, P, T = self.fwd, self.dt, self.B, self.P, self.training
        Ho = Hin // 2
        Mo = B * Ho * Ho
        (lane, r0, r1, b0, b1), = self._fsplits(Ho * Ho)           # output rows of this forward chain (whole images)
        i0, i1 = b0 * Hin * Hin, b1 * Hin * Hin
        if self._chain is not None:
            F.lane = lane
        Wf = self._w_plain(cname + 'weight', Cout, Cin, 3, 3, need_T=False)
        st = dict(x=x, Hin=Hin, Cin=Cin, Cout=Cout, cname=cname, nname=nname, bias=bias)
        if T:
            first = ('wD.' + cname) not in self.bufs
            st['Bt'] = self.buf('wD.' + cname, (4 * Cin, pad8(4 * Cout)))
            if first:
                self.prep.conv3s2_dgrad_prep(P[cname + 'weight'], st['Bt'], Cout, Cin, pad8(4 * Cout), dt, label='prep.' + cname + 'dgrad')
        st['c'] = self.act(cname + 'out', (Mo, Cout))
        F.gemm(x[i0:i1], Wf, st['c'][r0:r1], r1 - r0, Cout, 9 * Cin, dt, ldb=pad8(9 * Cin), a_kind=A_CONV3S2, a_dims=(Hin, Hin, Cin),
               bias=P[cname + 'bias'] if bias else None, label=cname + 'conv')
        st['mean'] = self.act(nname + 'mean', (Mo,), torch.float32)
        st['rstd'] = self.act(nname + 'rstd', (Mo,), torch.float32)
        y = self.buf(nname + 'out', (Mo, Cout))
        F.layernorm_fwd(st['c'][r0:r1], P[nname + 'weight'], P[nname + 'bias'], y[r0:r1], st['mean'][r0:r1], st['rstd'][r0:r1], r1 - r0,
                        Cout, 1e-5, dt, label=nname + 'ln')
        return y, st

    def _conv3s2_ln_bwd(self, st, dy, dprev, seed=None):
        """dy: gradient wrt the LayerNorm output; dprev (+= seed) = gradient wrt the conv input"""
        Bk, dt, B, P = self.bwd, self.dt, self.B, self.P
        Hin, Cin, Cout, cname, nname = st['Hin'], st['Cin'], st['Cout'], st['cname'], st['nname']
        Ho = Hin // 2
        Mo, Mi = B * Ho * Ho, B * Hin * Hin
        dc = self.tmp('dconv', (Mo, Cout))
        Bk.layernorm_bwd(dy, st['c'], st['mean'], st['rstd'], P[nname + 'weight'], None, dc, self.grad(nname + 'weight'),
                         self.grad(nname + 'bias'), Mo, Cout, False, dt, label=nname + 'lnb')
        G = self.gbuf((Cout, 9 * Cin))
        with self._wlane():
            Bk.wgrad(dc, st['x'], G, Mo, Cout, 9 * Cin, dt, x_kind=A_CONV3S2, x_dims=(Hin, Hin, Cin),
                     dbias=self.grad(cname + 'bias') if st['bias'] else None, label=cname + 'wg')
        Bk.weight_unfold(G, 9 * Cin, Cout, Cin, 3, 3, dW=self.grad(cname + 'weight'), label=cname + 'unf')
        if dprev is not None:
            Bk.gemm(dc, st['Bt'], dprev, Mo, 4 * Cin, 4 * Cout, dt, ldb=pad8(4 * Cout), a_kind=A_NEIGH2, a_dims=(Ho, Ho, Cout),
                    c_kind=C_UNPATCH2, c_dims=(Hin, Hin, Cin), label=cname + 'dg')
            if seed is not None:
                Bk.affine_act(dprev, None, None, seed, dprev, Mi, Cin, False, dt, label=cname + 'seed')

    # ------------------------------------------------------------------------------------------
    # build
    # ------------------------------------------------------------------------------------------
    def _build(self):
        cfg, m = self.cfg, self.m
        B, T, F, dt, P = self.B, self.training, self.fwd, self.dt, self.P
        e, d, dep = cfg['embed_dim'], cfg['dims'], cfg['depth']
        img = self.img
        self._init_group_mlp()
        self._lepe_ws_elems = 0      # floats of the largest LePE weight-gradient partial buffer a block's backward asks for
        if T:
            F.zero(self.bn_pool, label='zero.bn_sums')
        # ---------------- deep stem (ga_cswin.py:463-477) ----------------
        sp = 'stage1_conv_embed.'
        H1 = img // 2
        M1 = B * H1 * H1
        W0 = self._image_pack8_stem(sp + '0', e)
        W1 = self._w_plain(sp + '5.weight', e, e, 3, 3, flip=True)
        S = self.stem = {}
        S['c0'] = self.act(sp + 'c0', (M1, e))
        S['a0'] = self.act(sp + 'a0', (M1, e))
        S['m0'], S['r0'] = self.act(sp + 'm0', (M1,), torch.float32), self.act(sp + 'r0', (M1,), torch.float32)
        S['c1'] = self.act(sp + 'c1', (M1, e))
        S['a1'] = self.act(sp + 'a1', (M1, e))
        S['m1'], S['r1'] = self.act(sp + 'm1', (M1,), torch.float32), self.act(sp + 'r1', (M1,), torch.float32)
        stages = [m.stage1, m.stage2, m.stage3, m.stage4]
        taps_at = tap_after(dep[2], cfg['naggre'])
        # one pass per forward chain (batch part, EngineBase._chains): with GAEXT_FWD_SPLIT > 1 the deep stem and the four stages run as
        # independent chains on side streams -- every op of the trunk is per image, and its launches are too small to fill the chip
        # alone (the step timeline had one kernel running for 23 of 39 ms); every pass names the same full-batch buffers
        chains = self._chains()
        if any(mod.mlp_groups != 1 for st_ in stages for mod in st_):
            chains = [(0, 0, B)]
        for chain in chains:
            self._chain = chain if len(chains) > 1 else None
            (lane, r0, r1, b0, b1), = self._fsplits(H1 * H1)
            F.lane = lane
            F.gemm(self.x8[b0 * img * img:b1 * img * img], W0, S['c0'][r0:r1], r1 - r0, e, 72, dt, a_kind=A_CONV3S2, a_dims=(img, img, 8),
                   label=sp + 'conv0')
            F.layernorm_gelu_fwd(S['c0'][r0:r1], P[sp + '2.weight'], P[sp + '2.bias'], S['a0'][r0:r1], S['m0'][r0:r1], S['r0'][r0:r1],
                                 r1 - r0, e, 1e-5, dt, label=sp + 'ln0')
            F.gemm(S['a0'][r0:r1], W1, S['c1'][r0:r1], r1 - r0, e, 9 * e, dt, ldb=pad8(9 * e), a_kind=A_CONV3, a_dims=(H1, H1, e),
                   label=sp + 'conv1')
            F.layernorm_gelu_fwd(S['c1'][r0:r1], P[sp + '7.weight'], P[sp + '7.bias'], S['a1'][r0:r1], S['m1'][r0:r1], S['r1'][r0:r1],
                                 r1 - r0, e, 1e-5, dt, label=sp + 'ln1')
            x, S['conv2'] = self._conv3s2_ln_fwd(sp + '10.', sp + '12.', S['a1'], H1, e, d[0], bias=False)
            # ---------------- stages 1..4 ----------------
            feats, taps, self.merges = [], [], {}
            for si in range(4):
                if si > 0:
                    x, self.merges[si] = self._conv3s2_ln_fwd(f'merge{si}.conv.', f'merge{si}.norm.', x, stages[si - 1][0].reso,
                                                              d[si - 1], d[si], bias=True)
                for j, mod in enumerate(stages[si]):
                    x = self._tblock_fwd(f'stage{si + 1}.{j}.', x, cswin_block(mod))
                    if si == 2 and (j + 1) in taps_at:
                        taps.append((x, j))
                feats.append((x, stages[si][0].reso))
        self._chain = None
        F.lane = 0
        # ---------------- aggregate (ga_cswin.py:666-669) ----------------
        Hc = img // 16
        M4 = B * Hc * Hc
        assert len(taps) == cfg['naggre'], (len(taps), cfg['naggre'])
        cat, ctot = self._aggregate_fwd(feats, [t for t, _ in taps], d, Hc)
        assert ctot == sum(d) + d[2] * cfg['naggre']
        # ---------------- stage5 ----------------
        cur = d[3]
        self.cout = cur
        if cfg['stage5'] == 'CSWin':
            lp = 'stage5.1.'
            W5 = self._w_plain(lp + 'conv.weight', cur, ctot, 1, 1)
            L = self.lcf = dict(c=self.act(lp + 'c', (M4, cur)), mean=self.act(lp + 'mean', (M4,), torch.float32),
                                rstd=self.act(lp + 'rstd', (M4,), torch.float32))
            F.gemm(cat, W5, L['c'], M4, cur, ctot, dt, ldb=pad8(ctot), bias=P[lp + 'conv.bias'], label=lp + 'conv')
            t5 = self.buf(lp + 'out', (M4, cur))
            F.layernorm_fwd(L['c'], P[lp + 'norm.weight'], P[lp + 'norm.bias'], t5, L['mean'], L['rstd'], M4, cur, 1e-5, dt,
                            label=lp + 'ln')
            L['t5'] = t5
            x4 = self._tblock_fwd('stage5.2.', t5, cswin_block(m.stage5[2]))
        else:
            x4 = self._bottleneck_fwd(cat, M4, ctot, cur, pre='stage5.')
        # ---------------- heads ----------------
        self._build_heads(x4, M4, Hc)
        # ---------------- backward ----------------
        if T:
            self._build_backward(feats, taps, x4, M4, ctot, cat)

    # ------------------------------------------------------------------------------------------
    # grouped gram_contraction of all heads (ga_cswin.py:559-561): ONE batched GEMM, batch = heads x 8 groups
    # ------------------------------------------------------------------------------------------
    def _contract_all_fwd(self, x4, M4):
        cfg, T, F, dt, cout, P = self.cfg, self.training, self.fwd, self.dt, self.cout, self.P
        K, g_, gg = cfg['branches'], cfg['gram_dim'], cfg['gram_groups']
        gpo, cpi = g_ // gg, cout // gg
        assert g_ % gg == 0 and gpo % 8 == 0 and cpi % 8 == 0, 'grouped gram_contraction needs 8-aligned group widths'
        gc = self.gcon = self._conv_stack('gram_contraction', M4, cout, g_, self._contraction_heads())
        gc.update(gpo=gpo, cpi=cpi, dense=False)
        if dt == ops.GA_BF16 and os.environ.get('GAEXT_GC_DENSE', '1') != '0':
            # the five grouped convs as ONE dense product over block-diagonal weights ([K g_] x cout, zeros off the diagonal blocks):
            # 8 x the MACs of the grouped form, but one ring-form launch with N = 960 instead of 40 products with N = 24 whose 48-byte
            # output rows are partial cache lines (0.196 -> 0.07 ms forward; the data gradient of all heads one launch as well)
            gc['dense'] = True
            gc['Wm'] = self.buf('pad.gram_contraction.bd', (K * g_, cout), torch.float32, zero=True)     # block-diagonal fp32 master
            for k in range(K):
                self.prep.blockdiag_f32(P[f'gram_contraction.{k}.0.weight'], gc['Wm'][k * g_:], g_, gpo, gg, cpi, cout,
                                        label=f'prep.gram_contraction.{k}.bd')
            gc['Wd'] = self.buf('w.gram_contraction.bd', (K * g_, cout))
            gc['WdT'] = self.buf('wT.gram_contraction.bd', (cout, pad8(K * g_))) if T else None
            self.prep.weight_prep(gc['Wm'], 1, K * g_, cout, 1, 1, dt, out=gc['Wd'], ldo=cout, outT=gc['WdT'],
                                  ldt=pad8(K * g_) if T else 0, label='prep.gram_contraction.bd')
            gc['b'] = self.buf('w.gram_contraction.ball', (K * g_,), torch.float32)
            gc['s'], gc['q'] = self._bn_pool(K * g_), self._bn_pool(K * g_)
            for k in range(K):
                self.prep.bias_fold(None, P[f'gram_contraction.{k}.0.bias'], None, None, gc['b'][k * g_:], g_, cpi)
            gc['out'] = self.act('gram_contraction.all.out', (M4, K * g_))
            F.gemm(x4, gc['Wd'], gc['out'], M4, K * g_, cout, dt, bias=gc['b'], colsum=gc['s'] if T else None,
                   colsumsq=gc['q'] if T else None, label='gram_contraction.all')
            return
        gc['W'] = self.buf('w.gram_contraction.all', (K * g_, cpi))
        gc['WT'] = self.buf('wT.gram_contraction.all', (K, gg * cpi, pad8(gpo))) if T else None
        gc['b'] = self.buf('w.gram_contraction.ball', (K * g_,), torch.float32)
        gc['s'], gc['q'] = self._bn_pool(K * g_), self._bn_pool(K * g_)
        for k in range(K):
            pre = f'gram_contraction.{k}.'
            self.prep.weight_prep(P[pre + '0.weight'], gg, gpo, cpi, 1, 1, dt, out=gc['W'][k * g_:], ldo=cpi,
                                  outT=gc['WT'][k] if T else None, ldt=pad8(gpo) if T else 0, label='prep.' + pre + 'w')
            self.prep.bias_fold(None, P[pre + '0.bias'], None, None, gc['b'][k * g_:], g_, cpi)
        gc['out'] = self.act('gram_contraction.all.out', (M4, K * g_))
        F.gemm(x4, gc['W'], gc['out'], M4, gpo, cpi, dt, lda=cout, ldb=cpi, ldc=K * g_, batch=K * gg, a_batch_mod=gg, strideA=cpi,
               strideB=gpo * cpi, strideC=gpo, bias=gc['b'], strideBias=gpo, colsum=gc['s'] if T else None,
               colsumsq=gc['q'] if T else None, strideCol=gpo, label='gram_contraction.all')

    def _contract_all_bwd(self, x4, dx4, M4):
        Bk, dt, cfg, cout = self.bwd, self.dt, self.cfg, self.cout
        K, g_, gg = cfg['branches'], cfg['gram_dim'], cfg['gram_groups']
        gcn = self.gcon
        gpo, cpi = gcn['gpo'], gcn['cpi']
        R = None if self.shared_tok else dx4     # the first launch is the first writer of dx4 on the shared-token path

        if gcn['dense']:
            def wgrad(Gc, gbc, label):
                Gd = self.gbuf((K * g_, cout))
                Bk.wgrad(gcn['dout'], x4, Gd, M4, K * g_, cout, dt, dbias=gbc, label=label)
                Bk.blockdiag_f32(Gd, Gc, K * g_, gpo, gg, cpi, cout, to_diag=False, label=label + '.diag')

            def dgrad(label):
                Bk.gemm(gcn['dout'], gcn['WdT'], dx4, M4, cout, K * g_, dt, ldb=pad8(K * g_), R=R, ldr=cout, label=label)
        else:
            def wgrad(Gc, gbc, label):
                Bk.wgrad(gcn['dout'], x4, Gc, M4, gpo, cpi, dt, ldy=K * g_, ldx=cout, ldw=cpi, batch=K * gg, strideY=gpo, strideX=cpi,
                         x_batch_mod=gg, strideW=gpo * cpi, dbias=gbc, strideDbias=gpo, label=label)

            def dgrad(label):       # grouped data gradient, one batched GEMM per head
                for k in range(K):
                    Bk.gemm(gcn['dout'][:, k * g_:], gcn['WT'][k], dx4, M4, cpi, gpo, dt, lda=K * g_, ldb=pad8(gpo), ldc=cout, batch=gg,
                            strideA=gpo, strideB=cpi * pad8(gpo), strideC=cpi, R=R if k == 0 else dx4, ldr=cout, strideR=cpi,
                            label=f'gram_contraction.{k}.dg')
        self._conv_stack_bwd_close(gcn, x4, dx4, cin=cpi, wgrad=wgrad, dgrad=dgrad)

    # gram_layer[k] = CSWinBlock(gram_dim, 6 heads) at 14 x 14 (ga_cswin.py:564-574)
    def _gram_layer_fwd(self, h, k, Hc):
        h['blk'] = f'gram_layer.{k}.1.'
        return self._tblock_fwd(h['blk'], h['g0'], cswin_block(self.m.gram_layer[k][1]))

    def _gram_layer_bwd(self, h, dg1, dg0):
        self._tblock_bwd(h['blk'], dg1, dg0)

    # ------------------------------------------------------------------------------------------
    # whole-network backward plan
    # ------------------------------------------------------------------------------------------
    def _build_backward(self, feats, taps, x4, M4, ctot, cat):
        Bk, dt, B, P, W, cfg, m = self.bwd, self.dt, self.B, self.P, self.W, self.cfg, self.m
        d, dep, e = cfg['dims'], cfg['depth'], cfg['embed_dim']
        cur = self.cout
        dx4 = self._build_heads_backward(x4, M4)
        dcat = self.tmp('dcat', (M4, ctot))
        if cfg['stage5'] == 'CSWin':
            L = self.lcf
            lp = 'stage5.1.'
            dt5 = self.tmp('dt5', (M4, cur))
            self._tblock_bwd('stage5.2.', dx4, dt5)
            dc5 = self.tmp('dc5', (M4, cur))
            Bk.layernorm_bwd(dt5, L['c'], L['mean'], L['rstd'], P[lp + 'norm.weight'], None, dc5, self.grad(lp + 'norm.weight'),
                             self.grad(lp + 'norm.bias'), M4, cur, False, dt, label=lp + 'lnb')
            with self._wlane():
                Bk.wgrad(dc5, cat, self.grad(lp + 'conv.weight'), M4, cur, ctot, dt, dbias=self.grad(lp + 'conv.bias'),
                         label=lp + 'wg')
            Bk.gemm(dc5, W[lp + 'conv.weight.T'], dcat, M4, ctot, cur, dt, ldb=pad8(cur), label=lp + 'dg')
        else:
            self._bottleneck_bwd(dx4, dcat)
        self._seal('heads', 'stage5.', 'gram_contraction.', 'gram_layer.', 'gram_embedding.', 'ga.', 'fc.', flush='heads.',
                   then=self._unpad_all)
        # aggregate backward -> gradient seeds of the stage outputs / taps
        seeds = self._aggregate_bwd(dcat, ctot, 14)
        ntap = len(taps)
        d_taps = {j: seeds[2 + i] for i, (_, j) in enumerate(taps)}
        seed = {0: seeds[0], 1: seeds[1], 2: seeds[2 + ntap], 3: seeds[3 + ntap]}
        stages = [m.stage1, m.stage2, m.stage3, m.stage4]
        dy = seed[3]
        for si in (3, 2, 1, 0):
            reso = stages[si][0].reso
            Mi = B * reso * reso
            pp = [self.tmp(f'dxA{si}', (Mi, d[si])), self.tmp(f'dxB{si}', (Mi, d[si])), self.tmp(f'dxC{si}', (Mi, d[si]))]
            turn = 0
            for j in reversed(range(dep[si])):
                if si == 2 and j in d_taps:
                    Bk.affine_act(dy, None, None, d_taps[j], dy, Mi, d[si], False, dt, label=f'tap.add.{j}')
                dx = pp[turn % 3]          # not this block's dy nor the previous block's (still read by its asynchronous wgrads)
                turn += 1
                # the next block of the chain takes dx unchanged as its dy unless a tap gradient is added in between
                nxt = f'stage{si + 1}.{j - 1}.' if j > 0 and not (si == 2 and (j - 1) in d_taps) else None
                self._tblock_bwd(f'stage{si + 1}.{j}.', dy, dx, next_pre=nxt)
                dy = dx
            if si > 0:
                Hp = stages[si - 1][0].reso
                dprev = self.tmp(f'dprev{si}', (B * Hp * Hp, d[si - 1]))
                self._conv3s2_ln_bwd(self.merges[si], dy, dprev, seed=seed[si - 1])
                dy = dprev
            # gradients of trunk stage si+1 (incl. its merge) are final; stage1's stay with the stem's, under the end of the plan
            self._seal(f'stage{si}', *((f'stage{si + 1}.', f'merge{si}.') if si > 0 else ()), flush=f'stage{si + 1}.')
        # ---------------- deep stem ----------------
        S = self.stem
        sp = 'stage1_conv_embed.'
        H1 = self.img // 2
        M1 = B * H1 * H1
        da1 = self.tmp('stem.da1', (M1, e))
        self._conv3s2_ln_bwd(S['conv2'], dy, da1)
        dc1 = self.tmp('stem.dc', (M1, e))
        Bk.layernorm_gelu_bwd(da1, S['c1'], S['m1'], S['r1'], P[sp + '7.weight'], P[sp + '7.bias'], dc1, self.grad(sp + '7.weight'),
                              self.grad(sp + '7.bias'), M1, e, dt, label=sp + 'ln1b')
        G1 = self.gbuf((e, 9 * e))
        with self._wlane():
            Bk.wgrad(dc1, S['a0'], G1, M1, e, 9 * e, dt, x_kind=A_CONV3, x_dims=(H1, H1, e), label=sp + 'conv1.wg')
        Bk.weight_unfold(G1, 9 * e, e, e, 3, 3, dW=self.grad(sp + '5.weight'), label=sp + 'conv1.unf')
        da0 = da1   # da1 is dead after the LayerNorm+GELU backward above
        Bk.gemm(dc1, W[sp + '5.weight.T'], da0, M1, e, 9 * e, dt, a_kind=A_CONV3, a_dims=(H1, H1, e), ldb=pad8(9 * e),
                label=sp + 'conv1.dg')
        dc0 = self.tmp('stem.dc0', (M1, e))   # dc1 is still read by the asynchronous conv1 weight gradient
        Bk.layernorm_gelu_bwd(da0, S['c0'], S['m0'], S['r0'], P[sp + '2.weight'], P[sp + '2.bias'], dc0, self.grad(sp + '2.weight'),
                              self.grad(sp + '2.bias'), M1, e, dt, label=sp + 'ln0b')
        G0 = self.gbuf((e, 72))
        with self._wlane():
            Bk.wgrad(dc0, self.x8, G0, M1, e, 72, dt, x_kind=A_CONV3S2, x_dims=(self.img, self.img, 8), label=sp + 'conv0.wg')
            Bk.convw_unpack_grad(G0, self.grad(sp + '0.weight'), e, 3, 9, 8, 72, label=sp + 'conv0.unf')   # same lane: after the wgrad
