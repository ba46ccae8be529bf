"""MAPViTEngine: launch plans of a ViT trunk (timm VisionTransformer: PatchEmbed, cls_token + pos_embed, `Block`s -- the block the
reference uses through /root/reference/MAP/models/map_pit.py:14,35-44) feeding the MAP head (engine_map.MAPHead, map.py).  The block itself is
engine_blocks.TransformerBlocks with timm_block's facts, which the PiT trunk records too.

The composition (BASELINE configs[4] "MAP-ViT-B/16 @ 384") is builder-defined, modelled on how map_pit.py attaches the head
(PoolingTransformer.forward_features :185-201: the position-embedded patch tokens and the output of every stage are the feature
maps handed to MAPHead): here the 12 blocks are cut into three equal "stages"; features = [tokens after pos_embed, after block
d/3, after block 2d/3, final norm of the last block], class token dropped, each a (B, C, H/16, W/16) map.  MultiScale resizes
them to half that resolution (bilinear reduction, as map.py:322-333 does for maps above its level's size).

Trunk kernels: ga_patchify + ga_gemm (patch embedding), ga_vit_embed, per block LayerNorm(1e-6, affine folded into the next
linear) -> qkv ga_gemm -> ga_attn (global attention, flash-style MFMA in bf16) -> proj ga_gemm (+ DropPath + residual) ->
LayerNorm -> fc1 (+GELU) -> fc2 (+ DropPath + residual); weight gradients on the asynchronous lane as in the other engines.
"""
import torch

from . import ops  # noqa: F401
from .engine_base import EngineBase
from .engine_blocks import TransformerBlocks, timm_block
from .engine_map import MAPHead


class MAPViTEngine(TransformerBlocks, MAPHead, EngineBase):
    def _drop_path_rates(self):
        """timm VisionTransformer: linspace(0, drop_path_rate, depth); a Block applies it to both branches"""
        cfg = self.cfg
        dpr = torch.linspace(0, cfg['drop_path_rate'], cfg['depth']).tolist()
        out = {}
        for i in range(cfg['depth']):
            out[f'blocks.{i}.#1'] = out[f'blocks.{i}.#2'] = dpr[i]
        return out

    def _build(self):
        cfg = self.cfg
        B, T, F, dt, P = self.B, self.training, self.fwd, self.dt, self.P
        img = self.img
        C, depth, heads, ps = cfg['embed_dim'], cfg['depth'], cfg['vit_heads'], cfg['patch_size']
        gw = img // ps
        Np, Ntok = gw * gw, gw * gw + 1
        M, Mp = B * Ntok, B * Np
        K0 = 3 * ps * ps
        if T:
            F.zero(self.bn_pool, label='zero.bn_sums')
        # ---------------- patch embedding + class token + position embedding ----------------
        self.x_placeholder = torch.zeros(B, 3, img, img, device=self.dev)
        patches = self.patches = self.act('patch.cols', (Mp, K0))
        self.input_call = len(F.calls)
        F.patchify(self.x_placeholder, patches, ps, dt, label='patch.pack')
        Wpe = self._w_plain('patch_embed.proj.weight', C, K0, 1, 1, need_T=False)
        tok = self.tmp('patch.tok', (Mp, C))
        x0 = self.buf('embed.x0', (M, C))
        spec = timm_block(C, heads, Ntok)
        taps = cfg['taps']                                   # block counts after which a feature map is taken (the last = depth)
        # ---------------- embedding, blocks, feature taps: one pass per forward chain (batch part on its own lane) ----------------
        chains = self._chains()
        for chain in chains:
            self._chain = chain if len(chains) > 1 else None
            (lane, r0, r1, b0, b1), = self._fsplits(Ntok)
            F.lane = lane
            p0, p1, nb = b0 * Np, b1 * Np, b1 - b0
            F.gemm(patches[p0:p1], Wpe, tok[p0:p1], p1 - p0, C, K0, dt, bias=P['patch_embed.proj.bias'], label='patch.proj')
            F.vit_embed_fwd(tok[p0:p1], P['cls_token'], P['pos_embed'], x0[r0:r1], nb, Np, C, dt, label='embed')
            x = x0
            feats = [self._tokens_to_map(x, 'f0', B, Np, Ntok, C)]
            self.tap_at = {}
            for i in range(depth):
                x = self._tblock_fwd(f'blocks.{i}.', x, spec)
                if i + 1 in taps:
                    self.tap_at[i + 1] = len(feats)
                    fm = self._tokens_to_map(x, f'f{len(feats)}', B, Np, Ntok, C)
                    if i + 1 == depth:       # final norm (timm forward_features) on the map rows: LayerNorm is per token
                        self.fn = dict(x=fm, y=self.act('norm.out', (Mp, C)), m=self.act('norm.m', (Mp,), torch.float32),
                                       r=self.act('norm.r', (Mp,), torch.float32))
                        F.layernorm_fwd(fm[p0:p1], P['norm.weight'], P['norm.bias'], self.fn['y'][p0:p1], self.fn['m'][p0:p1],
                                        self.fn['r'][p0:p1], p1 - p0, C, 1e-6, dt, label='norm')
                        fm = self.fn['y']
                    feats.append(fm)
        self._chain = None
        F.lane = 0
        self.x_last = x
        # ---------------- MultiScale: every map (gw x gw) reduced to gw/2 x gw/2, concat, conv1x1 + BN + GELU ----------------
        Hc = gw // 2
        M4 = B * Hc * Hc
        cat, ctot = self._ms_concat_fwd([(fm, gw, C) for fm in feats], Hc, labels=[f'agg.{j}' for j in range(len(feats))])
        xh = self._multi_scale_conv_fwd(cat, M4, ctot)
        self._build_map_head(xh, M4, Hc)
        if T:
            self._build_vit_backward(xh, M4, feats, B, Np, Ntok, C, M, Mp, K0)

    def _tokens_to_map(self, x, name, B, Np, Ntok, C):
        """drop the class token: rows 1.. of every image -> [B*Np, C] (the images of the current forward chain)"""
        fm = self.act('feat.' + name, (B * Np, C))
        (lane, r0, r1, b0, b1), = self._fsplits(Ntok)
        self.fwd.copy2d(x[r0 + 1:], Ntok * C, fm[b0 * Np:], Np * C, b1 - b0, Np * C, self.dt, label='feat.' + name)
        return fm

    def _build_vit_backward(self, xh, M4, feats, B, Np, Ntok, C, M, Mp, K0):
        Bk, dt, P, cfg = self.bwd, self.dt, self.P, self.cfg
        depth, gw = cfg['depth'], self.img // cfg['patch_size']
        seeds = self._ms_concat_bwd(self._build_head_backward(xh, M4))
        # gradient of the token sequence, three rotating buffers (the asynchronous weight gradients read dx of the block before)
        dxs = [self.buf(f'vit.dx{j}', (M, C)) for j in range(3)]
        cur = 0
        # last feature: through the final norm, into rows 1.. of a zeroed sequence gradient
        dfm = self.tmp('dnorm', (Mp, C))
        Bk.layernorm_bwd(seeds[-1], self.fn['x'], self.fn['m'], self.fn['r'], P['norm.weight'], None, dfm, self.grad('norm.weight'),
                         self.grad('norm.bias'), Mp, C, False, dt, label='normb')
        Bk.zero(dxs[cur], label='zero.dx')
        Bk.copy2d(dfm, Np * C, dxs[cur][1:], Ntok * C, B, Np * C, dt, label='feat.last.b')
        for i in range(depth - 1, -1, -1):
            nxt = (cur + 1) % 3
            j = self.tap_at.get(i) if i > 0 else 0           # the feature taken at this block's INPUT (after block i; 0 = the embedding)
            self._tblock_bwd(f'blocks.{i}.', dxs[cur], dxs[nxt], next_pre=f'blocks.{i - 1}.' if i > 0 and j is None else None)
            cur = nxt
            if j is not None:
                Bk.copy2d(seeds[j], Np * C, dxs[cur][1:], Ntok * C, B, Np * C, dt, accumulate=True, label=f'feat.{j}.b')
            if i == depth // 2:
                # every gradient of blocks[depth // 2 :] and of the final norm must be FINAL at the mark (TrainStep all-reduces
                # the group's slice from here on): wait for the weight-gradient lane, emit the deferred unfold jobs
                self._seal('stage2', 'norm.', *(f'blocks.{k}.' for k in range(depth // 2, depth)), flush='stage2.')
        # embedding: dtok, d(cls_token), d(pos_embed); patch projection weight gradient
        dtok = self.tmp('dtok', (Mp, C))
        Bk.vit_embed_bwd(dxs[cur], dtok, self.grad('cls_token'), self.grad('pos_embed'), B, Np, C, dt, label='embedb')
        with self._wlane():
            Bk.wgrad(dtok, self.patches, self.grad('patch_embed.proj.weight'), Mp, C, K0, dt, dbias=self.grad('patch_embed.proj.bias'),
                     label='patch.wg')
