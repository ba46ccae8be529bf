"""EngineBase: what every engine family shares -- the static launch plans (weight prep / forward / backward) of one model for a
fixed (batch, train|eval, math mode) over persistent NHWC device buffers, without any model in it.

Data layout in HBM (bf16 mode; fp32 mode is identical with 4-byte elements):
  * activations: row-major [B*H*W, C] (= NHWC), bf16; per-row LayerNorm rstd fp32; BatchNorm stats fp32 [C];
  * weights: fp32 masters in ONE flat buffer ([decay | no-decay]); per step they are re-laid-out once into the
    "effective" bf16 GEMM operands (k = (ky,kx,ci); LayerNorm scale and LayerScale gamma folded in; a transposed
    copy for the data-gradient product) by ga_weight_prep -- so the hot GEMMs only ever see bias / GELU / residual
    epilogues;
  * gradients: fp32, ONE flat buffer aliased by every param.grad; the wgrad kernels atomically accumulate either
    directly into it or into a zeroed scratch arena of effective-weight gradients that ga_weight_unfold maps back.

A family is `class XEngine(<builders...>, EngineBase)`: the builders (engine.ConvNeXtTrunk / GAHeads, engine_map.MAPHead,
engine_heads.GroupMlp / HeadStacks, engine_blocks.TransformerBlocks, engine_pit.PiTTrunk) are stateless classes of recording methods -- no __init__, attributes created by their own
build methods only -- and the family fills in the hooks `_drop_path_rates`, `_build` and, where it needs more gradient scratch,
`_arena_extra`.  The constructor runs `_build()` and then the tail every plan ends with (`_finish`).

Where a group of gradients is complete the family says so with `_seal(mark, prefixes...)`: the backward plan's mark at which
TrainStep may start reducing them (`grad_groups()`, `backward_to(mark)`); `grad()` refuses a sealed name for the rest of the build.
"""
import contextlib
import os

import torch

from . import ops
from .ops import ASYNC_LANE, GA_BF16, GA_F32, Plan


def pad8(n):
    return (n + 7) // 8 * 8


class GAFunction(torch.autograd.Function):
    """Autograd glue: one node for the whole network. Parameter gradients are accumulated by the HIP kernels
    straight into the flat gradient buffer behind every param.grad (so this node returns no tensor grads)."""

    @staticmethod
    def forward(ctx, eng, x, anchor):
        ctx.eng = eng
        return eng.forward(x)

    @staticmethod
    def backward(ctx, dlogits):
        ctx.eng.backward(dlogits)
        return None, None, None


class EngineBase:
    def __init__(self, model, batch, training, mode):
        self.m = model
        self.cfg = model.cfg
        self.B = batch
        self.training = training
        self.dt = GA_BF16 if mode == 'bf16' else GA_F32
        self.tdt = ops.torch_dtype(self.dt)
        flat = model.flat_state()
        self.dev = flat['params'].device
        self.P = dict(model.named_parameters())
        self.Bf = dict(model.named_buffers())
        self.bufs = {}
        self.tmps = {}
        self.tmp_prefix = ''     # per-head copies of the transients while the heads are recorded on concurrent lanes
        # trunk weight-gradient launches on the backward plan's asynchronous lane (GAEXT_ASYNC_WGRAD=0: in line)
        self.async_wgrad = os.environ.get('GAEXT_ASYNC_WGRAD', '1') != '0'
        self.fwd_split = max(1, int(os.environ.get('GAEXT_FWD_SPLIT', '2')))
        self.fuse_dp = os.environ.get('GAEXT_FUSE_DP', '1') != '0'
        self._chain = None       # (lane, first image, end image) while a forward chain is being recorded
        self._bwd_seq = 0        # trunk blocks recorded on the backward plan so far
        self._pre_dyz = {}       # block prefix -> DropPath-scaled dy already written by the block before it (backward order)
        self._sealed = {}        # backward-plan mark -> parameter-name prefixes whose gradients are final there, in sealing order
        self._bwd_pos = 0        # how far backward_to() has run the backward plan since the last forward
        self.sync_bn = getattr(model, 'sync_bn_comm', None)      # FlatModel.convert_sync_batchnorm(comm): --sync-bn (GA/train.py:449-455)
        self.W = {}
        self.weights_dirty = True
        self.anchor = torch.zeros((), device=self.dev, requires_grad=True)
        self.blocks = {}
        self.x_ref = None
        self.img = self.cfg.get('img_size', 224)
        # where set_input() writes the image pointer: argument 0 of forward call `input_call`, or field A of the forward
        # descriptor `input_desc`; and field X of the stem weight gradient's descriptor where the backward reads the image
        self.input_call = self.input_desc = self.input_bwd_desc = None
        self.fixed_masks = False     # parity tests: keep the DropPath / dropout masks they have set
        self.loss_cfg = None
        # DropPath schedule (ga_convnext.py:362,376,413)
        self.dp_rates = self._drop_path_rates()
        self.dp_scale = {}   # block prefix -> fp32 [B] (mask / keep): rows of ONE (n_sites, B) tensor
        if training:
            sites = [pre for pre, r in self.dp_rates.items() if r > 0]
            if sites:
                self.dp_all = torch.ones(len(sites), batch, device=self.dev)
                self.dp_keep = torch.tensor([1.0 - self.dp_rates[p] for p in sites], device=self.dev)
                self.dp_counter = torch.zeros(1, dtype=torch.int64, device=self.dev)
                self.dp_plan = Plan(name='droppath')
                self.dp_plan.drop_path_sample(self.dp_all, self.dp_keep, len(sites), batch, torch.initial_seed(), self.dp_counter)
                for i, pre in enumerate(sites):
                    self.dp_scale[pre] = self.dp_all[i]
        # scratch arena for effective-weight gradients (zeroed once per backward)
        self.arena = None
        self.arena_off = 0
        if training:
            self.arena = torch.zeros(int(flat['total'] * 1.15) + (1 << 20) + self._arena_extra(), device=self.dev)
        self.prep = Plan(name='prep', defer_small=True)
        self.fwd = Plan(name='fwd')
        self.bwd = Plan(name='bwd', defer_small=True) if training else None
        # BatchNorm column-sum accumulators live in one pool that the forward plan zeroes with a single memset
        self.bn_pool = torch.zeros(1 << 16, device=self.dev)
        self.bn_pool_off = 0
        self._build()
        self._finish()

    # ------------------------------------------------------------------------------------------
    # hooks of a family
    # ------------------------------------------------------------------------------------------
    def _drop_path_rates(self):
        """{DropPath site: rate}; a site is a block prefix, or prefix + '#1' / '#2' where a block has two"""
        raise NotImplementedError

    def _build(self):
        """record the prep / fwd / bwd plans"""
        raise NotImplementedError

    def _arena_extra(self):
        """floats of gradient scratch beyond 1.15 x the parameters"""
        return 0

    def _finish(self):
        """the tail of every build: the backward plan waits for its asynchronous lane, the deferred small jobs are emitted"""
        if self.training:
            if self.async_wgrad:
                self.bwd.join_async()
            self.bwd.flush('end.')
        self.prep.flush('prep.')

    # ------------------------------------------------------------------------------------------
    # buffers
    # ------------------------------------------------------------------------------------------
    def buf(self, name, shape, dtype=None, zero=False):
        dtype = dtype or self.tdt
        if name not in self.bufs:
            self.bufs[name] = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.dev)
        t = self.bufs[name]
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, name
        return t

    def _chains(self):
        """(lane, first image, end image) of the forward trunk's independent batch parts: with GAEXT_FWD_SPLIT=n > 1
        the trunk runs as n chains on side streams (rows of different images never mix before the first BatchNorm),
        so that one chain's launches fill the tails of the other's"""
        n = self.fwd_split if self.B >= 2 * self.fwd_split else 1
        if n <= 1:
            return [(0, 0, self.B)]
        per = self.B // n
        cuts = [s_ * per for s_ in range(n)] + [self.B]
        return [(1 + s_, cuts[s_], cuts[s_ + 1]) for s_ in range(n)]

    def _fsplits(self, HW):
        """(lane, first row, end row, first image, end image) the current pass of the trunk records"""
        ch = self._chain
        if ch is None:
            return [(0, 0, self.B * HW, 0, self.B)]
        lane, b0, b1 = ch
        return [(lane, b0 * HW, b1 * HW, b0, b1)]

    @contextlib.contextmanager
    def _wlane(self):
        """weight-gradient launches recorded inside go to the backward plan's asynchronous lane (trunk / shared parts
        only: inside a head's lane they stay in that lane)"""
        Bk = self.bwd
        prev = Bk.lane
        if self.async_wgrad and prev == 0:
            Bk.lane = ASYNC_LANE
        try:
            yield
        finally:
            Bk.lane = prev

    def _wgrad_window(self):
        """opens a trunk block's backward: True where its weight-gradient launches go to the asynchronous lane (not inside a head's
        lane).  The block is number `_bwd_seq` then; the launches read two alternating sets of transients (by the number's parity), so
        the block waits for the asynchronous launches of block t-2 only"""
        side = self.async_wgrad and self.bwd.lane == 0
        if side:
            self._bwd_seq += 1
            self.bwd.join_async(f'blk{self._bwd_seq - 2}')
        return side

    def _wgrad_window_mark(self, side):
        """after the block's last asynchronous launch: what block t+2 (and whoever rewrites a transient earlier) joins"""
        if side:
            self.bwd.async_mark(f'blk{self._bwd_seq}')

    def tmp(self, tag, shape, dtype=None):
        """transient buffer shared by every call site with the same (tag, shape, dtype) -- stream order makes it safe"""
        dtype = dtype or self.tdt
        key = (self.tmp_prefix + tag, tuple(shape), dtype)
        if key not in self.tmps:
            self.tmps[key] = torch.empty(shape, dtype=dtype, device=self.dev)
        return self.tmps[key]

    def act(self, name, shape, dtype=None):
        """activation saved for backward (uniquely named, persistent)"""
        return self.buf(name, shape, dtype)

    def blk_act(self, name, shape, dtype=None):
        """per-block saved activation: persistent when training, one shared transient per shape in eval"""
        return self.buf(name, shape, dtype) if self.training else self.tmp(name.rsplit('.', 1)[-1], shape, dtype)

    def gbuf(self, shape):
        n = 1
        for s in shape:
            n *= s
        off = (self.arena_off + 63) // 64 * 64
        assert off + n <= self.arena.numel(), 'gradient scratch arena too small'
        self.arena_off = off + n
        return self.arena[off:off + n].view(shape)

    def grad(self, name):
        """gradient buffer of a parameter, for a launch that is recorded NOW: a call recorded after the seal of its group would
        write (or read) the gradient after TrainStep has started reducing it"""
        for mark, prefixes in self._sealed.items():
            if name.startswith(prefixes):
                raise RuntimeError(f'gradient of {name} requested after mark {mark!r} sealed {prefixes}: it is final there')
        return self.P[name].grad

    def _seal(self, mark, *prefixes, flush, then=None):
        """the gradients of the parameters under `prefixes` are final from here on: wait for the asynchronous lane, emit the deferred
        small jobs under label `flush`, record `then()` (what must sit between flush and mark) and set `mark`.  flush=None: the
        segment defers nothing and has nothing on the asynchronous lane beyond what Plan.run_range joins at the end of every range,
        so neither join nor flush is recorded.  No prefixes: a mark nothing is claimed at"""
        Bk = self.bwd
        if flush is not None:
            if self.async_wgrad:
                Bk.join_async()
            Bk.flush(flush)
        if then is not None:
            then()
        Bk.mark(mark)
        if prefixes:
            self._sealed[mark] = prefixes

    def grad_groups(self):
        """[(backward-plan mark, parameter-name prefixes whose gradients are final at that mark)] in backward-completion order;
        parameters under no prefix are final at the end of backward.  trainer.make_buckets cuts the flat gradient buffer by it
        into all-reduce buckets that start while the rest of backward still runs.  An eval engine seals nothing: []"""
        return list(self._sealed.items())

    def sample_drop_path(self):
        """fresh per-sample Bernoulli(keep)/keep factors for every stochastic-depth site (timm DropPath): one launch of
        ga_drop_path_sample, keyed by torch.initial_seed() at build time and a device-side call counter"""
        if self.dp_scale:
            self.dp_plan.run()

    def set_drop_path_masks(self, masks):
        for pre, t in self.dp_scale.items():
            t.copy_(masks[pre].to(self.dev).float())

    @staticmethod
    def _last_desc(plan):
        # the ctypes descriptor of the most recently recorded gemm/wgrad call
        for obj in reversed(plan.keep):
            if hasattr(obj, '_fields_'):
                return obj
        raise RuntimeError('no descriptor')

    # ------------------------------------------------------------------------------------------
    # effective weights (recorded into self.prep)
    # ------------------------------------------------------------------------------------------
    def _w_plain(self, name, Co, Ci, KH, KW, stem=False, need_T=True, flip=False, groups=1, rs=None, cs=None,
                 row_perm=None, ldo=None, key=None, src=None):
        """effective copy (and transposed copy when training) of a conv/linear weight; returns the forward copy"""
        key = key or name
        if key in self.W:
            return self.W[key]
        KK = Ci * KH * KW
        ldo = ldo or pad8(KK)
        out = self.buf('w.' + key, (groups * Co, ldo))
        outT = None
        ldt = 0
        if need_T and self.training:
            if flip:
                ldt = pad8(KH * KW * Co)
                outT = self.buf('wT.' + key, (groups * Ci, ldt))
            else:
                ldt = pad8(Co)
                outT = self.buf('wT.' + key, (groups * KK, ldt))
            self.W[key + '.T'] = outT
        self.prep.weight_prep(self.P[name] if src is None else src, groups, Co, Ci, KH, KW, self.dt, out=out, ldo=ldo, outT=outT, ldt=ldt, rs=rs,
                              cs=cs, flip=flip, stem=stem, row_perm=row_perm, label='prep.' + key)
        self.W[key] = out
        return out

    # ------------------------------------------------------------------------------------------
    # BatchNorm helper (stats come from the producing GEMM's colsum epilogue)
    # ------------------------------------------------------------------------------------------
    def _bn_pool(self, C):
        off = (self.bn_pool_off + 63) // 64 * 64
        assert off + C <= self.bn_pool.numel()
        self.bn_pool_off = off + C
        return self.bn_pool[off:off + C]

    def _bn_bufs(self, pre, C, zero=False):
        return dict(s=self._bn_pool(C), q=self._bn_pool(C),
                    mean=self.buf(pre + 'bmean', (C,), torch.float32, zero=zero), rstd=self.buf(pre + 'brstd', (C,), torch.float32, zero=zero),
                    scale=self.buf(pre + 'scale', (C,), torch.float32, zero=zero), shift=self.buf(pre + 'shift', (C,), torch.float32, zero=zero))

    def _sync_allreduce(self, plan, t, label):
        """SyncBatchNorm (GA/train.py:449-455, --sync-bn): sum a small fp32 statistics vector over the ranks, enqueued on the lane the
        plan call runs on (ga_allreduce_bucket through the communicator convert_sync_batchnorm() attached to the model)"""
        c = self.sync_bn
        plan.record('ga_allreduce_bucket', c.handle, t, t.numel(), GA_F32, 1.0, None, 0, label=label)
        plan.keep.append(c)       # the handle is a host value: the communicator behind it must outlive the plan

    def _bn_finalize(self, pre, bn, n, C):
        if self.sync_bn is not None and self.training:       # batch statistics over the GLOBAL batch: sums of all ranks, n x world
            self._sync_allreduce(self.fwd, bn['s'], pre + 'sync.s')
            self._sync_allreduce(self.fwd, bn['q'], pre + 'sync.q')
            n = n * self.sync_bn.world
        self.fwd.bn_finalize(bn['s'], bn['q'], n, self.P[pre + 'weight'], self.P[pre + 'bias'], 1e-5, 0.1,
                             self.Bf[pre + 'running_mean'], self.Bf[pre + 'running_var'], bn['mean'], bn['rstd'],
                             bn['scale'], bn['shift'], C, self.training, label=pre + 'fin')

    def _bn_bwd(self, pre, bn, dy, y_relu, x, dx, rows, C, rowscale=None, rps=1, ldx=0, lddx=0, weight=None, c_real=None):
        """weight / c_real: the zero-padded copy of the BatchNorm weight and the real channel count of a padded branch"""
        Bk = self.bwd
        s1, s2 = self.gbuf((C,)), self.gbuf((C,))
        Bk.bn_bwd_reduce(dy, y_relu, x, bn['mean'], bn['rstd'], s1, s2, rows, C, self.dt, rowscale=rowscale,
                         rows_per_scale=rps, ldx=ldx, label=pre + 'bnr')
        n = rows
        if self.sync_bn is not None:
            # torch.nn.SyncBatchNorm's backward: the parameter gradients take the LOCAL column sums (the gradient all-reduce averages
            # them later), so they are accumulated right here -- not deferred to the stage flush --; then the two sums that enter dx
            # are summed over the ranks in place
            Bk.record('ga_axpy_f32', self.grad(pre + 'weight'), s2, 1.0, c_real or C, label=pre + 'dgamma')
            Bk.record('ga_axpy_f32', self.grad(pre + 'bias'), s1, 1.0, c_real or C, label=pre + 'dbeta')
            self._sync_allreduce(Bk, s1, pre + 'sync.s1')
            self._sync_allreduce(Bk, s2, pre + 'sync.s2')
            n = rows * self.sync_bn.world
        Bk.bn_bwd_apply(dy, y_relu, x, bn['mean'], bn['rstd'], self.P[pre + 'weight'] if weight is None else weight, s1, s2, n, dx,
                        rows, C, self.dt, rowscale=rowscale, rows_per_scale=rps, ldx=ldx, lddx=lddx, label=pre + 'bna')
        if self.sync_bn is None:
            Bk.axpy_f32(self.grad(pre + 'weight'), s2, 1.0, c_real or C)
            Bk.axpy_f32(self.grad(pre + 'bias'), s1, 1.0, c_real or C)

    # ------------------------------------------------------------------------------------------
    # pieces several families record alike
    # ------------------------------------------------------------------------------------------
    def _image_pack8_stem(self, wname, Co):
        """the image as NHWC with 8 channels (ga_nchw3_to_nhwc8, the input slot of set_input) for a 3 x 3 / stride-2 stem conv read
        through the GA_A_CONV3S2 gather; returns that conv's weight `wname` packed to the [Co][72] operand (k = 9 taps x 8 channels)"""
        B, img, F, dt = self.B, self.img, self.fwd, self.dt
        self.x8 = self.buf('stem.x8', (B * img * img, 8))
        self.x_placeholder = torch.zeros(8, device=self.dev)      # patched by set_input
        self.input_call = len(F.calls)
        F.nchw3_to_nhwc8(self.x_placeholder, self.x8, B, img, img, dt, label='stem.pack')
        W0 = self.buf('w.' + wname, (Co, 72))
        self.prep.convw_pack(self.P[wname + '.weight'], W0, Co, 3, 9, 8, 72, dt, label='prep.' + wname)
        return W0

    def _linear_head_fwd(self, x, wname, C, label):
        """the plain classifier: logits [1][B][NC] (fp32) = x [B, C] . W^T + b, the Linear's parameters under prefix `wname`"""
        NC = self.cfg['num_classes']
        assert NC % 8 == 0, 'num_classes must be a multiple of 8 (pad the classifier)'
        Wh = self._w_plain(wname + 'weight', NC, C, 1, 1)
        self.logits = self.buf('logits', (1, self.B, NC), torch.float32)
        self.fwd.gemm(x, Wh, self.logits[0], self.B, NC, C, self.dt, bias=self.P[wname + 'bias'], c_f32=True, label=label)

    def _linear_head_bwd(self, x, wname, C, dx_tag):
        """backward of _linear_head_fwd: the weight gradient on the asynchronous lane; returns the gradient wrt x (transient `dx_tag`)"""
        Bk, B, dt, NC = self.bwd, self.B, self.dt, self.cfg['num_classes']
        self.dlogits = self.buf('dlogits', (1, B, NC))
        dl = self.dlogits[0]
        with self._wlane():
            Bk.wgrad(dl, x, self.grad(wname + 'weight'), B, NC, C, dt, dbias=self.grad(wname + 'bias'), label=wname + 'wg')
        dx = self.tmp(dx_tag, (B, C))
        Bk.gemm(dl, self.W[wname + 'weight.T'], dx, B, C, NC, dt, ldb=pad8(NC), label=wname + 'dg')
        return dx

    # ------------------------------------------------------------------------------------------
    # run
    # ------------------------------------------------------------------------------------------
    # ImageNet statistics x 255, as timm's PrefetchLoader holds them for the uint8 batches of fast_collate (GA/train.py:567-595)
    U8_MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
    U8_STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)

    def input_stats(self):
        """(mean, std) of the uint8 normalisation, 0..255 units: the model's input_mean / input_std or the ImageNet ones"""
        return getattr(self.m, 'input_mean', None) or self.U8_MEAN, getattr(self.m, 'input_std', None) or self.U8_STD

    def normalize_u8(self, x):
        """a uint8 (B, 3, H, W) batch is normalised on the device into an engine-owned fp32 buffer (no host round trip)"""
        if x.dtype != torch.uint8:
            return x
        assert x.is_cuda and tuple(x.shape) == (self.B, 3, self.img, self.img), f'uint8 input of shape {tuple(x.shape)}'
        out = self.buf('x.u8norm', (self.B, 3, self.img, self.img), torch.float32)
        mean, std = self.input_stats()
        Plan(eager=True).u8_normalize(x.contiguous(), out, mean, std)
        return out

    def set_input(self, x):
        x = self.normalize_u8(x)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (self.B, 3, self.img, self.img), \
            f'input must be a float32 CUDA tensor of shape {(self.B, 3, self.img, self.img)}, got {tuple(x.shape)} {x.dtype}'
        if not x.is_contiguous():
            x = x.contiguous()   # channels_last callers (GA/train.py:729-730): the stem gather reads NCHW
        self.x_ref = x
        ptr = x.data_ptr()
        if self.input_call is not None:
            fn, args, label = self.fwd.calls[self.input_call]
            self.fwd.calls[self.input_call] = (fn, (ptr,) + tuple(args[1:]), label)
        else:
            self.input_desc.A = ptr
        if self.input_bwd_desc is not None:
            self.input_bwd_desc.X = ptr

    def forward(self, x):
        self.set_input(x)
        if self.training or self.weights_dirty:
            self.prep.run()
            self.weights_dirty = False
            if self.training:
                for e in self.m._engines.values():
                    if e is not self:
                        e.weights_dirty = True
        if self.training and self.dp_scale and not self.fixed_masks:
            self.sample_drop_path()
        self._bwd_pos = 0
        self.fwd.run()
        if self.training:
            self.m.count_training_forward()     # num_batches_tracked: host-side count, written on state_dict()
        return self.logits.view_as(self.logits)

    def _loss_operands(self):
        """(per-head logits, extra logits, d logits, d extra, heads) of the fused loss: every row of `logits` is a head"""
        return self.logits, None, self.dlogits, None, self.logits.shape[0]

    def build_loss(self, lam, kind=0, smoothing=0.0, grad_scale=1.0, dense=False, bce_threshold=-1.0, num_splits=0, jsd_alpha=12.0):
        """fused loss writing d(loss)/d(logits) * grad_scale straight into the backward plan's input buffer; dense: the target
        is a (B, NC) fp32 tensor (mixup / cutmix) instead of class indices.  kind 2: timm's JsdCrossEntropy(num_splits, jsd_alpha,
        smoothing) per head on a split-major batch of num_splits augmentation splits (ga_loss_jsd_fwd_bwd; the kernel reads the
        first B / num_splits labels of the target buffer)"""
        org, avg, dorg, davg, K = self._loss_operands()
        _, B, NC = self.logits.shape
        if kind == 2 and (dense or num_splits < 2 or B % num_splits):
            raise ValueError(f'the JSD loss runs on class indices and on a batch of num_splits >= 2 augmentation splits: batch {B}, '
                             f'num_splits {num_splits}, {"dense" if dense else "class-index"} target')
        self.loss_buf = self.buf('loss', (1,), torch.float32)
        self.target_buf = self.buf('target.dense', (B, NC), torch.float32) if dense else self.buf('target', (B,), torch.int64)
        lp = Plan(name='loss')
        lp.zero(self.loss_buf)
        if kind == 2:
            lp.loss_jsd_fwd_bwd(org, avg, self.target_buf, self.loss_buf, dorg, davg, K, B, NC, int(num_splits), float(lam),
                                float(smoothing), float(jsd_alpha), float(grad_scale), self.dt)
        else:
            lp.loss_dense_fwd_bwd(org, avg, None if dense else self.target_buf, self.target_buf if dense else None, self.loss_buf, dorg,
                                  davg, K, B, NC, float(lam), int(kind), float(smoothing), float(bce_threshold), float(grad_scale), self.dt)
        self.loss_plan = lp
        self.loss_cfg = (lam, kind, smoothing, grad_scale, dense, bce_threshold, num_splits, jsd_alpha)

    def forward_loss(self, x, target, lam, kind=0, smoothing=0.0, grad_scale=1.0, bce_threshold=-1.0, num_splits=0, jsd_alpha=12.0):
        """forward + loss (+ dlogits) without autograd; follow with backward_to(mark) ... backward_to('end'), or bwd.run().
        Returns the loss buffer.
        target: class indices (B,) or a dense (B, NC) floating-point target; kind 2 (JSD over num_splits augmentation splits): the
        class indices of all B rows, split-major, as AugSplits repeats them"""
        dense = target.dim() == 2
        if self.loss_cfg != (lam, kind, smoothing, grad_scale, dense, bce_threshold, num_splits, jsd_alpha):
            self.build_loss(lam, kind, smoothing, grad_scale, dense, bce_threshold, num_splits, jsd_alpha)
        self.forward(x)              # (resets backward_to's position)
        self.target_buf.copy_(target, non_blocking=True)
        self.loss_plan.run()
        return self.loss_buf

    def backward(self, dlogits):
        if dlogits.data_ptr() != self.dlogits.data_ptr():
            if dlogits.dtype == self.tdt:
                self.dlogits.copy_(dlogits)
            else:
                p = Plan(eager=True)
                p.cast_from_f32(dlogits.contiguous().float(), self.dlogits, self.dlogits.numel(), self.dt)
        self.bwd.run()

    def backward_to(self, mark):
        """run the backward plan from where the previous call stopped (the start, after a forward) up to `mark`; 'end': the end of
        the plan.  Nothing runs when the position is already there or past it"""
        bwd = self.bwd
        stop = len(bwd.calls) if mark == 'end' else bwd.marks[mark]
        if stop > self._bwd_pos:
            bwd.run_range(self._bwd_pos, stop)
            self._bwd_pos = stop
