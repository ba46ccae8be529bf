"""Launch plans over the libgaext C ABI.

A `Plan` is a pre-resolved list of C-ABI calls (ctypes function + fully built argument tuple) over persistent
device buffers.  The engine builds the forward / backward / optimizer plans ONCE per (batch size, mode) and then
replays them on a HIP stream every step: no per-step descriptor construction, no allocation, no host sync --
the MI355X-native replacement for the reference's eager ATen dispatch (and directly capturable in a hipGraph).
Every method records one call; `run()` enqueues them all.  `Plan(eager=True)` also executes each call as it is
recorded (used by the unit tests).
"""
import ctypes as C
import numbers
import os

import torch

from . import _lib as L
from ._lib import (A_CONV3, A_CONV3S2, A_NEIGH2, A_PATCH2, A_PLAIN, A_STEM4_NCHW, ACT_GELU, ACT_NONE, ACT_RELU, C_PLAIN, C_UNPATCH2,  # noqa: F401
                   GA_BF16, GA_F32)


def ga_dtype(t):
    if isinstance(t, torch.dtype):
        dt = t
    else:
        dt = t.dtype
    if dt == torch.bfloat16:
        return GA_BF16
    if dt == torch.float32:
        return GA_F32
    raise TypeError(f'unsupported dtype {dt}')


def torch_dtype(ga):
    return torch.bfloat16 if ga == GA_BF16 else torch.float32


def _ptr(t):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'libgaext operand must be a torch.Tensor or None, got {type(t).__name__}: {t!r}')
    assert t.is_cuda, 'libgaext operands must live in device memory (no CPU fallback)'
    return t.data_ptr()


def _set(d, **fields):
    """fill a descriptor from keyword fields.  Which fields are pointers (c_void_p, or an array of them) comes from `_fields_`:
    those take tensors, and the tensors are attached to the descriptor instance, so that whoever keeps `d` keeps its operands"""
    types = dict(d._fields_)
    held = d.__dict__.setdefault('operands', [])
    for name, v in fields.items():
        typ = types[name]
        if typ is C.c_void_p:
            held.append(v)
            v = _ptr(v)
        elif issubclass(typ, C.Array) and typ._type_ is C.c_void_p:
            held.extend(v)
            v = typ(*[_ptr(t) for t in v])
        setattr(d, name, v)
    return d


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _host_rows(vals, n):
    """per-channel host floats (mean / std) as the C array the entry point reads while it enqueues"""
    return (C.c_float * n)(*[float(v) for v in vals])


def _u64(v):
    """a seed / offset as the 64-bit unsigned value the entry point takes"""
    return int(v) & ((1 << 64) - 1)


def current_stream_ptr():
    return torch.cuda.current_stream().cuda_stream


_SIDE_POOL = {}    # device index -> (side streams, their "done" events, fork event): shared by every plan of the process


def _side_pool(n):
    dev = torch.cuda.current_device()
    streams, done, fork = _SIDE_POOL.get(dev, ([], [], None))
    while len(streams) < n:
        streams.append(torch.cuda.Stream())
        done.append(torch.cuda.Event())
    fork = fork or torch.cuda.Event()
    _SIDE_POOL[dev] = (streams, done, fork)
    return streams, done, fork


_ASYNC_POOL = {}   # device index -> (stream, done event, fork event) of the asynchronous lane


def _async_pool():
    dev = torch.cuda.current_device()
    if dev not in _ASYNC_POOL:
        _ASYNC_POOL[dev] = (torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event())
    return _ASYNC_POOL[dev]


def _join_marker(*_):
    """pseudo call recorded by Plan.join_async(); a no-op wherever a plan's calls are replayed one by one"""
    return 0


def _amark_marker(*_):
    """pseudo call recorded by Plan.async_mark(): a named point of the asynchronous lane that join_async(tag) waits for"""
    return 0


def _lsig_marker(*_):
    """pseudo call of Plan.lane_signal(): an event recorded on a side lane's stream"""
    return 0


def _lwait_marker(*_):
    """pseudo call of Plan.lane_wait(): a side lane waits for an event of another lane"""
    return 0


ASYNC_LANE = -1


class Plan:
    def __init__(self, eager=False, name='', defer_small=False):
        self.lib = L.load()
        self.calls = []      # (cfunc, args tuple, label)
        self.keep = []       # tensors / descriptors kept alive
        self.eager = eager
        self.name = name
        self.marks = {}
        # defer_small: weight-prep / un-fold / bias-fold / transpose / axpy jobs are collected and emitted by flush()
        # as ONE batched launch per kind over a device-resident descriptor array
        self.defer = defer_small and not eager
        self._pend = {'wprep': [], 'small': [], 'unfold': []}
        # lanes: calls recorded while lane > 0 form a PARALLEL REGION -- independent chains (the five GA heads) that
        # run() puts on side streams between a fork (side streams wait for the main stream) and a join (the main stream
        # waits for them).  Lane 0 is the stream run() is called on.
        # Lane -1 (ASYNC_LANE) is different: such a call runs on ONE extra stream after everything recorded before it on
        # lane 0, and lane 0 does not wait for it until join_async() (or the end of the range being run).  The trunk's
        # weight-gradient launches go there: nothing on the dgrad chain reads their results.
        # workspaces: ga_wgrad / ga_dwconv7_bwd_weight reduce per-workgroup partial results through CALLER-owned scratch
        # (include/gaext.h): one torch buffer per lane (launches of one lane are stream-ordered and may share it; lanes run
        # concurrently), sized to the largest request of that lane and allocated before the first run
        self._ws_req = []    # (lane, bytes, patch callable(ptr, bytes))
        self._ws = {}        # lane -> uint8 tensor
        self._ws_dirty = False
        self.lane = 0
        self.lanes = []      # lane of every call
        self._side = None    # number of side lanes (streams come from a process-wide pool)
        self._aevents = {}   # async_mark tag -> event

    def flush(self, label=''):
        for kind, fname, cls in (('wprep', 'ga_weight_prep_batch', L.WprepDesc), ('small', 'ga_small_batch', L.SmallDesc),
                                 ('unfold', 'ga_weight_unfold_batch', L.WunfoldDesc)):
            lst = self._pend[kind]
            if not lst:
                continue
            arr = (cls * len(lst))(*lst)
            dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
            self.record(fname, dev, len(lst), label=f'{label}{kind}.batch[{len(lst)}]')
            self.keep.append(arr)                     # the host copy, right after its device copy
            self._pend[kind] = []

    def _defer(self, kind, d):
        """a job for flush(): the batch holds a copy of `d`, so its operands are kept here"""
        self._pend[kind].append(d)
        self.keep.extend(d.operands)

    def _small(self, **kw):
        d = _set(L.SmallDesc(), **kw)
        self._defer('small', d)
        if os.environ.get('GAEXT_SMALL_SINGLE'):      # diagnosis: one launch per small job, labelled with its geometry
            self.flush(f'single.k{d.kind}.R{d.R}.C{d.C}.n{d.n}.')

    # -- core ---------------------------------------------------------------------------------------
    def _resolve(self, v):
        """one operand -> the value the entry point is called with at every replay; what that value points to is kept alive"""
        if v is None:
            return None
        if isinstance(v, bool):
            return int(v)
        if isinstance(v, (numbers.Number, C._SimpleCData)):      # sizes, scalars, flags; a host handle
            return v
        self.keep.append(v)
        if isinstance(v, C.Structure):                           # a descriptor: _set() attached its operands to it
            return C.byref(v)
        if isinstance(v, C.Array):                               # host rows, read while the call is enqueued
            return v
        return _ptr(v)

    def record(self, fname, *operands, label=None):
        """record one call of entry point `fname`.  `operands` are the arguments themselves -- tensors, descriptors, host arrays,
        None, numbers -- and are resolved ONCE, here: replay passes the resolved tuple as it is.  Operand lifetime is this
        function's job: no caller lists what it passes a second time"""
        fn = getattr(self.lib, fname)
        args = tuple(self._resolve(v) for v in operands)
        self.calls.append((fn, args, label or fname))
        self.lanes.append(self.lane)
        if self.eager:
            L.check(fn(*args, current_stream_ptr()), label or fname)

    def _record_ws(self, fname, need, *operands, label=None):
        """record() a call whose last two arguments are this lane's workspace pointer and its size (`need` bytes wanted): known at
        once when eager, else (None, 0) until finalize() puts the lane's buffer into the recorded tuple"""
        idx, ws = len(self.calls), [None, 0]

        def patch(ptr, nbytes):
            ws[:] = ptr, nbytes
            if idx < len(self.calls):
                fn, args, lb = self.calls[idx]
                self.calls[idx] = (fn, args[:-2] + (ptr, nbytes), lb)
        self._want_workspace(need, patch)
        self.record(fname, *operands, *ws, label=label)

    def _want_workspace(self, nbytes, patch):
        if self.eager:
            t = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
            self.keep.append(t)
            patch(t.data_ptr(), nbytes)
            return
        self._ws_req.append((self.lane, nbytes, patch))
        self._ws_dirty = True

    def finalize(self):
        """allocate / grow the per-lane workspaces and hand their addresses to the recorded calls"""
        if not self._ws_dirty:
            return
        need = {}
        for lane, nbytes, _ in self._ws_req:
            need[lane] = max(need.get(lane, 0), nbytes)
        for lane, nbytes in need.items():
            if lane not in self._ws or self._ws[lane].numel() < nbytes:
                self._ws[lane] = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        for lane, nbytes, patch in self._ws_req:
            patch(self._ws[lane].data_ptr(), self._ws[lane].numel())
        self._ws_dirty = False

    def run(self, stream=None):
        if os.environ.get('GAEXT_SYNC_DEBUG'):   # localise a faulting launch: label printed before, sync after
            self.finalize()
            s = current_stream_ptr() if stream is None else stream
            for fn, args, label in self.calls:
                print(f'[gaext] {self.name}:{label}', flush=True)
                L.check(fn(*args, s), f'{self.name}:{label}')
                torch.cuda.synchronize()
            return
        return self.run_range(0, len(self.calls), stream)

    def join_async(self, tag=None):
        """lane 0 waits here for everything recorded on the asynchronous lane so far (tag: up to async_mark(tag) only)"""
        self.calls.append((_join_marker, () if tag is None else (tag,), 'join_async'))
        self.lanes.append(0)

    def lane_signal(self, lane):
        """a point of side lane `lane` (inside a parallel region) that lane_wait() of another lane can wait for"""
        ev = torch.cuda.Event()
        self.calls.append((_lsig_marker, (lane, ev), 'lane_signal'))
        self.lanes.append(lane)
        return ev

    def lane_wait(self, lane, ev):
        self.calls.append((_lwait_marker, (lane, ev), 'lane_wait'))
        self.lanes.append(lane)

    def async_mark(self, tag):
        self.calls.append((_amark_marker, (tag,), 'async_mark'))
        self.lanes.append(0)

    def _run_lanes(self, start, end):
        """calls[start:end] with the parallel regions on side streams (the current torch stream is lane 0)"""
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = max(max(self.lanes), 0)
        streams, done, fork = _side_pool(self._side)
        astream, adone, afork = _async_pool()
        apend = False
        aev = {}                                  # named points recorded in THIS run (a range may start after a mark)
        lsig = set()
        s0 = main.cuda_stream
        used = []

        def ajoin():
            adone.record(astream)
            main.wait_event(adone)

        for i in range(start, end):
            fn, args, label = self.calls[i]
            lane = self.lanes[i]
            if fn is _join_marker:
                if args:                          # up to a named point of the asynchronous lane (recorded in this run)
                    ev = aev.get(args[0])
                    if ev is not None:
                        main.wait_event(ev)
                elif apend:
                    ajoin()
                    apend = False
                continue
            if fn is _amark_marker:
                if apend:
                    ev = self._aevents.get(args[0])
                    if ev is None:
                        ev = self._aevents[args[0]] = torch.cuda.Event()
                    ev.record(astream)
                    aev[args[0]] = ev
                continue
            if fn is _lsig_marker:
                if args[0] in used:
                    args[1].record(streams[args[0] - 1])
                    lsig.add(args[1])
                continue
            if fn is _lwait_marker:
                if args[1] in lsig:               # recorded in this run
                    if not used:
                        fork.record(main)
                    if args[0] not in used:
                        streams[args[0] - 1].wait_event(fork)
                        used.append(args[0])
                    streams[args[0] - 1].wait_event(args[1])
                continue
            if lane == ASYNC_LANE:
                if used:                          # the asynchronous lane starts from lane 0's point: close the region first
                    for ln in used:
                        done[ln - 1].record(streams[ln - 1])
                        main.wait_event(done[ln - 1])
                    used = []
                afork.record(main)
                astream.wait_event(afork)
                apend = True
                rc = fn(*args, astream.cuda_stream)
            elif lane == 0:
                if used:                          # join: everything after this point sees the side streams' work
                    for ln in used:
                        done[ln - 1].record(streams[ln - 1])
                        main.wait_event(done[ln - 1])
                    used = []
                rc = fn(*args, s0)
            else:
                if not used:                      # fork: the side streams start from the main stream's current point
                    if apend:
                        ajoin()
                        apend = False
                    fork.record(main)
                if lane not in used:
                    streams[lane - 1].wait_event(fork)
                    used.append(lane)
                rc = fn(*args, streams[lane - 1].cuda_stream)
            if rc != 0:
                L.check(rc, f'{self.name}:{label}')
        for ln in used:                           # a region that runs to the end of the range
            done[ln - 1].record(streams[ln - 1])
            main.wait_event(done[ln - 1])
        if apend:
            ajoin()

    def __len__(self):
        return len(self.calls)

    def mark(self, name):
        """remember the current position (used to run a plan in segments, e.g. to start a gradient all-reduce early)"""
        self.marks[name] = len(self.calls)

    def run_range(self, start, end, stream=None):
        self.finalize()
        s = current_stream_ptr() if stream is None else stream
        if any(self.lanes[start:end]):
            return self._run_lanes(start, end)
        for fn, args, label in self.calls[start:end]:
            rc = fn(*args, s)
            if rc != 0:
                L.check(rc, f'{self.name}:{label}')

    # -- GEMM family --------------------------------------------------------------------------------
    def gemm(self, A, B, Cout, M, N, K, dtype, lda=None, ldb=None, ldc=None, batch=1, strideA=0, strideB=0, strideC=0,
             a_batch_mod=0, a_kind=A_PLAIN, a_dims=(0, 0, 0), a_act=ACT_NONE, c_kind=C_PLAIN, c_dims=(0, 0, 0),
             c_f32=False, alpha=1.0, bias=None, strideBias=0, act=ACT_NONE, H=None, ldh=0, strideH=0, rowscale=None,
             rows_per_scale=1, R=None, ldr=0, strideR=0, relu_after=False, colsum=None, colsumsq=None, strideCol=0,
             C2=None, c2_mode=0, h_is_deriv=False, label=None):
        d = _set(L.GemmDesc(), M=M, N=N, K=K, batch=batch, dtype=dtype,
                 A=A, lda=(K if lda is None else lda), strideA=strideA, a_batch_mod=a_batch_mod, a_kind=a_kind, a_act=a_act,
                 B=B, ldb=(K if ldb is None else ldb), strideB=strideB,
                 C=Cout, ldc=(N if ldc is None else ldc), strideC=strideC, c_kind=c_kind, c_f32=c_f32, C2=C2, c2_mode=c2_mode,
                 h_is_deriv=h_is_deriv, alpha=alpha, bias=bias, strideBias=strideBias, act=act, H=H, ldh=ldh, strideH=strideH,
                 rowscale=rowscale, rows_per_scale=rows_per_scale, R=R, ldr=ldr, strideR=strideR, relu_after=relu_after,
                 colsum=colsum, colsumsq=colsumsq, strideCol=strideCol)
        d.a_H, d.a_W, d.a_C = a_dims
        d.c_H, d.c_W, d.c_C = c_dims
        # the heads' few-row products have kernel forms of their own behind their own entry point (gemm_fewrows.hip); asked once, here
        self.record('ga_gemm' if gemm_fewrows_form(d) == 'none' else 'ga_gemm_fewrows', d, label=label or 'ga_gemm')

    # -- global attention (ViT blocks) ---------------------------------------------------------------
    def attn_desc(self, qkv, out, lse, B, N, H, hd, scale, dtype, ldq=None, ldo=None):
        return _set(L.AttnDesc(), B=B, N=N, H=H, hd=hd, scale=scale, dtype=dtype, qkv=qkv, ldq=(3 * H * hd if ldq is None else ldq),
                    out=out, ldo=(H * hd if ldo is None else ldo), lse=lse)

    def attn_fwd(self, d, label=None):
        self.record('ga_attn_fwd', d, label=label)

    def attn_bwd(self, d, dout, dqkv, ws, label=None):
        """ws: fp32 tensor of B*H*N elements (delta)"""
        self.record('ga_attn_bwd', d, dout, dqkv, ws, _nbytes(ws), label=label)

    def patchify(self, x, out, P, dtype, label=None):
        B, CH, H, W = x.shape
        self.record('ga_patchify', x, out, B, CH, H, W, P, dtype, label=label)

    def patchify_strided(self, x, out, P, S, dtype, label=None):
        B, CH, H, W = x.shape
        self.record('ga_patchify_strided', x, out, B, CH, H, W, P, S, dtype, label=label)

    # -- pooling transformer (PiT) pieces ----------------------------------------------------------
    def pos_add_fwd(self, tok, pos, x0, B, Np, Cdim, dtype, label=None):
        self.record('ga_pos_add_fwd', tok, pos, x0, B, Np, Cdim, dtype, label=label)

    def pos_add_bwd(self, dx0, dpos, B, Np, Cdim, dtype, label=None):
        self.record('ga_pos_add_bwd', dx0, dpos, B, Np, Cdim, dtype, label=label)

    def dwpool_fwd(self, x, w, bias, y, B, H, W_, Cin, mult, dtype, label=None):
        self.record('ga_dwpool_fwd', x, w, bias, y, B, H, W_, Cin, mult, dtype, label=label)

    def dwpool_bwd_data(self, dy, w, dx, B, H, W_, Cin, mult, dtype, label=None):
        self.record('ga_dwpool_bwd_data', dy, w, dx, B, H, W_, Cin, mult, dtype, label=label)

    def dwpool_bwd_weight(self, dy, x, dw, db, B, H, W_, Cin, mult, dtype, label=None):
        self.record('ga_dwpool_bwd_weight', dy, x, dw, db, B, H, W_, Cin, mult, dtype, label=label)

    def resize_concat_fwd(self, src, dst, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, dtype, label=None):
        self.record('ga_resize_concat_fwd', src, dst, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, dtype, label=label)

    def resize_concat_bwd(self, dcat, dsrc, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, dtype, label=None):
        self.record('ga_resize_concat_bwd', dcat, dsrc, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, dtype, label=label)

    def rows_bcast(self, src, dst, B, HW, Cdim, scale, dtype, label=None):
        self.record('ga_rows_bcast', src, dst, B, HW, Cdim, scale, dtype, label=label)

    def token_gap_fwd(self, x, y, B, N, Cdim, dtype, label=None):
        self.record('ga_token_gap_fwd', x, y, B, N, Cdim, dtype, label=label)

    def token_gap_bwd(self, dy, dx, B, N, Cdim, dtype, label=None):
        self.record('ga_token_gap_bwd', dy, dx, B, N, Cdim, dtype, label=label)

    def vit_embed_fwd(self, tok, cls, pos, x0, B, Np, Cdim, dtype, label=None):
        self.record('ga_vit_embed_fwd', tok, cls, pos, x0, B, Np, Cdim, dtype, label=label)

    def vit_embed_bwd(self, dx0, dtok, dcls, dpos, B, Np, Cdim, dtype, label=None):
        self.record('ga_vit_embed_bwd', dx0, dtok, dcls, dpos, B, Np, Cdim, dtype, label=label)

    # -- alignment-free forms (odd-width variants) -------------------------------------------------
    def small_linear_desc(self, A, W, Y, rows, groups, Ng, Kg, dtype, lda, a_gstride, ldy, bias=None, a_perm=None, col_scale=None,
                          rowscale=None, rows_per_scale=1, R=None, ldr=0, Yraw=None):
        return _set(L.SmallLinearDesc(), rows=rows, groups=groups, Ng=Ng, Kg=Kg, dtype=dtype, A=A, lda=lda, a_gstride=a_gstride,
                    a_perm=a_perm, W=W, bias=bias, col_scale=col_scale, rowscale=rowscale, rows_per_scale=rows_per_scale, R=R, ldr=ldr,
                    Y=Y, ldy=ldy, Yraw=Yraw)

    def small_linear_fwd(self, d, label=None):
        self.record('ga_small_linear_fwd', d, label=label)

    def small_linear_bwd(self, d, dY, dA=None, accumulate_dA=False, dW=None, dbias=None, dcol_scale=None, label=None):
        self.record('ga_small_linear_bwd', d, dY, dA, accumulate_dA, dW, dbias, dcol_scale, label=label)

    def colstats(self, x, ld, rows, Cdim, s, q, dtype, label=None):
        self.record('ga_colstats', x, ld, rows, Cdim, s, q, dtype, label=label)

    def pad_copy_f32(self, src, dst, rows, cols, lds, ldd, accumulate=False, label=None):
        self.record('ga_pad_copy_f32', src, dst, rows, cols, lds, ldd, accumulate, label=label)

    def stem4_ln_fwd(self, x, W, ldw, bias, gamma, beta, pre, y, mean, rstd, B, H, W_, Cdim, eps, label=None):
        """ConvNeXt stem conv (4 x 4 / 4 from the fp32 NCHW image) + bias + LayerNorm in one bf16 launch"""
        self.record('ga_stem4_ln_fwd', x, W, ldw, bias, gamma, beta, pre, y, mean, rstd, B, H, W_, Cdim, eps, label=label)

    def blockdiag_f32(self, src, dst, R, rg, ng, cg, ld, to_diag=True, accumulate=False, label=None):
        self.record('ga_blockdiag_f32', src, dst, R, rg, ng, cg, ld, to_diag, accumulate, label=label)

    def pad_groups_f32(self, src, dst, R, Cdim, RG, RGp, CG, CGp, unpad=False, accumulate=False, label=None):
        self.record('ga_pad_groups_f32', src, dst, R, Cdim, RG, RGp, CG, CGp, unpad, accumulate, label=label)

    def pad_copy(self, src, dst, rows, cols, lds, ldd, dtype, accumulate=False, label=None):
        self.record('ga_pad_copy', src, dst, rows, cols, lds, ldd, accumulate, dtype, label=label)

    def mlp_fwd(self, X, W1, b1, W2, b2, Y, M, Cdim, dtype, ldw1=None, ldw2=None, R=None, rowscale=None, rows_per_scale=1, label=None):
        """fused fc1 -> GELU -> fc2 (+ DropPath row scale + residual): Y = R + rowscale * (gelu(X W1^T + b1) W2^T + b2)"""
        H = 4 * Cdim
        d = _set(L.MlpDesc(), X=X, ldx=Cdim, W1=W1, ldw1=(Cdim if ldw1 is None else ldw1), b1=b1, W2=W2, ldw2=(H if ldw2 is None else ldw2),
                 b2=b2, R=R, ldr=Cdim, rowscale=rowscale, rows_per_scale=rows_per_scale, Y=Y, ldy=Cdim, M=M, C=Cdim, H=H, dtype=dtype)
        self.record('ga_mlp_fwd', d, label=label)

    def mlp_bwd(self, X, DY, W1, b1, W2T, W1T, A, DH, DX, M, Cdim, dtype, ldw1=None, ldw2t=None, ldw1t=None, label=None,
                dW1=None, db1=None, partials=None, max_blocks=0):
        """fused dgrad2 -> dgrad1 with the hidden pre-activation re-computed: A = gelu(X W1^T + b1), DH = (DY W2) gelu'(.), DX = DH W1.
        A / DH = None: not stored.  dW1 (fp32 [4C, C], with db1 fp32 [4C]): the fc1 weight gradient DH^T X and the column sums of
        DH are accumulated into them inside the kernel (C = 96: mlp_bwd_wgrad_supported); partials: fp32 scratch of
        mlp_bwd_partials(...) bytes, free again once the call's work is done; max_blocks caps the persistent grid (0: automatic)"""
        H = 4 * Cdim
        d = _set(L.MlpBwdDesc(), X=X, ldx=Cdim, DY=DY, lddy=Cdim, W1=W1, ldw1=(Cdim if ldw1 is None else ldw1), b1=b1,
                 W2T=W2T, ldw2t=(Cdim if ldw2t is None else ldw2t), W1T=W1T, ldw1t=(H if ldw1t is None else ldw1t),
                 A=A, lda=H, DH=DH, lddh=H, DX=DX, lddx=Cdim, M=M, C=Cdim, H=H, dtype=dtype)
        if dW1 is not None:
            assert dW1.dtype == torch.float32 and db1 is not None and db1.dtype == torch.float32 and partials is not None
            assert dW1.stride(-1) == 1 and partials.dtype == torch.float32 and partials.is_contiguous()
            _set(d, dW1=dW1, ldw=dW1.stride(0), db1=db1, partials=partials, partials_bytes=partials.numel() * 4, max_blocks=max_blocks)
        self.record('ga_mlp_bwd', d, label=label)

    def wgrad(self, Y, X, dW, M, N, K, dtype, ldy=None, ldx=None, ldw=None, batch=1, strideY=0, strideX=0, strideW=0,
              x_kind=A_PLAIN, x_dims=(0, 0, 0), x_act=ACT_NONE, dbias=None, strideDbias=0, alpha=1.0, split_m=None,
              accumulate=True, x_batch_mod=0, label=None):
        if split_m is None:
            split_m = pick_split_m(M, N, K, batch, dtype)
        d = _set(L.WgradDesc(), M=M, N=N, K=K, batch=batch, dtype=dtype, Y=Y, ldy=(N if ldy is None else ldy), strideY=strideY,
                 X=X, ldx=(K if ldx is None else ldx), strideX=strideX, x_kind=x_kind, x_batch_mod=x_batch_mod, x_act=x_act,
                 dW=dW, ldw=(K if ldw is None else ldw), strideW=strideW, dbias=dbias, strideDbias=strideDbias, alpha=alpha,
                 split_m=split_m, accumulate=accumulate)
        d.x_H, d.x_W, d.x_C = x_dims
        need = self.lib.ga_wgrad_workspace(C.byref(d))
        if need:
            def patch(ptr, nbytes, d=d):
                d.workspace, d.ws_bytes = ptr, nbytes
            self._want_workspace(int(need), patch)
        self.record('ga_wgrad' if wgrad_fewrows_form(d) == 'none' else 'ga_wgrad_fewrows', d, label=label or 'ga_wgrad')

    def weight_prep(self, w, G, Co, Ci, KH, KW, dtype, out=None, ldo=0, outT=None, ldt=0, rs=None, cs=None, flip=False,
                    stem=False, row_perm=None, t_cols=0, label=None):
        d = _set(L.WprepDesc(), w=w, G=G, Co=Co, Ci=Ci, KH=KH, KW=KW, rs=rs, cs=cs, row_perm=row_perm, dtype=dtype,
                 out=out, ldo=ldo, outT=outT, ldt=ldt, flip=flip, stem=stem, t_cols=t_cols)
        if self.defer:
            return self._defer('wprep', d)
        self.record('ga_weight_prep', d, label=label)

    def bias_fold(self, W, b, rs, v, be, N, Cdim, row_perm=None, label=None):
        if self.defer:
            return self._small(kind=2, y=be, x=W, R=N, C=Cdim, b=b, rs=rs, v=v, row_perm=row_perm)
        self.record('ga_bias_fold', W, b, rs, v, row_perm, be, N, Cdim, label=label)

    def weight_unfold(self, G, ldg, N, Ci, KH=1, KW=1, gb=None, W=None, b=None, rs=None, cs=None, v=None, stem=False, dW=None,
                      db=None, d_rs=None, d_cs=None, d_v=None, row_perm=None, label=None):
        d = _set(L.WunfoldDesc(), G=G, ldg=ldg, gb=gb, W=W, b=b, rs=rs, cs=cs, v=v, row_perm=row_perm, N=N, Ci=Ci, KH=KH, KW=KW,
                 stem=stem, dW=dW, db=db, d_rs=d_rs, d_cs=d_cs, d_v=d_v)
        if self.defer:
            return self._defer('unfold', d)
        self.record('ga_weight_unfold', d, label=label)

    # -- depthwise conv / norms ---------------------------------------------------------------------
    def dwconv7_fwd(self, x, w49, bias, y, B, H, W, Cdim, dtype, label=None):
        self.record('ga_dwconv7_fwd', x, w49, bias, y, B, H, W, Cdim, dtype, label=label)

    def dwconv7_bwd_data(self, dy, w49, res, dx, B, H, W, Cdim, dtype, dx2=None, scale2=None, label=None):
        if dx2 is not None:
            return self.record('ga_dwconv7_bwd_data2', dy, w49, res, dx, dx2, scale2, B, H, W, Cdim, dtype, label=label)
        self.record('ga_dwconv7_bwd_data', dy, w49, res, dx, B, H, W, Cdim, dtype, label=label)

    def dwconv7_bwd_weight(self, dy, x, dw49, dbias, B, H, W, Cdim, dtype, label=None):
        need = int(self.lib.ga_dwconv7_bwd_weight_workspace(B, H, W, Cdim, dtype))
        self._record_ws('ga_dwconv7_bwd_weight', need, dy, x, dw49, dbias, B, H, W, Cdim, dtype, label=label)

    def dwconv3_fwd(self, x, w9, y, B, H, W, Cdim, stride, dtype, colsum=None, colsumsq=None, label=None):
        self.record('ga_dwconv3_fwd', x, w9, y, B, H, W, Cdim, stride, colsum, colsumsq, dtype, label=label)

    def dwconv3_bwd_data(self, dy, w9, dx, B, H, W, Cdim, stride, dtype, label=None):
        self.record('ga_dwconv3_bwd_data', dy, w9, dx, B, H, W, Cdim, stride, dtype, label=label)

    def dwconv3_bwd_weight(self, dy, x, dw9, B, H, W, Cdim, stride, dtype, label=None):
        """dw9 [C][9] += the weight gradient; per-workgroup partials in this plan's per-lane workspace (see dwconv7_bwd_weight)"""
        need = int(self.lib.ga_dwconv3_bwd_weight_workspace(B, H, W, Cdim, stride, dtype))
        self._record_ws('ga_dwconv3_bwd_weight', need, dy, x, dw9, B, H, W, Cdim, stride, dtype, label=label)

    # -- MAP-ResNet50 (csrc/resnet.hip) --------------------------------------------------------------
    def maxpool3s2_fwd(self, x, y, idx, B, H, W, Cdim, dtype, label=None):
        self.record('ga_maxpool3s2_fwd', x, y, idx, B, H, W, Cdim, dtype, label=label)

    def maxpool3s2_bwd(self, dy, idx, dx, B, H, W, Cdim, dtype, accumulate=False, label=None):
        self.record('ga_maxpool3s2_bwd', dy, idx, dx, B, H, W, Cdim, accumulate, dtype, label=label)

    def bn_gelu_fwd(self, x, scale, shift, y, rows, Cdim, dtype, label=None):
        self.record('ga_bn_gelu_fwd', x, scale, shift, y, rows, Cdim, dtype, label=label)

    def bn_gelu_bwd_reduce(self, dy, x, scale, shift, mean, rstd, s1, s2, rows, Cdim, dtype, label=None):
        """s1 / s2 (overwritten) = sum g, sum g * xhat with g = dy * gelu'(x * scale + shift); partials in this plan's per-lane workspace"""
        need = int(self.lib.ga_bn_gelu_bwd_workspace(rows, Cdim))
        self._record_ws('ga_bn_gelu_bwd_reduce', need, dy, x, scale, shift, mean, rstd, s1, s2, rows, Cdim, dtype, label=label)

    def bn_gelu_bwd_apply(self, dy, x, scale, shift, mean, rstd, w, s1, s2, n, dx, rows, Cdim, dtype, label=None):
        self.record('ga_bn_gelu_bwd_apply', dy, x, scale, shift, mean, rstd, w, s1, s2, n, dx, rows, Cdim, dtype, label=label)

    def se_bn_fwd(self, S, HW, scale3, shift3, W1, g1, b1, rmean, rvar, W2, b2, hpre, mean, rstd, h, gate, B, Cdim, R, training, label=None):
        self.record('ga_se_bn_fwd', S, HW, scale3, shift3, W1, g1, b1, rmean, rvar, W2, b2, hpre, mean, rstd, h, gate, B, Cdim, R, training,
                    label=label)

    def se_bn_bwd(self, P1, P2, rowscale, g3, b3, mean3, rstd3, S, HW, scale3, shift3, W1, g1, b1, W2, hpre, mean, rstd, h, gate, dz, dhpre,
                  ds, s1, s2, dW1, dg1, db1, dW2, db2, B, Cdim, R, label=None):
        self.record('ga_se_bn_bwd', P1, P2, rowscale, g3, b3, mean3, rstd3, S, HW, scale3, shift3, W1, g1, b1, W2, hpre, mean, rstd, h, gate,
                    dz, dhpre, ds, s1, s2, dW1, dg1, db1, dW2, db2, B, Cdim, R, label=label)

    def se_residual_fwd(self, x3, scale3, shift3, gate, rowscale, res, rscale, rshift, y, B, HW, Cdim, dtype, label=None):
        self.record('ga_se_residual_fwd', x3, scale3, shift3, gate, rowscale, res, rscale, rshift, y, B, HW, Cdim, dtype, label=label)

    def se_residual_bwd_a(self, dy, y, x3, mean3, rstd3, dm, P1, P2, B, HW, Cdim, dtype, label=None):
        self.record('ga_se_residual_bwd_a', dy, y, x3, mean3, rstd3, dm, P1, P2, B, HW, Cdim, dtype, label=label)

    def se_residual_bwd_b(self, dm, x3, mean3, rstd3, g3, gate, rowscale, ds, s1, s2, dx3, B, HW, Cdim, dtype, label=None):
        self.record('ga_se_residual_bwd_b', dm, x3, mean3, rstd3, g3, gate, rowscale, ds, s1, s2, dx3, B, HW, Cdim, dtype, label=label)

    def subsample2_fwd(self, x, y, B, H, W, Cdim, dtype, label=None):
        self.record('ga_subsample2_fwd', x, y, B, H, W, Cdim, dtype, label=label)

    def subsample2_bwd(self, dy, dx, B, H, W, Cdim, dtype, accumulate=False, label=None):
        self.record('ga_subsample2_bwd', dy, dx, B, H, W, Cdim, accumulate, dtype, label=label)

    def layernorm_fwd(self, x, w, b, y, mean, rstd, rows, Cdim, eps, dtype, label=None):
        self.record('ga_layernorm_fwd', x, w, b, y, mean, rstd, rows, Cdim, eps, dtype, label=label)

    def layernorm_bwd(self, g, x, mean, rstd, w, dres, dx, dw, db, rows, Cdim, x_is_normalized, dtype, label=None, dx2=None,
                      scale2=None, rows_per_scale=1):
        if dx2 is not None:        # second output: the stored dx times a per-sample scale (the consumer's DropPath factor)
            return self.record('ga_layernorm_bwd_dp', g, x, mean, rstd, w, dres, dx, dw, db, rows, Cdim, x_is_normalized, dx2, scale2,
                               rows_per_scale, dtype, label=label)
        self.record('ga_layernorm_bwd', g, x, mean, rstd, w, dres, dx, dw, db, rows, Cdim, x_is_normalized, dtype, label=label)

    def bn_finalize(self, ssum, ssq, n, w, b, eps, momentum, rmean, rvar, mean_out, rstd_out, scale, shift, Cdim,
                    training, label=None):
        self.record('ga_bn_finalize', ssum, ssq, n, w, b, eps, momentum, rmean, rvar, mean_out, rstd_out, scale, shift, Cdim, training,
                    label=label)

    def affine_act(self, x, scale, shift, res, y, rows, Cdim, relu, dtype, rowscale=None, rows_per_scale=1, ldx=0, label=None):
        self.record('ga_affine_act', x, scale, shift, res, rowscale, rows_per_scale, y, rows, Cdim, relu, dtype, ldx, label=label)

    def bn_bwd_reduce(self, dy, y_relu, x, mean, rstd, s1, s2, rows, Cdim, dtype, rowscale=None, rows_per_scale=1, ldx=0,
                      label=None):
        self.record('ga_bn_bwd_reduce', dy, y_relu, x, mean, rstd, rowscale, rows_per_scale, s1, s2, rows, Cdim, dtype, ldx, label=label)

    def bn_bwd_apply(self, dy, y_relu, x, mean, rstd, w, s1, s2, n, dx, rows, Cdim, dtype, rowscale=None,
                     rows_per_scale=1, ldx=0, lddx=0, label=None):
        self.record('ga_bn_bwd_apply', dy, y_relu, x, mean, rstd, w, s1, s2, rowscale, rows_per_scale, n, dx, rows, Cdim, dtype, ldx, lddx,
                    label=label)

    # -- head ---------------------------------------------------------------------------------------
    def pool_concat_fwd(self, src, dst, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, mode, dtype, label=None):
        self.record('ga_pool_concat_fwd', src, dst, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, mode, dtype, label=label)

    def pool_concat_bwd(self, dcat, dres, dsrc, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, mode, dtype, label=None):
        self.record('ga_pool_concat_bwd', dcat, dres, dsrc, B, Hin, Win, Cdim, Hout, Wout, ldd, c_off, mode, dtype, label=label)

    def spatial_sum(self, a, b2, out, B, HW, Cdim, scale, dtype, label=None):
        self.record('ga_spatial_sum', a, b2, out, B, HW, Cdim, scale, dtype, label=label)

    def se_mlp_fwd(self, s, W1, b1, W2, b2, hid, gate, B, Cdim, R, label=None):
        self.record('ga_se_mlp_fwd', s, W1, b1, W2, b2, hid, gate, B, Cdim, R, label=label)

    def se_mlp_bwd(self, dgate, gate, hid, s, W1, W2, ds, dW1, db1, dW2, db2, B, Cdim, R, ds_scale=1.0, label=None):
        self.record('ga_se_mlp_bwd', dgate, gate, hid, s, W1, W2, ds, ds_scale, dW1, db1, dW2, db2, B, Cdim, R, label=label)

    def chan_scale(self, x, g, add, y, B, HW, Cdim, dtype, label=None):
        self.record('ga_chan_scale', x, g, add, y, B, HW, Cdim, dtype, label=label)

    def gram_pack_fwd(self, G, out, inv_norm, B, Cdim, groups, Kp, dtype, label=None):
        self.record('ga_gram_pack_fwd', G, out, inv_norm, B, Cdim, groups, Kp, dtype, label=label)

    def gram_pack_bwd(self, dvec, vhat, inv_norm, S, B, Cdim, groups, Kp, dtype, label=None):
        self.record('ga_gram_pack_bwd', dvec, vhat, inv_norm, S, B, Cdim, groups, Kp, dtype, label=label)

    def gram_f64_fwd(self, x, vec, inv_norm, G64, B, HW, Cdim, H, groups, Kp, dtype, label=None):
        """get_gram's float64 branch: vec from the gram layer's output x; G64 (float64, >= B * ntri) and inv_norm (float64 [B])
        are kept for gram_f64_bwd"""
        self.record('ga_gram_f64_fwd', x, vec, inv_norm, G64, _nbytes(G64), B, HW, Cdim, H, groups, Kp, dtype, label=label)

    def gram_f64_bwd(self, dvec, x, G64, inv_norm, dx, ws, B, HW, Cdim, H, groups, Kp, dtype, label=None):
        """ws: float64 scratch of >= B * C * C entries (ga_gram_f64_bwd_workspace bytes)"""
        self.record('ga_gram_f64_bwd', dvec, x, G64, inv_norm, dx, ws, _nbytes(ws), B, HW, Cdim, H, groups, Kp, dtype, label=label)

    def token_cat(self, cls, tok, u, B, N, Cdim, dtype, label=None):
        self.record('ga_token_cat', cls, tok, u, B, N, Cdim, dtype, label=label)

    def token_split(self, du, dcls, dtok, B, N, Cdim, acc_cls, acc_tok, dtype, label=None):
        self.record('ga_token_split', du, dcls, dtok, B, N, Cdim, acc_cls, acc_tok, dtype, label=label)

    def class_attn_fwd(self, q, kv, out, P, B, N, heads, hd, scale, dtype, label=None):
        self.record('ga_class_attn_fwd', q, kv, out, P, B, N, heads, hd, scale, dtype, label=label)

    def class_attn_bwd(self, dout, q, kv, P, dq, dkv, B, N, heads, hd, scale, dtype, label=None):
        self.record('ga_class_attn_bwd', dout, q, kv, P, dq, dkv, B, N, heads, hd, scale, dtype, label=label)

    def class_attn_fwd2(self, q, kv_cls, kv_tok, out, P, B, N, heads, hd, scale, dtype, tok_ld=0, label=None):
        self.record('ga_class_attn_fwd2', q, kv_cls, kv_tok, tok_ld, out, P, B, N, heads, hd, scale, dtype, label=label)

    def class_attn_bwd2(self, dout, q, kv_cls, kv_tok, P, dq, dkv_cls, dkv_tok, B, N, heads, hd, scale, dtype, tok_ld=0,
                        label=None):
        self.record('ga_class_attn_bwd2', dout, q, kv_cls, kv_tok, tok_ld, P, dq, dkv_cls, dkv_tok, B, N, heads, hd, scale, dtype, label=label)

    # -- GA-CSWin ----------------------------------------------------------------------------------
    def cswin_desc(self, qkv, out, B, reso, Cdim, heads, stripes, lepe, scale, dtype, ldq=None, ldo=None):
        """descriptor of one CSWinBlock's stripe attention: stripes = [(Hs, Ws)] per branch, lepe = [(w [Cb,1,3,3], b [Cb])]"""
        br = list(zip(stripes, lepe))
        return _set(L.CswinAttnDesc(), B=B, reso=reso, C=Cdim, heads=heads, nbranch=len(stripes),
                    Hs=tuple(hs for (hs, _), _ in br), Ws=tuple(ws for (_, ws), _ in br),
                    lepe_w=[w for _, (w, _) in br], lepe_b=[b for _, (_, b) in br], scale=scale, dtype=dtype,
                    qkv=qkv, ldq=(3 * Cdim if ldq is None else ldq), out=out, ldo=(Cdim if ldo is None else ldo))

    def cswin_attn_fwd(self, d, label=None):
        self.record('ga_cswin_attn_fwd', d, label=label)

    def cswin_attn_bwd(self, d, dout, dqkv, lepe_ws=None, label=None):
        """lepe_ws: fp32 buffer of cswin_attn_bwd_workspace(d) bytes -> the kernel also leaves the LePE weight-gradient partials
        there (cswin_lepe_wgrad_reduce adds them up); None: use cswin_lepe_wgrad"""
        self.record('ga_cswin_attn_bwd', d, dout, dqkv, lepe_ws, _nbytes(lepe_ws), label=label)

    def cswin_lepe_wgrad_reduce(self, d, lepe_ws, grads, label=None):
        g = list(grads) + [(None, None)] * (2 - len(grads))
        self.record('ga_cswin_lepe_wgrad_reduce', d, lepe_ws, *g[0], *g[1], label=label)

    def cswin_lepe_wgrad(self, d, dout, grads, label=None):
        """grads = [(dw, db)] per branch (fp32, accumulated into)"""
        g = list(grads) + [(None, None)] * (2 - len(grads))
        self.record('ga_cswin_lepe_wgrad', d, dout, *g[0], *g[1], label=label)

    def layernorm_gelu_fwd(self, x, w, b, y, mean, rstd, rows, Cdim, eps, dtype, label=None):
        self.record('ga_layernorm_gelu_fwd', x, w, b, y, mean, rstd, rows, Cdim, eps, dtype, label=label)

    def layernorm_gelu_bwd(self, g, x, mean, rstd, w, b, dx, dw, db, rows, Cdim, dtype, label=None):
        self.record('ga_layernorm_gelu_bwd', g, x, mean, rstd, w, b, dx, dw, db, rows, Cdim, dtype, label=label)

    def nchw3_to_nhwc8(self, x, y, B, H, W, dtype, label=None):
        self.record('ga_nchw3_to_nhwc8', x, y, B, H, W, dtype, label=label)

    def convw_pack(self, w, out, Co, Ci, taps, Cp, ldo, dtype, label=None):
        self.record('ga_convw_pack', w, out, Co, Ci, taps, Cp, ldo, dtype, label=label)

    def convw_unpack_grad(self, G, dW, Co, Ci, taps, Cp, ldg, label=None):
        self.record('ga_convw_unpack_grad', G, dW, Co, Ci, taps, Cp, ldg, label=label)

    def conv3s2_dgrad_prep(self, w, out, Co, Ci, ldo, dtype, label=None):
        self.record('ga_conv3s2_dgrad_prep', w, out, Co, Ci, ldo, dtype, label=label)

    # -- MAP head -----------------------------------------------------------------------------------
    def gram_pack_fwd2(self, G, out, inv_norm, B, Cdim, groups, Kp, ntok, dtype, label=None):
        self.record('ga_gram_pack_fwd2', G, out, inv_norm, B, Cdim, groups, Kp, ntok, dtype, label=label)

    def gram_pack_bwd2(self, dvec, vhat, inv_norm, S, B, Cdim, groups, Kp, ntok, dtype, label=None):
        self.record('ga_gram_pack_bwd2', dvec, vhat, inv_norm, S, B, Cdim, groups, Kp, ntok, dtype, label=label)

    def map_tokens_fwd(self, e, tok, B, Cdim, T, add_mean, dtype, label=None):
        self.record('ga_map_tokens_fwd', e, tok, B, Cdim, T, add_mean, dtype, label=label)

    def map_tokens_bwd(self, dtok, de, B, Cdim, T, add_mean, dtype, label=None):
        self.record('ga_map_tokens_bwd', dtok, de, B, Cdim, T, add_mean, dtype, label=label)

    def class_attn_mt_fwd(self, q, kv_cls, kv_tok, tok_ld, out, P, mask, B, T, N, heads, hd, scale, dtype, label=None):
        self.record('ga_class_attn_mt_fwd', q, kv_cls, kv_tok, tok_ld, out, P, mask, B, T, N, heads, hd, scale, dtype, label=label)

    def class_attn_mt_bwd(self, dout, q, kv_cls, kv_tok, tok_ld, P, mask, dq, dkv_cls, dkv_tok, dtok_ld, B, T, N, heads, hd, scale,
                          dtype, label=None):
        self.record('ga_class_attn_mt_bwd', dout, q, kv_cls, kv_tok, tok_ld, P, mask, dq, dkv_cls, dkv_tok, dtok_ld, B, T, N, heads, hd,
                    scale, dtype, label=label)

    def class_attn_mt_ia_fwd(self, q, kv_cls, kv_tok, tok_ld, out, P, mask, W1, b1, W2, b2, B, T, N, heads, hd, scale, dtype, label=None):
        self.record('ga_class_attn_mt_ia_fwd', q, kv_cls, kv_tok, tok_ld, out, P, mask, W1, b1, W2, b2, B, T, N, heads, hd, scale, dtype,
                    label=label)

    def class_attn_mt_ia_bwd(self, dout, q, kv_cls, kv_tok, tok_ld, P, mask, W1, W2, b2, dq, dkv_cls, dkv_tok, dtok_ld, dW1, db1, dW2, db2,
                             B, T, N, heads, hd, scale, dtype, label=None):
        self.record('ga_class_attn_mt_ia_bwd', dout, q, kv_cls, kv_tok, tok_ld, P, mask, W1, W2, b2, dq, dkv_cls, dkv_tok, dtok_ld, dW1, db1,
                    dW2, db2, B, T, N, heads, hd, scale, dtype, label=label)

    def map_loss_fwd_bwd(self, org, avg, target, loss, dorg, davg, K, B, NC, lam, kind, smoothing, grad_scale, dtype, label=None):
        self.record('ga_map_loss_fwd_bwd', org, avg, target, loss, dorg, davg, K, B, NC, lam, kind, smoothing, grad_scale, dtype, label=label)

    def loss_dense_fwd_bwd(self, org, avg, target, dense, loss, dorg, davg, K, B, NC, lam, kind, smoothing, bce_threshold, grad_scale,
                           dtype, label=None):
        """GA (avg None) / MAP loss on class indices (`target`) or on a dense [B, NC] fp32 target (`dense`: mixup / cutmix)"""
        self.record('ga_loss_dense_fwd_bwd', org, avg, target, dense, loss, dorg, davg, K, B, NC, lam, kind, smoothing, bce_threshold,
                    grad_scale, dtype, label=label)

    def loss_jsd_fwd_bwd(self, org, avg, target, loss, dorg, davg, K, B, NC, num_splits, lam, smoothing, alpha, grad_scale, dtype,
                         label=None):
        """GA (avg None) / MAP loss with timm's JsdCrossEntropy per head on a split-major batch of num_splits augmentation splits"""
        self.record('ga_loss_jsd_fwd_bwd', org, avg, target, loss, dorg, davg, K, B, NC, num_splits, lam, smoothing, alpha, grad_scale,
                    dtype, label=label)

    def u8_normalize(self, x, out, mean, std, label=None):
        """uint8 (B, C, H, W) -> fp32, (x - mean[c]) / std[c]; mean / std: python sequences in 0..255 units"""
        B, CH, H, W = x.shape
        self.record('ga_u8_normalize', x, out, B, CH, H, W, _host_rows(mean, CH), _host_rows(std, CH), label=label)

    def input_erase(self, x, out, boxes, max_count, mode, seed, offset, mean=None, std=None, label=None):
        """RandomErasing fused with the uint8 normalisation (or a copy of an fp32 x): boxes = device int32 (B, max_count, 4) of
        top, left, h, w; mode 0 const / 1 rand / 2 pixel; mean / std (0..255 units) are used for uint8 x only"""
        B, CH, H, W = x.shape
        u8 = x.dtype == torch.uint8
        m, s = (_host_rows(mean, CH), _host_rows(std, CH)) if u8 else (None, None)
        self.record('ga_input_erase', x, u8, out, B, CH, H, W, m, s, boxes, int(max_count), int(mode), _u64(seed), _u64(offset), label=label)

    def input_collate(self, x, out, mix, boxes=None, max_count=0, mode=0, seed=0, offset=0, mean=None, std=None, label=None):
        """timm's collate-time order in one pass: per-sample mixup / cutmix of a uint8 batch (rounded back to uint8), the
        normalisation, RandomErasing last.  mix = device int32 (B, 8) rows {kind, yl, yh, xl, xh, bits(l), bits(m), 0}; boxes /
        max_count / mode / seed / offset as input_erase (boxes None: no erase).  An fp32 x is blended / box-copied as it is."""
        B, CH, H, W = x.shape
        u8 = x.dtype == torch.uint8
        m, s = (_host_rows(mean, CH), _host_rows(std, CH)) if u8 else (None, None)
        self.record('ga_input_collate', x, u8, out, B, CH, H, W, m, s, mix, boxes, int(max_count), int(mode), _u64(seed), _u64(offset),
                    label=label)

    def rand_augment(self, x, out, work, table, n_layers, fill, label=None):
        """timm RandAugment on a uint8 (B, 3, H, W) batch, out of place: table = device uint8 (B, n_layers, 64) of rows
        {kind, interp, iarg, farg, m[6]} (include/gaext.h), work = device uint8 scratch of rand_augment_work_bytes() bytes (None
        without layers), fill = the CH bytes a pixel without a source takes"""
        B, CH, H, W = x.shape
        self.record('ga_rand_augment', x, out, work, C.c_size_t(_nbytes(work)), B, CH, H, W, table, int(n_layers),
                    (C.c_ubyte * CH)(*[int(v) for v in fill]), label=label)

    def rand_augment_work_bytes(self, B, CH, H, W, n_layers):
        return int(self.lib.ga_rand_augment_work_bytes(B, CH, H, W, int(n_layers)))

    def resize_crop(self, src, table, out, work, B, OH, OW, label=None):
        """crop + PIL-exact resize (+ flip, + window) of decoded images: src = device uint8 byte buffer of interleaved HWC images,
        table = device uint8 (B, 64) of rows {src_off, src_h, src_w, top, left, h, w, vh, vw, oy, ox, interp, flip} (include/gaext.h),
        out = uint8 (B, 3, OH, OW), work = device uint8 scratch of ga_resize_crop_work_bytes(host table) bytes"""
        self.record('ga_resize_crop', src, _u64(_nbytes(src)), table, out, work, C.c_size_t(_nbytes(work)), int(B), int(OH), int(OW),
                    label=label)

    def resample_coeffs(self, in_size, out_size, interp, bounds, coeffs, ksize, label=None):
        """one axis of PIL's 8-bit resample coefficients: bounds = device int32 (out, 2), coeffs = device int32 (out, ksize)"""
        self.record('ga_resample_coeffs', int(in_size), int(out_size), int(interp), bounds, coeffs, int(ksize), label=label)

    def jpeg_reconstruct(self, table, n_images, coef, qt, work, dst, label=None):
        """quantised JPEG coefficients -> interleaved HWC RGB images, byte for byte libjpeg-turbo's: table = device uint8 (n, 64) of
        rows {coef_off, dst_off, work_off, qt_off, width, height, ncomp, hs, vs, mcus_w, mcus_h} (include/gaext.h), coef = device
        int16, qt = device uint16 (3 x 64 per image), work = device uint8 scratch of ga_jpeg_work_bytes(host table) bytes, dst = the
        RaggedBatch byte buffer"""
        self.record('ga_jpeg_reconstruct', table, int(n_images), coef, qt, work, dst, label=label)

    def mixup_target_elem(self, target, out, NC, lam, smoothing, label=None):
        """dense target of per-sample lams: lam = device fp32 (B,)"""
        self.record('ga_mixup_target_elem', target, out, target.numel(), NC, lam, float(smoothing), label=label)

    def mixup_batch(self, x, out, lam, cutmix=False, box=(0, 0, 0, 0), label=None):
        B, CH, H, W = x.shape
        yl, yh, xl, xh = (int(v) for v in box)
        self.record('ga_mixup_batch', x, out, B, CH, H, W, float(lam), int(cutmix), yl, yh, xl, xh, label=label)

    def mixup_target(self, target, out, NC, lam, smoothing, label=None):
        self.record('ga_mixup_target', target, out, target.numel(), NC, float(lam), float(smoothing), label=label)

    def agc_clip(self, params, grads, units, nunits, clip_factor, eps=1e-3, label=None):
        self.record('ga_agc_clip', params, grads, units, nunits, float(clip_factor), float(eps), label=label)

    def gelu_fwd(self, x, y, n, dtype, label=None):
        self.record('ga_gelu_fwd', x, y, n, dtype, label=label)

    def gelu_bwd(self, dy, x, dx, n, dtype, label=None):
        self.record('ga_gelu_bwd', dy, x, dx, n, dtype, label=label)

    def relu_drop(self, a, mask, out, deriv, n, dtype, label=None):
        self.record('ga_relu_drop', a, mask, out, deriv, n, dtype, label=label)

    def mask_mul(self, x, mask, res, y, n, dtype, label=None):
        self.record('ga_mask_mul', x, mask, res, y, n, dtype, label=label)

    def copy2d(self, src, lds, dst, ldd, rows, cols, dtype, accumulate=False, label=None):
        self.record('ga_copy2d', src, lds, dst, ldd, rows, cols, accumulate, dtype, label=label)

    # -- loss / metric / optimizer ------------------------------------------------------------------
    def loss_fwd_bwd(self, logits, target, loss, dlogits, K, B, NC, lam, kind, smoothing, grad_scale, dtype, label=None):
        self.record('ga_loss_fwd_bwd', logits, target, loss, dlogits, K, B, NC, lam, kind, smoothing, grad_scale, dtype, label=label)

    def heads_topk(self, logits, K, B, NC, topk, out_sum, out_idx, label=None):
        self.record('ga_heads_topk', logits, K, B, NC, topk, out_sum, out_idx, label=label)

    def sgd_step(self, p, g, buf, hp, n, nesterov, wd_mult, label=None):
        self.record('ga_sgd_step', p, g, buf, hp, n, nesterov, wd_mult, label=label)

    def adamw_step(self, p, g, m, v, hp, n, wd_mult, label=None):
        self.record('ga_adamw_step', p, g, m, v, hp, n, wd_mult, label=label)

    def adam_step(self, p, g, m, v, hp, n, wd_mult, label=None):
        self.record('ga_adam_step', p, g, m, v, hp, n, wd_mult, label=label)

    def rmsprop_step(self, p, g, sq, buf, hp, n, tf, wd_mult, label=None):
        self.record('ga_rmsprop_step', p, g, sq, buf, hp, n, bool(tf), wd_mult, label=label)

    def lion_step(self, p, g, m, hp, n, wd_mult, label=None):
        self.record('ga_lion_step', p, g, m, hp, n, wd_mult, label=label)

    def drop_path_sample(self, out, keep, sites, B, seed, counter, label=None):
        self.record('ga_drop_path_sample', out, keep, sites, B, _u64(seed), counter, label=label)

    def dropout_mask_sample(self, out, n, keep, seed, counter, label=None):
        self.record('ga_dropout_mask_sample', out, n, float(keep), _u64(seed), counter, label=label)

    # -- utilities ----------------------------------------------------------------------------------
    def transpose_f32(self, src, dst, R, Cdim, accumulate=False, label=None):
        if self.defer:
            return self._small(kind=1, y=dst, x=src, R=R, C=Cdim, accumulate=accumulate)
        self.record('ga_transpose_f32', src, dst, R, Cdim, accumulate, label=label)

    def axpy_f32(self, y, x, a, n, label=None):
        if self.defer:
            return self._small(kind=0, y=y, x=x, a=a, n=n)
        self.record('ga_axpy_f32', y, x, a, n, label=label)

    def lamb_stage1(self, p, g, m, v, u, hp, gsumsq, chunks, nchunks, norms, label=None):
        self.record('ga_lamb_stage1', p, g, m, v, u, hp, gsumsq, chunks, nchunks, norms, label=label)

    def lamb_stage2(self, p, u, hp, chunks, nchunks, norms, label=None):
        self.record('ga_lamb_stage2', p, u, hp, chunks, nchunks, norms, label=label)

    def lars_stage1(self, p, g, chunks, nchunks, norms, label=None):
        self.record('ga_lars_stage1', p, g, chunks, nchunks, norms, label=label)

    def lars_stage2(self, p, g, buf, hp, chunks, nchunks, norms, nesterov, trust_clip, label=None):
        self.record('ga_lars_stage2', p, g, buf, hp, chunks, nchunks, norms, bool(nesterov), bool(trust_clip), label=label)

    def lerp_f32(self, y, x, w, n, label=None):
        self.record('ga_lerp_f32', y, x, float(w), n, label=label)

    def sumsq_f32(self, x, n, out, label=None):
        self.record('ga_sumsq_f32', x, n, out, label=label)

    def clip_grad_f32(self, g, n, sumsq, limit, mode, label=None):
        self.record('ga_clip_grad_f32', g, n, sumsq, float(limit), int(mode), label=label)

    def rowscale(self, x, s, y, n, elems_per_scale, dtype, label=None):
        self.record('ga_rowscale', x, s, y, n, elems_per_scale, dtype, label=label)

    def cast_from_f32(self, src, dst, n, dtype, label=None):
        self.record('ga_cast_from_f32', src, dst, n, dtype, label=label)

    def cast_to_f32(self, src, dst, n, dtype, label=None):
        self.record('ga_cast_to_f32', src, dst, n, dtype, label=label)

    def zero(self, t, label=None):
        """memset a persistent buffer (hipMemsetAsync on the plan's stream)."""
        self.record('ga_memset', t, 0, _nbytes(t), label=label or 'zero')


def mlp_supported(Cdim, H, dtype):
    return bool(L.load().ga_mlp_supported(Cdim, H, dtype))


def mlp_bwd_wgrad_supported(Cdim, H, dtype):
    """Plan.mlp_bwd can accumulate the fc1 weight gradient itself (dW1=...) at this shape"""
    return bool(L.load().ga_mlp_bwd_wgrad_supported(Cdim, H, dtype))


def mlp_bwd_partials(M, Cdim, dtype, max_blocks=0):
    """bytes of the fp32 `partials` scratch Plan.mlp_bwd(dW1=...) takes for M rows (0: not supported)"""
    d = L.MlpBwdDesc()
    d.M, d.C, d.H, d.dtype, d.max_blocks = M, Cdim, 4 * Cdim, dtype, max_blocks
    return int(L.load().ga_mlp_bwd_partials(C.byref(d)))


def gemm_form(d):
    """name of the kernel form ga_gemm launches for this GemmDesc under the current knobs (include/gaext.h: ga_gemm_form);
    raises as the launch would for a descriptor it rejects.  Needs no GPU."""
    buf = C.create_string_buffer(64)
    L.check(L.load().ga_gemm_form(C.byref(d), buf, 64), 'ga_gemm_form')
    return buf.value.decode()


def wgrad_form(d):
    """... and ga_wgrad for this WgradDesc (ga_wgrad_form)"""
    buf = C.create_string_buffer(64)
    L.check(L.load().ga_wgrad_form(C.byref(d), buf, 64), 'ga_wgrad_form')
    return buf.value.decode()


def gemm_fewrows_form(d):
    """the few-row form ga_gemm_fewrows runs this GemmDesc on itself (ga_gemm_fewrows_form), 'none' when it forwards the descriptor
    to ga_gemm -- also for a descriptor the launch will reject: the error is the launch's to raise"""
    buf = C.create_string_buffer(64)
    return buf.value.decode() if L.load().ga_gemm_fewrows_form(C.byref(d), buf, 64) == 0 else 'none'


def wgrad_fewrows_form(d):
    """... and ga_wgrad_fewrows for this WgradDesc (ga_wgrad_fewrows_form)"""
    buf = C.create_string_buffer(64)
    return buf.value.decode() if L.load().ga_wgrad_fewrows_form(C.byref(d), buf, 64) == 0 else 'none'


def cswin_attn_bwd_workspace(d):
    """bytes of the LePE partial buffer Plan.cswin_attn_bwd takes for this descriptor (0: generic form, no fused partials)"""
    return int(L.load().ga_cswin_attn_bwd_workspace(C.byref(d)))


def zero_(t):
    """t.zero_() as a hipMemsetAsync on the current stream through the C ABI"""
    L.check(L.load().ga_memset(_ptr(t), 0, t.numel() * t.element_size(), current_stream_ptr()), 'ga_memset')
    return t


_NUM_CU = None


def num_cus():
    global _NUM_CU
    if _NUM_CU is None:
        n = C.c_int(256)
        L.check(L.load().ga_device_info(C.byref(n), None, None), 'ga_device_info')
        _NUM_CU = n.value
    return _NUM_CU


def pick_split_m(M, N, K, batch, dtype):
    """Number of row-range splits of a wgrad so that ~2 workgroups per CU are in flight, each with >= 4 slabs."""
    slab = 64 if dtype == GA_BF16 else 32
    tiles = ((N + 127) // 128) * ((K + 127) // 128) * batch
    want = max(1, (2 * 256) // tiles)
    return int(max(1, min(want, (M + 4 * slab - 1) // (4 * slab))))
