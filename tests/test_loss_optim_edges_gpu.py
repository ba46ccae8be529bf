"""The kernels of csrc/loss_optim.hip (the fused GA / MAP loss with its gradient, heads_topk, the flat SGD / AdamW steps, the two LAMB
stages, sumsq / clip / AGC, the two mask samplers, mixup_batch and u8_normalize) at the edges of their launch geometry, against the
float64 references of tests/_loss_optim_ref.py, through the C ABI, with outputs in NaN-filled guarded allocations.  Sizes follow from
the kernels' own constants (R.STRIDE, R.LDS_OPT_IN, R.LAMB_CHUNK): every flat kernel is run below, at and above the element count
at which it starts to loop, the loss and heads_topk on both sides of the 64 KiB LDS opt-in and at the 36000 limit.  No case skips; a
case whose size no longer reaches its regime fails on the assertion that states the regime.

Gate: R.gate(), per element |got - ref| <= r |ref| + a0 + EPS_FAST ce + floor, all derived from the kernels' roundings except
EPS_FAST (the hardware exp / log behind __expf / __logf).  tests/test_loss_optim_ref_cpu.py proves that fp32 arithmetic in the
kernels' order meets the gate and that the named wrong restatements do not.  Optimizer steps are gated one step at a time from the
state the kernel itself left.  Every case prints its worst err / allowed per tensor, the module prints the worst per kernel and
dtype and the largest EPS_FAST any loss case would have needed (run with -s).

Worst err / allowed seen on an MI355X, all 101 tests passing; the module takes 3.5 s (1.6 s inside the tests; slowest: the first
loss case with the library load, 0.5 s, and the 524288 / 1048583-element sampler cases, 0.1 s, whose masks the integer restatement
computes on the host).
                          p      m      v      buf    u      norms  gsumsq
    sgd            fp32   0.499                0.484
    adamw          fp32   0.555  0.647  0.716
    lamb (fused)   fp32   0.957  0.631  0.681         0.317  0.140  0.037
    lamb stages    fp32   0.950  0.611  0.484         0.315  0.061             (both runs the same figures)
                          loss   dorg   davg
    loss           fp32   0.032  0.912  0.241
    loss           bf16   0.032  0.995  0.992
    sumsq 0.043 (n = 4)   clip norm 0.087 (n = 7, clipping)   agc 0.218 (4 units)   everything else is bit-exact by assertion
Closest to the limit: the bf16 gradients at 0.99, all of it the ONE rounding of the store (r |ref|); dorg in fp32 at 0.91 on
K2-B3-NC16377-bce-randn30, the only case that needs any of the intrinsic allowance; LAMB's p at 0.91 - 0.96, whose bound counts the
three roundings of p - (lr trust) u at their worst on 73461 elements.

The fast-intrinsic allowance.  With EPS_FAST = 0 every loss case but one meets the gate on the derived roundings alone; K2-B3-NC16377-
bce-s0.0-dense1-thr0.2-noavg-gs0.25-randn30 (fp32 gradient) needs 1.68e-07 = 2^-22.5 per hardware exp / log.  Chosen: 4 x that, 6.72e-07
(R.EPS_FAST).  The weakest wrong loss restatement of tests/test_loss_optim_ref_cpu.py (`undetached`) would need 3.17e-05 to pass,
47 x the chosen value (asserted there: at least 4 x); every other one needs more than 0.2.

Found: one wrong kernel, no other.  The > 64 KiB LDS paths of the loss and of heads_topk (NC = 16377 / 16385 up to 36000), NC below a
wave, K = 1, B = 1, logits of magnitude 100 (softmax tails that underflow), rows that do not sum to 1, grad_scale 0.25 and 65536,
the three-trip grid strides of every flat kernel, LAMB's per-tensor trust ratio over one to three chunks with the plan's re-zeroing
(both accumulators poisoned beforehand), the range updates (bit-identical to step()), the samplers (bit-identical to the documented
generator, one counter step per call and per replay) and every refusal hold.
  * heads_topk_kernel stored a NaN sum as +inf in its LDS row ("torch.topk ranks NaN largest"), so a +inf at a LOWER index than the
    NaN tied with it and won on the index: row 4 of _topk_logits (+inf at 1, NaN at 3) gave 1, 3 where torch.topk and R.topk_ref give
    3, 1 (R.topk_restate(wrong='nan_as_inf') keeps that order on record; tests/test_loss_optim_ref_cpu.py shows it differs on exactly
    such rows).  The row is now kept as order-preserving unsigned keys: NaN has the largest, -0 and +0 share one, 0 marks an index
    already taken.  The comment's "k <= 8" was not a limit of the code: any topk <= NC works, and topk = NC is run here at NC = 5 .. 65.
  * not a defect, on record: the hp row carries beta2 as fp32, so the kernels' 1 - beta2 is 1 - fp32(0.999), smaller by 1.3e-5 of itself than the
    0.001 torch forms in double; the references therefore take the fp32 row as the kernels' input (R.hp_row, compared bit for bit
    with what FusedLamb pushes).  oracle.ga_convnext_oracle builds the smoothed BCE target in fp32, which the float64 comparison
    of the CPU module allows for by name.
"""
import ctypes as C
import math
import time

import pytest
import torch

import _loss_optim_ref as R
from _loss_optim_ref import BF, F32, F64
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu

WORST = {}       # (kernel, dtype, tensor) -> (worst ratio, case)
NEED = [0.0, '']
T0 = [None]
BAD_ARG = -1
I64 = torch.int64


def _L():
    from imagenet_models_amd import _lib
    return _lib


def _ops():
    from imagenet_models_amd import ops
    return ops


def _p(t):
    if t is None:
        return None
    return (t.view if isinstance(t, Guarded) else t).data_ptr()


def call(name, *args):
    """the C entry point on the current stream; Guarded / tensors pass as pointers"""
    a = [(_p(x) if (x is None or isinstance(x, (Guarded, torch.Tensor))) else x) for x in args]
    return getattr(_L().load(), name)(*a, torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    _L().check(rc, what)


def vec(data, dt=F32, off=0, n=None):
    """a guarded flat vector; `off` shifts it off 16-byte alignment"""
    n = data.numel() if data is not None else n
    return Guarded(1, n, n, dt, data=None if data is None else data.reshape(1, -1), off=off, guard=64)


def f64(g):
    return (g.inner() if isinstance(g, Guarded) else g).reshape(-1).double()


def note(kernel, dt, tensor, ratio, label):
    key = (kernel, 'bf16' if dt == BF else 'fp32', tensor)
    if ratio > WORST.get(key, (-1.0, ''))[0]:
        WORST[key] = (ratio, label)


def settle(kernel, dt, label, ratios):
    print(f'[{kernel} {label}] ' + '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    for n, v in ratios.items():
        note(kernel, dt, n, v, label)
    bad = {n: v for n, v in ratios.items() if not v < 1.0}
    assert not bad, f'{kernel} {label}: err / allowed {bad}'


def resnap(*gs):
    """what a refused call must leave alone is the state from here on"""
    torch.cuda.synchronize()
    for g in gs:
        g.before = _bits(g.flat).clone()
    return gs


def refused(rc, fn, outs):
    assert rc == BAD_ARG, rc
    assert fn in _L().last_error(), (fn, _L().last_error())
    torch.cuda.synchronize()
    for g in outs:
        g.check('refused', written=False)


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a test that leaves the device in error ends the session: nothing more is launched on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


@pytest.fixture(scope='module', autouse=True)
def _report():
    T0[0] = time.time()
    yield
    print(f'\nworst err / allowed per kernel, dtype and tensor (module wall time {time.time() - T0[0]:.1f} s):')
    for k in sorted(WORST):
        print(f'    {k[0]:14s} {k[1]:5s} {k[2]:8s} {WORST[k][0]:.3f}   {WORST[k][1]}')
    print(f'    largest EPS_FAST a loss case needs: {NEED[0]:.3g} = 2^{math.log2(NEED[0]) if NEED[0] > 0 else float("-inf"):.2f} ({NEED[1]}); '
          f'chosen {R.EPS_FAST:.3g} = 2^{math.log2(R.EPS_FAST):.0f}')


# ----------------------------------------------------------------------------------------------------------------------------
# loss
# ----------------------------------------------------------------------------------------------------------------------------
_LOSS = {}


def _loss_ref(c):
    if c.label not in _LOSS:
        i = R.loss_inputs(c)
        _LOSS[c.label] = (i, R.loss_ref(i, c))
    return _LOSS[c.label]


def _loss_call(c, dt, org, avg, target, dense, loss, dorg, davg):
    gd = 1 if dt == BF else 0
    e = c.entry()
    if e == 'ga_loss_fwd_bwd':
        return call(e, org, target, loss, dorg, c.K, c.B, c.NC, c.lam, c.kind, c.smooth, c.gs, gd)
    if e == 'ga_map_loss_fwd_bwd':
        return call(e, org, avg, target, loss, dorg, davg, c.K, c.B, c.NC, c.lam, c.kind, c.smooth, c.gs, gd)
    return call(e, org, avg, target, dense, loss, dorg, davg, c.K, c.B, c.NC, c.lam, c.kind, c.smooth, c.thr, c.gs, gd)


@pytest.mark.parametrize('dt', [F32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('c', R.LOSS_CASES, ids=repr)
def test_loss(c, dt):
    assert ((c.NC + 8) * 4 > R.LDS_OPT_IN) == (c.NC >= 16377) and c.NC <= R.NC_MAX, 'the LDS opt-in no longer starts at NC = 16377'
    i, ref = _loss_ref(c)
    K, B, NC = c.K, c.B, c.NC
    org = vec(i['org'])
    avg = None if i['avg'] is None else vec(i['avg'])
    dense = None if i['dense'] is None else vec(i['dense'])
    target = None if i['target'] is None else i['target'].cuda()
    loss = vec(torch.tensor([i['initial']], dtype=F64))
    dorg = Guarded(K * B, NC, NC, dt, guard=64) if c.grad else None
    davg = Guarded(K * B, NC, NC, dt, guard=64) if (c.grad and c.avg) else None
    ok(_loss_call(c, dt, org, avg, target, dense, loss, dorg, davg), c.entry())
    torch.cuda.synchronize()
    got = dict(loss=float(f64(loss)[0]) - i['initial'], dorg=None, davg=None)
    loss.check('loss')
    for n, g in (('dorg', dorg), ('davg', davg)):
        if g is not None:
            g.check(n)
            got[n] = g.inner().double().cpu().view(K, B, NC)
    for g in (org, avg, dense):
        if g is not None:
            g.check('input', written=False)
    if davg is not None and dt == F32:          # avg without davg: the same loss and dorg, nothing else
        loss2, dorg2 = vec(torch.tensor([i['initial']], dtype=F64)), Guarded(K * B, NC, NC, dt, guard=64)
        ok(_loss_call(c, dt, org, avg, target, dense, loss2, dorg2, None), 'without davg')
        torch.cuda.synchronize()
        dorg2.check('dorg (no davg)')
        assert torch.equal(_bits(dorg2.inner()), _bits(dorg.inner()))
        assert abs(float(f64(loss2)[0]) - float(f64(loss)[0])) <= ref['loss'][1] + R.EPS_FAST * ref['loss'][2]
    need = R.loss_need_eps(got, ref, dt, c.gs)
    if need > NEED[0]:
        NEED[0], NEED[1] = need, f'{c.label} {"bf16" if dt == BF else "fp32"}'
    ratios = R.loss_ratios(got, ref, dt, c.gs)
    print(f'    eps_fast needed {need:.3g}')
    settle('loss', dt, c.label, ratios)


def test_loss_refuses_what_it_cannot_run():
    c = R.LOSS_CASES[2]
    i, _ = _loss_ref(c)
    org, avg, loss = vec(i['org']), vec(i['avg']), vec(torch.tensor([1.5], dtype=F64))
    dorg, davg = vec(None, n=c.K * c.B * c.NC), vec(None, n=c.K * c.B * c.NC)
    t, dense = i['target'].cuda(), vec(torch.ones(c.B, c.NC, dtype=F64))
    outs = (loss, dorg, davg)
    a = lambda **kw: [kw.get('org', org), kw.get('avg', avg), kw.get('t', t), kw.get('dense', None), kw.get('loss', loss), dorg, davg,
                      kw.get('K', c.K), kw.get('B', c.B), kw.get('NC', c.NC), c.lam, kw.get('kind', 0), 0.1, -1.0, 1.0, 0]
    fn = 'ga_loss_fwd_bwd'            # the three entry points report under one name
    refused(call('ga_loss_dense_fwd_bwd', *a(NC=36001)), fn, outs)
    assert '36000' in _L().last_error()
    refused(call('ga_loss_dense_fwd_bwd', *a(org=None)), fn, outs)
    refused(call('ga_loss_dense_fwd_bwd', *a(loss=None)), fn, outs)
    refused(call('ga_loss_dense_fwd_bwd', *a(dense=dense)), fn, outs)             # both targets
    refused(call('ga_loss_dense_fwd_bwd', *a(t=None)), fn, outs)                  # neither
    refused(call('ga_loss_dense_fwd_bwd', *a(K=0)), fn, outs)
    refused(call('ga_loss_dense_fwd_bwd', *a(B=0)), fn, outs)
    refused(call('ga_loss_dense_fwd_bwd', *a(NC=0)), fn, outs)
    refused(call('ga_loss_dense_fwd_bwd', *a(kind=2)), fn, outs)
    refused(call('ga_loss_fwd_bwd', None, t, loss, dorg, c.K, c.B, c.NC, c.lam, 0, 0.1, 1.0, 0), fn, outs)
    refused(call('ga_map_loss_fwd_bwd', org, avg, None, loss, dorg, davg, c.K, c.B, c.NC, c.lam, 0, 0.1, 1.0, 0), fn, outs)


# ----------------------------------------------------------------------------------------------------------------------------
# heads_topk
# ----------------------------------------------------------------------------------------------------------------------------
def _topk_logits(NC):
    """K = 3 heads, 8 rows: random; ties inside one lane's stride (c, c + 64) and across lanes (c, c + 1); ties at 0 and NC - 1; all
    equal; -inf, +inf and NaN (the NaN behind the +inf); all -inf but one; signed zeros; random"""
    g = torch.Generator().manual_seed(40 + NC)
    x = torch.randn(3, 8, NC, generator=g)
    for r, cols, v in ((1, (3, 3 + 64, 3 + 128, 4, NC - 2), 9.0), (2, (0, NC - 1), 11.0)):
        for cc in cols:
            if 0 <= cc < NC:
                x[:, r, cc] = v
    x[:, 3, :] = 0.75
    x[0, 4, 1 % NC] = float('inf')
    if NC > 3:
        x[1, 4, 3] = float('nan')
        x[2, 4, 2] = float('-inf')
    x[:, 5, :] = float('-inf')
    x[:, 5, NC // 2] = -2.0
    x[:, 6, :] = 0.0
    x[0, 6, ::2] = -0.0
    if NC > 4:
        x[:, 6, 4] = 1.0
    return x


@pytest.mark.parametrize('NC', [5, 63, 64, 65, 1000, 16384, 16385, 36000])
def test_heads_topk(NC):
    assert (NC * 4 > R.LDS_OPT_IN) == (NC >= 16385), 'the LDS opt-in no longer starts at NC = 16385'
    x = _topk_logits(NC)
    xs = vec(x)
    for topk in sorted({1, 5, 8, NC if NC <= 65 else 1} & set(range(1, NC + 1))):
        s_ref, i_ref = R.topk_ref(x, topk)
        s = Guarded(8, NC, NC, F32, guard=64)
        idx, idx2 = torch.full((8, topk), -7, dtype=I64, device='cuda'), torch.full((8, topk), -7, dtype=I64, device='cuda')
        ok(call('ga_heads_topk', xs, 3, 8, NC, topk, s, idx), 'heads_topk')
        ok(call('ga_heads_topk', xs, 3, 8, NC, topk, None, idx2), 'heads_topk without out_sum')
        torch.cuda.synchronize()
        got = s.inner().cpu()
        nan = torch.isnan(s_ref)
        assert torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(s_ref)[~nan]), f'NC {NC}: out_sum is not the k-ordered fp32 sum'
        same = _bits(s.flat) == s.before
        inside = torch.zeros_like(same)
        inside[s.start:s.start + 8 * NC] = True
        assert bool(same[~inside].all()), 'out_sum guards written'
        bad = (idx.cpu() != i_ref).any(1).nonzero().flatten().tolist()
        assert not bad, f'NC {NC} topk {topk}: rows {bad} differ: {idx.cpu()[bad[0]].tolist()} != {i_ref[bad[0]].tolist()}'
        assert torch.equal(idx, idx2)
    xs.check('logits', written=False)
    idx = torch.full((8, 5), -7, dtype=I64, device='cuda')
    assert call('ga_heads_topk', xs, 3, 8, NC, NC + 1, None, idx) == BAD_ARG and 'ga_heads_topk' in _L().last_error()
    assert call('ga_heads_topk', None, 3, 8, NC, 1, None, idx) == BAD_ARG
    assert call('ga_heads_topk', xs, 3, 8, NC, 1, None, None) == BAD_ARG
    assert call('ga_heads_topk', xs, 3, 8, 36001, 1, None, idx) == BAD_ARG and '36000' in _L().last_error()
    torch.cuda.synchronize()
    assert bool((idx == -7).all())


# ----------------------------------------------------------------------------------------------------------------------------
# flat SGD / AdamW
# ----------------------------------------------------------------------------------------------------------------------------
S_OPT = 2097152
FLAT_N = [1, 255, 256, 257, S_OPT, S_OPT + 1, S_OPT + 8192 * 256 + 3]


def _flat_inputs(n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    rn = lambda sc: (torch.randn(n, generator=g, device='cuda') * sc).double()
    return rn(0.05), [rn(0.01) for _ in range(3)], rn(3.0)


@pytest.mark.parametrize('n', FLAT_N)
def test_flat_sgd(n):
    assert R.STRIDE['sgd'] == S_OPT and math.ceil(FLAT_N[-1] / S_OPT) == 3, 'the sizes no longer enter the stride loop'
    p0, grads, poison = _flat_inputs(n, 21)
    combos = [(True, 1.0), (False, 0.0)] if n > 4096 else [(True, 1.0), (True, 0.0), (False, 1.0), (False, 0.0)]
    for nesterov, mult in combos:
        p, buf = vec(p0, off=3), vec(poison, off=1)          # a stale nonzero buf: the first step must not read it
        worst = {}
        for s, g64 in enumerate(grads):
            hp = R.hp_row('sgd', 5e-3, 0.05, 0.9, first=s == 0)
            h = [float(v) for v in hp]
            g = vec(g64, off=3)
            (rp,), (rb,), (al,) = R.sgd_step([f64(p)], [g64], [f64(buf)], [mult != 0], h[0], h[1], h[2], nesterov, s == 0)
            ok(call('ga_sgd_step', p, g, buf, hp.cuda(), n, int(nesterov), mult), 'sgd_step')
            torch.cuda.synchronize()
            for name, gd in (('p', p), ('buf', buf)):
                gd.check(name)
            g.check('g', written=False)
            for name, got, ref in (('p', p, rp), ('buf', buf, rb)):
                worst[name] = max(worst.get(name, 0.0), R.gate(f64(got), ref, al[name]))
        settle('sgd', F32, f'n{n}-nesterov{int(nesterov)}-wd{mult:.0f}', worst)


@pytest.mark.parametrize('n', FLAT_N)
def test_flat_adamw(n):
    assert R.STRIDE['adamw'] == S_OPT
    p0, grads, _ = _flat_inputs(n, 22)
    for mult in (1.0, 0.0):
        p, m, v = vec(p0, off=3), vec(torch.zeros(n), off=1), vec(torch.zeros(n), off=2)
        worst = {}
        for s, g64 in enumerate(grads):
            hp = R.hp_row('adamw', 5e-3, 0.05, *R.BETAS, 1e-8, s + 1)
            h = [float(x) for x in hp]
            g = vec(g64, off=3)
            (rp,), (rm,), (rv,), (al,) = R.adamw_step([f64(p)], [g64], [f64(m)], [f64(v)], [mult != 0], h[0], h[1], h[2], h[3], h[4], bc1=h[5], bc2=h[6])
            ok(call('ga_adamw_step', p, g, m, v, hp.cuda(), n, mult), 'adamw_step')
            torch.cuda.synchronize()
            for name, gd in (('p', p), ('m', m), ('v', v)):
                gd.check(name)
            g.check('g', written=False)
            for name, got, ref in (('p', p, rp), ('m', m, rm), ('v', v, rv)):
                worst[name] = max(worst.get(name, 0.0), R.gate(f64(got), ref, al[name]))
        settle('adamw', F32, f'n{n}-wd{mult:.0f}', worst)


def test_flat_step_refusals():
    p, g, m, v = (vec(torch.ones(8)) for _ in range(4))
    hp = R.hp_row('adamw', 5e-3, 0.05, *R.BETAS, 1e-8, 1).cuda()
    outs = (p, m, v)
    for a in ((None, g, m, hp, 8), (p, None, m, hp, 8), (p, g, None, hp, 8), (p, g, m, None, 8), (p, g, m, hp, 0)):
        refused(call('ga_sgd_step', *a, 1, 1.0), 'ga_sgd_step', outs)
    for a in ((None, g, m, v, hp, 8), (p, None, m, v, hp, 8), (p, g, None, v, hp, 8), (p, g, m, None, hp, 8), (p, g, m, v, None, 8), (p, g, m, v, hp, 0)):
        refused(call('ga_adamw_step', *a, 1.0), 'ga_adamw_step', outs)


# ----------------------------------------------------------------------------------------------------------------------------
# LAMB
# ----------------------------------------------------------------------------------------------------------------------------
def _cpu_lists(stub, flat):
    return [t.double().cpu() for t in stub.split(flat)]


def _lamb_ref(c, ps, gs, ms, vs, t):
    hp = R.hp_row('lamb', R.LAMB_LR, c['wd'], *R.BETAS, c['eps'], t, grad_averaging=c['avg'])
    h = [float(x) for x in hp]
    return hp, R.lamb_step(ps, gs, ms, vs, R.decay_flags(), h[0], h[1], h[2], h[3], h[4], max_grad_norm=h[8], bc1=h[5], bc2=h[6], b3=h[7])


@pytest.mark.parametrize('label', list(R.LAMB_CASES))
def test_fused_lamb(label):
    from imagenet_models_amd.optim import FusedLamb
    c = R.LAMB_CASES[label]
    p0, grads = R.lamb_inputs(label)
    P, G = vec(torch.cat(p0)), vec(None, n=sum(R.LAMB_SIZES))
    stub = R.FlatStub(R.LAMB_SIZES, R.LAMB_NDECAY, params=P.view.view(-1), grads=G.view.view(-1))
    opt = FusedLamb(stub, lr=R.LAMB_LR, betas=R.BETAS, eps=c['eps'], weight_decay=c['wd'], max_grad_norm=1.0, grad_averaging=c['avg'])
    assert opt.CHUNK == R.LAMB_CHUNK and opt.chunks.shape[0] == sum(math.ceil(n / R.LAMB_CHUNK) for n in R.LAMB_SIZES)
    assert opt.chunks[:, 3].cpu().tolist() == [1] * 7 + [0] * 5            # the decay boundary in mid-table
    opt.norms.fill_(123.0)            # the plan re-zeroes both accumulators
    opt.gsumsq.fill_(1e9)
    worst = {}
    for s in range(R.LAMB_STEPS):
        ps, ms, vs = (_cpu_lists(stub, x) for x in (P.view.view(-1), opt.m, opt.v))
        hp, ref = _lamb_ref(c, ps, grads[s], ms, vs, s + 1)
        G.view.view(-1).copy_(torch.cat(grads[s]).float())
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(opt.hp.cpu(), hp), 'the hyper-parameter row differs from the float64 restatement rounded to fp32'
        assert (ref['gn'] > 1.0) == (label == 'clipped')
        nr = opt.norms.double().cpu().view(-1, 2)
        got = dict(p=_cpu_lists(stub, P.view.view(-1)), m=_cpu_lists(stub, opt.m), v=_cpu_lists(stub, opt.v), u=_cpu_lists(stub, opt.u),
                   norms=[(float(a), float(b)) for a, b in nr])
        for n, x in R.lamb_ratios(got, ref).items():
            worst[n] = max(worst.get(n, 0.0), x)
        gss = sum(float((g * g).sum()) for g in grads[s])
        worst['gsumsq'] = max(worst.get('gsumsq', 0.0), R.gate(float(opt.gsumsq), gss, R.U * R.n_sumsq(stub.flat_state()['total']) * gss))
        if c['wd'] != 0:
            assert s > 0 or ref['trust'][R.LAMB_ZERO_P] == 1.0           # |p| = 0 before the first step only
            assert all(t == 1.0 for t in ref['trust'][R.LAMB_NDECAY:])
            assert any(abs(t - 1.0) > 0.1 for t in ref['trust'][:R.LAMB_NDECAY])
        else:
            assert all(t == 1.0 for t in ref['trust'])
    P.check('params')
    G.check('grads')
    settle('lamb', F32, label, worst)


def test_lamb_stages_raw_and_run_to_run():
    """ga_sumsq_f32 + ga_lamb_stage1 + ga_lamb_stage2 directly, every output guarded, twice on the same inputs: the two runs differ
    by the order of the norm atomics only, so both meet the gate (bit equality is not demanded)"""
    c = R.LAMB_CASES['clipped']
    p0, grads = R.lamb_inputs('clipped')
    g = torch.Generator().manual_seed(4)
    ms = [(torch.randn(n, generator=g) * 0.01).double() for n in R.LAMB_SIZES]
    vs = [(torch.rand(n, generator=g) * 1e-4).double() for n in R.LAMB_SIZES]
    hp, ref = _lamb_ref(c, p0, grads[0], ms, vs, 2)
    rows, off = [], 0
    for tid, n in enumerate(R.LAMB_SIZES):
        for c0 in range(0, n, R.LAMB_CHUNK):
            rows.append((off + c0, min(R.LAMB_CHUNK, n - c0), tid, 1 if tid < R.LAMB_NDECAY else 0))
        off += n
    chunks = torch.tensor(rows, dtype=torch.int32, device='cuda')
    stub = R.FlatStub(R.LAMB_SIZES, R.LAMB_NDECAY, device='cpu')
    G = vec(torch.cat(grads[0]))
    for run in range(2):
        P, M, V, Uu = vec(torch.cat(p0)), vec(torch.cat(ms)), vec(torch.cat(vs)), vec(None, n=off)
        norms, gss = vec(torch.zeros(2 * len(R.LAMB_SIZES))), vec(torch.zeros(1))
        ok(call('ga_sumsq_f32', G, off, gss), 'sumsq')
        ok(call('ga_lamb_stage1', P, G, M, V, Uu, hp.cuda(), gss, chunks, len(rows), norms), 'lamb_stage1')
        torch.cuda.synchronize()
        P.check('p after stage 1', written=False)
        ok(call('ga_lamb_stage2', P, Uu, hp.cuda(), chunks, len(rows), norms), 'lamb_stage2')
        torch.cuda.synchronize()
        for n, x in (('p', P), ('m', M), ('v', V), ('u', Uu), ('norms', norms), ('gsumsq', gss)):
            x.check(n)
        G.check('g', written=False)
        got = {n: [t.double().cpu() for t in stub.split(x.view.view(-1))] for n, x in (('p', P), ('m', M), ('v', V), ('u', Uu))}
        got['norms'] = [(float(a), float(b)) for a, b in norms.inner().double().cpu().view(-1, 2)]
        settle('lamb stages', F32, f'run{run}', R.lamb_ratios(got, ref))
    outs = resnap(P, M, V, Uu, norms)
    h = hp.cuda()
    for a in ((None, G, M, V, Uu, h, gss, chunks, len(rows), norms), (P, G, M, V, None, h, gss, chunks, len(rows), norms),
              (P, G, M, V, Uu, h, None, chunks, len(rows), norms), (P, G, M, V, Uu, h, gss, None, len(rows), norms),
              (P, G, M, V, Uu, h, gss, chunks, 0, norms), (P, G, M, V, Uu, h, gss, chunks, len(rows), None)):
        refused(call('ga_lamb_stage1', *a), 'ga_lamb_stage1', outs)
    for a in ((None, Uu, h, chunks, len(rows), norms), (P, None, h, chunks, len(rows), norms), (P, Uu, None, chunks, len(rows), norms),
              (P, Uu, h, chunks, 0, norms), (P, Uu, h, chunks, len(rows), None)):
        refused(call('ga_lamb_stage2', *a), 'ga_lamb_stage2', outs)


# ----------------------------------------------------------------------------------------------------------------------------
# range updates: step_begin + step_range over a partition + step_end == step, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_range_updates_are_bit_identical_to_step(kind):
    from imagenet_models_amd.optim import FusedAdamW, FusedSGD
    sizes, nd = [5, 300, 1000, 7, 64], 3
    total, n_decay = sum(sizes), 1305
    g = torch.Generator().manual_seed(6)
    p0 = torch.randn(total, generator=g) * 0.05
    grads = [torch.randn(total, generator=g) * 0.01 for _ in range(2)]
    pieces = [(0, 1), (1, 700), (700, 1340), (1340, total)]          # a single element; a piece that straddles n_decay
    assert pieces[2][0] < n_decay < pieces[2][1]

    def make():
        P, G = vec(p0, off=1), vec(torch.zeros(total))
        stub = R.FlatStub(sizes, nd, params=P.view.view(-1), grads=G.view.view(-1))
        assert stub.flat_state()['n_decay'] == n_decay
        opt = (FusedSGD(stub, lr=5e-3, momentum=0.9, weight_decay=0.05, nesterov=True) if kind == 'sgd' else
               FusedAdamW(stub, lr=5e-3, betas=R.BETAS, eps=1e-8, weight_decay=0.05))
        return P, G, opt
    (Pa, Ga, a), (Pb, Gb, b) = make(), make()
    for s, gr in enumerate(grads):
        Ga.view.view(-1).copy_(gr)
        Gb.view.view(-1).copy_(gr)
        a.step()
        b.step_begin()
        for lo, hi in pieces[1:3]:
            b.step_range(lo, hi)
        torch.cuda.synchronize()
        gb = Gb.view.view(-1).cpu()
        assert bool((gb[1:1340] == 0).all()) and torch.equal(gb[:1], gr[:1]) and torch.equal(gb[1340:], gr[1340:]), 'g is zero on exactly the covered ranges'
        for lo, hi in (pieces[0], pieces[3]):
            b.step_range(lo, hi)
        b.step_end()
        torch.cuda.synchronize()
        assert bool((Gb.view.view(-1) == 0).all())
        assert torch.equal(_bits(Pa.inner()), _bits(Pb.inner())), f'{kind} step {s}: parameters differ'
        for n in a.moment_names:
            assert torch.equal(_bits(getattr(a, n)), _bits(getattr(b, n))), f'{kind} step {s}: {n} differs'
        assert not torch.equal(Pa.inner().cpu().view(-1), p0)
    for x in (Pa, Ga, Pb, Gb):
        x.check('flat buffer')


# ----------------------------------------------------------------------------------------------------------------------------
# clipping
# ----------------------------------------------------------------------------------------------------------------------------
S_SS, S_CLIP = 2097152, 1048576


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, S_SS, S_SS + 3, 3 * S_SS + 2])
def test_sumsq(n):
    assert R.STRIDE['sumsq'] == S_SS, 'the sizes no longer enter the stride loop'
    g = torch.Generator(device='cuda').manual_seed(30 + n % 97)
    x = (0.5 + torch.rand(n, generator=g, device='cuda')).double()
    x[-(n & 3 or 1):] = 700.0            # the tail (or the last element) outweighs the rest: a lost or doubled tail element shows
    x[0] = -650.0
    xs = vec(x)
    out = vec(torch.tensor([2.5], dtype=F64))
    ok(call('ga_sumsq_f32', xs, n, out), 'sumsq')
    torch.cuda.synchronize()
    out.check('out')
    xs.check('x', written=False)
    ref, a0 = R.sumsq_ref(x)
    settle('sumsq', F32, f'n{n}', dict(sumsq=R.gate(float(f64(out)[0]) - 2.5, ref, a0 + R.U * (ref + 2.5))))
    resnap(out)
    if n >= 5:
        refused(call('ga_sumsq_f32', xs.view.view(-1)[1:], n - 1, out), 'ga_sumsq_f32', (out,))       # misaligned
    refused(call('ga_sumsq_f32', None, n, out), 'ga_sumsq_f32', (out,))
    refused(call('ga_sumsq_f32', xs, 0, out), 'ga_sumsq_f32', (out,))
    assert call('ga_sumsq_f32', xs, n, None) == BAD_ARG


@pytest.mark.parametrize('n', [7, S_CLIP, S_CLIP + 1, 2 * S_CLIP + 5])
def test_clip_norm_and_value(n):
    assert R.STRIDE['clip'] == S_CLIP, 'the sizes no longer enter the stride loop'
    g = torch.Generator(device='cuda').manual_seed(31)
    x = (torch.randn(n, generator=g, device='cuda') * (1e-4 if n == 7 else 1.0)).double()
    nrm = math.sqrt(float((x * x).sum()))
    ss = torch.tensor([float((x * x).sum())], dtype=F64).float().cuda()
    worst = {}
    for name, limit in (('clipping', 0.5 * nrm), ('not clipping', 10 * nrm), ('at the norm', float(torch.tensor(nrm, dtype=F32)))):
        G = vec(x, off=1)
        ok(call('ga_clip_grad_f32', G, n, ss, limit, 0), 'clip norm')
        torch.cuda.synchronize()
        G.check(name)
        ref, a0, coef = R.clip_norm_ref(x, limit)
        worst[name] = R.gate(f64(G), ref, a0)
        if name == 'not clipping':
            assert coef == 1.0 and torch.equal(_bits(G.flat), G.before), 'an unclipped gradient keeps its bits'
        elif name == 'clipping':
            assert coef < 1.0
    settle('clip norm', F32, f'n{n}', worst)
    G = vec(x, off=1)
    lim = 0.3 * (1e-4 if n == 7 else 1.0)
    ok(call('ga_clip_grad_f32', G, n, None, lim, 1), 'clip value')
    torch.cuda.synchronize()
    G.check('clip value')
    l32 = float(torch.tensor(lim, dtype=F32))
    assert torch.equal(G.inner().view(-1), x.float().clamp(-l32, l32)), 'clip value is not clamp, bit for bit'
    before = _bits(G.flat).clone()
    for a in ((None, n, ss, 1.0, 0), (G, 0, ss, 1.0, 0), (G, n, ss, 0.0, 0), (G, n, ss, -1.0, 1), (G, n, None, 1.0, 0), (G, n, ss, 1.0, 2)):
        assert call('ga_clip_grad_f32', *a) == BAD_ARG and 'ga_clip_grad_f32' in _L().last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(G.flat), before)


@pytest.mark.parametrize('lengths,nunits', [([65], 1), ([4097, 65, 64, 63], 4), ([1, 63, 64, 65, 4097], 5)], ids=['1unit', '4units', '5units'])
def test_agc(lengths, nunits):
    p, g, units = R.agc_inputs(lengths, nunits)
    ref, a0, flags = R.agc_ref(p, g, units, 0.02)
    P, G = vec(p), vec(g)
    tab = torch.tensor(units, dtype=I64, device='cuda')
    ok(call('ga_agc_clip', P, G, tab, nunits, 0.02, 1e-3), 'agc_clip')
    torch.cuda.synchronize()
    G.check('g')
    P.check('p', written=False)
    got = f64(G).cpu()
    if nunits >= 4:
        assert flags[:4] == [0, 2, 1, 2], flags         # unclipped, clipped, at the threshold, |p| < eps
    for (off, ln), f in zip(units, flags):
        if f == 0:
            assert torch.equal(got[off:off + ln], g[off:off + ln]), 'an unclipped unit keeps its bits'
    settle('agc', F32, f'{nunits} units', dict(g=R.gate(got, ref, a0)))
    outs = resnap(G)
    for a in ((None, G, tab, nunits, 0.02, 1e-3), (P, None, tab, nunits, 0.02, 1e-3), (P, G, None, nunits, 0.02, 1e-3), (P, G, tab, 0, 0.02, 1e-3),
              (P, G, tab, nunits, 0.0, 1e-3)):
        refused(call('ga_agc_clip', *a), 'ga_agc_clip', outs)


# ----------------------------------------------------------------------------------------------------------------------------
# samplers
# ----------------------------------------------------------------------------------------------------------------------------
S_DROP = 524288
SEED = 0x9E3779B97F4A7C15 ^ 1234567


@pytest.mark.parametrize('n', [1, 257, S_DROP, S_DROP + 1, 2 * S_DROP + 7])
def test_dropout_mask_sample(n):
    assert R.STRIDE['dropout_mask'] == S_DROP, 'the sizes no longer enter the stride loop'
    ctr = torch.tensor([5], dtype=I64, device='cuda')
    for j, keep in enumerate((1.0, 0.9, 0.5)):
        out = vec(None, n=n, off=1)
        ok(call('ga_dropout_mask_sample', out, n, keep, C.c_uint64(SEED), ctr), 'dropout_mask_sample')
        torch.cuda.synchronize()
        out.check('mask')
        assert int(ctr) == 6 + j, 'the counter advances by exactly one per call'
        want = torch.from_numpy(R.dropout_mask_ref(n, keep, SEED, 5 + j))
        assert torch.equal(_bits(out.inner().view(-1).cpu()), _bits(want)), f'n {n} keep {keep}: the mask is not the documented generator\'s'
    # a recorded plan, replayed: one counter step per replay
    ops = _ops()
    out = vec(None, n=n)
    pl = ops.Plan(name='dropout-mask')
    pl.dropout_mask_sample(out.view.view(-1), n, 0.5, SEED, ctr)
    for j in range(2):
        pl.run()
        torch.cuda.synchronize()
        assert int(ctr) == 9 + j
        assert torch.equal(out.inner().view(-1).cpu(), torch.from_numpy(R.dropout_mask_ref(n, 0.5, SEED, 8 + j)))
    out.check('mask (plan)')
    resnap(out)
    for a in ((None, n, 0.5, C.c_uint64(SEED), ctr), (out, 0, 0.5, C.c_uint64(SEED), ctr), (out, n, 0.0, C.c_uint64(SEED), ctr),
              (out, n, 1.5, C.c_uint64(SEED), ctr), (out, n, 0.5, C.c_uint64(SEED), None)):
        refused(call('ga_dropout_mask_sample', *a), 'ga_dropout_mask_sample', (out,))
    assert int(ctr) == 10


@pytest.mark.parametrize('sites,B', [(1, 1), (2, 512), (5, 205), (7, 4096)])
def test_drop_path_sample(sites, B):
    assert sites * B in (1, 1024, 1025, 7 * 4096)
    keep = torch.linspace(0.5, 1.0, sites) if sites > 1 else torch.tensor([0.5])
    kd = keep.cuda()
    ctr = torch.tensor([41], dtype=I64, device='cuda')
    out = Guarded(sites, B, B, F32, guard=64, off=1)
    for j in range(2):
        ok(call('ga_drop_path_sample', out, kd, sites, B, C.c_uint64(SEED), ctr), 'drop_path_sample')
        torch.cuda.synchronize()
        out.check('mask')
        assert int(ctr) == 42 + j
        assert torch.equal(_bits(out.inner().cpu()), _bits(torch.from_numpy(R.drop_path_ref(keep.numpy(), sites, B, SEED, 41 + j))))
    pl = _ops().Plan(name='drop-path')
    pl.drop_path_sample(out.view, kd, sites, B, SEED, ctr)
    for j in range(2):
        pl.run()
        torch.cuda.synchronize()
        assert int(ctr) == 44 + j
        assert torch.equal(out.inner().cpu(), torch.from_numpy(R.drop_path_ref(keep.numpy(), sites, B, SEED, 43 + j)))
    out.check('mask (plan)')
    resnap(out)
    for a in ((None, kd, sites, B, C.c_uint64(SEED), ctr), (out, None, sites, B, C.c_uint64(SEED), ctr), (out, kd, 0, B, C.c_uint64(SEED), ctr),
              (out, kd, sites, 0, C.c_uint64(SEED), ctr), (out, kd, sites, B, C.c_uint64(SEED), None)):
        refused(call('ga_drop_path_sample', *a), 'ga_drop_path_sample', (out,))
    assert int(ctr) == 45


# ----------------------------------------------------------------------------------------------------------------------------
# the grid stride of the two input kernels
# ----------------------------------------------------------------------------------------------------------------------------
def test_mixup_batch_grid_stride():
    B, CH, H, W = 4, 3, 448, 448
    n = B * CH * H * W
    assert n > R.STRIDE['mixup_batch'] == 2097152, 'the size no longer enters the stride loop'
    x = torch.randn(B, CH, H, W, generator=torch.Generator().manual_seed(12))
    xs = vec(x)
    lam = 0.37
    out = vec(None, n=n)
    ok(call('ga_mixup_batch', xs, out, B, CH, H, W, lam, 0, 0, 0, 0, 0), 'mixup')
    torch.cuda.synchronize()
    out.check('mixup')
    want = x.clone().mul_(lam).add_(x.flip(0).mul_(1.0 - lam))
    assert torch.equal(out.inner().view(B, CH, H, W).cpu(), want)
    for yl, yh, xl, xh in ((300, H, 200, W), (100, 100, 50, 200)):          # touches the last row and column; empty
        out = vec(None, n=n)
        ok(call('ga_mixup_batch', xs, out, B, CH, H, W, lam, 1, yl, yh, xl, xh), 'cutmix')
        torch.cuda.synchronize()
        out.check('cutmix')
        want = x.clone()
        want[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        assert torch.equal(out.inner().view(B, CH, H, W).cpu(), want)
        assert (yl == yh) == torch.equal(want, x)
    xs.check('x', written=False)
    resnap(out)
    for a in ((None, out, B, CH, H, W, lam, 0, 0, 0, 0, 0), (xs, None, B, CH, H, W, lam, 0, 0, 0, 0, 0), (xs, xs, B, CH, H, W, lam, 0, 0, 0, 0, 0),
              (xs, out, 0, CH, H, W, lam, 0, 0, 0, 0, 0), (xs, out, B, CH, H, W, lam, 1, 0, H + 1, 0, 1), (xs, out, B, CH, H, W, lam, 1, 5, 4, 0, 1)):
        refused(call('ga_mixup_batch', *a), 'ga_mixup_batch', (out, xs))


def test_u8_normalize_grid_stride():
    B, CH, H, W = 16, 3, 448, 448
    n = B * CH * H * W
    assert n > R.STRIDE['u8_normalize'] == 8388608, 'the size no longer enters the stride loop'
    x8 = torch.randint(0, 256, (B, CH, H, W), generator=torch.Generator().manual_seed(13), dtype=torch.uint8)
    mean = [0.485 * 255, 0.456 * 255, 0.406 * 255]
    std = [0.229 * 255, 0.224 * 255, 0.225 * 255]
    xd = x8.cuda()
    out = vec(None, n=n)
    arr = lambda v: (C.c_float * 3)(*v)
    ok(call('ga_u8_normalize', xd, out, B, CH, H, W, arr(mean), arr(std)), 'u8_normalize')
    torch.cuda.synchronize()
    out.check('normalised')
    want = xd.float().sub_(torch.tensor(mean, device='cuda').view(1, 3, 1, 1)).div_(torch.tensor(std, device='cuda').view(1, 3, 1, 1))
    assert torch.equal(out.inner().view(B, CH, H, W), want)
    assert torch.equal(want[:, :, ::64, ::64].cpu(), x8[:, :, ::64, ::64].float().sub_(torch.tensor(mean).view(1, 3, 1, 1)).div_(torch.tensor(std).view(1, 3, 1, 1)))
    resnap(out)
    for a in ((None, out, B, CH, H, W, arr(mean), arr(std)), (xd, out, 0, CH, H, W, arr(mean), arr(std)), (xd, out, B, 5, H, W, arr(mean), arr(std)),
              (xd, out, B, CH, 1, 3, arr(mean), arr(std)), (xd, out.view.view(-1)[1:], B, CH, H, W, arr(mean), arr(std))):
        refused(call('ga_u8_normalize', *a), 'ga_u8_normalize', (out,))
