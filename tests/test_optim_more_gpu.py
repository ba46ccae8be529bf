"""The Adam, RMSprop / RMSpropTF, Lion and LARS steps of csrc/loss_optim.hip on the device, against the float64 steps of
tests/_optim_more_ref.py within their derived rounding bounds (tests/test_optim_more_cpu.py proves that fp32 arithmetic in the
kernels' order meets them and that the named wrong restatements do not), through the C ABI with every buffer in a NaN-filled guarded
allocation, and through the optimizer classes, TrainStep and train.py.

The flat kernels run at n = 1, 255, 256, 257, S, S + 1 and S + 8192 * 256 + 3 (S = 8192 * 256, their grid-stride span: the last
size makes three trips), three steps each from the state the kernel itself left, with both wd_mult values, with p = 0 and g = 0
elements in every step and a second step whose gradient is all zero.  LARS runs over LAMB's tensor sizes (one to three chunks per
tensor, six tensors decayed) in its four nesterov x trust_clip forms, with a tensor whose parameters are zero, one whose gradient
is zero, every gradient zero, weight_decay 0 and without momentum.  Every case prints its worst err / allowed (run with -s)."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _optim_more_ref as M
from _optim_more_ref import F32, F64
from _guarded import Guarded, _bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
S_OPT = 2097152
FLAT_N = [1, 255, 256, 257, S_OPT, S_OPT + 1, S_OPT + 8192 * 256 + 3]


def _L():
    from imagenet_models_amd import _lib
    return _lib


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


def vec(data, off=0, n=None):
    """a guarded flat fp32 vector; `off` shifts it off 16-byte alignment"""
    n = data.numel() if data is not None else n
    return Guarded(1, n, n, F32, data=None if data is None else data.reshape(1, -1), off=off, guard=64)


def f64(g):
    return (g.inner() if isinstance(g, Guarded) else g).reshape(-1).double()


def settle(kernel, label, ratios):
    print(f'[{kernel} {label}] ' + '  '.join(f'{n} {v:.3f}' for n, v in ratios.items()))
    bad = {n: v for n, v in ratios.items() if not v <= 1.0}
    assert not bad, f'{kernel} {label}: err / allowed {bad}'


def refused(rc, fn, outs):
    assert rc == BAD_ARG, rc
    assert fn in _L().last_error(), (fn, _L().last_error())
    torch.cuda.synchronize()
    for g in outs:
        g.check('refused', written=False)


def resnap(*gs):
    torch.cuda.synchronize()
    for g in gs:
        g.before = _bits(g.flat).clone()
    return gs


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a test that leaves the device in error ends the session: nothing more is launched on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def _worse(worst, name, got, ref, allowed):
    worst[name] = max(worst.get(name, 0.0), M.gate(f64(got), ref, allowed))


def _sizes_enter_the_stride_loop(kind):
    assert M.STRIDE[kind] == S_OPT and math.ceil(FLAT_N[-1] / S_OPT) == 3, 'the sizes no longer enter the stride loop'


# ----------------------------------------------------------------------------------------------------------------------------
# (a) the flat element-wise kernels
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', FLAT_N)
def test_flat_adam(n):
    _sizes_enter_the_stride_loop('adam')
    p0, grads = M.flat_inputs(n, 51, 'cuda')
    for mult in (1.0, 0.0):
        p, m, v = vec(p0, off=3), vec(torch.zeros(n), off=1), vec(torch.zeros(n), off=2)
        worst = {}
        for s, g64 in enumerate(grads):
            hp = M.hp_row('adam', M.LR, M.WD, *M.BETAS, eps=1e-8, t=s + 1)
            h = [float(x) for x in hp]
            g = vec(g64, off=3)
            (rp,), (rm,), (rv,), (al,) = M.adam_step([f64(p)], [g64], [f64(m)], [f64(v)], [mult != 0], h[0], h[1], h[2], h[3], h[4], bc1=h[5], bc2=h[6])
            ok(call('ga_adam_step', p, g, m, v, hp.cuda(), n, mult), 'adam_step')
            torch.cuda.synchronize()
            for name, gd in (('p', p), ('m', m), ('v', v)):
                gd.check(name)
            g.check('g', written=False)
            for name, got, ref in (('p', p, rp), ('m', m, rm), ('v', v, rv)):
                _worse(worst, name, got, ref, al[name])
        assert mult != 0.0 or not bool(f64(m)[5::11].any())          # g = 0 in every step, no decay: the moments stay exactly zero there
        settle('adam', f'n{n}-wd{mult:.0f}', worst)


@pytest.mark.parametrize('tf', [False, True], ids=['torch', 'tf'])
@pytest.mark.parametrize('n', FLAT_N)
def test_flat_rmsprop(n, tf):
    _sizes_enter_the_stride_loop('rmsprop')
    p0, grads = M.flat_inputs(n, 52, 'cuda')
    combos = [(0.0, 1.0), (0.9, 0.0)] if n > 4096 else [(0.0, 1.0), (0.0, 0.0), (0.9, 1.0), (0.9, 0.0)]
    for mu, mult in combos:
        p, sq = vec(p0, off=3), vec(torch.full((n,), 1.0 if tf else 0.0), off=1)
        buf = vec(torch.zeros(n), off=2) if mu else None
        worst = {}
        for s, g64 in enumerate(grads):
            hp = M.hp_row('rmsprop', M.LR, M.WD, mu=mu, alpha=M.RMS_ALPHA, eps=M.RMSTF_EPS if tf else M.RMS_EPS)
            h = [float(x) for x in hp]
            g = vec(g64, off=3)
            (rp,), (rs,), rb, (al,) = M.rmsprop_step([f64(p)], [g64], [f64(sq)], None if buf is None else [f64(buf)], [mult != 0],
                                                     h[0], h[1], h[2], h[3], h[4], tf=tf)
            ok(call('ga_rmsprop_step', p, g, sq, buf, hp.cuda(), n, int(tf), mult), 'rmsprop_step')
            torch.cuda.synchronize()
            for name, gd, ref in (('p', p, rp), ('sq', sq, rs)) + ((('buf', buf, rb[0]),) if buf is not None else ()):
                gd.check(name)
                _worse(worst, name, gd, ref, al[name])
            g.check('g', written=False)
        settle('rmsprop', f'n{n}-tf{int(tf)}-mu{mu}-wd{mult:.0f}', worst)


@pytest.mark.parametrize('n', FLAT_N)
def test_flat_lion(n):
    _sizes_enter_the_stride_loop('lion')
    p0, grads = M.flat_inputs(n, 53, 'cuda')
    for mult in (1.0, 0.0):
        p, m = vec(p0, off=3), vec(grads[2] * 0.5, off=1)          # a momentum that is not zero: sign(c) is not sign(g)
        worst, undetermined, moved = {}, 0, 0
        for g64 in grads:
            hp = M.hp_row('lion', M.LR, M.WD, *M.LION_BETAS)
            h = [float(x) for x in hp]
            g = vec(g64, off=3)
            before = f64(p).clone()
            (rp,), (rm,), (al,), (und,) = M.lion_step([before], [g64], [f64(m)], [mult != 0], h[0], h[1], h[2], h[3])
            ok(call('ga_lion_step', p, g, m, hp.cuda(), n, mult), 'lion_step')
            torch.cuda.synchronize()
            p.check('p')
            m.check('m')
            g.check('g', written=False)
            _worse(worst, 'p', p, rp, al['p'])
            _worse(worst, 'm', m, rm, al['m'])
            undetermined += int(und.sum())
            if mult == 0.0:          # no decay: every element moved by exactly lr or not at all
                d = (f64(p) - before).abs()
                assert bool(((d == 0) | ((d - h[0]).abs() <= 2 * M.U * (before.abs() + h[0]))).all())
                moved += int((d > 0).sum())
        # the 2 lr allowance is for the few elements whose float64 |c| lies within its own rounding of zero: about 3 U of them
        assert undetermined <= max(2, 3 * n * 12 * M.U), undetermined
        assert mult != 0.0 or n < 4 or moved > n
        settle('lion', f'n{n}-wd{mult:.0f} ({undetermined} undetermined signs)', worst)


# ----------------------------------------------------------------------------------------------------------------------------
# (b) LARS
# ----------------------------------------------------------------------------------------------------------------------------
def _cpu_lists(stub, flat):
    return [t.double().cpu() for t in stub.split(flat)]


def _lars_run(label, nesterov, clip, mu):
    from imagenet_models_amd.optim import FusedLars
    c = M.LARS_CASES[label]
    p0, grads = M.lars_inputs(label)
    decay = M.R.decay_flags(M.LARS_SIZES, M.LARS_NDECAY)
    P, G = vec(torch.cat(p0)), vec(None, n=sum(M.LARS_SIZES))
    stub = M.FlatStub(M.LARS_SIZES, M.LARS_NDECAY, params=P.view.view(-1), grads=G.view.view(-1))
    opt = FusedLars(stub, lr=M.LR, momentum=mu, weight_decay=c['wd'], nesterov=nesterov, trust_coeff=M.LARS_TC, eps=M.LARS_EPS, trust_clip=clip)
    assert opt.CHUNK == M.LAMB_CHUNK and opt.chunks.shape[0] == sum(math.ceil(n / M.LAMB_CHUNK) for n in M.LARS_SIZES)
    assert opt.chunks[:, 3].cpu().tolist() == [1] * 7 + [0] * 5            # the decay boundary in mid-table
    assert (opt.buf is None) == (mu == 0)
    opt.norms.fill_(123.0)            # the plan re-zeroes the accumulators
    if opt.buf is not None:
        opt.buf.fill_(3.0)            # a stale buffer: the first step must not read it
    worst, trusts = {}, []
    for s in range(M.STEPS):
        ps = _cpu_lists(stub, P.view.view(-1))
        bufs = None if opt.buf is None else _cpu_lists(stub, opt.buf)
        hp = M.hp_row('lars', M.LR, c['wd'], mu=mu, trust_coeff=M.LARS_TC, eps=M.LARS_EPS, first=s == 0)
        h = [float(x) for x in hp]
        ref = M.lars_step(ps, grads[s], bufs, decay, h[0], h[1], h[2], h[3], h[4], nesterov, clip, first=s == 0)
        G.view.view(-1).copy_(torch.cat(grads[s]).float())
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(opt.hp.cpu(), hp), 'the hyper-parameter row differs from the float64 restatement rounded to fp32'
        got = dict(p=_cpu_lists(stub, P.view.view(-1)), buf=None if opt.buf is None else _cpu_lists(stub, opt.buf),
                   norms=[(float(a), float(b)) for a, b in opt.norms.double().cpu().view(-1, 2)])
        for n, x in M.lars_ratios(got, ref).items():
            worst[n] = max(worst.get(n, 0.0), x)
        trusts.append(ref['trust'])
    P.check('params')
    G.check('grads')
    assert opt.steps == M.STEPS
    return worst, trusts


@pytest.mark.parametrize('nesterov,clip', M.LARS_FORMS, ids=['lars', 'nlars', 'larc', 'nlarc'])
@pytest.mark.parametrize('label', list(M.LARS_CASES))
def test_fused_lars(label, nesterov, clip):
    worst, trusts = _lars_run(label, nesterov, clip, 0.9)
    t = trusts[0]
    assert all(x == 1.0 for x in t[M.LARS_NDECAY:]) and t[M.LARS_ZERO_P] == 1.0 and t[M.LARS_ZERO_G] == 1.0      # |p| = 0, |g| = 0
    if label == 'decay':
        live = [x for i, x in enumerate(t[:M.LARS_NDECAY]) if i not in (M.LARS_ZERO_P, M.LARS_ZERO_G)]
        # trust_coeff w / (q + w wd + eps) < trust_coeff / wd = 0.02
        assert all(x < M.LARS_TC / M.LARS_CASES[label]['wd'] for x in live) if not clip else (any(x == 1.0 for x in live) and any(x < 0.9 for x in live)), live
    elif label == 'wd0':
        assert all(x == 1.0 for x in t)
    settle('lars', f'{label}-nesterov{int(nesterov)}-clip{int(clip)}', worst)


def test_fused_lars_without_momentum():
    worst, _ = _lars_run('decay', False, True, 0.0)
    assert set(worst) == {'p', 'norms'}
    settle('lars', 'decay-larc-mu0', worst)


# ----------------------------------------------------------------------------------------------------------------------------
# (c) range updates: step_begin + step_range over a partition + step_end == step, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'rmsproptf', 'lion'])
def test_range_updates_are_bit_identical_to_step(kind):
    import imagenet_models_amd as A
    sizes, nd = [5, 300, 1000, 7, 64], 3
    total, n_decay = sum(sizes), 1305
    g = torch.Generator().manual_seed(6)
    p0 = torch.randn(total, generator=g) * 0.05
    grads = [torch.randn(total, generator=g) * 0.01 for _ in range(2)]
    pieces = [(0, 1), (1, 700), (700, 1340), (1340, total)]          # a single element; a piece that straddles n_decay
    assert pieces[2][0] < n_decay < pieces[2][1]

    def make():
        P, G = vec(p0, off=1), vec(torch.zeros(total))
        stub = M.FlatStub(sizes, nd, params=P.view.view(-1), grads=G.view.view(-1))
        assert stub.flat_state()['n_decay'] == n_decay
        opt = A.create_optimizer_v2(stub, opt=kind, lr=5e-3, weight_decay=0.05, momentum=0.9)
        assert opt.supports_ranges and opt.kind == kind
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
        assert not torch.equal(Pa.inner().cpu().view(-1), p0) and a.steps == b.steps == s + 1
    for x in (Pa, Ga, Pb, Gb):
        x.check('flat buffer')


# ----------------------------------------------------------------------------------------------------------------------------
# (d) bad arguments are refused before any launch
# ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    p, g, m, v = (vec(torch.ones(8)) for _ in range(4))
    hp = M.hp_row('adam', M.LR, M.WD, *M.BETAS, eps=1e-8, t=1).cuda()
    outs = (p, m, v)
    for a in ((None, g, m, v, hp, 8), (p, None, m, v, hp, 8), (p, g, None, v, hp, 8), (p, g, m, None, hp, 8), (p, g, m, v, None, 8), (p, g, m, v, hp, 0),
              (p, g, m, v, hp, -3)):
        refused(call('ga_adam_step', *a, 1.0), 'ga_adam_step', outs)
    for a in ((None, g, m, v, hp, 8, 0), (p, None, m, v, hp, 8, 1), (p, g, None, v, hp, 8, 0), (p, g, m, v, None, 8, 1), (p, g, m, v, hp, 0, 0),
              (p, g, m, v, hp, 8, 2), (p, g, m, None, hp, 8, -1)):
        refused(call('ga_rmsprop_step', *a, 1.0), 'ga_rmsprop_step', outs)
    for a in ((None, g, m, hp, 8), (p, None, m, hp, 8), (p, g, None, hp, 8), (p, g, m, None, 8), (p, g, m, hp, 0)):
        refused(call('ga_lion_step', *a, 1.0), 'ga_lion_step', outs)
    chunks = torch.tensor([[0, 8, 0, 1]], dtype=torch.int32, device='cuda')
    norms = vec(torch.zeros(2))
    outs = (p, m, norms)
    for a in ((None, g, chunks, 1, norms), (p, None, chunks, 1, norms), (p, g, None, 1, norms), (p, g, chunks, 0, norms), (p, g, chunks, 1, None)):
        refused(call('ga_lars_stage1', *a), 'ga_lars_stage1', outs)
    for a in ((None, g, m, hp, chunks, 1, norms), (p, None, m, hp, chunks, 1, norms), (p, g, m, None, chunks, 1, norms), (p, g, m, hp, None, 1, norms),
              (p, g, m, hp, chunks, 0, norms), (p, g, m, hp, chunks, 1, None)):
        refused(call('ga_lars_stage2', *a, 1, 1), 'ga_lars_stage2', outs)


# ----------------------------------------------------------------------------------------------------------------------------
# (e) the command line, and resuming
# ----------------------------------------------------------------------------------------------------------------------------
MODEL = 'mobilenet_v1'          # the smallest registered model (4.2 M parameters), and the one RMSpropTF with step decay is the recipe of


def _cli(args, timeout=600):
    r = subprocess.run([sys.executable, 'train.py', '--synthetic', '--model', MODEL, '-b', '4', '--steps-per-epoch', '2', '--log-interval', '1',
                        '--mixup', '0', '--cutmix', '0'] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout + r.stderr


@pytest.mark.parametrize('name,lr', [('adam', '1e-3'), ('rmsprop', '1e-3'), ('rmsproptf', '1e-3'), ('lion', '1e-4'), ('lars', '0.05'), ('nlars', '0.05'),
                                     ('larc', '0.05'), ('nlarc', '0.05')])
def test_train_cli_runs_two_steps(name, lr):
    out = _cli(['--epochs', '1', '--opt', name, '--lr', lr, '--weight-decay', '1e-4', '--sched', 'step', '--decay-epochs', '1', '--warmup-epochs', '0'])
    assert '*** epoch 0: train loss' in out and 'nan' not in out.lower()


def test_rmsproptf_resumes_from_the_command_line(tmp_path):
    import imagenet_models_amd as A
    D = os.path.join(tmp_path, 'out')
    flags = ['--opt', 'rmsproptf', '--opt-eps', '0.001', '--lr', '1e-3', '--weight-decay', '1e-5', '--sched', 'step', '--decay-epochs', '1',
             '--decay-rate', '0.5', '--warmup-epochs', '0']
    out = _cli(flags + ['--epochs', '1', '--output', D])
    assert '*** epoch 0: train loss' in out
    ck = A.read_checkpoint(os.path.join(D, 'last.pth.tar'))
    o = ck['optimizer']
    assert o['kind'] == 'rmsproptf' and o['steps'] == 2 and list(o) == ['kind', 'steps', 'sq', 'buf', 'param_groups'] and o['param_groups'][0]['lr'] == 1e-3
    assert float(o['sq'].min()) > 0.5 and bool((o['sq'] != 1).any()) and bool(o['buf'].any())          # started at one, moved by two steps
    D2 = os.path.join(tmp_path, 'out2')
    out = _cli(flags + ['--epochs', '2', '--resume', os.path.join(D, 'last.pth.tar'), '--output', D2])
    mt = re.search(r'Resumed \S+: starting at epoch (\d+), batch (\d+) of 2, lr (\S+)', out)
    assert mt and (int(mt.group(1)), int(mt.group(2))) == (1, 0), out[-1500:]
    assert float(mt.group(3)) == pytest.approx(5e-4, rel=1e-6)          # the step schedule at epoch 1, set by the unchanged resume path
    assert '*** epoch 1: train loss' in out and 'Train: 0 [' not in out and 'nan' not in out.lower()
    o2 = A.read_checkpoint(os.path.join(D2, 'last.pth.tar'))['optimizer']
    assert o2['steps'] == 4 and o2['param_groups'][0]['lr'] == 5e-4 and not torch.equal(o2['sq'], o['sq'])


def test_rmsproptf_next_step_after_resume_equals_the_uninterrupted_runs(tmp_path):
    """two training steps (the optimizer behind backward, by ranges), save, rebuild from the file: the restored state is the saved
    state bit for bit, and the next optimizer step from one and the same gradient leaves both runs with the same bits -- parameters,
    square average, momentum buffer and hyper-parameter row.  (The gradient is given, not recomputed: the trunk's own run-to-run
    spread, tests/test_resume_gpu.py, is not what this test is about.)"""
    import imagenet_models_amd as A

    def build():
        m = A.create_model(MODEL, num_classes=16).cuda().train()
        o = A.create_optimizer_v2(m, opt='rmsproptf', lr=1e-3, weight_decay=1e-5, momentum=0.9, eps=1e-3)
        return m, o, A.TrainStep(m, o, 4, overlap_optimizer=True)
    torch.manual_seed(11)
    m, o, step = build()
    assert step.overlap_opt
    gen = torch.Generator().manual_seed(12)
    for _ in range(2):
        step(torch.randn(4, 3, 224, 224, generator=gen).cuda(), torch.randint(0, 16, (4,), generator=gen).cuda())
    torch.cuda.synchronize()
    assert o.steps == 2 and bool((o.sq != 1).any()) and bool(o.buf.any())
    path = os.path.join(tmp_path, 'k2.pth.tar')
    A.save_checkpoint(m, o, 0, path, arch=MODEL, train_state=A.capture_train_state(step))
    ck = A.read_checkpoint(path)
    torch.manual_seed(A.saved_initial_seed(ck['train_state']))
    m2, o2, step2 = build()
    assert bool((o2.sq == 1).all()) and o2.steps == 0
    A.resume_checkpoint(ck, m2, o2, None, step2)
    assert o2.steps == 2 and o2.param_groups == o.param_groups
    for a, b in ((o.sq, o2.sq), (o.buf, o2.buf), (o.p, o2.p)):
        assert torch.equal(_bits(a), _bits(b))
    g = torch.randn(o.total, generator=gen).cuda() * 0.01
    before = o.p.clone()
    for x in (o, o2):
        x.g.copy_(g)
        x.step()
    torch.cuda.synchronize()
    for a, b in ((o.sq, o2.sq), (o.buf, o2.buf), (o.p, o2.p), (o.hp, o2.hp)):
        assert torch.equal(_bits(a), _bits(b))
    assert o.steps == o2.steps == 3 and not torch.equal(o.p, before)
