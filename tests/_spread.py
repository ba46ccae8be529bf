"""Run-to-run spread of an fp32 train step under two launch schedules (test infrastructure).

The engines spread a step over several streams: the asynchronous weight-gradient lane (GAEXT_ASYNC_WGRAD), the MAP head lanes
(GAEXT_HEAD_STREAMS), the forward split into batch chains (GAEXT_FWD_SPLIT) and the parallel stage-4 shortcut (GAEXT_PAR_BRANCH).
SERIAL sets every one of them to a single lane; the engines read these switches when they are built, so a test sets them (pytest's
monkeypatch) before it builds the model.  Comparing two runs inside one schedule and across the two tells a race between lanes
(the default schedule spreads far more than the serial one) from order-dependent arithmetic that no lane causes (both spread alike).

The BatchNorm batch sums (s = sum x, q = sum x^2 per channel, accumulated by the GEMM epilogues into the engine's bn_pool) are
recorded per BatchNorm, so that the first BatchNorm whose sums differ between two runs can be named."""
import torch

SERIAL = {'GAEXT_ASYNC_WGRAD': '0', 'GAEXT_HEAD_STREAMS': '1', 'GAEXT_FWD_SPLIT': '1', 'GAEXT_PAR_BRANCH': '0'}


def set_schedule(monkeypatch, serial):
    for k in SERIAL:
        monkeypatch.delenv(k, raising=False)         # the default schedule: the switches as they ship
    if serial:
        for k, v in SERIAL.items():
            monkeypatch.setenv(k, v)


def record_bn_sums(monkeypatch):
    """every engine built after this call keeps [(BatchNorm prefix, its s / q pool slices)] in creation order (= forward order)"""
    from imagenet_models_amd.engine_base import EngineBase
    orig = EngineBase._bn_bufs

    def rec(self, pre, C, zero=False):
        d = orig(self, pre, C, zero=zero)
        if not hasattr(self, '_bn_record'):
            self._bn_record = []
        self._bn_record.append((pre, d))
        return d
    monkeypatch.setattr(EngineBase, '_bn_bufs', rec)


def bn_sums(model):
    """[(prefix, s, q)] of the training engine of `model` (CPU copies), after its step"""
    eng = [e for e in model._engines.values() if e.training]
    assert len(eng) == 1
    torch.cuda.synchronize()
    return [(pre, d['s'].detach().cpu().clone(), d['q'].detach().cpu().clone()) for pre, d in eng[0]._bn_record]


def grad_spread(g1, g2):
    """{name: ||g1 - g2|| / max(||g2||, 1e-3 x the largest norm)}: the measure of the run-to-run tests (analytically zero
    gradients -- biases before a softmax or a train-mode BatchNorm -- hold round-off only)"""
    gmax = max(float(g.double().norm()) for g in g2.values())
    return {n: float((g1[n] - g2[n]).double().norm()) / max(float(g2[n].double().norm()), 1e-3 * gmax) for n in g1}


def first_bn_difference(a, b):
    """the first BatchNorm (forward order) whose batch sums differ between two recordings: (index, prefix, max relative difference
    of s, of q), or None"""
    for i, ((pre, s1, q1), (pre2, s2, q2)) in enumerate(zip(a, b)):
        assert pre == pre2
        if not (torch.equal(s1, s2) and torch.equal(q1, q2)):
            es = float((s1 - s2).abs().max() / (s2.abs().max() + 1e-30))
            eq = float((q1 - q2).abs().max() / (q2.abs().max() + 1e-30))
            return i, pre, es, eq
    return None


def worst(errs):
    return max(errs.items(), key=lambda kv: kv[1])


def median(errs):
    v = sorted(errs.values())
    return v[len(v) // 2]


def measure(monkeypatch, tag, step, runs=2):
    """step() -> (loss, {name: grad}, model), run `runs` times under the serial and under the default schedule.  Prints the spread
    inside each schedule and between them and the first BatchNorm whose sums differ between two serial runs.
    Returns {'serial': worst spread, 'default': ..., 'between': ..., 'bn': first_bn_difference of the serial runs}"""
    record_bn_sums(monkeypatch)
    res = {}
    for sched in ('serial', 'default'):
        set_schedule(monkeypatch, sched == 'serial')
        res[sched] = []
        for _ in range(runs):
            loss, grads, m = step()
            res[sched].append((float(loss), grads, bn_sums(m)))
            del m
            torch.cuda.empty_cache()
    set_schedule(monkeypatch, False)
    out = {}
    for sched in ('serial', 'default'):
        (l1, g1, b1), (l2, g2, b2) = res[sched][:2]
        e = grad_spread(g1, g2)
        out[sched] = worst(e)[1]
        d = first_bn_difference(b1, b2)
        print(f'[{tag} fp32] {sched} vs {sched}: loss {abs(l1 - l2):.2e}, worst gradient {worst(e)}, median {median(e):.2e}; '
              f'BatchNorm sums: ' + ('all bitwise equal' if d is None else
                                     f'first difference at BatchNorm #{d[0]} {d[1]!r}: s {d[2]:.2e}, q {d[3]:.2e} (max relative)'))
        if sched == 'serial':
            out['bn'] = d
    eb = [worst(grad_spread(res['default'][i][1], res['serial'][j][1]))[1] for i in range(runs) for j in range(runs)]
    e = grad_spread(res['default'][0][1], res['serial'][0][1])
    out['between'] = max(eb)
    print(f'[{tag} fp32] default vs serial: worst gradient {worst(e)}, median {median(e):.2e}; worst over {len(eb)} pairs {max(eb):.2e}')
    return out
