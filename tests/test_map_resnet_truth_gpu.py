"""GPU: the MAP-ResNet50 fp32 train step against FLOAT64 ground truth, and where its run-to-run spread comes from.

tests/golden/map_rn50_train_b4_fp64.npz holds the B = 4 train step of test_map_resnet_gpu.py run through the reference classes in
float64 (tools/gen_golden_map_resnet.py --fp64: the same fill_state, gen_input(4, seed=1), target seed 99, dec_lam = -0.8 and the
head([stem, layer1..4]) composition).  The fp32 engine is gated against it per tensor with test_fp64_truth_gpu.py's measure.

The spread test runs the fp32 step twice with every lane switch at one lane (tests/_spread.py SERIAL) and twice as shipped, and prints
the spread inside and between the two schedules and the first BatchNorm whose batch sums differ between the serial runs; the same
diagnostic runs, print only, for mobilenet_v1.

Measured on MI355X in two sessions (per-tensor ||g1 - g2|| / ||g2||, worst / median): serial vs serial 2.3e-2 / 5.2e-3 and
1.7e-2 / 6.0e-3, default vs default 3.7e-2 / 7.5e-3 and 1.5e-2 / 4.6e-3, default vs serial (worst of 4 pairs) 4.2e-2 and 2.1e-2.
The spread does not come from a race between lanes: it is there with every lane serial, and the two schedules trade places
between sessions.  It starts in the GEMM epilogues' BatchNorm column sums (ga_gemm colsum / colsumsq,
accumulated with fp32 atomics across workgroups): the first BatchNorm, stem.0.1, already differs by 5e-7 (relative) in s and q
between two serial runs.  ga_bn_finalize turns that into different mean / rstd; ga_se_bn_fwd's hidden BatchNorm over the B = 4
pooled rows amplifies it most (the worst tensors are layer1.*.se.1.*: its normalisation divides by the spread of four per-sample
means that differ from the batch mean by a small fraction of it).  The fp32 engine sits 1.8e-2 from the float64 truth in its
worst tensor (first-16-value error of layer1.2.se.1.1.weight; norm errors up to 4.0e-3), inside that spread.
So the fp64 gate is the fixture test's pair (3e-2 on the norm, 5e-2 on the first 16 values) and not the 5e-3 of the other families; mobilenet_v1 (same BatchNorm-sum atomics, 27 train-mode
BatchNorms at B = 4): serial 1.6e-2 / 1.8e-2, default 1.9e-2 / 1.8e-2."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _fp64_grad_errors(z, grads):
    """test_fp64_truth_gpu.py's per-tensor measures, apart: the norm relative error and the 16-value head error / max |g|; tensors
    below 1e-4 of the global max (analytically zero gradients) are measured against that floor.  Returns both, worst first."""
    names = [str(n) for n in z['grad_names']]
    assert set(names) == set(grads), sorted(set(names) ^ set(grads))[:6]
    gmax = float(z['grad_absmax'].max())
    e_n, e_h = [], []
    for i, n in enumerate(names):
        amax, nref = float(z['grad_absmax'][i]), float(z['grad_norm'][i])
        g = grads[n].double()
        head = g.reshape(-1)[:16].numpy()
        dh = float(np.abs(head - z['grad_head'][i][:head.size]).max())
        floor = max(amax, 1e-4 * gmax)
        e_n.append((abs(float(g.norm()) - nref) / max(nref, 1e-4 * gmax), n))
        e_h.append((dh / floor, n))
    return sorted(e_n, reverse=True), sorted(e_h, reverse=True)


# the gate of the fp32-fixture test (test_map_resnet_gpu.GRAD_GATE_NORM / _HEAD), set above the serial spread (see above)
FP64_GATE_NORM, FP64_GATE_HEAD = 3e-2, 5e-2


def test_train_step_fp32_vs_fp64_ground_truth():
    import test_map_resnet_gpu as T
    z = np.load(os.path.join(GOLDEN, 'map_rn50_train_b4_fp64.npz'))
    z32, _, out, loss, grads = T._train_step('fp32')
    assert np.array_equal(z['target'], z32['target']) and float(z['dec_lam']) == float(z32['dec_lam'])
    e_out = T.rel(T._logits(out)[:, :, :z['logits'].shape[2]], z['logits'])
    e_loss = abs(float(loss.detach()) - float(z['loss'])) / abs(float(z['loss']))
    e_n, e_h = _fp64_grad_errors(z, grads)
    print(f'[{T.NAME} fp32 vs fp64 reference] logits {e_out:.2e} loss {e_loss:.2e} worst grad norm {e_n[:3]} (gate {FP64_GATE_NORM:.0e}) '
          f'worst grad head {e_h[:3]} (gate {FP64_GATE_HEAD:.0e})')
    assert e_out < 1e-3 and e_loss < 1e-3
    assert e_n[0][0] < FP64_GATE_NORM, e_n[:10]
    assert e_h[0][0] < FP64_GATE_HEAD, e_h[:10]


def test_fp32_spread_serial_vs_default_schedule(monkeypatch):
    import _spread
    import test_map_resnet_gpu as T

    def step():
        _, m, _, loss, grads = T._train_step('fp32')
        return loss.detach(), grads, m
    r = _spread.measure(monkeypatch, T.NAME, step)
    # both schedules within the gradient gate; the default one no further from the serial one than the run-to-run gate allows
    assert r['serial'] <= T.GRAD_GATE_HEAD and r['default'] <= T.GRAD_GATE_HEAD and r['between'] <= T.GRAD_GATE_HEAD
    assert r['bn'] is None or r['bn'][2] < 1e-5, 'the BatchNorm batch sums of two identical runs differ by more than fp32 ordering'


def test_mobilenet_v1_spread_serial_vs_default_schedule(monkeypatch):
    """print only: mobilenet_v1's gradient gate (1e-2) also sits above a measured spread"""
    import _spread
    import test_mobilenet_gpu as TM

    def step():
        _, m, _, loss, grads = TM._train_step('mobilenet_v1', 'fp32')
        return loss.detach(), grads, m
    _spread.measure(monkeypatch, 'mobilenet_v1', step)
