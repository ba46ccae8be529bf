"""GPU: GA-ConvNeXt with gram_fp64=True -- get_gram's float64 branch (`training and B < 128`, ga_convnext.py:452-467) on the
fp64 kernels of csrc/gram64.hip -- through the engine: which plans take it, the existing parity gates with it on, the Gram
vector's error against the oracle with it on and off, the bf16 mode, and train.py --gram-fp64."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from _gradcheck import assert_grads_close, BF16_REL, BF16_COS
from test_model_gpu import load_golden, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ['v2', 't768']


def _oracle():
    from oracle import ga_convnext_oracle as O
    return O


def make_model(tag, mode, **kw):
    """the V2 parity config / ga_convnext_tiny_768 with the oracle's deterministic state, as tests/test_model_gpu.py builds them;
    kw: gram_fp64 (or nothing: the model as every other test creates it)"""
    import imagenet_models_amd as A
    O = _oracle()
    _, cfg = load_golden(f'{tag}_train_b4.npz')
    if tag == 'v2':
        m = A.GA_ConvNeXt(num_classes=cfg['num_classes'], depths=cfg['depths'], dims=cfg['dims'],
                          gram_embedding_gropus=cfg['gram_groups'], dim_embed=cfg['dim_embed'], stage3_naggre=cfg['naggre'],
                          gram_dim=cfg['gram_dim'], math_mode=mode, **kw)
    else:
        m = A.create_model('ga_convnext_tiny_768', math_mode=mode, **kw)
    m.load_state_dict(O.fill_state(cfg))
    return m.cuda()


def labels(plan):
    return [c[2] for c in plan.calls]


_STEPS = {}


def train_step(tag, mode, gram_fp64):
    """one train step at B = 4 on the golden files' input; computed once per configuration and shared (read-only) by the tests"""
    key = (tag, mode, gram_fp64)
    if key not in _STEPS:
        import imagenet_models_amd as A
        O = _oracle()
        z, _ = load_golden(f'{tag}_train_b4.npz')
        m = make_model(tag, mode, gram_fp64=gram_fp64).train()
        m.zero_grad()
        outs = m(O.gen_input(4, seed=1).cuda())
        loss = A.ga_loss(outs, torch.from_numpy(z['target']).cuda(), float(z['lam']))
        loss.backward()
        eng = m.engine(4, True)
        heads = [dict(vec=h['vec'].float().cpu(), g1=h['g1'].float().cpu(), Kg=h['Kg'], Kp=h['Kp']) for h in eng.heads]
        _STEPS[key] = dict(outs=[o.detach().cpu() for o in outs], loss=float(loss.detach()), heads=heads,
                           grads={n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()},
                           fwd=labels(eng.fwd), bwd=labels(eng.bwd))
        del m, eng
        torch.cuda.empty_cache()
    return _STEPS[key]


def golden_errors(tag, st):
    """against the real reference's numbers ({tag}_train_b4.npz, written through the float64 branch), measured as
    test_t768_train_step_fp32_vs_reference_golden does: (logits, loss, worst gradient norm, worst 16-value gradient head)"""
    z, _ = load_golden(f'{tag}_train_b4.npz')
    e_out = rel(torch.stack(st['outs'])[:, :, :40], torch.from_numpy(z['logits']))
    e_loss = abs(st['loss'] - float(z['loss'])) / abs(float(z['loss']))
    gmax = float(np.abs(z['grad_head']).max())
    e_norm = e_head = 0.0
    for i, n in enumerate(str(n) for n in z['grad_names']):
        g = st['grads'][n]
        ref_norm = float(z['grad_norm'][i])
        if ref_norm > 1e-2 * gmax:
            e_norm = max(e_norm, abs(float(g.double().norm()) - ref_norm) / ref_norm)
        head = g.reshape(-1)[:16].numpy()
        ref_head = z['grad_head'][i][:head.size]
        e_head = max(e_head, float(np.abs(head - ref_head).max() / max(np.abs(ref_head).max(), 1e-2 * gmax)))
    return e_out, e_loss, e_norm, e_head


def fp64_errors(tag, st):
    """against the float64 run of the oracle ({tag}_train_b4_fp64.npz), measured as test_fp32_mode_gradients_vs_fp64_ground_truth
    does: (logits, loss, worst gradient)"""
    z, _ = load_golden(f'{tag}_train_b4_fp64.npz')
    e_out = rel(torch.stack(st['outs'])[:, :, :40].double(), torch.from_numpy(z['logits']))
    e_loss = abs(st['loss'] - float(z['loss'])) / abs(float(z['loss']))
    gmax = float(z['grad_absmax'].max())
    worst = []
    for i, n in enumerate(str(n) for n in z['grad_names']):
        g = st['grads'][n].double()
        amax, nref = float(z['grad_absmax'][i]), float(z['grad_norm'][i])
        head = g.reshape(-1)[:16].numpy()
        dh = float(np.abs(head - z['grad_head'][i][:head.size]).max())
        if amax >= 1e-4 * gmax:
            worst.append((max(abs(float(g.norm()) - nref) / nref, dh / amax), n))
        else:
            worst.append((dh / (1e-4 * gmax) * 5e-3, n))
    worst.sort(reverse=True)
    return e_out, e_loss, worst[0]


@pytest.mark.parametrize('tag', TAGS)
def test_plan_selection(tag):
    K = 5
    on = make_model(tag, 'fp32', gram_fp64=True)
    tr = on.engine(4, True)
    f, b = labels(tr.fwd), labels(tr.bwd)
    for k in range(K):
        assert f.count(f'gram.{k}.f64') == 1 and b.count(f'gram.{k}.f64b') == 1
        for gone in (f'gram.{k}', f'gram.{k}.pack'):
            assert gone not in f
        for gone in (f'gram.{k}.packb', f'gram.{k}.dx'):
            assert gone not in b
    ev = labels(on.engine(4, False).fwd)
    assert not any('.f64' in s for s in ev) and all(f'gram.{k}.pack' in ev for k in range(K))
    if tag == 'v2':         # B = 128 is the reference's threshold: no float64 there
        big = on.engine(128, True)
        assert not any('.f64' in s for s in labels(big.fwd) + labels(big.bwd))
        assert all(f'gram.{k}.pack' in labels(big.fwd) and f'gram.{k}.dx' in labels(big.bwd) for k in range(K))
    del on, tr
    torch.cuda.empty_cache()
    # off (the default): the plans of a model built without the kwarg
    off, plain = make_model(tag, 'fp32', gram_fp64=False), make_model(tag, 'fp32')
    assert plain.cfg['gram_fp64'] is False
    for training in (True, False):
        eo, ep = off.engine(4, training), plain.engine(4, training)
        assert labels(eo.fwd) == labels(ep.fwd) and not any('.f64' in s for s in labels(ep.fwd))
        if training:
            assert labels(eo.bwd) == labels(ep.bwd) and not any('.f64' in s for s in labels(ep.bwd))


@pytest.mark.parametrize('tag', TAGS)
def test_existing_fp32_gates_hold_with_the_float64_gram(tag):
    """the gates of test_v2_train_step_fp32_vs_oracle_and_reference / test_t768_train_step_fp32_vs_reference_golden (logits, loss
    1e-3; gradient norms and heads 2e-2 against the fp32 reference) and of test_fp32_mode_gradients_vs_fp64_ground_truth (logits,
    loss 1e-3; every gradient 5e-3 against float64)"""
    st = train_step(tag, 'fp32', True)
    assert any('.f64' in s for s in st['fwd']) and any('.f64b' in s for s in st['bwd'])
    g_out, g_loss, g_norm, g_head = golden_errors(tag, st)
    d_out, d_loss, d_worst = fp64_errors(tag, st)
    print(f'[{tag} gram_fp64] vs reference golden: logits {g_out:.2e} loss {g_loss:.2e} grad norm {g_norm:.2e} head {g_head:.2e}; '
          f'vs float64 oracle: logits {d_out:.2e} loss {d_loss:.2e} worst grad {d_worst}')
    assert g_out < 1e-3 and g_loss < 1e-3 and g_norm < 2e-2
    if tag == 't768':       # the tiny_768 test also gates the first 16 values of every gradient
        assert g_head < 2e-2
    assert d_out < 1e-3 and d_loss < 1e-3 and d_worst[0] < 5e-3


def vec_error(st):
    """worst |vec - ref| / (2^-23 |ref| + 1e-12 max|ref|) over the five heads, ref = the oracle's get_gram (float64 branch, result
    through .float()) of the engine's own gram-layer output: <= 1 is the one-step rule of tests/test_gram_f64_kernels_gpu.py"""
    O = _oracle()
    worst = 0.0
    for h in st['heads']:
        g1 = h['g1']
        B, C = 4, g1.shape[1]
        HW = g1.shape[0] // B
        H = int(round(HW ** 0.5))
        ref = O.get_gram(g1.reshape(B, HW, C).permute(0, 2, 1).reshape(B, C, H, H), training=True).reshape(B, -1).double()
        vec = h['vec'].reshape(B, -1, h['Kp'])
        assert bool((vec[:, :, h['Kg']:] == 0).all())
        vec = vec[:, :, :h['Kg']].reshape(B, -1).double()
        bound = 2.0 ** -23 * ref.abs() + 1e-12 * ref.abs().amax(dim=1, keepdim=True)
        worst = max(worst, float(((vec - ref).abs() / bound).max()))
    return worst


@pytest.mark.parametrize('tag', TAGS)
def test_gram_vector_error_before_and_after(tag):
    """the Gram vectors of the five heads against the oracle fed the engine's own g1: within one fp32 step with the flag on, not
    with it off (the fp32-accumulate path); and the step's errors against the reference's golden numbers, both ways (reported)"""
    on, off = train_step(tag, 'fp32', True), train_step(tag, 'fp32', False)
    assert not any('.f64' in s for s in off['fwd'])
    e_on, e_off = vec_error(on), vec_error(off)
    print(f'[{tag}] Gram vector, worst |vec - ref| in units of the one-step gate: gram_fp64 on {e_on:.3f}, off {e_off:.1f}')
    for name, st in (('on', on), ('off', off)):
        g_out, g_loss, g_norm, g_head = golden_errors(tag, st)
        d_out, d_loss, d_worst = fp64_errors(tag, st)
        print(f'[{tag}] gram_fp64 {name}: vs {tag}_train_b4.npz logits {g_out:.3e} loss {g_loss:.3e} worst grad norm {g_norm:.3e} '
              f'head {g_head:.3e}; vs float64 oracle worst grad {d_worst[0]:.3e} ({d_worst[1]})')
    assert e_on <= 1.0
    assert e_off > 1.0
    assert e_on < e_off


def test_bf16_mode_step_with_the_float64_gram():
    """bf16 mode, flag on, against the fp32-mode step (flag on): the gates of test_v2_train_step_bf16_small_batch_is_finite_and_close
    (logits 8e-2, loss 2e-2) and the whole-tensor gradient gates of tests/_gradcheck.py"""
    lo, hi = train_step('v2', 'bf16', True), train_step('v2', 'fp32', True)
    assert any('.f64' in s for s in lo['fwd']) and any('.f64b' in s for s in lo['bwd'])
    e_out = max(rel(a, b) for a, b in zip(lo['outs'], hi['outs']))
    e_loss = abs(lo['loss'] - hi['loss']) / abs(hi['loss'])
    print(f'[v2 bf16 gram_fp64 vs fp32 mode] logits {e_out:.2e} loss {e_loss:.2e}')
    assert all(torch.isfinite(g).all() for g in lo['grads'].values())
    assert e_out < 8e-2 and e_loss < 2e-2
    assert_grads_close(lo['grads'], hi['grads'], BF16_REL, BF16_COS, 'v2 bf16 gram_fp64 B=4 vs fp32 mode')


def test_train_cli_gram_fp64():
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, 'train.py', '--synthetic', '--model', 'ga_convnext_tiny_768',
                        '-b', '8', '--steps-per-epoch', '2', '--epochs', '1', '--gram-fp64', '--device', 'cuda', '--log-interval', '1'],
                       cwd=ROOT, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    loss = re.search(r'\*\*\* epoch 0: train loss (\S+)', out)
    assert loss is not None and math.isfinite(float(loss.group(1))), out[-2000:]
