"""CPU: the float64 closed form of the JSD loss (tests/_loss_jsd_ref.py) against float64 autograd of timm's own formulation, the gate
against an fp32 restatement in the kernel's order and against three wrong restatements, the underflow case, the row placement and
draw consumption of AugSplits.sample_table, and the train.py surface of --aug-splits / --jsd-loss / --resplit / --split-bn.

"1e-12 relative" below is relative to the largest magnitude of the tensor compared: the gradient has elements that cancel to 0."""
import random

import numpy as np
import pytest
import torch

import _loss_jsd_ref as J
import test_recipe_flags_cpu as RF
from test_recipe_flags_cpu import ga_dir, map_dir, _print_config      # noqa: F401  (the two folder fixtures)

F32, F64 = J.F32, J.F64
_REF = {}


def _ref(c):
    if c.label not in _REF:
        i = J.jsd_inputs(c)
        _REF[c.label] = (i, J.JsdRef(i, c))
    return _REF[c.label]


def test_case_table_covers_what_the_kernel_distinguishes():
    cs = J.JSD_CASES
    assert {c.NC for c in cs} >= {1, 2, 63, 64, 65, 255, 256, 257, 1000, 8188, 8189, 20476}
    assert {c.S for c in cs} == {2, 3, 4, 8} and {c.Bs for c in cs} == {1, 3} and {c.K for c in cs} == {1, 5}
    assert {c.avg for c in cs} == {True, False} and {c.smooth for c in cs} == {0.0, 0.1} and {c.gs for c in cs} == {1.0, 0.25, 65536.0}
    assert {c.regime for c in cs} == {'randn2', 'randn8', 'randn30', 'same', 'spike', 'const'}
    assert any(J.lds_bytes(c.S, c.NC) == J.LDS_OPT_IN for c in cs) and any(J.lds_bytes(c.S, c.NC) == J.LDS_MAX for c in cs)
    assert len(cs) <= 30


@pytest.mark.parametrize('c', [c for c in J.JSD_CASES if c.NC <= 1000], ids=repr)
def test_closed_form_is_float64_autograd(c):
    """(i) wherever no probability underflows in float64 (every case: the spike's exp(-130) is an ordinary double)"""
    i, ref = _ref(c)
    ag = J.jsd_autograd(i, c)
    for n, (r, _, _) in ref.out.items():
        assert torch.isfinite(torch.as_tensor(ag[n])).all(), n
        scale = max(float(torch.as_tensor(r).abs().max()), 1e-300)
        assert float((torch.as_tensor(ag[n]) - r).abs().max()) <= 1e-12 * scale, (n, float((torch.as_tensor(ag[n]) - r).abs().max()) / scale)


@pytest.mark.parametrize('c', J.JSD_CASES, ids=repr)
def test_fp32_restatement_meets_the_gate_and_wrong_ones_do_not(c):
    """(ii) fp32 in the kernel's order passes on the derived roundings alone (eps = 0: torch's exp / log are not the hardware's);
    (iii) each wrong restatement fails wherever it differs: the ignored clamp on every case with a clamped column, CE over all
    rows and batchmean over B wherever there is more than one class (and, for the latter, a JSD term at all)"""
    i, ref = _ref(c)
    ratios = J.jsd_ratios(J.jsd_restate(i, c), ref.out, F32, c.gs, eps=0.0)
    assert max(ratios.values()) < 1.0, ratios
    assert int(ref.near_clamp().sum()) == 0
    worst = {w: max(J.jsd_ratios(J.jsd_restate(i, c, wrong=w), ref.out, F32, c.gs).values()) for w in J.JSD_WRONG}
    if bool(ref.clamped.any()):
        assert worst['clamp_ignored'] > 4.0, worst
    else:
        assert worst['clamp_ignored'] < 1.0, worst          # the same arithmetic where nothing is clamped
    if c.NC > 1:
        assert worst['ce_all_rows'] > 4.0, worst
        if c.regime != 'same':
            assert worst['batchmean_over_B'] > 4.0, worst


def test_regimes_are_what_their_names_say():
    share = {c.label: float(_ref(c)[1].clamped.double().mean()) for c in J.JSD_CASES}
    for c in J.JSD_CASES:
        if c.regime == 'randn2':
            assert share[c.label] == 0.0, c
        if c.regime == 'randn8' and c.NC == 1000:
            assert 0.3 < share[c.label] < 0.9, (c, share[c.label])
        if c.regime == 'randn30' and c.NC >= 1000:
            assert share[c.label] > 0.9, (c, share[c.label])
        if c.regime == 'same':
            assert float(_ref(c)[1].parts['dx'].abs().max()) <= 1e-12


@pytest.mark.parametrize('c', [c for c in J.JSD_CASES if c.regime == 'spike'], ids=repr)
def test_underflow_case_is_finite_in_the_closed_form(c):
    """(iv) one logit 120 above the rest in split 1 only: fp32 p is 0 there; the closed form in log space and the fp32 restatement
    stay finite and meet the gate, where fp32 autograd of the xlogy form gives NaN"""
    i, ref = _ref(c)
    for n, (r, a0, ce) in ref.out.items():
        assert torch.isfinite(torch.as_tensor(r)).all() and torch.isfinite(torch.as_tensor(a0)).all(), n
    got = J.jsd_restate(i, c)
    assert torch.isfinite(got['dorg']).all() and torch.isfinite(got['loss'])
    p32 = torch.softmax(i['org'].to(F32), -1).view(c.K, c.S, c.Bs, c.NC)[:, 1]
    assert bool((p32 == 0).any()), 'no fp32 probability underflows: the case lost its point'
    x = i['org'][0].to(F32).requires_grad_(True)
    probs = [torch.softmax(s, 1) for s in torch.split(x, c.Bs)]
    logm = torch.clamp(torch.stack(probs).mean(0), 1e-7, 1).log()
    sum(torch.nn.functional.kl_div(logm, p, reduction='batchmean') for p in probs).backward()
    assert bool(torch.isnan(x.grad).any()), 'fp32 autograd no longer gives NaN here: the documented deviation has gone'


# ---- (v) AugSplits.sample_table ----------------------------------------------------------------------------------------------
class _RecRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def random(self):
        self.calls.append('random')
        return super().random()

    def gauss(self, mu, sigma):
        self.calls.append('gauss')
        return super().gauss(mu, sigma)

    def uniform(self, a, b):
        self.calls.append('uniform')
        return super().uniform(a, b)

    def choice(self, seq):
        self.calls.append('choice')
        return super().choice(seq)


class _RecNp:
    def __init__(self, seed):
        self.r, self.calls = np.random.RandomState(seed), []

    def choice(self, a, size):
        self.calls.append(('choice', a, size))
        return self.r.choice(a, size)


@pytest.mark.parametrize('S,b', [(3, 4), (2, 1), (8, 3)])
def test_sample_table_places_the_draws_split_major(S, b):
    import imagenet_models_amd as A
    from imagenet_models_amd import rand_augment as RA
    H = W = 32
    r1, n1, r2, n2 = _RecRandom(11), _RecNp(5), _RecRandom(11), _RecNp(5)
    ra1 = A.RandAugment('rand-m9-mstd0.5-inc1', rng=r1, np_rng=n1)
    ra2 = A.RandAugment('rand-m9-mstd0.5-inc1', rng=r2, np_rng=n2)
    tab = A.AugSplits(S).sample_table(ra1, b, H, W)
    draws = ra2.sample(b * (S - 1), H, W)
    assert r1.calls == r2.calls and n1.calls == n2.calls and len(n1.calls) == b * (S - 1)       # exactly those draws, in that order
    assert r1.getstate() == r2.getstate()
    assert tab.dtype == RA.ROW and tab.shape == (S * b, ra1.num_layers)
    none = ra2.__class__('rand-m9-mstd0.5-inc1-p0', rng=random.Random(0), np_rng=np.random.RandomState(0)).sample(b, H, W)
    assert (none['kind'] == RA.NONE).all() and tab[:b].tobytes() == none.tobytes()       # split 0: the rows sample() initialises
    for i in range(b):
        for j in range(1, S):
            assert tab[j * b + i].tobytes() == draws[i * (S - 1) + (j - 1)].tobytes(), (i, j)
    assert (tab[b:]['kind'] != RA.NONE).any()
    with pytest.raises(ValueError, match='at least 2'):
        A.AugSplits(1)


def test_input_stage_takes_and_refusals_need_no_device():
    import imagenet_models_amd as A
    sp = A.AugSplits(3)
    assert A.InputStage(aug_splits=sp).takes == 'uint8'
    assert A.InputStage(aug_splits=sp, crop=A.RandomResizedCrop(32)).takes == 'ragged'
    assert A.InputStage().takes == 'any'
    with pytest.raises(TypeError, match='aug_splits'):
        A.InputStage(aug_splits=sp).check(torch.zeros(3, 3, 8, 8))
    mix = A.Mixup(mixup_alpha=0.2, cutmix_alpha=0., num_classes=10)
    with pytest.raises(ValueError, match='aug_splits cannot be combined with mixup_fn / collate_mixup'):
        A.InputStage(aug_splits=sp, mixup_fn=mix)
    with pytest.raises(ValueError, match='aug_splits cannot be combined with mixup_fn / collate_mixup'):
        A.InputStage(aug_splits=sp, collate_mixup=A.FastCollateMixup(mixup_alpha=0.2, cutmix_alpha=0., num_classes=10))
    with pytest.raises(ValueError, match='num_splits = 2 does not match'):
        A.InputStage(aug_splits=sp, random_erasing=A.RandomErasing(probability=1.0, num_splits=2))
    for ns in (0, 3):
        A.InputStage(aug_splits=sp, random_erasing=A.RandomErasing(probability=1.0, num_splits=ns))


def test_python_losses_name_the_kind_and_refuse_dense_targets():
    from imagenet_models_amd import loss as L
    assert L._KINDS == {'ce': 0, 'bce': 1, 'jsd': 2}
    t = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match='num_splits >= 2'):
        L._jsd_args(2, t, 6, None)
    with pytest.raises(TypeError, match='no dense-target'):
        L._jsd_args(2, torch.zeros(6, 10), 6, 3)
    with pytest.raises(ValueError, match='does not divide'):
        L._jsd_args(2, t, 6, 4)
    assert L._jsd_args(2, t, 6, 3).shape == (2,) and L._jsd_args(2, t[:2], 6, 3).shape == (2,)


def test_entry_point_is_declared_bound_and_refuses_on_the_host():
    import os
    from imagenet_models_amd import _lib
    hdr = open(os.path.join(RF.ROOT, 'include', 'gaext.h')).read()
    assert 'int ga_loss_jsd_fwd_bwd(' in hdr and '4 (S NC + 8) bytes' in hdr and 'ga_loss_jsd_fwd_bwd' in _lib.exported_symbols()
    lib = _lib.load()
    assert lib.ga_loss_jsd_fwd_bwd(None, None, None, None, None, None, 1, 6, 10, 3, 0.0, 0.0, 12.0, 1.0, 0, None) != 0
    assert 'ga_loss_jsd_fwd_bwd' in _lib.last_error()
    n = len(_lib.exported_symbols())
    for doc, phrase in (('README.md', f'{n} entry points'), ('DESIGN.md', f'{n} `extern "C"` entry points'),
                        ('INTEGRATION.md', f'all {n} entry points')):
        assert phrase in open(os.path.join(RF.ROOT, doc)).read(), (doc, phrase)


# ---- (vi) - (viii) train.py ----------------------------------------------------------------------------------------------------
SYN = ['--synthetic', '--model', 'map_convnext_tiny', '-b', '32']


@pytest.mark.parametrize('argv,reason', [
    (['--aug-splits', '1'], 'a split count of 1 makes no sense'),
    (['--jsd-loss'], '--jsd-loss is only valid with --aug-splits'),
    (['--aug-splits', '3', '--mixup', '0.8'], 'cannot be combined with mixup / cutmix'),
    (['--aug-splits', '3', '--cutmix', '1.0', '--mixup', '0'], 'cannot be combined with mixup / cutmix'),
    (['--aug-splits', '2', '--split-bn'], '--split-bn'),
    (['--split-bn'], 'not built'),
])
def test_train_refusals(argv, reason):
    r, out = _print_config(SYN + argv, ok=False)
    assert r.returncode != 0 and reason in out and '{' not in r.stdout, out[-2000:]


def test_print_config_keys():
    _, cfg = _print_config(SYN + ['--aug-splits', '3', '--jsd-loss', '--aa', 'rand-m9-mstd0.5-inc1', '--reprob', '0.25', '--remode', 'pixel',
                                  '--resplit', '--dec-lam', '-0.8', '-tb', '128'])
    assert cfg['aug_splits'] == 3 and cfg['jsd_loss'] is True and cfg['model_batch'] == 96 and cfg['batch_size'] == 32
    assert cfg['grad_accumulation'] == 4                         # -tb keeps dividing by the base batch (MAP/train.py:406)
    _, cfg = _print_config(SYN + ['--aug-splits', '2', '--mixup', '0', '--cutmix', '0', '--bce-loss'])      # legal without --jsd-loss
    assert cfg['aug_splits'] == 2 and cfg['jsd_loss'] is False and cfg['model_batch'] == 64
    _, cfg = _print_config(SYN + ['--resplit'])                   # --resplit alone stays accepted and inert
    assert cfg['aug_splits'] == 0 and cfg['jsd_loss'] is False and cfg['model_batch'] == 32


@pytest.mark.parametrize('model,lr,dp', RF.GA_LINES)
def test_ga_readme_lines_still_resolve(model, lr, dp, ga_dir):      # noqa: F811
    argv = [ga_dir] + RF.GA_COMMON.format(model=model, lr=lr, dp=dp).split() + ['--aug-repeats', '3', '--cooldown-epochs', '10']
    _, cfg = _print_config(argv)
    assert cfg['model'] == model and cfg['aug_repeats'] == 3 and cfg['selected_round'] == 256 and cfg['grad_accumulation'] == 4
    assert cfg['epochs'] == 310 and cfg['train_images'] == 256 and cfg['batches_per_epoch'] == 2 and cfg['distinct_files_per_epoch'] == 86
    assert cfg['aug_splits'] == 0 and cfg['jsd_loss'] is False and cfg['model_batch'] == cfg['batch_size'] == 128


@pytest.mark.parametrize('recipe', sorted(RF.MAP_EXPECT))
def test_map_recipes_still_resolve(recipe, map_dir):                # noqa: F811
    model, batch, accum, crop_pct = RF.MAP_EXPECT[recipe]
    argv = [map_dir] + RF.MAP_RECIPES[recipe].split() + ['--model', model, '--selected-round', '0', '--dec-lam', '-0.8']
    _, cfg = _print_config(argv)
    assert cfg['model'] == model and cfg['batch_size'] == batch and cfg['grad_accumulation'] == accum and cfg['crop_pct'] == crop_pct
    assert cfg['aug_repeats'] == 3 and cfg['epochs'] == 300 and cfg['batches_per_epoch'] == 300 // batch
    assert cfg['aug_splits'] == 0 and cfg['jsd_loss'] is False and cfg['model_batch'] == batch
