"""GPU: what every training engine seals (`EngineBase._seal` -> `grad_groups()`) against what its backward plan really does.

TrainStep (trainer.py) all-reduces the flat-gradient slices a group claims as soon as the backward plan has been issued up to
the group's mark (the DDP reducer of /root/reference/GA/train.py:514, overlapped with backward).  That is only correct if every
gradient of the group is FINAL at its mark: no later launch (a weight-gradient GEMM still on the asynchronous lane, a deferred
weight-unfold batch, a pooling-conv weight gradient recorded after the mark) may write it.  The engine refuses, while it records,
to hand out a gradient it has sealed (`EngineBase.grad`); for every registered family this test also runs the backward plan in
the same segments (`backward_to`), snapshots the slices each mark owns when the mark is reached, finishes the backward pass and
requires the snapshots to be bit-identical to the final gradients.  One GPU, no process group."""
import pytest
import torch

from test_host_cpu import GA_CONVNEXT_GROUPS, _small

pytestmark = pytest.mark.gpu

B = 2
FAMILIES = [          # every name of tools/plan_fingerprint.py's NAMED
    ('ga_convnext_tiny_768', {}),
    ('ga_convnext_tiny_768', dict(gram_fp64=True)),
    ('ga_convnext_tiny_688', {}),         # padded parameter gradients of the odd-width heads: copied back before the 'heads' mark
    ('ga_CSWin_64_12211_tiny_224', {}),
    ('map_convnext_tiny', {}),
    ('map_vit_small_patch16_224', {}),
    ('map_pit_s', {}),
    ('pit_s', {}),
    ('convnext_tiny', {}),
    ('mobilenet_v1', {}),
    ('map_mobilenet_v1', {}),
    ('map_resnet50', {}),
]


@pytest.fixture(scope='module', params=FAMILIES, ids=[n + ''.join(f'+{k}' for k in kw) for n, kw in FAMILIES])
def family(request):
    """(name, model, its training engine at B = 2): built once for the tests of this module"""
    import imagenet_models_amd as A
    name, kw = request.param
    torch.manual_seed(0)
    m = A.create_model(name, **kw).cuda().train()
    # the reference's init leaves layer-scale at 1e-6: gradients would be denormal-small in places; any non-trivial values do
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() <= 1 and float(p.abs().max()) < 1e-3:
                p.fill_(0.1)
    return name, m, m.engine(B, True)


def test_group_slices_are_final_at_their_mark(family):
    from imagenet_models_amd.trainer import make_buckets
    name, m, eng = family
    st = m.flat_state()
    g = st['grads']
    groups = eng.grad_groups()
    assert groups, f'{name}: no gradient groups declared'
    buckets = make_buckets(st, groups, 1 << 40)
    img = getattr(eng, 'img', 224) or 224
    x = torch.randn(B, 3, img, img, device='cuda')
    y = torch.randint(0, m.num_classes, (B,), device='cuda')
    m.zero_grad()
    eng.forward_loss(x, y, -0.8, 0, 0.0, 1.0)
    marks = eng.bwd.marks
    for mark, _ in groups:
        assert mark in marks, f'{name}: group mark {mark!r} is not recorded by the backward plan ({list(marks)})'
    snaps, pos = [], 0
    for mark, a, b in buckets:
        stop = len(eng.bwd.calls) if mark == 'end' else marks[mark]
        assert stop >= pos, f'{name}: marks out of order at {mark!r}'
        pos = stop
        eng.backward_to(mark)
        torch.cuda.synchronize()
        snaps.append((mark, a, b, g[a:b].clone()))
    eng.backward_to('end')
    torch.cuda.synchronize()
    bad = []
    for mark, a, b, snap in snaps:
        if not torch.equal(snap, g[a:b]):
            # name the parameters that moved
            for n, (off, k) in st['slices'].items():
                if a <= off < b and not torch.equal(snap[off - a:off - a + k], g[off:off + k]):
                    bad.append((mark, n))
    assert not bad, f'{name}: gradients written AFTER the mark that declares them final: {bad[:12]} ({len(bad)} tensors)'
    # the test is vacuous if the claimed slices never received a gradient
    for mark, _ in groups:
        tot = sum(float(s.abs().sum()) for mk, a, b, s in snaps if mk == mark)
        assert tot > 0.0, f'{name}: group {mark!r} holds no gradient at all'


def test_every_sealed_prefix_names_parameters_and_no_parameter_is_sealed_twice(family):
    name, m, eng = family
    names = [n for n, _ in m.named_parameters()]
    groups = eng.grad_groups()
    for mark, prefixes in groups:
        for pre in prefixes:
            assert any(n.startswith(pre) for n in names), f'{name}: prefix {pre!r} of mark {mark!r} matches no parameter'
    for n in names:
        owners = [mark for mark, prefixes in groups if n.startswith(tuple(prefixes))]
        assert len(owners) <= 1, f'{name}: {n} is claimed by the marks {owners}'


def _small_engines():
    m = _small().cuda().train()
    return m, m.engine(B, True), m.engine(B, False)


def test_engine_refuses_a_sealed_gradient_and_reports_what_it_sealed():
    m, eng, ev = _small_engines()
    P = dict(m.named_parameters())
    # the literal the CPU tests of make_buckets use is what the engine seals
    assert eng.grad_groups() == GA_CONVNEXT_GROUPS
    assert ev.grad_groups() == []
    for mark, pname in (('heads', 'fc.4.weight'), ('heads', 'ga.0.attn.k.weight'), ('stage3', 'stages.3.blocks.0.mlp.fc1.weight'),
                        ('stage1', 'stages.1.downsample.1.weight')):
        assert pname in P
        with pytest.raises(RuntimeError, match=f'(?s){pname}.*{mark!r}'):
            eng.grad(pname)
    for pname in ('stem.0.weight', 'stem.1.bias', 'stages.0.blocks.0.gamma'):       # final at the end of the plan only: never sealed
        assert eng.grad(pname) is P[pname].grad


def test_pit_seals_its_classifier_and_the_stages_of_map_pit():
    """one PiTTrunk builder under two heads: the plain PiT seals `head.` as 'heads' and the trunk's stages exactly as MAP-PiT does"""
    import imagenet_models_amd as A
    groups = {name: dict(A.create_model(name).cuda().train().engine(B, True).grad_groups()) for name in ('pit_s', 'map_pit_s')}
    for name in groups:
        assert list(groups[name]) == ['heads', 'stage3', 'stage2'] and groups[name]['heads'] == ('head.',), name
    assert groups['pit_s'] == {**groups['map_pit_s'], 'heads': ('head.',)}
