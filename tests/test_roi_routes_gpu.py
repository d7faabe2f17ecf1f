"""Every route of the RoIAlign launchers (csrc/roi_align.hip: roi_route / roi_emit) at the smallest shape that reaches it: the
plan (ops.roi_align_plan) says which route the call takes, the result is held to the oracle at the tolerances
tests/test_ops_gpu.py and tests/test_htc_gpu.py use for that route."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops
from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

TOL = dict(atol=1e-4, rtol=1e-4)


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _case(N, C, levels=1, seed=50):
    """`levels` maps of a 128 x 128 image (32 x 32, 16 x 16) on the CPU and N RoIs inside it, both levels used where there are two."""
    from dynamask_amd import synth
    feats = synth.make_fpn(2, 128, 128, C, seed=seed)[:levels]
    rois = synth.make_rois(2, (N + 1) // 2, 128, 128, seed=seed + 1, max_size=400.0)[:N].contiguous()
    if levels == 2 and N >= 3:
        assert set(ref_ops.map_roi_levels(rois, 2).tolist()) == {0, 1}
    return feats, rois


def _kernels(ops, plan):
    return [ops.ROI_KERNELS[r['kernel']] for r in plan]


@pytest.mark.parametrize('route,N,C,P,levels', [(['order', 'tile'], 200, 64, 14, 2), (['tile'], 5, 16, 7, 1), (['band'], 3, 8, 28, 1),
                                                (['generic', 'generic'], 3, 6, 14, 1)])
def test_forward_routes_against_the_oracle(ops, route, N, C, P, levels):
    feats, rois = _case(N, C, levels)
    strides = (4, 8)[:levels]
    plan = ops.roi_align_plan('forward', [tuple(f.shape[2:]) for f in feats], 2, C, N, P)
    assert _kernels(ops, plan) == route
    assert [r['levels'] for r in plan] == ([1, 0] if route[0] == 'order' else [1] * len(route))
    ref = ref_ops.single_roi_extractor(feats, rois, P, strides)
    out, lv = ops.roi_align([f.cuda() for f in feats], rois.cuda(), P, [1.0 / s for s in strides], return_levels=True)
    torch.testing.assert_close(out.cpu(), ref, **TOL)
    assert torch.equal(lv.cpu().long(), ref_ops.map_roi_levels(rois, levels) if levels > 1 else torch.zeros(N, dtype=torch.long))


@pytest.mark.parametrize('pool', [1, 2])
@pytest.mark.parametrize('N', [200, 5])
def test_add_entry_has_the_forward_plans_channels_and_its_bits(ops, N, pool):
    """pool 1: the bits of ops.roi_align + an add; pool 2: against roi_align + adaptive_avg_pool2d + add through float64
    (tests/test_htc_gpu.py's checks); the launch has the channels per workgroup of the forward of these RoIs: 32 where that
    call orders them (200 RoIs), else 16."""
    C, P = 64, 14
    (sem,), rois = _case(N, C, seed=60)
    fwd = ops.roi_align_plan('forward', [tuple(sem.shape[2:])], 2, C, N, P)
    add, = ops.roi_align_plan('add', [tuple(sem.shape[2:])], 2, C, N, P, pool=pool)
    assert _kernels(ops, fwd) == (['order', 'tile'] if N == 200 else ['tile']) and _kernels(ops, [add]) == ['tile']
    assert add['P0'] == pool and add['CT'] == fwd[-1]['CT'] == (32 if N == 200 else 16) and add['grid'] == fwd[-1]['grid']
    S = P // pool
    feats = torch.randn(N, C, S, S, generator=torch.Generator().manual_seed(61))
    crop = ops.roi_align([sem.cuda()], rois.cuda(), P, [0.25])
    out = feats.cuda()
    ops.roi_align_add_(out, sem.cuda(), rois.cuda(), P, 0.25)
    if pool == 1:
        assert torch.equal(out, feats.cuda() + crop)
    else:
        ref32 = feats.cuda() + F.adaptive_avg_pool2d(crop, (S, S))
        ref64 = feats.double() + F.adaptive_avg_pool2d(ref_ops.roi_align(sem.double(), rois, P, 0.25), (S, S))
        assert_close_via_f64(out, ref32, ref64, 'RoIAlign-add (2 x 2 mean)')


@pytest.mark.parametrize('route,P', [('generic', 14), ('bwd_gather', 28)])
def test_backward_routes_against_autograd_of_the_oracle(ops, route, P):
    feats, rois = _case(6, 8, 2, seed=70)
    feats = [f.requires_grad_(True) for f in feats]
    one, = ops.roi_align_plan('backward', [tuple(f.shape[2:]) for f in feats], 2, 8, 6, P)
    assert ops.ROI_KERNELS[one['kernel']] == route and one['P0'] == (1 if route == 'generic' else 0)
    ref = ref_ops.single_roi_extractor(feats, rois, P, (4, 8))
    go = torch.randn(ref.shape, generator=torch.Generator().manual_seed(71))
    ref.backward(go)
    grads = ops.roi_align_backward(go.cuda(), [tuple(f.shape) for f in feats], rois.cuda(), P, [0.25, 0.125])
    for lvl, (gr, f) in enumerate(zip(grads, feats)):
        assert_grad_close(gr, f.grad, f'level {lvl}', rel=1e-4)
