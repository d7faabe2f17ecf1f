"""Every build the six training-side launchers of csrc/backward.hip can name (ops.BWD_BUILDS: the values their route
functions write into a plan record) is reached by a GPU case.  The cases of tests/test_bwd_gpu.py and
tests/test_fixed_point_gpu.py carry the route they are meant to reach next to them and assert it through the launcher's own
plan before they run; here those routes are asked of the plan once more, on this device, and their union per launcher must
equal what the launcher can name -- a build that loses its last case, or a new build without one, fails here."""
import pytest
import torch

import fixed_point_ref as fr
import test_bwd_gpu as tb
import test_fixed_point_gpu as tf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _calls(ops):
    """(op, the plan call's shape, its keywords, the launches the case says it reaches) of every case that names a route."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = []
    for (N, C, S, dg), routes in tb.DCN_BWD_ROUTES.items():
        out += [(op, (N, C, S, S, dg), {}, [r]) for op, r in zip(('im2col', 'coord_grad', 'col2im'), routes)]
    for (N, C, dg, H, W), routes in tb.DCN_BWD_RECT_ROUTES.items():
        out += [(op, (N, C, H, W, dg), {}, [r]) for op, r in zip(('im2col', 'coord_grad', 'col2im'), routes)]
    for (N, C, H, W), routes in tb.DCN_NON_SQUARE_ROUTES.items():
        out += [(op, (N, C, H, W, 2), {}, [r]) for op, r in zip(('im2col', 'coord_grad', 'col2im'), routes)]
    for (N, C, S), routes in tb.COORD_FAR_ROUTES.items():
        out += [(op, (N, C, S, S, 2), {}, [r]) for op, r in zip(('coord_grad', 'col2im'), routes)]
    for ct, shapes in fr.COL2IM_SHAPES.items():
        out += [('col2im', (N, C, H, W, dg), {}, [tb.COL2IM[ct]]) for N, C, dg, H, W in shapes]
    for (n, c, H, W), routes in list(tb.UPSAMPLE_ROUTES.items()) + [((1, 2 * cus + 1, 2, 3), tb.UPSAMPLE_MANY_PLANES_ROUTES)]:
        out += [('upsample', (n * c, H, W), dict(align_corners=ac), [routes[ac]]) for ac in (False, True)]
    out += [('point_sample', (2, 22, 25, 42, 11, S), dict(mode='atomics'), [tb.POINT_SAMPLE_ROUTE]) for S in (14, 28, 56)]
    for (S, target), route in tf.PS_ROUTES.items():
        out.append(('point_sample', fr.PS_FEAT_SHAPE + (fr.ps_rois().shape[0], S), dict(mode='fx' if target == 'fx' else 'atomics'), [route]))
    clb = [(7, 64, 28 * 28, tb.CLASS_LOGITS_ROUTES), (1100, 40, 14 * 14, tb.CLASS_LOGITS_SHARED_ROUTES),
           (1100, 40, 14 * 14, {tb.FX: [tf.CLB_FX_ROUTE]})]
    clb += [(N, C, H * W, routes) for N, C, H, W, _, routes in tb.CLASS_LOGITS_BUILD_CASES]
    for N, C, HW, routes in clb:
        out += [('class_logits', (N, C, HW, 80), dict(mode=ops.BWD_MODES[accum]), route) for accum, route in routes.items()]
    return out


def test_the_gpu_cases_reach_every_build_each_launcher_can_name(ops):
    reached = {op: set() for op in ops.BWD_OPS}
    for op, shape, kw, want in _calls(ops):
        got = tb._route(ops, op, *shape, **kw)
        assert got == want, (op, shape, kw)
        reached[op] |= {(ops.BWD_KERNELS.index(k),) + tuple(p) for k, *p in got}
    for op in ops.BWD_OPS:
        assert reached[op] == ops.BWD_BUILDS[op], (op, sorted(ops.BWD_BUILDS[op] - reached[op]), sorted(reached[op] - ops.BWD_BUILDS[op]))
