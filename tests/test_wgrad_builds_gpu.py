"""Every build the weight-gradient launcher can name (csrc/backward.hip: the seven conv_wgrad_kernel builds for each kernel
size, conv_wgrad3_narrow_kernel with and without its tail rows, wgrad_slab_reduce_kernel at every P), each at the smallest
shape dm_conv2d_wgrad_plan routes there -- the test asks the plan and asserts the route, so no shape is trusted -- in slab,
atomic and fixed-point accumulation, against float64 sums at the gate of tests/test_bwd_gpu.py (`_close_sum`).  Three RoIs:
the pixel count is no multiple of the 32-pixel chunk.  Each call carries a bias, two sources (the second at a column offset)
and accumulates into existing dw / db."""
import pytest
import torch

from test_bwd_gpu import _close_sum, _g

pytestmark = pytest.mark.gpu

GEMM, NARROW = 0, 1
# (kernel, build, reduce P in slab mode, Cout, Cs, H, W, ksize).  TN by the cost rule: J = Cs k^2 <= 64 -> 64 columns, <= 128 ->
# 128, 129 .. 256 -> 256 (64-cout tiles only).  7-wide maps keep <= 36 couts off the narrow kernel; 147 px = 5 chunks: at most 5
# splits, 5 .. 20 slabs.  The last two: 588 px = 19 chunks -> 76 slabs, 2352 px = 74 chunks -> 296 slabs
CASES = [
    (GEMM, (1, 2, 2, 1, 0), 1, 65, 128, 7, 7, 1),
    (GEMM, (1, 2, 1, 2, 0), 4, 65, 64, 7, 7, 1),
    (GEMM, (1, 1, 4, 1, 1), 1, 36, 256, 7, 7, 1),
    (GEMM, (1, 1, 2, 2, 1), 4, 33, 128, 7, 7, 1),
    (GEMM, (1, 1, 4, 1, 0), 1, 32, 256, 7, 7, 1),
    (GEMM, (1, 1, 2, 2, 0), 4, 64, 128, 7, 7, 1),
    (GEMM, (1, 1, 1, 4, 0), 4, 5, 30, 7, 7, 1),
    (GEMM, (3, 2, 2, 1, 0), 1, 65, 8, 7, 7, 3),
    (GEMM, (3, 2, 1, 2, 0), 4, 65, 4, 7, 7, 3),
    (GEMM, (3, 1, 4, 1, 1), 1, 36, 24, 7, 7, 3),
    (GEMM, (3, 1, 2, 2, 1), 4, 33, 8, 7, 7, 3),
    (GEMM, (3, 1, 4, 1, 0), 1, 32, 24, 7, 7, 3),
    (GEMM, (3, 1, 2, 2, 0), 4, 64, 8, 7, 7, 3),
    (GEMM, (3, 1, 1, 4, 0), 4, 5, 4, 7, 7, 3),
    (NARROW, (3, 0, 0, 0, 0), 1, 16, 24, 5, 8, 3),
    (NARROW, (3, 0, 0, 0, 1), 1, 36, 40, 5, 8, 3),
    (GEMM, (1, 1, 1, 4, 0), 16, 5, 30, 14, 14, 1),
    (GEMM, (1, 1, 1, 4, 0), 64, 5, 30, 28, 28, 1),
]
NB, CS2 = 3, 3         # RoIs; channels of the second source


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _modes(ops, slab, det):
    saved = ops.WGRAD_SLAB[0], ops.DETERMINISTIC[0]
    ops.WGRAD_SLAB[0], ops.DETERMINISTIC[0] = slab, det
    return saved


def _build(rec):
    return rec['kernel'], tuple(rec[k] for k in ('P0', 'P1', 'P2', 'P3', 'P4'))


@pytest.mark.parametrize('kernel,build,P,cout,cs,H,W,ks', CASES, ids=[f'k{c[0]}-{"".join(map(str, c[1]))}-P{c[2]}' for c in CASES])
def test_build_in_every_accumulation_against_float64(ops, kernel, build, P, cout, cs, H, W, ks):
    # the route of the first source, as the launcher says it (the strides and alignment of the tensors below)
    slab_plan = ops.conv2d_wgrad_plan(NB, cout, cs, H, W, ks, mode='slab', has_bias=True)
    assert _build(slab_plan[0]) == (kernel, build) and slab_plan[0]['accum'] == ops.WGRAD_MODES.index('slab')
    assert len(slab_plan) == 2 and _build(slab_plan[1]) == (2, (P, 0, 0, 0, 0))
    for mode in ('atomics', 'fx'):
        one, = ops.conv2d_wgrad_plan(NB, cout, cs, H, W, ks, mode=mode, has_bias=True)
        assert _build(one) == (kernel, build) and one['accum'] == ops.WGRAD_MODES.index(mode)
    dy = torch.randn(NB, cout, H, W, generator=_g(500))
    xs = [torch.randn(NB, c, H, W, generator=_g(501 + i)) for i, c in enumerate((cs, CS2))]
    dw0 = torch.randn(cout, cs + CS2, ks, ks, generator=_g(503))
    db0 = torch.randn(cout, generator=_g(504))
    xd, dyd, shape = torch.cat(xs, 1).double(), dy.double(), tuple(dw0.shape)
    ref_w = dw0.double() + torch.nn.grad.conv2d_weight(xd, shape, dyd, padding=ks // 2)
    mag_w = dw0.double().abs() + torch.nn.grad.conv2d_weight(xd.abs(), shape, dyd.abs(), padding=ks // 2)
    ref_b, mag_b = db0.double() + dyd.sum((0, 2, 3)), db0.double().abs() + dyd.abs().sum((0, 2, 3))
    dyc, xc = dy.cuda(), [x.cuda() for x in xs]
    assert dyc.data_ptr() % 8 == 0 and all(x.data_ptr() % 8 == 0 for x in xc)

    def run():
        dw, db = dw0.cuda(), db0.cuda()
        ops.conv2d_wgrad(dyc, xc, ks, dw=dw, db=db)
        return dw, db

    for name, slab, det, same_bits in (('slab', True, False, True), ('atomics', False, False, False), ('fx', False, True, True),
                                       ('slab, deterministic', True, True, True)):
        saved = _modes(ops, slab, det)
        try:
            dw, db = run()
            n_cond = _close_sum(dw, ref_w, mag_w, f'dw, {name}') + _close_sum(db, ref_b, mag_b, f'db, {name}')
            print(f'{name}: {n_cond} of {dw.numel() + db.numel()} sums outside 1e-4 but within 8 ulp of their magnitude sum')
            if same_bits:
                dw2, db2 = run()
                assert torch.equal(dw, dw2) and torch.equal(db, db2), name
        finally:
            ops.WGRAD_SLAB[0], ops.DETERMINISTIC[0] = saved


def test_a_deterministic_call_whose_slabs_do_not_fit_takes_the_fixed_point_form(ops):
    """1024 -> 1024 channels 3x3: 8 x 72 output tiles, more than a launch is split down to, so the one slab is the padded dw --
    9.44 M floats against the 8.52 M of dm_conv2d_wgrad_scratch_floats() at 256 compute units.  dm_conv2d_wgrad_slab adds such
    a call with float atomics (the plan says so); with DETERMINISTIC on, ops.conv2d_wgrad asks the plan and takes the
    fixed-point form: the same bits twice, the float64 sums at the same gate."""
    cout, cs, H, W, ks = 1024, 1024, 8, 8, 3
    one, = ops.conv2d_wgrad_plan(1, cout, cs, H, W, ks, mode='slab', has_bias=True)
    assert one['accum'] == ops.WGRAD_MODES.index('atomics') and one['MT'] * one['JT'] > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    dy = torch.randn(1, cout, H, W, generator=_g(510)).cuda()
    x = torch.randn(1, cs, H, W, generator=_g(511)).cuda()
    # float64 sums on the device: dw[co][(ci, tap)] = dy[co][q] . xcol[(ci, tap)][q]
    cols, dyd = torch.nn.functional.unfold(x.double(), ks, padding=1)[0], dy.double().reshape(cout, H * W)
    ref_w, mag_w = (dyd @ cols.t()).reshape(cout, cs, ks, ks).cpu(), (dyd.abs() @ cols.abs().t()).reshape(cout, cs, ks, ks).cpu()
    ref_b, mag_b = dyd.sum(1).cpu(), dyd.abs().sum(1).cpu()
    saved = _modes(ops, True, True)
    try:
        dw, db = ops.conv2d_wgrad(dy, x, ks, want_bias=True)
        dw2, db2 = ops.conv2d_wgrad(dy, x, ks, want_bias=True)
    finally:
        ops.WGRAD_SLAB[0], ops.DETERMINISTIC[0] = saved
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    _close_sum(dw, ref_w, mag_w, 'dw')
    _close_sum(db, ref_b, mag_b, 'db')
