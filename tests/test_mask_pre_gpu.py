"""The kernels of csrc/mask_pre.hip -- train-mode BatchNorm statistics, the fused BatchNorm -> ReLU -> MaxPool(3, 2, 1)
forward, its argmax diagnostic and its backward -- on every route their launchers can take, against float64.

Every case names the route it is meant to reach and asserts it through the launchers' own plan (ops.mask_pre_plan) before
it runs; `test_the_cases_reach_every_build_the_routes_can_name` holds the union of those routes to ops.MASK_PRE_BUILDS, so a
build that loses its last case, or a new build without one, fails.  Inputs and references: tests/mask_pre_cases.py (x on a
grid of 1/8, so that the tap every window takes is a property of the input: nothing is left out of any comparison, ties
included).  Every comparison goes through tolerances.assert_close_via_f64: the product may be as far from float64 autograd
as fp32 autograd itself is, or 1e-4 of the tensor's scale."""
import pytest
import torch
import torch.nn.functional as F

import mask_pre_cases as mc
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu
EPS = mc.EPS
LDS_LIMIT = 64 * 1024
SUMS, CSTAR = mc.SUMS, 'C*'          # C*: the smallest channel count that takes the sums route on this device (mc.sums_channels)
ROWS, GENERIC = [('fwd_rows', 0, 0)], [('fwd', 0, 0)]
PLAIN_STATS = [('stats', 0, 0)]
SPLIT_STATS = {vec: [('stats_split', 0, vec), ('stats_split', 1, vec), ('stats_finalize', 0, 0)] for vec in (0, 1)}
LDS_PLAIN, LDS_SPLIT = mc.BWD_FORMS['plane in LDS'], mc.BWD_FORMS['plane in LDS + split BatchNorm backward']
SCATTER_PLAIN, SCATTER_SPLIT = mc.BWD_FORMS['atomic scatter'], mc.BWD_FORMS['atomic scatter + split BatchNorm backward']


def _sums(even, pre):
    return [(SUMS, even, pre)] + mc.SUMS_BN


# id: (NB, C, H, W), the routes of the statistics, the forward and the backward (None: whichever the plan names)
CASES = {
    'forward rows, one block per plane': ((2, 3, 12, 20), PLAIN_STATS, ROWS, LDS_PLAIN),
    'forward rows, odd H': ((2, 3, 7, 12), PLAIN_STATS, ROWS, LDS_PLAIN),
    'forward rows, two blocks, ragged last': ((1, 2, 66, 64), PLAIN_STATS, ROWS, LDS_PLAIN),
    'forward generic, odd W; backward atomic scatter': ((2, 7, 7, 9), PLAIN_STATS, GENERIC, SCATTER_PLAIN),
    'forward generic, W = 2': ((2, 3, 6, 2), PLAIN_STATS, GENERIC, LDS_PLAIN),
    'forward generic, 65536 outputs a plane': ((1, 1, 512, 512), PLAIN_STATS, GENERIC, SCATTER_PLAIN),
    'backward sums, 2x2 blocks, prefetch': ((16, CSTAR, 12, 20), SPLIT_STATS[1], ROWS, _sums(1, 1)),
    'backward sums, 2x2 blocks, every prefetch slot full': ((16, CSTAR, 64, 64), SPLIT_STATS[1], ROWS, _sums(1, 1)),
    'backward sums, element form, prefetch': ((17, CSTAR, 7, 12), SPLIT_STATS[1], ROWS, _sums(0, 1)),
    'backward sums, 2x2 blocks, no prefetch': ((16, CSTAR, 66, 64), SPLIT_STATS[1], ROWS, _sums(1, 0)),
    'backward sums, element form, no prefetch': ((16, CSTAR, 65, 68), SPLIT_STATS[1], ROWS, _sums(0, 0)),
    'backward plane in LDS, one-workgroup BN backward': ((3, 5, 10, 6), PLAIN_STATS, ROWS, LDS_PLAIN),
    'backward plane in LDS, split BN backward': ((16, 4, 12, 20), SPLIT_STATS[1], ROWS, LDS_SPLIT),
    'backward plane in LDS, workgroups walk several planes': ((15, 300, 2, 2), PLAIN_STATS, GENERIC, LDS_PLAIN),
    'backward atomic scatter, split BN backward': ((16, 3, 7, 9), SPLIT_STATS[0], GENERIC, SCATTER_SPLIT),
    'backward plane too large for LDS': ((1, 2, 112, 112), PLAIN_STATS, ROWS, SCATTER_PLAIN),
    'backward the 64 KiB plane': ((16, CSTAR, 1, 8192), SPLIT_STATS[1], ROWS, None),
}
# the statistics by themselves: (images, H, W) -> route.  7 x 8 = 56 elements take the vector loop of the split form, 7 x 9 = 63 its
# scalar loop; 16, 17 and 31 images make splits of one image, of one or two, and of two (one of one)
STATS_C = 6
STATS_CASES = {(n, h, w): (PLAIN_STATS if n < 16 else SPLIT_STATS[int(h * w % 4 == 0)]) for n in (4, 15, 16, 17, 31) for h, w in ((7, 8), (7, 9))}
# the forms compared bit for bit (test_*_same_bits_*): id -> (shape, aligned route, route of the copy one float into a buffer)
FORWARD_PAIR = ((2, 3, 12, 20), ROWS, GENERIC)
BACKWARD_PAIRS = {
    'plane in LDS': ((3, 5, 10, 6), LDS_PLAIN, SCATTER_PLAIN),
    'sums, 2x2 blocks': ((16, CSTAR, 12, 20), _sums(1, 1), SCATTER_SPLIT),
    'sums, element form': ((17, CSTAR, 7, 12), _sums(0, 1), SCATTER_SPLIT),
}


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


def _shape(ops, shape):
    return tuple(mc.sums_channels(ops) if v == CSTAR else v for v in shape)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _assert_routes(ops, shape, stats, fwd, bwd, **kw):
    """The case's routes, asserted through the plan; returns the backward's records."""
    assert mc.route(ops, 'stats', *shape, **kw) == stats, ('stats', shape)
    assert mc.route(ops, 'fwd', *shape, **kw) == fwd, ('fwd', shape)
    recs = ops.mask_pre_plan('bwd', *shape, **kw)
    assert bwd is None or mc.route(ops, 'bwd', *shape, **kw) == bwd, ('bwd', shape, mc.route(ops, 'bwd', *shape, **kw))
    assert all(0 <= r['lds_bytes'] <= LDS_LIMIT for r in recs), recs
    return recs


def _run(ops, inp, momentum=0.1):
    d = {k: v.cuda() for k, v in inp.items()}
    rm, rv = d['rm'].clone(), d['rv'].clone()
    mean, var = ops.bn_stats(d['x'], rm, rv, momentum)
    out = ops.bn_relu_maxpool(d['x'], mean, var, d['gamma'], d['beta'], EPS)
    gx, gg, gb = ops.bn_relu_maxpool_backward(d['x'], mean, var, d['gamma'], d['beta'], d['go'], EPS)
    torch.cuda.synchronize()
    return dict(out=out, grad_x=gx, grad_gamma=gg, grad_beta=gb, mean=mean, var=var, running_mean=rm, running_var=rv)


@pytest.mark.parametrize('case', list(CASES), ids=[c.replace(' ', '_') for c in CASES])
def test_block_against_float64_on_its_route(ops, case):
    shape, stats, fwd, bwd = CASES[case]
    shape = _shape(ops, shape)
    recs = _assert_routes(ops, shape, stats, fwd, bwd)
    if case == 'backward plane in LDS, workgroups walk several planes':
        assert recs[0]['grid_x'] < shape[0] * shape[1]
    if case == 'backward the 64 KiB plane':
        assert 4 * (8192 + 2 * 4096) == LDS_LIMIT and recs[0]['kernel'] != ops.MASK_PRE_KERNELS.index('pool_scatter')
    r32, r64 = mc.reference(*shape)
    inp = mc.inputs(*shape)
    got = _run(ops, inp)
    for name in ('mean', 'var', 'running_mean', 'running_var', 'out', 'grad_x', 'grad_gamma', 'grad_beta'):
        err, ref_err, scale = assert_close_via_f64(got[name], r32[name], r64[name], f'{case}: {name}')
        print(f'{case} {shape} {name}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
    print(f'{case} {shape}: {r64["tied_share"]:.1%} of the windows that pass a gradient hold a tie')
    # a window whose maximum is zero passes nothing, and the choice of tap is exact: the gradient lands on the reference's pixels
    assert torch.equal(got['out'].cpu() > 0, r64['out'] > 0)
    # the routes without atomics give the same bits on every run
    if 'pool_scatter' not in [ops.MASK_PRE_KERNELS[r['kernel']] for r in recs]:
        again = _run(ops, inp)
        for name in ('mean', 'var', 'out', 'grad_x', 'grad_gamma', 'grad_beta'):
            assert torch.equal(_bits(got[name]), _bits(again[name])), f'{case}: {name} differs between two runs'


def test_the_cases_reach_every_build_the_routes_can_name(ops):
    reached = {op: set() for op in ops.MASK_PRE_OPS}

    def add(op, shape, want, **kw):
        got = mc.route(ops, op, *shape, **kw)
        assert want is None or got == want, (op, shape, kw, got)
        reached[op] |= {(ops.MASK_PRE_KERNELS.index(k), p0, p1, 0) for k, p0, p1 in got}

    for shape, stats, fwd, bwd in CASES.values():
        for op, want in (('stats', stats), ('fwd', fwd), ('bwd', bwd)):
            add(op, _shape(ops, shape), want)
    for (n, h, w), want in STATS_CASES.items():
        add('stats', (n, STATS_C, h, w), want)
    add('fwd', FORWARD_PAIR[0], FORWARD_PAIR[2], aligned=False)
    for shape, _, second in BACKWARD_PAIRS.values():
        add('bwd', _shape(ops, shape), second, aligned=False)
    for op in ops.MASK_PRE_OPS:
        assert reached[op] == ops.MASK_PRE_BUILDS[op], (op, sorted(ops.MASK_PRE_BUILDS[op] - reached[op]), sorted(reached[op] - ops.MASK_PRE_BUILDS[op]))


# ------------------------------------------------------------------------------------------------ the same bits across forms
GUARD = -777.0


def _one_float_in(t, pad=8):
    """(buffer, view): a contiguous copy of t that starts one float into a larger buffer -- 4-byte aligned and no more -- with
    guard elements before and after it"""
    buf = torch.full((t.numel() + 1 + pad,), GUARD, device='cuda')
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return buf, view


def _guards_untouched(buf, n):
    return bool((buf[0] == GUARD).item()) and bool((buf[1 + n:] == GUARD).all().item())


def _fwd_into(ops, x, mean, var, gamma, beta, out, eps=EPS):
    NB, C, H, W = x.shape
    ops.check(ops.lib().dm_bn_relu_maxpool_fwd(ops._p(x), NB, C, H, W, ops._p(mean), ops._p(var), ops._p(gamma), ops._p(beta), eps, ops._p(out),
                                              ops._stream()), 'dm_bn_relu_maxpool_fwd')


def _bwd_into(ops, x, mean, var, gamma, beta, go, gx, eps=EPS):
    NB, C, H, W = x.shape
    gg, gb = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    ops.check(ops.lib().dm_bn_relu_maxpool_bwd(ops._p(x), NB, C, H, W, ops._p(mean), ops._p(var), ops._p(gamma), ops._p(beta), eps, ops._p(go),
                                              ops._p(gx), ops._p(gg), ops._p(gb), ops._p(ops._bn_scratch(x.device, C)), ops._stream()),
              'dm_bn_relu_maxpool_bwd')
    return gg, gb


def test_rows_and_generic_forward_give_the_same_bits(ops):
    """One input through the rows kernel (a fresh allocation) and, copied one float into a larger buffer, through the generic
    kernel: the plan names the scalar route for a pointer with 4 bytes of alignment, `out` has the same bits, and the guard
    elements around the misaligned input and output are untouched."""
    shape, first, second = FORWARD_PAIR
    assert mc.route(ops, 'fwd', *shape) == first and mc.route(ops, 'fwd', *shape, aligned=False) == second
    d = {k: v.cuda() for k, v in mc.inputs(*shape).items()}
    mean, var = ops.bn_stats(d['x'])
    out = ops.bn_relu_maxpool(d['x'], mean, var, d['gamma'], d['beta'], EPS)
    xbuf, xv = _one_float_in(d['x'])
    obuf, ov = _one_float_in(torch.zeros_like(out))
    _fwd_into(ops, xv, mean, var, d['gamma'], d['beta'], ov)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ov), _bits(out))
    assert _guards_untouched(xbuf, xv.numel()) and _guards_untouched(obuf, ov.numel()) and torch.equal(_bits(xv), _bits(d['x']))
    # the statistics of the misaligned copy: the scalar loop or the one-workgroup kernel, the values of the reference
    r32, r64 = mc.reference(*shape)
    m2, v2 = ops.bn_stats(xv)
    assert_close_via_f64(m2, r32['mean'], r64['mean'], 'mean of the misaligned copy')
    assert_close_via_f64(v2, r32['var'], r64['var'], 'var of the misaligned copy')


@pytest.mark.parametrize('pair', list(BACKWARD_PAIRS), ids=[p.replace(' ', '_') for p in BACKWARD_PAIRS])
def test_plane_kernels_and_the_scalar_route_give_the_same_pooling_adjoint(ops, pair):
    """The gather forms (plane in LDS; the sums kernel's 2 x 2 blocks and its element form) against the atomic scatter, which a
    copy of the input one float into a larger buffer takes (the plan with aligned=False names it; guards around the
    misaligned x and grad_x stay untouched).  Observed through grad_x, with numbers that make every sum exact so that the
    order of additions cannot show: x and grad_out on a grid of 1/8, mean 0, var 1 and eps 0 (xhat = x, products are
    multiples of 1/64, every partial sum far below 2^24 / 64).  Both routes end in the same BatchNorm backward expression,
    so equal adjoints give equal bits, and an adjoint routed to another tap of a tie does not."""
    shape, first, second = BACKWARD_PAIRS[pair]
    shape = _shape(ops, shape)
    assert mc.route(ops, 'bwd', *shape) == first and mc.route(ops, 'bwd', *shape, aligned=False) == second
    NB, C, H, W = shape
    inp = mc.inputs(*shape)
    x, gamma, beta = inp['x'].cuda(), inp['gamma'].cuda(), inp['beta'].cuda()
    go = (torch.randint(-16, 17, inp['go'].shape, generator=mc.gen(77)).float() / 8).cuda()
    mean, var = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    gx = torch.empty_like(x)
    gg, gb = _bwd_into(ops, x, mean, var, gamma, beta, go, gx, eps=0.0)
    xbuf, xv = _one_float_in(x)
    gbuf, gv = _one_float_in(torch.zeros_like(x))
    gg2, gb2 = _bwd_into(ops, xv, mean, var, gamma, beta, go, gv, eps=0.0)
    torch.cuda.synchronize()
    assert _guards_untouched(xbuf, x.numel()) and _guards_untouched(gbuf, x.numel()) and torch.equal(_bits(xv), _bits(x))
    assert torch.equal(_bits(gb), _bits(gb2)) and torch.equal(_bits(gg), _bits(gg2))
    assert torch.equal(_bits(gx), _bits(gv)), f'{int((_bits(gx) != _bits(gv)).sum())} of {gx.numel()} elements of grad_x differ'
    # and both are autograd's numbers: float64 of the same affine block (batch_norm in eval mode with these statistics)
    refs = []
    for dt in (torch.float32, torch.float64):
        xr, gr, br = (t.cpu().to(dt).requires_grad_(True) for t in (x, gamma, beta))
        z = F.relu((xr - 0.0) * 1.0 * gr.view(1, -1, 1, 1) + br.view(1, -1, 1, 1))
        F.max_pool2d(z, 3, 2, 1).backward(go.cpu().to(dt))
        refs.append((gr.grad, br.grad))
    # (grad_x of the kernel is train-mode BatchNorm's; with these statistics only the parameter gradients are autograd's)
    assert_close_via_f64(gg, refs[0][0], refs[1][0], f'{pair}: grad_gamma')
    assert_close_via_f64(gb, refs[0][1], refs[1][1], f'{pair}: grad_beta')


# ------------------------------------------------------------------------------------------------ the statistics by themselves
def _stats_ref(x, rm, rv, momentum, dt):
    rm, rv = rm.to(dt).clone(), rv.to(dt).clone()
    F.batch_norm(x.to(dt), rm, rv, None, None, True, momentum, EPS)
    flat = x.to(dt).transpose(0, 1).reshape(x.shape[1], -1)
    return dict(mean=flat.mean(1), var=flat.var(1, unbiased=False), running_mean=rm, running_var=rv)


@pytest.mark.parametrize('momentum', (0.1, 0.3))
@pytest.mark.parametrize('N,H,W', list(STATS_CASES), ids=[f'{n}x{h}x{w}' for n, h, w in STATS_CASES])
def test_bn_stats_against_float64(ops, N, H, W, momentum):
    """mean, biased variance and the running statistics (unbiased variance, the momentum given) of both forms and both loops
    of the split form; then `mean_shift`: the running mean moves as it does for x + shift[c], nothing else moves."""
    shape = (N, STATS_C, H, W)
    assert mc.route(ops, 'stats', *shape) == STATS_CASES[(N, H, W)]
    g = mc.gen(950 + N + H * W)
    x = torch.randn(shape, generator=g) * 1.5 + torch.randn(1, STATS_C, 1, 1, generator=g)
    rm0, rv0, shift = torch.randn(STATS_C, generator=g), torch.rand(STATS_C, generator=g) + 0.5, torch.randn(STATS_C, generator=g) * 2
    r32, r64 = (_stats_ref(x, rm0, rv0, momentum, dt) for dt in (torch.float32, torch.float64))
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, var = ops.bn_stats(x.cuda(), rm, rv, momentum)
    got = dict(mean=mean, var=var, running_mean=rm, running_var=rv)
    for name in got:
        err, ref_err, scale = assert_close_via_f64(got[name], r32[name], r64[name], f'bn_stats {shape} {name}')
        print(f'bn_stats {shape} momentum {momentum} {name}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
    xs = x + shift.view(1, -1, 1, 1)
    s32, s64 = (_stats_ref(xs, rm0, rv0, momentum, dt) for dt in (torch.float32, torch.float64))
    assert float((s64['running_mean'] - r64['running_mean']).abs().min()) > 1e-3       # the shift shows in the reference
    rm2, rv2 = rm0.cuda(), rv0.cuda()
    mean2, var2 = ops.bn_stats(x.cuda(), rm2, rv2, momentum, mean_shift=shift.cuda())
    assert torch.equal(_bits(mean2), _bits(mean)) and torch.equal(_bits(var2), _bits(var)) and torch.equal(_bits(rv2), _bits(rv))
    err, ref_err, scale = assert_close_via_f64(rm2, s32['running_mean'], s64['running_mean'], f'bn_stats {shape} running_mean, shifted')
    print(f'bn_stats {shape} momentum {momentum} running_mean with mean_shift: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
    assert_close_via_f64(rv2, s32['running_var'], s64['running_var'], f'bn_stats {shape} running_var, shifted')


@pytest.mark.parametrize('N,H,W', [(4, 7, 8), (17, 7, 8), (17, 7, 9)], ids=['plain', 'split-vector', 'split-scalar'])
def test_bn_stats_variance_of_offset_data_is_two_pass(ops, N, H, W):
    """x = 100 + 0.1 N(0, 1): the variance is 1e-6 of the mean's square.  The two-pass form (mean, then centred squares) keeps it
    to fp32 rounding; E[x^2] - mean^2 in fp32 loses it (asserted of a restatement here: more than 1 % off).  The triangle's
    gate, 2e-4 of the variance, separates the two."""
    assert mc.route(ops, 'stats', N, STATS_C, H, W) == STATS_CASES[(N, H, W)]
    x = 100 + 0.1 * torch.randn(N, STATS_C, H, W, generator=mc.gen(960 + N))
    r32, r64 = (_stats_ref(x, torch.zeros(STATS_C), torch.ones(STATS_C), 0.1, dt) for dt in (torch.float32, torch.float64))
    assert float(((r32['var'].double() - r64['var']) / r64['var']).abs().max()) < 1e-5
    flat = x.transpose(0, 1).reshape(STATS_C, -1)
    one_pass = (flat * flat).mean(1) - flat.mean(1) ** 2
    with pytest.raises(AssertionError):
        assert_close_via_f64(one_pass, r32['var'], r64['var'], 'the one-pass variance')
    assert float(((one_pass.double() - r64['var']) / r64['var']).abs().max()) > 0.01
    mean, var = ops.bn_stats(x.cuda())
    for name, got in (('mean', mean), ('var', var)):
        err, ref_err, scale = assert_close_via_f64(got, r32[name], r64[name], f'offset data {name}')
        print(f'bn_stats offset data {(N, STATS_C, H, W)} {name}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')


# ------------------------------------------------------------------------------------------------ the argmax diagnostic
@pytest.mark.parametrize('shape', [(2, 3, 12, 20), (2, 7, 7, 9), (1, 2, 66, 64), (2, 3, 6, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_argmax_reports_torchs_indices_on_every_window_that_passes_a_gradient(ops, shape):
    r32, r64 = mc.reference(*shape)
    d = {k: v.cuda() for k, v in mc.inputs(*shape).items()}
    mean, var = ops.bn_stats(d['x'])
    arg = ops.bn_relu_maxpool_argmax(d['x'], mean, var, d['gamma'], d['beta'], EPS).cpu().long()
    out = ops.bn_relu_maxpool(d['x'], mean, var, d['gamma'], d['beta'], EPS)
    positive = r64['out'] > 0
    assert int(positive.sum()) > 0.9 * positive.numel()
    assert torch.equal(arg[positive], r64['idx'][positive]), 'a window reports another tap than max_pool2d(return_indices=True)'
    assert int(arg.min()) >= 0 and int(arg.max()) < shape[2] * shape[3]
    # out is relu(bn(x)) at the reported taps
    inp = mc.inputs(*shape)
    g32, g64 = (mc.activation(inp, dt).flatten(2).gather(2, arg.flatten(2)).view_as(out) for dt in (torch.float32, torch.float64))
    err, ref_err, scale = assert_close_via_f64(out, g32, g64, f'out at the reported taps {shape}')
    print(f'argmax {shape}: out at the reported taps err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
