"""NaN and Inf activations through the forward kernels, against torch's own operators (tests/nonfinite_cases.py has the
table, the planting and the comparison; tests/test_nonfinite_cpu.py holds the references to "can show a failure").

Every table case asks the launcher's own plan which path the call takes and asserts the path it is named for, runs the
kernel on the planted input and holds the NaN / +Inf / -Inf patterns to the float64 reference exactly, the finite rest to
the project's gate.  Behind the table: MaskPre (statistics, pooling, argmax, the four backward forms), the ReLU looking
backward (autograd's threshold_backward: the gradient passes at y = NaN), the three losses, and the ReLU by itself.

Out of scope: void and padding taps of the gather kernels, the bf16x3 mode, non-finite boxes / offsets.
conv2d(mask=...) never splits its K loop (no entry point takes a mask and a workspace), so the mask branches of the
split-K reduce are not reachable from a call."""
import pytest
import torch
import torch.nn.functional as F

import mask_pre_cases as mc
import nonfinite_cases as nf
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu
NAN, INF = nf.NAN, nf.INF
FLT_MAX, DENORM = 3.4028234663852886e38, 1.401298464324817e-45


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


@pytest.mark.parametrize('case', nf.CASES, ids=[c.id for c in nf.CASES])
def test_forward_kernel_keeps_torchs_nonfinite_pattern(ops, case):
    inp = case.inputs()
    if case.plan is not None:
        case.plan(ops, inp)
    ref32, ref64 = case.refs()
    got = case.run(ops, nf.to_dev(inp))
    torch.cuda.synchronize()
    err, ref_err, scale = nf.assert_same_nonfinite(got, ref32, ref64, case.id)
    print(f'{case.id}: patterns equal ({int(torch.isnan(ref64).sum())} NaN, {int((ref64 == INF).sum())} +Inf); finite part '
          f'|product - f64| {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')


def test_group_norm_nan_poisons_exactly_its_group(ops):
    N, C, G, H, W = 3, 12, 3, 7, 9
    x = torch.randn(N, C, H, W, generator=nf.gen(500))
    x[1, 6, 3, 4] = NAN            # sample 1, group 1 (channels 4..7)
    g, b = torch.rand(C, generator=nf.gen(501)) + 0.5, torch.randn(C, generator=nf.gen(502))
    got = ops.group_norm(x.cuda(), g.cuda(), b.cuda(), G, 1e-5, relu=True).cpu()
    want = torch.zeros(N, C, H, W, dtype=torch.bool)
    want[1, 4:8] = True
    assert torch.equal(torch.isnan(got), want)
    ref = [F.relu(F.group_norm(x.to(dt), G, g.to(dt), b.to(dt), 1e-5)) for dt in (torch.float32, torch.float64)]
    nf.assert_same_nonfinite(got, ref[0], ref[1], 'group_norm, one NaN')


# ------------------------------------------------------------------------------------------------ MaskPre
def _bn_ref(x, rm, rv, dt):
    """(mean, biased var, running_mean, running_var) as F.batch_norm(training=True) leaves them."""
    rm, rv = rm.to(dt).clone(), rv.to(dt).clone()
    F.batch_norm(x.to(dt), rm, rv, None, None, True, 0.1, 1e-5)
    xd = x.to(dt).transpose(0, 1).reshape(x.shape[1], -1)
    return xd.mean(1), xd.var(1, unbiased=False), rm, rv


@pytest.mark.parametrize('N,form', [(4, 'plain'), (17, 'split')])
def test_bn_stats_nonfinite_channel_has_batch_norms_pattern(ops, N, form):
    """Channel 1 holds a NaN, channel 3 a +Inf, channel 4 a -Inf: mean, var and the running statistics of those channels
    have F.batch_norm's classes, the other channels hold to it at the gate.  17 images: the split form (16 or more)."""
    C, H, W = 6, 7, 8
    assert (N >= 16) == (form == 'split')
    x = torch.randn(N, C, H, W, generator=nf.gen(510 + N)) * 1.5 + 0.3
    x[2, 1, 3, 3], x[0, 3, 2, 5], x[N - 1, 4, 4, 2] = NAN, INF, -INF
    rm0, rv0 = torch.randn(C, generator=nf.gen(511)), torch.rand(C, generator=nf.gen(512)) + 0.5
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, var = ops.bn_stats(x.cuda(), rm, rv, 0.1)
    r32, r64 = _bn_ref(x, rm0, rv0, torch.float32), _bn_ref(x, rm0, rv0, torch.float64)
    assert bool(torch.isnan(r64[1][[1, 3, 4]]).all()) and bool(torch.isfinite(r64[1][[0, 2, 5]]).all())
    for name, got, a, b in zip(('mean', 'var', 'running_mean', 'running_var'), (mean, var, rm, rv), r32, r64):
        nf.assert_same_nonfinite(got, a, b, f'bn_stats {form} {name}')


@pytest.mark.parametrize('H,W', nf.POOL_MAPS)
def test_bn_relu_maxpool_argmax_reports_torchs_index_on_nan_windows(ops, H, W):
    """Every window that holds a NaN reports the index max_pool2d(return_indices=True) reports (the last NaN in scan
    order); every window whose fp32 maximum is unique reports that one."""
    inp = nf.pool_case(H, W).inputs()
    x = inp['x'].clone()
    x[0, 1, 3, 3] = NAN            # a second NaN in a window of the first: the LATER one is reported
    inp = dict(inp, x=x)
    dev = nf.to_dev(inp)
    arg = ops.bn_relu_maxpool_argmax(dev['x'], dev['mean'], dev['var'], dev['gamma'], dev['beta'], 1e-5).cpu().long()
    val, idx = nf.pool_ref(inp, torch.float32)
    nanw = torch.isnan(val)
    assert int(nanw.sum()) >= 4
    assert torch.equal(arg[nanw], idx[nanw]), 'a window with a NaN reports another tap than max_pool2d'
    # window (1, 1) of that plane holds the NaN at (2, 2) and the one at (3, 3): the later one is reported
    assert int(idx[0, 1, 1, 1]) == 3 * W + 3 and int(arg[0, 1, 1, 1]) == 3 * W + 3
    z = F.relu(F.batch_norm(x, inp['mean'], inp['var'], inp['gamma'], inp['beta'], False, 0.1, 1e-5))
    taken = z.flatten(2).gather(2, arg.clamp(min=0).flatten(2)).view_as(val)
    pos = ~nanw & (val > 0)
    assert torch.equal(taken[pos], val[pos]), 'a reported tap does not hold the window\'s maximum'


# (N, C, H, W) -> which backward form (tests/test_bwd_gpu.py::test_bn_relu_maxpool_forward_and_backward_odd_shapes), asserted
# through the launcher's own plan.  The 64 channels of the sums-kernel shapes stand for "as many as that route needs on this
# device" (64 at 256 compute units): the count is asked of the plan.
BWD_SHAPES = [(16, 64, 12, 20, 'sums kernel, 2x2 blocks'), (17, 64, 7, 12, 'sums kernel, element form'), (3, 5, 10, 6, 'plane in LDS'),
              (2, 7, 7, 9, 'atomic scatter'), (16, 3, 7, 9, 'atomic scatter + split BatchNorm backward')]


@pytest.mark.parametrize('N,C,H,W,form', BWD_SHAPES, ids=[s[4] for s in BWD_SHAPES])
def test_bn_relu_maxpool_backward_with_a_poisoned_channel(ops, N, C, H, W, form):
    """One NaN pixel in channel 1, train-mode statistics from bn_stats: out, gx and gamma.grad of that channel are all NaN, as
    autograd's.  beta.grad of that channel is NOT NaN in autograd: it is the sum of the pooled gradients, which max_pool2d
    routes to each window's last NaN tap and threshold_backward passes there -- a finite number, and the kernel must give
    that number (a kernel that blocks the gradient at a NaN maximum gives 0).  Every other channel holds to autograd at the
    existing gate (tests/test_bwd_gpu.py: 1e-5 forward, 1e-4 gradients)."""
    if form.startswith('sums kernel'):
        C = mc.sums_channels(ops)
    assert mc.route(ops, 'bwd', N, C, H, W) == mc.BWD_FORMS[form], form
    x = torch.randn(N, C, H, W, generator=nf.gen(520)) * 1.5 + 0.3
    x[N - 1, 1, H - 3, 2] = NAN
    gamma, beta = torch.rand(C, generator=nf.gen(521)) + 0.5, torch.randn(C, generator=nf.gen(522)) * 0.2
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.max_pool2d(F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5)), 3, 2, 1)
    go = torch.randn(y.shape, generator=nf.gen(523))
    y.backward(go)
    assert bool(torch.isnan(y[:, 1]).all() and torch.isnan(xr.grad[:, 1]).all() and torch.isnan(gr.grad[1]))
    assert bool(torch.isfinite(br.grad[1])) and abs(float(br.grad[1])) > 0.1
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    mean, var = ops.bn_stats(xd)
    out = ops.bn_relu_maxpool(xd, mean, var, gd, bd, 1e-5).cpu()
    gx, gg, gb = (t.cpu() for t in ops.bn_relu_maxpool_backward(xd, mean, var, gd, bd, go.cuda(), 1e-5))
    for name, t in (('out', out[:, 1]), ('gx', gx[:, 1]), ('gamma.grad', gg[1])):
        assert bool(torch.isnan(t).all()), f'{form}: {name} of the poisoned channel is not all NaN ({int(torch.isnan(t).sum())} of {t.numel()})'
    torch.testing.assert_close(gb[1], br.grad[1], atol=1e-4, rtol=1e-4)
    others = [c for c in range(C) if c != 1]
    torch.testing.assert_close(out[:, others], y.detach()[:, others], atol=1e-5, rtol=1e-5)
    for name, got, ref in (('gx', gx[:, others], xr.grad[:, others]), ('gamma.grad', gg[others], gr.grad[others]),
                           ('beta.grad', gb[others], br.grad[others])):
        assert bool(torch.isfinite(got).all()), f'{form}: {name} of a clean channel is not finite'
        torch.testing.assert_close(got, ref, atol=1e-4, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ the ReLU looking backward
def _relu_backward_ref(y, g):
    """F.relu(...).backward in float64: threshold_backward zeroes the gradient where the output is <= 0, so it passes at NaN."""
    yr = y.double().clone().requires_grad_(True)
    F.relu(yr).backward(g.double())
    return yr.grad


def _relu_output_with_nans(shape, seed):
    y = torch.randn(shape, generator=nf.gen(seed)).clamp(min=0)            # a ReLU output: half zeros
    flat = y.view(-1)
    for i in (1, flat.numel() // 3, flat.numel() // 2 + 1, flat.numel() - 1):
        flat[i] = NAN
    flat[2] = -0.0
    return y


@pytest.mark.parametrize('n', [4096, 4099])
def test_relu_backward_passes_the_gradient_at_nan(ops, n):
    """n % 4 == 0 on an aligned tensor: the 16-byte form; n odd: the scalar one."""
    y = _relu_output_with_nans((n,), 530)
    g = torch.randn(n, generator=nf.gen(531))
    ref = _relu_backward_ref(y, g)
    assert bool((ref[torch.isnan(y)] == g.double()[torch.isnan(y)]).all()) and bool((ref[y == 0] == 0).all())
    got = ops.relu_backward_(g.clone().cuda(), y.cuda()).cpu()
    assert torch.equal(got.double(), ref), f'{int((got.double() != ref).sum())} gradients differ from threshold_backward'


@pytest.mark.parametrize('cout,build', [(37, nf.B64), (36, nf.BTAIL)], ids=['store_all', 'tail'])
def test_conv2d_mask_passes_the_gradient_at_nan(ops, cout, build):
    srcs, NB, H, W = [12], 4, 14, 14
    rec, = ops.conv2d_plan(srcs, NB, H, W, cout, 3, has_mask=True)
    assert nf._bm(rec) == build and rec['ksplit'] == 1, rec
    x = torch.randn(NB, 12, H, W, generator=nf.gen(540))
    w = torch.randn(cout, 12, 3, 3, generator=nf.gen(541)) / 108 ** 0.5
    y = _relu_output_with_nans((NB, cout, H, W), 542)
    y[:, cout - 1, 5, 5] = NAN                    # (36 couts: the last four rows are the TAIL epilogue's)
    got = ops.conv2d(x.cuda(), ops.pack_conv_weight(w.cuda()), None, cout, 3, mask=y.cuda()).cpu()
    g32, g64 = F.conv2d(x, w, padding=1), F.conv2d(x.double(), w.double(), padding=1)
    ref64 = _relu_backward_ref(y, g64)
    ref32 = torch.where(y <= 0, torch.zeros(()), g32)
    nan = torch.isnan(y)
    assert bool((ref64[nan] == g64[nan]).all()) and bool((ref64[nan] != 0).all())
    assert torch.equal(got == 0, ref64 == 0), 'the mask zeroes other outputs than threshold_backward'
    assert_close_via_f64(got, ref32, ref64, f'conv2d mask {cout} couts')


# ------------------------------------------------------------------------------------------------ losses
def test_losses_return_nan_for_one_nan_input(ops):
    """What makes a divergence visible: one NaN logit / prediction gives a NaN loss."""
    g = nf.gen(550)
    N, S = 5, 14
    ml = F.softmax(torch.randn(N, 4, generator=g), dim=1)
    ip, dp = torch.randn(N, S, S, generator=g), torch.randn(N, S, S, generator=g)
    it, dt = (torch.rand(N, S, S, generator=g) > 0.5).float(), (torch.rand(N, S, S, generator=g) > 0.7).float()
    for which in ('inst', 'det'):
        a, b = ip.clone(), dp.clone()
        (a if which == 'inst' else b)[2, 6, 7] = NAN
        terms, grad_ml = torch.zeros(2, device='cuda'), torch.zeros(N, 4, device='cuda')
        ops.mask_loss_stage(a.cuda(), b.cuda(), it.cuda(), dt.cuda(), ml.cuda(), 0, 0.7, terms, grad_ml, True)
        assert bool(torch.isnan(terms[0 if which == 'inst' else 1])), f'mask_loss_stage: a NaN {which} logit left the loss {terms.tolist()}'
    s = torch.randn(7, 11, generator=g)
    s[3, 4] = NAN
    labels = torch.randint(0, 11, (7,), generator=g)
    loss, _, _ = ops.softmax_ce(s.cuda(), labels.cuda(), None, 1.0 / 7)
    assert bool(torch.isnan(loss)), f'softmax_ce: a NaN score left the loss {float(loss)}'
    nc = 5
    pred, tgt, w = torch.randn(6, nc * 4, generator=g), torch.randn(6, 4, generator=g), torch.ones(6, 4)
    lab = torch.tensor([0, 1, 2, 3, 4, 2])
    pred.view(6, nc, 4)[1, 1, 2] = NAN            # row 1 is positive with class 1: the loss reads this column
    loss, _ = ops.l1_loss_pos(pred.cuda(), lab.cuda(), tgt.cuda(), w.cuda(), nc, 1.0 / 6)
    assert bool(torch.isnan(loss)), f'l1_loss_pos: a NaN prediction left the loss {float(loss)}'


# ------------------------------------------------------------------------------------------------ the ReLU by itself
def test_relu_by_itself_value_for_value(ops):
    """A 1 -> 1 channel 1x1 conv2d with weight 1, no bias, relu=True is the epilogue's ReLU alone: torch.relu value for
    value (-0 == +0), NaN at the NaN."""
    vals = [NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, FLT_MAX, -FLT_MAX, DENORM, -DENORM]
    x = torch.zeros(1, 1, 3, 4)
    x.view(-1)[:len(vals)] = torch.tensor(vals)
    assert float(x.view(-1)[9]) == DENORM                                  # (the CPU kept the denormal)
    got = ops.conv2d(x.cuda(), ops.pack_conv_weight(torch.ones(1, 1, 1, 1, device='cuda')), None, 1, 1, relu=True).cpu()
    ref = torch.relu(x)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and int(torch.isnan(got).sum()) == 1
    keep = ~torch.isnan(ref)
    assert torch.equal(got[keep], ref[keep]), (got.view(-1).tolist(), ref.view(-1).tolist())
