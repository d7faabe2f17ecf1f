"""The loss, optimiser and layout kernels of the training step, each against a plain float64 restatement on the CPU (the
same restatement in float32 is the third corner of the triangle of tests/tolerances.py): dm_mask_loss_stage,
dm_class_balance_fwd_bwd, dm_gumbel_select_fwd / _bwd, dm_softmax_ce_fwd_bwd, dm_l1_loss_fwd_bwd, dm_bbox_encode,
dm_sgd_momentum_step, dm_sumsq / dm_clip_scale / dm_scale, dm_upsample2x_nearest_fwd / _bwd, dm_pixel_unshuffle2x,
dm_threshold_ge and dm_mask_target_rois -- at row counts that are no multiple of 256, 64 or 4, class counts either side
of a wave, zero normalisers, saturated logits, the class-agnostic column and the accumulation across stages, none of
which the one-shape end-to-end goldens reach."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model
from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

CANARY = 7.0
GUARD = 4096
INVALID_ARG = -1            # DM_ERR_INVALID_ARG of include/dynamask_hip.h


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t):
    return t.detach().cuda().contiguous()


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


class Guarded:
    """A device tensor of ``shape`` between two guard bands of CANARY."""

    def __init__(self, shape, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), CANARY, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == CANARY).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == CANARY).all()), f'{what}: the guard band past the output was overwritten'


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ mask_loss_stage
STAGES = 4
DETAIL_W = (0.5, 0.7, 1.0, 1.3)


def _stage_ref(ip, dp, it, dt, ml, col, detail_w, dtype):
    """One stage of DynaCrossEntropyLoss (cross_entropy_loss.py:455-466): terms[0] = mean BCE-with-logits,
    terms[1] += detail_w * N / (sum_n w_n + 1e-5) * mask_cross_entropy(dp, dt, w) with the normaliser detached; the
    gradients by autograd with w = mask_labels[:, col] as a leaf."""
    ip, dp = ip.detach().clone().to(dtype).requires_grad_(True), dp.detach().clone().to(dtype).requires_grad_(True)
    w = ml[:, col].detach().clone().to(dtype).requires_grad_(True)
    N = ip.shape[0]
    t0 = F.binary_cross_entropy_with_logits(ip, it.to(dtype), reduction='none').mean()
    t1 = detail_w * N / (w.detach().sum() + 1e-5) * ref_model.mask_cross_entropy(dp, dt.to(dtype), w.view(-1, 1, 1))
    gi, = torch.autograd.grad(t0, ip)
    gd, gw = torch.autograd.grad(t1, (dp, w))
    return t0.detach(), t1.detach(), gi, gd, gw


def _mask_labels(N, kind, g):
    if kind == 'onehot':
        return F.one_hot(torch.randint(0, STAGES, (N,), generator=g), STAGES).float()
    ml = F.softmax(torch.randn(N, STAGES, generator=g) * 2.0, dim=1)
    if kind == 'zerocol':
        ml[:, 2] = 0.0
    return ml


def _stage_inputs(N, S, kind, seed):
    g = _g(seed)
    ml = _mask_labels(N, kind, g)
    stages = []
    for s in range(STAGES):
        it = (torch.rand(N, S, S, generator=g) > 0.5).float()
        dt = (torch.rand(N, S, S, generator=g) > 0.7).float()
        ip = torch.randn(N, S, S, generator=g) * (1.0 + s)            # distinct BCE per stage: terms[0] is overwritten
        dp = torch.randn(N, S, S, generator=g) * 3.0                  # sigma = 3: sigmoid within 1e-4 of 0 and 1
        stages.append((ip, dp, it, dt))
    return ml, stages


def _run_stages(ops, ml, stages, want_inst=lambda s: True):
    N = ml.shape[0]
    mld = _dev(ml)
    terms = Guarded((2,), torch.zeros(2))
    grad_ml = Guarded((N, STAGES), torch.zeros(N, STAGES))
    outs, terms_after = [], []
    for s, (ip, dp, it, dt) in enumerate(stages):
        gi, gd = ops.mask_loss_stage(_dev(ip), _dev(dp), _dev(it), _dev(dt), mld, s, DETAIL_W[s], terms.t, grad_ml.t,
                                     want_inst(s))
        outs.append((gi, gd))
        terms_after.append(terms.t.cpu().clone())
    terms.check('loss_terms')
    grad_ml.check('grad_ml')
    assert torch.equal(mld.cpu(), ml), 'mask_labels was modified'
    return terms_after, grad_ml.t.cpu().clone(), outs


@pytest.mark.parametrize('kind', ['soft', 'onehot', 'zerocol'])
@pytest.mark.parametrize('N,S', [(300, 14), (5, 28), (3, 5), (1, 56)])
def test_mask_loss_stage(ops, N, S, kind):
    ml, stages = _stage_inputs(N, S, kind, 7 * N + S)
    terms_after, grad_ml, outs = _run_stages(ops, ml, stages)
    r32 = [_stage_ref(*st, ml, s, DETAIL_W[s], torch.float32) for s, st in enumerate(stages)]
    r64 = [_stage_ref(*st, ml, s, DETAIL_W[s], torch.float64) for s, st in enumerate(stages)]
    name = f'mask_loss_stage N={N} S={S} {kind}'
    seen = []             # (|product - f64| max, the fp32 reference's own error, scale, what) of every triangle comparison
    for s in range(STAGES):
        # terms[0] is the stage's own mean BCE (overwritten), terms[1] the sum of the detail terms so far (accumulated)
        e0 = assert_close_via_f64(terms_after[s][0:1], r32[s][0].reshape(1), r64[s][0].reshape(1), f'{name} terms[0] after stage {s}')
        acc32, acc64 = sum(r[1] for r in r32[:s + 1]), sum(r[1] for r in r64[:s + 1])
        if float(acc64) != 0.0:
            e1 = assert_close_via_f64(terms_after[s][1:2], acc32.reshape(1), acc64.reshape(1), f'{name} terms[1] after stage {s}')
            seen.append((*e1, f'terms[1] after stage {s}'))
        else:
            assert float(terms_after[s][1]) == 0.0
        seen.append((*e0, f'terms[0] of stage {s}'))
        gi, gd = outs[s]
        assert _finite(gi, gd)
        assert_grad_close(gi, r64[s][2], f'{name} grad_inst stage {s}', rel=1e-4)
        zero_w = bool((ml[:, s] == 0).all())
        assert_grad_close(gd, r64[s][3], f'{name} grad_det stage {s}', rel=1e-4, zero=zero_w)
        # each grad_ml column is its own stage's (a sum over the pixels of a RoI: the triangle)
        eg = assert_close_via_f64(grad_ml[:, s], r32[s][4], r64[s][4], f'{name} grad_ml[:, {s}]')
        seen.append((*eg, f'grad_ml[:, {s}]'))
    # the four BCEs differ by far more than the tolerance, so "the last stage's alone" is a real statement
    bces = [float(r[0]) for r in r64]
    assert min(abs(bces[3] - b) for b in bces[:3]) > 0.05 * bces[3]
    assert _finite(grad_ml, *terms_after)
    err, ref_err, scale, what = max(seen, key=lambda e: e[0] / (max(e[1], 1e-4 * min(e[2], 1.0)) + 1e-4 * e[2]))
    print(f'{name}: nearest to its bound is {what}: |product - f64| {err:.3g}, allowed {max(ref_err, 1e-4 * min(scale, 1.0)):.3g} '
          f'+ 1e-4 |f64| (fp32 reference {ref_err:.3g}, scale {scale:.3g})')


def test_mask_loss_stage_without_inst_grad(ops):
    ml, stages = _stage_inputs(5, 28, 'soft', 99)
    ta, ga, oa = _run_stages(ops, ml, stages)
    tb, gb, ob = _run_stages(ops, ml, stages, want_inst=lambda s: False)
    for s in range(STAGES):
        assert ob[s][0] is None and oa[s][0] is not None
        assert torch.equal(oa[s][1], ob[s][1]) and torch.equal(ta[s], tb[s])
    assert torch.equal(ga, gb)


def test_mask_loss_stage_saturated_logits(ops):
    """Detail logit +40 on target 0 and -40 on target 1: sigmoid is 1 / ~4e-18 in float32, the eps-BCE's per-pixel loss is
    -log(1e-10f) for both, and the +40 gradient is exactly 0 (s * (1 - s) == 0)."""
    N, S = 2, 5
    ml = torch.tensor([[1.0, 0, 0, 0], [0.5, 0.5, 0, 0]])
    dp = torch.stack([torch.full((S, S), 40.0), torch.full((S, S), -40.0)])
    dt = torch.stack([torch.zeros(S, S), torch.ones(S, S)])
    ip = torch.stack([torch.full((S, S), 40.0), torch.full((S, S), -40.0)])
    it = torch.stack([torch.zeros(S, S), torch.zeros(S, S)])
    terms, grad_ml = torch.zeros(2, device='cuda'), torch.zeros(N, 4, device='cuda')
    gi, gd = ops.mask_loss_stage(_dev(ip), _dev(dp), _dev(it), _dev(dt), _dev(ml), 0, 0.7, terms, grad_ml, True)
    assert _finite(gi, gd, terms, grad_ml)
    assert float(gd[0].abs().max()) == 0.0, 'logit +40 on target 0: the gradient is exactly 0'
    r32 = _stage_ref(ip, dp, it, dt, ml, 0, 0.7, torch.float32)
    r64 = _stage_ref(ip, dp, it, dt, ml, 0, 0.7, torch.float64)
    assert_close_via_f64(terms.cpu(), torch.stack(r32[:2]), torch.stack(r64[:2]), 'saturated terms')
    assert_close_via_f64(grad_ml[:, 0].cpu(), r32[4], r64[4], 'saturated grad_ml')
    # known answers: every pixel costs L = -log(1e-10f); terms[1] = w * sum_n ml_n L / den, grad_ml[n] = w * L / den
    L = -np.log(np.float64(np.float32(1e-10)))
    den = 1.5 + 1e-5
    known = torch.tensor([0.7 * L * 1.5 / den, 0.7 * L / den, 0.7 * L / den], dtype=torch.float64)
    got = torch.stack([terms[1], grad_ml[0, 0], grad_ml[1, 0]]).cpu()
    assert_close_via_f64(got, known.float(), known, 'saturated known answers')


def test_dyna_loss_composition_against_float64(ops):
    """DynaCrossEntropyLoss through the registry at N = 300 with odd map sizes against autograd of ref_model.dyna_loss in
    float64: the stage kernel, class_balance and the stage / class-balance weights together."""
    from dynamask_amd import losses, registry  # noqa: F401
    N, sizes, g = 300, (7, 13, 20, 9), _g(41)
    dw, cbw, start = [0.5, 0.7, 1.1, 1.3], 0.8, 2
    mod = registry.build_loss(dict(type='DynaCrossEntropyLoss', stage_instance_loss_weight=[1.0, 1.0, 1.0],
                                   stage_detail_loss_weight=dw, cb_loss_weight=cbw, start_stage=start)).cuda()
    tgts, ips, dps = [], [], []
    for S in sizes:
        yy, xx = torch.meshgrid(torch.arange(S).float(), torch.arange(S).float(), indexing='ij')
        c = torch.rand(N, 2, generator=g) * S
        r = (0.2 + 0.3 * torch.rand(N, generator=g)) * S
        t = (((yy[None] - c[:, 0, None, None]) ** 2 + (xx[None] - c[:, 1, None, None]) ** 2) < r[:, None, None] ** 2).float()
        tgts.append(t)
        ips.append(((t * 2 - 1) * 1.5 + torch.randn(N, S, S, generator=g)).unsqueeze(1))
        dps.append((torch.randn(N, S, S, generator=g) * 2.0).unsqueeze(1))
    ml = F.softmax(torch.randn(N, 4, generator=g) * 2.0 + torch.linspace(-1, 1, 4), dim=1)

    def ref(dtype):
        i_ = [t.detach().clone().to(dtype).requires_grad_(True) for t in ips]
        d_ = [t.detach().clone().to(dtype).requires_grad_(True) for t in dps]
        m_ = ml.detach().clone().to(dtype).requires_grad_(True)
        loss = ref_model.dyna_loss(i_, d_, tgts, m_, stage_detail_loss_weight=dw, cb_loss_weight=cbw, start_stage=start)
        loss.backward()
        return loss.detach(), m_.grad, [t.grad for t in i_], [t.grad for t in d_]
    l32, m32, _, _ = ref(torch.float32)
    l64, m64, i64, d64 = ref(torch.float64)
    i_d = [_dev(t).requires_grad_(True) for t in ips]
    d_d = [_dev(t).requires_grad_(True) for t in dps]
    m_d = _dev(ml).requires_grad_(True)
    loss = mod(i_d, d_d, [_dev(t) for t in tgts], m_d)['loss_masks']
    loss.backward()
    assert_close_via_f64(loss.detach().reshape(1), l32.reshape(1), l64.reshape(1), 'dyna loss')
    assert_grad_close(m_d.grad, m64, 'd loss / d mask_labels', rel=1e-4)
    for s in range(4):
        assert_grad_close(d_d[s].grad, torch.zeros(1) if d64[s] is None else d64[s], f'detail pred {s}', rel=1e-4, zero=s > start)
        assert_grad_close(i_d[s].grad, torch.zeros(1) if i64[s] is None else i64[s], f'instance pred {s}', rel=1e-4, zero=s != start)


# ------------------------------------------------------------------------------------------------ class_balance
def _cb_ref(ml, dtype):
    m = ml.detach().clone().to(dtype).requires_grad_(True)
    p = m.sum(0) / m.sum()
    cb = (p * torch.log(p + 1e-10)).sum()
    cb.backward()
    return cb.detach(), m.grad


@pytest.mark.parametrize('zero_col', [False, True])
@pytest.mark.parametrize('N,K', [(1, 4), (300, 4), (257, 3), (7, 8)])
def test_class_balance(ops, N, K, zero_col):
    ml = F.softmax(torch.randn(N, K, generator=_g(N + K)) * 2.0 + torch.linspace(-1, 1, K), dim=1)
    if zero_col:
        ml[:, K // 2] = 0.0
    cb, grad = ops.class_balance(_dev(ml))
    assert _finite(cb, grad)
    (c32, g32), (c64, g64) = _cb_ref(ml, torch.float32), _cb_ref(ml, torch.float64)
    assert_close_via_f64(cb.reshape(1), c32.reshape(1), c64.reshape(1), f'class_balance {N}x{K}')
    assert_grad_close(grad, g64, f'class_balance grad {N}x{K}', rel=1e-4)
    assert torch.equal(grad, grad[:1].expand_as(grad)), 'the gradient is the same for every RoI'


def test_class_balance_one_hot_rows(ops):
    """What training feeds it: one-hot rows with an exit that is never chosen (p = 0 exactly)."""
    ml = F.one_hot(torch.tensor([0, 1, 1, 3, 1, 0, 3] * 43), 4).float()
    cb, grad = ops.class_balance(_dev(ml))
    (c32, _), (c64, g64) = _cb_ref(ml, torch.float32), _cb_ref(ml, torch.float64)
    assert _finite(cb, grad)
    assert_close_via_f64(cb.reshape(1), c32.reshape(1), c64.reshape(1), 'class_balance one-hot')
    assert_grad_close(grad, g64, 'class_balance one-hot grad', rel=1e-4)


def test_class_balance_refuses_nine_columns(ops):
    from dynamask_amd._lib import lib
    ml = torch.rand(5, 9, device='cuda')
    loss, grad = torch.zeros(1, device='cuda'), torch.zeros(5, 9, device='cuda')
    assert lib().dm_class_balance_fwd_bwd(ops._p(ml), 5, 9, ops._p(loss), ops._p(grad), ops._stream()) == INVALID_ARG
    with pytest.raises(RuntimeError):
        ops.class_balance(ml)


# ------------------------------------------------------------------------------------------------ gumbel_select
def _gumbel_soft(logits, U, T, dtype):
    lg, U = logits.to(dtype), U.to(dtype)
    g = -torch.log(-torch.log(U + 1e-20) + 1e-20)
    return F.softmax((lg + g) / T, dim=-1)


@pytest.mark.parametrize('T', [0.5, 1.0])
@pytest.mark.parametrize('K', [2, 4])
@pytest.mark.parametrize('N', [1, 65, 300])
def test_gumbel_select_forward_and_backward(ops, N, K, T):
    g = _g(100 * N + 10 * K + int(T * 2))
    logits = torch.randn(N, K, generator=g) * 1.5
    U = torch.rand(N, K, generator=g)
    logits[0], U[0] = 0.3, 0.25                          # every column equal: the first maximum is column 0
    if N > 1:
        logits[1], U[1] = -5.0, 0.5
        logits[1, K - 2:] = 2.0                          # the last two columns tie at the top: K - 2 wins
    y, hot, idx = ops.gumbel_select(_dev(logits), _dev(U), T)
    y32, y64 = _gumbel_soft(logits, U, T, torch.float32), _gumbel_soft(logits, U, T, torch.float64)
    assert_close_via_f64(y, y32, y64, f'gumbel y_soft {N}x{K} T={T}')
    yc = y.cpu()
    assert float(yc[0].max()) == float(yc[0].min()), 'equal logits and noise must give equal probabilities'
    first_max = torch.from_numpy(np.argmax(yc.numpy(), axis=1))          # numpy: the first of equal maxima
    assert torch.equal(idx.cpu().long(), first_max)
    assert int(idx[0]) == 0 and (N == 1 or int(idx[1]) == K - 2)
    assert torch.equal(hot.cpu(), F.one_hot(first_max, K).float())
    # backward of the soft branch: autograd of softmax((logits + g) / T) in float64
    gy = torch.randn(N, K, generator=g)
    lg64 = logits.double().requires_grad_(True)
    _gumbel_soft(lg64, U, T, torch.float64).backward(gy.double())
    assert_grad_close(ops.gumbel_select_backward(y, _dev(gy), T), lg64.grad, f'gumbel backward {N}x{K} T={T}', rel=1e-4)


def test_gumbel_select_refuses_nine_columns(ops):
    from dynamask_amd._lib import lib
    a, b, c = (torch.rand(5, 9, device='cuda') for _ in range(3))
    idx = torch.zeros(5, dtype=torch.int32, device='cuda')
    assert lib().dm_gumbel_select_fwd(ops._p(a), ops._p(b), 5, 9, 0.5, ops._p(c), ops._p(c.clone()), ops._p(idx),
                                      ops._stream()) == INVALID_ARG
    assert lib().dm_gumbel_select_bwd(ops._p(a), ops._p(b), 5, 9, 0.5, ops._p(c), ops._stream()) == INVALID_ARG
    with pytest.raises(RuntimeError):
        ops.gumbel_select(a, b, 0.5)
    with pytest.raises(RuntimeError):
        ops.gumbel_select_backward(a, b, 0.5)


# ------------------------------------------------------------------------------------------------ softmax_ce
MIN_GAP = 1e-3


def _ce_inputs(N, C, seed):
    g = _g(seed)
    s = torch.randn(N, C, generator=g) * 3.0
    top = s.topk(2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < 10 * MIN_GAP
    s[close, top.indices[close, 0]] += 0.1              # float32 and float64 then agree on every argmax
    top = s.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= MIN_GAP
    labels = torch.where(torch.rand(N, generator=g) < 0.5, s.argmax(1), torch.randint(0, C, (N,), generator=g))
    labels[0] = C - 1 if N == 1 else 0
    labels[-1] = C - 1
    w = torch.rand(N, generator=g) + 0.5
    w[torch.rand(N, generator=g) < 0.3] = 0.0
    if N > 1:
        w[0], w[1] = 0.0, 1.25
    return s, labels, w


def _ce_ref(s, labels, w, scale, dtype):
    sr = s.detach().clone().to(dtype).requires_grad_(True)
    ce = F.cross_entropy(sr, labels, reduction='none')
    loss = (ce if w is None else ce * w.to(dtype)).sum() * scale
    loss.backward()
    acc = (s.argmax(1) == labels).to(dtype).sum() * torch.tensor(100.0 / s.shape[0], dtype=dtype)
    return loss.detach(), acc, sr.grad


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('N,C', [(1, 2), (3, 64), (5, 65), (1025, 81), (6, 1204)])
def test_softmax_ce(ops, N, C, weighted):
    s, labels, w = _ce_inputs(N, C, 31 * N + C)
    w = w if weighted else None
    scale = 1.7 / N
    wd = None if w is None else _dev(w)
    loss, acc, grad = ops.softmax_ce(_dev(s), _dev(labels), wd, scale)
    (l32, a32, _), (l64, a64, g64) = _ce_ref(s, labels, w, scale, torch.float32), _ce_ref(s, labels, w, scale, torch.float64)
    name = f'softmax_ce {N}x{C} weighted={weighted}'
    assert _finite(loss, acc, grad)
    if float(l64) != 0.0:
        assert_close_via_f64(loss.reshape(1), l32.reshape(1), l64.reshape(1), f'{name} loss')
    else:
        assert float(loss) == 0.0
    if float(a64) != 0.0:
        assert_close_via_f64(acc.reshape(1), a32.reshape(1), a64.reshape(1), f'{name} accuracy')
    else:
        assert float(acc) == 0.0
    if float(g64.abs().max()) != 0.0:
        assert_grad_close(grad, g64, f'{name} grad', rel=1e-4)
    else:
        assert float(grad.abs().max()) == 0.0
    loss2, acc2, none = ops.softmax_ce(_dev(s), _dev(labels), wd, scale, need_grad=False)
    assert none is None and torch.equal(loss2, loss) and torch.equal(acc2, acc)
    if weighted:
        zero = w == 0
        assert float(grad.cpu()[zero].abs().max() if bool(zero.any()) else 0.0) == 0.0, 'a zero-weight row has a gradient'
        # ... and adds exactly 0 to the loss: other logits in those rows leave every bit of it
        s2 = s.clone()
        s2[zero] = torch.randn(int(zero.sum()), C, generator=_g(5)) * 5.0
        loss3, _, _ = ops.softmax_ce(_dev(s2), _dev(labels), wd, scale, need_grad=False)
        assert torch.equal(loss3, loss)


def test_softmax_ce_huge_logits_stay_finite(ops):
    s = torch.randn(3, 65, generator=_g(8))
    s[0, 5], s[0, 64] = 1e4, -1e4
    s[1, 5], s[1, 64] = 1e4, -1e4
    labels = torch.tensor([5, 64, 2])
    loss, acc, grad = ops.softmax_ce(_dev(s), _dev(labels), None, 0.5)
    assert _finite(loss, acc, grad)
    (l32, a32, _), (l64, a64, g64) = _ce_ref(s, labels, None, 0.5, torch.float32), _ce_ref(s, labels, None, 0.5, torch.float64)
    assert_close_via_f64(loss.reshape(1), l32.reshape(1), l64.reshape(1), 'huge logits loss')
    assert_grad_close(grad, g64, 'huge logits grad', rel=1e-4)
    assert_close_via_f64(acc.reshape(1), a32.reshape(1), a64.reshape(1), 'huge logits accuracy')


def test_softmax_ce_tie_takes_the_lowest_index(ops):
    """An exact tie at the top: the kernel's prediction is the lowest index among the maxima (within a lane's strided
    scan and across the lanes), the rule in ops.softmax_ce's docstring."""
    s = torch.randn(4, 81, generator=_g(9)).clamp(max=2.0)
    s[0, 3] = s[0, 67] = 5.0          # the same lane (3 and 3 + 64)
    s[1, 3] = s[1, 67] = 5.0
    s[2, 70] = s[2, 5] = 5.0          # two lanes
    s[3, 70] = s[3, 5] = 5.0
    labels = torch.tensor([3, 67, 5, 70])
    w = torch.tensor([1.0, 0.0, 0.0, 0.0])
    for lab, want in ((labels, 50.0), (torch.tensor([67, 67, 70, 70]), 0.0), (torch.tensor([3, 3, 5, 5]), 100.0)):
        _, acc, _ = ops.softmax_ce(_dev(s), _dev(lab), _dev(w), 1.0, need_grad=False)
        assert float(acc) == want


# ------------------------------------------------------------------------------------------------ l1_loss_pos
def _l1_ref(pred, labels, tgt, w, num_classes, scale, dtype):
    p = pred.detach().clone().to(dtype).requires_grad_(True)
    N, nb = p.shape[0], p.shape[1] // 4
    pos = (labels >= 0) & (labels < num_classes)
    col = labels[pos] if nb > 1 else torch.zeros_like(labels[pos])
    sel = p.view(N, nb, 4)[pos, col]
    loss = ((sel - tgt.to(dtype)[pos]).abs() * w.to(dtype)[pos]).sum() * scale
    loss.backward()
    return loss.detach(), p.grad, pos, col


@pytest.mark.parametrize('N', [1, 257, 600])
@pytest.mark.parametrize('nb', [80, 1])
def test_l1_loss_pos(ops, nb, N):
    nc, g = 80, _g(3 * N + nb)
    pred = torch.randn(N, nb * 4, generator=g)
    labels = torch.randint(-1, nc + 1, (N,), generator=g)            # -1 negative, nc background, the rest positive
    labels[0] = nc - 1
    if N > 2:
        labels[1], labels[2] = nc, -1
    tgt = torch.randn(N, 4, generator=g)
    w = torch.rand(N, 4, generator=g) + 0.5
    w[torch.rand(N, 4, generator=g) < 0.2] = 0.0
    w[0] = 1.0
    pred.view(N, nb, 4)[0, (nc - 1) if nb > 1 else 0, 1] = tgt[0, 1]      # pred == target: the gradient is 0, not +-1
    scale = 1.3 / N
    loss, grad = ops.l1_loss_pos(_dev(pred), _dev(labels), _dev(tgt), _dev(w), nc, scale)
    (l32, _, _, _), (l64, g64, pos, col) = (_l1_ref(pred, labels, tgt, w, nc, scale, dt) for dt in (torch.float32, torch.float64))
    assert_close_via_f64(loss.reshape(1), l32.reshape(1), l64.reshape(1), f'l1 loss N={N} nb={nb}')
    assert_grad_close(grad, g64, f'l1 grad N={N} nb={nb}', rel=1e-4)
    gc = grad.cpu().view(N, nb, 4)
    outside = torch.ones(N, nb, dtype=torch.bool)
    outside[pos.nonzero().flatten(), col] = False
    assert float(gc[outside].abs().max() if bool(outside.any()) else 0.0) == 0.0, 'a gradient outside the positive rows\' class columns'
    assert float(gc[0, (nc - 1) if nb > 1 else 0, 1]) == 0.0 and float(gc[0, (nc - 1) if nb > 1 else 0, 0]) != 0.0
    loss2, none = ops.l1_loss_pos(_dev(pred), _dev(labels), _dev(tgt), _dev(w), nc, scale, need_grad=False)
    assert none is None and torch.equal(loss2, loss)
    # no positive row: the loss is exactly 0
    neg = torch.where(torch.arange(N) % 2 == 0, torch.full((N,), nc), torch.full((N,), -1))
    loss0, grad0 = ops.l1_loss_pos(_dev(pred), _dev(neg), _dev(tgt), _dev(w), nc, scale)
    assert float(loss0) == 0.0 and float(grad0.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ bbox_encode
def _bbox2delta64(p, g, means, stds):
    p, g = p.double(), g.double()
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    d = torch.stack([((g[:, 0] + g[:, 2]) * 0.5 - (p[:, 0] + p[:, 2]) * 0.5) / pw,
                     ((g[:, 1] + g[:, 3]) * 0.5 - (p[:, 1] + p[:, 3]) * 0.5) / ph,
                     torch.log((g[:, 2] - g[:, 0]) / pw), torch.log((g[:, 3] - g[:, 1]) / ph)], dim=-1)
    return (d - torch.tensor(means, dtype=torch.float64)) / torch.tensor(stds, dtype=torch.float64)


@pytest.mark.parametrize('N', [1, 255, 257])
def test_bbox_encode(ops, N):
    g = _g(N)

    def boxes():
        xy = torch.rand(N, 2, generator=g) * 200
        wh = torch.rand(N, 2, generator=g) * 95 + 5
        return torch.cat([xy, xy + wh], 1)
    p, gt = boxes(), boxes()
    means, stds = (0.1, -0.2, 0.05, 0.3), (0.1, 0.1, 0.2, 0.2)
    got = ops.bbox_encode(_dev(p), _dev(gt), means, stds)
    assert_close_via_f64(got, ref_model.bbox2delta(p, gt, means, stds), _bbox2delta64(p, gt, means, stds), f'bbox_encode N={N}')


# ------------------------------------------------------------------------------------------------ optimiser and norm
@pytest.mark.parametrize('count', [1, 255, 257, 4096 * 256 + 3])
def test_sgd_momentum_step(ops, count):
    """torch.optim.SGD's arithmetic: d = g * grad_scale + wd * p; buf = d on the first step, then momentum * buf + d;
    p -= lr * buf.  (The triangle, not bits: the build may contract a multiply-add.)"""
    g = _g(count % 1000)
    p0 = torch.randn(count, generator=g)
    grads = [torch.randn(count, generator=g), torch.randn(count, generator=g)]
    lr, mom, wd, gs = 0.02, 0.9, 1e-4, 0.5

    def ref(dtype):
        p, buf, out = p0.to(dtype), None, []
        for i, gr in enumerate(grads):
            d = gr.to(dtype) * gs + wd * p
            buf = d if i == 0 else mom * buf + d
            p = p - lr * buf
            out.append((p.clone(), buf.clone()))
        return out
    r32, r64 = ref(torch.float32), ref(torch.float64)
    pd = Guarded((count,), p0)
    md = Guarded((count,), torch.full((count,), float('nan')))            # the first step must not read the buffer
    for i, gr in enumerate(grads):
        gd = _dev(gr)
        ops.sgd_momentum_step_(pd.t, gd, md.t, lr, mom, wd, gs, first_step=(i == 0))
        pd.check('params')
        md.check('momentum')
        assert torch.equal(gd.cpu(), gr), 'the gradient was modified'
        assert_close_via_f64(pd.t, r32[i][0], r64[i][0], f'sgd params step {i} count={count}')
        assert_close_via_f64(md.t, r32[i][1], r64[i][1], f'sgd momentum step {i} count={count}')


@pytest.mark.parametrize('count', [0, 1, 255, 16384, 16385, 1024 * 16384 + 3])
def test_sumsq(ops, count):
    x = torch.randn(count, generator=_g(count % 977)) * 0.7
    xd = _dev(x)
    a, b = ops.sumsq(xd), ops.sumsq(xd)
    assert torch.equal(a, b), 'fixed-order sum: two runs must give the same bits'
    if count == 0:
        assert float(a) == 0.0
        return
    assert_close_via_f64(a, (x * x).sum().reshape(1), (x.double() * x.double()).sum().reshape(1), f'sumsq count={count}')


def test_clip_scale(ops):
    max_norm = 1.0
    small = torch.randn(1003, generator=_g(1)) * 0.01               # norm ~0.3 < max_norm: every bit stays
    sd = _dev(small)
    ops.clip_scale_(sd, ops.sumsq(sd), max_norm)
    assert torch.equal(sd.cpu(), small)
    big = torch.randn(1003, generator=_g(2))                         # norm ~32
    bd = Guarded((1003,), big)
    ops.clip_scale_(bd.t, ops.sumsq(bd.t), max_norm)
    bd.check('clip_scale_')

    def ref(dtype):
        b = big.to(dtype)
        return b * (max_norm / (torch.sqrt((b * b).sum()) + 1e-6))
    assert_close_via_f64(bd.t, ref(torch.float32), ref(torch.float64), 'clip_scale_')


def test_scale(ops):
    x = torch.randn(1003, generator=_g(3))
    xd = Guarded((1003,), x)
    ops.scale_(xd.t, 0.37)
    xd.check('scale_')
    assert torch.equal(xd.t.cpu(), x * torch.tensor(0.37, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ layout kernels: bits
LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 5, 13, 9)]         # odd H and W; N*C*H*W no multiple of 256


@pytest.mark.parametrize('shape', LAYOUT_SHAPES)
def test_upsample2x_nearest_and_backward(ops, shape):
    N, C, H, W = shape
    assert (N * C * H * W) % 256 != 0
    x = torch.randn(*shape, generator=_g(H))
    assert torch.equal(ops.upsample2x_nearest(_dev(x)).cpu(), F.interpolate(x, scale_factor=2, mode='nearest'))
    go = torch.randn(N, C, 2 * H, 2 * W, generator=_g(W))
    want = (go[..., 0::2, 0::2] + go[..., 0::2, 1::2]) + (go[..., 1::2, 0::2] + go[..., 1::2, 1::2])      # the kernel's order
    assert torch.equal(ops.upsample2x_nearest_backward(_dev(go)).cpu(), want)


@pytest.mark.parametrize('shape', LAYOUT_SHAPES)
def test_pixel_unshuffle2x(ops, shape):
    """out[n, (dy*2+dx)*C + c, y, x] = in[n, c, 2y+dy, 2x+dx] (include/dynamask_hip.h): the sub-pixel index is the SLOW
    channel index -- not torch's pixel_unshuffle, where it is the fast one."""
    N, C, H, W = shape
    x = torch.randn(N, C, 2 * H, 2 * W, generator=_g(H + W))
    want = x.view(N, C, H, 2, W, 2).permute(0, 3, 5, 1, 2, 4).reshape(N, 4 * C, H, W)
    got = ops.pixel_unshuffle2x(_dev(x)).cpu()
    assert torch.equal(got, want)
    if C > 1:
        assert not torch.equal(got, F.pixel_unshuffle(x, 2))


@pytest.mark.parametrize('thr', [0.5, 0.3])
def test_threshold_ge_on_the_threshold(ops, thr):
    t = np.float32(thr)
    x = torch.randn(3, 5, 7, generator=_g(4))
    x.view(-1)[:3] = torch.tensor([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))])
    x.view(-1)[-1] = float(t)
    got = ops.threshold_ge(_dev(x), thr).cpu()
    assert torch.equal(got, (x >= torch.tensor(t)).float())
    assert got.view(-1)[:3].tolist() == [1.0, 0.0, 1.0] and float(got.view(-1)[-1]) == 1.0


@pytest.mark.parametrize('N', [1, 65, 300])
def test_mask_target_rois(ops, N):
    g = _g(N)
    boxes = torch.randn(N, 4, generator=g) * 150 + 100             # below 0 and beyond the image on every side
    boxes[0] = torch.tensor([-3.0, 0.0, 319.0, 400.0])             # exactly on the limits
    inds = torch.randint(0, 1000, (N,), generator=g)
    max_w, max_h = 319.0, 255.0
    want = torch.stack([inds.float(), boxes[:, 0].clamp(0, max_w), boxes[:, 1].clamp(0, max_h), boxes[:, 2].clamp(0, max_w),
                        boxes[:, 3].clamp(0, max_h)], dim=1)
    assert torch.equal(ops.mask_target_rois(_dev(boxes), _dev(inds), max_w, max_h).cpu(), want)
