"""The 64-bit fixed-point accumulators of the training step (include/dynamask_hip.h, "Fixed-point accumulators") against
the float64 references of tests/fixed_point_ref.py: the LDS cells of dm_deform_col2im and of the scatter form of
dm_point_sample_bwd, and the *_fx entry points dm_channel_sum_fx, dm_point_sample_bwd_fx, dm_class_logits_bwd_fx,
dm_conv2d_wgrad_fx and dm_fx_to_float -- across the range of gradient scales (x 2^e, e in 0, -12, -24, -33, +16; the
scaling is exact in float32), and the poison rules for any number of bad addends.

The bound of every value test is per cell and derived, not tuned:

    |got - sum| <= (c * 2^-24 * A_cell + u * 2^-36 * K_cell) * (1 + 2^-20)

A_cell = sum |g * w| and K_cell = number of addends of the cell, both from the reference; the last factor covers the
second-order terms ((1 + d)^c - 1 - c d, and the final conversion's rounding of the grid error).

c counts the float32 roundings of relative size 2^-24 between a gradient and its cell; each is relative to an addend or
to a partial sum, and both are bounded by A_cell:
  * the sample position: 0 -- the reference computes it in float32 operation for operation (col2im: one addition;
    point sample: ps_coord with the two contracted multiply-adds), so kernel and reference place a sample at the same spot;
  * 1 - l per axis: 2 (l itself, position - floor, is exact);
  * the weight product: 1;
  * g * w: 1 in float32 (col2im, the gather form, direct atomics); 0 in the LDS route of the point sample, which rounds
    the exact double product;
  * col2im's merged path (H * W % 4 == 0) adds the products of two linked pixels in float32: 1;
  * the final conversion of a cell to float32: 1;
  * sums formed in float32 before the cell: the gather form adds a RoI's n <= K_cell products of a cell in sequence
    (<= K_cell roundings); a float TARGET takes one float atomic per addend of the direct route and one per RoI of an LDS
    route, each relative to the running sum (<= K_direct + R_lds); channel_sum and class_logits_backward form a
    workgroup's partial sum through a chain of `depth` additions (counted at the tests).
  So: col2im scatter() path c = 5, merged path c = 6; point sample, scatter form, fx target c = 5, float target
  c = 5 + K_direct + R_lds per cell; gather form, fx target c = 4 + K_cell.

u is the cut to the grid per addend: dm_fix36_abs16 truncates (u = 1); dm_fix36_mul truncates its low word, and at the
tie rem = 2^31 the saturating convert loses one more unit (u = 2); the __double2ll_rn paths round to nearest (u = 1/2).
At e = -33 the K term dominates: that is the contract (an ABSOLUTE resolution of 2^-36 per addend) being pinned.

Each value test prints its largest error / bound ratio.  Outputs lie between guard bands."""
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import torch

import fixed_point_ref as fr

pytestmark = pytest.mark.gpu

CANARY = 7.0
GUARD = 4096
EPS = 2.0 ** -24
GRID = 2.0 ** -36
SLACK = 1.0 + 2.0 ** -20
NAN, INF = float('nan'), float('inf')


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.detach().cuda().contiguous()


class Guarded:
    """A device tensor of ``shape`` between two guard bands of CANARY."""

    def __init__(self, shape, fill=0.0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), CANARY, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.fill_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == CANARY).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == CANARY).all()), f'{what}: the guard band past the output was overwritten'
        return self.t


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


class _flags:
    """Set ops flags for a block and restore them."""

    def __init__(self, ops, **kw):
        self.ops, self.kw = ops, kw

    def __enter__(self):
        self.saved = {k: getattr(self.ops, k)[0] for k in self.kw}
        for k, v in self.kw.items():
            getattr(self.ops, k)[0] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            getattr(self.ops, k)[0] = v


def _check_bound(got, ref, bound, what):
    """got: float32 device / host tensor; ref, bound: float64 arrays.  Returns the peak error / bound ratio."""
    got = got.detach().cpu().double().numpy()
    assert np.isfinite(got).all(), f'{what}: non-finite cells from in-range inputs'
    err = np.abs(got - ref)
    bound = bound * SLACK
    zero = bound == 0
    assert (err[zero] == 0).all(), f'{what}: a cell no addend reaches is not zero'
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f'[fixed-point ratio] {what}: peak error / bound = {ratio:.4f} (peak error {float(err.max()):.3e})')
    assert ratio <= 1.0, f'{what}: error / bound peaks at {ratio:.3f}'
    return ratio


# ------------------------------------------------------------------------------------------------ B1 col2im
@lru_cache(maxsize=None)
def _col2im_case(shape, variant):
    N, C, dg, H, W = shape
    colgrad, off = fr.col2im_inputs(shape, variant)
    return (colgrad, off) + fr.col2im_ref(colgrad, off, (N, C, H, W), dg)


@pytest.mark.parametrize('variant', fr.COL2IM_VARIANTS)
@pytest.mark.parametrize('ct,shape', [(ct, s) for ct, ss in fr.COL2IM_SHAPES.items() for s in ss], ids=str)
def test_col2im_every_build_and_both_branches_across_the_range(ops, ct, shape, variant):
    """Every CT build of dm_deform_col2im, as the launcher's own plan says the shape takes it; H * W % 4 == 0 takes the
    merged path (dm_fix36_abs16 / dm_fix36_accumulate), else scatter() (dm_fix36_mul)."""
    N, C, dg, H, W = shape
    one, = ops.backward_plan('col2im', N, C, H, W, dg)
    assert (one['kernel'], one['P0'], one['threads']) == (ops.BWD_KERNELS.index('col2im_lds'), ct, 512 if ct == 2 else 256)
    colgrad, off, s, a, k = _col2im_case(shape, variant)
    assert float(a.max()) * 2.0 ** 16 < 2.0 ** 24             # every input of every exponent is in range by construction
    merged = (H * W) % 4 == 0
    c, u = (6, 1.0) if merged else (5, 2.0)
    offd = _dev(off)
    worst = 0.0
    for e in fr.EXPONENTS:
        sc = 2.0 ** e
        out = Guarded((N, C, H, W), fill=CANARY)
        ops.deform_col2im(_dev(colgrad * np.float32(sc)), offd, (N, C, H, W), dg, out=out.t)
        got = out.check(f'col2im {shape}')
        worst = max(worst, _check_bound(got, s * sc, c * EPS * a * sc + u * GRID * k,
                                        f'col2im CT={ct} {"merged" if merged else "scatter"} {shape} {variant} e={e}'))
    print(f'[fixed-point ratio] col2im CT={ct} {shape} {variant}: worst over exponents {worst:.4f}')


# ------------------------------------------------------------------------------------------------ B2 point-sample adjoint
@lru_cache(maxsize=None)
def _ps_case(S):
    """Per-RoI references, so that a cell's float32 roundings can be counted by the route of each RoI over it."""
    rois, go = fr.ps_rois(), fr.ps_go(S)
    B, C, H, W = fr.PS_FEAT_SHAPE
    routes = [fr.ps_scatter_route(r, S, H, W, fr.PS_SCALE, B) for r in rois]
    s, a = np.zeros(fr.PS_FEAT_SHAPE), np.zeros(fr.PS_FEAT_SHAPE)
    k, k_direct, r_lds = (np.zeros(fr.PS_FEAT_SHAPE, np.int64) for _ in range(3))
    for n in range(rois.shape[0]):
        sn, an, kn = fr.point_sample_adjoint_ref(go[n:n + 1], fr.PS_FEAT_SHAPE, rois[n:n + 1], fr.PS_SCALE)
        s, a, k = s + sn, a + an, k + kn
        if routes[n] == 'direct':
            k_direct = k_direct + kn
        elif routes[n] != 'skip':
            r_lds = r_lds + (kn > 0)
    s_all, a_all, k_all = fr.point_sample_adjoint_ref(go, fr.PS_FEAT_SHAPE, rois, fr.PS_SCALE)
    assert (k_all == k).all() and np.allclose(s_all, s, rtol=0, atol=1e-12 * max(1.0, float(a.max())))
    return rois, go, routes, s, a, k, k_direct, r_lds


# the launch each case is meant to reach, asserted through ops.backward_plan: (kernel, CT, 0, accumulation: 0 float atomics, 2
# fixed point)
PS_ROUTES = {(64, 'float'): ('point_sample_scatter', 4, 0, 0), (64, 'fx'): ('point_sample_scatter', 4, 0, 2),
             (14, 'fx'): ('point_sample_gather', 4, 0, 2)}


@pytest.mark.parametrize('S,target', [(64, 'float'), (64, 'fx'), (14, 'fx')])
def test_point_sample_adjoint_scatter_and_gather_forms_across_the_range(ops, S, target):
    """S = 64 is the scatter form (the gather form's LDS need, 4 planes of S * S floats, passes 64 KB): one 80 x 100 map,
    6 channels (one full channel quad, one short), RoIs whose footprints take the LDS sub-routes with 4, 2 and 1 planes
    per pass and the direct atomics, and the corner-case RoIs.  S = 14 is the gather form."""
    rois, go, routes, s, a, k, k_direct, r_lds = _ps_case(S)
    if S == 64:
        assert {'cpp4', 'cpp2', 'cpp1', 'direct'} <= set(routes), routes
        print('[fixed-point routes] S=64: ' + ', '.join(f'{tuple(float(v) for v in r)}: {rt}' for r, rt in zip(rois, routes)))
        c = 5 + k_direct + r_lds if target == 'float' else 5
    else:
        c = 4 + k
    assert float(a.max()) * 2.0 ** 16 < 2.0 ** 25             # every running sum of every exponent is in an fx cell's range
    roisd = _dev(rois)
    worst = 0.0
    with _flags(ops, DETERMINISTIC=target == 'fx'):
        one, = ops.backward_plan('point_sample', *fr.PS_FEAT_SHAPE, rois.shape[0], S)
        assert (ops.BWD_KERNELS[one['kernel']], one['P0'], one['P1'], one['P2']) == PS_ROUTES[(S, target)]
        for e in fr.EXPONENTS:
            sc = 2.0 ** e
            god = _dev(go * np.float32(sc))
            out = Guarded(fr.PS_FEAT_SHAPE)
            ops.point_sample_backward(god, fr.PS_FEAT_SHAPE, roisd, fr.PS_SCALE, grad_feat=out.t)
            got = out.check(f'point-sample adjoint S={S}').clone()
            worst = max(worst, _check_bound(got, s * sc, c * EPS * a * sc + 0.5 * GRID * k,
                                            f'point-sample adjoint S={S} {target} target e={e}'))
            if target == 'fx':
                again = Guarded(fr.PS_FEAT_SHAPE)
                ops.point_sample_backward(god, fr.PS_FEAT_SHAPE, roisd, fr.PS_SCALE, grad_feat=again.t)
                assert torch.equal(again.check('second run'), got)
    print(f'[fixed-point ratio] point-sample adjoint S={S} {target}: worst over exponents {worst:.4f}')


# ------------------------------------------------------------------------------------------------ B3 channel_sum, class logits
def _cs_splits(NB, C, HW):
    return max(min(max(1, 2048 // C), (NB * HW + 1023) // 1024), 1)          # dm_channel_sum_fx


CS_SHAPES = [((4, 512, 28, 28), 4), ((42, 256, 14, 14), 8), ((1, 600, 56, 56), 3), ((2, 5, 3, 3), 1)]


def _cs_input(shape, strided=False, seed=0):
    NB, C, H, W = shape
    rng = np.random.RandomState(3000 + seed + C)
    if not strided:
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda(), None
    wide = torch.from_numpy(rng.standard_normal((NB, C + 8, H, W)).astype(np.float32)).cuda()
    g = wide[:, 4:4 + C]
    assert not g.is_contiguous() and g.stride(0) == (C + 8) * H * W
    return g, wide


def _cs_check(ops, g, splits, what, wide=None):
    NB, C, H, W = g.shape
    scaled = (lambda sc: g * sc) if wide is None else (lambda sc: (wide * sc)[:, 4:4 + C])
    assert _cs_splits(NB, C, H * W) == splits
    g64 = g.cpu().double().numpy()
    s, a = g64.sum(axis=(0, 2, 3)), np.abs(g64).sum(axis=(0, 2, 3))
    # a workgroup's partial sum: a thread adds its elements in sequence (with four-element loads: two levels inside a quad,
    # then the running sum), six wave-shuffle levels, three additions of the four waves' sums; + the final conversion
    depth = -(-NB * H * W // (splits * 256)) + 2 + 6 + 3 + 1
    worst = 0.0
    with _flags(ops, DETERMINISTIC=True):
        for e in fr.EXPONENTS:
            sc = 2.0 ** e
            out = Guarded((C,), fill=CANARY)
            gs = scaled(sc)
            assert gs.stride(0) == g.stride(0)
            fresh = ops.channel_sum(gs)
            ops.channel_sum(gs, out=out.t.zero_())
            got = out.check(what)
            assert torch.equal(got, fresh)
            worst = max(worst, _check_bound(got, s * sc, depth * EPS * a * sc + 0.5 * GRID * splits, f'{what} e={e}'))
    print(f'[fixed-point ratio] {what}: worst over exponents {worst:.4f}')


@pytest.mark.parametrize('shape,splits', CS_SHAPES, ids=str)
def test_channel_sum_fx_against_float64(ops, shape, splits):
    g, _ = _cs_input(shape)
    _cs_check(ops, g, splits, f'channel_sum_fx {shape} splits={splits}')


def test_channel_sum_fx_of_a_channel_slice_against_float64(ops):
    g, wide = _cs_input((3, 20, 14, 14), strided=True)
    _cs_check(ops, g, 1, 'channel_sum_fx (3, 20 of 28, 14, 14) strided', wide=wide)


def _clb_run(ops, x, wi, wd, labels, g1, g2, nc):
    N, C = x.shape[:2]
    gx = torch.empty_like(x)
    outs = [Guarded((nc, C)), Guarded((nc,)), Guarded((nc, C)), Guarded((nc,))]
    with _flags(ops, CLB_SLAB=False, DETERMINISTIC=True):
        ops.class_logits_backward(x, wi, wd, labels, g1, g2, gx, False, *[o.t for o in outs])
    return [o.check('class_logits_backward parameter gradient').clone() for o in outs]


CLB_FX_ROUTE = ('class_logits_wave', 4, 1, 2)       # 14 x 14: one quad a lane; accumulation 2: fixed point


def test_class_logits_bwd_fx_against_float64(ops):
    """The shapes of test_class_logits_backward_slab_matches_atomics_with_shared_classes: 1100 RoIs over three classes."""
    N, C, S, nc = 1100, 40, 14, 80
    g = torch.Generator().manual_seed(57)
    x = torch.randn(N, C, S, S, generator=g)
    wi, wd = torch.randn(nc, C, generator=g).cuda(), torch.randn(nc, C, generator=g).cuda()
    labels = torch.tensor([5, 17, 79])[torch.randint(0, 3, (N,), generator=g)]
    labels[1024:] = 17
    g1, g2 = torch.randn(N, 1, S, S, generator=g), torch.randn(N, 1, S, S, generator=g)
    x64 = x.double().view(N, C, S * S)
    onehot = torch.zeros(nc, N, dtype=torch.float64)
    onehot[labels, torch.arange(N)] = 1.0
    k_cls = onehot.sum(1).numpy()
    refs = []
    for gg in (g1, g2):
        g64 = gg.double().view(N, 1, S * S)
        per_roi, per_roi_a = (g64 * x64).sum(2), (g64 * x64).abs().sum(2)
        refs.append((onehot @ per_roi, onehot @ per_roi_a, onehot @ g64.sum(2)[:, 0], onehot @ g64.abs().sum(2)[:, 0]))
    # a RoI's sum of H * W = 196 products (class_logits_bwd_wave_kernel, one quad per lane): the product, four additions in
    # sequence, six wave-shuffle levels; + the final conversion
    depth = 1 + 4 + 6 + 1
    xd, ld = x.cuda(), labels.cuda()
    one, = ops.backward_plan('class_logits', N, C, S * S, nc, mode='fx')          # (what _clb_run's flags ask for)
    assert (ops.BWD_KERNELS[one['kernel']], one['P0'], one['P1'], one['P2']) == CLB_FX_ROUTE
    worst = 0.0
    for e in (0, -24):
        sc = 2.0 ** e
        got = _clb_run(ops, xd, wi, wd, ld, (g1 * sc).cuda(), (g2 * sc).cuda(), nc)
        for (w_ref, w_a, b_ref, b_a), gw, gb, name in ((refs[0], got[0], got[1], 'inst'), (refs[1], got[2], got[3], 'det')):
            worst = max(worst, _check_bound(gw, w_ref.numpy() * sc, depth * EPS * w_a.numpy() * sc + 0.5 * GRID * k_cls[:, None],
                                            f'class_logits_bwd_fx gw_{name} e={e}'))
            worst = max(worst, _check_bound(gb, b_ref.numpy() * sc, depth * EPS * b_a.numpy() * sc + 0.5 * GRID * k_cls,
                                            f'class_logits_bwd_fx gb_{name} e={e}'))
    print(f'[fixed-point ratio] class_logits_bwd_fx: worst {worst:.4f}')


# ------------------------------------------------------------------------------------------------ B4 dm_fx_to_float
def _fx_to_float(ops, fx, out, accumulate, clear, n=None):
    from dynamask_amd._lib import lib
    rc = lib().dm_fx_to_float(ops._p(fx), fx.numel() if n is None else n, ops._p(out), accumulate, clear, ops._stream())
    torch.cuda.synchronize()
    return rc


FX_CLEAN = [0, 1, -1, 2 ** 36, -2 ** 36, 3 * 2 ** 35, -5 * 2 ** 20, 2 ** 61 - 1, -(2 ** 61 - 1)]
FX_POISONED = [2 ** 61, -2 ** 61, 2 ** 61 + 1, 2 ** 62, -2 ** 62, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 5]


@pytest.mark.parametrize('clear', [0, 1])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_fx_to_float_converts_exactly_and_reads_poison(ops, accumulate, clear):
    cells = FX_CLEAN + FX_POISONED
    fx = torch.tensor(cells, dtype=torch.int64).cuda()
    out = Guarded((len(cells),), fill=3.0)
    assert _fx_to_float(ops, fx, out.t, accumulate, clear) == 0
    got = out.check('dm_fx_to_float').cpu()
    want = torch.tensor([float(Fraction(q, 2 ** 36)) for q in FX_CLEAN], dtype=torch.float64).float()      # nearest float32
    if accumulate:
        want = want + 3.0
    assert torch.equal(got[:len(FX_CLEAN)], want)
    assert bool(torch.isnan(got[len(FX_CLEAN):]).all())
    assert fx.cpu().tolist() == ([0] * len(cells) if clear else cells)


def test_fx_to_float_of_no_cells_touches_nothing(ops):
    fx = torch.tensor([5, 6], dtype=torch.int64).cuda()
    out = Guarded((2,), fill=3.0)
    assert _fx_to_float(ops, fx, out.t, 0, 1, n=0) == 0
    assert _fx_to_float(ops, None, None, 0, 1, n=0) == 0
    assert out.check('n = 0').cpu().tolist() == [3.0, 3.0] and fx.cpu().tolist() == [5, 6]
    assert _fx_to_float(ops, fx, out.t, 0, 0, n=-1) != 0


# ------------------------------------------------------------------------------------------------ B5 poison, any count
def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('shape,splits', CS_SHAPES + [((2, 256, 64, 64), 8), ((5, 400, 32, 32), 5), ((2, 1000, 32, 32), 2)], ids=str)
def test_channel_sum_fx_poison_for_any_number_of_splits(ops, shape, splits):
    """A whole channel NaN (or Inf, or mixed): one bad addend per split, k = splits = 1, 2, 3, 4, 5, 8
    ((2, 256, 64, 64) is the mask head's bias gradient: 256 channels, 8192 elements each).  A single NaN element:
    k = 1 among finite addends of both signs.  Every other channel has the bits of the clean run."""
    NB, C, H, W = shape
    assert _cs_splits(NB, C, H * W) == splits
    g, _ = _cs_input(shape, seed=1)
    with _flags(ops, DETERMINISTIC=True):
        clean = ops.channel_sum(g)
        bad = g.clone()
        bad[:, 0] = NAN
        bad[:, 1] = INF
        bad[:, 2] = -INF
        bad[:, 3] = NAN
        bad[0, 3, 0, 0] = 1.0                     # one split's sum is still NaN
        bad[NB - 1, 4, H - 1, W - 1] = NAN        # a single element
        got = ops.channel_sum(bad)
        again = ops.channel_sum(bad, out=torch.zeros(C, device='cuda'))
    torch.cuda.synchronize()
    assert bool(torch.isnan(got[:5]).all()), got[:5]
    assert bool(torch.isnan(again[:5]).all())
    assert _same_bits(got[5:], clean[5:]) and _same_bits(again[5:], clean[5:])


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 8])
def test_class_logits_bwd_fx_poison_for_any_number_of_rois(ops, k):
    """k RoIs of one class carry a NaN in g_inst: alone (class 1) and mixed with finite RoIs of both signs (class 2); the
    rows of the other classes and the detail branch keep the bits of the clean run."""
    C, S, nc = 8, 14, 6
    finite = 6
    labels = torch.tensor([1] * k + [2] * k + [2] * finite + [3] * finite + [4])
    N = labels.numel()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(k))
    labels = labels[perm]
    g = torch.Generator().manual_seed(300 + k)
    x = torch.randn(N, C, S, S, generator=g).cuda()
    wi, wd = torch.randn(nc, C, generator=g).cuda(), torch.randn(nc, C, generator=g).cuda()
    g1, g2 = torch.randn(N, 1, S, S, generator=g), torch.randn(N, 1, S, S, generator=g)
    bad = g1.clone()
    for cls in (1, 2):
        rows = torch.nonzero(labels == cls)[:k, 0]
        bad[rows, 0, 3, rows % S] = NAN
    # class 4: a single finite addend beyond an fx cell's range (2^25) in the bias sum
    bad[torch.nonzero(labels == 4)[0, 0]] = 0.0
    bad[torch.nonzero(labels == 4)[0, 0], 0, 0, 0] = 2.0 ** 25
    ld = labels.cuda()
    clean = _clb_run(ops, x, wi, wd, ld, g1.cuda(), g2.cuda(), nc)
    got = _clb_run(ops, x, wi, wd, ld, bad.cuda(), g2.cuda(), nc)
    assert bool(torch.isnan(got[0][[1, 2]]).all()) and bool(torch.isnan(got[1][[1, 2, 4]]).all()), (got[0][[1, 2]], got[1])
    assert _same_bits(got[0][[0, 3, 5]], clean[0][[0, 3, 5]]) and _same_bits(got[1][[0, 3, 5]], clean[1][[0, 3, 5]])
    assert _same_bits(got[2], clean[2]) and _same_bits(got[3], clean[3])


@pytest.mark.parametrize('value', [2.0 ** 25, 1e9, 3e38, -1e9])
@pytest.mark.parametrize('count', [1, 2])
def test_fx_cells_poison_finite_addends_beyond_their_range(ops, value, count):
    """Single finite addends of 2^25, 1e9 and 3e38 (and two of them) into an fx cell: NaN, not a saturated or wrapped
    number.  The bias sums of `count` RoIs of class 1 whose only non-zero logit gradient is `value`."""
    C, S, nc = 8, 14, 4
    labels = torch.tensor([1] * count + [2, 2, 3])
    N = labels.numel()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, C, S, S, generator=g).cuda()
    wi, wd = torch.randn(nc, C, generator=g).cuda(), torch.randn(nc, C, generator=g).cuda()
    g1, g2 = torch.randn(N, 1, S, S, generator=g), torch.randn(N, 1, S, S, generator=g)
    big = g1.clone()
    big[:count] = 0.0
    big[:count, 0, 5, 5] = value
    clean = _clb_run(ops, x, wi, wd, labels.cuda(), g1.cuda(), g2.cuda(), nc)
    got = _clb_run(ops, x, wi, wd, labels.cuda(), big.cuda(), g2.cuda(), nc)
    assert bool(torch.isnan(got[1][1])), got[1]
    assert _same_bits(got[1][[0, 2, 3]], clean[1][[0, 2, 3]]) and _same_bits(got[0][[0, 2, 3]], clean[0][[0, 2, 3]])
    # and one addend per split of a channel sum: (2, 5, 3, 3) has one split
    gch = torch.zeros(2, 5, 3, 3)
    gch[1, 2, 1, 1] = value
    gch[:, 4] = 0.25
    with _flags(ops, DETERMINISTIC=True):
        cs = ops.channel_sum(gch.cuda()).cpu()
    assert bool(torch.isnan(cs[2])) and cs[[0, 1, 3]].tolist() == [0.0, 0.0, 0.0] and float(cs[4]) == 4.5


@pytest.mark.parametrize('shape', [(4, 16, 8, 14, 14, 3), (8, 16, 8, 14, 14, 3), (16, 16, 8, 14, 14, 3)], ids=str)
def test_conv2d_wgrad_fx_poison_with_a_multiple_of_four_splits(ops, shape):
    """One addend per pixel split lands in a dw cell: with a whole dy channel NaN every split brings one, and the splits of
    these shapes are 4, 8 and 16 (the plan says so)."""
    NB, cout, cs, H, W, ks = shape
    plan = ops.conv2d_wgrad_plan(NB, cout, cs, H, W, ks, mode='fx', has_bias=True)
    assert len(plan) == 1 and plan[0]['accum'] == ops.WGRAD_MODES.index('fx')
    assert plan[0]['splits'] >= 4 and plan[0]['splits'] % 4 == 0, plan
    g = torch.Generator().manual_seed(400 + NB)
    dy = torch.randn(NB, cout, H, W, generator=g)
    x = torch.randn(NB, cs, H, W, generator=g).cuda()
    bad = dy.clone()
    bad[:, 3] = NAN
    bad[:, 9] = INF
    with _flags(ops, WGRAD_SLAB=False, DETERMINISTIC=True):
        dw0, db0 = ops.conv2d_wgrad(dy.cuda(), x, ks, want_bias=True)
        dw1, db1 = ops.conv2d_wgrad(bad.cuda(), x, ks, want_bias=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw1[[3, 9]]).all()) and bool(torch.isnan(db1[[3, 9]]).all()), (dw1[3], db1)
    keep = [c for c in range(cout) if c not in (3, 9)]
    assert bool(torch.isfinite(dw0).all()) and _same_bits(dw1[keep], dw0[keep]) and _same_bits(db1[keep], db0[keep])


@pytest.mark.parametrize('k', [1, 4, 8])
@pytest.mark.parametrize('S,box', [(14, 'small'), (64, 'small'), (64, 'whole')])
def test_point_sample_bwd_fx_poison_for_any_number_of_rois(ops, S, box, k):
    """k RoIs over the same cells, each with a NaN in channel 2 at the same lattice point: S = 14 the gather form, S = 64
    the scatter form by its LDS route ('small', 4 planes per pass) and by direct atomics ('whole' map).  The cells of
    the NaN sample are NaN; the other channels have the bits of the clean run."""
    B, C, H, W = fr.PS_FEAT_SHAPE
    roi = {'small': [0, 40.0, 30.0, 196.0, 146.0], 'whole': [0, 0.0, 0.0, 399.0, 319.0]}[box]
    if S == 64:
        assert fr.ps_scatter_route(roi, S, H, W, fr.PS_SCALE, B) == {'small': 'cpp4', 'whole': 'direct'}[box]
    rois = np.array([roi] * k + [[0, 20.0, 10.0, 300.0, 200.0], [1, 40.0, 30.0, 196.0, 146.0]], dtype=np.float32)
    go = np.random.RandomState(k + S).standard_normal((k + 2, C, S, S)).astype(np.float32)
    bad = go.copy()
    bad[:k, 2, S // 2, S // 3] = NAN
    sx = float(fr.ps_coord(roi[1], roi[3], np.array([S // 3]), S, W, fr.PS_SCALE)[0])
    sy = float(fr.ps_coord(roi[2], roi[4], np.array([S // 2]), S, H, fr.PS_SCALE)[0])
    x0, y0 = int(np.floor(sx)), int(np.floor(sy))
    assert 0 < x0 < W - 2 and 0 < y0 < H - 2            # (NaN * w is NaN whatever the weight: all four corners)
    with _flags(ops, DETERMINISTIC=True):
        clean = ops.point_sample_backward(_dev(go), fr.PS_FEAT_SHAPE, _dev(rois), fr.PS_SCALE)
        got = ops.point_sample_backward(_dev(bad), fr.PS_FEAT_SHAPE, _dev(rois), fr.PS_SCALE)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(got[0, 2, y0:y0 + 2, x0:x0 + 2]).all()), got[0, 2, y0:y0 + 2, x0:x0 + 2]
    others = [c for c in range(C) if c != 2]
    assert _same_bits(got[:, others], clean[:, others]) and _same_bits(got[1], clean[1])


@pytest.mark.parametrize('value', [2.0 ** 27, 1e9, 3e38, -1e9, NAN])
def test_lds_planes_poison_gradients_beyond_their_range(ops, value):
    """A finite gradient the LDS cells cannot hold (|g| >= 2^27) is no plausible number near 2^27: it poisons its plane,
    as NaN does, and the other planes keep their bits -- in dm_deform_col2im (merged and scatter() paths) and in the LDS
    route of the scatter adjoint."""
    for shape in ((2, 16, 1, 6, 6), (2, 16, 2, 5, 7), (2, 6, 2, 6, 6)):
        N, C, dg, H, W = shape
        colgrad, off = fr.col2im_inputs(shape, 'planted')
        bad = colgrad.copy()
        bad[1, 4 * C + 5, 2, 2] = value               # tap 4, channel 5 of image 1 (zero offsets: lands on (2, 2))
        gx0 = ops.deform_col2im(_dev(colgrad), _dev(off), (N, C, H, W), dg)
        gx1 = ops.deform_col2im(_dev(bad), _dev(off), (N, C, H, W), dg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(gx1[1, 5]).all()), (shape, gx1[1, 5])
        keep = torch.ones(N, C, dtype=torch.bool)
        keep[1, 5] = False
        assert bool(torch.isfinite(gx0).all()) and _same_bits(gx1.cpu()[keep], gx0.cpu()[keep])
    B, C, H, W = fr.PS_FEAT_SHAPE
    S = 64
    rois, go = fr.ps_rois(), fr.ps_go(S)
    routes = [fr.ps_scatter_route(r, S, H, W, fr.PS_SCALE, B) for r in rois]
    for route, ch in (('cpp4', 1), ('cpp2', 3), ('cpp1', 5)):
        n = routes.index(route)
        b = int(rois[n, 0])
        bad = go.copy()
        bad[n, ch, 20, 30] = value
        sx = float(fr.ps_coord(rois[n, 1], rois[n, 3], np.array([30]), S, W, fr.PS_SCALE)[0])
        sy = float(fr.ps_coord(rois[n, 2], rois[n, 4], np.array([20]), S, H, fr.PS_SCALE)[0])
        x0, y0 = int(np.floor(sx)), int(np.floor(sy))
        for det in (True, False):
            with _flags(ops, DETERMINISTIC=det):
                clean = ops.point_sample_backward(_dev(go), fr.PS_FEAT_SHAPE, _dev(rois), fr.PS_SCALE)
                got = ops.point_sample_backward(_dev(bad), fr.PS_FEAT_SHAPE, _dev(rois), fr.PS_SCALE)
            torch.cuda.synchronize()
            assert bool(torch.isnan(got[b, ch, y0:y0 + 2, x0:x0 + 2]).all()), (route, det, got[b, ch, y0:y0 + 2, x0:x0 + 2])
            keep = torch.ones(B, C, dtype=torch.bool)
            keep[b, ch] = False
            assert bool(torch.isfinite(got.cpu()[keep]).all())
            if det:
                assert _same_bits(got.cpu()[keep], clean.cpu()[keep])
