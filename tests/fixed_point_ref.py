"""Plain numpy float64 restatements of the two scatter gradients whose accumulators are 64-bit fixed point
(include/dynamask_hip.h, "Fixed-point accumulators"): the DCNv1 data gradient from the column gradient
(dm_deform_col2im) and the adjoint of SimpleRoIAlign's point sample (dm_point_sample_bwd).

Both compute the SAMPLE POSITIONS in float32, operation for operation as the kernels do (a position decides which
cells a sample reaches: it is part of the operation's definition, not of its rounding), and everything after that --
the bilinear weights, the products, the sums -- in float64.  Both return three maps shaped like the gradient:
    sum  the gradient,
    A    sum |g * w| over the addends of the cell (what a rounding of relative size 2^-24 per addend is relative to),
    K    the number of addends of the cell: in-map corners of non-void samples, whatever their weight (what a cut to
         the 2^-36 grid per addend is counted by).
tests/test_fixed_point_ref_cpu.py holds `sum` to float64 autograd through the oracle's forward operators."""
import numpy as np

F32 = np.float32


def _fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 a, b, c: the product of two 24-bit mantissas is exact in float64;
    the sum is rounded to 53 bits and then to 24, which equals the single rounding except when the 53-bit rounding
    lands exactly on a float32 tie (about 2^-29 of the cases; a test's inputs are fixed, so it either happens or not)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _scatter(out_sum, out_a, out_k, idx, ok, g, w):
    """Add g[c, i] * w[i] into cell idx[i] of every channel row c, for the samples i with ok[i]."""
    m = np.nonzero(ok)[0]
    if m.size == 0:
        return
    v = g[:, m] * w[m][None, :]
    sel = (slice(None), idx[m])
    np.add.at(out_sum, sel, v)
    np.add.at(out_a, sel, np.abs(v))
    np.add.at(out_k, sel, 1)


def col2im_ref(colgrad, offset, x_shape, dg):
    """colgrad [N, 9 * C, H, W] with rows (tap * C + c); offset [N, dg * 18, H, W], per tap the row offset, then the
    column offset; 3 x 3, stride 1, pad 1.  A sample is void unless -1 < h < H and -1 < w < W; of a non-void sample the
    corners outside the map are dropped (deform_conv_cuda_kernel.cu:279-335).  Returns sum, A, K of shape x_shape."""
    N, C, H, W = x_shape
    HW, cpg = H * W, C // dg
    cg = np.asarray(colgrad, F32).reshape(N, 9, C, HW).astype(np.float64)
    off = np.asarray(offset, F32).reshape(N, dg, 9, 2, HW)
    ys = np.repeat(np.arange(H), W)
    xs = np.tile(np.arange(W), H)
    s = np.zeros((N, C, HW), np.float64)
    a = np.zeros((N, C, HW), np.float64)
    k = np.zeros((N, C, HW), np.int64)
    for n in range(N):
        for g in range(dg):
            cs = slice(g * cpg, (g + 1) * cpg)
            for tap in range(9):
                ki, kj = divmod(tap, 3)
                h_im = (ys - 1 + ki).astype(F32) + off[n, g, tap, 0]            # one float32 addition, as the kernel's
                w_im = (xs - 1 + kj).astype(F32) + off[n, g, tap, 1]
                assert h_im.dtype == F32 and w_im.dtype == F32
                valid = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
                h_im, w_im = np.where(valid, h_im, 0).astype(np.float64), np.where(valid, w_im, 0).astype(np.float64)
                hl, wl = np.floor(h_im), np.floor(w_im)
                lh, lw = h_im - hl, w_im - wl
                hl, wl = hl.astype(np.int64), wl.astype(np.int64)
                for dh, dw in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    hi, wi = hl + dh, wl + dw
                    ok = valid & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
                    wgt = (lh if dh else 1 - lh) * (lw if dw else 1 - lw)
                    _scatter(s[n, cs], a[n, cs], k[n, cs], hi * W + wi, ok, cg[n, tap, cs], wgt)
    shape = (N, C, H, W)
    return s.reshape(shape), a.reshape(shape), k.reshape(shape)


def ps_coord(lo, hi, i, S, size, scale):
    """The sample coordinate of lattice index i on an axis of `size` cells, in float32 as the kernels' ps_coord computes
    it: point_sample's chain (rel_roi_point_to_rel_img_point, then grid_sample's unnormalisation with
    align_corners = False), every operation rounded to float32, with the two multiply-adds the device compiler
    contracts (p * (hi - lo) + lo and (g + 1) * size - 1) as fused ones."""
    lo, hi, scale, fs = F32(lo), F32(hi), F32(scale), F32(size)
    g0 = (2 * np.asarray(i) + 1).astype(F32) / F32(S) - F32(1)
    p = (g0 + F32(1)) / F32(2)
    p = _fma32(p, hi - lo, lo)
    p = p / fs * scale
    g = p * F32(2) - F32(1)                                 # (p * 2 is exact: fused or not, the same value)
    s = _fma32(g + F32(1), fs, F32(-1)) / F32(2)
    assert s.dtype == F32
    return s


def point_sample_adjoint_ref(go, feat_shape, rois, scale):
    """go [N, C, S, S]; rois [N, 5] (batch index, x1, y1, x2, y2 in image pixels).  A sample reaches the four cells
    around its coordinate, those outside the map dropped (grid_sample, bilinear, zeros padding); a RoI whose batch index
    is not in [0, B) is skipped.  Returns sum, A, K of shape feat_shape."""
    B, C, H, W = feat_shape
    go = np.asarray(go, F32).astype(np.float64)
    rois = np.asarray(rois, F32)
    N, _, S, _ = go.shape
    s = np.zeros((B, C, H * W), np.float64)
    a = np.zeros((B, C, H * W), np.float64)
    k = np.zeros((B, C, H * W), np.int64)
    for n in range(N):
        b = int(rois[n, 0])
        if b < 0 or b >= B:
            continue
        sx = ps_coord(rois[n, 1], rois[n, 3], np.arange(S), S, W, scale)
        sy = ps_coord(rois[n, 2], rois[n, 4], np.arange(S), S, H, scale)
        sx = np.tile(sx, S).astype(np.float64)               # pos = iy * S + ix
        sy = np.repeat(sy, S).astype(np.float64)
        fx, fy = np.floor(sx), np.floor(sy)
        near = (fx >= -1) & (fx <= W) & (fy >= -1) & (fy <= H)
        lx, ly = sx - fx, sy - fy
        x0, y0 = np.where(near, fx, 0).astype(np.int64), np.where(near, fy, 0).astype(np.int64)
        g = go[n].reshape(C, S * S)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            xi, yi = x0 + dx, y0 + dy
            ok = near & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            wgt = (lx if dx else 1 - lx) * (ly if dy else 1 - ly)
            _scatter(s[b], a[b], k[b], yi * W + xi, ok, g, wgt)
    return s.reshape(feat_shape), a.reshape(feat_shape), k.reshape(feat_shape)


def ps_footprint(roi, S, H, W, scale):
    """(TW, TH): the footprint of a RoI's lattice in cells, as point_sample_bwd_kernel computes it, or None where every
    sample is void."""
    sxa, sxb = (float(ps_coord(roi[1], roi[3], np.array([i]), S, W, scale)[0]) for i in (0, S - 1))
    sya, syb = (float(ps_coord(roi[2], roi[4], np.array([i]), S, H, scale)[0]) for i in (0, S - 1))
    sxmin, sxmax, symin, symax = min(sxa, sxb), max(sxa, sxb), min(sya, syb), max(sya, syb)
    if sxmax < -1 or sxmin > W or symax < -1 or symin > H:
        return None
    fx0, fx1 = max(int(np.floor(max(sxmin, -1.0))), 0), min(int(np.floor(min(sxmax, float(W)))) + 1, W - 1)
    fy0, fy1 = max(int(np.floor(max(symin, -1.0))), 0), min(int(np.floor(min(symax, float(H)))) + 1, H - 1)
    return fx1 - fx0 + 1, fy1 - fy0 + 1


def ps_scatter_route(roi, S, H, W, scale, B, ct=4, lds_elems=6144):
    """Which sub-route point_sample_bwd_kernel<CT = 4> takes for a RoI (its channel passes hold 4, 2 or 1 planes of
    the footprint in 6144 LDS cells, else global atomics): 'cpp4', 'cpp2', 'cpp1', 'direct', or 'skip' (bad batch
    index, every sample void)."""
    b = int(roi[0])
    if b < 0 or b >= B:
        return 'skip'
    fp = ps_footprint(roi, S, H, W, scale)
    if fp is None:
        return 'skip'
    tw, th = fp
    if tw <= 0 or th <= 0:
        return 'direct'
    if tw * th * ct <= lds_elems:
        return 'cpp4'
    if tw * th * 2 <= lds_elems:
        return 'cpp2'
    if tw * th <= lds_elems:
        return 'cpp1'
    return 'direct'


# ------------------------------------------------------------------------------------------------ shared test inputs
# (N, C, dg, H, W) by the CT of the build dm_deform_col2im launches (the tests that use them ask the launcher's plan,
# ops.backward_plan('col2im', ...)).  6 x 6 and 8 x 8 take the merged path (H * W % 4 == 0; at 6 x 6 an item of four
# pixels wraps a row), 5 x 7 the scatter() path.
COL2IM_SHAPES = {
    8: [(2, 16, 1, 6, 6), (2, 16, 1, 8, 8), (2, 16, 2, 5, 7)],
    4: [(2, 8, 2, 6, 6), (2, 8, 2, 5, 7)],
    2: [(2, 12, 2, 6, 6), (2, 12, 2, 5, 7)],
    1: [(2, 6, 2, 6, 6), (2, 6, 2, 5, 7)],
}
COL2IM_VARIANTS = ('planted', 'collapse')
EXPONENTS = (0, -12, -24, -33, 16)


def col2im_inputs(shape, variant, seed=0):
    """colgrad ~ N(0, 1), offsets ~ N(0, 1.5^2) with planted cases.
    'planted':  image 0 random with, at fixed pixels and for every tap, integer offsets, samples in the strips (-1, 0)
                and (H - 1, H), at exactly -1 and exactly H / W (void), and far outside the map (1e4, -3e9); image 1 all
                zero offsets (weights exactly 1 and 0, every neighbour linked).
    'collapse': image 0 sends every tap of every pixel of a row y to (y + 0.375, W // 2 - 1 + 0.25): 9 W addends per
                cell; image 1 random."""
    N, C, dg, H, W = shape
    rng = np.random.RandomState(1000 + seed + 7 * C + 31 * H + W + (0 if variant == 'planted' else 500))
    colgrad = rng.standard_normal((N, 9 * C, H, W)).astype(F32)
    off = (rng.standard_normal((N, dg, 9, 2, H, W)) * 1.5).astype(F32)
    if variant == 'planted':
        off[1] = 0
        o = off[0]
        o[:, :, 0, 1, 1], o[:, :, 1, 1, 1] = 1.0, -1.0                       # integer offsets
        o[:, :, :, 0, 3], o[:, :, :, H - 1, 3] = 0.0, 0.0                    # ki = 0 at y = 0: h = -1; ki = 2 at y = H - 1: h = H
        o[:, :, :, 2, 0], o[:, :, :, 2, W - 1] = 0.0, 0.0                    # kj = 0 at x = 0: w = -1; kj = 2 at x = W - 1: w = W
        o[:, :, 0, 0, 2], o[:, :, 1, 0, 2] = 0.5, 0.25                       # ki = 0: h = -0.5, the strip (-1, 0)
        o[:, :, 0, H - 1, 2], o[:, :, 1, H - 1, 2] = -0.5, 0.25              # ki = 2: h = H - 0.5, the strip (H - 1, H)
        o[:, :, 0, 1, 0], o[:, :, 1, 1, 0] = 0.25, 0.5                       # kj = 0: w = -0.5
        o[:, :, 0, 3, W - 1], o[:, :, 1, 3, W - 1] = 0.25, -0.5              # kj = 2: w = W - 0.5
        o[:, :, 0, 3, 3], o[:, :, 1, 3, 3] = 1e4, -1e4                       # far outside
        o[:, :, 0, 4, 1], o[:, :, 1, 4, 1] = -3e9, 3e9                       # beyond the range of an int
    else:
        ys, xs = np.arange(H).reshape(H, 1), np.arange(W).reshape(1, W)
        for tap in range(9):
            ki, kj = divmod(tap, 3)
            off[0, :, tap, 0] = (ys + 0.375 - (ys - 1 + ki)) + 0 * xs
            off[0, :, tap, 1] = (W // 2 - 1 + 0.25) - (xs - 1 + kj) + 0 * ys
    return colgrad, off.reshape(N, dg * 18, H, W)


# The scatter form of the point-sample adjoint starts where the gather form's LDS need passes 64 KB: S = 64.
PS_FEAT_SHAPE = (2, 6, 80, 100)          # B, C (one full channel quad, one short), H, W
PS_SCALE = 0.25


def ps_rois():
    """RoIs in image pixels (scale 0.25: 4 pixels per cell) on the 80 x 100 map, grouped by image as bbox2roi gives them:
    footprints of about 30 x 40, 50 x 58, 70 x 80 cells and the whole map (the four sub-routes of the scatter kernel at
    S = 64), then the corner cases of test_point_sample_backward_corner_case_rois."""
    r = np.array([
        [0, 40.0, 30.0, 196.0, 146.0],            # about 40 x 30 cells
        [1, 60.5, 50.0, 288.0, 246.0],            # about 58 x 50
        [0, 50.0, 20.0, 366.0, 296.0],            # about 80 x 70
        [1, 0.0, 0.0, 399.0, 319.0],              # the whole map
        [0, -30.0, -20.0, 40.0, 35.0],            # over the top-left corner
        [1, 340.0, 280.0, 460.0, 370.0],          # over the bottom-right corner
        [0, -50.0, -50.0, 500.0, 400.0],          # larger than the map
        [1, 60.0, 40.0, 61.0, 41.0],              # one image pixel
        [0, 77.3, 20.0, 77.3, 60.0],              # zero width
        [1, 30.0, 55.5, 90.0, 55.5],              # zero height
        [0, 120.0, 70.0, 40.0, 10.0],             # inverted
        [1, 900.0, 700.0, 1000.0, 780.0],         # off the map
        [0, 3.999, 3.999, 4.001, 4.001],          # around a cell boundary
        [2, 10.0, 10.0, 50.0, 50.0],              # bad batch index
        [-1, 10.0, 10.0, 50.0, 50.0],
    ], dtype=F32)
    return r[np.argsort(np.where((r[:, 0] < 0) | (r[:, 0] > 1), 9, r[:, 0]), kind='stable')]


def ps_go(S, seed=0):
    """N(0, 1/16): the one-pixel RoI puts all S * S samples into four cells, and sum |g * w| of a cell, times the largest
    scale of the tests (2^16), has to stay below an fx cell's range of 2^25."""
    n = ps_rois().shape[0]
    return np.random.RandomState(2000 + seed + S).standard_normal((n, PS_FEAT_SHAPE[1], S, S)).astype(F32) * F32(0.25)
