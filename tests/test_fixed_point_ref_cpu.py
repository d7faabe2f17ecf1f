"""tests/fixed_point_ref.py -- the float64 reference of tests/test_fixed_point_gpu.py -- against float64 autograd through
the oracle's forward operators, at every shape the GPU tests use.

Tolerance.  The reference takes its sample positions in float32 (as the kernels do), the oracle here is fed float64 and
takes them in float64 (deform_conv2d) or through another float32 chain (simple_roi_align: torch's point arithmetic, then
grid_sample's unnormalisation in float64).  A position that differs by d moves each bilinear weight of its sample by at
most |d| per axis, i.e. an addend g * w by at most |g| * (|dh| + |dw|); where the floor differs too the sample reaches a
neighbouring cell with a weight below |d|, the same bound.  So per cell

    |ref - oracle| <= (K_cell + 8) * g_max * 2 * d_max * 2    (two axes; twice, and 8 addends more, for what a floor
                                                               change moves in from the neighbouring cells)
                      + 64 * 2^-53 * A_max                     (float64 rounding of either side: far below the first term)

with d_max = r * 2^-24 * coord_max: r float32 roundings of magnitude up to coord_max between the inputs and the
coordinate.  col2im: r = 1 (one addition), coord_max = max(H, W) + 1.  Point sample: r = 8 (ps_coord's operations; the
oracle's chain has as many) and coord_max the largest |image coordinate| * scale of a RoI with a sample near the map,
or the map size.  A structural mistake (a wrong corner, tap order, void rule) is an error of the order of g_max itself,
10^3 to 10^5 times these tolerances."""
import numpy as np
import pytest
import torch

import fixed_point_ref as fr
from oracle import ref_ops


def _col2im_tol(shape, colgrad, a, k):
    H, W = shape[3], shape[4]
    d = 1 * 2.0 ** -24 * (max(H, W) + 1)
    return (k + 8) * float(np.abs(colgrad).max()) * 4 * d + 64 * 2.0 ** -53 * float(a.max())


@pytest.mark.parametrize('variant', fr.COL2IM_VARIANTS)
@pytest.mark.parametrize('shape', [s for ss in fr.COL2IM_SHAPES.values() for s in ss], ids=str)
def test_col2im_ref_is_the_float64_adjoint_of_the_oracle(shape, variant):
    N, C, dg, H, W = shape
    colgrad, off = fr.col2im_inputs(shape, variant)
    s, a, k = fr.col2im_ref(colgrad, off, (N, C, H, W), dg)
    # a weight that makes the oracle's output channel (tap * C + c) the column (c, tap): its output gradient is then the
    # tap-major column gradient
    w = torch.zeros(9 * C, C, 3, 3, dtype=torch.float64)
    for tap in range(9):
        w[tap * C + torch.arange(C), torch.arange(C), tap // 3, tap % 3] = 1.0
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    y = ref_ops.deform_conv2d(x, torch.from_numpy(off).double(), w, deform_groups=dg)
    y.backward(torch.from_numpy(colgrad).double())
    err = np.abs(s - x.grad.numpy())
    tol = _col2im_tol(shape, colgrad, a, k)
    assert float(np.abs(s).max()) > 0.1
    assert (err <= tol).all(), (float(err.max()), float((err / tol).max()))
    assert (a >= np.abs(s) - 1e-12).all() and ((k == 0) <= (a == 0)).all()
    if variant == 'collapse':
        assert int(k[0].max()) >= 9 * W                     # every tap of a row in one cell
    else:
        # all-zero offsets: every weight is exactly 1 or 0 and a cell's nine unit-weight addends come from its 3 x 3
        # neighbourhood -- each of them brings four corners: K = 4 * 9 in the interior
        assert int(k[1, :, 2, 2].min()) == 36


@pytest.mark.parametrize('S', [64, 14])
def test_point_sample_adjoint_ref_is_the_float64_adjoint_of_the_oracle(S):
    rois, go = fr.ps_rois(), fr.ps_go(S)
    B, C, H, W = fr.PS_FEAT_SHAPE
    s, a, k = fr.point_sample_adjoint_ref(go, fr.PS_FEAT_SHAPE, rois, fr.PS_SCALE)
    good = (rois[:, 0] >= 0) & (rois[:, 0] < B)              # the oracle has no row for a RoI of no image
    assert good[:-2].all() and not good[-2:].any()
    feat = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    out = ref_ops.simple_roi_align(feat, torch.from_numpy(rois[good]), S, fr.PS_SCALE)
    out.backward(torch.from_numpy(go[good]).double())
    coord_max = max(float(np.abs(rois[good][:-1, 1:]).max()) * fr.PS_SCALE, W)
    d = 8 * 2.0 ** -24 * coord_max
    tol = (k + 8) * float(np.abs(go).max()) * 4 * d + 64 * 2.0 ** -53 * float(a.max())
    err = np.abs(s - feat.grad.numpy())
    assert float(np.abs(s).max()) > 0.1
    assert (err <= tol).all(), (float(err.max()), float((err / tol).max()))
    assert (a >= np.abs(s) - 1e-12).all()


def test_the_point_sample_rois_reach_every_sub_route_of_the_scatter_form():
    B, _, H, W = fr.PS_FEAT_SHAPE
    routes = [fr.ps_scatter_route(r, 64, H, W, fr.PS_SCALE, B) for r in fr.ps_rois()]
    assert {'cpp4', 'cpp2', 'cpp1', 'direct', 'skip'} <= set(routes), routes


def test_col2im_shapes_take_the_builds_they_are_listed_under():
    from dynamask_amd import ops
    for ct, shapes in fr.COL2IM_SHAPES.items():
        for N, C, dg, H, W in shapes:
            one, = ops.backward_plan('col2im', N, C, H, W, dg)
            assert (one['kernel'], one['P0']) == (ops.BWD_KERNELS.index('col2im_lds'), ct)
    assert set(fr.COL2IM_SHAPES) == {b[1] for b in ops.BWD_BUILDS['col2im']}
    assert {(H * W) % 4 == 0 for ss in fr.COL2IM_SHAPES.values() for _, _, _, H, W in ss} == {True, False}
