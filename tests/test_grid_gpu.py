"""Grid R-CNN inference on the MI355X: the kernels of csrc/grid_head.hip against float64 PyTorch on the CPU through the
triangle of tests/tolerances.py (GroupNorm, the neighbour fusion, the grouped 4x4 stride-2 deconvolution, the box vote
with known answers), the 576-channel shapes of the two existing 3x3 convolutions, and GridHead / GridRoIHead through the
registry against the reference (tests/golden/g23_grid.npz: the reference's own float32 and float64 runs): heatmaps, boxes,
simple_test with and without rescale, zero detections, batches, run-to-run bits and the bf16x3 mode.  Every kernel
output is written between two canary guard bands that must survive."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

CANARY = 7.0
GUARD = 4096


def _g(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """A device tensor of ``shape`` between two guard bands of CANARY."""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), CANARY, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == CANARY).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == CANARY).all()), f'{what}: the guard band past the output was overwritten'


# ------------------------------------------------------------------------------------------------ GroupNorm
# (N, C, G, H, W): one value per group; the eight convs' shape; norm1's shape (12 544 values per group); odd sizes
GN_CASES = [(1, 16, 1, 1, 1), (3, 576, 36, 7, 7), (2, 576, 9, 14, 14), (2, 24, 3, 5, 3)]


def _gn_ref(x, gamma, beta, G, relu, dtype):
    y = F.group_norm(x.to(dtype), G, gamma.to(dtype), beta.to(dtype), eps=1e-5)
    return F.relu(y) if relu else y


@pytest.mark.parametrize('inplace', (False, True))
@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('N,C,G,H,W', GN_CASES)
def test_group_norm(N, C, G, H, W, relu, inplace):
    from dynamask_amd import ops
    g = _g(N + C + G + H + W)
    x = torch.randn(N, C, H, W, generator=g) * 2.0 + 0.5
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    xd = Guarded(x.shape, x)
    assert ops.group_norm_supported(xd.t, G)
    out = xd if inplace else Guarded(x.shape)
    got = ops.group_norm(xd.t, gamma.cuda(), beta.cuda(), G, relu=relu, out=out.t)
    again = ops.group_norm(x.cuda(), gamma.cuda(), beta.cuda(), G, relu=relu)
    out.check('group_norm')
    xd.check('group_norm input')
    assert got.data_ptr() == out.t.data_ptr() and torch.equal(got, again), 'in-place / out-of-place or two runs differ'
    if not inplace:
        assert torch.equal(xd.t.cpu(), x), 'the input was modified'
    r32, r64 = _gn_ref(x, gamma, beta, G, relu, torch.float32), _gn_ref(x, gamma, beta, G, relu, torch.float64)
    if H * W * (C // G) == 1:
        # one value per group: the normalised value is exactly 0, the output exactly beta (the float64 reference too)
        expect = F.relu(beta) if relu else beta
        assert torch.equal(got.cpu().reshape(-1), expect.repeat(N))
        return
    assert_close_via_f64(got, r32, r64, f'group_norm {N}x{C}x{H}x{W} G={G} relu={relu}')


def test_group_norm_constant_group_gives_beta():
    from dynamask_amd import ops
    g = _g(3)
    x = torch.randn(2, 24, 5, 3, generator=g)
    x[1, 8:16] = 3.7                     # group 1 of sample 1 (8 channels x 15 pixels)
    x[0, 16:24] = -0.1
    gamma = 1.0 + 0.3 * torch.randn(24, generator=g)
    beta = 0.5 * torch.randn(24, generator=g)
    got = ops.group_norm(x.cuda(), gamma.cuda(), beta.cuda(), 3).cpu()
    assert torch.equal(got[1, 8:16], beta[8:16, None, None].expand(8, 5, 3))
    assert torch.equal(got[0, 16:24], beta[16:24, None, None].expand(8, 5, 3))
    assert not torch.equal(got[0, 8:16], beta[8:16, None, None].expand(8, 5, 3))


def test_group_norm_large_mean():
    """Mean 1e3, unit spread: E[x^2] - E[x]^2 would lose every digit of the variance in float32."""
    from dynamask_amd import ops
    g = _g(4)
    x = 1000.0 + torch.randn(2, 576, 7, 7, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(576, generator=g)
    beta = 0.5 * torch.randn(576, generator=g)
    got = ops.group_norm(x.cuda(), gamma.cuda(), beta.cuda(), 36)
    r32, r64 = _gn_ref(x, gamma, beta, 36, False, torch.float32), _gn_ref(x, gamma, beta, 36, False, torch.float64)
    assert_close_via_f64(got, r32, r64, 'group_norm mean 1e3')


def test_group_norm_refusals():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    assert lib().dm_group_norm_supported(2, 24, 5, 5, 3) == 0            # C % G
    assert lib().dm_group_norm_supported(2, 24, 0, 5, 3) == 0
    assert lib().dm_group_norm_supported(0, 24, 3, 5, 3) == 1
    x = torch.randn(2, 24, 5, 3, device='cuda')
    w = torch.ones(24, device='cuda')
    with pytest.raises(RuntimeError):
        ops.group_norm(x, w, w, 5)
    with pytest.raises(RuntimeError):
        ops.group_norm(x, w, w, 3, eps=0.0)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.group_norm(x.cpu(), w, w, 3)
    empty = ops.group_norm(x[:0].contiguous(), w, w, 3)
    assert tuple(empty.shape) == (0, 24, 5, 3)


# ------------------------------------------------------------------------------------------------ neighbour fusion
def _fusion_weights(P, c, seed):
    from dynamask_amd import ops
    g = _g(seed)
    trans = []
    for nb in ops.grid_neighbors(P):
        trans.append([(torch.randn(c, 1, 5, 5, generator=g) * (1.0 / 25) ** 0.5, torch.randn(c, generator=g) * 0.1,
                       torch.randn(c, c, 1, 1, generator=g) * (1.0 / c) ** 0.5, torch.randn(c, generator=g) * 0.1)
                      for _ in nb])
    return trans


def _fusion_ref(x, src, trans, P, c, dtype):
    """grid_head.py:157-170 restated: x_i + the transitions of the neighbours' ``src`` slices, added in neighbour order."""
    from dynamask_amd import ops
    x, src = x.to(dtype), src.to(dtype)
    outs = []
    for i, nb in enumerate(ops.grid_neighbors(P)):
        acc = x[:, i * c:(i + 1) * c]
        for j, p in enumerate(nb):
            dw_w, dw_b, w1, b1 = (t.to(dtype) for t in trans[i][j])
            t = F.conv2d(src[:, p * c:(p + 1) * c], dw_w, dw_b, padding=2, groups=c)
            acc = acc + F.conv2d(t, w1, b1)
        outs.append(acc)
    return torch.cat(outs, 1)


def _table(trans, P, c):
    from dynamask_amd import ops
    return ops.pack_grid_fusion_table([[tuple(t.cuda() for t in slot) for slot in point] for point in trans], P, c)


# (points, c, S, N): the head's shape; a small one where most of the 5 x 5 window is padding
@pytest.mark.parametrize('P,c,S,N', [(9, 64, 7, 3), (4, 8, 3, 1)])
def test_grid_fusion_both_orders(P, c, S, N):
    from dynamask_amd import ops
    g = _g(P * 100 + c + S + N)
    x = torch.randn(N, P * c, S, S, generator=g)
    fo_w, so_w = _fusion_weights(P, c, 11), _fusion_weights(P, c, 12)
    xd = x.cuda()
    assert ops.grid_fusion_supported(xd, P)
    fo = Guarded(x.shape)
    ops.grid_fusion(xd, xd, _table(fo_w, P, c), P, out=fo.t)
    fo.check('first order')
    assert_close_via_f64(fo.t, _fusion_ref(x, x, fo_w, P, c, torch.float32), _fusion_ref(x, x, fo_w, P, c, torch.float64),
                         f'fusion first order P={P} c={c} S={S}')
    # second order: x_i again, the transitions read the first order's result
    src = fo.t.cpu()
    so = Guarded(x.shape)
    ops.grid_fusion(xd, fo.t.contiguous(), _table(so_w, P, c), P, out=so.t)
    so.check('second order')
    assert_close_via_f64(so.t, _fusion_ref(x, src, so_w, P, c, torch.float32), _fusion_ref(x, src, so_w, P, c, torch.float64),
                         f'fusion second order P={P} c={c} S={S}')
    assert torch.equal(so.t, ops.grid_fusion(xd, fo.t.contiguous(), _table(so_w, P, c), P)), 'two runs differ'
    assert torch.equal(xd.cpu(), x), 'the input was modified'


def test_grid_fusion_neighbour_order():
    """Swapping the weights of two neighbour slots of one point changes that point's result (and only it), and the
    swapped table still matches the restated loop with the swapped weights: slot j belongs to the j-th neighbour in the
    reference's order left, up, down, right."""
    from dynamask_amd import ops
    P, c, S = 9, 64, 7
    x = torch.randn(2, P * c, S, S, generator=_g(5))
    w = _fusion_weights(P, c, 13)
    xd = x.cuda()
    base = ops.grid_fusion(xd, xd, _table(w, P, c), P).cpu()
    sw = [list(point) for point in w]
    sw[4][0], sw[4][1] = sw[4][1], sw[4][0]
    got = ops.grid_fusion(xd, xd, _table(sw, P, c), P).cpu()
    assert not torch.equal(got[:, 4 * c:5 * c], base[:, 4 * c:5 * c])
    keep = [i for i in range(P * c) if not 4 * c <= i < 5 * c]
    assert torch.equal(got[:, keep], base[:, keep])
    assert_close_via_f64(got, _fusion_ref(x, x, sw, P, c, torch.float32), _fusion_ref(x, x, sw, P, c, torch.float64),
                         'fusion with two slots swapped')


def test_grid_fusion_refusals():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_grid_fusion_supported(3, 9, 64, 7) == 1 and L.dm_grid_fusion_supported(0, 4, 8, 3) == 1
    for bad in ((3, 16, 64, 7), (3, 9, 32, 7), (3, 9, 64, 14), (-1, 9, 64, 7)):
        assert L.dm_grid_fusion_supported(*bad) == 0, bad
    assert L.dm_grid_fusion_table_floats(9, 64) == 9 * 4 * (25 * 64 + 64 + 64 * 64 + 64)
    assert L.dm_grid_fusion_table_floats(9, 32) == -1
    x = torch.randn(1, 9 * 64, 7, 7, device='cuda')
    tab = torch.zeros(9 * 4 * (25 * 64 + 64 + 64 * 64 + 64), device='cuda')
    with pytest.raises(RuntimeError):
        ops.grid_fusion(x, x, tab, 9, out=x)                      # out may not alias an input
    assert not ops.grid_fusion_supported(torch.empty(1, 9 * 64, 14, 14, device='cuda'), 9)


# ------------------------------------------------------------------------------------------------ grouped deconv
# (groups, cin / g, cout / g, S, N): deconv1; deconv2; a 1 x 1 map (every output has one tap); a small odd one
@pytest.mark.parametrize('G,ci,co,S,N', [(9, 64, 64, 7, 2), (9, 64, 1, 14, 2), (4, 8, 8, 1, 1), (4, 8, 1, 3, 3)])
def test_deconv4x4_s2_grouped(G, ci, co, S, N):
    from dynamask_amd import ops
    g = _g(G * 1000 + ci + co + S + N)
    x = torch.randn(N, G * ci, S, S, generator=g)
    w = torch.randn(G * ci, co, 4, 4, generator=g) * (1.0 / (4 * ci)) ** 0.5
    b = torch.randn(G * co, generator=g) * 0.1
    xd = x.cuda()
    assert ops.deconv4x4_s2_grouped_supported(xd, G * co, G)
    out = Guarded((N, G * co, 2 * S, 2 * S))
    ops.deconv4x4_s2_grouped(xd, w.cuda(), b.cuda(), G, out=out.t)
    out.check('deconv')
    assert torch.equal(out.t, ops.deconv4x4_s2_grouped(xd, w.cuda(), b.cuda(), G)), 'two runs differ'
    r32 = F.conv_transpose2d(x, w, b, stride=2, padding=1, groups=G)
    r64 = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1, groups=G)
    assert_close_via_f64(out.t, r32, r64, f'deconv G={G} {ci}->{co} S={S}')
    nobias = ops.deconv4x4_s2_grouped(xd, w.cuda(), None, G)
    assert_close_via_f64(nobias, F.conv_transpose2d(x, w, None, stride=2, padding=1, groups=G),
                         F.conv_transpose2d(x.double(), w.double(), None, stride=2, padding=1, groups=G), 'deconv, no bias')


def test_deconv4x4_s2_grouped_refusals():
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_deconv4x4_s2_grouped_supported(2, 9, 64, 64, 7) == 1
    for bad in ((2, 8, 64, 64, 7), (2, 9, 32, 64, 7), (2, 9, 64, 2, 7), (2, 9, 64, 64, 28), (-1, 9, 64, 64, 7)):
        assert L.dm_deconv4x4_s2_grouped_supported(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the box vote
def _sub_regions(P, half):
    from dynamask_amd.mask_heads import grid_sub_regions
    return grid_sub_regions(P, 2 * half)


def _vote(det, scores, cells, sub, HS, dtype):
    """grid_head.py:313-355 restated from the cells of the maxima: offsets, the box grown by half its size, the
    score-weighted mean of each side's points."""
    P = scores.shape[1]
    gs = int(round(P ** 0.5))
    det, scores = det.to(dtype), scores.to(dtype)
    xs = (cells % HS + torch.tensor([r[0] for r in sub])).to(dtype)
    ys = (cells // HS + torch.tensor([r[1] for r in sub])).to(dtype)
    w, h = (det[:, 2] - det[:, 0])[:, None], (det[:, 3] - det[:, 1])[:, None]
    ax = (xs + 0.5) / HS * w + (det[:, 0, None] - w / 2)
    ay = (ys + 0.5) / HS * h + (det[:, 1, None] - h / 2)
    sides = ((ax, list(range(gs))), (ay, [i * gs for i in range(gs)]), (ax, [P - gs + i for i in range(gs)]),
             (ay, [(i + 1) * gs - 1 for i in range(gs)]))
    cols = [(a[:, idx] * scores[:, idx]).sum(1) / scores[:, idx].sum(1) for a, idx in sides]
    return torch.stack(cols + [det[:, -1]], 1)


def test_get_bboxes_constant_heatmap_takes_cell_zero():
    from dynamask_amd import ops
    HS, P = 28, 9
    det = torch.tensor([[10.0, 20.0, 110.0, 90.0, 0.5], [2.0, 2.0, 50.0, 50.0, 0.25]])
    heat = torch.full((2, P, HS, HS), -1.5)
    sub = _sub_regions(P, HS)
    out = Guarded((2, 5))
    _, cells = ops.grid_get_bboxes(heat.cuda(), det.cuda(), sub, out=out.t, return_cells=True)
    out.check('get_bboxes')
    assert bool((cells == 0).all())
    sc = torch.sigmoid(heat.double()).amax((2, 3))
    z = torch.zeros(2, P, dtype=torch.long)
    assert_close_via_f64(out.t, _vote(det, sc.float(), z, sub, HS, torch.float32), _vote(det, sc, z, sub, HS, torch.float64),
                         'constant heatmap')
    # Quirk Q21: the vote of the second box lands left of and above the image and stays there (no clip)
    assert float(out.t[1, 0]) < 0 and float(out.t[1, 1]) < 0
    assert torch.equal(out.t[:, 4].cpu(), det[:, 4])


def test_get_bboxes_first_maximum_of_the_sigmoid():
    """Logits 20 (earlier cell) and 30 (later cell) both give sigmoid 1.0f: the earlier one is the maximum, as for
    torch.max over the sigmoid values; logit 16 (earlier still) gives 0.99999988 and does not tie."""
    from dynamask_amd import ops
    HS, P = 28, 9
    heat = torch.full((1, P, HS, HS), -3.0)
    flat = heat.view(1, P, -1)
    for p in range(P):
        flat[0, p, 5 + p] = 16.0
        flat[0, p, 100 + 20 * p] = 20.0
        flat[0, p, 300 + p] = 30.0
    assert float(torch.sigmoid(torch.tensor(20.0))) == 1.0 and float(torch.sigmoid(torch.tensor(16.0))) < 1.0
    det = torch.tensor([[40.0, 30.0, 140.0, 170.0, 0.75]])
    sub = _sub_regions(P, HS)
    out, cells = ops.grid_get_bboxes(heat.cuda(), det.cuda(), sub, return_cells=True)
    want = torch.tensor([[100 + 20 * p for p in range(P)]])
    assert torch.equal(cells.cpu().long(), want)
    ones = torch.ones(1, P, dtype=torch.float64)
    assert_close_via_f64(out, _vote(det, ones.float(), want, sub, HS, torch.float32), _vote(det, ones, want, sub, HS, torch.float64),
                         'saturated heatmap')
    # a map whose last cell is the maximum, and P = 4 on a small map
    heat4 = torch.randn(3, 4, 6, 6, generator=_g(8))
    heat4[1, 2, 5, 5] = 9.0
    det4 = torch.tensor([[0.0, 0.0, 30.0, 20.0, 1.0, 0.5]] * 3)            # D = 6: the score is the last column
    sub4 = _sub_regions(4, 6)
    out4, cells4 = ops.grid_get_bboxes(heat4.cuda(), det4.cuda(), sub4, return_cells=True)
    want4 = heat4.view(3, 4, -1).argmax(2)
    assert torch.equal(cells4.cpu().long(), want4) and int(cells4[1, 2]) == 35
    sc4 = torch.sigmoid(heat4.double()).amax((2, 3))
    assert_close_via_f64(out4, _vote(det4, sc4.float(), want4, sub4, 6, torch.float32), _vote(det4, sc4, want4, sub4, 6, torch.float64),
                         'P = 4')
    assert bool((out4[:, 4] == 0.5).all())


def test_get_bboxes_golden(golden_dir):
    """The reference's heatmaps -> the reference's boxes: the same cells (the generator asserted a top-2 logit gap of
    1e-3 below saturation) and coordinates inside the float64 triangle."""
    from dynamask_amd import ops
    z = np.load(os.path.join(golden_dir, 'g23_grid.npz'))
    heat, det = torch.from_numpy(z['heat']), torch.from_numpy(z['heat_dets'])
    sub = _sub_regions(9, 28)
    out, cells = ops.grid_get_bboxes(heat.cuda(), det.cuda(), sub, return_cells=True)
    want = torch.from_numpy(z['heat64']).view(8, 9, -1).argmax(2)
    assert torch.equal(heat.view(8, 9, -1).argmax(2), want)
    assert torch.equal(cells.cpu().long(), want)
    assert_close_via_f64(out, z['heat_boxes'], z['heat_boxes64'], 'golden boxes')
    b = z['heat_boxes']
    assert (b[:, :2] < 0).any() or (b[:, 2] > 256).any() or (b[:, 3] > 192).any()      # Q21: the reference does not clip
    assert torch.equal(out.cpu()[:, :4] < 0, torch.from_numpy(b[:, :4] < 0))


def test_get_bboxes_refusals():
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_grid_get_bboxes_supported(5, 9, 28, 5) == 1 and L.dm_grid_get_bboxes_supported(0, 4, 6, 6) == 1
    for bad in ((5, 16, 28, 5), (5, 9, 0, 5), (5, 9, 28, 4), (-1, 9, 28, 5), (5, 9, 2000, 5)):
        assert L.dm_grid_get_bboxes_supported(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the 576-channel convs
def test_convs_take_576_channels():
    """The head's two convolution shapes on the existing exact-fp32 3x3 kernels: 256 -> 576 at stride 2 (one split) and
    576 -> 576 on 7 x 7 maps (ops.conv2d: 4.5 cout tiles of 128, RoIs packed into flat 128-pixel tiles)."""
    from dynamask_amd import ops
    g = _g(576)
    x = torch.randn(5, 256, 14, 14, generator=g)
    w0 = torch.randn(576, 256, 3, 3, generator=g) * (2.0 / (9 * 256)) ** 0.5
    b0 = torch.randn(576, generator=g) * 0.1
    xd = x.cuda()
    assert ops.conv3x3_s2_supported(xd, 576, 1)
    y0 = Guarded((5, 576, 7, 7))
    ops.conv3x3_s2(xd, ops.pack_conv_weight(w0.cuda()), b0.cuda(), 576, splits=1, out=y0.t)
    y0.check('conv 0')
    assert_close_via_f64(y0.t, F.conv2d(x, w0, b0, stride=2, padding=1),
                         F.conv2d(x.double(), w0.double(), b0.double(), stride=2, padding=1), 'conv 0')
    x1 = torch.randn(5, 576, 7, 7, generator=g)
    w1 = torch.randn(576, 576, 3, 3, generator=g) * (2.0 / (9 * 576)) ** 0.5
    y1 = Guarded((5, 576, 7, 7))
    ops.conv2d([x1.cuda()], ops.pack_conv_weight(w1.cuda()), b0.cuda(), 576, 3, out=y1.t)
    y1.check('conv 1')
    assert_close_via_f64(y1.t, F.conv2d(x1, w1, b0, padding=1), F.conv2d(x1.double(), w1.double(), b0.double(), padding=1),
                         'conv 1')
    # a RoI's bits do not depend on the other RoIs of the call (no split-K on this path)
    one = ops.conv2d([x1[3:4].cuda()], ops.pack_conv_weight(w1.cuda()), b0.cuda(), 576, 3)
    assert torch.equal(one, y1.t[3:4])
    one0 = ops.conv3x3_s2(xd[3:4].contiguous(), ops.pack_conv_weight(w0.cuda()), b0.cuda(), 576, splits=1)
    assert torch.equal(one0, y0.t[3:4])


# ------------------------------------------------------------------------------------------------ head and RoI head
@pytest.fixture(scope='module')
def grid(golden_dir):
    """(GridRoIHead on the device with the fixture's seeded weights, the fixture, grid_inputs)."""
    import grid_inputs as gi
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    z = np.load(os.path.join(golden_dir, 'g23_grid.npz'))
    with open(os.path.join(golden_dir, 'g23_grid_configs.json')) as f:
        cfg = registry._to_cfgdict(json.load(f)['r50_2x'])
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=None, test_cfg=cfg.test_cfg.rcnn)
    m = registry.build_head(rh)
    mine = {k: v.shape for k, v in m.state_dict().items() if k.startswith(('bbox_head.', 'grid_head.'))}
    missing = m.load_state_dict(gi.head_state(mine, int(z['weight_seed'])), strict=False)
    assert not missing.unexpected_keys and all(not k.startswith(('bbox_head.', 'grid_head.')) for k in missing.missing_keys)
    return m.cuda().eval(), z, gi


def _class_major(bbox_results):
    dets = np.asarray([row for b in bbox_results for row in b], np.float32).reshape(-1, 5)
    return dets, np.asarray([c for c, b in enumerate(bbox_results) for _ in range(len(b))], np.int64)


def test_head_heatmap_against_the_reference(grid):
    from dynamask_amd.roi_head import bbox2roi
    m, z, gi = grid
    feats = [f.cuda() for f in gi.fpn_feats()]
    det = gi.detections().cuda()
    with torch.no_grad():
        rois = bbox2roi([det[:, :4]]).contiguous()
        pred = m.grid_head(m.grid_roi_extractor(feats, rois))
        boxes = m.grid_head.get_bboxes(det, pred['fused'], gi.img_metas())
    assert pred['unfused'] is pred['fused'] and tuple(pred['fused'].shape) == (8, 9, 28, 28)
    assert_close_via_f64(pred['fused'], z['heat'], z['heat64'], 'fused heatmap')
    assert torch.equal(pred['fused'].view(8, 9, -1).argmax(2).cpu(), torch.from_numpy(z['heat64']).view(8, 9, -1).argmax(2))
    assert_close_via_f64(boxes, z['heat_boxes'], z['heat_boxes64'], 'boxes of the heatmap fixture')


@pytest.mark.parametrize('tag,rescale', [('plain', False), ('rescale', True)])
def test_simple_test_against_the_reference(grid, tag, rescale):
    m, z, gi = grid
    feats = [f.cuda() for f in gi.fpn_feats()]
    props = gi.proposals().cuda()
    metas = gi.img_metas(gi.SCALE_FACTOR if rescale else 1.0)
    res = m.simple_test(feats, [props], metas, rescale=rescale)
    assert len(res) == 80 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res)
    dets, labels = _class_major(res)
    assert len(labels) == len(z[f'{tag}_labels']) and np.array_equal(labels, z[f'{tag}_labels'])
    assert_close_via_f64(dets, z[f'{tag}_dets'], z[f'{tag}_dets64'], f'simple_test rescale={rescale}')
    again = m.simple_test(feats, [props], metas, rescale=rescale)
    assert all(np.array_equal(a, b) for a, b in zip(res, again)), 'two identical calls differ'
    d1, l1 = m.simple_test_grid(feats, [props], metas, rescale=rescale)
    d2, l2 = m.simple_test_grid(feats, [props], metas, rescale=rescale)
    assert torch.equal(d1, d2) and torch.equal(l1, l2)


def test_zero_detections(grid):
    """A score threshold nothing passes: per-class empty (0, 5) arrays, and the grid head launches nothing."""
    from dynamask_amd import ops, registry
    m, z, gi = grid
    feats = [f.cuda() for f in gi.fpn_feats()]
    keep = m.test_cfg
    calls = []
    orig = ops.grid_fusion
    try:
        m.test_cfg = registry._to_cfgdict(dict(keep, score_thr=2.0))
        ops.grid_fusion = lambda *a, **k: calls.append(1) or orig(*a, **k)
        res = m.simple_test(feats, [gi.proposals().cuda()], gi.img_metas())
        batch = m.batch_simple_test([f.repeat(2, 1, 1, 1) for f in feats], [gi.proposals().cuda()] * 2, gi.img_metas() * 2)
    finally:
        m.test_cfg = keep
        ops.grid_fusion = orig
    assert not calls
    for r in [res] + batch:
        assert len(r) == 80 and all(a.shape == (0, 5) and a.dtype == np.float32 for a in r)


def test_batch_equals_one_image_calls(grid):
    m, z, gi = grid
    x2 = [f.cuda() for f in gi.fpn_feats(batch=2)]
    props = [gi.proposals().cuda(), gi.proposals(seed=99, n=13).cuda()]
    for rescale in (False, True):
        sf = gi.SCALE_FACTOR if rescale else 1.0
        metas = gi.img_metas(sf) * 2
        batch = m.batch_simple_test_grid(x2, props, metas, rescale=rescale)
        batch_res = m.batch_simple_test(x2, props, metas, rescale=rescale)
        assert len(batch) == 2 and len(batch_res) == 2
        for b in range(2):
            xb = [f[b:b + 1].contiguous() for f in x2]
            d, lab = m.simple_test_grid(xb, [props[b]], [metas[b]], rescale=rescale)
            assert d.shape[0] > 0
            assert torch.equal(batch[b][0], d) and torch.equal(batch[b][1], lab), f'image {b} rescale={rescale}'
            one = m.simple_test(xb, [props[b]], [metas[b]], rescale=rescale)
            assert all(np.array_equal(p, q) for p, q in zip(batch_res[b], one))
    # image 0 of the batch is the fixture's image
    dets, labels = _class_major(batch_res[0])
    assert np.array_equal(labels, z['rescale_labels'])


def test_bf16x3_mode_changes_no_bit(grid):
    """The grid kernels have no bf16x3 build and GridHead's 3x3 convolutions always take the exact layout: under
    set_conv_precision('bf16x3') every launch of the head gives the bits of the fp32 mode."""
    from dynamask_amd import conv_precision, ops
    m, z, gi = grid
    feats = [f.cuda() for f in gi.fpn_feats()]
    props = gi.proposals().cuda()
    g = _g(77)
    x = torch.randn(3, 576, 7, 7, generator=g).cuda()
    gamma, beta = torch.randn(576, generator=g).cuda(), torch.randn(576, generator=g).cuda()
    tab = _table(_fusion_weights(9, 64, 14), 9, 64)
    w = (torch.randn(576, 64, 4, 4, generator=g) * 0.06).cuda()
    heat = torch.randn(3, 9, 28, 28, generator=g).cuda()
    det = torch.tensor([[10.0, 20.0, 110.0, 90.0, 0.5]] * 3).cuda()

    def run():
        with torch.no_grad():
            feat = m.grid_roi_extractor(feats, torch.cat([props.new_zeros(len(props), 1), props], 1).contiguous())
            return (ops.group_norm(x, gamma, beta, 36, relu=True), ops.grid_fusion(x, x, tab, 9),
                    ops.deconv4x4_s2_grouped(x, w, beta, 9), ops.grid_get_bboxes(heat, det, m.grid_head.sub_regions),
                    m.grid_head(feat)['fused'], m.simple_test_grid(feats, [props], gi.img_metas())[0])
    exact = run()
    with conv_precision('bf16x3'):
        mode = run()
    for a, b in zip(exact, mode):
        assert torch.equal(a, b)
