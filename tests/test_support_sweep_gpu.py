"""The point, grid and head kernels at every shape of tests/support_cases.py, and the grid-stride launchers past their caps.

The family tests run these kernels at the shapes of their own configs; a kernel picks its tile layout from the shape, so
the host's ``dm_*_supported`` predicate and the kernel can only disagree at the shapes the predicate accepts and nobody
runs (tests/test_fused_shapes_gpu.py found the DCN + 1x1 weight stride that way).  Every case here checks
  (a) the result against a float64 CPU reference of the same torch expression the family's test uses
      (``tolerances.assert_close_via_f64`` with the float32 CPU computation as ``ref32``; ``rel`` as in the family's test),
  (b) ``torch.equal`` where the kernel is exact: the selects (against the stable sort of the key, cut at P, ascending),
      the copied coarse channels of dm_point_feat_gather, the cells nobody selected, the cells of dm_grid_get_bboxes,
  (c) the fused and the unfused form against each other where both exist, in the relation the family's test holds,
  (d) guard bands of a canary on both sides of the output,
  (e) for every refused neighbour: the predicate says no, the entry point returns DM_ERR_UNSUPPORTED, the output keeps
      its bits.
The sampled coarse channels of dm_point_gather_fwd are bilinear samples, not copies: they go through (a) like the fine
ones (``rel = 1e-5``, tests/test_pointrend_gpu.py).  The second half sends each capped grid-stride launcher of
support_cases.CAPPED round its loop a second time on planes of one or two pixels: every element against a closed form
computed on the device, and the first, the last and the planes around item ``cap * 256`` against float64 on the host."""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import support_cases as sc
from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

CANARY = 7.0
ICANARY = -12345
GUARD = 4096
UNSUPPORTED = -3


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _vp(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Guarded:
    """A device tensor of ``shape`` between two guard bands of a canary."""

    def __init__(self, shape, fill=None, dtype=torch.float32):
        n = int(np.prod(shape))
        self.canary = CANARY if dtype == torch.float32 else ICANARY
        self.buf = torch.full((n + 2 * GUARD,), self.canary, device='cuda', dtype=dtype)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == self.canary).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == self.canary).all()), f'{what}: the guard band past the output was overwritten'


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    return o


@pytest.fixture(scope='module')
def L():
    from dynamask_amd._lib import lib
    return lib()


def _sorted_cells(n, HW, P, g):
    return torch.stack([torch.sort(torch.randperm(HW, generator=g)[:P]).values for _ in range(n)]).int()


# ================================================================================================ point MLP (PointRend)
def _point_mlp_ref(x, ws, bs, wl, bl, dtype):
    """MaskPointHead.forward (coarse_pred_each_layer) -> all-class logits [n, NCL, P] (tests/test_pointrend_gpu.py _mlp_ref)."""
    x = x.to(dtype)
    crs = x[:, 256:]
    h = x
    for w, b in zip(ws, bs):
        h = torch.cat([torch.relu(torch.einsum('ok,nkp->nop', w.to(dtype), h) + b.to(dtype)[None, :, None]), crs], 1)
    return torch.einsum('ok,nkp->nop', wl.to(dtype), h) + bl.to(dtype)[None, :, None]


@pytest.mark.parametrize('NC,nfc', sorted({(r[3], r[5]) for r in sc.POINT_MLP_RUN}))
def test_point_mlp(ops, NC, nfc):
    CT = 256 + NC
    g = _g(7000 + NC + nfc)
    ws = [torch.randn(256, CT, generator=g) * (2.0 / CT) ** 0.5 for _ in range(nfc)]
    bs = [torch.randn(256, generator=g) * 0.1 for _ in range(nfc)]
    wl_all, bl_all = torch.randn(81, CT, generator=g) * 0.05, torch.randn(81, generator=g) * 0.1
    wq = [ops.pack_conv_weight(w[:, :, None, None].contiguous().cuda()) for w in ws]
    bd = [b.cuda() for b in bs]
    rows = [r for r in sc.POINT_MLP_RUN if (r[3], r[5]) == (NC, nfc)]
    for n, P, C, _, Fc, _, NCL, HW in rows:
        assert (C, Fc) == (256, 256)
        x = torch.randn(n, CT, P, generator=g)
        assert ops.point_mlp_supported(x, nfc, NCL, HW)
        wl, bl = wl_all[:NCL].contiguous(), bl_all[:NCL].contiguous()
        labels = torch.tensor([0, NCL - 1] + [NCL // 2] * (n - 2))[:n]
        idx = _sorted_cells(n, HW, P, g)
        refined = torch.randn(n, 1, HW, generator=g)
        ar = torch.arange(n)
        r32, r64 = refined.clone(), refined.double()
        r32.view(n, HW).scatter_(1, idx.long(), _point_mlp_ref(x, ws, bs, wl, bl, torch.float32)[ar, labels])
        r64.view(n, HW).scatter_(1, idx.long(), _point_mlp_ref(x, ws, bs, wl, bl, torch.float64)[ar, labels])
        keep = torch.ones(n, HW, dtype=torch.bool)
        keep.scatter_(1, idx.long(), False)
        outs = {}
        for fused in (True, False):
            what = f'point MLP fused={fused} NC={NC} nfc={nfc} P={P} HW={HW} NCL={NCL}'
            out = Guarded((n, 1, HW), refined)
            ops.point_mlp_scatter(x.cuda(), wq, bd, wl.cuda(), bl.cuda(), labels.cuda(), idx.cuda(), out.t, fused=fused)
            out.check(what)
            got = out.t.cpu()
            assert torch.equal(got.view(n, HW)[keep], refined.view(n, HW)[keep]), f'{what}: cells that were not selected changed'
            assert_close_via_f64(got, r32, r64, what, rel=1e-5)
            outs[fused] = got
        np.testing.assert_allclose(outs[True].numpy(), outs[False].numpy(), rtol=1e-5, atol=1e-5)


# ================================================================================================ point MLP (PointRefine)
def _refine_mlp_ref(x, ws, bs, feat, idx, dt):
    """SFMStage's point MLP and its scatter (tests/test_pointrefine_gpu.py _mlp_ref), feat [n, C, HW]."""
    n, CT, P = x.shape
    C = ws[0].shape[0]
    x, feat = x.to(dt), feat.to(dt).clone()
    coarse, h = x[:, C:], x[:, :C]
    for i in range(len(ws)):
        y = torch.einsum('ok,nkp->nop', ws[i].to(dt), torch.cat([h, coarse], 1)) + bs[i].to(dt)[None, :, None]
        h = y.clamp_min(0) if i < len(ws) - 1 else y
    cell = torch.arange(P).repeat(n, 1) if idx is None else idx.long()
    feat.scatter_(2, cell[:, None].expand(-1, C, -1), h)
    return feat


@pytest.mark.parametrize('C,NC,nfc', sc.REFINE_CNF)
def test_point_refine_mlp(ops, C, NC, nfc):
    CT = C + NC
    g = _g(8000 + C + NC + nfc)
    ws = [torch.randn(C, CT, generator=g) * (2.0 / CT) ** 0.5 for _ in range(nfc + 1)]
    bs = [torch.randn(C, generator=g) * 0.1 for _ in range(nfc + 1)]
    wq = [ops.pack_conv_weight(w.cuda().view(C, CT, 1, 1).contiguous()) for w in ws]
    bd = [b.cuda() for b in bs]
    rows = [r for r in sc.REFINE_MLP_RUN if (r[2], r[3], r[4]) == (C, NC, nfc)]
    assert len(rows) == 7
    for n, P, _, _, _, HW, has_idx in rows:
        assert ops.point_refine_mlp_supported(n, C, NC, P, nfc, HW, has_idx=bool(has_idx))
        x = torch.randn(n, CT, P, generator=g)
        feat = torch.randn(n, C, HW, generator=g)
        idx = _sorted_cells(n, HW, P, g) if has_idx else None
        r32, r64 = _refine_mlp_ref(x, ws, bs, feat, idx, torch.float32), _refine_mlp_ref(x, ws, bs, feat, idx, torch.float64)
        outs = {}
        for form in ('fused', 'unfused'):
            what = f'refine MLP {form} C={C} NC={NC} nfc={nfc} P={P} HW={HW} idx={has_idx}'
            out = Guarded((n, C, HW), feat)
            ops.point_refine_mlp(x.cuda(), C, wq, bd, None if idx is None else idx.cuda(), out.t, form=form)
            out.check(what)
            got = out.t.cpu()
            assert_close_via_f64(got, r32, r64, what, rel=1e-5)
            if idx is not None:
                keep = torch.ones(n, HW, dtype=torch.bool)
                keep.scatter_(1, idx.long(), False)
                assert torch.equal(got.permute(0, 2, 1)[keep], feat.permute(0, 2, 1)[keep]), f'{what}: unselected cells changed'
            outs[form] = got
        assert_grad_close(outs['fused'], outs['unfused'], f'fused vs unfused C={C} NC={NC} nfc={nfc} P={P}', rel=1e-4)


# ================================================================================================ the selects
def _f32_from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def _order_key(ops, mode, m):
    """float64 [n, HW], SMALLER is better: |v|; -v; -sigmoid(v) with the library's own logistic (the key the header names)."""
    if mode == 'mag':
        return np.abs(m.numpy().astype(np.float64))
    if mode == 'raw':
        return -m.numpy().astype(np.float64) + 0.0          # (+ 0.0: -0 and +0 are one key)
    return -ops.sigmoid(m.cuda()).cpu().numpy().astype(np.float64)


def _select_ref(key, P):
    """The stable sort of the key, cut at P, indices ascending: the lower flat index first among equal keys at the cut."""
    order = np.argsort(key, axis=1, kind='stable')[:, :P]
    return torch.from_numpy(np.sort(order, axis=1).astype(np.int32))


def _select_inputs(mode, n, HW, P, seed):
    g = _g(seed)
    i = np.arange(n * HW, dtype=np.uint64)
    zeros = torch.randn(n, HW, generator=g)
    flat = zeros.view(-1)
    flat[0::3] = 0.0
    flat[1::3] = -0.0
    sign = ((i * 31 >> 3) & 1).astype(np.uint32) << 31
    return {
        'random': torch.randn(n, HW, generator=g),
        'constant': torch.full((n, HW), 0.5),
        'tie at the cut': torch.stack([sc.cut_tie_map(mode, HW, P, g) for _ in range(n)]),
        'shared upper 24 bits': _f32_from_bits(0x3F800000 | ((i * 37 + 11) & 255).astype(np.uint32)).view(n, HW),
        '+0 and -0': zeros,
        'denormals': _f32_from_bits(((i * 7919) % 1000 + 1).astype(np.uint32) | sign).view(n, HW),
    }


def _run_select(ops, mode, m, P, out):
    if mode == 'mag':
        return ops.point_select(m, P, out=out)
    return ops.point_topk_select(m, P, use_sigmoid=(mode == 'sigmoid'), out=out)


@pytest.mark.parametrize('HW', sc.SELECT_HW)
@pytest.mark.parametrize('mode', sc.SELECT_MODES)
def test_select(ops, L, mode, HW):
    for n, _, P in [r for r in sc.SELECT_RUN if r[1] == HW]:
        if mode == 'mag':
            assert L.dm_point_select_supported(n, HW, P) == 1
        else:
            assert L.dm_point_topk_select_supported(n, HW, P, 1 if mode == 'sigmoid' else 0) == 1
        for kind, m in _select_inputs(mode, n, HW, P, 9000 + 7 * HW + P + n).items():
            m = m.contiguous()
            what = f'select {mode} n={n} HW={HW} P={P} on {kind}'
            out = Guarded((n, P), dtype=torch.int32)
            _run_select(ops, mode, m.cuda(), P, out.t)
            out.check(what)
            ref = _select_ref(_order_key(ops, mode, m), P)
            assert torch.equal(out.t.cpu(), ref), what
            if kind == 'constant':
                assert torch.equal(ref, torch.arange(P, dtype=torch.int32).expand(n, P)), what


def test_select_largest_map(ops, L):
    """HW = 2^24 (SEL_MAX_HW, point_refine.hip:31), P = 2^12, one row.  Measured on the MI355X: 44 ms for the launch."""
    n, HW, P = sc.SELECT_BIG
    assert L.dm_point_select_supported(n, HW, P) == 1
    torch.manual_seed(5)
    m = torch.randn(n, HW, device='cuda')
    out = Guarded((n, P), dtype=torch.int32)
    ops.point_select(m[:, :4096].contiguous(), 16)                 # (the first launch loads the code object)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.point_select(m, P, out=out.t)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f'dm_point_select at HW = 2^24, P = 2^12: {ms:.1f} ms on the device')
    out.check('select at 2^24')
    a = np.abs(m.cpu().numpy().astype(np.float64))[0]
    cut = np.partition(a, P - 1)[P - 1]
    below = np.flatnonzero(a < cut)
    ref = np.sort(np.concatenate([below, np.flatnonzero(a == cut)[:P - len(below)]])).astype(np.int32)
    assert torch.equal(out.t.cpu()[0], torch.from_numpy(ref))


# ================================================================================================ the gathers
FEAT_H, FEAT_W, SCALE = 6, 9, 0.25      # a 24 x 36 image at stride 4


def _gather_rois():
    """image 0, image 1, an image index outside the batch, partly outside the map, wholly outside it (zero samples)."""
    return torch.tensor([[0.0, 2.0, 3.0, 20.0, 15.0], [1.0, 5.5, 1.25, 30.0, 22.0], [7.0, 2.0, 3.0, 20.0, 15.0],
                         [0.0, -10.0, -8.0, 12.0, 30.0], [1.0, 100.0, 100.0, 140.0, 130.0]])


def _point_sample(inp, pts):
    return F.grid_sample(inp, pts.unsqueeze(2) * 2.0 - 1.0, align_corners=False).squeeze(3)


def _centres(idx, mh, mw, dtype):
    """get_roi_rel_points_test's cell centres (fp32 chain when dtype is float32): tests/test_pointrend_gpu.py."""
    w_step, h_step = 1.0 / mw, 1.0 / mh
    px = w_step / 2.0 + (idx % mw).to(dtype) * w_step
    py = h_step / 2.0 + (idx // mw).to(dtype) * h_step
    return torch.stack([px, py], -1)


def _gather_ref(feat, rois, coarse, idx, mh, mw, scale, dtype, sample_coarse):
    """[n, C + NC, P]: the fine channels of point_rend_roi_head._get_fine_grained_point_feats (zeros for a RoI of no image
    of the batch); the coarse ones point_sample'd (dm_point_gather_fwd) or gathered (dm_point_feat_gather)."""
    feat, rois, coarse = feat.to(dtype), rois.to(dtype), coarse.to(dtype)
    rel = _centres(idx.long(), mh, mw, dtype)
    B, C, H, W = feat.shape
    n, NC = coarse.shape[:2]
    out = []
    for r in range(n):
        b = int(rois[r, 0])
        if 0 <= b < B:
            ab = rel[r].clone()
            ab[:, 0] = ab[:, 0] * (rois[r, 3] - rois[r, 1]) + rois[r, 1]
            ab[:, 1] = ab[:, 1] * (rois[r, 4] - rois[r, 2]) + rois[r, 2]
            img = ab / torch.tensor([W, H], dtype=dtype) * scale
            fine = _point_sample(feat[b:b + 1], img[None])[0]
        else:
            fine = torch.zeros(C, idx.shape[1], dtype=dtype)
        if sample_coarse:
            crs = _point_sample(coarse[r:r + 1], rel[r][None])[0]
        else:
            crs = torch.gather(coarse[r].reshape(NC, -1), 1, idx[r].long()[None].expand(NC, -1))
        out.append(torch.cat([fine, crs], 0))
    return torch.stack(out)


@pytest.mark.parametrize('C,NC', sorted({(r[1], r[5]) for r in sc.GATHER_RUN}))
def test_point_gather(ops, L, C, NC):
    g = _g(10000 + C + NC)
    rois = _gather_rois()
    feat = torch.randn(2, C, FEAT_H, FEAT_W, generator=g)
    for row in [r for r in sc.GATHER_RUN if (r[1], r[5]) == (C, NC)]:
        B, _, H, W, n, _, CH, CW, P, MH, MW = row
        assert L.dm_point_gather_supported(*row) == 1 and (B, H, W, n) == (2, FEAT_H, FEAT_W, len(rois))
        coarse = torch.randn(n, NC, CH, CW, generator=g)
        idx = _sorted_cells(n, MH * MW, P, g)
        what = f'point_gather C={C} NC={NC} coarse {CH}x{CW} grid {MH}x{MW} P={P}'
        out = Guarded((n, C + NC, P))
        ops.point_gather(feat.cuda(), rois.cuda(), coarse.cuda(), idx.cuda(), MH, MW, SCALE, out=out.t)
        out.check(what)
        got = out.t.cpu()
        r32 = _gather_ref(feat, rois, coarse, idx, MH, MW, SCALE, torch.float32, True)
        r64 = _gather_ref(feat, rois, coarse, idx, MH, MW, SCALE, torch.float64, True)
        assert_close_via_f64(got[:, :C], r32[:, :C], r64[:, :C], what + ' fine', rel=1e-5)
        assert_close_via_f64(got[:, C:], r32[:, C:], r64[:, C:], what + ' coarse', rel=1e-5)
        assert bool((got[2, :C] == 0).all()), f'{what}: a RoI of no image of the batch has fine channels'
        assert bool((got[4, :C] == 0).all()) and bool((r64[4, :C] == 0).all()), f'{what}: a RoI wholly outside the map samples it'
        if P == MH * MW:
            assert bool((r64[3, :C] != 0).any()), f'{what}: the RoI partly outside the map samples nothing'


@pytest.mark.parametrize('C,NC', sorted({(r[1], r[5]) for r in sc.FEAT_GATHER_RUN}))
def test_point_feat_gather(ops, L, C, NC):
    g = _g(11000 + C + NC)
    rois = _gather_rois()
    feat = torch.randn(2, C, FEAT_H, FEAT_W, generator=g)
    for row in [r for r in sc.FEAT_GATHER_RUN if (r[1], r[5]) == (C, NC)]:
        B, _, H, W, n, _, P, S, has_idx = row
        assert L.dm_point_feat_gather_supported(*row) == 1 and (B, H, W, n) == (2, FEAT_H, FEAT_W, len(rois))
        coarse = torch.randn(n, NC, S, S, generator=g)
        idx = _sorted_cells(n, S * S, P, g) if has_idx else None
        idx_full = idx if has_idx else torch.arange(P, dtype=torch.int32).repeat(n, 1)
        what = f'point_feat_gather C={C} NC={NC} S={S} P={P} idx={has_idx}'
        out = Guarded((n, C + NC, P))
        ops.point_feat_gather(feat.cuda(), rois.cuda(), coarse.cuda(), None if idx is None else idx.cuda(), SCALE, out=out.t)
        out.check(what)
        got = out.t.cpu()
        r32 = _gather_ref(feat, rois, coarse, idx_full, S, S, SCALE, torch.float32, False)
        r64 = _gather_ref(feat, rois, coarse, idx_full, S, S, SCALE, torch.float64, False)
        assert_close_via_f64(got[:, :C], r32[:, :C], r64[:, :C], what + ' fine')
        assert torch.equal(got[:, C:], r32[:, C:]), f'{what}: the coarse channels are copies'
        assert bool((got[2, :C] == 0).all()) and bool((got[4, :C] == 0).all()), what


# ================================================================================================ the Grid head
@pytest.mark.parametrize('G,ci,co', sorted({r[1:4] for r in sc.DECONV_RUN}))
def test_deconv4x4_s2_grouped(ops, G, ci, co):
    g = _g(12000 + 100 * G + ci + co)
    w = torch.randn(G * ci, co, 4, 4, generator=g) * (1.0 / (4 * ci)) ** 0.5
    b = torch.randn(G * co, generator=g) * 0.1
    wd, bd = w.cuda(), b.cuda()
    rows = [r for r in sc.DECONV_RUN if r[1:4] == (G, ci, co)]
    assert len(rows) == 8
    for N, _, _, _, S in rows:
        x = torch.randn(N, G * ci, S, S, generator=g)
        xd = x.cuda()
        assert ops.deconv4x4_s2_grouped_supported(xd, G * co, G)
        what = f'deconv G={G} {ci}->{co} S={S} N={N}'
        out = Guarded((N, G * co, 2 * S, 2 * S))
        ops.deconv4x4_s2_grouped(xd, wd, bd, G, out=out.t)
        out.check(what)
        r32 = F.conv_transpose2d(x, w, b, stride=2, padding=1, groups=G)
        r64 = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1, groups=G)
        assert_close_via_f64(out.t, r32, r64, what)
        assert torch.equal(xd.cpu(), x), f'{what}: the input was modified'


def _fusion_weights(ops, P, c, seed):
    g = _g(seed)
    return [[(torch.randn(c, 1, 5, 5, generator=g) * (1.0 / 25) ** 0.5, torch.randn(c, generator=g) * 0.1,
              torch.randn(c, c, 1, 1, generator=g) * (1.0 / c) ** 0.5, torch.randn(c, generator=g) * 0.1) for _ in nb]
            for nb in ops.grid_neighbors(P)]


def _fusion_ref(ops, x, src, trans, P, c, dtype):
    """grid_head.py:157-170 restated (tests/test_grid_gpu.py _fusion_ref)."""
    x, src = x.to(dtype), src.to(dtype)
    outs = []
    for i, nb in enumerate(ops.grid_neighbors(P)):
        acc = x[:, i * c:(i + 1) * c]
        for j, p in enumerate(nb):
            dw_w, dw_b, w1, b1 = (t.to(dtype) for t in trans[i][j])
            acc = acc + F.conv2d(F.conv2d(src[:, p * c:(p + 1) * c], dw_w, dw_b, padding=2, groups=c), w1, b1)
        outs.append(acc)
    return torch.cat(outs, 1)


@pytest.mark.parametrize('P,c,S', sc.FUSION_SHAPES)
def test_grid_fusion(ops, P, c, S):
    trans = _fusion_weights(ops, P, c, 13000 + P + c + S)
    table = ops.pack_grid_fusion_table([[tuple(t.cuda() for t in slot) for slot in point] for point in trans], P, c)
    rows = [r for r in sc.FUSION_RUN if r[1:] == (P, c, S)]
    assert [r[0] for r in rows] == [1, 3]
    for N, _, _, _ in rows:
        g = _g(N + S)
        x, src = torch.randn(N, P * c, S, S, generator=g), torch.randn(N, P * c, S, S, generator=g)
        xd = x.cuda()
        assert ops.grid_fusion_supported(xd, P)
        what = f'fusion P={P} c={c} S={S} N={N}'
        for s, tag in ((x, 'first order'), (src, 'second order')):          # src = x, and a src of its own
            out = Guarded(x.shape)
            ops.grid_fusion(xd, xd if s is x else s.cuda(), table, P, out=out.t)
            out.check(f'{what} {tag}')
            assert_close_via_f64(out.t, _fusion_ref(ops, x, s, trans, P, c, torch.float32),
                                 _fusion_ref(ops, x, s, trans, P, c, torch.float64), f'{what} {tag}')
        assert torch.equal(xd.cpu(), x), f'{what}: the input was modified'


def _vote(det, scores, cells, sub_x, sub_y, HS, dtype):
    """grid_head.py:313-355 restated from the cells of the maxima (tests/test_grid_gpu.py _vote)."""
    P = scores.shape[1]
    gs = int(round(P ** 0.5))
    det, scores = det.to(dtype), scores.to(dtype)
    xs = (cells % HS + torch.tensor(sub_x)).to(dtype)
    ys = (cells // HS + torch.tensor(sub_y)).to(dtype)
    w, h = (det[:, 2] - det[:, 0])[:, None], (det[:, 3] - det[:, 1])[:, None]
    ax = (xs + 0.5) / HS * w + (det[:, 0, None] - w / 2)
    ay = (ys + 0.5) / HS * h + (det[:, 1, None] - h / 2)
    sides = ((ax, list(range(gs))), (ay, [i * gs for i in range(gs)]), (ax, [P - gs + i for i in range(gs)]),
             (ay, [(i + 1) * gs - 1 for i in range(gs)]))
    cols = [(a[:, idx] * scores[:, idx]).sum(1) / scores[:, idx].sum(1) for a, idx in sides]
    return torch.stack(cols + [det[:, -1]], 1)


@pytest.mark.parametrize('HS,P', sorted({(r[2], r[1]) for r in sc.GET_BBOXES_RUN}))
def test_grid_get_bboxes(ops, L, HS, P):
    """Sample 0 has every point's maximum in the first cell, sample 1 in the last, sample 2 twice (the earlier cell wins);
    the background is a ramp below every planted logit.  The reference votes from the planted cells and logits."""
    n, cells = 3, HS * HS
    base = (torch.arange(cells, device='cuda') % 97).float() * 0.01 - 5.0            # -5 .. -4.04
    heat = base.repeat(n * P).view(n, P, cells)
    want = torch.zeros(n, P, dtype=torch.long)
    logit = torch.zeros(n, P)
    first, second = cells // 3, cells - 1
    for p in range(P):
        logit[0, p], logit[1, p], logit[2, p] = 1.5 + 0.1 * p, 2.0 - 0.1 * p, 1.0 + 0.05 * p
        want[1, p], want[2, p] = cells - 1, first
        heat[0, p, 0] = float(logit[0, p])
        heat[1, p, cells - 1] = float(logit[1, p])
        heat[2, p, second] = float(logit[2, p])
        heat[2, p, first] = float(logit[2, p])
    heat = heat.view(n, P, HS, HS)
    sub_x, sub_y = [3 * p for p in range(P)], [(5 * p) % 7 for p in range(P)]
    sub = [(sub_x[p], sub_y[p], 0, 0) for p in range(P)]
    for D in sorted({r[3] for r in sc.GET_BBOXES_RUN if (r[2], r[1]) == (HS, P)}):
        assert L.dm_grid_get_bboxes_supported(n, P, HS, D) == 1
        det = torch.tensor([[10.0, 20.0, 110.0, 90.0], [2.0, 2.0, 50.0, 50.0], [40.0, 30.0, 140.0, 170.0]])
        det = torch.cat([det, torch.tensor([[0.125], [0.25], [0.375]]).repeat(1, D - 5), torch.tensor([[0.5], [0.25], [0.75]])], 1)
        what = f'get_bboxes HS={HS} P={P} D={D}'
        out = Guarded((n, 5))
        _, got_cells = ops.grid_get_bboxes(heat, det.cuda(), sub, out=out.t, return_cells=True)
        out.check(what)
        assert torch.equal(got_cells.cpu().long(), want), what
        sc32, sc64 = torch.sigmoid(logit), torch.sigmoid(logit.double())
        assert_close_via_f64(out.t, _vote(det, sc32, want, sub_x, sub_y, HS, torch.float32),
                             _vote(det, sc64, want, sub_x, sub_y, HS, torch.float64), what)
        assert torch.equal(out.t[:, 4].cpu(), det[:, -1])


# ================================================================================================ strided, dilated, pooled
def _conv_case(NB, C, H, W, cout, seed):
    g = _g(seed)
    x = torch.randn(NB, C, H, W, generator=g) + torch.arange(NB, dtype=torch.float32).view(NB, 1, 1, 1) * 0.01
    w = torch.randn(cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize('NB,C,H,W', sorted({r[:4] for r in sc.CONV_S2_RUN}))
def test_conv3x3_s2(ops, NB, C, H, W):
    rows = [r for r in sc.CONV_S2_RUN if r[:4] == (NB, C, H, W)]
    for cout in sorted({r[4] for r in rows}):
        x, w, b = _conv_case(NB, C, H, W, cout, 14000 + C + 31 * H + W + cout)
        xd, wq, bd = x.cuda(), ops.pack_conv_weight(w.cuda()), b.cuda()
        r32 = F.relu(F.conv2d(x, w, b, stride=2, padding=1))
        r64 = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))
        for splits in [r[5] for r in rows if r[4] == cout]:
            assert ops.conv3x3_s2_supported(xd, cout, splits)
            what = f'conv3x3_s2 NB={NB} C={C} {H}x{W} Cout={cout} splits={splits}'
            out = Guarded(tuple(r64.shape))
            ops.conv3x3_s2(xd, wq, bd, cout, relu=True, splits=splits, out=out.t)
            out.check(what)
            assert_close_via_f64(out.t, r32, r64, what, rel=1e-5)


def _dil_ref(x, w, b, d, dt):
    return F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=d, dilation=d).clamp_min(0)


@pytest.mark.parametrize('C,cout,d', sorted({(r[1], r[4], r[5]) for r in sc.DIL_RUN}))
def test_conv3x3_dil(ops, C, cout, d):
    for NB, _, H, W, _, _ in [r for r in sc.DIL_RUN if (r[1], r[4], r[5]) == (C, cout, d)]:
        x, w, b = _conv_case(NB, C, H, W, cout, 15000 + 17 * H + W + cout + d)
        xd = x.cuda()
        assert ops.conv3x3_dil_supported(xd, cout, d)
        what = f'conv3x3_dil C={C} {H}x{W} Cout={cout} d={d}'
        out = Guarded((NB, cout, H, W))
        ops.conv3x3_dil(xd, ops.pack_conv_weight(w.cuda()), b.cuda(), cout, d, relu=True, out=out.t)
        out.check(what)
        assert_close_via_f64(out.t, _dil_ref(x, w, b, d, torch.float32), _dil_ref(x, w, b, d, torch.float64), what)


@pytest.mark.parametrize('NB,C,H,W,cout,dil', sc.MULTIDIL_RUN)
def test_conv3x3_multidil(ops, NB, C, H, W, cout, dil):
    g = _g(16000 + H + W + cout)
    x = torch.randn(NB, C, H, W, generator=g)
    ws = [torch.randn(cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5 for _ in dil]
    bs = [torch.randn(cout, generator=g) * 0.1 for _ in dil]
    xd, wq, bd = x.cuda(), [ops.pack_conv_weight(w.cuda()) for w in ws], [b.cuda() for b in bs]
    assert ops.conv3x3_multidil_supported(xd, cout, dil)
    outs = {}
    for fused in (True, False):
        out = Guarded((NB, cout, H, W))
        ops.conv3x3_multidil(xd, wq, bd, cout, dil, out=out.t, fused=fused)
        out.check(f'multidil fused={fused}')
        outs[fused] = out.t.cpu()
    assert torch.equal(outs[True], outs[False]), 'fused and unfused branch sums differ'
    r32 = sum(_dil_ref(x, w, b, d, torch.float32) for w, b, d in zip(ws, bs, dil))
    r64 = sum(_dil_ref(x, w, b, d, torch.float64) for w, b, d in zip(ws, bs, dil))
    assert_close_via_f64(outs[True], r32, r64, f'multidil {H}x{W} Cout={cout} d={dil}')


@pytest.mark.parametrize('n,C,H,W', sc.MASK_IOU_RUN)
def test_mask_iou_input(L, n, C, H, W):
    g = _g(17000 + C + H + W)
    pred = torch.randn(n, C, H, W, generator=g) * 4
    labels = torch.tensor([0, C - 1, C // 2])[:n]
    ho, wo = H // 2, W // 2
    out = Guarded((n, 1, ho, wo))
    pd, ld = pred.cuda(), labels.cuda()
    assert L.dm_mask_iou_input_supported(n, C, H, W) == 1
    assert L.dm_mask_iou_input(_vp(pd), n, C, H, W, _vp(ld if C > 1 else None), _vp(out.t), None) == 0
    out.check(f'mask_iou_input C={C} {H}x{W}')
    sel = pred[torch.arange(n), labels]
    r32 = F.max_pool2d(torch.sigmoid(sel)[:, None], 2, 2)
    r64 = F.max_pool2d(torch.sigmoid(sel.double())[:, None], 2, 2)
    assert tuple(r64.shape) == (n, 1, ho, wo)
    assert_close_via_f64(out.t, r32, r64, f'mask_iou_input C={C} {H}x{W}')


@pytest.mark.parametrize('HW', sorted({r[2] for r in sc.GAP_RUN}))
def test_global_avg_pool(ops, HW):
    for N, C, _ in [r for r in sc.GAP_RUN if r[2] == HW]:
        x = torch.randn(N, C, HW, 1, generator=_g(18000 + N * C + HW)) * 2.0 + 0.5
        xd = x.cuda()
        assert ops.global_avg_pool_supported(xd)
        out = Guarded((N, C))
        ops.global_avg_pool(xd, out=out.t)
        out.check(f'global_avg_pool {N}x{C}x{HW}')
        assert_close_via_f64(out.t, x.mean((2, 3)), x.double().mean((2, 3)), f'global_avg_pool {N}x{C}x{HW}')


# ================================================================================================ refused neighbours
def _ptrs(t, k):
    return (ctypes.c_void_p * k)(*[t.data_ptr()] * k)


def _refused_call(L, name, row, d, di, out, iout):
    """The entry point behind predicate ``name`` at the refused ``row``: inputs from the scratch tensors ``d`` (float) and
    ``di`` (int), outputs into ``out`` / ``iout``.  Nothing is launched, so the scratch sizes do not matter."""
    x, xi, o, oi = _vp(d), _vp(di), _vp(out), _vp(iout)
    if name == 'dm_point_mlp_supported':
        n, P, C, NC, Fc, nfc, NCL, HW = row
        return L.dm_point_mlp_fwd(x, n, P, C, NC, Fc, nfc, _ptrs(d, 8), _ptrs(d, 8), x, x, NCL, xi, xi, 0, o, HW, None)
    if name == 'dm_point_refine_mlp_supported':
        n, P, C, NC, nfc, HW, has_idx = row
        return L.dm_point_refine_mlp(x, n, P, C, NC, nfc, _ptrs(d, 8), _ptrs(d, 8), xi if has_idx else None, 0, o, HW, None)
    if name == 'dm_point_select_supported':
        return L.dm_point_select(x, *row, oi, None)
    if name == 'dm_point_topk_select_supported':
        return L.dm_point_topk_select(x, *row, oi, None)
    if name == 'dm_point_gather_supported':
        B, C, H, W, n, NC, CH, CW, P, MH, MW = row
        return L.dm_point_gather_fwd(x, B, C, H, W, x, n, x, NC, CH, CW, xi, P, MH, MW, SCALE, o, None)
    if name == 'dm_point_feat_gather_supported':
        B, C, H, W, n, NC, P, S, has_idx = row
        return L.dm_point_feat_gather(x, B, C, H, W, x, n, x, NC, xi if has_idx else None, P, S, SCALE, o, None)
    if name == 'dm_deconv4x4_s2_grouped_supported':
        return L.dm_deconv4x4_s2_grouped_fwd(x, *row, x, x, o, None)
    if name == 'dm_grid_fusion_supported':
        return L.dm_grid_fusion_fwd(x, x, *row, x, o, None)
    if name == 'dm_grid_get_bboxes_supported':
        n, P, HS, D = row
        sub = (ctypes.c_int * 16)()
        return L.dm_grid_get_bboxes(x, n, P, HS, x, D, sub, sub, o, oi, None)
    if name == 'dm_conv3x3_s2_supported':
        NB, C, H, W, cout, splits = row
        return L.dm_conv3x3_s2_fwd(x, NB, C, H, W, x, x, cout, splits, 0, o, x, d.numel(), None)
    if name == 'dm_conv3x3_dil_supported':
        NB, C, H, W, cout, dil = row
        return L.dm_conv3x3_dil_fwd(x, NB, C, H, W, x, x, cout, dil, 0, o, None)
    if name == 'dm_conv3x3_multidil_supported':
        NB, C, H, W, cout, dil = row
        return L.dm_conv3x3_multidil_fwd(x, NB, C, H, W, _ptrs(d, 4), _ptrs(d, 4), cout, len(dil), (ctypes.c_int * len(dil))(*dil),
                                         0, o, None)
    if name == 'dm_mask_iou_input_supported':
        return L.dm_mask_iou_input(x, *row, xi, o, None)
    if name == 'dm_global_avg_pool_supported':
        return L.dm_global_avg_pool_fwd(x, *row, o, None)
    raise KeyError(name)


@pytest.mark.parametrize('name', sorted(sc.TABLES))
def test_refused_neighbours_return_unsupported_and_touch_nothing(L, name):
    d = torch.zeros(1 << 16, device='cuda')
    di = torch.zeros(1 << 16, device='cuda', dtype=torch.int64)
    out = torch.full((1 << 16,), CANARY, device='cuda')
    iout = torch.full((1 << 16,), ICANARY, device='cuda', dtype=torch.int32)
    for row in sc.TABLES[name][1]:
        if name == 'dm_conv3x3_multidil_supported':
            ok = L.dm_conv3x3_multidil_supported(*row[:-1], len(row[-1]), (ctypes.c_int * len(row[-1]))(*row[-1]))
        else:
            ok = getattr(L, name)(*row)
        assert ok == 0, f'{name}{row}'                        # (asked first: an accepted row would launch on the scratch)
        assert _refused_call(L, name, row, d, di, out, iout) == UNSUPPORTED, f'{name}{row}'
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((iout == ICANARY).all()), f'{name}: a refused call wrote to its output'


def test_refused_shapes_raise_through_the_wrappers(ops):
    """The same through ``ops``: a RuntimeError, the output as it was."""
    iout = torch.full((1, 65), ICANARY, device='cuda', dtype=torch.int32)
    out = torch.full((2, 72, 16, 16), CANARY, device='cuda')
    with pytest.raises(RuntimeError, match='not supported'):
        ops.point_select(torch.zeros(1, 64, device='cuda'), 65, out=iout)
    with pytest.raises(RuntimeError, match='not supported'):
        ops.point_topk_select(torch.zeros(1, 64, device='cuda'), 65, out=iout)
    with pytest.raises(RuntimeError, match='not supported'):
        ops.deconv4x4_s2_grouped(torch.zeros(2, 72, 8, 8, device='cuda'), torch.zeros(72, 8, 4, 4, device='cuda'), None, 9, out=out)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((iout == ICANARY).all())


# ================================================================================================ the capped grids
def _planes_around(item_edge, items_per_plane, NC):
    """The first plane, the last, and the planes that hold the items either side of ``item_edge`` = cap * 256."""
    s = item_edge // items_per_plane
    return sorted({0, NC - 1} | {p for p in (s - 1, s, s + 1) if 0 <= p < NC})


def _cap(name):
    return sc.CAPPED[name][3]


def _ramp(NC):
    """float(k % 8191) per plane k: exact in fp32, and no two planes 8191 apart share it with their neighbours' order."""
    return (torch.arange(NC, device='cuda') % 8191).float()


def _sample(got, ref32, ref64, what):
    assert torch.equal(got.cpu().double(), ref64), f'{what}: the sampled planes differ from float64'
    assert torch.equal(ref32.double(), ref64)


def test_capped_maxpool3x3_s2(ops):
    """stem.hip:310 caps the grid at 65536 workgroups; an item is four outputs of a row (WoG, stem.hip:308).  Planes of
    2 x 1 give one item each: 65536 * 256 + 3 planes, 128 MB in, 64 MB out.  Plane k holds (v, -v), v = k % 8191: max = v."""
    NC = _cap('dm_maxpool3x3_s2_fwd') * 256 + 3
    v = _ramp(NC)
    x = torch.stack([v, -v], 1).view(1, NC, 2, 1)
    out = ops.maxpool3x3_s2(x)
    assert torch.equal(out.view(-1), v)
    pl = _planes_around(65536 * 256, 1, NC)
    xs = x[0, pl].cpu()[None]
    _sample(out[0, pl][None], F.max_pool2d(xs, 3, 2, 1), F.max_pool2d(xs.double(), 3, 2, 1), 'maxpool3x3_s2')


def test_capped_subsample2(ops):
    """pointwise.hip:1332 caps at 16384 workgroups, one output per thread.  Planes of 2 x 1 holding (v, -v): out = v."""
    NC = _cap('dm_subsample2_fwd') * 256 + 3
    v = _ramp(NC)
    x = torch.stack([v, -v], 1).view(1, NC, 2, 1)
    out = ops.subsample2(x)
    assert torch.equal(out.view(-1), v)
    pl = _planes_around(16384 * 256, 1, NC)
    xs = x[0, pl].cpu()[None]
    _sample(out[0, pl][None], F.max_pool2d(xs, 1, stride=2), F.max_pool2d(xs.double(), 1, stride=2), 'subsample2')


def test_capped_avgpool2x2_ceil(ops):
    """pointwise.hip:1372 caps at 16384 workgroups, one output per thread.  Planes of 2 x 1 holding (v, v + 2): out = v + 1."""
    NC = _cap('dm_avgpool2x2_ceil_fwd') * 256 + 3
    v = _ramp(NC)
    x = torch.stack([v, v + 2], 1).view(1, NC, 2, 1)
    out = ops.avgpool2x2_ceil(x)
    assert torch.equal(out.view(-1), v + 1)
    pl = _planes_around(16384 * 256, 1, NC)
    xs = x[0, pl].cpu()[None]
    _sample(out[0, pl][None], F.avg_pool2d(xs, 2, 2, ceil_mode=True, count_include_pad=False),
            F.avg_pool2d(xs.double(), 2, 2, ceil_mode=True, count_include_pad=False), 'avgpool2x2_ceil')


def test_capped_threshold_ge(ops):
    """pointwise.hip:1236 caps at 16384 workgroups, one element per thread: 16384 * 256 + 3 elements (i % 7 - 3) / 4."""
    n = _cap('dm_threshold_ge') * 256 + 3
    r = torch.arange(n, device='cuda') % 7
    x = (r.float() - 3.0) * 0.25
    out = ops.threshold_ge(x, 0.25)
    assert torch.equal(out, (r >= 4).float())
    pl = _planes_around(16384 * 256, 1, n)
    xs = x[pl].cpu()
    _sample(out[pl], (xs >= 0.25).float(), (xs.double() >= 0.25).double(), 'threshold_ge')


def test_capped_resize_bilinear(ops):
    """pointwise.hip:999 caps at 65536 workgroups, one output per thread.  Planes of 1 x 2 holding (v, v + 2) resized to
    1 x 3 (align_corners): (v, v + 1, v + 2), every product exact.  ceil((65536 * 256 + 3) / 3) planes: 45 MB in, 67 MB out."""
    cap = _cap('dm_resize_bilinear_fwd')
    NC = -(-(cap * 256 + 3) // 3)
    v = _ramp(NC)
    x = torch.stack([v, v + 2], 1).view(1, NC, 1, 2)
    out = ops.resize_bilinear(x, (1, 3))
    assert torch.equal(out.view(NC, 3), torch.stack([v, v + 1, v + 2], 1))
    pl = _planes_around(cap * 256, 3, NC)
    xs = x[0, pl].cpu()[None]
    _sample(out[0, pl][None], F.interpolate(xs, size=(1, 3), mode='bilinear', align_corners=True),
            F.interpolate(xs.double(), size=(1, 3), mode='bilinear', align_corners=True), 'resize_bilinear')


def test_capped_upsample2x_generic(ops):
    """pointwise.hip:988 caps the generic build at 32768 workgroups; an item is four outputs of a row (OWq,
    pointwise.hip:340).  Planes of 1 x 1 give two items (the two output rows): 32768 * 128 + 3 planes of v -> 2 x 2 of v."""
    cap = _cap('dm_upsample2x_bilinear_fwd/generic')
    NC = cap * 256 // 2 + 3
    v = _ramp(NC)
    x = v.view(1, NC, 1, 1)
    pl = _planes_around(cap * 256, 2, NC)
    xs = x[0, pl].cpu()[None]
    for ac in (True, False):
        out = ops.upsample2x(x, align_corners=ac)
        assert torch.equal(out.view(NC, 4), v[:, None].expand(NC, 4)), ac
        _sample(out[0, pl][None], F.interpolate(xs, scale_factor=2, mode='bilinear', align_corners=ac),
                F.interpolate(xs.double(), scale_factor=2, mode='bilinear', align_corners=ac), f'upsample2x ac={ac}')


def test_capped_upsample2x_half_pixel(ops):
    """pointwise.hip:983 caps the half-pixel build (W even, H, W >= 2) at 65536 workgroups; an item is two input pixels
    (eight outputs).  Planes of 2 x 2 give two items: 65536 * 128 + 3 planes, 134 MB in, 537 MB out.  Plane k holds
    v + (0, 4; 8, 12): the weights are 0, 1/4, 3/4, 1, so every output is v plus a pattern that is exact in fp32."""
    cap = _cap('dm_upsample2x_bilinear_fwd/half')
    NC = cap * 256 // 2 + 3
    v = _ramp(NC)
    plane = torch.tensor([0.0, 4.0, 8.0, 12.0], device='cuda')
    x = (v[:, None] + plane[None]).view(1, NC, 2, 2)
    out = ops.upsample2x(x, align_corners=False)
    pattern = F.interpolate(plane.cpu().double().view(1, 1, 2, 2), scale_factor=2, mode='bilinear', align_corners=False).view(16)
    assert torch.equal(pattern * 4, (pattern * 4).round())
    assert torch.equal(out.view(NC, 16) - v[:, None], pattern.float().cuda()[None].expand(NC, 16))
    pl = _planes_around(cap * 256, 2, NC)
    xs = x[0, pl].cpu()[None]
    _sample(out[0, pl][None], F.interpolate(xs, scale_factor=2, mode='bilinear', align_corners=False),
            F.interpolate(xs.double(), scale_factor=2, mode='bilinear', align_corners=False), 'upsample2x half-pixel')


def test_capped_sgd_momentum_step(ops):
    """api_misc.hip:53 caps at 4096 workgroups, one element per thread.  First step, lr 1/2, gradient 2, no decay:
    momentum = 2, parameter i % 8191 goes down by one."""
    n = _cap('dm_sgd_momentum_step') * 256 + 3
    p0 = _ramp(n)
    p, gr, m = p0.clone(), torch.full((n,), 2.0, device='cuda'), torch.full((n,), CANARY, device='cuda')
    ops.sgd_momentum_step_(p, gr, m, 0.5, momentum=0.9, weight_decay=0.0, grad_scale=1.0, first_step=True)
    assert torch.equal(p, p0 - 1) and bool((m == 2.0).all()) and bool((gr == 2.0).all())
    pl = _planes_around(4096 * 256, 1, n)
    _sample(p[pl], p0[pl].cpu() - 0.5 * 2.0, p0[pl].cpu().double() - 0.5 * 2.0, 'sgd step')


def test_capped_sumsq(ops):
    """bbox_train.hip:496 caps at 1024 workgroups of 16384 elements; past that a workgroup's slice grows (bbox_train.hip:216).
    1024 * 16384 + 3 elements i % 3 - 1: every partial sum is an integer below 2^24, so the total is exact whatever the
    order -- the number of elements that are not zero."""
    n = _cap('dm_sumsq') * 16384 + 3
    r = torch.arange(n, device='cuda') % 3
    x = r.float() - 1.0
    want = n - (n + 1) // 3                                   # i % 3 == 1 holds for ceil((n - 1) / 3) of the i below n
    assert int((r != 1).sum()) == want < 1 << 24
    out = ops.sumsq(x)
    assert float(out[0]) == float(want)
    assert float(x.double().pow(2).sum()) == float(want)


def test_capped_merge_aug_masks(ops):
    """rle.hip:409 caps at 8192 workgroups, one cell per thread: 33 masks of 256 x 256 are 8192 * 256 + 65536 cells.  Two
    views, the second flipped horizontally: (sigmoid(a) + flip(sigmoid(b))) / 2 in the kernel's operations, the library's
    own logistic included, so every cell is held bit for bit; masks 0, 31, 32 (cell 8192 * 256 opens mask 32) to float64."""
    cap = _cap('dm_merge_aug_masks')
    n, S = 33, 256
    assert n * S * S > cap * 256 >= (n - 1) * S * S
    g = _g(20000)
    a, b = (torch.randn(n, 1, S, S, generator=g) * 4).cuda(), (torch.randn(n, 1, S, S, generator=g) * 4).cuda()
    metas = [dict(img_shape=(S, S, 3), scale_factor=1.0, flip=d is not None, flip_direction=d) for d in (None, 'horizontal')]
    got = ops.merge_aug_masks([a, b], None, ops.aug_view_table(metas, a.device))
    assert torch.equal(got, (ops.sigmoid(a) + torch.flip(ops.sigmoid(b), [3])) / 2)
    pl = [0, 31, 32]
    ref = [(torch.sigmoid(a[pl].cpu().to(dt)) + torch.flip(torch.sigmoid(b[pl].cpu().to(dt)), [3])) / 2 for dt in (torch.float32, torch.float64)]
    assert_close_via_f64(got[pl], ref[0], ref[1], 'merge_aug_masks past the cap')


def _relu_bwd_case(ops, n):
    r = torch.arange(n, device='cuda')
    grad0, out = (r % 8191).float() + 1.0, (r % 3).float() - 1.0
    grad = grad0.clone()
    ops.relu_backward_(grad, out)
    assert torch.equal(grad, torch.where(r % 3 == 2, grad0, torch.zeros_like(grad0)))
    pl = _planes_around(16384 * 256 * (4 if n % 4 == 0 else 1), 1, n)
    g0, o = grad0[pl].cpu(), out[pl].cpu()
    _sample(grad[pl], torch.where(o <= 0, torch.zeros_like(g0), g0), torch.where(o <= 0, torch.zeros_like(g0), g0).double(), 'relu_bwd')


def test_capped_relu_bwd(ops):
    """backward.hip:1866 grid_for caps at 16384 workgroups.  dm_relu_bwd (:1874, :1878) has a float4 build for aligned
    buffers of a multiple of four elements and a scalar one: 4 * (16384 * 256 + 3) elements, and 16384 * 256 + 3."""
    cap = _cap('grid_for')
    _relu_bwd_case(ops, 4 * (cap * 256 + 3))
    _relu_bwd_case(ops, cap * 256 + 3)


def test_capped_sigmoid_bwd(ops):
    """dm_sigmoid_bwd (backward.hip:1886, grid_for): one element per thread.  16384 * 64 + 1 maps of 2 x 2; sig alternates
    1/2 and 1/4, ga = i % 8191, gb = 1: (ga + gb) * s * (1 - s) is exact, the same expression on the device."""
    cap = _cap('grid_for')
    N = cap * 256 // 4 + 1
    r = torch.arange(N * 4, device='cuda')
    sig = torch.where(r % 2 == 0, 0.5, 0.25).view(N, 1, 2, 2)
    ga, gb = (r % 8191).float().view(N, 1, 2, 2), torch.ones(N, 1, 2, 2, device='cuda')
    got = ops.sigmoid_backward(sig, ga, gb)
    assert torch.equal(got, (ga + gb) * sig * (1 - sig))
    pl = _planes_around(cap * 256, 4, N)
    s, a = sig[pl].cpu(), ga[pl].cpu()
    _sample(got[pl], (a + 1) * s * (1 - s), (a.double() + 1) * s.double() * (1 - s.double()), 'sigmoid_bwd')


def _up_bwd_f64(go, shape, ac, dt):
    x = torch.zeros(shape, dtype=dt, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=ac).backward(go.to(dt))
    return x.grad


def test_capped_upsample2x_bwd_plane_loops(ops):
    """backward.hip:2203 gives the LDS builds of the adjoint min(planes, 8 x compute units) workgroups, each walking planes
    blockIdx.x, + gridDim.x, ...: 8 x CUs + 3 planes of 2 x 2 send three workgroups round again, half-pixel (BK_UP_LDS) and
    align_corners (BK_UP_AC_LDS, its 256-thread build).  The gradient of plane k is v = k % 8191 + 1 everywhere, so every
    input pixel receives 4 v: exactly with the half-pixel weights (1, 3/4, 1/4); with align_corners the weights are thirds,
    each off by at most 2^-22, sixteen of them per pixel and as many roundings: within 1e-5 of 4 v."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    NC = _cap('dm_upsample2x_bilinear_bwd/lds') * cus + 3
    v = _ramp(NC) + 1.0
    go = v[:, None].expand(NC, 16).contiguous().view(1, NC, 4, 4)
    pl = sorted({0, 8 * cus - 1, 8 * cus, NC - 1})
    for ac in (False, True):
        gin = ops.upsample2x_backward(go, None, (1, NC, 2, 2), align_corners=ac)
        want = (4 * v)[:, None].expand(NC, 4)
        if ac:
            assert torch.allclose(gin.view(NC, 4), want, rtol=1e-5, atol=0), ac
        else:
            assert torch.equal(gin.view(NC, 4), want)
        gs = go[0, pl].cpu()[None]
        assert_close_via_f64(gin[0, pl][None], _up_bwd_f64(gs, (1, len(pl), 2, 2), ac, torch.float32),
                             _up_bwd_f64(gs, (1, len(pl), 2, 2), ac, torch.float64), f'upsample2x_bwd planes ac={ac}')


def test_capped_upsample2x_bwd_gather_and_scatter(ops):
    """The routes on grid_for (backward.hip:2209, :2217; 16384 workgroups, one item per thread).  Gather: half-pixel planes
    past the 64 KB LDS plane, 2 x 2050, one item per input pixel: 1024 planes are 16384 * 256 + 4096 items; the gradient of
    plane k is v everywhere, every input pixel receives exactly 4 v.  Scatter: planes of 1 x 1, one item per OUTPUT pixel:
    16384 * 64 + 1 planes; the four gradients v, 1, 2, 3 of a plane add to v + 6 in any order."""
    cap = _cap('grid_for')
    NC, H, W = 1024, 2, 2050
    assert NC * H * W > cap * 256 and 16 * H * W > 64 * 1024
    v = _ramp(NC) + 1.0
    go = v[:, None].expand(NC, 4 * H * W).contiguous().view(1, NC, 2 * H, 2 * W)
    gin = ops.upsample2x_backward(go, None, (1, NC, H, W), align_corners=False)
    assert torch.equal(gin.view(NC, H * W), (4 * v)[:, None].expand(NC, H * W))
    pl = _planes_around(cap * 256, H * W, NC)
    go_s = torch.randn(1, len(pl), 2 * H, 2 * W, generator=_g(21000))
    go2 = go.clone()
    go2[0, pl] = go_s[0].cuda()
    gin2 = ops.upsample2x_backward(go2, None, (1, NC, H, W), align_corners=False)
    assert_close_via_f64(gin2[0, pl][None], _up_bwd_f64(go_s, (1, len(pl), H, W), False, torch.float32),
                         _up_bwd_f64(go_s, (1, len(pl), H, W), False, torch.float64), 'upsample2x_bwd gather')
    NC = cap * 256 // 4 + 1
    v = _ramp(NC)
    go = torch.stack([v, torch.ones_like(v), torch.full_like(v, 2.0), torch.full_like(v, 3.0)], 1).view(1, NC, 2, 2)
    pl = _planes_around(cap * 256, 4, NC)
    for ac in (False, True):
        gin = ops.upsample2x_backward(go, None, (1, NC, 1, 1), align_corners=ac)
        assert torch.equal(gin.view(-1), v + 6), ac
        gs = go[0, pl].cpu()[None]
        _sample(gin[0, pl][None], _up_bwd_f64(gs, (1, len(pl), 1, 1), ac, torch.float32),
                _up_bwd_f64(gs, (1, len(pl), 1, 1), ac, torch.float64), f'upsample2x_bwd scatter ac={ac}')


# ------------------------------------------------------------------------------------------------ the split-K finishes
def test_capped_conv_split_k_finish(ops, L):
    """conv_igemm.hip:1274 caps the finish of a split launch at 4096 workgroups of 256 float4.  100 RoIs of 14 x 14 at
    256 -> 256 channels split in two (the plan says so) and have 5 017 600 outputs, 4900 workgroups' worth: the RoIs from
    83 on lie past the cap.  RoIs 0, 83, 84, 99 to float64; every output within 1e-5 of the scale of the unsplit launch
    (another association of the same products: the relation tests/test_ops_gpu.py holds the split to)."""
    NB, C, H, W, cout = sc.SPLITK_FINISH_CASE
    cap = _cap('dm_conv2d_fwd_ws/reduce')
    nws = int(L.dm_conv2d_splitk_floats(NB, H, W, cout, 3))
    rec, = ops.conv2d_plan([C], NB, H, W, cout, 3, relu=True, workspace_floats=nws)
    assert rec['ksplit'] >= 2 and NB * cout * H * W // 4 > cap * 256
    x, w, b = _conv_case(NB, C, H, W, cout, 22000)
    xd, wq, bd = x.cuda(), ops.pack_conv_weight(w.cuda()), b.cuda()
    plain = ops.conv2d(xd, wq, bd, cout, 3, relu=True)
    out = Guarded((NB, cout, H, W))
    with ops.splitk_scope():
        assert ops.CONV_SPLITK[0]
        ops.conv2d(xd, wq, bd, cout, 3, relu=True, out=out.t)
    out.check('split-K conv')
    assert not torch.equal(out.t, plain), 'the call did not split: the test exercises nothing'
    assert float((out.t - plain).abs().max()) <= 1e-5 * max(float(plain.abs().max()), 1.0)
    first_past = cap * 256 * 4 // (cout * H * W)
    rows = [0, first_past, first_past + 1, NB - 1]
    r32 = F.relu(F.conv2d(x[rows], w, b, padding=1))
    r64 = F.relu(F.conv2d(x[rows].double(), w.double(), b.double(), padding=1))
    assert_close_via_f64(out.t[rows], r32, r64, 'split-K conv past the cap')


def test_capped_dcn_split_k_finish(ops, L):
    """deform_conv.hip:1428, the same cap behind dm_deform_conv_fwd_ws: the same shape splits in three (:1262-1267)."""
    from oracle import ref_ops
    NB, C, H, W, cout = sc.SPLITK_FINISH_CASE
    cap = _cap('dm_deform_conv_fwd_ws/reduce')
    ws = int(L.dm_deform_conv_splitk_floats(NB, C, H, W, cout))
    recs = ops.deform_conv_plan(NB, C, H, W, cout, 2, relu=True, workspace_floats=ws)
    assert recs[0]['reduce'] == 1 and recs[0]['ksplit'] >= 2 and NB * cout * H * W // 4 > cap * 256
    g = _g(23000)
    x = torch.randn(NB, C, H, W, generator=g)
    off = torch.randn(NB, 36, H, W, generator=g) * 1.5
    w = torch.randn(cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
    xd, offd, wq = x.cuda(), off.cuda(), ops.pack_conv_weight(w.cuda())
    plain = ops.deform_conv(xd, offd, wq, cout, 2, relu=True)
    with ops.splitk_scope():
        out = ops.deform_conv(xd, offd, wq, cout, 2, relu=True)
    assert not torch.equal(out, plain), 'the call did not split: the test exercises nothing'
    assert float((out - plain).abs().max()) <= 1e-5 * max(float(plain.abs().max()), 1.0)
    first_past = cap * 256 * 4 // (cout * H * W)
    rows = [0, first_past, first_past + 1, NB - 1]
    r32 = F.relu(ref_ops.deform_conv2d(x[rows], off[rows], w, 1, 1, 1, 2))
    r64 = F.relu(ref_ops.deform_conv2d(x[rows].double(), off[rows].double(), w.double(), 1, 1, 1, 2))
    assert_close_via_f64(out[rows], r32, r64, 'split-K DCN past the cap')
