"""PointRefine inference on the MI355X: the K24 kernels of csrc/point_refine.hip (descending point selection, point-feature
gather, point MLP + scatter, multi-row scatter) against float64 restatements, PointRefineRoIHead against the reference
(tests/golden/g20_pointrefine.npz), and the RoI head through the registry, batched and under test-time augmentation.

Kernel outputs are written into buffers followed by a canary that must survive; the cells the selection leaves out keep
their input values bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

CANARY = 7.0
NC = 160


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _with_canary(shape, fill=None):
    n = int(np.prod(shape))
    buf = torch.full((n + 4096,), CANARY, device='cuda')
    view = buf[:n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _check_canary(buf, shape, what):
    n = int(np.prod(shape))
    assert bool((buf[n:] == CANARY).all()), f'{what}: the canary past the output was overwritten'


# ------------------------------------------------------------------ selection
def _topk_ref(key, P):
    """Indices (ascending) of the P largest keys per row, the lower index first among equal keys (float64 host)."""
    out = []
    for row in key:
        order = np.lexsort((np.arange(row.size), -row))      # key descending, then index ascending
        out.append(np.sort(order[:P]))
    return np.stack(out).astype(np.int32)


@pytest.mark.parametrize('n', (1, 3, 7))
@pytest.mark.parametrize('S,P', ((56, 784), (28, 300), (14, 195), (112, 784)))
def test_topk_select_raw(n, S, P):
    """mode 0 (mask_use_sigmoid=False): the keys are the values; exact."""
    from dynamask_amd import ops
    x = torch.randn(n, 1, S, S, generator=_g(S + n))
    x[:, :, :3, :5] = 0.75                                  # ties, some at the cut for small P
    got = ops.point_topk_select(x.cuda(), P, use_sigmoid=False).cpu().numpy()
    np.testing.assert_array_equal(got, _topk_ref(x.view(n, -1).double().numpy(), P))


@pytest.mark.parametrize('n', (1, 5))
def test_topk_select_sigmoid_and_saturated_ties(n):
    """mode 1: the key is the library's sigmoid.  Saturated logits (> 17) all give 1.0f: more saturated cells than P,
    so the P lowest indices among them are taken."""
    from dynamask_amd import ops
    S, P = 56, 784
    x = torch.randn(n, 1, S, S, generator=_g(9)) * 3
    sat = torch.rand(n, 1, S, S, generator=_g(10)) < 0.4        # ~1250 saturated cells per RoI
    x[sat] = 20.0 + torch.rand(int(sat.sum()), generator=_g(11)) * 30
    xc = x.cuda()
    got = ops.point_topk_select(xc, P, use_sigmoid=True).cpu().numpy()
    key = ops.sigmoid(xc).view(n, -1).double().cpu().numpy()        # the same expression on the device
    assert (key == 1.0).sum(1).min() > P
    np.testing.assert_array_equal(got, _topk_ref(key, P))
    for r in range(n):
        np.testing.assert_array_equal(got[r], np.flatnonzero(key[r] == 1.0)[:P])


def test_topk_select_support():
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_point_topk_select_supported(3, 3136, 784, 1) == 1
    assert L.dm_point_topk_select_supported(3, 3136, 784, 0) == 1
    assert L.dm_point_topk_select_supported(3, 3136, 784, 2) == 0
    assert L.dm_point_topk_select_supported(3, 3136, 3137, 1) == 0
    assert L.dm_point_topk_select_supported(3, 3136, 0, 1) == 0
    assert L.dm_point_topk_select_supported(0, 3136, 784, 1) == 1


# ------------------------------------------------------------------ gather
def _rois(n, B, seed):
    g = _g(seed)
    xy = torch.rand(n, 2, generator=g) * 220 - 20
    wh = torch.rand(n, 2, generator=g) * 120 + 1
    b = torch.randint(0, B, (n, 1), generator=g).float()
    return torch.cat([b, xy, xy + wh], 1)


@pytest.mark.parametrize('C,S,P', ((256, 14, 196), (128, 28, 784), (64, 56, 784), (64, 56, 3136)))
@pytest.mark.parametrize('n', (1, 5))
def test_feat_gather(C, S, P, n):
    """Fine channels: within rounding of dm_point_gather_fwd's (the same expressions; the compiler may contract
    another pair of them into an fma) and of a float64 grid_sample; coarse channels: exactly torch.gather of the logit
    maps."""
    from dynamask_amd import ops
    B = 2
    g = _g(C + S + n)
    sem = torch.randn(B, C, 48, 64, generator=g).cuda()
    coarse = torch.randn(n, NC, S, S, generator=g).cuda()
    rois = _rois(n, B, S).cuda()
    if P == S * S:
        idx = None
        idx_full = torch.arange(P, dtype=torch.int32).repeat(n, 1).cuda()
    else:
        idx = torch.stack([torch.randperm(S * S, generator=g)[:P].sort().values for _ in range(n)]).int().cuda()
        idx_full = idx
    shape = (n, C + NC, P)
    buf, out = _with_canary(shape)
    ops.point_feat_gather(sem, rois, coarse, idx, 0.25, out=out)
    _check_canary(buf, shape, 'point_feat_gather')
    ref_fine = ops.point_gather(sem, rois, coarse[:, :8].contiguous(), idx_full, S, S, 0.25)[:, :C]
    assert_grad_close(out[:, :C], ref_fine, 'fine channels against dm_point_gather_fwd', rel=1e-4)
    ref_coarse = torch.gather(coarse.view(n, NC, -1), 2, idx_full.long()[:, None].expand(-1, NC, -1))
    assert torch.equal(out[:, C:], ref_coarse)
    # float64: the cell centres through rel_roi_point_to_rel_img_point, grid_sample(zeros, align_corners=False)
    cell = idx_full.long().cpu()
    px = ((cell % S).double() + 0.5) / S
    py = ((cell // S).double() + 0.5) / S
    r = rois.cpu().double()
    ax = px * (r[:, 3:4] - r[:, 1:2]) + r[:, 1:2]
    ay = py * (r[:, 4:5] - r[:, 2:3]) + r[:, 2:3]
    gx, gy = ax / 64 * 0.25 * 2 - 1, ay / 48 * 0.25 * 2 - 1
    sem64 = sem.cpu().double()
    for i in range(n):
        b = int(r[i, 0])
        grid = torch.stack([gx[i], gy[i]], -1).view(1, 1, P, 2)
        ref = F.grid_sample(sem64[b:b + 1], grid, align_corners=False).view(C, P)
        np.testing.assert_allclose(out[i, :C].cpu().double().numpy(), ref.numpy(), atol=1e-4, rtol=1e-4)


def test_feat_gather_support():
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_point_feat_gather_supported(2, 64, 48, 64, 5, 160, 784, 56, 1) == 1
    assert L.dm_point_feat_gather_supported(2, 64, 48, 64, 5, 160, 784, 56, 0) == 0      # no index: every cell
    assert L.dm_point_feat_gather_supported(2, 64, 48, 64, 5, 160, 3136, 56, 0) == 1
    assert L.dm_point_feat_gather_supported(2, 60, 48, 64, 5, 160, 784, 56, 1) == 0
    assert L.dm_point_feat_gather_supported(2, 64, 48, 64, 5, 150, 784, 56, 1) == 0
    assert L.dm_point_feat_gather_supported(0, 64, 48, 64, 5, 160, 784, 56, 1) == 0


# ------------------------------------------------------------------ point MLP + scatter
def _mlp_case(n, C, S, P, nfc, seed):
    g = _g(seed)
    x = torch.randn(n, C + NC, P, generator=g)
    ws = [torch.randn(C, C + NC, generator=g) * (2.0 / (C + NC)) ** 0.5 for _ in range(nfc + 1)]
    bs = [torch.randn(C, generator=g) * 0.1 for _ in range(nfc + 1)]
    feat = torch.randn(n, C, S, S, generator=g)
    if P == S * S:
        idx = None
    else:
        idx = torch.stack([torch.randperm(S * S, generator=g)[:P].sort().values for _ in range(n)]).int()
    return x, ws, bs, feat, idx


def _mlp_ref(x, ws, bs, feat, idx, dt):
    n, CT, P = x.shape
    C = ws[0].shape[0]
    x, feat = x.to(dt), feat.to(dt).clone()
    coarse, h = x[:, C:], x[:, :C]
    for L in range(len(ws)):
        y = torch.einsum('ok,nkp->nop', ws[L].to(dt), torch.cat([h, coarse], 1)) + bs[L].to(dt)[None, :, None]
        h = y.clamp_min(0) if L < len(ws) - 1 else y
    f = feat.view(n, C, -1)
    cell = torch.arange(P).repeat(n, 1) if idx is None else idx.long()
    f.scatter_(2, cell[:, None].expand(-1, C, -1), h)
    return feat


def _run_mlp(x, ws, bs, feat, idx, form):
    from dynamask_amd import ops
    n, C = feat.shape[:2]
    shape = tuple(feat.shape)
    buf, f = _with_canary(shape, feat.cuda())
    wq = [ops.pack_conv_weight(w.cuda().view(C, -1, 1, 1).contiguous()) for w in ws]
    ops.point_refine_mlp(x.cuda(), C, wq, [b.cuda() for b in bs], None if idx is None else idx.cuda(), f, form=form)
    _check_canary(buf, shape, f'point_refine_mlp ({form})')
    return f.cpu()


@pytest.mark.parametrize('form', ('fused', 'unfused'))
@pytest.mark.parametrize('nfc', (1, 2))
@pytest.mark.parametrize('n,C,S,P', ((3, 256, 14, 196), (1, 256, 14, 100), (5, 128, 28, 784), (3, 128, 28, 333),
                                     (3, 64, 56, 784), (1, 64, 56, 3136)))
def test_point_refine_mlp(n, C, S, P, nfc, form):
    """Every C row of fc_logits at the selected cells, against float64; the other cells keep their input bits."""
    x, ws, bs, feat, idx = _mlp_case(n, C, S, P, nfc, n * 1000 + C + P + nfc)
    got = _run_mlp(x, ws, bs, feat, idx, form)
    assert_close_via_f64(got, _mlp_ref(x, ws, bs, feat, idx, torch.float32), _mlp_ref(x, ws, bs, feat, idx, torch.float64),
                         f'point MLP {form} n={n} C={C} P={P}', rel=1e-4)
    if idx is not None:
        keep = torch.ones(n, S * S, dtype=torch.bool)
        keep.scatter_(1, idx.long(), False)
        fv, gv = feat.view(n, C, -1), got.view(n, C, -1)
        assert torch.equal(gv.permute(0, 2, 1)[keep], fv.permute(0, 2, 1)[keep])


@pytest.mark.parametrize('C', (64, 128, 256))
def test_fused_unfused_dense_agree(C):
    """P == S^2: the fused kernel without an index, the unfused sequence with the identity index (conv + scatter) and
    the dense form (the unfused sequence without an index: fc_logits writes the features) agree within rounding."""
    S = {64: 56, 128: 28, 256: 14}[C]
    n, P = 4, S * S
    x, ws, bs, feat, _ = _mlp_case(n, C, S, P, 2, C)
    ident = torch.arange(P, dtype=torch.int32).repeat(n, 1)
    fused = _run_mlp(x, ws, bs, feat, None, 'fused')
    unfused = _run_mlp(x, ws, bs, feat, ident, 'unfused')
    dense = _run_mlp(x, ws, bs, feat, None, 'unfused')
    fused_idx = _run_mlp(x, ws, bs, feat, ident, 'fused')
    assert torch.equal(fused, fused_idx)
    assert torch.equal(unfused, dense)
    assert_grad_close(fused, dense, f'fused vs dense C={C}', rel=1e-4)


def test_scatter_rows():
    from dynamask_amd import ops
    n, C, S, P = 3, 64, 56, 500
    g = _g(4)
    vals = torch.randn(n, C, P, generator=g)
    idx = torch.stack([torch.randperm(S * S, generator=g)[:P] for _ in range(n)]).int()
    feat = torch.randn(n, C, S, S, generator=g)
    shape = (n, C, S, S)
    buf, f = _with_canary(shape, feat.cuda())
    ops.point_scatter_rows(vals.cuda(), idx.cuda(), f)
    _check_canary(buf, shape, 'point_scatter_rows')
    ref = feat.clone().view(n, C, -1)
    ref.scatter_(2, idx.long()[:, None].expand(-1, C, -1), vals)
    assert torch.equal(f.cpu(), ref.view(shape))


def test_point_refine_mlp_refusals():
    from dynamask_amd._lib import lib
    L = lib()
    sup = L.dm_point_refine_mlp_supported
    assert sup(100, 784, 64, 160, 2, 3136, 1) == 1
    assert sup(100, 3136, 64, 160, 2, 3136, 0) == 1
    assert sup(100, 784, 64, 160, 2, 3136, 0) == 0          # no index: P must be every cell
    assert sup(100, 784, 96, 160, 2, 3136, 1) == 0          # C outside {64, 128, 256}
    assert sup(100, 784, 32, 160, 2, 3136, 1) == 0
    assert sup(100, 784, 64, 168, 2, 3136, 1) == 0          # NC above 160
    assert sup(100, 784, 64, 160, 0, 3136, 1) == 0
    assert sup(100, 784, 64, 160, 5, 3136, 1) == 0
    assert sup(100, 3137, 64, 160, 2, 3136, 1) == 0
    x = torch.zeros(2, 224, 64, device='cuda')
    w = torch.zeros(4096 * 224, device='cuda')
    feat = torch.zeros(2, 64, 196, device='cuda')
    idx = torch.zeros(2, 64, dtype=torch.int32, device='cuda')
    vp = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    ws = (ctypes.c_void_p * 3)(w.data_ptr(), w.data_ptr(), w.data_ptr())
    call = lambda flags: L.dm_point_refine_mlp(vp(x), 2, 64, 64, 160, 2, ws, None, vp(idx), flags, vp(feat), 196, None)  # noqa: E731
    assert call(16) == -3                                   # bit 4: the bf16x3 mode is refused
    assert call(1) == -1
    assert L.dm_point_scatter_rows(vp(x), vp(idx), 2, 64, 197, vp(feat), 196, None) == -3
    torch.cuda.synchronize()


# ------------------------------------------------------------------ heads
def _configs(golden_dir):
    import json
    from dynamask_amd import registry
    with open(f'{golden_dir}/g20_pointrefine_configs.json') as f:
        return registry._to_cfgdict(json.load(f))['coco']


def _roi_head(golden_dir):
    """The config's PointRefineRoIHead through the registry, mask head with the fixture's seeded weights, on the GPU."""
    import pointrefine_inputs as pi
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _configs(golden_dir)
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=registry._to_cfgdict(dict(pi.TEST_CFG)))
    torch.manual_seed(0)
    m = registry.build_head(rh)
    sd = m.mask_head.state_dict()
    st = pi.head_state({'mask_head.' + k: v.shape for k, v in sd.items()})
    m.mask_head.load_state_dict({k[len('mask_head.'):]: v for k, v in st.items()}, strict=True)
    return m.cuda().eval()


def _feats():
    import pointrefine_inputs as pi
    return [f.cuda() for f in pi.fpn_feats()]


def _golden(golden_dir):
    return np.load(f'{golden_dir}/g20_pointrefine.npz')


def test_head_matches_the_reference(golden_dir):
    """The stage 1-3 label-row predictions against the reference's, and the stage-2 selection: the reference's set and
    ours differ only in cells whose key lies within rounding of our cut."""
    import pointrefine_inputs as pi
    from dynamask_amd import ops
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    det, lab = pi.detections()
    rois = torch.cat([torch.zeros(len(det), 1), det[:, :4]], 1).cuda()
    seen = []
    orig = ops.point_topk_select

    def spy(detail, num_points, **kw):
        out = orig(detail, num_points, **kw)
        seen.append((detail.clone(), out.clone()))
        return out
    ops.point_topk_select = spy
    try:
        with torch.no_grad():
            res = m._mask_forward(_feats(), rois, lab.cuda())
    finally:
        ops.point_topk_select = orig
    for i in (1, 2, 3):
        assert_grad_close(res['stage_instance_preds'][i], z[f'stage{i}'], f'stage {i} logits', rel=1e-3)
    assert len(seen) == 1                                   # stages 0 and 1 take every cell: no selection launch
    detail, idx = seen[0]
    key = ops.sigmoid(detail).view(len(det), -1).double().cpu().numpy()
    got, ref, gap = idx.cpu().numpy(), z['select2'], z['select2_gap']
    for r in range(len(det)):
        a, b = set(got[r].tolist()), set(ref[r].tolist())
        cut = np.sort(key[r])[::-1][got.shape[1] - 1]
        diff = sorted(a ^ b)
        assert all(abs(key[r][c] - cut) <= 1e-5 for c in diff), f'RoI {r}: cells far from the cut differ'
        if gap[r] > 1e-4:
            assert a == b


def _paste_check(merged, det, ref_bits, shape, got):
    from dynamask_amd import ops
    diff = got != ref_bits
    if diff.any():
        tol = 1e-3
        boxes = det[:, :4].contiguous()
        lo = ops.paste_masks(merged.cuda().contiguous(), boxes, shape[1], shape[2], 0.5 - tol, apply_sigmoid=True).cpu().numpy()
        hi = ops.paste_masks(merged.cuda().contiguous(), boxes, shape[1], shape[2], 0.5 + tol, apply_sigmoid=True).cpu().numpy()
        bad = diff & ~(lo.astype(bool) != hi.astype(bool))
        assert not bad.any(), f'{int(bad.sum())} bitmap pixels differ away from the threshold'


def _per_det(segm, labels):
    seen, out = {}, []
    for c in labels:
        j = seen.get(c, 0)
        seen[c] = j + 1
        out.append(np.asarray(segm[c][j]))
    return np.stack(out)


def test_simple_test_mask_matches_the_reference(golden_dir):
    """simple_test_mask: the merged 112 x 112 logits and the bitmaps (equal except at pixels whose pasted probability is
    within rounding of the threshold)."""
    import pointrefine_inputs as pi
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    det, lab = pi.detections()
    det, lab = det.cuda(), lab.cuda()
    x = _feats()
    with torch.no_grad():
        merged = m.simple_test_mask_logits(x, det, lab).cpu()
        segm = m.simple_test_mask(x, pi.img_metas(), det, lab)
    ref = torch.from_numpy(z['merged'])
    close = (merged - ref).abs() <= 1e-3 * (1 + ref.abs())
    assert float(close.float().mean()) > 0.995, f'merged logits: {float((~close).float().mean()):.4f} of the pixels differ'
    shape = tuple(z['bitmap_shape'])
    ref_bits = np.unpackbits(z['bitmaps'], axis=-1)[..., :shape[-1]].astype(bool)
    got = _per_det(segm, lab.tolist())
    assert got.shape == ref_bits.shape
    _paste_check(merged, det, ref_bits, shape, got)


def _proposals(n, seed):
    import pointrefine_inputs as pi
    g = _g(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([pi.IMG_W, pi.IMG_H]) * 0.8
    wh = torch.rand(n, 2, generator=g) * 120 + 8
    return torch.cat([xy, xy + wh, torch.rand(n, 1, generator=g)], 1).cuda()


@pytest.mark.parametrize('n_det', (0, 1, 100))
def test_simple_test_through_the_registry(golden_dir, n_det):
    """simple_test (bbox branch + masks) with 0, 1 and 100 detections: per-class bitmaps of the image's size."""
    import pointrefine_inputs as pi
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = max(n_det, 1)
    x = _feats()
    props = _proposals(400, 11)
    with torch.no_grad():
        if n_det == 0:
            det = props.new_zeros((0, 5))
            lab = torch.zeros((0,), dtype=torch.long, device='cuda')
            segm = m.simple_test_mask(x, pi.img_metas(), det, lab)
            assert len(segm) == 80 and all(s == [] for s in segm)
            assert tuple(m.simple_test_mask_logits(x, det, lab).shape) == (0, 1, 112, 112)
            return
        bbox_res, segm = m.simple_test(x, [props], pi.img_metas())
    n = sum(len(b) for b in bbox_res)
    assert n == n_det
    assert len(segm) == 80 and sum(len(s) for s in segm) == n
    for c in range(80):
        assert len(segm[c]) == len(bbox_res[c])
        for s in segm[c]:
            assert s.shape == (pi.IMG_H, pi.IMG_W) and s.dtype == np.bool_


def test_100_detections_fused_vs_unfused(golden_dir):
    """At 100 RoIs the fused point MLP and the unfused sequence give the same merged logits within rounding."""
    m = _roi_head(golden_dir)
    det = _proposals(100, 13)
    lab = torch.randint(0, 80, (100,), generator=_g(3)).cuda()
    rois = torch.cat([det.new_zeros((100, 1)), det[:, :4]], 1)
    x = _feats()
    with torch.no_grad():
        a = m.merge_stage_preds(m._mask_forward(x, rois, lab, form='fused')['stage_instance_preds']).cpu()
        b = m.merge_stage_preds(m._mask_forward(x, rois, lab, form='unfused')['stage_instance_preds']).cpu()
    assert torch.isfinite(a).all()
    close = (a - b).abs() <= 1e-3 * (1 + b.abs())
    assert float((~close).float().mean()) < 1e-3


def test_encode_equals_host_rle(golden_dir):
    """simple_test_mask(encode=True): the COCO RLE of simple_test_mask's bitmaps (the host encoder of oracle/ref_ops)."""
    import pointrefine_inputs as pi
    from oracle import ref_ops
    m = _roi_head(golden_dir)
    x = _feats()
    det, lab = pi.detections()
    det, lab = det.cuda(), lab.cuda()
    with torch.no_grad():
        bits = m.simple_test_mask(x, pi.img_metas(), det, lab)
        rles = m.simple_test_mask(x, pi.img_metas(), det, lab, encode=True)
    assert [len(c) for c in bits] == [len(c) for c in rles] and sum(len(c) for c in bits) == len(det)
    for cb, cr in zip(bits, rles):
        for b, r in zip(cb, cr):
            assert r == ref_ops.rle_encode(b.astype(np.uint8))


@pytest.mark.parametrize('B', (2, 3))
def test_batch_equals_simple_test(golden_dir, B):
    """batch_simple_test over B images equals per-image simple_test: each RoI's fine points come from its own image."""
    import pointrefine_inputs as pi
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 20
    g = _g(21 + B)
    xs = [[torch.randn(1, 256, pi.IMG_H // s, pi.IMG_W // s, generator=g).cuda() for s in pi.STRIDES] for _ in range(B)]
    props = [_proposals(200, 30 + b) for b in range(B)]
    metas = [pi.img_metas()[0] for _ in range(B)]
    with torch.no_grad():
        xb = [torch.cat([xs[b][l] for b in range(B)]) for l in range(4)]
        batch = m.batch_simple_test(xb, props, metas)
        for b in range(B):
            single = m.simple_test(xs[b], [props[b]], [metas[b]])
            for c in range(80):
                assert len(single[1][c]) == len(batch[b][1][c])
                for u, v in zip(single[1][c], batch[b][1][c]):
                    assert np.array_equal(u, v)


def test_one_view_aug_test_equals_simple_test(golden_dir):
    import pointrefine_inputs as pi
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 20
    x = _feats()
    props = _proposals(200, 40)
    meta = pi.img_metas()[0]
    with torch.no_grad():
        aug = m.aug_test([x], [props[:, :4]], [[meta]])
        single = m.simple_test(x, [props[:, :4]], [meta])
    assert sum(len(c) for c in single[1]) > 0
    for c in range(80):
        assert len(aug[1][c]) == len(single[1][c])
        for u, v in zip(aug[1][c], single[1][c]):
            assert np.array_equal(u, v)


def test_bf16x3_bitmaps_agree_with_fp32(golden_dir):
    """Under set_conv_precision('bf16x3') the instance 3x3s and the 1x1s on the existing kernels may run the split
    kernel (the new kernels stay exact fp32); the bitmaps agree with the exact ones except near the threshold."""
    import pointrefine_inputs as pi
    from dynamask_amd.precision import conv_precision
    m = _roi_head(golden_dir)
    det, lab = pi.detections()
    det, lab = det.cuda(), lab.cuda()
    x = _feats()
    with torch.no_grad():
        merged = m.simple_test_mask_logits(x, det, lab).cpu()
        exact = _per_det(m.simple_test_mask(x, pi.img_metas(), det, lab), lab.tolist())
        with conv_precision('bf16x3'):
            split = _per_det(m.simple_test_mask(x, pi.img_metas(), det, lab), lab.tolist())
    _paste_check(merged, det, exact, exact.shape, split)
