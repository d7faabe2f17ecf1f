"""PointRend inference on the MI355X: the subdivision kernels of csrc/point_refine.hip against float64 torch restatements
(point selection, point gather, the fused point MLP + scatter and its unfused A/B sequence), and PointRendRoIHead against
the reference (tests/golden/g18_pointrend.npz), through the registry, batched and under test-time augmentation.  Output
buffers are followed by a canary that must survive."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

CANARY = 7.0
ICANARY = -12345


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ restatements
def _select_ref(m, P):
    """topk(-|v|, P) per row with the documented tie rule (lower index first), indices ascending."""
    a = m.flatten(1).double().abs()
    order = torch.sort(a, dim=1, stable=True).indices[:, :P]
    return torch.sort(order, dim=1).values


def _centres(idx, mh, mw, dtype):
    """get_roi_rel_points_test's cell centres (fp32 chain when dtype is float32)."""
    w_step, h_step = 1.0 / mw, 1.0 / mh
    px = w_step / 2.0 + (idx % mw).to(dtype) * w_step
    py = h_step / 2.0 + (idx // mw).to(dtype) * h_step
    return torch.stack([px, py], -1)


def _point_sample(inp, pts):
    return F.grid_sample(inp, pts.unsqueeze(2) * 2.0 - 1.0, align_corners=False).squeeze(3)


def _gather_ref(feat, rois, coarse, idx, mh, mw, scale, dtype):
    """[n, C + NC, P] of point_rend_roi_head._get_fine_grained_point_feats + point_sample(coarse) in ``dtype``."""
    feat, rois, coarse = feat.to(dtype), rois.to(dtype), coarse.to(dtype)
    rel = _centres(idx.long(), mh, mw, dtype)
    H, W = feat.shape[2:]
    out = []
    for r in range(rois.shape[0]):
        b = int(rois[r, 0])
        ab = rel[r].clone()
        ab[:, 0] = ab[:, 0] * (rois[r, 3] - rois[r, 1]) + rois[r, 1]
        ab[:, 1] = ab[:, 1] * (rois[r, 4] - rois[r, 2]) + rois[r, 2]
        img = ab / torch.tensor([W, H], dtype=dtype) * scale
        fine = _point_sample(feat[b:b + 1], img[None])[0]
        crs = _point_sample(coarse[r:r + 1], rel[r][None])[0]
        out.append(torch.cat([fine, crs], 0))
    return torch.stack(out) if out else feat.new_zeros((0, feat.shape[1] + coarse.shape[1], idx.shape[1]))


def _mlp_ref(x, ws, bs, wl, bl, dtype):
    """MaskPointHead.forward (coarse_pred_each_layer) -> all-class logits [n, NCL, P] in ``dtype``."""
    x = x.to(dtype)
    crs = x[:, 256:]
    h = x
    for w, b in zip(ws, bs):
        h = torch.cat([torch.relu(torch.einsum('ok,nkp->nop', w.to(dtype), h) + b.to(dtype)[None, :, None]), crs], 1)
    return torch.einsum('ok,nkp->nop', wl.to(dtype), h) + bl.to(dtype)[None, :, None]


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize('S', (28, 56, 112, 224))
@pytest.mark.parametrize('n', (0, 1, 7))
def test_point_select(S, n):
    from dynamask_amd import ops
    P = min(784, S * S)
    m = torch.randn(n, 1, S, S, generator=_g(S + n)).cuda()
    buf = torch.full((n * P + 1024,), ICANARY, dtype=torch.int32, device='cuda')
    got = ops.point_select(m, P, out=buf[:n * P].view(n, P))
    assert bool((buf[n * P:] == ICANARY).all()), 'the canary past the indices was overwritten'
    assert torch.equal(got.cpu().long(), _select_ref(m.cpu(), P))


def test_point_select_all_cells_and_ties():
    """P >= H * W selects every cell; planted ties at the cut follow the documented rule (lower index), and +0 / -0
    count as equal."""
    from dynamask_amd import ops
    m = torch.randn(3, 1, 28, 28, generator=_g(1)).cuda()
    assert torch.equal(ops.point_select(m, 784).cpu(), torch.arange(784, dtype=torch.int32).expand(3, 784))
    for S in (56, 224):
        g = _g(S)
        q = torch.randint(-12, 13, (4, 1, S, S), generator=g).float() / 8   # 25 magnitudes: thousands of ties per cut
        q[0].view(-1)[::7] = -0.0
        q[1] = 0.5
        q[2].view(-1)[5000 % (S * S):] *= -1
        m = q.cuda()
        got = ops.point_select(m, 784).cpu().long()
        ref = _select_ref(q, 784)
        assert torch.equal(got, ref)
        a = q.reshape(4, -1).abs()
        cut = a.gather(1, ref).max(1).values
        n_eq = (a == cut[:, None]).sum(1)
        print(f'S={S}: cut magnitudes {cut.tolist()}, cells tied at the cut {n_eq.tolist()}')
        assert int(n_eq.min()) > 1
    assert torch.equal(ops.point_select(torch.full((1, 1, 56, 56), 0.5).cuda(), 784).cpu(),
                       torch.arange(784, dtype=torch.int32)[None])


def test_point_select_support():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    assert ops.point_select_supported(224 * 224, 784) and ops.point_select_supported(784, 784)
    assert not ops.point_select_supported(100, 101) and not ops.point_select_supported(100, 0)
    assert lib().dm_point_select(None, 1, 100, 101, None, None) == -3


# ------------------------------------------------------------------------------------------------ gather
def _gather_case(n, S, seed):
    g = _g(seed)
    feat = torch.randn(2, 256, 48, 64, generator=g)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([300.0, 220.0]) - 20   # boxes partly outside the 256 x 192 image
    wh = torch.rand(n, 2, generator=g) * 120
    wh[0::3, 0] = 0.0                                                          # zero-width boxes
    wh[1::4, 1] = 0.0                                                          # zero-height boxes
    rois = torch.cat([(torch.arange(n) % 2).float()[:, None], xy, xy + wh], 1)
    coarse = torch.randn(n, 80, 7, 7, generator=g)
    P = min(784, S * S)
    idx = torch.stack([torch.sort(torch.randperm(S * S, generator=g)[:P]).values for _ in range(n)]).int() if n else \
        torch.zeros((0, P), dtype=torch.int32)
    return feat, rois, coarse, idx, P


@pytest.mark.parametrize('S', (28, 56, 224))
def test_point_gather(S):
    from dynamask_amd import ops
    n = 9
    feat, rois, coarse, idx, P = _gather_case(n, S, 40 + S)
    tot = n * 336 * P
    buf = torch.full((tot + 4096,), CANARY, device='cuda')
    got = ops.point_gather(feat.cuda(), rois.cuda(), coarse.cuda(), idx.cuda(), S, S, 0.25,
                           out=buf[:tot].view(n, 336, P)).cpu()
    assert bool((buf[tot:] == CANARY).all()), 'the canary past the point features was overwritten'
    r32 = _gather_ref(feat, rois, coarse, idx, S, S, 0.25, torch.float32)
    r64 = _gather_ref(feat, rois, coarse, idx, S, S, 0.25, torch.float64)
    assert_close_via_f64(got[:, :256], r32[:, :256], r64[:, :256], f'fine point features S={S}', rel=1e-5)
    assert_close_via_f64(got[:, 256:], r32[:, 256:], r64[:, 256:], f'coarse point features S={S}', rel=1e-5)
    # a RoI of no image of the batch: zero fine channels
    bad = rois.clone()
    bad[0, 0] = 5
    got = ops.point_gather(feat.cuda(), bad.cuda(), coarse.cuda(), idx.cuda(), S, S, 0.25).cpu()
    assert bool((got[0, :256] == 0).all())


def test_point_gather_matches_point_sample_at_28():
    """At the 28^2 step every cell is selected: the fine channels are SimpleRoIAlign(28)'s samples (dm_point_sample_fwd,
    whose affine_grid coordinate chain may differ in the last bits) -- a cross-check to a few ulps, not bit equality."""
    from dynamask_amd import ops
    n = 9
    feat, rois, coarse, _, _ = _gather_case(n, 28, 7)
    idx = torch.arange(784, dtype=torch.int32).expand(n, 784).contiguous()
    got = ops.point_gather(feat.cuda(), rois.cuda(), coarse.cuda(), idx.cuda(), 28, 28, 0.25)[:, :256]
    ref = ops.point_sample(feat.cuda(), rois.cuda(), 28, 0.25).view(n, 256, 784)
    # the two coordinate chains land within a few ulps of the map coordinate (ulp(64) = 2^-17 here), so the samples
    # agree within that many ulps times the map's steepest step between neighbouring cells
    step = max(float((feat[..., 1:] - feat[..., :-1]).abs().max()), float((feat[..., 1:, :] - feat[..., :-1, :]).abs().max()))
    err = float((got - ref).abs().max())
    allowed = 4 * 2.0 ** -23 * 64 * step
    print(f'gather vs dm_point_sample_fwd at 28^2: max |diff| {err:.3g}, allowed {allowed:.3g} (4 coordinate ulps)')
    assert err <= allowed


# ------------------------------------------------------------------------------------------------ point MLP
def _mlp_case(n, P, HW, seed, ncl=80):
    g = _g(seed)
    x = torch.randn(n, 336, P, generator=g)
    ws = [torch.randn(256, 336, generator=g) * (2.0 / 336) ** 0.5 for _ in range(3)]
    bs = [torch.randn(256, generator=g) * 0.1 for _ in range(3)]
    wl = torch.randn(ncl, 336, generator=g) * 0.05
    bl = torch.randn(ncl, generator=g) * 0.1
    labels = torch.randint(0, ncl, (n,), generator=g)
    idx = torch.stack([torch.sort(torch.randperm(HW, generator=g)[:P]).values for _ in range(n)]).int() if n else \
        torch.zeros((0, P), dtype=torch.int32)
    refined = torch.randn(n, 1, HW, generator=g)
    return x, ws, bs, wl, bl, labels, idx, refined


@pytest.mark.parametrize('n,P,HW', ((0, 784, 3136), (1, 784, 784), (5, 784, 50176), (3, 100, 3136), (2, 64, 64)))
def test_point_mlp_fused_and_unfused(n, P, HW):
    from dynamask_amd import ops
    x, ws, bs, wl, bl, labels, idx, refined = _mlp_case(n, P, HW, 100 + n + P)
    wq = [ops.pack_conv_weight(w[:, :, None, None].contiguous().cuda()) for w in ws]
    r32 = refined.clone()
    r64 = refined.double().clone()
    if n:
        ar = torch.arange(n)
        r32.view(n, HW).scatter_(1, idx.long(), _mlp_ref(x, ws, bs, wl, bl, torch.float32)[ar, labels])
        r64.view(n, HW).scatter_(1, idx.long(), _mlp_ref(x, ws, bs, wl, bl, torch.float64)[ar, labels])
    outs = {}
    for fused in (True, False):
        tot = n * HW
        buf = torch.full((tot + 4096,), CANARY, device='cuda')
        out = buf[:tot].view(n, 1, HW)
        out.copy_(refined.cuda())
        ops.point_mlp_scatter(x.cuda(), wq, [b.cuda() for b in bs], wl.cuda(), bl.cuda(), labels.cuda(), idx.cuda(), out,
                              fused=fused)
        assert bool((buf[tot:] == CANARY).all()), f'fused={fused}: the canary past the refined map was overwritten'
        got = out.cpu()
        outs[fused] = got
        if n:
            keep = torch.ones(n, HW, dtype=torch.bool)
            keep.scatter_(1, idx.long(), False)
            assert torch.equal(got.view(n, HW)[keep], refined.view(n, HW)[keep]), 'cells that were not selected changed'
            assert_close_via_f64(got, r32, r64, f'point MLP fused={fused} n={n} P={P}', rel=1e-5)
    if n:
        np.testing.assert_allclose(outs[True].numpy(), outs[False].numpy(), rtol=1e-5, atol=1e-5)


def test_point_mlp_refusals():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    x = torch.zeros(1, 336, 16, device='cuda')
    assert ops.point_mlp_supported(x, 3, 80, 784)
    assert not ops.point_mlp_supported(torch.zeros(1, 300, 16, device='cuda'), 3, 80, 784)   # NC = 44
    assert not ops.point_mlp_supported(x, 5, 80, 784) and not ops.point_mlp_supported(x, 3, 80, 8)
    assert lib().dm_point_mlp_fwd(None, 1, 16, 256, 80, 256, 3, None, None, None, None, 80, None, None, 16, None, 784,
                                  None) == -3       # bit 4: the bf16x3 mode is refused, the kernels are exact fp32


# ------------------------------------------------------------------------------------------------ the head
def _configs(golden_dir):
    import json
    from dynamask_amd import registry
    with open(f'{golden_dir}/g18_pointrend_configs.json') as f:
        return registry._to_cfgdict(json.load(f))['coco']


def _roi_head(golden_dir):
    import pointrend_inputs as pi
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _configs(golden_dir)
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=registry._to_cfgdict(dict(pi.TEST_CFG)))
    torch.manual_seed(0)
    m = registry.build_head(rh)
    sd = {k: v.shape for k, v in m.state_dict().items() if k.startswith(('mask_head.', 'point_head.'))}
    m.load_state_dict(pi.head_state(sd), strict=False)
    return m.cuda().eval()


def _golden(golden_dir):
    return np.load(f'{golden_dir}/g18_pointrend.npz')


def _rois(det):
    return torch.cat([det.new_zeros((len(det), 1)), det[:, :4]], 1).contiguous()


class _Capture:
    """Records the index sets ops.point_select returns."""

    def __init__(self, monkeypatch):
        from dynamask_amd import ops
        self.sets = []
        orig = ops.point_select

        def sel(*a, **k):
            r = orig(*a, **k)
            self.sets.append(r.clone())
            return r
        monkeypatch.setattr(ops, 'point_select', sel)


def _bits(z, key):
    shape = tuple(z[key + '_shape'])
    return np.unpackbits(z[key + 's'], axis=-1)[..., :shape[-1]].astype(bool)


def _stack_segm(segm, labels):
    seen, out = {}, []
    for c in labels:
        j = seen.get(c, 0)
        seen[c] = j + 1
        out.append(np.asarray(segm[c][j]))
    return np.stack(out)


def _assert_bitmaps(got, ref, probs, boxes, shape, what, apply_sigmoid=True):
    """Equal except at pixels whose pasted probability is within 1e-3 of the threshold."""
    from dynamask_amd import ops
    assert got.shape == ref.shape
    diff = got != ref
    if diff.any():
        lo = ops.paste_masks(probs, boxes, shape[1], shape[2], 0.5 - 1e-3, apply_sigmoid=apply_sigmoid).cpu().numpy()
        hi = ops.paste_masks(probs, boxes, shape[1], shape[2], 0.5 + 1e-3, apply_sigmoid=apply_sigmoid).cpu().numpy()
        bad = diff & ~(lo.astype(bool) != hi.astype(bool))
        assert not bad.any(), f'{what}: {int(bad.sum())} bitmap pixels differ away from the threshold'
    print(f'{what}: {int(diff.sum())} of {diff.size} pixels differ (all at the threshold)')


def test_head_matches_the_reference(golden_dir, monkeypatch):
    """Coarse logits, the index sets of every refined step, the refined 224^2 label-channel logits and the bitmaps of
    simple_test_mask against the reference.  Index sets must be equal wherever the reference's cut has a gap (P-th to
    (P+1)-th smallest |v|) above the rounding level; the ties are counted."""
    import pointrend_inputs as pi
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    det, lab = pi.detections()
    det, lab = det.cuda(), lab.cuda()
    x = [pi.p2().cuda()]
    cap = _Capture(monkeypatch)
    with torch.no_grad():
        coarse = m._mask_forward(x, _rois(det))['mask_pred']
        refined = m.simple_test_mask_logits(x, det, lab)
        segm = m.simple_test_mask(x, pi.img_metas(), det, lab)
    assert_grad_close(coarse, z['coarse'], 'coarse logits', rel=1e-4)
    assert len(cap.sets) >= 4
    ties = 0
    for s in range(4):
        got = cap.sets[s].cpu().numpy()
        gap = z[f'select{s}_gap']
        for r in range(len(gap)):
            if gap[r] <= 1e-5:
                ties += 1
                continue
            assert np.array_equal(got[r], z[f'select{s}'][r]), f'step {s} RoI {r}: index sets differ'
    print(f'cuts within the rounding level (not compared): {ties}')
    assert_grad_close(refined, z['refined'], 'refined label-channel logits', rel=1e-4)
    ref_bits = _bits(z, 'bitmap')
    _assert_bitmaps(_stack_segm(segm, lab.tolist()), ref_bits, refined, det[:, :4].contiguous(), ref_bits.shape,
                    'simple_test_mask bitmaps')


def test_label_channel_equals_the_all_class_computation(golden_dir):
    """The label-only shortcut against the whole [n, 80, 224, 224] computation of the reference loop, restated in
    float64 on the same coarse logits and features (two RoIs)."""
    import pointrend_inputs as pi
    m = _roi_head(golden_dir)
    det, lab = pi.detections()
    det, lab = det[:2].cuda(), lab[:2].cuda()
    x = [pi.p2().cuda()]
    rois = _rois(det)
    with torch.no_grad():
        coarse = m._mask_forward(x, rois)['mask_pred']
        got = m._mask_point_forward_test(x, rois, lab, coarse).cpu().double()
    ph = m.point_head
    ws = [f.conv.weight.detach().cpu()[..., 0] for f in ph.fcs]
    bs = [f.conv.bias.detach().cpu() for f in ph.fcs]
    wl, bl = ph.fc_logits.weight.detach().cpu()[..., 0], ph.fc_logits.bias.detach().cpu()
    n = 2
    crs, feat, r64, lab_c = coarse.cpu().double(), x[0].cpu().double(), rois.cpu().double(), lab.cpu()
    full = crs.clone()
    for step in range(5):
        full = F.interpolate(full, scale_factor=2, mode='bilinear', align_corners=False)
        H, W = full.shape[2:]
        if 784 >= 4 * H * W and step < 4:
            continue
        idx = _select_ref(full[torch.arange(n), lab_c], min(784, H * W))
        pts = _gather_ref(feat, r64, crs, idx, H, W, 0.25, torch.float64)
        logits = _mlp_ref(pts, ws, bs, wl, bl, torch.float64)
        full = full.view(n, 80, H * W).scatter_(2, idx[:, None].expand(-1, 80, -1), logits).view(n, 80, H, W)
    ref = full[torch.arange(n), lab_c][:, None]
    assert full.shape == (2, 80, 224, 224)
    assert_grad_close(got, ref, 'label channel vs the all-class float64 loop', rel=1e-4)


def _feats4(seed, h, w, B=1):
    g = _g(seed)
    return [torch.randn(B, 256, h // s, w // s, generator=g).cuda() for s in (4, 8, 16, 32)]


def _proposals(n, seed, h, w):
    g = _g(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([w, h]) * 0.8
    wh = torch.rand(n, 2, generator=g) * torch.tensor([w, h]) * 0.3 + 8
    return torch.cat([xy, xy + wh, torch.rand(n, 1, generator=g)], 1).cuda()


def test_zero_and_one_detection(golden_dir):
    import pointrend_inputs as pi
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    x = [pi.p2().cuda()]
    det, lab = pi.detections()
    with torch.no_grad():
        segm = m.simple_test_mask(x, pi.img_metas(), det[:0].cuda(), lab[:0].cuda())
        assert len(segm) == 80 and all(s == [] for s in segm)
        assert tuple(m.simple_test_mask_logits(x, det[:0].cuda(), lab[:0].cuda()).shape) == (0, 1, 224, 224)
        one = m.simple_test_mask_logits(x, det[:1].cuda(), lab[:1].cuda())
    assert_grad_close(one, z['refined'][:1], 'one detection', rel=1e-4)


def test_100_detections_fused_vs_unfused(golden_dir):
    """100 detections at 1333 x 800: the refined maps of the fused and the unfused point MLP.  A cell may differ where
    the two disagree about a selection at a cut within rounding; the rest agree to fp32 tolerance."""
    from dynamask_amd import ops
    m = _roi_head(golden_dir)
    x = _feats4(9, 800, 1344)
    det = _proposals(100, 10, 800, 1333)
    lab = torch.randint(0, 80, (100,), generator=_g(2)).cuda()
    outs = {}
    for fused in (True, False):
        old = ops.FUSED_POINT_MLP[0]
        ops.FUSED_POINT_MLP[0] = fused
        try:
            with torch.no_grad():
                outs[fused] = m.simple_test_mask_logits(x, det, lab).cpu()
        finally:
            ops.FUSED_POINT_MLP[0] = old
    a, b = outs[True], outs[False]
    assert a.shape == (100, 1, 224, 224) and bool(torch.isfinite(a).all())
    close = (a - b).abs() <= 1e-4 * (1 + b.abs())
    frac = float((~close).float().mean())
    print(f'100 detections: {frac:.2e} of the cells differ between fused and unfused')
    assert frac < 1e-3


def test_encode_equals_host_rle(golden_dir):
    """simple_test_mask(encode=True): the COCO RLE of simple_test_mask's bitmaps (the host encoder of oracle/ref_ops)."""
    import pointrend_inputs as pi
    from oracle import ref_ops
    m = _roi_head(golden_dir)
    x = [pi.p2().cuda()]
    det, lab = pi.detections()
    det, lab = det.cuda(), lab.cuda()
    with torch.no_grad():
        bits = m.simple_test_mask(x, pi.img_metas(), det, lab)
        rles = m.simple_test_mask(x, pi.img_metas(), det, lab, encode=True)
    assert [len(c) for c in bits] == [len(c) for c in rles] and sum(len(c) for c in bits) == 3
    for cb, cr in zip(bits, rles):
        for b, r in zip(cb, cr):
            assert r == ref_ops.rle_encode(b.astype(np.uint8))


@pytest.mark.parametrize('B', (1, 2, 4))
def test_batch_equals_simple_test(golden_dir, B):
    import pointrend_inputs as pi
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 12
    h, w = pi.IMG_H, pi.IMG_W
    xs = [_feats4(50 + b, h, w) for b in range(B)]
    props = [_proposals(60, 70 + b, h, w) for b in range(B)]
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


def test_aug_test(golden_dir):
    """One view equals simple_test bit for bit; the flip pair matches the reference's aug_test_mask."""
    import pointrend_inputs as pi
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    h, w = pi.IMG_H, pi.IMG_W
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 12
    x = _feats4(80, h, w)
    props = _proposals(60, 81, h, w)
    meta = pi.img_metas()[0]
    with torch.no_grad():
        aug = m.aug_test([x], [props[:, :4]], [[meta]])
        single = m.simple_test(x, [props[:, :4]], [meta])
    for c in range(80):
        assert len(aug[1][c]) == len(single[1][c])
        for u, v in zip(aug[1][c], single[1][c]):
            assert np.array_equal(u, v)
    xs, metas = pi.aug_views()
    det, lab = pi.detections()
    det, lab = det.cuda(), lab.cuda()
    with torch.no_grad():
        segm = m.aug_test_mask([[v.cuda()] for v in xs], metas, det, lab)
        probs = m.aug_test_mask_probs([[v.cuda()] for v in xs], metas, det, lab)
    ref_bits = _bits(z, 'aug_bitmap')
    _assert_bitmaps(_stack_segm(segm, lab.tolist()), ref_bits, probs, det[:, :4].contiguous(), ref_bits.shape,
                    'aug_test_mask bitmaps', apply_sigmoid=False)
