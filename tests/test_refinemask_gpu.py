"""RefineMask inference on the MI355X: the dilated / any-width 3x3 kernels (csrc/conv_dilated.hip) at every shape of the
grid their support checks take, RefineMaskHead / RefineRoIHead against the reference (tests/golden/g17_refine.npz), and the
RoI head through the registry, batched and under test-time augmentation.

Kernel cases compare with ``F.conv2d(..., dilation=d, padding=d)`` on the CPU in float64 (``assert_close_via_f64``, the
float32 CPU convolution as the fp32 reference).  Large cases check a spread of output channels (every 32-row block of
the cout tile, both halves of the MFMA rows) at every pixel, so that a leak across tile, RoI or image edges shows; the
output buffer is followed by a canary that must survive."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

CANARY = 7.0


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _sel(cout, full):
    """Output channels checked: all, or a spread that hits every 32-row block and both 4-row halves of the MFMA rows."""
    if full:
        return torch.arange(cout)
    s = sorted({c for b in range(0, cout, 32) for c in (b, b + 5, b + 13, b + 22, b + 31) if c < cout} | {cout - 1})
    return torch.tensor(s)


def _ref(x, w, b, d, sel, relu=True):
    """(fp32, fp64) CPU references of relu(conv3x3_d(x) + b) for the output channels ``sel``."""
    outs = []
    for dt in (torch.float32, torch.float64):
        y = F.conv2d(x.to(dt), w[sel].to(dt), b[sel].to(dt), padding=d, dilation=d)
        outs.append(y.clamp_min(0) if relu else y)
    return outs


def _case(N, C, H, W, cout, seed):
    g = _g(seed)
    x = torch.randn(N, C, H, W, generator=g)
    # distinct content per RoI / image: an offset that grows with the index
    x += torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1) * 0.01
    ws = [torch.randn(cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5 for _ in range(3)]
    bs = [torch.randn(cout, generator=g) * 0.1 for _ in range(3)]
    return x, ws, bs


def _out_with_canary(N, cout, H, W):
    n = N * cout * H * W
    buf = torch.full((n + 4096,), CANARY, device='cuda')
    return buf, buf[:n].view(N, cout, H, W)


def _check_canary(buf, n, what):
    assert bool((buf[n:] == CANARY).all()), f'{what}: the canary past the output was overwritten'


ROI_GRID = [(N, C, S) for N in (1, 3, 50, 100, 300) for C, S in ((256, 14), (128, 28), (64, 56))]


@pytest.mark.parametrize('N,C,S', ROI_GRID)
def test_dilated_conv_roi_maps(N, C, S):
    """Each single dilation (1, 3, 5) and the multi-branch sum, fused and unfused, on [N, C, S, S] RoI maps."""
    from dynamask_amd import ops
    x, ws, bs = _case(N, C, S, S, C, 1000 * N + S)
    xd = x.cuda()
    wps = [ops.pack_conv_weight(w.cuda()) for w in ws]
    bds = [b.cuda() for b in bs]
    sel = _sel(C, N * C * C * S * S <= 3 * 256 * 256 * 196)
    dil = (1, 3, 5)
    refs = []
    for i, d in enumerate(dil):
        assert ops.conv3x3_dil_supported(xd, C, d)
        buf, out = _out_with_canary(N, C, S, S)
        ops.conv3x3_dil(xd, wps[i], bds[i], C, d, relu=True, out=out)
        r32, r64 = _ref(x, ws[i], bs[i], d, sel)
        assert_close_via_f64(out.cpu()[:, sel], r32, r64, name=f'd={d} N={N} C={C} S={S}')
        _check_canary(buf, out.numel(), f'd={d}')
        refs.append((r32, r64))
    assert ops.conv3x3_multidil_supported(xd, C, dil)
    buf_f, fused = _out_with_canary(N, C, S, S)
    ops.conv3x3_multidil(xd, wps, bds, C, dil, out=fused, fused=True)
    buf_u, unfused = _out_with_canary(N, C, S, S)
    ops.conv3x3_multidil(xd, wps, bds, C, dil, out=unfused, fused=False)
    assert torch.equal(fused, unfused), 'fused and unfused branch sums differ'
    r32 = refs[0][0] + refs[1][0] + refs[2][0]
    r64 = refs[0][1] + refs[1][1] + refs[2][1]
    assert_close_via_f64(fused.cpu()[:, sel], r32, r64, name=f'multi-branch N={N} C={C} S={S}')
    _check_canary(buf_f, fused.numel(), 'fused')
    _check_canary(buf_u, unfused.numel(), 'unfused')


@pytest.mark.parametrize('B', (1, 2))
@pytest.mark.parametrize('H,W', ((200, 336), (336, 200), (256, 512), (13, 17)))
def test_semantic_conv_whole_maps(B, H, W):
    """RefineMask's semantic 3x3 (d = 1, 256 -> 256 + ReLU) on whole stride-4 maps, landscape, portrait, Cityscapes."""
    from dynamask_amd import ops
    C = 256
    x, ws, bs = _case(B, C, H, W, C, 7 * H + W + B)
    xd = x.cuda()
    assert ops.conv3x3_dil_supported(xd, C, 1)
    buf, out = _out_with_canary(B, C, H, W)
    ops.conv3x3_dil(xd, ops.pack_conv_weight(ws[0].cuda()), bs[0].cuda(), C, 1, relu=True, out=out)
    sel = _sel(C, H * W < 1000)
    r32, r64 = _ref(x, ws[0], bs[0], 1, sel)
    assert_close_via_f64(out.cpu()[:, sel], r32, r64, name=f'semantic B={B} {H}x{W}')
    _check_canary(buf, out.numel(), 'semantic')


@pytest.mark.parametrize('d', (2, 4, 7, 8))
def test_dilations_beyond_the_config(d):
    """Every dilation the support check takes has its own halo: d = 2, 4, 7, 8 on a ragged map, bias-free, no ReLU,
    the ADD epilogue (out += value), and a cout count that is not a multiple of 32."""
    from dynamask_amd import ops
    N, C, H, W, cout = 3, 24, 19, 37, 40
    x, ws, bs = _case(N, C, H, W, cout, 50 + d)
    xd = x.cuda()
    wp = ops.pack_conv_weight(ws[0].cuda())
    base = torch.randn(N, cout, H, W, generator=_g(d))
    out = base.cuda()
    ops.conv3x3_dil(xd, wp, None, cout, d, relu=False, add=True, out=out)
    sel = torch.arange(cout)
    r32, r64 = _ref(x, ws[0], torch.zeros(cout), d, sel, relu=False)
    assert_close_via_f64(out.cpu(), r32 + base, r64 + base.double(), name=f'd={d} add')


def test_support_checks_and_refusals():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    x = torch.randn(2, 64, 14, 14, device='cuda')
    w = ops.pack_conv_weight(torch.randn(64, 64, 3, 3, device='cuda'))
    assert not ops.conv3x3_dil_supported(x, 64, 0) and not ops.conv3x3_dil_supported(x, 64, 9)
    assert not ops.conv3x3_dil_supported(torch.empty(2, 12, 14, 14, device='cuda'), 64, 1)      # C % 8
    assert not ops.conv3x3_multidil_supported(x, 64, (1, 3)) and not ops.conv3x3_multidil_supported(x, 64, (1, 3, 9))
    out = torch.full((2, 64, 14, 14), CANARY, device='cuda')
    for d in (0, 9):
        with pytest.raises(RuntimeError):
            ops.conv3x3_dil(x, w, None, 64, d, out=out)
    # bit 1 (dm_conv2d_fwd's add-before-ReLU) is not a flag of these launches; bit 4 (bf16x3) is unsupported
    from dynamask_amd.ops import _p, _stream
    assert lib().dm_conv3x3_dil_fwd(_p(x), 2, 64, 14, 14, _p(w), None, 64, 1, 2, _p(out), _stream()) == -1
    assert lib().dm_conv3x3_dil_fwd(_p(x), 2, 64, 14, 14, _p(w), None, 64, 1, 16, _p(out), _stream()) == -3
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    with pytest.raises(ValueError):
        ops.conv3x3_dil(x, ops.pack_conv_weight(torch.randn(64, 64, 3, 3, device='cuda'), precision='bf16x3'), None, 64, 1)


def test_whole_map_is_past_the_flat_row_kernel():
    """The reason for the new kernel: dm_conv2d_fwd's 3x3 plane of whole rows does not fit a 336-wide map."""
    from dynamask_amd import ops
    x = torch.randn(1, 256, 200, 336, device='cuda')
    w = ops.pack_conv_weight(torch.randn(256, 256, 3, 3, device='cuda'))
    with pytest.raises(RuntimeError, match='dm_conv2d_fwd'):
        ops.conv2d([x], w, None, 256, 3, relu=True)
    y = ops.conv3x3_dil(x, w, None, 256, 1, relu=True)
    assert torch.isfinite(y).all()


def test_precision_mode_leaves_the_new_kernels_exact():
    """Under set_conv_precision('bf16x3') the dilated kernels give the fp32 bits, in the ops and inside the head (the
    semantic convs, the branch sums); the head's other convolutions follow the mode as everywhere else."""
    import dynamask_amd
    from dynamask_amd import ops
    x, ws, bs = _case(5, 128, 28, 28, 128, 3)
    xd = x.cuda()
    wps = [ops.pack_conv_weight(w.cuda()) for w in ws]
    bds = [b.cuda() for b in bs]
    head, (feats, sem, rois, labels) = _small_head()
    mbf = head.stages[1].fuse_conv[1]
    y = torch.randn(4, 128, 28, 28, generator=_g(9)).cuda()

    def run():
        return [ops.conv3x3_dil(xd, wps[0], bds[0], 128, 3, relu=True), ops.conv3x3_multidil(xd, wps, bds, 128, (1, 3, 5)),
                *head.semantic_forward(sem), mbf.branch_sum(y), mbf.branch_sum(y, fused=False)]
    with torch.no_grad():
        a = run()
        with dynamask_amd.conv_precision('bf16x3'):
            b = run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ------------------------------------------------------------------ heads
def _configs(golden_dir):
    import json
    from dynamask_amd import registry
    with open(f'{golden_dir}/g17_refine_configs.json') as f:
        return registry._to_cfgdict(json.load(f))


def _roi_head(golden_dir, name='coco', **mask_head_kw):
    """The config's RefineRoIHead through the registry, mask head with the fixture's seeded weights, on the GPU."""
    import refine_inputs as ri
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _configs(golden_dir)[name]
    rh = dict(cfg.model.roi_head)
    if mask_head_kw:
        mh = dict(rh['mask_head'])
        mh.update(mask_head_kw)
        rh['mask_head'] = mh
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=cfg.test_cfg.rcnn)
    torch.manual_seed(0)
    m = registry.build_head(rh)
    sd = m.mask_head.state_dict()
    m.mask_head.load_state_dict(ri.head_state({k: v.shape for k, v in sd.items()}), strict=True)
    return m.cuda().eval()


def _small_head():
    import refine_inputs as ri
    from dynamask_amd import registry, mask_heads, losses  # noqa: F401
    from dynamask_amd.mask_heads import RefineMaskHead
    head = RefineMaskHead(**ri.HEAD_CFG)
    head.load_state_dict(ri.head_state({k: v.shape for k, v in head.state_dict().items()}), strict=True)
    head = head.cuda().eval()
    g = _g(5)
    n = 6
    feats = torch.randn(n, 256, 14, 14, generator=g).cuda()
    sem = torch.randn(1, 256, 48, 64, generator=g).cuda()
    xy = torch.rand(n, 2, generator=g) * 200
    wh = torch.rand(n, 2, generator=g) * 60 + 2
    rois = torch.cat([torch.zeros(n, 1), xy, xy + wh], 1).cuda()
    labels = torch.randint(0, 80, (n,), generator=g).cuda()
    return head, (feats, sem, rois, labels)


def _golden(golden_dir):
    return np.load(f'{golden_dir}/g17_refine.npz')


def _feats():
    import refine_inputs as ri
    return [f.cuda() for f in ri.fpn_feats()]


def test_head_matches_the_reference(golden_dir):
    """The four stage logits and semantic_pred of RefineRoIHead._mask_forward against the reference's, and the
    boundary merge of the reference's own stage logits against its merged logits."""
    import refine_inputs as ri
    from dynamask_amd import ops
    from tolerances import assert_grad_close
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    det, lab = ri.detections()
    rois = torch.cat([torch.zeros(len(det), 1), det[:, :4]], 1).cuda()
    with torch.no_grad():
        res = m._mask_forward(_feats(), rois, lab.cuda())
    assert_grad_close(res['semantic_pred'], z['semantic_pred'], 'semantic_pred', rel=1e-4)
    for i, p in enumerate(res['stage_instance_preds']):
        assert_grad_close(p, z[f'stage{i}'], f'stage {i} logits', rel=1e-3)
    # the merge itself, on the reference's stage logits (the reference interpolates with F.interpolate on the CPU: the
    # interpolated values may differ in the last bits, the boundary decisions may not)
    preds = [torch.from_numpy(z[f'stage{i}']).cuda() for i in range(4)]
    merged = m.merge_stage_preds(preds).cpu()
    ref = torch.from_numpy(z['merged'])
    assert_grad_close(merged, ref, 'merged logits of the reference stage logits', rel=1e-5)


def test_simple_test_mask_matches_the_reference(golden_dir):
    """simple_test_mask: the merged 112 x 112 logits and the bitmaps.  A merged pixel may differ where a stage's
    probability sits within the tolerance of the 0.5 boundary decision; bitmaps must be equal except at pixels whose
    pasted probability is within the tolerance of the threshold."""
    import refine_inputs as ri
    from dynamask_amd import ops
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    det, lab = ri.detections()
    det, lab = det.cuda(), lab.cuda()
    x = _feats()
    with torch.no_grad():
        merged = m.simple_test_mask_logits(x, det, lab).cpu()
        segm = m.simple_test_mask(x, ri.img_metas(), det, lab)
    ref = torch.from_numpy(z['merged'])
    close = (merged - ref).abs() <= 1e-3 * (1 + ref.abs())
    assert float(close.float().mean()) > 0.995, f'merged logits: {float((~close).float().mean()):.4f} of the pixels differ'
    shape = tuple(z['bitmap_shape'])
    ref_bits = np.unpackbits(z['bitmaps'], axis=-1)[..., :shape[-1]].astype(bool)
    seen, got = {}, []
    for c in lab.tolist():
        j = seen.get(c, 0)
        seen[c] = j + 1
        got.append(segm[c][j])
    got = np.stack(got)
    assert got.shape == ref_bits.shape
    diff = got != ref_bits
    if diff.any():
        tol = 1e-3
        boxes = det[:, :4].contiguous()
        lo = ops.paste_masks(merged.cuda().contiguous(), boxes, shape[1], shape[2], 0.5 - tol, apply_sigmoid=True).cpu().numpy()
        hi = ops.paste_masks(merged.cuda().contiguous(), boxes, shape[1], shape[2], 0.5 + tol, apply_sigmoid=True).cpu().numpy()
        ambiguous = lo.astype(bool) != hi.astype(bool)
        bad = diff & ~ambiguous
        assert not bad.any(), f'{int(bad.sum())} bitmap pixels differ away from the threshold'


def _proposals(n, seed):
    import refine_inputs as ri
    g = _g(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([ri.IMG_W, ri.IMG_H]) * 0.8
    wh = torch.rand(n, 2, generator=g) * 120 + 8
    return torch.cat([xy, xy + wh, torch.rand(n, 1, generator=g)], 1).cuda()


@pytest.mark.parametrize('n_det', (0, 1, 100))
def test_simple_test_through_the_registry(golden_dir, n_det):
    """simple_test (bbox branch + masks) with 0, 1 and 100 detections: bitmaps of the image's size per class, and for
    the masks the same as simple_test_mask on the same detections."""
    import refine_inputs as ri
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = max(n_det, 1)
    x = _feats()
    props = _proposals(400, 11)
    with torch.no_grad():
        if n_det == 0:
            det = props.new_zeros((0, 5))
            lab = torch.zeros((0,), dtype=torch.long, device='cuda')
            segm = m.simple_test_mask(x, ri.img_metas(), det, lab)
            assert len(segm) == 80 and all(s == [] for s in segm)
            return
        bbox_res, segm = m.simple_test(x, [props], ri.img_metas())
        n = sum(len(b) for b in bbox_res)
        assert n == n_det
        assert len(segm) == 80 and sum(len(s) for s in segm) == n
        for c in range(80):
            assert len(segm[c]) == len(bbox_res[c])
            for s in segm[c]:
                assert s.shape == (ri.IMG_H, ri.IMG_W) and s.dtype == np.bool_


def test_lvis_shape_300_detections(golden_dir):
    """simple_test_mask with 300 given detections, 1203 classes and the class-agnostic last stage (the LVIS config)."""
    import refine_inputs as ri
    m = _roi_head(golden_dir, 'lvis')
    assert m.mask_head.stage_num_classes[0] == 1203 and m.mask_head.stage_num_classes[-1] == 1
    det = _proposals(300, 12)
    lab = torch.randint(0, 1203, (300,), generator=_g(3)).cuda()
    with torch.no_grad():
        res = m._mask_forward(_feats(), torch.cat([det.new_zeros((300, 1)), det[:, :4]], 1), lab)
        segm = m.simple_test_mask(_feats(), ri.img_metas(), det, lab)
    assert [tuple(p.shape) for p in res['stage_instance_preds']] == [(300, 1, s, s) for s in (14, 28, 56, 112)]
    assert all(torch.isfinite(p).all() for p in res['stage_instance_preds'])
    assert len(segm) == 1203 and sum(len(s) for s in segm) == 300
    for c, lst in enumerate(segm):
        assert len(lst) == int((lab == c).sum())


def test_batch_and_tta_equal_simple_test(golden_dir):
    """batch_simple_test over B = 3 images equals per-image simple_test; one aug_test view at scale 1.0 equals
    simple_test's masks."""
    import refine_inputs as ri
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 20
    g = _g(21)
    xs = [[torch.randn(1, 256, ri.IMG_H // s, ri.IMG_W // s, generator=g).cuda() for s in ri.STRIDES] for _ in range(3)]
    props = [_proposals(200, 30 + b) for b in range(3)]
    metas = [ri.img_metas()[0] for _ in range(3)]
    with torch.no_grad():
        xb = [torch.cat([xs[b][l] for b in range(3)]) for l in range(4)]
        batch = m.batch_simple_test(xb, props, metas)
        for b in range(3):
            single = m.simple_test(xs[b], [props[b]], [metas[b]])
            for c in range(80):
                assert len(single[1][c]) == len(batch[b][1][c])
                for u, v in zip(single[1][c], batch[b][1][c]):
                    assert np.array_equal(u, v)
        aug = m.aug_test([xs[0]], [props[0][:, :4]], [[metas[0]]])
        single = m.simple_test(xs[0], [props[0][:, :4]], [metas[0]])
    for c in range(80):
        assert len(aug[1][c]) == len(single[1][c])
        for u, v in zip(aug[1][c], single[1][c]):
            assert np.array_equal(u, v)
