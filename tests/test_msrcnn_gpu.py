"""Mask Scoring R-CNN inference on the MI355X: the kernels of csrc/conv_strided.hip against torch restatements (the
stride-2 3x3 convolution in float64 at every shape form its support check admits and in every split form, the IoU-head
input, the mask scores), and MaskScoringRoIHead against the reference (tests/golden/g19_msrcnn.npz) through the
registry: simple_test_mask (masks and scores), encode=True, empty detections, batches, one mask branch per call and the
bf16x3 mode.  Output buffers are followed by a canary that must survive."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

CANARY = 7.0


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _vp(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------ the stride-2 conv
# (NB, C, H, W, Cout, splits): even / odd maps (14, 13, 2, 1, mixed), 1 .. 300 RoIs, Cout below, at and past a tile
# (64 / 128) and not a multiple of it, the automatic split and each forced one
S2_CASES = [
    (1, 8, 1, 1, 1, 1),
    (3, 16, 2, 2, 33, 2),
    (2, 24, 1, 14, 64, 0),
    (5, 256, 13, 13, 256, 0),
    (16, 256, 14, 14, 256, 0),
    (100, 256, 14, 14, 256, 0),
    (7, 64, 14, 13, 200, 4),
    (300, 16, 14, 14, 40, 2),
    (4, 32, 13, 2, 130, 4),
    (9, 256, 14, 14, 256, 1),
    (9, 256, 14, 14, 256, 2),
    (9, 256, 14, 14, 256, 4),
    (9, 256, 14, 14, 256, 8),
]


@pytest.mark.parametrize('NB,C,H,W,cout,splits', S2_CASES)
def test_conv3x3_s2(NB, C, H, W, cout, splits):
    from dynamask_amd import ops
    g = _g(NB * 1000 + C + H + W + cout + splits)
    x = torch.randn(NB, C, H, W, generator=g)
    w = torch.randn(cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xd = x.cuda()
    assert ops.conv3x3_s2_supported(xd, cout, splits)
    wq = ops.pack_conv_weight(w.cuda())
    shape = (NB, cout, (H + 1) // 2, (W + 1) // 2)
    total = int(np.prod(shape))
    buf = torch.full((total + 257,), CANARY, device='cuda')
    out = buf[:total].view(shape)
    with torch.no_grad():
        ops.conv3x3_s2(xd, wq, b.cuda(), cout, relu=True, splits=splits, out=out)
        again = ops.conv3x3_s2(xd, wq, b.cuda(), cout, relu=True, splits=splits)
    torch.cuda.synchronize()
    assert bool((buf[total:] == CANARY).all()), 'the canary past the output was overwritten'
    assert torch.equal(out, again), 'two runs differ'
    r32 = F.relu(F.conv2d(x, w, b, stride=2, padding=1))
    r64 = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))
    assert tuple(r64.shape) == shape
    assert_close_via_f64(out, r32, r64, f'conv3x3_s2 NB={NB} C={C} {H}x{W} Cout={cout} splits={splits}', rel=1e-5)


def test_conv3x3_s2_without_relu_and_bias():
    from dynamask_amd import ops
    g = _g(5)
    x = torch.randn(6, 32, 14, 14, generator=g)
    w = torch.randn(96, 32, 3, 3, generator=g) * 0.1
    with torch.no_grad():
        got = ops.conv3x3_s2(x.cuda(), ops.pack_conv_weight(w.cuda()), None, 96, relu=False, splits=2)
    r32 = F.conv2d(x, w, None, stride=2, padding=1)
    r64 = F.conv2d(x.double(), w.double(), None, stride=2, padding=1)
    assert float(r64.min()) < 0
    assert_close_via_f64(got, r32, r64, 'conv3x3_s2 without ReLU / bias', rel=1e-5)


@pytest.mark.parametrize('NB,C,H,W,cout', ((3, 16, 5, 7, 33), (2, 24, 14, 13, 130)))
def test_conv3x3_s2_is_the_subsampled_dilation_1_conv(NB, C, H, W, cout):
    """One split of the stride-2 kernel gives the bits of the stride-1 kernel (conv3x3_dil, d = 1) at the even pixels:
    both walk K as 8-channel chunks x taps 0 .. 8 x the same quad order (the tap loop of csrc/mfma_tile.h, which the
    dilated kernel holds written out), and padding contributes fma(0, w, acc) in both."""
    from dynamask_amd import ops
    g = _g(NB + C + H + W + cout)
    x = torch.randn(NB, C, H, W, generator=g).cuda()
    wq = ops.pack_conv_weight((torch.randn(cout, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda())
    b = (torch.randn(cout, generator=g) * 0.1).cuda()
    for relu in (False, True):
        with torch.no_grad():
            s2 = ops.conv3x3_s2(x, wq, b, cout, relu=relu, splits=1)
            d1 = ops.conv3x3_dil(x, wq, b, cout, 1, relu=relu)
        assert torch.equal(s2, d1[..., ::2, ::2]), f'relu={relu}'


def test_conv3x3_s2_refusals():
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_conv3x3_s2_supported(16, 256, 14, 14, 256, 0) == 1
    for args in ((0, 256, 14, 14, 256, 0), (16, 12, 14, 14, 256, 0), (16, 4, 14, 14, 256, 0), (16, 256, 0, 14, 256, 0),
                 (16, 256, 14, 14, 0, 0), (16, 256, 14, 14, 256, 3), (16, 256, 14, 14, 256, 16),
                 (16, 32, 14, 14, 256, 8)):         # 8 splits of 4 chunks
        assert L.dm_conv3x3_s2_supported(*args) == 0, args
        assert L.dm_conv3x3_s2_workspace_floats(*args) == -1, args
    assert L.dm_conv3x3_s2_workspace_floats(2, 32, 14, 14, 64, 1) == 0
    assert L.dm_conv3x3_s2_workspace_floats(2, 32, 14, 14, 64, 4) == 4 * 2 * 64 * 49
    x = torch.zeros(2, 32, 14, 14, device='cuda')
    wq = torch.zeros(9 * 8 * 64 * 4, device='cuda')
    out = torch.zeros(2, 64, 7, 7, device='cuda')
    ws = torch.zeros(4 * 2 * 64 * 49, device='cuda')
    call = lambda flags, splits=1, ws_=None, n=0: L.dm_conv3x3_s2_fwd(_vp(x), 2, 32, 14, 14, _vp(wq), None, 64, splits,
                                                                     flags, _vp(out), _vp(ws_), n, None)
    assert call(16) == -3                          # bit 4: the bf16x3 mode is refused, the kernel is exact fp32
    assert call(2) == -1                           # dm_conv2d_fwd's add-before-ReLU bit is not one of its flags
    assert call(4) == -1
    assert call(0, splits=4, ws_=ws, n=ws.numel() - 1) == -1     # workspace too small
    assert call(0, splits=4, ws_=None, n=0) == -1
    assert call(0, splits=3) == -3
    assert call(9) == 0                            # ReLU + the scheduling hint
    assert call(0, splits=4, ws_=ws, n=ws.numel()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ IoU-head input, scores
@pytest.mark.parametrize('C,S', ((80, 28), (1, 28), (80, 13)))
def test_mask_iou_input(C, S):
    from dynamask_amd._lib import lib
    n = 7
    g = _g(C + S)
    pred = torch.randn(n, C, S, S, generator=g) * 4
    pred[0, :, 0, 0] = float('nan')
    labels = torch.randint(0, C, (n,), generator=g)
    ho = S // 2
    total = n * ho * ho
    buf = torch.full((total + 64,), CANARY, device='cuda')
    lab = labels.cuda() if C > 1 else None
    pred_d = pred.cuda()
    rc = lib().dm_mask_iou_input(_vp(pred_d), n, C, S, S, _vp(lab), _vp(buf), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[total:] == CANARY).all()), 'the canary past the pooled map was overwritten'
    got = buf[:total].view(n, 1, ho, ho).cpu()
    sel = pred[torch.arange(n), labels if C > 1 else torch.zeros(n, dtype=torch.long)]
    ref = F.max_pool2d(torch.sigmoid(sel)[:, None], 2, 2)
    assert bool(torch.isnan(got[0, 0, 0, 0])) and bool(torch.isnan(ref[0, 0, 0, 0]))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-6, atol=1e-7, equal_nan=True)
    assert lib().dm_mask_iou_input_supported(n, C, 1, S) == 0
    assert lib().dm_mask_iou_input(_vp(pred_d), n, C, S, 1, _vp(lab), _vp(buf), None) == -3
    if C > 1:
        assert lib().dm_mask_iou_input(_vp(pred_d), n, C, S, S, None, _vp(buf), None) == -1     # labels missing


def test_mask_iou_scores():
    from dynamask_amd import ops
    g = _g(3)
    iou = torch.randn(9, 80, generator=g)
    labels = torch.randint(0, 80, (9,), generator=g)
    dets = torch.rand(9, 5, generator=g)
    got = ops.mask_iou_scores(iou.cuda(), labels.cuda(), dets.cuda()).cpu()
    assert torch.equal(got, iou[torch.arange(9), labels] * dets[:, -1])
    assert ops.mask_iou_scores(iou[:0].cuda(), labels[:0].cuda(), dets[:0].cuda()).shape == (0,)


# ------------------------------------------------------------------------------------------------ the head
def _configs(golden_dir):
    import json
    from dynamask_amd import registry
    with open(f'{golden_dir}/g19_msrcnn_configs.json') as f:
        return registry._to_cfgdict(json.load(f))['coco']


def _roi_head(golden_dir):
    import msrcnn_inputs as mi
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _configs(golden_dir)
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=registry._to_cfgdict(dict(mi.TEST_CFG)))
    torch.manual_seed(0)
    m = registry.build_head(rh)
    sd = {k: v.shape for k, v in m.state_dict().items() if k.startswith(('mask_head.', 'mask_iou_head.'))}
    m.load_state_dict(mi.head_state(sd), strict=False)
    return m.cuda().eval()


def _golden(golden_dir):
    return np.load(f'{golden_dir}/g19_msrcnn.npz')


def _inputs():
    import msrcnn_inputs as mi
    det, lab = mi.detections()
    return [f.cuda() for f in mi.fpn()], det.cuda(), lab.cuda(), mi.img_metas()


def _rois(det):
    return torch.cat([det.new_zeros((len(det), 1)), det[:, :4]], 1).contiguous()


def _bits(z, key):
    shape = tuple(z[key + '_shape'])
    return np.unpackbits(z[key + 's'], axis=-1)[..., :shape[-1]].astype(bool)


def _per_detection(per_class, labels):
    seen, out = {}, []
    for c in labels:
        j = seen.get(c, 0)
        seen[c] = j + 1
        out.append(per_class[c][j])
    return out


def _assert_bitmaps(got, ref, probs, boxes, shape, what):
    """Equal except at pixels whose pasted probability is within 1e-3 of the threshold."""
    from dynamask_amd import ops
    assert got.shape == ref.shape
    diff = got != ref
    if diff.any():
        lo = ops.paste_masks(probs, boxes, shape[1], shape[2], 0.5 - 1e-3, apply_sigmoid=True).cpu().numpy()
        hi = ops.paste_masks(probs, boxes, shape[1], shape[2], 0.5 + 1e-3, apply_sigmoid=True).cpu().numpy()
        bad = diff & ~(lo.astype(bool) != hi.astype(bool))
        assert not bad.any(), f'{what}: {int(bad.sum())} bitmap pixels differ away from the threshold'
    print(f'{what}: {int(diff.sum())} of {diff.size} pixels differ (all at the threshold)')


def test_head_matches_the_reference(golden_dir):
    """MaskIoUHead.forward and simple_test_mask (bitmaps and mask scores) against the reference modules."""
    from dynamask_amd.mask_heads import select_label_channel
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    x, det, lab, metas = _inputs()
    n = len(lab)
    with torch.no_grad():
        res = m._mask_forward(x, _rois(det))
        iou = m.mask_iou_head(res['mask_feats'], res['mask_pred'], lab)
        iou_ref_form = m.mask_iou_head(res['mask_feats'], res['mask_pred'][torch.arange(n, device='cuda'), lab])
        segm, scores = m.simple_test_mask(x, metas, det, lab)
        probs = select_label_channel(res['mask_pred'], lab)
    assert tuple(iou.shape) == (n, 80)
    assert torch.equal(iou, iou_ref_form), 'the [n, C, S, S] + labels form and the reference [n, S, S] form differ'
    assert_grad_close(iou, z['mask_iou_pred'], 'mask_iou_pred', rel=1e-4)
    assert len(scores) == 80 and len(segm) == 80
    assert all(isinstance(s, np.ndarray) and s.dtype == np.float32 for s in scores)
    labels = lab.tolist()
    got_scores = np.array(_per_detection(scores, labels), dtype=np.float32)
    assert_grad_close(got_scores, z['mask_scores'], 'mask scores', rel=1e-4)
    ref_bits = _bits(z, 'bitmap')
    got_bits = np.stack([np.asarray(s) for s in _per_detection(segm, labels)])
    _assert_bitmaps(got_bits, ref_bits, probs, det[:, :4].contiguous(), ref_bits.shape, 'simple_test_mask bitmaps')


def test_encode_equals_host_rle(golden_dir):
    """simple_test_mask(encode=True) -> (COCO RLEs of the bitmaps, the same scores)."""
    from oracle import ref_ops
    m = _roi_head(golden_dir)
    x, det, lab, metas = _inputs()
    with torch.no_grad():
        bits, scores = m.simple_test_mask(x, metas, det, lab)
        rles, scores_e = m.simple_test_mask(x, metas, det, lab, encode=True)
    assert [len(c) for c in bits] == [len(c) for c in rles] and sum(len(c) for c in bits) == len(lab)
    for cb, cr in zip(bits, rles):
        for b, r in zip(cb, cr):
            assert r == ref_ops.rle_encode(b.astype(np.uint8))
    for a, b in zip(scores, scores_e):
        assert np.array_equal(a, b)


def test_empty_and_one_detection(golden_dir):
    z = _golden(golden_dir)
    m = _roi_head(golden_dir)
    x, det, lab, metas = _inputs()
    with torch.no_grad():
        segm, scores = m.simple_test_mask(x, metas, det[:0], lab[:0])
        assert segm == [[] for _ in range(80)] and scores == [[] for _ in range(80)]
        segm, scores = m.simple_test_mask(x, metas, det[:1], lab[:1])
    c = int(lab[0])
    assert len(segm[c]) == 1 and sum(len(s) for s in segm) == 1
    assert [len(s) for s in scores] == [1 if i == c else 0 for i in range(80)]
    assert_grad_close(scores[c], z['mask_scores'][:1], 'one detection', rel=1e-4)


def _proposals(n, seed, h, w):
    g = _g(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([w, h]) * 0.8
    wh = torch.rand(n, 2, generator=g) * torch.tensor([w, h]) * 0.3 + 8
    return torch.cat([xy, xy + wh, torch.rand(n, 1, generator=g)], 1).cuda()


def _batch_case(golden_dir, B):
    import msrcnn_inputs as mi
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 12
    xs = [[f.cuda() for f in mi.fpn(seed=50 + b)] for b in range(B)]
    props = [_proposals(60, 70 + b, mi.IMG_H, mi.IMG_W) for b in range(B)]
    props[1] = props[1][:0]                  # an image without proposals: its empty pair inside the batch
    metas = [mi.img_metas()[0] for _ in range(B)]
    xb = [torch.cat([xs[b][lvl] for b in range(B)]) for lvl in range(4)]
    return m, xs, xb, props, metas


def test_batch_equals_simple_test(golden_dir):
    """batch_simple_test at B = 3 gives per image what simple_test gives: bitmaps bit for bit, the scores to fp32
    rounding (the IoU head's launches split their K loops by the RoI count of the call)."""
    m, xs, xb, props, metas = _batch_case(golden_dir, 3)
    with torch.no_grad():
        batch = m.batch_simple_test(xb, props, metas)
        for b in range(3):
            segm_b, scores_b = batch[b][1]
            if b == 1:
                assert segm_b == [[] for _ in range(80)] and scores_b == [[] for _ in range(80)]
                continue
            single = m.simple_test(xs[b], [props[b]], [metas[b]])
            segm_s, scores_s = single[1]
            for c in range(80):
                assert len(segm_s[c]) == len(segm_b[c])
                for u, v in zip(segm_s[c], segm_b[c]):
                    assert np.array_equal(u, v)
                np.testing.assert_allclose(scores_b[c], scores_s[c], rtol=1e-5, atol=1e-6)
    assert sum(len(s) for s in batch[0][1][1]) > 0


def test_mask_branch_runs_once_per_call(golden_dir):
    """RoIAlign and FCNMaskHead run once per simple_test_mask / batch_simple_test call; the IoU head reads their output."""
    m, xs, xb, props, metas = _batch_case(golden_dir, 3)
    calls = {'roi': 0, 'mask': 0, 'iou': 0}

    def counted(mod, key):
        orig = mod.forward

        def f(*a, **k):
            calls[key] += 1
            return orig(*a, **k)
        mod.forward = f
    counted(m.mask_roi_extractor, 'roi')
    counted(m.mask_head, 'mask')
    counted(m.mask_iou_head, 'iou')
    x, det, lab, meta = _inputs()
    with torch.no_grad():
        m.simple_test_mask(x, meta, det, lab)
        assert calls == {'roi': 1, 'mask': 1, 'iou': 1}
        m.batch_simple_test(xb, props, metas)
        assert calls == {'roi': 2, 'mask': 2, 'iou': 2}


def test_aug_test_gives_masks_without_scores(golden_dir):
    """aug_test is the base's (the reference does not override it): one view gives simple_test's masks, no scores."""
    import msrcnn_inputs as mi
    m = _roi_head(golden_dir)
    m.test_cfg.score_thr = 0.0
    m.test_cfg.max_per_img = 12
    x = [f.cuda() for f in mi.fpn(seed=80)]
    props = _proposals(60, 81, mi.IMG_H, mi.IMG_W)
    meta = mi.img_metas()[0]
    with torch.no_grad():
        aug = m.aug_test([x], [props[:, :4]], [[meta]])
        single = m.simple_test(x, [props[:, :4]], [meta])
    assert len(aug[1]) == 80
    for c in range(80):
        assert len(aug[1][c]) == len(single[1][0][c])
        for u, v in zip(aug[1][c], single[1][0][c]):
            assert np.array_equal(u, v)


def test_bf16x3_scores_stay_close(golden_dir):
    """Under set_conv_precision('bf16x3') the stride-1 convs of both heads may run the split kernel; the scores stay
    within 1e-3 of the exact ones."""
    from dynamask_amd.precision import conv_precision
    m = _roi_head(golden_dir)
    x, det, lab, metas = _inputs()
    with torch.no_grad():
        _, exact = m.simple_test_mask(x, metas, det, lab)
        with conv_precision('bf16x3'):
            _, split = m.simple_test_mask(x, metas, det, lab)
    labels = lab.tolist()
    a = np.array(_per_detection(exact, labels))
    b = np.array(_per_detection(split, labels))
    np.testing.assert_allclose(b, a, rtol=1e-3, atol=1e-4)
