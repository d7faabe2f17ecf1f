"""Cascade Mask R-CNN on the MI355X: the stage-grouped convolution / deconvolution launches against per-problem launches
(bit for bit), the cascade stage step against bbox_decode + torch, and CascadeRoIHead's simple_test / aug_test against
the reference fixture g21 (tests/golden/make_golden_cascade.py), batch_simple_test against simple_test, and the grouped
path against the per-stage path."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=_g(seed)) * scale).cuda()


def _problems(count, NB, cin, cout, ksize, H, W, shared, seed=0):
    from dynamask_amd import ops
    x0 = _rand((NB, cin, H, W), seed)
    xs = [x0 if shared else _rand((NB, cin, H, W), seed + 10 + i) for i in range(count)]
    ws = [_rand((cout, cin, ksize, ksize), seed + 20 + i, (2.0 / (cin * ksize * ksize)) ** 0.5) for i in range(count)]
    bs = [_rand((cout,), seed + 30 + i, 0.1) for i in range(count)]
    return xs, [ops.pack_conv_weight(w) for w in ws], bs


def _per_problem_ws(x, wp, b, cout, ksize, S):
    """dm_conv2d_fwd_ws with a workspace of S problem-sized slabs (S = 1: no split)."""
    from dynamask_amd import ops
    from dynamask_amd._lib import check, lib
    NB, cin, H, W = x.shape
    out = torch.empty((NB, cout, H, W), device='cuda')
    per = NB * cout * H * W
    ws = torch.empty((max(S * per, 1),), device='cuda')
    check(lib().dm_conv2d_fwd_ws(ops._ptr_array([x]), ops._int_array([cin]), (ctypes.c_longlong * 1)(x.stride(0)), 1, NB, H,
                                 W, ops._p(wp), ops._p(b), cout, ksize, 1, ops._p(out), cout, 0, ops._p(ws), S * per,
                                 ops._stream()), 'dm_conv2d_fwd_ws')
    return out


@pytest.mark.parametrize('ksize,cin,cout,H,W', [(3, 256, 256, 14, 14), (3, 64, 48, 14, 14), (3, 32, 32, 9, 7),
                                                (1, 256, 80, 28, 28), (1, 96, 160, 14, 14), (1, 40, 24, 6, 11)])
@pytest.mark.parametrize('NB', [0, 1, 3, 16, 50])
def test_conv2d_group_equals_per_problem(ksize, cin, cout, H, W, NB):
    """Counts 1-3, distinct and shared inputs, without (= conv2d) and with a workspace (= dm_conv2d_fwd_ws of the same
    split count): bit for bit."""
    from dynamask_amd import ops
    for count in (1, 2, 3):
        for shared in (False, True):
            xs, wps, bs = _problems(count, NB, cin, cout, ksize, H, W, shared, seed=count + 7 * NB)
            got = ops.conv2d_group(xs, wps, bs, cout, ksize, relu=True, split=False)
            for i in range(count):
                if NB == 0:
                    assert tuple(got[i].shape) == (0, cout, H, W)
                    continue
                ref = ops.conv2d(xs[i], wps[i], bs[i], cout, ksize, relu=True)
                assert torch.equal(got[i], ref), f'no split: count {count} problem {i}'
            got = ops.conv2d_group(xs, wps, bs, cout, ksize, relu=True, split=True)
            nws = int(ops.lib().dm_conv2d_group_splitk_floats(count, NB, H, W, cin, cout, ksize))
            S = ops.conv2d_group_splits(count, NB, H, W, cin, cout, ksize, nws) if nws > 0 else 1
            if ksize == 1 or NB == 0:
                assert S == 1
            for i in range(count):
                if NB == 0:
                    assert got[i].shape[0] == 0
                    continue
                ref = _per_problem_ws(xs[i], wps[i], bs[i], cout, ksize, S)
                assert torch.equal(got[i], ref), f'split {S}: count {count} problem {i}'


def test_conv2d_group_splits_less_than_a_lone_launch():
    """The split is decided on the grouped workgroup count: three 16-RoI stages split less than one, and still split."""
    from dynamask_amd import ops
    per = 16 * 256 * 196
    s1 = ops.conv2d_group_splits(1, 16, 14, 14, 256, 256, 3, 8 * per)
    s3 = ops.conv2d_group_splits(3, 16, 14, 14, 256, 256, 3, 24 * per)
    assert 2 <= s3 < s1
    assert ops.conv2d_group_splits(3, 16, 14, 14, 256, 256, 3, 0) == 1
    assert ops.conv2d_group_splits(3, 16, 14, 14, 256, 256, 1, 24 * per) == 1


@pytest.mark.parametrize('NB', [0, 1, 5, 16])
def test_deconv2x2_group_equals_per_problem(NB):
    from dynamask_amd import ops
    for count in (1, 2, 3):
        x0 = _rand((NB, 256, 14, 14), 40 + NB)
        xs = [x0] + [_rand((NB, 256, 14, 14), 41 + i) for i in range(count - 1)]
        wps = [ops.pack_deconv_weight(_rand((256, 256, 2, 2), 50 + i, 0.05)) for i in range(count)]
        bs = [_rand((256,), 60 + i, 0.1) for i in range(count)]
        got = ops.deconv2x2_group(xs, wps, bs, 256, relu=True)
        for i in range(count):
            if NB == 0:
                assert tuple(got[i].shape) == (0, 256, 28, 28)
                continue
            assert torch.equal(got[i], ops.deconv2x2(xs[i], wps[i], bs[i], 256, relu=True)), f'count {count} problem {i}'


def test_grouped_launches_refuse():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    xs, wps, bs = _problems(3, 2, 32, 32, 3, 8, 8, False)
    with pytest.raises(ValueError):
        ops.conv2d_group([], [], [], 32, 3)
    with pytest.raises(ValueError):
        ops.conv2d_group(xs + xs[:1], wps + wps[:1], bs + bs[:1], 32, 3)
    with pytest.raises(ValueError):
        ops.conv2d_group([xs[0], xs[1][:1]], wps[:2], bs[:2], 32, 3)
    with pytest.raises(ValueError):
        ops.conv2d_group(xs, wps, bs, 32, 5)
    with pytest.raises(ValueError, match='bf16x3'):
        w16 = ops.pack_conv_weight(_rand((32, 32, 3, 3), 3), precision='bf16x3')
        ops.conv2d_group(xs[:1], [w16], bs[:1], 32, 3)
    out = [torch.empty((2, 32, 8, 8), device='cuda')]
    args = lambda count, ks, cout, relu: (count, ops._ptr_array(xs[:1]), 2, 8, 8, 32, cout, ks, ops._ptr_array(wps[:1]),
                                          None, relu, ops._ptr_array(out), None, 0, ops._stream())
    assert lib().dm_conv2d_group_fwd(*args(0, 3, 32, 1)) != 0
    assert lib().dm_conv2d_group_fwd(*args(4, 3, 32, 1)) != 0
    assert lib().dm_conv2d_group_fwd(*args(1, 5, 32, 1)) != 0
    assert lib().dm_conv2d_group_fwd(*args(1, 3, 32, 16)) != 0          # the bf16x3 flag
    assert lib().dm_conv2d_group_fwd(*args(1, 3, 32, 32)) != 0          # an unknown flag
    assert lib().dm_conv2d_group_fwd(*args(1, 3, 34, 1)) != 0           # the 36-cout tail build has no grouped form
    assert lib().dm_deconv2x2_group_fwd(0, ops._ptr_array(xs[:1]), 2, 32, 8, 8, ops._ptr_array(wps[:1]), None, 8, 1,
                                        ops._ptr_array(out), ops._stream()) != 0


# ------------------------------------------------------------------ the stage step
def _stage_inputs(n, C, B, seed, agnostic=True):
    g = _g(seed)
    img = torch.tensor([[100.0 + 37 * b, 140.0 + 23 * b] for b in range(B)])
    bidx = torch.randint(0, B, (n,), generator=g).sort().values.float()
    xy = torch.rand(n, 2, generator=g) * 120 - 10
    wh = torch.rand(n, 2, generator=g) * 60 + 2
    rois = torch.cat([bidx[:, None], xy, xy + wh], 1)
    cls = torch.randn(n, C + 1, generator=g)
    pred = torch.randn(n, 4 if agnostic else 4 * C, generator=g) * 1.5
    if n >= 3:
        cls[::7, 3] = cls[::7, 5] = 9.0                  # ties: the first maximum
        cls[1, -1] = 50.0                                 # the background column never wins
        pred[2, 2] = 40.0                                 # wh_ratio_clip
    return rois.cuda(), cls.cuda(), pred.cuda(), img.cuda()


@pytest.mark.parametrize('agnostic', [True, False])
def test_cascade_refine_equals_decode_and_cat(agnostic):
    from dynamask_amd import ops
    C, B = 80, 3
    means, stds = (0.01, -0.02, 0.0, 0.05), (0.1, 0.1, 0.2, 0.2)
    for n in (0, 1, 37, 1000):
        rois, cls, pred, img = _stage_inputs(n, C, B, seed=n + 3, agnostic=agnostic)
        acc = torch.empty_like(cls)
        got = ops.cascade_refine(rois, cls, pred, C, img, acc, first=True, class_agnostic=agnostic, means=means, stds=stds)
        if n == 0:
            assert got.shape == (0, 5)
            continue
        label = cls[:, :-1].argmax(1)
        assert n < 3 or bool((label[::7] == 3).all())
        d = pred if agnostic else torch.gather(pred, 1, torch.stack([label * 4 + k for k in range(4)], 1))
        for b in range(B):
            rows = rois[:, 0] == b
            if not bool(rows.any()):
                continue
            h, w = img[b].tolist()
            bx, _ = ops.bbox_decode(rois[rows].contiguous(), None, d[rows].contiguous(), C, means, stds, max_shape=(h, w),
                                    class_agnostic=True)
            ref = torch.cat([rois[rows][:, [0]], bx], 1)
            assert torch.equal(got[rows], ref), f'image {b}'
        assert torch.equal(acc, 0 + cls)


def test_cascade_score_sum_order():
    """((0 + s0) + s1) + s2 in fp32, then the reference's ``/ num_stages``: bit for bit, also for -0.0 entries."""
    from dynamask_amd import ops
    n, C = 300, 80
    ss = [_rand((n, C + 1), 90 + i, 3.0) for i in range(3)]
    for s in ss:
        s[0, :5] = -0.0                                   # 0 + (-0) = +0: python's sum starts from the int 0
    acc = torch.empty_like(ss[0])
    for i, s in enumerate(ss):
        assert ops.cascade_refine(None, s, None, C, None, acc, first=i == 0, regress=False) is None
    assert torch.equal(acc, sum(ss))
    assert torch.equal(acc / 3, sum(ss) / 3)
    assert not bool(torch.signbit(acc[0, :5]).any())


# ------------------------------------------------------------------ the RoI head
def _configs(golden_dir):
    import json
    from dynamask_amd import registry
    with open(f'{golden_dir}/g21_cascade_configs.json') as f:
        return registry._to_cfgdict(json.load(f))['coco']


def _roi_head(golden_dir):
    import cascade_inputs as ci
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _configs(golden_dir)
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=registry._to_cfgdict(dict(ci.TEST_CFG)))
    torch.manual_seed(0)
    m = registry.build_head(rh)
    sd = {k: v.shape for k, v in m.state_dict().items() if k.startswith(('bbox_head.', 'mask_head.'))}
    m.load_state_dict(ci.head_state(sd), strict=False)
    return m.cuda().eval()


def _cuda(x):
    return [f.cuda() for f in x]


def _flat(bbox_res, segm_res):
    dets = np.concatenate([b for b in bbox_res], 0)
    labels = np.array([c for c, b in enumerate(bbox_res) for _ in range(len(b))], np.int64)
    bits = np.stack([np.asarray(m, bool) for c in segm_res for m in c]) if len(labels) else None
    return dets, labels, bits


def _bits(z, key):
    shape = tuple(z[key + '_bits_shape'])
    return np.unpackbits(z[key + '_bits'], axis=-1)[..., :shape[-1]].astype(bool)


def _assert_against_golden(z, key, bbox_res, segm_res, probs, boxes):
    from dynamask_amd import ops
    from tolerances import assert_grad_close
    dets, labels, bits = _flat(bbox_res, segm_res)
    assert np.array_equal(labels, z[f'{key}_labels']), f'{key}: labels'
    assert_grad_close(dets, z[f'{key}_dets'], f'{key} dets', rel=1e-4)
    assert_grad_close(probs, z[f'{key}_probs'], f'{key} merged probabilities', rel=1e-4)
    ref = _bits(z, key)
    assert bits.shape == ref.shape
    diff = bits != ref
    if diff.any():
        # pixels may differ only where the pasted probability is within 1e-3 of the threshold
        p = torch.from_numpy(probs).cuda()[:, None].contiguous()
        lo = ops.paste_masks(p, boxes, ref.shape[1], ref.shape[2], 0.5 - 1e-3, apply_sigmoid=False).cpu().numpy()
        hi = ops.paste_masks(p, boxes, ref.shape[1], ref.shape[2], 0.5 + 1e-3, apply_sigmoid=False).cpu().numpy()
        bad = diff & ~(lo.astype(bool) != hi.astype(bool))
        assert not bad.any(), f'{key}: {int(bad.sum())} bitmap pixels differ away from the threshold'
    print(f'{key}: {int(diff.sum())} of {diff.size} pixels differ (all at the threshold)')


def _class_major(det, lab):
    """The detections in the order of the per-class lists (class-major, detection order within a class)."""
    order = torch.from_numpy(np.argsort(lab.cpu().numpy(), kind='stable')).cuda()
    return det[order].contiguous(), lab[order].contiguous()


def test_simple_test_matches_the_reference(golden_dir):
    import cascade_inputs as ci
    z = np.load(f'{golden_dir}/g21_cascade.npz')
    m = _roi_head(golden_dir)
    x, props, metas = ci.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        bbox_res, segm_res = m.simple_test(x, [props], metas)
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        det, lab = _class_major(det, lab)
        probs = m.simple_test_mask_logits(x, det, lab)
    dets, labels, _ = _flat(bbox_res, segm_res)
    assert np.array_equal(dets, det.cpu().numpy())
    _assert_against_golden(z, 'simple', bbox_res, segm_res, probs[:, 0].cpu().numpy(), det[:, :4].contiguous())


def test_aug_test_matches_the_reference(golden_dir):
    import cascade_inputs as ci
    z = np.load(f'{golden_dir}/g21_cascade.npz')
    m = _roi_head(golden_dir)
    xs, props, metas = ci.aug_inputs()
    xs, props = [_cuda(x) for x in xs], props.cuda()
    with torch.no_grad():
        bbox_res, segm_res = m.aug_test(xs, [props], metas, rescale=True)
        det, lab = m.aug_test_bboxes(xs, metas, [props], m.test_cfg)
        det, lab = _class_major(det, lab)
        probs = m.aug_test_mask_probs(xs, metas, det, lab)
        bbox_nr, _ = m.aug_test(xs, [props], metas, rescale=False)
    for a, b in zip(bbox_nr, bbox_res):
        assert np.array_equal(a, b)                  # the reference's cascade aug_test ignores rescale for the boxes
    _assert_against_golden(z, 'aug', bbox_res, segm_res, probs[:, 0].cpu().numpy(), det[:, :4].contiguous())


def test_flip_meta_unflips_the_stage_masks(golden_dir):
    """Quirk Q16: simple_test with a flip=True meta mirrors every stage's mask, as the reference's merge_aug_masks call."""
    import cascade_inputs as ci
    m = _roi_head(golden_dir)
    x, props, metas = ci.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        m._merge_metas = [dict(metas[0], flip=True, flip_direction='horizontal')]
        flipped, _ = m._mask_test_pred(x, [det], [lab], [det])
        m._merge_metas = None
        plain = m.simple_test_mask_logits(x, det, lab)
    assert torch.equal(flipped, torch.flip(plain, [3]))


def _proposals(n, seed, h, w):
    import cascade_inputs as ci
    return ci.proposals(seed=seed, h=h, w=w, n=n).cuda()


def test_batch_equals_simple_test(golden_dir):
    """Three images of different shapes (one without proposals) in one cascade: per image, boxes and labels bit for bit
    and the bitmaps equal to simple_test's."""
    import cascade_inputs as ci
    from dynamask_amd import synth
    m = _roi_head(golden_dir)
    shapes = [(128, 160), (96, 120), (112, 144)]
    H, W = 128, 160
    xb = synth.make_fpn(3, H, W, 256, seed=77)
    xb = [t.cuda() for t in xb]
    props = [_proposals(40, 500 + b, h, w) for b, (h, w) in enumerate(shapes)]
    props[1] = props[1][:0]
    metas = [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False,
                  flip_direction=None) for h, w in shapes]
    props[2] = torch.cat([props[2], torch.tensor([[100.0, 90.0, 160.0, 128.0]], device='cuda')])   # past image 2's edge
    with torch.no_grad():
        batch = m.batch_simple_test(xb, props, metas)
        for b in range(3):
            x1 = [t[b:b + 1].contiguous() for t in xb]
            bbox_s, segm_s = m.simple_test(x1, [props[b]], [metas[b]])
            bbox_b, segm_b = batch[b]
            assert len(bbox_b) == len(bbox_s) == 80
            for c in range(80):
                assert np.array_equal(bbox_b[c], bbox_s[c]), f'image {b} class {c}'
                assert len(segm_b[c]) == len(segm_s[c])
                for p, q in zip(segm_b[c], segm_s[c]):
                    assert np.array_equal(p, q)
            if b == 1:
                assert sum(len(c) for c in bbox_b) == 0
            else:
                dets = np.concatenate(bbox_b)
                h, w = shapes[b]
                assert dets.shape[0] > 0 and dets[:, [0, 2]].max() <= w and dets[:, [1, 3]].max() <= h


def test_grouped_and_per_stage_paths_agree(golden_dir):
    import cascade_inputs as ci
    from dynamask_amd import ops
    m = _roi_head(golden_dir)
    x, props, metas = ci.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
    was_g, was_s = ops.CASCADE_GROUPED[0], ops.CONV_SPLITK[0]
    try:
        out = {}
        for split in (False, True):
            for grouped in (True, False):
                ops.CONV_SPLITK[0], ops.CASCADE_GROUPED[0] = split, grouped
                with torch.no_grad():
                    for k in (1, 16, det.shape[0]):
                        out[(split, grouped, k)] = m.simple_test_mask_logits(x, det[:k], lab[:k])
    finally:
        ops.CASCADE_GROUPED[0], ops.CONV_SPLITK[0] = was_g, was_s
    for k in (1, 16, int(det.shape[0])):
        assert torch.equal(out[(False, True, k)], out[(False, False, k)]), f'{k} detections, no split'
        torch.testing.assert_close(out[(True, True, k)], out[(True, False, k)], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out[(True, True, k)], out[(False, True, k)], rtol=1e-5, atol=1e-6)


def test_bf16x3_takes_the_per_stage_path(golden_dir):
    import cascade_inputs as ci
    from dynamask_amd import ops, precision
    m = _roi_head(golden_dir)
    x, props, metas = ci.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        exact = m.simple_test_mask_logits(x, det, lab)
        precision.set_conv_precision('bf16x3')
        try:
            assert not m._grouped_ok()
            split = m.simple_test_mask_logits(x, det, lab)
        finally:
            precision.set_conv_precision('fp32')
    torch.testing.assert_close(split, exact, rtol=1e-4, atol=1e-5)


def test_zero_proposals_and_zero_detections(golden_dir):
    import cascade_inputs as ci
    m = _roi_head(golden_dir)
    x, props, metas = ci.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        bbox_res, segm_res = m.simple_test(x, [props[:0]], metas)
        assert [b.shape for b in bbox_res] == [(0, 5)] * 80 and segm_res == [[] for _ in range(80)]
        m.test_cfg.score_thr = 1.1                 # nothing passes
        bbox_res, segm_res = m.simple_test(x, [props], metas)
        assert [b.shape for b in bbox_res] == [(0, 5)] * 80 and segm_res == [[] for _ in range(80)]
        xs, props_a, metas_a = ci.aug_inputs()
        bbox_res, segm_res = m.aug_test([_cuda(v) for v in xs], [props_a.cuda()], metas_a)
        assert [b.shape for b in bbox_res] == [(0, 5)] * 80 and segm_res == [[] for _ in range(80)]
