"""Double-Head R-CNN inference on the MI355X: the rescaled RoIAlign (levels from the unscaled box) and the global average
pool against float64 through the triangle of tests/tolerances.py, the head's five convolution shapes at 7 x 7 on the
existing exact-fp32 entry points at every build the 1000-RoI call takes (tests/test_double_cpu.py holds the RoI counts to the
launcher's report), and DoubleConvFCBBoxHead / DoubleHeadRoIHead through the registry against the reference
(tests/golden/g24_double.npz: the reference's own float32 and float64 runs).  Every kernel output is written between two
canary guard bands that must survive."""
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
SCALES = [1.0 / 4, 1.0 / 8, 1.0 / 16, 1.0 / 32]


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


def _rois(boxes):
    return torch.cat([boxes.new_zeros(len(boxes), 1), boxes], 1).contiguous()


# ------------------------------------------------------------------------------------------------ RoIAlign with a factor
@pytest.mark.parametrize('C', (16, 256))
def test_roi_align_with_a_factor(C):
    import double_inputs as di
    from dynamask_amd import ops
    from dynamask_amd.roi_extractors import BaseRoIExtractor
    from oracle import ref_ops
    feats_h = [f[:, :C].contiguous() for f in di.fpn_feats()]
    feats = [f.cuda() for f in feats_h]
    rois_h = _rois(di.proposals())
    rois = rois_h.cuda()
    n = len(rois_h)
    plain, plain_lv = ops.roi_align(feats, rois, 7, SCALES, 0, float(di.FINEST_SCALE), return_levels=True)
    want_lv = ref_ops.map_roi_levels(rois_h, 4, di.FINEST_SCALE)
    assert torch.equal(plain_lv.cpu().long(), want_lv) and set(want_lv.tolist()) == {0, 1}       # (a 256 x 192 image: sqrt(w h) < 224)

    # factor 1.0: the plain extraction's bits
    one = Guarded((n, C, 7, 7))
    got1, lv1 = ops.roi_align(feats, rois, 7, SCALES, 0, float(di.FINEST_SCALE), return_levels=True, roi_scale_factor=1.0,
                              out=one.t)
    one.check('factor 1.0')
    assert torch.equal(got1, plain) and torch.equal(lv1, plain_lv)

    # factor 1.3: levels of the unscaled boxes; per RoI the bits of the single-level call with the host-rescaled box
    f = di.REG_ROI_SCALE_FACTOR
    out = Guarded((n, C, 7, 7))
    got, lv = ops.roi_align(feats, rois, 7, SCALES, 0, float(di.FINEST_SCALE), return_levels=True, roi_scale_factor=f,
                            out=out.t)
    out.check('factor 1.3')
    assert got.data_ptr() == out.t.data_ptr()
    assert torch.equal(lv.cpu().long(), want_lv)
    scaled_h = BaseRoIExtractor.roi_rescale(rois_h, f).contiguous()
    r32, r64 = torch.zeros(n, C, 7, 7), torch.zeros(n, C, 7, 7, dtype=torch.float64)
    for level in range(4):
        rows = (want_lv == level).nonzero()[:, 0]
        if len(rows) == 0:
            continue
        single = ops.roi_align([feats[level]], scaled_h[rows].contiguous().cuda(), 7, [SCALES[level]], 0)
        assert torch.equal(got[rows.cuda()], single), f'level {level}'
        r32[rows] = ref_ops.roi_align(feats_h[level], scaled_h[rows], 7, SCALES[level], 0, True)
        r64[rows] = ref_ops.roi_align(feats_h[level].double(), scaled_h[rows], 7, SCALES[level], 0, True)
    assert_close_via_f64(got, r32, r64, f'rescaled RoIAlign, {C} channels')
    assert not torch.equal(got, plain)

    # the wrong order (levels after the rescale) gives other features for the level-changing boxes
    wrong, wrong_lv = ops.roi_align(feats, scaled_h.cuda(), 7, SCALES, 0, float(di.FINEST_SCALE), return_levels=True)
    for name in di.LEVEL_CHANGING:
        i = di.hand_index(name)
        assert int(wrong_lv[i]) == int(lv[i]) + 1, name
        assert not torch.equal(got[i], wrong[i]), name
    same = [i for i in range(n) if int(wrong_lv[i]) == int(lv[i])]
    assert same and torch.equal(got[same], wrong[same])

    # a RoI's bits do not depend on the others; two runs agree
    assert torch.equal(ops.roi_align(feats, rois[3:4].contiguous(), 7, SCALES, 0, float(di.FINEST_SCALE), roi_scale_factor=f), got[3:4])
    assert torch.equal(ops.roi_align(feats, rois, 7, SCALES, 0, float(di.FINEST_SCALE), roi_scale_factor=f), got)


def test_single_level_extractor_ignores_the_factor():
    """single_level_roi_extractor.py:64-67: with one feature level the reference returns before it rescales."""
    import double_inputs as di
    from dynamask_amd import roi_extractors
    ext = roi_extractors.SingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                                            featmap_strides=[4])
    feats = [di.fpn_feats()[0].cuda()]
    rois = _rois(di.proposals()).cuda()
    assert torch.equal(ext(feats, rois, roi_scale_factor=1.3), ext(feats, rois))
    four = roi_extractors.SingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256,
                                             featmap_strides=[4, 8, 16, 32])
    feats4 = [f.cuda() for f in di.fpn_feats()]
    assert not torch.equal(four(feats4, rois, roi_scale_factor=1.3), four(feats4, rois))


def test_roi_align_factor_edges():
    import double_inputs as di
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    feats = [f[:, :16].contiguous().cuda() for f in di.fpn_feats()]
    rois = _rois(di.proposals()).cuda()
    empty = ops.roi_align(feats, rois[:0].contiguous(), 7, SCALES, 0, 56.0, roi_scale_factor=1.3)
    assert tuple(empty.shape) == (0, 16, 7, 7)
    for bad in (0.0, -1.3, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ops.roi_align(feats, rois, 7, SCALES, 0, 56.0, roi_scale_factor=bad)
    with pytest.raises(TypeError):
        ops.roi_align(feats, rois, 7, SCALES, 0, 56.0, roi_scale_factor='1.3')
    # the library itself refuses the factor before it launches anything
    out = Guarded((len(rois), 16, 7, 7))
    for bad in (0.0, -1.3):
        rc = lib().dm_roi_align_scaled_fwd(ops._ptr_array(feats), ops._int_array([f.shape[2] for f in feats]),
                                           ops._int_array([f.shape[3] for f in feats]), ops._float_array(SCALES), 4, 1, 16,
                                           ops._p(rois), len(rois), 7, 0, 56.0, bad, ops._p(out.t), None, ops._stream())
        assert rc == -1, bad          # DM_ERR_INVALID_ARG
    out.check('refused factor')
    assert bool((out.t == CANARY).all())


# ------------------------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize('N,C,H,W', [(1, 1, 1, 1), (3, 1024, 7, 7), (2, 5, 3, 2), (0, 1024, 7, 7)])
def test_global_avg_pool(N, C, H, W):
    from dynamask_amd import ops
    x = torch.randn(N, C, H, W, generator=_g(N + C + H + W)) * 2.0 + 0.5
    xd = Guarded(x.shape, x)
    assert ops.global_avg_pool_supported(xd.t)
    out = Guarded((N, C))
    got = ops.global_avg_pool(xd.t, out=out.t)
    out.check('global_avg_pool')
    xd.check('global_avg_pool input')
    assert got.data_ptr() == out.t.data_ptr() and tuple(got.shape) == (N, C)
    assert torch.equal(xd.t.cpu(), x), 'the input was modified'
    if N == 0:
        return
    assert_close_via_f64(got, x.mean((2, 3)), x.double().mean((2, 3)), f'global_avg_pool {N}x{C}x{H}x{W}')
    assert torch.equal(got, ops.global_avg_pool(x.cuda()))
    for i in range(N):          # row i of the batch has the bits of that sample alone
        assert torch.equal(ops.global_avg_pool(x[i:i + 1].cuda()), got[i:i + 1])


def test_global_avg_pool_refusals():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    L = lib()
    assert L.dm_global_avg_pool_supported(0, 1024, 49) == 1 and L.dm_global_avg_pool_supported(1000, 1024, 49) == 1
    for bad in ((-1, 4, 49), (2, 0, 49), (2, 4, 0), (2, 4, (1 << 24) + 1), (1 << 20, 1 << 12, 49)):
        assert L.dm_global_avg_pool_supported(*bad) == 0, bad
    with pytest.raises(ValueError):
        ops.global_avg_pool(torch.zeros(2, 4, 7, device='cuda'))
    with pytest.raises(ValueError):
        ops.global_avg_pool(torch.zeros(2, 4, 7, 7, device='cuda')[:, :, :, ::2])


# ------------------------------------------------------------------------------------------------ the five conv shapes
def _conv_cases():
    import double_inputs as di
    return [(name, nb) for name in di.CONV_SHAPES for nb in di.CONV_TEST_NBS[name]]


@pytest.mark.parametrize('name,nb', _conv_cases())
def test_conv_shapes_of_the_head(name, nb):
    """The launches of BasicResBlock and Bottleneck on ops.conv2d (exact fp32), each at 3 RoIs and at the smallest RoI
    count of every further build its 1000-RoI call takes, against float64 F.conv2d."""
    import double_inputs as di
    from dynamask_amd import ops
    src, cout, k, acc = di.CONV_SHAPES[name]
    g = _g(nb + cout + k + len(src))
    xs = [torch.randn(nb, c, 7, 7, generator=g) for c in src]
    cin = sum(src)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    wq = ops.pack_conv_weight(w.cuda(), src_channels=list(src))
    assert ops.conv_layout(wq) == 'fp32'
    x = torch.cat(xs, 1)
    dest = torch.randn(nb, cout, 7, 7, generator=g) * 1.5 if acc else None

    def ref(dtype):
        y = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=k // 2)
        return F.relu(y + dest.to(dtype)) if acc else F.relu(y)
    out = Guarded((nb, cout, 7, 7), dest)
    got = ops.conv2d([t.cuda() for t in xs], wq, b.cuda(), cout, k, relu=True, out=out.t, accumulate=acc)
    out.check(name)
    assert got.data_ptr() == out.t.data_ptr()
    r64 = ref(torch.float64)
    if acc:
        # values of both signs on both sides: the ReLU after the sum is neither relu(conv) + dest nor conv + relu(dest)
        y64 = F.conv2d(x.double(), w.double(), b.double())
        assert float((F.relu(y64) + dest.double() - r64).abs().max()) > 0.5
        assert float((y64 + F.relu(dest.double()) - r64).abs().max()) > 0.5
        assert bool(((dest < 0) & (r64 > 0)).any()) and bool(((dest > 0) & (r64 == 0)).any())
    assert_close_via_f64(got, ref(torch.float32), r64, f'{name} at {nb} RoIs')
    if nb > 3:
        # one association of the K sum in every build (no split-K on this path): a RoI's bits do not depend on how many
        # RoIs the call has, which is what lets batch_simple_test give simple_test's bits at any proposal count
        few = ops.conv2d([t[:3].contiguous().cuda() for t in xs], wq, b.cuda(), cout, k, relu=True,
                         out=dest[:3].contiguous().cuda() if acc else None, accumulate=acc)
        assert torch.equal(few, got[:3]), 'the first RoIs of the large call differ from the 3-RoI call'


# ------------------------------------------------------------------------------------------------ head and RoI head
@pytest.fixture(scope='module')
def double(golden_dir):
    """(DoubleHeadRoIHead on the device with the fixture's seeded weights, the fixture, double_inputs, the config)."""
    import double_inputs as di
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    z = np.load(os.path.join(golden_dir, 'g24_double.npz'))
    with open(os.path.join(golden_dir, 'g24_double_configs.json')) as f:
        cfg = registry._to_cfgdict(json.load(f)['dh_r50_1x'])
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=None, test_cfg=cfg.test_cfg.rcnn)
    m = registry.build_head(rh)
    b = m.bbox_head
    b.load_state_dict(di.head_state({k: v.shape for k, v in b.state_dict().items()}, int(z['weight_seed'])), strict=True)
    return m.cuda().eval(), z, di, cfg


def _class_major(bbox_results):
    dets = np.asarray([row for b in bbox_results for row in b], np.float32).reshape(-1, 5)
    return dets, np.asarray([c for c, b in enumerate(bbox_results) for _ in range(len(b))], np.int64)


def test_bbox_head_forward_against_the_reference(double):
    from dynamask_amd import conv_precision
    m, z, di, _ = double
    feats = [f.cuda() for f in di.fpn_feats()]
    rois = _rois(di.proposals()).cuda()
    nh = len(di.HAND_BOXES)
    ext = m.bbox_roi_extractor
    with torch.no_grad():
        x_cls = ext(feats, rois)
        x_reg = ext(feats, rois, roi_scale_factor=m.reg_roi_scale_factor)
        keep = x_reg.clone()
        cls_score, bbox_pred = m.bbox_head(x_cls, x_reg)
        again = m.bbox_head(x_cls, x_reg)
        with conv_precision('bf16x3'):
            mode = m.bbox_head(x_cls, x_reg)
    assert torch.equal(x_reg, keep), 'the in-place bottlenecks wrote into the RoI features'
    assert_close_via_f64(x_cls[:nh].sum((2, 3)), z['cls_feat_sums'], z['cls_feat_sums64'], 'cls RoI features')
    assert_close_via_f64(x_reg[:nh].sum((2, 3)), z['reg_feat_sums'], z['reg_feat_sums64'], 'reg RoI features')
    assert tuple(cls_score.shape) == (len(rois), 81) and tuple(bbox_pred.shape) == (len(rois), 320)
    e = assert_close_via_f64(cls_score, z['cls_score'], z['cls_score64'], 'cls_score')
    print('cls_score: err %.3g, reference err %.3g, scale %.3g' % e)
    e = assert_close_via_f64(bbox_pred, z['bbox_pred'], z['bbox_pred64'], 'bbox_pred')
    print('bbox_pred: err %.3g, reference err %.3g, scale %.3g' % e)
    assert torch.equal(again[0], cls_score) and torch.equal(again[1], bbox_pred), 'two identical calls differ'
    assert torch.equal(mode[0], cls_score) and torch.equal(mode[1], bbox_pred), 'the bf16x3 mode changed a bit'


def test_bbox_forward_of_the_roi_head(double):
    m, z, di, _ = double
    feats = [f.cuda() for f in di.fpn_feats()]
    rois = _rois(di.proposals()).cuda()
    with torch.no_grad():
        res = m._bbox_forward(feats, rois)
        plain = m.bbox_roi_extractor(feats, rois)
    assert set(res) == {'cls_score', 'bbox_pred', 'bbox_feats'}
    n = len(rois)
    assert tuple(res['cls_score'].shape) == (n, 81) and tuple(res['bbox_pred'].shape) == (n, 320)
    assert tuple(res['bbox_feats'].shape) == (n, 256, 7, 7) and torch.equal(res['bbox_feats'], plain)
    assert_close_via_f64(res['bbox_pred'], z['bbox_pred'], z['bbox_pred64'], 'bbox_pred')


@pytest.mark.parametrize('tag,rescale', [('plain', False), ('rescale', True)])
def test_simple_test_against_the_reference(double, tag, rescale):
    m, z, di, _ = double
    feats = [f.cuda() for f in di.fpn_feats()]
    props = di.proposals().cuda()
    metas = di.img_metas(di.SCALE_FACTOR if rescale else 1.0)
    res = m.simple_test(feats, [props], metas, rescale=rescale)
    assert isinstance(res, list) and len(res) == 80 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res)
    dets, labels = _class_major(res)
    assert len(labels) == len(z[f'{tag}_labels']) and np.array_equal(labels, z[f'{tag}_labels'])
    assert_close_via_f64(dets, z[f'{tag}_dets'], z[f'{tag}_dets64'], f'simple_test rescale={rescale}')
    again = m.simple_test(feats, [props], metas, rescale=rescale)
    assert all(np.array_equal(a, b) for a, b in zip(res, again)), 'two identical calls differ'


def test_zero_proposals(double):
    m, z, di, _ = double
    feats = [f.cuda() for f in di.fpn_feats()]
    none = di.proposals()[:0].cuda()
    res = m.simple_test(feats, [none], di.img_metas())
    assert len(res) == 80 and all(a.shape == (0, 5) and a.dtype == np.float32 for a in res)
    batch = m.batch_simple_test([f.repeat(2, 1, 1, 1) for f in feats], [none, none], di.img_metas() * 2)
    assert len(batch) == 2 and all(a.shape == (0, 5) for r in batch for a in r)
    with torch.no_grad():
        r = m._bbox_forward(feats, none.new_zeros((0, 5)))
    assert tuple(r['cls_score'].shape) == (0, 81) and tuple(r['bbox_pred'].shape) == (0, 320)


def test_batch_equals_one_image_calls(double):
    m, z, di, _ = double
    x2 = [f.cuda() for f in di.fpn_feats(batch=2)]
    props = [di.proposals().cuda(), di.proposals(seed=99, n=13).cuda()]
    for rescale in (False, True):
        metas = di.img_metas(di.SCALE_FACTOR if rescale else 1.0) * 2
        batch = m.batch_simple_test(x2, props, metas, rescale=rescale)
        assert len(batch) == 2
        for b in range(2):
            xb = [f[b:b + 1].contiguous() for f in x2]
            one = m.simple_test(xb, [props[b]], [metas[b]], rescale=rescale)
            assert sum(len(c) for c in one) > 0
            assert all(np.array_equal(p, q) for p, q in zip(batch[b], one)), f'image {b} rescale={rescale}'
    _, labels = _class_major(batch[0])          # image 0 of the batch is the fixture's image
    assert np.array_equal(labels, z['rescale_labels'])


def test_aug_test_of_one_plain_view_is_simple_test(double):
    m, z, di, _ = double
    feats = [f.cuda() for f in di.fpn_feats()]
    props = di.proposals().cuda()
    metas = di.img_metas(1.0)
    one = m.simple_test(feats, [props], metas, rescale=True)
    aug = m.aug_test([feats], [props], [metas], rescale=True)
    assert isinstance(aug, list) and len(aug) == 80
    assert all(np.array_equal(p, q) for p, q in zip(aug, one))
    assert np.array_equal(_class_major(aug)[1], z['plain_labels'])


def test_a_configured_mask_branch_is_the_templates(double):
    """FCNMaskHead + a mask extractor added to the config: ``simple_test_mask`` on given detections is StandardRoIHead's
    with the same mask weights, bit for bit, and ``simple_test`` returns (bbox_results, segm_results)."""
    from dynamask_amd import registry, synth
    m, z, di, cfg = double
    mask_cfg = dict(mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
                    mask_head=dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG))
    test_cfg = registry._to_cfgdict(dict(cfg.test_cfg.rcnn, mask_thr_binary=0.5))
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=None, test_cfg=test_cfg, **mask_cfg)
    torch.manual_seed(5)
    dm = registry.build_head(rh)
    assert dm.with_mask
    dm.bbox_head.load_state_dict(m.bbox_head.state_dict(), strict=True)
    std = registry.build_head(dict(type='StandardRoIHead', train_cfg=None, test_cfg=test_cfg,
                                   bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
                                   bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG), **mask_cfg))
    std.mask_head.load_state_dict(dm.mask_head.state_dict(), strict=True)
    dm, std = dm.cuda().eval(), std.cuda().eval()
    feats = [f.cuda() for f in di.fpn_feats()]
    boxes = di.hand_boxes()
    det_bboxes = torch.cat([boxes, torch.linspace(0.9, 0.3, len(boxes))[:, None]], 1).cuda()
    det_labels = torch.tensor([3, 0, 17, 3, 79, 42, 0]).cuda()
    metas = di.img_metas(1.0)
    a = dm.simple_test_mask(feats, metas, det_bboxes, det_labels)
    b = std.simple_test_mask(feats, metas, det_bboxes, det_labels)
    assert len(a) == len(b) == 80 and sum(len(c) for c in a) == len(boxes)
    for ca, cb in zip(a, b):
        assert len(ca) == len(cb) and all(np.array_equal(p, q) for p, q in zip(ca, cb))
    assert any(p.any() for c in a for p in c)
    bbox_results, segm_results = dm.simple_test(feats, [di.proposals().cuda()], metas)
    assert np.array_equal(_class_major(bbox_results)[1], z['plain_labels'])
    assert [len(c) for c in segm_results] == [len(c) for c in bbox_results]
