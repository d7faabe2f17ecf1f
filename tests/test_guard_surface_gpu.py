"""The memory-safety net over the whole launching surface of include/dynamask_hip.h.

Every pass builds its modules first, then runs inside ``guard_arena.guarded`` + ``guard_arena.LaunchLog``: every device
tensor the package allocates -- outputs, scratch, workspaces, intermediates, the inputs handed over -- sits between two
NaN-patterned guard bands.  A pass asserts that the bands are intact (no store past either end of any buffer) and that
every floating result is finite (no out-of-range read reached a result), and hands its launch log to the coverage test,
which holds it to the tables of guard_arena.py: ``EXPECTED_REACHED`` per pass, ``UNGUARDED_STORES`` over all passes.

Shapes are the smallest ragged ones: images 67 x 131 and 2 x 37 x 53 for the backbones, necks and RPN (stage maps 34 x 66
... 3 x 5: odd widths, 66 columns cross two 32-column tiles); a 200 x 333 pyramid (50 x 84 ... 4 x 6) with 1, 7 and 193
proposals for the RoI heads (193: the first count past the 192 at which RoIAlign orders its RoIs); u8 images of 75 x 131
and 101 x 60 for the detectors.  Each pass runs once per session, whatever the order or selection of the tests."""
import copy
import json
import os
import time
import types

import numpy as np
import pytest
import torch

import guard_arena as ga
from guard_arena import _finite, _put, guarded

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
H, W = 200, 333                     # the RoI heads' image: levels 50 x 84, 25 x 42, 13 x 21, 7 x 11, 4 x 6
H2, W2 = 136, 200                   # the second image of the batched call
COUNTS = (1, 7, 193)
ODD_DETS = 37


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _meta(h, w, scale_factor=1.0, ori=None, flip=False, pad=None):
    return dict(img_shape=(h, w, 3), ori_shape=ori or (h, w, 3), pad_shape=pad or (h, w, 3), scale_factor=scale_factor,
                flip=flip, flip_direction='horizontal' if flip else None)


def _leaves(r):
    """The tensors and arrays of a nested result."""
    if isinstance(r, torch.Tensor):
        yield r
    elif isinstance(r, np.ndarray):
        if r.dtype.kind == 'f':
            yield torch.from_numpy(np.ascontiguousarray(r))
    elif isinstance(r, dict):
        for v in r.values():
            yield from _leaves(v)
    elif isinstance(r, (list, tuple)):
        for v in r:
            yield from _leaves(v)


def _generic_state(shapes, seed):
    """Seeded state for the parts no fixture module draws: He-scaled weights, norm weights around 1, small biases and
    running means, running variances in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros(shape, dtype=torch.long)
        elif k.endswith('running_var'):
            out[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith('.weight') and len(shape) == 1:
            out[k] = (0.5 if '.bn3.' in k or '.downsample.1.' in k else 1.0) + 0.05 * torch.randn(shape, generator=g)
        elif len(shape) > 1:
            out[k] = torch.randn(shape, generator=g) * (2.0 / max(int(np.prod(shape[1:])), 1)) ** 0.5
        else:
            out[k] = 0.1 * torch.randn(shape, generator=g)
    return out


def _shapes(m, prefixes=None):
    return {k: v.shape for k, v in m.state_dict().items() if prefixes is None or k.startswith(prefixes)}


# ------------------------------------------------------------------------------------------------ backbones
def _backbones():
    """name -> the net on the device with its fixture module's seeded weights."""
    import backbone_inputs as bi
    import res2net_inputs as ri
    import resnext_inputs as xi
    from dynamask_amd import backbones, registry  # noqa: F401
    g28, g30, g31 = _json('g28_backbone_configs.json'), _json(xi.CONFIGS), _json(ri.CONFIGS)
    caffe64 = dict(type='ResNeXt', depth=50, groups=64, base_width=4, style='caffe', num_stages=3, strides=(1, 2, 2),
                   dilations=(1, 1, 1), out_indices=(2,), frozen_stages=-1)            # test_resnext_gpu.py CAFFE
    cfgs = {'r50_pytorch': (g28['pytorch']['model']['backbone'], bi.head_state, bi.WEIGHT_SEED),
            'r50_caffe_c4': (g28['caffe_c4']['model']['backbone'], bi.head_state, bi.WEIGHT_SEED),
            'x101_32x4d': (g30['x101_32x4d']['model']['backbone'], xi.head_state, xi.WEIGHT_SEED),
            'x50_caffe_64x4d': (caffe64, xi.head_state, xi.WEIGHT_SEED),
            'r2_101': (g31[ri.RUN]['model']['backbone'], ri.head_state, ri.WEIGHT_SEED)}
    nets = {}
    for name, (cfg, draw, seed) in cfgs.items():
        m = registry.build_backbone(copy.deepcopy(dict(cfg)))
        m.load_state_dict(draw(_shapes(m), seed), strict=True)
        nets[name] = m.cuda().eval()
    return nets


def _images():
    import backbone_inputs as bi
    return [bi.inputs(1, 67, 131, seed=67131), bi.inputs(2, 37, 53)]


def pass_backbones():
    nets = _backbones()

    def run(arena):
        imgs = [_put(arena, i) for i in _images()]
        out = []
        with torch.no_grad():
            for name, m in nets.items():
                for img in imgs:
                    out.append(m(img))
        assert [tuple(o.shape[2:]) for o in out[0]] == [(17, 33), (9, 17), (5, 9), (3, 5)]
        return out
    return run


# ------------------------------------------------------------------------------------------------ necks and RPN
def pass_necks_rpn():
    import backbone_inputs as bi
    import fpn_carafe_inputs as ci
    import fpn_inputs as fi
    import rpn_inputs as ri
    from dynamask_amd import backbones, dense_heads, necks, registry  # noqa: F401
    g28, g27, g32, g26 = (_json('g28_backbone_configs.json'), _json('g27_fpn_configs.json'), _json(ci.CONFIGS),
                          _json('g26_rpn_configs.json'))
    nets = {}
    for form in ('pytorch', 'caffe_c4'):
        m = registry.build_backbone(copy.deepcopy(g28[form]['model']['backbone']))
        m.load_state_dict(bi.head_state(_shapes(m), bi.WEIGHT_SEED), strict=True)
        nets[form] = m.cuda().eval()
    fpns = {}
    for form in ('mask_rcnn', 'retinanet', 'fcos'):           # no extra convolution / on_input / on_output with relu
        m = registry.build_neck(copy.deepcopy(g27[form]['model']['neck']))
        m.load_state_dict(fi.head_state(_shapes(m), fi.WEIGHT_SEED), strict=True)
        fpns[form] = m.cuda().eval()
    m = registry.build_neck(copy.deepcopy(g32[ci.NECK_ENTRY]['model']['neck']))
    m.load_state_dict(ci.head_state(_shapes(m), ci.WEIGHT_SEED), strict=True)
    fpns['carafe'] = m.cuda().eval()
    rpns = {}
    for form in ('fpn', 'c4'):
        cfg = registry._to_cfgdict(copy.deepcopy(g26[form]))
        rh = dict(cfg.model.rpn_head)
        rh.update(train_cfg=None, test_cfg=dict(cfg.test_cfg.rpn, nms_pre=64))
        m = registry.build_head(rh)
        m.load_state_dict(ri.head_state(_shapes(m), 26), strict=True)
        rpns[form] = m.cuda().eval()

    def run(arena):
        imgs = [_put(arena, i) for i in _images()]
        metas = [[_meta(67, 131)], [_meta(37, 53), _meta(37, 53)]]
        out = []
        with torch.no_grad():
            for img, meta in zip(imgs, metas):
                stages = nets['pytorch'](img)
                for form, neck in fpns.items():
                    pyramid = neck(stages)
                    out.append(pyramid)
                    if form in ('mask_rcnn', 'carafe'):
                        out.append(rpns['fpn'].simple_test_rpn(pyramid, meta))
                c4 = nets['caffe_c4'](img)
                assert len(c4) == 1
                out.append(rpns['c4'].simple_test_rpn(c4, meta))
        return out
    return run


# ------------------------------------------------------------------------------------------------ RoI heads
def _test_cfg(base, **kw):
    from dynamask_amd import registry
    return registry._to_cfgdict(dict(dict(base), score_thr=0.0, **kw))


def _build_dynamask():
    from dynamask_amd import registry, synth
    m = registry.build_head(dict(
        type='DynaMaskRoIHead', bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG), test_cfg=_test_cfg(synth.RCNN_TEST_CFG)))
    m.load_state_dict({**synth.init_dynamask_head_state(seed=5, test_mode=True), **synth.init_mask_pre_state(seed=6),
                       **synth.init_bbox_head_state(seed=8)}, strict=True)
    return m


def _build_fcn():
    import aug_inputs as ai
    from dynamask_amd import registry, synth
    m = registry.build_head(dict(
        type='StandardRoIHead', bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG), test_cfg=_test_cfg(ai.TEST_CFG)))
    m.load_state_dict(ai.head_state(), strict=True)
    return m


def _from_config(file, entry, test_cfg=None):
    """(the entry's RoI head through the registry with ``score_thr=0``, its config)."""
    from dynamask_amd import registry
    cfg = registry._to_cfgdict(copy.deepcopy(_json(file)[entry]))
    rh = dict(cfg.model.roi_head)
    train_cfg = cfg.train_cfg.rcnn if 'train_cfg' in cfg and cfg.train_cfg is not None else None
    rh.update(train_cfg=train_cfg, test_cfg=_test_cfg(test_cfg if test_cfg is not None else cfg.test_cfg.rcnn))
    torch.manual_seed(0)
    return registry.build_head(rh), cfg


def _build_refine():
    import refine_inputs as ri
    m, _ = _from_config('g17_refine_configs.json', 'coco')
    m.mask_head.load_state_dict(ri.head_state(_shapes(m.mask_head)), strict=True)
    return m


def _build_pointrend():
    import pointrend_inputs as pi
    m, _ = _from_config('g18_pointrend_configs.json', 'coco', pi.TEST_CFG)
    m.load_state_dict(pi.head_state(_shapes(m, ('mask_head.', 'point_head.'))), strict=False)
    return m


def _build_msrcnn():
    import msrcnn_inputs as mi
    m, _ = _from_config('g19_msrcnn_configs.json', 'coco', mi.TEST_CFG)
    m.load_state_dict(mi.head_state(_shapes(m, ('mask_head.', 'mask_iou_head.'))), strict=False)
    return m


def _build_pointrefine():
    import pointrefine_inputs as pi
    m, _ = _from_config('g20_pointrefine_configs.json', 'coco', pi.TEST_CFG)
    st = pi.head_state({'mask_head.' + k: v for k, v in _shapes(m.mask_head).items()})
    m.mask_head.load_state_dict({k[len('mask_head.'):]: v for k, v in st.items()}, strict=True)
    return m


def _build_cascade():
    import cascade_inputs as ci
    m, _ = _from_config('g21_cascade_configs.json', 'coco', ci.TEST_CFG)
    m.load_state_dict(ci.head_state(_shapes(m, ('bbox_head.', 'mask_head.'))), strict=False)
    return m


def _build_htc():
    import htc_inputs as hi
    m, _ = _from_config('g22_htc_configs.json', 'coco', hi.TEST_CFG)
    m.load_state_dict(hi.head_state(_shapes(m, ('bbox_head.', 'mask_head.', 'semantic_head.'))), strict=False)
    return m


def _build_grid():
    import grid_inputs as gi
    m, _ = _from_config('g23_grid_configs.json', 'r50_2x')
    m.load_state_dict(gi.head_state(_shapes(m, ('bbox_head.', 'grid_head.')), gi.WEIGHT_SEEDS[0]), strict=False)
    return m


def _build_double():
    import double_inputs as di
    m, _ = _from_config('g24_double_configs.json', 'dh_r50_1x')
    m.bbox_head.load_state_dict(di.head_state(_shapes(m.bbox_head), di.WEIGHT_SEEDS[0]), strict=True)
    return m


def _build_c4():
    import c4_inputs as ci
    m, _ = _from_config('g25_c4_configs.json', 'mask_c4')
    m.load_state_dict(ci.head_state(_shapes(m), ci.WEIGHT_SEEDS[0]), strict=False)
    return m


# family -> (builder, the channels of a single stride-16 map or None for the FPN pyramid, has aug_test)
FAMILIES = {'dynamask': (_build_dynamask, None, True), 'fcn': (_build_fcn, None, True), 'refinemask': (_build_refine, None, True),
            'pointrend': (_build_pointrend, None, True), 'msrcnn': (_build_msrcnn, None, True),
            'pointrefine': (_build_pointrefine, None, True), 'cascade': (_build_cascade, None, True),
            'htc': (_build_htc, None, True), 'grid': (_build_grid, None, False), 'double': (_build_double, None, True),
            'c4': (_build_c4, 1024, True)}


def _maps(batch, c4_channels, seed):
    from dynamask_amd import synth
    if c4_channels is None:
        return synth.make_fpn(batch, H, W, 256, seed=seed)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(batch, c4_channels, -(-H // 16), -(-W // 16), generator=g)]


def _boxes(n, h, w, seed):
    from dynamask_amd import synth
    return synth.make_rois(1, n, h, w, seed=seed, max_size=float(max(h, w)))[:, 1:].contiguous()


def _roi_pass(family):
    def make():
        build, c4, has_aug = FAMILIES[family]
        from dynamask_amd import bbox_heads, losses, mask_heads, roi_extractors, roi_head, shared_heads  # noqa: F401
        m = build().cuda().eval()

        def run(arena):
            out = []
            x = [_put(arena, f) for f in _maps(1, c4, seed=H)]
            xf = [_put(arena, f) for f in _maps(1, c4, seed=H + 1)]
            x2 = [_put(arena, f) for f in _maps(2, c4, seed=H + 2)]
            plain = [_meta(H, W)]
            sf = np.array([1.5, 1.25, 1.5, 1.25], dtype=np.float32)
            scaled = [_meta(H, W, scale_factor=sf, ori=(160, 222, 3))]
            with torch.no_grad():
                for n in COUNTS:
                    props = _put(arena, _boxes(n, H, W, seed=n))
                    out.append(m.simple_test(x, [props], plain, rescale=False, encode=n != 7))          # (7: bitmaps, not RLE)
                out.append(m.simple_test(x, [props], scaled, rescale=True, encode=True))
                keep = m.test_cfg['max_per_img']
                m.test_cfg['max_per_img'] = ODD_DETS
                try:
                    res = m.simple_test(x, [props], scaled, rescale=True, encode=True)
                finally:
                    m.test_cfg['max_per_img'] = keep
                boxes = res[0] if isinstance(res, tuple) else res
                assert sum(len(b) for b in boxes) == ODD_DETS, f'{family}: {sum(len(b) for b in boxes)} detections'
                out.append(res)
                # two images of different size in one call
                props2 = [_put(arena, _boxes(ODD_DETS, H, W, seed=2)), _put(arena, _boxes(11, H2, W2, seed=3))]
                metas2 = [_meta(H, W), _meta(H2, W2, pad=(H, W, 3))]
                out.append(m.batch_simple_test(x2, props2, metas2, rescale=False, encode=True))
                out.append(m.batch_simple_test(x2, props2, metas2, rescale=False, encode=False))          # bitmaps: one paste launch
                if has_aug:
                    props = _put(arena, _boxes(7, H, W, seed=7))
                    out.append(m.aug_test([x, xf], [props], [plain, [_meta(H, W, flip=True)]], rescale=False, encode=True))
                if family == 'dynamask':
                    from dynamask_amd import synth
                    rois = _put(arena, synth.make_rois(1, 7, H, W, seed=7))
                    labels = _put(arena, synth.make_labels(7, seed=8))
                    r = m._mask_forward(x, rois, labels)
                    out += [r['stage_instance_preds'], r['stage_detail_preds']]
                    out.append(m._mask_forward(x, rois, labels, last_stage=1)['stage_instance_preds'])
                    out.append(m.dynamic_mask_logits(x, rois[:, 1:].contiguous(), labels)['preds'])
                    out.append(m.dynamic_mask_logits(x, rois[:, 1:].contiguous(), labels, exits=(torch.arange(7) * 7 + 3) % 4)['preds'])
            return out
        return run
    return make


# ------------------------------------------------------------------------------------------------ detectors from u8
DETECTORS = [('g29_detector_configs.json', 'dynamask'), ('g29_detector_configs.json', 'mask_rcnn'),
             ('g29_detector_configs.json', 'mask_c4'), ('g30_resnext_configs.json', 'mask_rcnn_x101_32x4d'),
             ('g31_res2net_configs.json', 'mask_rcnn_r2_101'), ('g32_fpn_carafe_configs.json', 'mask_rcnn_carafe')]


def pass_detectors():
    import backbone_inputs as bi
    import fpn_carafe_inputs as ci
    import fpn_inputs as fi
    import rpn_inputs as ri
    from dynamask_amd import build_detector, detectors
    norm = _json('g29_detector_configs.json')['mask_rcnn']['img_norm_cfg']
    dets = {}
    for file, entry in DETECTORS:
        cfg = copy.deepcopy(_json(file)[entry])
        cfg['test_cfg']['rpn'].update(nms_pre=64, nms_post=32, max_num=32)          # as test_detector_gpu.py does
        cfg['test_cfg']['rcnn'].update(score_thr=0.0, max_per_img=8)
        det = build_detector(copy.deepcopy(cfg['model']), test_cfg=copy.deepcopy(cfg['test_cfg']))
        own, state = det.state_dict(), {}
        draw = dict(backbone=bi.head_state, neck=ci.head_state if 'carafe' in entry else fi.head_state, rpn_head=ri.head_state,
                    roi_head=_generic_state)
        for part, fn in draw.items():
            shapes = {k[len(part) + 1:]: v.shape for k, v in own.items() if k.startswith(part + '.')}
            if shapes:
                state.update({f'{part}.{k}': v for k, v in fn(shapes, 29).items()})
        assert set(state) == set(own), entry
        det.load_state_dict(state, strict=True)
        dets[entry] = (det.cuda().eval(), cfg.get('img_norm_cfg', norm))

    def run(arena):
        rng = np.random.default_rng(29)
        images = [_put(arena, torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8))) for h, w in ((75, 131), (101, 60))]
        out = []
        with torch.no_grad():
            for entry, (det, norm_cfg) in dets.items():
                for kw in (dict(img_scale=(160, 96)), dict(flip=True)):          # one view resized with keep_ratio, one flipped
                    img, metas = detectors.preprocess(images, norm_cfg, **kw)
                    out.append(img)
                    out.append(det.simple_test(img, metas, rescale=True, encode=True))
                if entry == 'mask_rcnn':          # both views at once: the proposals of each mapped back and merged
                    views = [detectors.preprocess(images[:1], norm_cfg, **kw) for kw in (dict(img_scale=(160, 96)), dict(flip=True))]
                    out.append(det.aug_test([v[0] for v in views], [v[1] for v in views], rescale=True))
        return out
    return run


# ------------------------------------------------------------------------------------------------ training
class _Polygons:
    """A PolygonMasks-like holder: per object a list of flat (x, y) vertex arrays."""

    def __init__(self, boxes, height, width):
        self.height, self.width, self.masks = height, width, []
        t = np.linspace(0.0, 2 * np.pi, 9)[:-1]
        for x1, y1, x2, y2 in boxes.numpy().astype(np.float64):
            cx, cy, ax, ay = (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) / 2, (y2 - y1) / 2
            self.masks.append([np.stack([cx + ax * np.cos(t), cy + ay * np.sin(t)], 1).reshape(-1)])


def pass_training():
    from dynamask_amd import bbox_heads, losses, mask_heads, ops, registry, roi_extractors, roi_head, synth  # noqa: F401
    from dynamask_amd.dist import FlatParamGroup

    def head():
        m = registry.build_head(dict(
            type='DynaMaskRoIHead', bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
            bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
            mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
            mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG),
            train_cfg=registry._to_cfgdict(synth.RCNN_TRAIN_CFG), test_cfg=None))
        m.load_state_dict({**synth.init_dynamask_head_state(seed=5), **synth.init_mask_pre_state(seed=6),
                           **synth.init_bbox_head_state(seed=8)}, strict=True)
        return m.cuda().train()
    heads = {det: head() for det in (False, True)}
    tb = synth.make_train_batch(batch=2, img_h=H, img_w=W, n_props=193, n_gt=(5, 3), seed=30)

    def run(arena):
        out = []
        keep = ops.DETERMINISTIC[0]
        try:
            for det, m in heads.items():
                ops.DETERMINISTIC[0] = det
                feats = [_put(arena, f).requires_grad_(True) for f in synth.make_fpn(2, H, W, 256, seed=H + 1)]
                props = [_put(arena, p) for p in tb['proposals']]
                # image 1 has no ground truth; image 0's masks are bitmaps in one run and polygons in the other
                gtb = [_put(arena, tb['gt_bboxes'][0]), _put(arena, torch.zeros((0, 4)))]
                gtl = [_put(arena, tb['gt_labels'][0]), _put(arena, torch.zeros((0,), dtype=torch.long))]
                none = _put(arena, torch.zeros((0, H, W), dtype=torch.uint8))
                gtm = [_Polygons(tb['gt_bboxes'][0], H, W) if det else _put(arena, tb['gt_masks'][0]), none]
                grp = FlatParamGroup(m.parameters())
                grp.zero_grad()
                torch.manual_seed(3)
                res = m.forward_train(feats, tb['img_metas'], props, gtb, gtl, None, gtm)
                assert set(res) >= {'loss_cls', 'loss_bbox', 'loss_masks'}
                sum(v for k, v in res.items() if 'loss' in k).backward()
                norm = grp.clip_grad_norm_(35.0)
                grp.scale_grads_(list(m.mask_predictor.parameters()), 0.05)
                grp.sgd_step(lr=0.02, momentum=0.9, weight_decay=1e-4)
                out += [[v.detach() for v in res.values()], norm, grp.flat_grad, grp.flat_param, [f.grad for f in feats[:4]]]
                grp.release()
        finally:
            ops.DETERMINISTIC[0] = keep
        return out
    return run


# ------------------------------------------------------------------------------------------------ leftovers
def pass_leftovers():
    """Direct ``ops`` calls for the launching entry points with a call site in the package that no module-level pass
    reaches: the accumulation forms the default flags do not take (float atomics, 64-bit fixed point), the bf16x3 weight
    packs, diagnostics and the adjoints of layers whose training is not built.  Small ragged shapes of each op's own tests."""
    from dynamask_amd import ops

    def run(arena):
        g = torch.Generator().manual_seed(99)

        def rnd(*shape, scale=1.0):
            return _put(arena, torch.randn(*shape, generator=g) * scale)

        out = []
        keep = ops.DETERMINISTIC[0], ops.CLB_SLAB[0], ops.WGRAD_SLAB[0]
        try:
            # MaskPre: batch statistics into guarded running statistics, the pooling's argmax
            x = rnd(3, 16, 14, 14)
            rm, rv = _put(arena, torch.zeros(16)), _put(arena, torch.ones(16))
            mean, var = ops.bn_stats(x, rm, rv, 0.1)
            out += [mean, var, rm, rv, ops.bn_relu_maxpool_argmax(x, mean, var, rnd(16), rnd(16))]
            # the adjoints of CARAFE and of the nearest upsampling (test_carafe_gpu.py BWD_CASES, odd W)
            out += list(ops.carafe_backward(rnd(1, 4, 3, 5), rnd(1, 100, 3, 5), rnd(1, 4, 6, 10), 5, 1, 2))
            out += [ops.upsample2x_nearest(rnd(2, 3, 5, 7)), ops.upsample2x_nearest_backward(rnd(2, 3, 10, 14))]
            # class-logit and weight gradients by float atomics and in fixed point; the fixed-point channel sum
            labels = _put(arena, torch.tensor([3, 3, 79]))
            for slab, det in ((False, False), (False, True)):
                ops.CLB_SLAB[0], ops.WGRAD_SLAB[0], ops.DETERMINISTIC[0] = slab, slab, det
                grads = [_put(arena, torch.zeros(s)) for s in ((80, 8), (80,), (80, 8), (80,))]
                gx = _put(arena, torch.ones(3, 8, 9, 9))
                ops.class_logits_backward(rnd(3, 8, 9, 9), rnd(80, 8, scale=0.1), rnd(80, 8, scale=0.1), labels, rnd(3, 1, 9, 9),
                                          rnd(3, 1, 9, 9), gx, True, grads[0], grads[1], grads[2], grads[3])
                out += grads + [gx]
                out += list(ops.conv2d_wgrad(rnd(2, 16, 7, 9), [rnd(2, 8, 7, 9)], 3, want_bias=True))
                out.append(ops.channel_sum(rnd(2, 8, 5, 7)))
            ops.DETERMINISTIC[0], ops.CLB_SLAB[0], ops.WGRAD_SLAB[0] = keep
            # the bf16x3 weight layouts
            out.append(ops.pack_conv_weight(rnd(16, 8, 3, 3), precision='bf16x3'))
            out.append(ops.pack_deconv_weight(rnd(8, 16, 2, 2), precision='bf16x3'))
            # DCN: the fused column-gradient scatter (test_bwd_gpu.py)
            out += list(ops.deform_col2im_coord(rnd(2, 144, 14, 14), rnd(2, 16, 14, 14), rnd(2, 36, 14, 14, scale=0.5), 2))
            # assigner: ignore regions
            ov = _put(arena, torch.rand(3, 37, generator=g))
            out.append(ops.ignore_columns_(ov, _put(arena, torch.rand(37, 2, generator=g)), 0.5))
            # the one-stage mask loss, the sigmoid adjoint
            t = _put(arena, (torch.rand(5, 14, 14, generator=g) > 0.5).float())
            out += list(ops.mask_loss(rnd(5, 1, 14, 14), rnd(5, 1, 14, 14), t, t, _put(arena, torch.rand(5, generator=g))))
            sig = _put(arena, torch.rand(4, 2, 9, 9, generator=g))
            out.append(ops.sigmoid_backward(sig[:, 0:1], rnd(4, 1, 9, 9), rnd(4, 1, 9, 9)))
            # bitmaps: paste on a canvas, encode the canvas
            boxes = _put(arena, _boxes(5, 33, 47, seed=5))
            canvas = ops.paste_masks(rnd(5, 1, 28, 28), boxes, 33, 47, 0.5, apply_sigmoid=True)
            rles = ops.rle_encode(canvas)
            assert len(rles) == 5
            out.append(canvas)
            # the unfused point heads' scatters
            idx = _put(arena, torch.stack([torch.randperm(81, generator=g)[:50] for _ in range(3)]).int())
            out.append(ops.point_scatter(rnd(3, 50), idx, _put(arena, torch.zeros(3, 1, 9, 9))))
            out.append(ops.point_scatter_rows(rnd(3, 8, 50), idx, _put(arena, torch.zeros(3, 8, 9, 9))))
        finally:
            ops.DETERMINISTIC[0], ops.CLB_SLAB[0], ops.WGRAD_SLAB[0] = keep
        return out
    return run


PASSES = {'backbones': pass_backbones, 'necks_rpn': pass_necks_rpn,
          **{f'roi_{f}': _roi_pass(f) for f in FAMILIES},
          'detectors': pass_detectors, 'training': pass_training, 'leftovers': pass_leftovers}

_CACHE = {}
_DEAD = []          # a pass that ended in anything but a failed assertion: nothing more is launched in this process


def run_pass(name):
    """The pass's outcome, run on first use: dict(log, blocks, launches, seconds) or the AssertionError it raised."""
    if name not in _CACHE:
        if _DEAD:
            pytest.fail(f'not run: pass {_DEAD[0]!r} ended in an error that is no assertion', pytrace=False)
        from dynamask_amd import ops
        t0 = time.perf_counter()
        mp = pytest.MonkeyPatch()
        ops._BN_SCRATCH.clear()          # the per-stream scratch an earlier test left behind: this pass allocates its own, guarded
        try:
            run = PASSES[name]()                                  # modules, weights: before the arena
            with guarded(mp) as arena, ga.LaunchLog(arena) as log:
                results = run(arena)
                blocks = arena.check()
                bad = [tuple(t.shape) for t in _leaves(results) if not _finite([t])]
                assert not bad, f'{name}: non-finite results of shapes {bad[:8]}'
            _CACHE[name] = types.SimpleNamespace(log=log, blocks=blocks, seconds=time.perf_counter() - t0)
        except AssertionError as e:
            _CACHE[name] = e
        except BaseException:
            _DEAD.append(name)
            raise
        finally:
            mp.undo()
            ops._BN_SCRATCH.clear()
    if isinstance(_CACHE[name], AssertionError):
        raise _CACHE[name]
    return _CACHE[name]


@pytest.mark.parametrize('name', list(PASSES))
def test_pass_keeps_its_guard_bands(name):
    r = run_pass(name)
    n, stores, reads = r.log.shares()
    print(f'{name}: {n} launches of {len(r.log.launches)} entry points, {r.blocks} guarded buffers, all bands intact; '
          f'{stores:.1%} of the store pointers and {reads:.1%} of the read pointers inside the arena; {r.seconds:.1f} s')
    assert n > 0


def test_coverage_is_the_committed_tables():
    logs = {name: run_pass(name).log for name in PASSES}
    assert set(ga.EXPECTED_REACHED) == set(PASSES)
    unguarded, reached, missing = set(), set(), {}
    for name, log in logs.items():
        n, stores, reads = log.shares()
        print(f'{name}: {n} launches, store pointers guarded {stores:.1%}, read pointers guarded {reads:.1%}')
        unguarded |= log.unguarded_stores()
        reached |= log.reached_guarded()
        lost = set(ga.EXPECTED_REACHED[name]) - log.reached_guarded()
        if lost:
            missing[name] = sorted(lost)
    assert not missing, f'entry points a pass no longer reaches with every store pointer guarded: {missing}'
    assert unguarded == set(ga.UNGUARDED_STORES), (
        f'stores outside the arena: new {sorted(unguarded - set(ga.UNGUARDED_STORES))}, '
        f'gone {sorted(set(ga.UNGUARDED_STORES) - unguarded)}')
    from dynamask_amd import hazard
    surface = ga.launching(hazard.parse_header()) - set(ga.NO_CALL_SITE)
    print(f'{len(reached & surface)} of {len(surface)} launching entry points with a call site reached under guard bands')
    assert surface <= reached, sorted(surface - reached)
