"""The detector without a device: ``build_detector`` on the reference's whole configs (tests/golden/
g29_detector_configs.json), the ``state_dict`` keys, ``load_checkpoint``, the refusals, ``forward_test``'s checks, and the
host side of the image pre-processing (``rescale_size``, the per-axis table, the pipeline parser) against hand-computed
values."""
import copy
import json
import os

import numpy as np
import pytest
import torch

TYPES = dict(dynamask=('MaskRCNN', 'DynaMaskRoIHead'), mask_rcnn=('MaskRCNN', 'StandardRoIHead'),
             mask_c4=('MaskRCNN', 'StandardRoIHead'), faster_c4=('FasterRCNN', 'StandardRoIHead'),
             cascade=('CascadeRCNN', 'CascadeRoIHead'), htc=('HybridTaskCascade', 'HybridTaskCascadeRoIHead'),
             msrcnn=('MaskScoringRCNN', 'MaskScoringRoIHead'), pointrend=('PointRend', 'PointRendRoIHead'),
             grid=('GridRCNN', 'GridRoIHead'), double=('FasterRCNN', 'DoubleHeadRoIHead'))


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g29_detector_configs.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def mask_rcnn(cfgs):
    from dynamask_amd import build_detector
    torch.manual_seed(0)
    return build_detector(copy.deepcopy(cfgs['mask_rcnn']['model']), test_cfg=copy.deepcopy(cfgs['mask_rcnn']['test_cfg']))


def _pinned(golden_dir, name, key):
    with open(os.path.join(golden_dir, name)) as f:
        return [k for k, _ in json.load(f)[key]['state_dict']]


# ------------------------------------------------------------------------------------------------ build
@pytest.mark.parametrize('name', sorted(TYPES))
def test_build_detector_from_the_references_config(cfgs, name):
    import dynamask_amd
    from dynamask_amd import detectors, registry
    cfg = cfgs[name]
    assert set(cfgs) == set(TYPES) and cfg['model']['type'] == TYPES[name][0]
    before = copy.deepcopy(cfg)
    det = dynamask_amd.build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert cfg == before, 'the build changed the caller\'s config'
    assert type(det) is getattr(detectors, TYPES[name][0]) and isinstance(det, detectors.TwoStageDetector)
    assert dynamask_amd.DETECTORS is registry.DETECTORS and registry.DETECTORS.get(TYPES[name][0]) is type(det)
    assert type(det.roi_head).__name__ == TYPES[name][1]
    assert det.with_rpn and det.with_roi_head and det.with_bbox
    assert det.with_neck == ('neck' in cfg['model']) and det.with_neck == hasattr(det, 'neck')
    assert det.with_mask == ('mask_head' in cfg['model']['roi_head'] or name in ('cascade', 'htc'))
    assert det.with_shared_head == ('shared_head' in cfg['model']['roi_head'])
    assert det.pretrained == cfg['model']['pretrained'] and det.train_cfg is None and det.test_cfg == cfg['test_cfg']
    # test_cfg.rpn reaches the RPN, test_cfg.rcnn the RoI head
    assert det.rpn_head.test_cfg == cfg['test_cfg']['rpn'] and det.roi_head.test_cfg == cfg['test_cfg']['rcnn']
    assert det.rpn_head.train_cfg is None and det.roi_head.train_cfg is None
    if name == 'htc':
        assert det.with_semantic
    # the keys: the parts', built one by one, under the reference's prefixes
    m = registry._to_cfgdict(cfg['model'])
    parts = [('backbone', registry.build_backbone(dict(m.backbone)))]
    if 'neck' in m:
        parts.append(('neck', registry.build_neck(dict(m.neck))))
    parts.append(('rpn_head', registry.build_head(dict(m.rpn_head, train_cfg=None, test_cfg=cfg['test_cfg']['rpn']))))
    parts.append(('roi_head', registry.build_head(dict(m.roi_head, train_cfg=None, test_cfg=cfg['test_cfg']['rcnn']))))
    want = [(f'{p}.{k}', tuple(v.shape)) for p, mod in parts for k, v in mod.state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in det.state_dict().items()] == want


def test_state_dict_keys_are_the_pinned_parts(golden_dir, mask_rcnn, cfgs):
    from dynamask_amd import build_detector
    keys = list(mask_rcnn.state_dict())
    want = ['backbone.' + k for k in _pinned(golden_dir, 'g28_backbone_configs.json', 'pytorch')] + \
        ['neck.' + k for k in _pinned(golden_dir, 'g27_fpn_configs.json', 'mask_rcnn')] + \
        ['rpn_head.' + k for k in _pinned(golden_dir, 'g26_rpn_configs.json', 'fpn')]
    assert keys[:len(want)] == want and all(k.startswith('roi_head.') for k in keys[len(want):])
    c4 = build_detector(cfgs['mask_c4']['model'], test_cfg=cfgs['mask_c4']['test_cfg'])
    keys = list(c4.state_dict())
    want = ['backbone.' + k for k in _pinned(golden_dir, 'g28_backbone_configs.json', 'caffe_c4')] + \
        ['rpn_head.' + k for k in _pinned(golden_dir, 'g26_rpn_configs.json', 'c4')]
    assert keys[:len(want)] == want
    assert set(keys[len(want):]) >= {'roi_head.' + k for k in _pinned(golden_dir, 'g25_c4_configs.json', 'mask_c4')}


def test_train_cfg_reaches_the_parts_and_fast_rcnn_has_no_rpn(cfgs):
    from dynamask_amd import build_detector, registry
    cfg = copy.deepcopy(cfgs['mask_rcnn'])
    model = {k: v for k, v in cfg['model'].items() if k != 'rpn_head'}
    model['type'] = 'FastRCNN'
    det = build_detector(model, train_cfg=None, test_cfg=dict(rcnn=cfg['test_cfg']['rcnn']))
    assert not det.with_rpn and det.with_neck and det.roi_head.test_cfg == cfg['test_cfg']['rcnn']
    assert not any(k.startswith('rpn_head.') for k in det.state_dict())
    with pytest.raises(ValueError, match='proposals'):
        det.simple_test(torch.zeros(1, 3, 32, 32), [dict()])
    with pytest.raises(NotImplementedError, match='augmentation'):
        det.forward_test([0, 1], [[], []], proposals=[[], []])
    with pytest.raises(ValueError, match=r'num of augmentations \(2\) != num of image meta \(1\)'):
        det.forward_test([0, 1], [[]], proposals=[[]])
    with pytest.raises(KeyError, match='detector registry'):
        build_detector(dict(cfg['model'], type='RetinaNet'), test_cfg=cfg['test_cfg'])
    with pytest.raises(KeyError, match='NoSuchDetector is not in the detector registry'):
        registry.build_detector(dict(type='NoSuchDetector'))


# ------------------------------------------------------------------------------------------------ checkpoints
def test_load_checkpoint(mask_rcnn, cfgs, tmp_path):
    from dynamask_amd import build_detector, detectors
    g = torch.Generator().manual_seed(3)
    state = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in mask_rcnn.state_dict().items()}
    meta = {'CLASSES': ('person', 'cat'), 'epoch': 12}
    fresh = build_detector(copy.deepcopy(cfgs['mask_rcnn']['model']), test_cfg=copy.deepcopy(cfgs['mask_rcnn']['test_cfg']))
    for prefix in ('', 'module.'):
        path = str(tmp_path / f'ckpt{len(prefix)}.pth')
        torch.save({'state_dict': {prefix + k: v for k, v in state.items()}, 'meta': meta}, path)
        for p in fresh.parameters():
            p.data.zero_()
        got = detectors.load_checkpoint(fresh, path, strict=True)
        assert got == (meta, [], [])
        assert all(torch.equal(v, state[k]) for k, v in fresh.state_dict().items())
    # the dict itself, and a bare state dict: no meta
    assert detectors.load_checkpoint(fresh, {'state_dict': state, 'meta': meta}) == (meta, [], [])
    assert detectors.load_checkpoint(fresh, dict(state), strict=True) == ({}, [], [])
    # a missing and an unexpected key: named when strict (and nothing loaded), returned when not
    broken = dict(state)
    del broken['neck.fpn_convs.0.conv.bias']
    broken['roi_head.extra.weight'] = torch.zeros(1)
    broken['backbone.conv1.weight'] = torch.full_like(state['backbone.conv1.weight'], 7.0)
    with pytest.raises(RuntimeError, match=r"missing keys \['neck.fpn_convs.0.conv.bias'\], unexpected keys \['roi_head.extra.weight'\]"):
        detectors.load_checkpoint(fresh, {'state_dict': broken}, strict=True)
    assert torch.equal(fresh.backbone.conv1.weight, state['backbone.conv1.weight'])
    m, missing, unexpected = detectors.load_checkpoint(fresh, {'state_dict': broken, 'meta': None})
    assert (m, missing, unexpected) == ({}, ['neck.fpn_convs.0.conv.bias'], ['roi_head.extra.weight'])
    assert bool((fresh.backbone.conv1.weight == 7.0).all())
    assert torch.equal(fresh.neck.fpn_convs[0].conv.bias, state['neck.fpn_convs.0.conv.bias'])       # left as it was


# ------------------------------------------------------------------------------------------------ refusals and dispatch
def test_training_and_the_rest_raise_naming_what_is_missing(mask_rcnn):
    import asyncio
    img, metas = torch.zeros(1, 3, 32, 32), [dict()]
    with pytest.raises(NotImplementedError, match='forward_train.*training'):
        mask_rcnn.forward_train(img, metas)
    with pytest.raises(NotImplementedError, match='forward_train'):
        mask_rcnn.forward(img, metas, return_loss=True)
    with pytest.raises(NotImplementedError, match='forward_train'):
        mask_rcnn(img, metas, return_loss=True, gt_bboxes=[])
    with pytest.raises(NotImplementedError, match='forward_dummy'):
        mask_rcnn.forward_dummy(img)
    with pytest.raises(NotImplementedError, match='show_result'):
        mask_rcnn.show_result(None, None)
    with pytest.raises(NotImplementedError, match='async_simple_test'):
        asyncio.run(mask_rcnn.async_simple_test(img, metas))
    with pytest.raises(NotImplementedError, match='aforward_test'):
        asyncio.run(mask_rcnn.aforward_test(img=[img], img_metas=[metas]))


def test_forward_test_checks_as_the_reference_does(mask_rcnn):
    img, metas = torch.zeros(1, 3, 32, 32), [dict()]
    with pytest.raises(TypeError, match='imgs must be a list'):
        mask_rcnn.forward_test(img, [metas])
    with pytest.raises(TypeError, match='img_metas must be a list'):
        mask_rcnn.forward_test([img], tuple([metas]))
    with pytest.raises(ValueError, match=r'num of augmentations \(2\) != num of image meta \(1\)'):
        mask_rcnn.forward_test([img, img], [metas])
    with pytest.raises(ValueError, match=r'num of augmentations \(1\) != num of image meta \(2\)'):
        mask_rcnn(([img]), [metas, metas])
    with pytest.raises(AssertionError):
        mask_rcnn.forward_test([img, img], [metas, metas], proposals=[[], []])
    # the maps reach the operators, which want the GPU: no CPU fallback
    with pytest.raises(RuntimeError, match='no CPU fallback'), torch.no_grad():
        mask_rcnn.forward_test([img], [metas])


# ------------------------------------------------------------------------------------------------ the pipeline's host side
def test_rescale_size_by_hand():
    from dynamask_amd.detectors import rescale_size
    # (480, 640): s = min(1333 / 640, 800 / 480) = 5 / 3 -> 640 * 5 / 3 + 0.5 = 1067.17, 480 * 5 / 3 + 0.5 = 800.5
    nh, nw, sf = rescale_size(480, 640, (1333, 800))
    assert (nh, nw) == (800, 1067) and sf.dtype == np.float32 and sf.shape == (4,)
    assert np.array_equal(sf, np.array([1067 / 640, 800 / 480, 1067 / 640, 800 / 480], dtype=np.float32))
    # (427, 640): s = min(2.0828, 800 / 427 = 1.87354) -> 640 * 1.87354 + 0.5 = 1199.56, 427 * s + 0.5 = 800.5
    nh, nw, sf = rescale_size(427, 640, (800, 1333))
    assert (nh, nw) == (800, 1199) and sf.dtype == np.float32
    assert np.array_equal(sf, np.array([1199 / 640, 800 / 427, 1199 / 640, 800 / 427], dtype=np.float32))
    assert rescale_size(640, 480, (1333, 800))[:2] == (1067, 800)
    with pytest.raises(NotImplementedError, match='scale factor'):
        rescale_size(480, 640, 2.0)
    with pytest.raises(ValueError, match='empty'):
        rescale_size(0, 640, (1333, 800))


def test_axis_table_by_hand():
    """n_src = 5, n_dst = 11: f(d) = (d + 0.5) * 5 / 11 - 0.5.  d = 0: f = -0.2727 -> below the axis: tap 0 alone.
    d = 1: f = 0.18182 -> taps 0, 1 with t = 0.18182: c1 = rint(372.36) = 372, c0 = rint(1675.64) = 1676.
    d = 10: f = 4.2727 -> i = 4 is the last source index: tap 4 alone."""
    from dynamask_amd import ops
    i0, i1, c0, c1 = ops.resize_axis_table(5, 11)
    assert (i0.dtype, i1.dtype, c0.dtype, c1.dtype) == (np.int32, np.int32, np.int16, np.int16) and len(i0) == 11
    assert (i0[0], i1[0], c0[0], c1[0]) == (0, 1, 2048, 0)
    assert (i0[1], i1[1], c0[1], c1[1]) == (0, 1, 1676, 372)
    assert (i0[10], i1[10], c0[10], c1[10]) == (4, 4, 2048, 0)
    assert ((c0.astype(int) + c1) == 2048).all() and (i0 >= 0).all() and (i1 <= 4).all()
    assert ops.resize_axis_table(5, 11) is ops.resize_axis_table(5, 11)                 # cached per (n_src, n_dst)
    same = ops.resize_axis_table(9, 9)
    assert (same[0] == np.arange(9)).all() and (same[2] == 2048).all() and (same[3] == 0).all()
    one = ops.resize_axis_table(1, 3)
    assert (one[0] == 0).all() and (one[1] == 0).all() and (one[2] == 2048).all()
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError, match='at least 1'):
            ops.resize_axis_table(*bad)


def test_pipeline_parser_reads_the_references_dicts(cfgs):
    from dynamask_amd import detectors, registry
    for name, cfg in cfgs.items():
        p = detectors.parse_test_pipeline(cfg['test_pipeline'])
        assert p['img_scales'] == [(1333, 800)] and p['flip'] is False and p['keep_ratio'] is True and p['size_divisor'] == 32
        assert p['flip_directions'] == ['horizontal']
        assert p['img_norm_cfg'] == dict(cfg['img_norm_cfg'], to_rgb=cfg['img_norm_cfg']['to_rgb']), name
    assert detectors.parse_test_pipeline(cfgs['mask_c4']['test_pipeline'])['img_norm_cfg']['to_rgb'] is False
    pipe = copy.deepcopy(cfgs['mask_rcnn']['test_pipeline'])
    aug = pipe[1]
    assert aug['type'] == 'MultiScaleFlipAug'
    aug.update(img_scale=[(1333, 800), (2000, 1200)], flip=True, flip_direction=['horizontal', 'vertical'])
    for holder in (pipe, dict(test_pipeline=pipe), registry._to_cfgdict(dict(data=dict(test=dict(pipeline=pipe))))):
        p = detectors.parse_test_pipeline(holder)
        assert p['img_scales'] == [(1333, 800), (2000, 1200)] and p['flip'] is True
        assert p['flip_directions'] == ['horizontal', 'vertical']
    aug['transforms'] = [t for t in aug['transforms'] if t['type'] != 'RandomFlip']
    assert detectors.parse_test_pipeline(pipe)['flip'] is False              # flip has no effect without RandomFlip
    for change, match in ((dict(scale_factor=1.0, img_scale=None), 'scale_factor'),
                          (dict(transforms=[dict(type='Resize', keep_ratio=True), dict(type='Albu')]), 'Albu'),
                          (dict(transforms=[dict(type='Resize'), dict(type='Normalize', mean=[0] * 3, std=[1] * 3),
                                            dict(type='Pad', size=(800, 800))]), 'Pad')):
        bad = copy.deepcopy(pipe)
        bad[1].update(change)
        with pytest.raises(NotImplementedError, match=match):
            detectors.parse_test_pipeline(bad)
    with pytest.raises(KeyError, match='test_pipeline'):
        detectors.parse_test_pipeline(dict(model=dict()))
    with pytest.raises(NotImplementedError, match='keep_ratio'):
        detectors.preprocess([torch.zeros(4, 4, 3, dtype=torch.uint8)], cfgs['mask_rcnn']['img_norm_cfg'], keep_ratio=False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        detectors.preprocess([torch.zeros(4, 4, 3, dtype=torch.uint8)], cfgs['mask_rcnn']['img_norm_cfg'], img_scale=(8, 8))


def test_package_exports_are_lazy():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys, dynamask_amd\n'
            'assert "dynamask_amd.detectors" not in sys.modules and "dynamask_amd.ops" not in sys.modules\n'
            'd = dynamask_amd.build_detector\n'
            'assert "dynamask_amd.detectors" in sys.modules and "MaskRCNN" in dynamask_amd.DETECTORS\n'
            'import dynamask_amd.roi_head, dynamask_amd.dense_heads, dynamask_amd.necks, dynamask_amd.backbones\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=root, env=dict(os.environ, PYTHONPATH=root))
    # nothing below the detectors imports them
    code = ('import sys\nimport dynamask_amd.roi_head, dynamask_amd.dense_heads, dynamask_amd.necks, dynamask_amd.backbones\n'
            'assert "dynamask_amd.detectors" not in sys.modules\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=root, env=dict(os.environ, PYTHONPATH=root))
