"""Host-side checks of test-time augmentation (DynaMaskRoIHead.aug_test and the pieces under it): argument and meta
validation before any device work, the empty-detection result, the g16 fixture, and the new C-ABI entry points."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(kind='dynamask'):
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, synth  # noqa: F401
    from dynamask_amd.registry import ConfigDict
    mask_head = dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG) if kind == 'dynamask' else \
        dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG)
    return registry.build_head(dict(
        type='DynaMaskRoIHead' if kind == 'dynamask' else 'StandardRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=mask_head, test_cfg=ConfigDict(**synth.RCNN_TEST_CFG)))


def _meta(flip=False, direction=None, sf=1.0):
    return [dict(img_shape=(64, 80, 3), ori_shape=(64, 80, 3), scale_factor=sf, flip=flip, flip_direction=direction)]


def _x():
    return [torch.zeros(1, 256, 16 // s, 20 // s) for s in (1, 2, 4, 8, 16)]


@pytest.mark.parametrize('kind', ['dynamask', 'fcn'])
def test_aug_test_validates_before_any_device_work(kind):
    """Every check raises on CPU tensors: nothing reached the device (which these tensors cannot)."""
    m = _head(kind)
    props = [torch.zeros(3, 4)]
    dets, labels = torch.zeros(2, 5), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match='non-empty'):
        m.aug_test([_x()], props, [])
    with pytest.raises(ValueError, match='x has 2 views, img_metas 1'):
        m.aug_test([_x(), _x()], props, [_meta()])
    with pytest.raises(ValueError, match='x has 1 views, img_metas 2'):
        m.aug_test_mask([_x()], [_meta(), _meta(True, 'horizontal')], dets, labels)
    with pytest.raises(ValueError, match="invalid flipping direction 'diagonal'"):
        m.aug_test([_x(), _x()], props, [_meta(), _meta(True, 'diagonal')])
    with pytest.raises(ValueError, match="invalid flipping direction 'diagonal'"):
        m.aug_test_mask_probs([_x(), _x()], [_meta(), _meta(True, 'diagonal')], dets, labels)
    with pytest.raises(ValueError, match="invalid flipping direction"):
        m.aug_test_bboxes([_x(), _x()], [_meta(True, 'horizontal'), _meta(True, None)], props, m.test_cfg)
    bad = _meta()
    del bad[0]['flip']
    with pytest.raises(ValueError, match=r"img_metas\[1\]\[0\] lacks \['flip'\]"):
        m.aug_test([_x(), _x()], props, [_meta(), bad])
    with pytest.raises(ValueError, match='one meta per view'):
        m.aug_test([_x()], props, [_meta() * 2])
    with pytest.raises(ValueError, match='batch dimension 2'):
        m.aug_test([[torch.zeros(2, 256, 16, 20)]], props, [_meta()])
    with pytest.raises(ValueError, match='scale_factor has 3 values'):
        m.aug_test([_x()], props, [_meta(sf=np.ones(3, np.float32))])


def test_aug_view_rows():
    from dynamask_amd import ops
    rows = ops.aug_view_rows([dict(img_shape=(60, 90, 3), scale_factor=1.5, flip=False, flip_direction='horizontal'),
                              dict(img_shape=(60, 90, 3), scale_factor=np.array([1.5, 1.25, 1.5, 1.25]), flip=True,
                                   flip_direction='horizontal'),
                              dict(img_shape=(61, 91), scale_factor=0.1, flip=True, flip_direction='vertical')])
    assert rows[0] == [1.5] * 4 + [60.0, 90.0, 0.0, 0.0]
    assert rows[1] == [1.5, 1.25, 1.5, 1.25, 60.0, 90.0, 1.0, 0.0]
    assert rows[2] == [float(np.float32(0.1))] * 4 + [61.0, 91.0, 2.0, 0.0]       # fp32, as new_tensor(scale_factor)
    assert len(rows[0]) == ops.AUG_VIEW_FLOATS


@pytest.mark.parametrize('kind', ['dynamask', 'fcn'])
def test_aug_empty_detections_need_no_device(kind):
    m = _head(kind)
    metas = [_meta(), _meta(True, 'horizontal'), _meta(True, 'vertical', sf=0.5)]
    xs = [_x()] * 3
    segm = m.aug_test_mask(xs, metas, torch.zeros(0, 5), torch.zeros(0, dtype=torch.long))
    assert segm == [[] for _ in range(80)]
    assert m.aug_test_mask(xs, metas, torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), encode=True) == segm
    probs = m.aug_test_mask_probs(xs, metas, torch.zeros(0, 5), torch.zeros(0, dtype=torch.long))
    assert probs.shape[:2] == (0, 1)
    dets, labels = m.aug_test_bboxes(xs, metas, [torch.zeros(0, 4)], m.test_cfg)
    assert dets.shape == (0, 5) and labels.shape == (0,) and labels.dtype == torch.long
    bbox_results, segm_results = m.aug_test(xs, [torch.zeros(0, 4)], metas)
    assert len(bbox_results) == 80 and all(b.shape == (0, 5) and b.dtype == np.float32 for b in bbox_results)
    assert segm_results == [[] for _ in range(80)]


def test_aug_golden_fixture_present():
    import aug_inputs as ai
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g16_aug.npz'))
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g16_aug.npz')) < 2 * 1024 * 1024
    h, w = ai.ORI_SHAPE[:2]
    for case in ai.CASES:
        n = g[f'{case}_labels'].shape[0]
        assert n > 0
        assert g[f'{case}_dets'].shape == (n, 5) and g[f'{case}_dets'].dtype == np.float32
        assert g[f'{case}_probs'].shape == (n, 28, 28) and g[f'{case}_probs'].dtype == np.float32
        assert g[f'{case}_bits'].shape == (n, h, w)
        assert g[f'{case}_bbox_counts'].shape == (80,) and g[f'{case}_bbox_counts'].sum() == n
        assert np.all(np.diff(g[f'{case}_dets'][:, 4]) <= 0)          # score order
    assert any(d == 'vertical' for s, d in ai.CASES['vf']) and len(ai.CASES['ms']) == 4


def test_aug_entry_points_are_declared():
    from dynamask_amd import _lib, hazard
    hdr = open(os.path.join(ROOT, 'include', 'dynamask_hip.h')).read()
    roles = hazard.parse_header()
    for name in ('dm_bbox_mapping_multi', 'dm_merge_aug_bboxes', 'dm_merge_aug_masks'):
        assert name in _lib.SIGNATURES and f'{name}(' in hdr
        assert len(roles[name]) == len(_lib.SIGNATURES[name][0])
    assert '#define DM_AUG_VIEW_FLOATS 8' in hdr
