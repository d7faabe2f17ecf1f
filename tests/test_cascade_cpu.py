"""Cascade Mask R-CNN through the registry, without a GPU: the ``roi_head`` of
configs/cascade_rcnn/cascade_mask_rcnn_r50_fpn_1x_coco.py (as resolved from the reference tree:
tests/golden/g21_cascade_configs.json) builds unchanged, the module tree has the reference CascadeRoIHead's
``state_dict`` keys (tests/golden/g21_cascade.npz), the calls out of scope raise and malformed stage counts raise."""
import json
import os

import numpy as np
import pytest
import torch


def _cfg(golden_dir):
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    with open(os.path.join(golden_dir, 'g21_cascade_configs.json')) as f:
        cfg = registry._to_cfgdict(json.load(f)['coco'])
    rh = dict(cfg.model.roi_head)
    assert rh['type'] == 'CascadeRoIHead'
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=cfg.test_cfg.rcnn)
    return rh


def _build(golden_dir, **over):
    from dynamask_amd import registry
    rh = _cfg(golden_dir)
    rh.update(over)
    return registry.build_head(rh)


def test_config_builds(golden_dir):
    m = _build(golden_dir)
    assert type(m).__name__ == 'CascadeRoIHead' and m.num_stages == 3
    assert list(m.stage_loss_weights) == [1, 0.5, 0.25]
    assert len(m.bbox_head) == len(m.bbox_roi_extractor) == len(m.mask_head) == len(m.mask_roi_extractor) == 3
    stds = [tuple(h.bbox_coder.stds) for h in m.bbox_head]
    assert stds == [(0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067)]
    assert all(h.reg_class_agnostic and h.num_classes == 80 for h in m.bbox_head)
    assert all(tuple(h.fc_reg.weight.shape) == (4, 1024) for h in m.bbox_head)
    assert all(type(h).__name__ == 'FCNMaskHead' and h.num_convs == 4 and h.upsample_method == 'deconv'
               for h in m.mask_head)
    assert m._one_mask_extraction and m._mask_logits_size() == (80, 28) and m._segm_num_classes() == 80
    assert m.test_cfg.mask_thr_binary == 0.5


def test_state_dict_keys_equal_the_reference(golden_dir):
    """Every key is the reference's, incl. the mask_predictor block of the fork's BaseRoIHead (Quirk Q4)."""
    z = np.load(os.path.join(golden_dir, 'g21_cascade.npz'))
    ref = set(z['state_dict_keys'].tolist())
    m = _build(golden_dir)
    sd = m.state_dict()
    assert set(sd) == ref
    assert any(k.startswith('mask_predictor.') for k in sd)
    assert tuple(sd['bbox_head.2.shared_fcs.0.weight'].shape) == (1024, 12544)
    assert tuple(sd['mask_head.1.conv_logits.weight'].shape) == (80, 256, 1, 1)


def test_per_stage_lists_build(golden_dir):
    """Lists of one config per stage, and stage heads that differ: class-specific regression in the last stage."""
    rh = _cfg(golden_dir)
    bh = [dict(h) for h in rh['bbox_head']]
    bh[2]['reg_class_agnostic'] = False
    ext = dict(rh['mask_roi_extractor'])
    m = _build(golden_dir, bbox_head=bh, mask_roi_extractor=[ext, ext, dict(ext, out_channels=256)],
               mask_head=[dict(rh['mask_head'])] * 3)
    assert tuple(m.bbox_head[2].fc_reg.weight.shape) == (320, 1024) and m.bbox_head[0].reg_class_agnostic
    assert m._one_mask_extraction


def test_out_of_scope_calls_raise(golden_dir):
    m = _build(golden_dir)
    with pytest.raises(NotImplementedError, match='Q5'):
        m.forward_train(None, [], [], [], [])
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.enable_inference_graphs(True)
    assert m.enable_inference_graphs(False) is None
    with pytest.raises(NotImplementedError, match='shared-extractor'):
        _build(golden_dir, mask_roi_extractor=None)
    with pytest.raises(NotImplementedError, match='Shared head'):
        _build(golden_dir, shared_head=dict(type='ResLayer'))


@pytest.mark.parametrize('over', [
    dict(num_stages=0), dict(num_stages='3'), dict(num_stages=2.0), dict(num_stages=True),
    dict(stage_loss_weights=[1, 0.5]), dict(num_stages=2),
    dict(bbox_roi_extractor=None), dict(bbox_head=None),
])
def test_malformed_stage_counts_raise(golden_dir, over):
    with pytest.raises(ValueError):
        _build(golden_dir, **over)


def test_malformed_per_stage_lists_raise(golden_dir):
    rh = _cfg(golden_dir)
    with pytest.raises(ValueError, match='bbox_head'):
        _build(golden_dir, bbox_head=list(rh['bbox_head'])[:2])
    with pytest.raises(ValueError, match='mask_head'):
        _build(golden_dir, mask_head=[rh['mask_head']] * 4)
    with pytest.raises(ValueError, match='mask_roi_extractor'):
        _build(golden_dir, mask_roi_extractor=[rh['mask_roi_extractor']])
    with pytest.raises(ValueError, match='bbox_roi_extractor'):
        _build(golden_dir, bbox_roi_extractor=[rh['bbox_roi_extractor']] * 2)


def test_empty_detections_give_empty_lists(golden_dir):
    """cascade_roi_head.py:333-335: ``[[] for _ in range(80)]`` -- one image and each image of a batch (no device work)."""
    m = _build(golden_dir)
    meta = dict(ori_shape=(64, 80, 3), img_shape=(64, 80, 3), scale_factor=1.0, flip=False, flip_direction=None)
    segm = m.simple_test_mask(None, [meta], torch.zeros((0, 5)), torch.zeros((0,), dtype=torch.long))
    assert segm == [[] for _ in range(80)]
    res = m.batch_simple_test_mask(None, [meta, meta], [torch.zeros((0, 5))] * 2, [torch.zeros((0,), dtype=torch.long)] * 2)
    assert res == [[[] for _ in range(80)]] * 2
