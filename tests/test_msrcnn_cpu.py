"""Mask Scoring R-CNN through the registry, without a GPU: the ``roi_head`` of configs/ms_rcnn (merged over its mask_rcnn
base, as resolved from the reference tree: tests/golden/g19_msrcnn_configs.json) builds unchanged, the module tree has
the reference MaskScoringRoIHead's ``state_dict`` keys (tests/golden/g19_msrcnn.npz), the empty mask test has the
reference's two-list form, and the calls out of scope (training, graph capture) and the unsupported constructor forms
raise."""
import json
import os

import numpy as np
import pytest
import torch


def _build(golden_dir):
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    with open(os.path.join(golden_dir, 'g19_msrcnn_configs.json')) as f:
        cfg = registry._to_cfgdict(json.load(f)['coco'])
    rh = dict(cfg.model.roi_head)
    assert rh['type'] == 'MaskScoringRoIHead' and rh['mask_iou_head']['type'] == 'MaskIoUHead'
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=cfg.test_cfg.rcnn)
    return registry.build_head(rh), cfg


def test_config_builds(golden_dir):
    m, cfg = _build(golden_dir)
    assert type(m).__name__ == 'MaskScoringRoIHead' and type(m.mask_head).__name__ == 'FCNMaskHead'
    h = m.mask_iou_head
    assert type(h).__name__ == 'MaskIoUHead' and h.num_classes == 80
    assert [tuple(c.weight.shape) for c in h.convs] == [(256, 257, 3, 3)] + [(256, 256, 3, 3)] * 3
    assert [tuple(fc.weight.shape) for fc in h.fcs] == [(1024, 12544), (1024, 1024)]
    assert tuple(h.fc_mask_iou.weight.shape) == (80, 1024)
    assert type(h.loss_iou).__name__ == 'MSELoss' and h.loss_iou.loss_weight == 0.5
    assert m.train_cfg.mask_thr_binary == 0.5 and m.test_cfg.mask_thr_binary == 0.5


def test_state_dict_keys_equal_the_reference(golden_dir):
    """Every key and shape is the reference's, incl. the mask_predictor block of the fork's BaseRoIHead (Quirk Q4)."""
    z = np.load(os.path.join(golden_dir, 'g19_msrcnn.npz'))
    ref = set(z['state_dict_keys'].tolist())
    m, _ = _build(golden_dir)
    keys = set(m.state_dict())
    assert keys == ref
    assert any(k.startswith('mask_predictor.') for k in keys)
    sd = m.state_dict()
    assert tuple(sd['mask_iou_head.convs.0.weight'].shape) == (256, 257, 3, 3)
    assert tuple(sd['mask_iou_head.fc_mask_iou.bias'].shape) == (80,)


def test_empty_detections_give_two_empty_lists(golden_dir):
    """mask_scoring_roi_head.py:69-71: ``([[]] * C, [[]] * C)`` -- one image and each image of a batch (no device work)."""
    m, _ = _build(golden_dir)
    meta = dict(ori_shape=(64, 80, 3), img_shape=(64, 80, 3), scale_factor=1.0)
    segm, scores = m.simple_test_mask(None, [meta], torch.zeros((0, 5)), torch.zeros((0,), dtype=torch.long))
    assert segm == [[] for _ in range(80)] and scores == [[] for _ in range(80)]
    res = m.batch_simple_test_mask(None, [meta, meta], [torch.zeros((0, 5))] * 2, [torch.zeros((0,), dtype=torch.long)] * 2)
    assert len(res) == 2
    for segm, scores in res:
        assert segm == [[] for _ in range(80)] and scores == [[] for _ in range(80)]


def test_group_mask_scores():
    """maskiou_head.py:178-181: per class, that class's scores in detection order."""
    from dynamask_amd.mask_heads import group_mask_scores
    s = np.array([0.5, 0.25, 0.125, 1.0], dtype=np.float32)
    g = group_mask_scores(s, np.array([2, 0, 2, 4]), 5)
    assert [x.tolist() for x in g] == [[0.25], [], [0.5, 0.125], [], [1.0]]
    assert all(x.dtype == np.float32 for x in g)


def test_out_of_scope_calls_raise(golden_dir):
    m, _ = _build(golden_dir)
    with pytest.raises(NotImplementedError, match='Q5'):
        m.forward_train(None, [], [], [], [])
    with pytest.raises(NotImplementedError, match='Q5'):
        m.mask_iou_head.get_targets([], [], None, None, m.train_cfg)
    with pytest.raises(NotImplementedError, match='Q5'):
        m.mask_iou_head.loss(None, None)
    with pytest.raises(NotImplementedError, match='Q5'):
        m.mask_iou_head.loss_iou(None, None)
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.enable_inference_graphs(True)
    assert m.enable_inference_graphs(False) is None


def test_unsupported_constructor_forms_raise(golden_dir):
    from dynamask_amd import mask_heads, roi_head
    with pytest.raises(NotImplementedError):
        mask_heads.MaskIoUHead(num_convs=1)
    with pytest.raises(NotImplementedError):
        mask_heads.MaskIoUHead(num_fcs=0)
    with pytest.raises(NotImplementedError):
        mask_heads.MaskIoUHead(roi_feat_size=13)
    with pytest.raises(NotImplementedError):
        mask_heads.MaskIoUHead(conv_out_channels=20)
    _, cfg = _build(golden_dir)
    rh = dict(cfg.model.roi_head)
    rh.pop('type')
    iou = rh.pop('mask_iou_head')
    with pytest.raises(ValueError):
        roi_head.MaskScoringRoIHead(**rh)
    no_mask = {k: v for k, v in rh.items() if k not in ('mask_head', 'mask_roi_extractor')}
    with pytest.raises(ValueError):
        roi_head.MaskScoringRoIHead(mask_iou_head=iou, **no_mask)
