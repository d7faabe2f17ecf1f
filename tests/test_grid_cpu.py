"""Grid R-CNN through the registry, without a GPU: the ``roi_head`` of the three configs/grid_rcnn files (as resolved from
the reference tree: tests/golden/g23_grid_configs.json) builds unchanged, the module tree has the reference
GridRoIHead's ``state_dict`` keys and shapes (tests/golden/g23_grid.npz) and loads such a ``state_dict`` strictly,
``calc_sub_regions`` gives the reference's values for 4, 9 and 16 points, ``Shared2FCBBoxHead(with_reg=False)`` has no
regression branch, the empty case launches nothing, and the calls out of scope and the unsupported constructor forms
raise."""
import json
import os

import numpy as np
import pytest
import torch

CONFIGS = ('r50_1x', 'r50_2x', 'r101_2x')


def _cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g23_grid_configs.json')) as f:
        return json.load(f)


def _build(golden_dir, name='r50_2x', **extra):
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = registry._to_cfgdict(_cfgs(golden_dir)[name])
    rh = dict(cfg.model.roi_head)
    assert rh['type'] == 'GridRoIHead' and rh['grid_head']['type'] == 'GridHead'
    rh.update(train_cfg=None, test_cfg=cfg.test_cfg.rcnn)
    rh.update(extra)
    return registry.build_head(rh), cfg


@pytest.mark.parametrize('name', CONFIGS)
def test_config_builds(golden_dir, name):
    m, cfg = _build(golden_dir, name)
    assert type(m).__name__ == 'GridRoIHead' and not m.with_mask and not m.share_roi_extractor
    assert m.grid_roi_extractor is not m.bbox_roi_extractor
    h = m.grid_head
    assert type(h).__name__ == 'GridHead' and h.grid_points == 9 and h.conv_out_channels == 576 and h.whole_map_size == 56
    assert [tuple(c.conv.weight.shape) for c in h.convs] == [(576, 256, 3, 3)] + [(576, 576, 3, 3)] * 7
    assert [c.stride for c in h.convs] == [2] + [1] * 7 and all(c.gn.num_groups == 36 for c in h.convs)
    assert h.neighbor_points == [(1, 3), (0, 2, 4), (1, 5), (0, 4, 6), (1, 3, 5, 7), (2, 4, 8), (3, 7), (4, 6, 8), (5, 7)]
    assert h.num_edges == 24 and h.norm1.num_groups == 9
    assert not m.bbox_head.with_reg and not hasattr(m.bbox_head, 'fc_reg')
    assert m.test_cfg.score_thr == 0.03 and m.test_cfg.max_per_img == 100 and m.test_cfg.nms.iou_threshold == 0.3


def test_state_dict_keys_and_shapes_equal_the_reference(golden_dir):
    """Every key and shape is the reference's (incl. the mask_predictor block of the fork's BaseRoIHead, Quirk Q4), and a
    reference-keyed ``state_dict`` loads with ``strict=True``."""
    z = np.load(os.path.join(golden_dir, 'g23_grid.npz'))
    ref = {k: tuple(json.loads(s)) for k, s in zip(z['state_dict_keys'].tolist(), z['state_dict_shapes'].tolist())}
    m, _ = _build(golden_dir)
    sd = m.state_dict()
    assert set(sd) == set(ref)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert ref['grid_head.deconv1.weight'] == (576, 64, 4, 4) and ref['grid_head.deconv2.weight'] == (576, 1, 4, 4)
    assert ref['grid_head.deconv2.bias'] == (9,) and ref['grid_head.convs.3.gn.weight'] == (576,)
    assert ref['grid_head.forder_trans.4.3.0.weight'] == (64, 1, 5, 5)
    assert ref['grid_head.sorder_trans.8.1.1.weight'] == (64, 64, 1, 1)
    assert 'grid_head.forder_trans.0.2.0.weight' not in ref          # a corner point has two neighbours
    assert not any(k.startswith('bbox_head.fc_reg') for k in ref)
    m.load_state_dict({k: torch.zeros(s) for k, s in ref.items()}, strict=True)


def test_shared_extractor_when_none(golden_dir):
    m, _ = _build(golden_dir, grid_roi_extractor=None)
    assert m.share_roi_extractor and m.grid_roi_extractor is m.bbox_roi_extractor
    assert not any(k.startswith('grid_roi_extractor') for k in m.state_dict())


def test_mask_head_constructs(golden_dir):
    """grid_roi_head.py:159-164: a config may add a mask branch; it is the base class's."""
    m, _ = _build(golden_dir, mask_roi_extractor=dict(
        type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0), out_channels=256,
        featmap_strides=[4, 8, 16, 32]), mask_head=dict(type='FCNMaskHead', num_convs=4, in_channels=256,
                                                        conv_out_channels=256, num_classes=80))
    assert m.with_mask and type(m.mask_head).__name__ == 'FCNMaskHead'


@pytest.mark.parametrize('points', (4, 9, 16))
def test_calc_sub_regions_equal_the_reference(golden_dir, points):
    from dynamask_amd.mask_heads import grid_sub_regions
    ref = _cfgs(golden_dir)['r50_2x']['sub_regions'][str(points)]
    assert [list(r) for r in grid_sub_regions(points, 56)] == ref
    if points == 9:
        m, _ = _build(golden_dir)
        assert [list(r) for r in m.grid_head.calc_sub_regions()] == ref == [list(r) for r in m.grid_head.sub_regions]


def test_neighbour_order_is_left_up_down_right():
    from dynamask_amd import ops
    assert ops.grid_neighbors(9)[4] == (1, 3, 5, 7)
    assert ops.grid_neighbors(4) == [(1, 2), (0, 3), (0, 3), (1, 2)]


def test_bbox_head_without_regression():
    from dynamask_amd import bbox_heads
    h = bbox_heads.Shared2FCBBoxHead(with_reg=False, num_classes=80)
    keys = set(h.state_dict())
    assert not any(k.startswith('fc_reg') for k in keys) and not hasattr(h, 'fc_reg')
    assert keys == {f'{m}.{p}' for m in ('shared_fcs.0', 'shared_fcs.1', 'fc_cls') for p in ('weight', 'bias')}
    h.init_weights()
    with pytest.raises(NotImplementedError, match='with_reg=False'):
        h(torch.zeros(2, 256, 7, 7))                 # grad enabled: the training path
    assert 'fc_reg.weight' in bbox_heads.Shared2FCBBoxHead().state_dict()
    for bad in (dict(with_avg_pool=True), dict(with_cls=False), dict(norm_cfg=dict(type='GN', num_groups=32)),
                dict(reg_decoded_bbox=True)):
        with pytest.raises(NotImplementedError):
            bbox_heads.Shared2FCBBoxHead(with_reg=False, **bad)


def test_zero_detections(golden_dir):
    """No device work: an empty heatmap, empty boxes and per-class (0, 5) arrays."""
    m, _ = _build(golden_dir)
    m.eval()
    with torch.no_grad():
        out = m.grid_head(torch.zeros(0, 256, 14, 14))
    assert tuple(out['fused'].shape) == (0, 9, 28, 28) and out['unfused'] is out['fused']
    assert tuple(m.grid_head.get_bboxes(torch.zeros(0, 5), out['fused']).shape) == (0, 5)
    assert tuple(m._grid_refine(None, [torch.zeros(0, 5)]).shape) == (0, 5)
    assert tuple(m._grid_refine(None, [torch.zeros(0, 5), torch.zeros(0, 5)]).shape) == (0, 5)
    from dynamask_amd.postprocess import bbox2result
    res = bbox2result(torch.zeros(0, 5), torch.zeros(0, dtype=torch.long), 80)
    assert len(res) == 80 and all(r.shape == (0, 5) and r.dtype == np.float32 for r in res)


def test_out_of_scope_calls_raise(golden_dir):
    m, _ = _build(golden_dir)
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.forward_train(None, [], [], [], [])
    with pytest.raises(NotImplementedError, match='aug_test'):
        m.aug_test(None, [], [])
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.enable_inference_graphs(True)
    assert m.enable_inference_graphs(False) is None
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.grid_head.get_targets([], None)
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.grid_head.loss(None, None)
    m.train()
    with pytest.raises(NotImplementedError, match='eval mode'):
        m.grid_head(torch.zeros(1, 256, 14, 14))
    m.eval()
    with pytest.raises(NotImplementedError, match='eval mode'):
        m.grid_head(torch.zeros(1, 256, 14, 14, requires_grad=True))
    with torch.no_grad(), pytest.raises(ValueError, match='RoI features'):
        m.grid_head(torch.zeros(1, 256, 7, 7))
    with pytest.raises(NotImplementedError, match='does not run alone'):
        m.grid_head.forder_trans[0][0](torch.zeros(1, 64, 7, 7))


def test_unsupported_constructor_forms_raise(golden_dir):
    from dynamask_amd import losses  # noqa: F401
    from dynamask_amd.mask_heads import ConvModule, GNConvModule, GridHead
    from dynamask_amd.roi_head import GridRoIHead
    for bad in (dict(grid_points=4), dict(grid_points=16), dict(point_feat_channels=32), dict(roi_feat_size=28),
                dict(conv_kernel_size=5), dict(deconv_kernel_size=2), dict(num_convs=0), dict(in_channels=100),
                dict(conv_cfg=dict(type='ConvWS')), dict(norm_cfg=None), dict(norm_cfg=dict(type='BN'))):
        with pytest.raises(NotImplementedError):
            GridHead(**bad)
    with pytest.raises(ValueError):
        GridHead(grid_points=8)
    with pytest.raises(ValueError):
        GridHead(grid_points=1)
    with pytest.raises(ValueError):
        GridHead(roi_feat_size=(14, 14))
    with pytest.raises(ValueError):
        GridHead(norm_cfg=dict(type='GN', num_groups=7))
    for bad in (dict(norm_cfg=None), dict(norm_cfg=dict(type='BN')), dict(kernel_size=1, padding=0), dict(stride=3),
                dict(bias=False), dict(conv_cfg=dict(type='ConvWS')), dict(in_channels=12)):
        kw = dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, norm_cfg=dict(type='GN', num_groups=4))
        kw.update(bad)
        with pytest.raises(NotImplementedError):
            GNConvModule(**kw)
    with pytest.raises(NotImplementedError):          # the norm-free ConvModule still refuses a norm
        ConvModule(64, 64, 3, padding=1, norm_cfg=dict(type='GN', num_groups=4))
    with pytest.raises(ValueError, match='grid_head'):
        GridRoIHead(grid_roi_extractor=None, grid_head=None)
    rh = dict(_cfgs(golden_dir)['r50_2x']['model']['roi_head'])
    rh.pop('type')
    rh.pop('bbox_head')
    with pytest.raises(ValueError, match='bbox branch'):
        GridRoIHead(**rh)
