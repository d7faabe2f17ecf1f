"""Host-side checks of the batched inference entry points: argument and metadata validation happens before any GPU
work, the graph buckets of batched calls, and the new C-ABI entry points are declared."""
import numpy as np
import pytest
import torch


def _head():
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, synth  # noqa: F401
    from dynamask_amd.registry import ConfigDict
    return registry.build_head(dict(
        type='DynaMaskRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG), test_cfg=ConfigDict(**synth.RCNN_TEST_CFG)))


META = dict(img_shape=(64, 80, 3), ori_shape=(64, 80, 3), scale_factor=1.0)


def _x(B):
    return [torch.zeros(B, 256, 16 // s, 20 // s) for s in (1, 2, 4, 8, 16)]


def test_batch_simple_test_validates_before_any_device_work():
    m = _head()
    props = [torch.zeros(0, 4)] * 2
    with pytest.raises(ValueError, match='non-empty'):
        m.batch_simple_test(_x(2), [], [])
    with pytest.raises(ValueError, match='proposal_list: 2 entries for 3 images'):
        m.batch_simple_test(_x(3), props, [META] * 3)
    with pytest.raises(ValueError, match=r"img_metas\[1\] lacks \['ori_shape'\]"):
        m.batch_simple_test(_x(2), props, [META, dict(img_shape=(64, 80, 3), scale_factor=1.0)])
    with pytest.raises(ValueError, match='batch dimension 3 for 2 images'):
        m.batch_simple_test(_x(3), props, [META] * 2)
    with pytest.raises(ValueError, match='det_labels_list: 1 entries for 2 images'):
        m.batch_simple_test_mask(_x(2), [META] * 2, [torch.zeros(0, 5)] * 2, [torch.zeros(0, dtype=torch.long)])
    with pytest.raises(ValueError, match='rescale=True needs scale_factors'):
        m.batch_simple_test_mask_logits(_x(2), [torch.zeros(0, 5)] * 2, [torch.zeros(0, dtype=torch.long)] * 2,
                                        rescale=True)


def test_batch_empty_detections_need_no_device():
    """No detection in any image: the empty per-class lists of simple_test_mask, without a launch."""
    m = _head()
    dets = [torch.zeros(0, 5)] * 3
    labs = [torch.zeros(0, dtype=torch.long)] * 3
    assert m.batch_simple_test_mask(_x(3), [META] * 3, dets, labs) == [[[] for _ in range(80)] for _ in range(3)]
    z, offs = m.batch_simple_test_mask_logits(_x(3), dets, labs, [1.0, np.ones(4, np.float32), 0.5], rescale=True)
    assert z.shape == (0, 1, 112, 112) and offs == [0, 0, 0, 0]


def test_batch_graph_buckets_extend_the_single_image_ones():
    from dynamask_amd import graphs
    assert graphs.BUCKETS == (16, 24, 32, 48, 64, 80, 100)
    assert graphs.BATCH_BUCKETS[:len(graphs.BUCKETS)] == graphs.BUCKETS
    assert list(graphs.BATCH_BUCKETS) == sorted(set(graphs.BATCH_BUCKETS)) and graphs.BATCH_BUCKETS[-1] >= 400


def test_multi_image_entry_points_are_declared():
    import os
    from dynamask_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dynamask_hip.h')).read()
    for name in ('dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_paste_masks_multi', 'dm_paste_rle_multi',
                 'dm_rle_multi_scratch_ints'):
        assert name in _lib.SIGNATURES and f'{name}(' in hdr
