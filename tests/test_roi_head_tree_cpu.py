"""The RoI heads' class tree, without a GPU: StandardRoIHead is the base of the other three heads (as in the reference),
holds none of DynaMask's own methods, and defines the mask-test entry points once for all four; its empty mask results
have the shape of a non-empty call."""
import pytest
import torch

SHARED = ('simple_test_mask', 'batch_simple_test_mask_logits', 'batch_simple_test_mask', 'aug_test_mask_probs',
          'aug_test_mask')


def _classes():
    from dynamask_amd import roi_head
    return roi_head.StandardRoIHead, roi_head.DynaMaskRoIHead, roi_head.RefineRoIHead, roi_head.PointRendRoIHead


def _standard_head():
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, synth  # noqa: F401
    from dynamask_amd.registry import ConfigDict
    return registry.build_head(dict(
        type='StandardRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG), test_cfg=ConfigDict(**synth.RCNN_TEST_CFG)))


def test_standard_roi_head_is_the_base_of_every_head():
    standard, *others = _classes()
    for cls in others:
        assert standard in cls.__mro__
    assert standard.__mro__[1] is torch.nn.Module


def test_standard_roi_head_has_no_dynamask_method():
    standard, dynamask, refine, pointrend = _classes()
    for name in ('dynamic_mask_logits', 'dynamic_test_mask', 'get_mask_label', 'merge_stage_preds', '_mask_forward_infer'):
        assert not hasattr(standard, name), name
        assert hasattr(dynamask, name), name
    assert not hasattr(refine, 'dynamic_mask_logits') and not hasattr(pointrend, 'dynamic_mask_logits')
    # the stage merge is shared by DynaMask and RefineMask, not copied
    assert refine.merge_stage_preds is dynamask.merge_stage_preds


def test_mask_test_entry_points_are_defined_once():
    for cls in _classes():
        for name in SHARED:
            assert getattr(cls, name).__qualname__.startswith('StandardRoIHead.'), (cls.__name__, name)


def test_graph_capture_is_dynamask_only():
    m = _standard_head()
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.enable_inference_graphs(True)
    assert m.enable_inference_graphs(False) is None


def test_standard_empty_results_have_the_shape_of_a_non_empty_call():
    """FCNMaskHead (deconv x2 of the 14 x 14 RoI features, 80 classes): logits [n, 80, 28, 28], merged TTA probabilities
    of the label channel [n, 1, 28, 28] -- and [0, ...] of the same C and S without a detection (no device needed)."""
    import numpy as np
    m = _standard_head()
    assert m._mask_logits_size() == (80, 28) and m._segm_num_classes() == 80
    x = [torch.zeros(2, 256, 16 // s, 20 // s) for s in (1, 2, 4, 8, 16)]
    dets, labs = [torch.zeros(0, 5)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    z, offs = m.batch_simple_test_mask_logits(x, dets, labs, [1.0, np.ones(4, np.float32)], rescale=True)
    assert tuple(z.shape) == (0, 80, 28, 28) and offs == [0, 0, 0]
    assert tuple(m.simple_test_mask_logits([f[:1] for f in x], dets[0], labs[0]).shape) == (0, 80, 28, 28)
    meta = [dict(img_shape=(64, 80, 3), ori_shape=(64, 80, 3), scale_factor=1.0, flip=False, flip_direction=None)]
    probs = m.aug_test_mask_probs([[f[:1] for f in x]], [meta], dets[0], labs[0])
    assert tuple(probs.shape) == (0, 1, 28, 28)
