"""RefineMask through the registry, without a GPU: the COCO, Cityscapes and LVIS ``roi_head`` sections of
configs/refinemask (as resolved from the reference tree: tests/golden/g17_refine_configs.json) build unchanged, the
module tree has the reference RefineRoIHead's ``state_dict`` keys (tests/golden/g17_refine.npz), and the calls that
belong to the training follow-up raise NotImplementedError."""
import json
import os

import numpy as np
import pytest


def _build(golden_dir, name):
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    with open(os.path.join(golden_dir, 'g17_refine_configs.json')) as f:
        cfg = registry._to_cfgdict(json.load(f)[name])
    rh = dict(cfg.model.roi_head)
    assert rh['type'] == 'RefineRoIHead' and rh['mask_head']['type'] == 'RefineMaskHead'
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=cfg.test_cfg.rcnn)
    return registry.build_head(rh), cfg


@pytest.mark.parametrize('name,classes', (('coco', 80), ('cityscapes', 8), ('lvis', 1203)))
def test_configs_build_unchanged(golden_dir, name, classes):
    m, cfg = _build(golden_dir, name)
    assert type(m).__name__ == 'RefineRoIHead' and type(m.mask_head).__name__ == 'RefineMaskHead'
    h = m.mask_head
    assert h.stage_num_classes[0] == classes and h.stage_sup_size == [14, 28, 56, 112]
    assert h.stage_num_classes[-1] == (1 if name == 'lvis' else classes)
    assert type(h.loss_func).__name__ == 'RefineCrossEntropyLoss' and h.loss_func.start_stage == 1
    assert m.with_bbox and m.with_mask and m.test_cfg.mask_thr_binary == 0.5
    assert m._segm_num_classes() == classes
    # MultiBranchFusion at every stage: 256 @14, 128 @28, 64 @56, dilations 1 / 3 / 5
    for stage, (c, s) in zip(h.stages, ((256, 14), (128, 28), (64, 56))):
        mbf = stage.fuse_conv[1]
        assert stage.out_size == s and mbf.feat_dim == c and mbf.dilations == [1, 3, 5]
        assert [b.dilation for b in mbf.branches()] == [1, 3, 5]


def test_state_dict_keys_equal_the_reference(golden_dir):
    """The mask branch's keys are the reference RefineRoIHead's, incl. the mask_predictor block of the fork's
    BaseRoIHead (Quirk Q4); the bbox branch carries Shared2FCBBoxHead's keys."""
    z = np.load(os.path.join(golden_dir, 'g17_refine.npz'))
    ref = set(z['state_dict_keys'].tolist())
    m, _ = _build(golden_dir, 'coco')
    keys = set(m.state_dict())
    assert {k for k in keys if not k.startswith('bbox_head.')} == ref
    assert {k for k in keys if k.startswith('bbox_head.')} == {'bbox_head.' + k for k in (
        'shared_fcs.0.weight', 'shared_fcs.0.bias', 'shared_fcs.1.weight', 'shared_fcs.1.bias', 'fc_cls.weight', 'fc_cls.bias',
        'fc_reg.weight', 'fc_reg.bias')}
    for k in ('mask_head.stages.0.fuse_conv.1.dilation_conv_3.conv.weight', 'mask_head.stages.2.fuse_conv.1.merge_conv.conv.bias',
              'mask_head.semantic_convs.3.conv.weight', 'mask_head.semantic_logits.weight', 'mask_predictor.fc2.weight'):
        assert k in keys
    assert tuple(m.state_dict()['mask_head.stages.1.fuse_conv.1.dilation_conv_2.conv.weight'].shape) == (128, 128, 3, 3)


def test_out_of_scope_calls_raise(golden_dir):
    m, _ = _build(golden_dir, 'coco')
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.forward_train(None, [], [], [], [])
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.enable_inference_graphs()
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.mask_head.loss_func(None, None, None, None)
    with pytest.raises(NotImplementedError, match='follow-up'):
        m.mask_head.loss(None, None, None, None)
    assert m.enable_inference_graphs(False) is None


def test_unsupported_constructor_arguments_raise():
    from dynamask_amd import mask_heads
    with pytest.raises(NotImplementedError):
        mask_heads.MultiBranchFusion(64, dilations=[1, 3])
    with pytest.raises(NotImplementedError):
        mask_heads.DilatedConvModule(64, 64, 3, padding=1, dilation=9)
    with pytest.raises(NotImplementedError):
        mask_heads.RefineSFMStage(fusion_type='MultiBranchFusionAvg')
