"""PointRefine through the registry, without a GPU: the ``roi_head`` of configs/point_refine (as resolved from the
reference tree: tests/golden/g20_pointrefine_configs.json) builds, the module tree has the reference PointRefineRoIHead's
``state_dict`` keys in the reference's order (tests/golden/g20_pointrefine.npz), and the forms the kernels do not cover,
training and graph capture raise."""
import json
import os

import numpy as np
import pytest


def _cfg(golden_dir):
    from dynamask_amd import registry
    with open(os.path.join(golden_dir, 'g20_pointrefine_configs.json')) as f:
        return registry._to_cfgdict(json.load(f)['coco'])


def _build(golden_dir):
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _cfg(golden_dir)
    rh = dict(cfg.model.roi_head)
    assert rh['type'] == 'PointRefineRoIHead' and rh['mask_head']['type'] == 'PointRefineMaskHead'
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=cfg.test_cfg.rcnn)
    return registry.build_head(rh), cfg


def _head_kwargs(golden_dir, **over):
    kw = dict(_cfg(golden_dir).model.roi_head.mask_head)
    kw.pop('type')
    kw.update(over)
    return kw


def test_config_builds(golden_dir):
    m, cfg = _build(golden_dir)
    assert type(m).__name__ == 'PointRefineRoIHead'
    h = m.mask_head
    assert type(h).__name__ == 'PointRefineMaskHead'
    assert len(h.stages) == 3 and [st.channels for st in h.stages] == [256, 128, 64]
    assert h.mask_use_sigmoid and h.num_fcs == 2
    assert m.test_cfg.num_points == 784
    assert m._mask_logits_size() == (1, 112) and m._segm_num_classes() == 80
    # the loss config is kept, not built (Quirk Q15)
    assert h.loss_cfg['type'] == 'PointRefineCrossEntropyLoss' and not hasattr(h, 'loss_func')


def test_state_dict_keys_and_order_equal_the_reference(golden_dir):
    """Every key of the reference's PointRefineRoIHead, incl. the fork's mask_predictor block (Quirk Q4); the mask
    branch and the mask_predictor block in the reference's order, the branches in the reference's order (the shared
    Shared2FCBBoxHead orders its own four parameters differently, as for every RoI head here); the point MLP layers are
    Conv1d weights [C, C + 160, 1]."""
    import itertools
    z = np.load(os.path.join(golden_dir, 'g20_pointrefine.npz'))
    ref = z['state_dict_keys'].tolist()
    m, _ = _build(golden_dir)
    mine = list(m.state_dict().keys())
    assert set(mine) == set(ref) and len(mine) == len(ref)
    for pre in ('mask_head.', 'mask_predictor.'):
        assert [k for k in mine if k.startswith(pre)] == [k for k in ref if k.startswith(pre)]
    top = lambda keys: [k for k, _ in itertools.groupby(k.split('.')[0] for k in keys)]  # noqa: E731
    assert top(mine) == top(ref)
    sd = m.state_dict()
    for i, c in enumerate((256, 128, 64)):
        for j in range(2):
            assert tuple(sd[f'mask_head.stages.{i}.fcs.{j}.conv.weight'].shape) == (c, c + 160, 1)
        assert tuple(sd[f'mask_head.stages.{i}.fc_logits.weight'].shape) == (c, c + 160, 1)
        assert tuple(sd[f'mask_head.stages.{i}.semantic_transform_in.weight'].shape) == (c, 256, 1, 1)
        assert tuple(sd[f'mask_head.stages.{i}.fuse_transform_out.weight'].shape) == (c // 2, c, 1, 1)
    assert tuple(sd['mask_head.final_instance_logits.weight'].shape) == (80, 32, 1, 1)


def test_unsupported_forms_raise(golden_dir):
    from dynamask_amd import mask_heads
    with pytest.raises(NotImplementedError, match='class_agnostic'):
        mask_heads.PointRefineMaskHead(**_head_kwargs(golden_dir, class_agnostic=True))
    with pytest.raises(NotImplementedError, match='coarse_pred_each_layer'):
        mask_heads.PointRefineMaskHead(**_head_kwargs(golden_dir, coarse_pred_each_layer=False))
    with pytest.raises(NotImplementedError, match='odd'):
        mask_heads.PointRefineMaskHead(**_head_kwargs(golden_dir, conv_out_channels_instance=254))
    with pytest.raises(NotImplementedError, match='even width'):
        mask_heads.PointRefineSFMStage(semantic_out_channel=63, fc_in_channels=63, fc_channels=63)
    with pytest.raises(NotImplementedError):
        mask_heads.PointRefineMaskHead(**_head_kwargs(golden_dir, upsample_cfg=dict(type='deconv', scale_factor=2)))


def test_training_and_graphs_raise(golden_dir):
    m, _ = _build(golden_dir)
    with pytest.raises(NotImplementedError, match='Q15'):
        m.forward_train(None, [{}], None, None, None)
    with pytest.raises(NotImplementedError, match='Q15'):
        m.mask_head.loss()
    with pytest.raises(NotImplementedError, match='Q15'):
        m.mask_head.get_targets()
    with pytest.raises(NotImplementedError):
        m.enable_inference_graphs(True)
