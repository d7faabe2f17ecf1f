"""Hybrid Task Cascade through the registry, without a GPU: the ``roi_head`` of configs/htc/htc_r50_fpn_1x_coco.py and of
htc_without_semantic_r50_fpn_1x_coco.py (as resolved from the reference tree: tests/golden/g22_htc_configs.json) build
unchanged, the module trees have the reference HybridTaskCascadeRoIHead's ``state_dict`` keys (tests/golden/g22_htc.npz),
the calls out of scope raise, and the host-side rules of the new kernels -- the resize coordinates and the RoI feature
pooling -- are those of torch."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _cfg(golden_dir, name='coco'):
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    with open(os.path.join(golden_dir, 'g22_htc_configs.json')) as f:
        cfg = registry._to_cfgdict(json.load(f)[name])
    rh = dict(cfg.model.roi_head)
    assert rh['type'] == 'HybridTaskCascadeRoIHead'
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=cfg.test_cfg.rcnn)
    return rh


def _build(golden_dir, name='coco', **over):
    from dynamask_amd import registry
    rh = _cfg(golden_dir, name)
    rh.update(over)
    return registry.build_head(rh)


def test_config_with_semantic_head_builds(golden_dir):
    m = _build(golden_dir)
    assert type(m).__name__ == 'HybridTaskCascadeRoIHead' and m.num_stages == 3 and m.with_semantic
    assert m.interleaved and m.mask_info_flow and tuple(m.semantic_fusion) == ('bbox', 'mask')
    assert [type(h).__name__ for h in m.mask_head] == ['HTCMaskHead'] * 3
    assert [h.with_conv_res for h in m.mask_head] == [False, True, True]
    sh = m.semantic_head
    assert type(sh).__name__ == 'FusedSemanticHead' and sh.num_ins == 5 and sh.fusion_level == 1 and sh.num_convs == 4
    assert tuple(sh.conv_logits.weight.shape) == (183, 256, 1, 1)
    lay = m.semantic_roi_extractor.roi_layers[0]
    assert lay.output_size == (14, 14) and lay.spatial_scale == 1 / 8 and list(m.semantic_roi_extractor.featmap_strides) == [8]
    assert m._mask_logits_size() == (80, 28) and m._segm_num_classes() == 80


def test_config_without_semantic_head_builds(golden_dir):
    """Quirk Q4: without a semantic head the 56 x 56 stride-4 extractor of the fork's BaseRoIHead stays."""
    m = _build(golden_dir, 'nosem')
    assert type(m).__name__ == 'HybridTaskCascadeRoIHead' and not m.with_semantic
    assert not hasattr(m, 'semantic_head')
    lay = m.semantic_roi_extractor.roi_layers[0]
    assert lay.output_size == (56, 56) and list(m.semantic_roi_extractor.featmap_strides) == [4]


@pytest.mark.parametrize('name,prefix', [('coco', ''), ('nosem', 'nosem_')])
def test_state_dict_keys_equal_the_reference(golden_dir, name, prefix):
    z = np.load(os.path.join(golden_dir, 'g22_htc.npz'))
    ref = set(z[prefix + 'state_dict_keys'].tolist())
    sd = _build(golden_dir, name).state_dict()
    assert set(sd) == ref
    assert any(k.startswith('mask_predictor.') for k in sd)
    assert not any(k.startswith('mask_head.0.conv_res.') for k in sd)
    assert tuple(sd['mask_head.2.conv_res.conv.weight'].shape) == (256, 256, 1, 1)
    assert any(k.startswith('semantic_head.conv_logits.') for k in sd) == (name == 'coco')


def test_registered_heads_build_alone():
    from dynamask_amd import registry, mask_heads, roi_head  # noqa: F401
    h = registry.build_head(dict(type='HTCMaskHead', with_conv_res=False, num_convs=2, in_channels=32, conv_out_channels=32,
                                 num_classes=5))
    assert not hasattr(h, 'conv_res') and h.num_convs == 2
    s = registry.build_head(dict(type='FusedSemanticHead', num_ins=3, fusion_level=0, num_convs=1, in_channels=16,
                                 conv_out_channels=24, num_classes=7))
    keys = set(s.state_dict())
    assert keys == {f'lateral_convs.{i}.conv.{p}' for i in range(3) for p in ('weight', 'bias')} | \
        {f'convs.0.conv.{p}' for p in ('weight', 'bias')} | {f'conv_embedding.conv.{p}' for p in ('weight', 'bias')} | \
        {f'conv_logits.{p}' for p in ('weight', 'bias')}
    assert tuple(s.convs[0].conv.weight.shape) == (24, 16, 3, 3)


def test_refusals(golden_dir):
    from dynamask_amd import registry
    with pytest.raises(NotImplementedError, match='htc_roi_head.py:351'):
        _build(golden_dir, mask_info_flow=False)
    with pytest.raises(NotImplementedError, match='Shared head'):
        _build(golden_dir, shared_head=dict(type='ResLayer'))
    m = _build(golden_dir)
    with pytest.raises(NotImplementedError, match='Q5'):
        m.forward_train(None, None, None, None, None)
    with pytest.raises(NotImplementedError, match='graph'):
        m.enable_inference_graphs(True)
    assert m.enable_inference_graphs(False) is None
    # semantic / RoI feature sizes that neither the identity nor the 2 x 2 mean joins
    rh = _cfg(golden_dir)
    ext = dict(rh['semantic_roi_extractor'])
    ext['roi_layer'] = dict(ext['roi_layer'], output_size=28)
    with pytest.raises(NotImplementedError, match='2 x 2'):
        _build(golden_dir, semantic_roi_extractor=ext)
    ext['roi_layer'] = dict(ext['roi_layer'], output_size=7)       # the box branch fits, the mask branch (14) does not
    with pytest.raises(NotImplementedError):
        _build(golden_dir, semantic_roi_extractor=ext)
    for bad in (dict(norm_cfg=dict(type='BN')), dict(conv_cfg=dict(type='ConvWS'))):
        with pytest.raises(NotImplementedError):
            registry.build_head(dict(type='FusedSemanticHead', num_ins=5, fusion_level=1, **bad))
    with pytest.raises(NotImplementedError, match='HTCMaskHead'):
        _build(golden_dir, mask_head=dict(type='FCNMaskHead', num_convs=4, in_channels=256, conv_out_channels=256,
                                          num_classes=80))


def test_semantic_cache_does_not_outlive_the_call(golden_dir):
    """The cache opens with the outermost public entry point and is gone after it, also when the call raises."""
    m = _build(golden_dir)
    assert m._sem_cache is None
    with pytest.raises(Exception):
        m.simple_test(None, None, None)               # (fails inside, without a device)
    assert m._sem_cache is None and m._sem_depth == 0
    with pytest.raises(Exception):
        m.aug_test_mask_probs(None, None, None, None)
    assert m._sem_cache is None and m._sem_depth == 0 and not m._aug_mask


@pytest.mark.parametrize('n_in,n_out', [(32, 16), (8, 16), (4, 16), (2, 16), (25, 13), (13, 25), (7, 7), (9, 1), (1, 5),
                                        (200, 100), (50, 100), (13, 100), (334, 168), (84, 168), (21, 168)])
def test_resize_coordinate_rule_is_interpolates(n_in, n_out):
    """ops.resize_coords (the kernel's taps, computed the same way on the host) against F.interpolate(align_corners=True)
    of a ramp and of random rows: a ramp is reproduced to fp32 rounding, random data to the interpolation's rounding."""
    from dynamask_amd import ops
    lo, hi, w = ops.resize_coords(n_in, n_out)
    assert lo.min() >= 0 and hi.max() <= n_in - 1 and ((hi == lo) | (hi == lo + 1)).all()
    assert (w >= 0).all() and (w < 1).all()
    if n_out > 1:
        assert lo[0] == 0 and w[0] == 0 and (lo[-1] + w[-1]) == pytest.approx(n_in - 1, abs=1e-4)
    else:
        assert lo[0] == 0 and w[0] == 0
    g = torch.Generator().manual_seed(n_in * 1000 + n_out)
    x = torch.randn(3, n_in, generator=g, dtype=torch.float64)
    ref = F.interpolate(x[None, :, None, :], size=(1, n_out), mode='bilinear', align_corners=True)[0, :, 0].numpy()
    xn = x.numpy()
    got = xn[:, lo] * (1.0 - w.astype(np.float64)) + xn[:, hi] * w.astype(np.float64)
    # (the weights are fp32 numbers: they differ from the float64 reference's by fp32 rounding of the coordinate)
    np.testing.assert_allclose(got, ref, atol=2e-5 * max(n_in, 1) / max(n_out, 1) + 2e-5, rtol=0)
    ref32 = F.interpolate(x.float()[None, :, None, :], size=(1, n_out), mode='bilinear', align_corners=True)[0, :, 0].numpy()
    x32 = x.float().numpy()
    got32 = x32[:, lo] * (np.float32(1) - w) + x32[:, hi] * w
    np.testing.assert_allclose(got32, ref32, atol=1e-5, rtol=1e-5)


def test_pooling_rule_is_adaptive_avg_pool():
    """ops.roi_align_pool picks the identity or the 2 x 2 mean, and the 2 x 2 mean in the kernel's order
    ((a + b) + (c + d)) * 0.25 is adaptive_avg_pool2d 14 -> 7 to fp32 rounding."""
    from dynamask_amd import ops
    assert ops.roi_align_pool(14, 14) == 1 and ops.roi_align_pool(14, 7) == 2 and ops.roi_align_pool(8, 4) == 2
    for size, out in ((14, 5), (14, 28), (7, 14), (15, 7)):
        with pytest.raises(NotImplementedError):
            ops.roi_align_pool(size, out)
    x = torch.randn(5, 8, 14, 14, generator=torch.Generator().manual_seed(3))
    ref = F.adaptive_avg_pool2d(x, (7, 7))
    got = ((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])) * 0.25
    ref64 = F.adaptive_avg_pool2d(x.double(), (7, 7))
    assert float((got.double() - ref64).abs().max()) <= max(float((ref.double() - ref64).abs().max()), 1e-6)
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)
