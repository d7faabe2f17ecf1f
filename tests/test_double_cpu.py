"""Double-Head R-CNN without a GPU: the registry builds DoubleHeadRoIHead / DoubleConvFCBBoxHead from the unchanged config
(tests/golden/g24_double_configs.json: the config as resolved, and the reference module's state_dict list), the eval-mode
BatchNorm fold against float64 conv -> BatchNorm on the CPU, its refresh, the RoI rescale arithmetic, the refusals, and the
launcher's own report (dm_conv2d_plan, no device) of the builds the head's five convolution shapes take."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64


@pytest.fixture(scope='module')
def cfg(golden_dir):
    with open(os.path.join(golden_dir, 'g24_double_configs.json')) as f:
        return json.load(f)['dh_r50_1x']


@pytest.fixture(scope='module')
def roi_head(cfg):
    from dynamask_amd import registry, roi_head, bbox_heads, losses, roi_extractors  # noqa: F401
    c = registry._to_cfgdict(cfg)
    rh = dict(c.model.roi_head)
    rh.update(train_cfg=None, test_cfg=c.test_cfg.rcnn)
    return registry.build_head(rh)


def _small_head():
    import double_inputs as di
    from dynamask_amd import bbox_heads
    h = bbox_heads.DoubleConvFCBBoxHead(num_convs=1, num_fcs=1, in_channels=16, conv_out_channels=32, fc_out_channels=8,
                                        num_classes=3)
    h.load_state_dict(di.head_state({k: v.shape for k, v in h.state_dict().items()}, 5), strict=True)
    return h.eval()


def test_builds_from_the_config(cfg, roi_head):
    from dynamask_amd import bbox_heads
    from dynamask_amd import roi_head as rh
    assert cfg['source'] == 'configs/double_heads/dh_faster_rcnn_r50_fpn_1x_coco.py'
    assert type(roi_head) is rh.DoubleHeadRoIHead and isinstance(roi_head, rh.StandardRoIHead)
    assert roi_head.reg_roi_scale_factor == 1.3 and not roi_head.with_mask
    b = roi_head.bbox_head
    assert type(b) is bbox_heads.DoubleConvFCBBoxHead
    assert (b.num_convs, b.num_fcs, b.conv_out_channels, b.fc_out_channels, b.num_classes) == (4, 2, 1024, 1024, 80)
    assert b.with_avg_pool and b.roi_feat_size == (7, 7) and b.bbox_coder.stds == (0.1, 0.1, 0.2, 0.2)
    # only _bbox_forward and forward_train are the class's own: the test entry points are the template's
    own = set(vars(rh.DoubleHeadRoIHead)) - {'__module__', '__doc__', '__init__'}
    assert own == {'_bbox_forward', 'forward_train'}


def test_state_dict_is_the_references(cfg, roi_head):
    import double_inputs as di
    want = [(k, tuple(s)) for k, s in cfg['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in roi_head.state_dict().items()]
    assert sorted(got) == sorted(want)
    keys = dict(got)
    assert keys['bbox_head.fc_reg.weight'] == (320, 1024) and keys['bbox_head.fc_cls.weight'] == (81, 1024)
    assert keys['bbox_head.fc_branch.0.weight'] == (1024, 256 * 49)
    assert 'bbox_head.res_block.conv_identity.conv.bias' not in keys
    b = roi_head.bbox_head
    state = di.head_state({k: v.shape for k, v in b.state_dict().items()}, 25)
    res = b.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(b.conv_branch[3].bn3.running_var, state['conv_branch.3.bn3.running_var'])


def test_constructor_asserts_and_refusals():
    from dynamask_amd.bbox_heads import DoubleConvFCBBoxHead as H
    for bad in (dict(num_convs=0, num_fcs=2), dict(num_convs=4, num_fcs=0), dict(num_convs=1, num_fcs=1, with_avg_pool=False)):
        with pytest.raises(AssertionError):
            H(**bad)
    with pytest.raises(NotImplementedError):
        H(num_convs=1, num_fcs=1, conv_cfg=dict(type='ConvWS'))
    with pytest.raises(NotImplementedError):
        H(num_convs=1, num_fcs=1, norm_cfg=dict(type='GN', num_groups=32))
    with pytest.raises(NotImplementedError):
        H(num_convs=1, num_fcs=1, norm_cfg=None)


def _conv_bn(x, w, bn, dtype):
    y = F.conv2d(x.to(dtype), w.detach().to(dtype), padding=w.shape[-1] // 2)
    return F.batch_norm(y, bn.running_mean.to(dtype), bn.running_var.to(dtype), bn.weight.detach().to(dtype),
                        bn.bias.detach().to(dtype), False, 0.0, bn.eps)


def test_bn_fold_equals_conv_then_batchnorm():
    """conv -> BatchNorm(eval) in float64 against the folded convolution in float32, with the running statistics of
    double_inputs.head_state (variances in [0.5, 1.5]): the 3x3 layer, a 1x1 layer, and the merged [W2' | Wid'] layer."""
    h = _small_head()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 16, 7, 7, generator=g)
    hmid = torch.randn(3, 16, 7, 7, generator=g)
    x32 = torch.randn(3, 32, 7, 7, generator=g)
    rb, bt = h.res_block, h.conv_branch[0]
    assert not torch.equal(rb.conv1.bn.running_var, torch.ones(16))
    # 3x3
    w, b = rb._f1.folded()
    assert w.dtype == torch.float32 and w.shape == (16, 16, 3, 3) and b.shape == (16,)
    assert_close_via_f64(F.conv2d(x, w, b, padding=1), _conv_bn(x, rb.conv1.conv.weight, rb.conv1.bn, torch.float32),
                         _conv_bn(x, rb.conv1.conv.weight, rb.conv1.bn, torch.float64), '3x3 fold')
    # 1x1 (the bottleneck's first)
    w, b = bt._f[0].folded()
    assert w.shape == (8, 32, 1, 1)
    assert_close_via_f64(F.conv2d(x32, w, b), _conv_bn(x32, bt.conv1.weight, bt.bn1, torch.float32),
                         _conv_bn(x32, bt.conv1.weight, bt.bn1, torch.float64), '1x1 fold')
    # merged: bn(conv2(h)) + bn(conv_identity(x)) as one convolution of cat([h, x])
    w, b = rb._f2.folded()
    assert w.shape == (32, 32, 1, 1)
    ref = {d: _conv_bn(hmid, rb.conv2.conv.weight, rb.conv2.bn, d) + _conv_bn(x, rb.conv_identity.conv.weight, rb.conv_identity.bn, d)
           for d in (torch.float32, torch.float64)}
    assert_close_via_f64(F.conv2d(torch.cat([hmid, x], 1), w, b), ref[torch.float32], ref[torch.float64], 'merged fold')
    # without the fold the answer is far away: the comparison above can fail
    with pytest.raises(AssertionError):
        assert_close_via_f64(F.conv2d(x, rb.conv1.conv.weight.detach(), padding=1),
                             _conv_bn(x, rb.conv1.conv.weight, rb.conv1.bn, torch.float32),
                             _conv_bn(x, rb.conv1.conv.weight, rb.conv1.bn, torch.float64), 'no fold')


def test_bn_fold_is_float64_rounded_once():
    from dynamask_amd.layers import fold_bn
    h = _small_head()
    c, bn = h.res_block.conv1.conv, h.res_block.conv1.bn
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w, b = fold_bn([(c.weight, bn)])
    assert torch.equal(w, (c.weight.detach().double() * s[:, None, None, None]).float())
    assert torch.equal(b, (bn.bias.detach().double() - bn.running_mean.double() * s).float())


def test_fold_is_refreshed_when_a_parameter_or_buffer_changes():
    import double_inputs as di
    from dynamask_amd.layers import fold_bn
    h = _small_head()
    f = h.conv_branch[0]._f[2]
    w0, b0 = f.folded()
    assert f.folded()[0] is w0                                    # cached
    h.load_state_dict(di.head_state({k: v.shape for k, v in h.state_dict().items()}, 6), strict=True)
    w1, b1 = f.folded()
    assert not torch.equal(w1, w0) and not torch.equal(b1, b0)
    want = fold_bn([(h.conv_branch[0].conv3.weight, h.conv_branch[0].bn3)])
    assert torch.equal(w1, want[0]) and torch.equal(b1, want[1])
    with torch.no_grad():
        h.conv_branch[0].bn3.running_mean.add_(1.0)               # a buffer alone
    w2, b2 = f.folded()
    assert torch.equal(w2, w1) and not torch.equal(b2, b1)
    with torch.no_grad():
        h.conv_branch[0].bn3.weight.mul_(2.0)                     # a parameter alone
    assert torch.equal(f.folded()[0], w1.double().mul(2.0).float())


def _rescale_np(rois, f):
    """The reference formula (base_roi_extractor.py:57-80) with every operation rounded to float32 by numpy."""
    r = rois.numpy().astype(np.float32)
    f, half = np.float32(f), np.float32(0.5)
    cx, cy = (r[:, 1] + r[:, 3]) * half, (r[:, 2] + r[:, 4]) * half
    new_w, new_h = (r[:, 3] - r[:, 1]) * f, (r[:, 4] - r[:, 2]) * f
    return np.stack([r[:, 0], cx - new_w * half, cy - new_h * half, cx + new_w * half, cy + new_h * half], 1)


def test_rescale_arithmetic_bit_for_bit():
    import double_inputs as di
    from dynamask_amd.roi_extractors import BaseRoIExtractor
    from oracle import ref_ops
    g = torch.Generator().manual_seed(3)
    boxes = torch.cat([di.proposals(), torch.rand(500, 4, generator=g) * 300.0 - 20.0])
    rois = torch.cat([torch.zeros(len(boxes), 1), boxes], 1)
    for f in (1.3, 0.7, 2.0):
        got = BaseRoIExtractor.roi_rescale(rois, f)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), _rescale_np(rois, f)), f
    # the hand-written boxes do what their names say
    hand = torch.cat([torch.zeros(len(di.HAND_BOXES), 1), di.hand_boxes()], 1)
    scaled = BaseRoIExtractor.roi_rescale(hand, di.REG_ROI_SCALE_FACTOR)
    lv, lv_scaled = ref_ops.map_roi_levels(hand, 4, di.FINEST_SCALE), ref_ops.map_roi_levels(scaled, 4, di.FINEST_SCALE)
    i0, i1 = di.hand_index('level_0_not_1'), di.hand_index('level_1_not_2')
    assert (int(lv[i0]), int(lv_scaled[i0])) == (0, 1) and (int(lv[i1]), int(lv_scaled[i1])) == (1, 2)
    two = scaled[di.hand_index('leaves_two_sides')]
    assert two[1] < 0 and two[2] < 0 and two[3] < di.IMG_W and two[4] < di.IMG_H
    br = scaled[di.hand_index('bottom_right')]
    assert br[3] > di.IMG_W and br[4] > di.IMG_H


def test_training_is_refused(roi_head):
    h = _small_head()
    x = torch.zeros(2, 16, 7, 7)
    with pytest.raises(NotImplementedError, match='training'):
        h(x, x)
    with pytest.raises(NotImplementedError, match='training'):
        roi_head.forward_train(None, None, None, None, None)


def test_extractors_and_the_factor():
    from dynamask_amd import ops, roi_extractors
    gen = roi_extractors.GenericRoIExtractor(roi_layer=dict(type='SimpleRoIAlign', output_size=14), out_channels=256,
                                             featmap_strides=[4])
    with pytest.raises(NotImplementedError):
        gen([torch.zeros(1, 256, 8, 8)], torch.zeros(1, 5), roi_scale_factor=1.3)
    single = roi_extractors.SingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                               out_channels=256, featmap_strides=[4, 8, 16, 32])
    feats = [torch.zeros(1, 256, 8, 8) for _ in range(4)]
    assert tuple(single(feats, torch.zeros(0, 5), roi_scale_factor=1.3).shape) == (0, 256, 7, 7)
    with pytest.raises(RuntimeError, match='no CPU fallback'):      # the factor reaches the operator, which wants the GPU
        single(feats, torch.zeros(2, 5), roi_scale_factor=1.3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.global_avg_pool(torch.zeros(2, 4, 7, 7))


def _builds(name, nb):
    import double_inputs as di
    from dynamask_amd import ops
    src, cout, k, acc = di.CONV_SHAPES[name]
    recs = ops.conv2d_plan(list(src), nb, 7, 7, cout, k, relu=True, accumulate=acc)
    return {tuple(r[f] for f in ops.CONV_PLAN_FIELDS[:9]) for r in recs}


@pytest.mark.parametrize('name', ['res_conv1_3x3', 'res_merged_1x1', 'bottleneck_conv1_1x1', 'bottleneck_conv2_3x3',
                                  'bottleneck_conv3_1x1_accumulate'])
def test_gpu_test_sizes_reach_every_build_of_the_1000_roi_call(name):
    """dm_conv2d_plan needs no device: the launcher takes every one of the head's five shapes, and the RoI counts
    tests/test_double_gpu.py runs select, between them, every build (record ints 0-8: kernel size, tile, K chunk, tail,
    precision, epilogue) that the 1000-RoI call selects -- at the smallest count that does."""
    import double_inputs as di
    nbs = di.CONV_TEST_NBS[name]
    assert 3 in nbs
    at_1000 = _builds(name, 1000)
    assert at_1000 and at_1000 <= set().union(*[_builds(name, nb) for nb in nbs])
    for nb in nbs:
        if nb > 3:
            assert _builds(name, nb) != _builds(name, nb - 1), f'{nb} is not the smallest count of its build'
