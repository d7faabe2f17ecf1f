"""ResNeXt without a device: the registry builds ``backbones.ResNeXt`` from the reference's unchanged x101 configs
(tests/golden/g30_resnext_configs.json) with the reference's keys and shapes, the widths, the flags ``ResNet`` keeps, the
refusals, the five whole detectors with ``load_checkpoint``, the default ``Bottleneck``'s draws against the recorded
digest, and the host side of the grouped kernel: the weight layout and ``dm_conv3x3_grouped_supported``."""
import copy
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ['x101_32x4d', 'x101_64x4d', 'x101_32x8d']
DETECTORS = {'mask_rcnn_x101_32x4d': 'MaskRCNN', 'mask_rcnn_x101_64x4d': 'MaskRCNN', 'mask_rcnn_x101_32x8d': 'MaskRCNN',
             'cascade_x101_32x4d': 'CascadeRCNN', 'htc_x101_64x4d': 'HybridTaskCascade'}
# conv2's channels per stage, and its groups
WIDTHS = {'x101_32x4d': ([128, 256, 512, 1024], 32), 'x101_64x4d': ([256, 512, 1024, 2048], 64),
          'x101_32x8d': ([256, 512, 1024, 2048], 32)}


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g30_resnext_configs.json')) as f:
        return json.load(f)


def _build(cfg):
    from dynamask_amd import backbones, registry  # noqa: F401
    return registry.build_backbone(copy.deepcopy(cfg))


# ------------------------------------------------------------------------------------------------ the backbone
def test_fixture_has_the_shape_the_digest_tool_expects(cfgs):
    """Per-part entries hold a depth-101 backbone and nothing else (tools/module_digest.py records depth 50 only); every
    other entry is a whole detector, ``type`` included."""
    assert set(cfgs) == set(PARTS) | set(DETECTORS)
    for name in PARTS:
        assert set(cfgs[name]['model']) == {'backbone'} and cfgs[name]['model']['backbone']['depth'] == 101
        assert cfgs[name]['model']['backbone']['type'] == 'ResNeXt'
    for name, typ in DETECTORS.items():
        assert cfgs[name]['model']['type'] == typ and set(cfgs[name]['test_cfg']) == {'rpn', 'rcnn'}


@pytest.mark.parametrize('name', PARTS)
def test_registry_builds_resnext_with_the_references_keys(cfgs, name):
    import resnext_inputs as xi
    import dynamask_amd
    from dynamask_amd import backbones, layers
    cfg = cfgs[name]['model']['backbone']
    before = copy.deepcopy(cfg)
    m = _build(cfg)
    assert cfg == before
    assert type(m) is backbones.ResNeXt and isinstance(m, backbones.ResNet) and dynamask_amd.ResNeXt is backbones.ResNeXt
    assert dynamask_amd.BACKBONES.get('ResNeXt') is backbones.ResNeXt
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == cfgs[name]['state_dict']
    assert [[k, list(s)] for k, s in xi.state_shapes(cfg).items()] == cfgs[name]['state_dict']
    widths, groups = WIDTHS[name]
    assert xi.widths(cfg) == widths and (m.groups, m.base_width) == (groups, cfg['base_width'])
    for i, w in enumerate(widths):
        blocks = getattr(m, f'layer{i + 1}')
        assert len(blocks) == (3, 4, 23, 3)[i]
        for j, b in enumerate(blocks):
            assert isinstance(b, layers.Bottleneck) and (b.width, b.groups) == (w, groups)
            assert tuple(b.conv2.weight.shape) == (w, w // groups, 3, 3)
            assert tuple(b.conv1.weight.shape) == (w, b.inplanes, 1, 1) and tuple(b.conv3.weight.shape) == (256 * 2 ** i, w, 1, 1)
            assert b.stride == (2 if j == 0 and i > 0 else 1) and (b.downsample is not None) == (j == 0)
    # what ResNet keeps, ResNeXt keeps
    assert m.feat_dim == 2048 and m.res_layers == ['layer1', 'layer2', 'layer3', 'layer4'] and m.frozen_stages == 1
    assert tuple(m.out_indices) == (0, 1, 2, 3) and m.style == cfg['style'] and m.norm1 is m.bn1
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    stem_and_layer1 = [k for k, _ in m.named_parameters() if k.startswith(('conv1.', 'bn1.', 'layer1.'))]
    if cfg['norm_cfg'].get('requires_grad', True):
        assert frozen == stem_and_layer1
    else:                       # the 32x8d form: every BatchNorm parameter is frozen too
        assert name == 'x101_32x8d'
        assert set(frozen) == set(stem_and_layer1) | {k for k, _ in m.named_parameters() if '.bn' in k or '.downsample.1.' in k}
        assert all(p.requires_grad for k, p in m.named_parameters() if k.startswith('layer2.') and '.conv' in k)


def test_groups_1_is_resnet(cfgs):
    from dynamask_amd import backbones
    torch.manual_seed(5)
    a = backbones.ResNeXt(depth=50, groups=1)
    torch.manual_seed(5)
    b = backbones.ResNet(depth=50)
    sa, sb = a.state_dict(), b.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sa.items()] == [(k, tuple(v.shape)) for k, v in sb.items()]
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(blk.groups == 1 and blk.width == blk.planes for blk in a.modules() if isinstance(blk, backbones.Bottleneck))
    assert backbones.ResNeXt.arch_settings[101][1] == (3, 4, 23, 3) and sorted(backbones.ResNeXt.arch_settings) == [50, 101, 152]


def test_default_bottleneck_draws_what_it_drew_before(golden_dir):
    """The blocks with default ``groups`` construct the same modules in the same order with the same draws: the ResNet-50
    section and the C4 shared head (``ResLayer``) still have their recorded digests -- here built through ``ResNeXt`` at
    ``groups=1`` and through ``Bottleneck()`` itself."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import module_digest
    from dynamask_amd import backbones, layers
    with open(module_digest.FIXTURE) as f:
        recorded = json.load(f)
    with open(os.path.join(golden_dir, 'g28_backbone_configs.json')) as f:
        cfg = json.load(f)['pytorch']['model']['backbone']
    cfg = {k: v for k, v in cfg.items() if k != 'type'}
    got = module_digest.digest(lambda: backbones.ResNeXt(groups=1, **copy.deepcopy(cfg)))
    assert got == recorded['g28_backbone/pytorch/backbone']
    # one block: the draws of Bottleneck(inplanes, planes) are those of the three holders in order
    torch.manual_seed(3)
    blk = layers.Bottleneck(64, 16, downsample=True)
    torch.manual_seed(3)
    want = [layers._conv_weight(16, 64, 1), layers._conv_weight(16, 16, 3), layers._conv_weight(64, 16, 1), layers._conv_weight(64, 64, 1)]
    for a, b in zip((blk.conv1, blk.conv2, blk.conv3, blk.downsample[0]), want):
        assert torch.equal(a.weight, b.weight)
    assert list(blk.state_dict())[:1] == ['conv1.weight'] and blk.groups == 1 and blk.width == 16


def test_what_is_not_built_raises_by_name():
    from dynamask_amd import backbones
    with pytest.raises(NotImplementedError, match=r'groups=32, base_width=3 .* 3 channels per group'):
        backbones.ResNeXt(depth=50, groups=32, base_width=3)
    with pytest.raises(NotImplementedError, match=r'groups=3, base_width=4'):
        backbones.ResNeXt(depth=50, groups=3)
    with pytest.raises(NotImplementedError, match=r'groups=32, base_width=32 .* 128 channels per group'):
        backbones.ResNeXt(depth=50, groups=32, base_width=32, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1), out_indices=(2,))
    with pytest.raises(NotImplementedError, match='depth=18'):
        backbones.ResNeXt(depth=18, groups=32)
    with pytest.raises(NotImplementedError, match='dcn='):
        backbones.ResNeXt(depth=101, groups=32, dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False),
                          stage_with_dcn=(False, True, True, True))
    with pytest.raises(NotImplementedError, match='deep_stem'):
        backbones.ResNeXt(depth=50, groups=32, deep_stem=True)
    with pytest.raises(KeyError, match='invalid depth'):
        backbones.ResNeXt(depth=51, groups=32)
    m = backbones.ResNeXt(depth=50, groups=32, base_width=4)
    with pytest.raises(NotImplementedError, match='training'):
        m(torch.zeros(1, 3, 32, 32))


# ------------------------------------------------------------------------------------------------ the detectors
@pytest.mark.parametrize('name', sorted(DETECTORS))
def test_build_detector_and_load_checkpoint(cfgs, golden_dir, name):
    import dynamask_amd
    from dynamask_amd import backbones, detectors
    cfg = cfgs[name]
    before = copy.deepcopy(cfg)
    det = dynamask_amd.build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert cfg == before, 'the build changed the caller\'s config'
    assert type(det) is getattr(detectors, DETECTORS[name]) and type(det.backbone) is backbones.ResNeXt
    assert det.pretrained == cfg['model']['pretrained'] and det.pretrained.startswith('open-mmlab://')
    assert det.with_neck and det.with_rpn and det.with_mask
    own = det.state_dict()
    have = [[k, list(v.shape)] for k, v in own.items()]
    want = cfg['state_dict']
    assert have[:len(want)] == want
    rest = [k for k, _ in have[len(want):]]
    assert rest and all(k.startswith('roi_head.') for k in rest)
    if cfg['roi_head_keys'] is not None:
        assert sorted(k[len('roi_head.'):] for k in rest) == cfg['roi_head_keys']
    else:           # Mask R-CNN: the RoI head is the r50 detector's, whose keys the detector tests pin
        with open(os.path.join(golden_dir, 'g29_detector_configs.json')) as f:
            r50 = json.load(f)['mask_rcnn']
        assert cfg['model']['roi_head'] == r50['model']['roi_head']
        ref = dynamask_amd.build_detector(r50['model'], test_cfg=r50['test_cfg']).state_dict()
        assert [(k, tuple(own[k].shape)) for k in rest] == [(k, tuple(v.shape)) for k, v in ref.items() if k.startswith('roi_head.')]
    # a whole seeded state, strict
    g = torch.Generator().manual_seed(30)
    state = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in own.items()}
    for p in det.parameters():
        p.data.zero_()
    assert detectors.load_checkpoint(det, {'state_dict': {'module.' + k: v for k, v in state.items()}, 'meta': {'epoch': 1}},
                                     strict=True) == ({'epoch': 1}, [], [])
    assert all(torch.equal(v, state[k]) for k, v in det.state_dict().items())
    broken = dict(state)
    del broken['backbone.layer3.22.conv2.weight']
    with pytest.raises(RuntimeError, match=r"missing keys \['backbone.layer3.22.conv2.weight'\]"):
        detectors.load_checkpoint(det, {'state_dict': broken}, strict=True)
    wrong = dict(state)             # a ResNet-101 conv2 where the grouped one belongs
    wrong['backbone.layer1.0.conv2.weight'] = torch.zeros(64, 64, 3, 3)
    with pytest.raises(RuntimeError, match='layer1.0.conv2.weight'):
        detectors.load_checkpoint(det, {'state_dict': wrong}, strict=True)


# ------------------------------------------------------------------------------------------------ the kernel's host side
# (C / groups, groups) -> couts side by side in the packed weight
COUTS_PER_WAVE = {4: 4, 8: 4, 16: 4, 32: 8, 64: 16}


def test_supported_answers_from_host_arguments():
    from dynamask_amd import _lib
    L = _lib.lib()
    for cg, T in COUTS_PER_WAVE.items():
        for groups in (1, 3, 32, 64):
            C = cg * groups
            assert L.dm_conv3x3_grouped_couts_per_wave(C, groups) == T
            assert L.dm_conv3x3_grouped_packed_floats(C, groups) == 9 * C * cg
            for stride in (1, 2):
                assert L.dm_conv3x3_grouped_supported(1, C, 1, 1, groups, stride) == 1
                assert L.dm_conv3x3_grouped_supported(4, C, 200, 336, groups, stride) == 1
            for stride in (0, 3, 4, -1):
                assert L.dm_conv3x3_grouped_supported(1, C, 8, 8, groups, stride) == 0
            assert L.dm_conv3x3_grouped_supported(0, C, 8, 8, groups, 1) == 0 and L.dm_conv3x3_grouped_supported(-1, C, 8, 8, groups, 1) == 0
            assert L.dm_conv3x3_grouped_supported(1, C, 0, 8, groups, 1) == 0 and L.dm_conv3x3_grouped_supported(1, C, 8, 0, groups, 1) == 0
    for cg in (1, 2, 3, 5, 12, 24, 48, 128):
        assert L.dm_conv3x3_grouped_supported(1, cg * 2, 8, 8, 2, 1) == 0
        assert L.dm_conv3x3_grouped_couts_per_wave(cg * 2, 2) == 0 and L.dm_conv3x3_grouped_packed_floats(cg * 2, 2) == -1
    assert L.dm_conv3x3_grouped_supported(1, 33, 8, 8, 8, 1) == 0          # C no multiple of groups
    assert L.dm_conv3x3_grouped_supported(1, 32, 8, 8, 0, 1) == 0 and L.dm_conv3x3_grouped_supported(1, 32, 8, 8, -8, 1) == 0
    # a grid of 2^31 workgroups or more is refused: 4 channels per group tile 32 x 32 outputs
    assert L.dm_conv3x3_grouped_supported(1, 4 * 64, 1 << 14, 1 << 14, 64, 1) == 1          # 2^24 blocks
    assert L.dm_conv3x3_grouped_supported(128, 4 * 64, 1 << 14, 1 << 14, 64, 1) == 0        # 2^31
    assert L.dm_conv3x3_grouped_supported(1, 4, (1 << 24) + 1, 1, 1, 1) == 0


@pytest.mark.parametrize('cg,groups', [(4, 32), (8, 3), (16, 2), (32, 2), (64, 1)])
def test_pack_is_the_librarys_layout(cg, groups):
    from dynamask_amd import _lib, ops
    L = _lib.lib()
    C, T = cg * groups, COUTS_PER_WAVE[cg]
    w = torch.randn(C, cg, 3, 3, generator=torch.Generator().manual_seed(cg + groups))
    got = ops.pack_grouped_conv_weight(w, groups)
    assert got.dim() == 1 and got.numel() == 9 * C * cg and got.is_contiguous()
    lib_out = torch.full((9 * C * cg,), float('nan'))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.dm_conv3x3_grouped_pack(p(w), C, groups, p(lib_out)) == 0
    assert torch.equal(got, lib_out)
    # by hand: [C / T][cg][9][T]
    v = got.view(C // T, cg, 9, T)
    for co, ci, tap in ((0, 0, 0), (C - 1, cg - 1, 8), (T, 1, 4), (C // 2 + 1, cg // 2, 5)):
        assert v[co // T, ci, tap, co % T] == w[co, ci, tap // 3, tap % 3]
    assert L.dm_conv3x3_grouped_pack(None, C, groups, p(lib_out)) == -1 and L.dm_conv3x3_grouped_pack(p(w), C, groups, None) == -1
    assert L.dm_conv3x3_grouped_pack(p(w), C + 1, groups, p(lib_out)) == -3


def test_pack_refuses_other_shapes():
    from dynamask_amd import ops
    for shape, groups in (((64, 4, 3, 3), 8), ((64, 8, 1, 1), 8), ((64, 8, 3), 8), ((64, 8, 5, 5), 8), ((60, 8, 3, 3), 8), ((64, 8, 3, 3), 0)):
        with pytest.raises(ValueError, match='pack_grouped_conv_weight'):
            ops.pack_grouped_conv_weight(torch.zeros(shape), groups)
    with pytest.raises(NotImplementedError, match='12 channels per group'):
        ops.pack_grouped_conv_weight(torch.zeros(24, 12, 3, 3), 2)
    with pytest.raises(TypeError):
        ops.pack_grouped_conv_weight(torch.zeros(64, 8, 3, 3, dtype=torch.float64), 8)


def test_folded_grouped_weight_is_cached_and_refreshed():
    """The folded, packed conv2 of a grouped block is made once and again when a parameter, a statistic or the weight
    changes (on the CPU: the fold and the permutation need no device)."""
    from dynamask_amd import layers, ops
    torch.manual_seed(1)
    blk = layers.Bottleneck(256, 64, groups=32, base_width=4)
    assert (blk.width, blk.groups) == (128, 32) and tuple(blk.conv2.weight.shape) == (128, 4, 3, 3)
    f = blk._f[1]
    assert isinstance(f, layers._FoldedGroupedConv)
    w0, b0 = f.packed()
    assert f.packed()[0] is w0
    wf, bf = layers.fold_bn([(blk.conv2.weight, blk.bn2)])
    assert torch.equal(w0, ops.pack_grouped_conv_weight(wf, 32)) and torch.equal(b0, bf)
    with torch.no_grad():
        blk.bn2.running_var.mul_(2.0)
    w1, _ = f.packed()
    assert w1 is not w0 and not torch.equal(w1, w0)
    with torch.no_grad():
        blk.conv2.weight.add_(1.0)
    assert not torch.equal(f.packed()[0], w1)
