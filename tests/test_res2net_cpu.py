"""Res2Net without a device: the registry builds ``backbones.Res2Net`` from the reference's unchanged r2_101 configs
(tests/golden/g31_res2net_configs.json) with the reference's keys and shapes in order, the forms it always takes, the flags
``ResNet`` keeps, the refusals by name, the five whole detectors with ``load_checkpoint``, the torch restatement against the
stored outputs, and the host side of the sliced kernel: the weight layout and ``dm_conv3x3_slices_supported``."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tolerances import assert_close_via_f64

DETECTORS = {'mask_rcnn_r2_101': 'MaskRCNN', 'cascade_mask_rcnn_r2_101': 'CascadeRCNN', 'htc_r2_101': 'HybridTaskCascade',
             'faster_rcnn_r2_101': 'FasterRCNN', 'cascade_rcnn_r2_101': 'CascadeRCNN'}
WITH_MASK = {'mask_rcnn_r2_101', 'cascade_mask_rcnn_r2_101', 'htc_r2_101'}
WIDTHS = [26, 52, 104, 208]


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g31_res2net_configs.json')) as f:
        return json.load(f)


def _build(cfg):
    from dynamask_amd import backbones, registry  # noqa: F401
    return registry.build_backbone(copy.deepcopy(cfg))


# ------------------------------------------------------------------------------------------------ the backbone
def test_fixture_entries(cfgs):
    assert set(cfgs) == {'r2_101'} | set(DETECTORS)
    b = cfgs['r2_101']['model']['backbone']
    assert set(cfgs['r2_101']['model']) == {'backbone'}
    assert (b['type'], b['depth'], b['scales'], b['base_width']) == ('Res2Net', 101, 4, 26)
    for name, typ in DETECTORS.items():
        assert cfgs[name]['model']['type'] == typ and set(cfgs[name]['test_cfg']) == {'rpn', 'rcnn'}
        assert cfgs[name]['model']['backbone'] == b, 'the five configs share one backbone'


@pytest.mark.parametrize('name', ['r2_101'] + sorted(DETECTORS))
def test_registry_builds_res2net_with_the_references_keys(cfgs, name):
    import res2net_inputs as xi
    import dynamask_amd
    from dynamask_amd import backbones, layers
    cfg = cfgs[name]['model']['backbone']
    before = copy.deepcopy(cfg)
    m = _build(cfg)
    assert cfg == before
    assert type(m) is backbones.Res2Net and isinstance(m, backbones.ResNet) and dynamask_amd.Res2Net is backbones.Res2Net
    assert dynamask_amd.BACKBONES.get('Res2Net') is backbones.Res2Net
    want = cfgs['r2_101']['state_dict']
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want
    assert [[k, list(s)] for k, s in xi.state_shapes(cfg).items()] == want
    assert not any(k.startswith(('conv1.', 'bn1.')) or '.conv2.' in k or '.bn2.' in k for k, _ in want)
    assert xi.widths(cfg) == WIDTHS and (m.scales, m.base_width) == (4, 26)
    assert (m.style, m.deep_stem, m.avg_down) == ('pytorch', True, True)
    # ``stem`` is the submodule, as in the reference, and ``named_modules`` knows it under that name
    assert isinstance(m.stem, backbones.DeepStem) and dict(m.named_modules())['stem'] is m.stem
    assert [tuple(m.stem[i].weight.shape) for i in (0, 3, 6)] == [(32, 3, 3, 3), (32, 32, 3, 3), (64, 32, 3, 3)]
    for i, w in enumerate(WIDTHS):
        blocks = getattr(m, f'layer{i + 1}')
        assert len(blocks) == (3, 4, 23, 3)[i]
        for j, b in enumerate(blocks):
            assert isinstance(b, layers.Bottle2neck) and (b.width, b.scales) == (w, 4)
            assert b.stage_type == ('stage' if j == 0 else 'normal')
            assert b.stride == (2 if j == 0 and i > 0 else 1) and (b.downsample is not None) == (j == 0)
            assert tuple(b.conv1.weight.shape) == (4 * w, b.inplanes, 1, 1) and tuple(b.conv3.weight.shape) == (256 * 2 ** i, 4 * w, 1, 1)
            assert [tuple(c.weight.shape) for c in b.convs] == [(w, w, 3, 3)] * 3 and len(b.bns) == 3
            assert not hasattr(b, 'conv2') and not hasattr(b, 'bn2')
    assert m.feat_dim == 2048 and m.res_layers == ['layer1', 'layer2', 'layer3', 'layer4'] and m.frozen_stages == 1
    assert tuple(m.out_indices) == (0, 1, 2, 3)
    # frozen_stages=1: the stem and layer1 (resnet.py:573-589)
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    assert frozen == [k for k, _ in m.named_parameters() if k.startswith(('stem.', 'layer1.'))] and frozen


def test_flags_and_what_the_reference_ignores():
    from dynamask_amd import backbones, layers
    # style / deep_stem / avg_down are the reference's constants whatever the caller passes (res2net.py:298-308)
    torch.manual_seed(7)
    a = backbones.Res2Net(depth=50, style='caffe', deep_stem=False, avg_down=False)
    torch.manual_seed(7)
    b = backbones.Res2Net(depth=50)
    assert (a.style, a.deep_stem, a.avg_down) == ('pytorch', True, True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(p.requires_grad for p in b.parameters())                    # frozen_stages=-1
    assert backbones.Res2Net.arch_settings[101] == (layers.Bottle2neck, (3, 4, 23, 3)) and sorted(backbones.Res2Net.arch_settings) == [50, 101, 152]
    # norm_cfg.requires_grad=False freezes every BatchNorm parameter and nothing else
    c = backbones.Res2Net(depth=50, norm_cfg=dict(type='BN', requires_grad=False))
    for k, p in c.named_parameters():
        is_bn = p.dim() == 1
        assert p.requires_grad == (not is_bn), k
    d = backbones.Res2Net(depth=50, frozen_stages=0)
    assert [k for k, p in d.named_parameters() if not p.requires_grad] == [k for k, _ in d.named_parameters() if k.startswith('stem.')]
    # zero_init_residual reaches bn3 of Bottle2neck
    b.init_weights()
    blocks = [m for m in b.modules() if isinstance(m, layers.Bottle2neck)]
    assert len(blocks) == 16
    assert all(float(m.bn3.weight.detach().abs().sum()) == 0 and float(m.bns[0].weight.detach().min()) == 1 for m in blocks)
    e = backbones.Res2Net(depth=50, zero_init_residual=False)
    e.init_weights()
    assert all(float(m.bn3.weight.detach().min()) == 1 for m in e.modules() if isinstance(m, layers.Bottle2neck))
    with pytest.raises(NotImplementedError, match='load_state_dict'):
        b.init_weights('open-mmlab://res2net101_v1d_26w_4s')


def test_what_is_not_built_raises_by_name():
    from dynamask_amd import backbones, layers
    with pytest.raises(NotImplementedError, match='deep_stem'):
        backbones.ResNet(depth=50, deep_stem=True)
    with pytest.raises(NotImplementedError, match='avg_down'):
        backbones.ResNet(depth=50, avg_down=True)
    with pytest.raises(NotImplementedError, match='deep_stem'):
        backbones.ResNeXt(depth=50, groups=32, deep_stem=True)
    with pytest.raises(NotImplementedError, match='scales=1'):
        backbones.Res2Net(depth=50, scales=1)
    with pytest.raises(NotImplementedError, match=r'scales=3, base_width=26 .* 26 channels per scale, 78 in all'):
        backbones.Res2Net(depth=50, scales=3)
    with pytest.raises(NotImplementedError, match=r'base_width=25 .* 25 channels per scale, 100 in all'):
        backbones.Res2Net(depth=50, base_width=25)
    with pytest.raises(NotImplementedError, match='scales=1'):
        layers.Bottle2neck(256, 64, scales=1)
    with pytest.raises(NotImplementedError, match='78 in all'):
        layers.Bottle2neck(256, 64, scales=3)
    with pytest.raises(NotImplementedError, match='stride=2'):
        layers.Bottle2neck(256, 64, stride=2)                      # a normal block has no stride
    with pytest.raises(NotImplementedError, match='downsample'):
        layers.Bottle2neck(64, 64)
    with pytest.raises(KeyError, match='invalid depth'):
        backbones.Res2Net(depth=18)
    with pytest.raises(NotImplementedError, match='dcn='):
        backbones.Res2Net(depth=101, dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False),
                          stage_with_dcn=(False, True, True, True))
    with pytest.raises(NotImplementedError, match='plugins='):
        backbones.Res2Net(depth=50, plugins=[dict(cfg=dict(type='ContextBlock', ratio=1. / 16), position='after_conv3')])
    with pytest.raises(NotImplementedError, match='conv_cfg='):
        backbones.Res2Net(depth=50, conv_cfg=dict(type='ConvWS'))
    with pytest.raises(NotImplementedError, match='norm_cfg='):
        backbones.Res2Net(depth=50, norm_cfg=dict(type='GN', num_groups=32))
    with pytest.raises(NotImplementedError, match='dilations='):
        backbones.Res2Net(depth=50, strides=(1, 2, 2, 1), dilations=(1, 1, 1, 2))
    with pytest.raises(NotImplementedError, match='stem_channels=24'):
        backbones.Res2Net(depth=50, stem_channels=24)
    m = backbones.Res2Net(depth=50)
    with pytest.raises(NotImplementedError, match='training'):
        m(torch.zeros(1, 3, 32, 32))
    # the registries the issue leaves alone
    import dynamask_amd
    assert dynamask_amd.BACKBONES.get('RetinaNet') is None and dynamask_amd.NECKS.get('PAFPN') is None


def test_bottle2neck_keys_and_folded_slices():
    """One block of each kind: the reference's key order, and the folded, packed slices made once and again when a
    parameter or a statistic changes (on the CPU: the fold and the permutation need no device)."""
    from dynamask_amd import layers, ops
    torch.manual_seed(2)
    stage = layers.Bottle2neck(64, 16, downsample=True, stride=2, base_width=32, stage_type='stage')
    normal = layers.Bottle2neck(64, 16, base_width=32)
    assert (stage.width, normal.width) == (8, 8)
    assert [k for k in stage.state_dict() if k.endswith('weight') and '.' in k and 'bn' not in k and 'downsample.2' not in k] == \
        ['conv1.weight', 'conv3.weight', 'downsample.1.weight', 'convs.0.weight', 'convs.1.weight', 'convs.2.weight']
    assert not any(k.startswith('downsample.0') for k in stage.state_dict()) and normal.downsample is None
    assert len(stage._f2) == 1 and len(normal._f2) == 3
    for blk, G in ((stage, 3), (normal, 1)):
        f = blk._f2[0]
        wq, b = f.packed()
        assert f.packed()[0] is wq
        folds = [layers.fold_bn([(c.weight, bn)]) for c, bn in list(zip(blk.convs, blk.bns))[:G]]
        assert torch.equal(wq, ops.pack_conv_slices_weight(torch.stack([w for w, _ in folds])))
        assert torch.equal(b, torch.cat([bb for _, bb in folds]))
        with torch.no_grad():
            blk.bns[0].running_var.mul_(2.0)
        w1, _ = f.packed()
        assert w1 is not wq and not torch.equal(w1, wq)
        with torch.no_grad():
            blk.convs[0].weight.add_(1.0)
        assert not torch.equal(f.packed()[0], w1)


def test_restate_reproduces_the_stored_outputs(cfgs, golden_dir):
    """The torch restatement, on the CPU in float32, against the reference module's stored outputs and their float64
    twins: the fixture and the restatement the device tests lean on say the same thing."""
    import res2net_inputs as xi
    cfg = cfgs['r2_101']['model']['backbone']
    state = xi.head_state({k: tuple(s) for k, s in cfgs['r2_101']['state_dict']}, xi.WEIGHT_SEED)
    z = np.load(os.path.join(golden_dir, xi.FILE))
    torch.set_num_threads(min(8, torch.get_num_threads()))
    with torch.no_grad():
        outs = xi.restate(cfg, state, xi.inputs())
    assert len(outs) == 4
    for l, got in enumerate(outs):
        ref32 = z[f'r2_101_out{l}']
        assert tuple(got.shape) == ref32.shape
        err, ref_err, scale = assert_close_via_f64(got, ref32, xi.unpack_f64(ref32, z[f'r2_101_out{l}_err16']), f'output {l}')
        print(f'restate output {l}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')


# ------------------------------------------------------------------------------------------------ the detectors
@pytest.mark.parametrize('name', sorted(DETECTORS))
def test_build_detector_and_load_checkpoint(cfgs, golden_dir, tmp_path, name):
    import dynamask_amd
    from dynamask_amd import backbones, detectors
    cfg = cfgs[name]
    before = copy.deepcopy(cfg)
    det = dynamask_amd.build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert cfg == before, 'the build changed the caller\'s config'
    assert type(det) is getattr(detectors, DETECTORS[name]) and type(det.backbone) is backbones.Res2Net
    assert det.pretrained == cfg['model']['pretrained'] == 'open-mmlab://res2net101_v1d_26w_4s'
    assert det.with_neck and det.with_rpn and det.with_mask == (name in WITH_MASK)
    own = det.state_dict()
    have = [[k, list(v.shape)] for k, v in own.items()]
    want = [['backbone.' + k, s] for k, s in cfgs['r2_101']['state_dict']] + cfg['state_dict_behind_backbone']
    assert have[:len(want)] == want
    rest = [k for k, _ in have[len(want):]]
    assert rest and all(k.startswith('roi_head.') for k in rest)
    if cfg['roi_head_keys'] is not None:
        assert sorted(k[len('roi_head.'):] for k in rest) == cfg['roi_head_keys']
    elif name == 'mask_rcnn_r2_101':          # the RoI head is the r50 detector's, whose keys the detector tests pin
        with open(os.path.join(golden_dir, 'g29_detector_configs.json')) as f:
            r50 = json.load(f)['mask_rcnn']
        assert cfg['model']['roi_head'] == r50['model']['roi_head']
        ref = dynamask_amd.build_detector(r50['model'], test_cfg=r50['test_cfg']).state_dict()
        assert [(k, tuple(own[k].shape)) for k in rest] == [(k, tuple(v.shape)) for k, v in ref.items() if k.startswith('roi_head.')]
    else:                                     # box only: bbox heads and no mask head
        assert not any('.mask_head.' in k for k in rest) and any('.bbox_head.' in k for k in rest)
    # a whole seeded checkpoint with the reference's keys, through a file
    g = torch.Generator().manual_seed(31)
    state = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in own.items()}
    path = str(tmp_path / 'r2.pth')
    torch.save({'state_dict': {'module.' + k: v for k, v in state.items()}, 'meta': {'epoch': 2}}, path)
    for p in det.parameters():
        p.data.zero_()
    assert detectors.load_checkpoint(det, path, strict=True) == ({'epoch': 2}, [], [])
    assert all(torch.equal(v, state[k]) for k, v in det.state_dict().items())
    broken = dict(state)
    del broken['backbone.layer3.22.convs.2.weight']
    with pytest.raises(RuntimeError, match=r"missing keys \['backbone.layer3.22.convs.2.weight'\]"):
        detectors.load_checkpoint(det, {'state_dict': broken}, strict=True)
    wrong = dict(state)             # a ResNet-101 stem where the deep stem belongs
    wrong['backbone.conv1.weight'] = torch.zeros(64, 3, 7, 7)
    with pytest.raises(RuntimeError, match='conv1.weight'):
        detectors.load_checkpoint(det, {'state_dict': wrong}, strict=True)


# ------------------------------------------------------------------------------------------------ the kernels' host side
def test_supported_answers_from_host_arguments():
    from dynamask_amd import _lib
    L = _lib.lib()
    for w in (1, 6, 8, 9, 26, 52, 104, 208, 1000):
        assert L.dm_conv3x3_slices_packed_floats(3, w) == 3 * ((w + 7) // 8) * w * 72
        for G in (1, 3):
            for stride in (1, 2):
                for tail in ((0, 1, 2) if stride == 1 else (0, 2)):
                    assert L.dm_conv3x3_slices_supported(1, w, G, 1, 1, stride, 4 * w, 4 * w, tail) == 1
                    assert L.dm_conv3x3_slices_supported(4, w, G, 200, 336, stride, 4 * w, 4 * w, tail) == 1
                assert L.dm_conv3x3_slices_supported(1, w, G, 8, 8, stride, G * w, G * w, 0) == 1
                assert L.dm_conv3x3_slices_supported(1, w, G, 8, 8, stride, G * w, G * w, 2) == 0       # no room for the tail
                assert L.dm_conv3x3_slices_supported(1, w, G, 8, 8, stride, G * w - 1, 4 * w, 0) == 0
            assert L.dm_conv3x3_slices_supported(1, w, G, 8, 8, 2, 4 * w, 4 * w, 1) == 0                # the copy is stride 1's
            for stride in (0, 3, -1):
                assert L.dm_conv3x3_slices_supported(1, w, G, 8, 8, stride, 4 * w, 4 * w, 0) == 0
            assert L.dm_conv3x3_slices_supported(0, w, G, 8, 8, 1, 4 * w, 4 * w, 0) == 0
            assert L.dm_conv3x3_slices_supported(1, w, G, 0, 8, 1, 4 * w, 4 * w, 0) == 0
            assert L.dm_conv3x3_slices_supported(1, w, G, 8, 8, 1, 4 * w, 4 * w, 3) == 0
    assert L.dm_conv3x3_slices_supported(1, 0, 1, 8, 8, 1, 8, 8, 0) == 0 and L.dm_conv3x3_slices_supported(1, 8, 0, 8, 8, 1, 8, 8, 0) == 0
    assert L.dm_conv3x3_slices_packed_floats(0, 8) == -1 and L.dm_conv3x3_slices_packed_floats(1, 0) == -1
    # a grid of 2^31 workgroups or more is refused: w <= 8 tiles 32 x 32 outputs
    assert L.dm_conv3x3_slices_supported(1, 8, 1, 1 << 14, 1 << 14, 1, 8, 8, 0) == 1          # 2^18 blocks
    assert L.dm_conv3x3_slices_supported(1 << 13, 8, 1, 1 << 14, 1 << 14, 1, 8, 8, 0) == 0    # 2^31
    assert L.dm_conv3x3_slices_supported(1, 8, 1, (1 << 24) + 1, 1, 1, 8, 8, 0) == 0
    assert L.dm_avgpool2x2_ceil_supported(0, 1, 1) == 1 and L.dm_avgpool2x2_ceil_supported(8, 37, 53) == 1
    assert L.dm_avgpool2x2_ceil_supported(8, 0, 53) == 0 and L.dm_avgpool2x2_ceil_supported(-1, 3, 3) == 0
    assert L.dm_avgpool2x2_ceil_supported(1 << 30, 1 << 10, 1 << 10) == 0
    assert L.dm_conv3x3_s2_c3_supported(1, 3, 1, 1, 32) == 1 and L.dm_conv3x3_s2_c3_supported(4, 3, 800, 1344, 33) == 1
    assert L.dm_conv3x3_s2_c3_supported(1, 4, 8, 8, 32) == 0 and L.dm_conv3x3_s2_c3_supported(0, 3, 8, 8, 32) == 0
    assert L.dm_conv3x3_s2_c3_supported(1, 3, 0, 8, 32) == 0 and L.dm_conv3x3_s2_c3_supported(1, 3, 8, 8, 0) == 0


@pytest.mark.parametrize('w,G', [(6, 3), (8, 1), (26, 3), (52, 1)])
def test_pack_is_the_librarys_layout(w, G):
    from dynamask_amd import _lib, ops
    L = _lib.lib()
    T = (w + 7) // 8
    wt = torch.randn(G, w, w, 3, 3, generator=torch.Generator().manual_seed(w + G))
    got = ops.pack_conv_slices_weight(wt)
    n = G * T * w * 72
    assert got.dim() == 1 and got.numel() == n == L.dm_conv3x3_slices_packed_floats(G, w) and got.is_contiguous()
    lib_out = torch.full((n,), float('nan'))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.dm_conv3x3_slices_pack(p(wt), G, w, p(lib_out)) == 0
    assert torch.equal(got, lib_out)
    # by hand: [G][T][w][9][8], zeros for the couts from w on
    v = got.view(G, T, w, 9, 8)
    for g, co, ci, tap in ((0, 0, 0, 0), (G - 1, w - 1, w - 1, 8), (G // 2, w // 2, 1, 4)):
        assert v[g, co // 8, ci, tap, co % 8] == wt[g, co, ci, tap // 3, tap % 3]
    if w % 8:
        assert float(v[:, T - 1, :, :, w % 8:].abs().sum()) == 0
    assert L.dm_conv3x3_slices_pack(None, G, w, p(lib_out)) == -1 and L.dm_conv3x3_slices_pack(p(wt), G, w, None) == -1
    assert L.dm_conv3x3_slices_pack(p(wt), G, 0, p(lib_out)) == -3
    for shape in ((w, w, 3, 3), (G, w, w + 1, 3, 3), (G, w, w, 1, 1)):
        with pytest.raises(ValueError, match='pack_conv_slices_weight'):
            ops.pack_conv_slices_weight(torch.zeros(shape))
    with pytest.raises(TypeError):
        ops.pack_conv_slices_weight(wt.double())
