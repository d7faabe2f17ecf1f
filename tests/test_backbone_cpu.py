"""``backbones.ResNet`` without a device: it builds from the unchanged ``model.backbone`` of the reference's configs
(tests/golden/g28_backbone_configs.json) with the reference's state_dict keys, refuses what is not built by name, folds the
stem's BatchNorm in float64, and the stem's ``_supported`` entry points answer on the host."""
import json
import os

import pytest
import torch

CONFIGS = ['pytorch', 'caffe_c4', 'pytorch_r101', 'caffe_c4_r101']


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g28_backbone_configs.json')) as f:
        return json.load(f)


def _build(cfg):
    from dynamask_amd import backbones, registry  # noqa: F401  (backbones registers ResNet)
    return registry.build_backbone(dict(cfg))


@pytest.mark.parametrize('name', CONFIGS)
def test_builds_from_the_unchanged_config_with_the_reference_keys(cfgs, name):
    import backbone_inputs as bi
    import dynamask_amd
    from dynamask_amd import backbones
    cfg = cfgs[name]['model']['backbone']
    assert cfg['type'] == 'ResNet' and cfg['depth'] == (101 if name.endswith('r101') else 50)
    m = _build(cfg)
    assert type(m) is backbones.ResNet is dynamask_amd.ResNet and dynamask_amd.BACKBONES.get('ResNet') is backbones.ResNet
    assert dynamask_amd.build_backbone is dynamask_amd.registry.build_backbone
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == cfgs[name]['state_dict']        # keys, shapes and their order
    state = bi.head_state({k: s for k, s in cfgs[name]['state_dict']}, 3)
    m.load_state_dict(state, strict=True)
    assert torch.equal(m.layer1[0].downsample[0].weight, state['layer1.0.downsample.0.weight'])
    assert m.state_dict()['bn1.num_batches_tracked'].dtype == torch.long
    caffe = name.startswith('caffe')
    assert m.style == ('caffe' if caffe else 'pytorch') and m.res_layers == [f'layer{i + 1}' for i in range(3 if caffe else 4)]
    assert m.feat_dim == (1024 if caffe else 2048) and m.frozen_stages == 1 and m.norm_eval
    # frozen_stages = 1: the stem and layer1 ask for no gradient; requires_grad=False in norm_cfg: no BatchNorm does
    assert not m.conv1.weight.requires_grad and not any(p.requires_grad for p in m.layer1.parameters())
    assert m.layer2[0].conv1.weight.requires_grad
    assert m.layer2[0].bn1.weight.requires_grad == (not caffe)
    assert m.train() is m and m.eval() is m


def test_what_is_not_built_raises_by_name():
    from dynamask_amd.backbones import ResNet
    for kw, word in ((dict(depth=18), 'depth=18'), (dict(depth=34), 'depth=34'),
                     (dict(depth=50, deep_stem=True), 'deep_stem'), (dict(depth=50, avg_down=True), 'avg_down'),
                     (dict(depth=50, dcn=dict(type='DCN', deform_groups=1), stage_with_dcn=(False, True, True, True)), 'dcn'),
                     (dict(depth=50, plugins=[dict(cfg=dict(type='ContextBlock', ratio=1. / 16), position='after_conv3')]), 'plugins'),
                     (dict(depth=50, conv_cfg=dict(type='ConvWS')), 'conv_cfg'),
                     (dict(depth=50, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)), 'norm_cfg'),
                     (dict(depth=50, norm_cfg=dict(type='SyncBN', requires_grad=True)), 'norm_cfg'),
                     (dict(depth=50, strides=(1, 2, 2, 1), dilations=(1, 1, 1, 2)), 'dilations')):
        with pytest.raises(NotImplementedError, match=word):
            ResNet(**kw)
    # the reference's own checks
    with pytest.raises(KeyError, match='invalid depth 20'):
        ResNet(depth=20)
    with pytest.raises(AssertionError):
        ResNet(depth=50, num_stages=5, strides=(1, 2, 2, 2, 2), dilations=(1,) * 5)
    with pytest.raises(AssertionError):
        ResNet(depth=50, num_stages=0, strides=(), dilations=(), out_indices=())
    with pytest.raises(AssertionError):
        ResNet(depth=50, num_stages=3)                                   # strides / dilations keep four entries
    with pytest.raises(AssertionError):
        ResNet(depth=50, num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1))         # out_indices reaches stage 3
    with pytest.raises(AssertionError):
        ResNet(depth=50, dcn=dict(type='DCN'), stage_with_dcn=(False, True))
    m = ResNet(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(1,))
    with pytest.raises(NotImplementedError, match='load_state_dict'):
        m.init_weights(pretrained='torchvision://resnet50')
    with pytest.raises(TypeError):
        m.init_weights(pretrained=5)
    # training: grad enabled and something asks for a gradient
    with pytest.raises(NotImplementedError, match='training'):
        m(torch.zeros(1, 3, 8, 8))
    for p in m.parameters():
        p.requires_grad = False
    with pytest.raises(NotImplementedError, match='training'):
        m(torch.zeros(1, 3, 8, 8, requires_grad=True))
    with torch.no_grad(), pytest.raises(ValueError, match=r'\[B, 3, H, W\]'):
        m(torch.zeros(1, 4, 8, 8))


def test_init_weights():
    from dynamask_amd.backbones import ResNet
    from dynamask_amd.bbox_heads import Bottleneck
    m = ResNet(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(1,))
    with torch.no_grad():
        for p in m.parameters():
            p.fill_(7.0)
    m.init_weights()
    blocks = [b for b in m.modules() if isinstance(b, Bottleneck)]
    assert len(blocks) == 7
    for b in blocks:
        assert not bool(b.bn3.weight.detach().any()) and not bool(b.bn3.bias.detach().any())       # zero_init_residual
        assert bool((b.bn1.weight == 1).all()) and bool((b.bn1.bias == 0).all())
        assert 0 < float(b.conv2.weight.detach().std()) < 1 and abs(float(b.conv2.weight.detach().mean())) < 0.01
    # kaiming, fan_out: std = sqrt(2 / (64 * 49))
    assert abs(float(m.conv1.weight.detach().std()) - (2 / (64 * 49)) ** 0.5) < 0.003
    m2 = ResNet(depth=50, num_stages=1, strides=(1,), dilations=(1,), out_indices=(0,), zero_init_residual=False)
    m2.init_weights()
    assert bool((m2.layer1[0].bn3.weight == 1).all())


def test_the_stem_fold_is_float64_rounded_once(cfgs):
    import backbone_inputs as bi
    m = _build(cfgs['pytorch']['model']['backbone'])
    state = bi.head_state({k: s for k, s in cfgs['pytorch']['state_dict']}, 11)
    m.load_state_dict(state, strict=True)
    w, b = m._stem.folded()
    s = state['bn1.weight'].double() / torch.sqrt(state['bn1.running_var'].double() + 1e-5)
    want_w = (state['conv1.weight'].double() * s[:, None, None, None]).float()
    want_b = (state['bn1.bias'].double() - state['bn1.running_mean'].double() * s).float()
    assert w.dtype == torch.float32 and tuple(w.shape) == (64, 3, 7, 7) and tuple(b.shape) == (64,)
    assert torch.equal(w, want_w) and torch.equal(b, want_b)
    # the cache follows the parameters: load_state_dict copies in place
    state2 = bi.head_state({k: s for k, s in cfgs['pytorch']['state_dict']}, 12)
    m.load_state_dict(state2, strict=True)
    assert not torch.equal(m._stem.folded()[0], want_w)


def test_bottleneck_defaults_are_the_block_the_heads_use():
    """The backbone's arguments are optional: a block built without them is the stride-1 'pytorch' block on ops.conv2d."""
    from dynamask_amd.bbox_heads import Bottleneck
    b = Bottleneck(256, 64)
    assert (b.stride, b.style, b.wide_from, b.downsample) == (1, 'pytorch', None, None)
    d = Bottleneck(64, 64, downsample=True)
    assert (d.stride, d.style, d.wide_from) == (1, 'pytorch', None) and d.downsample is not None
    with pytest.raises(NotImplementedError, match='stride=2'):
        Bottleneck(256, 64, stride=2)
    with pytest.raises(NotImplementedError, match='stride=3'):
        Bottleneck(256, 64, downsample=True, stride=3)


def test_supported_entry_points_answer_on_the_host():
    from dynamask_amd import _lib, ops
    from dynamask_amd.backbones import ResNet
    L = _lib.lib()
    conv, pool = L.dm_conv7x7_s2_supported, L.dm_maxpool3x3_s2_supported
    assert conv(1, 3, 1, 1, 1) == 1 and conv(2, 3, 800, 1344, 64) == 1 and conv(1, 3, 37, 53, 24) == 1
    assert conv(0, 3, 8, 8, 64) == 0 and conv(1, 3, 0, 8, 64) == 0 and conv(1, 3, 8, 0, 64) == 0 and conv(1, 3, 8, 8, 0) == 0
    assert all(conv(1, C, 8, 8, 64) == 0 for C in (1, 2, 4, 5, 8))
    # workgroups: NB * ceil(Ho / 8) * ceil(Wo / 16) * ceil(CoutP / 64) < 2^31
    assert conv(1, 3, 16, 32, 64 * 65536) == 1 and conv(32768, 3, 16, 32, 64 * 65536) == 0
    assert pool(0, 1, 1) == 1 and pool(128, 400, 672) == 1 and pool(-1, 4, 4) == 0 and pool(1, 0, 4) == 0 and pool(1, 4, 0) == 0
    assert pool(1 << 40, 1, 1) == 1 and pool((1 << 40) + 1, 1, 1) == 0
    assert ops.conv7x7_s2_supported((1, 3, 9, 9), 64) and not ops.conv7x7_s2_supported((1, 5, 9, 9), 64)
    # launchers validate before they touch the device
    assert L.dm_conv7x7_s2_fwd(None, 1, 3, 8, 8, None, None, 64, 0, None, None) == -1
    assert L.dm_maxpool3x3_s2_fwd(None, 1, 0, 8, None, None) == -3
    # the module refuses a stem the kernel does not take, by name
    m = ResNet(depth=50, in_channels=5, num_stages=1, strides=(1,), dilations=(1,), out_indices=(0,))
    with torch.no_grad(), pytest.raises(NotImplementedError, match='in_channels=5'):
        m(torch.zeros(1, 5, 8, 8))
