"""FPN neck without a GPU: the registry builds ``FPN`` from the unchanged ``model.neck`` of the Mask R-CNN, RetinaNet and FCOS
configs (tests/golden/g27_fpn_configs.json: the configs as resolved and the reference module's state_dict list), the
nearest-neighbour index tables against torch's own ``F.interpolate``, the constructor's argument rules, every refusal, and
fpn_inputs' restatement of the forward against the reference's float32 outputs (g27_fpn*.npz) bit for bit."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

FORMS = ['mask_rcnn', 'retinanet', 'fcos']


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g27_fpn_configs.json')) as f:
        return json.load(f)


def _build(cfg, **over):
    from dynamask_amd import necks, registry  # noqa: F401
    neck = dict(cfg['model']['neck'])
    neck.update(over)
    return registry.build_neck(neck)


def _fpn(**kw):
    from dynamask_amd import necks
    args = dict(in_channels=[8, 16, 32], out_channels=8, num_outs=3)
    args.update(kw)
    return necks.FPN(**args)


# ------------------------------------------------------------------------------------------------ configs and keys
def test_registry_and_exports():
    import dynamask_amd
    from dynamask_amd import necks, registry
    assert registry.NECKS.name == 'neck' and registry.NECKS.get('FPN') is necks.FPN
    assert dynamask_amd.NECKS is registry.NECKS and dynamask_amd.build_neck is registry.build_neck
    assert dynamask_amd.FPN is necks.FPN
    with pytest.raises(KeyError, match='PAFPN is not in the neck registry'):
        registry.build_neck(dict(type='PAFPN', in_channels=[8], out_channels=8, num_outs=1))


@pytest.mark.parametrize('form', FORMS)
def test_every_config_builds_unchanged(cfgs, form):
    from dynamask_amd import necks
    import fpn_inputs as fi
    assert cfgs[form]['source'] == fi.FORMS[form][0] and cfgs[form]['batch'] == fi.FORMS[form][1]
    m = _build(cfgs[form])
    assert type(m) is necks.FPN
    want = [(k, tuple(s)) for k, s in cfgs[form]['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want                    # the keys, their shapes and their order
    assert all(c.conv.exact for c in list(m.lateral_convs) + list(m.fpn_convs))   # the bf16x3 mode does not reach the neck
    used = 4 if form == 'mask_rcnn' else 3
    assert len(m.lateral_convs) == used and len(m.fpn_convs) == (4 if form == 'mask_rcnn' else 5)
    assert m.add_extra_convs == {'mask_rcnn': False, 'retinanet': 'on_input', 'fcos': 'on_output'}[form]
    assert m.relu_before_extra_convs == (form == 'fcos') and m.start_level == (0 if form == 'mask_rcnn' else 1)
    assert dict(got)['lateral_convs.0.conv.weight'] == (256, 256 if form == 'mask_rcnn' else 512, 1, 1)
    if form != 'mask_rcnn':
        assert dict(got)['fpn_convs.3.conv.weight'] == (256, 2048 if form == 'retinanet' else 256, 3, 3)
        assert [c.stride for c in m.fpn_convs] == [1, 1, 1, 2, 2]
    state = fi.head_state({k: v.shape for k, v in m.state_dict().items()}, 3)
    m.load_state_dict(state, strict=True)
    assert torch.equal(m.fpn_convs[-1].conv.bias, state[f'fpn_convs.{len(m.fpn_convs) - 1}.conv.bias'])


def test_init_weights_is_xavier_uniform():
    m = _fpn(num_outs=5, add_extra_convs='on_output')
    for c in list(m.lateral_convs) + list(m.fpn_convs):
        torch.nn.init.constant_(c.conv.bias, 1.0)
    m.init_weights()
    for c in list(m.lateral_convs) + list(m.fpn_convs):
        w = c.conv.weight.detach()
        fan_in, fan_out = w.shape[1] * w.shape[2] * w.shape[3], w.shape[0] * w.shape[2] * w.shape[3]
        bound = (6.0 / (fan_in + fan_out)) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound
        assert float(c.conv.bias.detach().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ index tables
@pytest.mark.parametrize('n_in,n_out', [(1, 2), (3, 5), (4, 7), (7, 14), (14, 27), (7, 20)])
def test_nearest_index_is_torchs_interpolate(n_in, n_out):
    from dynamask_amd import necks
    t = necks.nearest_index(n_in, n_out)
    assert t.dtype == torch.int32 and tuple(t.shape) == (n_out,) and t.device.type == 'cpu'
    ramp = torch.arange(n_in, dtype=torch.float32)
    want = F.interpolate(ramp.view(1, 1, 1, n_in).expand(1, 1, 2, n_in), size=(3, n_out), mode='nearest')[0, 0, 0]
    assert torch.equal(t.float(), want)
    # along the rows of a map, and as a gather of a random map on both axes
    x = torch.randn(2, 3, n_in, n_in, generator=torch.Generator().manual_seed(n_out))
    up = F.interpolate(x, size=(n_out, n_out), mode='nearest')
    assert torch.equal(x[:, :, t.long()][:, :, :, t.long()], up)
    assert int(t.min()) == 0 and int(t.max()) == n_in - 1 and bool((t[1:] >= t[:-1]).all())
    assert necks.nearest_index(n_in, n_out) is t            # cached


def test_nearest_index_with_a_scale_factor():
    from dynamask_amd import necks
    for n_in in (1, 4, 7):
        t = necks.nearest_index(n_in, 2 * n_in, scale_factor=2)
        x = torch.randn(1, 2, n_in, n_in, generator=torch.Generator().manual_seed(n_in))
        up = F.interpolate(x, scale_factor=2, mode='nearest')
        assert t.dtype == torch.int32 and torch.equal(x[:, :, t.long()][:, :, :, t.long()], up)
        assert t.tolist() == [i // 2 for i in range(2 * n_in)]
    # the reference's `+=` fails where the produced size is not the lower lateral's: so does the table
    with pytest.raises(ValueError, match='scale_factor'):
        necks.nearest_index(4, 7, scale_factor=2)
    with pytest.raises(ValueError):
        necks.nearest_index(0, 4)


# ------------------------------------------------------------------------------------------------ argument rules
def test_constructor_argument_rules():
    m = _fpn()
    assert (m.num_ins, m.backbone_end_level, m.start_level, m.end_level, m.add_extra_convs) == (3, 3, 0, -1, False)
    assert m.upsample_cfg == dict(mode='nearest') and not m.fp16_enabled
    # the legacy mapping of add_extra_convs=True
    assert _fpn(num_outs=4, add_extra_convs=True).add_extra_convs == 'on_input'
    assert _fpn(num_outs=4, add_extra_convs=True, extra_convs_on_inputs=False).add_extra_convs == 'on_output'
    assert _fpn(num_outs=4, add_extra_convs='on_lateral', extra_convs_on_inputs=False).add_extra_convs == 'on_lateral'
    # the extra convolutions sit behind the level convolutions; only the first reads the input's channels
    m = _fpn(num_outs=5, add_extra_convs='on_input')
    assert [(c.conv.in_channels, c.stride) for c in m.fpn_convs] == [(8, 1), (8, 1), (8, 1), (32, 2), (8, 2)]
    m = _fpn(num_outs=5, add_extra_convs='on_output')
    assert [(c.conv.in_channels, c.stride) for c in m.fpn_convs] == [(8, 1), (8, 1), (8, 1), (8, 2), (8, 2)]
    assert len(_fpn(num_outs=5).fpn_convs) == 3                  # the max-pool levels have no parameters
    # start_level / end_level
    m = _fpn(start_level=1, num_outs=2)
    assert [c.conv.in_channels for c in m.lateral_convs] == [16, 32]
    m = _fpn(start_level=0, end_level=2, num_outs=2)
    assert m.backbone_end_level == 2 and [c.conv.in_channels for c in m.lateral_convs] == [8, 16]
    with pytest.raises(ValueError, match='num_outs'):
        _fpn(num_outs=2)
    with pytest.raises(ValueError, match='num_outs'):
        _fpn(end_level=2, num_outs=3)                             # no extra level with an end_level
    with pytest.raises(ValueError, match='end_level'):
        _fpn(end_level=4, num_outs=4)
    with pytest.raises(ValueError, match='add_extra_convs'):
        _fpn(num_outs=4, add_extra_convs='on_top')
    with pytest.raises(TypeError, match='add_extra_convs'):
        _fpn(num_outs=4, add_extra_convs=1)
    with pytest.raises(TypeError, match='in_channels'):
        _fpn(in_channels=8, num_outs=1)


@pytest.mark.parametrize('kw,word', [
    (dict(conv_cfg=dict(type='ConvWS')), 'conv_cfg'),
    (dict(norm_cfg=dict(type='GN', num_groups=32)), 'norm_cfg'),
    (dict(act_cfg=dict(type='ReLU')), 'act_cfg'),
    (dict(upsample_cfg=dict(mode='bilinear')), 'upsample_cfg'),
    (dict(upsample_cfg=dict(mode='nearest', align_corners=False)), 'upsample_cfg'),
    (dict(out_channels=12), 'out_channels'),
    (dict(in_channels=[8, 16, 36], num_outs=4, add_extra_convs='on_input'), 'in_channels'),
])
def test_refusals_name_the_argument(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _fpn(**kw)


def test_refusals_leave_the_neighbours_alone():
    # channels that are no multiple of 8 are fine where no 3x3 kernel reads them
    _fpn(in_channels=[3, 5, 36])
    _fpn(in_channels=[8, 16, 36], num_outs=4, add_extra_convs='on_output')
    _fpn(upsample_cfg=dict(mode='nearest', scale_factor=2))


def test_forward_refuses_training_and_wrong_inputs():
    m = _fpn()
    xs = [torch.zeros(1, c, s, s) for c, s in zip([8, 16, 32], [8, 4, 2])]
    with pytest.raises(NotImplementedError, match='FPN: training'):
        m(xs)
    with torch.no_grad():
        with pytest.raises(ValueError, match='3 inputs'):
            m(xs[:2])
        with pytest.raises(ValueError, match='input 1'):
            m([xs[0], xs[0], xs[2]])
        # no CPU fallback: the launches refuse a host tensor
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m(xs)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('form', FORMS)
def test_restatement_is_the_reference_in_float32(cfgs, golden_dir, form):
    import fpn_inputs as fi
    z = np.load(os.path.join(golden_dir, fi.FILES[form]))
    assert os.path.getsize(os.path.join(golden_dir, fi.FILES[form])) < (1 << 20)
    neck = cfgs[form]['model']['neck']
    state = fi.head_state({k: tuple(s) for k, s in cfgs[form]['state_dict']}, fi.WEIGHT_SEED)
    xs = fi.inputs(neck['in_channels'], cfgs[form]['batch'])
    assert [tuple(x.shape[2:]) for x in xs] == [(18, 27), (9, 14), (5, 7), (3, 4)]
    with torch.no_grad():
        outs = fi.restate(neck, state, xs)
        outs64 = fi.restate(neck, state, [x.double() for x in xs])
    assert len(outs) == neck['num_outs'] == 5
    sizes = [(18, 27), (9, 14), (5, 7), (3, 4), (2, 2)] if form == 'mask_rcnn' else [(9, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
    for l, (o, o64) in enumerate(zip(outs, outs64)):
        ref = z[f'{form}_out{l}']
        assert tuple(o.shape) == ref.shape == (cfgs[form]['batch'], 256) + sizes[l]
        assert np.array_equal(o.numpy().view(np.int32), ref.view(np.int32)), f'{form} level {l}'
        twin = fi.unpack_f64(ref, z[f'{form}_out{l}_err16'])
        assert float(np.abs(twin - o64.numpy()).max()) < 1e-8
