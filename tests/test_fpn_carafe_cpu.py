"""FPN_CARAFE without a device: the neck and the two detectors of configs/carafe build from the unchanged configs with the
reference's keys (tests/golden/g32_fpn_carafe_configs.json), what is not built raises by name, the reference's asserts
hold, ``dm_carafe_map_supported`` answers on the host, and the restatement the device tests lean on reproduces the
stored outputs."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tolerances import assert_close_via_f64

NECK = dict(in_channels=[16, 32, 64], out_channels=16, num_outs=4,
            upsample_cfg=dict(type='carafe', up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1, compressed_channels=8))


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g32_fpn_carafe_configs.json')) as f:
        return json.load(f)


def test_the_neck_builds_from_the_unchanged_config(cfgs):
    import dynamask_amd
    import fpn_carafe_inputs as ci
    from dynamask_amd import necks
    cfg = cfgs['mask_rcnn_carafe']['model']['neck']
    before = copy.deepcopy(cfg)
    assert cfg['type'] == 'FPN_CARAFE' and cfg['upsample_cfg']['type'] == 'carafe' and cfg['num_outs'] == 5
    m = dynamask_amd.build_neck(cfg)
    assert cfg == before, 'the build changed the caller\'s config'
    assert type(m) is necks.FPN_CARAFE is dynamask_amd.FPN_CARAFE is dynamask_amd.NECKS.get('FPN_CARAFE')
    have = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert have == cfgs['mask_rcnn_carafe']['neck_state_dict']
    assert have == [[k, list(s)] for k, s in ci.state_shapes(cfg).items()]
    assert len(m.lateral_convs) == len(m.fpn_convs) == 5 and len(m.upsample_modules) == 4
    assert [c.stride for c in m.lateral_convs] == [1, 1, 1, 1, 2]
    assert have[8] == ['lateral_convs.4.conv.weight', [256, 2048, 3, 3]]           # the extra level reads in_channels[-1]
    # every convolution is exact fp32 whatever the precision mode
    convs = [c.conv for c in list(m.lateral_convs) + list(m.fpn_convs)] + \
        [c for u in m.upsample_modules for c in (u.channel_compressor, u.content_encoder)]
    assert len(convs) == 18 and all(c.exact for c in convs)
    with dynamask_amd.conv_precision('bf16x3'):
        assert all(c.precision_for(200, 336) == 'fp32' for c in convs)
    # two extra levels: the second reads the first's lateral
    two = necks.FPN_CARAFE(**dict(NECK, num_outs=5))
    assert [tuple(c.conv.weight.shape) for c in two.lateral_convs][3:] == [(16, 64, 3, 3), (16, 16, 3, 3)]
    assert len(two.upsample_modules) == 4 and two.upsample_modules[0].content_encoder.weight.shape == (100, 8, 3, 3)
    # start_level / end_level as the reference builds them
    part = necks.FPN_CARAFE(**dict(NECK, start_level=1, end_level=3, num_outs=2))
    assert [tuple(c.conv.weight.shape) for c in part.lateral_convs] == [(16, 32, 1, 1), (16, 64, 1, 1)] and len(part.upsample_modules) == 1
    k3 = necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(NECK['upsample_cfg'], up_kernel=3, up_group=2)))
    assert k3.upsample_modules[0].content_encoder.weight.shape == (72, 8, 3, 3)


@pytest.mark.parametrize('name', ['mask_rcnn_carafe', 'faster_rcnn_carafe'])
def test_build_detector_and_load_checkpoint(cfgs, golden_dir, tmp_path, name):
    import dynamask_amd
    from dynamask_amd import backbones, detectors, necks
    cfg = cfgs[name]
    before = copy.deepcopy(cfg)
    det = dynamask_amd.build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert cfg == before, 'the build changed the caller\'s config'
    assert type(det).__name__ == cfg['model']['type'] and type(det.backbone) is backbones.ResNet and type(det.neck) is necks.FPN_CARAFE
    assert det.with_neck and det.with_rpn and det.with_mask == (name == 'mask_rcnn_carafe')
    own = det.state_dict()
    have = [[k, list(v.shape)] for k, v in own.items()]
    want = cfg['state_dict']
    assert [k for k, _ in want if k.startswith('neck.')] == ['neck.' + k for k, _ in cfgs['mask_rcnn_carafe']['neck_state_dict']]
    assert have[:len(want)] == want
    rest = [k for k, _ in have[len(want):]]
    assert rest and all(k.startswith('roi_head.') for k in rest) and cfg['roi_head_keys'] is None
    with open(os.path.join(golden_dir, 'g29_detector_configs.json')) as f:
        r50 = json.load(f)['mask_rcnn']
    ref = dynamask_amd.build_detector(r50['model'], test_cfg=r50['test_cfg']).state_dict()
    if name == 'mask_rcnn_carafe':          # the plain detector's RoI head with CARAFEPack where the deconv stood
        assert cfg['model']['roi_head']['mask_head']['upsample_cfg']['type'] == 'carafe'
        up = [k for k in rest if '.mask_head.upsample.' in k]
        assert up == ['roi_head.mask_head.upsample.' + k for k in ('channel_compressor.weight', 'channel_compressor.bias',
                                                                  'content_encoder.weight', 'content_encoder.bias')]
        assert [k for k in rest if k not in up] == [k for k in ref if k.startswith('roi_head.') and '.mask_head.upsample.' not in k]
    else:
        assert rest == [k for k in ref if k.startswith('roi_head.') and '.mask_head.' not in k]         # box only
    # the test pipeline pads to a multiple of 64
    assert detectors.parse_test_pipeline(cfg['test_pipeline'])['size_divisor'] == 64
    # a whole seeded checkpoint with the reference's keys, through a file
    g = torch.Generator().manual_seed(32)
    state = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in own.items()}
    path = str(tmp_path / 'carafe.pth')
    torch.save({'state_dict': {'module.' + k: v for k, v in state.items()}, 'meta': {'epoch': 3}}, path)
    for p in det.parameters():
        p.data.zero_()
    assert detectors.load_checkpoint(det, path, strict=True) == ({'epoch': 3}, [], [])
    assert all(torch.equal(v, state[k]) for k, v in det.state_dict().items())
    broken = dict(state)
    del broken['neck.upsample_modules.3.content_encoder.weight']
    with pytest.raises(RuntimeError, match=r"missing keys \['neck.upsample_modules.3.content_encoder.weight'\]"):
        detectors.load_checkpoint(det, {'state_dict': broken}, strict=True)


def test_what_is_not_built_raises_by_name():
    from dynamask_amd import necks
    up = NECK['upsample_cfg']
    with pytest.raises(NotImplementedError, match='norm_cfg'):
        necks.FPN_CARAFE(**dict(NECK, norm_cfg=dict(type='GN', num_groups=32)))
    with pytest.raises(NotImplementedError, match='act_cfg'):
        necks.FPN_CARAFE(**dict(NECK, act_cfg=dict(type='ReLU')))
    with pytest.raises(NotImplementedError, match='order'):
        necks.FPN_CARAFE(**dict(NECK, order=('act', 'conv', 'norm')))
    for kind in ('nearest', 'bilinear', 'deconv', 'pixel_shuffle', None):
        with pytest.raises(NotImplementedError, match=f'upsample_cfg type={kind!r}'):
            necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(type=kind)))
    with pytest.raises(NotImplementedError, match='encoder_kernel=5'):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(up, encoder_kernel=5)))
    with pytest.raises(NotImplementedError, match='encoder_dilation=2'):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(up, encoder_dilation=2)))
    with pytest.raises(NotImplementedError, match='out_channels=20'):
        necks.FPN_CARAFE(**dict(NECK, out_channels=20))
    with pytest.raises(NotImplementedError, match='compressed_channels=12'):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(up, compressed_channels=12)))
    with pytest.raises(NotImplementedError, match='up_kernel=7'):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(up, up_kernel=7)))
    with pytest.raises(NotImplementedError, match='up_group=8'):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(up, up_group=8)))            # 2 channels per group
    with pytest.raises(NotImplementedError, match='scale_factor'):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(up, scale_factor=4)))
    # training
    m = necks.FPN_CARAFE(**NECK)
    xs = [torch.zeros(1, c, 8 >> i, 8 >> i) for i, c in enumerate(NECK['in_channels'])]
    with pytest.raises(NotImplementedError, match='training'):
        m(xs)
    # the registries the issue leaves alone
    import dynamask_amd
    assert dynamask_amd.NECKS.get('PAFPN') is None and dynamask_amd.DETECTORS.get('RetinaNet') is None


def test_the_references_asserts_hold():
    from dynamask_amd import necks
    with pytest.raises(AssertionError):
        necks.FPN_CARAFE(**dict(NECK, in_channels=(16, 32, 64)))                    # a list
    with pytest.raises(AssertionError):
        necks.FPN_CARAFE(**dict(NECK, order=('conv', 'act', 'norm')))
    with pytest.raises(AssertionError):
        necks.FPN_CARAFE(**dict(NECK, upsample_cfg=dict(type='bicubic')))
    with pytest.raises(AssertionError):
        necks.FPN_CARAFE(**dict(NECK, num_outs=2))                                  # num_outs >= the used inputs
    with pytest.raises(AssertionError):
        necks.FPN_CARAFE(**dict(NECK, end_level=4, num_outs=4))                     # end_level <= len(in_channels)
    with pytest.raises(AssertionError):
        necks.FPN_CARAFE(**dict(NECK, end_level=2, num_outs=3))                     # num_outs == end_level - start_level
    m = necks.FPN_CARAFE(**NECK)
    with torch.no_grad(), pytest.raises(AssertionError):
        m([torch.zeros(1, 16, 8, 8)])                                               # len(inputs) == len(in_channels)
    with torch.no_grad(), pytest.raises(ValueError, match='input 1'):
        m([torch.zeros(1, 16, 8, 8), torch.zeros(1, 16, 4, 4), torch.zeros(1, 64, 2, 2)])


def test_init_weights():
    from dynamask_amd import necks
    torch.manual_seed(3)
    m = necks.FPN_CARAFE(**NECK)
    for p in m.parameters():
        torch.nn.init.constant_(p, 7.0)
    m.init_weights()
    for mod in list(m.lateral_convs) + list(m.fpn_convs):
        w = mod.conv.weight.detach()
        fan_in, fan_out = w.shape[1] * w.shape[2] * w.shape[3], w.shape[0] * w.shape[2] * w.shape[3]
        bound = (6.0 / (fan_in + fan_out)) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.8 * bound and float(mod.conv.bias.detach().abs().sum()) == 0
    for u in m.upsample_modules:
        w = u.channel_compressor.weight.detach()
        assert float(w.abs().max()) <= (6.0 / (16 + 8)) ** 0.5 and float(w.std()) > 0.1
        e = u.content_encoder.weight.detach()
        assert 0.0005 < float(e.std()) < 0.002 and float(e.abs().max()) < 0.01                 # normal, std 0.001
        assert float(u.channel_compressor.bias.detach().abs().sum()) == 0 and float(u.content_encoder.bias.detach().abs().sum()) == 0


def test_abi_has_the_two_entry_points():
    import ctypes
    from dynamask_amd import _lib, hazard
    assert _lib.ABI_VERSION == 29
    assert 'dm_carafe_map_supported' in _lib.SIGNATURES and 'dm_carafe_map_fwd' in _lib.SIGNATURES
    args, res = _lib.SIGNATURES['dm_carafe_map_supported']
    assert args == [ctypes.c_int] * 8 and res is ctypes.c_int
    args, res = _lib.SIGNATURES['dm_carafe_map_fwd']
    P, I = ctypes.c_void_p, ctypes.c_int
    assert args == [P, P, I, I, I, I, I, I, P, I, I, I, P, P] and res is ctypes.c_int
    roles = hazard.parse_header()['dm_carafe_map_fwd']
    assert [r for r in roles if r != 'scalar'] == ['in', 'in', 'in', 'out', 'stream']


def test_supported_answers_from_host_arguments():
    from dynamask_amd import _lib, ops
    S = _lib.lib().dm_carafe_map_supported
    for K in (3, 5):
        for (NB, C, H, W, G) in ((1, 8, 1, 1, 1), (1, 8, 1, 1, 2), (0, 8, 1, 1, 1), (4, 256, 100, 168, 1), (2, 24, 37, 53, 2), (1, 4, 3, 3, 1)):
            for OH in (2 * H - 1, 2 * H):
                for OW in (2 * W - 1, 2 * W):
                    assert S(NB, C, H, W, K, G, OH, OW) == 1, (NB, C, H, W, K, G, OH, OW)
            assert S(NB, C, H, W, K, G, 2 * H - 2, 2 * W) == 0 and S(NB, C, H, W, K, G, 2 * H + 1, 2 * W) == 0
            assert S(NB, C, H, W, K, G, 2 * H, 2 * W - 2) == 0 and S(NB, C, H, W, K, G, 2 * H, 2 * W + 1) == 0
    for K in (0, 1, 2, 4, 7, -5):
        assert S(1, 8, 4, 4, K, 1, 8, 8) == 0
    assert S(1, 8, 4, 4, 5, 3, 8, 8) == 0                    # C % group
    assert S(1, 12, 4, 4, 5, 2, 8, 8) == 0                   # 6 channels per group: not whole quads
    assert S(1, 6, 4, 4, 5, 1, 8, 8) == 0
    assert S(1, 8, 4, 4, 5, 0, 8, 8) == 0 and S(1, 0, 4, 4, 5, 1, 8, 8) == 0 and S(-1, 8, 4, 4, 5, 1, 8, 8) == 0
    assert S(1, 8, 0, 4, 5, 1, 0, 8) == 0 and S(1, 8, 4, 0, 5, 1, 8, 0) == 0
    # element counts of 2^31 and more: out = 4 x that of x; enc = 100 / C x that of x
    assert S(1, 256, 1024, 2047, 5, 1, 2048, 4094) == 1      # out: 2^31 - 2^20
    assert S(1, 256, 1024, 1024, 5, 1, 2048, 2048) == 1      # out: 2^30
    assert S(1, 256, 1024, 2048, 5, 1, 2048, 4096) == 0      # out: 2^31
    assert S(2, 256, 1024, 1024, 5, 1, 2048, 2048) == 0      # out: 2^31 through the batch
    assert S(1, 4, 4096, 4096, 5, 1, 8192, 8192) == 1        # enc: 100 x 2^24 < 2^31, out 2^28
    assert S(1, 4, 8192, 4096, 5, 1, 16384, 8192) == 0       # enc: 100 x 2^25 >= 2^31 (x and out are below)
    assert S(1, 4, 8192, 4096, 3, 1, 16384, 8192) == 1       # ... 36 x 2^25 is not
    # the wrapper: a tensor or a shape, out_size defaults to 2H x 2W
    assert ops.carafe_map_supported((1, 256, 100, 168), 5, 1) and ops.carafe_map_supported(torch.zeros(1, 8, 3, 4), 3, 2, (5, 8))
    assert not ops.carafe_map_supported((1, 256, 100, 168), 5, 1, (198, 336)) and not ops.carafe_map_supported((1, 8, 3, 4), 4, 1)
    # CPU tensors: the operators run on the device only
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.carafe_map(torch.zeros(1, 8, 2, 2), torch.zeros(1, 100, 2, 2))


def test_restate_reproduces_the_stored_outputs(cfgs, golden_dir):
    """The torch restatement, on the CPU in float32, against the reference module's stored outputs and their float64
    twins: the fixture and the restatement the device tests lean on say the same thing.  The stored kernels are far from
    a box filter."""
    import fpn_carafe_inputs as ci
    cfg = cfgs['mask_rcnn_carafe']['model']['neck']
    state = ci.head_state({k: tuple(s) for k, s in cfgs['mask_rcnn_carafe']['neck_state_dict']}, ci.WEIGHT_SEED)
    xs = ci.inputs(cfg['in_channels'], ci.BATCH, seed=ci.FEAT_SEED)
    with torch.no_grad():
        outs, steps = ci.restate(cfg, state, xs, every_level=True)
    assert len(outs) == 5 and [s['level'] for s in steps] == [4, 3, 2, 1]
    assert [tuple(s['merged'].shape[2:]) for s in steps] == [(3, 4), (5, 7), (9, 14), (18, 27)]
    assert [tuple(s['src'].shape[2:]) for s in steps] == [(2, 2), (3, 4), (5, 7), (9, 14)]
    z = {}
    for name in sorted(set(ci.FILES)):
        z.update(np.load(os.path.join(golden_dir, name)))
    assert float(z['mean_max_tap']) > 2 / 25
    for l, got in enumerate(outs):
        ref32 = z[f'out{l}']
        assert tuple(got.shape) == ref32.shape
        assert_close_via_f64(got, ref32, ci.unpack_f64(ref32, z[f'out{l}_err16']), f'level {l}')
