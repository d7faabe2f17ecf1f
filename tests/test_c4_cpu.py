"""Mask R-CNN / Faster R-CNN C4 without a GPU: the registry builds StandardRoIHead with the ResLayer shared head and the plain
BBoxHead from the two unchanged configs (tests/golden/g25_c4_configs.json: the configs as resolved, and the reference
modules' state_dict lists), the eval-mode BatchNorm fold of a ResNet layer's blocks against float64 conv -> BatchNorm
(-> add -> ReLU) on the CPU and its refresh, every refusal, and the launchers' own reports (no device): the strided RoIAlign's
route (dm_roi_align_plan entry 3) and the builds the five convolution shapes of layer4 take (dm_conv2d_plan)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

SHARED = dict(type='ResLayer', depth=50, stage=3, stride=2, style='caffe', norm_cfg=dict(type='BN', requires_grad=False),
              norm_eval=True)


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g25_c4_configs.json')) as f:
        return json.load(f)


def _build(cfg):
    from dynamask_amd import registry, roi_head, bbox_heads, mask_heads, losses, roi_extractors  # noqa: F401
    c = registry._to_cfgdict(cfg)
    rh = dict(c.model.roi_head)
    rh.update(train_cfg=None, test_cfg=c.test_cfg.rcnn)
    return registry.build_head(rh)


@pytest.fixture(scope='module')
def heads(cfgs):
    return {name: _build(cfgs[name]) for name in cfgs}


def _small_layer(stride=2, seed=5):
    """ResLayer at planes 16: 32 -> 64 channels, six blocks."""
    import c4_inputs as ci
    from dynamask_amd.shared_heads import ResLayer
    m = ResLayer(depth=50, stage=-2, stride=stride, style='caffe')
    state = ci.head_state({'shared_head.' + k: v.shape for k, v in m.state_dict().items()}, seed)
    m.load_state_dict({k[len('shared_head.'):]: v for k, v in state.items()}, strict=True)
    return m.eval()


# ------------------------------------------------------------------------------------------------ configs and keys
def test_both_configs_build_unchanged(cfgs, heads):
    from dynamask_amd import bbox_heads, mask_heads, registry, shared_heads
    from dynamask_amd import roi_head as rh
    assert cfgs['mask_c4']['source'] == 'configs/mask_rcnn/mask_rcnn_r50_caffe_c4_1x_coco.py'
    assert cfgs['faster_c4']['source'] == 'configs/faster_rcnn/faster_rcnn_r50_caffe_c4_1x_coco.py'
    assert registry.SHARED_HEADS.get('ResLayer') is shared_heads.ResLayer and registry.HEADS.get('BBoxHead') is bbox_heads.BBoxHead
    for name, m in heads.items():
        assert type(m) is rh.StandardRoIHead and m.with_shared_head and m.with_bbox
        assert type(m.shared_head) is shared_heads.ResLayer and type(m.bbox_head) is bbox_heads.BBoxHead
        s, b = m.shared_head, m.bbox_head
        assert (s.depth, s.stage, s.stride, s.style, s.inplanes, s.planes, s.out_channels) == (50, 3, 2, 'caffe', 1024, 512, 2048)
        assert len(s.layer4) == 3 and s.layer4[0].downsample is not None and s.layer4[1].downsample is None
        assert b.with_avg_pool and b.in_channels == 2048 and b.roi_feat_size == (7, 7) and b.num_classes == 80
        assert b.fc_cls.in_features == 2048 and b.fc_reg.out_features == 320
        assert m.bbox_roi_extractor.roi_layers[0].output_size == (14, 14) and m.bbox_roi_extractor.featmap_strides == [16]
    mask, faster = heads['mask_c4'], heads['faster_c4']
    assert mask.with_mask and mask.share_roi_extractor is True and mask.mask_roi_extractor is mask.bbox_roi_extractor
    assert type(mask.mask_head) is mask_heads.FCNMaskHead and mask.mask_head.num_convs == 0
    assert mask._mask_logits_size() == (80, 14)          # 14 -> 7 by the shared head's stride, x 2 by the deconvolution
    assert not faster.with_mask
    # without the two arguments nothing changed: the stock head has neither attribute set
    stock = rh.StandardRoIHead()
    assert not stock.with_shared_head and not hasattr(stock, 'share_roi_extractor')


@pytest.mark.parametrize('name', ['mask_c4', 'faster_c4'])
def test_state_dict_is_the_references(cfgs, heads, name):
    want = [(k, tuple(s)) for k, s in cfgs[name]['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in heads[name].state_dict().items()]
    assert sorted(got) == sorted(want)
    keys = dict(got)
    assert keys['shared_head.layer4.0.conv1.weight'] == (512, 1024, 1, 1)
    assert keys['shared_head.layer4.0.downsample.0.weight'] == (2048, 1024, 1, 1)
    assert keys['shared_head.layer4.0.downsample.1.running_var'] == (2048,)
    assert keys['shared_head.layer4.2.conv3.weight'] == (2048, 512, 1, 1)
    assert 'shared_head.layer4.1.downsample.0.weight' not in keys and 'shared_head.layer4.0.conv1.bias' not in keys
    assert keys['bbox_head.fc_cls.weight'] == (81, 2048) and keys['bbox_head.fc_reg.weight'] == (320, 2048)
    if name == 'mask_c4':
        assert keys['mask_head.upsample.weight'] == (2048, 256, 2, 2) and keys['mask_head.conv_logits.weight'] == (80, 256, 1, 1)
        assert not any(k.startswith('mask_roi_extractor.') for k in keys)


def test_head_state_loads_strictly(heads):
    import c4_inputs as ci
    m = heads['mask_c4']
    state = ci.head_state({k: v.shape for k, v in m.state_dict().items()}, 26)
    own = {k for k in m.state_dict() if k.startswith(ci.HEAD_PREFIXES)}
    assert set(state) == own
    res = m.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and all(not k.startswith(ci.HEAD_PREFIXES) for k in res.missing_keys)
    assert torch.equal(m.shared_head.layer4[0].downsample[1].running_var, state['shared_head.layer4.0.downsample.1.running_var'])


# ------------------------------------------------------------------------------------------------ the fold
def _conv_bn(x, w, bn, dtype):
    y = F.conv2d(x.to(dtype), w.detach().to(dtype), padding=w.shape[-1] // 2)
    return F.batch_norm(y, bn.running_mean.to(dtype), bn.running_var.to(dtype), bn.weight.detach().to(dtype),
                        bn.bias.detach().to(dtype), False, 0.0, bn.eps)


def _block_ref(b, x, dtype):
    """backbones/resnet.py's Bottleneck.forward in eval mode (the stride already taken from ``x``)."""
    h = F.relu(_conv_bn(x, b.conv1.weight, b.bn1, dtype))
    h = F.relu(_conv_bn(h, b.conv2.weight, b.bn2, dtype))
    h = _conv_bn(h, b.conv3.weight, b.bn3, dtype)
    idn = x.to(dtype) if b.downsample is None else _conv_bn(x, b.downsample[0].weight, b.downsample[1], dtype)
    return F.relu(h + idn)


def _block_folded(b, x):
    """The block's three launches as F.conv2d of its folded weights on the CPU."""
    (w1, b1), (w2, b2), (w3, b3) = (f.folded() for f in b._f)
    h = F.relu(F.conv2d(x, w1, b1))
    h = F.relu(F.conv2d(h, w2, b2, padding=1))
    if b.downsample is not None:
        return F.relu(F.conv2d(torch.cat([h, x], 1), w3, b3))
    return F.relu(x + F.conv2d(h, w3, b3))


def test_fold_of_the_merged_launch_and_of_a_plain_bottleneck():
    m = _small_layer()
    g = torch.Generator().manual_seed(11)
    b0, b1 = m.res_layer[0], m.res_layer[1]
    assert not torch.equal(b0.downsample[1].running_var, torch.ones(64))
    # block 0: [W3' | Wd'] with bias b3' + bd'
    w, b = b0._f[2].folded()
    assert w.dtype == torch.float32 and tuple(w.shape) == (64, 16 + 32, 1, 1) and tuple(b.shape) == (64,)
    assert b0._f[2].src_channels == [16, 32]
    hmid, x = torch.randn(3, 16, 7, 7, generator=g), torch.randn(3, 32, 7, 7, generator=g)
    ref = {d: _conv_bn(hmid, b0.conv3.weight, b0.bn3, d) + _conv_bn(x, b0.downsample[0].weight, b0.downsample[1], d)
           for d in (torch.float32, torch.float64)}
    assert_close_via_f64(F.conv2d(torch.cat([hmid, x], 1), w, b), ref[torch.float32], ref[torch.float64], 'merged fold')
    assert_close_via_f64(_block_folded(b0, x), _block_ref(b0, x, torch.float32), _block_ref(b0, x, torch.float64), 'block 0')
    # a plain bottleneck: conv -> BatchNorm -> add -> ReLU
    x64 = torch.randn(3, 64, 7, 7, generator=g)
    w, b = b1._f[2].folded()
    assert tuple(w.shape) == (64, 16, 1, 1)
    assert_close_via_f64(_block_folded(b1, x64), _block_ref(b1, x64, torch.float32), _block_ref(b1, x64, torch.float64), 'block 1')
    # without the fold the answer is far away: the comparison above can fail
    with pytest.raises(AssertionError):
        assert_close_via_f64(F.conv2d(torch.cat([hmid, x], 1), torch.cat([b0.conv3.weight, b0.downsample[0].weight], 1).detach()),
                             ref[torch.float32], ref[torch.float64], 'no fold')


def test_fold_is_float64_rounded_once_and_shared_with_the_double_head():
    from dynamask_amd import bbox_heads, layers, shared_heads
    assert shared_heads.Bottleneck is bbox_heads.Bottleneck          # one block class, one fold
    m = _small_layer()
    b0 = m.res_layer[0]
    pairs = [(b0.conv3.weight, b0.bn3), (b0.downsample[0].weight, b0.downsample[1])]
    w, b = layers.fold_bn(pairs)
    ws, bs = [], 0
    for cw, bn in pairs:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        ws.append(cw.detach().double() * s[:, None, None, None])
        bs = bs + bn.bias.detach().double() - bn.running_mean.double() * s
    assert torch.equal(w, torch.cat(ws, 1).float()) and torch.equal(b, bs.float())
    got = b0._f[2].folded()
    assert torch.equal(got[0], w) and torch.equal(got[1], b)


def test_fold_is_refreshed_after_load_state_dict():
    import c4_inputs as ci
    from dynamask_amd.layers import fold_bn
    m = _small_layer(seed=5)
    f = m.res_layer[0]._f[2]
    w0, b0 = f.folded()
    assert f.folded()[0] is w0                                    # cached
    state = ci.head_state({'shared_head.' + k: v.shape for k, v in m.state_dict().items()}, 6)
    m.load_state_dict({k[len('shared_head.'):]: v for k, v in state.items()}, strict=True)
    w1, b1 = f.folded()
    assert not torch.equal(w1, w0) and not torch.equal(b1, b0)
    blk = m.res_layer[0]
    want = fold_bn([(blk.conv3.weight, blk.bn3), (blk.downsample[0].weight, blk.downsample[1])])
    assert torch.equal(w1, want[0]) and torch.equal(b1, want[1])
    with torch.no_grad():
        blk.downsample[1].running_mean.add_(1.0)                  # a buffer of the identity path alone
    w2, b2 = f.folded()
    assert torch.equal(w2, w1) and not torch.equal(b2, b1)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('arg,kw', [
    ('depth', dict(depth=18)), ('depth', dict(depth=34)), ('stride', dict(stride=3)), ('stride', dict(stride=0)),
    ('dilation', dict(dilation=2)), ('style', dict(style='pytorch')), ('style', dict()),
    ('norm_cfg', dict(norm_cfg=dict(type='GN', num_groups=32))), ('norm_cfg', dict(norm_cfg=dict(type='SyncBN'))),
    ('norm_cfg', dict(norm_cfg=None)), ('dcn', dict(dcn=dict(type='DCN', deform_groups=1)))])
def test_res_layer_refusals_name_the_argument(arg, kw):
    from dynamask_amd.shared_heads import ResLayer
    args = dict(depth=50, style='caffe')
    if kw == dict():
        args.pop('style')                                          # the reference's default is 'pytorch'
    args.update(kw)
    with pytest.raises(NotImplementedError, match=arg):
        ResLayer(**args)


def test_res_layer_accepts_what_the_table_says():
    from dynamask_amd.shared_heads import ResLayer
    with pytest.raises(KeyError):
        ResLayer(depth=51, style='caffe')
    for depth, blocks in ((50, 3), (101, 3), (152, 3)):
        m = ResLayer(depth=depth, stage=3, style='caffe', with_cp=True)
        assert len(m.layer4) == blocks
    assert len(ResLayer(depth=101, stage=2, stride=1, style='caffe').layer3) == 23
    m = ResLayer(depth=50, stage=1, stride=1, style='caffe')
    assert (m.inplanes, m.planes, m.out_channels) == (256, 128, 512) and len(m.layer2) == 4
    small = _small_layer()
    with torch.no_grad():
        assert tuple(small.forward_sampled(torch.zeros(0, 32, 4, 4)).shape) == (0, 64, 4, 4)
        assert tuple(small(torch.zeros(0, 32, 7, 7)).shape) == (0, 64, 4, 4)
        with pytest.raises(ValueError):
            small.forward_sampled(torch.zeros(2, 16, 4, 4))        # the channel count
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        with torch.no_grad():
            small(torch.zeros(2, 32, 7, 7))


def test_training_is_refused(heads):
    small = _small_layer()
    x = torch.zeros(2, 32, 7, 7)
    with pytest.raises(NotImplementedError, match='training'):
        small(x)
    with pytest.raises(NotImplementedError, match='training'):
        small.forward_sampled(x)
    with torch.no_grad():
        for p in small.parameters():
            p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='training'):
        small(x.requires_grad_(True))
    from dynamask_amd.bbox_heads import BBoxHead
    with pytest.raises(NotImplementedError, match='training'):
        BBoxHead(with_avg_pool=True, in_channels=8, num_classes=3)(torch.zeros(2, 8, 7, 7))
    for m in heads.values():
        with pytest.raises(NotImplementedError, match='shared head'):
            m.forward_train(None, None, None, None, None)


def test_bbox_head_arguments():
    from dynamask_amd.bbox_heads import BBoxHead
    with pytest.raises(NotImplementedError, match='reg_decoded_bbox'):
        BBoxHead(reg_decoded_bbox=True)
    with pytest.raises(AssertionError):
        BBoxHead(with_cls=False, with_reg=False)
    flat = BBoxHead(with_avg_pool=False, in_channels=8, roi_feat_size=7, num_classes=3)
    assert flat.fc_cls.in_features == 8 * 49 and flat.fc_reg.out_features == 12
    assert sorted(flat.state_dict()) == ['fc_cls.bias', 'fc_cls.weight', 'fc_reg.bias', 'fc_reg.weight']
    only_cls = BBoxHead(with_avg_pool=True, in_channels=8, num_classes=3, with_reg=False)
    assert sorted(only_cls.state_dict()) == ['fc_cls.bias', 'fc_cls.weight'] and only_cls.fc_cls.in_features == 8
    only_reg = BBoxHead(with_avg_pool=True, in_channels=8, num_classes=3, with_cls=False, reg_class_agnostic=True)
    assert sorted(only_reg.state_dict()) == ['fc_reg.bias', 'fc_reg.weight'] and only_reg.fc_reg.out_features == 4
    with torch.no_grad():
        c, r = only_cls(torch.zeros(0, 8, 7, 7))
        assert tuple(c.shape) == (0, 4) and r is None
        c, r = only_reg(torch.zeros(0, 8, 7, 7))
        assert c is None and tuple(r.shape) == (0, 4)
        with pytest.raises(ValueError):
            only_cls(torch.zeros(2, 8, 14, 14))                     # the average pool is over roi_feat_size
    torch.manual_seed(0)
    flat.init_weights()
    assert float(flat.fc_cls.bias.detach().abs().max()) == 0 and 0.005 < float(flat.fc_cls.weight.detach().std()) < 0.02
    assert float(flat.fc_reg.bias.detach().abs().max()) == 0 and 0.0005 < float(flat.fc_reg.weight.detach().std()) < 0.002
    assert BBoxHead.get_bboxes is __import__('dynamask_amd.bbox_heads', fromlist=['x']).Shared2FCBBoxHead.get_bboxes


def test_subclasses_refuse_a_shared_head_in_their_constructors():
    from dynamask_amd import roi_head as rh
    cases = [(rh.DynaMaskRoIHead, {}), (rh.RefineRoIHead, {}), (rh.PointRendRoIHead, dict(point_head=None)),
             (rh.PointRefineRoIHead, {}), (rh.MaskScoringRoIHead, dict(mask_iou_head=dict(type='MaskIoUHead'))),
             (rh.GridRoIHead, dict(grid_head=dict(type='GridHead'))), (rh.DoubleHeadRoIHead, dict(reg_roi_scale_factor=1.3))]
    assert {c for c, _ in cases} | {rh.StandardRoIHead, rh.CascadeRoIHead, rh.HybridTaskCascadeRoIHead} == \
        {c for c in vars(rh).values() if isinstance(c, type) and issubclass(c, rh.StandardRoIHead)}
    for cls, kw in cases:
        with pytest.raises(NotImplementedError, match='shared_head'):
            cls(shared_head=dict(SHARED), **kw)
        assert cls._applies_shared_head() is False
    assert rh.StandardRoIHead._applies_shared_head() is True
    assert type('Renamed', (rh.StandardRoIHead,), {})._applies_shared_head() is True       # no path of its own


def test_strided_extraction_arguments_without_a_device():
    from dynamask_amd import roi_extractors
    ext = roi_extractors.SingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0), out_channels=1024,
                                            featmap_strides=[16])
    feats = [torch.zeros(1, 1024, 20, 30)]
    assert tuple(ext(feats, torch.zeros(0, 5), bin_step=2).shape) == (0, 1024, 7, 7)
    assert tuple(ext(feats, torch.zeros(0, 5)).shape) == (0, 1024, 14, 14)
    assert ext.supports_bin_step(feats, 2) and not ext.supports_bin_step([torch.zeros(1, 1022, 20, 30)], 2)
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError):
            ext(feats, torch.zeros(2, 5), bin_step=bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):      # the step reaches the operator, which wants the GPU
        ext(feats, torch.zeros(2, 5), bin_step=2)
    four = roi_extractors.SingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=8,
                                             featmap_strides=[4, 8, 16, 32])
    with pytest.raises(NotImplementedError):
        four([torch.zeros(1, 8, 8, 8)] * 4, torch.zeros(2, 5), roi_scale_factor=1.3, bin_step=2)


# ------------------------------------------------------------------------------------------------ the launchers' reports
PYRAMID = [(200, 336), (100, 168), (50, 84), (25, 42)]


@pytest.mark.parametrize('N', [1, 193, 1030])
def test_the_strided_entry_is_one_launch_at_16_channels(N, monkeypatch):
    """dm_roi_align_plan entry 3: whatever N and the DM_ROI_SORT* knobs say, one tile launch at 16 channels per workgroup
    that writes the levels -- the unordered dense call's route, where the ordered call of 193 RoIs takes 32 channels."""
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    assert ops.ROI_ENTRY_STRIDED == 'strided' and 'strided' not in ops.ROI_ENTRIES
    tile = ops.ROI_KERNELS.index('tile')
    for maps, C in (([(50, 84)], 1024), (PYRAMID, 72)):
        one, = ops.roi_align_plan('strided', maps, 2, C, N, 14, bin_step=2)
        chunks = -(-C // 16)
        assert one == dict(kernel=tile, P0=3, P1=2, grid=N * chunks, threads=256, lds_bytes=(2048 + 64) * 16, CT=16,
                           order=1 if chunks % 8 == 0 else 0, lds_floats=0, levels=1)
        dense, = ops.roi_align_plan('forward', maps, 2, C, N, 14, workspace=0)
        assert (dense['kernel'], dense['P0'], dense['CT'], dense['grid'], dense['order'], dense['lds_bytes']) == \
            (tile, 0, 16, one['grid'], one['order'], one['lds_bytes'])
        for sort, sort_min in (('0', '192'), ('1', '1')):
            monkeypatch.setenv('DM_ROI_SORT', sort)
            monkeypatch.setenv('DM_ROI_SORT_MIN', sort_min)
            lib().dm_reload_env_knobs()
            assert ops.roi_align_plan('strided', maps, 2, C, N, 14, bin_step=2) == [one]
        monkeypatch.delenv('DM_ROI_SORT')
        monkeypatch.delenv('DM_ROI_SORT_MIN')
        lib().dm_reload_env_knobs()
    if N == 193:
        assert [r['CT'] for r in ops.roi_align_plan('forward', [(50, 84)], 2, 1024, N, 14)] == [0, 32]


def test_strided_support_is_the_tile_kernels():
    from dynamask_amd import ops
    from dynamask_amd._abi import load
    consts = load()[1]
    INVALID, UNSUPPORTED = consts['DM_ERR_INVALID_ARG'], consts['DM_ERR_UNSUPPORTED']
    sup = ops.roi_align_strided_supported
    raw = lambda maps, C, P, step, N=5: ops.roi_align_plan_raw('strided', maps, 2, C, N, P, pool=step)[0]      # noqa: E731
    one = [(50, 84)]
    for maps in (one, PYRAMID[:2], PYRAMID[:3], PYRAMID):
        for P in (2, 7, 14, 16):
            for C in (4, 20, 1024):
                assert sup(maps, C, P, 2) and raw(maps, C, P, 2) == 1, (len(maps), P, C)
    # where the dense call leaves the tile kernel the strided one is refused
    for maps, C, P in ((one, 6, 14), (one, 1022, 14), (one, 256, 17), (one, 256, 28), (one, 256, 1), ([(2796203, 3)], 256, 14)):
        assert not sup(maps, C, P, 2) and raw(maps, C, P, 2) == UNSUPPORTED, (maps, C, P)
        assert ops.ROI_KERNELS[ops.roi_align_plan('forward', maps, 2, C, 5, P)[0]['kernel']] != 'tile' or P == 1
    assert sup(one, 256, 14, 1) and sup(one, 256, 14, 14) and not sup(one, 256, 14, 15) and not sup(one, 256, 14, 0)
    assert raw(one, 256, 14, 15) == UNSUPPORTED and raw(one, 256, 14, 0) == INVALID and raw(one, 256, 14, -2) == INVALID
    assert not sup(PYRAMID + [(13, 21)], 256, 14, 2) and not sup([], 256, 14, 2)
    assert raw(one, 256, 14, 2, N=0) == 0 and raw(one, 0, 14, 2) == INVALID and raw(one, 256, 14, 2, N=-1) == INVALID
    # the entry takes no workspace
    assert ops.roi_align_plan_raw('strided', one, 2, 256, 5, 14, workspace_bytes=64, workspace=1, pool=2)[0] == INVALID


def _builds(name, nb):
    import c4_inputs as ci
    from dynamask_amd import ops
    src, cout, k, acc = ci.CONV_SHAPES[name]
    recs = ops.conv2d_plan(list(src), nb, 7, 7, cout, k, relu=True, accumulate=acc)
    return {tuple(r[f] for f in ops.CONV_PLAN_FIELDS[:9]) for r in recs}


@pytest.mark.parametrize('name', ['block0_conv1_1x1', 'conv2_3x3', 'block0_merged_1x1', 'conv1_1x1', 'conv3_1x1_accumulate'])
def test_gpu_test_sizes_reach_every_build_of_the_1000_roi_call(name):
    """dm_conv2d_plan needs no device: the launcher takes every one of layer4's five shapes, and the RoI counts
    tests/test_c4_gpu.py runs select, between them, every build that the 1000-RoI call selects -- at the smallest count
    that does; no launch of the 1000-RoI call is split along K."""
    import c4_inputs as ci
    from dynamask_amd import ops
    nbs = ci.CONV_TEST_NBS[name]
    assert 3 in nbs
    at_1000 = _builds(name, 1000)
    assert at_1000 and at_1000 <= set().union(*[_builds(name, nb) for nb in nbs])
    for nb in nbs:
        if nb > 3:
            assert _builds(name, nb) != _builds(name, nb - 1), f'{nb} is not the smallest count of its build'
    src, cout, k, acc = ci.CONV_SHAPES[name]
    for rec in ops.conv2d_plan(list(src), 1000, 7, 7, cout, k, relu=True, accumulate=acc):
        assert rec.get('splits', 1) in (0, 1), rec
