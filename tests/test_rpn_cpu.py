"""RPN inference without a GPU: the registry builds RPNHead from the unchanged ``model.rpn_head`` / ``test_cfg.rpn`` of the FPN
and the C4 Mask R-CNN configs (tests/golden/g26_rpn_configs.json: the configs as resolved and the reference module's
state_dict list), AnchorGenerator's base anchors and grid against the reference's bit for bit (g26_rpn.npz), every refusal,
and the ``dm_rpn_*_supported`` checks at their stated limits (no device)."""
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, 'g26_rpn_configs.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'g26_rpn.npz')))


def _build(cfg, **over):
    from dynamask_amd import dense_heads, registry  # noqa: F401
    c = registry._to_cfgdict(cfg)
    rh = dict(c.model.rpn_head)
    rh.update(train_cfg=None, test_cfg=c.test_cfg.rpn)
    rh.update(over)
    return registry.build_head(rh)


@pytest.fixture(scope='module')
def heads(cfgs):
    return {form: _build(cfgs[form]) for form in cfgs}


# ------------------------------------------------------------------------------------------------ configs and keys
def test_both_configs_build_unchanged(cfgs, heads):
    from dynamask_amd import anchors, dense_heads, registry
    assert cfgs['fpn']['source'] == 'configs/_base_/models/mask_rcnn_r50_fpn.py'
    assert cfgs['c4']['source'] == 'configs/_base_/models/mask_rcnn_r50_caffe_c4.py'
    assert registry.HEADS.get('RPNHead') is dense_heads.RPNHead
    assert registry.ANCHOR_GENERATORS.get('AnchorGenerator') is anchors.AnchorGenerator
    fpn, c4 = heads['fpn'], heads['c4']
    for m in (fpn, c4):
        assert type(m) is dense_heads.RPNHead and type(m.anchor_generator) is anchors.AnchorGenerator
        assert m.use_sigmoid_cls and m.cls_out_channels == 1 and m.bbox_coder.means == (0., 0., 0., 0.)
        assert m.bbox_coder.stds == (1., 1., 1., 1.)
        assert m.rpn_conv.exact and m.rpn_cls.exact and m.rpn_reg.exact      # the bf16x3 mode does not reach the RPN
        assert m.test_cfg.nms_post == 1000 and m.test_cfg.nms_thr == 0.7 and m.test_cfg.min_bbox_size == 0
    assert (fpn.in_channels, fpn.feat_channels, fpn.num_anchors, fpn.anchor_generator.num_levels) == (256, 256, 3, 5)
    assert fpn.anchor_generator.strides == [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64)] and fpn.test_cfg.nms_pre == 1000
    assert fpn.anchor_generator.num_base_anchors == [3] * 5
    assert (c4.in_channels, c4.feat_channels, c4.num_anchors, c4.anchor_generator.num_levels) == (1024, 1024, 15, 1)
    assert c4.anchor_generator.strides == [(16, 16)] and c4.test_cfg.nms_pre == 6000
    # the loss configs are stored, not built
    assert fpn.loss_cls_cfg['type'] == 'CrossEntropyLoss' and fpn.loss_bbox_cfg['type'] == 'L1Loss'
    assert not any(isinstance(v, torch.nn.Module) and 'loss' in k.lower() for k, v in fpn.named_modules())


@pytest.mark.parametrize('form', ['fpn', 'c4'])
def test_state_dict_is_the_references(cfgs, heads, form):
    want = [(k, tuple(s)) for k, s in cfgs[form]['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in heads[form].state_dict().items()]
    assert sorted(got) == sorted(want)
    assert sorted(k for k, _ in got) == ['rpn_cls.bias', 'rpn_cls.weight', 'rpn_conv.bias', 'rpn_conv.weight', 'rpn_reg.bias',
                                         'rpn_reg.weight']
    A, C, F = heads[form].num_anchors, heads[form].in_channels, heads[form].feat_channels
    assert dict(got)['rpn_conv.weight'] == (F, C, 3, 3) and dict(got)['rpn_cls.weight'] == (A, F, 1, 1)
    assert dict(got)['rpn_reg.weight'] == (4 * A, F, 1, 1)


def test_head_state_loads_strictly(heads):
    import rpn_inputs as ri
    m = heads['fpn']
    state = ri.head_state({k: v.shape for k, v in m.state_dict().items()}, 3)
    m.load_state_dict(state, strict=True)
    assert torch.equal(m.rpn_cls.bias, state['rpn_cls.bias'])
    torch.manual_seed(0)
    m.init_weights()
    assert float(m.rpn_conv.bias.detach().abs().max()) == 0 and 0.009 < float(m.rpn_conv.weight.detach().std()) < 0.011


# ------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('form', ['fpn', 'c4'])
def test_anchors_are_the_references_bit_for_bit(golden, heads, form):
    import rpn_inputs as ri
    gen = heads[form].anchor_generator
    base = torch.cat(gen.base_anchors)
    assert base.dtype == torch.float32 and np.array_equal(base.numpy(), golden[f'{form}_base_anchors'])
    assert np.array_equal(torch.cat(gen.gen_base_anchors()).numpy(), golden[f'{form}_base_anchors'])
    sizes = ri.map_sizes([s[0] for s in gen.strides])
    grids = gen.grid_anchors(sizes, device='cpu')
    seen = 0
    for l, g in enumerate(grids):
        assert tuple(g.shape) == (sizes[l][0] * sizes[l][1] * gen.num_base_anchors[l], 4) and g.dtype == torch.float32
        if f'{form}_grid{l}' in golden:
            assert np.array_equal(g.numpy(), golden[f'{form}_grid{l}'])
            seen += 1
    assert seen == (3 if form == 'fpn' else 1)
    table, rows = gen.base_anchor_table('cpu')
    assert torch.equal(table, base) and rows == [sum(gen.num_base_anchors[:l]) for l in range(gen.num_levels)]
    with pytest.raises(ValueError):
        gen.grid_anchors(sizes + [(1, 1)], device='cpu')


def test_anchor_generator_arguments():
    from dynamask_amd.anchors import AnchorGenerator
    # the reference's docstring example (anchor_generator.py:41-47)
    g = AnchorGenerator([16], [1.], [1.], [9])
    want = torch.tensor([[-4.5, -4.5, 4.5, 4.5], [11.5, -4.5, 20.5, 4.5], [-4.5, 11.5, 4.5, 20.5], [11.5, 11.5, 20.5, 20.5]])
    assert torch.equal(g.grid_anchors([(2, 2)], device='cpu')[0], want)
    # octave scales, non-square strides (the smaller one is the base size), scale_major, centers, center_offset
    o = AnchorGenerator(strides=[(8, 16)], ratios=[0.5, 2.0], octave_base_scale=4, scales_per_octave=3)
    assert o.base_sizes == [8] and o.num_base_anchors == [6]
    assert torch.allclose(o.scales, torch.tensor([4.0, 4 * 2 ** (1 / 3), 4 * 2 ** (2 / 3)]))
    grid = o.grid_anchors([(2, 3)], device='cpu')[0].view(2, 3, 6, 4)
    assert torch.equal(grid[0, 0], o.base_anchors[0])
    assert torch.equal(grid[1, 2], o.base_anchors[0] + torch.tensor([2 * 8., 1 * 16., 2 * 8., 1 * 16.]))
    major = AnchorGenerator([8], [0.5, 2.0], [1., 2.]).base_anchors[0]
    minor = AnchorGenerator([8], [0.5, 2.0], [1., 2.], scale_major=False).base_anchors[0]
    assert torch.equal(major[[0, 2, 1, 3]], minor) and not torch.equal(major, minor)
    c = AnchorGenerator([8], [1.], [1.], centers=[(3.0, 5.0)]).base_anchors[0]
    assert torch.equal(c, torch.tensor([[-1., 1., 7., 9.]]))
    off = AnchorGenerator([8], [1.], [1.], center_offset=0.5).base_anchors[0]
    assert torch.equal(off, torch.tensor([[0., 0., 8., 8.]]))
    for bad in (dict(scales=None), dict(scales=[1.], octave_base_scale=4, scales_per_octave=3), dict(scales=[1.], center_offset=2.0),
                dict(scales=[1.], centers=[(0, 0)], center_offset=0.5), dict(scales=[1.], centers=[(0, 0), (1, 1)]),
                dict(scales=[1.], base_sizes=[4, 8])):
        with pytest.raises(ValueError):
            AnchorGenerator(strides=[8], ratios=[1.], **bad)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_argument(cfgs, heads):
    with pytest.raises(NotImplementedError, match='use_sigmoid'):
        _build(cfgs['fpn'], loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    with pytest.raises(NotImplementedError, match='use_sigmoid'):
        _build(cfgs['fpn'], loss_cls=dict(type='CrossEntropyLoss', loss_weight=1.0))
    m = heads['fpn']
    for name in ('loss', 'forward_train', 'aug_test_rpn'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(m, name)(None, None)
    import rpn_inputs as ri
    metas = ri.img_metas()
    cls = [torch.zeros(2, 3, h, w) for h, w in ri.map_sizes([4, 8, 16, 32, 64])]
    reg = [torch.zeros(2, 12, h, w) for h, w in ri.map_sizes([4, 8, 16, 32, 64])]
    base = dict(m.test_cfg)
    with pytest.raises(NotImplementedError, match='min_bbox_size'):
        m.get_bboxes(cls, reg, metas, cfg=dict(base, min_bbox_size=2))
    with pytest.raises(NotImplementedError, match='nms_across_levels'):
        m.get_bboxes(cls, reg, metas, cfg=dict(base, nms_across_levels=True))
    with pytest.raises(ValueError, match='levels'):
        m.get_bboxes(cls[:4], reg[:4], metas)
    with pytest.raises(ValueError, match='level 0'):
        m.get_bboxes([reg[0]] + cls[1:], reg, metas)
    with pytest.raises(ValueError, match='level 2'):
        m.get_bboxes(cls, reg[:2] + [reg[2][:1]] + reg[3:], metas)
    assert m.get_bboxes([c[:0] for c in cls], [r[:0] for r in reg], []) == []
    # the maps reach the operators, which want the GPU: no CPU fallback, in either path
    from dynamask_amd import dense_heads
    for fused in (True, False):
        dense_heads.RPN_FUSED[0] = fused
        try:
            with pytest.raises((RuntimeError, TypeError), match='no CPU fallback|on the device'):
                m.get_bboxes(cls, reg, metas)
        finally:
            dense_heads.RPN_FUSED[0] = True
    with pytest.raises(NotImplementedError, match='training'):
        m([torch.zeros(1, 256, 4, 4)])
    with torch.no_grad():
        with pytest.raises(ValueError, match='256'):
            m([torch.zeros(1, 128, 4, 4)])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m([torch.zeros(1, 256, 4, 4)])


def test_fused_flag_follows_the_environment(monkeypatch):
    from dynamask_amd import dense_heads
    assert dense_heads.RPN_FUSED == [dense_heads._env_fused()]
    monkeypatch.setenv('DM_RPN_FUSED', '0')
    assert dense_heads._env_fused() is False
    monkeypatch.setenv('DM_RPN_FUSED', '1')
    assert dense_heads._env_fused() is True
    monkeypatch.delenv('DM_RPN_FUSED')
    assert dense_heads._env_fused() is True


# ------------------------------------------------------------------------------------------------ the support checks
def test_supported_functions_at_their_limits():
    from dynamask_amd import ops
    from dynamask_amd._abi import load
    from dynamask_amd._lib import lib
    consts = load()[1]
    assert consts['DM_ABI_VERSION'] == 29 and consts['DM_RPN_SEG_WORDS'] == 12 and consts['DM_RPN_SELECT_CHUNK'] == 4096
    assert ops.RPN_SELECT_CHUNK == 4096 and ops.RPN_SEG_WORDS == 12
    M = 1 << 20
    sel = ops.rpn_select_supported
    assert sel(1, 1) and sel(0, 0) and sel(5, 201600, 268569) and sel(65535, M, 65535 * M) and sel(1, M)
    assert not sel(65536, 10) and not sel(1, M + 1) and not sel(-1, 10) and not sel(1, -1)
    assert not sel(2, 10, 21) and sel(2, 10, 20) and not sel(2, 10, -1)
    dec = ops.rpn_decode_supported
    assert dec(1, 1) and dec(0, 0) and dec(65535, M, 7) and not dec(65536, 1) and not dec(1, M + 1) and not dec(1, 1, 0)
    assert not dec(-1, 1) and not dec(1, -1)
    mer = ops.rpn_merge_supported
    assert mer(1, 1, 1, 1) and mer(0, 1, 0, 1) and mer(65535, 64, M, 1000)
    assert not mer(65536, 1, 1, 1) and not mer(1, 65, 1, 1) and not mer(1, 0, 1, 1) and not mer(1, 1, M + 1, 1)
    assert not mer(1, 1, 1, 0) and not mer(-1, 1, 1, 1) and not mer(1, 1, -1, 1)
    # the entry points agree with them before anything is enqueued (null pointers: never dereferenced on these paths)
    UNSUPPORTED, INVALID = consts['DM_ERR_UNSUPPORTED'], consts['DM_ERR_INVALID_ARG']
    L = lib()
    assert L.dm_rpn_select(None, 65536, 10, 10, 10, 0, None, 0, None, None, None) == UNSUPPORTED
    assert L.dm_rpn_select(None, 1, M + 1, 10, 10, 0, None, 0, None, None, None) == UNSUPPORTED
    assert L.dm_rpn_select(None, -1, 10, 10, 10, 0, None, 0, None, None, None) == INVALID
    assert L.dm_rpn_select(None, 0, 0, 0, 0, 1000, None, 0, None, None, None) == 0          # nothing to do
    assert L.dm_rpn_select(None, 3, 0, 0, 0, 1000, None, 0, None, None, None) == 0          # empty segments
    assert L.dm_rpn_select(None, 1, 10, 10, 10, 0, None, 0, None, None, None) == INVALID      # null table
    assert L.dm_rpn_select_workspace_bytes(65536, 1, 1, 1) == -1 and L.dm_rpn_select_workspace_bytes(1, 10, 10, 11) == -1
    n = L.dm_rpn_select_workspace_bytes(5, 201600, 268569, 2561)
    assert n >= 2561 * 8 + 268569 * 4 + 5 * 3 * 1024 * 4 and n % 4 == 0
    import ctypes
    four = (ctypes.c_float * 4)(0, 0, 0, 0)
    assert L.dm_rpn_decode(None, 65536, 1, None, None, None, 1, four, four, 0.016, None, None) == UNSUPPORTED
    assert L.dm_rpn_decode(None, 1, 1, None, None, None, 0, four, four, 0.016, None, None) == UNSUPPORTED
    assert L.dm_rpn_decode(None, 1, 1, None, None, None, 1, four, four, 0.0, None, None) == INVALID
    assert L.dm_rpn_decode(None, 0, 0, None, None, None, 1, four, four, 0.016, None, None) == 0
    assert L.dm_rpn_decode(None, 4, 0, None, None, None, 1, four, four, 0.016, None, None) == 0
    assert L.dm_rpn_merge(None, 1, 65, 1, None, None, None, None, 10, None, None, None) == UNSUPPORTED
    assert L.dm_rpn_merge(None, 1, 1, 1, None, None, None, None, 0, None, None, None) == UNSUPPORTED
    assert L.dm_rpn_merge(None, 0, 1, 0, None, None, None, None, 10, None, None, None) == 0
    assert L.dm_rpn_merge(None, 2, 1, 0, None, None, None, None, 10, None, None, None) == INVALID


def test_segment_table_is_checked_on_the_host():
    from dynamask_amd import ops
    with pytest.raises(TypeError, match='on the device'):
        ops.RPNSegments([torch.zeros(3, 4, 5)], 10)
    with pytest.raises(TypeError, match='on the device'):
        ops.RPNSegments([torch.zeros(1, 3, 4, 5)], 10)
    empty = ops.RPNSegments([], 10)
    assert len(empty) == 0 and empty.total_rows == 0 and empty.tab is None and empty.max_candidates == 0
