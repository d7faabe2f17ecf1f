"""FPN neck inference on the MI355X: ``ops.conv2d_up_add`` bit for bit against ``ops.conv2d`` followed by a gather and an
add at every 1x1 build the launcher can choose, ``ops.subsample2`` against slicing, ``FPN.forward`` against the reference's
own float32 and float64 runs (tests/golden/g27_fpn*.npz), the fused path against the composed one, a map wider than the
row-staging 3x3 kernel takes, the host waits of a call, and the chain FPN -> RPNHead -> StandardRoIHead."""
import json
import os

import numpy as np
import pytest
import torch

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

FORMS = ['mask_rcnn', 'retinanet', 'fcos']


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ conv2d_up_add
# (NB, (H, W), (Hs, Ws)): the smallest map; a 128-pixel tile that spans both images; several tiles with a ragged last one;
# Q = 768, full tiles only (the unpredicated store path); and 113 x 183 = 20679 pixels, the smallest 2 n - 1 map whose
# 2 x 162 tiles of 128 couts x 128 pixels exceed 1.25 x 256 compute units -- where a 256-cout launch leaves the
# 128 x 32 build for the 128 x 128 one (full tiles and a ragged last one)
SHAPES = [(1, (2, 2), (1, 1)), (2, (5, 7), (3, 4)), (1, (18, 27), (9, 14)), (3, (16, 16), (8, 8)), (1, (113, 183), (57, 92))]
BUILDS = {(4, 1, 1, 1, 32), (2, 2, 2, 2, 16), (2, 2, 1, 2, 16), (1, 4, 1, 1, 32)}       # (WGM, WGN, WM, WN, CK) of the 1x1 launcher


def _up_add_cases():
    cases = []
    for s, (nb, hw, hsws) in enumerate(SHAPES):
        big = hw[0] * hw[1] > 4096
        for cout in ((256,) if big else (256, 40, 24)):
            cases.append(dict(nb=nb, hw=hw, hsws=hsws, cout=cout, cins=[16], relu=False))
        if s == 0:
            cases.append(dict(nb=nb, hw=hw, hsws=hsws, cout=256, cins=[2048], relu=False))
    cases.append(dict(nb=2, hw=(5, 7), hsws=(3, 4), cout=40, cins=[16], relu=True))
    cases.append(dict(nb=1, hw=(18, 27), hsws=(9, 14), cout=256, cins=[8, 8], relu=False))
    cases.append(dict(nb=1, hw=(18, 27), hsws=(9, 14), cout=24, cins=[16], relu=True, tables='random'))
    return cases


def _case_id(c):
    return f"{c['nb']}x{c['hw'][0]}x{c['hw'][1]}-cout{c['cout']}-cin{'+'.join(map(str, c['cins']))}" + \
        ('-relu' if c['relu'] else '') + ('-' + c['tables'] if 'tables' in c else '')


def test_up_add_cases_cover_every_1x1_build():
    from dynamask_amd import ops
    seen = set()
    for c in _up_add_cases():
        recs = ops.conv2d_plan(c['cins'], c['nb'], c['hw'][0], c['hw'][1], c['cout'], 1, relu=c['relu'], has_addend=True)
        assert len(recs) == 1 and recs[0]['KS'] == 1 and recs[0]['POST'] == 1 and recs[0]['ksplit'] == 1
        seen.add(tuple(recs[0][k] for k in ('WGM', 'WGN', 'WM', 'WN', 'CK')))
        # the addend call takes the tiles the plain call of the shape takes
        plain = ops.conv2d_plan(c['cins'], c['nb'], c['hw'][0], c['hw'][1], c['cout'], 1, relu=c['relu'])
        assert [{k: v for k, v in r.items() if k != 'POST'} for r in recs] == [{k: v for k, v in r.items() if k != 'POST'} for r in plain]
    assert seen == BUILDS, f'builds without a case: {BUILDS - seen}'
    # a case of only full tiles and a case with a ragged last tile exist for the unpredicated and the predicated stores
    q = [c['nb'] * c['hw'][0] * c['hw'][1] for c in _up_add_cases()]
    assert any(n % 128 == 0 for n in q) and any(n % 128 for n in q)


@pytest.mark.parametrize('c', _up_add_cases(), ids=_case_id)
def test_up_add_is_conv2d_then_a_gathered_add(c):
    from dynamask_amd import necks, ops
    nb, (H, W), (Hs, Ws), cout, cins = c['nb'], c['hw'], c['hsws'], c['cout'], c['cins']
    cin = sum(cins)
    seed = H * 1000 + W + cout + cin
    srcs = [torch.randn(nb, ci, H, W, generator=_g(seed + i)).cuda() for i, ci in enumerate(cins)]
    w = (torch.randn(cout, cin, 1, 1, generator=_g(seed + 7)) * (2.0 / cin) ** 0.5).cuda()
    b = (torch.randn(cout, generator=_g(seed + 8)) * 0.1).cuda()
    addend = torch.randn(nb, cout, Hs, Ws, generator=_g(seed + 9)).cuda()
    if c.get('tables') == 'random':       # any table with values inside the addend, not only a monotone one
        iy = torch.randint(0, Hs, (H,), generator=_g(seed + 10), dtype=torch.int32).cuda()
        ix = torch.randint(0, Ws, (W,), generator=_g(seed + 11), dtype=torch.int32).cuda()
    else:
        iy, ix = necks.nearest_index(Hs, H, device='cuda'), necks.nearest_index(Ws, W, device='cuda')
    wq = ops.pack_conv_weight(w, src_channels=cins)
    before = addend.clone()
    got = ops.conv2d_up_add(srcs, wq, b, cout, addend, iy, ix, relu=c['relu'])
    conv = ops.conv2d(srcs, wq, b, cout, 1, relu=c['relu'])
    want = conv + addend[:, :, iy.long()][:, :, :, ix.long()]
    assert tuple(got.shape) == (nb, cout, H, W)
    assert torch.equal(_bits(got), _bits(want)), f'{int((got != want).sum())} of {got.numel()} outputs differ'
    assert torch.equal(addend, before)
    if c['relu']:
        assert bool((conv == 0).any()) and bool((got < 0).any())      # the addend joins after the activation
    # into a given tensor; two identical calls; without a bias
    out = torch.full_like(got, float('nan'))
    assert ops.conv2d_up_add(srcs, wq, b, cout, addend, iy, ix, relu=c['relu'], out=out) is out and torch.equal(_bits(out), _bits(got))
    nobias = ops.conv2d_up_add(srcs, wq, None, cout, addend, iy, ix, relu=c['relu'])
    want = ops.conv2d(srcs, wq, None, cout, 1, relu=c['relu']) + addend[:, :, iy.long()][:, :, :, ix.long()]
    assert torch.equal(_bits(nobias), _bits(want))


def test_up_add_argument_checks():
    from dynamask_amd import _lib, necks, ops
    x = torch.randn(1, 16, 4, 6, generator=_g(1)).cuda()
    w = torch.randn(24, 16, 1, 1, generator=_g(2)).cuda()
    wq = ops.pack_conv_weight(w)
    addend = torch.randn(1, 24, 2, 3, generator=_g(3)).cuda()
    iy, ix = necks.nearest_index(2, 4, device='cuda'), necks.nearest_index(3, 6, device='cuda')
    with pytest.raises(ValueError, match='addend'):
        ops.conv2d_up_add(x, wq, None, 24, addend[:, :16].contiguous(), iy, ix)
    with pytest.raises(ValueError, match='iy'):
        ops.conv2d_up_add(x, wq, None, 24, addend, ix, iy)
    with pytest.raises(TypeError, match='iy'):
        ops.conv2d_up_add(x, wq, None, 24, addend, iy.long(), ix)
    with pytest.raises(ValueError, match='bf16x3'):
        ops.conv2d_up_add(x, ops.pack_conv_weight(w, precision='bf16x3'), None, 24, addend, iy, ix)
    # the entry point itself: ksize 3 is unsupported, a flag other than ReLU and a null table are invalid
    import ctypes
    L = _lib.lib()
    out = torch.empty(1, 24, 4, 6).cuda()
    ptrs, chans, strides = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int * 1)(16), (ctypes.c_longlong * 1)(x.stride(0))

    def call(ksize=1, relu=0, iy_ptr=iy.data_ptr(), hs=2):
        return L.dm_conv2d_up_add_fwd(ptrs, chans, strides, 1, 1, 4, 6, ctypes.c_void_p(wq.data_ptr()), None, 24, ksize, relu,
                                      ctypes.c_void_p(addend.data_ptr()), hs, 3, ctypes.c_void_p(iy_ptr),
                                      ctypes.c_void_p(ix.data_ptr()), ctypes.c_void_p(out.data_ptr()), 24, 0, None)
    assert call() == 0
    assert call(ksize=3) == -3 and call(relu=2) == -1 and call(iy_ptr=0) == -1 and call(hs=0) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ subsample2
@pytest.mark.parametrize('H,W', [(1, 1), (2, 3), (5, 7), (25, 42)])
def test_subsample2_is_every_second_row_and_column(H, W):
    import torch.nn.functional as F
    from dynamask_amd import ops
    x = torch.randn(2, 5, H, W, generator=_g(H * 100 + W)).cuda()
    got = ops.subsample2(x)
    assert tuple(got.shape) == (2, 5, (H + 1) // 2, (W + 1) // 2) and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(x[:, :, ::2, ::2]))
    assert torch.equal(got, F.max_pool2d(x, 1, stride=2))
    out = torch.full_like(got, float('nan'))
    assert ops.subsample2(x, out=out) is out and torch.equal(_bits(out), _bits(got))
    assert ops.subsample2(x[:0]).shape == (0, 5, (H + 1) // 2, (W + 1) // 2)


# ------------------------------------------------------------------------------------------------ the neck
@pytest.fixture(scope='module')
def fpn(golden_dir):
    """({form: FPN on the device with the fixture's seeded weights}, {form: its stages on the device}, the JSON, fpn_inputs)."""
    import fpn_inputs as fi
    from dynamask_amd import necks, registry  # noqa: F401
    with open(os.path.join(golden_dir, 'g27_fpn_configs.json')) as f:
        cfgs = json.load(f)
    necks_, xs = {}, {}
    for form in FORMS:
        m = registry.build_neck(dict(cfgs[form]['model']['neck']))
        m.load_state_dict(fi.head_state({k: v.shape for k, v in m.state_dict().items()}, fi.WEIGHT_SEED), strict=True)
        necks_[form] = m.cuda().eval()
        xs[form] = [x.cuda() for x in fi.inputs(m.in_channels, cfgs[form]['batch'])]
    return necks_, xs, cfgs, fi


@pytest.mark.parametrize('form', FORMS)
def test_forward_against_the_reference(fpn, golden_dir, form):
    from dynamask_amd import conv_precision, necks
    necks_, xs, cfgs, fi = fpn
    z = np.load(os.path.join(golden_dir, fi.FILES[form]))
    m = necks_[form]
    assert necks.FPN_FUSED[0]
    with torch.no_grad():
        outs = m(xs[form])
        with conv_precision('bf16x3'):
            outs3 = m(xs[form])
    assert isinstance(outs, tuple) and len(outs) == m.num_outs == 5
    for l, (got, other) in enumerate(zip(outs, outs3)):
        ref32 = z[f'{form}_out{l}']
        assert tuple(got.shape) == ref32.shape, f'{form} level {l}'
        assert_close_via_f64(got, ref32, fi.unpack_f64(ref32, z[f'{form}_out{l}_err16']), f'{form} level {l}')
        assert torch.equal(got, other), f'{form} level {l}: the bf16x3 mode changed the neck'


def _both_paths(m, xs, monkeypatch):
    from dynamask_amd import necks
    with torch.no_grad():
        monkeypatch.setattr(necks, 'FPN_FUSED', [True])
        fused = m(xs)
        monkeypatch.setattr(necks, 'FPN_FUSED', [False])
        composed = m(xs)
        monkeypatch.setattr(necks, 'FPN_FUSED', [True])
    assert len(fused) == len(composed) == m.num_outs
    for l, (a, b) in enumerate(zip(fused, composed)):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f'level {l}: {int((a != b).sum())} values differ'
    return fused


@pytest.mark.parametrize('form', FORMS)
def test_fused_and_composed_paths_give_the_same_bits(fpn, form, monkeypatch):
    necks_, xs, cfgs, _ = fpn
    m = necks_[form]
    fused = _both_paths(m, xs[form], monkeypatch)
    if cfgs[form]['batch'] > 1:            # an image's bits do not depend on the batch
        with torch.no_grad():
            alone = m([x[1:] for x in xs[form]])
        assert all(torch.equal(a[0], f[1]) for a, f in zip(alone, fused))


def test_fused_and_composed_paths_with_a_scale_factor(monkeypatch):
    import fpn_inputs as fi
    from dynamask_amd import necks
    m = necks.FPN([16, 32, 64], 16, 4, upsample_cfg=dict(mode='nearest', scale_factor=2))
    state = fi.head_state({k: v.shape for k, v in m.state_dict().items()}, 5)
    m.load_state_dict(state, strict=True)
    m = m.cuda().eval()
    xs = fi.inputs([16, 32, 64], 2, seed=55, sizes=((16, 24), (8, 12), (4, 6)))
    fused = _both_paths(m, [x.cuda() for x in xs], monkeypatch)
    assert [tuple(o.shape[2:]) for o in fused] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    neck = dict(in_channels=[16, 32, 64], out_channels=16, num_outs=4, upsample_cfg=dict(mode='nearest', scale_factor=2))
    with torch.no_grad():
        ref32 = fi.restate(neck, state, xs)
        ref64 = fi.restate(neck, state, [x.double() for x in xs])
    for l in range(4):
        assert_close_via_f64(fused[l], ref32[l], ref64[l], f'scale_factor level {l}')
    # a produced size that is not the lower lateral's: the reference's += fails there too
    odd = fi.inputs([16, 32, 64], 1, seed=56, sizes=((15, 24), (8, 12), (4, 6)))
    for flag in (True, False):
        monkeypatch.setattr(necks, 'FPN_FUSED', [flag])
        with torch.no_grad(), pytest.raises(ValueError, match='scale_factor'):
            m([x.cuda() for x in odd])


def test_forward_on_a_wide_map(monkeypatch):
    """The level convolution leaves ops.conv2d (whole rows in LDS) for the any-width 3x3 kernel above
    CONV2D_3X3_MAX_WIDTH: a 4 x 130 level (and its 2 x 65 neighbour on ops.conv2d) against float64."""
    import fpn_inputs as fi
    from dynamask_amd import dense_heads, necks, ops
    assert dense_heads.CONV2D_3X3_MAX_WIDTH == 128 and necks.CONV2D_3X3_MAX_WIDTH == 128
    neck = dict(in_channels=[8, 16], out_channels=8, num_outs=3)
    m = necks.FPN(**neck)
    state = fi.head_state({k: v.shape for k, v in m.state_dict().items()}, 130)
    m.load_state_dict(state, strict=True)
    m = m.cuda().eval()
    xs = fi.inputs([8, 16], 2, seed=130, sizes=((4, 130), (2, 65)))
    routes = []
    real = ops.conv3x3_dil
    monkeypatch.setattr(ops, 'conv3x3_dil', lambda x, *a, **k: (routes.append(tuple(x.shape)), real(x, *a, **k))[1])
    outs = _both_paths(m, [x.cuda() for x in xs], monkeypatch)
    assert routes == [(2, 8, 4, 130)] * 2               # the wide level only, in either path
    assert [tuple(o.shape) for o in outs] == [(2, 8, 4, 130), (2, 8, 2, 65), (2, 8, 1, 33)]
    with torch.no_grad():
        ref32 = fi.restate(neck, state, xs)
        ref64 = fi.restate(neck, state, [x.double() for x in xs])
    for l in range(3):
        assert_close_via_f64(outs[l], ref32[l], ref64[l], f'wide map, level {l}')


def test_forward_makes_no_host_wait(fpn):
    import bench
    necks_, xs, _, _ = fpn
    for form in FORMS:
        m = necks_[form]
        with torch.no_grad():
            m(xs[form])                     # (the index tables reach the device once, at the first call of a size)
            assert bench.count_host_syncs(lambda: m(xs[form])) == 0, form


def test_chain_into_the_rpn_and_the_roi_head(fpn):
    """FPN's output is what RPNHead.simple_test_rpn takes, and its proposals what StandardRoIHead.simple_test takes: a
    64 x 96 image from the backbone's stages to detections with no stock module between."""
    import c4_inputs as ci
    import fpn_inputs as fi
    import rpn_inputs as ri
    from dynamask_amd import bbox_heads, dense_heads, losses, mask_heads, registry, roi_extractors, roi_head  # noqa: F401
    necks_, _, cfgs, _ = fpn
    cfg = registry._to_cfgdict(cfgs['mask_rcnn'])
    neck = necks_['mask_rcnn']
    rh = dict(cfg.model.rpn_head)
    rh.update(train_cfg=None, test_cfg=dict(cfg.test_cfg.rpn, nms_post=24))
    rpn = registry.build_head(rh)
    rpn.load_state_dict(ri.head_state({k: v.shape for k, v in rpn.state_dict().items()}, 27), strict=True)
    rpn = rpn.cuda().eval()
    rc = dict(cfg.model.roi_head)
    rc.update(train_cfg=None, test_cfg=cfg.test_cfg.rcnn)
    roi = registry.build_head(rc)
    assert type(roi) is roi_head.StandardRoIHead and roi.with_mask
    roi.load_state_dict(ci.head_state({k: v.shape for k, v in roi.state_dict().items()}, 27), strict=False)
    roi = roi.cuda().eval()
    H, W = 64, 96
    stages = [x.cuda() for x in fi.inputs(neck.in_channels, 1, seed=6496, sizes=tuple((H // s, W // s) for s in (4, 8, 16, 32)))]
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False, flip_direction=None)]
    with torch.no_grad():
        feats = neck(stages)
        assert [tuple(f.shape) for f in feats] == [(1, 256, 16, 24), (1, 256, 8, 12), (1, 256, 4, 6), (1, 256, 2, 3), (1, 256, 1, 2)]
        assert all(bool(torch.isfinite(f).all()) for f in feats)
        proposals = rpn.simple_test_rpn(feats, metas)
        assert len(proposals) == 1 and proposals[0].dim() == 2 and proposals[0].shape[1] == 5 and 0 < len(proposals[0]) <= 24
        assert bool(torch.isfinite(proposals[0]).all())
        bbox_results, segm_results = roi.simple_test(feats, proposals, metas)
    assert len(bbox_results) == 80 and len(segm_results) == 80
    for b, s in zip(bbox_results, segm_results):
        assert b.ndim == 2 and b.shape[1] == 5 and np.isfinite(b).all() and len(s) == len(b)
        assert all(tuple(np.asarray(mask).shape) == (H, W) for mask in s)
