"""ResNet backbone inference on the device: the stem kernels (dm_conv7x7_s2_fwd against torch's CPU convolution in float32
and float64, dm_maxpool3x3_s2_fwd against torch's CPU max-pool bit for bit), ``backbones.ResNet`` against the reference's
own module (tests/golden/g28_backbone*.npz) and, stage by stage, against backbone_inputs.restate; the wide-map route, host
waits, batch independence and the chain into the neck, the RPN and the RoI head."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

FORMS = ['pytorch', 'caffe_c4']


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ conv7x7_s2
# The kernel's output tile is 8 rows x 16 columns (csrc/stem.hip: S7_TH, S7_TW), 64 couts per workgroup.
#   (1, 38, 74): 19 x 37 outputs = 3 tile rows (the last of 3 rows) x 3 tile columns (the last of 5 columns);
#   (1, 5, 33):  3 x 17 outputs: the width is one tile column and 1.
# (NB, H, W, Cout)
CONV_CASES = [(1, 1, 1, 64), (1, 7, 9, 64), (1, 7, 9, 24), (2, 37, 53, 64), (2, 37, 53, 24), (1, 38, 74, 64), (1, 5, 33, 64)]


def _conv_problem(NB, H, W, cout, seed):
    x = torch.randn(NB, 3, H, W, generator=_g(seed))
    w = torch.randn(cout, 3, 7, 7, generator=_g(seed + 1)) * (2.0 / 147) ** 0.5
    b = torch.randn(cout, generator=_g(seed + 2)) * 0.5
    return x, w, b


@pytest.mark.parametrize('NB,H,W,cout', CONV_CASES, ids=lambda v: str(v))
def test_conv7x7_s2_against_torch(NB, H, W, cout):
    from dynamask_amd import ops
    x, w, b = _conv_problem(NB, H, W, cout, 7000 + H * 100 + W + cout)
    assert ops.conv7x7_s2_supported(x, cout)
    xd, bd = x.cuda(), b.cuda()
    wq = ops.pack_conv7x7_weight(w.cuda())
    for relu in (False, True):
        for bias in (True, False):
            ref32 = F.conv2d(x, w, b if bias else None, stride=2, padding=3)
            ref64 = F.conv2d(x.double(), w.double(), b.double() if bias else None, stride=2, padding=3)
            if relu:
                ref32, ref64 = F.relu(ref32), F.relu(ref64)
            got = ops.conv7x7_s2(xd, wq, bd if bias else None, cout, relu=relu)
            name = f'conv7x7_s2 {(NB, H, W, cout)} relu={relu} bias={bias}'
            assert tuple(got.shape) == (NB, cout, (H + 1) // 2, (W + 1) // 2) == tuple(ref32.shape), name
            err, ref_err, scale = assert_close_via_f64(got, ref32, ref64, name)
            print(f'{name}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
            out = torch.full_like(got, float('nan'))
            assert ops.conv7x7_s2(xd, wq, bd if bias else None, cout, relu=relu, out=out) is out
            assert torch.equal(_bits(out), _bits(got)), name + ': a second call, into a given out, gives other bits'
    assert torch.equal(xd.cpu(), x)


def test_conv7x7_s2_image_bits_do_not_depend_on_the_batch():
    from dynamask_amd import ops
    x, w, b = _conv_problem(3, 37, 53, 64, 7100)
    xd, bd, wq = x.cuda(), b.cuda(), ops.pack_conv7x7_weight(w.cuda())
    batch = ops.conv7x7_s2(xd, wq, bd, 64, relu=True)
    for i in range(3):
        alone = ops.conv7x7_s2(xd[i:i + 1].contiguous(), wq, bd, 64, relu=True)
        assert torch.equal(_bits(alone[0]), _bits(batch[i])), f'image {i}'


def test_conv7x7_s2_output_bits_do_not_depend_on_the_position():
    """A 60 x 90 map that is zero outside the window rows 22 .. 42, columns 38 .. 68 (an even origin: the stride-2 grid of the
    crop is the map's) against the 21 x 31 crop run alone: the crop's outputs whose 7 x 7 windows lie inside the crop --
    rows 2 .. 8, columns 2 .. 13: no padding tap -- are the map's outputs 11 rows and 19 columns further, in other tiles and
    other lanes, in bits."""
    from dynamask_amd import ops
    r0, c0, h, w_ = 22, 38, 21, 31
    crop, w, b = _conv_problem(1, h, w_, 64, 7200)
    full = torch.zeros(1, 3, 60, 90)
    full[:, :, r0:r0 + h, c0:c0 + w_] = crop
    wq, bd = ops.pack_conv7x7_weight(w.cuda()), b.cuda()
    a = ops.conv7x7_s2(crop.cuda(), wq, bd, 64)
    f = ops.conv7x7_s2(full.cuda(), wq, bd, 64)
    ys = [y for y in range(a.shape[2]) if 2 * y - 3 >= 0 and 2 * y + 3 <= h - 1]
    xs = [x for x in range(a.shape[3]) if 2 * x - 3 >= 0 and 2 * x + 3 <= w_ - 1]
    assert ys == list(range(2, 9)) and xs == list(range(2, 14))
    inner = a[:, :, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
    moved = f[:, :, ys[0] + r0 // 2:ys[-1] + 1 + r0 // 2, xs[0] + c0 // 2:xs[-1] + 1 + c0 // 2]
    assert float(inner.abs().max()) > 0.1
    assert torch.equal(_bits(inner), _bits(moved))


def test_stem_argument_checks():
    from dynamask_amd import _lib, ops
    L = _lib.lib()
    x, w, b = _conv_problem(1, 9, 11, 24, 7300)
    xd, wd = x.cuda(), w.cuda()
    wq = ops.pack_conv7x7_weight(wd)
    out = torch.empty(1, 24, 5, 6).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(xp=p(xd), wp=p(wq), op=p(out), C=3, flags=0, NB=1):
        return L.dm_conv7x7_s2_fwd(xp, NB, C, 9, 11, wp, None, 24, flags, op, None)
    assert call() == 0
    assert call(flags=1) == 0 and call(flags=8) == 0
    assert call(flags=16) == -3 and call(flags=17) == -3                  # bf16x3: unsupported
    assert call(flags=2) == -1 and call(flags=4) == -1 and call(flags=32) == -1 and call(flags=1 << 20) == -1
    assert call(xp=None) == -1 and call(wp=None) == -1 and call(op=None) == -1
    for C in (1, 5, 8):
        assert L.dm_conv7x7_s2_supported(1, C, 9, 11, 24) == 0 and call(C=C) == -3
    assert L.dm_conv7x7_s2_supported(0, 3, 9, 11, 24) == 0 and call(NB=0) == -3
    # the wrapper: weights packed for bf16x3 are refused by the library, others by their size
    marked = wq.clone()
    marked._dm_bf16x3 = True               # what pack_conv_weight(precision='bf16x3') marks its result with
    assert ops.conv_layout(marked) == 'bf16x3'
    with pytest.raises(RuntimeError, match='dm_conv7x7_s2_fwd'):
        ops.conv7x7_s2(xd, marked, None, 24)
    with pytest.raises(AssertionError):
        ops.conv7x7_s2(xd, ops.pack_conv_weight(torch.zeros(24, 8, 1, 1).cuda()), None, 24)
    with pytest.raises(ValueError, match='7, 7'):
        ops.pack_conv7x7_weight(torch.zeros(24, 3, 3, 3).cuda())
    # the pool
    pin, pout = torch.zeros(2, 4, 5).cuda(), torch.empty(2, 2, 3).cuda()
    assert L.dm_maxpool3x3_s2_fwd(p(pin), 2, 4, 5, p(pout), None) == 0
    assert L.dm_maxpool3x3_s2_fwd(None, 2, 4, 5, p(pout), None) == -1 and L.dm_maxpool3x3_s2_fwd(p(pin), 2, 4, 5, None, None) == -1
    assert L.dm_maxpool3x3_s2_fwd(p(pin), 2, 0, 5, p(pout), None) == -3 and L.dm_maxpool3x3_s2_fwd(p(pin), -1, 4, 5, p(pout), None) == -3
    assert L.dm_maxpool3x3_s2_fwd(None, 0, 4, 5, None, None) == 0          # nothing to do
    assert ops.maxpool3x3_s2(torch.zeros(0, 4, 5, 6).cuda()).shape == (0, 4, 3, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ maxpool3x3_s2
# the issue's shapes, and two whose rows are 16-byte aligned (W % 4 == 0: the float4 loads; at W = 20 the last group of
# four outputs reads past column 16 + 8 and takes the scalar tail)
POOL_SHAPES = [(1, 1), (2, 3), (3, 2), (10, 14), (33, 67), (12, 16), (7, 20)]


def _plant(x, seed):
    """-inf, +inf and NaN over ~4 % of the values each."""
    r = torch.rand(x.shape, generator=_g(seed))
    x = x.clone()
    x[r < 0.04] = float('-inf')
    x[(r >= 0.04) & (r < 0.08)] = float('inf')
    x[(r >= 0.08) & (r < 0.12)] = float('nan')
    return x


@pytest.mark.parametrize('NC', [1, 5, 128])
@pytest.mark.parametrize('H,W', POOL_SHAPES)
def test_maxpool3x3_s2_is_torchs(H, W, NC):
    from nonfinite_cases import assert_same_nonfinite
    from dynamask_amd import ops
    neg = -(torch.rand(1, NC, H, W, generator=_g(H * 1000 + W * 10 + NC)) + 0.1)        # negative only: zero padding would win
    got = ops.maxpool3x3_s2(neg.cuda())
    ref = F.max_pool2d(neg, 3, stride=2, padding=1)
    assert tuple(got.shape) == (1, NC, (H + 1) // 2, (W + 1) // 2) == tuple(ref.shape) and got.is_contiguous()
    assert torch.equal(_bits(got).cpu(), _bits(ref))
    assert bool((got < 0).all())
    out = torch.full_like(got, float('nan'))
    assert ops.maxpool3x3_s2(neg.cuda(), out=out) is out and torch.equal(_bits(out), _bits(got))
    mixed = _plant(torch.randn(1, NC, H, W, generator=_g(H * 1000 + W * 10 + NC + 1)), H * 1000 + W * 10 + NC + 2)
    got = ops.maxpool3x3_s2(mixed.cuda()).cpu()
    ref = F.max_pool2d(mixed, 3, stride=2, padding=1)
    if bool((torch.isfinite(ref) & (ref != 0)).any()):          # (the float64 triangle wants a non-zero reference)
        assert_same_nonfinite(got, ref, F.max_pool2d(mixed.double(), 3, stride=2, padding=1), f'maxpool {(NC, H, W)}')
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(_bits(torch.nan_to_num(got, nan=0.0)), _bits(torch.nan_to_num(ref, nan=0.0)))


def test_maxpool3x3_s2_nan_in_every_tap_position_and_a_window_of_minus_inf():
    """Output (oy, ox) reads rows 2 oy - 1 .. 2 oy + 1 and columns 2 ox - 1 .. 2 ox + 1 of a 10 x 14 map."""
    from dynamask_amd import ops
    x = torch.randn(1, 3, 10, 14, generator=_g(99))
    nan, ninf = float('nan'), float('-inf')
    x[0, 0, 3, 3] = nan           # first tap of output (2, 2), last tap of (1, 1)
    x[0, 1, 4, 10] = nan          # middle tap of output (2, 5) alone
    x[0, 2, 7, 7] = nan           # last tap of output (3, 3), first tap of (4, 4)
    x[0, 0, 7:10, 1:4] = ninf     # the whole window of output (4, 1)
    x[0, 1, 0:2, 0:2] = ninf      # the corner window (0, 0): its four taps inside the map
    got = ops.maxpool3x3_s2(x.cuda()).cpu()
    ref = F.max_pool2d(x, 3, stride=2, padding=1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref, nan=0.0))
    assert torch.isnan(got[0, 0, 2, 2]) and torch.isnan(got[0, 0, 1, 1]) and int(torch.isnan(got[0, 0]).sum()) == 4
    assert torch.isnan(got[0, 1, 2, 5]) and int(torch.isnan(got[0, 1]).sum()) == 1
    assert torch.isnan(got[0, 2, 3, 3]) and torch.isnan(got[0, 2, 4, 4]) and int(torch.isnan(got[0, 2]).sum()) == 4
    assert got[0, 0, 4, 1] == ninf and got[0, 1, 0, 0] == ninf


# ------------------------------------------------------------------------------------------------ the module
@pytest.fixture(scope='module')
def backbone(golden_dir):
    """({form: ResNet on the device with the fixture's seeded weights}, {form: the seeded state}, the JSON, backbone_inputs,
    the fixture's images on the device)."""
    import backbone_inputs as bi
    from dynamask_amd import backbones, registry  # noqa: F401
    with open(os.path.join(golden_dir, 'g28_backbone_configs.json')) as f:
        cfgs = json.load(f)
    nets, states = {}, {}
    for form in FORMS:
        m = registry.build_backbone(dict(cfgs[form]['model']['backbone']))
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == cfgs[form]['state_dict']
        states[form] = bi.head_state({k: v.shape for k, v in m.state_dict().items()}, bi.WEIGHT_SEED)
        m.load_state_dict(states[form], strict=True)
        nets[form] = m.cuda().eval()
    return nets, states, cfgs, bi, bi.inputs().cuda()


@pytest.fixture(scope='module')
def stage_refs(backbone):
    """{form: (stem, [stage outputs])} of backbone_inputs.restate in float32 on the CPU, computed once."""
    _, states, cfgs, bi, _ = backbone
    with torch.no_grad():
        return {form: bi.restate(cfgs[form]['model']['backbone'], states[form], bi.inputs(), every_stage=True) for form in FORMS}


@pytest.mark.parametrize('form', FORMS)
def test_forward_against_the_reference(backbone, golden_dir, form):
    from dynamask_amd import conv_precision
    nets, _, cfgs, bi, img = backbone
    z = np.load(os.path.join(golden_dir, bi.FILES[form]))
    m = nets[form]
    before = img.clone()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
        with conv_precision('bf16x3'):
            outs3 = m(img)
    assert torch.equal(_bits(img), _bits(before)), 'forward wrote into its input'
    assert isinstance(outs, tuple) and len(outs) == len(cfgs[form]['model']['backbone']['out_indices'])
    for l, (got, second, other) in enumerate(zip(outs, again, outs3)):
        ref32 = z[f'{form}_out{l}']
        assert tuple(got.shape) == ref32.shape, f'{form} output {l}'
        err, ref_err, scale = assert_close_via_f64(got, ref32, bi.unpack_f64(ref32, z[f'{form}_out{l}_err16']), f'{form} output {l}')
        print(f'{form} output {l}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
        assert torch.equal(_bits(got), _bits(second)), f'{form} output {l}: a second call gives other bits'
        assert torch.equal(_bits(got), _bits(other)), f'{form} output {l}: the bf16x3 mode changed the backbone'


@pytest.mark.parametrize('form', FORMS)
def test_every_stage_on_the_references_input(backbone, stage_refs, form):
    """The stem and every stage on the float32 reference's own input to it: an error shows at the stage that makes it."""
    nets, states, cfgs, bi, img = backbone
    m, cfg = nets[form], cfgs[form]['model']['backbone']
    stem32, stages32 = stage_refs[form]
    with torch.no_grad():
        stem64 = bi.restate_stem(states[form], bi.inputs().double())
        assert_close_via_f64(m.stem(img), stem32, stem64, f'{form} stem')
        x = stem32
        for i, ref32 in enumerate(stages32):
            ref64 = bi.restate_stage(cfg, states[form], i, x.double())
            xd = x.cuda()
            keep = xd.clone()
            got = m.run_stage(i, xd)
            assert torch.equal(_bits(xd), _bits(keep)), f'{form} stage {i} wrote into its input'
            err, ref_err, scale = assert_close_via_f64(got, ref32, ref64, f'{form} stage {i}')
            print(f'{form} stage {i}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
            x = ref32


def test_forward_on_a_wide_map(monkeypatch):
    """A 3 x 40 x 520 image: the stem gives 10 x 130, wider than CONV2D_3X3_MAX_WIDTH, so layer1's three 3x3 convolutions
    run on ops.conv3x3_dil; layer2's (65 wide behind the stride-2 one) on ops.conv2d."""
    import backbone_inputs as bi
    from dynamask_amd import backbones, dense_heads, ops
    assert dense_heads.CONV2D_3X3_MAX_WIDTH == 128 and backbones.CONV2D_3X3_MAX_WIDTH == 128
    cfg = dict(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1), style='pytorch')
    m = backbones.ResNet(**cfg)
    state = bi.head_state({k: v.shape for k, v in m.state_dict().items()}, 520)
    m.load_state_dict(state, strict=True)
    m = m.cuda().eval()
    img = bi.inputs(1, 40, 520, seed=520)
    routes, strided = [], []
    real, real_s2 = ops.conv3x3_dil, ops.conv3x3_s2
    monkeypatch.setattr(ops, 'conv3x3_dil', lambda x, *a, **k: (routes.append(tuple(x.shape)), real(x, *a, **k))[1])
    monkeypatch.setattr(ops, 'conv3x3_s2', lambda x, *a, **k: (strided.append((tuple(x.shape), k.get('splits'))), real_s2(x, *a, **k))[1])
    with torch.no_grad():
        outs = m(img.cuda())
        ref32 = bi.restate(cfg, state, img)
        ref64 = bi.restate(cfg, state, img.double())
    assert routes == [(1, 64, 10, 130)] * 3
    assert strided == [((1, 128, 10, 130), 1)]
    assert [tuple(o.shape) for o in outs] == [(1, 256, 10, 130), (1, 512, 5, 65)]
    for l in range(2):
        assert_close_via_f64(outs[l], ref32[l], ref64[l], f'wide map, output {l}')


def test_forward_makes_no_host_wait(backbone):
    import bench
    nets, _, _, _, img = backbone
    for form in FORMS:
        m = nets[form]
        with torch.no_grad():
            m(img)
            assert bench.count_host_syncs(lambda: m(img)) == 0, form


@pytest.mark.parametrize('form', FORMS)
def test_image_bits_do_not_depend_on_the_batch(backbone, form):
    nets, _, _, _, img = backbone
    with torch.no_grad():
        both = nets[form](img)
        alone = nets[form](img[:1].contiguous())
    assert len(both) == len(alone)
    for l, (a, b) in enumerate(zip(alone, both)):
        assert torch.equal(_bits(a[0]), _bits(b[0])), f'{form} output {l}'


def test_chain_from_the_image_to_detections(backbone):
    """ResNet -> FPN -> RPNHead.simple_test_rpn -> StandardRoIHead.simple_test from one config: a 64 x 96 image to detections
    with no stock module between; the neck reads the backbone's outputs themselves and nothing behind it writes them."""
    import c4_inputs as ci
    import fpn_inputs as fi
    import rpn_inputs as ri
    from dynamask_amd import bbox_heads, dense_heads, losses, mask_heads, necks, registry, roi_extractors, roi_head  # noqa: F401
    nets, _, cfgs, bi, _ = backbone
    cfg = registry._to_cfgdict(cfgs['pytorch'])
    net = nets['pytorch']
    neck = registry.build_neck(dict(cfg.model.neck))
    neck.load_state_dict(fi.head_state({k: v.shape for k, v in neck.state_dict().items()}, fi.WEIGHT_SEED), strict=True)
    neck = neck.cuda().eval()
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
    img = bi.inputs(1, H, W, seed=6496).cuda()
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False, flip_direction=None)]
    seen = []
    real = neck.forward
    neck.forward = lambda inputs: (seen.extend(inputs), real(inputs))[1]
    with torch.no_grad():
        stages = net(img)
        assert [tuple(s.shape) for s in stages] == [(1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
        kept = [s.clone() for s in stages]
        feats = neck(stages)
        assert [tuple(f.shape) for f in feats] == [(1, 256, 16, 24), (1, 256, 8, 12), (1, 256, 4, 6), (1, 256, 2, 3), (1, 256, 1, 2)]
        assert all(bool(torch.isfinite(f).all()) for f in feats)
        proposals = rpn.simple_test_rpn(feats, metas)
        assert len(proposals) == 1 and proposals[0].dim() == 2 and proposals[0].shape[1] == 5 and 0 < len(proposals[0]) <= 24
        assert bool(torch.isfinite(proposals[0]).all())
        bbox_results, segm_results = roi.simple_test(feats, proposals, metas)
        again = net(img)
    assert len(seen) == 4 and all(a is b for a, b in zip(seen, stages))
    for l, (s, k, a) in enumerate(zip(stages, kept, again)):
        assert torch.equal(_bits(s), _bits(k)), f'stage {l} was written behind the backbone'
        assert torch.equal(_bits(s), _bits(a)), f'stage {l}: a second call gives other bits'
    assert len(bbox_results) == 80 and len(segm_results) == 80
    for b, s in zip(bbox_results, segm_results):
        assert b.ndim == 2 and b.shape[1] == 5 and np.isfinite(b).all() and len(s) == len(b)
        assert all(tuple(np.asarray(mask).shape) == (H, W) for mask in s)
