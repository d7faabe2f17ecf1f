"""Mask R-CNN / Faster R-CNN C4 inference on the MI355X: the strided RoIAlign (dm_roi_align_strided_fwd) bit for bit against
the kept bins of the unordered dense call, the five convolution shapes of ResNet layer4 at 7 x 7 and the mask branch's
deconvolution / logits convolution against float64 through the triangle of tests/tolerances.py, the ResLayer shared head,
and StandardRoIHead with it through the registry against the reference (tests/golden/g25_c4.npz: the reference's own float32
and float64 runs).  Every kernel output of the new entry point is written between two canary guard bands that must
survive."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

CANARY = 7.0
GUARD = 4096


def _g(seed):
    return torch.Generator().manual_seed(seed)


class Guarded:
    """A device tensor of ``shape`` between two guard bands of CANARY."""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), CANARY, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == CANARY).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == CANARY).all()), f'{what}: the guard band past the output was overwritten'


def _rois(boxes, batch=0):
    return torch.cat([boxes.new_full((len(boxes), 1), float(batch)), boxes], 1).contiguous()


# ------------------------------------------------------------------------------------------------ strided RoIAlign
# name -> (map sizes, strides): one level and four, the finest map 13 x 9 or 50 x 84
PYRAMIDS = {
    'one_13x9': ([(13, 9)], [4]),
    'one_50x84': ([(50, 84)], [4]),
    'four_13x9': ([(13, 9), (7, 5), (4, 3), (2, 2)], [4, 8, 16, 32]),
    'four_50x84': ([(50, 84), (25, 42), (13, 21), (7, 11)], [4, 8, 16, 32]),
}


def _strided_rois(n, img_h, img_w, seed):
    """[n, 5] over two images: the hand-written boxes first (spanning the image and beyond -- a sampling grid above 4 x 4 at
    P = 14 on the finest level --, partly outside, under one pixel, zero area), then seeded ones."""
    from dynamask_amd import synth
    h, w = float(img_h), float(img_w)
    hand = torch.tensor([[0, -2.4 * w, -2.6 * h, 3.4 * w, 3.5 * h],
                         [1, -0.2 * w, -0.1 * h, 0.45 * w, 0.5 * h],
                         [0, 0.41 * w, 0.52 * h, 0.41 * w + 0.6, 0.52 * h + 0.7],
                         [1, 0.3 * w, 0.3 * h, 0.3 * w, 0.3 * h],
                         [1, 0.0, 0.0, w, h],
                         [0, 0.8 * w, 0.7 * h, 1.3 * w, 1.2 * h]], dtype=torch.float32)
    if n <= len(hand):
        return hand[:n].contiguous()
    seeded = synth.make_rois(2, n - len(hand), img_h, img_w, seed=seed, min_size=2.0, max_size=float(max(img_h, img_w)))
    return torch.cat([hand, seeded[:n - len(hand)]]).contiguous()


def _dense_kept(ops, feats, rois, P, scales, sr, step=2):
    """The reference: the dense extraction in chunks of at most 128 RoIs (the unordered 16-channel route), its kept bins."""
    outs, lvs = [], []
    for lo in range(0, len(rois), 128):
        o, lv = ops.roi_align(feats, rois[lo:lo + 128].contiguous(), P, scales, sr, 56.0, return_levels=True)
        outs.append(o[:, :, ::step, ::step])
        lvs.append(lv)
    return torch.cat(outs).contiguous(), torch.cat(lvs)


@pytest.mark.parametrize('N', [1, 7, 193, 1030])
@pytest.mark.parametrize('pyramid', list(PYRAMIDS))
def test_strided_roi_align_is_the_dense_calls_kept_bins(pyramid, N):
    from dynamask_amd import ops
    maps, strides = PYRAMIDS[pyramid]
    scales = [1.0 / s for s in strides]
    img_h, img_w = maps[0][0] * strides[0], maps[0][1] * strides[0]
    rois = _strided_rois(N, img_h, img_w, seed=N).cuda()
    tile = ops.ROI_KERNELS.index('tile')
    levels_seen = set()
    for C in (4, 20, 72):
        feats = [torch.randn(2, C, h, w, generator=_g(C + h)).cuda() for h, w in maps]
        for P in (14, 7, 2):
            # the chunks of the reference are the unordered 16-channel route
            ref_plan, = ops.roi_align_plan('forward', maps, 2, C, min(N, 128), P)
            assert (ref_plan['kernel'], ref_plan['P0'], ref_plan['CT']) == (tile, 0, 16)
            Po = -(-P // 2)
            for sr in (0, 2):
                want, want_lv = _dense_kept(ops, feats, rois, P, scales, sr)
                out = Guarded((N, C, Po, Po))
                got, lv = ops.roi_align(feats, rois, P, scales, sr, 56.0, return_levels=True, bin_step=2, out=out.t)
                out.check(f'strided C={C} P={P} sr={sr}')
                assert got.data_ptr() == out.t.data_ptr() and tuple(got.shape) == (N, C, Po, Po)
                assert torch.equal(got, want), f'C={C} P={P} sr={sr}: {int((got != want).sum())} of {got.numel()} values differ'
                assert torch.equal(lv, want_lv)
                levels_seen |= set(lv.cpu().tolist())
                again = ops.roi_align(feats, rois, P, scales, sr, 56.0, bin_step=2)
                assert torch.equal(again, got), 'two identical calls differ'
                k = N // 2
                alone = ops.roi_align(feats, rois[k:k + 1].contiguous(), P, scales, sr, 56.0, bin_step=2)
                assert torch.equal(alone, got[k:k + 1]), 'a RoI\'s bits depend on the other RoIs of the call'
            if C == 20 and P == 14:
                assert bool((got.abs().sum((1, 2, 3)) > 0).any())
    if len(maps) == 1:
        assert levels_seen == {0}
    elif N >= 193:
        assert len(levels_seen) >= 2 and levels_seen <= set(range(4))          # more than one level in one launch


def test_strided_roi_align_samples_grids_above_four():
    """The hand-written spanning box has a sampling grid above 4 x 4 at P = 14: no merged stencil (on this 50 x 84 map its
    footprint is the whole map, above the tile buffer: the direct global taps; on the 13 x 9 map of the test above the
    run-time sampling loop of the tile), and the zero-area box gives zeros."""
    from dynamask_amd import ops
    maps, strides = PYRAMIDS['one_50x84']
    rois = _strided_rois(6, 200, 336, seed=0).cuda()
    spans = rois[0]
    assert float(spans[3] - spans[1]) / 4 / 14 > 4 and float(spans[4] - spans[2]) / 4 / 14 > 4
    feats = [torch.randn(2, 8, 50, 84, generator=_g(3)).cuda()]
    got = ops.roi_align(feats, rois, 14, [0.25], 0, 56.0, bin_step=2)
    assert bool((got[3] == 0).all()) and bool((got[0] != 0).any())
    other = ops.roi_align(feats, rois, 14, [0.25], 0, 56.0, bin_step=3)           # any step inside the grid
    dense = ops.roi_align(feats, rois, 14, [0.25], 0, 56.0)
    assert tuple(other.shape) == (6, 8, 5, 5) and torch.equal(other, dense[:, :, ::3, ::3].contiguous())
    assert torch.equal(ops.roi_align(feats, rois, 14, [0.25], 0, 56.0, bin_step=1), dense)


def test_strided_roi_align_edges_and_refusals():
    from dynamask_amd import ops
    from dynamask_amd._abi import load
    from dynamask_amd._lib import lib
    consts = load()[1]
    feats = [torch.randn(2, 8, 13, 9, generator=_g(1)).cuda()]
    rois = _strided_rois(7, 52, 36, seed=2).cuda()
    empty = ops.roi_align(feats, rois[:0].contiguous(), 14, [0.25], 0, 56.0, bin_step=2)
    assert tuple(empty.shape) == (0, 8, 7, 7)
    e, lv = ops.roi_align(feats, rois[:0].contiguous(), 7, [0.25], 0, 56.0, bin_step=2, return_levels=True)
    assert tuple(e.shape) == (0, 8, 4, 4) and tuple(lv.shape) == (0,)
    with pytest.raises(ValueError):
        ops.roi_align(feats, rois, 14, [0.25], 0, 56.0, bin_step=0)
    with pytest.raises(TypeError):
        ops.roi_align(feats, rois, 14, [0.25], 0, 56.0, bin_step=2.0)
    with pytest.raises(NotImplementedError):
        ops.roi_align(feats, rois, 14, [0.25], 0, 56.0, bin_step=2, roi_scale_factor=1.3)
    six = [torch.randn(2, 6, 13, 9, generator=_g(1)).cuda()]
    with pytest.raises(RuntimeError, match='dm_roi_align_strided_fwd'):
        ops.roi_align(six, rois, 14, [0.25], 0, 56.0, bin_step=2)            # C % 4 != 0: the dense call's generic kernel
    with pytest.raises(RuntimeError, match='dm_roi_align_strided_fwd'):
        ops.roi_align(feats, rois, 28, [0.25], 0, 56.0, bin_step=2)          # P * P > 256: the dense call's band kernel
    # the library itself refuses before it launches anything
    out = Guarded((7, 8, 7, 7))

    def call(C, P, step, n=7):
        return lib().dm_roi_align_strided_fwd(ops._ptr_array(feats), ops._int_array([13]), ops._int_array([9]),
                                              ops._float_array([0.25]), 1, 2, C, ops._p(rois), n, P, 0, 56.0, step,
                                              ops._p(out.t), None, ops._stream())
    assert call(8, 14, 0) == consts['DM_ERR_INVALID_ARG'] and call(8, 14, -1) == consts['DM_ERR_INVALID_ARG']
    assert call(8, 14, 15) == consts['DM_ERR_UNSUPPORTED'] and call(8, 28, 2) == consts['DM_ERR_UNSUPPORTED']
    assert call(6, 14, 2) == consts['DM_ERR_UNSUPPORTED'] and call(8, 14, 2, n=-1) == consts['DM_ERR_INVALID_ARG']
    assert call(8, 14, 2, n=0) == 0
    out.check('refused calls')
    assert bool((out.t == CANARY).all())
    assert call(8, 14, 2) == 0
    out.check('the accepted call')
    assert torch.equal(out.t, ops.roi_align(feats, rois, 14, [0.25], 0, 56.0)[:, :, ::2, ::2])


def test_extractor_with_a_bin_step():
    import c4_inputs as ci
    from dynamask_amd import roi_extractors
    ext = roi_extractors.SingleRoIExtractor(roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0), out_channels=1024,
                                            featmap_strides=[16])
    feats = [f.cuda() for f in ci.c4_feats()]
    rois = _rois(ci.proposals()).cuda()
    dense = ext(feats, rois)
    assert tuple(dense.shape) == (len(rois), 1024, 14, 14)
    assert torch.equal(ext(feats, rois, bin_step=2), dense[:, :, ::2, ::2].contiguous())
    assert torch.equal(ext(feats, rois), dense)                      # the default is today's call


# ------------------------------------------------------------------------------------------------ the five conv shapes
def _conv_cases():
    import c4_inputs as ci
    return [(name, nb) for name in ci.CONV_SHAPES for nb in ci.CONV_TEST_NBS[name]]


@pytest.mark.parametrize('name,nb', _conv_cases())
def test_conv_shapes_of_layer4(name, nb):
    """The launches of the downsample block and of a plain Bottleneck on ops.conv2d (exact fp32), each at 3 RoIs and at the
    smallest RoI count of every further build its 1000-RoI call takes, against float64 F.conv2d."""
    import c4_inputs as ci
    from dynamask_amd import ops
    src, cout, k, acc = ci.CONV_SHAPES[name]
    g = _g(nb + cout + k + len(src))
    xs = [torch.randn(nb, c, 7, 7, generator=g) for c in src]
    cin = sum(src)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    wq = ops.pack_conv_weight(w.cuda(), src_channels=list(src))
    assert ops.conv_layout(wq) == 'fp32'
    x = torch.cat(xs, 1)
    dest = torch.randn(nb, cout, 7, 7, generator=g) * 1.5 if acc else None

    def ref(dtype):
        y = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=k // 2)
        return F.relu(y + dest.to(dtype)) if acc else F.relu(y)
    out = Guarded((nb, cout, 7, 7), dest)
    got = ops.conv2d([t.cuda() for t in xs], wq, b.cuda(), cout, k, relu=True, out=out.t, accumulate=acc)
    out.check(name)
    assert got.data_ptr() == out.t.data_ptr()
    r64 = ref(torch.float64)
    if acc:
        assert bool(((dest < 0) & (r64 > 0)).any()) and bool(((dest > 0) & (r64 == 0)).any())
    assert_close_via_f64(got, ref(torch.float32), r64, f'{name} at {nb} RoIs')
    if nb > 3:
        # one association of the K sum in every build (no split-K on this path): a RoI's bits do not depend on how many
        # RoIs the call has, which is what lets batch_simple_test give simple_test's bits at any proposal count
        few = ops.conv2d([t[:3].contiguous().cuda() for t in xs], wq, b.cuda(), cout, k, relu=True,
                         out=dest[:3].contiguous().cuda() if acc else None, accumulate=acc)
        assert torch.equal(few, got[:3]), 'the first RoIs of the large call differ from the 3-RoI call'


def test_mask_branch_deconv_and_logits_convolution():
    """FCNMaskHead(num_convs=0, in_channels=2048): deconv2x2 2048 -> 256 at 7 x 7 (+ ReLU), then the 1x1 256 -> 80 at 14 x 14."""
    from dynamask_amd.mask_heads import FCNMaskHead
    torch.manual_seed(3)
    h = FCNMaskHead(num_convs=0, in_channels=2048, conv_out_channels=256, num_classes=80)
    g = _g(8)
    with torch.no_grad():
        h.upsample.weight.copy_(torch.randn(2048, 256, 2, 2, generator=g) * (2.0 / 2048) ** 0.5)
        h.upsample.bias.copy_(torch.randn(256, generator=g) * 0.1)
        h.conv_logits.weight.copy_(torch.randn(80, 256, 1, 1, generator=g) * (2.0 / 256) ** 0.5)
        h.conv_logits.bias.copy_(torch.randn(80, generator=g) * 0.1)
    x = torch.relu(torch.randn(5, 2048, 7, 7, generator=g))
    sd = {k: v.detach().clone() for k, v in h.state_dict().items()}
    h = h.cuda().eval()

    def ref(dtype):
        up = F.relu(F.conv_transpose2d(x.to(dtype), sd['upsample.weight'].to(dtype), sd['upsample.bias'].to(dtype), stride=2))
        return up, F.conv2d(up, sd['conv_logits.weight'].to(dtype), sd['conv_logits.bias'].to(dtype))
    with torch.no_grad():
        up = h.upsample(x.cuda(), relu=True)
        logits = h(x.cuda())
    (u32, l32), (u64, l64) = ref(torch.float32), ref(torch.float64)
    assert tuple(up.shape) == (5, 256, 14, 14) and tuple(logits.shape) == (5, 80, 14, 14)
    assert_close_via_f64(up, u32, u64, 'deconv2x2 2048 -> 256 at 7 x 7')
    assert_close_via_f64(logits, l32, l64, '1x1 256 -> 80 at 14 x 14')


# ------------------------------------------------------------------------------------------------ ResLayer
def _small_layer(stride, seed=5):
    import c4_inputs as ci
    from dynamask_amd.shared_heads import ResLayer
    m = ResLayer(depth=50, stage=-2, stride=stride, style='caffe')
    state = ci.head_state({'shared_head.' + k: v.shape for k, v in m.state_dict().items()}, seed)
    m.load_state_dict({k[len('shared_head.'):]: v for k, v in state.items()}, strict=True)
    return m.eval()


def _conv_bn(x, w, bn, dtype, stride=1):
    y = F.conv2d(x.to(dtype), w.detach().to(dtype), padding=w.shape[-1] // 2, stride=stride)
    return F.batch_norm(y, bn.running_mean.to(dtype), bn.running_var.to(dtype), bn.weight.detach().to(dtype),
                        bn.bias.detach().to(dtype), False, 0.0, bn.eps)


def _layer_ref(m, x, dtype):
    """backbones/resnet.py's caffe Bottlenecks in eval mode: the layer's stride in block 0's conv1 and downsample.0."""
    x = x.to(dtype)
    for i, b in enumerate(m.res_layer):
        s = m.stride if i == 0 else 1
        h = F.relu(_conv_bn(x, b.conv1.weight, b.bn1, dtype, stride=s))
        h = F.relu(_conv_bn(h, b.conv2.weight, b.bn2, dtype))
        h = _conv_bn(h, b.conv3.weight, b.bn3, dtype)
        idn = x if b.downsample is None else _conv_bn(x, b.downsample[0].weight, b.downsample[1], dtype, stride=s)
        x = F.relu(h + idn)
    return x


@pytest.mark.parametrize('stride,hw', [(1, (7, 7)), (2, (14, 14)), (2, (7, 5))])
def test_res_layer_against_float64(stride, hw):
    """32 -> 64 channels, six blocks (stage -2: planes 16), against the float64 conv -> BatchNorm -> add -> ReLU chain of
    the CPU copy of the same weights; ``forward`` and ``forward_sampled`` agree bit for bit; nothing writes the input."""
    from dynamask_amd import conv_precision
    cpu = _small_layer(stride)
    x = torch.randn(5, 32, *hw, generator=_g(stride + hw[1]))
    m = _small_layer(stride).cuda()
    xd = Guarded(x.shape, x)
    with torch.no_grad():
        got = m(xd.t)
        sub = Guarded((5, 32, -(-hw[0] // stride), -(-hw[1] // stride)), x[:, :, ::stride, ::stride])
        sampled = m.forward_sampled(sub.t)
        again = m(xd.t)
        with conv_precision('bf16x3'):
            mode = m(xd.t)
    xd.check('ResLayer input')
    sub.check('ResLayer subsampled input')
    assert torch.equal(xd.t.cpu(), x) and torch.equal(sub.t.cpu(), x[:, :, ::stride, ::stride]), 'the input was written'
    assert tuple(got.shape) == (5, 64, -(-hw[0] // stride), -(-hw[1] // stride))
    assert torch.equal(sampled, got), 'forward(dense) and forward_sampled(dense[..., ::s, ::s]) differ'
    assert torch.equal(again, got), 'two identical calls differ'
    assert torch.equal(mode, got), 'the bf16x3 mode changed a bit'
    e = assert_close_via_f64(got, _layer_ref(cpu, x, torch.float32), _layer_ref(cpu, x, torch.float64), f'ResLayer stride {stride}')
    print('ResLayer stride %d: err %.3g, reference err %.3g, scale %.3g' % ((stride,) + e))
    for i in (0, 4):          # a RoI's bits do not depend on the RoI count
        with torch.no_grad():
            assert torch.equal(m(x[i:i + 1].cuda()), got[i:i + 1])


# ------------------------------------------------------------------------------------------------ against the fixture
@pytest.fixture(scope='module')
def c4(golden_dir):
    """({config name: StandardRoIHead on the device with the fixture's seeded weights}, the fixture, c4_inputs)."""
    import c4_inputs as ci
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    z = np.load(os.path.join(golden_dir, 'g25_c4.npz'))
    with open(os.path.join(golden_dir, 'g25_c4_configs.json')) as f:
        cfgs = json.load(f)
    heads, state = {}, None
    for name in ('mask_c4', 'faster_c4'):
        cfg = registry._to_cfgdict(cfgs[name])
        rh = dict(cfg.model.roi_head)
        rh.update(train_cfg=None, test_cfg=cfg.test_cfg.rcnn)
        m = registry.build_head(rh)
        if state is None:           # the Faster head takes the mask config's weights (the generator draws them once)
            state = ci.head_state({k: v.shape for k, v in m.state_dict().items()}, int(z['weight_seed']))
        res = m.load_state_dict({k: v for k, v in state.items() if m.with_mask or not k.startswith('mask_head.')}, strict=False)
        assert not res.unexpected_keys and not any(k.startswith(ci.HEAD_PREFIXES) for k in res.missing_keys)
        heads[name] = m.cuda().eval()
    return heads, z, ci


def _class_major(bbox_results):
    dets = np.asarray([row for b in bbox_results for row in b], np.float32).reshape(-1, 5)
    return dets, np.asarray([c for c, b in enumerate(bbox_results) for _ in range(len(b))], np.int64)


def _inputs(ci):
    return [f.cuda() for f in ci.c4_feats()], ci.proposals().cuda()


def test_bbox_forward_against_the_reference(c4):
    from dynamask_amd import conv_precision
    heads, z, ci = c4
    m = heads['mask_c4']
    feats, props = _inputs(ci)
    rois = _rois(props)
    keep = feats[0].clone()
    with torch.no_grad():
        res = m._bbox_forward(feats, rois)
        again = m._bbox_forward(feats, rois)
        with conv_precision('bf16x3'):
            mode = m._bbox_forward(feats, rois)
        faster = heads['faster_c4']._bbox_forward(feats, rois)
    assert torch.equal(feats[0], keep)
    n = len(rois)
    assert set(res) == {'cls_score', 'bbox_pred', 'bbox_feats'}
    assert tuple(res['bbox_feats'].shape) == (n, 2048, 7, 7)          # what the shared head returns
    assert tuple(res['cls_score'].shape) == (n, 81) and tuple(res['bbox_pred'].shape) == (n, 320)
    e = assert_close_via_f64(res['bbox_feats'].sum((2, 3)), z['shared_sums'], z['shared_sums64'], 'shared-head sums')
    print('shared sums: err %.3g, reference err %.3g, scale %.3g' % e)
    e = assert_close_via_f64(res['cls_score'], z['cls_score'], z['cls_score64'], 'cls_score')
    print('cls_score: err %.3g, reference err %.3g, scale %.3g' % e)
    e = assert_close_via_f64(res['bbox_pred'], z['bbox_pred'], z['bbox_pred64'], 'bbox_pred')
    print('bbox_pred: err %.3g, reference err %.3g, scale %.3g' % e)
    for k in res:
        assert torch.equal(again[k], res[k]), f'{k}: two identical calls differ'
        assert torch.equal(mode[k], res[k]), f'{k}: the bf16x3 mode changed a bit'
        assert torch.equal(faster[k], res[k]), f'{k}: the Faster config has the same weights'
    zero = ci.hand_index('zero_area')
    # the zero-area proposal: zero features into the shared head, whose biases alone make its (finite, non-zero) output
    assert bool((m.bbox_roi_extractor(feats, rois[zero:zero + 1].contiguous(), bin_step=2) == 0).all())
    assert bool(torch.isfinite(res['bbox_feats'][zero]).all()) and bool((res['bbox_feats'][zero] != 0).any())


def test_the_strided_route_equals_the_dense_route(c4):
    heads, z, ci = c4
    m = heads['mask_c4']
    feats, props = _inputs(ci)
    rois = _rois(props)
    assert m.shared_head_strided_extraction(m.bbox_roi_extractor, feats)
    calls = []
    ext_forward = type(m.bbox_roi_extractor).forward

    def spy(self, feats, rois, roi_scale_factor=None, bin_step=None):
        calls.append(bin_step)
        return ext_forward(self, feats, rois, roi_scale_factor=roi_scale_factor, bin_step=bin_step)
    type(m.bbox_roi_extractor).forward = spy
    try:
        with torch.no_grad():
            strided = m._bbox_forward(feats, rois)
            strided_mask = m._mask_forward(feats, rois)
            assert calls == [2, 2]
            m.STRIDED_EXTRACTION = False
            assert not m.shared_head_strided_extraction(m.bbox_roi_extractor, feats)
            dense = m._bbox_forward(feats, rois)
            dense_mask = m._mask_forward(feats, rois)
            assert calls == [2, 2, None, None]
    finally:
        type(m.bbox_roi_extractor).forward = ext_forward
        del m.STRIDED_EXTRACTION
    assert m.STRIDED_EXTRACTION is True
    for k in strided:
        assert torch.equal(strided[k], dense[k]), k
    assert tuple(strided_mask['mask_pred'].shape) == (len(rois), 80, 14, 14)
    assert tuple(strided_mask['mask_feats'].shape) == (len(rois), 2048, 7, 7)
    assert torch.equal(strided_mask['mask_pred'], dense_mask['mask_pred'])
    assert torch.equal(strided_mask['mask_feats'], strided['bbox_feats'])


@pytest.mark.parametrize('tag,rescale', [('plain', False), ('rescale', True)])
def test_simple_test_against_the_reference(c4, tag, rescale):
    from dynamask_amd.roi_head import bbox2roi
    heads, z, ci = c4
    m = heads['mask_c4']
    feats, props = _inputs(ci)
    metas = ci.img_metas(ci.SCALE_FACTOR if rescale else 1.0)
    bbox_results, segm_results = m.simple_test(feats, [props], metas, rescale=rescale)
    assert len(bbox_results) == 80 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in bbox_results)
    dets, labels = _class_major(bbox_results)
    assert len(labels) == len(z[f'{tag}_labels']) and np.array_equal(labels, z[f'{tag}_labels'])
    e = assert_close_via_f64(dets, z[f'{tag}_dets'], z[f'{tag}_dets64'], f'simple_test rescale={rescale}')
    print('dets: err %.3g, reference err %.3g, scale %.3g' % e)
    # the bitmaps, exactly
    assert [len(c) for c in segm_results] == [len(c) for c in bbox_results]
    shape = tuple(z[f'{tag}_bits_shape'])
    want = np.unpackbits(z[f'{tag}_bits'])[:int(np.prod(shape))].reshape(shape).astype(bool)
    got = np.stack([s for c in segm_results for s in c])
    assert got.shape == want.shape == (len(labels), ci.IMG_H, ci.IMG_W) and got.dtype == np.bool_
    full = want.reshape(len(want), -1).any(1)
    assert full.any() and not full.all()
    assert np.array_equal(got, want), f'{int((got != want).sum())} pixels differ'
    # the label channel of the 14 x 14 logits
    det, lab = m.simple_test_bboxes(feats, metas, [props], m.test_cfg, rescale=rescale)
    boxes, _ = m._mask_boxes(det, metas[0]['scale_factor'], rescale)
    logits = m._mask_logits(feats, bbox2roi([boxes]).contiguous(), lab)
    assert tuple(logits.shape) == (len(lab), 80, 14, 14)
    order = torch.sort(lab, stable=True)[1]
    picked = logits[torch.arange(len(lab), device=lab.device), lab][order]
    e = assert_close_via_f64(picked, z[f'{tag}_logits'], z[f'{tag}_logits64'], f'mask logits rescale={rescale}')
    print('logits: err %.3g, reference err %.3g, scale %.3g' % e)
    again = m.simple_test(feats, [props], metas, rescale=rescale)
    assert all(np.array_equal(a, b) for a, b in zip(bbox_results, again[0])), 'two identical calls differ'
    assert all(np.array_equal(p, q) for a, b in zip(segm_results, again[1]) for p, q in zip(a, b))


@pytest.mark.parametrize('tag,rescale', [('plain', False), ('rescale', True)])
def test_faster_config_returns_boxes_only(c4, tag, rescale):
    heads, z, ci = c4
    m = heads['faster_c4']
    feats, props = _inputs(ci)
    res = m.simple_test(feats, [props], ci.img_metas(ci.SCALE_FACTOR if rescale else 1.0), rescale=rescale)
    assert isinstance(res, list) and len(res) == 80 and all(isinstance(r, np.ndarray) for r in res)
    dets, labels = _class_major(res)
    assert np.array_equal(labels, z[f'faster_{tag}_labels'])
    assert_close_via_f64(dets, z[f'faster_{tag}_dets'], z[f'faster_{tag}_dets64'], f'faster simple_test rescale={rescale}')


def test_batch_equals_one_image_calls(c4):
    heads, z, ci = c4
    m = heads['mask_c4']
    x2 = [f.cuda() for f in ci.c4_feats(batch=2)]
    props = [ci.proposals().cuda(), ci.proposals(seed=99, n=9).cuda()]
    for rescale in (False, True):
        metas = ci.img_metas(ci.SCALE_FACTOR if rescale else 1.0) * 2
        batch = m.batch_simple_test(x2, props, metas, rescale=rescale)
        assert len(batch) == 2
        for b in range(2):
            xb = [f[b:b + 1].contiguous() for f in x2]
            one_boxes, one_masks = m.simple_test(xb, [props[b]], [metas[b]], rescale=rescale)
            assert sum(len(c) for c in one_boxes) > 0
            assert all(np.array_equal(p, q) for p, q in zip(batch[b][0], one_boxes)), f'image {b} rescale={rescale}'
            assert [len(c) for c in batch[b][1]] == [len(c) for c in one_masks]
            assert all(np.array_equal(p, q) for a, c in zip(batch[b][1], one_masks) for p, q in zip(a, c))
    assert np.array_equal(_class_major(batch[0][0])[1], z['rescale_labels'])          # image 0 is the fixture's image
    faster = heads['faster_c4'].batch_simple_test(x2, props, metas, rescale=True)
    assert all(np.array_equal(p, q) for b in range(2) for p, q in zip(faster[b], batch[b][0]))


def test_aug_test_of_one_plain_view_is_simple_test(c4):
    heads, z, ci = c4
    m = heads['mask_c4']
    feats, props = _inputs(ci)
    metas = ci.img_metas(1.0)
    one_boxes, one_masks = m.simple_test(feats, [props], metas, rescale=True)
    aug_boxes, aug_masks = m.aug_test([feats], [props], [metas], rescale=True)
    assert all(np.array_equal(p, q) for p, q in zip(aug_boxes, one_boxes))
    assert np.array_equal(_class_major(aug_boxes)[1], z['plain_labels'])
    assert [len(c) for c in aug_masks] == [len(c) for c in one_masks]
    assert all(np.array_equal(p, q) for a, c in zip(aug_masks, one_masks) for p, q in zip(a, c))


def test_zero_proposals_and_zero_detections(c4):
    heads, z, ci = c4
    m = heads['mask_c4']
    feats, props = _inputs(ci)
    none = props[:0]
    bbox_results, segm_results = m.simple_test(feats, [none], ci.img_metas())
    assert len(bbox_results) == 80 and all(a.shape == (0, 5) and a.dtype == np.float32 for a in bbox_results)
    assert len(segm_results) == 80 and all(c == [] for c in segm_results)
    x2 = [f.cuda() for f in ci.c4_feats(batch=2)]
    batch = m.batch_simple_test(x2, [none, none], ci.img_metas() * 2)
    assert len(batch) == 2 and all(a.shape == (0, 5) for r in batch for a in r[0]) and all(c == [] for r in batch for c in r[1])
    mixed = m.batch_simple_test(x2, [props, none], ci.img_metas() * 2)                # one image without proposals
    assert np.array_equal(_class_major(mixed[0][0])[1], z['plain_labels']) and all(a.shape == (0, 5) for a in mixed[1][0])
    with torch.no_grad():
        r = m._bbox_forward(feats, none.new_zeros((0, 5)))
    assert tuple(r['cls_score'].shape) == (0, 81) and tuple(r['bbox_pred'].shape) == (0, 320)
    assert tuple(r['bbox_feats'].shape) == (0, 2048, 7, 7)
    # zero detections into the mask branch: the logits are 14 x 14, the shared head's stride accounted for
    det, lab = none.new_zeros((0, 5)), torch.zeros((0,), dtype=torch.long, device='cuda')
    assert tuple(m.simple_test_mask_logits(feats, det, lab).shape) == (0, 80, 14, 14)
    assert m.simple_test_mask(feats, ci.img_metas(), det, lab) == [[] for _ in range(80)]
    faster = heads['faster_c4'].simple_test(feats, [none], ci.img_metas())
    assert len(faster) == 80 and all(a.shape == (0, 5) for a in faster)
