"""The opt-in bf16x3 mode of the implicit-GEMM convolutions (dynamask_amd/precision.py, csrc/conv_igemm.hip PREC):
per-op error against float64 next to the exact kernel's, proof that the split kernel runs, determinism, inputs that
stress the split, path parity against the oracle, HIP graphs across a mode switch, and no change outside the mode."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from oracle import ref_model, ref_ops
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu


def _conv_layer(cin, cout, k, seed):
    from dynamask_amd.mask_heads import _Conv
    torch.manual_seed(seed)
    c = _Conv(cin, cout, k)
    with torch.no_grad():
        c.bias.uniform_(-0.1, 0.1)
    return c.cuda()


def _refs(srcs, c, relu=False):
    """The same convolution on the CPU in fp32 and in float64 (torch)."""
    x = torch.cat([s.cpu() for s in srcs], 1)
    out = []
    for dt in (torch.float32, torch.float64):
        y = torch.nn.functional.conv2d(x.to(dt), c.weight.detach().cpu().to(dt), c.bias.detach().cpu().to(dt),
                                       padding=c.kernel_size // 2)
        out.append(torch.relu(y) if relu else y)
    return out


def _both_modes(fn):
    """fn() under no_grad in the exact mode and in bf16x3."""
    from dynamask_amd import conv_precision
    res = {}
    for p in ('fp32', 'bf16x3'):
        with conv_precision(p), torch.no_grad():
            res[p] = fn()
            res[p] = [t.clone() for t in res[p]] if isinstance(res[p], (list, tuple)) else res[p].clone()
    return res['fp32'], res['bf16x3']


def _check_triangle(name, exact, split, ref32, ref64):
    err_split, ref_err, _ = assert_close_via_f64(split, ref32, ref64, name=f'{name} bf16x3')
    err_exact, _, _ = assert_close_via_f64(exact, ref32, ref64, name=f'{name} fp32')
    print(f'{name}: |.-f64| exact {err_exact:.3g}, bf16x3 {err_split:.3g} (fp32 CPU {ref_err:.3g})')
    assert err_split <= 1.25 * err_exact, (name, err_split, err_exact)


def _rand(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def test_conv3x3_256_to_256_at_14_is_split_and_within_the_f64_triangle():
    from dynamask_amd import ops
    c = _conv_layer(256, 256, 3, 1)
    x = _rand(64, 256, 14, 14, seed=2)
    assert ops.bf16x3_routed(256, 3, 14, 14)
    exact, split = _both_modes(lambda: c.run(x, relu=False))
    r32, r64 = _refs([x], c)
    _check_triangle('conv3x3 256->256 @14', exact, split, r32, r64)
    # the split kernel ran: its sums are not the exact kernel's bits (this fails where no bf16x3 kernel exists)
    assert not torch.equal(exact, split)


def test_conv3x3_tail_couts_and_multi_source_slice_and_grouped_semantic():
    from dynamask_amd import ops
    # 3x3 with tail couts (the DCN offset convolution's shape)
    c = _conv_layer(256, 36, 3, 3)
    x = _rand(48, 256, 14, 14, seed=4)
    exact, split = _both_modes(lambda: c.run(x))
    r32, r64 = _refs([x], c)
    _check_triangle('conv3x3 256->36 @14', exact, split, r32, r64)
    # multi-source 1x1 into a channel slice of a wider tensor (the fuse convolution)
    c = _conv_layer(514, 256, 1, 5)
    a, b, t = _rand(40, 256, 14, 14, seed=6), _rand(40, 256, 14, 14, seed=7), _rand(40, 2, 14, 14, seed=8)

    def fuse():
        big = torch.zeros(40, 300, 14, 14, device='cuda')
        c.run([a, b, t], relu=True, out=big, out_ch_offset=20)
        return big
    exact, split = _both_modes(fuse)
    r32, r64 = _refs([a, b, t], c, relu=True)
    for o in (exact, split):
        assert not o[:, :20].any() and not o[:, 276:].any()
    _check_triangle('fuse 1x1 [256,256,2]->256 slice', exact[:, 20:276], split[:, 20:276], r32, r64)
    assert ops.bf16x3_routed(256, 1, 14, 14) and not torch.equal(exact, split)
    # the grouped FPN-wide semantic 1x1s (one launch): both layouts through ops.conv1x1_group
    convs = [_conv_layer(256, co, 1, 9 + i) for i, co in enumerate((256, 128, 64))]
    feats = [_rand(1, 256, h, w, seed=20 + i) for i, (h, w) in enumerate(((16, 20), (32, 40), (64, 80)))]
    outs = {}
    for p in ('fp32', 'bf16x3'):
        with torch.no_grad():
            outs[p] = ops.conv1x1_group(feats, [cv.packed([256], p) for cv in convs], [cv.bias.detach() for cv in convs],
                                        [cv.out_channels for cv in convs], relu=True)
    for i, (cv, f) in enumerate(zip(convs, feats)):
        r32, r64 = _refs([f], cv, relu=True)
        _check_triangle(f'semantic 1x1 256->{cv.out_channels}', outs['fp32'][i], outs['bf16x3'][i], r32, r64)
        # the grouped launch gives a single launch's bits in either layout
        with torch.no_grad():
            one = ops.conv2d([f], cv.packed([256], 'bf16x3'), cv.bias.detach(), cv.out_channels, 1, relu=True)
        assert torch.equal(one, outs['bf16x3'][i])


def test_split_k_workspace_call_at_16_rois():
    from dynamask_amd import ops
    c = _conv_layer(256, 256, 3, 30)
    x = _rand(16, 256, 14, 14, seed=31)
    assert ops.lib().dm_conv2d_splitk_floats(16, 14, 14, 256, 3) > 0

    def run():
        with ops.splitk_scope():
            return c.run(x, relu=True)
    exact, split = _both_modes(run)
    r32, r64 = _refs([x], c, relu=True)
    _check_triangle('conv3x3 256->256 @14 split-K, 16 RoIs', exact, split, r32, r64)
    assert not torch.equal(exact, split)
    _, again = _both_modes(run)
    assert torch.equal(split, again)


def test_bf16x3_is_deterministic():
    c = _conv_layer(256, 256, 3, 40)
    x = _rand(100, 256, 14, 14, seed=41)
    _, s1 = _both_modes(lambda: c.run(x))
    _, s2 = _both_modes(lambda: c.run(x))
    assert torch.equal(s1, s2)


def _decode_bf16x3(wp, cin, cout, kk):
    """Host decode of the bf16x3 pack of ONE source of ``cin`` channels: -> hi, mid, lo [kk, cin, coutP] (float64)."""
    coutp = (cout + 31) // 32 * 32
    kq = (cin + 15) // 16 * 6
    raw = wp.view(torch.int32).cpu().numpy().astype(np.uint32).reshape(kk, kq, coutp, 4)
    halves = np.stack([raw & 0xFFFF, raw >> 16], -1).reshape(kk, kq, coutp, 8)       # bf16 bits, 8 channels per word
    planes = (halves.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    blocks = planes.reshape(kk, kq // 6, 2, 3, coutp, 8)          # [tap][block][half][part][col][channel in half]
    out = blocks.transpose(3, 0, 1, 2, 5, 4).reshape(3, kk, (kq // 6) * 16, coutp)
    return out[0][:, :cin], out[1][:, :cin], out[2][:, :cin]


def test_weight_split_keeps_subnormal_residuals_and_zeroes_non_finite():
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(50)
    w = torch.randn(32, 48, 1, 1, generator=g)
    w[:, :16] *= 1e-36                          # hi ~2^-120: residuals (~2^-129) below the fp32 normal range (2^-126)
    w[:, 16:32] = torch.exp(torch.empty(32, 16, 1, 1).uniform_(-69, 69, generator=g))      # 1e-30 .. 1e30
    w[0, 40, 0, 0], w[1, 41, 0, 0], w[2, 42, 0, 0] = float('inf'), float('-inf'), 0.0
    wp = ops.pack_conv_weight(w.cuda(), precision='bf16x3')
    assert ops.conv_layout(wp) == 'bf16x3'
    hi, mid, lo = _decode_bf16x3(wp, 48, 32, 1)
    x = w.reshape(32, 48).t().double().numpy()
    fin = np.isfinite(x)
    rec = (hi[0] + mid[0] + lo[0])[:, :32]
    # exact where the residuals are normal; within bf16's subnormal spacing (2^-133) where they are not
    assert np.all(np.abs(rec[fin] - x[fin]) <= np.maximum(2.0 ** -24 * np.abs(x[fin]), 2.0 ** -133))
    assert hi[0][40, 0] == np.inf and hi[0][41, 1] == -np.inf
    assert mid[0][40, 0] == 0 and lo[0][40, 0] == 0 and mid[0][41, 1] == 0 and lo[0][41, 1] == 0


def test_inputs_that_stress_the_split():
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(60)
    c = _conv_layer(64, 128, 1, 61)
    # magnitudes 1e-30 .. 1e30 with zeros: the gate (1e-4 of scale) or the exact kernel's bits
    mag = torch.exp(torch.empty(8, 64, 14, 14).uniform_(-69, 69, generator=g))
    x = (mag * torch.randn(8, 64, 14, 14, generator=g).sign())
    x[torch.rand(8, 64, 14, 14, generator=g) < 0.1] = 0.0
    x = x.cuda()

    def run():
        return ops.conv2d([x], c.packed([64], ops.inference_precision()), c.bias.detach(), 128, 1)
    exact, split = _both_modes(run)
    r32, r64 = _refs([x], c)
    assert torch.isfinite(split).all() and torch.isfinite(exact).all()
    if not torch.equal(exact, split):
        assert_close_via_f64(split, r32, r64, name='1e-30 .. 1e30')
    # subnormal residuals: activations whose bf16 remainders fall below the fp32 normal range, beside normal ones
    x2 = torch.randn(8, 64, 14, 14, generator=g)
    x2[:, :32] *= 3e-37
    x2 = x2.cuda()
    exact, split = _both_modes(lambda: ops.conv2d([x2], c.packed([64], ops.inference_precision()), c.bias.detach(), 128, 1))
    r32, r64 = _refs([x2], c)
    assert torch.isfinite(split).all()
    if not torch.equal(exact, split):
        assert_close_via_f64(split, r32, r64, name='subnormal residuals')
    # an Inf in the input: the same non-finite pattern as the exact kernel (3x3: it reaches the 3 x 3 neighbourhood)
    c3 = _conv_layer(256, 256, 3, 62)
    x3 = _rand(4, 256, 14, 14, seed=63)
    x3[1, 7, 5, 5] = float('inf')
    x3[2, 100, 0, 13] = float('-inf')
    exact, split = _both_modes(lambda: c3.run(x3))
    assert not torch.equal(exact, split)
    bad_e, bad_s = ~torch.isfinite(exact), ~torch.isfinite(split)
    assert bad_e.any() and torch.equal(bad_e, bad_s)


def _roi_head():
    from dynamask_amd import registry, roi_head, losses, mask_heads, roi_extractors  # noqa: F401  (registers the classes)
    cfg = dict(type='DynaMaskRoIHead',
               mask_roi_extractor=dict(type='SingleRoIExtractor', **gi.MASK_ROI_EXTRACTOR_CFG),
               mask_head=dict(type='DynaMaskHead', **gi.MASK_HEAD_CFG),
               train_cfg=registry.ConfigDict(flops=[0.23, 0.62, 1.01, 1.4], Lambda=0.3, mask_size=28),
               test_cfg=registry.ConfigDict(mask_thr_binary=0.5))
    m = registry.build_head(cfg)
    m.load_state_dict({**gi.head_state(), **gi.mask_pre_state()}, strict=True)
    return m.cuda().eval()


def _dev(t):
    return t.cuda().contiguous()


def test_simple_test_mask_logits_under_bf16x3_vs_oracle():
    from dynamask_amd import conv_precision
    hi = gi.head_inputs()
    m = _roi_head()
    sel = hi['rois'][:, 0] == 0
    boxes, labels = hi['rois'][sel][:, 1:], hi['labels'][sel]
    with torch.no_grad():
        plain = m.simple_test_mask_logits([_dev(f) for f in hi['feats']], _dev(boxes), _dev(labels)).clone()
        with conv_precision('bf16x3'):
            out = m.simple_test_mask_logits([_dev(f) for f in hi['feats']], _dev(boxes), _dev(labels))
        rois = torch.cat([torch.zeros(len(boxes), 1), boxes], 1)
        ips, _ = ref_model.mask_forward(gi.head_state(), hi['feats'], rois, labels)
        ref = ref_model.boundary_merge(ips)
    assert not torch.equal(out, plain)
    got = out.cpu()
    # test_path_gpu.py's gate: ties are PROVEN -- the oracle's merge with the threshold at -1e-4, 0 and +1e-4 on the logit;
    # where the three agree the product must agree to 1e-4, everywhere else with one of the three
    import torch.nn.functional as F

    def merge_thr(stage_preds, thr):
        preds = [p.clone() for p in stage_preds[1:]]
        for idx in range(len(preds) - 1):
            inst = preds[idx].squeeze(1) >= thr
            nb = (ref_model.generate_block_target(inst, boundary_width=1) != 1).unsqueeze(1)
            nb = F.interpolate(nb.float(), preds[idx + 1].shape[-2:], mode='bilinear', align_corners=True) >= 0.5
            pre_pred = F.interpolate(preds[idx], preds[idx + 1].shape[-2:], mode='bilinear', align_corners=True)
            preds[idx + 1][nb] = pre_pred[nb]
        return preds[-1]
    lo, hi_ = merge_thr(ips, -1e-4), merge_thr(ips, 1e-4)

    def near(a, b):
        return (a - b).abs() <= 1e-4 + 1e-4 * b.abs()
    certain = near(lo, ref) & near(hi_, ref)
    assert bool(near(got, ref)[certain].all()), 'a pixel no threshold tie can reach differs from the oracle'
    tied = ~certain
    assert bool((near(got, ref) | near(got, lo) | near(got, hi_))[tied].all()), 'a tie-affected pixel matches no side of its tie'
    print(f'bf16x3 merge: {int(tied.sum())} of {tied.numel()} pixels within reach of a tie, '
          f'{int((~near(got, ref)).sum())} of them on the other side than the oracle')
    assert float(tied.float().mean()) < 1e-2
    # the stage logits themselves, at the existing gate
    with torch.no_grad(), conv_precision('bf16x3'):
        res = m._mask_forward([_dev(f) for f in hi['feats']], _dev(rois), _dev(labels))
    for k, (g_, r_) in enumerate(zip(res['stage_instance_preds'], ips)):
        np.testing.assert_allclose(g_.cpu().numpy(), r_.numpy(), atol=1e-4, rtol=1e-4, err_msg=f'stage {k}')


def test_dynamic_mask_logits_under_bf16x3_keeps_the_exits():
    from dynamask_amd import conv_precision, synth
    feats = synth.make_fpn(1, 256, 320, 256, seed=11)
    rois = synth.make_rois(1, 21, 256, 320, seed=12)
    labels = synth.make_labels(21, seed=13)
    m = _roi_head()
    fd = [_dev(f) for f in feats]
    sd = {**gi.head_state(), **gi.mask_pre_state()}
    with torch.no_grad():
        r_exact = m.dynamic_mask_logits(fd, _dev(rois[:, 1:]), _dev(labels))
        with conv_precision('bf16x3'):
            r_split = m.dynamic_mask_logits(fd, _dev(rois[:, 1:]), _dev(labels))
        ips, _ = ref_model.mask_forward(sd, feats, rois, labels)
    assert torch.equal(r_exact['exits'], r_split['exits']) and torch.equal(r_exact['order'], r_split['order'])
    exits = r_split['exits'].cpu()
    ref = ref_model.dynamic_exit_logits(ips, exits, merge=True)
    flips = 0
    for p, j in enumerate(r_split['order'].cpu().tolist()):
        got = r_split['preds'][int(exits[j])][p].cpu()
        flips += int(((got - ref[j]).abs() > 1e-4 + 1e-4 * ref[j].abs()).sum())
    assert flips <= 20, flips          # test_path_gpu.py's gate for the exact mode


def test_standard_roi_head_with_fcn_mask_head_under_bf16x3():
    from dynamask_amd import conv_precision, registry, roi_head, bbox_heads, losses, mask_heads, roi_extractors  # noqa: F401
    from dynamask_amd.registry import ConfigDict
    up = 'deconv'
    mcfg = dict(type='FCNMaskHead', **gi.FCN_HEAD_CFG)        # (deconv upsample: the default)
    m = registry.build_head(dict(
        type='StandardRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **gi.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **gi.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **gi.MASK_ROI_EXTRACTOR_CFG), mask_head=mcfg,
        train_cfg=registry._to_cfgdict(gi.RCNN_TRAIN_CFG), test_cfg=ConfigDict(**gi.RCNN_TEST_CFG)))
    fsd = gi.fcn_state(up)
    m.load_state_dict({**fsd, **gi.bbox_head_state(), **gi.mask_pre_state()}, strict=True)
    m = m.cuda().eval()
    hi = gi.head_inputs()
    feats = [_dev(f) for f in hi['feats']]
    sel = hi['rois'][:, 0] == 0
    rois = hi['rois'][sel].contiguous()
    sdo = {k[len('mask_head.'):]: v for k, v in fsd.items()}
    ref_feats = ref_ops.single_roi_extractor(hi['feats'][:4], rois, 14, (4, 8, 16, 32))
    ref_pred = ref_model.fcn_mask_head_forward(sdo, ref_feats, upsample=up)
    with torch.no_grad():
        exact = m._mask_forward(feats, _dev(rois))['mask_pred'].clone()
        with conv_precision('bf16x3'):
            split = m._mask_forward(feats, _dev(rois))['mask_pred']
    assert not torch.equal(exact, split)
    np.testing.assert_allclose(split.cpu().numpy(), ref_pred.numpy(), atol=1e-4, rtol=1e-4)


def test_deconv_bf16x3_within_the_f64_triangle():
    from dynamask_amd import ops
    from dynamask_amd.mask_heads import _Deconv
    torch.manual_seed(80)
    d = _Deconv(256, 256).cuda()
    with torch.no_grad():
        d.bias.uniform_(-0.1, 0.1)
    x = _rand(48, 256, 14, 14, seed=81)
    assert ops.deconv_precision_for(14, 14) == 'fp32'
    exact, split = _both_modes(lambda: d(x, relu=True))
    xs = x.cpu()
    r32, r64 = [torch.relu(torch.nn.functional.conv_transpose2d(xs.to(dt), d.weight.detach().cpu().to(dt),
                                                                d.bias.detach().cpu().to(dt), stride=2))
                for dt in (torch.float32, torch.float64)]
    _check_triangle('deconv 2x2/s2 256->256 @14', exact, split, r32, r64)
    if ops.BF16X3_DECONV_MAX_HW[0] >= 14 * 14:
        assert not torch.equal(exact, split)
    with torch.no_grad():        # both layouts through the op itself, whatever the routing
        wp = ops.pack_deconv_weight(d.weight.detach(), precision='bf16x3')
        direct = ops.deconv2x2(x, wp, d.bias.detach(), 256, relu=True)
    _check_triangle('deconv 2x2/s2 bf16x3 layout', exact, direct, r32, r64)
    assert not torch.equal(exact, direct)


def test_first_forked_bf16x3_calls_read_finished_packs():
    """The first bf16x3 call of a fresh head makes its bf16x3 packs; from 80 detections (eager) the RoIs run as chunks on
    side streams, so the packs must exist before the fork (DynaMaskHead.prepack).  The first call of each entry point must
    give the bits of the second (run under DM_HAZARD=1, the tracker reports a chain that reads an unordered pack)."""
    from dynamask_amd import conv_precision, synth
    feats = [_dev(f) for f in synth.make_fpn(1, 608, 1024, 256, seed=90)]
    rois = synth.make_rois(1, 512, 608, 1024, seed=91)
    labels = _dev(synth.make_labels(512, seed=92))
    with torch.no_grad(), conv_precision('bf16x3'):
        m = _roi_head()
        assert m.num_streams > 1 and 100 >= m.stream_split_min
        first = m.simple_test_mask_logits(feats, _dev(rois[:100, 1:]), labels[:100]).clone()
        second = m.simple_test_mask_logits(feats, _dev(rois[:100, 1:]), labels[:100])
        assert torch.equal(first, second)
        m = _roi_head()
        first = m._mask_forward(feats, _dev(rois), labels, last_stage=1)['stage_instance_preds'][1].clone()
        second = m._mask_forward(feats, _dev(rois), labels, last_stage=1)['stage_instance_preds'][1]
        assert torch.equal(first, second)
        # after a weight update the packs are stale again: the next first call repacks before the fork
        with torch.no_grad():
            m.mask_head.instance_convs[0].conv.weight.mul_(1.01)
        first = m._mask_forward(feats, _dev(rois), labels, last_stage=1)['stage_instance_preds'][1].clone()
        second = m._mask_forward(feats, _dev(rois), labels, last_stage=1)['stage_instance_preds'][1]
        assert torch.equal(first, second)


def test_small_maps_without_a_3x3_build_run_exact():
    """3x3 maps whose staged plane exceeds the bf16x3 build's (6 x 6, 8 x 32, 1 x 40) are routed to the exact kernel."""
    from dynamask_amd import ops
    c = _conv_layer(64, 64, 3, 95)
    for h, w in ((6, 6), (8, 32), (1, 40), (4, 4)):
        x = _rand(3, 64, h, w, seed=96)
        assert not ops.bf16x3_routed(64, 3, h, w)
        exact, split = _both_modes(lambda: c.run(x))
        assert torch.equal(exact, split), (h, w)
    assert ops.bf16x3_routed(64, 3, 14, 14) and ops.bf16x3_routed(64, 3, 16, 16)


def test_graphs_follow_the_mode():
    from dynamask_amd import conv_precision, ops, synth
    m = _roi_head()
    feats = [_dev(f) for f in synth.make_fpn(1, 608, 1024, 256, seed=3)]
    rois = synth.make_rois(1, 16, 608, 1024, seed=4)
    labels = _dev(synth.make_labels(16, seed=5))
    boxes = _dev(rois[:, 1:])
    was = ops.CONV_SPLITK[0]
    ops.CONV_SPLITK[0] = False          # (a bucket pads the RoI count and split-K depends on it: as test_path_gpu.py)
    try:
        with torch.no_grad():
            with conv_precision('bf16x3'):
                eager_s = m.simple_test_mask_logits(feats, boxes, labels).clone()
            eager_e = m.simple_test_mask_logits(feats, boxes, labels).clone()
            assert not torch.equal(eager_s, eager_e)
            gl = m.enable_inference_graphs(True)
            with conv_precision('bf16x3'):
                assert torch.equal(m.simple_test_mask_logits(feats, boxes, labels), eager_s)
            # captured in fp32, then the mode switches: the replay must be the bf16x3 eager result, never the fp32 graph
            assert torch.equal(m.simple_test_mask_logits(feats, boxes, labels), eager_e)
            n = gl.captures
            with conv_precision('bf16x3'):
                assert torch.equal(m.simple_test_mask_logits(feats, boxes, labels), eager_s)
            assert gl.captures == n
            assert torch.equal(m.simple_test_mask_logits(feats, boxes, labels), eager_e) and gl.captures == n
            m.enable_inference_graphs(False)
    finally:
        ops.CONV_SPLITK[0] = was


def test_no_behaviour_change_with_grad_or_in_the_default_mode():
    from dynamask_amd import conv_precision, get_conv_precision
    c = _conv_layer(256, 256, 3, 70)
    x = _rand(16, 256, 14, 14, seed=71)
    with torch.enable_grad():
        a = c.run(x).detach().clone()
        with conv_precision('bf16x3'):
            b = c.run(x).detach().clone()
    assert torch.equal(a, b)
    hi = gi.head_inputs()
    m = _roi_head()
    sel = hi['rois'][:, 0] == 0
    boxes, labels = _dev(hi['rois'][sel][:, 1:]), _dev(hi['labels'][sel])
    feats = [_dev(f) for f in hi['feats']]
    assert get_conv_precision() == 'fp32'
    with torch.no_grad():
        untouched = m.simple_test_mask_logits(feats, boxes, labels).clone()
        with conv_precision('fp32'):
            default = m.simple_test_mask_logits(feats, boxes, labels)
    assert torch.equal(untouched, default)
