"""Hybrid Task Cascade on the MI355X: the three kernels of section K26 (bilinear resize to any size, the convolution with
the addend after the activation, the single-map RoIAlign added into RoI features) against float64 and against the launches
they replace, and HybridTaskCascadeRoIHead's simple_test / aug_test against the reference fixture g22
(tests/golden/make_golden_htc.py), with and without the semantic head, batched, grouped against per-stage, encoded and in
the bf16x3 mode.  Kernel outputs are written into buffers followed by a canary that must survive."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64, assert_grad_close

pytestmark = pytest.mark.gpu

CANARY = 12345.678


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_g(seed)) * scale


def _with_canary(shape, fill=None):
    n = int(np.prod(shape))
    buf = torch.full((n + 4096,), CANARY, device='cuda')
    view = buf[:n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _check_canary(buf, shape, what):
    n = int(np.prod(shape))
    assert bool((buf[n:] == CANARY).all()), f'{what}: the canary past the output was overwritten'


# ------------------------------------------------------------------ resize
# (the level geometries of the 128 x 160 and the 800 x 1333 pyramids towards their stride-8 maps, odd sizes, out == 1)
@pytest.mark.parametrize('hin,win,hout,wout', [(32, 40, 16, 20), (8, 10, 16, 20), (4, 5, 16, 20), (2, 3, 16, 20),
                                               (200, 336, 100, 168), (50, 84, 100, 168), (25, 42, 100, 168),
                                               (13, 21, 100, 168), (7, 11, 13, 5), (9, 4, 1, 1), (5, 7, 1, 9), (1, 1, 3, 4),
                                               (6, 6, 6, 6)])
def test_resize_against_float64(hin, win, hout, wout):
    from dynamask_amd import ops
    x = _rand((2, 3, hin, win), hin * 100 + wout)
    shape = (2, 3, hout, wout)
    buf, out = _with_canary(shape)
    ops.resize_bilinear(x.cuda(), (hout, wout), out=out)
    _check_canary(buf, shape, 'resize_bilinear')
    ref32 = F.interpolate(x, size=(hout, wout), mode='bilinear', align_corners=True)
    ref64 = F.interpolate(x.double(), size=(hout, wout), mode='bilinear', align_corners=True)
    assert_close_via_f64(out, ref32, ref64, f'resize {hin}x{win} -> {hout}x{wout}')
    if (hin, win) == (hout, wout):
        assert torch.equal(out.cpu(), x)


@pytest.mark.parametrize('h,w', [(14, 14), (7, 9), (1, 5), (50, 84)])
def test_resize_equals_upsample2x_at_x2(h, w):
    from dynamask_amd import ops
    x = _rand((2, 5, h, w), h + w).cuda()
    assert torch.equal(ops.resize_bilinear(x, (2 * h, 2 * w)), ops.upsample2x(x, align_corners=True))


# ------------------------------------------------------------------ the addend after the activation
@pytest.mark.parametrize('NB,cin,cout,H,W', [(1, 256, 256, 16, 20), (3, 256, 256, 14, 14), (2, 64, 48, 9, 7), (2, 40, 24, 6, 11),
                                             (1, 96, 160, 14, 14), (50, 256, 256, 14, 14), (2, 256, 256, 100, 168)])
@pytest.mark.parametrize('alias', [False, True])
def test_post_add_equals_conv_relu_then_add(NB, cin, cout, H, W, alias):
    """Bit for bit the two-launch form; ``out`` a new tensor (the addend survives) or the addend itself."""
    from dynamask_amd import ops
    x = _rand((NB, cin, H, W), NB + cin).cuda()
    wp = ops.pack_conv_weight(_rand((cout, cin, 1, 1), cout, (2.0 / cin) ** 0.5).cuda())
    b = _rand((cout,), 5, 0.1).cuda()
    addend = _rand((NB, cout, H, W), 7).cuda()
    ref = ops.conv2d(x, wp, b, cout, 1, relu=True) + addend
    shape = (NB, cout, H, W)
    if alias:
        buf, out = _with_canary(shape, addend)
        got = ops.conv1x1_post_add(x, wp, b, cout, out, relu=True, out=out)
        assert got is out
    else:
        buf, out = _with_canary(shape)
        keep = addend.clone()
        ops.conv1x1_post_add(x, wp, b, cout, addend, relu=True, out=out)
        assert torch.equal(addend, keep), 'the addend must survive'
    _check_canary(buf, shape, 'conv1x1_post_add')
    assert torch.equal(out, ref)


def test_post_add_against_float64():
    from dynamask_amd import ops
    x, w, b, a = _rand((2, 72, 11, 13), 1), _rand((40, 72, 1, 1), 2, 0.2), _rand((40,), 3), _rand((2, 40, 11, 13), 4)
    got = ops.conv1x1_post_add(x.cuda(), ops.pack_conv_weight(w.cuda()), b.cuda(), 40, a.cuda())
    ref = lambda t: a.to(t) + F.relu(F.conv2d(x.to(t), w.to(t), b.to(t)))
    assert_close_via_f64(got, ref(torch.float32), ref(torch.float64), 'post-activation add')
    # no activation: addend + (conv + bias)
    got = ops.conv1x1_post_add(x.cuda(), ops.pack_conv_weight(w.cuda()), b.cuda(), 40, a.cuda(), relu=False)
    ref = lambda t: a.to(t) + F.conv2d(x.to(t), w.to(t), b.to(t))
    assert_close_via_f64(got, ref(torch.float32), ref(torch.float64), 'post add without ReLU')


# ------------------------------------------------------------------ RoIAlign added into RoI features
def _sem_case(B, counts, H, W, C, seed):
    """A semantic map and RoIs per image: inside, partly outside, wholly outside, tiny, and the whole map."""
    g = _g(seed)
    sem = torch.randn(B, C, H, W, generator=g)
    rows = []
    for b, n in enumerate(counts):
        xy = torch.rand(n, 2, generator=g) * torch.tensor([W * 8.0, H * 8.0]) - 20
        wh = torch.rand(n, 2, generator=g) * torch.tensor([W * 4.0, H * 4.0]) + 1
        r = torch.cat([torch.full((n, 1), float(b)), xy, xy + wh], 1)
        if n >= 5:
            r[0, 1:] = torch.tensor([-300.0, -200.0, -100.0, -50.0])            # wholly outside
            r[1, 1:] = torch.tensor([W * 8 + 40.0, 10.0, W * 8 + 90.0, 60.0])    # wholly outside (right)
            r[2, 1:] = torch.tensor([-30.0, -30.0, W * 8 + 30.0, H * 8 + 30.0])  # the whole map and more
            r[3, 1:] = torch.tensor([17.3, 9.1, 18.0, 9.9])                      # below one bin
            r[4, 1:] = torch.tensor([W * 8 - 25.0, H * 8 - 31.0, W * 8 + 50.0, H * 8 + 12.0])   # over the corner
        rows.append(r)
    return sem, torch.cat(rows).contiguous()


def _roi_align_f64(sem, rois, P, scale):
    """RoIAlign (aligned, avg, adaptive grid) in float64 on the host, straight from the definition."""
    sem = sem.double()
    N, C = rois.shape[0], sem.shape[1]
    H, W = sem.shape[2:]
    out = torch.zeros(N, C, P, P, dtype=torch.float64)
    for n in range(N):
        b = int(rois[n, 0])
        x1, y1, x2, y2 = [float(np.float32(v) * np.float32(scale) - np.float32(0.5)) for v in rois[n, 1:].tolist()]
        rw, rh = np.float32(np.float32(x2) - np.float32(x1)), np.float32(np.float32(y2) - np.float32(y1))
        gh, gw = int(np.ceil(rh / np.float32(P))), int(np.ceil(rw / np.float32(P)))
        if gh <= 0 or gw <= 0:
            continue
        bh, bw = float(rh) / P, float(rw) / P
        ys = (y1 + (torch.arange(P * gh, dtype=torch.float64) + 0.5) * bh / gh)
        xs = (x1 + (torch.arange(P * gw, dtype=torch.float64) + 0.5) * bw / gw)

        def taps(c, size):
            valid = ~((c < -1.0) | (c > size))
            c = c.clamp(min=0)
            lo = c.floor().long()
            top = lo >= size - 1
            lo = torch.where(top, torch.full_like(lo, size - 1), lo)
            hi = torch.where(top, lo, lo + 1)
            c = torch.where(top, lo.double(), c)
            wh = c - lo.double()
            return lo, hi, (1 - wh) * valid, wh * valid
        ylo, yhi, wyl, wyh = taps(ys, H)
        xlo, xhi, wxl, wxh = taps(xs, W)
        f = sem[b]
        v = (f[:, ylo][:, :, xlo] * (wyl[:, None] * wxl[None]) + f[:, ylo][:, :, xhi] * (wyl[:, None] * wxh[None]) +
             f[:, yhi][:, :, xlo] * (wyh[:, None] * wxl[None]) + f[:, yhi][:, :, xhi] * (wyh[:, None] * wxh[None]))
        out[n] = v.view(C, P, gh, P, gw).mean((2, 4))
    return out


@pytest.mark.parametrize('B,counts,H,W,C', [(1, [37], 16, 20, 256), (3, [40, 0, 9], 16, 20, 64), (3, [5, 130, 70], 100, 168, 32),
                                            (2, [300, 7], 25, 42, 16)])
def test_roi_align_add_identity_is_roi_align_plus_add(B, counts, H, W, C):
    """pool == 1: the bits of ops.roi_align (one level) followed by an add."""
    from dynamask_amd import ops
    sem, rois = _sem_case(B, counts, H, W, C, sum(counts))
    sem, rois = sem.cuda(), rois.cuda()
    N = rois.shape[0]
    feats = _rand((N, C, 14, 14), 3).cuda()
    ref = feats + ops.roi_align([sem], rois, 14, [0.125], 0)
    shape = (N, C, 14, 14)
    buf, out = _with_canary(shape, feats)
    ops.roi_align_add_(out, sem, rois, 14, 0.125)
    _check_canary(buf, shape, 'roi_align_add_ (identity)')
    assert torch.equal(out, ref)
    ref64 = feats.cpu().double() + _roi_align_f64(sem.cpu(), rois.cpu(), 14, 0.125)
    assert_close_via_f64(out, ref, ref64, 'RoIAlign-add (identity) against float64')


@pytest.mark.parametrize('B,counts,H,W,C', [(1, [37], 16, 20, 256), (3, [40, 0, 9], 16, 20, 64), (3, [5, 130, 70], 100, 168, 32),
                                            (2, [300, 7], 25, 42, 16)])
def test_roi_align_add_pooled_against_float64(B, counts, H, W, C):
    """pool == 2 against ops.roi_align + adaptive_avg_pool2d + add, both measured against float64; B images with uneven
    RoI counts, boxes partly and wholly outside the map."""
    from dynamask_amd import ops
    sem, rois = _sem_case(B, counts, H, W, C, sum(counts) + 1)
    sem, rois = sem.cuda(), rois.cuda()
    N = rois.shape[0]
    feats = _rand((N, C, 7, 7), 4).cuda()
    ref32 = feats + F.adaptive_avg_pool2d(ops.roi_align([sem], rois, 14, [0.125], 0), (7, 7))
    ref64 = feats.cpu().double() + F.adaptive_avg_pool2d(_roi_align_f64(sem.cpu(), rois.cpu(), 14, 0.125), (7, 7))
    shape = (N, C, 7, 7)
    buf, out = _with_canary(shape, feats)
    ops.roi_align_add_(out, sem, rois, 14, 0.125)
    _check_canary(buf, shape, 'roi_align_add_ (2 x 2 mean)')
    assert_close_via_f64(out, ref32, ref64, 'RoIAlign-add (2 x 2 mean)')
    # the same launch twice adds twice: deterministic
    again = feats.clone()
    ops.roi_align_add_(again, sem, rois, 14, 0.125)
    assert torch.equal(again, out)


def test_roi_align_add_touches_only_its_rows():
    """N == 0 is a no-op; the rows of the RoIs of one image read that image's map only and leave the other rows alone."""
    from dynamask_amd import ops
    sem, rois = _sem_case(3, [12, 20, 6], 16, 20, 32, 9)
    sem, rois = sem.cuda(), rois.cuda()
    for size in (14, 7):
        feats = _rand((rois.shape[0], 32, size, size), 5).cuda()
        keep = feats.clone()
        ops.roi_align_add_(feats[:0].contiguous(), sem, rois[:0].contiguous(), 14, 0.125)
        assert torch.equal(feats, keep)
        whole = feats.clone()
        ops.roi_align_add_(whole, sem, rois, 14, 0.125)
        # image 1 alone, through a map in which the other images are NaN
        poisoned = sem.clone()
        poisoned[0] = float('nan')
        poisoned[2] = float('nan')
        sub = feats[12:32].clone()
        ops.roi_align_add_(sub, poisoned, rois[12:32].contiguous(), 14, 0.125)
        assert torch.equal(sub, whole[12:32])
        # a batch index outside the map's images adds zeros
        bad = rois[:4].clone()
        bad[:, 0] = 7
        out = feats[:4].clone()
        ops.roi_align_add_(out, sem, bad.contiguous(), 14, 0.125)
        assert torch.equal(out, keep[:4] + 0.0)


def test_refusals_return_the_error_code():
    from dynamask_amd import ops
    from dynamask_amd._lib import lib
    x = _rand((1, 8, 6, 6), 1).cuda()
    out = torch.empty((1, 8, 12, 12), device='cuda')
    L = lib()
    assert L.dm_resize_bilinear_fwd(ops._p(x), 8, 6, 6, 0, 12, ops._p(out), ops._stream()) != 0
    assert L.dm_resize_bilinear_fwd(None, 8, 6, 6, 12, 12, ops._p(out), ops._stream()) != 0
    assert L.dm_resize_bilinear_fwd(ops._p(x), -1, 6, 6, 12, 12, ops._p(out), ops._stream()) != 0
    with pytest.raises(ValueError):
        ops.resize_bilinear(x, (0, 4))
    # post-activation add: 3x3, the accumulate flag, the bf16x3 flag, no addend
    w1 = ops.pack_conv_weight(_rand((8, 8, 1, 1), 2).cuda())
    w3 = ops.pack_conv_weight(_rand((8, 8, 3, 3), 3).cuda())
    o = torch.zeros((1, 8, 6, 6), device='cuda')
    args = lambda w, ks, flags, add: (ops._ptr_array([x]), ops._int_array([8]), None, 1, 1, 6, 6, ops._p(w), None, 8, ks, flags,
                                      ops._p(add), ops._p(o), 8, 0, ops._stream())
    assert L.dm_conv2d_post_add_fwd(*args(w1, 1, 1, o)) == 0
    assert L.dm_conv2d_post_add_fwd(*args(w3, 3, 1, o)) == -3
    assert L.dm_conv2d_post_add_fwd(*args(w1, 1, 3, o)) == -1
    assert L.dm_conv2d_post_add_fwd(*args(w1, 1, 17, o)) == -3
    assert L.dm_conv2d_post_add_fwd(*args(w1, 1, 1, None)) == -1
    with pytest.raises(ValueError, match='bf16x3'):
        ops.conv1x1_post_add(x, ops.pack_conv_weight(_rand((8, 8, 1, 1), 2).cuda(), precision='bf16x3'), None, 8, o)
    with pytest.raises(ValueError, match='addend'):
        ops.conv1x1_post_add(x, w1, None, 8, o[:, :4].contiguous())
    # RoIAlign-add: pool, odd P under the mean, P too large, channels not in quads
    sem = _rand((1, 8, 6, 6), 4).cuda()
    rois = torch.tensor([[0.0, 1.0, 1.0, 30.0, 30.0]], device='cuda')
    f = torch.zeros((1, 8, 14, 14), device='cuda')
    call = lambda C, P, pool: L.dm_roi_align_add_fwd(ops._p(sem), 1, C, 6, 6, 0.125, ops._p(rois), 1, P, 0, pool, ops._p(f),
                                                     ops._stream())
    assert call(8, 14, 1) == 0 and call(8, 14, 2) == 0
    assert call(8, 14, 3) == -1 and call(8, 14, 0) == -1
    assert call(8, 7, 2) == -3 and call(8, 18, 1) == -3 and call(6, 14, 1) == -3
    with pytest.raises(NotImplementedError):
        ops.roi_align_add_(torch.zeros((1, 8, 5, 5), device='cuda'), sem, rois, 14, 0.125)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the heads
def _configs(golden_dir, name):
    import json
    from dynamask_amd import registry
    with open(f'{golden_dir}/g22_htc_configs.json') as f:
        return registry._to_cfgdict(json.load(f))[name]


def _roi_head(golden_dir, name='coco'):
    import htc_inputs as hi
    from dynamask_amd import registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    cfg = _configs(golden_dir, name)
    rh = dict(cfg.model.roi_head)
    rh.update(train_cfg=cfg.train_cfg.rcnn, test_cfg=registry._to_cfgdict(dict(hi.TEST_CFG)))
    torch.manual_seed(0)
    m = registry.build_head(rh)
    sd = {k: v.shape for k, v in m.state_dict().items() if k.startswith(('bbox_head.', 'mask_head.', 'semantic_head.'))}
    m.load_state_dict(hi.head_state(sd), strict=False)
    return m.cuda().eval()


def _cuda(x):
    return [f.cuda() for f in x]


def _count_semantic_calls(m):
    calls = []
    if m.with_semantic:
        fwd = m.semantic_head.forward
        m.semantic_head.forward = lambda feats: (calls.append(int(feats[0].shape[0])), fwd(feats))[1]
    return calls


def test_semantic_head_matches_the_reference(golden_dir):
    import htc_inputs as hi
    z = np.load(f'{golden_dir}/g22_htc.npz')
    m = _roi_head(golden_dir)
    x, _, _ = hi.simple_inputs()
    with torch.no_grad():
        sem = m.semantic_head(_cuda(x))
    assert tuple(sem.shape) == tuple(z['sem_feat_shape']) == (1, 256, 16, 20)
    got = sem.cpu().numpy().reshape(-1)[hi.sem_sample_index(sem.numel())]
    assert_grad_close(got, z['sem_feat'], 'semantic feature map', rel=1e-4)


def test_semantic_head_on_a_batch(golden_dir):
    """B images in one call (NB = B): each image's map has the bits of its own call."""
    from dynamask_amd import synth
    m = _roi_head(golden_dir)
    xb = [t.cuda() for t in synth.make_fpn(3, 96, 128, 256, seed=5)]
    with torch.no_grad():
        both = m.semantic_head(xb)
        for b in range(3):
            assert torch.equal(both[b:b + 1], m.semantic_head([t[b:b + 1].contiguous() for t in xb]))


@pytest.mark.parametrize('name,prefix', [('coco', ''), ('nosem', 'nosem_')])
def test_simple_test_matches_the_reference(golden_dir, name, prefix):
    import htc_inputs as hi
    from test_cascade_gpu import _assert_against_golden, _class_major, _flat
    z = np.load(f'{golden_dir}/g22_htc.npz')
    m = _roi_head(golden_dir, name)
    calls = _count_semantic_calls(m)
    x, props, metas = hi.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        bbox_res, segm_res = m.simple_test(x, [props], metas)
        assert calls == ([1] if name == 'coco' else []), 'one semantic feature per call'
        assert m._sem_cache is None
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        det, lab = _class_major(det, lab)
        probs = m.simple_test_mask_logits(x, det, lab)
        assert len(calls) == (3 if name == 'coco' else 0), 'a partial entry point computes the semantic feature itself'
    dets, labels, _ = _flat(bbox_res, segm_res)
    assert np.array_equal(dets, det.cpu().numpy())
    _assert_against_golden(z, prefix + 'simple', bbox_res, segm_res, probs[:, 0].cpu().numpy(), det[:, :4].contiguous())


@pytest.mark.parametrize('name,prefix', [('coco', ''), ('nosem', 'nosem_')])
def test_aug_test_matches_the_reference(golden_dir, name, prefix):
    import htc_inputs as hi
    from test_cascade_gpu import _assert_against_golden, _class_major
    z = np.load(f'{golden_dir}/g22_htc.npz')
    m = _roi_head(golden_dir, name)
    calls = _count_semantic_calls(m)
    xs, props, metas = hi.aug_inputs()
    xs, props = [_cuda(x) for x in xs], props.cuda()
    with torch.no_grad():
        bbox_res, segm_res = m.aug_test(xs, [props], metas, rescale=True)
        assert calls == ([1] * 4 if name == 'coco' else []), 'one semantic feature per view'
        det, lab = m.aug_test_bboxes(xs, metas, [props], m.test_cfg)
        det, lab = _class_major(det, lab)
        probs = m.aug_test_mask_probs(xs, metas, det, lab)
        bbox_nr, _ = m.aug_test(xs, [props], metas, rescale=False)
    for a, b in zip(bbox_nr, bbox_res):
        assert np.array_equal(a, b)
    _assert_against_golden(z, prefix + 'aug', bbox_res, segm_res, probs[:, 0].cpu().numpy(), det[:, :4].contiguous())


def test_fusion_and_information_flow_are_live(golden_dir):
    """A port that dropped the mask fusion or the information flow gives other probabilities (far beyond the tolerance)."""
    import htc_inputs as hi
    m = _roi_head(golden_dir)
    x, props, metas = hi.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        full = m.simple_test_mask_logits(x, det, lab)
        m.semantic_fusion = ('bbox',)
        no_mask_fusion = m.simple_test_mask_logits(x, det, lab)
        # Quirk Q17: aug_test fuses into the mask branch whatever semantic_fusion says
        m._aug_mask = True
        as_aug = m.simple_test_mask_logits(x, det, lab)
        m._aug_mask = False
        m.semantic_fusion = ('bbox', 'mask')
        stages = m._stage_mask_logits(x, torch.cat([det.new_zeros((det.shape[0], 1)), det[:, :4]], 1).contiguous())
    assert float((full - no_mask_fusion).abs().max()) > 1e-2
    assert torch.equal(as_aug, full)
    for i in range(3):
        for j in range(i + 1, 3):
            assert float((stages[i] - stages[j]).abs().max()) > 1e-2


def test_batch_equals_simple_test(golden_dir):
    """Three images of different shapes (one without proposals) in one call: per image, boxes and labels bit for bit and
    the bitmaps equal to simple_test's; the semantic head runs once, on the batch."""
    import htc_inputs as hi
    from dynamask_amd import synth
    m = _roi_head(golden_dir)
    shapes = [(128, 160), (96, 120), (112, 144)]
    H, W = 128, 160
    xb = [t.cuda() for t in synth.make_fpn(3, H, W, 256, seed=77)]
    props = [hi.proposals(seed=500 + b, h=h, w=w, n=40).cuda() for b, (h, w) in enumerate(shapes)]
    props[1] = props[1][:0]
    metas = [dict(ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False,
                  flip_direction=None) for h, w in shapes]
    calls = _count_semantic_calls(m)
    with torch.no_grad():
        batch = m.batch_simple_test(xb, props, metas)
        assert calls == [3], 'the semantic head runs once with NB = B'
        total = 0
        for b in range(3):
            x1 = [t[b:b + 1].contiguous() for t in xb]
            bbox_s, segm_s = m.simple_test(x1, [props[b]], [metas[b]])
            bbox_b, segm_b = batch[b]
            assert len(bbox_b) == len(bbox_s) == 80
            for c in range(80):
                assert np.array_equal(bbox_b[c], bbox_s[c]), f'image {b} class {c}'
                assert len(segm_b[c]) == len(segm_s[c])
                for p, q in zip(segm_b[c], segm_s[c]):
                    assert np.array_equal(p, q)
            total += sum(len(c) for c in bbox_b)
            if b == 1:
                assert sum(len(c) for c in bbox_b) == 0
    assert total > 0


def test_grouped_and_per_stage_paths_agree(golden_dir):
    """The stages' deconvs and logits convs as one grouped launch each against one launch per stage: bit for bit, with
    and without the K split of the conv chains."""
    import htc_inputs as hi
    from dynamask_amd import ops
    m = _roi_head(golden_dir)
    x, props, metas = hi.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
    was_g, was_s = ops.CASCADE_GROUPED[0], ops.CONV_SPLITK[0]
    out = {}
    try:
        for split in (False, True):
            for grouped in (True, False):
                ops.CONV_SPLITK[0], ops.CASCADE_GROUPED[0] = split, grouped
                assert m._grouped_ok() == grouped
                with torch.no_grad():
                    for k in (1, 16, int(det.shape[0])):
                        out[(split, grouped, k)] = m.simple_test_mask_logits(x, det[:k], lab[:k])
    finally:
        ops.CASCADE_GROUPED[0], ops.CONV_SPLITK[0] = was_g, was_s
    for k in (1, 16, int(det.shape[0])):
        for split in (False, True):
            assert torch.equal(out[(split, True, k)], out[(split, False, k)]), f'{k} detections, split {split}'
        # the K split re-associates the sums of twelve chained 3x3 convolutions: another rounding of the same products, held to
        # the project's bound for a different summation order (1e-4 of scale)
        assert_grad_close(out[(True, True, k)], out[(False, True, k)], f'{k} detections, split against unsplit', rel=1e-4)


def test_encode_equals_the_bitmaps(golden_dir):
    import htc_inputs as hi
    from oracle import ref_ops
    m = _roi_head(golden_dir)
    x, props, metas = hi.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        bbox_a, segm_a = m.simple_test(x, [props], metas)
        bbox_b, segm_b = m.simple_test(x, [props], metas, encode=True)
    n = 0
    for c in range(80):
        assert np.array_equal(bbox_a[c], bbox_b[c]) and len(segm_a[c]) == len(segm_b[c])
        for bm, rle in zip(segm_a[c], segm_b[c]):
            assert rle == ref_ops.rle_encode(np.asarray(bm).astype(np.uint8))
            n += 1
    assert n >= 8


def test_bf16x3_mode(golden_dir):
    """The existing routing (the 14 x 14 stage convs and deconvs on the bf16x3 kernels, the K26 kernels exact): within
    test_cascade_gpu's bound of the exact path."""
    import htc_inputs as hi
    from dynamask_amd import precision
    m = _roi_head(golden_dir)
    x, props, metas = hi.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        exact = m.simple_test_mask_logits(x, det, lab)
        precision.set_conv_precision('bf16x3')
        try:
            assert not m._grouped_ok()
            split = m.simple_test_mask_logits(x, det, lab)
        finally:
            precision.set_conv_precision('fp32')
    torch.testing.assert_close(split, exact, rtol=1e-4, atol=1e-5)


def test_zero_proposals_and_zero_detections(golden_dir):
    import htc_inputs as hi
    m = _roi_head(golden_dir)
    x, props, metas = hi.simple_inputs()
    x, props = _cuda(x), props.cuda()
    with torch.no_grad():
        bbox_res, segm_res = m.simple_test(x, [props[:0]], metas)
        assert [b.shape for b in bbox_res] == [(0, 5)] * 80 and segm_res == [[] for _ in range(80)]
        m.test_cfg.score_thr = 1.1                 # nothing passes
        bbox_res, segm_res = m.simple_test(x, [props], metas)
        assert [b.shape for b in bbox_res] == [(0, 5)] * 80 and segm_res == [[] for _ in range(80)]
        xs, props_a, metas_a = hi.aug_inputs()
        bbox_res, segm_res = m.aug_test([_cuda(v) for v in xs], [props_a.cuda()], metas_a)
        # htc_roi_head.py:497-500: the empty aug_test result has num_classes - 1 lists (Quirk Q19)
        assert [b.shape for b in bbox_res] == [(0, 5)] * 80 and segm_res == [[] for _ in range(79)]
    assert m._sem_cache is None
