"""The detector on the device: ``build_detector``'s object against the parts composed by hand (bit for bit: it adds no
arithmetic and no host wait), ``RPNHead.aug_test_rpn`` against CPU restatements of ``bbox_mapping_back`` and
``merge_aug_proposals``, ``aug_test``, ``detect`` and a whole-detector checkpoint.  Small images -- (128, 160) and
(96, 128) --, seeded weights with randomised BatchNorm statistics, ``test_cfg`` cut down to a few proposals and
``score_thr=0`` so that random weights still give detections.  The results are asked for on the original image
(``rescale=True``): the mask paste with ``rescale=False`` takes a scalar ``scale_factor`` only, as the reference's does,
and the pipeline writes the four-value array."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(128, 160), (96, 128)]
CONFIGS = ('dynamask', 'mask_rcnn', 'mask_c4')
SEED = 29


def _roi_state(shapes, seed):
    """Seeded RoI-head state: He-scaled weights, norm weights around 1, small biases and running means, running variances
    in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros(shape, dtype=torch.long)
        elif k.endswith('running_var'):
            out[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith('.weight') and len(shape) == 1:
            out[k] = (0.5 if '.bn3.' in k or '.downsample.1.' in k else 1.0) + 0.05 * torch.randn(shape, generator=g)
        elif len(shape) > 1:
            out[k] = torch.randn(shape, generator=g) * (2.0 / max(int(np.prod(shape[1:])), 1)) ** 0.5
        else:
            out[k] = 0.1 * torch.randn(shape, generator=g)
    return out


def _state(model, seed=SEED):
    """A seeded state dict of the whole detector, every section drawn by its own fixture module's rule."""
    import backbone_inputs as bi
    import fpn_inputs as fi
    import rpn_inputs as ri
    draw = dict(backbone=bi.head_state, neck=fi.head_state, rpn_head=ri.head_state, roi_head=_roi_state)
    own = model.state_dict()
    out = {}
    for part, fn in draw.items():
        shapes = {k[len(part) + 1:]: v.shape for k, v in own.items() if k.startswith(part + '.')}
        if shapes:
            out.update({f'{part}.{k}': v for k, v in fn(shapes, seed).items()})
    assert set(out) == set(own)
    return out


def _cfg(golden_dir, name):
    with open(os.path.join(golden_dir, 'g29_detector_configs.json')) as f:
        cfg = json.load(f)[name]
    cfg['test_cfg']['rpn'].update(nms_pre=64, nms_post=32, max_num=32)
    cfg['test_cfg']['rcnn'].update(score_thr=0.0, max_per_img=8)
    return cfg


@pytest.fixture(scope='module')
def built(golden_dir):
    """name -> (detector, (backbone, neck or None, rpn, roi) built one by one with the same weights, cfg), made on first use."""
    from dynamask_amd import build_detector, registry
    cache = {}

    def get(name):
        if name not in cache:
            cfg = _cfg(golden_dir, name)
            det = build_detector(copy.deepcopy(cfg['model']), test_cfg=copy.deepcopy(cfg['test_cfg']))
            state = _state(det)
            det.load_state_dict(state, strict=True)
            det = det.cuda().eval()
            m, tc = registry._to_cfgdict(cfg['model']), registry._to_cfgdict(cfg['test_cfg'])
            parts = {'backbone': registry.build_backbone(dict(m.backbone)),
                     'neck': registry.build_neck(dict(m.neck)) if 'neck' in m else None,
                     'rpn_head': registry.build_head(dict(m.rpn_head, train_cfg=None, test_cfg=tc.rpn)),
                     'roi_head': registry.build_head(dict(m.roi_head, train_cfg=None, test_cfg=tc.rcnn))}
            for part, mod in parts.items():
                if mod is not None:
                    mod.load_state_dict({k[len(part) + 1:]: v for k, v in state.items() if k.startswith(part + '.')}, strict=True)
                    parts[part] = mod.cuda().eval()
            cache[name] = (det, parts, cfg)
        return cache[name]
    return get


def _images(n=2, seed=SEED):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).cuda() for h, w in SHAPES[:n]]


def _inputs(cfg, n, **kw):
    from dynamask_amd import detectors
    return detectors.preprocess(_images(n), cfg['img_norm_cfg'], **kw)


def _feats(parts, img):
    x = parts['backbone'](img)
    return parts['neck'](x) if parts['neck'] is not None else x


def _same(a, b, path='result'):
    if isinstance(a, torch.Tensor):
        a, b = a.cpu().numpy(), (b.cpu().numpy() if isinstance(b, torch.Tensor) else b)
    if isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, path
        assert a.tobytes() == b.tobytes(), f'{path}: other bits'
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f'{path}[{i}]')
    elif isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), path
        for k in a:
            _same(a[k], b[k], f'{path}[{k!r}]')
    else:
        assert a == b, path


def _num_dets(result):
    bbox_results = result[0] if isinstance(result, tuple) else result
    assert all(r.ndim == 2 and r.shape[1] == 5 and np.isfinite(r).all() for r in bbox_results)
    return sum(len(r) for r in bbox_results)


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize('name', CONFIGS)
def test_simple_test_is_the_parts_composed(built, name):
    import bench
    det, parts, cfg = built(name)
    assert det.with_neck == (name != 'mask_c4') and det.with_mask and det.with_rpn
    img, metas = _inputs(cfg, 1)

    def hand():
        x = _feats(parts, img)
        return parts['roi_head'].simple_test(x, parts['rpn_head'].simple_test_rpn(x, metas), metas, rescale=True)

    with torch.no_grad():
        got, want = det.simple_test(img, metas, rescale=True), hand()
        assert _num_dets(got) > 0
        _same(got, want)
        # the detector adds no host wait
        assert bench.count_host_syncs(lambda: det.simple_test(img, metas, rescale=True)) == bench.count_host_syncs(hand)
        _same(det.forward([img], [metas], rescale=True), want)
        _same(det([img], [metas], return_loss=False, rescale=True, encode=True), det.simple_test(img, metas, rescale=True, encode=True))


@pytest.mark.parametrize('name', CONFIGS)
def test_two_images_are_batch_simple_test_composed(built, name):
    import bench
    det, parts, cfg = built(name)
    img, metas = _inputs(cfg, 2)
    assert tuple(img.shape) == (2, 3, 128, 160) and [m['img_shape'] for m in metas] == [(128, 160, 3), (96, 128, 3)]
    assert all(m['pad_shape'] == (128, 160, 3) for m in metas)

    def hand():
        x = _feats(parts, img)
        return parts['roi_head'].batch_simple_test(x, parts['rpn_head'].simple_test_rpn(x, metas), metas, rescale=True)

    with torch.no_grad():
        got, want = det.simple_test(img, metas, rescale=True), hand()
        assert isinstance(got, list) and len(got) == 2 and all(_num_dets(r) > 0 for r in got)
        _same(got, want)
        assert bench.count_host_syncs(lambda: det.simple_test(img, metas, rescale=True)) == bench.count_host_syncs(hand)


def test_given_proposals_bypass_the_rpn(built, monkeypatch):
    det, parts, cfg = built('mask_rcnn')
    img, metas = _inputs(cfg, 1)
    g = torch.Generator().manual_seed(SEED)
    xy = torch.rand(12, 2, generator=g) * torch.tensor([100.0, 70.0])
    wh = 16 + torch.rand(12, 2, generator=g) * 40
    props = [torch.cat([xy, xy + wh, torch.rand(12, 1, generator=g)], 1).cuda()]
    monkeypatch.setattr(det.rpn_head, 'simple_test_rpn', lambda *a, **k: pytest.fail('the RPN ran'))
    with torch.no_grad():
        got = det.simple_test(img, metas, proposals=props, rescale=True)
        want = parts['roi_head'].simple_test(_feats(parts, img), props, metas, rescale=True)
        assert _num_dets(got) > 0
        _same(got, want)
        _same(det.forward_test([img], [metas], proposals=[props], rescale=True), want)


# ------------------------------------------------------------------------------------------------ aug_test_rpn
def _views(cfg, n):
    """Two views of the first n images: (scale 1.0, no flip) and (scale 1.25 for the 128 x 160 image, horizontal flip)."""
    a = _inputs(cfg, n, img_scale=(160, 128))
    b = _inputs(cfg, n, img_scale=(200, 160), flip=True, flip_direction='horizontal')
    assert a[1][0]['img_shape'] == (128, 160, 3) and b[1][0]['img_shape'] == (160, 200, 3) and b[1][0]['flip']
    assert a[1][0]['scale_factor'].dtype == np.float32 and np.array_equal(b[1][0]['scale_factor'], np.float32([1.25] * 4))
    return [a[0], b[0]], [a[1], b[1]]


def _mapping_back_cpu(p, meta):
    """bbox_mapping_back (core/bbox/transforms.py:42-51) on the CPU: the flip against img_shape, then / scale_factor."""
    b = p[:, :4].clone()
    if meta['flip']:
        f = b.clone()
        if meta['flip_direction'] == 'vertical':
            f[:, 1], f[:, 3] = meta['img_shape'][0] - b[:, 3], meta['img_shape'][0] - b[:, 1]
        else:
            f[:, 0], f[:, 2] = meta['img_shape'][1] - b[:, 2], meta['img_shape'][1] - b[:, 0]
        b = f
    b = b.view(-1, 4) / b.new_tensor(meta['scale_factor'])
    return torch.cat([b, p[:, 4:5]], 1)


def _merge_cpu(cat, thr, max_num):
    """merge_aug_proposals' second half: greedy NMS in score order (IoU in float64), the max_num best.  Also the smallest
    distance of any pair's IoU from the threshold."""
    order = torch.sort(cat[:, 4], descending=True, stable=True)[1]
    d = cat[order].double()
    area = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
    w = (torch.min(d[:, None, 2], d[None, :, 2]) - torch.max(d[:, None, 0], d[None, :, 0])).clamp(min=0)
    h = (torch.min(d[:, None, 3], d[None, :, 3]) - torch.max(d[:, None, 1], d[None, :, 1])).clamp(min=0)
    iou = w * h / (area[:, None] + area[None, :] - w * h)
    off = ~torch.eye(len(d), dtype=torch.bool)
    # (two boxes of no area give 0 / 0: NaN is above no threshold, here as in the kernel, and is at no distance from it)
    gaps = (iou[off] - thr).abs()
    gaps = gaps[torch.isfinite(gaps)]
    margin = float(gaps.min()) if len(gaps) else 1.0
    alive, keep = torch.ones(len(d), dtype=torch.bool), []
    for i in range(len(d)):
        if alive[i]:
            keep.append(i)
            alive &= ~(iou[i] > thr)
    return cat[order][keep[:max_num]], margin


@pytest.mark.parametrize('n', [1, 2])
def test_aug_test_rpn_against_the_cpu_restatement(built, n):
    from dynamask_amd import ops
    det, parts, cfg = built('mask_rcnn')
    rpn = det.rpn_head
    imgs, metas = _views(cfg, n)
    with torch.no_grad():
        feats = det.extract_feats(imgs)
        per_view = [rpn.simple_test_rpn(x, m) for x, m in zip(feats, metas)]
        got = rpn.aug_test_rpn(feats, metas)
        flat = [(per_view[v][b], metas[v][b]) for b in range(n) for v in range(2)]
        mapped = ops.proposals_mapping_back([p for p, _ in flat], [m for _, m in flat]).cpu()
    assert len(got) == n
    want_rows = torch.cat([_mapping_back_cpu(p.cpu(), m) for p, m in flat])
    _same(mapped, want_rows, 'mapped-back proposals')
    r0 = 0
    for b in range(n):
        rows = sum(len(per_view[v][b]) for v in range(2))
        want, margin = _merge_cpu(want_rows[r0:r0 + rows], rpn.test_cfg['nms_thr'], rpn.test_cfg['max_num'])
        r0 += rows
        print(f'image {b}: {rows} proposals of 2 views, {len(want)} kept, IoU margin to nms_thr {margin:.3g}')
        assert margin > 1e-5, 'the seed puts a pair at the NMS threshold: pick another'
        assert 0 < len(want) <= rpn.test_cfg['max_num'] and rows > rpn.test_cfg['max_num']
        _same(got[b], want, f'image {b}')


OVERLAP_SEED = 3        # (every pair's IoU at least 2e-3 from nms_thr for one and for two images; checked on the CPU, asserted below)


def _overlapping_proposals(metas, n, seed=OVERLAP_SEED):
    """Seeded proposals per view and image that overlap across and within the views (the random weights' own hardly do):
    24 boxes of the original image, each twice with a jitter of a few pixels, mapped into the view (bbox_mapping: times
    scale_factor, then the flip), distinct scores.  CPU tensors, [view][image] -> [48, 5]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for v, view in enumerate(metas):
        per_image = []
        for b in range(n):
            h, w = view[b]['ori_shape'][:2]
            xy = torch.rand(24, 2, generator=g) * torch.tensor([w * 0.6, h * 0.6])
            wh = 12 + torch.rand(24, 2, generator=g) * torch.tensor([w * 0.35, h * 0.35])
            base = torch.cat([xy, xy + wh], 1).repeat(2, 1) + torch.randn(48, 4, generator=g) * 2.5
            boxes = base * base.new_tensor(view[b]['scale_factor'])
            if view[b]['flip']:
                f = boxes.clone()
                f[:, 0], f[:, 2] = view[b]['img_shape'][1] - boxes[:, 2], view[b]['img_shape'][1] - boxes[:, 0]
                boxes = f
            score = torch.rand(48, generator=g).sort(descending=True)[0]
            per_image.append(torch.cat([boxes, score[:, None]], 1).contiguous())
        out.append(per_image)
    return out


@pytest.mark.parametrize('n', [1, 2])
def test_aug_test_rpn_merge_suppresses_overlapping_proposals(built, monkeypatch, n):
    """The merge alone, on proposals that do overlap: ``simple_test_rpn`` is replaced by seeded proposals, so the mapping
    back, the suppression across the views and the ``max_num`` cut are all at work."""
    det, parts, cfg = built('mask_rcnn')
    rpn = det.rpn_head
    imgs, metas = _views(cfg, n)
    props = _overlapping_proposals(metas, n)
    calls = []
    monkeypatch.setattr(rpn, 'simple_test_rpn', lambda x, m: (calls.append(m), [p.cuda() for p in props[len(calls) - 1]])[1])
    with torch.no_grad():
        got = rpn.aug_test_rpn([None, None], metas)
    assert len(calls) == 2 and len(got) == n
    for b in range(n):
        cat = torch.cat([_mapping_back_cpu(props[v][b], metas[v][b]) for v in range(2)])
        want, margin = _merge_cpu(cat, rpn.test_cfg['nms_thr'], rpn.test_cfg['max_num'])
        full, _ = _merge_cpu(cat, rpn.test_cfg['nms_thr'], len(cat))
        print(f'image {b}: {len(cat)} proposals, {len(full)} survive the NMS, {len(want)} kept, IoU margin {margin:.3g}')
        assert margin > 1e-5, 'the seed puts a pair at the NMS threshold: pick another'
        assert rpn.test_cfg['max_num'] < len(full) < len(cat) - 20, 'the NMS and the max_num cut must both bite'
        _same(got[b], want, f'image {b}')


def test_aug_test_rpn_host_waits_do_not_grow_with_the_batch(built):
    import bench
    det, parts, cfg = built('mask_rcnn')
    counts = []
    for n in (1, 2):
        imgs, metas = _views(cfg, n)
        with torch.no_grad():
            feats = det.extract_feats(imgs)
            det.rpn_head.aug_test_rpn(feats, metas)
            counts.append(bench.count_host_syncs(lambda: det.rpn_head.aug_test_rpn(feats, metas)))
    assert counts[0] == counts[1] and counts[0] <= 2 + 1, counts          # each view's one wait, one for the merge


@pytest.mark.parametrize('name', ['mask_rcnn', 'dynamask'])
def test_aug_test_is_the_roi_heads_on_the_merged_proposals(built, name):
    det, parts, cfg = built(name)
    imgs, metas = _views(cfg, 1)
    with torch.no_grad():
        got = det.aug_test(imgs, metas, rescale=True)
        feats = [_feats(parts, i) for i in imgs]
        props = parts['rpn_head'].aug_test_rpn(feats, metas)
        want = parts['roi_head'].aug_test(feats, props, metas, rescale=True)
        assert _num_dets(got) > 0
        _same(got, want)
        _same(det.forward(imgs, metas, rescale=True), want)


# ------------------------------------------------------------------------------------------------ detect
def _pipeline(cfg, img_scale, flip=False):
    p = copy.deepcopy(cfg['test_pipeline'])
    aug = [t for t in p if t['type'] == 'MultiScaleFlipAug'][0]
    aug.update(img_scale=img_scale, flip=flip)
    return p


def test_detect_is_preprocess_then_simple_test(built):
    from dynamask_amd import detectors
    det, parts, cfg = built('mask_rcnn')
    images = _images(2)
    kw = dict(img_scale=(200, 160), size_divisor=32)
    with torch.no_grad():
        for n in (1, 2):
            got = det.detect(images[:n], _pipeline(cfg, [200, 160]))
            want = det.simple_test(*detectors.preprocess(images[:n], cfg['img_norm_cfg'], **kw), rescale=True)
            assert (_num_dets(got) if n == 1 else min(_num_dets(r) for r in got)) > 0
            _same(got, want)
        # host numpy arrays are copied up; a config holding the pipeline is read as the pipeline is
        _same(det.detect([i.cpu().numpy() for i in images[:1]], dict(test_pipeline=_pipeline(cfg, (200, 160)))),
              det.detect(images[:1], _pipeline(cfg, [200, 160])))


def test_detect_with_two_scales_is_aug_test(built):
    from dynamask_amd import detectors
    det, parts, cfg = built('mask_rcnn')
    images = _images(1)
    with torch.no_grad():
        got = det.detect(images, _pipeline(cfg, [[160, 128], [200, 160]]))
        views = [detectors.preprocess(images, cfg['img_norm_cfg'], img_scale=s) for s in [(160, 128), (200, 160)]]
        want = det.aug_test([v[0] for v in views], [v[1] for v in views], rescale=True)
        assert _num_dets(got) > 0
        _same(got, want)
        flipped = det.detect(images, _pipeline(cfg, [200, 160], flip=True))
        views = [detectors.preprocess(images, cfg['img_norm_cfg'], img_scale=(200, 160), flip=f) for f in (False, True)]
        _same(flipped, det.aug_test([v[0] for v in views], [v[1] for v in views], rescale=True))


# ------------------------------------------------------------------------------------------------ whole checkpoint
def test_one_load_checkpoint_call_reproduces_the_composed_run(built, tmp_path):
    from dynamask_amd import build_detector, detectors
    det, parts, cfg = built('mask_rcnn')
    path = str(tmp_path / 'whole.pth')
    torch.save({'state_dict': {'module.' + k: v.cpu() for k, v in det.state_dict().items()},
                'meta': {'CLASSES': ('a', 'b'), 'epoch': 12}}, path)
    fresh = build_detector(copy.deepcopy(cfg['model']), test_cfg=copy.deepcopy(cfg['test_cfg']))
    meta, missing, unexpected = detectors.load_checkpoint(fresh, path, strict=True)
    assert meta == {'CLASSES': ('a', 'b'), 'epoch': 12} and missing == [] and unexpected == []
    fresh = fresh.cuda().eval()
    img, metas = _inputs(cfg, 1)
    with torch.no_grad():
        x = _feats(parts, img)
        want = parts['roi_head'].simple_test(x, parts['rpn_head'].simple_test_rpn(x, metas), metas, rescale=True)
        got = fresh.simple_test(img, metas, rescale=True)
    assert _num_dets(got) > 0
    _same(got, want)
