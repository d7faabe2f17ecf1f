"""FCOS timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800, B = 1 and B = 4.

    python tools/fcos_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Every step runs in a child process of its own under its own time limit (the harness of tools/resnext_infer_bench.py); a step
that fails or runs out of time ends the run.  Reports, one JSON object per line:

  step ``kernel``: ``ops.group_norm`` (+ ReLU, in place) on the stacked towers [B, 512, H, W] with 64 groups at the five FCOS
      level sizes (100 x 168 down to 7 x 11: groups of 134400, 33600, 8400, 2184 and 616 floats), and at groups of 16385,
      20000 and 65536 floats, under both builds of dm_group_norm_fwd: the wide one (1024 threads, 16-byte loads; routed from
      ``ops.GN_WIDE_MIN_L`` floats) and the old one (``DM_GN_WIDE=0``, the parent commit's kernel unchanged; the knob is
      re-read through dm_reload_env_knobs between the two).  Below the switch length both rows time the old build.
      ``wide_faster``: the wide build's slowest round is faster than the old build's fastest round.
  step ``modules``: ``FCOSHead.forward_single`` per level and ``FCOSHead.forward`` in total (256 channels, GN, 80 classes)
      under both builds, the level's four stacked GroupNorm launches alone under both builds (the GN share), and
      ``get_bboxes`` on the head's outputs with its host waits.
  step ``detector``: ``FCOS.simple_test`` (fcos_r50_caffe_fpn_gn-head of tests/golden/g33_fcos_configs.json) beside
      ``MaskRCNN.simple_test`` (mask_rcnn_r50_fpn of g29_detector_configs.json) in the same run, seeded synthetic weights.

Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls; the variants compared are timed
alternately, ``--rounds`` times each, and the min .. max of the rounds' medians is reported beside the median.  There is no
pass / fail threshold."""
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import resnext_infer_bench as rb  # noqa: E402

STRIDES = (8, 16, 32, 64, 128)
F, G, NUM_CLASSES = 256, 32, 80


def level_sizes():
    h, w, out = rb.PAD_H // 8, rb.PAD_W // 8, []
    for _ in STRIDES:
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def set_gn_build(wide):
    from dynamask_amd import _lib
    if wide:
        os.environ.pop('DM_GN_WIDE', None)
    else:
        os.environ['DM_GN_WIDE'] = '0'
    _lib.lib().dm_reload_env_knobs()


def both_builds(fn, args):
    """{'wide' | 'old': dict(ms, ms_min, ms_max)} of ``fn`` under the two GroupNorm builds, timed in turn."""
    ts = {'wide': [], 'old': []}
    try:
        for _ in range(args.rounds):
            for build in ts:
                set_gn_build(build == 'wide')
                ts[build].append(rb.timed(fn, args.reps, args.warmup))
    finally:
        set_gn_build(True)
    return {k: dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4)) for k, v in ts.items()}


def _flat(t):
    return {f'{b}_{k}': v for b, r in t.items() for k, v in r.items()}


def step_kernel(args, report):
    import torch
    from dynamask_amd import ops
    shapes = [(f'stride {s}', 2 * F, 2 * G, h, w) for s, (h, w) in zip(STRIDES, level_sizes())]
    shapes += [(f'{L} floats', 64, 64, 1, L) for L in (16385, 20000, 65536)]
    for B in (1, 4):
        for name, C, groups, H, W in shapes:
            g = torch.Generator(device='cuda').manual_seed(B)
            x = torch.randn(B, C, H, W, device='cuda', generator=g)
            gamma, beta = torch.rand(C, device='cuda', generator=g) + 0.5, torch.randn(C, device='cuda', generator=g)
            L = C // groups * H * W
            set_gn_build(True)
            a = ops.group_norm(x, gamma, beta, groups, relu=True)
            set_gn_build(False)
            b = ops.group_norm(x, gamma, beta, groups, relu=True)
            diff = float((a - b).abs().max())
            y = x.clone()
            t = both_builds(lambda: ops.group_norm(y, gamma, beta, groups, relu=True, out=y), args)
            nbytes = 8 * x.numel()
            report(what='group_norm+relu', shape=name, B=B, x=[B, C, H, W], groups=groups, L=L, workgroups=B * groups,
                   routed_wide=L >= ops.GN_WIDE_MIN_L, rounds=args.rounds, **_flat(t), mbytes=round(nbytes / 1e6, 2),
                   wide_hbm_peak_share=round(nbytes / (t['wide']['ms'] * 1e-3) / rb.HBM_PEAK, 4),
                   old_over_wide=round(t['old']['ms'] / t['wide']['ms'], 2), wide_faster=t['wide']['ms_max'] < t['old']['ms_min'],
                   max_abs_diff_between_builds=diff)
            del x, y, a, b
            torch.cuda.empty_cache()


def _head():
    import torch
    from dynamask_amd import dense_heads
    h = dense_heads.FCOSHead(NUM_CLASSES, F, strides=list(STRIDES),
                             test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5),
                                           max_per_img=100))
    state = rb.seeded_state(h)
    state['conv_cls.bias'] = torch.full_like(state['conv_cls.bias'], -6.0)        # (a trained head: few scores above score_thr)
    state['conv_reg.bias'] = torch.full_like(state['conv_reg.bias'], 3.0)
    for k in state:
        if k.startswith('scales.'):
            state[k] = torch.ones(())
    h.load_state_dict(state, strict=True)
    return h.cuda().eval()


def step_modules(args, report):
    import numpy as np
    import torch
    import bench
    from dynamask_amd import ops
    h = _head()
    for B in (1, 4):
        g = torch.Generator(device='cuda').manual_seed(B)
        feats = [torch.randn(B, F, hh, ww, device='cuda', generator=g) for hh, ww in level_sizes()]
        for l, x in enumerate(feats):
            t = both_builds(lambda: h.forward_single(x, h.scales[l], h.strides[l]), args)
            y = torch.randn(B, 2 * F, x.shape[2], x.shape[3], device='cuda', generator=g)
            gamma, beta = torch.ones(2 * F, device='cuda'), torch.zeros(2 * F, device='cuda')

            def norms():
                for _ in range(h.stacked_convs):
                    ops.group_norm(y, gamma, beta, 2 * G, relu=True, out=y)
            tg = both_builds(norms, args)
            report(what='FCOSHead.forward_single', level=l, stride=STRIDES[l], B=B, map=list(x.shape[2:]), rounds=args.rounds, **_flat(t),
                   **{f'gn_{k}': v for k, v in _flat(tg).items()},
                   gn_share_wide=round(tg['wide']['ms'] / t['wide']['ms'], 3), gn_share_old=round(tg['old']['ms'] / t['old']['ms'], 3))
            del y
        t = both_builds(lambda: h(feats), args)
        outs = h(feats)
        metas = [dict(img_shape=(800, 1333, 3), scale_factor=np.full(4, 1.0664, dtype=np.float32)) for _ in range(B)]
        dets = h.get_bboxes(*outs, metas, rescale=True)
        tb = rb.alternately({'get_bboxes': lambda: h.get_bboxes(*outs, metas, rescale=True)}, args)
        report(what='FCOSHead.forward', B=B, image=[rb.PAD_H, rb.PAD_W], rounds=args.rounds, **_flat(t),
               host_waits=bench.count_host_syncs(lambda: h(feats)))
        report(what='FCOSHead.get_bboxes', B=B, rounds=args.rounds, **tb['get_bboxes'], detections=[int(d.shape[0]) for d, _ in dets],
               host_waits=bench.count_host_syncs(lambda: h.get_bboxes(*outs, metas, rescale=True)))
        del feats, outs
        torch.cuda.empty_cache()


def step_detector(args, report):
    import torch
    import bench
    from dynamask_amd import build_detector, detectors
    golden = os.path.join(ROOT, 'tests', 'golden')
    with open(os.path.join(golden, 'g33_fcos_configs.json')) as f:
        fcos = json.load(f)['r50_caffe_gn']
    with open(os.path.join(golden, 'g29_detector_configs.json')) as f:
        mask = json.load(f)['mask_rcnn']
    for name, cfg in (('fcos_r50_caffe_fpn_gn-head', fcos), ('mask_rcnn_r50_fpn', mask)):
        cfg = copy.deepcopy(cfg)
        single = cfg['model']['type'] == 'FCOS'
        if not single:
            cfg['test_cfg']['rcnn']['score_thr'] = 0.0
        p = detectors.parse_test_pipeline(cfg['test_pipeline'])
        det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
        state = rb.seeded_state(det)
        if single:
            state['bbox_head.conv_cls.bias'] = torch.full_like(state['bbox_head.conv_cls.bias'], -6.0)
            for k in state:
                if k.startswith('bbox_head.scales.'):
                    state[k] = torch.ones(())
        det.load_state_dict(state, strict=True)
        det = det.cuda().eval()
        for B in (1, 4):
            g = torch.Generator().manual_seed(B)
            imgs = [torch.randint(0, 256, (rb.SRC_H, rb.SRC_W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
            img, metas = detectors.preprocess(imgs, p['img_norm_cfg'], img_scale=p['img_scales'][0], size_divisor=p['size_divisor'])
            res = det.simple_test(img, metas, rescale=True)
            dets = [sum(len(c) for c in (r[0] if isinstance(r, tuple) else r)) for r in ([res] if B == 1 else res)]
            run = lambda: det.simple_test(img, metas, rescale=True)      # noqa: E731
            t = both_builds(run, args) if single else {'wide': rb.alternately({'t': run}, args)['t']}
            report(what=f"{cfg['model']['type']}.simple_test", config=name, B=B, img=list(img.shape), rounds=args.rounds, **_flat(t),
                   img_per_s=round(1000.0 * B / t['wide']['ms'], 2), detections=dets, host_waits=bench.count_host_syncs(run))
            del img, imgs
            torch.cuda.empty_cache()
        del det
        torch.cuda.empty_cache()


if __name__ == '__main__':
    rb.main({'kernel': step_kernel, 'modules': step_modules, 'detector': step_detector}, script=__file__)
