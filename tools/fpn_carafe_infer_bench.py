"""FPN_CARAFE timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800 (a multiple of 64,
configs/carafe's ``Pad``), B = 1 and B = 4.

    python tools/fpn_carafe_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

On the harness of tools/resnext_infer_bench.py: every step runs in a child process of its own under its own time limit; a
step that fails or runs out of time ends the run.  Reports, one JSON object per line:

  step ``kernel``: each of the neck's four top-down merges (13 x 21 -> 25 x 42 up to 100 x 168 -> 200 x 336, 256 channels,
      K = 5, one group) as the ONE launch the neck makes, ``ops.carafe_map(x, enc, addend=lat, out=lat)``
      (dm_carafe_map_fwd), beside the path the library had before it for the same step on the same inputs: ``ops.carafe``
      (dm_carafe_fwd: its generic kernel at these sizes, the full 2H x 2W map) and the slice and add in torch.  The
      algorithmic bytes 4 (x + enc + addend + out) over the time as a share of the 8 TB/s HBM peak and of the 6.29 TB/s a
      float4 copy measures.  ``faster``: the new launch's slowest round is faster than the old path's fastest round.
  step ``modules``: ``FPN_CARAFE.forward`` beside ``FPN.forward`` (the plain neck of configs/mask_rcnn) on the same stages.
  step ``detector``: ``MaskRCNN.simple_test`` of configs/carafe (tests/golden/g32_fpn_carafe_configs.json) beside the plain
      Mask R-CNN R-50 FPN detector (g29_detector_configs.json), seeded synthetic weights, ``score_thr`` 0.

Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls; the launches compared are
timed alternately, ``--rounds`` times each, and the min .. max of the rounds' medians is reported beside the median.  There
is no pass / fail threshold."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import resnext_infer_bench as rb  # noqa: E402

MAPS = [(rb.PAD_H // s, rb.PAD_W // s) for s in (4, 8, 16, 32)] + [(13, 21)]       # (the stride-2 extra level on 25 x 42)
C, K, GROUP = 256, 5, 1


def step_kernel(args, report):
    import torch
    from dynamask_amd import ops
    for B in (1, 4):
        for level in range(4, 0, -1):
            (H, W), (OH, OW) = MAPS[level], MAPS[level - 1]
            g = torch.Generator(device='cuda').manual_seed(level * 10 + B)
            x = torch.randn(B, C, H, W, device='cuda', generator=g)
            enc = torch.randn(B, K * K * GROUP * 4, H, W, device='cuda', generator=g)
            lat = torch.randn(B, C, OH, OW, device='cuda', generator=g)
            out = torch.empty_like(lat)
            assert ops.carafe_map_supported(x, K, GROUP, (OH, OW))

            def old():
                return lat + ops.carafe(x, enc, K, GROUP, 2)[:, :, :OH, :OW]

            def new():
                return ops.carafe_map(x, enc, K, GROUP, addend=lat, out=out)
            diff = float((old() - new()).abs().max())
            t = rb.alternately({'new': new, 'old': old, 'old_kernel_alone': lambda: ops.carafe(x, enc, K, GROUP, 2)}, args)
            nbytes = 4 * (x.numel() + enc.numel() + 2 * lat.numel())
            report(what='carafe_map', level=level, B=B, map=[H, W], out=[OH, OW], rounds=args.rounds, **t['new'],
                   mbytes=round(nbytes / 1e6, 2), hbm_peak_share=round(nbytes / (t['new']['ms'] * 1e-3) / rb.HBM_PEAK, 3),
                   copy_peak_share=round(nbytes / (t['new']['ms'] * 1e-3) / rb.COPY_PEAK, 3),
                   **{f'old_{k}': v for k, v in t['old'].items()}, **{f'old_kernel_{k}': v for k, v in t['old_kernel_alone'].items()},
                   old_over_new=round(t['old']['ms'] / t['new']['ms'], 2), faster=t['new']['ms_max'] < t['old']['ms_min'],
                   max_abs_diff_to_old=diff)
            del x, enc, lat, out
            torch.cuda.empty_cache()


def _stages(B, seed):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [torch.randn(B, c, h, w, device='cuda', generator=g) for c, (h, w) in zip((256, 512, 1024, 2048), MAPS[:4])]


def step_modules(args, report):
    import torch
    import bench
    from dynamask_amd import necks
    carafe = necks.FPN_CARAFE([256, 512, 1024, 2048], 256, 5, upsample_cfg=dict(type='carafe', up_kernel=5, up_group=1, encoder_kernel=3,
                                                                                 encoder_dilation=1, compressed_channels=64))
    plain = necks.FPN([256, 512, 1024, 2048], 256, 5)
    for m in (carafe, plain):
        m.load_state_dict(rb.seeded_state(m), strict=True)
    carafe, plain = carafe.cuda().eval(), plain.cuda().eval()
    for B in (1, 4):
        xs = _stages(B, B)
        outs = carafe(xs)
        assert [tuple(o.shape[2:]) for o in outs] == MAPS and all(bool(torch.isfinite(o).all()) for o in outs)
        t = rb.alternately({'carafe': lambda: carafe(xs), 'plain': lambda: plain(xs)}, args)
        report(what='FPN_CARAFE.forward', B=B, image=[rb.PAD_H, rb.PAD_W], rounds=args.rounds, **t['carafe'],
               **{f'plain_fpn_{k}': v for k, v in t['plain'].items()}, host_waits=bench.count_host_syncs(lambda: carafe(xs)))
        del xs, outs
        torch.cuda.empty_cache()


def step_detector(args, report):
    import torch
    import bench
    from dynamask_amd import build_detector, detectors
    golden = os.path.join(ROOT, 'tests', 'golden')
    with open(os.path.join(golden, 'g29_detector_configs.json')) as f:
        r50 = json.load(f)['mask_rcnn']
    with open(os.path.join(golden, 'g32_fpn_carafe_configs.json')) as f:
        car = json.load(f)['mask_rcnn_carafe']
    for name, cfg in (('mask_rcnn_carafe', car), ('mask_rcnn_r50_fpn', r50)):
        cfg = copy.deepcopy(cfg)
        cfg['test_cfg']['rcnn']['score_thr'] = 0.0
        p = detectors.parse_test_pipeline(cfg['test_pipeline'])
        det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
        det.load_state_dict(rb.seeded_state(det), strict=True)
        det = det.cuda().eval()
        for B in (1, 4):
            g = torch.Generator().manual_seed(B)
            imgs = [torch.randint(0, 256, (rb.SRC_H, rb.SRC_W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
            img, metas = detectors.preprocess(imgs, p['img_norm_cfg'], img_scale=p['img_scales'][0], size_divisor=p['size_divisor'])
            res = det.simple_test(img, metas, rescale=True)
            dets = [sum(len(c) for c in (r[0] if isinstance(r, tuple) else r)) for r in ([res] if B == 1 else res)]
            stages = det.backbone(img)
            t = rb.alternately({'simple_test': lambda: det.simple_test(img, metas, rescale=True), 'neck': lambda: det.neck(stages)}, args)
            report(what='MaskRCNN.simple_test', config=name, size_divisor=p['size_divisor'], B=B, img=list(img.shape), rounds=args.rounds,
                   **t['simple_test'], img_per_s=round(1000.0 * B / t['simple_test']['ms'], 2),
                   **{f'neck_{k}': v for k, v in t['neck'].items()}, detections=dets,
                   host_waits=bench.count_host_syncs(lambda: det.simple_test(img, metas, rescale=True)))
            del img, imgs, stages
            torch.cuda.empty_cache()
        del det
        torch.cuda.empty_cache()


if __name__ == '__main__':
    rb.main({'kernel': step_kernel, 'modules': step_modules, 'detector': step_detector}, script=__file__)
