"""Cascade Mask R-CNN inference timing on the MI355X.  Each figure is the median of ``--reps`` calls timed with HIP events
after ``--warmup`` calls.

    python tools/cascade_infer_bench.py [--reps 20] [--warmup 5] [--out FILE]

Reports (one JSON object per line) on a 1333 x 800 image (FPN of 1344 x 800), the config of
configs/cascade_rcnn/cascade_mask_rcnn_r50_fpn_1x_coco.py with seeded weights:
  * the mask ensemble (every stage's FCNMaskHead on the shared 14 x 14 features, then the merge) at 16 / 50 / 100
    detections, stage-grouped launches against the three stage chains one after the other (ops.CASCADE_GROUPED);
  * the three-stage bbox cascade (RoIAlign 7 x 7, the FC heads, dm_cascade_refine) at 1000 proposals;
  * ``simple_test_mask`` (bitmaps to the host) at 16 / 50 / 100 detections in both forms."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def head_cfg():
    ext = lambda s: dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=s, sampling_ratio=0),
                         out_channels=256, featmap_strides=[4, 8, 16, 32])
    bbox = lambda stds: dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=80,
                             bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0.] * 4, target_stds=stds),
                             reg_class_agnostic=True)
    return dict(type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25], bbox_roi_extractor=ext(7),
                bbox_head=[bbox([0.1, 0.1, 0.2, 0.2]), bbox([0.05, 0.05, 0.1, 0.1]), bbox([0.033, 0.033, 0.067, 0.067])],
                mask_roi_extractor=ext(14),
                mask_head=dict(type='FCNMaskHead', num_convs=4, in_channels=256, conv_out_channels=256, num_classes=80),
                test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=0.5))


def detections(n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    xy = torch.rand(n, 2, device='cuda', generator=g) * torch.tensor([1100.0, 600.0], device='cuda')
    wh = torch.rand(n, 2, device='cuda', generator=g) * 300 + 16
    det = torch.cat([xy, xy + wh, torch.rand(n, 1, device='cuda', generator=g)], 1)
    return det, torch.randint(0, 80, (n,), device='cuda', generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import ops, registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads, synth  # noqa: F401
    torch.manual_seed(0)
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    m = registry.build_head(registry._to_cfgdict(head_cfg()))
    m.init_weights()
    m = m.cuda().eval()
    x = [t.cuda() for t in synth.make_fpn(1, 800, 1344, 256, seed=5)]
    meta = dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0, flip=False, flip_direction=None)
    was = ops.CASCADE_GROUPED[0]
    try:
        with torch.no_grad():
            for n in (16, 50, 100):
                det, lab = detections(n, 11 + n)
                rois = torch.cat([det.new_zeros((n, 1)), det[:, :4]], 1).contiguous()
                t = {}
                for grouped in (True, False):
                    ops.CASCADE_GROUPED[0] = grouped
                    t[grouped] = timed(lambda: m._stage_mask_logits(x, rois), args.reps, args.warmup)
                report(what='mask ensemble (3 x FCNMaskHead, shared RoIAlign)', detections=n, grouped_ms=round(t[True], 4),
                       per_stage_ms=round(t[False], 4), ratio=round(t[True] / t[False], 3))
                for grouped in (True, False):
                    ops.CASCADE_GROUPED[0] = grouped
                    t[grouped] = timed(lambda: m.simple_test_mask(x, [meta], det, lab), args.reps, args.warmup)
                report(what='simple_test_mask (1333 x 800, bitmaps to the host)', detections=n,
                       grouped_ms=round(t[True], 4), per_stage_ms=round(t[False], 4), ratio=round(t[True] / t[False], 3))
            ops.CASCADE_GROUPED[0] = was
            props = synth.make_rois(1, 1000, 800, 1333, seed=9).cuda()
            tab = ops.image_shape_table([meta], props.device)
            report(what='bbox cascade (3 stages, RoIAlign 7x7 + FC heads + dm_cascade_refine)', proposals=1000,
                   ms=round(timed(lambda: m._bbox_test_preds(x, props, [meta]), args.reps, args.warmup), 4))
            cls = torch.randn(1000, 81, device='cuda')
            pred = torch.randn(1000, 4, device='cuda')
            acc = torch.empty_like(cls)
            report(what='dm_cascade_refine alone', proposals=1000,
                   ms=round(timed(lambda: ops.cascade_refine(props, cls, pred, 80, tab, acc, first=True), args.reps,
                                  args.warmup), 4))
    finally:
        ops.CASCADE_GROUPED[0] = was
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
