"""PointRend inference timing on the MI355X: the subdivision kernels (csrc/point_refine.hip) and the whole
``simple_test_mask`` call.  Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls.

    python tools/pointrend_infer_bench.py [--reps 20] [--warmup 5] [--out FILE]

Reports (one JSON object per line):
  * ``PointRendRoIHead.simple_test_mask`` at 16 and 100 detections on a 1333 x 800 image (P2 of 1344 x 800), bitmaps to
    the host, and ``simple_test_mask_logits`` (the refined 224^2 logits, no paste);
  * per refined step (28^2, 56^2, 112^2, 224^2) at 16 / 100 RoIs: the x2 upsample, the point selection, the point
    gather, and the point MLP + scatter fused (one launch) and unfused (three 1x1 convolutions, the label-row logits,
    the scatter), with TFLOP/s of the MLP (2 * 256 * 336 * 3 per point; the logit row not counted) and the fraction of
    the 157.3 TFLOP/s fp32 matrix peak."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 157.3e12


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
    return dict(type='PointRendRoIHead',
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                        out_channels=256, featmap_strides=[4, 8, 16, 32]),
                bbox_head=dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                               num_classes=80),
                mask_roi_extractor=dict(type='GenericRoIExtractor', aggregation='concat',
                                        roi_layer=dict(type='SimpleRoIAlign', output_size=14), out_channels=256,
                                        featmap_strides=[4]),
                mask_head=dict(type='CoarseMaskHead', num_fcs=2, in_channels=256, conv_out_channels=256,
                               fc_out_channels=1024, num_classes=80),
                point_head=dict(type='MaskPointHead', num_fcs=3, in_channels=256, fc_channels=256, num_classes=80,
                                coarse_pred_each_layer=True),
                test_cfg=dict(mask_thr_binary=0.5, subdivision_steps=5, subdivision_num_points=784, scale_factor=2))


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
    from dynamask_amd import ops, registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    torch.manual_seed(0)
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    with torch.no_grad():
        cfg = head_cfg()
        cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
        m = registry.build_head(cfg).cuda().eval()
        for p in m.point_head.parameters():
            p.mul_(0.05)                       # keep the refined logits in a sane range
        x = tuple(torch.randn(1, 256, 800 // s, 1344 // s, device='cuda') for s in (4, 8, 16, 32))
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        ph = m.point_head
        wq = [f.conv.packed() for f in ph.fcs]
        bs = [f.conv.bias for f in ph.fcs]
        wl, bl = ph.fc_logits.weight.view(80, 336), ph.fc_logits.bias
        for n in (16, 100):
            det, lab = detections(n, n)
            ms = timed(lambda: m.simple_test_mask(x, metas, det, lab), args.reps, args.warmup)
            report(what='simple_test_mask', detections=n, image='1333x800', ms=round(ms, 4))
            ms = timed(lambda: m.simple_test_mask_logits(x, det, lab), args.reps, args.warmup)
            report(what='simple_test_mask_logits', detections=n, image='1333x800', ms=round(ms, 4))
            rois = torch.cat([det.new_zeros((n, 1)), det[:, :4]], 1).contiguous()
            coarse = m._mask_forward(x, rois)['mask_pred']
            for S in (28, 56, 112, 224):
                low = torch.randn(n, 1, S // 2, S // 2, device='cuda')
                ms = timed(lambda: ops.upsample2x(low), args.reps, args.warmup)
                report(what='upsample2x', rois=n, S=S, ms=round(ms, 4))
                refined = ops.upsample2x(low)
                P = min(784, S * S)
                ms = timed(lambda: ops.point_select(refined, P), args.reps, args.warmup)
                report(what='select', rois=n, S=S, points=P, ms=round(ms, 4))
                idx = ops.point_select(refined, P)
                ms = timed(lambda: ops.point_gather(x[0], rois, coarse, idx, S, S, 0.25), args.reps, args.warmup)
                report(what='gather', rois=n, S=S, points=P, ms=round(ms, 4))
                pts = ops.point_gather(x[0], rois, coarse, idx, S, S, 0.25)
                fl = 3 * 2 * 256 * 336 * n * P
                for fused in (True, False):
                    ms = timed(lambda: ops.point_mlp_scatter(pts, wq, bs, wl, bl, lab, idx, refined, fused=fused),
                               args.reps, args.warmup)
                    report(what='point_mlp', rois=n, S=S, points=P, fused=fused, ms=round(ms, 4),
                           tflops=round(fl / ms / 1e9, 2), frac_peak=round(fl / ms / 1e9 / (PEAK / 1e12), 3))
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
