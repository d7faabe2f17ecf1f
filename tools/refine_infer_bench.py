"""RefineMask inference timing on the MI355X: the dilated / any-width 3x3 kernels (csrc/conv_dilated.hip) and the whole
``simple_test_mask`` call.  Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls.

    python tools/refine_infer_bench.py [--reps 20] [--warmup 5] [--out FILE]

Reports (one JSON object per line, and a table):
  * the semantic 3x3 (256 -> 256, d = 1, + ReLU) on the whole stride-4 map at 336 x 200 (1333 x 800) and 512 x 256;
  * the MultiBranchFusion branch sum (three 3x3 at d = 1, 3, 5) at 16 / 50 / 100 RoIs per stage shape (256 @ 14^2,
    128 @ 28^2, 64 @ 56^2), fused (one launch) and unfused (three launches);
  * ``RefineRoIHead.simple_test_mask`` at 100 detections on a 1333 x 800 image (FPN maps of 1344 x 800), bitmaps to the host.
TFLOP/s count 2 * Cout * Cin * 9 * pixels per 3x3; the fraction is of the 157.3 TFLOP/s fp32 matrix peak."""
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
    return dict(type='RefineRoIHead',
                bbox_roi_extractor=None, bbox_head=None,
                mask_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0),
                                        out_channels=256, featmap_strides=[4, 8, 16, 32]),
                mask_head=dict(type='RefineMaskHead', num_convs_instance=2, num_convs_semantic=4, dilations=[1, 3, 5],
                               semantic_out_stride=4, mask_use_sigmoid=True, stage_num_classes=[80, 80, 80, 80],
                               stage_sup_size=[14, 28, 56, 112], upsample_cfg=dict(type='bilinear', scale_factor=2)),
                test_cfg=dict(mask_thr_binary=0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import ops, registry, roi_head, mask_heads, losses, roi_extractors  # noqa: F401
    torch.manual_seed(0)
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    with torch.no_grad():
        for H, W in ((200, 336), (256, 512)):
            x = torch.randn(1, 256, H, W, device='cuda')
            w = ops.pack_conv_weight(torch.randn(256, 256, 3, 3, device='cuda') * 0.03)
            b = torch.zeros(256, device='cuda')
            ms = timed(lambda: ops.conv3x3_dil(x, w, b, 256, 1, relu=True), args.reps, args.warmup)
            fl = 2 * 256 * 256 * 9 * H * W
            report(what='semantic_conv3x3', shape=f'1x256x{H}x{W}', ms=round(ms, 4), tflops=round(fl / ms / 1e9, 2),
                   frac_peak=round(fl / ms / 1e9 / (PEAK / 1e12), 3))
        for n in (16, 50, 100):
            for C, S in ((256, 14), (128, 28), (64, 56)):
                x = torch.randn(n, C, S, S, device='cuda')
                ws = [ops.pack_conv_weight(torch.randn(C, C, 3, 3, device='cuda') * 0.03) for _ in range(3)]
                bs = [torch.zeros(C, device='cuda') for _ in range(3)]
                out = torch.empty(n, C, S, S, device='cuda')
                fl = 3 * 2 * C * C * 9 * n * S * S
                for fused in (True, False):
                    ms = timed(lambda: ops.conv3x3_multidil(x, ws, bs, C, (1, 3, 5), out=out, fused=fused), args.reps, args.warmup)
                    report(what='multibranch', rois=n, shape=f'{C}@{S}', fused=fused, ms=round(ms, 4),
                           tflops=round(fl / ms / 1e9, 2), frac_peak=round(fl / ms / 1e9 / (PEAK / 1e12), 3))
        cfg = head_cfg()
        cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
        m = registry.build_head(cfg).cuda().eval()
        x = tuple(torch.randn(1, 256, 800 // s, 1344 // s, device='cuda') for s in (4, 8, 16, 32))
        g = torch.Generator(device='cuda').manual_seed(1)
        xy = torch.rand(100, 2, device='cuda', generator=g) * torch.tensor([1100.0, 600.0], device='cuda')
        wh = torch.rand(100, 2, device='cuda', generator=g) * 300 + 16
        det = torch.cat([xy, xy + wh, torch.rand(100, 1, device='cuda', generator=g)], 1)
        lab = torch.randint(0, 80, (100,), device='cuda', generator=g)
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        ms = timed(lambda: m.simple_test_mask(x, metas, det, lab), args.reps, args.warmup)
        report(what='simple_test_mask', detections=100, image='1333x800', ms=round(ms, 4))
        ms = timed(lambda: m.simple_test_mask_logits(x, det, lab), args.reps, args.warmup)
        report(what='simple_test_mask_logits', detections=100, image='1333x800', ms=round(ms, 4))
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
