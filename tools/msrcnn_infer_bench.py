"""Mask Scoring R-CNN inference timing on the MI355X: MaskIoUHead's launches (csrc/conv_strided.hip, conv_igemm, fc) and
the whole ``simple_test_mask`` call.  Each figure is the median of ``--reps`` calls timed with HIP events after
``--warmup`` calls.

    python tools/msrcnn_infer_bench.py [--reps 20] [--warmup 5] [--out FILE]

Reports (one JSON object per line), at 16 and 100 detections on a 1333 x 800 image (FPN of 1344 x 800):
  * each IoU-head conv (the 257 -> 256 two-source conv, the two 256 -> 256 convs at 14^2, the stride-2 conv) with
    TFLOP/s and the fraction of the 157.3 TFLOP/s fp32 matrix peak;
  * the stride-2 kernel against the stand-in it replaces: the stride-1 conv_igemm launch at 14^2 followed by a
    ``[..., ::2, ::2]`` subsample (TFLOP/s of the stand-in counted on the useful stride-2 work);
  * the IoU-head input (dm_mask_iou_input), the three fully connected layers, the whole IoU head;
  * ``MaskScoringRoIHead.simple_test_mask`` (bitmaps and scores to the host) and the same call without the IoU branch
    (``StandardRoIHead.simple_test_mask`` on the same weights)."""
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
    ext = lambda s: dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=s, sampling_ratio=0),
                         out_channels=256, featmap_strides=[4, 8, 16, 32])
    return dict(type='MaskScoringRoIHead', bbox_roi_extractor=ext(7),
                bbox_head=dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                               num_classes=80),
                mask_roi_extractor=ext(14),
                mask_head=dict(type='FCNMaskHead', num_convs=4, in_channels=256, conv_out_channels=256, num_classes=80),
                mask_iou_head=dict(type='MaskIoUHead', num_convs=4, num_fcs=2, roi_feat_size=14, in_channels=256,
                                   conv_out_channels=256, fc_out_channels=1024, num_classes=80),
                test_cfg=dict(mask_thr_binary=0.5))


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

    def rate(fl, ms):
        return dict(tflops=round(fl / ms / 1e9, 2), frac_peak=round(fl / ms / 1e9 / (PEAK / 1e12), 3))

    with torch.no_grad():
        cfg = head_cfg()
        cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
        m = registry.build_head(cfg).cuda().eval()
        m.init_weights()
        cfg_plain = dict(cfg, type='StandardRoIHead')
        cfg_plain.pop('mask_iou_head')
        plain = registry.build_head(cfg_plain).cuda().eval()           # the same mask branch without the IoU head
        plain.load_state_dict(m.state_dict(), strict=False)
        x = tuple(torch.randn(1, 256, 800 // s, 1344 // s, device='cuda') for s in (4, 8, 16, 32))
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        h = m.mask_iou_head
        for n in (16, 100):
            det, lab = detections(n, n)
            ms = timed(lambda: m.simple_test_mask(x, metas, det, lab), args.reps, args.warmup)
            report(what='simple_test_mask', iou_branch=True, detections=n, image='1333x800', ms=round(ms, 4))
            ms = timed(lambda: plain.simple_test_mask(x, metas, det, lab), args.reps, args.warmup)
            report(what='simple_test_mask', iou_branch=False, detections=n, image='1333x800', ms=round(ms, 4))
            rois = torch.cat([det.new_zeros((n, 1)), det[:, :4]], 1).contiguous()
            res = m._mask_forward(x, rois)
            feats, pred = res['mask_feats'], res['mask_pred']
            ms = timed(lambda: h(feats, pred, lab), args.reps, args.warmup)
            report(what='MaskIoUHead.forward', rois=n, ms=round(ms, 4))
            ms = timed(lambda: ops.mask_iou_input(pred, lab), args.reps, args.warmup)
            report(what='mask_iou_input', rois=n, ms=round(ms, 4))
            pooled = ops.mask_iou_input(pred, lab)
            y = torch.randn(n, 256, 14, 14, device='cuda').relu_()
            with ops.splitk_scope():
                fl = 2.0 * n * 196 * 256 * 257 * 9
                ms = timed(lambda: h.convs[0].run([feats, pooled], relu=True), args.reps, args.warmup)
                report(what='conv 257->256 14^2 (two sources)', rois=n, ms=round(ms, 4), **rate(fl, ms))
                fl = 2.0 * n * 196 * 256 * 256 * 9
                for i in (1, 2):
                    ms = timed(lambda: h.convs[i].run(y, relu=True), args.reps, args.warmup)
                    report(what=f'conv {i} 256->256 14^2', rois=n, ms=round(ms, 4), **rate(fl, ms))
                last = h.convs[3]
                wq, b = last.packed(), last.bias.detach()
                fl = 2.0 * n * 49 * 256 * 256 * 9
                ms = timed(lambda: ops.conv3x3_s2(y, wq, b, 256, relu=True), args.reps, args.warmup)
                report(what='conv 3 stride 2 (conv3x3_s2, auto splits)', rois=n, ms=round(ms, 4), **rate(fl, ms))
                for s in (1, 2, 4, 8):
                    ms = timed(lambda: ops.conv3x3_s2(y, wq, b, 256, relu=True, splits=s), args.reps, args.warmup)
                    report(what=f'conv 3 stride 2 (conv3x3_s2, splits={s})', rois=n, ms=round(ms, 4), **rate(fl, ms))
                wq1 = last.packed([256], 'fp32')
                ms = timed(lambda: ops.conv2d([y], wq1, b, 256, 3, relu=True)[..., ::2, ::2].contiguous(), args.reps,
                           args.warmup)
                report(what='conv 3 stand-in (stride-1 conv_igemm 14^2 + [::2, ::2])', rois=n, ms=round(ms, 4),
                       **rate(fl, ms))
            z = torch.randn(n, 12544, device='cuda').relu_()
            z1 = torch.randn(n, 1024, device='cuda').relu_()
            fcs = [(h.fcs[0], z, True), (h.fcs[1], z1, True), (h.fc_mask_iou, z1, False)]
            for i, (fc, inp, relu) in enumerate(fcs):
                fl = 2.0 * n * fc.weight.shape[0] * fc.weight.shape[1]
                ms = timed(lambda: ops.fc(inp, fc.weight, fc.bias, relu=relu), args.reps, args.warmup)
                report(what=f'fc {i} {fc.weight.shape[1]}->{fc.weight.shape[0]}', rois=n, ms=round(ms, 4), **rate(fl, ms))
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
