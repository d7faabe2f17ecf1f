"""Mask R-CNN C4 inference timing on the MI355X at the reference's test shape: 1000 proposals and 100 detections on a
1333 x 800 image (one stride-16 map of 1024 x 50 x 84), 14 x 14 RoIAlign, ResNet layer4 as the shared head.  Each figure is the
median of ``--reps`` calls timed with HIP events after ``--warmup`` calls.

    python tools/c4_infer_bench.py [--reps 20] [--warmup 5] [--rois 1000] [--out FILE]

Reports (one JSON object per line):
  * the extraction: strided (``bin_step=2``, [N, 1024, 7, 7]) against the dense 14 x 14 extraction followed by the
    ``[:, :, ::2, ::2]`` copy, in the same run, with the bytes each writes;
  * each of the five convolution shapes of layer4 alone on ``ops.conv2d``, with TFLOP/s of its algorithmic flops
    2 * 49 * N * Cin * Cout * k^2 and ``frac_peak`` of the 157.3 TFLOP/s fp32 matrix peak, and the nine launches summed;
  * the shared head in sequence, the bbox branch (``_bbox_forward``: extraction, shared head, pool, two FCs), the mask branch
    (``_mask_forward`` of the kept detections) and ``StandardRoIHead.simple_test``.
There is no pass / fail threshold."""
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
    norm_cfg = dict(type='BN', requires_grad=False)
    return dict(type='StandardRoIHead',
                shared_head=dict(type='ResLayer', depth=50, stage=3, stride=2, dilation=1, style='caffe', norm_cfg=norm_cfg,
                                 norm_eval=True),
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0),
                                        out_channels=1024, featmap_strides=[16]),
                bbox_head=dict(type='BBoxHead', with_avg_pool=True, roi_feat_size=7, in_channels=2048, num_classes=80,
                               reg_class_agnostic=False),
                mask_roi_extractor=None,
                mask_head=dict(type='FCNMaskHead', num_convs=0, in_channels=2048, conv_out_channels=256, num_classes=80),
                test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rois', type=int, default=1000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import ops, registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads  # noqa: F401
    torch.manual_seed(0)
    rows = []
    n = args.rois

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def launch(what, flop, fn, **more):
        ms = timed(fn, args.reps, args.warmup)
        r = dict(what=what, rois=n, ms=round(ms, 4), **more)
        if flop:
            r.update(tflops=round(flop / ms / 1e9, 2), frac_peak=round(flop / ms / 1e9 / (PEAK / 1e12), 4))
        report(**r)
        return ms

    with torch.no_grad():
        cfg = head_cfg()
        cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
        m = registry.build_head(cfg).cuda().eval()
        m.shared_head.init_weights()
        m.bbox_head.init_weights()
        m.mask_head.init_weights()
        # BatchNorm as after training: non-trivial statistics, bn3 / downsample scaled down so that the residual sums stay O(1)
        g = torch.Generator().manual_seed(1)
        for name, mod in m.shared_head.named_modules():
            if hasattr(mod, 'running_var'):
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                if name.endswith('bn3') or name.endswith('downsample.1'):
                    mod.weight.data.mul_(0.5)
        dev = 'cuda'
        x = (torch.randn(1, 1024, 50, 84, device=dev),)
        gd = torch.Generator(device=dev).manual_seed(1)
        pxy = torch.rand(n, 2, device=dev, generator=gd) * torch.tensor([1100.0, 600.0], device=dev)
        pwh = torch.rand(n, 2, device=dev, generator=gd) * 300 + 16
        props = torch.cat([pxy, pxy + pwh], 1).contiguous()
        rois = torch.cat([props.new_zeros(n, 1), props], 1).contiguous()
        ext = m.bbox_roi_extractor

        # ---- the extraction
        mb = lambda p: round(n * 1024 * p * p * 4 / 1e6, 1)         # noqa: E731
        strided = launch('RoIAlign 14x14, bin_step=2 (the 7 x 7 kept bins)', 0, lambda: ext(x, rois, bin_step=2), written_MB=mb(7))
        dense = launch('RoIAlign 14x14, dense', 0, lambda: ext(x, rois), written_MB=mb(14))
        full = ext(x, rois)
        sl = launch('the [:, :, ::2, ::2] copy of the dense features', 0, lambda: full[:, :, ::2, ::2].contiguous())
        both = launch('dense + slice, in sequence', 0, lambda: ext(x, rois)[:, :, ::2, ::2].contiguous())
        report(what='strided extraction against dense + slice', rois=n, strided_ms=round(strided, 4), dense_ms=round(dense, 4),
               slice_ms=round(sl, 4), dense_plus_slice_ms=round(both, 4), saved_ms=round(both - strided, 4))
        del full

        # ---- the nine convolutions
        b0, b1 = m.shared_head.layer4[0], m.shared_head.layer4[1]
        mac = lambda cin, cout, k: 2 * 49 * n * cin * cout * k * k         # noqa: E731
        x1024 = torch.randn(n, 1024, 7, 7, device=dev)
        x2048 = torch.randn(n, 2048, 7, 7, device=dev)
        h512 = torch.randn(n, 512, 7, 7, device=dev)
        y512, y2048 = torch.empty_like(h512), torch.empty_like(x2048)
        (wa, ba), (wb, bb), (wc, bc) = (f.packed() for f in b0._f)
        (wd, bd), (we, be), (wf, bf) = (f.packed() for f in b1._f)
        each = {}
        each['b0 conv1'] = launch('block 0 conv1 1024->512 1x1 +relu', mac(1024, 512, 1),
                                  lambda: ops.conv2d(x1024, wa, ba, 512, 1, relu=True, out=y512))
        each['conv2'] = launch('conv2 512->512 3x3 +relu', mac(512, 512, 3),
                               lambda: ops.conv2d(h512, wb, bb, 512, 3, relu=True, out=y512))
        each['b0 merged'] = launch('block 0 [conv3 | downsample] (512+1024)->2048 1x1 +relu, two sources', mac(1536, 2048, 1),
                                   lambda: ops.conv2d([h512, x1024], wc, bc, 2048, 1, relu=True, out=y2048))
        each['conv1'] = launch('conv1 2048->512 1x1 +relu', mac(2048, 512, 1),
                               lambda: ops.conv2d(x2048, wd, bd, 512, 1, relu=True, out=y512))
        y2048.copy_(x2048)
        # (in place and accumulating: the time of the launch does not depend on the values)
        each['conv3'] = launch('conv3 512->2048 1x1 relu|accumulate, in place', mac(512, 2048, 1),
                               lambda: ops.conv2d(h512, wf, bf, 2048, 1, relu=True, out=y2048, accumulate=True))
        total = each['b0 conv1'] + each['b0 merged'] + 3 * each['conv2'] + 2 * (each['conv1'] + each['conv3'])
        conv_flop = mac(1024, 512, 1) + mac(1536, 2048, 1) + 3 * mac(512, 512, 3) + 2 * (mac(2048, 512, 1) + mac(512, 2048, 1))
        report(what='the 9 conv launches, each timed alone, summed', rois=n, ms=round(total, 4), gflop=round(conv_flop / 1e9, 1),
               tflops=round(conv_flop / total / 1e9, 2), frac_peak=round(conv_flop / total / 1e9 / (PEAK / 1e12), 4))
        del x2048, y2048, h512, y512, x1024

        # ---- the branches
        sub = ext(x, rois, bin_step=2)
        launch('ResLayer.forward_sampled (9 convs), in sequence', conv_flop, lambda: m.shared_head.forward_sampled(sub))
        feats = m.shared_head.forward_sampled(sub)
        launch('BBoxHead.forward (pool + fc_cls + fc_reg)', 0, lambda: m.bbox_head(feats))
        del feats, sub
        launch('StandardRoIHead._bbox_forward (the bbox branch)', conv_flop, lambda: m._bbox_forward(x, rois))
        m.STRIDED_EXTRACTION = False
        launch('StandardRoIHead._bbox_forward, dense extraction + ResLayer.forward', conv_flop, lambda: m._bbox_forward(x, rois))
        del m.STRIDED_EXTRACTION
        # simple_test: a classifier bias puts every proposal in one class (N NMS candidates), of which max_per_img are kept
        m.bbox_head.fc_cls.bias.data[3] = 10.0
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        det, lab = m.simple_test_bboxes(x, metas, [props], m.test_cfg)
        kept = int(det.shape[0])
        drois = torch.cat([det.new_zeros(kept, 1), det[:, :4]], 1).contiguous()
        launch('StandardRoIHead._mask_forward (the mask branch)', conv_flop * kept / n, lambda: m._mask_forward(x, drois),
               detections=kept)
        ms = timed(lambda: m.simple_test_mask(x, metas, det, lab), args.reps, args.warmup)
        report(what='StandardRoIHead.simple_test_mask (mask branch + paste + copy to the host)', detections=kept, ms=round(ms, 4))
        ms = timed(lambda: m.simple_test(x, [props], metas), args.reps, args.warmup)
        report(what='StandardRoIHead.simple_test', proposals=n, detections=kept, image='1333x800', ms=round(ms, 4))
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
