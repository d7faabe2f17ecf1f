"""Grid R-CNN inference timing on the MI355X: the launches of GridHead (csrc/grid_head.hip and the two 3x3 convolutions it
takes from csrc/conv_strided.hip / conv_igemm.hip) and the whole calls.  Each figure is the median of ``--reps`` calls
timed with HIP events after ``--warmup`` calls.

    python tools/grid_infer_bench.py [--reps 20] [--warmup 5] [--out FILE]

Reports (one JSON object per line):
  * at 16 / 50 / 100 RoIs, per launch: conv 0 (256 -> 576, 3x3 stride 2, 14 -> 7, one split), one of convs 1-7
    (576 -> 576 3x3 on 7 x 7), GroupNorm + ReLU (36 groups at 7 x 7; 9 groups at 14 x 14), one fusion order, deconv1
    (9 x 64 -> 64, 7 -> 14), deconv2 (9 x 64 -> 1, 14 -> 28) and the box kernel;
  * ``probe`` rows: the 7 x 7 conv with 512 / 640 output channels at 100 RoIs (full cout tiles) and with 576 at
    91 / 92 / 200 / 400 RoIs (both tile builds; more workgroups), to tell the tail tile from the launch size;
  * ``GridHead.forward`` and ``GridRoIHead.simple_test`` at 100 detections on a 1333 x 800 image (FPN maps of 1344 x 800).
TFLOP/s count 2 * MACs of the operator as the reference defines it (deconv: 4 taps per output); ``frac_peak`` is of the
157.3 TFLOP/s fp32 matrix peak, the yardstick of the 3x3 convolutions -- the VALU launches are listed with it only to put
them on one scale."""
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


def head_cfg(max_per_img=100):
    ext = lambda s: dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=s, sampling_ratio=0),  # noqa: E731
                         out_channels=256, featmap_strides=[4, 8, 16, 32])
    return dict(type='GridRoIHead', bbox_roi_extractor=ext(7),
                bbox_head=dict(type='Shared2FCBBoxHead', with_reg=False, in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                               num_classes=80, reg_class_agnostic=False),
                grid_roi_extractor=ext(14),
                grid_head=dict(type='GridHead', grid_points=9, num_convs=8, in_channels=256, point_feat_channels=64,
                               norm_cfg=dict(type='GN', num_groups=36)),
                test_cfg=dict(score_thr=0.03, nms=dict(type='nms', iou_threshold=0.3), max_per_img=max_per_img))


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

    def launch(what, rois, flop, fn):
        ms = timed(fn, args.reps, args.warmup)
        report(what=what, rois=rois, ms=round(ms, 4), tflops=round(flop / ms / 1e9, 2),
               frac_peak=round(flop / ms / 1e9 / (PEAK / 1e12), 4))

    with torch.no_grad():
        cfg = head_cfg()
        cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
        m = registry.build_head(cfg).cuda().eval()
        m.init_weights()
        h = m.grid_head
        dev = 'cuda'
        for n in (16, 50, 100):
            x14 = torch.randn(n, 256, 14, 14, device=dev)
            x7 = torch.randn(n, 576, 7, 7, device=dev)
            y7 = torch.empty_like(x7)
            x14b = torch.randn(n, 576, 14, 14, device=dev)
            c0, c1 = h.convs[0].conv, h.convs[1].conv
            launch('conv0 256->576 3x3 s2 14->7', n, 2 * 576 * 256 * 9 * n * 49,
                   lambda: ops.conv3x3_s2(x14, c0.packed(), c0.bias.detach(), 576, splits=1, out=y7))
            launch('conv1-7 576->576 3x3 7x7', n, 2 * 576 * 576 * 9 * n * 49,
                   lambda: ops.conv2d([x7], c1.packed(), c1.bias.detach(), 576, 3, out=y7))
            gn = h.convs[1].gn
            launch('group_norm+relu 36 groups 7x7', n, 8 * x7.numel(), lambda: gn.run_(y7, relu=True))
            launch('group_norm+relu 9 groups 14x14', n, 8 * x14b.numel(), lambda: h.norm1.run_(x14b, relu=True))
            tab = h._fusion_table('forder_trans')
            launch('fusion, one order', n, 2 * 24 * (64 * 64 + 64 * 25) * 49 * n, lambda: ops.grid_fusion(x7, x7, tab, 9, out=y7))
            x14b = torch.randn(n, 576, 14, 14, device=dev)      # fresh: the in-place GroupNorm above rewrote the first
            launch('deconv1 9x(64->64) 7->14', n, 2 * 9 * 64 * 64 * 4 * 196 * n, lambda: h.deconv1.run(x7))
            launch('deconv2 9x(64->1) 14->28', n, 2 * 9 * 64 * 4 * 784 * n, lambda: h.deconv2.run(x14b))
            heat = torch.randn(n, 9, 28, 28, device=dev)
            det = torch.rand(n, 5, device=dev) * 100
            launch('get_bboxes', n, 12 * heat.numel(), lambda: ops.grid_get_bboxes(heat, det, h.sub_regions))
        # where the 576 -> 576 conv loses time: the same launch with 512 / 640 output channels (4 / 5 full cout tiles of
        # 128 against 4.5), and around the RoI count at which the launcher leaves the 128 x 32 tiles for the 128 x 128
        # ones (conv_igemm.hip: up to 0.7 tiles of 128 x 128 per CU; 5 cout tiles x ceil(49 n / 128): n <= 91)
        for n, cout in ((100, 512), (100, 640), (91, 576), (92, 576), (200, 576), (400, 576)):
            x7 = torch.randn(n, 576, 7, 7, device=dev)
            y = torch.empty(n, cout, 7, 7, device=dev)
            wq = ops.pack_conv_weight(torch.randn(cout, 576, 3, 3, device=dev) * 0.02)
            b = torch.zeros(cout, device=dev)
            launch(f'probe 576->{cout} 3x3 7x7', n, 2 * cout * 576 * 9 * n * 49,
                   lambda: ops.conv2d([x7], wq, b, cout, 3, out=y))
        # the whole calls, 100 detections on a 1333 x 800 image
        x = tuple(torch.randn(1, 256, 800 // s, 1344 // s, device=dev) for s in (4, 8, 16, 32))
        g = torch.Generator(device=dev).manual_seed(1)
        xy = torch.rand(100, 2, device=dev, generator=g) * torch.tensor([1100.0, 600.0], device=dev)
        wh = torch.rand(100, 2, device=dev, generator=g) * 300 + 16
        boxes = torch.cat([xy, xy + wh], 1)
        rois = torch.cat([boxes.new_zeros(100, 1), boxes], 1).contiguous()
        feats = m.grid_roi_extractor(x, rois)
        ms = timed(lambda: h(feats), args.reps, args.warmup)
        flop = 100 * 2 * 49 * 9 * 576 * (256 + 7 * 576)
        report(what='GridHead.forward', rois=100, ms=round(ms, 4), conv_tflops=round(flop / ms / 1e9, 2),
               conv_frac_peak=round(flop / ms / 1e9 / (PEAK / 1e12), 4))
        # simple_test: 1000 proposals; a classifier bias puts every proposal in one class (1000 NMS candidates), of which
        # max_per_img = 100 are kept
        m.bbox_head.fc_cls.bias.data[3] = 10.0
        pxy = torch.rand(1000, 2, device=dev, generator=g) * torch.tensor([1100.0, 600.0], device=dev)
        pwh = torch.rand(1000, 2, device=dev, generator=g) * 300 + 16
        props = torch.cat([pxy, pxy + pwh], 1).contiguous()
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        kept = int(m.simple_test_grid(x, [props], metas)[0].shape[0])
        ms = timed(lambda: m.simple_test(x, [props], metas), args.reps, args.warmup)
        report(what='GridRoIHead.simple_test', proposals=1000, detections=kept, image='1333x800', ms=round(ms, 4))
        ms = timed(lambda: m.simple_test_bboxes(x, metas, [props], m.test_cfg), args.reps, args.warmup)
        report(what='  of which simple_test_bboxes', proposals=1000, detections=kept, ms=round(ms, 4))
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
