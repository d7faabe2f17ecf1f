"""Double-Head R-CNN inference timing on the MI355X at the reference's test shape: 1000 proposals on a 1333 x 800 image (FPN
maps of 1344 x 800), 7 x 7 RoI features.  Each figure is the median of ``--reps`` calls timed with HIP events after
``--warmup`` calls.

    python tools/double_infer_bench.py [--reps 20] [--warmup 5] [--rois 1000] [--out FILE]

Reports (one JSON object per line):
  * each launch of the conv branch alone (the five shapes of BasicResBlock and Bottleneck on ``ops.conv2d``), with TFLOP/s
    of its algorithmic flops 2 * 49 * N * Cin * Cout * k^2 and ``frac_peak`` of the 157.3 TFLOP/s fp32 matrix peak;
  * the two RoIAligns (plain, and rescaled by ``reg_roi_scale_factor``), the global average pool and the fully connected
    layers;
  * the bbox branch (``DoubleConvFCBBoxHead.forward``, and its conv branch alone with the flops of all 14 launches), and
    ``DoubleHeadRoIHead.simple_test``.
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
    return dict(type='DoubleHeadRoIHead', reg_roi_scale_factor=1.3,
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                        out_channels=256, featmap_strides=[4, 8, 16, 32]),
                bbox_head=dict(type='DoubleConvFCBBoxHead', num_convs=4, num_fcs=2, in_channels=256, conv_out_channels=1024,
                               fc_out_channels=1024, roi_feat_size=7, num_classes=80, reg_class_agnostic=False),
                test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100))


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
        m.init_weights()
        h = m.bbox_head
        h.init_weights()
        # BatchNorm as after training: non-trivial statistics, bn3 scaled down so that the residual sums stay O(1)
        g = torch.Generator().manual_seed(1)
        for name, mod in h.named_modules():
            if hasattr(mod, 'running_var'):
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                if name.endswith('bn3'):
                    mod.weight.data.mul_(0.5)
        dev = 'cuda'
        rb, bt = h.res_block, h.conv_branch[0]
        mac = lambda cin, cout, k: 2 * 49 * n * cin * cout * k * k         # noqa: E731
        x256 = torch.randn(n, 256, 7, 7, device=dev)
        h256 = torch.randn(n, 256, 7, 7, device=dev)
        x1024 = torch.randn(n, 1024, 7, 7, device=dev)
        y256, y1024 = torch.empty_like(x256), torch.empty_like(x1024)
        (w1, b1), (w2, b2) = rb._f1.packed(), rb._f2.packed()
        (wa, ba), (wb, bb), (wc, bc) = (f.packed() for f in bt._f)
        each = {}
        each['res conv1'] = launch('res_block conv1 256->256 3x3 +relu', mac(256, 256, 3),
                                   lambda: ops.conv2d(x256, w1, b1, 256, 3, relu=True, out=y256))
        each['res merged'] = launch('res_block [conv2 | conv_identity] (256+256)->1024 1x1 +relu, two sources', mac(512, 1024, 1),
                                    lambda: ops.conv2d([h256, x256], w2, b2, 1024, 1, relu=True, out=y1024))
        each['b conv1'] = launch('bottleneck conv1 1024->256 1x1 +relu', mac(1024, 256, 1),
                                 lambda: ops.conv2d(x1024, wa, ba, 256, 1, relu=True, out=y256))
        each['b conv2'] = launch('bottleneck conv2 256->256 3x3 +relu', mac(256, 256, 3),
                                 lambda: ops.conv2d(h256, wb, bb, 256, 3, relu=True, out=y256))
        y1024.copy_(x1024)
        # (in place and accumulating: the destination saturates towards relu's fixed point over the repetitions; the time
        # of the launch does not depend on the values)
        each['b conv3'] = launch('bottleneck conv3 256->1024 1x1 relu|accumulate, in place', mac(256, 1024, 1),
                                 lambda: ops.conv2d(h256, wc, bc, 1024, 1, relu=True, out=y1024, accumulate=True))
        total = each['res conv1'] + each['res merged'] + 4 * (each['b conv1'] + each['b conv2'] + each['b conv3'])
        conv_flop = mac(256, 256, 3) + mac(512, 1024, 1) + 4 * (mac(1024, 256, 1) + mac(256, 256, 3) + mac(256, 1024, 1))
        report(what='the 14 conv launches, each timed alone, summed', rois=n, ms=round(total, 4),
               tflops=round(conv_flop / total / 1e9, 2), frac_peak=round(conv_flop / total / 1e9 / (PEAK / 1e12), 4))
        launch('global_avg_pool 1024 x 7 x 7', 0, lambda: ops.global_avg_pool(x1024))
        flat = x256.flatten(1)
        launch('fc_branch.0 12544->1024 +relu', 2 * n * 12544 * 1024, lambda: h.fc_branch[0].run(flat, relu=True))
        v1024 = torch.randn(n, 1024, device=dev)
        launch('fc_branch.1 1024->1024 +relu', 2 * n * 1024 * 1024, lambda: h.fc_branch[1].run(v1024, relu=True))
        launch('fc_cls 1024->81', 2 * n * 1024 * 81, lambda: h.fc_cls.run(v1024))
        launch('fc_reg 1024->320', 2 * n * 1024 * 320, lambda: h.fc_reg.run(v1024))
        # the whole calls
        x = tuple(torch.randn(1, 256, 800 // s, 1344 // s, device=dev) for s in (4, 8, 16, 32))
        gd = torch.Generator(device=dev).manual_seed(1)
        pxy = torch.rand(n, 2, device=dev, generator=gd) * torch.tensor([1100.0, 600.0], device=dev)
        pwh = torch.rand(n, 2, device=dev, generator=gd) * 300 + 16
        props = torch.cat([pxy, pxy + pwh], 1).contiguous()
        rois = torch.cat([props.new_zeros(n, 1), props], 1).contiguous()
        ext = m.bbox_roi_extractor
        launch('RoIAlign 7x7, plain', 0, lambda: ext(x, rois))
        launch('RoIAlign 7x7, rescaled by 1.3', 0, lambda: ext(x, rois, roi_scale_factor=1.3))
        x_cls, x_reg = ext(x, rois), ext(x, rois, roi_scale_factor=1.3)
        launch('conv branch of the head (14 convs + pool), in sequence', conv_flop, lambda: h.conv_features(x_reg))
        launch('DoubleConvFCBBoxHead.forward (the bbox branch)', conv_flop, lambda: h(x_cls, x_reg))
        launch('DoubleHeadRoIHead._bbox_forward', conv_flop, lambda: m._bbox_forward(x, rois))
        # simple_test: a classifier bias puts every proposal in one class (N NMS candidates), of which max_per_img are kept
        h.fc_cls.bias.data[3] = 10.0
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        kept = sum(len(c) for c in m.simple_test(x, [props], metas))
        ms = timed(lambda: m.simple_test(x, [props], metas), args.reps, args.warmup)
        report(what='DoubleHeadRoIHead.simple_test', proposals=n, detections=kept, image='1333x800', ms=round(ms, 4))
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
