"""Hybrid Task Cascade inference timing on the MI355X.  Each figure is the median of ``--reps`` calls timed with HIP events
after ``--warmup`` calls, with the min .. max of the calls beside it; a fused form and its baseline are alternated
``--rounds`` times and compared by their round medians.

    python tools/htc_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Reports (one JSON object per line) on a 1333 x 800 image (FPN of 1344 x 800, P2..P6), the config of
configs/htc/htc_r50_fpn_1x_coco.py with seeded weights, 1000 proposals and 16 / 50 / 100 detections:
  * the semantic head (FusedSemanticHead) and its parts: the resizes, the lateral convs with the fused add, the four 3x3
    convs + embedding;
  * the semantic fusion into RoI features, ops.roi_align_add_ against the sequence composed from launches the library
    had before (ops.roi_align + torch pooling + add): the box form (1000 RoIs, 14 -> 7) and the mask form;
  * ``conv_res`` with the fused add (ops.conv1x1_post_add) against ops.conv2d + add;
  * the three-stage bbox cascade with the fusion, the mask branch (information flow; grouped against per-stage tails) and
    ``simple_test`` end to end."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    """(median, min, max) in ms."""
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
    return statistics.median(ts), min(ts), max(ts)


def head_cfg():
    ext = lambda s, strides: dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=s, sampling_ratio=0),
                                  out_channels=256, featmap_strides=strides)
    bbox = lambda stds: dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=80,
                             bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0.] * 4, target_stds=stds),
                             reg_class_agnostic=True)
    mask = lambda res: dict(type='HTCMaskHead', with_conv_res=res, num_convs=4, in_channels=256, conv_out_channels=256,
                            num_classes=80)
    return dict(type='HybridTaskCascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25], interleaved=True,
                mask_info_flow=True, bbox_roi_extractor=ext(7, [4, 8, 16, 32]),
                bbox_head=[bbox([0.1, 0.1, 0.2, 0.2]), bbox([0.05, 0.05, 0.1, 0.1]), bbox([0.033, 0.033, 0.067, 0.067])],
                mask_roi_extractor=ext(14, [4, 8, 16, 32]), mask_head=[mask(False), mask(True), mask(True)],
                semantic_roi_extractor=ext(14, [8]),
                semantic_head=dict(type='FusedSemanticHead', num_ins=5, fusion_level=1, num_convs=4, in_channels=256,
                                   conv_out_channels=256, num_classes=183),
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
    ap.add_argument('--rounds', type=int, default=5, help='alternations of a fused form and its baseline')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import ops, registry, roi_head, mask_heads, losses, roi_extractors, bbox_heads, synth  # noqa: F401
    torch.manual_seed(0)
    rows = []

    def report(what, t=None, **r):
        r = dict(what=what, **r)
        if t is not None:
            r.update(ms=round(t[0], 4), min_ms=round(t[1], 4), max_ms=round(t[2], 4))
        rows.append(r)
        print(json.dumps(r), flush=True)

    def ab(what, fused, composed, **r):
        """A fused form against its composed baseline, alternated ``--rounds`` times in this call: each round gives one
        median per form; the spread is the range of a form's round medians, and the fused form is "faster beyond the
        spread" when its slowest round beats the baseline's fastest."""
        tf, tc = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused, args.reps, args.warmup)[0])
            tc.append(timed(composed, args.reps, args.warmup)[0])
        mf, mc = statistics.median(tf), statistics.median(tc)
        report(what, fused_ms=round(mf, 4), fused_rounds_min_max=[round(min(tf), 4), round(max(tf), 4)],
               composed_ms=round(mc, 4), composed_rounds_min_max=[round(min(tc), 4), round(max(tc), 4)],
               ratio=round(mf / mc, 3), faster_beyond_spread=bool(max(tf) < min(tc)), **r)

    T = lambda fn: timed(fn, args.reps, args.warmup)
    m = registry.build_head(registry._to_cfgdict(head_cfg()))
    m.init_weights()
    m = m.cuda().eval()
    x = [t.cuda() for t in synth.make_fpn(1, 800, 1344, 256, seed=5)]
    assert len(x) == 5
    meta = dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0, flip=False, flip_direction=None)
    sh = m.semantic_head
    was = ops.CASCADE_GROUPED[0]
    try:
        with torch.no_grad():
            # ---- the semantic head and its parts
            sem = sh(x)
            size = tuple(sem.shape[-2:])
            report('FusedSemanticHead (5 levels -> %d x %d x 256)' % size, T(lambda: sh(x)))
            others = [i for i in range(5) if i != sh.fusion_level]
            report('  4 resizes to the fusion level (dm_resize_bilinear_fwd)',
                   T(lambda: [ops.resize_bilinear(x[i], size) for i in others]))
            rs = [ops.resize_bilinear(x[i], size) for i in others]
            acc = sh.lateral_convs[sh.fusion_level](x[sh.fusion_level])

            def laterals(fused):
                for i, r in zip(others, rs):
                    c = sh.lateral_convs[i].conv
                    if fused:
                        ops.conv1x1_post_add(r, c.packed([256]), c.bias.detach(), 256, acc, relu=True, out=acc)
                    else:
                        acc.add_(ops.conv2d(r, c.packed([256]), c.bias.detach(), 256, 1, relu=True))
            ab('  4 lateral 1x1 convs summed into the map: post-activation addend against conv2d + add',
               lambda: laterals(True), lambda: laterals(False))

            def tail():
                y = acc
                for conv in sh.convs:
                    y = conv(y)
                return sh.conv_embedding(y)
            report('  4 x conv3x3 (ops.conv3x3_dil) + embedding', T(tail))

            # ---- the fusion into RoI features
            lay = m.semantic_roi_extractor.roi_layers[0]
            props = synth.make_rois(1, 1000, 800, 1333, seed=9).cuda()
            bf = torch.randn(1000, 256, 7, 7, device='cuda')
            ab('semantic fusion, box form (14 -> 7): roi_align_add_ against roi_align + adaptive_avg_pool2d + add',
               lambda: ops.roi_align_add_(bf, sem, props, 14, lay.spatial_scale),
               lambda: bf.add_(F.adaptive_avg_pool2d(ops.roi_align([sem], props, 14, [lay.spatial_scale], 0), (7, 7))),
               rois=1000)
            for n in (16, 50, 100):
                det, lab = detections(n, 11 + n)
                rois = torch.cat([det.new_zeros((n, 1)), det[:, :4]], 1).contiguous()
                mf = torch.randn(n, 256, 14, 14, device='cuda')
                ab('semantic fusion, mask form (14 x 14): roi_align_add_ against roi_align + add',
                   lambda: ops.roi_align_add_(mf, sem, rois, 14, lay.spatial_scale),
                   lambda: mf.add_(ops.roi_align([sem], rois, 14, [lay.spatial_scale], 0)), rois=n)
                c = m.mask_head[1].conv_res.conv
                last = torch.randn(n, 256, 14, 14, device='cuda')
                ab('conv_res + add: conv1x1_post_add against conv2d + add',
                   lambda: ops.conv1x1_post_add(last, c.packed([256]), c.bias.detach(), 256, mf, relu=True),
                   lambda: ops.conv2d(last, c.packed([256]), c.bias.detach(), 256, 1, relu=True) + mf, rois=n)

            # ---- the branches and the head
            report('bbox cascade with semantic fusion (3 stages; semantic head not included)',
                   T(lambda: _bbox_only(m, x, props, meta, sem)), proposals=1000)
            for n in (16, 50, 100):
                det, lab = detections(n, 11 + n)
                rois = torch.cat([det.new_zeros((n, 1)), det[:, :4]], 1).contiguous()
                t = {}
                for grouped in (True, False):
                    ops.CASCADE_GROUPED[0] = grouped
                    t[grouped] = timed(lambda: _mask_only(m, x, rois, sem), args.reps, args.warmup)
                report('mask branch (RoIAlign, fusion, 3 x HTCMaskHead with information flow; semantic head not included)',
                       detections=n, grouped_ms=round(t[True][0], 4), grouped_min_max=[round(t[True][1], 4), round(t[True][2], 4)],
                       per_stage_ms=round(t[False][0], 4), per_stage_min_max=[round(t[False][1], 4), round(t[False][2], 4)],
                       ratio=round(t[True][0] / t[False][0], 3))
                ops.CASCADE_GROUPED[0] = was
                report('simple_test_mask (semantic head + mask branch + paste, bitmaps to the host)',
                       T(lambda: m.simple_test_mask(x, [meta], det, lab)), detections=n)
            report('simple_test end to end (semantic head once, 1000 proposals, the detections NMS keeps)',
                   T(lambda: m.simple_test(x, [props[:, 1:].contiguous()], [meta])), proposals=1000)
    finally:
        ops.CASCADE_GROUPED[0] = was
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


def _with_sem(m, x, sem, fn):
    """``fn()`` with the semantic feature of ``x`` already in the head's cache (times a branch without the semantic head)."""
    m._sem_cache, m._sem_depth = {id(x): (x, sem)}, 1
    try:
        return fn()
    finally:
        m._sem_cache, m._sem_depth = None, 0


def _bbox_only(m, x, props, meta, sem):
    return _with_sem(m, x, sem, lambda: m._bbox_test_preds(x, props, [meta]))


def _mask_only(m, x, rois, sem):
    return _with_sem(m, x, sem, lambda: m._stage_mask_logits(x, rois))


if __name__ == '__main__':
    main()
