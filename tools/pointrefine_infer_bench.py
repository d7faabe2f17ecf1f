"""PointRefine inference timing on the MI355X: PointRefineRoIHead's mask call and its launches (csrc/point_refine.hip,
section K24).  Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls.

    python tools/pointrefine_infer_bench.py [--reps 20] [--warmup 5] [--out FILE]

Reports (one JSON object per line), on a 1333 x 800 image (P2 of 1344 x 800), at 16 and 100 detections:
  * ``simple_test_mask`` (bitmaps to the host) and ``simple_test_mask_logits`` (the merged 112^2 logits, no paste);
  * the semantic branch: the four 3x3 convolutions on P2 and the three semantic_transform_in 1x1s as one grouped launch;
  * the two instance 3x3 convolutions on the 14 x 14 RoI features;
  * per SFM stage (S = 14 / 28 / 56, C = 256 / 128 / 64): the two 80-row logit 1x1s, the label rows, the selection
    (only where P < S^2), the point-feature gather, the point MLP + scatter fused and unfused (TFLOP/s of the MLP:
    2 * C * (C + 160) * (num_fcs + 1) per point), fuse_transform_out and the x2 upsample."""
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
    """configs/point_refine's roi_head (mask branch and bbox branch) with its test_cfg.rcnn."""
    return dict(type='PointRefineRoIHead',
                bbox_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                        out_channels=256, featmap_strides=[4, 8, 16, 32]),
                bbox_head=dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                               num_classes=80),
                mask_roi_extractor=dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=14, sampling_ratio=0),
                                        out_channels=256, featmap_strides=[4, 8, 16, 32]),
                mask_head=dict(type='PointRefineMaskHead', num_convs_instance=2, num_convs_semantic=4, num_fcs=2,
                               mask_use_sigmoid=True, stage_num_classes=[80, 80, 80, 80], stage_sup_size=[14, 28, 56, 112],
                               loss_cfg=dict(type='PointRefineCrossEntropyLoss')),
                test_cfg=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), num_points=784, max_per_img=100,
                              mask_thr_binary=0.5))


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

    def t(fn):
        return round(timed(fn, args.reps, args.warmup), 4)

    with torch.no_grad():
        cfg = head_cfg()
        cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
        m = registry.build_head(cfg).cuda().eval()
        h = m.mask_head
        for st in h.stages:                      # keep the refined features in a sane range
            for p in list(st.fcs.parameters()) + list(st.fc_logits.parameters()):
                p.mul_(0.3)
        x = tuple(torch.randn(1, 256, 800 // s, 1344 // s, device='cuda') for s in (4, 8, 16, 32))
        metas = [dict(ori_shape=(800, 1333, 3), img_shape=(800, 1333, 3), scale_factor=1.0)]
        report(what='semantic_branch', image='1333x800', ms=t(lambda: h.semantic_forward(x[0])))
        _, sems = h.semantic_forward(x[0])
        for n in (16, 100):
            det, lab = detections(n, n)
            report(what='simple_test_mask', detections=n, image='1333x800', ms=t(lambda: m.simple_test_mask(x, metas, det, lab)))
            report(what='simple_test_mask_logits', detections=n, image='1333x800',
                   ms=t(lambda: m.simple_test_mask_logits(x, det, lab)))
            rois = torch.cat([det.new_zeros((n, 1)), det[:, :4]], 1).contiguous()
            ins = m.mask_roi_extractor(x, rois)

            def inst_convs():
                f = ins
                for conv in h.instance_convs:
                    f = conv(f)
                return f
            report(what='instance_convs', rois=n, ms=t(inst_convs))
            feats = inst_convs()
            for st, sem in zip(h.stages, sems):
                C, S = st.channels, feats.shape[2]
                nc = st.num_classes
                coarse = torch.empty((n, 2 * nc, S, S), device='cuda')

                def logits():
                    st.instance_logits.run(feats, out=coarse, out_ch_offset=0)
                    st.detail_logits.run(feats, out=coarse, out_ch_offset=nc)
                report(what='logit_1x1s', rois=n, S=S, C=C, ms=t(logits))
                logits()
                wi, bi = st.instance_logits.weight.view(nc, C), st.instance_logits.bias
                wd, bd = st.detail_logits.weight.view(nc, C), st.detail_logits.bias
                lab_l = lab.long().contiguous()
                report(what='label_rows', rois=n, S=S, ms=t(lambda: ops.class_logits(feats, wi, bi, wd, bd, lab_l)))
                _, dp = ops.class_logits(feats, wi, bi, wd, bd, lab_l)
                P = min(S * S, 784)
                idx = None
                if P < S * S:
                    report(what='select', rois=n, S=S, points=P, ms=t(lambda: ops.point_topk_select(dp, P)))
                    idx = ops.point_topk_select(dp, P)
                report(what='gather', rois=n, S=S, points=P, ms=t(lambda: ops.point_feat_gather(sem, rois, coarse, idx, 0.25)))
                pts = ops.point_feat_gather(sem, rois, coarse, idx, 0.25)
                wq, bs = st.mlp_params()
                fl = 2 * C * (C + 2 * nc) * (st.num_fcs + 1) * n * P
                work = feats.clone()
                for form in ('fused', 'unfused'):
                    ms = t(lambda: ops.point_refine_mlp(pts, C, wq, bs, idx, work, form=form))
                    report(what='point_mlp', rois=n, S=S, C=C, points=P, form=form, ms=ms, tflops=round(fl / ms / 1e9, 2))
                report(what='fuse_transform_out', rois=n, S=S, ms=t(lambda: st.fuse_transform_out.run(feats, relu=True)))
                fused = st.fuse_transform_out.run(feats, relu=True)
                report(what='upsample2x', rois=n, S=S, ms=t(lambda: ops.upsample2x(fused, relu=True)))
                feats = ops.upsample2x(fused, relu=True)
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
