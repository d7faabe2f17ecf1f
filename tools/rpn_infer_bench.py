"""RPN inference timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800 -- FPN form:
five maps of 256 channels from 200 x 336 down to 13 x 21, A = 3, nms_pre 1000, for B = 1 and B = 4; C4 form: one map of
1024 x 50 x 84, A = 15, nms_pre 6000, B = 1.  Each figure is the median of ``--reps`` calls timed with HIP events after
``--warmup`` calls; the fused and the composed post-processing are timed alternately, ``--rounds`` times each, and the
spread of the rounds' medians is reported beside them.

    python tools/rpn_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Reports (one JSON object per line): ``RPNHead.forward``; each launch of the fused post-processing alone (``rpn_select``,
``rpn_decode``, ``nms_segmented``, ``rpn_merge``); ``get_bboxes`` fused and composed (``DM_RPN_FUSED=0``: ``ops.sigmoid``,
``torch.sort``, gathers, ``grid_anchors``, ``ops.bbox_decode``, ``ops.nms_segmented``, concatenate + sort -- launches that
existed before the RPN kernels) with min / median / max over the rounds, after checking that both give the same bits; and
the whole ``simple_test_rpn``.  There is no pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAD_H, PAD_W = 800, 1344
IMG_SHAPE = (800, 1333, 3)
FORMS = {
    'fpn': dict(in_channels=256, feat_channels=256,
                anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                test_cfg=dict(nms_across_levels=False, nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7, min_bbox_size=0)),
    'c4': dict(in_channels=1024, feat_channels=1024,
               anchor_generator=dict(type='AnchorGenerator', scales=[2, 4, 8, 16, 32], ratios=[0.5, 1.0, 2.0], strides=[16]),
               test_cfg=dict(nms_across_levels=False, nms_pre=6000, nms_post=1000, max_num=1000, nms_thr=0.7, min_bbox_size=0)),
}


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


def build(form):
    from dynamask_amd import dense_heads, registry  # noqa: F401
    cfg = dict(FORMS[form])
    cfg['test_cfg'] = registry._to_cfgdict(cfg['test_cfg'])
    m = registry.build_head(dict(type='RPNHead', bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.],
                                                                target_stds=[1., 1., 1., 1.]),
                                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                                 loss_bbox=dict(type='L1Loss', loss_weight=1.0), train_cfg=None, **cfg))
    g = torch.Generator().manual_seed(1)
    for c in (m.rpn_conv, m.rpn_cls, m.rpn_reg):       # He-scaled: the logits span several units, the scores are distinct
        fan_in = c.weight[0].numel()
        c.weight.data.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
        c.bias.data.copy_(torch.randn(c.bias.shape, generator=g) * 0.1)
    return m.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import dense_heads, ops
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    with torch.no_grad():
        for form, B in (('fpn', 1), ('fpn', 4), ('c4', 1)):
            m = build(form)
            gen = m.anchor_generator
            L = gen.num_levels
            tag = dict(form=form, B=B, image='1333x800')
            x = [torch.randn(B, m.in_channels, -(-PAD_H // s[1]), -(-PAD_W // s[0]), device='cuda',
                             generator=torch.Generator(device='cuda').manual_seed(l)) for l, s in enumerate(gen.strides)]
            metas = [dict(img_shape=IMG_SHAPE, ori_shape=IMG_SHAPE, pad_shape=(PAD_H, PAD_W, 3), scale_factor=1.0)] * B
            report(what='RPNHead.forward', ms=round(timed(lambda: m(x), args.reps, args.warmup), 4), **tag)
            cls, reg = m(x)
            cfg = m.test_cfg
            # ---- the launches of the fused post-processing, each alone
            table, base_rows = gen.base_anchor_table('cuda')
            img_tab = ops.image_shape_table(metas, 'cuda')
            segs = ops.RPNSegments([cls[l][b] for b in range(B) for l in range(L)], cfg.nms_pre,
                                   [reg[l][b] for b in range(B) for l in range(L)],
                                   strides=[gen.strides[l] for _ in range(B) for l in range(L)],
                                   base_rows=[base_rows[l] for _ in range(B) for l in range(L)],
                                   images=[b for b in range(B) for _ in range(L)], num_levels=L)
            info = dict(candidates=segs.total_candidates, rows=segs.total_rows, **tag)
            report(what='rpn_select (6 kernels)', ms=round(timed(lambda: ops.rpn_select(segs), args.reps, args.warmup), 4), **info)
            idx, score = ops.rpn_select(segs)
            report(what='rpn_decode', **info,
                   ms=round(timed(lambda: ops.rpn_decode(segs, idx, table, img_tab), args.reps, args.warmup), 4))
            boxes = ops.rpn_decode(segs, idx, table, img_tab)
            report(what='nms_segmented', **info,
                   ms=round(timed(lambda: ops.nms_segmented(boxes, segs.rows, cfg.nms_thr), args.reps, args.warmup), 4))
            keep, kept = ops.nms_segmented(boxes, segs.rows, cfg.nms_thr)
            report(what='rpn_merge', kept=int(kept.sum()), **info,
                   ms=round(timed(lambda: ops.rpn_merge(segs, keep, kept, boxes, score, cfg.nms_post), args.reps, args.warmup), 4))
            # ---- get_bboxes: fused against composed, alternately
            def run(fused):
                dense_heads.RPN_FUSED[0] = fused
                try:
                    return m.get_bboxes(cls, reg, metas)
                finally:
                    dense_heads.RPN_FUSED[0] = True
            a, c = run(True), run(False)
            same = all(torch.equal(p, q) for p, q in zip(a, c))
            t = {True: [], False: []}
            for _ in range(args.rounds):
                for fused in (True, False):
                    t[fused].append(timed(lambda: run(fused), args.reps, args.warmup))
            for fused, name in ((True, 'get_bboxes, fused'), (False, 'get_bboxes, composed (DM_RPN_FUSED=0)')):
                report(what=name, proposals=[len(p) for p in a], same_bits=same, ms=round(statistics.median(t[fused]), 4),
                       ms_min=round(min(t[fused]), 4), ms_max=round(max(t[fused]), 4), rounds=args.rounds, **tag)
            report(what='RPNHead.simple_test_rpn', **tag,
                   ms=round(timed(lambda: m.simple_test_rpn(x, metas), args.reps, args.warmup), 4))
            del m, x, cls, reg, segs
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
