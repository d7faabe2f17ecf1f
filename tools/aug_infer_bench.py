#!/usr/bin/env python
"""Test-time augmentation (DynaMaskRoIHead.aug_test) against the same result assembled from the
public one-view pieces.

One 1333x800 image, 64 proposals, score_thr 0 and max_per_img 100 (the call keeps exactly 100 detections), for
V = 1 (no flip), 2 (flip) and 4 (scales 1.0 and 0.75 x flip; FPN maps P2..P6 of each view's padded size).  One JSON
line per V with, eager and graphed (enable_inference_graphs):
  call_ms_*      the whole call with encode=True (boxes merged over the views, NMS, masks merged over the views, paste +
                 RLE to COCO dicts on the host): ``aug`` = aug_test, ``composed`` = a per-view loop of the one-view
                 pieces (``_bbox_forward`` + ``get_bboxes``, ``simple_test_mask_logits``) with the mapping and the
                 merges as torch operations, then multiclass_nms and ops.paste_rle;
  probs_ms_*     the mask merge alone from the detections (aug_test_mask_probs / the composed per-view loop);
and, per call, the C-ABI launches and host waits counted as tools/batch_infer_bench.py counts them.  Times: median of
individually event-timed calls (bench.time_kernel_median), host work included.

    python tools/aug_infer_bench.py [--views 1 2 4] [--iters 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench  # noqa: E402
from batch_infer_bench import build_head, count_launches, count_syncs  # noqa: E402

IMG_H, IMG_W = 800, 1333
N_PROPS = 64
VIEW_SETS = {1: [(1.0, None)], 2: [(1.0, None), (1.0, 'horizontal')],
             4: [(1.0, None), (1.0, 'horizontal'), (0.75, None), (0.75, 'horizontal')]}


def _flip(b, h, w, d):
    f = b.clone()
    if d == 'horizontal':
        f[:, 0::4] = w - b[:, 2::4]
        f[:, 2::4] = w - b[:, 0::4]
    elif d == 'vertical':
        f[:, 1::4] = h - b[:, 3::4]
        f[:, 3::4] = h - b[:, 1::4]
    return f


def _mapping(boxes, meta):
    b = boxes[:, :4] * boxes.new_tensor(meta['scale_factor'])
    return _flip(b, meta['img_shape'][0], meta['img_shape'][1], meta['flip_direction'] if meta['flip'] else None)


def composed_bboxes(m, xs, props, metas):
    from dynamask_amd.postprocess import multiclass_nms
    from dynamask_amd.roi_head import bbox2roi
    bl, sl = [], []
    for x, (meta,) in zip(xs, metas):
        rois = bbox2roi([_mapping(props, meta)]).contiguous()
        res = m._bbox_forward(x, rois)
        b, s = m.bbox_head.get_bboxes(rois, res['cls_score'], res['bbox_pred'], meta['img_shape'], meta['scale_factor'],
                                      rescale=False, cfg=None)
        h, w = meta['img_shape'][:2]
        b = _flip(b, h, w, meta['flip_direction'] if meta['flip'] else None)
        bl.append((b.view(-1, 4) / b.new_tensor(meta['scale_factor'])).view(b.shape))
        sl.append(s)
    cfg = m.test_cfg
    return multiclass_nms(torch.stack(bl).mean(0), torch.stack(sl).mean(0), cfg.score_thr, cfg.nms, cfg.max_per_img)


def composed_probs(m, xs, metas, dets, labels):
    ps = []
    graphed = getattr(m, '_mask_graphs', None) is not None
    for x, (meta,) in zip(xs, metas):
        logits = m.simple_test_mask_logits(x, _mapping(dets, meta), labels)
        p = torch.sigmoid(logits.clone() if graphed else logits)
        if meta['flip']:
            p = torch.flip(p, [3] if meta['flip_direction'] == 'horizontal' else [2])
        ps.append(p)
    return torch.stack(ps).mean(0).contiguous()


def composed_call(m, xs, props, metas):
    from dynamask_amd import ops
    from dynamask_amd.postprocess import bbox2result
    dets, labels = composed_bboxes(m, xs, props, metas)
    bbox_results = bbox2result(dets, labels, m.bbox_head.num_classes)
    probs = composed_probs(m, xs, metas, dets, labels)
    h, w = metas[0][0]['ori_shape'][:2]
    rles = ops.paste_rle(probs, dets[:, :4].contiguous(), h, w, m.test_cfg.mask_thr_binary, apply_sigmoid=False)
    segm = [[] for _ in range(m.bbox_head.num_classes)]
    for c, r in zip(labels.tolist(), rles):
        segm[c].append(r)
    return bbox_results, segm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, nargs='+', default=[1, 2, 4])
    ap.add_argument('--iters', type=int, default=7)
    args = ap.parse_args()
    from dynamask_amd import synth
    dev = torch.device('cuda:0')
    m = build_head(dev)
    props = synth.make_rois(1, N_PROPS, IMG_H, IMG_W, seed=60)[:, 1:].contiguous().to(dev)
    maps = {}
    for V in args.views:
        xs, metas = [], []
        for s, d in VIEW_SETS[V]:
            h, w = int(round(IMG_H * s)), int(round(IMG_W * s))
            if s not in maps:
                maps[s] = [f.to(dev) for f in synth.make_fpn(1, h, w, 256, seed=50 + int(s * 100))]
            xs.append(maps[s] if d is None else [torch.flip(f, [3]).contiguous() for f in maps[s]])
            metas.append([dict(img_shape=(h, w, 3), ori_shape=(IMG_H, IMG_W, 3), scale_factor=np.float32(s) * np.ones(4, np.float32),
                               flip=d is not None, flip_direction=d)])
        with torch.no_grad():
            dets, labels = m.aug_test_bboxes(xs, metas, [props], m.test_cfg)
            row = {'V': V, 'views': VIEW_SETS[V], 'detections': int(dets.shape[0]), 'map': f'{IMG_W}x{IMG_H}'}
            fns = {('call', 'aug'): lambda: m.aug_test(xs, [props], metas, encode=True),
                   ('call', 'composed'): lambda: composed_call(m, xs, props, metas),
                   ('probs', 'aug'): lambda: m.aug_test_mask_probs(xs, metas, dets, labels),
                   ('probs', 'composed'): lambda: composed_probs(m, xs, metas, dets, labels)}
            for mode in ('eager', 'graphed'):
                m.enable_inference_graphs(mode == 'graphed')
                for (name, kind), fn in fns.items():
                    row[f'{name}_ms_{kind}_{mode}'] = round(bench.time_kernel_median(fn, iters=args.iters, warmup=2), 4)
                    if name == 'call':
                        row[f'launches_per_call_{kind}_{mode}'] = count_launches(fn)
                        row[f'host_syncs_per_call_{kind}_{mode}'] = count_syncs(fn)
                for name in ('call', 'probs'):
                    a, c = row[f'{name}_ms_aug_{mode}'], row[f'{name}_ms_composed_{mode}']
                    row[f'{name}_aug_over_composed_{mode}'] = round(a / c, 3) if c > 0 else None
            m.enable_inference_graphs(False)
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
