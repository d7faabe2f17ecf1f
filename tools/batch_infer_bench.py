#!/usr/bin/env python
"""Batched multi-image inference against a Python loop of one-image calls.

For B = 1, 2, 4, 8 images of 1333x800 (FPN maps P2..P6, batch dimension B) with 100 detections per image
(64 proposals per image, score_thr 0, max_per_img 100: every image keeps exactly 100 detections), prints one JSON line
per B with, per image:
  call_ms_*      the whole simple_test (bbox branch, NMS, mask chain, paste + RLE to COCO dicts on the host):
                 ``loop`` = B calls of simple_test, ``batch`` = one batch_simple_test; eager and graphed
                 (enable_inference_graphs: the one-image buckets for the loop, graphs.BATCH_BUCKETS for the batch;
                 totals above the largest bucket run eagerly);
  logits_ms_*    the mask chain alone (simple_test_mask_logits per image / batch_simple_test_mask_logits);
and, per call, the number of C-ABI launches (dm_* calls that enqueue work) and of host waits (torch's sync debug
mode + explicit stream synchronisations).  Times: median of individually event-timed calls (bench.time_kernel_median),
host work included.

    python tools/batch_infer_bench.py [--batches 1 2 4 8] [--iters 7]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

IMG_H, IMG_W = 800, 1333
N_PROPS = 64
_QUERIES = ('dm_error_string', 'dm_abi_version', 'dm_build_info', 'dm_rle_string', 'dm_nms_reduce')


def build_head(dev):
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, synth  # noqa: F401
    from dynamask_amd.registry import ConfigDict
    m = registry.build_head(dict(
        type='DynaMaskRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG),
        test_cfg=ConfigDict(score_thr=0.0, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100,
                            mask_thr_binary=0.5)))
    m.load_state_dict({**synth.init_dynamask_head_state(seed=5, test_mode=True), **synth.init_mask_pre_state(seed=6),
                       **synth.init_bbox_head_state(seed=8)}, strict=True)
    return m.to(dev).eval()


class _CountingLib:
    """Stands in for the loaded library and counts the calls that enqueue device work."""

    def __init__(self, real):
        self._real, self.launches = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith('dm_') and name not in _QUERIES and 'scratch' not in name and 'supported' not in name \
                and 'packed_' not in name and 'workspace' not in name and 'splitk_floats' not in name:
            def counted(*a):
                self.launches += 1
                return fn(*a)
            return counted
        return fn


def count_launches(fn):
    from dynamask_amd import _lib
    _lib.lib()
    real = _lib._LIB
    proxy = _CountingLib(real)
    _lib._LIB = proxy
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib._LIB = real
    return proxy.launches


def count_syncs(fn):
    calls = [0]
    real = torch.cuda.Stream.synchronize

    def counting(self):
        calls[0] += 1
        return real(self)
    torch.cuda.Stream.synchronize = counting
    try:
        n = bench.count_host_syncs(fn)
    finally:
        torch.cuda.Stream.synchronize = real
    return None if n is None else n + calls[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 2, 4, 8])
    ap.add_argument('--iters', type=int, default=7)
    args = ap.parse_args()
    from dynamask_amd import synth
    dev = torch.device('cuda:0')
    m = build_head(dev)
    for B in args.batches:
        x = [f.to(dev) for f in synth.make_fpn(B, IMG_H, IMG_W, 256, seed=50)]
        xs = [[f[b:b + 1].contiguous() for f in x] for b in range(B)]
        props = [synth.make_rois(1, N_PROPS, IMG_H, IMG_W, seed=60 + b)[:, 1:].contiguous().to(dev) for b in range(B)]
        metas = [dict(img_shape=(IMG_H, IMG_W, 3), ori_shape=(IMG_H, IMG_W, 3), scale_factor=1.0) for _ in range(B)]
        with torch.no_grad():
            dets = m.batch_simple_test_bboxes(x, metas, props, m.test_cfg)
            n_det = [int(d.shape[0]) for d, _ in dets]
            boxes, labels = [d for d, _ in dets], [l for _, l in dets]

            def loop_call():
                return [m.simple_test(xs[b], [props[b]], [metas[b]], encode=True) for b in range(B)]

            def batch_call():
                return m.batch_simple_test(x, props, metas, encode=True)

            def loop_logits():
                return [m.simple_test_mask_logits(xs[b], boxes[b], labels[b]) for b in range(B)]

            def batch_logits():
                return m.batch_simple_test_mask_logits(x, boxes, labels)
            row = {'B': B, 'detections_per_image': n_det, 'map': f'{IMG_W}x{IMG_H}'}
            for mode in ('eager', 'graphed'):
                m.enable_inference_graphs(mode == 'graphed')
                for name, fn in (('call', loop_call), ('call', batch_call), ('logits', loop_logits),
                                 ('logits', batch_logits)):
                    kind = 'loop' if fn in (loop_call, loop_logits) else 'batch'
                    ms = bench.time_kernel_median(fn, iters=args.iters, warmup=2)
                    row[f'{name}_ms_per_image_{kind}_{mode}'] = round(ms / B, 4)
                    if name == 'call':
                        row[f'launches_per_call_{kind}_{mode}'] = count_launches(fn)
                        row[f'host_syncs_per_call_{kind}_{mode}'] = count_syncs(fn)
                for name in ('call', 'logits'):
                    lo, ba = row[f'{name}_ms_per_image_loop_{mode}'], row[f'{name}_ms_per_image_batch_{mode}']
                    row[f'{name}_batch_over_loop_{mode}'] = round(ba / lo, 3) if lo > 0 else None
            m.enable_inference_graphs(False)
        print(json.dumps(row), flush=True)
        del x, xs


if __name__ == '__main__':
    main()
