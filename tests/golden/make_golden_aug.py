"""Golden vectors for test-time augmentation from the REFERENCE's own modules: ``StandardRoIHead.aug_test``
(standard_roi_head.py:264-290) with ``BBoxTestMixin.aug_test_bboxes`` / ``MaskTestMixin.aug_test_mask``
(test_mixins.py:73-107,178-208), ``bbox_mapping`` / ``bbox_mapping_back`` / ``bbox_flip`` (core/bbox/transforms.py),
``merge_aug_bboxes`` / ``merge_aug_masks`` (core/post_processing/merge_augs.py), ``multiclass_nms`` and
``FCNMaskHead.get_seg_masks``, run on the CPU.  Loaded by path with the stand-ins of make_golden.py; mmcv's operators
delegate to oracle/ (RoIAlign, CARAFE: ref_ops.py; batched_nms: ref_model.py), as in g10, g11 and g14.

Two cases over one 128 x 160 image (FPN maps and weights from fixed seeds, re-derived by the test):
  * ``ms``: four views, scales 1.0 and 1.5 x {no flip, horizontal flip};
  * ``vf``: three views, scale 1.0 unflipped, scale 1.0 vertically flipped, scale 1.25 horizontally flipped.
Stored per case: the dets and labels of ``aug_test(rescale=True)``, the merged probabilities of each detection's class
(the ``merge_aug_masks`` result ``aug_test_mask`` pastes), and the bitmaps.

Run ONLY in the authoring container:  python tests/golden/make_golden_aug.py  ->  tests/golden/g16_aug.npz"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aug_inputs as ai  # noqa: E402
import make_golden as mg  # noqa: E402
from oracle import ref_model  # noqa: E402


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def load_aug_reference():
    R = mg.load_reference()
    core = mg._pkg('mmdet.core')
    core.multi_apply = lambda f, *a, **k: tuple(map(list, zip(*map(f, *a))))
    tr = sys.modules['mmdet.core.bbox.transforms']
    bb = mg._pkg('mmdet.core.bbox')
    bb.bbox_mapping_back = tr.bbox_mapping_back
    core.bbox_mapping, core.bbox2result = tr.bbox_mapping, tr.bbox2result
    # bbox coder + Shared2FCBBoxHead (as make_golden_bbox.py)
    bld = mg._pkg('mmdet.core.bbox.builder')
    bld.BBOX_CODERS = mg.Registry('bbox_coder')
    bld.build_bbox_coder = lambda cfg, **kw: mg.build_from_cfg(cfg, bld.BBOX_CODERS, kw)
    core.build_bbox_coder = bld.build_bbox_coder
    mg._pkg('mmdet.core.bbox.coder')
    mg._load('mmdet.core.bbox.coder.base_bbox_coder', 'mmdet/core/bbox/coder/base_bbox_coder.py')
    mg._load('mmdet.core.bbox.coder.delta_xywh_bbox_coder', 'mmdet/core/bbox/coder/delta_xywh_bbox_coder.py')
    nmsmod = mg._pkg('mmcv.ops.nms')
    nmsmod.batched_nms = lambda boxes, scores, idxs, cfg, class_agnostic=False: ref_model.batched_nms(boxes, scores, idxs, cfg)
    mg._pkg('mmcv.ops').nms = None                      # (merge_aug_proposals only)
    mg._pkg('mmdet.core.post_processing')
    pp = mg._load('mmdet.core.post_processing.bbox_nms', 'mmdet/core/post_processing/bbox_nms.py')
    ma = mg._load('mmdet.core.post_processing.merge_augs', 'mmdet/core/post_processing/merge_augs.py')
    core.multiclass_nms, core.merge_aug_bboxes, core.merge_aug_masks = pp.multiclass_nms, ma.merge_aug_bboxes, ma.merge_aug_masks
    R['builder'].build_loss = lambda cfg: None
    mg._pkg('mmdet.models.losses').accuracy = lambda *a, **k: None
    mg._pkg('mmdet.models.roi_heads.bbox_heads')
    mg._load('mmdet.models.roi_heads.bbox_heads.bbox_head', 'mmdet/models/roi_heads/bbox_heads/bbox_head.py')
    mg._load('mmdet.models.roi_heads.bbox_heads.convfc_bbox_head', 'mmdet/models/roi_heads/bbox_heads/convfc_bbox_head.py')
    # the real mixins in place of make_golden.py's empty ones, then StandardRoIHead again on top of them
    mg._pkg('mmdet.utils.contextmanagers').completed = None
    tm = mg._load('mmdet.models.roi_heads.test_mixins', 'mmdet/models/roi_heads/test_mixins.py')
    srh = mg._load('mmdet.models.roi_heads.standard_roi_head', 'mmdet/models/roi_heads/standard_roi_head.py')
    R.update(tr=tr, ma=ma, pp=pp, tm=tm, srh=srh)
    return R


def build_reference_head(R):
    head = R['srh'].StandardRoIHead(
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **ai.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **ai.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **ai.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='FCNMaskHead', **ai.FCN_HEAD_CFG), train_cfg=None,
        test_cfg=_Cfg(ai.TEST_CFG))
    head.load_state_dict(ai.head_state(), strict=True)
    return head.eval()


def run_case(R, head, case):
    x, proposals, img_metas = ai.case_inputs(case)
    with torch.no_grad():
        bbox_results, segm_results = head.aug_test(x, [proposals], img_metas, rescale=True)
        det_bboxes, det_labels = head.aug_test_bboxes(x, img_metas, [proposals], head.test_cfg)
        # the probabilities aug_test_mask pastes: its own loop up to merge_aug_masks (test_mixins.py:183-198)
        aug_masks = []
        for xv, meta in zip(x, img_metas):
            m = meta[0]
            b = R['tr'].bbox_mapping(det_bboxes[:, :4], m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'])
            aug_masks.append(head._mask_forward(xv, R['tr'].bbox2roi([b]))['mask_pred'].sigmoid().cpu().numpy())
        merged = R['ma'].merge_aug_masks(aug_masks, img_metas, head.test_cfg)
        # the merged candidate scores: no two within 1e-5 (the NMS order must not hang on an ulp)
        rois = []
        aug_scores = []
        for xv, meta in zip(x, img_metas):
            m = meta[0]
            p = R['tr'].bbox_mapping(proposals[:, :4], m['img_shape'], m['scale_factor'], m['flip'], m['flip_direction'])
            r = R['tr'].bbox2roi([p])
            res = head._bbox_forward(xv, r)
            _, s = head.bbox_head.get_bboxes(r, res['cls_score'], res['bbox_pred'], m['img_shape'], m['scale_factor'],
                                             rescale=False, cfg=None)
            aug_scores.append(s)
            rois.append(r)
    ms = torch.stack(aug_scores).mean(0)[:, :-1]
    cand = np.sort(ms[ms > ai.TEST_CFG['score_thr']].numpy())
    gap = float(np.diff(cand).min())
    assert gap > 1e-5, f'{case}: two candidate scores {gap} apart'
    n = det_bboxes.shape[0]
    assert n > 0 and [len(c) for c in bbox_results] == [len(c) for c in segm_results]
    lab = det_labels.numpy()
    probs = merged[np.arange(n), lab]
    # bitmaps in detection order (the per-class lists keep detection order)
    seen, bits = {}, []
    for c in lab.tolist():
        k = seen.get(c, 0)
        bits.append(segm_results[c][k])
        seen[c] = k + 1
    bits = np.stack(bits).astype(np.uint8)
    band = int((np.abs(probs - ai.TEST_CFG['mask_thr_binary']) < 1e-3).sum())
    print(f'{case}: {n} detections, {len(cand)} candidates (min score gap {gap:.2e}), {band} of {probs.size} merged '
          f'probabilities within 1e-3 of the threshold, {int(bits.sum())} foreground pixels')
    return {f'{case}_dets': det_bboxes.numpy(), f'{case}_labels': lab.astype(np.int64),
            f'{case}_probs': probs.astype(np.float32), f'{case}_bits': bits,
            f'{case}_bbox_counts': np.array([len(c) for c in bbox_results], np.int32)}


def main():
    torch.set_num_threads(8)
    R = load_aug_reference()
    head = build_reference_head(R)
    out = {}
    for case in ai.CASES:
        out.update(run_case(R, head, case))
    path = os.path.join(HERE, 'g16_aug.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
