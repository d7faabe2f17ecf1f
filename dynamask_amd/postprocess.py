"""Host-side result code of the RoI heads: class-wise NMS, the mask paste and its device -> host copies, the per-class
result lists.  Everything on the device goes through ``ops``; no head class is touched."""
import numpy as np
import torch

from . import ops


# ---------------------------------------------------------------- boxes
def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv.ops.nms.batched_nms (mmcv 1.0.5): boxes of different classes are moved apart by
    (max coordinate + 1) * class so that one NMS handles all classes."""
    cfg = dict(nms_cfg)
    cfg.pop('type', 'nms')
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    if class_agnostic:
        boxes_for_nms = boxes
    else:
        max_coordinate = boxes.max()
        offsets = idxs.to(boxes) * (max_coordinate + 1)
        boxes_for_nms = boxes + offsets[:, None]
    dets, keep = ops.nms(boxes_for_nms.contiguous(), scores.contiguous(), cfg.get('iou_threshold', cfg.get('iou_thr', 0.5)))
    return torch.cat([boxes[keep], dets[:, -1:]], 1), keep


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None):
    """core/post_processing/bbox_nms.py:5-68 -> (dets [k, 5], labels [k]), labels 0-based; the
    last score column (background) is ignored."""
    n, ncls = multi_scores.shape[0], multi_scores.shape[1] - 1
    fg = multi_scores[:, :ncls]
    cand = (fg > score_thr).nonzero(as_tuple=False)          # row-major: the reference's masked_select order
    if cand.shape[0] == 0:
        return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
    ri, ci = cand[:, 0], cand[:, 1]
    per_class = multi_bboxes.view(n, -1, 4)
    boxes = per_class[ri, ci] if per_class.shape[1] > 1 else per_class[ri, 0]
    scores = fg[ri, ci] if score_factors is None else (fg * score_factors[:, None])[ri, ci]
    dets, keep = batched_nms(boxes, scores, ci, nms_cfg)
    if max_num > 0:
        dets, keep = dets[:max_num], keep[:max_num]
    return dets, ci[keep]


def multiclass_nms_batch(multi_bboxes_list, multi_scores_list, score_thr, nms_cfg, max_num=-1):
    """``multiclass_nms`` of B images at once -> list of B (dets [k, 5], labels [k]), each what ``multiclass_nms`` gives
    for that image alone, bit for bit.  The score cut runs on all images' rows together; every image is one segment of
    ``ops.nms_segmented`` (suppression bits only within the image, greedy pass on the device, ``max_num`` per image).
    ``batched_nms``'s class offsets use each image's OWN largest coordinate, as the per-image call does.  Host waits: the
    candidate count, the per-image candidate counts and the per-image kept counts -- three, whatever B is."""
    B = len(multi_scores_list)
    assert len(multi_bboxes_list) == B
    if B == 0:
        return []
    ref = multi_bboxes_list[0]
    empty = lambda: (ref.new_zeros((0, 5)), ref.new_zeros((0,), dtype=torch.long))      # noqa: E731
    rows = [int(s.shape[0]) for s in multi_scores_list]
    if sum(rows) == 0:
        return [empty() for _ in range(B)]
    scores_all = torch.cat([s for s in multi_scores_list if s.shape[0] > 0], 0)
    ncls = scores_all.shape[1] - 1
    bboxes_all = torch.cat([b.reshape(b.shape[0], -1) for b in multi_bboxes_list if b.shape[0] > 0], 0)
    n = scores_all.shape[0]
    fg = scores_all[:, :ncls]
    cand = (fg > score_thr).nonzero(as_tuple=False)          # row-major: image after image, the per-image order in each
    if cand.shape[0] == 0:
        return [empty() for _ in range(B)]
    ri, ci = cand[:, 0], cand[:, 1]
    per_class = bboxes_all.view(n, -1, 4)
    boxes = per_class[ri, ci] if per_class.shape[1] > 1 else per_class[ri, 0]
    scores = fg[ri, ci]
    row_start = ops._upload([sum(rows[:b + 1]) for b in range(B)], torch.int64, ref.device)
    img = torch.searchsorted(row_start, ri, right=True)       # image of every candidate
    counts = torch.bincount(img, minlength=B).cpu().tolist()
    cfg = dict(nms_cfg)
    cfg.pop('type', 'nms')
    class_agnostic = cfg.pop('class_agnostic', False)
    if class_agnostic:
        boxes_for_nms = boxes
    else:
        # batched_nms: boxes.max() of the image's own candidates, the same fp32 operations in the same order
        seg_max = torch.full((B,), float('-inf'), device=boxes.device, dtype=boxes.dtype)
        seg_max = seg_max.scatter_reduce(0, img, boxes.amax(1), 'amax')
        offsets = ci.to(boxes) * (seg_max + 1)[img]
        boxes_for_nms = boxes + offsets[:, None]
    # per-image stable descending sort == stable descending sort of all, then a stable sort by image
    o1 = torch.sort(scores, descending=True, stable=True)[1]
    order = o1[torch.sort(img[o1], stable=True)[1]]
    sb = boxes_for_nms[order].contiguous()
    keep, kept = ops.nms_segmented(sb, counts, cfg.get('iou_threshold', cfg.get('iou_thr', 0.5)), max_num=max_num)
    kept = kept.cpu().tolist()
    out, start = [], 0
    for b in range(B):
        k = kept[b]
        if k == 0:
            out.append(empty())
        else:
            g = order[keep[start:start + k].long() + start]
            out.append((torch.cat([boxes[g], scores[g][:, None]], 1), ci[g]))
        start += counts[b]
    return out


def bbox2result(bboxes, labels, num_classes):
    """core/bbox/transforms.py:76-96."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    bboxes = bboxes.cpu().numpy()
    labels = labels.cpu().numpy()
    return [bboxes[labels == i, :] for i in range(num_classes)]


def _bbox2result_host(bboxes, labels, num_classes):
    """``bbox2result`` on host arrays already copied (the batched call copies all images' detections at once)."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    return [bboxes[labels == i, :] for i in range(num_classes)]


# ---------------------------------------------------------------- masks
def _paste_geometry(det_bboxes, ori_shape, scale_factor, rescale):
    """The canvas size and the boxes in canvas pixels, as both heads' ``get_seg_masks`` derive them
    (dynamask_head.py:293-305 = fcn_mask_head.py:176-186)."""
    bboxes = det_bboxes[:, :4]
    if rescale:
        img_h, img_w = ori_shape[:2]
    else:
        img_h = int(np.round(ori_shape[0] * scale_factor).astype(np.int32))
        img_w = int(np.round(ori_shape[1] * scale_factor).astype(np.int32))
        scale_factor = 1.0
    if not isinstance(scale_factor, (float, torch.Tensor)):
        scale_factor = bboxes.new_tensor(scale_factor)
    return (bboxes / scale_factor).contiguous(), int(img_h), int(img_w)


def _to_host_pending(*tensors):
    """Enqueue device -> host copies into fresh pinned buffers WITHOUT a synchronisation: the buffers hold the values once
    the current stream has been synchronised by the caller's next host wait (the mask paste's copy, or its RLE
    collection).  -> the pinned host tensors."""
    hosts = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors]
    for h, t in zip(hosts, tensors):
        h.copy_(t, non_blocking=True)
    return hosts


def _to_host(*tensors):
    """device -> host as the reference does (``t.cpu().numpy()``), but every tensor into a fresh pinned buffer (PCIe rate
    instead of the pageable-memory rate; the reference copies each mask on its own), all copies non-blocking and ONE
    synchronisation of the current stream -> the numpy arrays."""
    hosts = _to_host_pending(*tensors)
    torch.cuda.current_stream().synchronize()
    return [h.numpy() for h in hosts]


def _mask_threshold(rcnn_test_cfg):
    threshold = rcnn_test_cfg.mask_thr_binary
    if threshold < 0:
        raise NotImplementedError('visualisation mode (mask_thr_binary < 0) is not on the path')
    return threshold


def select_label_channel(mask_pred, labels):
    """[n, C, S, S] -> the channel of every detection's label [n, 1, S, S] (fcn_mask_head.py:211-212): one gather when
    C > 1 (the sigmoid of the paste commutes with it)."""
    if mask_pred.shape[1] > 1:
        mask_pred = mask_pred[torch.arange(len(mask_pred), device=mask_pred.device), labels.to(mask_pred.device)][:, None]
    return mask_pred.contiguous()


def paste_segms(mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale, encode=False,
                apply_sigmoid=True, num_classes=None, labels_host=None):
    """The paste of every ``get_seg_masks`` / ``get_seg_rles`` (dynamask_head.py:279-342, fcn_mask_head.py:151-237) and
    of the RoI heads' one-image mask tests: ``mask_pred`` [n, 1, S, S] (the label channel; ``apply_sigmoid``: logits)
    pasted into the image, thresholded, by one kernel for all detections.  Bitmaps: ONE device -> host copy of all masks
    -> (h, w) bool arrays.  ``encode``: ``get_seg_masks`` followed by ``encode_mask_results`` (core/mask/utils.py:36-63)
    without the bitmaps -- paste, threshold and run-length encoding on the device, only run boundaries are copied to the
    host: COCO RLE dicts, what ``mask_util.encode(np.array(m[:, :, None], order='F'))[0]`` yields for the bitmap.
    Returns one entry per detection, or with ``num_classes`` the per-class lists (``cls_segms``: a class's detections in
    detection order; ``labels_host``: ``det_labels`` already on the host)."""
    bboxes, img_h, img_w = _paste_geometry(det_bboxes, ori_shape, scale_factor, rescale)
    threshold = _mask_threshold(rcnn_test_cfg)
    if len(mask_pred) == 0:
        return [] if num_classes is None else [[] for _ in range(num_classes)]
    if encode:
        segs = ops.paste_rle(mask_pred, bboxes, img_h, img_w, threshold, apply_sigmoid=apply_sigmoid)
    else:
        im, = _to_host(ops.paste_masks(mask_pred, bboxes, img_h, img_w, threshold, apply_sigmoid=apply_sigmoid))
        segs = list(im)
    if num_classes is None:
        return segs
    cls_segms = [[] for _ in range(num_classes)]
    for c, segm in zip(det_labels.tolist() if labels_host is None else labels_host, segs):
        cls_segms[c].append(segm)
    return cls_segms


def group_mask_scores(scores, labels, num_classes):
    """Host arrays [n] -> ``[scores[labels == i] for i in range(num_classes)]`` (maskiou_head.py:178-181)."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    return [scores[labels == i] for i in range(num_classes)]
