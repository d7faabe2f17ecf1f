"""Cascade Mask R-CNN fixture from the REFERENCE's own modules: tests/golden/g21_cascade.npz and g21_cascade_configs.json.

    python tests/golden/make_golden_cascade.py REFERENCE_ROOT

Loads ``cascade_roi_head.py`` by path under the stand-ins of make_golden.py / make_golden_aug.py (RoIAlign and batched_nms
delegate to oracle/), builds the reference ``CascadeRoIHead`` from configs/cascade_rcnn/cascade_mask_rcnn_r50_fpn_1x_coco.py's
``roi_head`` (three stages, per-stage stds, class-agnostic regression) with the seeded weights of cascade_inputs.py and
runs on the CPU:

  * ``simple_test(rescale=False)`` on one 128 x 160 image: the detections, their labels and the bitmaps (np.packbits) in
    detection order, and the merged probabilities of each detection's class;
  * ``aug_test(rescale=True)`` over two scales x {no flip, horizontal flip}: the same four arrays;
  * the reference RoI head's ``state_dict`` key list.

The JSON holds the config's ``model.roi_head`` / ``train_cfg.rcnn`` / ``test_cfg.rcnn`` as ``registry.Config.fromfile``
resolves them."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CONFIG = 'configs/cascade_rcnn/cascade_mask_rcnn_r50_fpn_1x_coco.py'


def _configs(ref):
    from dynamask_amd import registry
    cfg = registry.Config.fromfile(os.path.join(ref, CONFIG))
    return {'coco': {'source': CONFIG, 'model': {'roi_head': cfg.model.roi_head},
                     'train_cfg': {'rcnn': cfg.train_cfg.rcnn}, 'test_cfg': {'rcnn': cfg.test_cfg.rcnn}}}


def load_cascade_reference(ref):
    import make_golden as mg
    import make_golden_aug as mga
    mg.REF = ref
    R = mga.load_aug_reference()
    R['crh'] = mg._load('mmdet.models.roi_heads.cascade_roi_head', 'mmdet/models/roi_heads/cascade_roi_head.py')
    return R


def _per_detection(per_class, labels):
    """per-class lists -> the entries in detection order (the lists keep detection order within a class)."""
    seen, out = {}, []
    for lab in labels:
        j = seen.get(lab, 0)
        seen[lab] = j + 1
        out.append(per_class[lab][j])
    return out


def _merged_probs(head, R, x_views, metas_views, det_bboxes, det_labels, simple):
    """The probabilities the reference pastes: its own loop up to merge_aug_masks (cascade_roi_head.py:340-349 /
    424-437), the detection's class channel."""
    aug_masks, aug_metas = [], []
    for xv, meta in zip(x_views, metas_views):
        m = meta[0]
        b = det_bboxes[:, :4] if simple else R['tr'].bbox_mapping(det_bboxes[:, :4], m['img_shape'], m['scale_factor'],
                                                                 m['flip'], m['flip_direction'])
        rois = R['tr'].bbox2roi([b])
        for i in range(head.num_stages):
            aug_masks.append(head._mask_forward(i, xv, rois)['mask_pred'].sigmoid().cpu().numpy())
            aug_metas.append(meta)
    merged = R['ma'].merge_aug_masks(aug_masks, aug_metas, head.test_cfg)
    return merged[np.arange(det_bboxes.shape[0]), det_labels.numpy()].astype(np.float32)


def _record(prefix, bbox_results, segm_results, probs):
    """dets / labels / bitmaps in detection order from the per-class lists."""
    dets, labels = [], []
    for c, b in enumerate(bbox_results):
        for row in b:
            dets.append(row)
            labels.append(c)
    # bbox2result groups by class; the detection order within a class is kept, so the class-major order is the one the
    # port's per-class lists give as well
    bm = np.stack([np.asarray(m, dtype=bool) for m in _per_detection(segm_results, labels)])
    return {f'{prefix}_dets': np.asarray(dets, np.float32), f'{prefix}_labels': np.asarray(labels, np.int64),
            f'{prefix}_bits': np.packbits(bm, axis=-1), f'{prefix}_bits_shape': np.array(bm.shape, np.int64),
            f'{prefix}_probs': probs}


def main(ref):
    import cascade_inputs as ci
    from dynamask_amd import registry
    torch.manual_seed(0)
    torch.set_num_threads(4)
    R = load_cascade_reference(ref)
    cfgs = _configs(ref)
    rh = dict(cfgs['coco']['model']['roi_head'])
    rh.pop('type')
    test_cfg = registry._to_cfgdict(dict(ci.TEST_CFG))
    head = R['crh'].CascadeRoIHead(test_cfg=test_cfg, train_cfg=None, **rh).eval()
    sd = head.state_dict()
    keys = sorted(sd.keys())
    mine = {k: v.shape for k, v in sd.items() if k.startswith(('bbox_head.', 'mask_head.'))}
    head.load_state_dict(ci.head_state(mine), strict=False)
    out = {'state_dict_keys': np.array(keys)}
    with torch.no_grad():
        # simple_test, one image
        x, props, metas = ci.simple_inputs()
        bbox_res, segm_res = head.simple_test(x, [props], metas, rescale=False)
        dets = torch.from_numpy(np.concatenate([b for b in bbox_res if len(b)], 0))
        labs = torch.tensor([c for c, b in enumerate(bbox_res) for _ in range(len(b))], dtype=torch.long)
        probs = _merged_probs(head, R, [x], [metas], dets, labs, simple=True)
        out.update(_record('simple', bbox_res, segm_res, probs))
        # aug_test, four views
        xs, props, metas_v = ci.aug_inputs()
        bbox_res, segm_res = head.aug_test(xs, [props], metas_v, rescale=True)
        dets = torch.from_numpy(np.concatenate([b for b in bbox_res if len(b)], 0))
        labs = torch.tensor([c for c, b in enumerate(bbox_res) for _ in range(len(b))], dtype=torch.long)
        probs = _merged_probs(head, R, xs, metas_v, dets, labs, simple=False)
        out.update(_record('aug', bbox_res, segm_res, probs))
    for p in ('simple', 'aug'):
        pr = out[f'{p}_probs']
        band = int((np.abs(pr - ci.TEST_CFG['mask_thr_binary']) < 1e-3).sum())
        print(f"{p}: {len(out[f'{p}_labels'])} detections, {band} of {pr.size} merged probabilities within 1e-3 of the "
              f"threshold, {int(np.unpackbits(out[f'{p}_bits']).sum())} foreground bits")
    path = os.path.join(HERE, 'g21_cascade.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    path = os.path.join(HERE, 'g21_cascade_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_cascade.py REFERENCE_ROOT')
    main(sys.argv[1])
