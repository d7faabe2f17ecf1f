"""RefineMask fixture from the REFERENCE's own modules: tests/golden/g17_refine.npz and g17_refine_configs.json.

    python tests/golden/make_golden_refine.py REFERENCE_ROOT

Loads ``mmdet/models/roi_heads/mask_heads/refine_mask_head.py`` and ``mmdet/models/roi_heads/refine_roi_head.py`` by
path under the stand-ins of make_golden.py (ConvModule = nn.Conv2d (+ ReLU) with its dilation, RoIAlign = oracle/ref_ops),
builds the reference ``RefineRoIHead`` from the COCO config's ``roi_head`` (mask branch; the bbox branch is the one the
other RoI heads share, pinned by g10) with the seeded weights of refine_inputs.py, and runs on the CPU:

  * ``_mask_forward`` of the detections: the four stage logits and ``semantic_pred``;
  * ``simple_test_mask``: the merged 112 x 112 logits handed to ``get_seg_masks`` and the bitmaps it returns;
  * the reference RoI head's ``state_dict`` key list.

The JSON holds the COCO (r50 1x), Cityscapes and LVIS configs' ``model.roi_head`` / ``train_cfg.rcnn`` /
``test_cfg.rcnn`` as ``registry.Config.fromfile`` resolves them (make_golden_configs.py's form)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CONFIGS = {'coco': 'configs/refinemask/coco/r50-refinemask-1x.py',
           'cityscapes': 'configs/refinemask/cityscapes/r50-refinemask.py',
           'lvis': 'configs/refinemask/lvis/r50-refinemask-1x.py'}


def _configs(ref):
    from dynamask_amd import registry
    out = {}
    for name, rel in CONFIGS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        out[name] = {'source': rel, 'model': {'roi_head': cfg.model.roi_head},
                     'train_cfg': {'rcnn': cfg.train_cfg.rcnn}, 'test_cfg': {'rcnn': cfg.test_cfg.rcnn}}
    return out


def main(ref):
    import make_golden as mg
    import refine_inputs as ri
    mg.REF = ref
    torch.manual_seed(0)
    torch.set_num_threads(4)
    mg.load_reference()
    mh = mg._load('mmdet.models.roi_heads.mask_heads.refine_mask_head', 'mmdet/models/roi_heads/mask_heads/refine_mask_head.py')
    rr = mg._load('mmdet.models.roi_heads.refine_roi_head', 'mmdet/models/roi_heads/refine_roi_head.py')

    cfgs = _configs(ref)
    rh = cfgs['coco']['model']['roi_head']
    test_cfg = cfgs['coco']['test_cfg']['rcnn']
    from dynamask_amd import registry
    roi = rr.RefineRoIHead(mask_roi_extractor=dict(rh['mask_roi_extractor']), mask_head=dict(rh['mask_head']),
                           test_cfg=registry._to_cfgdict(test_cfg))
    roi.eval()
    head = roi.mask_head
    assert isinstance(head, mh.RefineMaskHead)
    sd = head.state_dict()
    head.load_state_dict(ri.head_state({k: v.shape for k, v in sd.items()}), strict=True)

    feats = ri.fpn_feats()
    det_bboxes, det_labels = ri.detections()
    metas = ri.img_metas()
    out = {}
    with torch.no_grad():
        rois = torch.cat([det_bboxes.new_zeros((len(det_bboxes), 1)), det_bboxes[:, :4]], 1)
        res = roi._mask_forward(feats, rois, det_labels)
        for i, p in enumerate(res['stage_instance_preds']):
            out[f'stage{i}'] = p.numpy().astype(np.float32)
        out['semantic_pred'] = res['semantic_pred'].numpy().astype(np.float32)
        captured = {}
        orig = head.get_seg_masks

        def get_seg_masks(mask_pred, *a, **k):
            captured['merged'] = mask_pred.clone()
            return orig(mask_pred, *a, **k)
        head.get_seg_masks = get_seg_masks
        segm = roi.simple_test_mask(feats, metas, det_bboxes, det_labels, rescale=False)
    out['merged'] = captured['merged'].numpy().astype(np.float32)
    # bitmaps in detection order (simple_test_mask groups them by class, in detection order within a class)
    seen = {}
    bitmaps = []
    for lab in det_labels.tolist():
        j = seen.get(lab, 0)
        seen[lab] = j + 1
        bitmaps.append(np.asarray(segm[lab][j], dtype=bool))
    out['bitmaps'] = np.packbits(np.stack(bitmaps), axis=-1)
    out['bitmap_shape'] = np.array(np.stack(bitmaps).shape, dtype=np.int64)
    out['det_bboxes'] = det_bboxes.numpy()
    out['det_labels'] = det_labels.numpy()
    keys = sorted(roi.state_dict().keys())
    out['state_dict_keys'] = np.array(keys)
    path = os.path.join(HERE, 'g17_refine.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    path = os.path.join(HERE, 'g17_refine_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_refine.py REFERENCE_ROOT')
    main(sys.argv[1])
