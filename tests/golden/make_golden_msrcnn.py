"""Mask Scoring R-CNN fixture from the REFERENCE's own modules: tests/golden/g19_msrcnn.npz and g19_msrcnn_configs.json.

    python tests/golden/make_golden_msrcnn.py REFERENCE_ROOT

Loads ``maskiou_head.py`` and ``mask_scoring_roi_head.py`` by path under the stand-ins of make_golden.py /
make_golden_aug.py, plus ``mmcv.ops.Conv2d`` / ``Linear`` / ``MaxPool2d`` (nn.Conv2d / nn.Linear / nn.MaxPool2d, what the
mmcv wrappers are for non-empty inputs) and no-op ``kaiming_init`` / ``normal_init`` (the weights are seeded).  It builds
the reference ``MaskScoringRoIHead`` from configs/ms_rcnn's ``roi_head`` (merged over its mask_rcnn base) with the seeded
weights of msrcnn_inputs.py and runs on the CPU:

  * ``MaskIoUHead.forward`` on the ``_mask_forward`` results of the detections: ``mask_iou_pred`` [n, 80];
  * ``simple_test_mask``: the bitmaps (np.packbits) on the 256 x 320 canvas and the mask scores, both in detection order;
  * the reference RoI head's ``state_dict`` key list.

The JSON holds the config's ``model.roi_head`` / ``train_cfg.rcnn`` / ``test_cfg.rcnn`` as ``registry.Config.fromfile``
resolves them."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CONFIG = 'configs/ms_rcnn/ms_rcnn_r50_fpn_1x_coco.py'


def _configs(ref):
    from dynamask_amd import registry
    cfg = registry.Config.fromfile(os.path.join(ref, CONFIG))
    return {'coco': {'source': CONFIG, 'model': {'roi_head': cfg.model.roi_head},
                     'train_cfg': {'rcnn': cfg.train_cfg.rcnn}, 'test_cfg': {'rcnn': cfg.test_cfg.rcnn}}}


def load_msrcnn_reference(ref):
    import make_golden as mg
    import make_golden_aug as mga
    mg.REF = ref
    R = mga.load_aug_reference()
    cnn = mg._pkg('mmcv.cnn')
    cnn.kaiming_init = lambda m, *a, **k: None
    cnn.normal_init = lambda m, *a, **k: None
    ops = mg._pkg('mmcv.ops')
    ops.Conv2d, ops.Linear, ops.MaxPool2d = nn.Conv2d, nn.Linear, nn.MaxPool2d
    R['maskiou'] = mg._load('mmdet.models.roi_heads.mask_heads.maskiou_head',
                            'mmdet/models/roi_heads/mask_heads/maskiou_head.py')
    R['msrh'] = mg._load('mmdet.models.roi_heads.mask_scoring_roi_head', 'mmdet/models/roi_heads/mask_scoring_roi_head.py')
    return R


def _per_detection(per_class, labels):
    """per-class lists -> the entries in detection order (the lists keep detection order within a class)."""
    seen, out = {}, []
    for lab in labels:
        j = seen.get(lab, 0)
        seen[lab] = j + 1
        out.append(per_class[lab][j])
    return out


def main(ref):
    import msrcnn_inputs as mi
    from dynamask_amd import registry
    torch.manual_seed(0)
    torch.set_num_threads(4)
    R = load_msrcnn_reference(ref)
    cfgs = _configs(ref)
    rh = dict(cfgs['coco']['model']['roi_head'])
    rh.pop('type')
    test_cfg = registry._to_cfgdict(dict(mi.TEST_CFG))
    head = R['msrh'].MaskScoringRoIHead(test_cfg=test_cfg, train_cfg=None, **rh).eval()
    sd = head.state_dict()
    keys = sorted(sd.keys())
    mine = {k: v.shape for k, v in sd.items() if k.startswith(('mask_head.', 'mask_iou_head.'))}
    head.load_state_dict(mi.head_state(mine), strict=False)

    feats = mi.fpn()
    det_bboxes, det_labels = mi.detections()
    metas = mi.img_metas()
    labels = det_labels.tolist()
    out = {}
    with torch.no_grad():
        rois = torch.cat([det_bboxes.new_zeros((len(det_bboxes), 1)), det_bboxes[:, :4]], 1)
        res = head._mask_forward(feats, rois)
        n = len(labels)
        out['mask_iou_pred'] = head.mask_iou_head(res['mask_feats'], res['mask_pred'][range(n), det_labels]).numpy()
        segm, scores = head.simple_test_mask(feats, metas, det_bboxes, det_labels, rescale=False)
        bm = np.stack([np.asarray(m, dtype=bool) for m in _per_detection(segm, labels)])
        out['bitmaps'] = np.packbits(bm, axis=-1)
        out['bitmap_shape'] = np.array(bm.shape, dtype=np.int64)
        out['mask_scores'] = np.array(_per_detection(scores, labels), dtype=np.float32)
        assert all(isinstance(s, np.ndarray) for s in scores) and len(scores) == 80
    out['det_bboxes'] = det_bboxes.numpy()
    out['det_labels'] = det_labels.numpy()
    out['state_dict_keys'] = np.array(keys)
    path = os.path.join(HERE, 'g19_msrcnn.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    path = os.path.join(HERE, 'g19_msrcnn_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_msrcnn.py REFERENCE_ROOT')
    main(sys.argv[1])
