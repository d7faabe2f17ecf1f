"""PointRefine fixture from the REFERENCE's own modules: tests/golden/g20_pointrefine.npz and g20_pointrefine_configs.json.

    python tests/golden/make_golden_pointrefine.py REFERENCE_ROOT

Loads ``mask_point_refine.py`` and ``point_refine_head.py`` by path under the stand-ins of make_golden_pointrend.py
(ConvModule with ``conv_cfg=dict(type='Conv1d')``, mmcv's ``point_sample`` / ``rel_roi_point_to_rel_img_point``), plus
a parameterless stand-in registered as ``PointRefineCrossEntropyLoss``: the config names that loss, and the reference
registers it nowhere (Quirk Q15), so without the stand-in the reference cannot build the head at all.  It builds the
reference ``PointRefineRoIHead`` from configs/point_refine's ``roi_head`` with the seeded weights of
pointrefine_inputs.py and runs on the CPU:

  * ``_mask_forward`` of the detections: the label-row instance predictions of stages 1-3 (28^2, 56^2, 112^2);
  * the stage-2 (56 x 56) selected index sets (sorted) and, per RoI, the gap between the P-th and (P + 1)-th largest
    key (stages 0 and 1 select every cell);
  * ``simple_test_mask``: the merged 112 x 112 logits handed to ``get_seg_masks`` and the bitmaps (np.packbits) on the
    192 x 256 canvas;
  * the reference RoI head's ``state_dict`` key list, in the reference's order.

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

CONFIG = 'configs/point_refine/r50-point-refine-1x.py'


class PointRefineCrossEntropyLoss(nn.Module):
    """Parameterless stand-in for the config's loss (Quirk Q15): inference never calls it."""

    def __init__(self, **kw):
        super().__init__()
        self.cfg = kw


def _configs(ref):
    from dynamask_amd import registry
    cfg = registry.Config.fromfile(os.path.join(ref, CONFIG))
    return {'coco': {'source': CONFIG, 'model': {'roi_head': cfg.model.roi_head},
                     'train_cfg': {'rcnn': cfg.train_cfg.rcnn}, 'test_cfg': {'rcnn': cfg.test_cfg.rcnn}}}


def load_pointrefine_reference(ref):
    import make_golden as mg
    import make_golden_pointrend as mgp
    R = mgp.load_pointrend_reference(ref)
    b = R['builder']
    b.LOSSES.module_dict['PointRefineCrossEntropyLoss'] = PointRefineCrossEntropyLoss
    b.build_loss = lambda cfg: mg.build_from_cfg(cfg, b.LOSSES)
    R['mpr'] = mg._load('mmdet.models.roi_heads.mask_heads.mask_point_refine',
                        'mmdet/models/roi_heads/mask_heads/mask_point_refine.py')
    R['prh2'] = mg._load('mmdet.models.roi_heads.point_refine_head', 'mmdet/models/roi_heads/point_refine_head.py')
    return R


def _bitmaps(segm, labels):
    """per-class lists -> [n, h, w] in detection order (the lists keep detection order within a class)."""
    seen, out = {}, []
    for lab in labels:
        j = seen.get(lab, 0)
        seen[lab] = j + 1
        out.append(np.asarray(segm[lab][j], dtype=bool))
    return np.stack(out)


def main(ref):
    import pointrefine_inputs as pi
    from dynamask_amd import registry
    torch.manual_seed(0)
    torch.set_num_threads(4)
    R = load_pointrefine_reference(ref)
    cfgs = _configs(ref)
    rh = dict(cfgs['coco']['model']['roi_head'])
    rh.pop('type')
    test_cfg = registry._to_cfgdict(dict(pi.TEST_CFG))
    head = R['prh2'].PointRefineRoIHead(test_cfg=test_cfg, train_cfg=None, **rh).eval()
    sd = head.state_dict()
    keys = list(sd.keys())
    mine = {k: v.shape for k, v in sd.items() if k.startswith('mask_head.')}
    head.load_state_dict({'mask_head.' + k[len('mask_head.'):]: v for k, v in pi.head_state(mine).items()}, strict=False)

    feats = pi.fpn_feats()
    det_bboxes, det_labels = pi.detections()
    metas = pi.img_metas()
    out = {}
    sels = []
    stage2 = head.mask_head.stages[2]
    orig_sel = stage2.get_roi_rel_points_train

    def get_roi_rel_points_train(detail_pred, cfg):
        inds, coords = orig_sel(detail_pred, cfg)
        n = detail_pred.shape[0]
        key = detail_pred.reshape(n, -1)
        srt = key.sort(dim=1, descending=True).values
        P = inds.shape[1]
        gap = (srt[:, P - 1] - srt[:, P]) if P < key.shape[1] else torch.full((n,), float('inf'))
        sels.append((inds.clone(), gap))
        return inds, coords
    stage2.get_roi_rel_points_train = get_roi_rel_points_train

    with torch.no_grad():
        rois = torch.cat([det_bboxes.new_zeros((len(det_bboxes), 1)), det_bboxes[:, :4]], 1)
        res = head._mask_forward(feats, rois, det_labels, test_cfg)
        for i, p in enumerate(res['stage_instance_preds']):
            if i >= 1:
                out[f'stage{i}'] = p.numpy().astype(np.float32)
        inds, gap = sels[0]
        out['select2'] = np.sort(inds.numpy(), axis=1).astype(np.int32)
        out['select2_gap'] = gap.numpy().astype(np.float32)
        captured = {}
        orig = head.mask_head.get_seg_masks

        def get_seg_masks(mask_pred, *a, **k):
            captured['merged'] = mask_pred.clone()
            return orig(mask_pred, *a, **k)
        head.mask_head.get_seg_masks = get_seg_masks
        segm = head.simple_test_mask(feats, metas, det_bboxes, det_labels, rescale=False)
    out['merged'] = captured['merged'].numpy().astype(np.float32)
    bm = _bitmaps(segm, det_labels.tolist())
    out['bitmaps'] = np.packbits(bm, axis=-1)
    out['bitmap_shape'] = np.array(bm.shape, dtype=np.int64)
    out['det_bboxes'] = det_bboxes.numpy()
    out['det_labels'] = det_labels.numpy()
    out['state_dict_keys'] = np.array(keys)
    path = os.path.join(HERE, 'g20_pointrefine.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    path = os.path.join(HERE, 'g20_pointrefine_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_pointrefine.py REFERENCE_ROOT')
    main(sys.argv[1])
