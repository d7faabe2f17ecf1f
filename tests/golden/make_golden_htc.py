"""Hybrid Task Cascade fixture from the REFERENCE's own modules: tests/golden/g22_htc.npz and g22_htc_configs.json.

    python tests/golden/make_golden_htc.py REFERENCE_ROOT

Loads ``htc_roi_head.py``, ``htc_mask_head.py`` and ``fused_semantic_head.py`` by path under the stand-ins of
make_golden.py / make_golden_aug.py / make_golden_cascade.py, builds the reference ``HybridTaskCascadeRoIHead`` from
configs/htc/htc_r50_fpn_1x_coco.py's ``roi_head`` (and a second one from htc_without_semantic_r50_fpn_1x_coco.py) with the
seeded weights of htc_inputs.py and runs on the CPU:

  * ``simple_test(rescale=False)`` on one 128 x 160 image and ``aug_test(rescale=True)`` over two scales x {no flip,
    horizontal flip}: the detections, their labels, the bitmaps (np.packbits) in detection order and the merged
    probabilities of each detection's class -- keys ``simple_*`` / ``aug_*`` with the semantic head, ``nosem_simple_*`` /
    ``nosem_aug_*`` without;
  * a seeded subsample (htc_inputs.sem_sample_index) of the semantic feature map of the simple view, ``sem_feat``;
  * both heads' ``state_dict`` key lists.

The JSON holds both configs' ``model.roi_head`` / ``train_cfg.rcnn`` / ``test_cfg.rcnn`` as ``registry.Config.fromfile``
resolves them.

The generator asserts what the tests need to bite on (TOL = 1e-4, the tests' relative tolerance); measured:
  coco  simple: 24 detections in 6 classes; stages differ by >= 0.938; 0.367 % of the merged probabilities within 1e-3 of the threshold
  nosem simple: 24 detections in 6 classes; stages differ by >= 0.863; 0.250 % of the merged probabilities within 1e-3 of the threshold
  simple: detections with / without the semantic head differ by inf (inf: other labels or counts; tolerance 0.0001)
  coco  aug   : 24 detections in 3 classes; stages differ by >= 0.949; 0.531 % of the merged probabilities within 1e-3 of the threshold
  nosem aug   : 24 detections in 4 classes; stages differ by >= 0.926; 0.399 % of the merged probabilities within 1e-3 of the threshold
  aug   : detections with / without the semantic head differ by inf (inf: other labels or counts; tolerance 0.0001)
("stages differ by": over the stage pairs of a view, the smallest over the detections of the largest probability difference.)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CONFIGS = {'coco': 'configs/htc/htc_r50_fpn_1x_coco.py', 'nosem': 'configs/htc/htc_without_semantic_r50_fpn_1x_coco.py'}
TOL = 1e-4


def _configs(ref):
    from dynamask_amd import registry
    out = {}
    for name, rel in CONFIGS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        out[name] = {'source': rel, 'model': {'roi_head': cfg.model.roi_head}, 'train_cfg': {'rcnn': cfg.train_cfg.rcnn},
                     'test_cfg': {'rcnn': cfg.test_cfg.rcnn}}
    return out


def load_htc_reference(ref):
    import make_golden as mg
    import make_golden_cascade as mgc
    R = mgc.load_cascade_reference(ref)
    mg._pkg('mmcv.cnn').kaiming_init = lambda m, *a, **k: None          # (the weights are seeded)
    mg._load('mmdet.models.roi_heads.mask_heads.htc_mask_head', 'mmdet/models/roi_heads/mask_heads/htc_mask_head.py')
    mg._load('mmdet.models.roi_heads.mask_heads.fused_semantic_head', 'mmdet/models/roi_heads/mask_heads/fused_semantic_head.py')
    R['htc'] = mg._load('mmdet.models.roi_heads.htc_roi_head', 'mmdet/models/roi_heads/htc_roi_head.py')
    return R


def _stage_probs(head, R, x_views, metas_views, det_bboxes, det_labels, simple):
    """The reference's own mask loop up to merge_aug_masks (htc_roi_head.py:333-354 / 507-545): the per-(view, stage)
    probabilities of each detection's class [V * stages, n, S, S] and their merge [n, S, S]."""
    aug_masks, aug_metas = [], []
    for xv, meta in zip(x_views, metas_views):
        m = meta[0]
        b = det_bboxes[:, :4] if simple else R['tr'].bbox_mapping(det_bboxes[:, :4], m['img_shape'], m['scale_factor'],
                                                                 m['flip'], m['flip_direction'])
        rois = R['tr'].bbox2roi([b])
        ext = head.mask_roi_extractor[-1]
        mask_feats = ext(xv[:len(ext.featmap_strides)], rois)
        if head.with_semantic and (not simple or 'mask' in head.semantic_fusion):
            mask_feats += head.semantic_roi_extractor([head.semantic_head(xv)[1]], rois)
        last_feat = None
        for i in range(head.num_stages):
            mask_pred, last_feat = head.mask_head[i](mask_feats, last_feat)
            aug_masks.append(mask_pred.sigmoid().cpu().numpy())
            aug_metas.append(meta)
    merged = R['ma'].merge_aug_masks(aug_masks, aug_metas, head.test_cfg)
    idx = np.arange(det_bboxes.shape[0])
    lab = det_labels.numpy()
    return np.stack([a[idx, lab] for a in aug_masks]), merged[idx, lab].astype(np.float32)


def _run(head, R, prefix):
    import htc_inputs as hi
    from make_golden_cascade import _record
    out, stats = {}, {}
    for key, simple in (('simple', True), ('aug', False)):
        if simple:
            x, props, metas = hi.simple_inputs()
            bbox_res, segm_res = head.simple_test(x, [props], metas, rescale=False)
            xs, metas_v = [x], [metas]
        else:
            xs, props, metas_v = hi.aug_inputs()
            bbox_res, segm_res = head.aug_test(xs, [props], metas_v, rescale=True)
        dets = torch.from_numpy(np.concatenate([b for b in bbox_res if len(b)], 0))
        labs = torch.tensor([c for c, b in enumerate(bbox_res) for _ in range(len(b))], dtype=torch.long)
        stages, probs = _stage_probs(head, R, xs, metas_v, dets, labs, simple)
        out.update(_record(prefix + key, bbox_res, segm_res, probs))
        # the stages of the un-flipped first view: the smallest distance between two stages' probabilities of a detection
        n = head.num_stages
        gap = min(float(np.abs(stages[i] - stages[j]).reshape(len(labs), -1).max(1).min())
                  for i in range(n) for j in range(i + 1, n))
        band = float((np.abs(probs - hi.TEST_CFG['mask_thr_binary']) < 1e-3).mean())
        stats[key] = dict(dets=len(labs), classes=len(set(labs.tolist())), stage_gap=gap, band=band)
    return out, stats


def main(ref):
    import htc_inputs as hi
    from dynamask_amd import registry
    torch.manual_seed(0)
    torch.set_num_threads(4)
    R = load_htc_reference(ref)
    cfgs = _configs(ref)
    test_cfg = registry._to_cfgdict(dict(hi.TEST_CFG))
    out, stats = {}, {}
    with torch.no_grad():
        for name, prefix in (('coco', ''), ('nosem', 'nosem_')):
            rh = dict(cfgs[name]['model']['roi_head'])
            rh.pop('type')
            head = R['htc'].HybridTaskCascadeRoIHead(test_cfg=test_cfg, train_cfg=None, **rh).eval()
            sd = head.state_dict()
            out[prefix + 'state_dict_keys'] = np.array(sorted(sd.keys()))
            mine = {k: v.shape for k, v in sd.items() if k.startswith(('bbox_head.', 'mask_head.', 'semantic_head.'))}
            head.load_state_dict(hi.head_state(mine), strict=False)
            o, stats[name] = _run(head, R, prefix)
            out.update(o)
            if name == 'coco':
                sem = head.semantic_head(hi.simple_inputs()[0])[1].numpy()
                out['sem_feat_shape'] = np.array(sem.shape, np.int64)
                out['sem_feat'] = sem.reshape(-1)[hi.sem_sample_index(sem.size)].astype(np.float32)
    lines = []
    for key in ('simple', 'aug'):
        a, b = out[f'{key}_dets'], out[f'nosem_{key}_dets']
        same = a.shape == b.shape and np.array_equal(out[f'{key}_labels'], out[f'nosem_{key}_labels'])
        fuse = float(np.abs(a - b).max()) if same else float('inf')
        scale = min(float(np.abs(a).max()), 1.0)
        for name in ('coco', 'nosem'):
            s = stats[name][key]
            lines.append(f"  {name:5s} {key:6s}: {s['dets']} detections in {s['classes']} classes; stages differ by >= "
                         f"{s['stage_gap']:.3g}; {100 * s['band']:.3f} % of the merged probabilities within 1e-3 of the threshold")
            assert s['dets'] >= 8 and s['classes'] >= 3, lines[-1]
            assert s['stage_gap'] > 10 * TOL, lines[-1]
            assert s['band'] <= 0.01, lines[-1]
        lines.append(f'  {key:6s}: detections with / without the semantic head differ by {fuse:.3g} '
                     f'(inf: other labels or counts; tolerance {TOL * scale:.3g})')
        assert fuse > 10 * TOL * (scale + float(np.abs(a).max())), lines[-1]
    print('\n'.join(lines))
    path = os.path.join(HERE, 'g22_htc.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    path = os.path.join(HERE, 'g22_htc_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_htc.py REFERENCE_ROOT')
    main(sys.argv[1])
