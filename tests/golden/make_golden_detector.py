"""Whole-detector configs: tests/golden/g29_detector_configs.json.

    python tests/golden/make_golden_detector.py REFERENCE_ROOT

Per detector of CONFIGS, what ``registry.Config.fromfile`` resolves from the reference's unchanged config file: the whole
``model`` dict (``type`` and ``pretrained`` included -- the keys the per-part fixtures g15 .. g28 leave out), ``test_cfg``
(``rpn`` and ``rcnn``), ``test_pipeline`` and ``img_norm_cfg``.  Settings only: nothing is computed and no module of the
reference is loaded.  JSON turns the tuples (``img_scale``, ``out_indices``) into lists; the package reads either."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CONFIGS = {
    'dynamask': 'configs/dynamask/coco/r50-dynamask-1x.py',
    'mask_rcnn': 'configs/mask_rcnn/mask_rcnn_r50_fpn_1x_coco.py',
    'mask_c4': 'configs/mask_rcnn/mask_rcnn_r50_caffe_c4_1x_coco.py',
    'faster_c4': 'configs/faster_rcnn/faster_rcnn_r50_caffe_c4_1x_coco.py',
    'cascade': 'configs/cascade_rcnn/cascade_mask_rcnn_r50_fpn_1x_coco.py',
    'htc': 'configs/htc/htc_r50_fpn_1x_coco.py',
    'msrcnn': 'configs/ms_rcnn/ms_rcnn_r50_fpn_1x_coco.py',
    'pointrend': 'configs/point_rend/point_rend_r50_caffe_fpn_mstrain_1x_coco.py',
    'grid': 'configs/grid_rcnn/grid_rcnn_r50_fpn_gn-head_1x_coco.py',
    'double': 'configs/double_heads/dh_faster_rcnn_r50_fpn_1x_coco.py',
}
# model.type of each, as the reference's files name it (asserted: a changed config is noticed here)
TYPES = dict(dynamask='MaskRCNN', mask_rcnn='MaskRCNN', mask_c4='MaskRCNN', faster_c4='FasterRCNN', cascade='CascadeRCNN',
             htc='HybridTaskCascade', msrcnn='MaskScoringRCNN', pointrend='PointRend', grid='GridRCNN', double='FasterRCNN')


def main(ref):
    from dynamask_amd import registry
    out = {}
    for name, rel in CONFIGS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        assert cfg.model['type'] == TYPES[name], (name, cfg.model['type'])
        assert set(cfg.test_cfg) >= {'rpn', 'rcnn'}
        out[name] = {'source': rel, 'model': cfg.model, 'test_cfg': {'rpn': cfg.test_cfg.rpn, 'rcnn': cfg.test_cfg.rcnn},
                     'test_pipeline': cfg.test_pipeline, 'img_norm_cfg': cfg.img_norm_cfg}
    path = os.path.join(HERE, 'g29_detector_configs.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_detector.py REFERENCE_ROOT')
    main(sys.argv[1])
