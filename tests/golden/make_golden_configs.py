"""The sections of the reference's configs that tests/test_host_cpu.py builds heads from, resolved by the product's own
``registry.Config.fromfile`` (``_base_`` chain merged) and stored as data: tests/golden/g15_configs.json.

    configs/dynamask/coco/r50-dynamask-1x.py                  -> "dynamask"   (BASELINE configs[1..3])
    configs/carafe/mask_rcnn_r50_fpn_carafe_1x_coco.py        -> "carafe"     (BASELINE configs[4], two ``_base_`` levels)

Each entry holds ``model.roi_head``, ``train_cfg.rcnn`` and ``test_cfg.rcnn`` under their config paths.  Run ONLY where
the reference tree exists:  python tests/golden/make_golden_configs.py REFERENCE_ROOT"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from dynamask_amd import registry  # noqa: E402

CONFIGS = {'dynamask': 'configs/dynamask/coco/r50-dynamask-1x.py',
           'carafe': 'configs/carafe/mask_rcnn_r50_fpn_carafe_1x_coco.py'}


def main(ref):
    out = {}
    for name, rel in CONFIGS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        out[name] = {'source': rel, 'model': {'roi_head': cfg.model.roi_head},
                     'train_cfg': {'rcnn': cfg.train_cfg.rcnn}, 'test_cfg': {'rcnn': cfg.test_cfg.rcnn}}
    path = os.path.join(HERE, 'g15_configs.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_configs.py REFERENCE_ROOT')
    main(sys.argv[1])
