"""Initial-state digest of every model section the registry can build on the CPU: what
tests/golden/module_init_digest.json holds and tests/test_layering_cpu.py compares against.

Per section: ``torch.manual_seed(0)``, build through ``registry``, ``init_weights()`` where the class has it, then the
ordered ``state_dict`` keys with their shapes and one SHA-256 over the tensors' bytes.  A change of a single random draw,
of the order of two constructors or of a key shows as another digest.  The sections are every ``model`` entry of
tests/golden/*_configs.json that holds parts (ResNet at depth 50 only; a whole detector's entry, whose ``model`` has a
``type``, repeats parts recorded from the per-part fixtures and is left out) and the RoI heads of ``synth``'s config values.

    python tools/module_digest.py            # print the digests as JSON
    python tools/module_digest.py --write    # store them in tests/golden/module_init_digest.json
"""
import glob
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURE = os.path.join(GOLDEN, 'module_init_digest.json')


def _register():
    from dynamask_amd import (backbones, bbox_heads, dense_heads, losses, mask_heads, necks,  # noqa: F401
                              roi_extractors, roi_head, shared_heads)


def _rcnn(cfg, key):
    """``train_cfg.rcnn`` / ``test_cfg.rcnn`` of a stored config, None where the fixture has none."""
    part = cfg.get(key)
    return None if part is None else part.get('rcnn')


def sections():
    """[(name, builder)], in a fixed order; a builder returns the module, built from a fresh copy of its config."""
    from dynamask_amd import registry, synth
    _register()
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, '*_configs.json'))):
        stem = os.path.basename(path)[:-len('_configs.json')]
        with open(path) as f:
            named = json.load(f)
        for name in sorted(named):
            if 'type' in named[name]['model']:
                continue                    # a whole detector (g29): its sections are the per-part fixtures' above
            for part in sorted(named[name]['model']):
                if part == 'backbone' and named[name]['model'][part].get('depth') != 50:
                    continue

                def make(raw=named[name], part=part):
                    cfg = registry._to_cfgdict(raw)
                    sec = dict(cfg.model[part])
                    if part == 'roi_head':
                        sec.update(train_cfg=_rcnn(cfg, 'train_cfg'), test_cfg=_rcnn(cfg, 'test_cfg'))
                        return registry.build_head(sec)
                    if part == 'rpn_head':
                        sec.update(train_cfg=None, test_cfg=cfg.test_cfg.rpn)
                        return registry.build_head(sec)
                    return {'neck': registry.build_neck, 'backbone': registry.build_backbone}[part](sec)
                out.append((f'{stem}/{name}/{part}', make))
    C = registry.ConfigDict
    out.append(('synth/dynamask_roi_head', lambda: registry.build_head(dict(
        type='DynaMaskRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG),
        train_cfg=C(**synth.RCNN_TRAIN_CFG), test_cfg=C(**synth.RCNN_TEST_CFG)))))
    out.append(('synth/standard_roi_head', lambda: registry.build_head(dict(
        type='StandardRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
        bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
        mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
        mask_head=dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG),
        train_cfg=C(**synth.RCNN_TRAIN_CFG), test_cfg=C(**synth.RCNN_TEST_CFG)))))
    return out


def digest(make):
    torch.manual_seed(0)
    m = make()
    if hasattr(m, 'init_weights'):
        m.init_weights()
    h = hashlib.sha256()
    keys = []
    for k, v in m.state_dict().items():
        t = v.detach().cpu().contiguous()
        keys.append([k, list(t.shape)])
        h.update(k.encode())
        h.update(str(t.dtype).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return dict(keys=keys, sha256=h.hexdigest())


def all_digests():
    return {name: digest(make) for name, make in sections()}


if __name__ == '__main__':
    d = all_digests()
    if '--write' in sys.argv:
        with open(FIXTURE, 'w') as f:       # one section per line
            f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(d[k])}' for k in sorted(d)) + '\n}\n')
        print(f'{len(d)} sections -> {FIXTURE}')
    else:
        json.dump(d, sys.stdout, indent=1, sort_keys=True)
