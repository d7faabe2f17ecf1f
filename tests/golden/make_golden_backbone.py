"""Backbone fixture from the REFERENCE's own module: tests/golden/g28_backbone*.npz and g28_backbone_configs.json.

    python tests/golden/make_golden_backbone.py REFERENCE_ROOT

Loads ``mmdet/models/backbones/resnet.py`` by path through make_golden_c4.load_c4_reference (the stand-ins of
make_golden.py / make_golden_double.py for what the file imports).  Builds the reference ``ResNet`` from the unchanged
``model.backbone`` of the two configs of backbone_inputs.FORMS, in ``eval()``, loads backbone_inputs.head_state weights
and runs it on backbone_inputs.inputs() on the CPU, in float32 and in float64.  Per form, in the file
backbone_inputs.FILES names (one file per form: each stays below 1 MiB):

  ``{form}_out{l}``: output l (of ``out_indices``) in float32, and ``{form}_out{l}_err16``, the float64 run's twin in
  rpn_inputs.pack_err's form (the fp32 result's error against float64, scaled, float16).

The generator ASSERTS that every stored output is finite with a standard deviation above 0.1, and that
backbone_inputs.restate -- the torch restatement the GPU tests use where no fixture reaches -- gives the reference's
outputs bit for bit, in float32 and in float64.

The JSON holds, per form, ``model.backbone`` as ``registry.Config.fromfile`` resolves it, the batch and the reference
module's ``state_dict`` as a [key, shape] list; the ``*_r101`` entries (the same dicts at ``depth=101``) hold config and
keys only, for the build and key tests.  The Mask R-CNN FPN form also carries ``model.neck`` / ``rpn_head`` / ``roi_head``
and ``test_cfg``, the stages behind the backbone."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def _configs(ref, bi):
    from dynamask_amd import registry
    out = {}
    for form, (rel, rel101) in bi.FORMS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        out[form] = {'source': rel, 'batch': bi.BATCH, 'model': {'backbone': cfg.model.backbone}}
        if form == 'pytorch':       # what follows the backbone in that detector: the chain test builds it as it stands
            out[form]['model'].update(neck=cfg.model.neck, rpn_head=cfg.model.rpn_head, roi_head=cfg.model.roi_head)
            out[form]['test_cfg'] = {'rpn': cfg.test_cfg.rpn, 'rcnn': cfg.test_cfg.rcnn}
        if rel101 is not None:
            b101 = registry.Config.fromfile(os.path.join(ref, rel101)).model.backbone
        else:                       # (the reference has no depth-101 C4 config: the depth is the one key that differs)
            b101 = dict(cfg.model.backbone, depth=101)
        assert b101['depth'] == 101 and {k: v for k, v in b101.items() if k != 'depth'} == \
            {k: v for k, v in cfg.model.backbone.items() if k != 'depth'}
        out[form + '_r101'] = {'source': rel101 or rel, 'model': {'backbone': b101}}
    return out


def _ref_module(R, backbone):
    cfg = dict(backbone)
    assert cfg.pop('type') == 'ResNet'
    m = R['resnet'].ResNet(**cfg)
    m.eval()            # (the reference's train() override returns nothing)
    assert not m.training and not m.bn1.training and not m.layer1[0].bn3.training
    return m


def main(ref):
    import backbone_inputs as bi
    import make_golden_c4 as mgc
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = mgc.load_c4_reference(ref)
    # resnet.py was loaded (for its Bottleneck) before the reference's ResLayer was: its ResNet gets the real one now
    R['resnet'].ResLayer = sys.modules['mmdet.models.utils'].ResLayer
    cfgs = _configs(ref, bi)
    img = bi.inputs()
    for form in bi.FORMS:
        entry = cfgs[form]
        backbone = entry['model']['backbone']
        m = _ref_module(R, backbone)
        sd = m.state_dict()
        state = bi.head_state({k: v.shape for k, v in sd.items()}, bi.WEIGHT_SEED)
        m.load_state_dict(state, strict=True)
        with torch.no_grad():
            out32 = m(img.clone())
            m.double()
            out64 = m(img.double())
            m.float()
            mine32 = bi.restate(backbone, state, img)
            mine64 = bi.restate(backbone, state, img.double())
        assert len(out32) == len(backbone['out_indices']) == len(mine32)
        out = {}
        for l, (a, b, c, d) in enumerate(zip(out32, out64, mine32, mine64)):
            assert a.dtype == torch.float32 and b.dtype == torch.float64
            assert torch.equal(a, c), f'{form} output {l}: the restatement is not the reference in float32'
            assert torch.equal(b, d), f'{form} output {l}: the restatement is not the reference in float64'
            assert bool(torch.isfinite(a).all()) and float(a.std()) > 0.1
            print(form, l, tuple(a.shape), 'std %.3g' % float(a.std()), 'max %.3g' % float(a.abs().max()),
                  'zeros %.2f' % float((a == 0).float().mean()), 'fp32 err %.3g' % float((a.double() - b).abs().max()))
            out[f'{form}_out{l}'] = a.numpy()
            out[f'{form}_out{l}_err16'] = bi.pack_err(a.numpy(), b.numpy())
        path = os.path.join(HERE, bi.FILES[form])
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print('wrote', path, size, 'bytes')
        assert size < (1 << 20), 'a committed file stays below 1 MiB'
        entry['state_dict'] = [[k, list(sd[k].shape)] for k in sd]
        sd101 = _ref_module(R, cfgs[form + '_r101']['model']['backbone']).state_dict()
        cfgs[form + '_r101']['state_dict'] = [[k, list(sd101[k].shape)] for k in sd101]
    path = os.path.join(HERE, 'g28_backbone_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_backbone.py REFERENCE_ROOT')
    main(sys.argv[1])
