"""Res2Net fixture from the REFERENCE's own module: tests/golden/g31_res2net.npz and g31_res2net_configs.json.

    python tests/golden/make_golden_res2net.py REFERENCE_ROOT

Loads ``mmdet/models/backbones/res2net.py`` by path behind make_golden_c4.load_c4_reference (the stand-ins of
make_golden.py / make_golden_double.py for what the file imports).  Builds the reference ``Res2Net`` from the unchanged
``model.backbone`` of res2net_inputs.RUN_CONFIG, in ``eval()``, loads backbone_inputs.head_state weights and runs it on
backbone_inputs.inputs() on the CPU (the module is pure torch), in float32 and in float64:

  ``r2_101_out{l}``: output l (of ``out_indices``) in float32, and ``r2_101_out{l}_err16``, the float64 run's twin in
  rpn_inputs.pack_err's form.

The generator ASSERTS that every stored output is finite with a standard deviation above 0.1, that
res2net_inputs.restate gives the reference's outputs bit for bit, in float32 and in float64, and that
res2net_inputs.state_shapes names the reference's keys and shapes in order.

The JSON holds
  * ``r2_101``: ``model`` with ONLY ``backbone`` as ``registry.Config.fromfile`` resolves it, ``source``, ``batch`` and
    the reference module's ``state_dict`` as a [key, shape] list in order;
  * per whole detector of res2net_inputs.DETECTORS (the five configs of configs/res2net/): the whole ``model`` dict with
    its ``type`` and ``pretrained``, ``test_cfg`` (``rpn`` and ``rcnn``) and the key list, composed as g30 composes it:
    the reference ``Res2Net``'s keys under ``backbone.`` -- stored ONCE, as ``r2_101``'s ``state_dict``: the five configs
    have the same backbone (asserted) --, followed by ``state_dict_behind_backbone``, the neck's and the RPN head's as
    g27_fpn_configs.json / g26_rpn_configs.json record them from the reference's modules (the generator asserts that the config has the very
    ``neck`` / ``rpn_head`` those were recorded for, the loss settings apart), each with its shape, in order;
    ``roi_head_keys``: the reference RoI head's sorted keys where a fixture records them for the same ``roi_head`` config
    (g21_cascade.npz, g22_htc.npz: asserted equal configs), else null (the StandardRoIHead of Mask R-CNN and Faster
    R-CNN and the box-only CascadeRoIHead, whose keys the tests pin through the detectors other fixtures record)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def _load_json(name):
    with open(os.path.join(HERE, name)) as f:
        return json.load(f)


def _plain(x):
    """A resolved config as JSON stores it (tuples become lists), for comparisons with stored fixtures."""
    return json.loads(json.dumps(x))


def _ref_module(X, backbone):
    cfg = dict(backbone)
    assert cfg.pop('type') == 'Res2Net'
    m = X.Res2Net(**cfg)
    m.eval()            # (the reference's train() override returns nothing)
    blk = m.layer1[0]
    assert not m.training and not m.stem[1].training and not blk.bn3.training and not blk.bns[0].training
    assert isinstance(blk, X.Bottle2neck) and blk.stage_type == 'stage' and m.layer1[1].stage_type == 'normal'
    assert m.deep_stem and m.avg_down and not hasattr(m, 'conv1') and not hasattr(blk, 'conv2')
    assert (blk.scales, blk.width) == (backbone.get('scales', 4), backbone.get('base_width', 26))
    return m


def _roi_head_keys(name, roi_head):
    """The recorded reference key list for this ``roi_head`` config, or None."""
    recorded = {'CascadeRoIHead': ('g21_cascade_configs.json', 'coco', 'g21_cascade.npz', 'state_dict_keys'),
                'HybridTaskCascadeRoIHead': ('g22_htc_configs.json', 'coco', 'g22_htc.npz', 'state_dict_keys')}
    if roi_head['type'] not in recorded or 'mask_head' not in roi_head:
        return None
    cfg_file, entry, npz, key = recorded[roi_head['type']]
    assert _plain(roi_head) == _load_json(cfg_file)[entry]['model']['roi_head'], f'{name}: another roi_head than {cfg_file} records'
    return [str(k) for k in np.load(os.path.join(HERE, npz))[key]]


def main(ref):
    import make_golden as mg
    import make_golden_c4 as mgc
    import res2net_inputs as xi
    from dynamask_amd import registry
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = mgc.load_c4_reference(ref)
    R['resnet'].ResLayer = sys.modules['mmdet.models.utils'].ResLayer
    X = mg._load('mmdet.models.backbones.res2net', 'mmdet/models/backbones/res2net.py')
    assert X.ResNet is R['resnet'].ResNet

    cfgs, keys = {}, {}
    backbone = registry.Config.fromfile(os.path.join(ref, xi.RUN_CONFIG)).model.backbone
    assert backbone['type'] == 'Res2Net' and backbone['depth'] == 101 and (backbone['scales'], backbone['base_width']) == (4, 26)
    m = _ref_module(X, backbone)
    sd = m.state_dict()
    keys[_plain_key(backbone)] = [[k, list(sd[k].shape)] for k in sd]
    assert keys[_plain_key(backbone)] == [[k, list(s)] for k, s in xi.state_shapes(backbone).items()], 'state_shapes is not the reference'
    cfgs[xi.RUN] = {'source': xi.RUN_CONFIG, 'model': {'backbone': backbone}, 'state_dict': keys[_plain_key(backbone)], 'batch': xi.BATCH}

    # ---- the run
    state = xi.head_state({k: v.shape for k, v in sd.items()}, xi.WEIGHT_SEED)
    m.load_state_dict(state, strict=True)
    img = xi.inputs()
    with torch.no_grad():
        out32 = m(img.clone())
        m.double()
        out64 = m(img.double())
        m.float()
        mine32 = xi.restate(backbone, state, img)
        mine64 = xi.restate(backbone, state, img.double())
    assert len(out32) == len(backbone['out_indices']) == len(mine32)
    out = {}
    for l, (a, b, c, d) in enumerate(zip(out32, out64, mine32, mine64)):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(a, c), f'output {l}: the restatement is not the reference in float32'
        assert torch.equal(b, d), f'output {l}: the restatement is not the reference in float64'
        assert bool(torch.isfinite(a).all()) and float(a.std()) > 0.1
        print(xi.RUN, l, tuple(a.shape), 'std %.3g' % float(a.std()), 'max %.3g' % float(a.abs().max()),
              'zeros %.2f' % float((a == 0).float().mean()), 'fp32 err %.3g' % float((a.double() - b).abs().max()))
        out[f'{xi.RUN}_out{l}'] = a.numpy()
        out[f'{xi.RUN}_out{l}_err16'] = xi.pack_err(a.numpy(), b.numpy())
    path = os.path.join(HERE, xi.FILE)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20), 'a committed file stays below 1 MiB'

    # ---- whole detectors
    fpn, rpn = _load_json('g27_fpn_configs.json')['mask_rcnn'], _load_json('g26_rpn_configs.json')['fpn']
    for name, (rel, typ) in xi.DETECTORS.items():
        assert name not in cfgs
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        assert cfg.model['type'] == typ and cfg.model.backbone['type'] == 'Res2Net' and set(cfg.test_cfg) >= {'rpn', 'rcnn'}

        def no_loss(d):      # (the cascade configs train the RPN with another loss: no parameter hangs on it)
            return {k: v for k, v in d.items() if not k.startswith('loss')}
        assert _plain(cfg.model.neck) == fpn['model']['neck'], name
        assert no_loss(_plain(cfg.model.rpn_head)) == no_loss(rpn['model']['rpn_head']), name
        bk = _plain_key(cfg.model.backbone)
        if bk not in keys:
            sdn = _ref_module(X, cfg.model.backbone).state_dict()
            keys[bk] = [[k, list(sdn[k].shape)] for k in sdn]
        assert keys[bk] == cfgs[xi.RUN]['state_dict'], f'{name}: another backbone than {xi.RUN}'
        behind = [['neck.' + k, s] for k, s in fpn['state_dict']] + [['rpn_head.' + k, s] for k, s in rpn['state_dict']]
        cfgs[name] = {'source': rel, 'model': cfg.model, 'test_cfg': {'rpn': cfg.test_cfg.rpn, 'rcnn': cfg.test_cfg.rcnn},
                      'state_dict_behind_backbone': behind, 'roi_head_keys': _roi_head_keys(name, _plain(cfg.model.roi_head))}
    path = os.path.join(HERE, xi.CONFIGS)
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=None, sort_keys=True, separators=(',', ':'))
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20), 'a committed file stays below 1 MiB'


def _plain_key(backbone):
    """A hashable form of a backbone config: equal configs share one reference module's key list."""
    return json.dumps(_plain(backbone), sort_keys=True)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_res2net.py REFERENCE_ROOT')
    main(sys.argv[1])
