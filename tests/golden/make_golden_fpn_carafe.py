"""FPN_CARAFE fixture from the REFERENCE's own module: tests/golden/g32_fpn_carafe*.npz and g32_fpn_carafe_configs.json.

    python tests/golden/make_golden_fpn_carafe.py REFERENCE_ROOT

Loads ``mmdet/models/necks/fpn_carafe.py`` by path behind the existing stand-ins for what the file imports:
make_golden_fpn's ``ConvModule`` (here also taking the ``bias=True`` and ``order=('conv', 'norm', 'act')`` the file passes)
and ``xavier_init``, make_golden's ``CARAFEPack`` / ``build_upsample_layer`` (the operator is oracle.ref_ops's) and a
``NECKS`` registry.  Builds the reference ``FPN_CARAFE`` from the unchanged ``model.neck`` of
fpn_carafe_inputs.NECK_CONFIG, loads fpn_carafe_inputs.head_state weights and runs it on fpn_carafe_inputs.inputs on the
CPU, in float32 and in float64.  In the files fpn_carafe_inputs.FILES names (each below 1 MiB):

  ``out{l}``: output level l in float32, and ``out{l}_err16``, the float64 run's twin in rpn_inputs.pack_err's form;
  ``mean_max_tap`` (in the first file): the mean over all top-down steps' output pixels of the largest normalised tap.

The generator ASSERTS that fpn_carafe_inputs.restate gives the reference's outputs bit for bit in float32 and in float64,
that fpn_carafe_inputs.state_shapes is the reference module's key list with its shapes in order, that every output is
finite with a standard deviation above 0.1, and that ``mean_max_tap`` is above 2 / 25: the normalised kernels are far
from uniform, so a box filter in CARAFE's place would fail the tests.

The JSON holds one entry per whole detector of fpn_carafe_inputs.DETECTORS and none of the neck alone: the resolved
``model.neck`` is the one inside each detector's ``model`` (asserted equal in both; the run above was built from it).  Per
entry: the whole ``model`` dict, ``test_cfg`` (``rpn`` and ``rcnn``), ``test_pipeline``, ``neck_state_dict`` (the
reference module's ``state_dict`` as a [key, shape] list in order), ``neck_batch`` and the key list composed as g30 / g31
compose it: ``state_dict`` = the ResNet-50's keys under ``backbone.`` as g28_backbone_configs.json records them from the
reference's module (the generator asserts that the config has the very backbone those were recorded for), the reference
FPN_CARAFE's under ``neck.`` and the RPN head's under ``rpn_head.`` as g26_rpn_configs.json records them (asserted: the
same ``rpn_head``), each with its shape, in order; ``roi_head_keys``: null (the StandardRoIHead of both detectors, whose
keys the tests pin through the fixtures that record them)."""
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
    return json.loads(json.dumps(x))


def load_fpn_carafe_reference(ref):
    import make_golden as mg
    import make_golden_fpn as mgf

    class ConvModule(mgf.ConvModule):
        def __init__(self, *a, bias=True, order=('conv', 'norm', 'act'), **k):
            assert bias is True and tuple(order) == ('conv', 'norm', 'act')
            super().__init__(*a, **k)

    mg.REF = ref
    cnn = mg._pkg('mmcv.cnn')
    cnn.ConvModule, cnn.xavier_init, cnn.build_upsample_layer = ConvModule, mgf.xavier_init, mg.build_upsample_layer
    mg._pkg('mmcv.ops')
    mg._pkg('mmcv.ops.carafe').CARAFEPack = mg.CARAFEPack
    mg._pkg('mmdet.models.builder').NECKS = mg.Registry('neck')
    mg._pkg('mmdet.models.necks')
    return mg._load('mmdet.models.necks.fpn_carafe', 'mmdet/models/necks/fpn_carafe.py')


def main(ref):
    import fpn_carafe_inputs as ci
    from dynamask_amd import registry
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = load_fpn_carafe_reference(ref)
    neck_cfg = registry.Config.fromfile(os.path.join(ref, ci.NECK_CONFIG)).model.neck
    neck = dict(neck_cfg)
    assert neck.pop('type') == 'FPN_CARAFE'
    neck['in_channels'] = list(neck['in_channels'])
    m = mod.FPN_CARAFE(**neck).eval()
    m.init_weights()                # (the stand-ins' initialisers run; the weights that count are head_state's)
    sd = m.state_dict()
    keys = [[k, list(sd[k].shape)] for k in sd]
    assert keys == [[k, list(s)] for k, s in ci.state_shapes(neck_cfg).items()], 'state_shapes is not the reference'
    state = ci.head_state({k: v.shape for k, v in sd.items()}, ci.WEIGHT_SEED)
    m.load_state_dict(state, strict=True)
    xs = ci.inputs(neck['in_channels'], ci.BATCH, seed=ci.FEAT_SEED)
    before = [x.clone() for x in xs]
    with torch.no_grad():
        out32 = m(xs)
        m.double()
        out64 = m([x.double() for x in xs])
        m.float()
        mine32, steps = ci.restate(neck_cfg, state, xs, every_level=True)
        mine64 = ci.restate(neck_cfg, state, [x.double() for x in xs])
    assert all(torch.equal(a, b) for a, b in zip(xs, before))
    assert len(out32) == neck['num_outs'] == len(mine32) == len(ci.FILES) and len(steps) == len(out32) - 1
    assert [tuple(o.shape[2:]) for o in out32] == list(ci.STAGE_SIZES) + [(2, 2)]
    # the normalised kernels are far from uniform
    tops = torch.cat([ci.normalised_kernels(s['enc'], 5, 1).view(ci.BATCH, 1, 25, -1).max(dim=2).values.flatten() for s in steps])
    mean_max = float(tops.mean())
    print('mean of the largest tap weight %.4f over %d output pixels (uniform: %.4f)' % (mean_max, tops.numel(), 1 / 25))
    assert mean_max > 2 / 25
    files = {}
    for l, (a, b, c, d) in enumerate(zip(out32, out64, mine32, mine64)):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.equal(a, c), f'level {l}: the restatement is not the reference in float32'
        assert torch.equal(b, d), f'level {l}: the restatement is not the reference in float64'
        assert bool(torch.isfinite(a).all()) and float(a.std()) > 0.1
        print(l, tuple(a.shape), 'std %.3g' % float(a.std()), 'fp32 err %.3g' % float((a.double() - b).abs().max()))
        out = files.setdefault(ci.FILES[l], {})
        out[f'out{l}'] = a.numpy()
        out[f'out{l}_err16'] = ci.pack_err(a.numpy(), b.numpy())
    files[ci.FILES[0]]['mean_max_tap'] = np.float64(mean_max)
    for name, out in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        print('wrote', path, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < (1 << 20), 'a committed file stays below 1 MiB'

    # ---- the configs
    cfgs = {}
    backbone, rpn = _load_json('g28_backbone_configs.json')['pytorch'], _load_json('g26_rpn_configs.json')['fpn']
    for name, (rel, typ) in ci.DETECTORS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        assert cfg.model['type'] == typ and set(cfg.test_cfg) >= {'rpn', 'rcnn'}
        assert _plain(cfg.model.neck) == _plain(neck_cfg), name
        assert _plain(cfg.model.backbone) == backbone['model']['backbone'], name
        assert _plain(cfg.model.rpn_head) == rpn['model']['rpn_head'], name
        composed = [['backbone.' + k, s] for k, s in backbone['state_dict']]
        cfgs[name] = {'source': rel, 'model': cfg.model, 'test_cfg': {'rpn': cfg.test_cfg.rpn, 'rcnn': cfg.test_cfg.rcnn},
                      'test_pipeline': cfg.test_pipeline, 'state_dict': composed + [['neck.' + k, s] for k, s in keys]
                      + [['rpn_head.' + k, s] for k, s in rpn['state_dict']], 'roi_head_keys': None,
                      'neck_state_dict': keys, 'neck_batch': ci.BATCH}
    path = os.path.join(HERE, ci.CONFIGS)
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=None, sort_keys=True, separators=(',', ':'))
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20), 'a committed file stays below 1 MiB'


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_fpn_carafe.py REFERENCE_ROOT')
    main(sys.argv[1])
