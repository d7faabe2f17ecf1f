"""FPN fixture from the REFERENCE's own module: tests/golden/g27_fpn*.npz and g27_fpn_configs.json.

    python tests/golden/make_golden_fpn.py REFERENCE_ROOT

Loads ``mmdet/models/necks/fpn.py`` by path under stand-ins of its own for what the file imports: a ``ConvModule`` that is
``nn.Conv2d`` + an optional ReLU and honours ``act_cfg=None`` (the neck's), ``xavier_init``, ``auto_fp16`` (the identity)
and a ``NECKS`` registry.  Builds the reference ``FPN`` from the unchanged ``model.neck`` of the three configs of
fpn_inputs.FORMS, loads fpn_inputs.head_state weights and runs it on fpn_inputs.inputs on the CPU, in float32 and in
float64.  Per form, in the file fpn_inputs.FILES names (one file per form: each stays below 1 MiB):

  ``{form}_out{l}``: output level l in float32, and ``{form}_out{l}_err16``, the float64 run's twin in
  rpn_inputs.pack_err's form (the fp32 result's error against float64, scaled, float16).

The generator ASSERTS that fpn_inputs.restate -- the torch restatement the GPU tests use where no fixture reaches -- gives
the reference's float32 outputs bit for bit, and the float64 ones too.

The JSON holds each form's ``model.neck`` as ``registry.Config.fromfile`` resolves it, the batch, and the reference
module's ``state_dict`` as a [key, shape] list; for the Mask R-CNN form also ``model.rpn_head`` / ``model.roi_head`` and
``test_cfg.rpn`` / ``test_cfg.rcnn``, the stages behind the neck."""
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


class ConvModule(nn.Module):
    """mmcv's ConvModule without norm: ``conv`` (bias) and, unless ``act_cfg`` is None, a ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type='ReLU'), inplace=True):
        super().__init__()
        assert conv_cfg is None and norm_cfg is None
        assert act_cfg is None or act_cfg['type'] == 'ReLU'
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding)
        self.activate = None if act_cfg is None else nn.ReLU(inplace=inplace)

    def forward(self, x):
        x = self.conv(x)
        return x if self.activate is None else self.activate(x)


def xavier_init(module, gain=1, bias=0, distribution='normal'):
    init = nn.init.xavier_uniform_ if distribution == 'uniform' else nn.init.xavier_normal_
    init(module.weight, gain=gain)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


def load_fpn_reference(ref):
    import make_golden as mg
    mg.REF = ref
    cnn = mg._pkg('mmcv.cnn')
    cnn.ConvModule, cnn.xavier_init = ConvModule, xavier_init
    mg._pkg('mmdet.core').auto_fp16 = mg._identity_decorator
    mg._pkg('mmdet.models.builder').NECKS = mg.Registry('neck')
    mg._pkg('mmdet.models.necks')
    return mg._load('mmdet.models.necks.fpn', 'mmdet/models/necks/fpn.py')


def _configs(ref, fi):
    from dynamask_amd import registry
    out = {}
    for form, (rel, batch) in fi.FORMS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        out[form] = {'source': rel, 'batch': batch, 'model': {'neck': cfg.model.neck}}
        if form == 'mask_rcnn':       # what follows the neck in that detector: the chain test builds it as it stands
            out[form]['model'].update(rpn_head=cfg.model.rpn_head, roi_head=cfg.model.roi_head)
            out[form]['test_cfg'] = {'rpn': cfg.test_cfg.rpn, 'rcnn': cfg.test_cfg.rcnn}
    return out


def main(ref):
    import fpn_inputs as fi
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = load_fpn_reference(ref)
    cfgs = _configs(ref, fi)
    for form, entry in cfgs.items():
        neck = dict(entry['model']['neck'])
        assert neck.pop('type') == 'FPN'
        m = mod.FPN(**neck).eval()
        m.init_weights()            # (the stand-in's xavier_init runs; the weights that count are head_state's)
        sd = m.state_dict()
        state = fi.head_state({k: v.shape for k, v in sd.items()}, fi.WEIGHT_SEED)
        m.load_state_dict(state, strict=True)
        xs = fi.inputs(neck['in_channels'], entry['batch'])
        with torch.no_grad():
            out32 = m(xs)
            m.double()
            out64 = m([x.double() for x in xs])
            m.float()
            mine32 = fi.restate(entry['model']['neck'], state, xs)
            mine64 = fi.restate(entry['model']['neck'], state, [x.double() for x in xs])
        assert len(out32) == neck['num_outs'] == len(mine32)
        out = {}
        for l, (a, b, c, d) in enumerate(zip(out32, out64, mine32, mine64)):
            assert a.dtype == torch.float32 and b.dtype == torch.float64
            assert torch.equal(a, c), f'{form} level {l}: the restatement is not the reference in float32'
            assert torch.equal(b, d), f'{form} level {l}: the restatement is not the reference in float64'
            assert bool(torch.isfinite(a).all()) and float(a.std()) > 0.1
            out[f'{form}_out{l}'] = a.numpy()
            out[f'{form}_out{l}_err16'] = fi.pack_err(a.numpy(), b.numpy())
        print(form, {k: (v.shape, str(v.dtype)) for k, v in out.items()})
        path = os.path.join(HERE, fi.FILES[form])
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print('wrote', path, size, 'bytes')
        assert size < (1 << 20), 'a committed file stays below 1 MiB'
        entry['state_dict'] = [[k, list(sd[k].shape)] for k in sd]
    path = os.path.join(HERE, 'g27_fpn_configs.json')
    with open(path, 'w') as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_fpn.py REFERENCE_ROOT')
    main(sys.argv[1])
