"""Forms and torch restatement of the Res2Net fixture (g31_res2net.npz, g31_res2net_configs.json), shared by
tests/golden/make_golden_res2net.py and the tests.  The images, the seeded weights and the error twins' form are the
backbone fixture's (backbone_inputs.inputs / head_state, rpn_inputs.pack_err): nothing of those files changes.
``restate_stem`` / ``restate_stage`` / ``restate`` restate the reference's ``Res2Net`` forward in plain torch (BatchNorm NOT
folded; ``split`` / ``cat`` as the reference makes them); the generator asserts that they give the reference's module bit
for bit on the CPU, in float32 and in float64.

The images are 2 x 3 x 37 x 53: the deep stem gives 19 x 27 and the max-pool 10 x 14, so C2 is 10 x 14, C3 5 x 7, C4 3 x 4
and C5 2 x 2: the stride-2 sliced convolutions, 3x3 average pools and ceil-mode 2x2 average pools of layers 2, 3 and 4 meet
an even, an odd and an even size (5 x 7 -> 3 x 4 has edge windows of one and two elements)."""
import torch
import torch.nn.functional as F

from backbone_inputs import (BATCH, IMG_H, IMG_SEED, IMG_W, STAGE_BLOCKS, WEIGHT_SEED, _bn, _params, head_state, inputs,  # noqa: F401
                             pack_err, resolve, unpack_f64)

# the backbone that is run: ``model.backbone`` of this config (all five configs have the same one)
RUN = 'r2_101'
RUN_CONFIG = 'configs/res2net/mask_rcnn_r2_101_fpn_2x_coco.py'
# whole detectors: name -> (config, model.type)
DETECTORS = {'mask_rcnn_r2_101': ('configs/res2net/mask_rcnn_r2_101_fpn_2x_coco.py', 'MaskRCNN'),
             'cascade_mask_rcnn_r2_101': ('configs/res2net/cascade_mask_rcnn_r2_101_fpn_20e_coco.py', 'CascadeRCNN'),
             'htc_r2_101': ('configs/res2net/htc_r2_101_fpn_20e_coco.py', 'HybridTaskCascade'),
             'faster_rcnn_r2_101': ('configs/res2net/faster_rcnn_r2_101_fpn_2x_coco.py', 'FasterRCNN'),
             'cascade_rcnn_r2_101': ('configs/res2net/cascade_rcnn_r2_101_fpn_20e_coco.py', 'CascadeRCNN')}
FILE = 'g31_res2net.npz'
CONFIGS = 'g31_res2net_configs.json'


def scales_of(backbone):
    return int(dict(backbone).get('scales', 4))


def widths(backbone):
    """Channels per scale and stage: res2net.py:31."""
    cfg = dict(backbone)
    bw, bc = cfg.get('base_width', 26), cfg.get('base_channels', 64)
    return [bc * 2 ** i * bw // bc for i in range(cfg.get('num_stages', 4))]


def restate_stem(state, img):
    """The deep stem (resnet.py:525-557) and the max-pool."""
    p = _params(state, img)
    x = F.relu(_bn(F.conv2d(img, p['stem.0.weight'], stride=2, padding=1), p, 'stem.1'))
    x = F.relu(_bn(F.conv2d(x, p['stem.3.weight'], padding=1), p, 'stem.4'))
    x = F.relu(_bn(F.conv2d(x, p['stem.6.weight'], padding=1), p, 'stem.7'))
    return F.max_pool2d(x, 3, stride=2, padding=1)


def restate_stage(backbone, state, i, x):
    """Stage ``i`` (``layer{i + 1}``) on its input ``x``, in the reference's order of operations (res2net.py:104-158)."""
    r = resolve(backbone)
    s, w = scales_of(backbone), widths(backbone)[i]
    p = _params(state, x)
    for j in range(r['blocks'][i]):
        pre = f'layer{i + 1}.{j}'
        stride = r['strides'][i] if j == 0 else 1
        out = F.relu(_bn(F.conv2d(x, p[pre + '.conv1.weight']), p, pre + '.bn1'))
        spx = torch.split(out, w, 1)
        sp = F.relu(_bn(F.conv2d(spx[0].contiguous(), p[pre + '.convs.0.weight'], stride=stride, padding=1), p, pre + '.bns.0'))
        out = sp
        for k in range(1, s - 1):
            sp = spx[k] if j == 0 else sp + spx[k]
            sp = F.relu(_bn(F.conv2d(sp.contiguous(), p[pre + f'.convs.{k}.weight'], stride=stride, padding=1), p, pre + f'.bns.{k}'))
            out = torch.cat((out, sp), 1)
        if j != 0 or stride == 1:
            out = torch.cat((out, spx[s - 1]), 1)
        else:
            out = torch.cat((out, F.avg_pool2d(spx[s - 1], 3, stride, 1)), 1)
        out = _bn(F.conv2d(out, p[pre + '.conv3.weight']), p, pre + '.bn3')
        identity = x
        if pre + '.downsample.1.weight' in p:
            identity = F.avg_pool2d(x, stride, stride, ceil_mode=True, count_include_pad=False)
            identity = _bn(F.conv2d(identity, p[pre + '.downsample.1.weight']), p, pre + '.downsample.2')
        out += identity
        x = F.relu(out)
    return x


def restate(backbone, state, img, every_stage=False):
    """The backbone's outputs for ``img`` with the parameters ``state`` (keys of Res2Net.state_dict), in the dtype and on
    the device of ``img``.  ``every_stage``: (the stem's output, [every stage's output]) instead of the ``out_indices``."""
    r = resolve(backbone)
    stem = restate_stem(state, img)
    x, stages = stem, []
    for i in range(len(r['blocks'])):
        x = restate_stage(backbone, state, i, x)
        stages.append(x)
    if every_stage:
        return stem, stages
    return tuple(stages[i] for i in range(len(stages)) if i in r['out_indices'])


def state_shapes(backbone):
    """{key: shape} of the reference ``Res2Net``'s ``state_dict`` for a backbone config (``type`` may be present), in the
    reference's order: in a block conv1, bn1, conv3, bn3, the downsample path, then ``convs`` and ``bns`` (the reference
    builds them after its parent class built the rest)."""
    cfg = dict(backbone)
    r, ws, s = resolve(cfg), widths(cfg), scales_of(cfg)
    bc = cfg.get('base_channels', 64)
    stem = cfg.get('stem_channels') or bc
    cin = cfg.get('in_channels', 3)
    out = {}

    def bn(prefix, c):
        out.update({prefix + '.weight': (c,), prefix + '.bias': (c,), prefix + '.running_mean': (c,),
                    prefix + '.running_var': (c,), prefix + '.num_batches_tracked': ()})
    for idx, (co, ci) in zip((0, 3, 6), ((stem // 2, cin), (stem // 2, stem // 2), (stem, stem // 2))):
        out[f'stem.{idx}.weight'] = (co, ci, 3, 3)
        bn(f'stem.{idx + 1}', co)
    inplanes = stem
    for i, nb in enumerate(r['blocks']):
        planes, w = bc * 2 ** i, ws[i]
        for j in range(nb):
            pre = f'layer{i + 1}.{j}'
            out[pre + '.conv1.weight'] = (w * s, inplanes, 1, 1)
            bn(pre + '.bn1', w * s)
            out[pre + '.conv3.weight'] = (4 * planes, w * s, 1, 1)
            bn(pre + '.bn3', 4 * planes)
            if j == 0 and (r['strides'][i] != 1 or inplanes != 4 * planes):
                out[pre + '.downsample.1.weight'] = (4 * planes, inplanes, 1, 1)
                bn(pre + '.downsample.2', 4 * planes)
            for k in range(s - 1):
                out[pre + f'.convs.{k}.weight'] = (w, w, 3, 3)
            for k in range(s - 1):
                bn(pre + f'.bns.{k}', w)
            inplanes = 4 * planes
    return out
