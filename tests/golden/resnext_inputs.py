"""Forms and torch restatement of the ResNeXt fixture (g30_resnext.npz, g30_resnext_configs.json), shared by
tests/golden/make_golden_resnext.py and the tests.  The images, the seeded weights and the error twins' form are the
backbone fixture's (backbone_inputs.inputs / head_state, rpn_inputs.pack_err): nothing of those files changes.
``restate_stage`` / ``restate`` are backbone_inputs' restatements with ``groups`` on conv2 (BatchNorm NOT folded); the
generator asserts that they give the reference's ``ResNeXt`` bit for bit on the CPU, in float32 and in float64.

The images are 2 x 3 x 37 x 53, so C2 is 10 x 14, C3 5 x 7, C4 3 x 4 and C5 2 x 2: the stride-2 grouped convolutions of
layers 2, 3 and 4 meet an even, an odd and an even size."""
import torch.nn.functional as F

from backbone_inputs import (BATCH, IMG_H, IMG_SEED, IMG_W, STAGE_BLOCKS, WEIGHT_SEED, _bn, _params, head_state, inputs,  # noqa: F401
                             pack_err, resolve, restate_stem, unpack_f64)

# per-part forms: name -> the config its ``model.backbone`` comes from.  Only the first is run; all are depth 101.
PARTS = {'x101_32x4d': 'configs/mask_rcnn/mask_rcnn_x101_32x4d_fpn_1x_coco.py',
         'x101_64x4d': 'configs/mask_rcnn/mask_rcnn_x101_64x4d_fpn_1x_coco.py',
         'x101_32x8d': 'configs/mask_rcnn/mask_rcnn_x101_32x8d_fpn_1x_coco.py'}
RUN = 'x101_32x4d'
# whole detectors: name -> (config, model.type)
DETECTORS = {'mask_rcnn_x101_32x4d': ('configs/mask_rcnn/mask_rcnn_x101_32x4d_fpn_1x_coco.py', 'MaskRCNN'),
             'mask_rcnn_x101_64x4d': ('configs/mask_rcnn/mask_rcnn_x101_64x4d_fpn_1x_coco.py', 'MaskRCNN'),
             'mask_rcnn_x101_32x8d': ('configs/mask_rcnn/mask_rcnn_x101_32x8d_fpn_1x_coco.py', 'MaskRCNN'),
             'cascade_x101_32x4d': ('configs/cascade_rcnn/cascade_mask_rcnn_x101_32x4d_fpn_1x_coco.py', 'CascadeRCNN'),
             'htc_x101_64x4d': ('configs/htc/htc_x101_64x4d_fpn_16x1_20e_coco.py', 'HybridTaskCascade')}
FILE = 'g30_resnext.npz'
CONFIGS = 'g30_resnext_configs.json'


def groups_of(backbone):
    return int(dict(backbone).get('groups', 1))


def widths(backbone):
    """conv2's channels per stage: resnext.py:28-32."""
    cfg = dict(backbone)
    groups, bw, bc = groups_of(cfg), cfg.get('base_width', 4), cfg.get('base_channels', 64)
    n = cfg.get('num_stages', 4)
    return [bc * 2 ** i if groups == 1 else (bc * 2 ** i * bw // bc) * groups for i in range(n)]


def restate_stage(backbone, state, i, x):
    """Stage ``i`` (``layer{i + 1}``) on its input ``x``, in the reference's order of operations, conv2 in ``groups``."""
    r = resolve(backbone)
    groups = groups_of(backbone)
    p = _params(state, x)
    for j in range(r['blocks'][i]):
        pre = f'layer{i + 1}.{j}'
        stride = r['strides'][i] if j == 0 else 1
        s1, s2 = (1, stride) if r['style'] == 'pytorch' else (stride, 1)
        out = F.relu(_bn(F.conv2d(x, p[pre + '.conv1.weight'], stride=s1), p, pre + '.bn1'))
        out = F.relu(_bn(F.conv2d(out, p[pre + '.conv2.weight'], stride=s2, padding=1, groups=groups), p, pre + '.bn2'))
        out = _bn(F.conv2d(out, p[pre + '.conv3.weight']), p, pre + '.bn3')
        identity = x
        if pre + '.downsample.0.weight' in p:
            identity = _bn(F.conv2d(x, p[pre + '.downsample.0.weight'], stride=stride), p, pre + '.downsample.1')
        out += identity
        x = F.relu(out)
    return x


def restate(backbone, state, img, every_stage=False):
    """The backbone's outputs for ``img`` with the parameters ``state`` (keys of ResNeXt.state_dict), in the dtype and on
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
    """{key: shape} of the reference ``ResNeXt``'s ``state_dict`` for a backbone config (``type`` may be present), in the
    reference's order -- for the forms no fixture entry records (the caffe-style stage test)."""
    cfg = dict(backbone)
    r, ws = resolve(cfg), widths(cfg)
    groups, bc = groups_of(cfg), cfg.get('base_channels', 64)
    stem = cfg.get('stem_channels') or bc
    out = {'conv1.weight': (stem, cfg.get('in_channels', 3), 7, 7)}

    def bn(prefix, c):
        out.update({prefix + '.weight': (c,), prefix + '.bias': (c,), prefix + '.running_mean': (c,),
                    prefix + '.running_var': (c,), prefix + '.num_batches_tracked': ()})
    bn('bn1', stem)
    inplanes = stem
    for i, nb in enumerate(r['blocks']):
        planes, w = bc * 2 ** i, ws[i]
        for j in range(nb):
            pre = f'layer{i + 1}.{j}'
            out[pre + '.conv1.weight'] = (w, inplanes, 1, 1)
            bn(pre + '.bn1', w)
            out[pre + '.conv2.weight'] = (w, w // groups, 3, 3)
            bn(pre + '.bn2', w)
            out[pre + '.conv3.weight'] = (4 * planes, w, 1, 1)
            bn(pre + '.bn3', 4 * planes)
            if j == 0 and (r['strides'][i] != 1 or inplanes != 4 * planes):
                out[pre + '.downsample.0.weight'] = (4 * planes, inplanes, 1, 1)
                bn(pre + '.downsample.1', 4 * planes)
            inplanes = 4 * planes
    return out
