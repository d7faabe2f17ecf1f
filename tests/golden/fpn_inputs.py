"""Seeded inputs and weights of the FPN fixture (g27_fpn*.npz: the unchanged ``model.neck`` of the Mask R-CNN, RetinaNet and
FCOS configs), shared by tests/golden/make_golden_fpn.py and the tests: the fixture stores outputs only.  ``restate`` is a
torch restatement of the neck's forward from a resolved config and a state_dict, for machines without the reference; the
generator asserts that it gives the reference's float32 outputs bit for bit on the CPU.

The backbone stages of every form are C2 18 x 27, C3 9 x 14, C4 5 x 7 and C5 3 x 4: the top-down merge meets an even step
(9 -> 18, 7 -> 14) and a 2 n - 1 step (14 -> 27, 5 -> 9, 3 -> 5, 4 -> 7) on both axes."""
import torch
import torch.nn.functional as F

from rpn_inputs import ERR_SCALE, head_state, pack_err, unpack_f64  # noqa: F401  (the twins' form is the RPN fixture's)

STAGE_SIZES = ((18, 27), (9, 14), (5, 7), (3, 4))
FEAT_SEED = 272727
WEIGHT_SEED = 27
# form -> (the config its ``model.neck`` comes from, batch)
FORMS = {'mask_rcnn': ('configs/_base_/models/mask_rcnn_r50_fpn.py', 1),
         'retinanet': ('configs/_base_/models/retinanet_r50_fpn.py', 2),
         'fcos': ('configs/fcos/fcos_r50_caffe_fpn_4x4_1x_coco.py', 2)}
# the file of each form's outputs: one file per form keeps every committed file below 1 MiB
FILES = {'mask_rcnn': 'g27_fpn.npz', 'retinanet': 'g27_fpn_retinanet.npz', 'fcos': 'g27_fpn_fcos.npz'}


def inputs(in_channels, batch, seed=FEAT_SEED, sizes=STAGE_SIZES):
    """Per stage [batch, in_channels[l], H, W], image b of stage l from seed + 16 * b + l."""
    return [torch.cat([torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(seed + 16 * b + l))
                       for b in range(batch)]).contiguous()
            for l, (c, (h, w)) in enumerate(zip(in_channels, sizes))]


def resolve(neck):
    """The settings the forward depends on, from a neck config (``type`` may be present): start level, number of backbone
    levels used, the extra levels' source ('' for the max-pool form) and the ReLU in front of the later extra convs."""
    cfg = dict(neck)
    cfg.pop('type', None)
    n_in = len(cfg['in_channels'])
    start = cfg.get('start_level', 0)
    end = cfg.get('end_level', -1)
    end = n_in if end == -1 else end
    extra = cfg.get('add_extra_convs', False)
    if extra is True:
        extra = 'on_input' if cfg.get('extra_convs_on_inputs', True) else 'on_output'
    return dict(start=start, end=end, num_outs=cfg['num_outs'], extra=extra or '',
                relu=bool(cfg.get('relu_before_extra_convs', False)), upsample=dict(cfg.get('upsample_cfg', dict(mode='nearest'))))


def restate(neck, state, xs):
    """The neck's outputs for the stages ``xs`` with the parameters ``state`` (keys of FPN.state_dict), in the dtype and
    on the device of ``xs``, with torch's own operators in the reference's order of operations."""
    r = resolve(neck)
    p = {k: v.to(xs[0].dtype).to(xs[0].device) for k, v in state.items()}
    used = r['end'] - r['start']
    lats = [F.conv2d(xs[r['start'] + i], p[f'lateral_convs.{i}.conv.weight'], p[f'lateral_convs.{i}.conv.bias'])
            for i in range(used)]
    for i in range(used - 1, 0, -1):
        if 'scale_factor' in r['upsample']:
            lats[i - 1] += F.interpolate(lats[i], **r['upsample'])
        else:
            lats[i - 1] += F.interpolate(lats[i], size=lats[i - 1].shape[2:], **r['upsample'])
    outs = [F.conv2d(lats[i], p[f'fpn_convs.{i}.conv.weight'], p[f'fpn_convs.{i}.conv.bias'], padding=1) for i in range(used)]
    for i in range(used, r['num_outs']):
        if not r['extra']:
            outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            continue
        if i == used:
            src = {'on_input': xs[r['end'] - 1], 'on_lateral': lats[-1], 'on_output': outs[-1]}[r['extra']]
        else:
            src = F.relu(outs[-1]) if r['relu'] else outs[-1]
        outs.append(F.conv2d(src, p[f'fpn_convs.{i}.conv.weight'], p[f'fpn_convs.{i}.conv.bias'], stride=2, padding=1))
    return tuple(outs)
