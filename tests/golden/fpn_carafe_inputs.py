"""Seeded inputs and weights of the FPN_CARAFE fixture (g32_fpn_carafe*.npz: the unchanged ``model.neck`` of
configs/carafe/mask_rcnn_r50_fpn_carafe_1x_coco.py), shared by tests/golden/make_golden_fpn_carafe.py and the tests: the
fixture stores outputs only.  ``restate`` is a torch restatement of the neck's forward from a resolved config and a
state_dict, for machines without the reference; the generator asserts that it gives the reference's outputs bit for bit on
the CPU, in float32 and in float64, and that ``state_shapes`` is the reference module's key list in order.

The backbone stages are fpn_inputs.STAGE_SIZES -- C2 18 x 27, C3 9 x 14, C4 5 x 7, C5 3 x 4 -- and the extra level P6 is
2 x 2: the top-down steps are 2 x 2 -> 3 x 4 (crops a row), 3 x 4 -> 5 x 7 (a row and a column), 5 x 7 -> 9 x 14 (a row)
and 9 x 14 -> 18 x 27 (a column)."""
import torch
import torch.nn.functional as F

from fpn_inputs import STAGE_SIZES, inputs  # noqa: F401  (the stages are the FPN fixture's)
from rpn_inputs import ERR_SCALE, head_state, pack_err, unpack_f64  # noqa: F401

FEAT_SEED = 323232
WEIGHT_SEED = 32
BATCH = 1                                           # (g27's Mask R-CNN form)
NECK_CONFIG = 'configs/carafe/mask_rcnn_r50_fpn_carafe_1x_coco.py'
# name -> (config, detector type)
DETECTORS = {'mask_rcnn_carafe': ('configs/carafe/mask_rcnn_r50_fpn_carafe_1x_coco.py', 'MaskRCNN'),
             'faster_rcnn_carafe': ('configs/carafe/faster_rcnn_r50_fpn_carafe_1x_coco.py', 'FasterRCNN')}
# output level -> its file: level 0 alone is 0.7 MB, so the outputs take two files below 1 MiB each
FILES = ('g32_fpn_carafe.npz', 'g32_fpn_carafe_1.npz', 'g32_fpn_carafe_1.npz', 'g32_fpn_carafe_1.npz', 'g32_fpn_carafe_1.npz')
CONFIGS = 'g32_fpn_carafe_configs.json'
NECK_ENTRY = 'mask_rcnn_carafe'                     # the entry of CONFIGS whose ``model.neck`` / ``neck_state_dict`` the run used


def resolve(neck):
    """The settings the forward depends on, from a neck config (``type`` may be present)."""
    cfg = dict(neck)
    cfg.pop('type', None)
    n_in = len(cfg['in_channels'])
    start = cfg.get('start_level', 0)
    end = cfg.get('end_level', -1)
    end = n_in if end == -1 else end
    up = dict(cfg.get('upsample_cfg', dict(type='carafe', up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1)))
    assert up['type'] == 'carafe' and up.get('encoder_kernel', 3) == 3 and up.get('encoder_dilation', 1) == 1
    return dict(start=start, end=end, num_outs=cfg['num_outs'], in_channels=list(cfg['in_channels']), out_channels=cfg['out_channels'],
                up_kernel=up.get('up_kernel', 5), up_group=up.get('up_group', 1), compressed=up.get('compressed_channels', 64))


def state_shapes(neck):
    """{key: shape} of FPN_CARAFE.state_dict() for a neck config, in the reference's order (fpn_carafe.py:84-199)."""
    r = resolve(neck)
    used, C = r['end'] - r['start'], r['out_channels']
    extra = r['num_outs'] - used
    lat, fpn, ups = {}, {}, {}
    for i in range(used + extra):
        if i < used:
            shape = (C, r['in_channels'][r['start'] + i], 1, 1)
        else:
            shape = (C, r['in_channels'][r['end'] - 1] if i == used else C, 3, 3)
        lat[f'lateral_convs.{i}.conv.weight'], lat[f'lateral_convs.{i}.conv.bias'] = shape, (C,)
        fpn[f'fpn_convs.{i}.conv.weight'], fpn[f'fpn_convs.{i}.conv.bias'] = (C, C, 3, 3), (C,)
    enc = r['up_kernel'] ** 2 * r['up_group'] * 4
    for i in range(used + extra - 1):
        pre = f'upsample_modules.{i}.'
        ups[pre + 'channel_compressor.weight'], ups[pre + 'channel_compressor.bias'] = (r['compressed'], C, 1, 1), (r['compressed'],)
        ups[pre + 'content_encoder.weight'], ups[pre + 'content_encoder.bias'] = (enc, r['compressed'], 3, 3), (enc,)
    return {**lat, **fpn, **ups}


def normalised_kernels(enc, up_kernel, up_group):
    """CARAFEPack.kernel_normalizer (mmcv/ops/carafe.py) at scale 2: [N, G K K 4, H, W] -> [N, G K K, 2H, 2W]."""
    mask = F.pixel_shuffle(enc, 2)
    n, mc, h, w = mask.shape
    return F.softmax(mask.view(n, up_group, up_kernel * up_kernel, h, w), dim=2).view(n, mc, h, w).contiguous()


def restate(neck, state, xs, every_level=False):
    """The neck's outputs for the stages ``xs`` with the parameters ``state`` (keys of FPN_CARAFE.state_dict), in the dtype
    and on the device of ``xs``, with torch's own operators in the reference's order of operations (the CARAFE operator is
    oracle.ref_ops's, as in every fixture).  ``every_level``: returns (outs, steps), one step per top-down merge in the
    order they run, each a dict ``level`` (i: lateral i is merged into lateral i - 1), ``src`` (lateral i as the step reads
    it), ``enc`` (the raw content-encoder output), ``lat`` (lateral i - 1 before the step) and ``merged`` (after it)."""
    from oracle import ref_ops
    r = resolve(neck)
    p = {k: v.to(xs[0].dtype).to(xs[0].device) for k, v in state.items()}
    used = r['end'] - r['start']
    n_lat = used + r['num_outs'] - used
    lats = []
    for i in range(n_lat):
        w, b = p[f'lateral_convs.{i}.conv.weight'], p[f'lateral_convs.{i}.conv.bias']
        if i < used:
            lats.append(F.conv2d(xs[r['start'] + i], w, b))
        else:
            src = xs[min(i + r['start'], len(xs) - 1)] if i <= used else lats[-1]
            lats.append(F.conv2d(src, w, b, stride=2, padding=1))
    steps = []
    for i in range(n_lat - 1, 0, -1):
        pre = f'upsample_modules.{i - 1}.'
        comp = F.conv2d(lats[i], p[pre + 'channel_compressor.weight'], p[pre + 'channel_compressor.bias'])
        enc = F.conv2d(comp, p[pre + 'content_encoder.weight'], p[pre + 'content_encoder.bias'], padding=1)
        up = ref_ops.carafe_reassemble(lats[i], normalised_kernels(enc, r['up_kernel'], r['up_group']), r['up_kernel'], r['up_group'], 2)
        before = lats[i - 1]
        h, w = before.shape[2:]
        lats[i - 1] = before + (up if tuple(up.shape[2:]) == (h, w) else up[:, :, :h, :w])
        steps.append(dict(level=i, src=lats[i], enc=enc, lat=before, merged=lats[i - 1]))
    outs = tuple(F.conv2d(lats[i], p[f'fpn_convs.{i}.conv.weight'], p[f'fpn_convs.{i}.conv.bias'], padding=1) for i in range(n_lat))
    return (outs, steps) if every_level else outs
