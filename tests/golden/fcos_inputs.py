"""Seeded inputs and weights of the FCOS fixture (tests/golden/g33_fcos.npz), shared by make_golden_fcos.py and the tests.

Reduced widths: ``in_channels = feat_channels = 64`` (GN at 32 groups), 5 classes, B = 2, five levels of 13 x 17, 7 x 9,
4 x 5, 2 x 3 and 1 x 1 at the FCOS strides, ``nms_pre = 50`` (so the first two levels are cut and the others are not).
Three forms of the head: ``gn`` (the reference's defaults), ``tricks`` (``norm_on_bbox`` + ``centerness_on_reg``, NMS at
0.6) and ``nonorm`` (``norm_cfg=None``: biased tower convolutions, no GroupNorm; head outputs only)."""
import numpy as np
import torch

CONFIGS = 'g33_fcos_configs.json'
DCN_CONFIG = 'g33_fcos_dcn.json'           # the one file of configs/fcos that is not built
FIXTURE = 'g33_fcos.npz'

B, CHANNELS, NUM_CLASSES = 2, 64, 5
LEVELS = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 1)]
STRIDES = [8, 16, 32, 64, 128]
NMS_PRE = 50
IMG_SHAPES = [(104, 136, 3), (99, 131, 3)]           # the second image is clipped inside the batch's maps
SCALE_FACTORS = [np.array([1.7, 1.6, 1.7, 1.6], dtype=np.float32), np.array([1.25, 1.3125, 1.25, 1.3125], dtype=np.float32)]
FEAT_SEED = 11
WEIGHT_SEEDS = list(range(40, 140))

_HEAD = dict(num_classes=NUM_CLASSES, in_channels=CHANNELS, feat_channels=CHANNELS, stacked_convs=4, strides=STRIDES)
FORMS = {
    'gn': dict(_HEAD, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)),
    'tricks': dict(_HEAD, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), norm_on_bbox=True,
                   centerness_on_reg=True),
    'nonorm': dict(_HEAD, norm_cfg=None),
}
DETECTION_FORMS = ('gn', 'tricks')
TEST_CFGS = {
    'gn': dict(nms_pre=NMS_PRE, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100),
    'tricks': dict(nms_pre=NMS_PRE, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=100),
    'nonorm': dict(nms_pre=NMS_PRE, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100),
}


def feats(batch=B, seed=FEAT_SEED, channels=CHANNELS, levels=LEVELS):
    """The neck's maps, one [batch, channels, H, W] tensor per level; image b's values do not depend on ``batch``."""
    out = []
    for l, (h, w) in enumerate(levels):
        maps = [torch.randn(channels, h, w, generator=torch.Generator().manual_seed(1000 * seed + 10 * l + b)) for b in range(batch)]
        out.append(torch.stack(maps))
    return out


def img_metas(rescaled=True, batch=B):
    return [dict(img_shape=IMG_SHAPES[b], ori_shape=IMG_SHAPES[b], pad_shape=(104, 136, 3),
                 scale_factor=SCALE_FACTORS[b] if rescaled else np.ones(4, dtype=np.float32), flip=False) for b in range(batch)]


def head_state(shapes, seed, form='gn'):
    """Seeded values for a head's ``state_dict`` ({key: shape}): tower weights at the kaiming scale, GroupNorm parameters
    near (1, 0), a class prior that leaves about half the scores under ``score_thr``, distances of about 12 pixels at
    stride 8 (boxes that overlap their neighbours), positive scales."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape in shapes.items():
        r = torch.randn(tuple(shape), generator=g)
        if k.startswith('scales.'):
            v = 1.0 + 0.1 * r
        elif '.gn.weight' in k:
            v = 1.0 + 0.1 * r
        elif '.gn.bias' in k or k.endswith('.conv.bias'):
            v = 0.1 * r
        elif k.endswith('.conv.weight'):
            v = r * (2.0 / (9 * shape[1])) ** 0.5
        elif k == 'conv_cls.weight':
            v = 0.3 * r             # (logits spread over +-5: few scores near score_thr, so a seed clears the margins)
        elif k == 'conv_cls.bias':
            v = -3.0 + 0.2 * r
        elif k == 'conv_reg.weight':
            v = (0.02 if form == 'tricks' else 0.03) * r
        elif k == 'conv_reg.bias':
            v = (2.0 if form == 'tricks' else 2.5) + 0.1 * r          # (tricks: distances in units of the stride)
        elif k == 'conv_centerness.weight':
            v = 0.06 * r
        elif k == 'conv_centerness.bias':
            v = 0.1 * r
        else:
            raise KeyError(k)
        out[k] = v
    return out
