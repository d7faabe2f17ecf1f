"""Seeded inputs and weights of the RefineMask fixture (g17_refine.npz), shared by tests/golden/make_golden_refine.py and
the tests: the fixture stores outputs only (the head's 3.6 M weights and the FPN maps would be tens of MB)."""
import numpy as np
import torch

# configs/refinemask/coco/r50-refinemask-1x.py, mask_head (without ``type``)
HEAD_CFG = dict(num_convs_instance=2, num_convs_semantic=4, conv_in_channels_instance=256, conv_in_channels_semantic=256,
                conv_kernel_size_instance=3, conv_kernel_size_semantic=3, conv_out_channels_instance=256,
                conv_out_channels_semantic=256, conv_cfg=None, norm_cfg=None, dilations=[1, 3, 5], semantic_out_stride=4,
                mask_use_sigmoid=True, stage_num_classes=[80, 80, 80, 80], stage_sup_size=[14, 28, 56, 112],
                upsample_cfg=dict(type='bilinear', scale_factor=2),
                loss_cfg=dict(type='RefineCrossEntropyLoss', stage_instance_loss_weight=[0.25, 0.5, 0.75, 1.0],
                              semantic_loss_weight=1.0, boundary_width=2, start_stage=1))

IMG_H, IMG_W = 192, 256          # P2 48 x 64
STRIDES = (4, 8, 16, 32)
THRESHOLD = 0.5


def head_state(shapes):
    """Seeded parameters for ``shapes`` {key: shape} (a RefineMaskHead state_dict's): He-scaled weights, small biases."""
    g = torch.Generator().manual_seed(17)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('.weight'):
            fan_in = int(np.prod(shape[1:]))
            out[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def fpn_feats():
    """Four FPN levels [1, 256, H / s, W / s]."""
    g = torch.Generator().manual_seed(1717)
    return [torch.randn(1, 256, IMG_H // s, IMG_W // s, generator=g) for s in STRIDES]


def detections():
    """det_bboxes [n, 5] (x1, y1, x2, y2, score), det_labels [n]: boxes over the border, tiny ones, one over the whole
    image, large and mid-sized ones (several FPN levels)."""
    boxes = [[-20.0, -12.0, 60.5, 70.25, 0.9],       # over the top-left corner
             [200.0, 150.0, 290.0, 230.0, 0.8],       # over the bottom-right corner
             [100.3, 80.7, 103.1, 82.2, 0.7],         # tiny
             [0.0, 0.0, 256.0, 192.0, 0.95],          # the whole image
             [30.0, 40.0, 180.0, 170.0, 0.6],
             [120.5, 10.25, 250.75, 95.5, 0.5],
             [64.0, 100.0, 96.0, 140.0, 0.4]]
    labels = [3, 17, 0, 79, 42, 3, 8]
    return torch.tensor(boxes, dtype=torch.float32), torch.tensor(labels, dtype=torch.int64)


def img_metas():
    return [dict(ori_shape=(IMG_H, IMG_W, 3), img_shape=(IMG_H, IMG_W, 3), pad_shape=(IMG_H, IMG_W, 3),
                 scale_factor=1.0, flip=False, flip_direction=None)]
