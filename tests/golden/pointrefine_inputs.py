"""Seeded inputs and weights of the PointRefine fixture (g20_pointrefine.npz), shared by
tests/golden/make_golden_pointrefine.py and the tests: the fixture stores outputs only (the mask head has 4.9 M weights)."""
import numpy as np
import torch

IMG_H, IMG_W = 192, 256          # P2 48 x 64
STRIDES = (4, 8, 16, 32)
THRESHOLD = 0.5
NUM_POINTS = 28 * 28             # configs/point_refine test_cfg.rcnn.num_points
TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), num_points=NUM_POINTS, max_per_img=100,
                mask_thr_binary=0.5)


def head_state(shapes):
    """Seeded parameters for ``shapes`` {key: shape} (a PointRefineRoIHead state_dict's mask_head entries): He-scaled
    weights, small biases; the logit maps are scaled down so that the detail sigmoid does not saturate everywhere."""
    g = torch.Generator().manual_seed(20)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('.weight'):
            fan_in = int(np.prod(shape[1:]))
            w = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
            if 'logits' in k:
                w = w * 0.5
            out[k] = w
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def fpn_feats():
    """Four FPN levels [1, 256, H / s, W / s]."""
    g = torch.Generator().manual_seed(2020)
    return [torch.randn(1, 256, IMG_H // s, IMG_W // s, generator=g) for s in STRIDES]


def detections():
    """det_bboxes [n, 5] (x1, y1, x2, y2, score), det_labels [n]: boxes over the border, a tiny one, one over the whole
    image, and mid-sized ones (several FPN levels)."""
    boxes = [[-20.0, -12.0, 60.5, 70.25, 0.9],       # over the top-left corner
             [100.3, 80.7, 103.1, 82.2, 0.7],         # tiny
             [0.0, 0.0, 256.0, 192.0, 0.95],          # the whole image
             [30.0, 40.0, 180.0, 170.0, 0.6],
             [120.5, 10.25, 250.75, 95.5, 0.5]]
    labels = [3, 0, 79, 42, 3]
    return torch.tensor(boxes, dtype=torch.float32), torch.tensor(labels, dtype=torch.int64)


def img_metas():
    return [dict(ori_shape=(IMG_H, IMG_W, 3), img_shape=(IMG_H, IMG_W, 3), pad_shape=(IMG_H, IMG_W, 3),
                 scale_factor=1.0, flip=False, flip_direction=None)]
