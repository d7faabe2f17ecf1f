"""Seeded inputs and weights of the Mask Scoring R-CNN fixture (g19_msrcnn.npz), shared by
tests/golden/make_golden_msrcnn.py and the tests: the fixture stores outputs only (the IoU head alone has 16 M weights)."""
import numpy as np
import torch

IMG_H, IMG_W = 256, 320          # FPN levels 64 x 80, 32 x 40, 16 x 20, 8 x 10
STRIDES = (4, 8, 16, 32)
TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=0.5)


def head_state(shapes):
    """Seeded parameters for ``shapes`` {key: shape} (a MaskScoringRoIHead state_dict's mask_head / mask_iou_head
    entries): He-scaled weights, small biases."""
    g = torch.Generator().manual_seed(19)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('.weight'):
            fan_in = int(np.prod(shape[1:]))
            out[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def fpn(seed=1919, batch=1):
    """The four FPN levels [batch, 256, IMG_H / s, IMG_W / s] (image b of a batch: seed + b)."""
    levels = []
    for s in STRIDES:
        levels.append(torch.cat([torch.randn(1, 256, IMG_H // s, IMG_W // s, generator=torch.Generator().manual_seed(seed + b + s))
                                 for b in range(batch)]))
    return levels


def detections():
    """det_bboxes [n, 5], det_labels [n]: a box past the top-left corner, one past the right edge, a large one, two
    small ones (two of the same class), scores last."""
    boxes = [[-18.0, -10.5, 70.25, 60.0, 0.95],
             [250.5, 120.0, 335.0, 230.75, 0.8],
             [30.0, 40.0, 220.0, 240.0, 0.7],
             [140.25, 20.5, 180.0, 58.0, 0.55],
             [100.0, 150.0, 128.5, 190.25, 0.3]]
    return torch.tensor(boxes, dtype=torch.float32), torch.tensor([3, 17, 42, 17, 79], dtype=torch.int64)


def img_metas():
    return [dict(ori_shape=(IMG_H, IMG_W, 3), img_shape=(IMG_H, IMG_W, 3), pad_shape=(IMG_H, IMG_W, 3),
                 scale_factor=1.0, flip=False, flip_direction=None)]
