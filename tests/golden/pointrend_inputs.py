"""Seeded inputs and weights of the PointRend fixture (g18_pointrend.npz), shared by tests/golden/make_golden_pointrend.py
and the tests: the fixture stores outputs only (the coarse head alone has 17 M weights)."""
import numpy as np
import torch

IMG_H, IMG_W = 192, 256          # P2 48 x 64
THRESHOLD = 0.5
TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=0.5,
                subdivision_steps=5, subdivision_num_points=784, scale_factor=2)


def head_state(shapes):
    """Seeded parameters for ``shapes`` {key: shape} (a PointRendRoIHead state_dict's mask_head / point_head entries):
    He-scaled weights, small biases; the coarse logits get a spread that puts the 7 x 7 map on both sides of zero."""
    g = torch.Generator().manual_seed(18)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('.weight'):
            fan_in = int(np.prod(shape[1:]))
            out[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def p2(seed=1818):
    """The stride-4 FPN level [1, 256, 48, 64]."""
    return torch.randn(1, 256, IMG_H // 4, IMG_W // 4, generator=torch.Generator().manual_seed(seed))


def detections():
    """det_bboxes [n, 5], det_labels [n]: a box over the top-left corner, a large one and a mid-sized one."""
    boxes = [[-20.0, -12.0, 60.5, 70.25, 0.9],
             [30.0, 40.0, 180.0, 170.0, 0.6],
             [120.5, 10.25, 250.75, 95.5, 0.5]]
    return torch.tensor(boxes, dtype=torch.float32), torch.tensor([3, 42, 8], dtype=torch.int64)


def img_metas(flip=False):
    return [dict(ori_shape=(IMG_H, IMG_W, 3), img_shape=(IMG_H, IMG_W, 3), pad_shape=(IMG_H, IMG_W, 3),
                 scale_factor=1.0, flip=flip, flip_direction='horizontal' if flip else None)]


def aug_views():
    """Two views of one image, the second flipped horizontally: (P2 per view, img_metas per view)."""
    x = p2()
    return [x, torch.flip(x, dims=[3]).contiguous()], [img_metas(False), img_metas(True)]
