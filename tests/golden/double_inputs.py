"""Seeded inputs and weights of the Double-Head R-CNN fixture (g24_double.npz), shared by
tests/golden/make_golden_double.py and the tests: the fixture stores outputs only (the bbox head holds 20 M weights).
The image, the FPN levels and the scale factors are grid_inputs.py's."""
import numpy as np
import torch

from grid_inputs import IMG_H, IMG_W, SCALE_FACTOR, STRIDES, fpn_feats, img_metas  # noqa: F401
from grid_inputs import proposals as _seeded_proposals

N_SEEDED = 20
PROPOSAL_SEED = 2424
REG_ROI_SCALE_FACTOR = 1.3
FINEST_SCALE = 56
# seeds the generator tries in order; the one it settles on is stored in the fixture (``weight_seed``)
WEIGHT_SEEDS = tuple(range(24, 64))

# name -> box; sqrt(w h) decides the FPN level: < 112 level 0, < 224 level 1, < 448 level 2
HAND_BOXES = {
    # sqrt(w h) = 100 in [112 / 1.3, 112): level 0; taken after the rescale (130) it would be level 1
    'level_0_not_1': [40.0, 30.0, 140.0, 130.0],
    # sqrt(250 * 150) = 193.6 in [224 / 1.3, 224): level 1; taken after the rescale (251.7) it would be level 2
    'level_1_not_2': [3.0, 20.0, 253.0, 170.0],
    # rescaled: x1 = 47.5 - 55.25 < 0 and y1 = 39 - 40.3 < 0: leaves the image at the left and at the top
    'leaves_two_sides': [5.0, 8.0, 90.0, 70.0],
    'tiny': [100.3, 80.7, 103.1, 82.2],
    'whole_image': [0.0, 0.0, float(IMG_W), float(IMG_H)],
    # rescaled past the right and bottom borders
    'bottom_right': [170.0, 120.0, 255.0, 190.5],
    'mid': [64.0, 100.0, 96.0, 140.0],
}
LEVEL_CHANGING = ('level_0_not_1', 'level_1_not_2')


def hand_boxes():
    return torch.tensor([HAND_BOXES[k] for k in HAND_BOXES], dtype=torch.float32)


def hand_index(name):
    return list(HAND_BOXES).index(name)


def proposals(seed=PROPOSAL_SEED, n=N_SEEDED):
    """The hand-written boxes, then ``n`` seeded ones: [7 + n, 4]."""
    return torch.cat([hand_boxes(), _seeded_proposals(seed=seed, n=n)]).contiguous()


def head_state(shapes, seed):
    """Seeded parameters and buffers for ``shapes`` {key: shape} (a DoubleConvFCBBoxHead state_dict, with or without a
    ``bbox_head.`` prefix): He-scaled convolution and FC weights (the classifier scaled up so that some scores pass
    ``score_thr``); BatchNorm weights around 1 -- around 0.5 for every ``bn3``, so that the five residual sums stay O(1) --
    small BatchNorm biases and running means, running variances in [0.5, 1.5] (not all ones: a missing fold shows)."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros(shape, dtype=torch.long)
        elif k.endswith('running_var'):
            out[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith('running_mean'):
            out[k] = 0.1 * torch.randn(shape, generator=g)
        elif k.endswith('.weight') and len(shape) == 1:
            out[k] = (0.5 + 0.05 * torch.randn(shape, generator=g)) if '.bn3.' in k else (1.0 + 0.1 * torch.randn(shape, generator=g))
        elif k.endswith('.weight'):
            w = torch.randn(shape, generator=g) * (2.0 / int(np.prod(shape[1:]))) ** 0.5
            out[k] = w * 6.0 if 'fc_cls.' in k else w
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


# The five launches of the conv branch at 7 x 7: name -> (source channels, Cout, kernel, accumulate).  All with ReLU.
CONV_SHAPES = {
    'res_conv1_3x3': ((256,), 256, 3, False),
    'res_merged_1x1': ((256, 256), 1024, 1, False),
    'bottleneck_conv1_1x1': ((1024,), 256, 1, False),
    'bottleneck_conv2_3x3': ((256,), 256, 3, False),
    'bottleneck_conv3_1x1_accumulate': ((256,), 1024, 1, True),
}
# The RoI counts the GPU test runs each launch at: 3, and the smallest count at which the launcher moves to the build its
# 1000-RoI call takes (tests/test_double_cpu.py holds the list to the launcher's own report, dm_conv2d_plan).
CONV_TEST_NBS = {
    'res_conv1_3x3': (3, 233),
    'res_merged_1x1': (3, 105),
    'bottleneck_conv1_1x1': (3, 418),
    'bottleneck_conv2_3x3': (3, 233),
    'bottleneck_conv3_1x1_accumulate': (3,),
}
