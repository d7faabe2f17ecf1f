"""Seeded inputs and weights of the C4 fixture (g25_c4.npz: Mask R-CNN / Faster R-CNN C4, StandardRoIHead with the ResLayer
shared head), shared by tests/golden/make_golden_c4.py and the tests: the fixture stores outputs only (layer4 holds 15 M
weights).  One stride-16 map of a 320 x 480 image; the hand-written proposals first, then seeded ones."""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from dynamask_amd import synth  # noqa: E402

IMG_H, IMG_W = 320, 480          # the C4 map: 20 x 30
STRIDE = 16
CHANNELS = 1024
N_SEEDED = 12
PROPOSAL_SEED = 2525
FEAT_SEED = 252525
# scale_factor of the rescale=True run: [w, h, w, h], two different factors
SCALE_FACTOR = np.array([1.5, 1.25, 1.5, 1.25], dtype=np.float32)
# seeds the generator tries in order; the one it settles on is stored in the fixture (``weight_seed``)
WEIGHT_SEEDS = tuple(range(25, 125))

# name -> box.  At stride 16 a 14-bin extraction samples a g x g grid per bin with g = ceil(extent / 16 / 14).
HAND_BOXES = {
    'partly_outside': [-40.0, -25.0, 150.0, 120.0],
    'under_one_pixel': [200.3, 150.6, 200.9, 151.2],
    # 1140 x 1120 pixels = 71.25 x 70 map pixels: a 6 x 5 sampling grid, above the merged stencils' 4 x 4
    'spans_the_image': [-330.0, -400.0, 810.0, 720.0],
    'zero_area': [100.0, 100.0, 100.0, 100.0],
    'over_the_corner': [400.0, 250.0, 520.5, 350.25],
    'mid': [64.0, 100.0, 196.0, 240.0],
}


def hand_boxes():
    return torch.tensor([HAND_BOXES[k] for k in HAND_BOXES], dtype=torch.float32)


def hand_index(name):
    return list(HAND_BOXES).index(name)


def proposals(seed=PROPOSAL_SEED, n=N_SEEDED):
    """The hand-written boxes, then ``n`` seeded ones: [6 + n, 4]."""
    seeded = synth.make_rois(1, n, IMG_H, IMG_W, seed=seed, min_size=12.0, max_size=100.0)[:, 1:]
    return torch.cat([hand_boxes(), seeded]).contiguous()


def c4_feats(batch=1, seed=FEAT_SEED):
    """The stride-16 map as a one-level tuple [batch, 1024, 20, 30]; image b of a batch has the map of seed + b."""
    maps = [torch.randn(1, CHANNELS, IMG_H // STRIDE, IMG_W // STRIDE, generator=torch.Generator().manual_seed(seed + b))
            for b in range(batch)]
    return [torch.cat(maps).contiguous()]


def img_metas(scale_factor=1.0):
    return [dict(ori_shape=(IMG_H, IMG_W, 3), img_shape=(IMG_H, IMG_W, 3), pad_shape=(IMG_H, IMG_W, 3),
                 scale_factor=scale_factor, flip=False, flip_direction=None)]


HEAD_PREFIXES = ('shared_head.', 'bbox_head.', 'mask_head.')
MASK_LOGIT_BIAS = 14.0


def head_state(shapes, seed):
    """Seeded parameters and buffers for ``shapes`` {key: shape}, the ``shared_head.*`` / ``bbox_head.*`` / ``mask_head.*``
    entries of a C4 StandardRoIHead state_dict: He-scaled convolution and FC weights (the classifier scaled up so that
    some scores pass ``score_thr``, its rows centred so that the positive mean of the pooled features favours no class); BatchNorm weights around 1 -- around 0.5 for every ``bn3`` and ``downsample.1``, so
    that the residual sums stay O(1) -- small BatchNorm biases and running means, running variances in [0.5, 1.5] (not all
    ones: a missing fold shows).  The mask logits get a class bias of +-MASK_LOGIT_BIAS over half-scaled weights: a class's
    masks are saturated, full or empty, so that a pasted probability comes near ``mask_thr_binary`` only where a pixel
    centre falls on a box edge or on the curve through a full mask's corner -- which the generator's seed search can then
    exclude (a noisy 14 x 14 mask crosses the threshold between any two cells, and some pixel of a 320 x 480 canvas always
    lands within 1e-3 of it).  The seeded proposals are small for the same reason: a corner's curve is as long as a mask cell."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes):
        if not k.startswith(HEAD_PREFIXES):
            continue
        shape = tuple(shapes[k])
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros(shape, dtype=torch.long)
        elif k.endswith('running_var'):
            out[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith('running_mean'):
            out[k] = 0.1 * torch.randn(shape, generator=g)
        elif k.endswith('.weight') and len(shape) == 1:
            half = '.bn3.' in k or '.downsample.1.' in k
            out[k] = (0.5 + 0.05 * torch.randn(shape, generator=g)) if half else (1.0 + 0.1 * torch.randn(shape, generator=g))
        elif k.endswith('.weight'):
            fan_in = int(np.prod(shape[1:]))
            if 'mask_head.upsample.' in k:
                fan_in = shape[0]                      # ConvTranspose2d [Cin, Cout, 2, 2]: one tap per output pixel
            w = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
            if 'fc_cls.' in k:
                w = (w - w.mean(1, keepdim=True)) * 12.0
            out[k] = w * 0.5 if 'conv_logits.' in k else w
        elif k == 'mask_head.conv_logits.bias':
            out[k] = MASK_LOGIT_BIAS * torch.sign(torch.randn(shape, generator=g))
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


# The five convolution shapes of layer4 at 7 x 7: name -> (source channels, Cout, kernel, accumulate).  All with ReLU.
CONV_SHAPES = {
    'block0_conv1_1x1': ((1024,), 512, 1, False),
    'conv2_3x3': ((512,), 512, 3, False),
    'block0_merged_1x1': ((512, 1024), 2048, 1, False),
    'conv1_1x1': ((2048,), 512, 1, False),
    'conv3_1x1_accumulate': ((512,), 2048, 1, True),
}
# The RoI counts the GPU test runs each launch at: 3, and the smallest count at which the launcher moves to the build its
# 1000-RoI call takes (tests/test_c4_cpu.py holds the list to the launcher's own report, dm_conv2d_plan).
CONV_TEST_NBS = {
    'block0_conv1_1x1': (3, 209),
    'conv2_3x3': (3, 115),
    'block0_merged_1x1': (3, 53),
    'conv1_1x1': (3, 209),
    'conv3_1x1_accumulate': (3,),
}
