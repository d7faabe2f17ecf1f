"""Seeded inputs and weights of the Hybrid Task Cascade fixture (g22_htc.npz), shared by tests/golden/make_golden_htc.py
and the tests: the fixture stores outputs only.  The image, the views and the proposals are those of the Cascade fixture
(cascade_inputs.py); the weights and the test config are HTC's own."""
import numpy as np
import torch

import cascade_inputs as ci
from cascade_inputs import AUG_VIEWS, ORI_SHAPE, aug_inputs, proposals, simple_inputs, view_maps, view_meta  # noqa: F401

# max_per_img keeps the four recorded result sets (with / without the semantic head x simple / aug) inside the size limit
# of a committed file
TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=24, mask_thr_binary=0.5)
SEM_SAMPLE_SEED = 2207
SEM_SAMPLES = 16384
EMB = 0.25                      # scale of the semantic embedding's weights (larger: one class takes every detection)


def head_state(shapes):
    """Seeded parameters for ``shapes`` {key: shape} (the ``bbox_head.*`` / ``mask_head.*`` / ``semantic_head.*`` entries
    of a HybridTaskCascadeRoIHead state_dict), drawn in sorted key order -- ``bbox_head`` and ``mask_head`` sort before
    ``semantic_head``, so the head without a semantic branch gets the same box and mask weights.  He-scaled weights, small
    biases; the regression layers scaled down and the classifiers up as in cascade_inputs.head_state; ``conv_res`` scaled
    up so that the information flow moves the stage probabilities well beyond the test tolerance, the semantic embedding
    likewise for the fusion."""
    g = torch.Generator().manual_seed(22)
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('.weight'):
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            if 'upsample' in k:                      # ConvTranspose2d [Cin, Cout, 2, 2]: fan-in Cin (per output phase)
                fan_in = shape[0]
            w = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
            if '.fc_reg.' in k:
                w = w * 0.5
            elif '.fc_cls.' in k:
                w = w * 4.0
            elif '.conv_res.' in k:
                w = w * 2.0
            elif '.conv_embedding.' in k:
                w = w * EMB
            elif k.startswith('mask_head.') and '.conv_logits.' in k:
                w = w * 4.0                          # logits spread out: few merged probabilities next to the threshold
            out[k] = w
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def sem_sample_index(numel):
    """The flat positions of the semantic feature map that the fixture records (all of them when it is small enough)."""
    if numel <= SEM_SAMPLES:
        return np.arange(numel)
    return np.sort(np.random.RandomState(SEM_SAMPLE_SEED).choice(numel, SEM_SAMPLES, replace=False))
