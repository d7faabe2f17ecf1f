"""Seeded inputs of the test-time augmentation fixture g16 (make_golden_aug.py on the reference side,
tests/test_aug_test_gpu.py on the device).  Pure data generation: the FPN maps of every view, the proposals of the
original image, the view metas and the RoI head's weights."""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from dynamask_amd import synth  # noqa: E402
from dynamask_amd.synth import (BBOX_HEAD_CFG, BBOX_ROI_EXTRACTOR_CFG, FCN_HEAD_CFG,  # noqa: E402,F401
                                MASK_ROI_EXTRACTOR_CFG)

ORI_SHAPE = (128, 160, 3)
N_PROPOSALS = 32
PROPOSAL_SEED = 323
TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=0.5)
# per case: the views as (scale, flip direction or None)
CASES = {
    'ms': [(1.0, None), (1.0, 'horizontal'), (1.5, None), (1.5, 'horizontal')],
    'vf': [(1.0, None), (1.0, 'vertical'), (1.25, 'horizontal')],
}


def head_state():
    """StandardRoIHead state_dict (bbox head, FCN mask head with deconv, and the fork's MaskPre keys)."""
    return {**synth.init_mask_pre_state(seed=6), **synth.init_bbox_head_state(seed=8),
            **synth.init_fcn_head_state(seed=7, upsample='deconv', test_mode=True)}


def view_meta(scale, direction):
    h, w = int(round(ORI_SHAPE[0] * scale)), int(round(ORI_SHAPE[1] * scale))
    sf = np.array([w / ORI_SHAPE[1], h / ORI_SHAPE[0]] * 2, dtype=np.float32)
    return dict(img_shape=(h, w, 3), ori_shape=ORI_SHAPE, pad_shape=(h, w, 3), scale_factor=sf,
                flip=direction is not None, flip_direction=direction)


def view_maps(scale, direction):
    """P2..P6 of the view's padded image: one seeded set per scale, mirrored along the flip's axis."""
    h, w = int(round(ORI_SHAPE[0] * scale)), int(round(ORI_SHAPE[1] * scale))
    x = synth.make_fpn(1, h, w, 256, seed=300 + int(round(scale * 100)))
    if direction == 'horizontal':
        x = [torch.flip(t, [3]) for t in x]
    elif direction == 'vertical':
        x = [torch.flip(t, [2]) for t in x]
    return [t.contiguous() for t in x]


def proposals():
    return synth.make_rois(1, N_PROPOSALS, ORI_SHAPE[0], ORI_SHAPE[1], seed=PROPOSAL_SEED, min_size=12.0, max_size=96.0)[:, 1:].contiguous()


def case_inputs(case):
    """-> (x: one FPN list per view, proposals [n, 4] of the original image, img_metas: one [meta] per view)."""
    views = CASES[case]
    return [view_maps(s, d) for s, d in views], proposals(), [[view_meta(s, d)] for s, d in views]
