"""Seeded inputs and weights of the Cascade Mask R-CNN fixture (g21_cascade.npz), shared by
tests/golden/make_golden_cascade.py and the tests: the fixture stores outputs only (three bbox heads hold 42 M weights)."""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from dynamask_amd import synth  # noqa: E402

ORI_SHAPE = (128, 160, 3)
N_PROPOSALS = 48
PROPOSAL_SEED = 421
TEST_CFG = dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=0.5)
# aug_test: two scales x {no flip, horizontal flip}
AUG_VIEWS = [(1.0, None), (1.0, 'horizontal'), (1.5, None), (1.5, 'horizontal')]


def head_state(shapes):
    """Seeded parameters for ``shapes`` {key: shape} (the ``bbox_head.*`` / ``mask_head.*`` entries of a CascadeRoIHead
    state_dict): He-scaled weights, small biases; the regression layers scaled down so that the three stages move the
    boxes by a few pixels each, the classifiers scaled up so that some of the averaged scores pass ``score_thr``."""
    g = torch.Generator().manual_seed(21)
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
                w = w * 4.0                          # confident enough for some scores above score_thr
            out[k] = w
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def view_meta(scale, direction):
    h, w = int(round(ORI_SHAPE[0] * scale)), int(round(ORI_SHAPE[1] * scale))
    sf = np.array([w / ORI_SHAPE[1], h / ORI_SHAPE[0]] * 2, dtype=np.float32)
    return dict(img_shape=(h, w, 3), ori_shape=ORI_SHAPE, pad_shape=(h, w, 3), scale_factor=sf,
                flip=direction is not None, flip_direction=direction)


def view_maps(scale, direction, seed=2100):
    """P2..P6 of the view's padded image: one seeded set per scale, mirrored along the flip's axis."""
    h, w = int(round(ORI_SHAPE[0] * scale)), int(round(ORI_SHAPE[1] * scale))
    x = synth.make_fpn(1, h, w, 256, seed=seed + int(round(scale * 100)))
    if direction == 'horizontal':
        x = [torch.flip(t, [3]) for t in x]
    elif direction == 'vertical':
        x = [torch.flip(t, [2]) for t in x]
    return [t.contiguous() for t in x]


def proposals(seed=PROPOSAL_SEED, h=ORI_SHAPE[0], w=ORI_SHAPE[1], n=N_PROPOSALS):
    return synth.make_rois(1, n, h, w, seed=seed, min_size=12.0, max_size=96.0)[:, 1:].contiguous()


def simple_inputs():
    """-> (x: the FPN list of one image, proposals [n, 4], img_metas [meta])."""
    meta = view_meta(1.0, None)
    meta['scale_factor'] = 1.0          # (the reference's get_seg_masks takes a float here when rescale=False)
    return view_maps(1.0, None), proposals(), [meta]


def aug_inputs():
    """-> (x: one FPN list per view, proposals [n, 4] of the original image, img_metas: one [meta] per view)."""
    return [view_maps(s, d) for s, d in AUG_VIEWS], proposals(), [[view_meta(s, d)] for s, d in AUG_VIEWS]
