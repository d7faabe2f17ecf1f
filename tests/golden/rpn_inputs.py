"""Seeded inputs and weights of the RPN fixture (g26_rpn.npz: RPNHead of the FPN and the C4 Mask R-CNN configs), shared by
tests/golden/make_golden_rpn.py and the tests: the fixture stores outputs only.  The maps of a padded 160 x 224 batch of
two images with different ``img_shape``s."""
import math

import torch

PAD_H, PAD_W = 160, 224
IMG_SHAPES = ((160, 224, 3), (150, 200, 3))      # image 1 is smaller than the padded batch: its boxes clip earlier
BATCH = len(IMG_SHAPES)
FEAT_SEED = 262626
# seeds the generator tries in order; the one it settles on is stored in the fixture (``seed``)
SEEDS = tuple(range(26, 126))
# form -> the config its ``model.rpn_head`` / ``test_cfg.rpn`` come from, and the ``nms_pre`` of the get_bboxes run
# (None: the config's own).  FPN: 6720 / 1680 / 420 / 105 / 36 anchors per level, the config's 1000 cuts the first two.
# C4: 15 x 10 x 14 = 2100 anchors, the config's 6000 would cut nothing.
FORMS = {'fpn': ('configs/_base_/models/mask_rcnn_r50_fpn.py', None),
         'c4': ('configs/_base_/models/mask_rcnn_r50_caffe_c4.py', 1200)}


def map_sizes(strides):
    return [(math.ceil(PAD_H / s), math.ceil(PAD_W / s)) for s in strides]


def img_metas():
    return [dict(ori_shape=s, img_shape=s, pad_shape=(PAD_H, PAD_W, 3), scale_factor=1.0, flip=False, flip_direction=None)
            for s in IMG_SHAPES]


def feats(in_channels, strides, seed=FEAT_SEED):
    """Per level [BATCH, in_channels, H, W], image b of level l from seed + 16 * b + l."""
    return [torch.cat([torch.randn(1, in_channels, h, w, generator=torch.Generator().manual_seed(seed + 16 * b + l))
                       for b in range(BATCH)]).contiguous()
            for l, (h, w) in enumerate(map_sizes(strides))]


def head_state(shapes, seed):
    """Seeded parameters for ``shapes`` {key: shape} of an RPNHead state_dict with the spread of c4_inputs.head_state:
    He-scaled weights, biases 0.1 x normal -- not the std-0.01 initialiser, so that the logits span several units."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('.weight'):
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            out[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        else:
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def synthetic_maps(num_anchors, strides, seed):
    """(cls_scores, bbox_preds) per level, [BATCH, A, H, W] and [BATCH, 4 A, H, W]: every (image, level)'s logits are a
    seeded permutation of linspace(-4, 4, A H W) (neighbouring scores at least 2e-5 apart at 6720 values); the deltas are
    0.5 x normal, dw and dh around -1 (boxes of a third of their anchors: with full-size boxes a dozen of the million
    same-level pairs land within 1e-4 of the NMS threshold, whatever the seed), with one value in 16 scaled by 12 --
    beyond wh_ratio_clip's |log(16 / 1000)| = 4.14 and far enough to leave the image; the boxes blown up that way clip
    to the whole image and suppress one another."""
    g = torch.Generator().manual_seed(int(seed))
    cls, reg = [], []
    for A, (h, w) in zip(num_anchors, map_sizes(strides)):
        n = A * h * w
        c = torch.stack([torch.linspace(-4, 4, n)[torch.randperm(n, generator=g)].view(A, h, w) for _ in range(BATCH)])
        d = 0.5 * torch.randn(BATCH, A, 4, h, w, generator=g)
        d[:, :, 2:] -= 1.0
        d = d.view(BATCH, 4 * A, h, w)
        far = torch.rand(d.shape, generator=g) < 1 / 16
        cls.append(c.contiguous())
        reg.append(torch.where(far, d * 12, d).contiguous())
    return cls, reg


# The float64 twins are stored as the fp32 result's error against them, scaled and rounded to float16: a twin is
# reproduced to 5e-4 of that error (some 1e-9 of a value), at 6 bytes a value instead of 12.
ERR_SCALE = float(2 ** 20)


def pack_err(v32, v64):
    import numpy as np
    err = (np.asarray(v32, np.float64) - np.asarray(v64, np.float64)) * ERR_SCALE
    assert float(np.abs(err).max(initial=0.0)) < 6.0e4, 'the fp32 result is too far from its float64 twin for float16'
    return err.astype(np.float16)


def unpack_f64(v32, err16):
    import numpy as np
    return np.asarray(v32, np.float64) - np.asarray(err16, np.float64) / ERR_SCALE
