"""The detectors behind the reference's DETECTORS registry, at inference: ``TwoStageDetector`` (mmdet/models/detectors/
two_stage.py over base.py) and its thin registered subclasses -- ``MaskRCNN``, ``FasterRCNN``, ``CascadeRCNN``,
``HybridTaskCascade``, ``MaskScoringRCNN``, ``PointRend``, ``GridRCNN``, ``FastRCNN`` -- the object that runs
``ResNet -> FPN -> RPNHead -> roi_head`` from the image to the results; and ``SingleStageDetector`` (single_stage.py) with
``FCOS``: ``backbone -> neck -> bbox_head``, no RPN and no RoI head.

This module sits above backbones, necks, dense_heads and roi_head; none of them imports it.  It adds no arithmetic to
the model: ``simple_test`` / ``aug_test`` call the parts in the reference's order and add no host wait.  What it does add
is the step in front of the backbone, which the reference does with cv2 on the host: ``preprocess`` turns decoded uint8
HWC images into the normalised, padded batch in ONE launch (``ops.preprocess_u8``: Resize(keep_ratio) -> RandomFlip ->
Normalize -> Pad -> ImageToTensor -> collate) and writes the metas the reference's ``Collect`` would; ``detect`` reads the
views from a config's ``test_pipeline`` and runs them.  ``load_checkpoint`` takes an mmcv-style checkpoint of the whole
detector.  Training (``forward_train``), ``forward_dummy``, the ``async_*`` methods and ``show_result`` are not built."""
import numpy as np
import torch
import torch.nn as nn

from . import backbones, dense_heads, necks, roi_head  # noqa: F401  (each registers its section's classes)
from . import ops
from .postprocess import _bbox2result_host, _to_host
from .registry import DETECTORS, _to_cfgdict, build_backbone, build_head, build_neck


# ---------------------------------------------------------------------------------------------- the pipeline's host side
def rescale_size(h, w, img_scale):
    """mmcv ``rescale_size`` as ``Resize(keep_ratio=True)`` uses it (transforms.py:198-213): the image (h, w) scaled by
    ``s = min(max_long / max(h, w), max_short / min(h, w))`` for ``img_scale`` = (a, b) in either order ->
    (nh, nw, scale_factor float32 [nw / w, nh / h, nw / w, nh / h])."""
    if isinstance(img_scale, (int, float)) or len(img_scale) != 2:
        raise NotImplementedError(f'rescale_size: img_scale={img_scale!r}; a (long edge, short edge) pair expected '
                                  '(a plain scale factor is not built)')
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'rescale_size: an empty image {h} x {w}')
    max_long, max_short = max(img_scale), min(img_scale)
    s = min(max_long / max(h, w), max_short / min(h, w))
    nw, nh = int(w * float(s) + 0.5), int(h * float(s) + 0.5)
    w_scale, h_scale = nw / w, nh / h
    return nh, nw, np.array([w_scale, h_scale, w_scale, h_scale], dtype=np.float32)


# the transforms of a test pipeline that carry no arithmetic of their own here
_PASSIVE_TRANSFORMS = ('LoadImageFromFile', 'LoadImageFromWebcam', 'ImageToTensor', 'Collect', 'DefaultFormatBundle')


def parse_test_pipeline(cfg_or_pipeline):
    """What ``detect`` needs of the reference's ``test_pipeline`` (a config holding one -- ``test_pipeline`` or
    ``data.test.pipeline`` -- or the list itself, tuples or JSON lists): dict(img_scales [(a, b), ...], flip,
    flip_directions, keep_ratio, img_norm_cfg, size_divisor) from its ``MultiScaleFlipAug``.  Raises NotImplementedError for
    what ``preprocess`` does not do: ``scale_factor=``, ``Pad(size=)``, a transform it does not know."""
    p = cfg_or_pipeline
    if isinstance(p, dict):
        if 'test_pipeline' in p:
            p = p['test_pipeline']
        elif 'data' in p and 'test' in p['data'] and 'pipeline' in p['data']['test']:
            p = p['data']['test']['pipeline']
        else:
            raise KeyError('parse_test_pipeline: the config has neither test_pipeline nor data.test.pipeline')
    if not isinstance(p, (list, tuple)):
        raise TypeError(f'parse_test_pipeline: a config or a list of transforms expected, got {type(p).__name__}')
    aug = [t for t in p if t.get('type') == 'MultiScaleFlipAug']
    if len(aug) != 1:
        raise ValueError(f'parse_test_pipeline: exactly one MultiScaleFlipAug expected, found {len(aug)}')
    for t in p:
        if t.get('type') not in _PASSIVE_TRANSFORMS + ('MultiScaleFlipAug',):
            raise NotImplementedError(f"parse_test_pipeline: transform {t.get('type')!r} is not built")
    aug = aug[0]
    if aug.get('scale_factor') is not None or aug.get('img_scale') is None:
        raise NotImplementedError('parse_test_pipeline: MultiScaleFlipAug(scale_factor=...) is not built; img_scale expected')
    s = aug['img_scale']
    if len(s) == 2 and all(isinstance(v, (int, float)) for v in s):
        s = [s]
    scales = [tuple(v) for v in s]
    if not scales or any(len(v) != 2 for v in scales):
        raise ValueError(f"parse_test_pipeline: img_scale={aug['img_scale']!r}: a pair or a list of pairs expected")
    d = aug.get('flip_direction', 'horizontal')
    out = dict(img_scales=scales, flip=bool(aug.get('flip', False)), flip_directions=list(d) if isinstance(d, (list, tuple)) else [d],
               keep_ratio=False, resize=False, img_norm_cfg=None, size_divisor=None, random_flip=False)
    for t in aug.get('transforms', []):
        kind = t.get('type')
        if kind == 'Resize':
            out['resize'], out['keep_ratio'] = True, bool(t.get('keep_ratio', True))
        elif kind == 'RandomFlip':
            out['random_flip'] = True
        elif kind == 'Normalize':
            out['img_norm_cfg'] = dict(mean=list(t['mean']), std=list(t['std']), to_rgb=bool(t.get('to_rgb', True)))
        elif kind == 'Pad':
            if t.get('size') is not None or t.get('pad_val', 0) != 0:
                raise NotImplementedError('parse_test_pipeline: Pad(size=...) / a pad value other than 0 is not built')
            out['size_divisor'] = t.get('size_divisor')
        elif kind not in _PASSIVE_TRANSFORMS:
            raise NotImplementedError(f'parse_test_pipeline: transform {kind!r} is not built')
    if out['img_norm_cfg'] is None:
        raise ValueError('parse_test_pipeline: the pipeline has no Normalize')
    if not out['resize']:
        raise NotImplementedError('parse_test_pipeline: MultiScaleFlipAug without a Resize transform is not built')
    if not out.pop('random_flip'):
        out['flip'] = False             # (test_time_aug.py:78-81: flip has no effect without RandomFlip)
    out.pop('resize')
    return out


def preprocess(images, img_norm_cfg, img_scale=None, keep_ratio=True, flip=False, flip_direction='horizontal',
               size_divisor=32):
    """The reference's test pipeline for one view of B images, one launch: ``images`` a list of uint8 [h, w, 3] device
    tensors (decoded, BGR as cv2 loads them when ``to_rgb``) -> (img [B, 3, Hp, Wp] float32, img_metas).  ``img_scale``
    None: no resize.  The metas carry ``Collect``'s keys -- ``ori_shape``, ``img_shape``, ``pad_shape`` (the batch's, as
    after collate), ``scale_factor`` (float32 [4]), ``flip``, ``flip_direction``, ``img_norm_cfg``."""
    if not keep_ratio:
        raise NotImplementedError('preprocess: Resize(keep_ratio=False) is not built')
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError('preprocess: a non-empty list of images expected')
    if flip and flip_direction not in ops.AUG_FLIP_CODES:
        raise ValueError(f"preprocess: invalid flipping direction '{flip_direction}'")
    mean = np.asarray(img_norm_cfg['mean'], dtype=np.float32)
    std = np.asarray(img_norm_cfg['std'], dtype=np.float32)
    if mean.shape != (3,) or std.shape != (3,):
        raise ValueError('preprocess: img_norm_cfg needs three means and three stds')
    stdinv = (1.0 / np.asarray(img_norm_cfg['std'], dtype=np.float64)).astype(np.float32)
    to_rgb = bool(img_norm_cfg.get('to_rgb', True))
    sizes, factors = [], []
    for im in images:
        h, w = int(im.shape[0]), int(im.shape[1])
        if img_scale is None:
            nh, nw, sf = h, w, np.ones(4, dtype=np.float32)
        else:
            nh, nw, sf = rescale_size(h, w, img_scale)
        sizes.append((nh, nw))
        factors.append(sf)
    d = int(size_divisor) if size_divisor else 1
    Hp = max(-(-nh // d) * d for nh, _ in sizes)
    Wp = max(-(-nw // d) * d for _, nw in sizes)
    img = ops.preprocess_u8(images, sizes, [flip_direction if flip else None] * len(images), mean, stdinv, to_rgb, (Hp, Wp))
    metas = [dict(ori_shape=(int(im.shape[0]), int(im.shape[1]), 3), img_shape=(nh, nw, 3), pad_shape=(Hp, Wp, 3),
                  scale_factor=sf, flip=bool(flip), flip_direction=flip_direction if flip else None,
                  img_norm_cfg=dict(mean=mean, std=std, to_rgb=to_rgb))
             for im, (nh, nw), sf in zip(images, sizes, factors)]
    return img, metas


# ---------------------------------------------------------------------------------------------- checkpoints
def load_checkpoint(model, filename_or_dict, strict=False, map_location='cpu'):
    """Load an mmcv-style checkpoint into ``model``: a file written by ``torch.save`` or the dict itself, either
    ``{'state_dict': ..., 'meta': ...}`` or a bare state dict; a leading ``module.`` (DataParallel) is stripped from the
    keys.  Always returns ``(meta, missing_keys, unexpected_keys)`` -- ``meta`` the checkpoint's (``CLASSES`` ...), {} for a
    bare state dict.  ``strict``: missing or unexpected keys raise RuntimeError naming them, and nothing is loaded."""
    ckpt = filename_or_dict
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt, map_location=map_location)
    if not isinstance(ckpt, dict):
        raise RuntimeError(f'load_checkpoint: no state dict found in {filename_or_dict!r}')
    state = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt
    meta = dict(ckpt.get('meta') or {}) if 'state_dict' in ckpt else {}
    state = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state.items()}
    own = model.state_dict()
    missing = [k for k in own if k not in state]
    unexpected = [k for k in state if k not in own]
    if strict and (missing or unexpected):
        raise RuntimeError(f'load_checkpoint: missing keys {missing}, unexpected keys {unexpected}')
    model.load_state_dict({k: v for k, v in state.items() if k in own}, strict=False)
    return meta, missing, unexpected


# ---------------------------------------------------------------------------------------------- the detectors
def _sub_cfg(cfg, key):
    return None if cfg is None else _to_cfgdict(cfg[key])


class _DetectorBase(nn.Module):
    """What ``BaseDetector`` (base.py) gives every detector at inference: the features, ``forward_test`` / ``forward``'s
    dispatch over the views, the path from decoded images, and the refusals."""

    @property
    def with_neck(self):
        return hasattr(self, 'neck') and self.neck is not None

    async def async_simple_test(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.async_simple_test: the async test paths of the RPN and RoI heads '
                                  'are not built')

    async def aforward_test(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.aforward_test: the async test paths of the RPN and RoI heads are '
                                  'not built')

    def show_result(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.show_result: drawing (mmcv.imshow_det_bboxes, cv2) is not built')

    def extract_feat(self, img):
        """two_stage.py:80-85: backbone, then the neck when there is one."""
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    def extract_feats(self, imgs):
        """base.py:54-65: one ``extract_feat`` per view."""
        assert isinstance(imgs, list)
        return [self.extract_feat(img) for img in imgs]

    def forward_test(self, imgs, img_metas, **kwargs):
        """base.py:123-158: ``imgs`` / ``img_metas`` hold one entry per view; one view goes to ``simple_test``, several
        to ``aug_test``.  (The reference's ``samples_per_gpu == 1`` assertion is not made.)"""
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError(f'{name} must be a list, but got {type(var)}')
        num_augs = len(imgs)
        if num_augs != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        if num_augs == 1:
            if 'proposals' in kwargs:
                kwargs['proposals'] = kwargs['proposals'][0]
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        assert 'proposals' not in kwargs
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas, return_loss=False, **kwargs):
        """base.py:160-173, with inference as the default: ``return_loss=True`` is ``forward_train``, which raises."""
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    # ------------------------------------------------------------------ from decoded images
    def _on_device(self, images):
        dev = next(self.parameters()).device
        if isinstance(images, (np.ndarray, torch.Tensor)) and images.ndim == 3:
            images = [images]
        out = []
        for im in images:
            if isinstance(im, np.ndarray):
                if im.dtype != np.uint8:
                    raise TypeError(f'detect: uint8 images expected, got {im.dtype}')
                im = torch.from_numpy(np.ascontiguousarray(im)).pin_memory().to(dev, non_blocking=True)
            out.append(im)
        return out

    def detect(self, images, cfg_or_pipeline, rescale=True, **kw_test):
        """From decoded uint8 HWC images (device tensors, or host numpy arrays, which are copied up) to results, the views
        read from the config's ``test_pipeline`` (``parse_test_pipeline``).  One scale and no flip: one ``preprocess``
        launch and ``simple_test`` (one image: its result; several: the list).  Several scales or ``flip=True``:
        ``aug_test`` over the views in ``MultiScaleFlipAug``'s order, one ``preprocess`` launch per view; test-time
        augmentation runs one image at a time, so several images give the list of their results.  Further keywords
        (``encode=`` of the two-stage detectors) go to ``simple_test`` / ``aug_test``."""
        p = parse_test_pipeline(cfg_or_pipeline)
        images = self._on_device(images)
        views = [(s, f, d) for s in p['img_scales']
                 for f, d in [(False, None)] + ([(True, d) for d in p['flip_directions']] if p['flip'] else [])]
        kw = dict(keep_ratio=p['keep_ratio'], size_divisor=p['size_divisor'])
        if len(views) == 1:
            img, metas = preprocess(images, p['img_norm_cfg'], img_scale=views[0][0], **kw)
            return self.simple_test(img, metas, rescale=rescale, **kw_test)
        results = []
        for im in images:
            imgs, metas = [], []
            for s, f, d in views:
                img, m = preprocess([im], p['img_norm_cfg'], img_scale=s, flip=f, flip_direction=d or 'horizontal', **kw)
                imgs.append(img)
                metas.append(m)
            results.append(self.aug_test(imgs, metas, rescale=rescale, **kw_test))
        return results[0] if len(images) == 1 else results


@DETECTORS.register_module()
class TwoStageDetector(_DetectorBase):
    """``TwoStageDetector`` -- two_stage.py:9-211 on ``BaseDetector`` (base.py).  ``state_dict`` keys: ``backbone.*``,
    ``neck.*``, ``rpn_head.*``, ``roi_head.*``, the reference's.  ``rpn_head`` gets ``test_cfg.rpn`` and ``roi_head``
    ``test_cfg.rcnn`` (two_stage.py:26-46), in copies: the caller's config is not changed.  ``pretrained`` is stored and
    otherwise ignored (no model zoo).  Inference only."""

    def __init__(self, backbone, neck=None, rpn_head=None, roi_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.fp16_enabled = False
        self.backbone = build_backbone(dict(backbone))
        if neck is not None:
            self.neck = build_neck(dict(neck))
        if rpn_head is not None:
            rpn_head_ = dict(rpn_head)
            rpn_head_.update(train_cfg=_sub_cfg(train_cfg, 'rpn'), test_cfg=_sub_cfg(test_cfg, 'rpn'))
            self.rpn_head = build_head(rpn_head_)
        if roi_head is not None:
            roi_head_ = dict(roi_head)
            roi_head_.update(train_cfg=_sub_cfg(train_cfg, 'rcnn'), test_cfg=_sub_cfg(test_cfg, 'rcnn'))
            self.roi_head = build_head(roi_head_)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.pretrained = pretrained

    # ------------------------------------------------------------------ what the detector has (base.py:22-47, two_stage.py:50-58)
    @property
    def with_rpn(self):
        return hasattr(self, 'rpn_head') and self.rpn_head is not None

    @property
    def with_roi_head(self):
        return hasattr(self, 'roi_head') and self.roi_head is not None

    @property
    def with_shared_head(self):
        return hasattr(self.roi_head, 'shared_head') and self.roi_head.shared_head is not None

    @property
    def with_bbox(self):
        return hasattr(self.roi_head, 'bbox_head') and self.roi_head.bbox_head is not None

    @property
    def with_mask(self):
        return hasattr(self.roi_head, 'mask_head') and self.roi_head.mask_head is not None

    # ------------------------------------------------------------------ refusals
    def forward_train(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.forward_train: backbone, neck and RPN training (their backward, the '
                                  'anchor targets and the RPN losses) are not built; the detector runs at inference only')

    def forward_dummy(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.forward_dummy: the RoI heads\' forward_dummy (the flops counter\'s '
                                  'path) is not built')

    # ------------------------------------------------------------------ inference
    def simple_test(self, img, img_metas, proposals=None, rescale=False, encode=False):
        """two_stage.py:187-199.  One image: what ``roi_head.simple_test`` returns.  B > 1 images (the reference asserts
        one): ``roi_head.batch_simple_test``'s list of B such results.  ``proposals``: used instead of the RPN's."""
        assert self.with_bbox, 'Bbox head must be implemented.'
        if proposals is None and not self.with_rpn:
            raise ValueError(f'{type(self).__name__}.simple_test: no rpn_head: pass proposals')
        x = self.extract_feat(img)
        if proposals is None:
            proposal_list = self.rpn_head.simple_test_rpn(x, img_metas)
        else:
            proposal_list = proposals
        if len(img_metas) == 1:
            return self.roi_head.simple_test(x, proposal_list, img_metas, rescale=rescale, encode=encode)
        return self.roi_head.batch_simple_test(x, proposal_list, img_metas, rescale=rescale, encode=encode)

    def aug_test(self, imgs, img_metas, rescale=False, encode=False):
        """two_stage.py:201-211: the views' features, the RPN's proposals merged over the views, the RoI head's
        ``aug_test``."""
        x = self.extract_feats(imgs)
        proposal_list = self.rpn_head.aug_test_rpn(x, img_metas)
        return self.roi_head.aug_test(x, proposal_list, img_metas, rescale=rescale, encode=encode)


@DETECTORS.register_module()
class MaskRCNN(TwoStageDetector):
    """mask_rcnn.py: the constructor only."""


@DETECTORS.register_module()
class FasterRCNN(TwoStageDetector):
    """faster_rcnn.py: the constructor only."""


@DETECTORS.register_module()
class CascadeRCNN(TwoStageDetector):
    """cascade_rcnn.py: the constructor, and a ``show_result`` (not built here)."""


@DETECTORS.register_module()
class HybridTaskCascade(CascadeRCNN):
    """htc.py: ``with_semantic`` beside CascadeRCNN."""

    @property
    def with_semantic(self):
        return self.roi_head.with_semantic


@DETECTORS.register_module()
class MaskScoringRCNN(TwoStageDetector):
    """mask_scoring_rcnn.py: the constructor only."""


@DETECTORS.register_module()
class PointRend(TwoStageDetector):
    """point_rend.py: the constructor only."""


@DETECTORS.register_module()
class GridRCNN(TwoStageDetector):
    """grid_rcnn.py: the constructor only."""


@DETECTORS.register_module()
class FastRCNN(TwoStageDetector):
    """fast_rcnn.py: no RPN -- ``proposals`` come with the call."""

    def __init__(self, backbone, roi_head, train_cfg, test_cfg, neck=None, pretrained=None):
        super().__init__(backbone=backbone, neck=neck, roi_head=roi_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained)

    def forward_test(self, imgs, img_metas, proposals, **kwargs):
        """fast_rcnn.py:24-55: one view only, with its proposals."""
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError(f'{name} must be a list, but got {type(var)}')
        num_augs = len(imgs)
        if num_augs != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        if num_augs != 1:
            raise NotImplementedError('FastRCNN.forward_test: test-time augmentation with given proposals is not built '
                                      '(nor is it in the reference)')
        return self.simple_test(imgs[0], img_metas[0], proposals[0], **kwargs)


# ---------------------------------------------------------------------------------------------- single-stage detectors
@DETECTORS.register_module()
class SingleStageDetector(_DetectorBase):
    """``SingleStageDetector`` -- single_stage.py:9-154 on ``BaseDetector``: ``backbone -> neck -> bbox_head``, no RPN and
    no RoI head.  ``state_dict`` keys: ``backbone.*``, ``neck.*``, ``bbox_head.*``, the reference's.  ``test_cfg`` goes
    whole to the head (single_stage.py:28-30), in a copy: the caller's config is not changed.  ``pretrained`` is stored
    and otherwise ignored.  Inference only; the detector adds no arithmetic of its own."""

    def __init__(self, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.fp16_enabled = False
        self.backbone = build_backbone(dict(backbone))
        if neck is not None:
            self.neck = build_neck(dict(neck))
        bbox_head_ = dict(bbox_head)
        bbox_head_.update(train_cfg=None if train_cfg is None else _to_cfgdict(train_cfg),
                          test_cfg=None if test_cfg is None else _to_cfgdict(test_cfg))
        self.bbox_head = build_head(bbox_head_)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.pretrained = pretrained

    @property
    def with_bbox(self):
        return hasattr(self, 'bbox_head') and self.bbox_head is not None

    # ------------------------------------------------------------------ refusals
    def forward_train(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.forward_train: backbone, neck and dense-head training (their '
                                  'backward, the point targets and the losses) are not built; the detector runs at inference only')

    def forward_dummy(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.forward_dummy: the flops counter\'s path is not built')

    def aug_test(self, imgs, img_metas, rescale=False):
        """single_stage.py:152-154: the reference raises too."""
        raise NotImplementedError(f'{type(self).__name__}.aug_test: test-time augmentation of a single-stage detector is not '
                                  'built (nor is it in the reference)')

    # ------------------------------------------------------------------ inference
    def simple_test(self, img, img_metas, rescale=False):
        """single_stage.py:116-150.  One image: its ``bbox2result`` list (one [k, 5] array per class).  B > 1 images (the
        reference returns the first only): the list of B such results.  The detections of all images reach the host in
        one copy."""
        x = self.extract_feat(img)
        outs = self.bbox_head(x)
        bbox_list = self.bbox_head.get_bboxes(*outs, img_metas, rescale=rescale)
        host = _to_host(*[t for pair in bbox_list for t in pair])
        results = [_bbox2result_host(host[2 * b], host[2 * b + 1], self.bbox_head.num_classes) for b in range(len(bbox_list))]
        return results[0] if len(img_metas) == 1 else results


@DETECTORS.register_module()
class FCOS(SingleStageDetector):
    """fcos.py: the constructor only."""
