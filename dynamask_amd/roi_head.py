"""The RoI heads behind the reference's HEADS registry, in the reference's class tree: ``StandardRoIHead``
(standard_roi_head.py + test_mixins.py) is the base of ``DynaMaskRoIHead``, ``RefineRoIHead``, ``PointRendRoIHead``,
``MaskScoringRoIHead``, ``PointRefineRoIHead``, ``GridRoIHead``, ``DoubleHeadRoIHead`` and ``CascadeRoIHead``.

The base holds the constructor (incl. ``base_roi_head.py:10-58``'s MaskPre, Quirk Q4), the assigner / sampler, the bbox
branch, the one-image / batched / test-time-augmentation entry points and one mask-test template over a head's
``_mask_logits``.  ``DynaMaskRoIHead`` mirrors ``mmdet/models/roi_heads/dynamask_roi_head.py:10-158`` for the MASK path:
``_mask_forward``, ``get_mask_label`` (MaskPre + straight-through Gumbel selector), ``_mask_forward_train`` (assigner +
sampler, bbox branch losses, mask targets on the device; dynamask_roi_head.py:21-46) and the merged logits of the test.
"""
import os

import numpy as np
import torch
import torch.nn as nn

# the modules whose classes the configs name: importing them here fills the registries the constructors build from
from . import bbox_heads, losses, mask_heads, roi_extractors, shared_heads  # noqa: F401
from . import ops, streams, train_path
from .assigners import build_assigner, build_sampler
from .graphs import BATCH_BUCKETS, BUCKETS, GraphedMaskLogits
from .layers import _BN, _Conv, _Linear
from .mask_heads import run_steps
from .postprocess import (_bbox2result_host, _mask_threshold, _paste_geometry, _to_host, _to_host_pending, bbox2result,
                          group_mask_scores, multiclass_nms, multiclass_nms_batch, paste_segms, select_label_channel)
from .registry import HEADS, SHARED_HEADS, build, build_head, build_roi_extractor


def bbox2roi(bbox_list):
    """mmdet/core/bbox/transforms.py:54-73."""
    rois_list = []
    for img_id, bboxes in enumerate(bbox_list):
        if bboxes.size(0) > 0:
            img_inds = bboxes.new_full((bboxes.size(0), 1), img_id)
            rois = torch.cat([img_inds, bboxes[:, :4]], dim=-1)
        else:
            rois = bboxes.new_zeros((0, 5))
        rois_list.append(rois)
    return torch.cat(rois_list, 0)


# inference: the final x2 upsample + both boundary merges as one launch per RoI chunk (0: the four launches, same bits)
FUSED_MERGE_TAIL = [os.environ.get('DM_FUSED_MERGE_TAIL', '1') != '0']
# training: MaskPre's conv1 on the P2 map + a 128-channel extraction (train_path.MaskPreMapFn); 0 = the reference's order
_MASKPRE_ON_MAP = os.environ.get('DM_MASKPRE_MAP', '1') != '0'


class MaskPre(nn.Module):
    """Resolution predictor -- base_roi_head.py:10-27."""

    def __init__(self):
        super().__init__()
        self.conv1 = _Conv(256, 128, 1)
        self.bn1 = _BN(128)
        self.conv2 = _Conv(128, 16, 3)
        self.bn2 = _BN(16)
        self.fc1 = _Linear(3136, 512)
        self.fc2 = _Linear(512, 4)
        # the selector's input: exact fp32 in every precision mode (dynamask_amd/precision.py), so exits cannot move
        self.conv1.exact = self.conv2.exact = True
        # torch defaults of the reference (nn.Conv2d): kaiming_uniform(a=sqrt(5))
        for m, ref in ((self.conv1, nn.Conv2d(256, 128, 1)), (self.conv2, nn.Conv2d(128, 16, 3, padding=1))):
            with torch.no_grad():
                m.weight.copy_(ref.weight)
                m.bias.copy_(ref.bias)

    def _bn_pool(self, x, bn):
        if self.training:
            mean, var = ops.bn_stats(x, bn.running_mean, bn.running_var, bn.momentum)
            bn.num_batches_tracked += 1
        else:
            mean, var = bn.running_mean, bn.running_var
        return ops.bn_relu_maxpool(x, mean, var, bn.weight.detach(), bn.bias.detach(), bn.eps)

    def forward(self, x):
        x = self._bn_pool(self.conv1.run(x), self.bn1)
        return self._tail(x)

    def _tail(self, x):
        x = self._bn_pool(self.conv2.run(x), self.bn2)
        x = x.reshape(x.size(0), 3136)
        x = self.fc1.run(x, relu=True)
        return self.fc2.run(x)

    @torch.no_grad()
    def forward_from_map(self, feat_map, rois, extractor):
        """Inference shortcut (eval mode): ``conv1`` is 1x1, hence linear per pixel, and RoIAlign is
        a linear interpolation, so  conv1(RoIAlign(x)) = RoIAlign(W1 x) + b1  (the bias is added
        after the RoIAlign: samples outside the map count as 0 on both sides).  W1 is applied once
        to the whole FPN map (4.4 GFLOP per image instead of 0.21 GFLOP per RoI) and RoIAlign56
        extracts 128 channels instead of 256; b1 is folded into the BatchNorm shift.  Same value
        as ``forward(extractor([feat_map], rois))`` up to fp32 rounding (~1e-6)."""
        assert not self.training, 'train-mode BatchNorm statistics are taken on the per-RoI tensor'
        wq = self.conv1.packed([feat_map.shape[1]])
        y_map = ops.conv2d([feat_map], wq, None, self.conv1.out_channels, 1)          # no bias
        roi = extractor([y_map], rois)                                               # [N, 128, 56, 56]
        bn = self.bn1
        x = ops.bn_relu_maxpool(roi, (bn.running_mean - self.conv1.bias.detach()).contiguous(), bn.running_var,
                                bn.weight.detach(), bn.bias.detach(), bn.eps)
        return self._tail(x)

def merge_stage_preds(stage_instance_preds):
    """Boundary-aware coarse-to-fine merge, dynamask_roi_head.py:138-149 = refine_roi_head.py:102-113
    (in place on the finer logits, as the reference; the 14x14 exit is unused)."""
    preds = stage_instance_preds[1:]
    for idx in range(len(preds) - 1):
        ops.boundary_merge_(preds[idx], preds[idx + 1])
    return preds[-1]


@HEADS.register_module()
class StandardRoIHead(nn.Module):
    """``StandardRoIHead`` -- mmdet/models/roi_heads/standard_roi_head.py:10-290 + ``MaskTestMixin`` (test_mixins.py):
    the RoI head of configs/mask_rcnn and configs/carafe (BASELINE configs[4]), whose mask head is ``FCNMaskHead``, and
    the base of the other three RoI heads, as in the reference.  It holds what they share: the constructor, the
    assigner / sampler, the bbox branch, ``simple_test`` / ``batch_simple_test`` / ``aug_test`` and the mask-test
    template.  A head supplies its mask prediction through ``_mask_logits(x, mask_rois, labels)`` -> [n, C, S, S] and
    its (C, S) through ``_mask_logits_size``; the template does the rest once for every head: rescale, ``bbox2roi``,
    the empty case, the label-channel selection, the paste, the device -> host copy and the grouping by class.  A head
    whose mask test returns more than the masks (MaskScoringRoIHead's scores) overrides ``_mask_test_pred`` and
    ``_mask_test_result``.  Here the
    mask branch is the stock one: ``_mask_forward(x, rois)`` -> ``{'mask_pred': [N, classes, 28, 28], 'mask_feats'}``.
    ``BaseRoIHead.__init__`` of the fork builds ``mask_predictor`` / ``semantic_roi_extractor`` for EVERY RoI head (Quirk
    Q4), so the ``state_dict`` carries the ``mask_predictor.*`` keys here too, as the reference's does.
    ``shared_head=`` (the C4 configs: ``ResLayer``, ResNet layer4 per RoI) and ``mask_roi_extractor=None`` (the mask branch
    shares the bbox extractor) follow standard_roi_head.py:28-44: ``_roi_feats`` runs extractor then shared head for both
    branches, inference only.
    Training: ``forward_train`` follows standard_roi_head.py:70-134; its mask loss ends in ``FCNMaskHead.loss``, which
    the fork broke (Quirk Q5) -- it raises here as it does there, the bbox losses and the mask targets are computed."""

    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None,
                 shared_head=None, train_cfg=None, test_cfg=None):
        super().__init__()
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        # bbox branch (inference only): built when configured
        self.bbox_roi_extractor_cfg = bbox_roi_extractor
        self.bbox_head_cfg = bbox_head
        if bbox_head is not None:
            self.bbox_roi_extractor = build_roi_extractor(bbox_roi_extractor)
            self.bbox_head = build_head(bbox_head)
        # standard_roi_head.py:28-44 / base_roi_head.py (shared_head): the C4 configs' per-RoI ResNet stage behind the
        # extractor of both branches.  Only this class's own forward paths apply it (``_roi_feats``): a subclass with a
        # mask or bbox path of its own refuses it here instead of ignoring it.
        if not self._applies_shared_head() and (shared_head is not None or (mask_head is not None and mask_roi_extractor is None)):
            raise NotImplementedError(f'{type(self).__name__}: shared_head / the shared RoI extractor (mask_roi_extractor=None) '
                                      'are built for StandardRoIHead alone (the C4 configs)')
        if shared_head is not None:
            self.shared_head = build(shared_head, SHARED_HEADS)
        if mask_head is not None:
            if mask_roi_extractor is not None:
                self.mask_roi_extractor = build_roi_extractor(mask_roi_extractor)
                self.share_roi_extractor = False
            else:
                if bbox_head is None:
                    raise ValueError('mask_roi_extractor=None shares the bbox RoI extractor: a bbox branch is needed')
                self.share_roi_extractor = True
                self.mask_roi_extractor = self.bbox_roi_extractor
            self.mask_head = build_head(mask_head)
        self.init_assigner_sampler()
        # base_roi_head.py:53-58 (created for every RoI head: Quirk Q4)
        self.semantic_roi_extractor = build_roi_extractor(dict(
            type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', output_size=56, sampling_ratio=0),
            out_channels=256, featmap_strides=[4, ]))
        self.mask_predictor = MaskPre()
        self._mask_graphs = None        # graphs.GraphedMaskLogits of ``_mask_logits`` (enable_inference_graphs)

    def init_assigner_sampler(self):
        """standard_roi_head.py:13-20."""
        self.bbox_assigner = None
        self.bbox_sampler = None
        if self.train_cfg and getattr(self.train_cfg, 'get', None) and self.train_cfg.get('assigner') is not None:
            self.bbox_assigner = build_assigner(self.train_cfg.assigner)
            self.bbox_sampler = build_sampler(self.train_cfg.sampler, context=self)

    @property
    def with_bbox(self):
        return hasattr(self, 'bbox_head') and self.bbox_head is not None

    @property
    def with_mask(self):
        return hasattr(self, 'mask_head') and self.mask_head is not None

    @property
    def with_shared_head(self):
        return hasattr(self, 'shared_head') and self.shared_head is not None

    # the methods of this class through which a shared head reaches both branches (``_roi_feats``)
    _SHARED_HEAD_PATH = ('_bbox_forward', '_mask_forward', '_mask_logits', '_bbox_test_preds', '_mask_test_pred', 'simple_test')

    @classmethod
    def _applies_shared_head(cls):
        """Are this class's forward paths the ones above?  A subclass that overrides one of them has a bbox or mask path
        of its own, which does not apply a shared head."""
        return all(getattr(cls, n) is getattr(StandardRoIHead, n) for n in StandardRoIHead._SHARED_HEAD_PATH)

    def _roi_feats(self, extractor, x, rois):
        """Extractor, then shared head (standard_roi_head.py:138-141, 204-207): the RoI features both branches' heads read.
        A stride-2 shared head reads only the even rows and columns of the extraction, so where the extractor can produce
        just those (``bin_step=2``) it does and the head runs on them (``forward_sampled``); else the dense extraction and
        ``forward``.  Same bits either way."""
        feats = x[:extractor.num_inputs]
        if not self.with_shared_head:
            return extractor(feats, rois)
        if self.shared_head_strided_extraction(extractor, feats):
            return self.shared_head.forward_sampled(extractor(feats, rois, bin_step=2))
        return self.shared_head(extractor(feats, rois))

    def shared_head_strided_extraction(self, extractor, feats):
        """Does ``_roi_feats`` take the strided extraction for these maps?"""
        return (self.STRIDED_EXTRACTION and getattr(self.shared_head, 'stride', 1) == 2 and hasattr(self.shared_head, 'forward_sampled')
                and hasattr(extractor, 'supports_bin_step') and extractor.supports_bin_step(feats, 2))

    STRIDED_EXTRACTION = True      # (tests compare with the dense extraction + ``forward`` by clearing it)

    def init_weights(self, pretrained=None):
        if self.with_mask:
            self.mask_head.init_weights()
            self.mask_roi_extractor.init_weights()

    # ------------------------------------------------------------------ training entry points
    def _assign_and_sample(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        """standard_roi_head.py:86-103: assign gts and sample proposals per image.  Assignment and sampling of every
        image are enqueued first; the host then waits ONCE for all the (positive, negative) counts that size the heads'
        tensors, not once per image (RandomSampler.sample_deferred)."""
        num_imgs = len(img_metas)
        if gt_bboxes_ignore is None:
            gt_bboxes_ignore = [None for _ in range(num_imgs)]
        deferred = hasattr(self.bbox_sampler, 'sample_deferred')
        do_sample = self.bbox_sampler.sample_deferred if deferred else self.bbox_sampler.sample
        sampling_results = []
        for i in range(num_imgs):
            assign_result = self.bbox_assigner.assign(proposal_list[i], gt_bboxes[i], gt_bboxes_ignore[i], gt_labels[i])
            sampling_results.append(do_sample(assign_result, proposal_list[i], gt_bboxes[i], gt_labels[i],
                                              feats=[lvl_feat[i][None] for lvl_feat in x]))
        if deferred:
            sampling_results = self.bbox_sampler.finish_samples(sampling_results)
        return sampling_results

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        """standard_roi_head.py:70-134."""
        if self.with_shared_head:
            raise NotImplementedError(f'{type(self).__name__}.forward_train with a shared head: the backward through the '
                                      'shared head (ResNet layer4) is not built; the C4 configs run inference')
        sampling_results = self._assign_and_sample(x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore)
        losses = dict()
        bbox_results = None
        if self.with_bbox:
            bbox_results = self._bbox_forward_train(x, sampling_results, gt_bboxes, gt_labels, img_metas)
            losses.update(bbox_results['loss_bbox'])
        if self.with_mask:
            mask_results = self._mask_forward_train(x, sampling_results, None if bbox_results is None else bbox_results['bbox_feats'],
                                                    gt_masks, img_metas)
            if mask_results['loss_mask'] is not None:
                losses.update(mask_results['loss_mask'])
        return losses

    def _bbox_forward_train(self, x, sampling_results, gt_bboxes, gt_labels, img_metas):
        """standard_roi_head.py:147-160."""
        rois = bbox2roi([res.bboxes for res in sampling_results]).contiguous()
        if torch.is_grad_enabled():
            bbox_feats = train_path.roi_extract_train(self.bbox_roi_extractor, x, rois)
        else:
            bbox_feats = self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)
        cls_score, bbox_pred = self.bbox_head(bbox_feats)
        bbox_results = dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)
        bbox_targets = self.bbox_head.get_targets(sampling_results, gt_bboxes, gt_labels, self.train_cfg)
        loss_bbox = self.bbox_head.loss(cls_score, bbox_pred, rois, *bbox_targets)
        bbox_results.update(loss_bbox=loss_bbox)
        return bbox_results

    def _mask_forward(self, x, rois=None, pos_inds=None, bbox_feats=None, **kw):
        """standard_roi_head.py:199-215."""
        assert (rois is not None) ^ (pos_inds is not None and bbox_feats is not None)
        if rois is not None:
            mask_feats = self._roi_feats(self.mask_roi_extractor, x, rois.contiguous())
        else:
            mask_feats = bbox_feats[pos_inds].contiguous()
        return dict(mask_pred=self.mask_head(mask_feats), mask_feats=mask_feats)

    def _mask_forward_train(self, x, sampling_results, bbox_feats, gt_masks, img_metas, **kw):
        """standard_roi_head.py:162-197 (the mask branch with its own RoI extractor)."""
        pos_rois = bbox2roi([res.pos_bboxes for res in sampling_results]).contiguous()
        if pos_rois.shape[0] == 0:
            return dict(loss_mask=None)
        mask_results = self._mask_forward(x, pos_rois)
        mask_targets = self.mask_head.get_targets(sampling_results, gt_masks, self.train_cfg)
        pos_labels = torch.cat([res.pos_gt_labels for res in sampling_results])
        loss_mask = self.mask_head.loss(mask_results['mask_pred'], mask_targets, pos_labels)
        mask_results.update(loss_mask=loss_mask, mask_targets=mask_targets)
        return mask_results

    # ------------------------------------------------------------ bbox branch (inference)
    def _bbox_forward(self, x, rois):
        """standard_roi_head.py:135-146 (``bbox_feats``: what the shared head returns, where there is one)."""
        bbox_feats = self._roi_feats(self.bbox_roi_extractor, x, rois)
        cls_score, bbox_pred = self.bbox_head(bbox_feats)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)

    def _bbox_num_classes(self):
        return self.bbox_head.num_classes

    def _bbox_test_preds(self, x, rois, img_metas):
        """The bbox branch of the test entry points: RoIs [N, 5] (batch column = index into ``img_metas``) -> (the RoIs
        the predictions refer to, cls_score, bbox_pred, the bbox head that decodes them).  Here one ``_bbox_forward``;
        CascadeRoIHead runs its stages."""
        res = self._bbox_forward(x, rois)
        return rois, res['cls_score'], res['bbox_pred'], self.bbox_head

    @torch.no_grad()
    def simple_test_bboxes(self, x, img_metas, proposals, rcnn_test_cfg, rescale=False):
        """test_mixins.py:52-71 (BBoxTestMixin.simple_test_bboxes), one image."""
        rois = bbox2roi(proposals).contiguous()
        rois, cls_score, bbox_pred, head = self._bbox_test_preds(x, rois, img_metas)
        return head.get_bboxes(rois, cls_score, bbox_pred, img_metas[0]['img_shape'],
                               img_metas[0]['scale_factor'], rescale=rescale, cfg=rcnn_test_cfg)

    @torch.no_grad()
    def simple_test(self, x, proposal_list, img_metas, proposals=None, rescale=False, encode=False):
        """standard_roi_head.py:217-236: boxes, then masks of the kept detections."""
        det_bboxes, det_labels = self.simple_test_bboxes(x, img_metas, proposal_list, self.test_cfg, rescale=rescale)
        bbox_results = bbox2result(det_bboxes, det_labels, self._bbox_num_classes())
        if not self.with_mask:
            return bbox_results
        segm_results = self.simple_test_mask(x, img_metas, det_bboxes, det_labels, rescale=rescale, encode=encode)
        return bbox_results, segm_results

    # ------------------------------------------------------------ mask test: the hooks of a head
    def _mask_logits(self, x, mask_rois, labels):
        """The mask prediction of the RoIs [n, C, S, S] that is pasted (after the label-channel selection) or merged
        over the views of test-time augmentation.  Here: ``_mask_forward``'s ``mask_pred`` (test_mixins.py:166-168)."""
        with torch.no_grad():
            return self._mask_forward(x, mask_rois)['mask_pred']

    def _mask_logits_size(self):
        """(C, S) of what ``_mask_logits`` returns (the shape of the empty results): FCNMaskHead's logits of the RoI
        extractor's features, upsampled by its ``scale_factor``."""
        h = self.mask_head
        s = self.mask_roi_extractor.roi_layers[0].output_size[0]
        if self.with_shared_head:
            s = -(-s // self.shared_head.stride)        # (the C4 configs: 14 -> 7 features, 14 x 14 logits)
        return h.conv_logits.out_channels, int(s * (h.scale_factor if h.upsample is not None else 1))

    def _segm_num_classes(self):
        """The number of per-class lists of ``simple_test_mask``."""
        return self.mask_head.num_classes

    def _mask_test_pred(self, x, boxes, labels, det_bboxes):
        """The mask prediction that ``simple_test_mask`` / ``batch_simple_test_mask`` paste, for the detections of the
        images of a call (per-image lists: the boxes the mask chain reads, the labels, the detections as given) ->
        (logits [sum n, C, S, S], what ``_mask_test_result`` adds to the masks or None).  Here: the logits of
        ``simple_test_mask_logits`` (one image) / ``batch_simple_test_mask_logits``, nothing beside them."""
        if len(boxes) == 1:
            return self.simple_test_mask_logits(x, boxes[0], labels[0]), None
        return self.batch_simple_test_mask_logits(x, boxes, labels)[0], None

    def _mask_test_result(self, segms, pending, start, count):
        """One image's mask-test result from its per-class ``segms`` and the second value of ``_mask_test_pred``
        (rows start:start + count are the image's; read only after the paste's host wait): here the masks alone."""
        return segms

    # whether ``_mask_test_pred`` gives logits (the paste applies the sigmoid) or probabilities (CascadeRoIHead's merge)
    _mask_test_sigmoid = True

    def _empty_mask_logits(self, ref, channels=None):
        c, s = self._mask_logits_size()
        return ref.new_zeros((0, c if channels is None else channels, s, s))

    def enable_inference_graphs(self, on=True, buckets=None, batch_buckets=None):
        """HIP-graph replay of the mask call: DynaMaskRoIHead's; for the other heads it is a follow-up."""
        if on:
            raise NotImplementedError(f'{type(self).__name__}: HIP-graph capture of its mask call is a follow-up')
        self._mask_graphs = None
        return None

    # ------------------------------------------------------------ mask test: one image
    def simple_test_mask_logits(self, x, det_bboxes, det_labels, scale_factor=1.0, rescale=False):
        """simple_test_mask up to the mask prediction ``_mask_logits`` [n, C, S, S] of the detections (pasting into the
        image is the step after the path).  With ``enable_inference_graphs`` the call replays a graph bucketed on the
        detection count (graphs.BUCKETS; larger counts run eagerly)."""
        if det_bboxes.shape[0] == 0:
            return self._empty_mask_logits(det_bboxes)
        _bboxes = det_bboxes[:, :4] * scale_factor if rescale else det_bboxes
        if self._mask_graphs is not None and not torch.is_grad_enabled():
            # bucketed HIP-graph replay (graphs.py); None: too many RoIs.  The boxes go straight into the graph's RoI buffer.
            merged = self._mask_graphs(x, None, det_labels, boxes=_bboxes)
            if merged is not None:
                return merged
        return self._mask_logits(x, bbox2roi([_bboxes]).contiguous(), det_labels)

    def simple_test_mask(self, x, img_metas, det_bboxes, det_labels, rescale=False, encode=False):
        """test_mixins.py:151-176 (dynamask_roi_head.py:117-158, point_rend_roi_head.py:130-155) -> per-class lists of
        (h, w) bool masks: the detections' ``simple_test_mask_logits``, their label channel pasted into the image.
        ``encode=True`` (extension): per-class lists of COCO RLE dicts instead, i.e. the result after the caller's
        ``encode_mask_results`` (apis/test.py:52-57), produced on the device."""
        num_classes = self._segm_num_classes()
        if det_bboxes.shape[0] == 0:
            return self._mask_test_result([[] for _ in range(num_classes)], None, 0, 0)
        _bboxes, scale_factor = self._mask_boxes(det_bboxes, img_metas[0]['scale_factor'], rescale)
        logits, pending = self._mask_test_pred(x, [_bboxes], [det_labels], [det_bboxes])
        segms = paste_segms(select_label_channel(logits, det_labels), _bboxes, det_labels, self.test_cfg,
                            img_metas[0]['ori_shape'], scale_factor, rescale, encode=encode, num_classes=num_classes,
                            apply_sigmoid=self._mask_test_sigmoid)
        return self._mask_test_result(segms, pending, 0, int(det_bboxes.shape[0]))

    # ------------------------------------------------------------ batched inference: B images per call
    # Each method gives, per image, what its one-image counterpart gives for that image alone; the B images share the
    # launches: one bbox branch over all proposals, one segmented NMS, one mask chain over all detections, one paste.
    _META_KEYS = ('img_shape', 'ori_shape', 'scale_factor')

    @classmethod
    def _check_batch(cls, img_metas, _name='img_metas', **lists):
        """Argument checks of the batch_* methods (before any GPU work): a non-empty per-image list ``img_metas`` (named
        ``_name`` in the message) and every other per-image list of the same length B."""
        if not isinstance(img_metas, (list, tuple)) or len(img_metas) == 0:
            raise ValueError(f'{_name}: a non-empty list with one entry per image')
        B = len(img_metas)
        for name, v in lists.items():
            if v is not None and len(v) != B:
                raise ValueError(f'{name}: {len(v)} entries for {B} images')
        return B

    @classmethod
    def _check_metas(cls, img_metas, keys):
        for i, m in enumerate(img_metas):
            missing = [k for k in keys if k not in m]
            if missing:
                raise ValueError(f'img_metas[{i}] lacks {missing}')

    @staticmethod
    def _scale_factor_on(scale_factor, device):
        """``torch.from_numpy(scale_factor).to(device)`` of the reference's mask tests (same dtype, same values) through
        a pinned buffer: no host wait per image."""
        if isinstance(scale_factor, float):
            return scale_factor
        return torch.from_numpy(np.ascontiguousarray(scale_factor)).pin_memory().to(device, non_blocking=True)

    def _mask_boxes(self, det_bboxes, scale_factor, rescale):
        """(The boxes the mask chain reads, the scale factor the paste divides them by) of one image's detections, as
        the reference's mask tests derive them (``rescale``: the boxes times ``scale_factor``, on the device)."""
        if not rescale or det_bboxes.shape[0] == 0:
            return det_bboxes, scale_factor
        scale_factor = self._scale_factor_on(scale_factor, det_bboxes.device)
        return det_bboxes[:, :4] * scale_factor, scale_factor

    def batch_simple_test_mask_logits(self, x, det_bboxes_list, det_labels_list, scale_factors=None, rescale=False):
        """``simple_test_mask_logits`` of B images as ONE mask chain: the [sum N, 5] RoI rows of all images (batch column
        = image index into the B-image FPN tuple ``x``) -> the logits [sum N, C, S, S] and the row offsets [B + 1]
        (image b: rows offsets[b]:offsets[b + 1]).  ``rescale``: image b's boxes are multiplied by ``scale_factors[b]``
        first.  B = 1 is ``simple_test_mask_logits`` itself.  With ``enable_inference_graphs`` the call replays a graph
        bucketed on the total RoI count (graphs.BATCH_BUCKETS; larger totals run eagerly)."""
        B = self._check_batch(det_bboxes_list, 'det_bboxes_list', det_labels_list=det_labels_list, scale_factors=scale_factors)
        if rescale and scale_factors is None:
            raise ValueError('rescale=True needs scale_factors')
        offsets = [0]
        for det in det_bboxes_list:
            offsets.append(offsets[-1] + int(det.shape[0]))
        sfs = scale_factors if rescale else [None] * B
        boxes = [self._mask_boxes(det, sf, rescale)[0] for det, sf in zip(det_bboxes_list, sfs)]
        if offsets[-1] == 0:
            return self._empty_mask_logits(det_bboxes_list[0]), offsets
        if B == 1:
            return self.simple_test_mask_logits(x, boxes[0], det_labels_list[0]), offsets
        mask_rois = bbox2roi(boxes).contiguous()
        labels = torch.cat(list(det_labels_list)).contiguous()
        if self._mask_graphs is not None and not torch.is_grad_enabled():
            merged = self._mask_graphs.batched(x, mask_rois, labels, B)
            if merged is not None:
                return merged, offsets
        return self._mask_logits(x, mask_rois, labels), offsets

    @torch.no_grad()
    def batch_simple_test_mask(self, x, img_metas, det_bboxes_list, det_labels_list, rescale=False, encode=False,
                               _labels_host=None):
        """``simple_test_mask`` of B images: per image the per-class lists of (h, w) bool masks (``encode``: COCO RLE
        dicts) of its detections, on its own canvas (``ori_shape``, ``scale_factor``).  One mask chain, one paste launch
        (dm_paste_masks_multi / dm_paste_rle_multi) and one device -> host copy for all images."""
        B = self._check_batch(img_metas, det_bboxes_list=det_bboxes_list, det_labels_list=det_labels_list)
        self._check_metas(img_metas, ('ori_shape', 'scale_factor'))
        num_classes = self._segm_num_classes()
        results = [[[] for _ in range(num_classes)] for _ in range(B)]
        counts = [int(d.shape[0]) for d in det_bboxes_list]
        if sum(counts) == 0:
            return [self._mask_test_result(r, None, 0, 0) for r in results]
        threshold = _mask_threshold(self.test_cfg)
        boxes, sfs = zip(*[self._mask_boxes(det, meta['scale_factor'], rescale)
                           for det, meta in zip(det_bboxes_list, img_metas)])
        labels = torch.cat(list(det_labels_list))
        logits, pending = self._mask_test_pred(x, boxes, det_labels_list, det_bboxes_list)
        preds = select_label_channel(logits, labels)
        canvas_boxes, sizes = [], []
        for b in range(B):
            if counts[b] == 0:
                sizes.append((1, 1))
                continue
            cb, h, w = _paste_geometry(boxes[b], img_metas[b]['ori_shape'], sfs[b], rescale)
            canvas_boxes.append(cb)
            sizes.append((h, w))
        canvas_boxes = torch.cat(canvas_boxes).contiguous()
        if encode:
            segs = ops.paste_rle_multi(preds, canvas_boxes, counts, sizes, threshold, apply_sigmoid=self._mask_test_sigmoid)
            labels_h = _labels_host if _labels_host is not None else labels.cpu().tolist()
        else:
            buf, offs, det_sizes = ops.paste_masks_multi(preds, canvas_boxes, counts, sizes, threshold,
                                                         apply_sigmoid=self._mask_test_sigmoid)
            if _labels_host is None:
                flat, labels_h = _to_host(buf, labels)
                labels_h = labels_h.tolist()
            else:
                (flat,), labels_h = _to_host(buf), _labels_host
            flat = flat.view(np.bool_)
            segs = [flat[o:o + h * w].reshape(h, w) for o, (h, w) in zip(offs, det_sizes)]
        start, out = 0, []
        for b in range(B):
            for j in range(start, start + counts[b]):
                results[b][labels_h[j]].append(segs[j])
            out.append(self._mask_test_result(results[b], pending, start, counts[b]))
            start += counts[b]
        return out

    @torch.no_grad()
    def batch_simple_test_bboxes(self, x, img_metas, proposals, rcnn_test_cfg, rescale=False):
        """``simple_test_bboxes`` of B images -> list of B (dets [k, 5], labels [k]): one bbox branch over the
        proposals of all images, per-image decode (its own ``img_shape`` clip and ``scale_factor``), one segmented NMS
        (postprocess.multiclass_nms_batch)."""
        B = self._check_batch(img_metas, proposals=proposals)
        self._check_metas(img_metas, ('img_shape', 'scale_factor'))
        rows = [int(p.shape[0]) for p in proposals]
        rois = bbox2roi(proposals).contiguous()
        if rois.shape[0] == 0:
            ref = proposals[0]
            return [(ref.new_zeros((0, 5)), ref.new_zeros((0,), dtype=torch.long)) for _ in range(B)]
        rois, cls_score, bbox_pred, head = self._bbox_test_preds(x, rois, img_metas)
        bl, sl, r0 = [], [], 0
        for b in range(B):
            r1 = r0 + rows[b]
            if r1 == r0:
                bl.append(rois.new_zeros((0, 4)))
                sl.append(rois.new_zeros((0, head.num_classes + 1)))
            else:
                bboxes, scores = head.get_bboxes(
                    rois[r0:r1], None if cls_score is None else cls_score[r0:r1],
                    None if bbox_pred is None else bbox_pred[r0:r1], img_metas[b]['img_shape'],
                    img_metas[b]['scale_factor'], rescale=rescale, cfg=None)
                bl.append(bboxes)
                sl.append(scores)
            r0 = r1
        cfg = rcnn_test_cfg
        return multiclass_nms_batch(bl, sl, cfg.score_thr, cfg.nms, cfg.max_per_img)

    @torch.no_grad()
    def batch_simple_test(self, x, proposal_list, img_metas, rescale=False, encode=False):
        """``simple_test`` of B images in one call (the contract of later mmdet releases): ``x`` the FPN tuple with
        batch dimension B, ``proposal_list`` / ``img_metas`` one entry per image -> list of B ``(bbox_results,
        segm_results)``, each what ``simple_test`` returns for that image alone (just ``bbox_results`` without a mask
        branch).  Host waits do not grow with B: the detections of all images cross to the host in one copy."""
        B = self._check_batch(img_metas, proposal_list=proposal_list)
        self._check_metas(img_metas, self._META_KEYS)
        for i, f in enumerate(x):
            if f.shape[0] != B:
                raise ValueError(f'x[{i}] has batch dimension {f.shape[0]} for {B} images')
        dets = self.batch_simple_test_bboxes(x, img_metas, proposal_list, self.test_cfg, rescale=rescale)
        counts = [int(d.shape[0]) for d, _ in dets]
        num_classes = self._bbox_num_classes()
        if sum(counts) == 0:
            bbox_results = [[np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)] for _ in range(B)]
            labels_h = []
        else:
            d_np, l_np = _to_host(torch.cat([d for d, _ in dets]), torch.cat([l for _, l in dets]))
            labels_h = l_np.tolist()
            bbox_results, start = [], 0
            for c in counts:
                bbox_results.append(_bbox2result_host(d_np[start:start + c], l_np[start:start + c], num_classes))
                start += c
        if not self.with_mask:
            return bbox_results
        segm_results = self.batch_simple_test_mask(x, img_metas, [d for d, _ in dets], [l for _, l in dets],
                                                   rescale=rescale, encode=encode, _labels_host=labels_h)
        return list(zip(bbox_results, segm_results))

    # ------------------------------------------------------------ test-time augmentation: V views of one image
    # standard_roi_head.py:264-290 + test_mixins.py:73-107,178-208 (MultiScaleFlipAug): ``x`` holds one FPN tuple per view
    # (batch size 1 each), ``img_metas`` one single-element list per view.  The views share three launches: the mapping of
    # the boxes into every view (dm_bbox_mapping_multi), the box / score merge (dm_merge_aug_bboxes) and the mask merge
    # (dm_merge_aug_masks); the bbox branch and the mask chain run once per view through the one-view path.  No host wait
    # inside the per-view loops.  A view's mask prediction is what ``simple_test_mask_logits`` returns for the mapped
    # boxes (for the DynaMask head this is the project's definition, the reference cannot run it: DESIGN.md section 4.10).
    _AUG_META_KEYS = ('img_shape', 'scale_factor', 'flip', 'flip_direction', 'ori_shape')

    @classmethod
    def _check_aug(cls, x, img_metas):
        """Argument checks of the aug_test* methods (before any GPU work) -> the V view metas."""
        if not isinstance(img_metas, (list, tuple)) or len(img_metas) == 0:
            raise ValueError('img_metas: a non-empty list with one single-element list per view')
        V = len(img_metas)
        if len(x) != V:
            raise ValueError(f'x has {len(x)} views, img_metas {V}')
        views = []
        for v, m in enumerate(img_metas):
            if not isinstance(m, (list, tuple)) or len(m) != 1:
                raise ValueError(f'img_metas[{v}]: one meta per view (test-time augmentation runs one image)')
            missing = [k for k in cls._AUG_META_KEYS if k not in m[0]]
            if missing:
                raise ValueError(f'img_metas[{v}][0] lacks {missing}')
            if x[v][0].shape[0] != 1:
                raise ValueError(f'x[{v}] has batch dimension {x[v][0].shape[0]}: one image per view')
            views.append(m[0])
        ops.aug_view_rows(views)                    # flip directions and scale factors
        return views

    @torch.no_grad()
    def aug_test_bboxes(self, x, img_metas, proposal_list, rcnn_test_cfg):
        """test_mixins.py:73-107: the proposals ``proposal_list[0]`` (original image) mapped into every view, the bbox
        branch and ``get_bboxes(rescale=False)`` per view, the views' boxes mapped back and averaged with their scores
        (merge_aug_bboxes), then ``multiclass_nms`` -> (dets [k, 5], labels [k]) in original-image coordinates."""
        views = self._check_aug(x, img_metas)
        props = proposal_list[0]
        if props.shape[0] == 0:
            return props.new_zeros((0, 5)), props.new_zeros((0,), dtype=torch.long)
        tab = ops.aug_view_table(views, props.device)
        rois = ops.bbox_mapping_multi(props, tab)
        aug_bboxes, aug_scores = [], []
        for v, meta in enumerate(views):
            view_rois, cls_score, bbox_pred, head = self._bbox_test_preds(x[v], rois[v], [meta])
            bboxes, scores = head.get_bboxes(view_rois, cls_score, bbox_pred, meta['img_shape'],
                                             meta['scale_factor'], rescale=False, cfg=None)
            aug_bboxes.append(bboxes.contiguous())
            aug_scores.append(scores.contiguous())
        merged_bboxes, merged_scores = ops.merge_aug_bboxes(aug_bboxes, aug_scores, tab)
        cfg = rcnn_test_cfg
        return multiclass_nms(merged_bboxes, merged_scores, cfg.score_thr, cfg.nms, cfg.max_per_img)

    @torch.no_grad()
    def aug_test_mask_probs(self, x, img_metas, det_bboxes, det_labels):
        """The merged mask probabilities of test-time augmentation [n, 1, S, S] on the device: ``det_bboxes`` (original
        image) mapped into every view, the view's mask prediction, then sigmoid, un-flip and mean over the views
        (merge_aug_masks) of the detection's class channel."""
        views = self._check_aug(x, img_metas)
        if det_bboxes.shape[0] == 0:
            return self._empty_mask_logits(det_bboxes, channels=1)
        tab = ops.aug_view_table(views, det_bboxes.device)
        rois = ops.bbox_mapping_multi(det_bboxes, tab)
        labels = det_labels.contiguous()
        logits = []
        for v in range(len(views)):
            view_logits = self.simple_test_mask_logits(x[v], rois[v][:, 1:], labels)
            if self._mask_graphs is not None:
                view_logits = view_logits.clone()       # a graph's static output: the next view's replay overwrites it
            logits.append(view_logits.contiguous())
        return ops.merge_aug_masks(logits, labels, tab)

    @torch.no_grad()
    def aug_test_mask(self, x, img_metas, det_bboxes, det_labels, encode=False, _labels_host=None):
        """test_mixins.py:178-208 -> per-class lists of (h, w) bool masks at ``ori_shape`` of the first view
        (``encode``: COCO RLE dicts): the merged probabilities (``aug_test_mask_probs``) pasted without a sigmoid,
        ``scale_factor=1.0, rescale=False``, thresholded at ``mask_thr_binary``."""
        views = self._check_aug(x, img_metas)
        num_classes = self._segm_num_classes()
        if det_bboxes.shape[0] == 0:
            return [[] for _ in range(num_classes)]
        _mask_threshold(self.test_cfg)              # (raises before any device work)
        probs = self.aug_test_mask_probs(x, img_metas, det_bboxes, det_labels)
        return paste_segms(probs, det_bboxes, det_labels, self.test_cfg, views[0]['ori_shape'], 1.0, False, encode=encode,
                           apply_sigmoid=False, num_classes=num_classes, labels_host=_labels_host)

    @torch.no_grad()
    def aug_test(self, x, proposal_list, img_metas, rescale=False, encode=False):
        """standard_roi_head.py:264-290: boxes merged over the views, then masks merged over the views ->
        ``(bbox_results, segm_results)`` (just ``bbox_results`` without a mask branch).  ``rescale=False`` scales only
        the boxes of ``bbox_results`` by the first view's ``scale_factor``, as the reference does; the masks stay at
        the original image's size either way."""
        views = self._check_aug(x, img_metas)
        det_bboxes, det_labels = self.aug_test_bboxes(x, img_metas, proposal_list, self.test_cfg)
        num_classes = self._bbox_num_classes()
        if det_bboxes.shape[0] == 0:
            bbox_results = [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
            labels_h = []
        else:
            _det_bboxes = det_bboxes
            if not rescale:
                _det_bboxes = det_bboxes.clone()
                sf = views[0]['scale_factor']
                _det_bboxes[:, :4] *= sf if isinstance(sf, float) else self._scale_factor_on(
                    np.asarray(sf, dtype=np.float32), det_bboxes.device)
            d_np, l_np = _to_host(_det_bboxes, det_labels)
            bbox_results = _bbox2result_host(d_np, l_np, num_classes)
            labels_h = l_np.tolist()
        if not self.with_mask:
            return bbox_results
        segm_results = self.aug_test_mask(x, img_metas, det_bboxes, det_labels, encode=encode, _labels_host=labels_h)
        return bbox_results, segm_results


@HEADS.register_module()
class DynaMaskRoIHead(StandardRoIHead):
    """dynamask_roi_head.py:10-158: the selector (MaskPre + straight-through Gumbel), its own training step (the bbox
    branch and the selector on side streams) and, for inference, the merged 112 x 112 logits of the three stages as the
    head's ``_mask_logits`` -- split over RoI chunks on HIP streams, optionally replayed as HIP graphs -- plus the per-RoI
    early exit (``dynamic_mask_logits`` / ``dynamic_test_mask``)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        # inference: RoI chunks on separate HIP streams (see _mask_forward)
        self.num_streams = 2
        # RoI chunks on two streams from this many RoIs on (profiles/r06_infer_notes.txt (12), 1 / 2 / 3 streams).  Replayed
        # as a HIP graph: 24 detections 0.734 / 0.764 / 0.767, 32: 0.885 / 0.871 / 0.907, 48: 1.175 / 1.157 / 1.140, 64: 1.459 /
        # 1.365 / 1.411, 80: 1.646 / 1.604 / 1.647, 100: 2.024 / 1.881 / 1.916 ms.  Eager, the host issues the two chains' launches
        # one after the other and a call cannot take less than that (~1.6-1.7 ms): 1 / 2 streams at 32 detections 0.88 / 1.69,
        # 48: 1.17 / 1.71, 64: 1.45 / 1.61, 80: 1.63 / 1.61, 100: 2.01 / 1.89 ms.
        self.stream_split_min = 80           # eager launches
        self.stream_split_min_graph = 32     # under HIP-graph capture (graphs.py)

    merge_stage_preds = staticmethod(merge_stage_preds)

    # ------------------------------------------------------------------ forward
    def _mask_forward(self, x, rois, roi_labels, last_stage=None, _between=None):
        """dynamask_roi_head.py:75-81.  (``_between``: see train_path.mask_head_forward_train.)"""
        if torch.is_grad_enabled() and last_stage is None:
            # training: same kernels, forward keeps what the hand-sequenced backward needs
            ins_feats = train_path.roi_extract_train(self.mask_roi_extractor, x, rois)
            ips, dps = train_path.mask_head_forward_train(self.mask_head, ins_feats, x, rois, roi_labels, between=_between)
            return dict(stage_instance_preds=ips, stage_detail_preds=dps)
        with ops.splitk_scope():           # inference: launches of few workgroups may split their K loop
            return self._mask_forward_infer(x, rois, roi_labels, last_stage)

    def _mask_forward_infer(self, x, rois, roi_labels, last_stage=None, merge=False):
        """Inference.  The FPN-wide semantic maps (``relu(semantic_transform_in(P_l))``, which no RoI enters) are one
        grouped launch in front of everything else (on a stream of their own beside the chains they measured neutral at
        100 detections and +2 % at 16 and on the 512-RoI headline -- a fork inside a HIP graph costs more than the ~100 us
        it hides; profiles/r06_infer_notes.txt; removed); the RoIs are independent, so from ``stream_split_min`` RoIs on they
        are split into chunks on separate HIP streams (the tail of every kernel -- its last, partially filled round of
        workgroups over the 256 CUs -- overlaps the other chunk's work) whose launches are issued in turn
        (``DynaMaskHead.steps``), every chunk writing its rows of the result tensors in place.

        ``merge`` (``simple_test_mask_logits``): hand back the merged 112 x 112 logits of dynamask_roi_head.py:138-149
        instead of the per-stage dict -- the last stage's logits then stay at 56 x 56 and ONE launch per chunk does the
        final align_corners x2 upsample and both boundary merges (ops.boundary_merge_chain; same bits as the four launches
        it replaces), on the chunk's own stream, in front of the join instead of behind it."""
        n = rois.shape[0]
        head, ext = self.mask_head, self.mask_roi_extractor
        dev = rois.device
        cur = torch.cuda.current_stream(dev)
        capturing = torch.cuda.is_current_stream_capturing()
        n_streams = self.num_streams if n >= (self.stream_split_min_graph if capturing else self.stream_split_min) else 1
        head.prepack()                 # packs are cached by whoever asks first: before the fork, on this stream
        sems = head.semantic_maps(x, last_stage)
        if merge:
            assert last_stage is None and self._merged_tail_supported()
            s_out = head.stage_sup_size[-1]
            merged = torch.empty((n, 1, s_out, s_out), device=dev, dtype=torch.float32)
            ips = dps = None
        else:
            # allocated here, on the caller's stream, before the fork: no concatenation after the join
            sizes = head.pred_sizes(last_stage)
            ips = [torch.empty((n, 1, s_, s_), device=dev, dtype=torch.float32) for s_ in sizes]
            dps = [torch.empty((n, 1, s_, s_), device=dev, dtype=torch.float32) for s_ in sizes]

        def chain(lo, hi):
            r, l = rois[lo:hi], roi_labels[lo:hi]
            out = None if merge else [(a[lo:hi], b[lo:hi]) for a, b in zip(ips, dps)]
            got, _ = yield from head.steps(None, x, r, l, last_stage=last_stage, sems=sems, pred_out=out, defer_final_up=merge,
                                           extract=lambda: ext(x[:ext.num_inputs], r))
            if merge:
                ops.boundary_merge_chain(got[1], got[2], got[3], out=merged[lo:hi])
                yield
        if n_streams <= 1:
            run_steps(chain(0, n))
        else:
            split = getattr(self, 'stream_split', None)      # optional cumulative fractions, e.g. (0.4, 1.0)
            if split is not None and len(split) == n_streams:
                bounds = [0] + [round(f * n) for f in split]
            else:
                bounds = [round(i * n / n_streams) for i in range(n_streams + 1)]
            streams = self._side_streams(n_streams, dev)
            chains = []
            for st, lo, hi in zip(streams, bounds[:-1], bounds[1:]):
                if hi > lo:
                    st.wait_stream(cur)
                    chains.append((st, chain(lo, hi)))
            hook = getattr(self, '_launch_hook', None)      # tools/chain_probe.py: an event behind every launch of every chain
            while chains:                   # one launch of every chain in turn
                for st, gen in list(chains):
                    with torch.cuda.stream(st), ops.overlapped_streams():
                        try:
                            next(gen)
                            if hook is not None:
                                hook(st)
                        except StopIteration:
                            chains.remove((st, gen))
            for st in streams:
                cur.wait_stream(st)
        return merged if merge else dict(stage_instance_preds=ips, stage_detail_preds=dps)

    def _side_streams(self, k, device):
        """k streams for k RoI chunks, from the package's shared pool (streams.py: hardware queues are few)."""
        return [streams.side(device, i) for i in range(k)]      # more chunks than pool streams: they share (still ordered)

    def sample_uniform(self, shape, device):
        """The reference draws on the CPU generator and copies (dynamask_roi_head.py:90-91, Q9).  Same draw here; the copy
        goes through a pinned staging buffer and does not block the host (a pageable-memory copy waits for the stream).
        The buffer is reused: the event of its previous copy is waited for before the next draw overwrites it."""
        device = torch.device(device)
        if device.type != 'cuda':
            return torch.rand(shape).to(device)
        n = 1
        for d in shape:
            n *= int(d)
        st = getattr(self, '_noise_stage', None)
        if st is None or st[0].numel() < n:
            st = self._noise_stage = [torch.empty(max(n, 1024), dtype=torch.float32).pin_memory(), None]
        if st[1] is not None:
            st[1].synchronize()
        host = st[0][:n].view(shape)
        torch.rand(shape, out=host)
        dev_t = host.to(device, non_blocking=True)
        st[1] = torch.cuda.current_stream(device).record_event()
        return dev_t

    def get_mask_label(self, ins_semantic_feats, noise=None, return_index=False):
        """dynamask_roi_head.py:84-87,97-114: logits -> ST-Gumbel-softmax (hard)."""
        train = torch.is_grad_enabled() and self.mask_predictor.training
        if train:
            logits = train_path.MaskPreFn.apply(self.mask_predictor, ins_semantic_feats.detach(),
                                                *list(self.mask_predictor.parameters()))
        else:
            logits = self.mask_predictor(ins_semantic_feats)
        if noise is None:
            noise = self.sample_uniform(logits.shape, logits.device)
        if train:
            hot, idx = train_path.GumbelSelectFn.apply(logits, noise, 0.5)
            y = None
        else:
            y, hot, idx = ops.gumbel_select(logits, noise.contiguous(), 0.5)
        return (hot, idx, logits, y) if return_index else hot

    def get_mask_label_from_map(self, feat_map, rois, noise=None):
        """``get_mask_label(semantic_roi_extractor([feat_map], rois), noise, return_index=True)`` of the training step
        (dynamask_roi_head.py:59-60) without the [N, 256, 56, 56] tensor: MaskPre's 1x1 conv1 runs on the map and 128
        channels are extracted (train_path.MaskPreMapFn).  The deterministic mode and DM_MASKPRE_MAP=0 take the
        reference's order of operations."""
        lay = self.semantic_roi_extractor.roi_layers[0]
        if ops.DETERMINISTIC[0] or not _MASKPRE_ON_MAP or self.semantic_roi_extractor.num_inputs != 1:
            return self.get_mask_label(self.semantic_roi_extractor([feat_map], rois), noise, return_index=True)
        logits = train_path.MaskPreMapFn.apply(self.mask_predictor, feat_map, rois, lay.output_size[0], lay.spatial_scale,
                                               lay.sampling_ratio, *list(self.mask_predictor.parameters()))
        if noise is None:
            noise = self.sample_uniform(logits.shape, logits.device)
        hot, idx = train_path.GumbelSelectFn.apply(logits, noise, 0.5)
        return hot, idx, logits, None

    # ------------------------------------------------------------------ training entry points
    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None,
                      noise=None):
        """dynamask_roi_head.py:21-46 (called from detectors/two_stage.py:161-164): assign gts and
        sample proposals per image, bbox branch forward + loss, mask branch forward + loss.
        Returns the dict of losses the detector's ``_parse_losses`` sums.  ``noise`` (extension):
        the uniform draw of the Gumbel selector, for reproducible tests."""
        sampling_results = self._assign_and_sample(x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore)
        # the bbox branch and the mask branch meet only in the sum of the losses: the bbox branch is issued on its own
        # stream (its backward follows it there) and joined before the losses are handed back
        losses = {}
        if not self.with_bbox:
            # dynamask_roi_head.py:40-45 guards both branches (with_bbox / with_mask)
            if self.with_mask:
                losses.update(self._mask_forward_train(x, sampling_results, None, gt_bboxes, gt_masks, gt_labels, img_metas,
                                                       noise=noise)['loss_mask'])
            return losses
        side = None
        if torch.is_grad_enabled() and x[0].is_cuda:
            side = train_path.side_stream(x[0].device, 'bbox')
        if side is not None:
            main = torch.cuda.current_stream(x[0].device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                bbox_results = self._bbox_forward_train(x, sampling_results, gt_bboxes, gt_labels, img_metas)
        else:
            bbox_results = self._bbox_forward_train(x, sampling_results, gt_bboxes, gt_labels, img_metas)
        mask_results = None
        if self.with_mask:
            mask_results = self._mask_forward_train(x, sampling_results, bbox_results['bbox_feats'], gt_bboxes, gt_masks,
                                                    gt_labels, img_metas, noise=noise)
        if side is not None:
            main.wait_stream(side)
            for v in bbox_results['loss_bbox'].values():
                if isinstance(v, torch.Tensor):
                    v.record_stream(main)
        losses.update(bbox_results['loss_bbox'])
        if mask_results is not None:
            losses.update(mask_results['loss_mask'])
        return losses

    def _mask_forward_train(self, x, sampling_results, bbox_feats=None, gt_bboxes=None, gt_masks=None, gt_labels=None,
                            img_metas=None, noise=None):
        """dynamask_roi_head.py:48-73, reference signature
        ``(x, sampling_results, bbox_feats, gt_bboxes, gt_masks, gt_labels, img_metas)``:
        positives of the sampler -> mask targets on the device -> the mask path.

        The tensor-level form of round 1, ``(x, pos_rois, pos_labels, stage_mask_targets)``, is
        still accepted (a tensor in the second position) and is what this method calls after
        the sampling results have been unpacked."""
        if isinstance(sampling_results, torch.Tensor):
            return self._mask_forward_train_tensors(x, sampling_results, bbox_feats, gt_bboxes, noise=noise)
        pos_bboxes = [res.pos_bboxes for res in sampling_results]
        pos_labels = [res.pos_gt_labels for res in sampling_results]
        pos_assigned_gt_inds = [res.pos_assigned_gt_inds for res in sampling_results]
        pos_rois = bbox2roi(pos_bboxes).contiguous()
        if pos_rois.shape[0] == 0:
            # no positive RoI on this rank (no GT in the batch).  The reference has no guard here (Quirk Q11: it
            # fails inside the head); the stock head returns no mask loss (standard_roi_head.py:167-170).  A zero
            # that keeps the graph connected serves a training loop better than either.
            return dict(loss_mask={'loss_masks': x[0].sum() * 0})
        stage_mask_targets = self.mask_head.get_targets(pos_bboxes, pos_assigned_gt_inds, gt_masks)
        return self._mask_forward_train_tensors(x, pos_rois, torch.cat(pos_labels), stage_mask_targets, noise=noise)

    def _selector(self, x, pos_rois, noise):
        """dynamask_roi_head.py:59-60: the 56 x 56 extraction of P2 (detached) -> MaskPre -> ST-Gumbel selection."""
        if torch.is_grad_enabled() and self.mask_predictor.training:
            return self.get_mask_label_from_map(x[0].detach(), pos_rois, noise)
        ins_semantic_feats = self.semantic_roi_extractor([x[0].detach(), ], pos_rois)
        return self.get_mask_label(ins_semantic_feats, noise, return_index=True)

    def _mask_forward_train_tensors(self, x, pos_rois, pos_labels, stage_mask_targets, noise=None):
        """dynamask_roi_head.py:57-73 from ``pos_rois`` on."""
        # The resolution selector (56x56 extraction of P2 -> MaskPre -> ST-Gumbel) shares nothing with the mask head
        # until the loss: it is issued on a second stream and runs beside the head (autograd replays each node on
        # the stream of its forward, so the two backward passes overlap the same way and are joined by the engine).
        side = train_path.side_stream(pos_rois.device, 'selector') if torch.is_grad_enabled() else None
        if side is not None:
            # the head is issued FIRST (the host feeds the chain of the step before anything that has slack, see
            # train_path.MaskHeadFn.forward); the selector waits for the inputs' event, not for the head
            main = torch.cuda.current_stream(pos_rois.device)
            ops.PACK_PLAN.refresh(pos_rois.device)          # every kernel-layout weight of the step in one launch, before the event
            ready = main.record_event()
            train_path._INPUTS_READY[0] = ready
            sel = {}

            def selector():
                side.wait_event(ready)
                with torch.cuda.stream(side):
                    sel['out'] = self._selector(x, pos_rois, noise)
            try:
                mask_results = self._mask_forward(x, pos_rois, pos_labels, _between=selector)
            finally:
                train_path._INPUTS_READY[0] = None
            mask_labels, idx, logits, y = sel['out']
            main.wait_stream(side)
            for t in (mask_labels, idx, logits):
                t.record_stream(main)
        else:
            mask_results = self._mask_forward(x, pos_rois, pos_labels)
            mask_labels, idx, logits, y = self._selector(x, pos_rois, noise)
        loss_mask = self.mask_head.loss_func(mask_results['stage_instance_preds'], mask_results['stage_detail_preds'],
                                             stage_mask_targets, mask_labels)
        mask_results.update(loss_mask=loss_mask, mask_labels=mask_labels, mask_index=idx, mask_logits=logits)
        if self.train_cfg is not None and getattr(self.train_cfg, 'get', None) and self.train_cfg.get('flops') is not None:
            # dynamask_roi_head.py:68-71: computed and attached, never added to the losses (Quirk Q3)
            key = (mask_labels.device, tuple(float(v) for v in self.train_cfg.flops))
            fl = getattr(self, '_flops_dev', (None, None))
            if fl[0] != key:      # (uploaded once: ``new_tensor`` of a Python list is a blocking host -> device copy per step)
                fl = self._flops_dev = (key, mask_labels.new_tensor(self.train_cfg.flops))
            fl = fl[1]
            budget = (mask_labels.detach() * fl).sum() / len(mask_labels) - 1.0
            mask_results['loss_flops'] = {'loss_flops': self.train_cfg.Lambda * torch.clamp(
                budget / (self.train_cfg.flops[-1] - self.train_cfg.flops[0]), min=0)}
        return mask_results

    # ------------------------------------------------------------------ mask test hooks
    def _mask_logits(self, x, mask_rois, det_labels):
        """The merged 112 x 112 logits [n, 1, 112, 112] (dynamask_roi_head.py:138-149): the launch sequence of
        ``simple_test_mask_logits`` (what graphs.GraphedMaskLogits captures)."""
        # the reference chunks by 100 RoIs "to avoid memory overflow" (:132); 288 GB of HBM do not need it
        if FUSED_MERGE_TAIL[0] and not torch.is_grad_enabled() and self._merged_tail_supported():
            with ops.splitk_scope():
                return self._mask_forward_infer(x, mask_rois, det_labels, merge=True)
        res = self._mask_forward(x, mask_rois, det_labels)
        return merge_stage_preds(res['stage_instance_preds'])

    def _mask_logits_size(self):
        return 1, 112

    def _segm_num_classes(self):
        return self.mask_head.stage_num_classes[0]

    def _merged_tail_supported(self):
        h = self.mask_head
        return (len(h.stages) == 3 and not h.pre_upsample_last_stage
                and list(h.stage_sup_size) == [h.stage_sup_size[0] * k for k in (1, 2, 4, 8)])

    def enable_inference_graphs(self, on=True, buckets=None, batch_buckets=None):
        """Replay ``simple_test_mask_logits`` as a HIP graph per bucket of detection counts (16 / 24 / 32 / 48 / 64 / 80 / 100 by
        default; see graphs.py for what a graph is tied to).  Off by default: the eager path is the reference one.
        ``batch_buckets``: the buckets of the total RoI count of ``batch_simple_test_mask_logits`` (graphs.BATCH_BUCKETS)."""
        self._mask_graphs = GraphedMaskLogits(self, buckets or BUCKETS,
                                              batch_buckets=batch_buckets or BATCH_BUCKETS) if on else None
        return self._mask_graphs

    # ------------------------------------------------------------ dynamic inference
    @torch.no_grad()
    def dynamic_mask_logits(self, x, det_bboxes, det_labels, noise=None, merge=True, exits=None):
        """Per-RoI early exit at the resolution the selector predicts (SURVEY 8f rank 3 --
        the method's point; the reference ships it only as commented-out code that still runs
        every exit for every RoI, dynamask_roi_head.py:160-204).

        MaskPre + ST-Gumbel pick an exit e_j in {0..3} (14/28/56/112) per detection; the
        detections are ordered deepest exit first so the RoIs alive at stage k are a prefix
        (no gathers), and stage k runs only on those.  ``noise`` = the uniform U of the Gumbel
        sampler; None = no sampling (argmax of the predictor logits).  ``exits`` overrides the
        selector (tests, fixed budgets).  With ``merge`` the boundary-aware merge of the live
        test path (:138-149) is applied up to each RoI's exit.

        Returns dict(exits [N] int64 in detection order, order [N] (sorted position ->
        detection), n_ge (list), preds: list over k of logits [n_ge[k], 1, S_k, S_k] in
        sorted order -- RoI at sorted position p with exit e reads preds[e][p])."""
        n = det_bboxes.shape[0]
        dev = det_bboxes.device
        rois = bbox2roi([det_bboxes[:, :4]]).contiguous()
        if exits is None:
            if noise is None:
                noise = torch.full((n, 4), 0.5, device=dev)       # constant Gumbel shift: argmax(logits)
            if self.mask_predictor.training:
                sem = self.semantic_roi_extractor([x[0], ], rois)
                _, idx, _, _ = self.get_mask_label(sem, noise, return_index=True)
            else:
                # conv1 commutes with RoIAlign: half the extraction, no per-RoI 256->128 conv
                logits = self.mask_predictor.forward_from_map(x[0], rois, self.semantic_roi_extractor)
                _, _, idx = ops.gumbel_select(logits, noise.contiguous(), 0.5)
            exits = idx.long()
        else:
            exits = torch.as_tensor(exits, device=dev).long()
        order = torch.argsort(exits, descending=True, stable=True)
        counts = torch.bincount(exits, minlength=4).tolist()        # host sync: the launches are sized by it
        n_ge = [sum(counts[k:]) for k in range(4)]
        rois_s, labels_s = rois[order].contiguous(), det_labels[order].contiguous()
        with torch.no_grad():
            ins = self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], rois_s)
            preds = self.mask_head.forward_dynamic(ins, x, rois_s, labels_s, n_ge)
            if merge:
                # merged_k = merge(merged_{k-1}[alive at k], pred_k), in place on pred_k (k >= 2)
                for k in range(2, len(preds)):
                    if n_ge[k] > 0:
                        ops.boundary_merge_(preds[k - 1][:n_ge[k]], preds[k])
        return dict(exits=exits, order=order, n_ge=n_ge, preds=preds)

    def dynamic_test_mask(self, x, img_metas, det_bboxes, det_labels, rescale=False, noise=None, merge=True, exits=None):
        """``simple_test_mask`` with per-RoI early exit: same inputs, same per-class lists of
        (h, w) bool masks; each detection is pasted from the logits of its own exit."""
        segm_result = [[] for _ in range(self._segm_num_classes())]
        n = det_bboxes.shape[0]
        if n == 0:
            return segm_result
        _bboxes, scale_factor = self._mask_boxes(det_bboxes[:, :4], img_metas[0]['scale_factor'], rescale)
        res = self.dynamic_mask_logits(x, _bboxes, det_labels, noise=noise, merge=merge, exits=exits)
        order, n_ge, preds = res['order'], res['n_ge'] + [0], res['preds']
        boxes_s, img_h, img_w = _paste_geometry(_bboxes[order], img_metas[0]['ori_shape'], scale_factor, rescale)
        canvas = torch.empty((n, img_h, img_w), device=_bboxes.device, dtype=torch.uint8)
        thr = self.test_cfg.mask_thr_binary
        for e in range(4):
            lo, hi = n_ge[e + 1], n_ge[e]
            if hi > lo:
                ops.paste_masks(preds[e][lo:hi], boxes_s[lo:hi], img_h, img_w, thr, apply_sigmoid=True, out=canvas[lo:hi])
        im, order_h = _to_host(canvas.view(torch.bool), order)
        by_det = [None] * n
        for p, j in enumerate(order_h.tolist()):
            by_det[j] = im[p]
        for c, segm in zip(det_labels.tolist(), by_det):
            segm_result[c].append(segm)
        return segm_result


@HEADS.register_module()
class RefineRoIHead(StandardRoIHead):
    """``RefineRoIHead`` -- mmdet/models/roi_heads/refine_roi_head.py:10-113, inference: the RoI head of
    configs/refinemask, whose mask head is ``RefineMaskHead``.  The bbox branch, ``simple_test``, ``batch_simple_test``,
    ``aug_test`` and the mask-test template are the base's; the head supplies ``_mask_forward`` (refine_roi_head.py:75-80)
    and, as ``_mask_logits``, the merged logits of the last stage (the boundary-aware merge from stage 1, :102-113, the
    same merge as DynaMask's: ``merge_stage_preds``).  The four semantic 3x3 convolutions run once per call on the whole
    stride-4 map of every image of the batch (the reference runs them once per chunk of 100 RoIs).  The fork's
    ``BaseRoIHead`` builds ``mask_predictor`` / ``semantic_roi_extractor`` for EVERY RoI head (Quirk Q4): the base's
    constructor does the same, so the ``state_dict`` keys are the reference's.  Training and HIP-graph capture are the
    follow-up (NotImplementedError)."""

    merge_stage_preds = staticmethod(merge_stage_preds)

    def _mask_forward(self, x, rois, roi_labels, **kw):
        """refine_roi_head.py:75-80 -> dict(stage_instance_preds, semantic_pred)."""
        ext = self.mask_roi_extractor
        rois = rois.contiguous()
        with torch.no_grad():
            ins_feats = ext(x[:ext.num_inputs], rois)
            ips, sem_pred = self.mask_head(ins_feats, x[0].contiguous(), rois, roi_labels)
        return dict(stage_instance_preds=ips, semantic_pred=sem_pred)

    def _mask_logits(self, x, mask_rois, det_labels):
        """The merged logits of the last stage [n, 1, S, S]: stage k's (k >= 1) merged into stage k + 1's where the
        coarser one is not on a boundary (refine_roi_head.py:102-113), in place."""
        res = self._mask_forward(x, mask_rois, det_labels)
        return merge_stage_preds(res['stage_instance_preds'])

    def _mask_logits_size(self):
        return 1, self.mask_head.stage_sup_size[-1]

    def _segm_num_classes(self):
        return self.mask_head.stage_num_classes[0]

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('RefineRoIHead.forward_train: RefineMask training (targets, RefineCrossEntropyLoss, the '
                                  'dilated-convolution gradients) is the follow-up to its inference')


@HEADS.register_module()
class PointRendRoIHead(StandardRoIHead):
    """``PointRendRoIHead`` -- mmdet/models/roi_heads/point_rend_roi_head.py, inference: the RoI head of configs/point_rend.
    The bbox branch, ``_mask_forward`` (the ``CoarseMaskHead`` logits [n, classes, 7, 7] of the GenericRoIExtractor's
    14 x 14 features) and the mask-test template are the base's; the head's ``_mask_logits`` refines the coarse
    prediction by the subdivision loop of ``_mask_point_forward_test`` (:96-128): ``subdivision_steps`` bilinear x2
    upsamples, and at every step that is not skipped the ``subdivision_num_points`` most uncertain cells re-predicted by
    ``point_head`` (ops.point_select -> ops.point_gather -> MaskPointHead.refine_).

    Only the label channel of the refined map is carried: every operation of the loop is per class channel except the
    point selection, which reads the label channel, and only the label channel is pasted or merged.  The result is that
    channel of the reference's [n, classes, 224, 224] map (the coarse point features still hold every class: they are
    inputs of the point MLP).  ``BaseRoIHead`` builds ``mask_predictor`` / ``semantic_roi_extractor`` for every RoI head
    (Quirk Q4): the ``state_dict`` keys are the reference's.  Training (Quirk Q5) and HIP-graph capture raise."""

    def __init__(self, point_head, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not (self.with_bbox and self.with_mask):
            raise ValueError('PointRendRoIHead needs a bbox and a mask branch (point_rend_roi_head.py:19)')
        if self.mask_roi_extractor.num_inputs != 1:
            raise NotImplementedError('PointRendRoIHead: one fine-grained feature level (configs/point_rend: P2)')
        self.point_head = build_head(point_head)

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained)
        self.point_head.init_weights()

    def _refine_size(self):
        s = self.mask_head.output_size[0]
        return s * 2 ** self.test_cfg.subdivision_steps

    def _mask_logits_size(self):
        return 1, self._refine_size()

    def _mask_point_forward_test(self, x, rois, label_pred, mask_pred):
        """point_rend_roi_head.py:96-128 on the label channel -> refined logits [n, 1, S', S']."""
        cfg = self.test_cfg
        if cfg.scale_factor != 2:
            raise NotImplementedError('PointRendRoIHead: subdivision scale_factor 2 only (configs/point_rend)')
        steps, num_points = int(cfg.subdivision_steps), int(cfg.subdivision_num_points)
        n = rois.shape[0]
        rois = rois.contiguous()
        labels = label_pred.to(torch.int64).contiguous()
        mask_pred = mask_pred.contiguous()
        sel = mask_pred if mask_pred.shape[1] == 1 else mask_pred[torch.arange(n, device=rois.device), labels][:, None]
        refined = sel.contiguous()
        feat = x[0].contiguous()
        scale = 1.0 / float(self.mask_roi_extractor.featmap_strides[0])
        for step in range(steps):
            refined = ops.upsample2x(refined)
            H, W = refined.shape[2:]
            if num_points >= 4 * H * W and step < steps - 1:
                continue
            idx = ops.point_select(refined, min(H * W, num_points))
            pts = ops.point_gather(feat, rois, mask_pred, idx, H, W, scale)
            self.point_head.refine_(pts, labels, idx, refined)
        return refined

    def _mask_logits(self, x, mask_rois, det_labels):
        """The refined label-channel logits [n, 1, S', S'] of the RoIs (S' = 224 in configs/point_rend)."""
        with torch.no_grad():
            coarse = self._mask_forward(x, mask_rois)['mask_pred']
            return self._mask_point_forward_test(x, mask_rois, det_labels, coarse)

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('PointRendRoIHead.forward_train: PointRend training is broken in the reference '
                                  '(CoarseMaskHead.loss and the point loss use mask_cross_entropy, Quirk Q5)')


@HEADS.register_module()
class PointRefineRoIHead(StandardRoIHead):
    """``PointRefineRoIHead`` -- mmdet/models/roi_heads/point_refine_head.py, inference: the RoI head of
    configs/point_refine, whose mask head is ``PointRefineMaskHead``.  The bbox branch, ``simple_test``,
    ``batch_simple_test``, ``aug_test`` and the mask-test template are the base's; the head supplies ``_mask_forward``
    (point_refine_head.py:86-92) and, as ``_mask_logits``, the merged logits of the last stage (the boundary-aware merge
    from stage 1, :114-127: ``merge_stage_preds``).  The semantic 3x3 convolutions and the stages' semantic 1x1s run once
    per call on the whole stride-4 map of every image; each RoI's fine point features come from its own image
    (``rois[:, 0]``), which is the reference's per-image concatenation whenever the RoIs are grouped by image, as
    ``bbox2roi`` groups them.  ``aug_test`` is the project's definition: the reference's ``aug_test_mask`` calls
    ``_mask_forward(x, rois)`` without the labels and fails.  ``BaseRoIHead`` builds ``mask_predictor`` /
    ``semantic_roi_extractor`` for every RoI head (Quirk Q4): the ``state_dict`` keys are the reference's.  Training
    (the config's loss exists nowhere in the reference, Quirk Q15) and HIP-graph capture raise."""

    merge_stage_preds = staticmethod(merge_stage_preds)

    def _mask_forward(self, x, rois, roi_labels, cfg=None, semantic_pred=True, form=None):
        """point_refine_head.py:86-92 -> dict(stage_instance_preds, stage_detail_preds, semantic_pred)."""
        ext = self.mask_roi_extractor
        rois = rois.contiguous()
        with torch.no_grad():
            ins_feats = ext(x[:ext.num_inputs], rois)
            ips, dps, sem_pred = self.mask_head(ins_feats, x[0].contiguous(), rois, roi_labels,
                                                self.test_cfg if cfg is None else cfg, semantic_pred=semantic_pred,
                                                form=form)
        return dict(stage_instance_preds=ips, stage_detail_preds=dps, semantic_pred=sem_pred)

    def _mask_logits(self, x, mask_rois, det_labels):
        """The merged logits of the last stage [n, 1, S, S]: stage k's (k >= 1) merged into stage k + 1's where the
        coarser one is not on a boundary (point_refine_head.py:114-127), in place."""
        res = self._mask_forward(x, mask_rois, det_labels, semantic_pred=False)
        return merge_stage_preds(res['stage_instance_preds'])

    def _mask_logits_size(self):
        return 1, self.mask_head.stage_sup_size[-1]

    def _segm_num_classes(self):
        return self.mask_head.stage_num_classes[0]

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('PointRefineRoIHead.forward_train: the config\'s PointRefineCrossEntropyLoss is '
                                  'registered nowhere in the reference, which cannot build or train this head (Quirk Q15)')


@HEADS.register_module()
class MaskScoringRoIHead(StandardRoIHead):
    """``MaskScoringRoIHead`` -- mmdet/models/roi_heads/mask_scoring_roi_head.py, inference: the RoI head of configs/ms_rcnn,
    a ``StandardRoIHead`` over ``FCNMaskHead`` plus ``mask_iou_head`` (``MaskIoUHead``).  ``simple_test_mask`` returns
    ``(segm_result, mask_scores)`` (:58-90; ``encode=True``: ``(rles, mask_scores)``, what ``encode_mask_results`` gives
    for a tuple), ``batch_simple_test_mask`` that pair per image; the empty form is ``([[]] * C, [[]] * C)``.  The mask
    branch runs once per call: RoIAlign and FCNMaskHead give ``mask_feats`` and ``mask_pred`` once, the IoU head reads
    both, and the scores (ops.mask_iou_scores) cross to the host behind the same host wait as the masks.  ``aug_test`` is
    the base's (masks without scores: the reference does not override it).  Training raises (Quirk Q5: the mask loss it
    would run first is broken in the fork), and so does HIP-graph capture."""

    def __init__(self, mask_iou_head=None, **kwargs):
        if mask_iou_head is None:
            raise ValueError('MaskScoringRoIHead needs a mask_iou_head (mask_scoring_roi_head.py:16)')
        super().__init__(**kwargs)
        if not self.with_mask:
            raise ValueError('MaskScoringRoIHead needs a mask branch')
        if type(self.mask_head).__name__ != 'FCNMaskHead':
            raise NotImplementedError('MaskScoringRoIHead: an FCNMaskHead mask branch (configs/ms_rcnn)')
        self.mask_iou_head = build_head(mask_iou_head)

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained)
        self.mask_iou_head.init_weights()

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('MaskScoringRoIHead.forward_train: the mask loss it runs before the IoU loss '
                                  '(FCNMaskHead.loss) is broken in the reference fork (Quirk Q5)')

    def _mask_test_pred(self, x, boxes, labels, det_bboxes):
        """One mask branch for the detections of all images: ``mask_pred`` to paste, and the mask scores of
        ``mask_iou_head`` on the same ``mask_feats`` / ``mask_pred``, copied to pinned host memory without a wait."""
        rois = bbox2roi(list(boxes)).contiguous()
        labels = torch.cat([lab.to(torch.int64) for lab in labels]).contiguous()
        dets = torch.cat(list(det_bboxes)).contiguous()
        with torch.no_grad():
            res = self._mask_forward(x, rois)
            mask_iou_pred = self.mask_iou_head(res['mask_feats'], res['mask_pred'], labels)
            scores = ops.mask_iou_scores(mask_iou_pred, labels, dets)
        return res['mask_pred'], _to_host_pending(scores, labels)

    def _mask_test_result(self, segms, pending, start, count):
        num_classes = self.mask_iou_head.num_classes
        if pending is None or count == 0:
            return segms, [[] for _ in range(num_classes)]
        scores, labels = (t.numpy()[start:start + count] for t in pending)
        return segms, group_mask_scores(scores, labels, num_classes)


@HEADS.register_module()
class GridRoIHead(StandardRoIHead):
    """``GridRoIHead`` -- mmdet/models/roi_heads/grid_roi_head.py, inference (:15-24, :127-164): the RoI head of
    configs/grid_rcnn, a ``StandardRoIHead`` whose bbox head only classifies (``Shared2FCBBoxHead(with_reg=False)``: the
    detections are the clipped proposals that survive the NMS) and whose ``grid_head`` (``GridHead``) then moves every kept
    box to the vote of nine predicted grid points.  ``grid_roi_extractor=None`` shares the bbox extractor.  ``simple_test``
    is the reference's sequence; ``batch_simple_test`` runs one grid chain for the detections of all images and gives,
    per image, ``simple_test``'s bits.  A configured ``mask_head`` runs the base class's mask test on the refined boxes.
    Training, test-time augmentation and HIP-graph capture raise."""

    def __init__(self, grid_roi_extractor=None, grid_head=None, **kwargs):
        if grid_head is None:
            raise ValueError('GridRoIHead needs a grid_head (grid_roi_head.py:16)')
        super().__init__(**kwargs)
        if not self.with_bbox:
            raise ValueError('GridRoIHead needs a bbox branch (grid_roi_head.py:134)')
        if grid_roi_extractor is not None:
            self.grid_roi_extractor = build_roi_extractor(grid_roi_extractor)
            self.share_roi_extractor = False
        else:
            self.share_roi_extractor = True
            self.grid_roi_extractor = self.bbox_roi_extractor
        self.grid_head = build_head(grid_head)

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained)
        self.grid_head.init_weights()
        if not self.share_roi_extractor:
            self.grid_roi_extractor.init_weights()

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('GridRoIHead.forward_train: Grid R-CNN training (the jittered positives, the grid targets, '
                                  'the unfused branch and the loss) is the follow-up to inference')

    def aug_test(self, x, proposal_list, img_metas, rescale=False, encode=False):
        raise NotImplementedError('GridRoIHead.aug_test: the reference has none for Grid R-CNN (grid_roi_head.py inherits '
                                  'StandardRoIHead.aug_test, which never runs the grid head)')

    def enable_inference_graphs(self, on=True, buckets=None, batch_buckets=None):
        if on:
            raise NotImplementedError('GridRoIHead: HIP-graph capture of the grid chain is a follow-up')
        self._mask_graphs = None
        return None

    def _grid_refine(self, x, det_bboxes_list):
        """The grid chain of grid_roi_head.py:139-147 for the detections of the images of a call, as one chain: RoIs from
        ``det_bboxes[:, :4]`` (batch column = image index), the 14 x 14 RoI features, ``grid_head``, ``get_bboxes`` on the
        ``fused`` heatmap -> the refined [sum n, 5].  Nothing is launched for zero detections."""
        dets = torch.cat(list(det_bboxes_list)).contiguous() if len(det_bboxes_list) > 1 else det_bboxes_list[0].contiguous()
        if dets.shape[0] == 0:
            return dets.new_zeros((0, 5))
        with torch.no_grad():
            grid_rois = bbox2roi([d[:, :4] for d in det_bboxes_list]).contiguous()
            ext = self.grid_roi_extractor
            grid_feats = ext(x[:len(ext.featmap_strides)], grid_rois)
            grid_pred = self.grid_head(grid_feats)
            return self.grid_head.get_bboxes(dets, grid_pred['fused'])

    def _rescale_(self, det_bboxes, scale_factor):
        """grid_roi_head.py:148-152."""
        if det_bboxes.shape[0] == 0:
            return det_bboxes
        if not isinstance(scale_factor, (float, torch.Tensor)):
            scale_factor = self._scale_factor_on(np.asarray(scale_factor, dtype=np.float32), det_bboxes.device)
        det_bboxes[:, :4] /= scale_factor
        return det_bboxes

    @torch.no_grad()
    def simple_test_grid(self, x, proposal_list, img_metas, rescale=False):
        """``simple_test`` up to the refined detections on the device -> (det_bboxes [n, 5], det_labels [n])."""
        det_bboxes, det_labels = self.simple_test_bboxes(x, img_metas, proposal_list, self.test_cfg, rescale=False)
        det_bboxes = self._grid_refine(x, [det_bboxes])
        if rescale:
            det_bboxes = self._rescale_(det_bboxes, img_metas[0]['scale_factor'])
        return det_bboxes, det_labels

    @torch.no_grad()
    def simple_test(self, x, proposal_list, img_metas, proposals=None, rescale=False, encode=False):
        """grid_roi_head.py:127-164."""
        det_bboxes, det_labels = self.simple_test_grid(x, proposal_list, img_metas, rescale=rescale)
        bbox_results = bbox2result(det_bboxes, det_labels, self._bbox_num_classes())
        if not self.with_mask:
            return bbox_results
        segm_results = self.simple_test_mask(x, img_metas, det_bboxes, det_labels, rescale=rescale, encode=encode)
        return bbox_results, segm_results

    @torch.no_grad()
    def batch_simple_test_grid(self, x, proposal_list, img_metas, rescale=False):
        """``simple_test_grid`` of B images -> list of B (det_bboxes, det_labels), each with the bits of the one-image
        call: one bbox branch, one segmented NMS and ONE grid chain over the detections of all images."""
        B = self._check_batch(img_metas, proposal_list=proposal_list)
        self._check_metas(img_metas, self._META_KEYS)
        for i, f in enumerate(x):
            if f.shape[0] != B:
                raise ValueError(f'x[{i}] has batch dimension {f.shape[0]} for {B} images')
        dets = self.batch_simple_test_bboxes(x, img_metas, proposal_list, self.test_cfg, rescale=False)
        refined = self._grid_refine(x, [d for d, _ in dets])
        out, start = [], 0
        for (d, labels), meta in zip(dets, img_metas):
            r = refined[start:start + d.shape[0]]
            start += d.shape[0]
            if rescale:
                r = self._rescale_(r.clone(), meta['scale_factor'])
            out.append((r, labels))
        return out

    @torch.no_grad()
    def batch_simple_test(self, x, proposal_list, img_metas, rescale=False, encode=False):
        dets = self.batch_simple_test_grid(x, proposal_list, img_metas, rescale=rescale)
        counts = [int(d.shape[0]) for d, _ in dets]
        num_classes = self._bbox_num_classes()
        if sum(counts) == 0:
            bbox_results = [_bbox2result_host(dets[0][0].new_zeros((0, 5)), None, num_classes) for _ in dets]
            labels_h = []
        else:
            d_np, l_np = _to_host(torch.cat([d for d, _ in dets]), torch.cat([l for _, l in dets]))
            labels_h = l_np.tolist()
            bbox_results, start = [], 0
            for c in counts:
                bbox_results.append(_bbox2result_host(d_np[start:start + c], l_np[start:start + c], num_classes))
                start += c
        if not self.with_mask:
            return bbox_results
        segm_results = self.batch_simple_test_mask(x, img_metas, [d for d, _ in dets], [l for _, l in dets],
                                                   rescale=rescale, encode=encode, _labels_host=labels_h)
        return list(zip(bbox_results, segm_results))


@HEADS.register_module()
class DoubleHeadRoIHead(StandardRoIHead):
    """``DoubleHeadRoIHead`` -- mmdet/models/roi_heads/double_roi_head.py, inference: the RoI head of configs/double_heads,
    a ``StandardRoIHead`` whose bbox head (``DoubleConvFCBBoxHead``) classifies from the RoI features of the proposals and
    regresses from those of the proposals enlarged by ``reg_roi_scale_factor`` about their centres (the FPN level is the
    proposal's own in both).  Only ``_bbox_forward`` differs: ``simple_test``, ``batch_simple_test``, ``aug_test`` and a
    configured mask branch are the base class's.  Training raises."""

    def __init__(self, reg_roi_scale_factor, **kwargs):
        super().__init__(**kwargs)
        if not self.with_bbox:
            raise ValueError('DoubleHeadRoIHead needs a bbox branch')
        self.reg_roi_scale_factor = reg_roi_scale_factor

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('DoubleHeadRoIHead.forward_train: Double-Head R-CNN training (BatchNorm in train mode, the '
                                  'backward of the conv branch) is the follow-up to inference')

    def _bbox_forward(self, x, rois):
        """double_roi_head.py:16-33; ``bbox_feats`` are the classification features."""
        ext = self.bbox_roi_extractor
        rois = rois.contiguous()
        bbox_cls_feats = ext(x[:ext.num_inputs], rois)
        bbox_reg_feats = ext(x[:ext.num_inputs], rois, roi_scale_factor=self.reg_roi_scale_factor)
        cls_score, bbox_pred = self.bbox_head(bbox_cls_feats, bbox_reg_feats)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_cls_feats)


@HEADS.register_module()
class CascadeRoIHead(StandardRoIHead):
    """cascade_roi_head.py:12-448 for inference: ``num_stages`` bbox stages, each re-regressing all RoIs by the class of
    its own argmax (``regress_by_class``), the classification scores averaged over the stages, and for the kept
    detections the mask heads of all stages, whose sigmoids are averaged (``merge_aug_masks``).  ``bbox_roi_extractor``,
    ``bbox_head``, ``mask_roi_extractor`` and ``mask_head`` are ``ModuleList``s built from a dict (the same config for
    every stage) or a list of ``num_stages`` dicts; the fork's ``mask_predictor.*`` keys are there (Quirk Q4), so the
    ``state_dict`` is the reference's.

    HIP: one ``dm_cascade_refine`` per stage boundary (argmax, class gather, decode, clip to the RoI's own image, batch
    column and the score sum in the reference's order), and the mask heads of up to three stages as ONE launch per layer
    (``ops.conv2d_group`` / ``deconv2x2_group`` / ``conv1x1_group``; ``ops.CASCADE_GROUPED[0] = False`` or
    DM_CASCADE_GROUPED=0: the stage chains one after the other).  The mask RoIAlign runs once when the stages' mask
    extractor configs are equal.  The mask prediction handed to the paste is the merged probabilities [n, 1, S, S]
    (``_mask_test_sigmoid = False``).  A meta with ``flip=True`` un-flips every stage's mask in ``simple_test`` as the
    reference's ``merge_aug_masks`` call does (Quirk Q16).  Out of scope: training (Quirk Q5), graph capture and the shared
    mask extractor form (``mask_roi_extractor=None``).  HybridTaskCascadeRoIHead builds on this head."""

    _mask_test_sigmoid = False

    def __init__(self, num_stages, stage_loss_weights, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None,
                 mask_head=None, shared_head=None, train_cfg=None, test_cfg=None):
        if isinstance(num_stages, bool) or not isinstance(num_stages, int) or num_stages < 1:
            raise ValueError(f'num_stages: a positive int (got {num_stages!r})')
        if not isinstance(stage_loss_weights, (list, tuple)) or len(stage_loss_weights) != num_stages:
            raise ValueError(f'stage_loss_weights: one weight per stage ({num_stages})')
        if bbox_roi_extractor is None or bbox_head is None:
            raise ValueError('CascadeRoIHead needs bbox_roi_extractor and bbox_head (cascade_roi_head.py:29-30)')
        if shared_head is not None:
            raise NotImplementedError('Shared head is not supported in Cascade RCNN anymore')
        if mask_head is not None and mask_roi_extractor is None:
            raise NotImplementedError('the shared-extractor form (mask_roi_extractor=None): no cascade mask config uses it')
        super().__init__(train_cfg=train_cfg, test_cfg=test_cfg)
        self._merge_metas = None        # the metas of the current mask test (the flip of Quirk Q16)
        self.num_stages = num_stages
        self.stage_loss_weights = stage_loss_weights
        exts, heads = self._per_stage(bbox_roi_extractor, 'bbox_roi_extractor'), self._per_stage(bbox_head, 'bbox_head')
        self.bbox_roi_extractor = nn.ModuleList([build_roi_extractor(c) for c in exts])
        self.bbox_head = nn.ModuleList([build_head(c) for c in heads])
        if mask_head is not None:
            mexts = self._per_stage(mask_roi_extractor, 'mask_roi_extractor')
            self.mask_head = nn.ModuleList([build_head(c) for c in self._per_stage(mask_head, 'mask_head')])
            self.share_roi_extractor = False
            self.mask_roi_extractor = nn.ModuleList([build_roi_extractor(c) for c in mexts])
            # RoIAlign has no parameters: equal configs give equal features, extracted once
            self._one_mask_extraction = all(dict(c) == dict(mexts[0]) for c in mexts)

    def _per_stage(self, cfg, name):
        if isinstance(cfg, (list, tuple)):
            if len(cfg) != self.num_stages:
                raise ValueError(f'{name}: {len(cfg)} configs for {self.num_stages} stages')
            return list(cfg)
        return [cfg for _ in range(self.num_stages)]

    def init_weights(self, pretrained=None):
        for h in self.bbox_head:
            h.init_weights()
        if self.with_mask:
            for h in self.mask_head:
                h.init_weights()

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None):
        raise NotImplementedError('CascadeRoIHead training: its mask loss ends in FCNMaskHead.loss, which the reference '
                                  'fork broke (Quirk Q5)')

    def enable_inference_graphs(self, on=True, buckets=None, batch_buckets=None):
        if on:
            raise NotImplementedError('CascadeRoIHead: HIP-graph capture of its mask call is a follow-up')
        self._mask_graphs = None
        return None

    # ------------------------------------------------------------ bbox stages
    def _bbox_num_classes(self):
        return self.bbox_head[-1].num_classes

    def _bbox_forward_stage(self, i, x, rois):
        """cascade_roi_head.py:126-137 (test form)."""
        ext = self.bbox_roi_extractor[i]
        cls_score, bbox_pred = self.bbox_head[i](ext(x[:ext.num_inputs], rois))
        return cls_score, bbox_pred

    @torch.no_grad()
    def _bbox_test_preds(self, x, rois, img_metas):
        """cascade_roi_head.py:304-318: the stages one after the other, each stage's RoIs ``regress_by_class`` of the
        previous ones clipped to the RoI's own image (``img_metas[rois[:, 0]]['img_shape']``), the scores summed in stage
        order and divided by ``num_stages`` as the reference's ``sum(ms_scores) / self.num_stages``."""
        n = rois.shape[0]
        head = self.bbox_head[-1]
        if n == 0:
            nb = 1 if head.reg_class_agnostic else head.num_classes
            return rois, rois.new_zeros((0, head.num_classes + 1)), rois.new_zeros((0, 4 * nb)), head
        img_tab = ops.image_shape_table(img_metas, rois.device)
        score_sum = None
        for i in range(self.num_stages):
            cls_score, bbox_pred = self._bbox_forward_stage(i, x, rois)
            if score_sum is None:
                score_sum = torch.empty_like(cls_score)
            h = self.bbox_head[i]
            last = i == self.num_stages - 1
            new_rois = ops.cascade_refine(rois, cls_score.contiguous(), bbox_pred.contiguous(), h.num_classes, img_tab,
                                          score_sum, first=i == 0, class_agnostic=h.reg_class_agnostic,
                                          means=h.bbox_coder.means, stds=h.bbox_coder.stds, regress=not last)
            if not last:
                rois = new_rois
        return rois, score_sum / self.num_stages, bbox_pred, head

    # ------------------------------------------------------------ mask stages
    def _mask_logits_size(self):
        h = self.mask_head[-1]
        s = self.mask_roi_extractor[-1].roi_layers[0].output_size[0]
        return h.conv_logits.out_channels, int(s * (h.scale_factor if h.upsample is not None else 1))

    def _segm_num_classes(self):
        return self.mask_head[-1].num_classes

    def _grouped_ok(self):
        """The stage-grouped launches take the stock FCNMaskHead (deconv upsample) of equal shapes, exact fp32."""
        if not ops.CASCADE_GROUPED[0] or ops.inference_precision() != 'fp32':
            return False
        h0 = self.mask_head[0]
        for h in self.mask_head:
            if type(h).__name__ != 'FCNMaskHead' or h.upsample_method != 'deconv' or h.num_convs != h0.num_convs or \
                    h.conv_kernel_size not in (1, 3) or h.conv_kernel_size != h0.conv_kernel_size or \
                    h.in_channels != h0.in_channels or h.conv_out_channels != h0.conv_out_channels or \
                    h.conv_logits.out_channels != h0.conv_logits.out_channels:
                return False
        return True

    def _fcn_group(self, heads, feats):
        """FCNMaskHead.forward of up to three stages on their features (one tensor per stage, possibly the same one):
        one launch per layer."""
        xs = list(feats)
        h0 = heads[0]
        for j in range(h0.num_convs):
            convs = [h.convs[j].conv for h in heads]
            xs = ops.conv2d_group(xs, [c.packed([xs[0].shape[1]]) for c in convs], [c.bias.detach() for c in convs],
                                  convs[0].out_channels, h0.conv_kernel_size, relu=True)
        ups = [h.upsample for h in heads]
        wps = [u._pk.get('w', u.weight, lambda w: ops.pack_deconv_weight(w, precision='fp32'), precision='fp32') for u in ups]
        xs = ops.deconv2x2_group(xs, wps, [u.bias.detach() for u in ups], ups[0].out_channels, relu=True)
        cls = [h.conv_logits for h in heads]
        return ops.conv1x1_group(xs, [c.packed([xs[0].shape[1]]) for c in cls], [c.bias.detach() for c in cls],
                                 [c.out_channels for c in cls])

    @torch.no_grad()
    def _stage_mask_logits(self, x, mask_rois):
        """Every stage's mask logits [n, C, S, S] of the RoIs (cascade_roi_head.py:340-344 / 430-433)."""
        feats = []
        for i in range(self.num_stages):
            if i > 0 and self._one_mask_extraction:
                feats.append(feats[0])
                continue
            ext = self.mask_roi_extractor[i]
            feats.append(ext(x[:ext.num_inputs], mask_rois))
        with ops.splitk_scope():                # inference: the 14 x 14 launches of few workgroups may split their K loop
            if not self._grouped_ok():
                return [self.mask_head[i](feats[i]) for i in range(self.num_stages)]
            out = []
            for s0 in range(0, self.num_stages, 3):
                idx = range(s0, min(s0 + 3, self.num_stages))
                out += self._fcn_group([self.mask_head[i] for i in idx], [feats[i] for i in idx])
            return out

    @staticmethod
    def _merge_view(meta):
        """The view row ``merge_aug_masks`` gives a stage's mask in simple_test: the meta's flip (Quirk Q16)."""
        flip = bool(meta.get('flip', False))
        return dict(img_shape=meta.get('img_shape', (1, 1)), scale_factor=1.0, flip=flip,
                    flip_direction=meta.get('flip_direction', 'horizontal') if flip else None)

    def _mask_test_pred(self, x, boxes, labels, det_bboxes):
        """The merged probabilities [sum n, 1, S, S]: every stage's logits of the detections, their label channel,
        sigmoid, un-flipped by the image's meta and averaged over the stages in stage order (dm_merge_aug_masks)."""
        mask_rois = bbox2roi(list(boxes)).contiguous()
        labels_all = torch.cat(list(labels)).contiguous()
        logits = [t.contiguous() for t in self._stage_mask_logits(x, mask_rois)]
        metas = self._merge_metas or [dict() for _ in boxes]          # (set by the mask-test entry points)
        views = [self._merge_view(m) for m in metas]
        codes = [ops.aug_view_rows([v])[0][6] for v in views]
        if all(c == codes[0] for c in codes):
            tab = ops.aug_view_table([views[0]] * self.num_stages, mask_rois.device)
            return ops.merge_aug_masks(logits, labels_all, tab), None
        out, r0 = [], 0
        for b, v in enumerate(views):
            r1 = r0 + int(boxes[b].shape[0])
            if r1 > r0:
                tab = ops.aug_view_table([v] * self.num_stages, mask_rois.device)
                out.append(ops.merge_aug_masks([t[r0:r1].contiguous() for t in logits], labels_all[r0:r1].contiguous(), tab))
            r0 = r1
        return torch.cat(out), None

    def simple_test_mask(self, x, img_metas, det_bboxes, det_labels, rescale=False, encode=False):
        self._merge_metas = img_metas
        try:
            return super().simple_test_mask(x, img_metas, det_bboxes, det_labels, rescale=rescale, encode=encode)
        finally:
            self._merge_metas = None

    @torch.no_grad()
    def batch_simple_test_mask(self, x, img_metas, det_bboxes_list, det_labels_list, rescale=False, encode=False,
                               _labels_host=None):
        self._merge_metas = img_metas
        try:
            return super().batch_simple_test_mask(x, img_metas, det_bboxes_list, det_labels_list, rescale=rescale,
                                                  encode=encode, _labels_host=_labels_host)
        finally:
            self._merge_metas = None

    def simple_test_mask_logits(self, x, det_bboxes, det_labels, scale_factor=1.0, rescale=False):
        """The detections' merged probabilities [n, 1, S, S] (no flip): what ``simple_test_mask`` pastes."""
        if det_bboxes.shape[0] == 0:
            return self._empty_mask_logits(det_bboxes, channels=1)
        _bboxes = det_bboxes[:, :4] * scale_factor if rescale else det_bboxes
        self._merge_metas = [dict()]
        try:
            return self._mask_test_pred(x, [_bboxes], [det_labels], [det_bboxes])[0]
        finally:
            self._merge_metas = None

    @torch.no_grad()
    def aug_test_mask_probs(self, x, img_metas, det_bboxes, det_labels):
        """cascade_roi_head.py:424-437: the detections mapped into every view, every stage's mask prediction there, and
        the V x num_stages sigmoids un-flipped and averaged in (view, stage) order -- one dm_merge_aug_masks call."""
        views = self._check_aug(x, img_metas)
        if det_bboxes.shape[0] == 0:
            return self._empty_mask_logits(det_bboxes, channels=1)
        tab = ops.aug_view_table(views, det_bboxes.device)
        rois = ops.bbox_mapping_multi(det_bboxes, tab)
        labels = det_labels.contiguous()
        logits, rows = [], []
        for v, meta in enumerate(views):
            logits += [t.contiguous() for t in self._stage_mask_logits(x[v], rois[v].contiguous())]
            rows += [meta] * self.num_stages
        return ops.merge_aug_masks(logits, labels, ops.aug_view_table(rows, det_bboxes.device))

    @torch.no_grad()
    def aug_test(self, x, proposal_list, img_metas, rescale=False, encode=False):
        """cascade_roi_head.py:360-448: the cascade per view, merge_aug_bboxes + NMS, the masks of every view and stage
        merged.  The reference returns the boxes in original-image coordinates whatever ``rescale`` is."""
        return super().aug_test(x, proposal_list, img_metas, rescale=True, encode=encode)


@HEADS.register_module()
class HybridTaskCascadeRoIHead(CascadeRoIHead):
    """htc_roi_head.py:11-560 for inference: CascadeRoIHead with (1) a semantic branch over the whole image
    (``semantic_head``, a FusedSemanticHead) whose feature map is RoIAligned (``semantic_roi_extractor``) and added to the
    RoI features of every box stage (pooled to their size) and of the mask branch (``semantic_fusion``), and (2) mask
    information flow: stage i's mask head reads ``mask_feats + relu(conv_res_i(stage i - 1's features))``.

    The semantic feature is computed once per public call and view and shared by the box stages and the mask branch: a
    cache that lives for the duration of the outermost public entry point and is keyed on the identity of the view's
    feature list; a partial entry point called alone computes it itself.  HIP: the fusion is ONE launch per use
    (ops.roi_align_add_: no [N, 256, 14, 14] intermediate); the mask RoIAlign runs once (``mask_roi_extractor[-1]``); the
    stages' conv chains run one after the other (the information flow orders them), their deconvs and logits convs as
    one grouped launch each (ops.CASCADE_GROUPED, exact fp32), the merge is CascadeRoIHead's (Quirk Q16 included).
    ``simple_test`` / ``aug_test`` never add a ``last_pred`` to the stage logits (only the reference's unused
    ``_mask_forward_test`` does).  Quirks Q17-Q20 are kept.  Out of scope: training, graph capture."""

    def __init__(self, num_stages, stage_loss_weights, semantic_roi_extractor=None, semantic_head=None,
                 semantic_fusion=('bbox', 'mask'), interleaved=True, mask_info_flow=True, **kwargs):
        super().__init__(num_stages, stage_loss_weights, **kwargs)
        if not (self.with_bbox and self.with_mask):
            raise ValueError('HybridTaskCascadeRoIHead needs bbox and mask heads (htc_roi_head.py:28)')
        if not mask_info_flow:
            raise NotImplementedError('mask_info_flow=False cannot run in the reference: HTCMaskHead.forward returns the list '
                                      '[mask_pred, res_feat] and htc_roi_head.py:351 calls .sigmoid() on it (Quirk Q20)')
        for h in self.mask_head:
            if type(h).__name__ != 'HTCMaskHead':
                raise NotImplementedError(f'mask information flow needs HTCMaskHead stages (got {type(h).__name__})')
        if semantic_head is not None:
            # (overwrites the 56 x 56 stride-4 extractor BaseRoIHead gives every RoI head: Quirk Q4)
            self.semantic_roi_extractor = build_roi_extractor(semantic_roi_extractor)
            self.semantic_head = build_head(semantic_head)
        self.semantic_fusion = semantic_fusion
        self.interleaved = interleaved
        self.mask_info_flow = mask_info_flow
        self._sem_cache = None          # {id(view feature list): (the list, its semantic feature)} inside a public call
        self._sem_depth = 0
        self._aug_mask = False          # inside aug_test_mask_probs (Quirk Q17)
        if self.with_semantic:
            if len(self.semantic_roi_extractor.roi_layers) != 1:
                raise NotImplementedError('semantic_roi_extractor: one feature level (the semantic map)')
            s = self._semantic_size()
            if 'bbox' in self.semantic_fusion:
                for e in self.bbox_roi_extractor:
                    ops.roi_align_pool(s, e.roi_layers[0].output_size[0])           # (raises NotImplementedError)
            # the mask branch: the identity only -- simple_test adds without pooling (Quirk Q18)
            if ops.roi_align_pool(s, self.mask_roi_extractor[-1].roi_layers[0].output_size[0]) != 1:
                raise NotImplementedError(f'semantic RoI features of {s} x {s} join mask RoI features of the same size only')

    @property
    def with_semantic(self):
        return getattr(self, 'semantic_head', None) is not None

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained)
        if self.with_semantic:
            self.semantic_head.init_weights()

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError('HybridTaskCascadeRoIHead training: its mask loss ends in FCNMaskHead.loss, which the '
                                  'reference fork broke (Quirk Q5); the semantic loss and the interleaved sampling are not built')

    # ------------------------------------------------------------ the semantic feature of a view
    def _semantic_size(self):
        return self.semantic_roi_extractor.roi_layers[0].output_size[0]

    def _semantic_feat(self, x):
        """``semantic_head(x)`` of the view whose feature list is ``x`` (None without a semantic head); inside a public
        entry point it is computed once per list object."""
        if not self.with_semantic:
            return None
        if self._sem_cache is None:
            return self.semantic_head(x)
        e = self._sem_cache.get(id(x))
        if e is None or e[0] is not x:
            e = (x, self.semantic_head(x))          # (the list is held: its id cannot be reused while the entry lives)
            self._sem_cache[id(x)] = e
        return e[1]

    def _fuse_semantic_(self, feats, x, rois):
        """``feats += pool(RoIAlign(semantic feature, rois))`` (htc_roi_head.py:170-176 / :339-342), one launch."""
        lay = self.semantic_roi_extractor.roi_layers[0]
        return ops.roi_align_add_(feats, self._semantic_feat(x), rois.contiguous(), lay.output_size[0], lay.spatial_scale,
                                  lay.sampling_ratio)

    # ------------------------------------------------------------ bbox stages
    def _bbox_forward_stage(self, i, x, rois):
        """htc_roi_head.py:165-181."""
        ext = self.bbox_roi_extractor[i]
        feats = ext(x[:ext.num_inputs], rois)
        if self.with_semantic and 'bbox' in self.semantic_fusion:
            self._fuse_semantic_(feats, x, rois)
        return self.bbox_head[i](feats)

    # ------------------------------------------------------------ mask stages
    def _grouped_ok(self):
        """CascadeRoIHead's condition for the HTC stages' deconvs and logits convs (their conv chains never group)."""
        if not ops.CASCADE_GROUPED[0] or ops.inference_precision() != 'fp32':
            return False
        h0 = self.mask_head[0]
        for h in self.mask_head:
            if h.upsample_method != 'deconv' or h.conv_out_channels != h0.conv_out_channels or \
                    h.conv_logits.out_channels != h0.conv_logits.out_channels or h.scale_factor != h0.scale_factor:
                return False
        return True

    @torch.no_grad()
    def _stage_mask_logits(self, x, mask_rois):
        """htc_roi_head.py:333-351 (simple_test) / :521-543 (aug_test): one RoIAlign, the semantic RoI feature added, the
        stages' conv chains in sequence with information flow, then every stage's deconv and logits."""
        ext = self.mask_roi_extractor[-1]
        mask_feats = ext(x[:ext.num_inputs], mask_rois)
        if self.with_semantic and (self._aug_mask or 'mask' in self.semantic_fusion):       # (Quirk Q17)
            self._fuse_semantic_(mask_feats, x, mask_rois)
        res, last = [], None
        with ops.splitk_scope():
            for h in self.mask_head:
                last = h.res_feat(mask_feats, last)
                res.append(last)
        # (outside the split scope: both forms of the tail then give the same bits)
        if not self._grouped_ok():
            return [h.logits(r) for h, r in zip(self.mask_head, res)]
        out = []
        for s0 in range(0, self.num_stages, 3):
            heads = [self.mask_head[i] for i in range(s0, min(s0 + 3, self.num_stages))]
            ups = [h.upsample for h in heads]
            wps = [u._pk.get('w', u.weight, lambda w: ops.pack_deconv_weight(w, precision='fp32'), precision='fp32') for u in ups]
            xs = ops.deconv2x2_group(res[s0:s0 + 3], wps, [u.bias.detach() for u in ups], ups[0].out_channels, relu=True)
            cls = [h.conv_logits for h in heads]
            out += ops.conv1x1_group(xs, [c.packed([xs[0].shape[1]]) for c in cls], [c.bias.detach() for c in cls],
                                     [c.out_channels for c in cls])
        return out

    @torch.no_grad()
    def aug_test_mask_probs(self, x, img_metas, det_bboxes, det_labels):
        self._aug_mask = True
        try:
            return self._scoped('aug_test_mask_probs', x, img_metas, det_bboxes, det_labels)
        finally:
            self._aug_mask = False

    @torch.no_grad()
    def aug_test_mask(self, x, img_metas, det_bboxes, det_labels, encode=False, _labels_host=None):
        if det_bboxes.shape[0] == 0:
            self._check_aug(x, img_metas)
            return [[] for _ in range(self._segm_num_classes() - 1)]        # htc_roi_head.py:497-500 (Quirk Q19)
        return self._scoped('aug_test_mask', x, img_metas, det_bboxes, det_labels, encode=encode, _labels_host=_labels_host)

    # ------------------------------------------------------------ the public entry points hold the semantic cache
    def _scoped(self, name, *args, **kwargs):
        """CascadeRoIHead's ``name`` with the semantic cache open; the outermost call closes (and empties) it."""
        if self._sem_depth == 0:
            self._sem_cache = {}
        self._sem_depth += 1
        try:
            return getattr(super(), name)(*args, **kwargs)
        finally:
            self._sem_depth -= 1
            if self._sem_depth == 0:
                self._sem_cache = None


def _scoped_entry(name):
    def entry(self, *args, **kwargs):
        return self._scoped(name, *args, **kwargs)
    entry.__name__ = name
    entry.__doc__ = getattr(CascadeRoIHead, name).__doc__
    return entry


for _name in ('simple_test', 'batch_simple_test', 'aug_test', 'simple_test_bboxes', 'batch_simple_test_bboxes',
              'aug_test_bboxes', 'simple_test_mask', 'batch_simple_test_mask', 'simple_test_mask_logits',
              'batch_simple_test_mask_logits'):
    setattr(HybridTaskCascadeRoIHead, _name, _scoped_entry(_name))
