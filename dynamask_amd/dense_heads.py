"""Dense heads behind the reference's HEADS registry, at inference: ``RPNHead`` (mmdet/models/dense_heads/rpn_head.py over
anchor_head.py and rpn_test_mixin.py) -- the proposals the RoI heads start from.

``forward`` is three exact-fp32 launches per level: ``rpn_conv`` 3x3 + ReLU (``dm_conv2d_fwd``; ``dm_conv3x3_dil_fwd`` at
dilation 1 on maps wider than CONV2D_3X3_MAX_WIDTH, which the former does not take), ``rpn_cls`` and ``rpn_reg`` 1x1
(``dm_conv2d_fwd``).  ``get_bboxes`` treats every (image, level) as one segment and runs ALL of them through one selection
(``dm_rpn_select``: the ``nms_pre`` best anchors in score order, read straight from the NCHW logits), one decode
(``dm_rpn_decode``: anchors made from the base-anchor table, deltas gathered from the NCHW map -- no anchor grid, no
permuted copy), one segmented NMS (``ops.nms_segmented``) and one merge (``dm_rpn_merge``: the image's best ``nms_post``);
the host waits once, for the per-image counts.  ``DM_RPN_FUSED=0`` (or clearing ``RPN_FUSED``) runs the same steps composed
of ``ops.sigmoid``, a stable ``torch.sort``, gathers, ``AnchorGenerator.grid_anchors``, ``ops.bbox_decode``,
``ops.nms_segmented`` and a stable sort of the concatenated survivors: the same bits.  ``aug_test_rpn`` (test-time
augmentation) runs ``simple_test_rpn`` per view and merges: one ``dm_proposals_mapping_back`` launch for all views and images,
one segmented NMS over the images, one more host wait whatever the batch.

Deviation from mmcv's ``batched_nms``: it shifts every level's boxes by ``level * (max coordinate + 1)`` in
fp32 before the IoU; here every level is suppressed on its own unshifted boxes."""
import os

import torch
import torch.nn as nn

from . import anchors  # noqa: F401  (registers AnchorGenerator)
from . import ops
from .bbox_heads import build_bbox_coder
from .layers import CONV2D_3X3_MAX_WIDTH, _exact_conv
from .registry import HEADS, build_anchor_generator

# DM_RPN_FUSED=0: the composed path (the launches that existed before the RPN kernels) instead of dm_rpn_*
def _env_fused():
    return os.environ.get('DM_RPN_FUSED', '1') != '0'


RPN_FUSED = [_env_fused()]


@HEADS.register_module()
class RPNHead(nn.Module):
    """``RPNHead`` -- rpn_head.py:12-168 on AnchorHead (anchor_head.py:13-148, :499-576) and RPNTestMixin.
    ``state_dict`` keys: ``rpn_conv.{weight,bias}``, ``rpn_cls.{weight,bias}``, ``rpn_reg.{weight,bias}``.  The loss
    configs are stored, not built; training (``loss``, ``forward_train``) is not built."""

    def __init__(self, in_channels, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', scales=[8, 16, 32], ratios=[0.5, 1.0, 2.0],
                                       strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0)),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), train_cfg=None, test_cfg=None):
        super().__init__()
        if not loss_cls.get('use_sigmoid', False):
            raise NotImplementedError('RPNHead: loss_cls use_sigmoid=False (the two-channel softmax score) is not built; '
                                      'every RPN config of the reference sets use_sigmoid=True')
        self.in_channels, self.feat_channels = in_channels, feat_channels
        self.num_classes, self.cls_out_channels, self.use_sigmoid_cls = 1, 1, True
        self.background_label = 0
        self.loss_cls_cfg, self.loss_bbox_cfg = loss_cls, loss_bbox
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.fp16_enabled = False
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.anchor_generator = build_anchor_generator(anchor_generator)
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        self.rpn_conv = _exact_conv(in_channels, feat_channels, 3)
        self.rpn_cls = _exact_conv(feat_channels, self.num_anchors * self.cls_out_channels, 1)
        self.rpn_reg = _exact_conv(feat_channels, self.num_anchors * 4, 1)
        self.init_weights()

    def init_weights(self):
        """rpn_head.py:32-36: normal(std=0.01) weights, zero biases."""
        for m in (self.rpn_conv, self.rpn_cls, self.rpn_reg):
            nn.init.normal_(m.weight, mean=0, std=0.01)
            nn.init.constant_(m.bias, 0)

    # ------------------------------------------------------------------ forward
    def forward_single(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('RPNHead: training is not built; run inference under torch.no_grad()')
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f'RPNHead: [B, {self.in_channels}, H, W] features expected, got {tuple(x.shape)}')
        x = x.contiguous()
        if x.shape[3] > CONV2D_3X3_MAX_WIDTH:
            c = self.rpn_conv
            h = ops.conv3x3_dil(x, c.packed([self.in_channels]), c.bias.detach(), self.feat_channels, 1, relu=True)
        else:
            h = self.rpn_conv.run(x, relu=True)
        return self.rpn_cls.run(h), self.rpn_reg.run(h)

    def forward(self, feats):
        """(cls_scores, bbox_preds): per level [B, A, H, W] logits and [B, 4 A, H, W] deltas (anchor_head.py:131-148)."""
        outs = [self.forward_single(x) for x in feats]
        return [o[0] for o in outs], [o[1] for o in outs]

    # ------------------------------------------------------------------ refusals
    def loss(self, *args, **kwargs):
        raise NotImplementedError('RPNHead.loss: RPN training (anchor targets, the sigmoid cross-entropy) is not built')

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError('RPNHead.forward_train: RPN training is not built')

    # ------------------------------------------------------------------ proposals
    def _checked_cfg(self, cfg):
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError('RPNHead.get_bboxes: no test_cfg')
        if cfg.get('nms_across_levels', False):
            raise NotImplementedError('RPNHead: nms_across_levels=True is not built (False in every config of the reference)')
        if cfg.get('min_bbox_size', 0) > 0:
            raise NotImplementedError('RPNHead: min_bbox_size > 0 is not built (0 in every config of the reference): the '
                                      'segment sizes of the NMS would have to come back from the device')
        if cfg['nms_post'] < 1:
            raise ValueError(f"RPNHead: nms_post={cfg['nms_post']}; at least 1 expected")
        return cfg

    def _check_maps(self, cls_scores, bbox_preds, img_metas):
        L = len(cls_scores)
        if L != len(bbox_preds) or L != self.anchor_generator.num_levels:
            raise ValueError(f'RPNHead.get_bboxes: {self.anchor_generator.num_levels} levels of scores and deltas expected, '
                             f'got {L} and {len(bbox_preds)}')
        B = len(img_metas)
        for l, (c, d) in enumerate(zip(cls_scores, bbox_preds)):
            A = self.anchor_generator.num_base_anchors[l]
            if c.dim() != 4 or d.dim() != 4 or c.shape[0] != B or d.shape[0] != B or c.shape[1] != A or \
                    d.shape[1] != 4 * A or c.shape[2:] != d.shape[2:]:
                raise ValueError(f'RPNHead.get_bboxes: level {l}: [{B}, {A}, H, W] scores and [{B}, {4 * A}, H, W] deltas '
                                 f'expected, got {tuple(c.shape)} and {tuple(d.shape)}')
        return B, L

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False):
        """Per image, a [n, 5] tensor (x1, y1, x2, y2, score) of at most ``nms_post`` proposals in descending score order
        (anchor_head.py:500-576 with rpn_head.py:79-168).  ``rescale`` is ignored and ``max_num`` unused, as there."""
        cfg = self._checked_cfg(cfg)
        B, L = self._check_maps(cls_scores, bbox_preds, img_metas)
        if B == 0:
            return []
        with torch.no_grad():
            if RPN_FUSED[0]:
                return self._get_bboxes_fused(cls_scores, bbox_preds, img_metas, cfg, B, L)
            return self._get_bboxes_composed(cls_scores, bbox_preds, img_metas, cfg, B, L)

    def _get_bboxes_fused(self, cls_scores, bbox_preds, img_metas, cfg, B, L):
        gen = self.anchor_generator
        dev = cls_scores[0].device
        table, base_rows = gen.base_anchor_table(dev)
        logits = [cls_scores[l][b].detach() for b in range(B) for l in range(L)]
        deltas = [bbox_preds[l][b].detach() for b in range(B) for l in range(L)]
        segs = ops.RPNSegments(logits, cfg['nms_pre'], deltas, strides=[gen.strides[l] for _ in range(B) for l in range(L)],
                               base_rows=[base_rows[l] for _ in range(B) for l in range(L)],
                               images=[b for b in range(B) for _ in range(L)], num_levels=L)
        idx, score = ops.rpn_select(segs)
        boxes = ops.rpn_decode(segs, idx, table, ops.image_shape_table(img_metas, dev), self.bbox_coder.means,
                               self.bbox_coder.stds)
        keep, kept = ops.nms_segmented(boxes, segs.rows, cfg['nms_thr'])
        out, counts = ops.rpn_merge(segs, keep, kept, boxes, score, cfg['nms_post'])
        counts = counts.cpu().tolist()                   # the call's one host wait
        return [out[b, :counts[b]] for b in range(B)]

    def _get_bboxes_composed(self, cls_scores, bbox_preds, img_metas, cfg, B, L):
        gen = self.anchor_generator
        dev = cls_scores[0].device
        mlvl_anchors = gen.grid_anchors([c.shape[-2:] for c in cls_scores], device=dev)
        nms_pre = cfg['nms_pre']
        seg_boxes, seg_scores, rows = [], [], []
        for b in range(B):
            shape = img_metas[b]['img_shape']
            for l in range(L):
                s = ops.sigmoid(cls_scores[l][b].detach().permute(1, 2, 0).reshape(-1).contiguous())
                ranked, order = torch.sort(s, descending=True, stable=True)
                if nms_pre > 0:
                    ranked, order = ranked[:nms_pre], order[:nms_pre]
                d = bbox_preds[l][b].detach().permute(1, 2, 0).reshape(-1, 4)[order].contiguous()
                a = mlvl_anchors[l][order].contiguous()
                bx, _ = ops.bbox_decode(a, None, d, 1, self.bbox_coder.means, self.bbox_coder.stds, 16 / 1000,
                                        (shape[0], shape[1]), class_agnostic=True)
                seg_boxes.append(bx)
                seg_scores.append(ranked.contiguous())
                rows.append(int(order.numel()))
        boxes, score = torch.cat(seg_boxes), torch.cat(seg_scores)
        keep, kept = ops.nms_segmented(boxes, rows, cfg['nms_thr'])
        kept = kept.cpu().tolist()                       # the call's one host wait
        out, r0 = [], 0
        for b in range(B):
            sel = []
            for l in range(L):
                s = b * L + l
                sel.append(keep[r0:r0 + kept[s]].long() + r0)
                r0 += rows[s]
            sel = torch.cat(sel)
            dets = torch.cat([boxes[sel], score[sel][:, None]], 1)
            order = torch.sort(dets[:, 4], descending=True, stable=True)[1][:cfg['nms_post']]
            out.append(dets[order])
        return out

    def simple_test_rpn(self, x, img_metas):
        """rpn_test_mixin.py:24-37."""
        return self.get_bboxes(*self(x), img_metas)

    def aug_test_rpn(self, feats, img_metas):
        """rpn_test_mixin.py:40-60 with ``merge_aug_proposals`` (merge_augs.py:8-47): ``feats[v]`` / ``img_metas[v]`` are
        view v's maps and its B metas.  Per image, a [n, 5] tensor in ORIGINAL-image coordinates: the views' proposals
        mapped back (one ``dm_proposals_mapping_back`` launch for all views and images), suppressed at ``nms_thr`` (one
        segmented NMS over the images), the ``max_num`` best in score order.  Host waits: each view's one, and one for the
        merge whatever B.  The list-of-views form is the one that is built: any other (no maps, one view's maps given
        bare) raises NotImplementedError."""
        if not isinstance(feats, (list, tuple)) or not isinstance(img_metas, (list, tuple)):
            raise NotImplementedError('RPNHead.aug_test_rpn: built for a list of views only -- feats[v] the maps and '
                                      f'img_metas[v] the metas of view v; got {type(feats).__name__} and '
                                      f'{type(img_metas).__name__}')
        cfg = self._checked_cfg(None)
        if len(feats) != len(img_metas) or len(feats) == 0:
            raise ValueError(f'RPNHead.aug_test_rpn: {len(feats)} views of maps and {len(img_metas)} of metas')
        B = len(img_metas[0])
        if any(len(m) != B for m in img_metas):
            raise ValueError('RPNHead.aug_test_rpn: every view needs the metas of the same images')
        views = [self.simple_test_rpn(x, m) for x, m in zip(feats, img_metas)]
        if B == 0:
            return []
        with torch.no_grad():
            V = len(views)
            # image after image, its views in order: the reference's torch.cat per image
            cat = ops.proposals_mapping_back([views[v][b] for b in range(B) for v in range(V)],
                                             [img_metas[v][b] for b in range(B) for v in range(V)])
            rows = [sum(int(views[v][b].shape[0]) for v in range(V)) for b in range(B)]
            # mmcv nms: descending score, the earlier row first among equals -- per image: one stable sort by score, one by image
            image = torch.repeat_interleave(ops._upload(list(range(B)), torch.int64, cat.device),
                                            ops._upload(rows, torch.int64, cat.device), output_size=sum(rows))
            by_score = torch.sort(cat[:, 4], descending=True, stable=True)[1]
            order = by_score[torch.sort(image[by_score], stable=True)[1]]
            dets = cat[order]
            keep, kept = ops.nms_segmented(dets[:, :4].contiguous(), rows, cfg['nms_thr'], max_num=cfg['max_num'])
            kept = kept.cpu().tolist()                   # the merge's one host wait
            out, r0 = [], 0
            for b in range(B):
                out.append(dets[keep[r0:r0 + kept[b]].long() + r0])
                r0 += rows[b]
            return out
