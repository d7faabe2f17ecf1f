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
import math
import os

import torch
import torch.nn as nn

from . import anchors  # noqa: F401  (registers AnchorGenerator)
from . import ops
from .bbox_heads import build_bbox_coder
from .layers import CONV2D_3X3_MAX_WIDTH, _Conv, _exact_conv, _Packed
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


# ---------------------------------------------------------------------------------------------------------- FCOSHead
# A level whose towers ops.conv2d takes runs them in ONE [B, 2 F, H, W] tensor (the cls half first); dm_conv2d_fwd refuses
# 3x3 maps wider than this and a 1 x 1 map at 64 output channels or fewer: such a level runs every convolution on
# ops.conv3x3_dil (dilation 1, any size) with the towers in two tensors, since that kernel reads no channel slice.
CONV2D_3X3_EXACT_MAX_WIDTH = 168

# get_bboxes: the class-wise NMS runs on the NMS_CANDIDATE_CAP best candidates of an image, a number the host knows without
# asking the device; the true candidate counts come back with the kept counts in the call's ONE host wait, and an image with
# more candidates than the cap (never seen at score_thr = 0.05) runs again at the next power of two that holds them.
NMS_CANDIDATE_CAP = 4096


class _Scale(nn.Module):
    """mmcv.cnn.Scale: the key ``scale``, a 0-d parameter."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


class _GN(nn.Module):
    """Parameter holder named like nn.GroupNorm (weight, bias [C]); the towers' norms run stacked, in ops.group_norm."""

    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__()
        self.num_groups, self.num_channels, self.eps = num_groups, num_channels, eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))


class _TowerConv(nn.Module):
    """mmcv ConvModule(3x3, padding 1, norm_cfg, bias) of a tower: keys ``conv.weight`` (``conv.bias`` with a bias),
    ``gn.weight`` / ``gn.bias`` under GN.  A parameter holder: the head stacks the two towers' layers and launches."""

    def __init__(self, in_channels, out_channels, bias, num_groups):
        super().__init__()
        self.conv = _Conv(in_channels, out_channels, 3, bias=bias)
        self.conv.exact = True
        if num_groups is not None:
            self.gn = _GN(num_groups, out_channels)


@HEADS.register_module()
class FCOSHead(nn.Module):
    """``FCOSHead`` -- fcos_head.py:13-153, :252-396 on AnchorFreeHead (anchor_free_head.py:12-227), at inference.
    ``state_dict`` keys, the reference's in its order: ``cls_convs.{i}.conv.weight`` (``.conv.bias`` only without a norm:
    ``conv_bias='auto'``), ``cls_convs.{i}.gn.{weight,bias}`` under GN, the same for ``reg_convs``, ``conv_cls.*``,
    ``conv_reg.*``, ``conv_centerness.*``, ``scales.{i}.scale`` (0-d).  A state dict without version metadata has its
    pre-2.0 keys renamed (``fcos_cls`` -> ``conv_cls``, ``fcos_reg`` -> ``conv_reg``, ``fcos_centerness`` ->
    ``conv_centerness``: anchor_free_head.py:150-186).  The loss configs are stored, not built.

    ``forward``: per level, both towers in one [B, 2 F, H, W] tensor.  Layer 0 is ONE 3x3 launch ``in_channels -> 2 F`` (the
    two weights stacked); layers 1 .. are one launch per tower, reading and writing the tower's channel slice; the
    GroupNorm + ReLU of both towers is ONE in-place ``ops.group_norm`` with 2 G groups and the concatenated gamma / beta (a
    group never crosses the halves); ``conv_centerness`` is stacked under the predictor that shares its input, so the
    predictors are two launches.  13 launches per level under GN and 9 without at four stacked convolutions.  A level
    ``ops.conv2d`` does not take (wider than 168, a 1 x 1 map at <= 64 output channels) runs on ``ops.conv3x3_dil`` at
    dilation 1 with the towers in two tensors: 18 and 10 launches.  Every convolution is exact fp32 in every precision
    mode; no host wait; an image's bits do not depend on the batch.  ``cls_score`` / ``centerness`` (or ``bbox_pred`` /
    ``centerness`` under ``centerness_on_reg``) are channel slices of one launch's output, not copies.

    Not built (NotImplementedError naming the argument): ``dcn_on_last_conv=True``, a ``conv_cfg``, a ``norm_cfg`` other
    than None or GN, GN groups that do not divide ``feat_channels``, training (``forward_train``, ``loss``,
    ``get_targets``)."""
    _version = 1

    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64),
                 regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8)), center_sampling=False,
                 center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False, dcn_on_last_conv=False,
                 conv_bias='auto', background_label=None,
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), train_cfg=None, test_cfg=None):
        super().__init__()
        if dcn_on_last_conv:
            raise NotImplementedError('FCOSHead: dcn_on_last_conv=True (DCNv2 in the last tower convolutions) is not built')
        if conv_cfg is not None:
            raise NotImplementedError(f'FCOSHead: conv_cfg={conv_cfg} is not built (None in every buildable FCOS config)')
        if norm_cfg is not None and (not isinstance(norm_cfg, dict) or norm_cfg.get('type') != 'GN' or
                                     set(norm_cfg) - {'type', 'num_groups', 'requires_grad'}):
            raise NotImplementedError(f'FCOSHead: norm_cfg={norm_cfg} is not built; None or dict(type="GN", num_groups=G)')
        groups = None if norm_cfg is None else int(norm_cfg['num_groups'])
        if groups is not None and (groups < 1 or feat_channels % groups != 0):
            raise NotImplementedError(f'FCOSHead: norm_cfg num_groups={groups} does not divide feat_channels={feat_channels}')
        assert conv_bias == 'auto' or isinstance(conv_bias, bool)
        if stacked_convs < 1:
            raise NotImplementedError(f'FCOSHead: stacked_convs={stacked_convs}; at least one tower convolution is built')
        if len(regress_ranges) != len(strides):
            raise ValueError(f'FCOSHead: {len(strides)} strides and {len(regress_ranges)} regress_ranges')
        self.num_classes = self.cls_out_channels = num_classes
        self.in_channels, self.feat_channels, self.stacked_convs = in_channels, feat_channels, stacked_convs
        self.strides, self.regress_ranges = strides, regress_ranges
        self.center_sampling, self.center_sample_radius = center_sampling, center_sample_radius
        self.norm_on_bbox, self.centerness_on_reg = norm_on_bbox, centerness_on_reg
        self.dcn_on_last_conv, self.conv_bias = dcn_on_last_conv, conv_bias
        self.loss_cls_cfg, self.loss_bbox_cfg, self.loss_centerness_cfg = loss_cls, loss_bbox, loss_centerness
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.fp16_enabled = False
        self.background_label = num_classes if background_label is None else background_label
        assert self.background_label == 0 or self.background_label == num_classes
        bias = norm_cfg is None if conv_bias == 'auto' else conv_bias
        self.num_groups, self.with_bias = groups, bias
        self.cls_convs = nn.ModuleList([_TowerConv(in_channels if i == 0 else feat_channels, feat_channels, bias, groups)
                                        for i in range(stacked_convs)])
        self.reg_convs = nn.ModuleList([_TowerConv(in_channels if i == 0 else feat_channels, feat_channels, bias, groups)
                                        for i in range(stacked_convs)])
        self.conv_cls = _exact_conv(feat_channels, self.cls_out_channels, 3)
        self.conv_reg = _exact_conv(feat_channels, 4, 3)
        self.conv_centerness = _exact_conv(feat_channels, 1, 3)
        self.scales = nn.ModuleList([_Scale(1.0) for _ in strides])
        self._pk = _Packed()
        self._points = {}
        self._routes = {}
        self.init_weights()

    def init_weights(self):
        """anchor_free_head.py:138-148, fcos_head.py:98-101: normal(std=0.01) weights, zero biases, ``conv_cls``'s bias at
        a prior probability of 0.01."""
        for m in list(self.cls_convs) + list(self.reg_convs):
            nn.init.normal_(m.conv.weight, mean=0, std=0.01)
            if m.conv.bias is not None:
                nn.init.constant_(m.conv.bias, 0)
        for m in (self.conv_cls, self.conv_reg, self.conv_centerness):
            nn.init.normal_(m.weight, mean=0, std=0.01)
            nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.conv_cls.bias, float(-math.log((1 - 0.01) / 0.01)))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """anchor_free_head.py:150-186: a state dict from before version 1 names the predictors ``fcos_*``."""
        if local_metadata.get('version', None) is None:
            renames = (('cls', 'conv_cls'), ('reg', 'conv_reg'), ('centerness', 'conv_centerness'))
            for key in [k for k in state_dict.keys() if k.startswith(prefix)]:
                parts = key[len(prefix):].split('.')
                for end, name in renames:
                    if parts[0].endswith(end) and parts[0] != name and parts[0] not in ('cls_convs', 'reg_convs'):
                        state_dict[prefix + '.'.join([name] + parts[1:])] = state_dict.pop(key)
                        break
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # ------------------------------------------------------------------ refusals
    def loss(self, *args, **kwargs):
        raise NotImplementedError('FCOSHead.loss: training (the focal, IoU and centerness losses) is not built')

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError('FCOSHead.forward_train: training is not built')

    def get_targets(self, *args, **kwargs):
        raise NotImplementedError('FCOSHead.get_targets: training (the point targets) is not built')

    # ------------------------------------------------------------------ stacked parameters
    def _stacked(self, i):
        """Layer i of both towers as one: (packed [2 F, Cin, 3, 3] for layer 0 or None, bias [2 F] or None, gamma, beta
        [2 F] or None)."""
        c, r = self.cls_convs[i], self.reg_convs[i]
        params = [c.conv.weight, r.conv.weight] + ([c.conv.bias, r.conv.bias] if self.with_bias else []) + \
            ([c.gn.weight, c.gn.bias, r.gn.weight, r.gn.bias] if self.num_groups is not None else [])

        def make():
            cat = lambda a, b: torch.cat([a.detach(), b.detach()]).contiguous()      # noqa: E731
            w = ops.pack_conv_weight(cat(c.conv.weight, r.conv.weight), src_channels=[c.conv.in_channels]) if i == 0 else None
            b = cat(c.conv.bias, r.conv.bias) if self.with_bias else None
            if self.num_groups is None:
                return w, b, None, None
            return w, b, cat(c.gn.weight, r.gn.weight), cat(c.gn.bias, r.gn.bias)
        return self._pk.get_multi(('layer', i), params, make)

    def _predictor(self, conv):
        """``conv`` with ``conv_centerness`` stacked under it: (packed [cout + 1, F, 3, 3], bias [cout + 1])."""
        ctr = self.conv_centerness

        def make():
            w = torch.cat([conv.weight.detach(), ctr.weight.detach()]).contiguous()
            return (ops.pack_conv_weight(w, src_channels=[self.feat_channels]),
                    torch.cat([conv.bias.detach(), ctr.bias.detach()]).contiguous())
        return self._pk.get_multi(('pred', conv.out_channels), [conv.weight, conv.bias, ctr.weight, ctr.bias], make)

    def _any_size(self, H, W):
        """Does this level leave ops.conv2d for ops.conv3x3_dil?  Decided from the map's size alone (the launcher's own
        answer for one image), so an image's kernels do not depend on the batch."""
        r = self._routes.get((H, W))
        if r is None:
            F = self.feat_channels
            both = self.centerness_on_reg
            shapes = {(self.in_channels, 2 * F), (F, F), (F, self.cls_out_channels + (0 if both else 1)), (F, 4 + (1 if both else 0))}
            r = W > CONV2D_3X3_EXACT_MAX_WIDTH or any(ops.conv2d_plan_raw([ci], 1, H, W, co, 3)[0] < 0 for ci, co in shapes)
            if r and (self.in_channels % 8 != 0 or F % 8 != 0):
                raise NotImplementedError(f'FCOSHead: a {H} x {W} level runs on the any-size 3x3 kernel, which walks the input '
                                          f'channels in chunks of 8 (in_channels={self.in_channels}, feat_channels={F})')
            self._routes[(H, W)] = r
        return r

    # ------------------------------------------------------------------ forward
    def _towers(self, x):
        """(cls_feat, reg_feat) [B, F, H, W] each -- channel slices of one tensor where ops.conv2d runs the level."""
        F, G, S = self.feat_channels, self.num_groups, self.stacked_convs
        act = G is None                   # without a norm the ReLU rides in the convolution's epilogue
        if self._any_size(x.shape[2], x.shape[3]):
            feats = []
            for tower in (self.cls_convs, self.reg_convs):
                t = x
                for m in tower:
                    c = m.conv
                    t = ops.conv3x3_dil(t, c.packed([c.in_channels]), None if c.bias is None else c.bias.detach(), F, 1, relu=act)
                    if G is not None:
                        ops.group_norm(t, m.gn.weight.detach(), m.gn.bias.detach(), G, m.gn.eps, relu=True, out=t)
                feats.append(t)
            return feats
        t = None
        for i in range(S):
            w, b, gamma, beta = self._stacked(i)
            if i == 0:
                t = ops.conv2d(x, w, b, 2 * F, 3, relu=act)
            else:
                n = torch.empty_like(t)
                for h, tower in enumerate((self.cls_convs, self.reg_convs)):
                    c = tower[i].conv
                    ops.conv2d(t[:, h * F:(h + 1) * F], c.packed([F]), None if c.bias is None else c.bias.detach(), F, 3,
                               relu=act, out=n, out_ch_offset=h * F)
                t = n
            if G is not None:
                ops.group_norm(t, gamma, beta, 2 * G, self.cls_convs[i].gn.eps, relu=True, out=t)
        return t[:, :F], t[:, F:]

    def forward_single(self, x, scale, stride):
        """fcos_head.py:124-153 -> (cls_score [B, num_classes, H, W], bbox_pred [B, 4, H, W], centerness [B, 1, H, W])."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('FCOSHead: training is not built; run inference under torch.no_grad()')
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f'FCOSHead: [B, {self.in_channels}, H, W] features expected, got {tuple(x.shape)}')
        x = x.contiguous()
        cls_feat, reg_feat = self._towers(x)
        nc = self.cls_out_channels
        any_size = self._any_size(x.shape[2], x.shape[3])

        def predict(feat, wq, b, cout):
            if any_size:
                return ops.conv3x3_dil(feat, wq, b, cout, 1)
            return ops.conv2d(feat, wq, b, cout, 3)
        if self.centerness_on_reg:
            cls_score = predict(cls_feat, self.conv_cls.packed([self.feat_channels]), self.conv_cls.bias.detach(), nc)
            both = predict(reg_feat, *self._predictor(self.conv_reg), 5)
            bbox_pred, centerness = both[:, :4], both[:, 4:]
        else:
            both = predict(cls_feat, *self._predictor(self.conv_cls), nc + 1)
            cls_score, centerness = both[:, :nc], both[:, nc:]
            bbox_pred = predict(reg_feat, self.conv_reg.packed([self.feat_channels]), self.conv_reg.bias.detach(), 4)
        bbox_pred = scale(bbox_pred).float()
        if self.norm_on_bbox:
            bbox_pred = torch.relu(bbox_pred)
            if not self.training:
                bbox_pred = bbox_pred * stride
        else:
            bbox_pred = bbox_pred.exp()
        return cls_score, bbox_pred, centerness

    def forward(self, feats):
        """(cls_scores, bbox_preds, centernesses): three lists over the levels (fcos_head.py:103-122)."""
        if len(feats) != len(self.strides):
            raise ValueError(f'FCOSHead: {len(self.strides)} levels expected, got {len(feats)}')
        outs = [self.forward_single(x, s, st) for x, s, st in zip(feats, self.scales, self.strides)]
        return [o[0] for o in outs], [o[1] for o in outs], [o[2] for o in outs]

    # ------------------------------------------------------------------ detections
    def _level_points(self, H, W, stride, device):
        """fcos_head.py:386-396: (x * stride + stride // 2, y * stride + stride // 2) of every cell, row-major, [H W, 2]."""
        key = (H, W, stride, str(device))
        p = self._points.get(key)
        if p is None:
            y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
            p = (torch.stack((x.reshape(-1) * stride, y.reshape(-1) * stride), dim=-1) + stride // 2).to(device)
            self._points[key] = p
        return p

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg=None, rescale=False):
        """fcos_head.py:252-384 for all images at once -> [(det_bboxes [n, 5], det_labels [n])] per image.  Per level:
        sigmoid(cls), sigmoid(centerness), the ``nms_pre`` largest ``max_c(score * centerness)`` where the level has more
        points (``torch.topk``: no promise among exactly equal keys, as in the reference), ``distance2bbox`` clipped to
        ``img_shape``, the division by ``scale_factor`` under ``rescale``; then ``multiclass_nms`` with the centerness as
        ``score_factors`` on the device (``ops.nms_segmented``, one segment per image).  Torch device operators; ONE host
        wait per call, whatever the batch."""
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError('FCOSHead.get_bboxes: no test_cfg')
        L, B = len(cls_scores), len(img_metas)
        if not (L == len(bbox_preds) == len(centernesses) == len(self.strides)):
            raise ValueError(f'FCOSHead.get_bboxes: {len(self.strides)} levels of scores, distances and centernesses expected, '
                             f'got {L}, {len(bbox_preds)} and {len(centernesses)}')
        if B == 0:
            return []
        nms_pre = cfg.get('nms_pre', -1)
        with torch.no_grad():
            dev = cls_scores[0].device
            shapes = ops.image_shape_table(img_metas, dev)                  # [B, 2] = (h, w)
            hmax, wmax = shapes[:, 0:1], shapes[:, 1:2]
            boxes, scores, ctrs = [], [], []
            for l in range(L):
                c = cls_scores[l].detach()
                if c.dim() != 4 or c.shape[0] != B or c.shape[1] != self.cls_out_channels or \
                        bbox_preds[l].shape != (B, 4) + c.shape[2:] or centernesses[l].shape != (B, 1) + c.shape[2:]:
                    raise ValueError(f'FCOSHead.get_bboxes: level {l}: [{B}, {self.cls_out_channels}, H, W] scores, [{B}, 4, H, W] '
                                     f'distances and [{B}, 1, H, W] centernesses expected, got {tuple(c.shape)}, '
                                     f'{tuple(bbox_preds[l].shape)} and {tuple(centernesses[l].shape)}')
                H, W = c.shape[2:]
                s = c.permute(0, 2, 3, 1).reshape(B, H * W, -1).sigmoid()
                ctr = centernesses[l].detach().permute(0, 2, 3, 1).reshape(B, H * W).sigmoid()
                d = bbox_preds[l].detach().permute(0, 2, 3, 1).reshape(B, H * W, 4)
                p = self._level_points(H, W, self.strides[l], dev)[None].expand(B, -1, -1)
                if nms_pre > 0 and H * W > nms_pre:
                    top = (s * ctr[:, :, None]).max(dim=2)[0].topk(nms_pre, dim=1)[1]
                    s = s.gather(1, top[:, :, None].expand(-1, -1, s.shape[2]))
                    ctr = ctr.gather(1, top)
                    d = d.gather(1, top[:, :, None].expand(-1, -1, 4))
                    p = p.gather(1, top[:, :, None].expand(-1, -1, 2))
                # distance2bbox (core/bbox/transforms.py:127-136), max_shape = the image's own
                x1 = torch.minimum((p[:, :, 0] - d[:, :, 0]).clamp(min=0), wmax)
                y1 = torch.minimum((p[:, :, 1] - d[:, :, 1]).clamp(min=0), hmax)
                x2 = torch.minimum((p[:, :, 0] + d[:, :, 2]).clamp(min=0), wmax)
                y2 = torch.minimum((p[:, :, 1] + d[:, :, 3]).clamp(min=0), hmax)
                boxes.append(torch.stack([x1, y1, x2, y2], -1))
                scores.append(s)
                ctrs.append(ctr)
            boxes, scores, ctrs = torch.cat(boxes, 1), torch.cat(scores, 1), torch.cat(ctrs, 1)
            if rescale:
                boxes = boxes / ops._upload([[float(v) for v in m['scale_factor']] for m in img_metas], torch.float32, dev)[:, None]
            return self._multiclass_nms(boxes, scores, ctrs, cfg['score_thr'], cfg['nms'], cfg['max_per_img'])

    @staticmethod
    def _multiclass_nms(boxes, scores, factors, score_thr, nms_cfg, max_num):
        """``multiclass_nms(..., score_factors=)`` (core/post_processing/bbox_nms.py:5-68) of B images with N rows each:
        boxes [B, N, 4], scores [B, N, C], factors [B, N].  The candidates (score > score_thr, scored score * factor) of an
        image in stable descending order are the head of a stable sort of all its N C products with the others at -inf; the
        K = min(N C, NMS_CANDIDATE_CAP) first are the image's segment of ``ops.nms_segmented``.  The entries behind the
        candidates can neither suppress one (they come later) nor count (dropped from the kept list, of which they are the
        tail).  ``batched_nms``'s class offsets use the image's own largest candidate coordinate."""
        B, N, C = scores.shape
        M = N * C
        dev = boxes.device
        cfg = dict(nms_cfg)
        cfg.pop('type', 'nms')
        class_agnostic = cfg.pop('class_agnostic', False)
        thr = cfg.get('iou_threshold', cfg.get('iou_thr', 0.5))
        valid = (scores > score_thr).reshape(B, M)
        prod = (scores * factors[:, :, None]).reshape(B, M)
        vcount = valid.sum(1)
        order_all = torch.sort(torch.where(valid, prod, prod.new_full((), float('-inf'))), dim=1, descending=True, stable=True)[1]
        K = max(min(M, NMS_CANDIDATE_CAP), 1)
        while True:
            order = order_all[:, :K]
            row, cls = torch.div(order, C, rounding_mode='floor'), order % C
            bx = boxes.gather(1, row[:, :, None].expand(-1, -1, 4))
            sc = prod.gather(1, order)
            pos = torch.arange(K, device=dev)[None]
            if class_agnostic:
                bn = bx
            else:
                live = (pos < vcount[:, None])[:, :, None]
                mx = torch.where(live, bx, bx.new_full((), float('-inf'))).amax((1, 2))
                mx = torch.where(vcount > 0, mx, torch.zeros_like(mx))
                bn = bx + (cls.to(bx) * (mx + 1)[:, None])[:, :, None]
            keep, kept = ops.nms_segmented(bn.reshape(B * K, 4).contiguous(), [K] * B, thr, max_num=max_num)
            keep = keep.view(B, K).long()
            n = ((pos < kept[:, None]) & (keep < vcount[:, None])).sum(1)
            n, most = torch.stack([n, vcount]).cpu().tolist()                # the call's one host wait
            if max(most) <= K:
                break
            K = min(M, 1 << (max(most) - 1).bit_length())                    # (an image outgrew the cap: once more, wider)
        out = []
        for b in range(B):
            g = keep[b, :n[b]]
            out.append((torch.cat([bx[b, g], sc[b, g][:, None]], 1), cls[b, g]))
        return out
