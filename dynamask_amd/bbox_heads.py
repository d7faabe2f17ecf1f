"""Bbox branch of the RoI head at inference: the reference's
``Shared2FCBBoxHead`` (roi_heads/bbox_heads/convfc_bbox_head.py:9-205, bbox_head.py:13-217),
``DeltaXYWHBBoxCoder`` (core/bbox/coder/delta_xywh_bbox_coder.py) and ``multiclass_nms``
(core/post_processing/bbox_nms.py) under their registry names, kwargs and ``state_dict`` keys.

The 7x7 RoI extraction is the same HIP kernel as the mask branch's; softmax + box decoding and
the NMS suppression matrix are HIP kernels (``dm_bbox_decode``, ``dm_nms_mask``); the four fully
connected layers run on ``dm_fc_fwd`` (fp32 MFMA GEMM with split-K over the long 12544 axis).
Training (second half): ``get_targets`` (bbox2delta = ``dm_bbox_encode``),
``loss`` (softmax CE + accuracy = ``dm_softmax_ce_fwd_bwd``, L1 on the positive rows' class
columns = ``dm_l1_loss_fwd_bwd``) and the backward of the FC stack (``BBoxHeadFn``: data and
weight gradients as fp32-MFMA GEMMs through the implicit-GEMM kernels on [N, C, 1, 1] tensors).
``DoubleConvFCBBoxHead`` (roi_heads/bbox_heads/double_bbox_head.py, inference): the regression from a convolution branch
-- ``BasicResBlock``, ``layers.Bottleneck``s with eval-mode BatchNorm folded into the exact-fp32 convolutions (``layers.fold_bn``),
a global average pool (``dm_global_avg_pool_fwd``) -- the classification from fully connected layers.
``BBoxHead`` (roi_heads/bbox_heads/bbox_head.py, inference): the two fully connected layers alone, behind the average pool in
the C4 configs; its ``Bottleneck`` sibling with a ``downsample`` path is the first block of shared_heads.ResLayer."""
import numpy as np
import torch
import torch.nn as nn

from . import hazard, ops
from .layers import _FC, BNConvModule, Bottleneck, _FoldedConv
from .losses import accuracy
from .postprocess import multiclass_nms
from .registry import HEADS, Registry, build_from_cfg, build_loss
from .train_path import _join_caller_after_backward, params_grad

BBOX_CODERS = Registry('bbox_coder')


def build_bbox_coder(cfg, **default_args):
    return build_from_cfg(cfg, BBOX_CODERS, default_args)


@BBOX_CODERS.register_module()
class DeltaXYWHBBoxCoder:
    """core/bbox/coder/delta_xywh_bbox_coder.py:9-60."""

    def __init__(self, target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.)):
        self.means = tuple(target_means)
        self.stds = tuple(target_stds)

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        assert pred_bboxes.size(0) == bboxes.size(0)
        nb = pred_bboxes.size(1) // 4
        out, _ = ops.bbox_decode(bboxes.contiguous(), None, pred_bboxes.contiguous(), nb, self.means, self.stds,
                                 wh_ratio_clip, max_shape)
        return out

    def encode(self, bboxes, gt_bboxes):
        """delta_xywh_bbox_coder.py:33-50 -> bbox2delta."""
        assert bboxes.size(0) == gt_bboxes.size(0)
        assert bboxes.size(-1) == gt_bboxes.size(-1) == 4
        return ops.bbox_encode(bboxes.float().contiguous(), gt_bboxes.float().contiguous(), self.means, self.stds)


@HEADS.register_module()
class Shared2FCBBoxHead(nn.Module):
    """convfc_bbox_head.py:189-205 (= ConvFCBBoxHead with 2 shared FCs) on top of BBoxHead
    (bbox_head.py:13-60).  ``state_dict`` keys: shared_fcs.{0,1}.{weight,bias}, fc_cls.*, fc_reg.*."""

    def __init__(self, fc_out_channels=1024, with_avg_pool=False, with_cls=True, with_reg=True, roi_feat_size=7,
                 in_channels=256, num_classes=80, bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.],
                                                                  target_stds=[0.1, 0.1, 0.2, 0.2]),
                 reg_class_agnostic=False, reg_decoded_bbox=False, loss_cls=None, loss_bbox=None,
                 conv_out_channels=256, conv_cfg=None, norm_cfg=None):
        super().__init__()
        if with_avg_pool or not with_cls or conv_cfg is not None or norm_cfg is not None:
            raise NotImplementedError('configs/dynamask use the plain Shared2FCBBoxHead')
        # with_reg=False (configs/grid_rcnn: the grid head regresses the box): no fc_reg, forward gives (cls_score, None),
        # get_bboxes returns the clipped RoIs (bbox_head.py:205-212)
        self.with_reg = with_reg
        self.roi_feat_size = (roi_feat_size, roi_feat_size) if isinstance(roi_feat_size, int) else tuple(roi_feat_size)
        self.roi_feat_area = self.roi_feat_size[0] * self.roi_feat_size[1]
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.reg_class_agnostic = reg_class_agnostic
        self.fc_out_channels = fc_out_channels
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.reg_decoded_bbox = reg_decoded_bbox
        if reg_decoded_bbox:
            raise NotImplementedError('reg_decoded_bbox=False in configs/dynamask')
        self.loss_cls_cfg, self.loss_bbox_cfg = loss_cls, loss_bbox
        # bbox_head.py:47-48 (no parameters; built when configured so that inference-only configs stay light)
        self.loss_cls = build_loss(loss_cls) if loss_cls is not None else None
        self.loss_bbox = build_loss(loss_bbox) if loss_bbox is not None else None
        self.shared_fcs = nn.ModuleList([_FC(in_channels * self.roi_feat_area, fc_out_channels),
                                         _FC(fc_out_channels, fc_out_channels)])
        self.fc_cls = _FC(fc_out_channels, num_classes + 1)
        if with_reg:
            self.fc_reg = _FC(fc_out_channels, 4 if reg_class_agnostic else 4 * num_classes)

    def init_weights(self):
        """bbox_head.py:62-70 + convfc_bbox_head.py:128-136."""
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.constant_(self.fc_cls.bias, 0)
        if self.with_reg:
            nn.init.normal_(self.fc_reg.weight, 0, 0.001)
            nn.init.constant_(self.fc_reg.bias, 0)
        for fc in self.shared_fcs:
            nn.init.xavier_uniform_(fc.weight)
            nn.init.constant_(fc.bias, 0)

    def forward(self, x):
        """convfc_bbox_head.py:138-186 for the Shared2FC configuration."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if not self.with_reg:
                raise NotImplementedError('Shared2FCBBoxHead(with_reg=False): the training path (BBoxHeadFn) has both '
                                          'branches; Grid R-CNN is inference only (run under torch.no_grad())')
            return BBoxHeadFn.apply(self, x, *list(self.parameters()))
        x = x.flatten(1)
        for fc in self.shared_fcs:
            x = fc.run(x, relu=True)
        return self.fc_cls.run(x), (self.fc_reg.run(x) if self.with_reg else None)

    # ------------------------------------------------------------------ training
    def _get_target_single(self, pos_bboxes, neg_bboxes, pos_gt_bboxes, pos_gt_labels, cfg):
        """bbox_head.py:85-116."""
        num_pos, num_neg = pos_bboxes.size(0), neg_bboxes.size(0)
        num_samples = num_pos + num_neg
        labels = pos_bboxes.new_full((num_samples,), self.num_classes, dtype=torch.long)
        label_weights = pos_bboxes.new_zeros(num_samples)
        bbox_targets = pos_bboxes.new_zeros(num_samples, 4)
        bbox_weights = pos_bboxes.new_zeros(num_samples, 4)
        if num_pos > 0:
            labels[:num_pos] = pos_gt_labels
            pos_weight = 1.0 if cfg.pos_weight <= 0 else cfg.pos_weight
            label_weights[:num_pos] = pos_weight
            bbox_targets[:num_pos, :] = self.bbox_coder.encode(pos_bboxes, pos_gt_bboxes)
            bbox_weights[:num_pos, :] = 1
        if num_neg > 0:
            label_weights[-num_neg:] = 1.0
        return labels, label_weights, bbox_targets, bbox_weights

    def get_targets(self, sampling_results, gt_bboxes, gt_labels, rcnn_train_cfg, concat=True):
        """bbox_head.py:118-141."""
        outs = [self._get_target_single(r.pos_bboxes, r.neg_bboxes, r.pos_gt_bboxes, r.pos_gt_labels, rcnn_train_cfg)
                for r in sampling_results]
        labels, label_weights, bbox_targets, bbox_weights = (list(t) for t in zip(*outs))
        if concat:
            labels = torch.cat(labels, 0)
            label_weights = torch.cat(label_weights, 0)
            bbox_targets = torch.cat(bbox_targets, 0)
            bbox_weights = torch.cat(bbox_weights, 0)
            # every sampled row carries a weight > 0 (_get_target_single: pos_weight, made 1 when <= 0, for positives; 1 for
            # negatives): the count the classification loss normalises by is the row count, known on the host -- ``loss``
            # below takes it from here instead of reading it back from the device (a host sync per step)
            label_weights._dm_num_weighted = int(label_weights.shape[0])
        return labels, label_weights, bbox_targets, bbox_weights

    def loss(self, cls_score, bbox_pred, rois, labels, label_weights, bbox_targets, bbox_weights, reduction_override=None):
        """bbox_head.py:143-184 -> {'loss_cls', 'acc', 'loss_bbox'}."""
        losses = dict()
        if cls_score is not None:
            known = getattr(label_weights, '_dm_num_weighted', None)      # set by get_targets: all of its rows are weighted
            avg_factor = max(float(known) if known is not None else torch.sum(label_weights > 0).float().item(), 1.)
            if cls_score.numel() > 0:
                losses['loss_cls'] = self.loss_cls(cls_score, labels, label_weights, avg_factor=avg_factor,
                                                   reduction_override=reduction_override)
                losses['acc'] = accuracy(cls_score, labels)
        if bbox_pred is not None and bbox_pred.shape[0] == 0:
            losses['loss_bbox'] = bbox_pred.sum() * 0            # no sampled RoI at all (bbox_head.py:181-182)
        elif bbox_pred is not None:
            # the reference gathers bbox_pred[pos, labels[pos]] and calls loss_bbox on the gathered rows
            # (avg_factor = number of samples); rows with a background label contribute nothing, and
            # with no positive row the loss is `bbox_pred.sum() * 0`: both are what the fused kernel gives
            losses['loss_bbox'] = self.loss_bbox.forward_pos(bbox_pred, labels, bbox_targets, bbox_weights,
                                                             self.num_classes, avg_factor=bbox_targets.size(0),
                                                             reduction_override=reduction_override)
        return losses

    def get_bboxes(self, rois, cls_score, bbox_pred, img_shape, scale_factor, rescale=False, cfg=None):
        """bbox_head.py:186-223."""
        if isinstance(cls_score, list):
            cls_score = sum(cls_score) / float(len(cls_score))
        scale = (1.0, 1.0)
        if rescale:
            if isinstance(scale_factor, float):
                scale = (scale_factor, scale_factor)
            else:
                sf = [float(v) for v in np.asarray(scale_factor).reshape(-1)]
                scale = (sf[0], sf[1])
                assert len(sf) == 4 and sf[2] == sf[0] and sf[3] == sf[1], 'scale_factor is [w, h, w, h]'
        coder = self.bbox_coder
        bboxes, scores = ops.bbox_decode(rois.contiguous(), None if cls_score is None else cls_score.contiguous(),
                                         None if bbox_pred is None else bbox_pred.contiguous(), self.num_classes,
                                         coder.means, coder.stds, 16 / 1000, img_shape, scale,
                                         class_agnostic=self.reg_class_agnostic or bbox_pred is None)
        if cfg is None:
            return bboxes, scores
        return multiclass_nms(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img)


# ---------------------------------------------------------------- Double-Head R-CNN (bbox_heads/double_bbox_head.py)
class BasicResBlock(nn.Module):
    """double_bbox_head.py:9-68 in eval mode: relu(bn(conv2(relu(bn(conv1 3x3(x))))) + bn(conv_identity(x))) as two
    launches -- conv1 + ReLU, then ONE two-source 1x1 convolution of [conv1 output, x] by [W2' | Wid'] with bias
    b2' + bid' and ReLU."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv1 = BNConvModule(in_channels, in_channels, 3)
        self.conv2 = BNConvModule(in_channels, out_channels, 1)
        self.conv_identity = BNConvModule(in_channels, out_channels, 1)
        self._f1 = _FoldedConv([(self.conv1.conv, self.conv1.bn)], [in_channels])
        self._f2 = _FoldedConv([(self.conv2.conv, self.conv2.bn), (self.conv_identity.conv, self.conv_identity.bn)],
                               [in_channels, in_channels])

    def forward(self, x):
        w1, b1 = self._f1.packed()
        h = ops.conv2d(x, w1, b1, self.in_channels, 3, relu=True)
        w2, b2 = self._f2.packed()
        return ops.conv2d([h, x], w2, b2, self.out_channels, 1, relu=True)


@HEADS.register_module()
class DoubleConvFCBBoxHead(nn.Module):
    """``DoubleConvFCBBoxHead`` -- bbox_heads/double_bbox_head.py:71-172 on BBoxHead (bbox_head.py:13-60), inference: the
    regression from a convolution branch (BasicResBlock, ``num_convs`` Bottlenecks, global average pool, ``fc_reg``) on the
    RoI features of the enlarged box, the classification from ``num_fcs`` fully connected layers on the plain ones.
    ``state_dict`` keys as the reference's.  BatchNorm runs in eval mode, folded into the convolutions (``fold_bn``); every
    launch is exact fp32 in every precision mode.  Training is not built."""

    def __init__(self, num_convs=0, num_fcs=0, conv_out_channels=1024, fc_out_channels=1024, conv_cfg=None,
                 norm_cfg=dict(type='BN'), with_avg_pool=True, with_cls=True, with_reg=True, roi_feat_size=7, in_channels=256,
                 num_classes=80, bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.],
                                                 target_stds=[0.1, 0.1, 0.2, 0.2]),
                 reg_class_agnostic=False, reg_decoded_bbox=False, loss_cls=None, loss_bbox=None):
        super().__init__()
        assert with_avg_pool
        assert num_convs > 0
        assert num_fcs > 0
        assert with_cls or with_reg           # (bbox_head.py:29; both branches are built whatever the flags say, as there)
        if conv_cfg is not None:
            raise NotImplementedError('DoubleConvFCBBoxHead: conv_cfg is None in configs/double_heads')
        if not isinstance(norm_cfg, dict) or norm_cfg.get('type') != 'BN' or set(norm_cfg) - {'type', 'requires_grad'}:
            raise NotImplementedError("DoubleConvFCBBoxHead: norm_cfg is dict(type='BN') in configs/double_heads (the "
                                      'eval-mode fold is BatchNorm\'s)')
        if reg_decoded_bbox:
            raise NotImplementedError('reg_decoded_bbox=False in configs/double_heads')
        if conv_out_channels % 4 != 0:
            raise ValueError('conv_out_channels must be a multiple of 4 (Bottleneck planes = conv_out_channels / 4)')
        self.with_avg_pool, self.with_cls, self.with_reg = True, with_cls, with_reg
        self.roi_feat_size = (roi_feat_size, roi_feat_size) if isinstance(roi_feat_size, int) else tuple(roi_feat_size)
        self.roi_feat_area = self.roi_feat_size[0] * self.roi_feat_size[1]
        self.in_channels, self.num_classes, self.reg_class_agnostic = in_channels, num_classes, reg_class_agnostic
        self.num_convs, self.num_fcs = num_convs, num_fcs
        self.conv_out_channels, self.fc_out_channels = conv_out_channels, fc_out_channels
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.reg_decoded_bbox = reg_decoded_bbox
        self.loss_cls_cfg, self.loss_bbox_cfg = loss_cls, loss_bbox
        self.loss_cls = build_loss(loss_cls) if loss_cls is not None else None
        self.loss_bbox = build_loss(loss_bbox) if loss_bbox is not None else None
        self.res_block = BasicResBlock(in_channels, conv_out_channels)
        self.conv_branch = nn.ModuleList([Bottleneck(conv_out_channels, conv_out_channels // 4) for _ in range(num_convs)])
        self.fc_branch = nn.ModuleList([_FC(in_channels * self.roi_feat_area if i == 0 else fc_out_channels, fc_out_channels)
                                        for i in range(num_fcs)])
        self.fc_reg = _FC(conv_out_channels, 4 if reg_class_agnostic else 4 * num_classes)
        self.fc_cls = _FC(fc_out_channels, num_classes + 1)

    def init_weights(self):
        """double_bbox_head.py:143-150 (the convolutions keep their constructors' initialisation)."""
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.constant_(self.fc_cls.bias, 0)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.constant_(self.fc_reg.bias, 0)
        for fc in self.fc_branch:
            nn.init.xavier_uniform_(fc.weight)
            nn.init.constant_(fc.bias, 0)

    def conv_features(self, x_reg):
        """res_block + conv_branch + the average pool of double_bbox_head.py:154-162 -> [N, conv_out_channels]."""
        if tuple(x_reg.shape[2:]) != self.roi_feat_size:
            raise ValueError(f'x_reg: {self.roi_feat_size} RoI features expected (AvgPool2d(roi_feat_size) then gives one '
                             f'value per channel), got {tuple(x_reg.shape[2:])}')
        x = self.res_block(x_reg.contiguous())
        for block in self.conv_branch:
            x = block(x)
        return ops.global_avg_pool(x)

    def forward(self, x_cls, x_reg):
        """double_bbox_head.py:152-172 -> (cls_score, bbox_pred)."""
        if torch.is_grad_enabled() and (x_cls.requires_grad or x_reg.requires_grad
                                        or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('DoubleConvFCBBoxHead: training (BatchNorm in train mode, the backward of the conv '
                                      'branch) is not built; run inference under torch.no_grad()')
        if x_cls.shape[0] != x_reg.shape[0]:
            raise ValueError(f'x_cls has {x_cls.shape[0]} RoIs, x_reg {x_reg.shape[0]}')
        if x_cls.shape[0] == 0:         # no RoI: nothing is launched
            return (x_cls.new_zeros((0, self.fc_cls.out_features)), x_cls.new_zeros((0, self.fc_reg.out_features)))
        bbox_pred = self.fc_reg.run(self.conv_features(x_reg))
        x_fc = x_cls.flatten(1)
        for fc in self.fc_branch:
            x_fc = fc.run(x_fc, relu=True)
        return self.fc_cls.run(x_fc), bbox_pred

    # get_bboxes, the targets and the loss are BBoxHead's: the code Shared2FCBBoxHead runs
    get_bboxes = Shared2FCBBoxHead.get_bboxes
    _get_target_single = Shared2FCBBoxHead._get_target_single
    get_targets = Shared2FCBBoxHead.get_targets
    loss = Shared2FCBBoxHead.loss


@HEADS.register_module()
class BBoxHead(nn.Module):
    """``BBoxHead`` -- bbox_heads/bbox_head.py:13-82, inference: the two fully connected layers ``fc_cls`` / ``fc_reg``
    (dm_fc_fwd) on the RoI features, averaged over the RoI first with ``with_avg_pool`` (dm_global_avg_pool_fwd; the C4
    configs, on the shared head's [N, 2048, 7, 7]) or flattened.  ``state_dict`` keys: fc_cls.*, fc_reg.*."""

    def __init__(self, with_avg_pool=False, with_cls=True, with_reg=True, roi_feat_size=7, in_channels=256, num_classes=80,
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2]),
                 reg_class_agnostic=False, reg_decoded_bbox=False, loss_cls=None, loss_bbox=None):
        super().__init__()
        assert with_cls or with_reg
        if reg_decoded_bbox:
            raise NotImplementedError('BBoxHead: reg_decoded_bbox=True is not built (False in the C4 configs)')
        self.with_avg_pool, self.with_cls, self.with_reg = with_avg_pool, with_cls, with_reg
        self.roi_feat_size = (roi_feat_size, roi_feat_size) if isinstance(roi_feat_size, int) else tuple(roi_feat_size)
        self.roi_feat_area = self.roi_feat_size[0] * self.roi_feat_size[1]
        self.in_channels, self.num_classes, self.reg_class_agnostic = in_channels, num_classes, reg_class_agnostic
        self.reg_decoded_bbox = reg_decoded_bbox
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.loss_cls_cfg, self.loss_bbox_cfg = loss_cls, loss_bbox
        self.loss_cls = build_loss(loss_cls) if loss_cls is not None else None
        self.loss_bbox = build_loss(loss_bbox) if loss_bbox is not None else None
        fc_in = in_channels if with_avg_pool else in_channels * self.roi_feat_area
        if with_cls:
            self.fc_cls = _FC(fc_in, num_classes + 1)
        if with_reg:
            self.fc_reg = _FC(fc_in, 4 if reg_class_agnostic else 4 * num_classes)

    def init_weights(self):
        """bbox_head.py:66-73."""
        if self.with_cls:
            nn.init.normal_(self.fc_cls.weight, 0, 0.01)
            nn.init.constant_(self.fc_cls.bias, 0)
        if self.with_reg:
            nn.init.normal_(self.fc_reg.weight, 0, 0.001)
            nn.init.constant_(self.fc_reg.bias, 0)

    def forward(self, x):
        """bbox_head.py:75-82 -> (cls_score or None, bbox_pred or None)."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('BBoxHead: training is not built; run inference under torch.no_grad()')
        if self.with_avg_pool and tuple(x.shape[2:]) != self.roi_feat_size:
            raise ValueError(f'x: {self.roi_feat_size} RoI features expected (AvgPool2d(roi_feat_size) then gives one value '
                             f'per channel), got {tuple(x.shape[2:])}')
        n = x.shape[0]
        if n == 0:          # no RoI: nothing is launched
            return (x.new_zeros((0, self.fc_cls.out_features)) if self.with_cls else None,
                    x.new_zeros((0, self.fc_reg.out_features)) if self.with_reg else None)
        x = ops.global_avg_pool(x.contiguous()) if self.with_avg_pool else x.flatten(1)
        return (self.fc_cls.run(x) if self.with_cls else None), (self.fc_reg.run(x) if self.with_reg else None)

    # get_bboxes, the targets and the loss are the shared code, as DoubleConvFCBBoxHead takes them
    get_bboxes = Shared2FCBBoxHead.get_bboxes
    _get_target_single = Shared2FCBBoxHead._get_target_single
    get_targets = Shared2FCBBoxHead.get_targets
    loss = Shared2FCBBoxHead.loss


class BBoxHeadFn(torch.autograd.Function):
    """Shared2FCBBoxHead.forward with a hand-sequenced backward.  Inputs: (head, bbox_feats
    [N, C, 7, 7], *head.parameters()); outputs (cls_score, bbox_pred).  nn.Linear's three
    products -- y = x W^T, dx = dy W, dW = dy^T x -- are the forward FC kernel and, for the
    gradients, the implicit-GEMM conv kernels on [N, C, 1, 1] tensors (one "pixel" per sample)."""

    @staticmethod
    def forward(ctx, head, x, *params):
        n = x.shape[0]
        flat = x.detach().reshape(n, -1).contiguous()
        acts = [flat]
        for fc in head.shared_fcs:
            acts.append(fc.run(acts[-1], relu=True))
        cls_score, bbox_pred = head.fc_cls.run(acts[-1]), head.fc_reg.run(acts[-1])
        ctx.head, ctx.acts, ctx.x_shape, ctx.need_x = head, acts, tuple(x.shape), x.requires_grad
        return cls_score, bbox_pred

    @staticmethod
    @hazard.backward_node
    def backward(ctx, g_cls, g_reg):
        head, acts = ctx.head, ctx.acts
        hazard.engine_handoff(g_cls, g_reg)
        n = acts[0].shape[0]
        pg = {}

        def fc_bwd(fc, gy, xin, need_data=True, out=None, accumulate=False):
            gy4 = gy.contiguous().view(n, fc.out_features, 1, 1)
            x4 = xin.view(n, fc.in_features, 1, 1)
            params_grad(fc.weight, fc.bias, gy4, x4, 1, pg, (fc.out_features, fc.in_features, 1, 1))
            if not need_data:
                return None
            wq = fc._pk.get('flip', fc.weight, lambda t: ops.pack_conv_weight(
                t.view(fc.out_features, fc.in_features, 1, 1), transpose_flip=True))
            return ops.conv2d(gy4, wq, None, fc.in_features, 1, out=out, accumulate=accumulate)

        h = acts[-1]
        g_h = None
        for fc, g in ((head.fc_cls, g_cls), (head.fc_reg, g_reg)):
            if g is None:
                continue
            if g_h is None:
                g_h = fc_bwd(fc, g, h)
            else:
                fc_bwd(fc, g, h, out=g_h, accumulate=True)
        g_x = None
        if g_h is not None:
            for i in reversed(range(len(head.shared_fcs))):
                ops.relu_backward_(g_h, acts[i + 1].view_as(g_h))
                need = i > 0 or ctx.need_x
                g_h = fc_bwd(head.shared_fcs[i], g_h, acts[i], need_data=need)
            if ctx.need_x:
                g_x = g_h.reshape(ctx.x_shape)
        _join_caller_after_backward(acts[0].device)
        return (None, g_x, *[pg.get(p) for p in head.parameters()])
