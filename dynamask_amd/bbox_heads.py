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
-- ``BasicResBlock``, ResNet ``Bottleneck``s with eval-mode BatchNorm folded into the exact-fp32 convolutions (``fold_bn``),
a global average pool (``dm_global_avg_pool_fwd``) -- the classification from fully connected layers.
``BBoxHead`` (roi_heads/bbox_heads/bbox_head.py, inference): the two fully connected layers alone, behind the average pool in
the C4 configs; its ``Bottleneck`` sibling with a ``downsample`` path is the first block of shared_heads.ResLayer."""
import numpy as np
import torch
import torch.nn as nn

from . import hazard, ops
from .registry import HEADS, Registry, build_from_cfg

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


class _FC(nn.Module):
    """nn.Linear parameters; the product runs on the fp32 MFMA FC kernel (dm_fc_fwd)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.in_features, self.out_features = cin, cout
        self.weight = nn.Parameter(torch.empty(cout, cin))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.xavier_uniform_(self.weight)
        from .mask_heads import _Packed
        self._pk = _Packed()      # transposed packed weights of the backward's data-gradient GEMM

    def run(self, x, relu=False):
        return ops.fc(x.contiguous(), self.weight.detach(), self.bias.detach(), relu=relu)


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
        from .registry import build_loss
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
        from .losses import accuracy
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
def fold_bn(pairs):
    """Eval-mode BatchNorm folded into the convolution in front of it: ``pairs`` = [(conv weight [Cout, Cin_i, k, k], bn),
    ...] -> (w' [Cout, sum Cin_i, k, k], b' [Cout]) with, per pair, s = gamma / sqrt(running_var + eps),
    w' = w * s[:, None, None, None], b' = beta - running_mean * s.  Several pairs are the summed outputs of convolutions
    of different inputs as ONE convolution of their concatenation: the weights side by side along Cin, the biases added.
    All of it in float64, rounded once to float32."""
    ws, b = [], None
    for w, bn in pairs:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        ws.append(w.detach().double() * s[:, None, None, None])
        bi = bn.bias.detach().double() - bn.running_mean.detach().double() * s
        b = bi if b is None else b + bi
    return torch.cat(ws, 1).float().contiguous(), b.float().contiguous()


class _FoldedConv:
    """Packed folded weights + bias of one launch, cached like ``_Packed`` caches packed weights: made again when any of
    the convolution weights, BatchNorm parameters or running statistics changes (``load_state_dict`` copies in place and
    moves their versions; a move to another device changes their addresses)."""

    def __init__(self, pairs, src_channels):
        from .mask_heads import _Packed
        self.modules, self.src_channels = pairs, list(src_channels)      # [(convolution holder, BatchNorm holder), ...]
        self._pk = _Packed()

    def _pairs(self):
        return [(conv.weight, bn) for conv, bn in self.modules]

    def _tensors(self):
        return [t for w, bn in self._pairs() for t in (w, bn.weight, bn.bias, bn.running_mean, bn.running_var)]

    def folded(self):
        """(w', b') in torch's layout, on the parameters' device (CPU included)."""
        return self._pk.get_multi('fold', self._tensors(), lambda: fold_bn(self._pairs()))

    def packed(self):
        """(packed w', b') for ops.conv2d: always the exact fp32 layout, whatever the precision mode."""
        def make():
            w, b = self.folded()
            return ops.pack_conv_weight(w, src_channels=self.src_channels), b
        return self._pk.get_multi('pack', self._tensors(), make)


def _conv_weight(cout, cin, k):
    """nn.Conv2d(bias=False) parameter holder: the key is ``weight`` alone."""
    from .mask_heads import _Conv
    return _Conv(cin, cout, k, bias=False)


class BNConvModule(nn.Module):
    """mmcv ConvModule(bias=False, norm_cfg=dict(type='BN')): keys ``conv.weight``, ``bn.*``.  A parameter holder: the
    block that owns it folds the BatchNorm and launches."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        from .roi_head import _BN
        self.conv = _conv_weight(out_channels, in_channels, kernel_size)
        self.bn = _BN(out_channels)


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


class Bottleneck(nn.Module):
    """backbones/resnet.py:95-300 (stride 1, no downsample, style 'pytorch') in eval mode; keys ``conv{1,2,3}.weight``,
    ``bn{1,2,3}.*``.  Three launches: 1x1 + ReLU, 3x3 + ReLU, then the 1x1 back to ``inplanes`` with the ``accumulate |
    ReLU`` epilogue -- relu(x + conv + bias), the residual sum before the activation -- written IN PLACE into ``x``.
    ``downsample=True`` (the first block of a ResNet layer, shared_heads.ResLayer): the identity path is
    ``downsample.0`` (1x1, ``inplanes`` -> 4 ``planes``) + ``downsample.1`` (BatchNorm), and the block is three launches
    too -- conv1, conv2, then ONE two-source 1x1 of [conv2 output, x] by [W3' | Wd'] with bias b3' + bd' and ReLU (the
    BasicResBlock pattern) into a NEW tensor: ``x`` is not written.  A stride (style 'caffe': in conv1 and
    ``downsample.0``, both 1x1) is the caller's subsampling of ``x``.

    The backbone's arguments (backbones.ResNet; the defaults are the block above).  ``stride=2`` (with ``downsample``):
    style 'caffe' runs the block on ``ops.subsample2(x)``; style 'pytorch' runs conv1 at full size, conv2 through
    ``ops.conv3x3_s2`` (one workgroup per tile walks all of K: ``splits=1``) and closes with the two-source 1x1 of
    [conv2 output, ``ops.subsample2(x)``].  ``wide_from``: a width above which the stride-1 conv2 runs on
    ``ops.conv3x3_dil`` (dilation 1, any width, the same packed weights) instead of ``ops.conv2d``."""
    expansion = 4

    def __init__(self, inplanes, planes, downsample=False, stride=1, style='pytorch', wide_from=None):
        super().__init__()
        from .roi_head import _BN
        if not downsample and inplanes != planes * self.expansion:
            raise NotImplementedError('Bottleneck: no downsample path (DoubleConvFCBBoxHead: planes = inplanes / 4)')
        if stride not in (1, 2) or style not in ('pytorch', 'caffe') or (stride == 2 and not downsample):
            raise NotImplementedError(f'Bottleneck: stride={stride}, style={style!r}, downsample={downsample}; stride 1, or '
                                      "stride 2 with a downsample path, in style 'pytorch' or 'caffe' are built")
        self.stride, self.style, self.wide_from = stride, style, wide_from
        self.inplanes, self.planes = inplanes, planes
        out = planes * self.expansion
        self.conv1, self.bn1 = _conv_weight(planes, inplanes, 1), _BN(planes)
        self.conv2, self.bn2 = _conv_weight(planes, planes, 3), _BN(planes)
        self.conv3, self.bn3 = _conv_weight(out, planes, 1), _BN(out)
        self._f = [_FoldedConv([(c, bn)], [c.in_channels]) for c, bn in ((self.conv1, self.bn1), (self.conv2, self.bn2))]
        if downsample:
            self.downsample = nn.Sequential(_conv_weight(out, inplanes, 1), _BN(out))
            self._f.append(_FoldedConv([(self.conv3, self.bn3), (self.downsample[0], self.downsample[1])], [planes, inplanes]))
        else:
            self.downsample = None
            self._f.append(_FoldedConv([(self.conv3, self.bn3)], [planes]))

    def forward(self, x):
        """Without ``downsample``: ``x`` [N, inplanes, H, W] is overwritten with the block's output and returned.  With
        it: a new [N, 4 planes, H, W] tensor."""
        (w1, b1), (w2, b2), (w3, b3) = (f.packed() for f in self._f)
        if self.stride == 2 and self.style == 'caffe':
            x = ops.subsample2(x)
        h = ops.conv2d(x, w1, b1, self.planes, 1, relu=True)
        if self.stride == 2 and self.style == 'pytorch':
            h = ops.conv3x3_s2(h, w2, b2, self.planes, relu=True, splits=1)
            x = ops.subsample2(x)
        elif self.wide_from is not None and h.shape[3] > self.wide_from:
            h = ops.conv3x3_dil(h, w2, b2, self.planes, 1, relu=True)
        else:
            h = ops.conv2d(h, w2, b2, self.planes, 3, relu=True)
        if self.downsample is not None:
            return ops.conv2d([h, x], w3, b3, self.planes * self.expansion, 1, relu=True)
        return ops.conv2d(h, w3, b3, self.inplanes, 1, relu=True, out=x, accumulate=True)


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
        from .registry import build_loss
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
        from .registry import build_loss
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
        from . import hazard
        hazard.engine_handoff(g_cls, g_reg)
        n = acts[0].shape[0]
        pg = {}

        def fc_bwd(fc, gy, xin, need_data=True, out=None, accumulate=False):
            from .train_path import params_grad
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
        from .train_path import _join_caller_after_backward
        _join_caller_after_backward(acts[0].device)
        return (None, g_x, *[pg.get(p) for p in head.parameters()])


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv.ops.nms.batched_nms (mmcv 1.0.5): boxes of different classes are moved apart by
    (max coordinate + 1) * class so that one NMS handles all classes."""
    cfg = dict(nms_cfg)
    cfg.pop('type', 'nms')
    class_agnostic = cfg.pop('class_agnostic', class_agnostic)
    if class_agnostic:
        boxes_for_nms = boxes
    else:
        max_coordinate = boxes.max()
        offsets = idxs.to(boxes) * (max_coordinate + 1)
        boxes_for_nms = boxes + offsets[:, None]
    dets, keep = ops.nms(boxes_for_nms.contiguous(), scores.contiguous(), cfg.get('iou_threshold', cfg.get('iou_thr', 0.5)))
    return torch.cat([boxes[keep], dets[:, -1:]], 1), keep


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None):
    """core/post_processing/bbox_nms.py:5-68 -> (dets [k, 5], labels [k]), labels 0-based; the
    last score column (background) is ignored."""
    n, ncls = multi_scores.shape[0], multi_scores.shape[1] - 1
    fg = multi_scores[:, :ncls]
    cand = (fg > score_thr).nonzero(as_tuple=False)          # row-major: the reference's masked_select order
    if cand.shape[0] == 0:
        return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
    ri, ci = cand[:, 0], cand[:, 1]
    per_class = multi_bboxes.view(n, -1, 4)
    boxes = per_class[ri, ci] if per_class.shape[1] > 1 else per_class[ri, 0]
    scores = fg[ri, ci] if score_factors is None else (fg * score_factors[:, None])[ri, ci]
    dets, keep = batched_nms(boxes, scores, ci, nms_cfg)
    if max_num > 0:
        dets, keep = dets[:max_num], keep[:max_num]
    return dets, ci[keep]


def multiclass_nms_batch(multi_bboxes_list, multi_scores_list, score_thr, nms_cfg, max_num=-1):
    """``multiclass_nms`` of B images at once -> list of B (dets [k, 5], labels [k]), each what ``multiclass_nms`` gives
    for that image alone, bit for bit.  The score cut runs on all images' rows together; every image is one segment of
    ``ops.nms_segmented`` (suppression bits only within the image, greedy pass on the device, ``max_num`` per image).
    ``batched_nms``'s class offsets use each image's OWN largest coordinate, as the per-image call does.  Host waits: the
    candidate count, the per-image candidate counts and the per-image kept counts -- three, whatever B is."""
    B = len(multi_scores_list)
    assert len(multi_bboxes_list) == B
    if B == 0:
        return []
    ref = multi_bboxes_list[0]
    empty = lambda: (ref.new_zeros((0, 5)), ref.new_zeros((0,), dtype=torch.long))      # noqa: E731
    rows = [int(s.shape[0]) for s in multi_scores_list]
    if sum(rows) == 0:
        return [empty() for _ in range(B)]
    scores_all = torch.cat([s for s in multi_scores_list if s.shape[0] > 0], 0)
    ncls = scores_all.shape[1] - 1
    bboxes_all = torch.cat([b.reshape(b.shape[0], -1) for b in multi_bboxes_list if b.shape[0] > 0], 0)
    n = scores_all.shape[0]
    fg = scores_all[:, :ncls]
    cand = (fg > score_thr).nonzero(as_tuple=False)          # row-major: image after image, the per-image order in each
    if cand.shape[0] == 0:
        return [empty() for _ in range(B)]
    ri, ci = cand[:, 0], cand[:, 1]
    per_class = bboxes_all.view(n, -1, 4)
    boxes = per_class[ri, ci] if per_class.shape[1] > 1 else per_class[ri, 0]
    scores = fg[ri, ci]
    row_start = ops._upload([sum(rows[:b + 1]) for b in range(B)], torch.int64, ref.device)
    img = torch.searchsorted(row_start, ri, right=True)       # image of every candidate
    counts = torch.bincount(img, minlength=B).cpu().tolist()
    cfg = dict(nms_cfg)
    cfg.pop('type', 'nms')
    class_agnostic = cfg.pop('class_agnostic', False)
    if class_agnostic:
        boxes_for_nms = boxes
    else:
        # batched_nms: boxes.max() of the image's own candidates, the same fp32 operations in the same order
        seg_max = torch.full((B,), float('-inf'), device=boxes.device, dtype=boxes.dtype)
        seg_max = seg_max.scatter_reduce(0, img, boxes.amax(1), 'amax')
        offsets = ci.to(boxes) * (seg_max + 1)[img]
        boxes_for_nms = boxes + offsets[:, None]
    # per-image stable descending sort == stable descending sort of all, then a stable sort by image
    o1 = torch.sort(scores, descending=True, stable=True)[1]
    order = o1[torch.sort(img[o1], stable=True)[1]]
    sb = boxes_for_nms[order].contiguous()
    keep, kept = ops.nms_segmented(sb, counts, cfg.get('iou_threshold', cfg.get('iou_thr', 0.5)), max_num=max_num)
    kept = kept.cpu().tolist()
    out, start = [], 0
    for b in range(B):
        k = kept[b]
        if k == 0:
            out.append(empty())
        else:
            g = order[keep[start:start + k].long() + start]
            out.append((torch.cat([boxes[g], scores[g][:, None]], 1), ci[g]))
        start += counts[b]
    return out


def bbox2result(bboxes, labels, num_classes):
    """core/bbox/transforms.py:76-96."""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    bboxes = bboxes.cpu().numpy()
    labels = labels.cpu().numpy()
    return [bboxes[labels == i, :] for i in range(num_classes)]
