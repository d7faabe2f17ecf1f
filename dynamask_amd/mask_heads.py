"""Mask heads behind the reference's HEADS registry.

``DynaMaskHead`` / ``SFMStage`` mirror
``mmdet/models/roi_heads/mask_heads/dynamask_head.py:54-244`` and
``FCNMaskHead`` mirrors ``mask_heads/fcn_mask_head.py:19-126``: same
constructor kwargs, same ``forward`` signatures, same ``state_dict`` keys
(SURVEY App. D), so reference checkpoints load.  The arithmetic is entirely in
libdynamask_hip.so; these classes only own parameters and sequence launches:

  * torch.cat never runs: concat sources are walked in the conv kernel's K loop,
    and producers write straight into channel slices of the consumer's input;
  * the 80-class logits conv + gather (dynamask_head.py:110-111) is a per-RoI
    gathered dot product (1/80 of the work);
  * bias, ReLU, sigmoid ride in the producing kernels' epilogues.
"""
import math

import torch
import torch.nn as nn

from . import losses  # noqa: F401  (registers CrossEntropyLoss, GridHead's default loss_grid)
from . import ops
from .layers import CARAFEPack, ConvModule, _Conv, _Packed  # noqa: F401  (layers registers CARAFEPack as the 'carafe' upsample layer)
from .postprocess import _to_host, group_mask_scores, paste_segms, select_label_channel
from .registry import HEADS, UPSAMPLE_LAYERS, build_loss
from .train_path import FCNMaskHeadFn


class DeformConv2dPack(nn.Module):
    """DCNv1 3x3 + its zero-initialised offset conv; keys ``weight``,
    ``conv_offset.weight/bias`` (mmdet/ops/dcn/deform_conv.py:189-275)."""

    def __init__(self, in_channels, out_channels, kernel_size=(3, 3), stride=(1, 1), padding=1, deform_groups=1):
        super().__init__()
        ks = kernel_size if isinstance(kernel_size, int) else kernel_size[0]
        if ks != 3:
            raise NotImplementedError('3x3 DCN only')
        self.in_channels, self.out_channels, self.deform_groups = in_channels, out_channels, deform_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        stdv = 1.0 / math.sqrt(in_channels * 9)
        nn.init.uniform_(self.weight, -stdv, stdv)
        self.conv_offset = _Conv(in_channels, deform_groups * 18, 3)
        nn.init.zeros_(self.conv_offset.weight)
        self._pk = _Packed()

    def forward(self, x, relu=False):
        offset = self.conv_offset.run(x)
        wp = self._pk.get('w', self.weight, ops.pack_conv_weight, job=(False, None, None, None))
        return ops.deform_conv(x, offset, wp, self.out_channels, self.deform_groups, relu=relu)


class SFMStage(nn.Module):
    """dynamask_head.py:54-125."""

    def __init__(self, semantic_in_channel=256, semantic_out_channel=256, instance_in_channel=256,
                 instance_out_channel=256, out_size=14, num_classes=80, semantic_out_stride=4,
                 mask_use_sigmoid=False, upsample_cfg=dict(type='bilinear', scale_factor=2)):
        super().__init__()
        self.semantic_out_stride = semantic_out_stride
        self.mask_use_sigmoid = mask_use_sigmoid
        self.num_classes = num_classes
        self.out_size = out_size
        self.instance_in_channel = instance_in_channel
        self.instance_out_channel = instance_out_channel
        if upsample_cfg.get('type') != 'bilinear' or upsample_cfg.get('scale_factor') != 2:
            raise NotImplementedError('SFMStage upsample is bilinear x2 in configs/dynamask '
                                      '(a carafe cfg cannot be passed unchanged: SURVEY K17)')
        self.semantic_transform_in = _Conv(semantic_in_channel, semantic_out_channel, 1)
        self.spatial_scale = 1.0 / semantic_out_stride
        self.instance_logits = _Conv(instance_in_channel, num_classes, 1)
        self.detail_logits = _Conv(instance_in_channel, num_classes, 1)
        fuse_in_channel = instance_in_channel + semantic_out_channel + 2
        self.fuse_conv = nn.ModuleList([
            _Conv(fuse_in_channel, instance_in_channel, 1),
            DeformConv2dPack(instance_in_channel, instance_in_channel, kernel_size=(3, 3), stride=(1, 1), padding=1,
                             deform_groups=2)])
        self.fuse_transform_out = _Conv(instance_in_channel, instance_out_channel - 2, 1)

    def semantic_map(self, semantic_feat):
        """relu(semantic_transform_in(P_l)) on the whole FPN map (dynamask_head.py:104); it does
        not depend on the RoIs, so RoI chunks running on different streams share it."""
        return self.semantic_transform_in.run(semantic_feat, relu=True)

    def forward(self, instance_feats, semantic_feat, rois, roi_labels, upsample=True, sem=None, pred_out=None):
        return run_steps(self.steps(instance_feats, semantic_feat, rois, roi_labels, upsample, sem, pred_out))

    def steps(self, instance_feats, semantic_feat, rois, roi_labels, upsample=True, sem=None, pred_out=None):
        """``forward`` as a generator that yields after every launch (``run_steps`` exhausts it): a caller that runs
        several RoI chunks on several streams issues their launches in turn (roi_head._mask_forward_infer), so that
        no stream waits for the host -- or for the graph's node order -- to get through another stream's whole chain."""
        n, c, s = instance_feats.shape[0], self.instance_in_channel, self.out_size
        co = self.instance_out_channel
        # instance-wise semantic feats: relu(conv1x1) on the whole FPN map, then point sample
        if sem is None:
            sem = self.semantic_map(semantic_feat)
            yield
        # [fused_feats(co-2) | sigmoid(ip) | sigmoid(dp)] is assembled in place
        tail = torch.empty((n, co, s, s), device=instance_feats.device, dtype=torch.float32)
        nc = self.num_classes
        logit_args = (instance_feats, self.instance_logits.weight.detach().view(nc, c), self.instance_logits.bias.detach(),
                      self.detail_logits.weight.detach().view(nc, c), self.detail_logits.bias.detach(), roi_labels)
        if FUSED_STAGE_HEAD[0] and n > 0:
            # the point sample and the two class-gathered logits share no data: one launch (ops.stage_head, same bits)
            ins_sem, ip, dp = ops.stage_head(sem, rois, s, self.spatial_scale, *logit_args, sig_out=tail, sig_ch_offset=co - 2,
                                             out=pred_out)
            yield
        else:
            ins_sem = ops.point_sample(sem, rois, s, self.spatial_scale)
            yield
            ip, dp = ops.class_logits(*logit_args, sig_out=tail, sig_ch_offset=co - 2, out=pred_out)
            yield
        fused = self.fuse_conv[0].run([instance_feats, ins_sem, tail[:, co - 2:]], relu=True)
        yield
        dcn = self.fuse_conv[1]
        offset = dcn.conv_offset.run(fused)
        yield
        wp = dcn._pk.get('w', dcn.weight, ops.pack_conv_weight, job=(False, None, None, None))
        tout = self.fuse_transform_out
        if (FUSED_DCN_TOUT[0] and not torch.is_grad_enabled() and tout.bias is not None
                and ops.deform_conv_tout_supported(fused, dcn.out_channels, tout.out_channels)):
            # 28 x 28 / 56 x 56 at more than a handful of RoIs: the 1x1 runs on the DCN's accumulators, the DCN output
            # ([N, 64, 56, 56]: 80 MB at 100 RoIs, written once and read once) never exists
            w2t = tout._pk.get('tout', tout.weight, ops.pack_tout_weight)
            ops.deform_conv_tout(fused, offset, wp, dcn.out_channels, dcn.deform_groups, w2t, tout.bias.detach(),
                                 tout.out_channels, tail)
            yield
        else:
            fused = ops.deform_conv(fused, offset, wp, dcn.out_channels, dcn.deform_groups, relu=True)
            yield
            tout.run(fused, relu=True, out=tail, out_ch_offset=0)
            yield
        if upsample:
            tail = ops.upsample2x(tail, align_corners=False, relu=True)
            yield
        return ip, dp, tail


# inference launches fused in round 6 (A/B switches for tools/infer_bench.py and the equality tests; same bits either way)
import os as _os
FUSED_STAGE_HEAD = [_os.environ.get('DM_FUSED_STAGE_HEAD', '1') != '0']      # point sample + class logits: one launch per stage
FUSED_DCN_TOUT = [_os.environ.get('DM_FUSED_DCN_TOUT', '1') != '0']            # DCN + fuse_transform_out: one launch (28^2 / 56^2)
GROUPED_SEMANTIC_MAPS = [_os.environ.get('DM_GROUPED_SEM', '1') != '0']       # the stages' FPN-wide 1x1 convolutions: one launch


def run_steps(gen):
    """Exhaust a ``steps`` generator and hand back what it returns."""
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


@HEADS.register_module()
class DynaMaskHead(nn.Module):
    """dynamask_head.py:128-244."""

    def __init__(self, num_convs_instance=2, num_convs_semantic=4, conv_in_channels_instance=256,
                 conv_in_channels_semantic=256, conv_kernel_size_instance=3, conv_kernel_size_semantic=3,
                 conv_out_channels_instance=256, conv_out_channels_semantic=256, conv_cfg=None, norm_cfg=None,
                 semantic_out_stride=[16, 8, 4], mask_use_sigmoid=False, pre_upsample_last_stage=False,
                 stage_num_classes=[80, 80, 80, 80], stage_sup_size=[14, 28, 56, 112],
                 upsample_cfg=dict(type='bilinear', scale_factor=2),
                 loss_cfg=dict(type='DynaCrossEntropyLoss')):
        super().__init__()
        self.num_convs_instance = num_convs_instance
        self.conv_kernel_size_instance = conv_kernel_size_instance
        self.conv_in_channels_instance = conv_in_channels_instance
        self.conv_out_channels_instance = conv_out_channels_instance
        self.num_convs_semantic = num_convs_semantic
        self.conv_kernel_size_semantic = conv_kernel_size_semantic
        self.conv_in_channels_semantic = conv_in_channels_semantic
        self.conv_out_channels_semantic = conv_out_channels_semantic
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.semantic_out_stride = semantic_out_stride
        self.stage_sup_size = stage_sup_size
        self.stage_num_classes = stage_num_classes
        self.pre_upsample_last_stage = pre_upsample_last_stage

        convs = []
        for i in range(num_convs_instance):
            cin = conv_in_channels_instance if i == 0 else conv_out_channels_instance
            convs.append(ConvModule(cin, conv_out_channels_instance, conv_kernel_size_instance, dilation=1, padding=1))
        self.instance_convs = nn.ModuleList(convs)
        self.loss_func = build_loss(loss_cfg)

        assert len(self.stage_sup_size) > 1
        self.stages = nn.ModuleList()
        out_channel = conv_out_channels_instance
        for idx, out_size in enumerate(self.stage_sup_size[:-1]):
            in_channel = out_channel
            out_channel = in_channel // 2
            self.stages.append(SFMStage(
                semantic_in_channel=conv_out_channels_semantic, semantic_out_channel=in_channel,
                instance_in_channel=in_channel, instance_out_channel=out_channel, out_size=out_size,
                num_classes=self.stage_num_classes[idx], semantic_out_stride=semantic_out_stride[-1],
                mask_use_sigmoid=mask_use_sigmoid, upsample_cfg=upsample_cfg))
        self.final_instance_logits = _Conv(out_channel, self.stage_num_classes[-1], 1)
        self.final_detail_logits = _Conv(out_channel, self.stage_num_classes[-1], 1)

    def init_weights(self):
        for m in [self.final_instance_logits, self.final_detail_logits]:
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)

    def semantic_maps(self, semantic_feats, last_stage=None):
        """Per-stage relu(semantic_transform_in(.)) maps (shared by all RoIs).  Without autograd, two or three of them
        are ONE launch (ops.conv1x1_group: no RoI enters them, and as three launches of 66 / 132 / 525 workgroups they
        headed the inference chain with ~100 us in which most of the chip idles); same bits either way."""
        n = len(self.stages) if last_stage is None else min(last_stage, len(self.stages))
        feats = [semantic_feats[-i - 3] for i in range(n)]
        convs = [self.stages[i].semantic_transform_in for i in range(n)]
        if (GROUPED_SEMANTIC_MAPS[0] and 2 <= n <= 3 and not torch.is_grad_enabled() and all(f.is_contiguous() for f in feats)
                and all(c.bias is not None for c in convs)):
            # (bf16x3 mode: the whole group or none of it, ops.BF16X3_SEMANTIC_GROUP)
            prec = 'bf16x3' if ops.inference_precision() == 'bf16x3' and ops.BF16X3_SEMANTIC_GROUP[0] else 'fp32'
            return ops.conv1x1_group(feats, [c.packed([c.in_channels], prec) for c in convs], [c.bias.detach() for c in convs],
                                     [c.out_channels for c in convs], relu=True)
        return [self.stages[i].semantic_map(feats[i]) for i in range(n)]

    def prepack(self, fused_dcn=None):
        """Refresh the kernel-layout weights of everything ``forward`` launches (except the semantic 1x1 convs, which
        ``semantic_maps`` owns) on the CURRENT stream.  The caches are filled by whoever asks first; a caller that is
        about to fork RoI chunks onto several streams calls this first, so that no stream reads a pack another
        stream is still writing.  ``fused_dcn``: per stage, whether the fused DCN kernel's layout is the one needed
        (default: all).  In the bf16x3 mode (ops.inference_precision) the bf16x3 layout of every convolution is made too:
        which of the two a chain asks for depends on the map size (ops.BF16X3_ROUTES), and both exist before the fork."""
        for conv in self.instance_convs:
            conv.conv.packed([conv.conv.in_channels])
            if ops.inference_precision() == 'bf16x3':
                conv.conv.packed([conv.conv.in_channels], 'bf16x3')
        for i, stage in enumerate(self.stages):
            c, dcn = stage.instance_in_channel, stage.fuse_conv[1]
            stage.fuse_conv[0].packed([c, stage.semantic_transform_in.out_channels, 2])
            dcn.conv_offset.packed([c])
            if fused_dcn is None or fused_dcn[i]:
                dcn._pk.get('w', dcn.weight, ops.pack_conv_weight, job=(False, None, None, None))
            stage.fuse_transform_out.packed([dcn.out_channels])
            if ops.inference_precision() == 'bf16x3':
                for conv, srcs in ((stage.fuse_conv[0], [c, stage.semantic_transform_in.out_channels, 2]),
                                   (dcn.conv_offset, [c]), (stage.fuse_transform_out, [dcn.out_channels])):
                    conv.packed(srcs, 'bf16x3')
            if FUSED_DCN_TOUT[0] and not torch.is_grad_enabled() and stage.fuse_transform_out.weight.is_cuda:
                stage.fuse_transform_out._pk.get('tout', stage.fuse_transform_out.weight, ops.pack_tout_weight)

    def pred_sizes(self, last_stage=None, defer_final_up=False):
        """Spatial size of every (instance, detail) logit pair ``forward`` returns, in order."""
        n = len(self.stages) if last_stage is None else min(last_stage, len(self.stages))
        sizes = [self.stages[i].out_size for i in range(n)]
        if last_stage is not None and last_stage < len(self.stages):
            return sizes + [self.stages[last_stage].out_size]
        last = 2 * self.stages[-1].out_size
        return sizes + [last // 2 if (defer_final_up and not self.pre_upsample_last_stage) else last]

    def forward(self, instance_feats, semantic_feats, rois, roi_labels, last_stage=None, sems=None, pred_out=None):
        """Returns (stage_instance_preds, stage_detail_preds) as the reference.

        ``last_stage`` (extension, default None = all): stop after the logits of
        that exit (1 = the fixed 28x28 exit of BASELINE configs[1]).
        ``sems`` (extension): precomputed ``semantic_maps`` (multi-stream inference).
        ``pred_out`` (extension): one ``(instance, detail)`` pair of [N, 1, S, S] tensors per returned logit pair
        (``pred_sizes``) to write into -- the row slices of a chunked, multi-stream caller's buffers."""
        return run_steps(self.steps(instance_feats, semantic_feats, rois, roi_labels, last_stage, sems, pred_out))

    def steps(self, instance_feats, semantic_feats, rois, roi_labels, last_stage=None, sems=None, pred_out=None, extract=None,
              defer_final_up=False):
        """``forward`` as a generator that yields after every launch (see ``SFMStage.steps``).  ``extract``: a
        callable producing ``instance_feats`` -- the RoI extraction as the chain's first step.  ``defer_final_up``: hand
        back the last stage's logits at ITS resolution (2S) -- the caller folds their align_corners x2 upsample into the
        boundary merge (ops.boundary_merge_chain)."""
        if extract is not None:
            instance_feats = extract()
            yield
        po = (lambda i: None) if pred_out is None else (lambda i: pred_out[i])
        for conv in self.instance_convs:
            instance_feats = conv(instance_feats)
            yield
        stage_instance_preds, stage_detail_preds = [], []
        roi_labels = roi_labels.long().contiguous()
        fused_exit = False
        for idx, stage in enumerate(self.stages):
            if last_stage is not None and idx == last_stage:
                # exit here: only the logits of this resolution are needed
                c, nc = stage.instance_in_channel, stage.num_classes
                logits = ops.class_logits_up2x if fused_exit else ops.class_logits
                ip, dp = logits(instance_feats, stage.instance_logits.weight.detach().view(nc, c),
                                stage.instance_logits.bias.detach(), stage.detail_logits.weight.detach().view(nc, c),
                                stage.detail_logits.bias.detach(), roi_labels, out=po(idx))
                stage_instance_preds.append(ip)
                stage_detail_preds.append(dp)
                return stage_instance_preds, stage_detail_preds
            upsample_flag = self.pre_upsample_last_stage or idx < len(self.stages) - 1
            # the stage before the exit: its x2 upsample would only feed the exit's two logit maps -- they are computed from
            # the stage's own resolution instead (ops.class_logits_up2x), the upsampled tensor never exists
            fused_exit = (last_stage is not None and idx + 1 == last_stage and idx + 1 < len(self.stages) and upsample_flag
                          and not torch.is_grad_enabled() and ops.class_logits_up2x_supported(instance_feats))
            ip, dp, instance_feats = yield from stage.steps(
                instance_feats, semantic_feats[-idx - 3], rois, roi_labels, upsample_flag and not fused_exit,
                sem=None if sems is None else sems[idx], pred_out=po(idx))
            stage_instance_preds.append(ip)
            stage_detail_preds.append(dp)
        # (dynamask_head.py:236-237 clamps the labels to 0 for the class-agnostic last stage: the kernel clamps every
        # label into [0, num_classes - 1] itself, which for one class is that clamp -- no torch launch for it)
        nc = self.stage_num_classes[-1]
        c = self.final_instance_logits.in_channels
        direct = self.pre_upsample_last_stage or defer_final_up
        ip, dp = ops.class_logits(instance_feats, self.final_instance_logits.weight.detach().view(nc, c),
                                  self.final_instance_logits.bias.detach(),
                                  self.final_detail_logits.weight.detach().view(nc, c),
                                  self.final_detail_logits.bias.detach(), roi_labels,
                                  out=po(len(self.stages)) if direct else None)
        yield
        if not direct:
            fin = po(len(self.stages))
            ip = ops.upsample2x(ip, align_corners=True, out=None if fin is None else fin[0])
            yield
            dp = ops.upsample2x(dp, align_corners=True, out=None if fin is None else fin[1])
            yield
        stage_instance_preds.append(ip)
        stage_detail_preds.append(dp)
        return stage_instance_preds, stage_detail_preds


    def forward_dynamic(self, instance_feats, semantic_feats, rois, roi_labels, n_ge, sems=None):
        """Per-RoI early exit (the reference's intent, present there only
        as commented-out code, dynamask_roi_head.py:160-204).  RoIs must be ordered by exit,
        deepest first; ``n_ge[k]`` = number of RoIs whose exit is >= k (``n_ge[0] == N``), so
        the RoIs still alive at stage k are the prefix ``[:n_ge[k]]`` and no gather is needed.
        Stage k's full body runs only on the RoIs that continue; the ones that exit at k get
        just the two class-gathered logits.  Returns a list over k of instance logits
        ``[n_ge[k], 1, S_k, S_k]`` -- row j equals the fixed path's exit-k prediction of RoI j
        bit for bit (RoIs never interact inside the head)."""
        n_ge = list(n_ge) + [0]
        assert n_ge[0] == instance_feats.shape[0] and all(a >= b for a, b in zip(n_ge[:-1], n_ge[1:]))
        for conv in self.instance_convs:
            instance_feats = conv(instance_feats)
        roi_labels = roi_labels.long().contiguous()
        preds = []
        exit_ip = None      # logits of the RoIs that exit at the coming stage, computed from the previous stage's own resolution
        for idx, stage in enumerate(self.stages):
            n_here, n_cont = n_ge[idx], n_ge[idx + 1]
            if n_here == 0:
                preds.append(instance_feats.new_zeros((0, 1, stage.out_size, stage.out_size)))
                continue
            parts = []
            feats_here = instance_feats
            carried, exit_ip = exit_ip, None
            if n_cont > 0:
                upsample_flag = self.pre_upsample_last_stage or idx < len(self.stages) - 1
                n_keep = n_ge[idx + 2] if idx + 2 < len(n_ge) else 0        # RoIs that go on past the next stage
                fuse_next = (upsample_flag and idx + 1 < len(self.stages) and n_keep < n_cont
                             and ops.class_logits_up2x_supported(feats_here))
                ip, _, tail = stage(feats_here[:n_cont], semantic_feats[-idx - 3], rois[:n_cont], roi_labels[:n_cont],
                                    upsample_flag and not fuse_next, sem=None if sems is None else sems[idx])
                if fuse_next:
                    # the RoIs that exit at the next stage need its two logit maps only: from this stage's resolution, the
                    # upsampled features exist for the rows that go on (same bits as the fixed path's exit: same kernel)
                    nxt = self.stages[idx + 1]
                    c, nc = nxt.instance_in_channel, nxt.num_classes
                    exit_ip, _ = ops.class_logits_up2x(tail[n_keep:n_cont], nxt.instance_logits.weight.detach().view(nc, c),
                                                       nxt.instance_logits.bias.detach(), nxt.detail_logits.weight.detach().view(nc, c),
                                                       nxt.detail_logits.bias.detach(), roi_labels[n_keep:n_cont])
                    instance_feats = (ops.upsample2x(tail[:n_keep], align_corners=False, relu=True) if n_keep > 0
                                      else tail.new_zeros((0, tail.shape[1], 2 * tail.shape[2], 2 * tail.shape[3])))
                else:
                    instance_feats = tail
                parts.append(ip)
            if n_cont < n_here:
                if carried is not None:
                    assert carried.shape[0] == n_here - n_cont
                    parts.append(carried)
                else:
                    c, nc = stage.instance_in_channel, stage.num_classes
                    ip, _ = ops.class_logits(feats_here[n_cont:n_here], stage.instance_logits.weight.detach().view(nc, c),
                                             stage.instance_logits.bias.detach(),
                                             stage.detail_logits.weight.detach().view(nc, c),
                                             stage.detail_logits.bias.detach(), roi_labels[n_cont:n_here])
                    parts.append(ip)
            preds.append(parts[0] if len(parts) == 1 else torch.cat(parts))
        n_last = n_ge[len(self.stages)]
        s_last = self.stage_sup_size[-1]
        if n_last == 0:
            preds.append(instance_feats.new_zeros((0, 1, s_last, s_last)))
            return preds
        lab = roi_labels[:n_last]
        if self.stage_num_classes[-1] == 1:
            lab = lab.clamp(max=0)
        nc = self.stage_num_classes[-1]
        c = self.final_instance_logits.in_channels
        ip, _ = ops.class_logits(instance_feats, self.final_instance_logits.weight.detach().view(nc, c),
                                 self.final_instance_logits.bias.detach(),
                                 self.final_detail_logits.weight.detach().view(nc, c),
                                 self.final_detail_logits.bias.detach(), lab)
        if not self.pre_upsample_last_stage:
            ip = ops.upsample2x(ip, align_corners=True)
        preds.append(ip)
        return preds

    # ------------------------------------------------ callers either side of the path
    def get_targets(self, pos_bboxes_list, pos_assigned_gt_inds_list, gt_masks_list):
        """dynamask_head.py:246-271 with the GT bitmaps already on the device
        ([G, H, W] tensors per image): clip + RoIAlign(scale 1, adaptive grid) on the
        bitmaps + (>= 0.5), for every supervision size -- no device->host->device trip
        (the reference goes through numpy per image and size)."""
        per_stage = [[] for _ in self.stage_sup_size]
        for boxes, inds, masks in zip(pos_bboxes_list, pos_assigned_gt_inds_list, gt_masks_list):
            if boxes.shape[0] == 0:              # an image without positives (no GT): nothing to crop
                for i, size in enumerate(self.stage_sup_size):
                    per_stage[i].append(boxes.new_zeros((0, size, size)))
                continue
            if hasattr(masks, 'masks') and isinstance(masks.masks, (list, tuple)):
                # a PolygonMasks-like holder (list over objects of lists of vertex arrays; .height / .width): the
                # polygons go to the device once and every size is rasterised there (structures.py:469-503, 583-599)
                packed = ops.pack_polygons(masks.masks, boxes.device)
                b = boxes[:, :4].contiguous().float().clone()
                b[:, 0::2].clamp_(0, float(masks.width))
                b[:, 1::2].clamp_(0, float(masks.height))
                for i, size in enumerate(self.stage_sup_size):
                    per_stage[i].append(ops.polygon_mask_targets(packed, b, inds.long().contiguous(), size))
                continue
            if hasattr(masks, 'masks'):           # a BitmapMasks-like holder of a numpy array
                masks = torch.from_numpy(masks.masks).to(boxes.device)
            m = masks.to(torch.float32).contiguous()[:, None]
            maxh, maxw = m.shape[-2:]
            rois = ops.mask_target_rois(boxes[:, :4].contiguous().float(), inds.long().contiguous(), maxw, maxh)
            for i, size in enumerate(self.stage_sup_size):
                t = ops.roi_align([m], rois, size, [1.0], 0)
                per_stage[i].append(ops.threshold_ge(t, 0.5).squeeze(1))
        return [torch.cat(t) for t in per_stage]

    def get_seg_masks(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale):
        """dynamask_head.py:279-342: sigmoid -> paste into the image -> threshold -> list of (h, w) bool numpy arrays,
        one per detection (one paste kernel for all detections)."""
        return paste_segms(select_label_channel(mask_pred, det_labels), det_bboxes, det_labels, rcnn_test_cfg, ori_shape,
                           scale_factor, rescale)

    def get_seg_rles(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale):
        """``get_seg_masks`` followed by ``encode_mask_results``, on the device (``paste_segms``): one COCO RLE dict per
        detection."""
        return paste_segms(select_label_channel(mask_pred, det_labels), det_bboxes, det_labels, rcnn_test_cfg, ori_shape,
                           scale_factor, rescale, encode=True)


# ---------------------------------------------------------------- FCN mask head
@UPSAMPLE_LAYERS.register_module(name='deconv')
class _Deconv(nn.Module):
    """nn.ConvTranspose2d(k=2, s=2) parameter holder: weight [Cin, Cout, 2, 2]."""

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=2):
        super().__init__()
        if kernel_size != 2 or stride != 2:
            raise NotImplementedError('deconv upsample is 2x2 stride 2 on the path')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, 2, 2))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.kaiming_normal_(self.weight, mode='fan_out', nonlinearity='relu')
        self._pk = _Packed()

    def forward(self, x, relu=False):
        p = ops.deconv_precision_for(x.shape[2], x.shape[3])
        wp = self._pk.get('w', self.weight, lambda w: ops.pack_deconv_weight(w, precision=p), precision=p)
        return ops.deconv2x2(x, wp, self.bias.detach(), self.out_channels, relu=relu)


@UPSAMPLE_LAYERS.register_module(name='bilinear')
class _BilinearUp(nn.Module):
    def __init__(self, scale_factor=2, mode='bilinear', align_corners=False):
        super().__init__()
        if scale_factor != 2:
            raise NotImplementedError('x2 upsampling only')
        self.align_corners = bool(align_corners)

    def forward(self, x, relu=False):
        return ops.upsample2x(x, align_corners=self.align_corners, relu=relu)


@UPSAMPLE_LAYERS.register_module(name='nearest')
class _NearestUp(nn.Module):
    """nn.Upsample(scale_factor=2, mode='nearest') (fcn_mask_head.py:88-96)."""

    def __init__(self, scale_factor=2, mode='nearest', align_corners=None):
        super().__init__()
        if scale_factor != 2:
            raise NotImplementedError('x2 upsampling only')

    def forward(self, x, relu=False):
        assert not relu
        return ops.upsample2x_nearest(x)


def build_upsample_layer(cfg):
    cfg = dict(cfg)
    t = cfg.pop('type')
    cls = UPSAMPLE_LAYERS.get(t)
    if cls is None:
        raise KeyError(f'unsupported upsample type {t!r}')
    return cls(**cfg)


@HEADS.register_module()
class FCNMaskHead(nn.Module):
    """fcn_mask_head.py:19-126.  Forward and (train_path.FCNMaskHeadFn) its backward for every upsample
    type; the fork's own ``loss`` is broken (``mask_cross_entropy`` changed its signature),
    so the head is differentiable but the reference cannot train it through ``loss_mask``."""

    def __init__(self, num_convs=4, roi_feat_size=14, in_channels=256, conv_kernel_size=3, conv_out_channels=256,
                 num_classes=80, class_agnostic=False, upsample_cfg=dict(type='deconv', scale_factor=2),
                 conv_cfg=None, norm_cfg=None, loss_mask=None):
        super().__init__()
        self.upsample_cfg = dict(upsample_cfg)
        if self.upsample_cfg['type'] not in [None, 'deconv', 'nearest', 'bilinear', 'carafe']:
            raise ValueError(f'Invalid upsample method {self.upsample_cfg["type"]}, accepted methods are '
                             '"deconv", "nearest", "bilinear", "carafe"')
        self.num_convs = num_convs
        self.in_channels = in_channels
        self.conv_kernel_size = conv_kernel_size
        self.conv_out_channels = conv_out_channels
        self.upsample_method = self.upsample_cfg.get('type')
        self.scale_factor = self.upsample_cfg.pop('scale_factor', None)
        self.num_classes = num_classes
        self.class_agnostic = class_agnostic
        self.convs = nn.ModuleList()
        for i in range(num_convs):
            cin = in_channels if i == 0 else conv_out_channels
            self.convs.append(ConvModule(cin, conv_out_channels, conv_kernel_size, padding=(conv_kernel_size - 1) // 2,
                                         conv_cfg=conv_cfg, norm_cfg=norm_cfg))
        up_in = conv_out_channels if num_convs > 0 else in_channels
        cfg_ = dict(self.upsample_cfg)
        if self.upsample_method is None:
            self.upsample = None
        elif self.upsample_method == 'deconv':
            cfg_.update(in_channels=up_in, out_channels=conv_out_channels, kernel_size=self.scale_factor,
                        stride=self.scale_factor)
            self.upsample = build_upsample_layer(cfg_)
        elif self.upsample_method == 'carafe':
            cfg_.update(channels=up_in, scale_factor=self.scale_factor)
            self.upsample = build_upsample_layer(cfg_)
        elif self.upsample_method == 'bilinear':
            cfg_.update(scale_factor=self.scale_factor, mode='bilinear', align_corners=False)
            self.upsample = build_upsample_layer(cfg_)
        else:
            cfg_.update(scale_factor=self.scale_factor, mode='nearest', align_corners=None)
            self.upsample = build_upsample_layer(cfg_)
        out_channels = 1 if class_agnostic else num_classes
        logits_in = conv_out_channels if self.upsample_method == 'deconv' else up_in
        self.conv_logits = _Conv(logits_in, out_channels, 1)

    def init_weights(self):
        for m in [self.upsample, self.conv_logits]:
            if m is None:
                continue
            if isinstance(m, CARAFEPack):
                m.init_weights()
            elif hasattr(m, 'weight'):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return FCNMaskHeadFn.apply(self, x, *list(self.parameters()))
        for conv in self.convs:
            x = conv(x)
        if self.upsample is not None:
            x = self.upsample(x, relu=(self.upsample_method == 'deconv'))
        return self.conv_logits.run(x)

    # ------------------------------------------------ callers either side of the path
    def get_targets(self, sampling_results, gt_masks, rcnn_train_cfg):
        """fcn_mask_head.py:128-135 + core/mask/mask_target.py:7-62: per image, clip the positive proposals to the GT
        canvas, crop-and-resize the assigned GT bitmap to ``rcnn_train_cfg.mask_size`` (RoIAlign, scale 1, adaptive
        grid, aligned) and threshold at 0.5 -> float [N, S, S].  On the device: ``gt_masks`` are [G, H, W] tensors, or
        BitmapMasks- / PolygonMasks-like holders (``.masks``), as ``DynaMaskHead.get_targets`` takes them."""
        ms = rcnn_train_cfg.mask_size if hasattr(rcnn_train_cfg, 'mask_size') else rcnn_train_cfg['mask_size']
        size = ms if isinstance(ms, int) else ms[0]
        if not isinstance(ms, int) and ms[0] != ms[1]:
            raise NotImplementedError('square mask targets only (mask_size is an int in every config of the reference)')
        out = []
        for res, masks in zip(sampling_results, gt_masks):
            boxes, inds = res.pos_bboxes, res.pos_assigned_gt_inds
            if boxes.shape[0] == 0:
                out.append(boxes.new_zeros((0, size, size)))
                continue
            if hasattr(masks, 'masks') and isinstance(masks.masks, (list, tuple)):
                packed = ops.pack_polygons(masks.masks, boxes.device)
                b = boxes[:, :4].contiguous().float().clone()
                b[:, 0::2].clamp_(0, float(masks.width))
                b[:, 1::2].clamp_(0, float(masks.height))
                out.append(ops.polygon_mask_targets(packed, b, inds.long().contiguous(), size).float())
                continue
            if hasattr(masks, 'masks'):
                masks = torch.from_numpy(masks.masks).to(boxes.device)
            m = masks.to(torch.float32).contiguous()[:, None]
            maxh, maxw = m.shape[-2:]
            rois = ops.mask_target_rois(boxes[:, :4].contiguous().float(), inds.long().contiguous(), maxw, maxh)
            out.append(ops.threshold_ge(ops.roi_align([m], rois, size, [1.0], 0), 0.5).squeeze(1).float())
        return torch.cat(out) if out else out

    def loss(self, mask_pred, mask_targets, labels):
        """fcn_mask_head.py:137-149 cannot run in the fork: ``mask_cross_entropy`` lost its ``label`` argument
        (cross_entropy_loss.py:90-120), so ``CrossEntropyLoss(use_mask=True)`` raises there too."""
        raise NotImplementedError('FCNMaskHead.loss is broken in the reference fork itself (SURVEY App. C Q5)')

    def _selected(self, mask_pred, det_bboxes, det_labels):
        if isinstance(mask_pred, torch.Tensor):
            apply_sigmoid = True            # single-scale testing hands over logits (fcn_mask_head.py:168-169)
        else:                               # multi-scale testing: probabilities, already averaged, as an ndarray (:170-171)
            mask_pred, apply_sigmoid = det_bboxes.new_tensor(mask_pred), False
        return select_label_channel(mask_pred, det_labels), apply_sigmoid

    def get_seg_masks(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale):
        """fcn_mask_head.py:151-237: (sigmoid ->) class select -> paste into the image -> threshold -> ``cls_segms``:
        one list per class holding the (h, w) bool arrays of that class's detections, in detection order.  The
        [n, classes, S, S] logits are gathered first (the sigmoid commutes with the selection), then one paste kernel
        runs for all detections and ONE device -> host copy carries the bitmaps."""
        sel, apply_sigmoid = self._selected(mask_pred, det_bboxes, det_labels)
        return paste_segms(sel, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale,
                           apply_sigmoid=apply_sigmoid, num_classes=self.num_classes)

    def get_seg_rles(self, mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale):
        """``get_seg_masks`` followed by ``encode_mask_results`` (core/mask/utils.py:36-63) without the bitmaps: paste,
        threshold and run-length encoding on the device; returns ``cls_segms`` of COCO RLE dicts."""
        sel, apply_sigmoid = self._selected(mask_pred, det_bboxes, det_labels)
        return paste_segms(sel, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale, encode=True,
                           apply_sigmoid=apply_sigmoid, num_classes=self.num_classes)


# ---------------------------------------------------------------- RefineMask head (inference)
class DilatedConvModule(nn.Module):
    """mmcv ConvModule(3x3, padding = dilation) without norm: conv(bias) (+ ReLU); keys ``conv.weight/bias``.  Runs on the
    any-width dilated kernel (ops.conv3x3_dil, exact fp32 in every precision mode): RefineMask's semantic convs on the
    whole stride-4 FPN map (d = 1) and MultiBranchFusion's branches."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, dilation=1, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type='ReLU')):
        super().__init__()
        if conv_cfg is not None or norm_cfg is not None:
            raise NotImplementedError('conv_cfg / norm_cfg are None in configs/refinemask')
        if kernel_size != 3 or padding != dilation or not 1 <= dilation <= 8:
            raise NotImplementedError('3x3 convolutions with padding = dilation in [1, 8] only')
        self.conv = _Conv(in_channels, out_channels, 3)
        self.dilation = dilation
        self.with_activation = act_cfg is not None

    def packed(self):
        return self.conv.packed([self.conv.in_channels], 'fp32')

    def forward(self, x):
        b = self.conv.bias.detach() if self.conv.bias is not None else None
        return ops.conv3x3_dil(x, self.packed(), b, self.conv.out_channels, self.dilation, relu=self.with_activation)


class MultiBranchFusion(nn.Module):
    """refine_mask_head.py:17-33: merge_conv(sum_b relu(conv_{d_b}(x) + b_b)), merge_conv 1x1 without activation (the
    caller's loop applies the ReLU: ``forward(x, relu=True)``).  The branch sum is ONE launch (ops.conv3x3_multidil; the
    unfused sequence with ops.FUSED_MULTIDIL[0] = False, same bits).  Keys dilation_conv_{1,2,3}.conv.*, merge_conv.conv.*."""

    def __init__(self, feat_dim, dilations=[1, 3, 5]):
        super().__init__()
        if len(dilations) != 3:
            raise NotImplementedError('MultiBranchFusion has three branches (refine_mask_head.py:28-31)')
        self.dilations = list(dilations)
        for idx, dilation in enumerate(dilations):
            self.add_module(f'dilation_conv_{idx + 1}', DilatedConvModule(feat_dim, feat_dim, 3, padding=dilation,
                                                                          dilation=dilation))
        self.merge_conv = ConvModule(feat_dim, feat_dim, 1, act_cfg=None)
        self.feat_dim = feat_dim

    def branches(self):
        return [getattr(self, f'dilation_conv_{i + 1}') for i in range(3)]

    def branch_sum(self, x, fused=None):
        br = self.branches()
        return ops.conv3x3_multidil(x, [m.packed() for m in br], [m.conv.bias.detach() for m in br], self.feat_dim,
                                    self.dilations, relu=True, fused=fused)

    def forward(self, x, relu=False):
        return self.merge_conv.conv.run(self.branch_sum(x), relu=relu)


class RefineSFMStage(nn.Module):
    """refine_mask_head.py:36-136 (fusion_type 'MultiBranchFusion'), inference.  Same keys as the reference's SFMStage."""

    def __init__(self, semantic_in_channel=256, semantic_out_channel=256, instance_in_channel=256, instance_out_channel=256,
                 fusion_type='MultiBranchFusion', dilations=[1, 3, 5], out_size=14, num_classes=80, semantic_out_stride=4,
                 mask_use_sigmoid=False, upsample_cfg=dict(type='bilinear', scale_factor=2)):
        super().__init__()
        if fusion_type != 'MultiBranchFusion':
            raise NotImplementedError('fusion_type is MultiBranchFusion in configs/refinemask')
        if upsample_cfg.get('type') != 'bilinear' or upsample_cfg.get('scale_factor') != 2:
            raise NotImplementedError('the SFM stage upsample is bilinear x2 in configs/refinemask')
        self.semantic_out_stride = semantic_out_stride
        self.mask_use_sigmoid = mask_use_sigmoid
        self.num_classes = num_classes
        self.out_size = out_size
        self.instance_in_channel = instance_in_channel
        self.instance_out_channel = instance_out_channel
        self.semantic_transform_in = _Conv(semantic_in_channel, semantic_out_channel, 1)
        self.semantic_transform_out = _Conv(semantic_out_channel, semantic_out_channel, 1)
        self.instance_logits = _Conv(instance_in_channel, num_classes, 1)
        fuse_in_channel = instance_in_channel + semantic_out_channel + 2
        self.fuse_conv = nn.ModuleList([_Conv(fuse_in_channel, instance_in_channel, 1),
                                        MultiBranchFusion(instance_in_channel, dilations=dilations)])
        self.fuse_transform_out = _Conv(instance_in_channel, instance_out_channel - 2, 1)

    def semantic_map(self, semantic_feat):
        """relu(semantic_transform_in(semantic_feat)) on the whole map (refine_mask_head.py:103): no RoI enters it."""
        return self.semantic_transform_in.run(semantic_feat, relu=True)

    def forward(self, instance_feats, semantic_feat, semantic_prob, rois, roi_labels, sem=None):
        """-> (instance logits [n, 1, S, S], the next stage's features [n, out, 2S, 2S]).  ``semantic_prob``: the
        (sigmoid of the) semantic logits [B, 1, H, W]; ``sem``: a precomputed ``semantic_map``."""
        n, c, s = instance_feats.shape[0], self.instance_in_channel, self.out_size
        if sem is None:
            sem = self.semantic_map(semantic_feat)
        scale = 1.0 / self.semantic_out_stride
        # instance-wise semantic feats: SingleRoIExtractor (RoIAlign aligned, sampling_ratio 0, one level) + relu(1x1)
        ins_sem = self.semantic_transform_out.run(ops.roi_align([sem], rois, s, [scale], 0), relu=True)
        # [instance mask | semantic mask]: the two extra channels of the fusion input (the same-size interpolations of
        # refine_mask_head.py:111,118-119 are identities)
        masks = torch.empty((n, 2, s, s), device=instance_feats.device, dtype=torch.float32)
        nc = self.num_classes
        w, b = self.instance_logits.weight.detach().view(nc, c), self.instance_logits.bias.detach()
        ip, _ = ops.class_logits(instance_feats, w, b, w, b, roi_labels, sig_out=masks if self.mask_use_sigmoid else None)
        if not self.mask_use_sigmoid:
            masks[:, 0:1].copy_(ip)
        masks[:, 1:2].copy_(ops.roi_align([semantic_prob], rois, s, [scale], 0))
        fused = self.fuse_conv[0].run([instance_feats, ins_sem, masks], relu=True)
        fused = self.fuse_conv[1](fused, relu=True)
        fused = self.fuse_transform_out.run(fused, relu=True)
        # relu(bilinear x2, align_corners=False) of the features, align_corners=True x2 of the two masks (:124-132)
        nxt = torch.cat([ops.upsample2x(fused, align_corners=False, relu=True), ops.upsample2x(masks, align_corners=True)], 1)
        return ip, nxt


@HEADS.register_module()
class RefineMaskHead(nn.Module):
    """refine_mask_head.py:139-337, inference: same constructor kwargs and ``state_dict`` keys as the reference, so
    RefineMask checkpoints load.  ``forward`` returns (stage_instance_preds, semantic_pred) as the reference.  Training
    (``loss``, ``get_targets``) is the follow-up: RefineCrossEntropyLoss.forward raises."""

    def __init__(self, num_convs_instance=2, num_convs_semantic=4, conv_in_channels_instance=256,
                 conv_in_channels_semantic=256, conv_kernel_size_instance=3, conv_kernel_size_semantic=3,
                 conv_out_channels_instance=256, conv_out_channels_semantic=256, conv_cfg=None, norm_cfg=None,
                 fusion_type='MultiBranchFusion', dilations=[1, 3, 5], semantic_out_stride=4, mask_use_sigmoid=False,
                 stage_num_classes=[80, 80, 80, 80], stage_sup_size=[14, 28, 56, 112],
                 upsample_cfg=dict(type='bilinear', scale_factor=2),
                 loss_cfg=dict(type='RefineCrossEntropyLoss', stage_instance_loss_weight=[0.25, 0.5, 0.75, 1.0],
                               semantic_loss_weight=1.0, boundary_width=2, start_stage=1)):
        super().__init__()
        self.num_convs_instance = num_convs_instance
        self.conv_kernel_size_instance = conv_kernel_size_instance
        self.conv_in_channels_instance = conv_in_channels_instance
        self.conv_out_channels_instance = conv_out_channels_instance
        self.num_convs_semantic = num_convs_semantic
        self.conv_kernel_size_semantic = conv_kernel_size_semantic
        self.conv_in_channels_semantic = conv_in_channels_semantic
        self.conv_out_channels_semantic = conv_out_channels_semantic
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.semantic_out_stride = semantic_out_stride
        self.stage_sup_size = stage_sup_size
        self.stage_num_classes = stage_num_classes
        self.mask_use_sigmoid = mask_use_sigmoid
        if conv_kernel_size_semantic != 3:
            raise NotImplementedError('the semantic convs are 3x3 in configs/refinemask')

        convs = []
        for i in range(num_convs_instance):
            cin = conv_in_channels_instance if i == 0 else conv_out_channels_instance
            convs.append(ConvModule(cin, conv_out_channels_instance, conv_kernel_size_instance, dilation=1, padding=1))
        self.instance_convs = nn.ModuleList(convs)
        convs = []
        for i in range(num_convs_semantic):
            cin = conv_in_channels_semantic if i == 0 else conv_out_channels_semantic
            convs.append(DilatedConvModule(cin, conv_out_channels_semantic, 3, padding=1, dilation=1))
        self.semantic_convs = nn.ModuleList(convs)
        self.loss_func = build_loss(loss_cfg)

        assert len(self.stage_sup_size) > 1
        self.stages = nn.ModuleList()
        out_channel = conv_out_channels_instance
        for idx, out_size in enumerate(self.stage_sup_size[:-1]):
            in_channel = out_channel
            out_channel = in_channel // 2
            self.stages.append(RefineSFMStage(
                semantic_in_channel=conv_out_channels_semantic, semantic_out_channel=in_channel,
                instance_in_channel=in_channel, instance_out_channel=out_channel, fusion_type=fusion_type,
                dilations=dilations, out_size=out_size, num_classes=self.stage_num_classes[idx],
                semantic_out_stride=semantic_out_stride, mask_use_sigmoid=mask_use_sigmoid, upsample_cfg=upsample_cfg))
        self.final_instance_logits = _Conv(out_channel, self.stage_num_classes[-1], 1)
        self.semantic_logits = _Conv(conv_out_channels_semantic, 1, 1)

    def init_weights(self):
        for m in [self.final_instance_logits, self.semantic_logits]:
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)

    def semantic_forward(self, semantic_feat):
        """The four 3x3 semantic convs on the whole stride-4 map, then semantic_logits -> (features, semantic_pred)
        (refine_mask_head.py:235-238): once per call, for all images of the batch."""
        for conv in self.semantic_convs:
            semantic_feat = conv(semantic_feat)
        return semantic_feat, self.semantic_logits.run(semantic_feat)

    def forward(self, instance_feats, semantic_feat, rois, roi_labels):
        """refine_mask_head.py:231-252 -> (stage_instance_preds [n, 1, S_k, S_k] per stage, semantic_pred [B, 1, H, W])."""
        for conv in self.instance_convs:
            instance_feats = conv(instance_feats)
        semantic_feat, semantic_pred = self.semantic_forward(semantic_feat)
        semantic_prob = ops.sigmoid(semantic_pred) if self.mask_use_sigmoid else semantic_pred
        roi_labels = roi_labels.long().contiguous()
        rois = rois.contiguous()
        stage_instance_preds = []
        for stage in self.stages:
            ip, instance_feats = stage(instance_feats, semantic_feat, semantic_prob, rois, roi_labels)
            stage_instance_preds.append(ip)
        # (refine_mask_head.py:247-248 clamps the labels to 0 for the class-agnostic last stage (LVIS): the kernel clamps
        # every label into [0, num_classes - 1] itself, which for one class is that clamp)
        nc = self.stage_num_classes[-1]
        c = self.final_instance_logits.in_channels
        w, b = self.final_instance_logits.weight.detach().view(nc, c), self.final_instance_logits.bias.detach()
        ip, _ = ops.class_logits(instance_feats, w, b, w, b, roi_labels)
        stage_instance_preds.append(ip)
        return stage_instance_preds, semantic_pred

    # refine_mask_head.py:289-337 = dynamask_head.py:279-342 (sigmoid, paste, threshold)
    get_seg_masks = DynaMaskHead.get_seg_masks
    get_seg_rles = DynaMaskHead.get_seg_rles

    def get_targets(self, *a, **k):
        raise NotImplementedError('RefineMask training (targets, RefineCrossEntropyLoss) is the follow-up to inference')

    def loss(self, *a, **k):
        raise NotImplementedError('RefineMask training (targets, RefineCrossEntropyLoss) is the follow-up to inference')


# ---------------------------------------------------------------- PointRend heads (inference)
class _DownsampleConv(nn.Module):
    """Parameter holder named like nn.Conv2d (weight [Cout, Cin, 2, 2], bias) of a 2 x 2 stride-2 convolution, run as
    dm_pixel_unshuffle2x + a 1x1 convolution over the 4 Cin unshuffled channels, whose weight is this one permuted to
    the unshuffle's channel order (dy * 2 + dx) * Cin + c."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 2, 2))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.kaiming_normal_(self.weight, mode='fan_out', nonlinearity='relu')
        self._pk = _Packed()

    def packed(self):
        cin4 = 4 * self.in_channels
        return self._pk.get('unshuffled', self.weight, lambda w: ops.pack_conv_weight(
            w.permute(0, 2, 3, 1).reshape(self.out_channels, cin4, 1, 1).contiguous()))

    def run(self, x, relu=True):
        return ops.conv2d([ops.pixel_unshuffle2x(x)], self.packed(), self.bias.detach(), self.out_channels, 1, relu=relu)


class _DownsampleConvModule(nn.Module):
    """ConvModule(k = s = 2, padding 0) without norm: keys ``conv.weight/bias``."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = _DownsampleConv(in_channels, out_channels)

    def forward(self, x):
        return self.conv.run(x, relu=True)


@HEADS.register_module()
class CoarseMaskHead(FCNMaskHead):
    """``CoarseMaskHead`` -- mmdet/models/roi_heads/mask_heads/coarse_mask_head.py, inference: ``num_convs`` 3x3
    convolutions, the 2 x 2 stride-2 ``downsample_conv`` (dm_pixel_unshuffle2x + a 1x1 convolution), ``flatten``,
    ``num_fcs`` fully connected layers with ReLU and ``fc_logits`` on dm_fc_fwd -> [n, classes, S / 2, S / 2].  No
    ``conv_logits`` (the reference deletes it).  ``get_seg_masks`` / ``get_seg_rles`` are FCNMaskHead's; PointRendRoIHead
    hands them the refined map of the label channel only ([n, 1, S, S]), which is pasted as it is."""

    def __init__(self, num_convs=0, num_fcs=2, fc_out_channels=1024, downsample_factor=2, *arg, **kwarg):
        super().__init__(*arg, num_convs=num_convs, upsample_cfg=dict(type=None), **kwarg)
        if num_fcs <= 0:
            raise ValueError('CoarseMaskHead needs num_fcs > 0')
        if downsample_factor not in (1, 2):
            raise NotImplementedError('CoarseMaskHead: downsample_factor 1 or 2 (configs/point_rend uses 2)')
        self.num_fcs = num_fcs
        self.fc_out_channels = fc_out_channels
        self.downsample_factor = downsample_factor
        del self.conv_logits
        roi = kwarg.get('roi_feat_size', 14)
        self.roi_feat_size = (roi, roi) if isinstance(roi, int) else tuple(roi)
        if downsample_factor > 1:
            cin = self.conv_out_channels if self.num_convs > 0 else self.in_channels
            self.downsample_conv = _DownsampleConvModule(cin, self.conv_out_channels)
            last = self.conv_out_channels
        else:
            self.downsample_conv = None
            last = self.conv_out_channels if self.num_convs > 0 else self.in_channels
        self.output_size = (self.roi_feat_size[0] // downsample_factor, self.roi_feat_size[1] // downsample_factor)
        self.output_area = self.output_size[0] * self.output_size[1]
        last_layer_dim = last * self.output_area
        self.fcs = nn.ModuleList()
        for i in range(num_fcs):
            self.fcs.append(nn.Linear(last_layer_dim if i == 0 else fc_out_channels, fc_out_channels))
        out_channels = 1 if self.class_agnostic else self.num_classes
        self.fc_logits = nn.Linear(fc_out_channels, out_channels * self.output_area)

    def init_weights(self):
        for m in self.fcs:
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.fc_logits.weight, 0.001)
        nn.init.constant_(self.fc_logits.bias, 0)

    def forward(self, x):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and x.requires_grad:
            raise NotImplementedError('CoarseMaskHead: training is broken in the reference fork itself (SURVEY App. C Q5)')
        for conv in self.convs:
            x = conv(x)
        if self.downsample_conv is not None:
            x = self.downsample_conv(x)
        n = x.shape[0]
        x = x.reshape(n, -1)
        for fc in self.fcs:
            x = ops.fc(x, fc.weight.detach(), fc.bias.detach(), relu=True)
        x = ops.fc(x, self.fc_logits.weight.detach(), self.fc_logits.bias.detach())
        return x.view(n, -1, *self.output_size)

    def _selected(self, mask_pred, det_bboxes, det_labels):
        if isinstance(mask_pred, torch.Tensor) and mask_pred.dim() == 4 and mask_pred.shape[1] == 1:
            return mask_pred.contiguous(), True     # PointRend's refined map: the label channel already
        return super()._selected(mask_pred, det_bboxes, det_labels)


class _Conv1d(nn.Module):
    """Parameter holder named like nn.Conv1d(kernel_size=1) (weight [Cout, Cin, 1], bias)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 1))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.kaiming_normal_(self.weight, mode='fan_out', nonlinearity='relu')
        self._pk = _Packed()

    def packed(self):
        return self._pk.get('1x1', self.weight, lambda w: ops.pack_conv_weight(w[..., None].contiguous()))


class _PointConvModule(nn.Module):
    """ConvModule(conv_cfg=Conv1d, 1x1, norm None, ReLU): keys ``conv.weight/bias``."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = _Conv1d(in_channels, out_channels)


@HEADS.register_module()
class MaskPointHead(nn.Module):
    """``MaskPointHead`` -- mmdet/models/roi_heads/mask_heads/mask_point_head.py, inference: ``num_fcs`` shared 1x1
    layers (256 + classes) -> 256 with ReLU, the coarse point logits re-concatenated after each (coarse_pred_each_layer),
    then ``fc_logits``.  ``refine_`` runs it on the points of ``ops.point_gather`` and stores the LABEL row of the logits
    into the refined map (ops.point_mlp_scatter): every other class row would be discarded by the paste.  Training
    (``get_targets``, ``loss``: ``mask_cross_entropy``, broken in the fork, Quirk Q5) raises."""

    def __init__(self, num_classes, num_fcs=3, in_channels=256, fc_channels=256, class_agnostic=False,
                 coarse_pred_each_layer=True, conv_cfg=dict(type='Conv1d'), norm_cfg=None, act_cfg=dict(type='ReLU'),
                 loss_point=dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0)):
        super().__init__()
        if not coarse_pred_each_layer:
            raise NotImplementedError('MaskPointHead: coarse_pred_each_layer=True only (configs/point_rend)')
        if conv_cfg is None or dict(conv_cfg).get('type') != 'Conv1d' or norm_cfg is not None:
            raise NotImplementedError('MaskPointHead: Conv1d layers without norm only (configs/point_rend)')
        if act_cfg is None or dict(act_cfg).get('type') != 'ReLU':
            raise NotImplementedError('MaskPointHead: ReLU activations only (configs/point_rend)')
        if in_channels != fc_channels:
            raise NotImplementedError('MaskPointHead: in_channels == fc_channels only (configs/point_rend: 256)')
        self.num_fcs = num_fcs
        self.in_channels = in_channels
        self.fc_channles = fc_channels          # (sic: the reference's attribute name)
        self.num_classes = num_classes
        self.class_agnostic = class_agnostic
        self.coarse_pred_each_layer = coarse_pred_each_layer
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.loss_point_cfg = loss_point
        cin = in_channels + num_classes
        self.fcs = nn.ModuleList()
        for _ in range(num_fcs):
            self.fcs.append(_PointConvModule(cin, fc_channels))
            cin = fc_channels + num_classes
        self.fc_logits = _Conv1d(cin, 1 if class_agnostic else num_classes)

    def init_weights(self):
        nn.init.normal_(self.fc_logits.weight, 0, 0.001)
        nn.init.constant_(self.fc_logits.bias, 0)

    def supported(self, point_feats, hw):
        return ops.point_mlp_supported(point_feats, self.num_fcs, self.fc_logits.out_channels, hw)

    def refine_(self, point_feats, labels, point_indices, refined, fused=None):
        """``refined`` [n, 1, H, W] (the label channel) at ``point_indices`` [n, P] <- the label row of
        ``forward(point_feats[:, :256], point_feats[:, 256:])``, in place (point_feats: ``ops.point_gather``)."""
        hw = ops._cells(refined)
        if not self.supported(point_feats, hw):
            raise NotImplementedError(f'MaskPointHead: no kernel for point features {tuple(point_feats.shape)}')
        fl = self.fc_logits
        return ops.point_mlp_scatter(point_feats, [m.conv.packed() for m in self.fcs], [m.conv.bias.detach() for m in self.fcs],
                                     fl.weight.detach().view(fl.out_channels, fl.in_channels), fl.bias.detach(),
                                     labels, point_indices, refined, fused=fused)

    def get_targets(self, *a, **k):
        raise NotImplementedError('MaskPointHead.get_targets: PointRend training is broken in the reference (Quirk Q5)')

    def loss(self, *a, **k):
        raise NotImplementedError('MaskPointHead.loss: mask_cross_entropy is broken in the reference fork (Quirk Q5)')


# ---------------------------------------------------------------- PointRefine: PointRefineMaskHead (inference)
class PointRefineSFMStage(nn.Module):
    """``SFMStage`` of mmdet/models/roi_heads/mask_heads/mask_point_refine.py:20-132, inference: same keys as the reference
    (``fcs.j.conv`` Conv1d [C, C + 2 * classes, 1], ``fc_logits``, ``semantic_transform_in``, ``instance_logits``,
    ``detail_logits``, ``fuse_transform_out``).  ``forward`` refines the stage features at the ``num_points`` cells of
    largest detail value (ops.point_topk_select -> ops.point_feat_gather -> ops.point_refine_mlp, all C rows of
    fc_logits into the features), then relu(fuse_transform_out) and relu(bilinear x2)."""

    def __init__(self, semantic_in_channel=256, semantic_out_channel=256, fc_in_channels=256, fc_channels=256,
                 fc_out_channels=256, num_fcs=3, num_classes=80, semantic_out_stride=4, mask_use_sigmoid=False,
                 class_agnostic=False, coarse_pred_each_layer=True, upsample_cfg=dict(type='bilinear', scale_factor=2)):
        super().__init__()
        if class_agnostic:
            raise NotImplementedError('PointRefineMaskHead: class_agnostic=False only (fc_logits refines every feature '
                                      'channel; configs/point_refine)')
        if not coarse_pred_each_layer:
            raise NotImplementedError('PointRefineMaskHead: coarse_pred_each_layer=True only (configs/point_refine)')
        if fc_in_channels != fc_channels or semantic_out_channel != fc_channels:
            raise NotImplementedError('PointRefineMaskHead: the stage width is one C (fc_in = fc = semantic_out channels)')
        if fc_channels % 2 != 0 or fc_channels < 8:
            raise NotImplementedError(f'PointRefineMaskHead: stage width {fc_channels}: an even width >= 8 only')
        if num_fcs < 1:
            raise NotImplementedError('PointRefineMaskHead: num_fcs >= 1 only')
        if upsample_cfg.get('type') != 'bilinear' or upsample_cfg.get('scale_factor') != 2:
            raise NotImplementedError('the SFM stage upsample is bilinear x2 in configs/point_refine')
        self.num_fcs = num_fcs
        self.semantic_out_stride = semantic_out_stride
        self.mask_use_sigmoid = mask_use_sigmoid
        self.num_classes = num_classes
        self.coarse_pred_each_layer = coarse_pred_each_layer
        self.class_agnostic = class_agnostic
        self.channels = fc_channels
        cin = fc_in_channels + 2 * num_classes
        self.fcs = nn.ModuleList()
        for _ in range(num_fcs):
            self.fcs.append(_PointConvModule(cin, fc_channels))
            cin = fc_channels + 2 * num_classes
        self.fc_logits = _Conv1d(cin, fc_channels)
        self.semantic_transform_in = _Conv(semantic_in_channel, semantic_out_channel, 1)
        self.instance_logits = _Conv(fc_channels, num_classes, 1)
        self.detail_logits = _Conv(fc_channels, num_classes, 1)
        self.fuse_transform_out = _Conv(fc_channels, fc_out_channels, 1)

    def mlp_params(self):
        """(packed weights, biases): the hidden layers, then fc_logits (ops.point_refine_mlp's order)."""
        layers = [m.conv for m in self.fcs] + [self.fc_logits]
        return [m.packed() for m in layers], [m.bias.detach() for m in layers]

    def forward(self, instance_feats, sem, rois, roi_labels, num_points, form=None):
        """mask_point_refine.py:95-132 -> (instance_preds, detail_preds [n, 1, S, S], refined features
        [n, C_out, 2S, 2S]).  ``sem``: relu(semantic_transform_in(semantic_feat)) of the whole map (computed once per call
        by the head); ``instance_feats`` [n, C, S, S] is refined IN PLACE (the reference refines a copy)."""
        n, c, S = instance_feats.shape[0], self.channels, instance_feats.shape[2]
        nc = self.num_classes
        dev = instance_feats.device
        # both logit maps, all classes: the point MLP's coarse inputs
        coarse = torch.empty((n, 2 * nc, S, S), device=dev, dtype=torch.float32)
        self.instance_logits.run(instance_feats, out=coarse, out_ch_offset=0)
        self.detail_logits.run(instance_feats, out=coarse, out_ch_offset=nc)
        # the label rows (the stage predictions and the selection key)
        wi, bi = self.instance_logits.weight.detach().view(nc, c), self.instance_logits.bias.detach()
        wd, bd = self.detail_logits.weight.detach().view(nc, c), self.detail_logits.bias.detach()
        ip, dp = ops.class_logits(instance_feats, wi, bi, wd, bd, roi_labels)
        hw = S * S
        P = min(hw, int(num_points))
        idx = None if P == hw else ops.point_topk_select(dp, P, use_sigmoid=self.mask_use_sigmoid)
        if form is None and not ops.point_refine_mlp_supported(n, c, 2 * nc, P, self.num_fcs, hw, idx is not None):
            form = 'unfused'            # (a width the fused kernel does not take: the 1x1 launch sequence)
        x = ops.point_feat_gather(sem, rois, coarse, idx, 1.0 / float(self.semantic_out_stride))
        wq, bs = self.mlp_params()
        ops.point_refine_mlp(x, c, wq, bs, idx, instance_feats, form=form)
        fused = self.fuse_transform_out.run(instance_feats, relu=True)
        return ip, dp, ops.upsample2x(fused, align_corners=False, relu=True)


@HEADS.register_module()
class PointRefineMaskHead(nn.Module):
    """``PointRefineMaskHead`` -- mmdet/models/roi_heads/mask_heads/mask_point_refine.py:174-402, inference: same
    constructor kwargs and ``state_dict`` keys (in the reference's order) as the reference, so PointRefine checkpoints
    load.  ``forward`` returns (stage_instance_preds, stage_detail_preds, semantic_pred) as the reference.  The config's
    loss, ``PointRefineCrossEntropyLoss``, is registered nowhere in the reference (Quirk Q15): ``loss_cfg`` is stored, not
    built, and training (``get_targets``, ``loss``) raises."""

    def __init__(self, num_convs_instance=2, num_convs_semantic=4, num_fcs=3, conv_in_channels_instance=256,
                 conv_in_channels_semantic=256, conv_kernel_size_instance=3, conv_kernel_size_semantic=3,
                 conv_out_channels_instance=256, conv_out_channels_semantic=256, conv_cfg=None, norm_cfg=None,
                 semantic_out_stride=4, mask_use_sigmoid=False, class_agnostic=False, coarse_pred_each_layer=True,
                 stage_num_classes=[80, 80, 80, 80], stage_sup_size=[14, 28, 56, 112],
                 upsample_cfg=dict(type='bilinear', scale_factor=2),
                 loss_cfg=dict(type='RefineCrossEntropyLoss', stage_instance_loss_weight=[0.25, 0.5, 0.75, 1.0],
                               semantic_loss_weight=1.0, boundary_width=2, start_stage=1)):
        super().__init__()
        self.num_convs_instance = num_convs_instance
        self.conv_kernel_size_instance = conv_kernel_size_instance
        self.conv_in_channels_instance = conv_in_channels_instance
        self.conv_out_channels_instance = conv_out_channels_instance
        self.num_convs_semantic = num_convs_semantic
        self.conv_kernel_size_semantic = conv_kernel_size_semantic
        self.conv_in_channels_semantic = conv_in_channels_semantic
        self.conv_out_channels_semantic = conv_out_channels_semantic
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.semantic_out_stride = semantic_out_stride
        self.stage_sup_size = stage_sup_size
        self.stage_num_classes = stage_num_classes
        self.mask_use_sigmoid = mask_use_sigmoid
        self.num_fcs = num_fcs
        self.loss_cfg = loss_cfg                 # (not built: Quirk Q15)
        if conv_kernel_size_semantic != 3:
            raise NotImplementedError('the semantic convs are 3x3 in configs/point_refine')
        if class_agnostic or any(k == 1 for k in stage_num_classes):
            raise NotImplementedError('PointRefineMaskHead: class_agnostic=False with per-class logits only '
                                      '(configs/point_refine)')

        convs = []
        for i in range(num_convs_instance):
            cin = conv_in_channels_instance if i == 0 else conv_out_channels_instance
            convs.append(ConvModule(cin, conv_out_channels_instance, conv_kernel_size_instance, dilation=1, padding=1))
        self.instance_convs = nn.ModuleList(convs)
        convs = []
        for i in range(num_convs_semantic):
            cin = conv_in_channels_semantic if i == 0 else conv_out_channels_semantic
            convs.append(DilatedConvModule(cin, conv_out_channels_semantic, 3, padding=1, dilation=1))
        self.semantic_convs = nn.ModuleList(convs)

        assert len(self.stage_sup_size) > 1
        self.stages = nn.ModuleList()
        out_channel = conv_out_channels_instance
        for idx, out_size in enumerate(self.stage_sup_size[:-1]):
            in_channel = out_channel
            out_channel = in_channel // 2
            if in_channel % 2 != 0:
                raise NotImplementedError(f'PointRefineMaskHead: stage {idx} width {in_channel} is odd')
            self.stages.append(PointRefineSFMStage(
                semantic_in_channel=conv_out_channels_semantic, semantic_out_channel=in_channel, fc_in_channels=in_channel,
                fc_channels=in_channel, fc_out_channels=out_channel, num_fcs=num_fcs, num_classes=self.stage_num_classes[idx],
                semantic_out_stride=semantic_out_stride, mask_use_sigmoid=mask_use_sigmoid, class_agnostic=class_agnostic,
                coarse_pred_each_layer=coarse_pred_each_layer, upsample_cfg=upsample_cfg))
        if len(self.stages) > 3:
            raise NotImplementedError('PointRefineMaskHead: at most three SFM stages (one grouped semantic 1x1 launch)')
        self.final_instance_logits = _Conv(out_channel, self.stage_num_classes[-1], 1)
        self.final_detail_logits = _Conv(out_channel, self.stage_num_classes[-1], 1)
        self.semantic_logits = _Conv(conv_out_channels_semantic, 1, 1)

    def init_weights(self):
        for m in [self.final_instance_logits, self.final_detail_logits, self.semantic_logits]:
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)

    def semantic_forward(self, semantic_feat):
        """The four 3x3 semantic convs on the whole stride-4 map (once per call, every image of the batch), then the
        stages' relu(semantic_transform_in) as ONE grouped 1x1 launch -> (semantic features, [sem per stage])."""
        for conv in self.semantic_convs:
            semantic_feat = conv(semantic_feat)
        ts = [st.semantic_transform_in for st in self.stages]
        prec = ts[0].precision_for(semantic_feat.shape[2], semantic_feat.shape[3])
        sems = ops.conv1x1_group([semantic_feat] * len(ts), [t.packed([t.in_channels], prec) for t in ts],
                                 [t.bias.detach() for t in ts], [t.out_channels for t in ts], relu=True)
        return semantic_feat, sems

    def forward(self, instance_feats, semantic_feat, rois, roi_labels, cfg, semantic_pred=True, form=None):
        """mask_point_refine.py:288-313 -> (stage_instance_preds, stage_detail_preds [n, 1, S_k, S_k] per stage,
        semantic_pred [B, 1, H, W] or None when ``semantic_pred`` is False: test time does not read it).
        ``cfg.num_points``: the points per stage.  ``form``: the point MLP's form (ops.point_refine_mlp)."""
        for conv in self.instance_convs:
            instance_feats = conv(instance_feats)
        semantic_feat, sems = self.semantic_forward(semantic_feat)
        sem_pred = self.semantic_logits.run(semantic_feat) if semantic_pred else None
        roi_labels = roi_labels.long().contiguous()
        rois = rois.contiguous()
        num_points = int(cfg.num_points)
        ips, dps = [], []
        for stage, sem in zip(self.stages, sems):
            ip, dp, instance_feats = stage(instance_feats, sem, rois, roi_labels, num_points, form=form)
            ips.append(ip)
            dps.append(dp)
        nc = self.stage_num_classes[-1]
        c = self.final_instance_logits.in_channels
        fi, fd = self.final_instance_logits, self.final_detail_logits
        ip, dp = ops.class_logits(instance_feats, fi.weight.detach().view(nc, c), fi.bias.detach(),
                                  fd.weight.detach().view(nc, c), fd.bias.detach(), roi_labels)
        ips.append(ip)
        dps.append(dp)
        return ips, dps, sem_pred

    # mask_point_refine.py:350-402 = dynamask_head.py:279-342 (sigmoid, paste, threshold)
    get_seg_masks = DynaMaskHead.get_seg_masks
    get_seg_rles = DynaMaskHead.get_seg_rles

    def get_targets(self, *a, **k):
        raise NotImplementedError('PointRefineMaskHead.get_targets: PointRefine training is out of reach -- the config\'s '
                                  'PointRefineCrossEntropyLoss is registered nowhere in the reference (Quirk Q15)')

    def loss(self, *a, **k):
        raise NotImplementedError('PointRefineMaskHead.loss: PointRefineCrossEntropyLoss is registered nowhere in the '
                                  'reference (Quirk Q15)')


# ---------------------------------------------------------------- Mask Scoring R-CNN: MaskIoUHead (inference)
@HEADS.register_module()
class MaskIoUHead(nn.Module):
    """``MaskIoUHead`` -- mmdet/models/roi_heads/mask_heads/maskiou_head.py, inference: the IoU of a detection's mask
    predicted from the RoI features and the mask head's prediction.  ``convs.{i}`` (3x3, stride 2 on the last),
    ``fcs.{i}`` and ``fc_mask_iou`` carry the reference's ``state_dict`` keys.  The first conv reads two sources,
    ``[mask_feat, max_pool2x2(sigmoid(mask_pred[label]))]`` (ops.mask_iou_input), with no concatenation; the stride-1
    convs run on conv_igemm through ``_Conv.run`` (they follow ``set_conv_precision``), the stride-2 conv on
    ops.conv3x3_s2 (exact fp32 in every mode), the fully connected layers on dm_fc_fwd.  ``get_targets`` / ``loss`` are
    reachable only past the fork's broken mask loss (Quirk Q5): they raise."""

    def __init__(self, num_convs=4, num_fcs=2, roi_feat_size=14, in_channels=256, conv_out_channels=256,
                 fc_out_channels=1024, num_classes=80, loss_iou=dict(type='MSELoss', loss_weight=0.5)):
        super().__init__()
        if num_convs < 2:
            raise NotImplementedError('MaskIoUHead: num_convs >= 2 (the stride-2 conv reads one source; configs/ms_rcnn: 4)')
        if num_fcs < 1:
            raise NotImplementedError('MaskIoUHead: num_fcs >= 1 (configs/ms_rcnn: 2)')
        if conv_out_channels % 8 != 0:
            raise NotImplementedError('MaskIoUHead: conv_out_channels a multiple of 8 (configs/ms_rcnn: 256)')
        roi = (roi_feat_size, roi_feat_size) if isinstance(roi_feat_size, int) else tuple(roi_feat_size)
        if roi[0] % 2 or roi[1] % 2:
            raise NotImplementedError('MaskIoUHead: an even roi_feat_size (the pooled mask and the stride-2 output '
                                      'must both be roi_feat_size / 2; configs/ms_rcnn: 14)')
        self.in_channels = in_channels
        self.conv_out_channels = conv_out_channels
        self.fc_out_channels = fc_out_channels
        self.num_classes = num_classes
        self.roi_feat_size = roi
        self.convs = nn.ModuleList()
        for i in range(num_convs):
            self.convs.append(_Conv(in_channels + 1 if i == 0 else conv_out_channels, conv_out_channels, 3))
        pooled_area = (roi[0] // 2) * (roi[1] // 2)
        self.fcs = nn.ModuleList()
        for i in range(num_fcs):
            self.fcs.append(nn.Linear(conv_out_channels * pooled_area if i == 0 else fc_out_channels, fc_out_channels))
        self.fc_mask_iou = nn.Linear(fc_out_channels, num_classes)
        self.loss_iou = build_loss(loss_iou)

    def init_weights(self):
        """maskiou_head.py:67-77."""
        for conv in self.convs:
            nn.init.kaiming_normal_(conv.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(conv.bias, 0)
        for fc in self.fcs:
            nn.init.kaiming_uniform_(fc.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
            nn.init.constant_(fc.bias, 0)
        nn.init.normal_(self.fc_mask_iou.weight, 0, 0.01)
        nn.init.constant_(self.fc_mask_iou.bias, 0)

    def forward(self, mask_feat, mask_pred, labels=None):
        """maskiou_head.py:79-91 -> mask_iou [n, num_classes].  ``mask_pred``: the reference's [n, S, S] (the label
        channel already selected), or the mask head's [n, C, S, S] logits with ``labels`` [n] (C == 1: class-agnostic),
        whose label channel ops.mask_iou_input selects in the same launch as the sigmoid and the 2 x 2 max pool."""
        if torch.is_grad_enabled() and mask_feat.requires_grad:
            raise NotImplementedError('MaskIoUHead: training is unreachable in the reference fork (Quirk Q5)')
        with torch.no_grad():
            return self._forward(mask_feat, mask_pred, labels)

    def _forward(self, mask_feat, mask_pred, labels):
        if mask_pred.dim() == 3:
            mask_pred, labels = mask_pred[:, None], None
        n = mask_feat.shape[0]
        if n == 0:
            return mask_feat.new_zeros((0, self.num_classes))
        labels = None if labels is None else labels.to(torch.int64).contiguous()
        pooled = ops.mask_iou_input(mask_pred.contiguous(), labels)
        x = [mask_feat.contiguous(), pooled]
        with ops.splitk_scope():            # inference on <= 100 RoIs: the 14 x 14 launches may split their K loop
            for conv in self.convs[:-1]:
                x = conv.run(x, relu=True)
            last = self.convs[-1]
            x = ops.conv3x3_s2(x, last.packed(), last.bias.detach(), last.out_channels, relu=True)
        x = x.reshape(n, -1)
        for fc in self.fcs:
            x = ops.fc(x, fc.weight.detach(), fc.bias.detach(), relu=True)
        return ops.fc(x, self.fc_mask_iou.weight.detach(), self.fc_mask_iou.bias.detach())

    def get_mask_scores(self, mask_iou_pred, det_bboxes, det_labels):
        """maskiou_head.py:171-181: mask_score = mask_iou[label] * bbox_score -> per-class lists (numpy float32) in
        detection order."""
        labels = det_labels.to(torch.int64).contiguous()
        scores = ops.mask_iou_scores(mask_iou_pred.contiguous(), labels, det_bboxes.contiguous())
        scores_h, labels_h = _to_host(scores, labels)
        return group_mask_scores(scores_h, labels_h, self.num_classes)

    def get_targets(self, *a, **k):
        raise NotImplementedError('MaskIoUHead.get_targets: Mask Scoring R-CNN training is unreachable in the reference '
                                  'fork (FCNMaskHead.loss is broken before it, Quirk Q5)')

    def loss(self, *a, **k):
        raise NotImplementedError('MaskIoUHead.loss: Mask Scoring R-CNN training is unreachable in the reference fork '
                                  '(FCNMaskHead.loss is broken before it, Quirk Q5)')


@HEADS.register_module()
class HTCMaskHead(FCNMaskHead):
    """htc_mask_head.py:8-43: FCNMaskHead whose input may carry the previous cascade stage's features (mask information
    flow): ``x + relu(conv_res(res_feat))`` in front of the convs, and the features after the convs handed on.  ``conv_res``
    and the add are ONE launch (ops.conv1x1_post_add: the addend joins after the ReLU; ``x`` is left as it was for the next
    stage), always the exact fp32 kernel.  Inference only (the fork's ``FCNMaskHead.loss`` is broken: Quirk Q5)."""

    def __init__(self, with_conv_res=True, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.with_conv_res = with_conv_res
        if self.with_conv_res:
            self.conv_res = ConvModule(self.conv_out_channels, self.conv_out_channels, 1)

    def res_feat(self, x, res_feat=None):
        """The features after the convs (htc_mask_head.py:27-33): what the next stage's ``conv_res`` and this stage's
        upsample read."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('HTCMaskHead is inference only (run under torch.no_grad()): its loss is '
                                      'FCNMaskHead.loss, which the reference fork broke (Quirk Q5)')
        if res_feat is not None:
            assert self.with_conv_res
            c = self.conv_res.conv
            x = ops.conv1x1_post_add(res_feat, c.packed([res_feat.shape[1]]), c.bias.detach(), c.out_channels, x, relu=True)
        for conv in self.convs:
            x = conv(x)
        return x

    def logits(self, res_feat):
        """htc_mask_head.py:36-40."""
        x = res_feat
        if self.upsample is not None:
            x = self.upsample(x, relu=(self.upsample_method == 'deconv'))
        return self.conv_logits.run(x)

    def forward(self, x, res_feat=None, return_logits=True, return_feat=True):
        res_feat = self.res_feat(x, res_feat)
        outs = []
        if return_logits:
            outs.append(self.logits(res_feat))
        if return_feat:
            outs.append(res_feat)
        return outs if len(outs) > 1 else outs[0]


@HEADS.register_module()
class FusedSemanticHead(nn.Module):
    """fused_semantic_head.py:9-107 for inference: every FPN level resized to the fusion level's size
    (``align_corners=True``), a 1x1 lateral conv + ReLU each, summed -- the fusion level first, then the others in
    ascending order, each as ``x += relu(conv1x1(resize(feat)))`` --, ``num_convs`` 3x3 convs and the 1x1 embedding.
    ``forward(feats)`` returns the embedded feature [B, conv_out_channels, H, W] of the B images of ``feats``; the
    ``num_classes`` segmentation logits (``conv_logits``) are a training output and are not computed, their weights stay
    in the ``state_dict``.  HIP: ops.resize_bilinear per level, the lateral conv and the add in one launch
    (ops.conv1x1_post_add, in place into the sum), the 3x3 convs on the any-width kernel (ops.conv3x3_dil, dilation 1: a
    100 x 168 map is wider than the tiles of ops.conv2d's 3x3 build stage), the embedding through ops.conv2d."""

    def __init__(self, num_ins, fusion_level, num_convs=4, in_channels=256, conv_out_channels=256, num_classes=183,
                 ignore_label=255, loss_weight=0.2, conv_cfg=None, norm_cfg=None):
        super().__init__()
        if not 0 <= fusion_level < num_ins:
            raise ValueError(f'fusion_level {fusion_level} of {num_ins} inputs')
        self.num_ins = num_ins
        self.fusion_level = fusion_level
        self.num_convs = num_convs
        self.in_channels = in_channels
        self.conv_out_channels = conv_out_channels
        self.num_classes = num_classes
        self.ignore_label = ignore_label
        self.loss_weight = loss_weight
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        self.fp16_enabled = False
        # (ConvModule raises NotImplementedError for a conv_cfg / norm_cfg other than None)
        self.lateral_convs = nn.ModuleList([ConvModule(in_channels, in_channels, 1, conv_cfg=conv_cfg, norm_cfg=norm_cfg)
                                            for _ in range(num_ins)])
        # (the 3x3 convs see the whole stride-8 map: the any-width kernel, as RefineMask's and PointRefine's semantic convs)
        self.convs = nn.ModuleList([DilatedConvModule(in_channels if i == 0 else conv_out_channels, conv_out_channels, 3,
                                                      padding=1, dilation=1, conv_cfg=conv_cfg, norm_cfg=norm_cfg)
                                    for i in range(num_convs)])
        self.conv_embedding = ConvModule(conv_out_channels, conv_out_channels, 1, conv_cfg=conv_cfg, norm_cfg=norm_cfg)
        self.conv_logits = _Conv(conv_out_channels, num_classes, 1)

    def init_weights(self):
        nn.init.kaiming_normal_(self.conv_logits.weight, mode='fan_out', nonlinearity='relu')
        nn.init.constant_(self.conv_logits.bias, 0)

    @torch.no_grad()
    def forward(self, feats):
        feats = list(feats)
        if len(feats) != self.num_ins:
            raise ValueError(f'FusedSemanticHead: {self.num_ins} feature maps expected, got {len(feats)}')
        x = self.lateral_convs[self.fusion_level](feats[self.fusion_level].contiguous())
        size = tuple(x.shape[-2:])
        for i, feat in enumerate(feats):
            if i == self.fusion_level:
                continue
            c = self.lateral_convs[i].conv
            r = ops.resize_bilinear(feat.contiguous(), size)
            ops.conv1x1_post_add(r, c.packed([r.shape[1]]), c.bias.detach(), c.out_channels, x, relu=True, out=x)
        for conv in self.convs:
            x = conv(x)
        return self.conv_embedding(x)

    def loss(self, mask_pred, labels):
        raise NotImplementedError('FusedSemanticHead: the semantic segmentation loss is training (HTC is inference only here)')


# ---------------------------------------------------------------- Grid R-CNN head (inference)
def grid_sub_regions(grid_points, whole_map_size):
    """grid_head.py:189-218 (calc_sub_regions), restated with its ``int(...)`` truncations: per point the
    (x1, y1, x2, y2) of its half-sized region of the ``whole_map_size`` map."""
    grid_size = int(math.sqrt(grid_points))
    half_size = whole_map_size // 4 * 2
    sub_regions = []
    for i in range(grid_points):
        x_idx = i // grid_size
        y_idx = i % grid_size
        if x_idx == 0:
            sub_x1 = 0
        elif x_idx == grid_size - 1:
            sub_x1 = half_size
        else:
            ratio = x_idx / (grid_size - 1) - 0.25
            sub_x1 = max(int(ratio * whole_map_size), 0)
        if y_idx == 0:
            sub_y1 = 0
        elif y_idx == grid_size - 1:
            sub_y1 = half_size
        else:
            ratio = y_idx / (grid_size - 1) - 0.25
            sub_y1 = max(int(ratio * whole_map_size), 0)
        sub_regions.append((sub_x1, sub_y1, sub_x1 + half_size, sub_y1 + half_size))
    return sub_regions


class _GroupNorm(nn.Module):
    """Parameter holder named like nn.GroupNorm (weight, bias [C]); the normalisation is ops.group_norm."""

    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__()
        if num_channels % num_groups != 0:
            raise ValueError(f'GroupNorm: {num_channels} channels do not split into {num_groups} groups')
        self.num_groups, self.num_channels, self.eps = num_groups, num_channels, eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def run_(self, x, relu=False):
        """In place."""
        return ops.group_norm(x, self.weight.detach(), self.bias.detach(), self.num_groups, self.eps, relu=relu, out=x)


class GNConvModule(nn.Module):
    """mmcv ConvModule with ``norm_cfg=dict(type='GN', num_groups=G)``: 3x3 conv (bias) -> GroupNorm -> ReLU, keys
    ``conv.weight / conv.bias / gn.weight / gn.bias``.  Stride 1 runs on ops.conv2d (conv_igemm), stride 2 on
    ops.conv3x3_s2, both always on the exact fp32 layout with one fixed association of the K sum (no split-K: a RoI's
    bits do not depend on how many RoIs share the call); the norm and the ReLU are one in-place ops.group_norm.
    (``ConvModule`` above stays the norm-free class: it refuses ``norm_cfg``.)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type='ReLU'), bias=True):
        super().__init__()
        if conv_cfg is not None:
            raise NotImplementedError('GNConvModule: conv_cfg is None in configs/grid_rcnn')
        if not isinstance(norm_cfg, dict) or norm_cfg.get('type') != 'GN' or set(norm_cfg) - {'type', 'num_groups', 'requires_grad'}:
            raise NotImplementedError('GNConvModule: norm_cfg=dict(type="GN", num_groups=G) only')
        if kernel_size != 3 or padding != 1 or stride not in (1, 2) or not bias:
            raise NotImplementedError('GNConvModule: 3x3 convolutions with padding 1, stride 1 or 2 and a bias only')
        if in_channels % 8 != 0:
            raise NotImplementedError('GNConvModule: in_channels a multiple of 8 (the 3x3 kernels\' K chunk)')
        self.stride = stride
        self.conv = _Conv(in_channels, out_channels, 3)
        self.conv.exact = True
        self.gn = _GroupNorm(norm_cfg['num_groups'], out_channels)
        self.with_activation = act_cfg is not None

    def forward(self, x):
        conv = self.conv
        if self.stride == 2:
            if not ops.conv3x3_s2_supported(x, conv.out_channels, 1):
                raise NotImplementedError(f'GNConvModule: no stride-2 kernel for {tuple(x.shape)} -> {conv.out_channels}')
            y = ops.conv3x3_s2(x, conv.packed(), conv.bias.detach(), conv.out_channels, relu=False, splits=1)
        else:
            y = ops.conv2d([x], conv.packed(), conv.bias.detach(), conv.out_channels, 3, relu=False)
        return self.gn.run_(y, relu=self.with_activation)


class _GridTransition(nn.Sequential):
    """One transition of the neighbour fusion, keys ``0.*`` (depthwise 5x5) and ``1.*`` (1x1) as the reference's
    nn.Sequential(nn.Conv2d(c, c, 5, padding=2, groups=c), nn.Conv2d(c, c, 1)); parameters only -- all transitions of an
    order run in one ops.grid_fusion launch."""

    def __init__(self, channels):
        dw, pw = nn.Module(), nn.Module()
        dw.weight = nn.Parameter(torch.empty(channels, 1, 5, 5))
        dw.bias = nn.Parameter(torch.zeros(channels))
        pw.weight = nn.Parameter(torch.empty(channels, channels, 1, 1))
        pw.bias = nn.Parameter(torch.zeros(channels))
        nn.init.kaiming_normal_(dw.weight, mode='fan_out', nonlinearity='relu')
        nn.init.kaiming_normal_(pw.weight, mode='fan_out', nonlinearity='relu')
        super().__init__(dw, pw)

    def forward(self, x):
        raise NotImplementedError('a transition does not run alone: GridHead fuses all of an order in one launch')


class _GroupedDeconv(nn.Module):
    """Parameter holder named like nn.ConvTranspose2d(cin, cout, 4, stride=2, padding=1, groups=g): weight
    [cin, cout / g, 4, 4], bias [cout]; runs on ops.deconv4x4_s2_grouped, which reads torch's layout as it is."""

    def __init__(self, in_channels, out_channels, groups):
        super().__init__()
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels // groups, 4, 4))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.normal_(self.weight, 0, 0.001)

    def run(self, x):
        if not ops.deconv4x4_s2_grouped_supported(x, self.out_channels, self.groups):
            raise NotImplementedError(f'grouped deconv: no kernel for {tuple(x.shape)} -> {self.out_channels} '
                                      f'in {self.groups} groups')
        return ops.deconv4x4_s2_grouped(x, self.weight.detach(), self.bias.detach(), self.groups)


@HEADS.register_module()
class GridHead(nn.Module):
    """``GridHead`` -- mmdet/models/roi_heads/mask_heads/grid_head.py, inference (:13-187, :189-218, :294-359): per RoI
    the heatmaps of ``grid_points`` grid points, from which ``get_bboxes`` votes the refined box.  The reference's
    constructor arguments and ``state_dict`` keys: ``convs.{i}.conv / .gn``, ``deconv1``, ``norm1``, ``deconv2``,
    ``forder_trans.{i}.{j}.{0,1}`` and ``sorder_trans.{i}.{j}.{0,1}`` (j in the reference's neighbour order left, up, down,
    right).  The launches: conv 0 on ops.conv3x3_s2, convs 1.. on ops.conv2d, GroupNorm + ReLU in place after each, one
    ops.grid_fusion per fusion order (the 48 transitions of an order in one launch, their weights in one packed table per
    weight version), ops.deconv4x4_s2_grouped twice, ops.grid_get_bboxes.  Everything is exact fp32 whatever
    ``set_conv_precision`` says.  What the kernels were not run on is refused here."""

    def __init__(self, grid_points=9, num_convs=8, roi_feat_size=14, in_channels=256, conv_kernel_size=3,
                 point_feat_channels=64, deconv_kernel_size=4, class_agnostic=False,
                 loss_grid=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=15), conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=36)):
        super().__init__()
        if grid_points < 4:
            raise ValueError('grid_points >= 4')
        grid_size = int(math.sqrt(grid_points))
        if grid_size * grid_size != grid_points:
            raise ValueError('grid_points must be a square number')
        if not isinstance(roi_feat_size, int):
            raise ValueError('Only square RoIs are supporeted in Grid R-CNN')
        if grid_points != 9:
            raise NotImplementedError('GridHead: grid_points=9 only (configs/grid_rcnn)')
        if point_feat_channels != 64:
            raise NotImplementedError('GridHead: point_feat_channels=64 only (configs/grid_rcnn; the fusion kernel\'s width)')
        if roi_feat_size != 14:
            raise NotImplementedError('GridHead: roi_feat_size=14 only (7 x 7 maps inside the head, 28 x 28 heatmaps)')
        if conv_kernel_size != 3 or deconv_kernel_size != 4:
            raise NotImplementedError('GridHead: conv_kernel_size=3 and deconv_kernel_size=4 only (configs/grid_rcnn)')
        if num_convs < 1:
            raise NotImplementedError('GridHead: num_convs >= 1 (the first convolution is the stride-2 one)')
        if in_channels % 8 != 0:
            raise NotImplementedError('GridHead: in_channels a multiple of 8 (configs/grid_rcnn: 256)')
        if conv_cfg is not None:
            raise NotImplementedError('GridHead: conv_cfg is None in configs/grid_rcnn')
        self.grid_points = grid_points
        self.num_convs = num_convs
        self.roi_feat_size = roi_feat_size
        self.in_channels = in_channels
        self.conv_kernel_size = conv_kernel_size
        self.point_feat_channels = point_feat_channels
        self.conv_out_channels = point_feat_channels * grid_points
        self.class_agnostic = class_agnostic
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        if not isinstance(norm_cfg, dict) or norm_cfg.get('type') != 'GN':
            raise NotImplementedError('GridHead: norm_cfg=dict(type="GN", num_groups=G) only (configs/grid_rcnn)')
        if self.conv_out_channels % norm_cfg['num_groups'] != 0:
            raise ValueError(f'GridHead: {self.conv_out_channels} channels do not split into {norm_cfg["num_groups"]} groups')
        self.grid_size = grid_size
        self.whole_map_size = roi_feat_size * 4
        self.sub_regions = self.calc_sub_regions()
        self.convs = nn.Sequential(*[
            GNConvModule(in_channels if i == 0 else self.conv_out_channels, self.conv_out_channels, 3,
                         stride=2 if i == 0 else 1, padding=1, norm_cfg=norm_cfg) for i in range(num_convs)])
        self.deconv1 = _GroupedDeconv(self.conv_out_channels, self.conv_out_channels, grid_points)
        self.norm1 = _GroupNorm(grid_points, self.conv_out_channels)
        self.deconv2 = _GroupedDeconv(self.conv_out_channels, grid_points, grid_points)
        self.neighbor_points = ops.grid_neighbors(grid_points)
        self.num_edges = sum(len(p) for p in self.neighbor_points)
        self.forder_trans = nn.ModuleList()
        self.sorder_trans = nn.ModuleList()
        for neighbors in self.neighbor_points:
            self.forder_trans.append(nn.ModuleList([_GridTransition(point_feat_channels) for _ in neighbors]))
            self.sorder_trans.append(nn.ModuleList([_GridTransition(point_feat_channels) for _ in neighbors]))
        self.loss_grid = build_loss(loss_grid)
        self._pk = _Packed()

    def init_weights(self):
        """grid_head.py:141-149."""
        for m in self.modules():
            if isinstance(m, (_Conv, _GridTransition)):
                for p in ([m.weight] if isinstance(m, _Conv) else [m[0].weight, m[1].weight]):
                    nn.init.kaiming_normal_(p, mode='fan_out', nonlinearity='relu')
                for b in ([m.bias] if isinstance(m, _Conv) else [m[0].bias, m[1].bias]):
                    nn.init.constant_(b, 0)
        for m in (self.deconv1, self.deconv2):
            nn.init.normal_(m.weight, 0, 0.001)
            nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.deconv2.bias, -math.log(0.99 / 0.01))

    def calc_sub_regions(self):
        """grid_head.py:189-218."""
        return grid_sub_regions(self.grid_points, self.whole_map_size)

    def _fusion_table(self, name):
        """The packed table of one fusion order, rebuilt when any of its parameters changes (``_Packed.get_multi``)."""
        trans = getattr(self, name)

        def pack():
            slots = [[(t[0].weight, t[0].bias, t[1].weight, t[1].bias) for t in point] for point in trans]
            return ops.pack_grid_fusion_table(slots, self.grid_points, self.point_feat_channels)
        return self._pk.get_multi(name, [p for t in trans for p in t.parameters()], pack)

    def forward(self, x):
        """grid_head.py:151-187 in eval mode -> ``dict(fused=heatmap [n, P, 28, 28], unfused=the same tensor)``."""
        if self.training or (torch.is_grad_enabled() and x.requires_grad):
            raise NotImplementedError('GridHead: training (the unfused branch, get_targets, the loss) is the follow-up to '
                                      'inference; call it in eval mode under torch.no_grad()')
        if x.dim() != 4 or x.shape[1] != self.in_channels or x.shape[-1] != self.roi_feat_size or \
                x.shape[-2] != self.roi_feat_size:
            raise ValueError(f'GridHead: RoI features [n, {self.in_channels}, {self.roi_feat_size}, {self.roi_feat_size}] '
                             f'expected, got {list(x.shape)}')
        half = self.whole_map_size // 4 * 2
        if x.shape[0] == 0:
            heat = x.new_zeros((0, self.grid_points, half, half))
            return dict(fused=heat, unfused=heat)
        with torch.no_grad():
            x = self.convs(x.contiguous())
            if not ops.grid_fusion_supported(x, self.grid_points):
                raise NotImplementedError(f'GridHead: no fusion kernel for {tuple(x.shape)}')
            x_fo = ops.grid_fusion(x, x, self._fusion_table('forder_trans'), self.grid_points)
            x_so = ops.grid_fusion(x, x_fo, self._fusion_table('sorder_trans'), self.grid_points)
            x2 = self.norm1.run_(self.deconv1.run(x_so), relu=True)
            heat = self.deconv2.run(x2)
        return dict(fused=heat, unfused=heat)

    def get_bboxes(self, det_bboxes, grid_pred, img_metas=None):
        """grid_head.py:294-359 on the device (ops.grid_get_bboxes) -> [n, 5], on ``det_bboxes``' device.  The boxes are
        not clipped to the image: the reference's ``clamp_`` works on a copy (Quirk Q21), ``img_metas`` is unread."""
        assert det_bboxes.shape[0] == grid_pred.shape[0]
        half = self.whole_map_size // 4 * 2
        assert grid_pred.shape[1] == self.grid_points and grid_pred.shape[2] == grid_pred.shape[3] == half
        if det_bboxes.shape[0] == 0:
            return det_bboxes.new_zeros((0, 5))
        return ops.grid_get_bboxes(grid_pred.contiguous(), det_bboxes.contiguous(), self.sub_regions)

    def get_targets(self, *a, **k):
        raise NotImplementedError('GridHead.get_targets: Grid R-CNN training is the follow-up to inference')

    def loss(self, *a, **k):
        raise NotImplementedError('GridHead.loss: Grid R-CNN training is the follow-up to inference')
