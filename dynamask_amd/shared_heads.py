"""Shared heads behind the reference's SHARED_HEADS registry: ``ResLayer`` (roi_heads/shared_heads/res_layer.py over
models/utils/res_layer.py and the caffe branch of backbones/resnet.py's ``Bottleneck``), the per-RoI ResNet stage of the C4
configs (configs/_base_/models/{mask,faster}_rcnn_r50_caffe_c4.py), at inference.

Every block is three exact-fp32 ``dm_conv2d_fwd`` launches with eval-mode BatchNorm folded into weights and bias
(layers.fold_bn, float64, rounded once); no split-K, so a RoI's bits do not depend on the RoI count.  With
``style='caffe'`` the stride of the layer sits in two 1x1 convolutions of block 0 (``conv1`` and ``downsample.0``) that read
only the even rows and columns of their input: the layer runs on that subsampled input, which the RoI head extracts
directly (``SingleRoIExtractor.forward(..., bin_step=2)``, dm_roi_align_strided_fwd) instead of extracting four times as
much and slicing."""
import torch
import torch.nn as nn

from .layers import _BASIC_BLOCK_DEPTHS, _STAGE_BLOCKS, Bottleneck
from .registry import SHARED_HEADS


@SHARED_HEADS.register_module()
class ResLayer(nn.Module):
    """``ResLayer`` -- roi_heads/shared_heads/res_layer.py:12-77.  ``state_dict`` keys as the reference's:
    ``layer{stage + 1}.{i}.conv{1,2,3}.weight``, ``.bn{1,2,3}.*`` and ``layer{stage + 1}.0.downsample.{0,1}.*``.
    Block 0 (the downsample block) writes a new tensor, the blocks behind it run in place on that one: the argument of
    ``forward`` / ``forward_sampled`` is never written.  Training is not built."""

    def __init__(self, depth, stage=3, stride=2, dilation=1, style='pytorch', norm_cfg=dict(type='BN', requires_grad=True),
                 norm_eval=True, with_cp=False, dcn=None):
        super().__init__()
        if depth in _BASIC_BLOCK_DEPTHS:
            raise NotImplementedError(f'ResLayer: depth={depth} is a BasicBlock net; the Bottleneck depths 50 / 101 / 152 are built')
        if depth not in _STAGE_BLOCKS:
            raise KeyError(f'invalid depth {depth} for resnet')
        if stride not in (1, 2):
            raise NotImplementedError(f'ResLayer: stride={stride}; 1 and 2 are built')
        if dilation != 1:
            raise NotImplementedError(f'ResLayer: dilation={dilation}; 1 is built')
        if style != 'caffe':
            raise NotImplementedError(f"ResLayer: style={style!r} puts the stride into the 3x3 convolution; 'caffe' (every C4 "
                                      'config of the reference) is built')
        if not isinstance(norm_cfg, dict) or norm_cfg.get('type') != 'BN' or set(norm_cfg) - {'type', 'requires_grad'}:
            raise NotImplementedError(f"ResLayer: norm_cfg={norm_cfg!r}; dict(type='BN') is built (the eval-mode fold is BatchNorm's)")
        if dcn is not None:
            raise NotImplementedError('ResLayer: dcn is None in the C4 configs')
        self.depth, self.stage, self.stride, self.dilation, self.style = depth, stage, stride, dilation, style
        self.norm_cfg, self.norm_eval, self.with_cp = norm_cfg, norm_eval, with_cp      # (with_cp: no effect at inference)
        self.fp16_enabled = False
        planes = 64 * 2 ** stage
        inplanes = 64 * 2 ** (stage - 1) * Bottleneck.expansion
        if planes != int(planes) or inplanes != int(inplanes) or int(planes) % 4 or int(inplanes) % 4:
            raise ValueError(f'ResLayer: stage={stage} gives planes={planes}, inplanes={inplanes}: multiples of 4 expected')
        planes, inplanes = int(planes), int(inplanes)
        self.inplanes, self.planes, self.out_channels = inplanes, planes, planes * Bottleneck.expansion
        blocks = [Bottleneck(inplanes, planes, downsample=True)]
        blocks += [Bottleneck(self.out_channels, planes) for _ in range(1, _STAGE_BLOCKS[depth][stage])]
        self.add_module(f'layer{stage + 1}', nn.Sequential(*blocks))

    @property
    def res_layer(self):
        return getattr(self, f'layer{self.stage + 1}')

    def init_weights(self, pretrained=None):
        """res_layer.py:49-66 without a checkpoint: kaiming convolutions, unit BatchNorm."""
        if pretrained is not None:
            raise NotImplementedError('ResLayer.init_weights: load a checkpoint with load_state_dict')
        for block in self.res_layer:
            for name, m in block.named_modules():
                if hasattr(m, 'running_mean'):
                    nn.init.constant_(m.weight, 1)
                    nn.init.constant_(m.bias, 0)
                elif getattr(m, 'weight', None) is not None and m.weight.dim() == 4:
                    nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def _check(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('ResLayer: training (BatchNorm in train mode, the backward of the layer) is not built; '
                                      'run inference under torch.no_grad()')
        if x.dim() != 4 or x.shape[1] != self.inplanes:
            raise ValueError(f'ResLayer: [N, {self.inplanes}, H, W] features expected, got {tuple(x.shape)}')

    def forward(self, x):
        """res_layer.py:68-72 on the dense RoI features [N, inplanes, H, W] -> [N, 4 planes, ceil(H / stride), ...].  The
        stride is a torch strided copy here (plumbing: the RoI head extracts the subsampled features directly)."""
        self._check(x)
        if self.stride == 2:
            x = x[:, :, ::2, ::2]
        return self.forward_sampled(x.contiguous())

    def forward_sampled(self, x_sub):
        """The layer on the input its strided convolutions read: ``x[:, :, ::stride, ::stride]`` of the dense features,
        [N, inplanes, ceil(H / stride), ceil(W / stride)].  ``x_sub`` is not written."""
        self._check(x_sub)
        if x_sub.shape[0] == 0:         # no RoI: nothing is launched
            return x_sub.new_zeros((0, self.out_channels) + tuple(x_sub.shape[2:]))
        x = x_sub.contiguous()
        for block in self.res_layer:
            x = block(x)
        return x
