"""Backbones behind the reference's BACKBONES registry, at inference: ``ResNet`` (mmdet/models/backbones/resnet.py) --
the image in, the stages the neck (or a C4 head) starts from out.

The stem is two launches: ``ops.conv7x7_s2`` (``dm_conv7x7_s2_fwd``: conv1 with ``bn1`` folded in and the ReLU on) and
``ops.maxpool3x3_s2``.  Every block is ``layers.Bottleneck``'s three launches with eval-mode BatchNorm folded into
weights and bias (``layers.fold_bn``: float64, rounded once): block 0 of a stage closes with ONE two-source 1x1
convolution of [conv2 output, identity input] into a new tensor, the blocks behind it run in place on that tensor.  A
stride of 2 sits, with ``style='caffe'``, in the two 1x1 convolutions of block 0 -- the block runs on
``ops.subsample2(x)`` -- and, with ``style='pytorch'``, in conv2 (``ops.conv3x3_s2``), the identity input of the closing
launch being ``ops.subsample2(x)``.  The stride-1 3x3 convolutions are ``ops.conv2d`` launches, ``ops.conv3x3_dil`` at
dilation 1 on maps wider than ``layers.CONV2D_3X3_MAX_WIDTH``: the width alone decides.  Every launch is exact fp32 in
every precision mode and none splits its K loop, so an image's bits do not depend on the other images of the call.  The
host never waits; the image is not written.

``ResNeXt`` (mmdet/models/backbones/resnext.py) is ``ResNet`` whose blocks run conv2 in ``groups`` groups: one
``ops.conv3x3_grouped`` launch (``dm_conv3x3_grouped_fwd``, stride 1 or 2) in place of the dense 3x3, at any map width.

``Res2Net`` (mmdet/models/backbones/res2net.py) is ``ResNet`` with the deep stem (``DeepStem``: ``ops.conv3x3_s2_c3``, two
``ops.conv3x3_dil`` and the max-pool), ``layers.Bottle2neck`` blocks -- the 3x3 convolutions on channel slices are
``ops.conv3x3_slices`` launches (``dm_conv3x3_slices_fwd``) -- and ``ops.avgpool2x2_ceil`` in the downsample path."""
import torch
import torch.nn as nn

from . import ops
from .layers import _BASIC_BLOCK_DEPTHS, _BN, _STAGE_BLOCKS, CONV2D_3X3_MAX_WIDTH, Bottle2neck, Bottleneck, _conv_weight, _FoldedConv
from .registry import BACKBONES


class _FoldedStem(_FoldedConv):
    """conv1 + bn1 folded, in ``ops.conv7x7_s2``'s layout."""

    def packed(self):
        def make():
            w, b = self.folded()
            return ops.pack_conv7x7_weight(w), b
        return self._pk.get_multi('pack7', self._tensors(), make)


@BACKBONES.register_module()
class ResNet(nn.Module):
    """``ResNet`` -- backbones/resnet.py:303-639, inference.  ``state_dict`` keys as the reference's: ``conv1.weight``,
    ``bn1.*``, ``layer{1..4}.{i}.conv{1,2,3}.weight``, ``.bn{1,2,3}.*``, ``.downsample.{0,1}.*``.  The Bottleneck depths
    (50 / 101 / 152) in both styles are built; BasicBlock depths, ``deep_stem``, ``avg_down``, DCN stages, plugins,
    ``conv_cfg``, norms other than BN, dilations and training are not.  BatchNorm is always evaluated from its running
    statistics: ``train()``, ``norm_eval`` and ``frozen_stages`` are kept (the latter also clears ``requires_grad`` as the
    reference does) and change nothing in ``forward``."""

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False,
                 frozen_stages=-1, conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True):
        super().__init__()
        if depth not in _STAGE_BLOCKS and depth not in _BASIC_BLOCK_DEPTHS:
            raise KeyError(f'invalid depth {depth} for resnet')
        self.depth = depth
        if stem_channels is None:
            stem_channels = base_channels
        self.stem_channels, self.base_channels, self.num_stages = stem_channels, base_channels, num_stages
        assert num_stages >= 1 and num_stages <= 4
        self.strides, self.dilations = strides, dilations
        assert len(strides) == len(dilations) == num_stages
        self.out_indices = out_indices
        assert max(out_indices) < num_stages
        self.style, self.deep_stem, self.avg_down, self.frozen_stages = style, deep_stem, avg_down, frozen_stages
        self.conv_cfg, self.norm_cfg, self.with_cp, self.norm_eval = conv_cfg, norm_cfg, with_cp, norm_eval
        self.dcn, self.stage_with_dcn = dcn, stage_with_dcn
        if dcn is not None:
            assert len(stage_with_dcn) == num_stages
        self.plugins, self.zero_init_residual = plugins, zero_init_residual
        self.fp16_enabled = False

        if depth in _BASIC_BLOCK_DEPTHS:
            raise NotImplementedError(f'ResNet: depth={depth} is a BasicBlock net; the Bottleneck depths 50 / 101 / 152 are built')
        if style not in ('pytorch', 'caffe'):
            raise ValueError(f"ResNet: style={style!r}; 'pytorch' or 'caffe'")
        self._check_stem_form()
        if dcn is not None:
            raise NotImplementedError(f'ResNet: dcn={dcn} (deformable conv2 in the stages) is not built')
        if plugins is not None:
            raise NotImplementedError(f'ResNet: plugins={plugins} are not built')
        if conv_cfg is not None:
            raise NotImplementedError(f'ResNet: conv_cfg={conv_cfg} is not built (None: nn.Conv2d)')
        if not isinstance(norm_cfg, dict) or norm_cfg.get('type') != 'BN' or set(norm_cfg) - {'type', 'requires_grad'}:
            raise NotImplementedError(f"ResNet: norm_cfg={norm_cfg!r}; dict(type='BN') is built (the eval-mode fold is BatchNorm's)")
        if any(d != 1 for d in dilations):
            raise NotImplementedError(f'ResNet: dilations={tuple(dilations)}; 1 in every stage is built')
        if any(s not in (1, 2) for s in strides):
            raise NotImplementedError(f'ResNet: strides={tuple(strides)}; 1 and 2 are built')
        if base_channels % 8 != 0:
            raise NotImplementedError(f'ResNet: base_channels={base_channels} is not a multiple of 8 (the any-width and the '
                                      'stride-2 3x3 kernels walk the input channels in chunks of 8)')

        self.stage_blocks = _STAGE_BLOCKS[depth][:num_stages]
        self.in_channels = in_channels
        self._make_stem(in_channels, stem_channels)

        self.res_layers = []
        inplanes = stem_channels
        for i, num_blocks in enumerate(self.stage_blocks):
            planes = base_channels * 2 ** i
            out = planes * Bottleneck.expansion
            blocks = self._make_stage(inplanes, planes, num_blocks, strides[i])
            inplanes = out
            name = f'layer{i + 1}'
            self.add_module(name, nn.Sequential(*blocks))
            self.res_layers.append(name)
        self.feat_dim = Bottleneck.expansion * base_channels * 2 ** (len(self.stage_blocks) - 1)

        if not norm_cfg.get('requires_grad', True):          # build_norm_layer: the norm's parameters
            for m in self.modules():
                if isinstance(m, _BN):
                    for p in m.parameters():
                        p.requires_grad = False
        self._freeze_stages()

    @property
    def norm1(self):
        return self.bn1

    def _check_stem_form(self):
        """The stem and downsample forms this class builds (Res2Net: the deep stem and ``avg_down``, always)."""
        if self.deep_stem:
            raise NotImplementedError('ResNet: deep_stem=True (three 3x3 stem convolutions) is not built')
        if self.avg_down:
            raise NotImplementedError('ResNet: avg_down=True (AvgPool2d in the downsample path) is not built')

    def _make_stem(self, in_channels, stem_channels):
        """The stem's parameter holders, registered where the reference registers them: in front of the stages."""
        self.conv1 = _conv_weight(stem_channels, in_channels, 7)
        self.bn1 = _BN(stem_channels)
        self._stem = _FoldedStem([(self.conv1, self.bn1)], [in_channels])

    def _stem_modules(self):
        """What ``frozen_stages >= 0`` freezes of the stem."""
        return (self.conv1, self.bn1)

    def _make_stage(self, inplanes, planes, num_blocks, stride):
        """The blocks of one stage (resnet.py:516-518, make_res_layer): the first has the stride and the downsample path."""
        out = planes * Bottleneck.expansion
        down = stride != 1 or inplanes != out
        kw = dict(wide_from=CONV2D_3X3_MAX_WIDTH, **self._block_kwargs(planes))
        blocks = [Bottleneck(inplanes, planes, downsample=down, stride=stride, style=self.style, **kw)]
        blocks += [Bottleneck(out, planes, **kw) for _ in range(1, num_blocks)]
        return blocks

    def _block_kwargs(self, planes):
        """What a stage of ``planes`` passes to its blocks beyond ResNet's own arguments (ResNeXt: the groups)."""
        return {}

    def _freeze_stages(self):
        """resnet.py:573-589: the stem and the first ``frozen_stages`` stages stop asking for gradients."""
        if self.frozen_stages >= 0:
            for m in self._stem_modules():
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            for p in getattr(self, f'layer{i}').parameters():
                p.requires_grad = False

    def init_weights(self, pretrained=None):
        """resnet.py:591-621 without a checkpoint: kaiming convolutions, unit BatchNorm, and with ``zero_init_residual``
        a zero ``bn3`` in every block."""
        if isinstance(pretrained, str):
            raise NotImplementedError('ResNet.init_weights: load a checkpoint with load_state_dict')
        if pretrained is not None:
            raise TypeError('pretrained must be a str or None')
        for m in self.modules():
            if isinstance(m, _BN):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif getattr(m, 'weight', None) is not None and m.weight.dim() == 4:
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, (Bottleneck, Bottle2neck)):
                    nn.init.constant_(m.bn3.weight, 0)
                    nn.init.constant_(m.bn3.bias, 0)

    def _check(self, img):
        if torch.is_grad_enabled() and (img.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('ResNet: training (BatchNorm in train mode, the backward of the stages) is not built; '
                                      'run inference under torch.no_grad()')
        if img.dim() != 4 or img.shape[1] != self.in_channels:
            raise ValueError(f'ResNet: [B, {self.in_channels}, H, W] images expected, got {tuple(img.shape)}')
        self._check_stem_shape(img)

    def _check_stem_shape(self, img):
        if not ops.conv7x7_s2_supported(img.shape, self.stem_channels):
            raise NotImplementedError(f'ResNet: in_channels={self.in_channels}, stem_channels={self.stem_channels} on a '
                                      f'{tuple(img.shape)} batch: dm_conv7x7_s2_supported refuses the stem (3 input '
                                      'channels and a non-empty batch are built)')

    def stem(self, img):
        """relu(bn1(conv1(img))) and the max-pool: two launches."""
        w, b = self._stem.packed()
        return ops.maxpool3x3_s2(ops.conv7x7_s2(img, w, b, self.stem_channels, relu=True))

    def run_stage(self, i, x):
        """Stage ``i`` (``layer{i + 1}``) on its input; ``x`` is not written."""
        blocks = getattr(self, self.res_layers[i])
        if blocks[0].downsample is None:          # no new tensor from block 0: the in-place blocks get a copy
            x = x.clone()
        for block in blocks:
            x = block(x)
        return x

    def forward(self, img):
        """``img`` [B, 3, H, W] float32 -> the tuple of the ``out_indices`` stages."""
        self._check(img)
        x = self.stem(img.contiguous())
        outs = []
        for i in range(len(self.res_layers)):
            x = self.run_stage(i, x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)


@BACKBONES.register_module()
class ResNeXt(ResNet):
    """``ResNeXt`` -- backbones/resnext.py:87-132, inference: ``ResNet`` whose blocks run conv2 in ``groups`` groups on
    ``width = floor(planes * base_width / base_channels) * groups`` channels (``layers.Bottleneck``: ONE
    ``ops.conv3x3_grouped`` launch, stride 1 or 2).  ``state_dict`` keys as ``ResNet``'s, the shapes the reference's:
    ``conv1`` [width, inplanes, 1, 1], ``conv2`` [width, width / groups, 3, 3], ``conv3`` [4 planes, width, 1, 1].  Every
    refusal of ``ResNet`` holds; the grouped kernel is built for 4, 8, 16, 32 and 64 channels per group -- what 32x4d,
    64x4d and 32x8d have in layers 1 to 4 --, anything else is refused here, at construction.  ``groups=1`` is
    ``ResNet``'s dense path."""

    arch_settings = {d: (Bottleneck, b) for d, b in _STAGE_BLOCKS.items()}
    CHANNELS_PER_GROUP = (4, 8, 16, 32, 64)

    def __init__(self, groups=1, base_width=4, **kwargs):
        self.groups, self.base_width = groups, base_width
        super().__init__(**kwargs)

    def _block_kwargs(self, planes):
        if self.groups == 1:
            return {}
        groups, bw, bc = self.groups, self.base_width, self.base_channels
        per_group = planes * bw // bc if isinstance(groups, int) and groups > 1 else 0
        if per_group not in self.CHANNELS_PER_GROUP or per_group * groups % 8 != 0:
            raise NotImplementedError(
                f'ResNeXt: groups={groups}, base_width={bw} (base_channels={bc}) give {per_group} channels per group, '
                f'{per_group * groups if per_group else 0} in all, in the stage of {planes} planes; the grouped 3x3 kernel is built for '
                f'{self.CHANNELS_PER_GROUP} channels per group and the 1x1 kernels beside it for widths that are multiples of 8')
        return dict(groups=groups, base_width=bw, base_channels=bc)


class _FoldedStemConv0(_FoldedConv):
    """``stem.0`` + ``stem.1`` folded, in ``ops.conv3x3_s2_c3``'s layout: torch's own."""

    def packed(self):
        return self.folded()


class DeepStem(nn.Sequential):
    """The reference's ``stem`` submodule of a ``deep_stem`` net (resnet.py:525-557) with its keys -- ``{0,3,6}.weight``,
    ``{1,4,7}.*``; 2, 5 and 8 are the ReLUs -- and the max-pool behind it (resnet.py:631), so that calling it is what
    ``ResNet.stem(img)`` is: four launches.  ``ops.conv3x3_s2_c3`` from the image, two ``ops.conv3x3_dil`` at dilation 1
    (any map width: the half-size map of a 1333 x 800 image is 672 wide) and ``ops.maxpool3x3_s2``, BatchNorm folded."""

    def __init__(self, in_channels, stem_channels):
        half = stem_channels // 2
        super().__init__(_conv_weight(half, in_channels, 3), _BN(half), nn.ReLU(inplace=True),
                         _conv_weight(half, half, 3), _BN(half), nn.ReLU(inplace=True),
                         _conv_weight(stem_channels, half, 3), _BN(stem_channels), nn.ReLU(inplace=True))
        self.half, self.stem_channels = half, stem_channels
        self._f = [_FoldedStemConv0([(self[0], self[1])], [in_channels]), _FoldedConv([(self[3], self[4])], [half]),
                   _FoldedConv([(self[6], self[7])], [half])]

    def forward(self, img):
        (w0, b0), (w1, b1), (w2, b2) = (f.packed() for f in self._f)
        x = ops.conv3x3_s2_c3(img, w0, b0, relu=True)
        x = ops.conv3x3_dil(x, w1, b1, self.half, 1, relu=True)
        x = ops.conv3x3_dil(x, w2, b2, self.stem_channels, 1, relu=True)
        return ops.maxpool3x3_s2(x)


@BACKBONES.register_module()
class Res2Net(ResNet):
    """``Res2Net`` -- backbones/res2net.py:240-315, inference: ``ResNet`` with ``layers.Bottle2neck`` blocks (``scales``
    slices of ``floor(planes * base_width / base_channels)`` channels), the first block of every stage of
    ``stage_type='stage'``, and -- ALWAYS, whatever the caller passes, as the reference does (res2net.py:298-308) --
    ``style='pytorch'``, ``deep_stem=True`` and ``avg_down=True``.  ``state_dict`` keys as the reference's: ``stem.{0,3,6}
    .weight``, ``stem.{1,4,7}.*`` (there is no ``conv1`` / ``bn1``), ``layer{1..4}.{i}.conv{1,3}.weight``, ``.bn{1,3}.*``,
    ``.convs.{j}.weight``, ``.bns.{j}.*``, ``.downsample.{1,2}.*``.  ``stem`` is the submodule here (``DeepStem``: calling
    it runs the stem as ``ResNet.stem`` does).  Every other refusal of ``ResNet`` holds; depths 50 / 101 / 152.

    Launches from the image: 4 (stem) + per stage 3 (stride 1) or 4 (stride 2) for the stage block + 5 for every
    normal block -- R2-101: 4 + 3 + 3 * 4 + 29 * 5 = 164."""

    arch_settings = {d: (Bottle2neck, b) for d, b in _STAGE_BLOCKS.items()}

    def __init__(self, scales=4, base_width=26, style='pytorch', deep_stem=True, avg_down=True, **kwargs):
        self.scales, self.base_width = scales, base_width
        depth = kwargs.get('depth')
        if depth not in self.arch_settings:
            raise KeyError(f'invalid depth {depth} for resnet')
        super().__init__(style='pytorch', deep_stem=True, avg_down=True, **kwargs)

    def _check_stem_form(self):
        if self.stem_channels % 16 != 0:
            raise NotImplementedError(f'Res2Net: stem_channels={self.stem_channels}; the deep stem has stem_channels / 2 '
                                      'channels inside, which the any-width 3x3 kernel walks in chunks of 8')

    def _make_stem(self, in_channels, stem_channels):
        # ``stem`` is a method of ResNet, so ``add_module`` would refuse the name: the submodule is registered directly
        # and the property below makes ``self.stem`` resolve to it
        self._modules['stem'] = DeepStem(in_channels, stem_channels)

    stem = property(lambda self: self._modules['stem'], doc='the reference\'s ``stem`` submodule; calling it runs the stem')

    def _stem_modules(self):
        return (self.stem,)

    def _make_stage(self, inplanes, planes, num_blocks, stride):
        """res2net.py:161-237 (Res2Layer): the first block is a 'stage' block with the downsample path."""
        out = planes * Bottle2neck.expansion
        down = stride != 1 or inplanes != out
        kw = dict(scales=self.scales, base_width=self.base_width, base_channels=self.base_channels)
        try:
            blocks = [Bottle2neck(inplanes, planes, downsample=down, stride=stride, stage_type='stage', **kw)]
            blocks += [Bottle2neck(out, planes, **kw) for _ in range(1, num_blocks)]
        except NotImplementedError as e:
            raise NotImplementedError(f'Res2Net: scales={self.scales}, base_width={self.base_width} in the stage of {planes} '
                                      f'planes: {e}') from None
        return blocks

    def _check_stem_shape(self, img):
        NB, _, H, W = img.shape
        half, Hh, Wh = self.stem_channels // 2, (H + 1) // 2, (W + 1) // 2
        if not ops.conv3x3_s2_c3_supported(img.shape, half):
            raise NotImplementedError(f'Res2Net: in_channels={self.in_channels} on a {tuple(img.shape)} batch: '
                                      'dm_conv3x3_s2_c3_supported refuses the stem (3 input channels and a non-empty '
                                      'batch are built)')
        for cout in (half, self.stem_channels):
            if not ops.lib().dm_conv3x3_dil_supported(NB, half, Hh, Wh, cout, 1):
                raise NotImplementedError(f'Res2Net: dm_conv3x3_dil_supported refuses the stem\'s {half} -> {cout} 3x3 on a '
                                          f'{(NB, half, Hh, Wh)} map')
