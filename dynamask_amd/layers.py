"""The parameter holders and weight caches every head, neck and backbone is made of.  They own parameters under the
reference's ``state_dict`` keys and launch through ``ops``; this module imports none of the modules that use them."""
import torch
import torch.nn as nn

from . import ops
from .registry import UPSAMPLE_LAYERS

# ops.conv2d's 3x3 builds stage whole rows of the map (csrc/conv_igemm.hip: the plane of a 128-pixel tile), which stops
# fitting their LDS at 169 pixels of width; the 3x3 kernel of csrc/conv_dilated.hip stages 8 x 16 blocks and takes any
# width, from the same packed weights, exact fp32 too.  rpn_conv runs on it (dilation 1) on maps wider than this -- the
# stride-4 and stride-8 maps of a 1333 x 800 image -- and on ops.conv2d below; the width alone decides, so a map's kernel
# does not depend on the batch.
CONV2D_3X3_MAX_WIDTH = 128

# backbones/resnet.py:356-362 (ResNet.arch_settings): depth -> blocks per stage; 18 / 34 are BasicBlock nets
_STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
_BASIC_BLOCK_DEPTHS = (18, 34)


class _Packed:
    """Cache of kernel-layout weights, refreshed when the parameter changes."""

    def __init__(self):
        self._c = {}

    def get(self, key, param, fn, job=None, precision='fp32'):
        """``job`` = (transpose_flip, src_channels | None, lo | None, hi | None): the pack is dm_conv_pack_weight of
        the parameter itself (or of its input-channel window lo:hi); such packs of contiguous device parameters are
        registered with ops.PACK_PLAN and refreshed together in one launch.  Anything else goes through ``fn``.
        ``precision='bf16x3'``: ``fn`` makes the bf16x3 layout (inference only: never a PACK_PLAN job), cached under a key
        of its own, so that both layouts of a weight coexist."""
        if precision != 'fp32':
            key, job = (precision, key), None
        if job is not None and param.is_cuda and param.dim() == 4 and param.is_contiguous():
            e = self._c.get(key)
            if e is None or e[0] != 'plan' or e[1]['param']() is not param:
                e = ('plan', ops.PACK_PLAN.register(param, *job))
                self._c[key] = e
            with torch.no_grad():
                return ops.PACK_PLAN.get(e[1])
        ver = (param.data_ptr(), param._version, param.device, ops.WEIGHT_EPOCH[0])
        e = self._c.get(key)
        if e is None or e[0] != ver:
            with torch.no_grad():
                e = (ver, fn(param.detach().contiguous()))
            self._c[key] = e
        return e[1]

    def get_multi(self, key, params, fn):
        """One pack made from several parameters (a table): ``fn()`` runs again when any of them changes."""
        ver = tuple((p.data_ptr(), p._version) for p in params) + (params[0].device, ops.WEIGHT_EPOCH[0])
        e = self._c.get(key)
        if e is None or e[0] != ver:
            with torch.no_grad():
                e = (ver, fn())
            self._c[key] = e
        return e[1]


class _Conv(nn.Module):
    """Parameter holder named like nn.Conv2d (weight [Cout,Cin,k,k], bias)."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        nn.init.kaiming_normal_(self.weight, mode='fan_out', nonlinearity='relu')
        self._pk = _Packed()

    exact = False         # True: always the exact fp32 kernel, whatever the precision mode (MaskPre, the selector)

    def packed(self, src_channels=None, precision='fp32'):
        key = tuple(src_channels) if src_channels is not None else (self.in_channels,)
        return self._pk.get(key, self.weight, lambda w: ops.pack_conv_weight(w, src_channels=list(key), precision=precision),
                            job=(False, list(key), None, None), precision=precision)

    def precision_for(self, H, W):
        """The kernel this layer's convolution of an H x W map runs now (ops.conv_precision_for)."""
        return 'fp32' if self.exact else ops.conv_precision_for(self.out_channels, self.kernel_size, H, W)

    def run(self, srcs, relu=False, out=None, out_ch_offset=0):
        b = self.bias.detach() if self.bias is not None else None
        if isinstance(srcs, torch.Tensor):
            srcs = [srcs]
        wq = self.packed([s.shape[1] for s in srcs], self.precision_for(srcs[0].shape[2], srcs[0].shape[3]))
        return ops.conv2d(srcs, wq, b, self.out_channels, self.kernel_size, relu=relu, out=out,
                          out_ch_offset=out_ch_offset)


def _exact_conv(cin, cout, k):
    c = _Conv(cin, cout, k)
    c.exact = True          # a changed score reorders proposals: the bf16x3 mode does not reach the RPN
    return c


def _conv_weight(cout, cin, k):
    """nn.Conv2d(bias=False) parameter holder: the key is ``weight`` alone."""
    return _Conv(cin, cout, k, bias=False)


class ConvModule(nn.Module):
    """mmcv ConvModule without norm: conv(bias) + ReLU; keys ``conv.weight/bias``."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, dilation=1, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type='ReLU')):
        super().__init__()
        if conv_cfg is not None or norm_cfg is not None:
            raise NotImplementedError('conv_cfg / norm_cfg are None in configs/dynamask')
        if dilation != 1 or padding != kernel_size // 2:
            raise NotImplementedError('only "same" stride-1 convolutions are on the path')
        self.conv = _Conv(in_channels, out_channels, kernel_size)
        self.with_activation = act_cfg is not None

    def forward(self, x):
        return self.conv.run(x, relu=self.with_activation)


@UPSAMPLE_LAYERS.register_module(name='carafe')
class CARAFEPack(nn.Module):
    """mmcv CARAFEPack: keys channel_compressor.*, content_encoder.*.  It lives here because two sections build it:
    FCNMaskHead's upsample (mask_heads.py) and FPN_CARAFE's top-down path (necks.py, on the whole-map kernel)."""

    def __init__(self, channels, scale_factor, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1,
                 compressed_channels=64):
        super().__init__()
        if encoder_kernel != 3 or encoder_dilation != 1:
            raise NotImplementedError('CARAFE encoder is 3x3, dilation 1 on the path')
        self.channels, self.scale_factor, self.up_kernel, self.up_group = channels, scale_factor, up_kernel, up_group
        self.channel_compressor = _Conv(channels, compressed_channels, 1)
        self.content_encoder = _Conv(compressed_channels, up_kernel * up_kernel * up_group * scale_factor ** 2, 3)
        self.init_weights()

    def init_weights(self):
        nn.init.xavier_uniform_(self.channel_compressor.weight)
        nn.init.zeros_(self.channel_compressor.bias)
        nn.init.normal_(self.content_encoder.weight, std=0.001)
        nn.init.zeros_(self.content_encoder.bias)

    def forward(self, x, relu=False):
        comp = self.channel_compressor.run(x)
        enc = self.content_encoder.run(comp)
        return ops.carafe(x, enc, self.up_kernel, self.up_group, self.scale_factor)


class _BN(nn.Module):
    """BatchNorm2d parameter/buffer holder (keys as nn.BatchNorm2d)."""

    def __init__(self, c, eps=1e-5, momentum=0.1):
        super().__init__()
        self.eps, self.momentum = eps, momentum
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer('running_mean', torch.zeros(c))
        self.register_buffer('running_var', torch.ones(c))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))


class _Linear(nn.Module):
    """nn.Linear parameter holder at nn.Linear's own initialisation; the product runs on the fp32 MFMA FC kernel
    (dm_fc_fwd)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.in_features, self.out_features = cin, cout
        self.weight, self.bias = (nn.Parameter(t) for t in self._init(cin, cout))
        self._pk = _Packed()      # transposed packed weights of the backward's data-gradient GEMM

    @staticmethod
    def _init(cin, cout):
        lin = nn.Linear(cin, cout)
        return lin.weight.detach().clone(), lin.bias.detach().clone()

    def run(self, x, relu=False):
        return ops.fc(x.contiguous(), self.weight.detach(), self.bias.detach(), relu=relu)


class _FC(_Linear):
    """``_Linear`` as the bbox heads start it: xavier-uniform weight, zero bias."""

    @staticmethod
    def _init(cin, cout):
        return nn.init.xavier_uniform_(torch.empty(cout, cin)), torch.zeros(cout)


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


class _FoldedGroupedConv(_FoldedConv):
    """A grouped 3x3 convolution (weight [C, C / groups, 3, 3]) + its BatchNorm folded -- ``fold_bn`` scales per output
    channel, whatever the weight's second dimension --, in ``ops.conv3x3_grouped``'s layout."""

    def __init__(self, pairs, groups):
        super().__init__(pairs, [pairs[0][0].out_channels])
        self.groups = groups

    def packed(self):
        def make():
            w, b = self.folded()
            return ops.pack_grouped_conv_weight(w, self.groups), b
        return self._pk.get_multi('pack3g', self._tensors(), make)


class BNConvModule(nn.Module):
    """mmcv ConvModule(bias=False, norm_cfg=dict(type='BN')): keys ``conv.weight``, ``bn.*``.  A parameter holder: the
    block that owns it folds the BatchNorm and launches."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        self.conv = _conv_weight(out_channels, in_channels, kernel_size)
        self.bn = _BN(out_channels)


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
    ``ops.conv3x3_dil`` (dilation 1, any width, the same packed weights) instead of ``ops.conv2d``.

    ``groups > 1`` (backbones/resnext.py:11-84, backbones.ResNeXt): conv1 and conv3 have ``width = floor(planes *
    base_width / base_channels) * groups`` channels between them and conv2 is ``width -> width`` in ``groups`` groups
    (weight [width, width / groups, 3, 3]): ONE ``ops.conv3x3_grouped`` launch at any map width (``wide_from`` does not
    apply), with ``stride=2`` where style 'pytorch' strides.  The block stays three launches."""
    expansion = 4

    def __init__(self, inplanes, planes, downsample=False, stride=1, style='pytorch', wide_from=None, groups=1, base_width=4,
                 base_channels=64):
        super().__init__()
        if not downsample and inplanes != planes * self.expansion:
            raise NotImplementedError('Bottleneck: no downsample path (DoubleConvFCBBoxHead: planes = inplanes / 4)')
        if stride not in (1, 2) or style not in ('pytorch', 'caffe') or (stride == 2 and not downsample):
            raise NotImplementedError(f'Bottleneck: stride={stride}, style={style!r}, downsample={downsample}; stride 1, or '
                                      "stride 2 with a downsample path, in style 'pytorch' or 'caffe' are built")
        self.stride, self.style, self.wide_from = stride, style, wide_from
        self.inplanes, self.planes, self.groups = inplanes, planes, groups
        width = self.width = planes if groups == 1 else (planes * base_width // base_channels) * groups
        if groups < 1 or width < groups:
            raise ValueError(f'Bottleneck: groups={groups}, base_width={base_width}, base_channels={base_channels} leave '
                             f'{width} channels for {groups} groups at planes={planes}')
        out = planes * self.expansion
        self.conv1, self.bn1 = _conv_weight(width, inplanes, 1), _BN(width)
        self.conv2, self.bn2 = _conv_weight(width, width // groups, 3), _BN(width)
        self.conv3, self.bn3 = _conv_weight(out, width, 1), _BN(out)
        self._f = [_FoldedConv([(self.conv1, self.bn1)], [inplanes]),
                   (_FoldedConv([(self.conv2, self.bn2)], [width]) if groups == 1 else
                    _FoldedGroupedConv([(self.conv2, self.bn2)], groups))]
        if downsample:
            self.downsample = nn.Sequential(_conv_weight(out, inplanes, 1), _BN(out))
            self._f.append(_FoldedConv([(self.conv3, self.bn3), (self.downsample[0], self.downsample[1])], [width, inplanes]))
        else:
            self.downsample = None
            self._f.append(_FoldedConv([(self.conv3, self.bn3)], [width]))

    def forward(self, x):
        """Without ``downsample``: ``x`` [N, inplanes, H, W] is overwritten with the block's output and returned.  With
        it: a new [N, 4 planes, H, W] tensor."""
        (w1, b1), (w2, b2), (w3, b3) = (f.packed() for f in self._f)
        if self.stride == 2 and self.style == 'caffe':
            x = ops.subsample2(x)
        h = ops.conv2d(x, w1, b1, self.width, 1, relu=True)
        strided = self.stride == 2 and self.style == 'pytorch'
        if self.groups > 1:
            h = ops.conv3x3_grouped(h, w2, b2, self.groups, stride=2 if strided else 1, relu=True)
        elif strided:
            h = ops.conv3x3_s2(h, w2, b2, self.planes, relu=True, splits=1)
        elif self.wide_from is not None and h.shape[3] > self.wide_from:
            h = ops.conv3x3_dil(h, w2, b2, self.planes, 1, relu=True)
        else:
            h = ops.conv2d(h, w2, b2, self.planes, 3, relu=True)
        if strided:
            x = ops.subsample2(x)
        if self.downsample is not None:
            return ops.conv2d([h, x], w3, b3, self.planes * self.expansion, 1, relu=True)
        return ops.conv2d(h, w3, b3, self.inplanes, 1, relu=True, out=x, accumulate=True)


class _FoldedSlices(_FoldedConv):
    """``pairs`` = G (3x3 convolution w -> w, its BatchNorm) of a Bottle2neck, each folded by itself (``fold_bn`` in
    float64), stacked [G, w, w, 3, 3] with the biases [G * w], in ``ops.conv3x3_slices``'s layout."""

    def __init__(self, pairs):
        super().__init__(pairs, [pairs[0][0].out_channels])

    def folded(self):
        def make():
            each = [fold_bn([p]) for p in self._pairs()]
            return torch.stack([w for w, _ in each]).contiguous(), torch.cat([b for _, b in each]).contiguous()
        return self._pk.get_multi('fold', self._tensors(), make)

    def packed(self):
        def make():
            w, b = self.folded()
            return ops.pack_conv_slices_weight(w), b
        return self._pk.get_multi('pack3s', self._tensors(), make)


class Bottle2neck(nn.Module):
    """backbones/res2net.py:13-158 in eval mode (style 'pytorch').  Keys as the reference's: ``conv1.weight`` [w scales,
    inplanes, 1, 1], ``bn1.*``, ``conv3.weight`` [4 planes, w scales, 1, 1], ``bn3.*``, with a downsample path
    ``downsample.1.weight``, ``downsample.2.*`` (index 0 is the parameterless average pool), ``convs.{i}.weight``
    [w, w, 3, 3] and ``bns.{i}.*`` for i < scales - 1; ``w = floor(planes * base_width / base_channels)``.  There is no
    ``conv2`` and no ``bn2``: in their place ``scales - 1`` 3x3 convolutions run on the w-channel slices ``spx[i]`` of
    conv1's output, and the last slice passes through.

    ``stage_type='normal'`` (stride 1): convolution i >= 1 reads ``spx[i]`` + the output of convolution i - 1
    (res2net.py:125), so they are ``scales - 1`` ``ops.conv3x3_slices`` launches in a row, each with G = 1, launch i >= 1
    with the previous slice of the concatenation buffer as its addend; the copy of ``spx[scales - 1]`` rides with the
    first as its tail.  ``stage_type='stage'`` (the first block of a layer, res2net.py:122-123): no hierarchical add, ONE
    launch with G = scales - 1 at stride 1 or 2 whose tail copies the last slice (stride 1) or takes its
    ``AvgPool2d(3, 2, 1)`` (stride 2, res2net.py:130-133).  No ``split`` and no ``cat`` is ever made: every launch reads
    and writes channel slices of the two wide tensors.

    Without ``downsample`` the block closes with conv3's ``accumulate | ReLU`` epilogue IN PLACE into ``x``, as
    ``Bottleneck`` does: 2 + (scales - 1) launches in a normal block.  With it (``avg_down``: ``AvgPool2d(stride, stride,
    ceil_mode=True, count_include_pad=False)`` -- ``ops.avgpool2x2_ceil`` at stride 2, the identity and no launch at
    stride 1 --, then the 1x1 + BatchNorm) it closes with ONE two-source 1x1 of [concatenation buffer, pooled x] by
    [W3' | Wd'] with ReLU into a NEW tensor: 3 launches at stride 1 and 4 at stride 2 in a stage block."""
    expansion = 4

    def __init__(self, inplanes, planes, downsample=False, stride=1, scales=4, base_width=26, base_channels=64,
                 stage_type='normal'):
        super().__init__()
        if stage_type not in ('normal', 'stage'):
            raise ValueError(f"Bottle2neck: stage_type={stage_type!r}; 'normal' or 'stage'")
        if not isinstance(scales, int) or scales < 2:
            raise NotImplementedError(f'Bottle2neck: scales={scales}; Res2Net degenerates to ResNet at scales = 1, 2 and more are built')
        if not downsample and inplanes != planes * self.expansion:
            raise NotImplementedError(f'Bottle2neck: inplanes={inplanes} != 4 * planes={planes} needs a downsample path')
        if stride not in (1, 2) or (stride == 2 and (not downsample or stage_type != 'stage')):
            raise NotImplementedError(f'Bottle2neck: stride={stride}, stage_type={stage_type!r}, downsample={downsample}; stride 1, or '
                                      "stride 2 in a 'stage' block with a downsample path, are built")
        width = planes * base_width // base_channels
        if width < 1 or width * scales % 8 != 0:
            raise NotImplementedError(
                f'Bottle2neck: planes={planes}, base_width={base_width}, base_channels={base_channels}, scales={scales} give '
                f'{width} channels per scale, {width * scales} in all; the 1x1 kernels beside the sliced 3x3 take widths '
                'that are multiples of 8')
        # (the map's size is the caller's: 8 x 8 stands for any -- only a launch of 2^31 workgroups depends on it)
        tail = 2 if stride == 2 else 1
        groups = scales - 1 if stage_type == 'stage' else 1
        if not ops.conv3x3_slices_supported((1, width * scales, 8, 8), width, groups, stride, tail=tail):
            raise NotImplementedError(f'Bottle2neck: dm_conv3x3_slices_supported refuses {groups} slice(s) of {width} channels at '
                                      f'stride {stride} in a {width * scales}-channel tensor')
        self.inplanes, self.planes, self.stride, self.scales = inplanes, planes, stride, scales
        self.base_width, self.base_channels, self.stage_type, self.width = base_width, base_channels, stage_type, width
        out = planes * self.expansion
        self.conv1, self.bn1 = _conv_weight(width * scales, inplanes, 1), _BN(width * scales)
        self.conv3, self.bn3 = _conv_weight(out, width * scales, 1), _BN(out)
        if downsample:
            self.downsample = nn.Sequential(nn.AvgPool2d(stride, stride, ceil_mode=True, count_include_pad=False),
                                            _conv_weight(out, inplanes, 1), _BN(out))
        else:
            self.downsample = None
        self.convs = nn.ModuleList([_conv_weight(width, width, 3) for _ in range(scales - 1)])
        self.bns = nn.ModuleList([_BN(width) for _ in range(scales - 1)])
        pairs = list(zip(self.convs, self.bns))
        self._f1 = _FoldedConv([(self.conv1, self.bn1)], [inplanes])
        self._f2 = [_FoldedSlices(pairs)] if stage_type == 'stage' else [_FoldedSlices([p]) for p in pairs]
        if downsample:
            self._f3 = _FoldedConv([(self.conv3, self.bn3), (self.downsample[1], self.downsample[2])], [width * scales, inplanes])
        else:
            self._f3 = _FoldedConv([(self.conv3, self.bn3)], [width * scales])

    def forward(self, x):
        """Without ``downsample``: ``x`` [N, inplanes, H, W] is overwritten with the block's output and returned.  With
        it: a new [N, 4 planes, ceil(H / stride), ceil(W / stride)] tensor; ``x`` is not written."""
        w, s, stride = self.width, self.scales, self.stride
        w1, b1 = self._f1.packed()
        h = ops.conv2d(x, w1, b1, w * s, 1, relu=True)
        N, _, H, W = h.shape
        cat = torch.empty((N, w * s, (H + stride - 1) // stride, (W + stride - 1) // stride), device=h.device, dtype=torch.float32)
        last = (s - 1) * w
        if self.stage_type == 'stage':
            wq, bq = self._f2[0].packed()
            ops.conv3x3_slices(h, wq, bq, w, s - 1, cat, stride=stride, relu=True, tail=2 if stride == 2 else 1,
                               tail_x_ch0=last, tail_o_ch0=last)
        else:
            for i, f in enumerate(self._f2):
                wq, bq = f.packed()
                ops.conv3x3_slices(h, wq, bq, w, 1, cat, relu=True, x_ch0=i * w, o_ch0=i * w, addend=cat if i else None,
                                   a_ch0=(i - 1) * w if i else 0, tail=0 if i else 1, tail_x_ch0=last, tail_o_ch0=last)
        w3, b3 = self._f3.packed()
        if self.downsample is None:
            return ops.conv2d(cat, w3, b3, self.inplanes, 1, relu=True, out=x, accumulate=True)
        if stride == 2:
            x = ops.avgpool2x2_ceil(x)
        return ops.conv2d([cat, x], w3, b3, self.planes * self.expansion, 1, relu=True)
