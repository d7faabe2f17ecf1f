"""Necks behind the reference's NECKS registry, at inference: ``FPN`` (mmdet/models/necks/fpn.py) and ``FPN_CARAFE``
(mmdet/models/necks/fpn_carafe.py, at the end of this file) -- the maps the RPN and the RoI heads start from, made from
the backbone's stages.

``forward`` walks the laterals from the top level down.  The top lateral is a plain 1x1 ``ops.conv2d``; every level below
is ONE ``ops.conv2d_up_add`` (``dm_conv2d_up_add_fwd``): the 1x1 lateral convolution whose epilogue adds the merged lateral
above it, read through two nearest-neighbour index tables -- ``laterals[i - 1] += F.interpolate(laterals[i])``
(fpn.py:177-186) without the upsampled map and without a second pass over the lateral.  The level convolutions are 3x3
``ops.conv2d`` launches, ``ops.conv3x3_dil`` at dilation 1 on maps wider than ``layers.CONV2D_3X3_MAX_WIDTH`` (the
width alone decides, so a map's kernel does not depend on the batch); extra levels are ``ops.subsample2``
(``F.max_pool2d(x, 1, stride=2)``) or ``ops.conv3x3_s2``.  Every convolution is exact fp32 in every precision mode: a
changed feature reorders the proposals made from it.  The host never waits.

``DM_FPN_FUSED=0`` (or clearing ``FPN_FUSED``) runs the merge composed: the lateral ``ops.conv2d`` and then
``lat += F.interpolate(...)`` in torch, the max-pool by slicing.  The same bits.

``FPN_CARAFE`` builds every lateral first (the extra levels' are stride-2 3x3 convolutions and take part in the merge) and
merges top-down with CARAFE: per level the compressor 1x1, the encoder 3x3 and ONE ``ops.carafe_map``
(``dm_carafe_map_fwd``), the reassembly at scale 2 whose epilogue adds the cropped result to the lateral below in place."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers import CONV2D_3X3_MAX_WIDTH, CARAFEPack, _exact_conv
from .registry import NECKS


def _env_fused():
    return os.environ.get('DM_FPN_FUSED', '1') != '0'


FPN_FUSED = [_env_fused()]

_TABLES = {}


def nearest_index(n_in, n_out, scale_factor=None, device=None):
    """int32 [n_out]: the source index of every output index of ``F.interpolate(mode='nearest')`` along an axis of
    ``n_in`` elements -- by running torch's own CPU ``F.interpolate`` over the ramp ``arange(n_in)``, with ``size=n_out``
    or, when ``scale_factor`` is given, with ``scale_factor=`` as the reference's call passes it: the table is the
    installed torch's rule by construction (torch divides by the scale factor it is given, and by ``n_out / n_in`` when
    it is given a size; the two differ at sizes like 2 n - 1).  With ``scale_factor`` the produced length must be
    ``n_out`` (ValueError otherwise: the reference's ``+=`` fails there too).  Cached per (n_in, n_out, scale_factor,
    device)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f'nearest_index: {n_in} -> {n_out}')
    sf = None if scale_factor is None else float(scale_factor)
    dev = torch.device('cpu') if device is None else torch.device(device)
    key = (n_in, n_out, sf, str(dev))
    t = _TABLES.get(key)
    if t is None:
        ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in)        # (exact up to 2^24 elements)
        if sf is None:
            up = F.interpolate(ramp, size=n_out, mode='nearest')
        else:
            up = F.interpolate(ramp, scale_factor=sf, mode='nearest')
            if up.shape[-1] != n_out:
                raise ValueError(f'upsample_cfg scale_factor={scale_factor}: {n_in} -> {up.shape[-1]} elements, but the '
                                 f'lateral below has {n_out}')
        t = up.view(-1).to(torch.int32).to(dev)
        _TABLES[key] = t
    return t


class _NeckConv(nn.Module):
    """ConvModule(norm_cfg=None, act_cfg=None): keys ``conv.weight`` / ``conv.bias``; exact fp32 in every precision mode."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1):
        super().__init__()
        self.conv = _exact_conv(in_channels, out_channels, kernel_size)
        self.stride = stride


@NECKS.register_module()
class FPN(nn.Module):
    """``FPN`` -- fpn.py:9-216, inference.  ``state_dict`` keys: ``lateral_convs.{i}.conv.{weight,bias}`` and
    ``fpn_convs.{i}.conv.{weight,bias}``, the extra stride-2 convolutions behind the level convolutions in ``fpn_convs``.
    Training, norm layers (``norm_cfg``), ``conv_cfg``, ``act_cfg`` and upsample modes other than 'nearest' are not
    built."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 extra_convs_on_inputs=True, relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, upsample_cfg=dict(mode='nearest')):
        super().__init__()
        if not isinstance(in_channels, (list, tuple)):
            raise TypeError(f'FPN: in_channels must be a list, got {type(in_channels).__name__}')
        if conv_cfg is not None:
            raise NotImplementedError(f'FPN: conv_cfg={conv_cfg} is not built (None in every FPN config the project reads)')
        if norm_cfg is not None:
            raise NotImplementedError(f'FPN: norm_cfg={norm_cfg} is not built (the GN necks of configs/gn)')
        if act_cfg is not None:
            raise NotImplementedError(f'FPN: act_cfg={act_cfg} is not built (None in every FPN config of the reference)')
        upsample_cfg = dict(upsample_cfg)
        if upsample_cfg.get('mode', 'nearest') != 'nearest':
            raise NotImplementedError(f"FPN: upsample_cfg mode={upsample_cfg['mode']!r} is not built; 'nearest' only")
        if set(upsample_cfg) - {'mode', 'scale_factor'}:
            raise NotImplementedError(f'FPN: upsample_cfg keys {sorted(set(upsample_cfg) - {"mode", "scale_factor"})} are '
                                      "not built; 'mode' and 'scale_factor' only")
        if out_channels % 8 != 0:
            raise NotImplementedError(f'FPN: out_channels={out_channels} is not a multiple of 8 (the any-width and the '
                                      'stride-2 3x3 kernels walk the input channels in chunks of 8)')
        self.in_channels = list(in_channels)
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.relu_before_extra_convs = relu_before_extra_convs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.fp16_enabled = False
        self.upsample_cfg = upsample_cfg
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            if num_outs < self.num_ins - start_level:
                raise ValueError(f'FPN: num_outs={num_outs} < {self.num_ins - start_level} used backbone levels')
        else:
            # if end_level < inputs, no extra level is allowed (fpn.py:92-96)
            self.backbone_end_level = end_level
            if end_level > self.num_ins:
                raise ValueError(f'FPN: end_level={end_level} > {self.num_ins} inputs')
            if num_outs != end_level - start_level:
                raise ValueError(f'FPN: num_outs={num_outs} != end_level - start_level = {end_level - start_level}')
        if not 0 <= start_level < self.backbone_end_level:
            raise ValueError(f'FPN: start_level={start_level} with {self.backbone_end_level} backbone levels')
        self.start_level = start_level
        self.end_level = end_level
        if not isinstance(add_extra_convs, (str, bool)):
            raise TypeError(f'FPN: add_extra_convs must be a str or a bool, got {add_extra_convs!r}')
        if isinstance(add_extra_convs, str):
            if add_extra_convs not in ('on_input', 'on_lateral', 'on_output'):
                raise ValueError(f"FPN: add_extra_convs={add_extra_convs!r}; 'on_input', 'on_lateral' or 'on_output'")
        elif add_extra_convs:
            # the legacy form (fpn.py:104-110): True means what extra_convs_on_inputs says
            add_extra_convs = 'on_input' if extra_convs_on_inputs else 'on_output'
        self.add_extra_convs = add_extra_convs

        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(_NeckConv(in_channels[i], out_channels, 1))
            self.fpn_convs.append(_NeckConv(out_channels, out_channels, 3))
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if self.add_extra_convs and extra_levels >= 1:
            for i in range(extra_levels):
                cin = in_channels[self.backbone_end_level - 1] if i == 0 and self.add_extra_convs == 'on_input' else out_channels
                if cin % 8 != 0:
                    raise NotImplementedError(f'FPN: the extra convolution reads in_channels[{self.backbone_end_level - 1}]='
                                              f'{cin} channels, not a multiple of 8 (the stride-2 3x3 kernel)')
                self.fpn_convs.append(_NeckConv(cin, out_channels, 3, stride=2))

    def init_weights(self):
        """fpn.py:158-162: xavier uniform weights, zero biases."""
        for m in list(self.lateral_convs) + list(self.fpn_convs):
            nn.init.xavier_uniform_(m.conv.weight, gain=1)
            nn.init.constant_(m.conv.bias, 0)

    # ------------------------------------------------------------------ forward
    def _tables(self, src, dst):
        """(iy, ix) of the merge of ``src`` into the lateral of ``dst``'s size."""
        sf = self.upsample_cfg.get('scale_factor')
        sfy, sfx = (sf if isinstance(sf, (list, tuple)) else (sf, sf))
        return (nearest_index(src.shape[2], dst.shape[2], sfy, dst.device),
                nearest_index(src.shape[3], dst.shape[3], sfx, dst.device))

    def _conv3x3(self, m, x):
        c = m.conv
        if x.shape[3] > CONV2D_3X3_MAX_WIDTH:
            return ops.conv3x3_dil(x, c.packed([c.in_channels]), c.bias.detach(), c.out_channels, 1)
        return c.run(x)

    def forward(self, inputs):
        """``inputs``: the backbone's stages, [B, in_channels[i], H_i, W_i]; returns the tuple of ``num_outs`` maps."""
        if len(inputs) != len(self.in_channels):
            raise ValueError(f'FPN: {len(self.in_channels)} inputs expected, got {len(inputs)}')
        if torch.is_grad_enabled() and (any(x.requires_grad for x in inputs) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('FPN: training is not built; run inference under torch.no_grad()')
        for i, x in enumerate(inputs):
            if x.dim() != 4 or x.shape[1] != self.in_channels[i]:
                raise ValueError(f'FPN: input {i}: [B, {self.in_channels[i]}, H, W] expected, got {tuple(x.shape)}')
        fused = FPN_FUSED[0]
        used = len(self.lateral_convs)
        xs = [inputs[i + self.start_level].contiguous() for i in range(used)]
        # laterals, from the top level down: each level below the top is written once, already merged
        laterals = [None] * used
        laterals[-1] = self.lateral_convs[-1].conv.run(xs[-1])
        for i in range(used - 1, 0, -1):
            c = self.lateral_convs[i - 1].conv
            iy, ix = self._tables(laterals[i], xs[i - 1])
            if fused:
                laterals[i - 1] = ops.conv2d_up_add(xs[i - 1], c.packed([c.in_channels]), c.bias.detach(), c.out_channels,
                                                    laterals[i], iy, ix)
            else:
                lat = c.run(xs[i - 1])
                if 'scale_factor' in self.upsample_cfg:
                    lat += F.interpolate(laterals[i], **self.upsample_cfg)
                else:
                    lat += F.interpolate(laterals[i], size=lat.shape[2:], **self.upsample_cfg)
                laterals[i - 1] = lat
        outs = [self._conv3x3(self.fpn_convs[i], laterals[i]) for i in range(used)]
        if self.num_outs > len(outs):
            if not self.add_extra_convs:
                for _ in range(self.num_outs - used):
                    outs.append(ops.subsample2(outs[-1]) if fused else outs[-1][:, :, ::2, ::2].contiguous())
            else:
                if self.add_extra_convs == 'on_input':
                    src = inputs[self.backbone_end_level - 1].contiguous()
                elif self.add_extra_convs == 'on_lateral':
                    src = laterals[-1]
                else:
                    src = outs[-1]
                for i in range(used, self.num_outs):
                    c = self.fpn_convs[i].conv
                    if i > used:
                        # (the ReLU in front of the second and later extra convolutions is torch's, out of place: the map
                        # it reads is an output of the call -- a few thousand values at stride 64 and above)
                        src = torch.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]
                    outs.append(ops.conv3x3_s2(src, c.packed([c.in_channels]), c.bias.detach(), c.out_channels))
        return tuple(outs)


# ---------------------------------------------------------------------------------------------------------- FPN_CARAFE
def _env_carafe_fused():
    return os.environ.get('DM_FPN_CARAFE_FUSED', '1') != '0'


# DM_FPN_CARAFE_FUSED=0 (or clearing this flag): the top-down merge composed -- ``ops.carafe_map`` without an addend at the
# full 2H x 2W, then ``lat + up[:, :, :h, :w]`` in torch.  The same bits.
FPN_CARAFE_FUSED = [_env_carafe_fused()]

_CARAFE_CFG_KEYS = ('type', 'up_kernel', 'up_group', 'encoder_kernel', 'encoder_dilation', 'compressed_channels')


class _CarafeUp(CARAFEPack):
    """``CARAFEPack`` at scale 2 on a whole map: the same keys and initialisation; the two convolutions are exact fp32 in
    every precision mode and the reassembly is the caller's ``ops.carafe_map`` (``forward`` stays the mask head's path)."""

    def __init__(self, channels, up_kernel, up_group, compressed_channels):
        super().__init__(channels, 2, up_kernel=up_kernel, up_group=up_group, compressed_channels=compressed_channels)
        self.channel_compressor.exact = self.content_encoder.exact = True

    def encode(self, x):
        """The raw content-encoder output [NB, up_group * K * K * 4, H, W] (before pixel_shuffle and softmax)."""
        comp = self.channel_compressor.run(x)
        c = self.content_encoder
        if comp.shape[3] > CONV2D_3X3_MAX_WIDTH:        # (as FPN._conv3x3: the width alone decides)
            return ops.conv3x3_dil(comp, c.packed([c.in_channels]), c.bias.detach(), c.out_channels, 1)
        return c.run(comp)


@NECKS.register_module()
class FPN_CARAFE(nn.Module):
    """``FPN_CARAFE`` -- fpn_carafe.py:8-267, inference, with the CARAFE upsample.  ``state_dict`` keys, in the reference's
    order: ``lateral_convs.{i}.conv.{weight,bias}`` (the extra levels' laterals are 3x3 stride-2 convolutions, the first
    on ``in_channels[-1]``), ``fpn_convs.{i}.conv.*``, ``upsample_modules.{i}.channel_compressor.*`` /
    ``.content_encoder.*`` (module i upsamples lateral i + 1).

    ``forward``: the laterals are 1x1 ``ops.conv2d`` launches, the extra levels ``ops.conv3x3_s2``.  Top-down, per level:
    the compressor 1x1, the encoder 3x3 and ONE ``ops.carafe_map(lat[i], enc, addend=lat[i - 1], out=lat[i - 1])`` --
    ``tensor_add(laterals[i - 1], upsample(laterals[i]))`` with ``slice_as`` (fpn_carafe.py:211-259) in the reassembly's
    epilogue: no upsampled map, no second pass over the lateral.  The outputs are the 3x3 level convolutions, as in
    ``FPN``.  Every convolution is exact fp32 in every precision mode; the host never waits; the inputs are not written;
    an image's bits do not depend on the batch.  22 launches for the five levels of configs/carafe.

    Not built (NotImplementedError naming the argument): ``norm_cfg``, ``act_cfg``, ``order=('act', 'conv', 'norm')``,
    every ``upsample_cfg['type']`` but 'carafe', an encoder that is not 3x3 at dilation 1, ``out_channels`` or
    ``compressed_channels`` that is no multiple of 8, training."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, norm_cfg=None, act_cfg=None,
                 order=('conv', 'norm', 'act'),
                 upsample_cfg=dict(type='carafe', up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1)):
        super().__init__()
        assert isinstance(in_channels, list)
        if norm_cfg is not None:
            raise NotImplementedError(f'FPN_CARAFE: norm_cfg={norm_cfg} is not built')
        if act_cfg is not None:
            raise NotImplementedError(f'FPN_CARAFE: act_cfg={act_cfg} is not built (None in configs/carafe)')
        order = tuple(order)
        assert order in [('conv', 'norm', 'act'), ('act', 'conv', 'norm')]
        if order != ('conv', 'norm', 'act'):
            raise NotImplementedError(f'FPN_CARAFE: order={order} is not built')
        upsample_cfg = dict(upsample_cfg)
        self.upsample = upsample_cfg.get('type')
        assert self.upsample in ['nearest', 'bilinear', 'deconv', 'pixel_shuffle', 'carafe', None]
        if self.upsample != 'carafe':
            raise NotImplementedError(f"FPN_CARAFE: upsample_cfg type={self.upsample!r} is not built; 'carafe' only")
        if set(upsample_cfg) - set(_CARAFE_CFG_KEYS):
            raise NotImplementedError(f'FPN_CARAFE: upsample_cfg keys {sorted(set(upsample_cfg) - set(_CARAFE_CFG_KEYS))} '
                                      'are not built')
        up_kernel, up_group = upsample_cfg.get('up_kernel', 5), upsample_cfg.get('up_group', 1)
        compressed = upsample_cfg.get('compressed_channels', 64)
        if upsample_cfg.get('encoder_kernel', 3) != 3:
            raise NotImplementedError(f"FPN_CARAFE: encoder_kernel={upsample_cfg['encoder_kernel']} is not built; 3 only")
        if upsample_cfg.get('encoder_dilation', 1) != 1:
            raise NotImplementedError(f"FPN_CARAFE: encoder_dilation={upsample_cfg['encoder_dilation']} is not built; 1 only")
        if up_kernel not in (3, 5):
            raise NotImplementedError(f'FPN_CARAFE: up_kernel={up_kernel} is not built; 3 and 5 are')
        if out_channels % 8 != 0:
            raise NotImplementedError(f'FPN_CARAFE: out_channels={out_channels} is not a multiple of 8 (the any-width and '
                                      'the stride-2 3x3 kernels walk the input channels in chunks of 8)')
        if compressed % 8 != 0:
            raise NotImplementedError(f'FPN_CARAFE: compressed_channels={compressed} is not a multiple of 8 (the encoder\'s '
                                      '3x3 kernels walk the input channels in chunks of 8)')
        if up_group < 1 or out_channels % up_group != 0 or (out_channels // up_group) % 4 != 0:
            raise NotImplementedError(f'FPN_CARAFE: up_group={up_group} does not divide out_channels={out_channels} into '
                                      'groups of a multiple of 4 channels (the reassembly walks channel quads)')
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.norm_cfg, self.act_cfg, self.order = norm_cfg, act_cfg, order
        self.with_bias = True
        self.upsample_cfg = upsample_cfg
        self.up_kernel, self.up_group = up_kernel, up_group
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            assert num_outs >= self.num_ins - start_level
        else:
            # if end_level < inputs, no extra level is allowed (fpn_carafe.py:77-80)
            self.backbone_end_level = end_level
            assert end_level <= len(in_channels)
            assert num_outs == end_level - start_level
        assert 0 <= start_level < self.backbone_end_level
        self.start_level = start_level
        self.end_level = end_level

        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        self.upsample_modules = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            if i != self.backbone_end_level - 1:
                self.upsample_modules.append(_CarafeUp(out_channels, up_kernel, up_group, compressed))
            self.lateral_convs.append(_NeckConv(in_channels[i], out_channels, 1))
            self.fpn_convs.append(_NeckConv(out_channels, out_channels, 3))
        # extra levels (fpn_carafe.py:139-199): a 3x3 stride-2 lateral, the first on the last backbone stage
        for i in range(num_outs - self.backbone_end_level + self.start_level):
            cin = in_channels[self.backbone_end_level - 1] if i == 0 else out_channels
            self.upsample_modules.append(_CarafeUp(out_channels, up_kernel, up_group, compressed))
            self.fpn_convs.append(_NeckConv(out_channels, out_channels, 3))
            self.lateral_convs.append(_NeckConv(cin, out_channels, 3, stride=2))

    def init_weights(self):
        """fpn_carafe.py:202-209: xavier uniform weights and zero biases, then CARAFEPack's own rule for its two."""
        for m in list(self.lateral_convs) + list(self.fpn_convs):
            nn.init.xavier_uniform_(m.conv.weight, gain=1)
            nn.init.constant_(m.conv.bias, 0)
        for m in self.upsample_modules:
            m.init_weights()

    _conv3x3 = FPN._conv3x3

    def forward(self, inputs):
        """``inputs``: the backbone's stages, [B, in_channels[i], H_i, W_i]; returns the tuple of ``num_outs`` maps."""
        assert len(inputs) == len(self.in_channels)
        if torch.is_grad_enabled() and (any(x.requires_grad for x in inputs) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('FPN_CARAFE: training is not built; run inference under torch.no_grad()')
        for i, x in enumerate(inputs):
            if x.dim() != 4 or x.shape[1] != self.in_channels[i]:
                raise ValueError(f'FPN_CARAFE: input {i}: [B, {self.in_channels[i]}, H, W] expected, got {tuple(x.shape)}')
        fused = FPN_CARAFE_FUSED[0]
        used = self.backbone_end_level - self.start_level
        laterals = []
        for i, m in enumerate(self.lateral_convs):
            # fpn_carafe.py:245-250: the first extra lateral reads the last input, the later ones the lateral before them
            src = inputs[min(i + self.start_level, len(inputs) - 1)].contiguous() if i <= used else laterals[-1]
            c = m.conv
            if m.stride == 1:
                laterals.append(c.run(src))
                continue
            if src.shape[1] % 8 != 0 or not ops.conv3x3_s2_supported(src, c.out_channels):
                raise NotImplementedError(f'FPN_CARAFE: the stride-2 3x3 kernel does not take the extra level\'s input '
                                          f'{list(src.shape)} (lateral_convs.{i})')
            laterals.append(ops.conv3x3_s2(src, c.packed([c.in_channels]), c.bias.detach(), c.out_channels))
        for i in range(len(laterals) - 1, 0, -1):
            up, src, dst = self.upsample_modules[i - 1], laterals[i], laterals[i - 1]
            size = tuple(dst.shape[2:])
            if not ops.carafe_map_supported(src, self.up_kernel, self.up_group, size):
                raise NotImplementedError(f'FPN_CARAFE: level {i} {list(src.shape)} does not upsample into the lateral below '
                                          f'{list(dst.shape)} (2H - 1 <= OH <= 2H, 2W - 1 <= OW <= 2W)')
            enc = up.encode(src)
            if fused:
                ops.carafe_map(src, enc, self.up_kernel, self.up_group, addend=dst, out=dst)
            else:
                full = ops.carafe_map(src, enc, self.up_kernel, self.up_group)
                laterals[i - 1] = dst + full[:, :, :size[0], :size[1]]
        return tuple(self._conv3x3(m, lat) for m, lat in zip(self.fpn_convs, laterals))
