"""RoI extractors behind the reference's ROI_EXTRACTORS registry.

Mirrors ``mmdet/models/roi_heads/roi_extractors/{base_roi_extractor,
single_level_roi_extractor}.py`` (constructor kwargs, ``num_inputs``,
``map_roi_levels``, ``forward(feats, rois)``).  The per-level loop + boolean
scatter of the reference (single_level_roi_extractor.py:73-80) is ONE fused
kernel launch here (level map inside the kernel).
"""
import torch
import torch.nn as nn

from . import ops
from .registry import ROI_EXTRACTORS, ROI_LAYERS


@ROI_LAYERS.register_module()
class RoIAlign(nn.Module):
    """Parameter holder with mmcv.ops.RoIAlign's constructor signature."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True,
                 use_torchvision=False):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size)
        if output_size[0] != output_size[1]:
            raise ValueError('only square RoIAlign outputs are supported')
        if pool_mode != 'avg' or not aligned:
            raise NotImplementedError('dynamask_amd RoIAlign implements pool_mode="avg", aligned=True '
                                      '(what configs/dynamask uses)')
        self.output_size = tuple(output_size)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)
        self.pool_mode = pool_mode
        self.aligned = aligned

    def forward(self, input, rois):
        return ops.roi_align([input], rois, self.output_size[0], [self.spatial_scale], self.sampling_ratio)


class BaseRoIExtractor(nn.Module):
    def __init__(self, roi_layer, out_channels, featmap_strides):
        super().__init__()
        self.roi_layers = self.build_roi_layers(roi_layer, featmap_strides)
        self.out_channels = out_channels
        self.featmap_strides = featmap_strides
        self.fp16_enabled = False

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def init_weights(self):
        pass

    @staticmethod
    def roi_rescale(rois, scale_factor):
        """base_roi_extractor.py:57-80: RoIs [n, 5] scaled about their centres, one float32 rounding per operation in the
        reference's order -- centre = (lo + hi) * 0.5, half = ((hi - lo) * scale_factor) * 0.5, centre -/+ half.  The
        extraction does this inside its launch (dm_roi_align_scaled_fwd); this is the host form of the same arithmetic."""
        lo, hi = rois[:, 1:3], rois[:, 3:5]
        centre = (lo + hi) * 0.5
        half = ((hi - lo) * scale_factor) * 0.5
        return torch.cat([rois[:, :1], centre - half, centre + half], dim=1)

    def build_roi_layers(self, layer_cfg, featmap_strides):
        cfg = layer_cfg.copy()
        layer_type = cfg.pop('type')
        layer_cls = ROI_LAYERS.get(layer_type)
        if layer_cls is None:
            raise KeyError(f'{layer_type} is not a supported RoI layer')
        return nn.ModuleList([layer_cls(spatial_scale=1 / s, **cfg) for s in featmap_strides])


@ROI_EXTRACTORS.register_module()
class SingleRoIExtractor(BaseRoIExtractor):
    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super().__init__(roi_layer, out_channels, featmap_strides)
        self.finest_scale = finest_scale

    def map_roi_levels(self, rois, num_levels):
        """Level index per RoI, computed by the kernel's own level map (so the
        answer is the one the extraction uses)."""
        if rois.shape[0] == 0:
            return torch.zeros((0,), dtype=torch.long, device=rois.device)
        lay = self.roi_layers[0]
        dummy = [torch.zeros((1, 1, 1, 1), device=rois.device) for _ in range(num_levels)]
        r = rois.clone()
        r[:, 0] = -1          # batch index out of range: the kernel writes zeros, but still reports levels
        _, lv = ops.roi_align(dummy, r.contiguous(), 1, [1.0] * num_levels, lay.sampling_ratio,
                              float(self.finest_scale), return_levels=True)
        return lv.long()

    def supports_bin_step(self, feats, bin_step):
        """Does ``forward(feats, rois, bin_step=bin_step)`` run (dm_roi_align_strided_supported)?  Host only."""
        feats = list(feats)[:self.num_inputs]
        return len(feats) == self.num_inputs and ops.roi_align_strided_supported(
            [tuple(f.shape[2:]) for f in feats], feats[0].shape[1], self.roi_layers[0].output_size[0], bin_step)

    def forward(self, feats, rois, roi_scale_factor=None, bin_step=None):
        """``roi_scale_factor`` (single_level_roi_extractor.py:69-71): the levels come from ``rois`` as given, the samples
        from the boxes rescaled about their centres (base_roi_extractor.py:57-80), inside the same launch.
        ``bin_step`` (extension; None: today's call): only the bins (i * bin_step, j * bin_step) of the extraction,
        [N, C, ceil(P / bin_step), ceil(P / bin_step)] -- what a stride-``bin_step`` 1x1 convolution reads of it."""
        lay = self.roi_layers[0]
        P = lay.output_size[0]
        feats = list(feats)[:self.num_inputs]
        if len(feats) != self.num_inputs:
            raise ValueError(f'expected {self.num_inputs} feature maps, got {len(feats)}')
        if self.num_inputs == 1:
            roi_scale_factor = None       # single_level_roi_extractor.py:64-67 returns before the rescale: one level ignores it
        if bin_step is not None:
            if isinstance(bin_step, bool) or not isinstance(bin_step, int) or bin_step < 1:
                raise ValueError(f'bin_step must be an int >= 1, got {bin_step!r}')
            if roi_scale_factor is not None:
                raise NotImplementedError('SingleRoIExtractor: bin_step together with roi_scale_factor is not built')
            P = -(-P // bin_step)
        if rois.shape[0] == 0:
            return feats[0].new_zeros((0, self.out_channels, P, P))
        scales = [l.spatial_scale for l in self.roi_layers]
        if bin_step is not None:
            return ops.roi_align(feats, rois, lay.output_size[0], scales, lay.sampling_ratio, float(self.finest_scale),
                                 bin_step=bin_step)
        return ops.roi_align(feats, rois, P, scales, lay.sampling_ratio, float(self.finest_scale),
                             roi_scale_factor=roi_scale_factor)


@ROI_LAYERS.register_module()
class SimpleRoIAlign(nn.Module):
    """Parameter holder with mmcv.ops.SimpleRoIAlign's constructor signature: ``point_sample`` of the feature map at
    the ``output_size`` x ``output_size`` RoI-relative cell centres (dm_point_sample_fwd)."""

    def __init__(self, output_size, spatial_scale, aligned=True):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size)
        if output_size[0] != output_size[1]:
            raise ValueError('only square SimpleRoIAlign outputs are supported')
        if not aligned:
            raise NotImplementedError('dynamask_amd SimpleRoIAlign implements aligned=True (align_corners=False)')
        self.output_size = tuple(output_size)
        self.spatial_scale = float(spatial_scale)
        self.aligned = aligned

    def forward(self, input, rois):
        return ops.point_sample(input, rois, self.output_size[0], self.spatial_scale)


@ROI_EXTRACTORS.register_module()
class GenericRoIExtractor(BaseRoIExtractor):
    """``GenericRoIExtractor`` -- mmdet/models/roi_heads/roi_extractors/generic_roi_extractor.py: the forms
    configs/point_rend uses, i.e. ONE level (then the extraction is ``roi_layers[0](feats[0], rois)``, :43-46) without
    pre- / post-processing modules.  Several levels or plugin modules raise NotImplementedError."""

    def __init__(self, aggregation='sum', pre_cfg=None, post_cfg=None, **kwargs):
        super().__init__(**kwargs)
        if aggregation not in ('sum', 'concat'):
            raise ValueError(f'aggregation must be "sum" or "concat", got {aggregation!r}')
        if len(self.featmap_strides) != 1:
            raise NotImplementedError('GenericRoIExtractor: one feature level only (configs/point_rend)')
        if pre_cfg is not None or post_cfg is not None:
            raise NotImplementedError('GenericRoIExtractor: pre_cfg / post_cfg are None in configs/point_rend')
        self.aggregation = aggregation
        self.with_pre = self.with_post = False

    def forward(self, feats, rois, roi_scale_factor=None):
        if roi_scale_factor is not None:
            raise NotImplementedError('roi_scale_factor is not used by the PointRend path')
        feats = list(feats)[:self.num_inputs]
        if len(feats) != self.num_inputs:
            raise ValueError(f'expected {self.num_inputs} feature maps, got {len(feats)}')
        lay = self.roi_layers[0]
        if rois.shape[0] == 0:
            P = lay.output_size[0]
            return feats[0].new_zeros((0, self.out_channels, P, P))
        return lay(feats[0].contiguous(), rois.contiguous())
