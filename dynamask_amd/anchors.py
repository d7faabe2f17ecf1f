"""``AnchorGenerator`` (mmdet/core/anchor/anchor_generator.py) under its registry name and kwargs.

The base anchors are computed on the host with the reference's own fp32 torch operations in its order
(``gen_single_level_base_anchors``), so that the device table the RPN kernels read (``base_anchor_table``) and the
materialised grid (``grid_anchors``, the composed path and the tests) carry the reference's bits."""
import numpy as np
import torch

from .registry import ANCHOR_GENERATORS


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


@ANCHOR_GENERATORS.register_module()
class AnchorGenerator:
    """anchor_generator.py:9-120.  ``strides`` per level (int or (x, y)); ``base_sizes`` default to the smaller stride;
    either ``scales`` or ``octave_base_scale`` with ``scales_per_octave``; ``centers`` per level or ``center_offset``."""

    def __init__(self, strides, ratios, scales=None, base_sizes=None, scale_major=True, octave_base_scale=None,
                 scales_per_octave=None, centers=None, center_offset=0.):
        if center_offset != 0 and centers is not None:
            raise ValueError(f'centers cannot be set when center_offset != 0, got {centers}')
        if not 0 <= center_offset <= 1:
            raise ValueError(f'center_offset should be in [0, 1], got {center_offset}')
        if centers is not None and len(centers) != len(strides):
            raise ValueError(f'one centre per stride expected, got {strides} and {centers}')
        self.strides = [_pair(s) for s in strides]
        self.base_sizes = [min(s) for s in self.strides] if base_sizes is None else list(base_sizes)
        if len(self.base_sizes) != len(self.strides):
            raise ValueError(f'one base size per stride expected, got {self.strides} and {self.base_sizes}')
        octave = octave_base_scale is not None and scales_per_octave is not None
        if octave == (scales is not None):
            raise ValueError('set either scales or octave_base_scale with scales_per_octave')
        if octave:
            scales = np.array([2 ** (i / scales_per_octave) for i in range(scales_per_octave)]) * octave_base_scale
        self.scales = torch.Tensor(scales)
        self.octave_base_scale, self.scales_per_octave = octave_base_scale, scales_per_octave
        self.ratios = torch.Tensor(ratios)
        self.scale_major, self.centers, self.center_offset = scale_major, centers, center_offset
        self.base_anchors = self.gen_base_anchors()
        self._tables = {}

    @property
    def num_base_anchors(self):
        return [b.size(0) for b in self.base_anchors]

    @property
    def num_levels(self):
        return len(self.strides)

    def gen_base_anchors(self):
        return [self.gen_single_level_base_anchors(size, self.scales, self.ratios,
                                                   None if self.centers is None else self.centers[i])
                for i, size in enumerate(self.base_sizes)]

    def gen_single_level_base_anchors(self, base_size, scales, ratios, center=None):
        """[len(ratios) * len(scales), 4] fp32 on the host: anchor_generator.py:142-185, operation for operation."""
        w = h = base_size
        if center is None:
            xc, yc = self.center_offset * w, self.center_offset * h
        else:
            xc, yc = center
        h_ratios = torch.sqrt(ratios)
        w_ratios = 1 / h_ratios
        if self.scale_major:
            ws = (w * w_ratios[:, None] * scales[None, :]).view(-1)
            hs = (h * h_ratios[:, None] * scales[None, :]).view(-1)
        else:
            ws = (w * scales[:, None] * w_ratios[None, :]).view(-1)
            hs = (h * scales[:, None] * h_ratios[None, :]).view(-1)
        return torch.stack([xc - 0.5 * ws, yc - 0.5 * hs, xc + 0.5 * ws, yc + 0.5 * hs], dim=-1)

    def single_level_grid_anchors(self, base_anchors, featmap_size, stride=(16, 16), device='cuda'):
        """[H * W * A, 4]: row (h * W + w) * A + a = base anchor a + (w sx, h sy, w sx, h sy), the integer shifts converted
        to fp32, one fp32 add per coordinate (anchor_generator.py:232-271)."""
        H, W = int(featmap_size[0]), int(featmap_size[1])
        sx = torch.arange(0, W, device=device) * stride[0]
        sy = torch.arange(0, H, device=device) * stride[1]
        xx = sx.repeat(H)
        yy = sy.view(-1, 1).repeat(1, W).view(-1)
        shifts = torch.stack([xx, yy, xx, yy], dim=-1).type_as(base_anchors)
        return (base_anchors[None, :, :] + shifts[:, None, :]).view(-1, 4)

    def grid_anchors(self, featmap_sizes, device='cuda'):
        if len(featmap_sizes) != self.num_levels:
            raise ValueError(f'{self.num_levels} feature map sizes expected, got {len(featmap_sizes)}')
        return [self.single_level_grid_anchors(self.base_anchors[i].to(device), featmap_sizes[i], self.strides[i], device)
                for i in range(self.num_levels)]

    def base_anchor_table(self, device):
        """(table fp32 [sum A_l, 4] on ``device``, first row of every level): what dm_rpn_decode reads."""
        key = str(torch.device(device))
        if key not in self._tables:
            rows, r = [], 0
            for b in self.base_anchors:
                rows.append(r)
                r += b.size(0)
            self._tables[key] = (torch.cat(self.base_anchors, 0).contiguous().to(device), rows)
        return self._tables[key]

    def __repr__(self):
        return (f'{type(self).__name__}(strides={self.strides}, ratios={self.ratios}, scales={self.scales}, '
                f'base_sizes={self.base_sizes}, scale_major={self.scale_major}, centers={self.centers}, '
                f'center_offset={self.center_offset})')
