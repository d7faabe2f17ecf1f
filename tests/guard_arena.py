"""The memory-safety net's tools, shared by test_guard_gpu.py, test_guard_surface_gpu.py and test_guard_arena_cpu.py.

``Arena`` / ``guarded``: while active, every device tensor made by torch's factories sits between two guard bands of
signalling patterns (float bands are NaN).  A store past either end of a buffer breaks a band (``Arena.check``); an
out-of-range READ that reaches a result makes it non-finite (``_finite``).

``LaunchLog``: a proxy around the loaded library for the duration of a ``with`` block.  From the argument roles of
include/dynamask_hip.h (``hazard.parse_header``) it notes, for every call of an entry point that takes a stream, whether
each non-null pointer the kernel stores through (``out``, ``out[]``) and reads through (``in``, ``in[]``) lies in the
interior of a live arena block.  The coverage tables at the end of this file are held to the header by
test_guard_arena_cpu.py and to the device runs by test_guard_surface_gpu.py."""
import bisect
import collections
import contextlib
import ctypes

import torch

GUARD = 256          # elements on each side (1 KB of fp32): keeps the interior 256-byte aligned
_PATTERN = {1: 0x5A, 2: 0x5A5A, 4: 0x7FC0DEAD, 8: 0x7FF8DEAD7FC0DEAD}      # 4 / 8 bytes: NaN bit patterns


class Arena:
    """Guarded allocation: replaces torch's tensor factories for CUDA tensors while active."""

    def __init__(self):
        self.blocks = []          # (parent int-view, n interior elements, pattern)
        self.spans = []           # (first interior byte, one past the last) of every block, for LaunchLog
        self.count = 0

    def _int_dtype(self, dtype):
        return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[torch.empty((), dtype=dtype).element_size()]

    def alloc(self, shape, dtype, device, fill=None):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        idt = self._int_dtype(dtype)
        esz = torch.empty((), dtype=dtype).element_size()
        pat = _PATTERN[esz]
        if esz == 1:
            raw = self._empty((n + 2 * GUARD,), dtype=idt, device=device)
            raw.fill_(pat)
        else:
            raw = self._full((n + 2 * GUARD,), pat if pat < 2 ** 63 else pat - 2 ** 64, dtype=torch.int64 if esz == 8 else idt,
                             device=device)
        inner = raw[GUARD:GUARD + n].view(dtype).view(shape)
        if fill is not None:
            inner.fill_(fill)
        self.blocks.append((raw, n, pat))
        self.spans.append((inner.data_ptr(), inner.data_ptr() + n * esz))
        self.count += 1
        return inner

    def check(self):
        torch.cuda.synchronize()
        bad = []
        for k, (raw, n, pat) in enumerate(self.blocks):
            p = pat if pat < 2 ** 63 else pat - 2 ** 64
            lo, hi = raw[:GUARD], raw[GUARD + n:]
            if not bool((lo == p).all()) or not bool((hi == p).all()):
                bad.append((k, n, int((lo != p).sum()), int((hi != p).sum())))
        assert not bad, f'guard bands overwritten (block, elements, cells before, cells after): {bad[:8]}'
        return len(self.blocks)


@contextlib.contextmanager
def guarded(monkeypatch):
    arena = Arena()
    o_empty, o_zeros, o_full, o_ones = torch.empty, torch.zeros, torch.full, torch.ones
    o_empty_like, o_zeros_like = torch.empty_like, torch.zeros_like
    arena._empty, arena._full = o_empty, o_full

    def _is_cuda(device):
        return device is not None and torch.device(device).type == 'cuda'

    def _shape(args):
        return tuple(args[0]) if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)) else tuple(args)

    def mk(orig, fill):
        def f(*args, dtype=None, device=None, **kw):
            if not _is_cuda(device) or kw.get('out') is not None or kw.get('memory_format') is not None:
                return orig(*args, dtype=dtype, device=device, **kw)
            t = arena.alloc(_shape(args), dtype or torch.float32, device, fill)
            return t.requires_grad_(True) if kw.get('requires_grad') else t
        return f

    def full(size, fill_value, *, dtype=None, device=None, **kw):
        if not _is_cuda(device):
            return o_full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = torch.float32 if isinstance(fill_value, float) else (torch.bool if isinstance(fill_value, bool) else torch.int64)
        return arena.alloc(size, dtype, device, fill_value)

    def like(fill):
        def f(t, *, dtype=None, device=None, **kw):
            device = device or t.device
            if not _is_cuda(device) or not t.is_contiguous():
                return (o_empty_like if fill is None else o_zeros_like)(t, dtype=dtype, device=device, **kw)
            return arena.alloc(t.shape, dtype or t.dtype, device, fill)
        return f

    def new(fill):
        def f(self, *args, dtype=None, device=None, **kw):
            device = device or self.device
            if not _is_cuda(device):
                return (o_empty if fill is None else o_zeros)(*args, dtype=dtype or self.dtype, device=device)
            return arena.alloc(_shape(args), dtype or self.dtype, device, fill)
        return f

    def new_full(self, size, fill_value, *, dtype=None, device=None, **kw):
        device = device or self.device
        if not _is_cuda(device):
            return o_full(size, fill_value, dtype=dtype or self.dtype, device=device)
        return arena.alloc(size, dtype or self.dtype, device, fill_value)

    # copies the package hands to a kernel as an output (``x.clone()`` as a ping-pong buffer or a gradient to accumulate
    # into, ``torch.cat`` of per-exit predictions merged in place): guarded where autograd does not have to see them
    o_clone, o_cat = torch.Tensor.clone, torch.cat

    def _plain(t):
        return t.is_cuda and t.is_contiguous() and not t.is_sparse and not (torch.is_grad_enabled() and t.requires_grad)

    def clone(self, *args, **kw):
        if args or kw or not _plain(self):
            return o_clone(self, *args, **kw)
        g = arena.alloc(self.shape, self.dtype, self.device)
        g.copy_(self)
        return g

    def cat(tensors, dim=0, **kw):
        ts = list(tensors) if isinstance(tensors, (list, tuple)) else None
        if kw or not ts or not isinstance(dim, int) or any(not isinstance(t, torch.Tensor) or not _plain(t) or t.dim() == 0
                                                          or t.dtype != ts[0].dtype or t.dim() != ts[0].dim() for t in ts):
            return o_cat(tensors, dim, **kw)
        d = dim % ts[0].dim()
        shape = list(ts[0].shape)
        shape[d] = sum(t.shape[d] for t in ts)
        return o_cat(ts, d, out=arena.alloc(shape, ts[0].dtype, ts[0].device))

    monkeypatch.setattr(torch.Tensor, 'clone', clone)
    monkeypatch.setattr(torch, 'cat', cat)
    monkeypatch.setattr(torch, 'empty', mk(o_empty, None))
    monkeypatch.setattr(torch, 'zeros', mk(o_zeros, 0))
    monkeypatch.setattr(torch, 'ones', mk(o_ones, 1))
    monkeypatch.setattr(torch, 'full', full)
    monkeypatch.setattr(torch, 'empty_like', like(None))
    monkeypatch.setattr(torch, 'zeros_like', like(0))
    monkeypatch.setattr(torch.Tensor, 'new_empty', new(None))
    monkeypatch.setattr(torch.Tensor, 'new_zeros', new(0))
    monkeypatch.setattr(torch.Tensor, 'new_full', new_full)
    try:
        yield arena
    finally:
        monkeypatch.undo()


def _put(arena, t):
    """Copy a host tensor into guarded device storage."""
    g = arena.alloc(t.shape, t.dtype, torch.device('cuda'))
    g.copy_(t)
    return g


def _finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t.is_floating_point())


# ------------------------------------------------------------------------------------------------ the launch log
def launching(roles):
    """The entry points of ``roles`` (hazard.parse_header()) that take a stream: those that launch."""
    return {name for name, r in roles.items() if 'stream' in r}


def _address(a):
    """The address in a pointer argument as ops.py passes them: a ctypes.c_void_p, an int or None."""
    v = getattr(a, 'value', a)
    return int(v) if isinstance(v, int) and v else 0


def _addresses(a):
    """The non-null addresses in a host array of device pointers (ops._ptr_array: a ctypes array of c_void_p)."""
    if a is None or isinstance(a, ctypes.c_void_p) and not a.value:
        return []
    return [int(v) for v in a if v]


class _LoggedLib:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        roles = self._log.roles.get(name)
        if roles is None or 'stream' not in roles:
            return fn

        def call(*args):
            self._log.note(name, roles, args)
            return fn(*args)
        return call


class LaunchLog:
    """with LaunchLog(arena) as log: ...   ``_lib.lib()`` hands out a logging proxy around what it handed out before
    (the library, or the hazard tracker's proxy under DM_HAZARD); both module attributes are restored afterwards.

      launches[name]                  calls of a launching entry point
      guarded_launches[name]          of those, the calls whose every non-null store pointer lay inside an arena block
      stores[(name, arg)] = [g, u]    store pointers seen in / outside the arena, per argument index
      reads[(name, arg)]  = [g, u]    the same for the pointers the kernel reads through (reported, not asserted)"""

    def __init__(self, arena, roles=None, module=None):
        if roles is None:
            from dynamask_amd import hazard
            roles = hazard.parse_header()
        self.arena, self.roles, self._module = arena, roles, module
        self.launches = collections.Counter()
        self.guarded_launches = collections.Counter()
        self.stores, self.reads = {}, {}
        self._lo, self._hi, self._seen = [], [], 0

    # ---- interval membership
    def inside(self, p):
        """Does address ``p`` lie in the interior of a live arena block?  (An empty block holds its own address only.)"""
        spans = self.arena.spans
        if self._seen != len(spans):
            order = sorted(spans)
            self._lo, self._hi, self._seen = [s[0] for s in order], [s[1] for s in order], len(spans)
        i = bisect.bisect_right(self._lo, p) - 1          # (the arena keeps every block alive: no two interiors overlap)
        return i >= 0 and (p < self._hi[i] or p == self._lo[i])

    def note(self, name, roles, args):
        self.launches[name] += 1
        clean = True
        for i, (role, a) in enumerate(zip(roles, args)):
            if role in ('in', 'out'):
                ptrs = [_address(a)] if _address(a) else []
            elif role in ('in[]', 'out[]'):
                ptrs = _addresses(a)
            else:
                continue
            table = self.stores if role.startswith('out') else self.reads
            for p in ptrs:
                ok = self.inside(p)
                table.setdefault((name, i), [0, 0])[0 if ok else 1] += 1
                if not ok and role.startswith('out'):
                    clean = False
        if clean:
            self.guarded_launches[name] += 1

    # ---- what the tests ask
    def reached_guarded(self):
        return {n for n, c in self.guarded_launches.items() if c > 0}

    def unguarded_stores(self):
        return {k for k, (g, u) in self.stores.items() if u > 0}

    def shares(self):
        """(launches, share of guarded store pointers, share of guarded read pointers)."""
        def share(table):
            g, u = sum(v[0] for v in table.values()), sum(v[1] for v in table.values())
            return g / (g + u) if g + u else 1.0
        return sum(self.launches.values()), share(self.stores), share(self.reads)

    def summary(self):
        return dict(launches=dict(self.launches), guarded_launches=dict(self.guarded_launches),
                    stores={f'{n}:{i}': v for (n, i), v in sorted(self.stores.items())},
                    reads={f'{n}:{i}': v for (n, i), v in sorted(self.reads.items())})

    # ---- installation
    def __enter__(self):
        m = self._module
        if m is None:
            from dynamask_amd import _lib as m
            m.lib()                                   # loaded (and, under DM_HAZARD, wrapped) before it is patched
            self._module = m
        self._saved = (m._LIB, m._PROXY)
        m._LIB = _LoggedLib(m._LIB, self)
        if m._PROXY is not None:
            m._PROXY = _LoggedLib(m._PROXY, self)
        return self

    def __exit__(self, *exc):
        self._module._LIB, self._module._PROXY = self._saved
        return False


# ------------------------------------------------------------------------------------------------ coverage tables
# pass of test_guard_surface_gpu.py -> the launching entry points it reaches with every store pointer inside the arena.
# Filled from a device run; test_guard_arena_cpu.py holds the union to the header, the GPU test holds each pass to its set.
EXPECTED_REACHED = {
    'backbones': {
        'dm_avgpool2x2_ceil_fwd', 'dm_conv2d_fwd', 'dm_conv3x3_dil_fwd', 'dm_conv3x3_grouped_fwd',
        'dm_conv3x3_s2_c3_fwd', 'dm_conv3x3_s2_fwd', 'dm_conv3x3_slices_fwd', 'dm_conv7x7_s2_fwd',
        'dm_conv_pack_weight', 'dm_maxpool3x3_s2_fwd', 'dm_subsample2_fwd'
    },
    'necks_rpn': {
        'dm_carafe_map_fwd', 'dm_conv2d_fwd', 'dm_conv2d_up_add_fwd', 'dm_conv3x3_s2_fwd', 'dm_conv7x7_s2_fwd',
        'dm_conv_pack_weight', 'dm_conv_pack_weight_batch', 'dm_maxpool3x3_s2_fwd', 'dm_nms_mask_segmented',
        'dm_nms_reduce_segmented', 'dm_rpn_decode', 'dm_rpn_merge', 'dm_rpn_select', 'dm_subsample2_fwd'
    },
    'roi_dynamask': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_bn_relu_maxpool_fwd', 'dm_boundary_merge',
        'dm_boundary_merge_chain', 'dm_class_logits_fwd', 'dm_class_logits_up2x_fwd', 'dm_conv1x1_group_fwd',
        'dm_conv2d_fwd', 'dm_conv2d_fwd_ws', 'dm_conv_pack_weight_batch', 'dm_deform_conv_fwd', 'dm_deform_conv_fwd_ws',
        'dm_deform_conv_tout_fwd', 'dm_fc_fwd', 'dm_gumbel_select_fwd', 'dm_merge_aug_bboxes', 'dm_merge_aug_masks',
        'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_paste_masks', 'dm_paste_masks_multi',
        'dm_paste_rle', 'dm_paste_rle_multi', 'dm_roi_align_fwd_ws', 'dm_stage_head_fwd', 'dm_upsample2x_bilinear_fwd'
    },
    'roi_fcn': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_conv2d_fwd', 'dm_conv_pack_weight_batch', 'dm_deconv2x2_fwd',
        'dm_deconv_pack_weight', 'dm_fc_fwd', 'dm_merge_aug_bboxes', 'dm_merge_aug_masks', 'dm_nms_mask',
        'dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_paste_masks', 'dm_paste_masks_multi', 'dm_paste_rle',
        'dm_paste_rle_multi', 'dm_roi_align_fwd_ws'
    },
    'roi_refinemask': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_boundary_merge', 'dm_class_logits_fwd', 'dm_conv2d_fwd',
        'dm_conv3x3_dil_fwd', 'dm_conv3x3_multidil_fwd', 'dm_conv_pack_weight_batch', 'dm_fc_fwd',
        'dm_merge_aug_bboxes', 'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented',
        'dm_paste_masks', 'dm_paste_masks_multi', 'dm_paste_rle', 'dm_paste_rle_multi', 'dm_roi_align_fwd_ws',
        'dm_sigmoid_fwd', 'dm_upsample2x_bilinear_fwd'
    },
    'roi_pointrend': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_conv2d_fwd', 'dm_conv_pack_weight', 'dm_fc_fwd',
        'dm_merge_aug_bboxes', 'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented',
        'dm_paste_masks', 'dm_paste_masks_multi', 'dm_paste_rle', 'dm_paste_rle_multi', 'dm_pixel_unshuffle2x',
        'dm_point_gather_fwd', 'dm_point_mlp_fwd', 'dm_point_sample_fwd', 'dm_point_select', 'dm_roi_align_fwd_ws',
        'dm_upsample2x_bilinear_fwd'
    },
    'roi_msrcnn': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_conv2d_fwd', 'dm_conv2d_fwd_ws', 'dm_conv3x3_s2_fwd',
        'dm_conv_pack_weight_batch', 'dm_deconv2x2_fwd', 'dm_deconv_pack_weight', 'dm_fc_fwd', 'dm_mask_iou_input',
        'dm_mask_iou_scores', 'dm_merge_aug_bboxes', 'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented',
        'dm_nms_reduce_segmented', 'dm_paste_masks', 'dm_paste_masks_multi', 'dm_paste_rle', 'dm_paste_rle_multi',
        'dm_roi_align_fwd_ws'
    },
    'roi_pointrefine': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_boundary_merge', 'dm_class_logits_fwd', 'dm_conv1x1_group_fwd',
        'dm_conv2d_fwd', 'dm_conv3x3_dil_fwd', 'dm_conv_pack_weight', 'dm_conv_pack_weight_batch', 'dm_fc_fwd',
        'dm_merge_aug_bboxes', 'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented',
        'dm_paste_masks', 'dm_paste_masks_multi', 'dm_paste_rle', 'dm_paste_rle_multi', 'dm_point_feat_gather',
        'dm_point_refine_mlp', 'dm_point_topk_select', 'dm_roi_align_fwd_ws', 'dm_upsample2x_bilinear_fwd'
    },
    'roi_cascade': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_cascade_refine', 'dm_conv1x1_group_fwd', 'dm_conv2d_group_fwd',
        'dm_conv_pack_weight_batch', 'dm_deconv2x2_group_fwd', 'dm_deconv_pack_weight', 'dm_fc_fwd',
        'dm_merge_aug_bboxes', 'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented',
        'dm_paste_masks', 'dm_paste_masks_multi', 'dm_paste_rle', 'dm_paste_rle_multi', 'dm_roi_align_fwd_ws'
    },
    'roi_htc': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_cascade_refine', 'dm_conv1x1_group_fwd', 'dm_conv2d_fwd',
        'dm_conv2d_fwd_ws', 'dm_conv2d_post_add_fwd', 'dm_conv3x3_dil_fwd', 'dm_conv_pack_weight_batch',
        'dm_deconv2x2_group_fwd', 'dm_deconv_pack_weight', 'dm_fc_fwd', 'dm_merge_aug_bboxes', 'dm_merge_aug_masks',
        'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_paste_masks', 'dm_paste_masks_multi',
        'dm_paste_rle', 'dm_paste_rle_multi', 'dm_resize_bilinear_fwd', 'dm_roi_align_add_fwd', 'dm_roi_align_fwd_ws'
    },
    'roi_grid': {
        'dm_bbox_decode', 'dm_conv2d_fwd', 'dm_conv3x3_s2_fwd', 'dm_conv_pack_weight_batch',
        'dm_deconv4x4_s2_grouped_fwd', 'dm_fc_fwd', 'dm_grid_fusion_fwd', 'dm_grid_get_bboxes', 'dm_group_norm_fwd',
        'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_roi_align_fwd_ws'
    },
    'roi_double': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_conv2d_fwd', 'dm_conv_pack_weight', 'dm_fc_fwd',
        'dm_global_avg_pool_fwd', 'dm_merge_aug_bboxes', 'dm_nms_mask', 'dm_nms_mask_segmented',
        'dm_nms_reduce_segmented', 'dm_roi_align_fwd_ws', 'dm_roi_align_scaled_fwd'
    },
    'roi_c4': {
        'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_conv2d_fwd', 'dm_conv_pack_weight', 'dm_conv_pack_weight_batch',
        'dm_deconv2x2_fwd', 'dm_deconv_pack_weight', 'dm_fc_fwd', 'dm_global_avg_pool_fwd', 'dm_merge_aug_bboxes',
        'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_paste_masks',
        'dm_paste_masks_multi', 'dm_paste_rle', 'dm_paste_rle_multi', 'dm_roi_align_strided_fwd'
    },
    'detectors': {
        'dm_avgpool2x2_ceil_fwd', 'dm_bbox_decode', 'dm_bbox_mapping_multi', 'dm_boundary_merge_chain', 'dm_carafe_fwd',
        'dm_carafe_map_fwd', 'dm_class_logits_fwd', 'dm_conv1x1_group_fwd', 'dm_conv2d_fwd', 'dm_conv2d_fwd_ws',
        'dm_conv2d_up_add_fwd', 'dm_conv3x3_dil_fwd', 'dm_conv3x3_grouped_fwd', 'dm_conv3x3_s2_c3_fwd',
        'dm_conv3x3_s2_fwd', 'dm_conv3x3_slices_fwd', 'dm_conv7x7_s2_fwd', 'dm_conv_pack_weight',
        'dm_conv_pack_weight_batch', 'dm_deconv2x2_fwd', 'dm_deconv_pack_weight', 'dm_deform_conv_fwd_ws',
        'dm_deform_conv_tout_fwd', 'dm_fc_fwd', 'dm_global_avg_pool_fwd', 'dm_maxpool3x3_s2_fwd', 'dm_merge_aug_bboxes',
        'dm_merge_aug_masks', 'dm_nms_mask', 'dm_nms_mask_segmented', 'dm_nms_reduce_segmented', 'dm_paste_masks',
        'dm_paste_rle_multi', 'dm_preprocess_u8_fwd', 'dm_proposals_mapping_back', 'dm_roi_align_fwd_ws',
        'dm_roi_align_strided_fwd', 'dm_rpn_decode', 'dm_rpn_merge', 'dm_rpn_select', 'dm_stage_head_fwd',
        'dm_subsample2_fwd', 'dm_upsample2x_bilinear_fwd'
    },
    'training': {
        'dm_bbox_encode', 'dm_bbox_overlaps', 'dm_bn_relu_maxpool_bwd', 'dm_bn_relu_maxpool_fwd', 'dm_channel_sum',
        'dm_class_balance_fwd_bwd', 'dm_class_logits_bwd_slab', 'dm_class_logits_fwd', 'dm_clip_scale', 'dm_conv2d_fwd',
        'dm_conv2d_fwd_masked', 'dm_conv2d_wgrad_fx', 'dm_conv2d_wgrad_slab', 'dm_conv_pack_weight',
        'dm_conv_pack_weight_batch', 'dm_dcn_weight_permute', 'dm_deform_col2im', 'dm_deform_conv_fwd',
        'dm_deform_coord_grad', 'dm_deform_im2col', 'dm_detail_target', 'dm_fc_fwd', 'dm_fx_to_float',
        'dm_gumbel_select_bwd', 'dm_gumbel_select_fwd', 'dm_l1_loss_fwd_bwd', 'dm_mask_loss_stage',
        'dm_mask_target_rois', 'dm_max_iou_assign', 'dm_point_sample_bwd', 'dm_point_sample_bwd_fx',
        'dm_point_sample_fwd', 'dm_polygon_mask_targets', 'dm_random_sample', 'dm_relu_bwd', 'dm_roi_align_bwd',
        'dm_roi_align_fwd_ws', 'dm_scale', 'dm_sgd_momentum_step', 'dm_sigmoid_bwd', 'dm_softmax_ce_fwd_bwd',
        'dm_sumsq', 'dm_threshold_ge', 'dm_upsample2x_bilinear_bwd', 'dm_upsample2x_bilinear_fwd'
    },
    'leftovers': {
        'dm_bn_relu_maxpool_argmax', 'dm_bn_stats', 'dm_carafe_bwd', 'dm_channel_sum', 'dm_channel_sum_fx',
        'dm_class_logits_bwd', 'dm_class_logits_bwd_fx', 'dm_conv2d_wgrad', 'dm_conv2d_wgrad_fx',
        'dm_conv_pack_weight_bf16x3', 'dm_deconv_pack_weight_bf16x3', 'dm_deform_col2im_coord', 'dm_fx_to_float',
        'dm_ignore_columns', 'dm_mask_loss_fwd_bwd', 'dm_paste_masks', 'dm_point_scatter', 'dm_point_scatter_rows',
        'dm_rle_encode_canvas', 'dm_sigmoid_bwd', 'dm_upsample2x_nearest_bwd', 'dm_upsample2x_nearest_fwd'
    },
}

# launching entry points that no file of dynamask_amd/ names: nothing in the package can launch them.
NO_CALL_SITE = {
    'dm_roi_align_fwd': 'superseded by dm_roi_align_fwd_ws, which ops.roi_align always calls (kept for C callers)',
}

# (entry point, argument index) pairs stored through while outside the arena, over all passes.
UNGUARDED_STORES = {
    # MaskPre's BatchNorm in train mode updates its running_mean buffer in place: a module buffer, allocated when the
    # head is built, before the pass (training pass, both accumulation modes)
    ('dm_bn_stats', 6): 'mask_predictor.bn*.running_mean, a module buffer from before the pass',
    # the same layers' running_var buffer
    ('dm_bn_stats', 7): 'mask_predictor.bn*.running_var, a module buffer from before the pass',
}
