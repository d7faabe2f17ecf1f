"""Operator bindings: torch device tensors -> raw pointers -> C ABI.

PyTorch is plumbing here (device memory, streams); all arithmetic runs in
libdynamask_hip.so.  Every function requires contiguous fp32 tensors on a HIP
device and raises otherwise -- no eager fallback.
"""
import ctypes

import torch

from . import _abi, _lib, hazard
from . import precision as _precision
from ._lib import check, lib


import os

# bumped whenever a kernel rewrites parameter memory behind torch's back (the fused
# SGD step), so that packed-weight caches refresh
WEIGHT_EPOCH = [0]

# DM_DETERMINISTIC=1 (or setting this flag): every cross-workgroup accumulation of the training step goes through
# the *_fx entry points (64-bit fixed-point cells, order-independent) and is converted once: two runs of a training
# loop give bit-identical parameters.  Costs one zero-fill and one conversion per accumulated tensor.
DETERMINISTIC = [os.environ.get('DM_DETERMINISTIC', '0') == '1']


def _fx_like(t):
    return torch.zeros(t.shape, device=t.device, dtype=torch.int64)


def _fx_finish(fx, out, accumulate):
    check(lib().dm_fx_to_float(_p(fx), fx.numel(), _p(out), 1 if accumulate else 0, 0, _stream()), 'dm_fx_to_float')
    return out


# the current stream's handle straight from the binding (0.4 us; torch.cuda.current_stream() builds a Stream object and
# resolves the device twice: 8 us x 160 calls of a training step), with the public path as the fallback
_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_CUR_DEVICE = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    if _RAW_STREAM is not None and _CUR_DEVICE is not None:
        return ctypes.c_void_p(_RAW_STREAM(_CUR_DEVICE()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a tensor')
    if not t.is_cuda:
        raise RuntimeError(f'{name}: dynamask_amd operators run on the MI355X only (got a {t.device} tensor); '
                           'there is no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: tensor must be contiguous (NCHW)')
    return t


def _chk_src(t):
    """A conv source may be a channel slice of a wider NCHW tensor: channels,
    rows and columns dense, arbitrary batch stride."""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and \
            not t.is_contiguous():
        _, C, H, W = t.shape
        if t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W and t.stride(0) >= C * H * W:
            return t
    return _chk(t, 'src')


def _p(t):
    if t is None:
        return ctypes.c_void_p(0)
    if hazard.ENABLED[0]:
        hazard.note_ptr(t)          # (DM_HAZARD: the tracker learns which tensor the pointer came from)
    return ctypes.c_void_p(t.data_ptr())


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    if hazard.ENABLED[0]:
        hazard.note_ptr_array(arr, tensors)
    return arr


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _float_array(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


# ------------------------------------------------------------------ RoIAlign
# Extractions go through dm_roi_align_fwd_ws with the scratch buffer dm_roi_align_workspace_bytes asks for (ROI_WORKSPACE
# below): where it asks for one (14x14 extractions of 192 .. 1024 RoIs by default) the library orders the RoIs by level and
# position on the device first (DM_ROI_SORT, default on: 57 -> 50.7 us for 512 RoIs, the same bits)
ROI_WORKSPACE = True          # (tests compare with the unordered kernel by clearing it)


def roi_align(feats, rois, output_size, spatial_scales, sampling_ratio=0, finest_scale=56.0, return_levels=False,
              roi_scale_factor=None, out=None, bin_step=None):
    """``bin_step`` (an int >= 1; None: the dense extraction): only the bins (i * bin_step, j * bin_step) are sampled and
    stored, out [N, C, Po, Po] with Po = ceil(output_size / bin_step) (dm_roi_align_strided_fwd): the bits of the dense call
    without a workspace at those bins.  Not together with ``roi_scale_factor``.
    ``roi_scale_factor`` (a float > 0; None: not given): the FPN level -- and ``levels`` -- is the box's as given, the
    samples are those of the box rescaled about its centre (dm_roi_align_scaled_fwd: SingleRoIExtractor.forward's
    ``map_roi_levels`` before ``roi_rescale``).  ``out``: the [N, C, P, P] tensor to write (default: a new one)."""
    feats = [_chk(f, 'feat') for f in feats]
    _chk(rois, 'rois')
    B, C = feats[0].shape[:2]
    N = rois.shape[0]
    if roi_scale_factor is not None:
        if isinstance(roi_scale_factor, bool) or not isinstance(roi_scale_factor, (int, float)):
            raise TypeError(f'roi_scale_factor: a number expected, got {type(roi_scale_factor).__name__}')
        if not 0.0 < float(roi_scale_factor) < float('inf'):
            raise ValueError(f'roi_scale_factor must be a finite number > 0, got {roi_scale_factor}')
    out_size = output_size
    if bin_step is not None:
        if isinstance(bin_step, bool) or not isinstance(bin_step, int):
            raise TypeError(f'bin_step: an int expected, got {type(bin_step).__name__}')
        if bin_step < 1:
            raise ValueError(f'bin_step must be >= 1, got {bin_step}')
        if roi_scale_factor is not None:
            raise NotImplementedError('roi_align: bin_step together with roi_scale_factor is not built')
        out_size = -(-output_size // bin_step)
    if out is None:
        out = torch.empty((N, C, out_size, out_size), device=rois.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (N, C, out_size, out_size)
    levels = torch.zeros((N,), device=rois.device, dtype=torch.int32) if return_levels else None
    if bin_step is not None:
        name, tail = 'dm_roi_align_strided_fwd', (int(bin_step), _p(out), _p(levels))
    elif roi_scale_factor is not None:
        name, tail = 'dm_roi_align_scaled_fwd', (float(roi_scale_factor), _p(out), _p(levels))
    else:
        # where the library says ordering pays, a workspace: the RoIs are first ordered by level and position (one extra
        # launch: neighbouring workgroups then share their footprints in the L2; same results)
        wsb = int(lib().dm_roi_align_workspace_bytes(N, output_size)) if ROI_WORKSPACE else 0
        ws = torch.empty(((wsb + 15) // 16 * 4,), device=rois.device, dtype=torch.int32) if wsb > 0 else None
        name, tail = 'dm_roi_align_fwd_ws', (_p(out), _p(levels), _p(ws), wsb)
    rc = getattr(lib(), name)(_ptr_array(feats), _int_array([f.shape[2] for f in feats]), _int_array([f.shape[3] for f in feats]),
                              _float_array(spatial_scales), len(feats), B, C, _p(rois), N, output_size, sampling_ratio,
                              finest_scale, *tail, _stream())
    check(rc, name)
    return (out, levels) if return_levels else out


def roi_align_strided_supported(map_sizes, C, output_size, bin_step):
    """dm_roi_align_strided_supported: does ``roi_align(..., bin_step=bin_step)`` take these maps?  Host only."""
    return bool(lib().dm_roi_align_strided_supported(len(map_sizes), _int_array([s[0] for s in map_sizes]),
                                                     _int_array([s[1] for s in map_sizes]), int(C), int(output_size), int(bin_step)))


ROI_PLAN_FIELDS = ('kernel', 'P0', 'P1', 'grid', 'threads', 'lds_bytes', 'CT', 'order', 'lds_floats', 'levels')
ROI_KERNELS = ('order', 'tile', 'band', 'generic', 'bwd_gather')          # field 'kernel' of a plan record
ROI_ENTRIES = ('forward', 'add', 'backward')                              # dm_roi_align_plan's `entry`
ROI_ENTRY_STRIDED = 'strided'                                             # ... and entry 3: roi_align(..., bin_step=), the step in `pool`


def roi_align_plan_raw(entry, map_sizes, B, C, N, output_size, sampling_ratio=0, workspace_bytes=0, workspace=0, pool=0):
    """dm_roi_align_plan: (return code, records).  The code is the number of launches or the (negative) error the call with
    these numbers would return.  ``entry``: one of ROI_ENTRIES; ``map_sizes``: the (H, W) of every level; ``workspace``: 0
    none, 1 a 16-byte aligned pointer, 2 a misaligned one.  Host only: no tensor, no device."""
    consts = _abi.load()[1]
    n, cap = consts['DM_ROI_PLAN_INTS'], consts['DM_ROI_PLAN_MAX_LAUNCHES']
    assert len(ROI_PLAN_FIELDS) == n
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    rc = lib().dm_roi_align_plan(len(ROI_ENTRIES) if entry == ROI_ENTRY_STRIDED else ROI_ENTRIES.index(entry), int(pool), len(map_sizes), _int_array([s[0] for s in map_sizes]),
                                 _int_array([s[1] for s in map_sizes]), int(B), int(C), int(N), int(output_size),
                                 int(sampling_ratio), int(workspace_bytes), int(workspace), rec, cap)
    return rc, [dict(zip(ROI_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def roi_align_plan(entry, map_sizes, B, C, N, output_size, sampling_ratio=0, workspace=None, pool=0, bin_step=None):
    """(``entry='strided'`` with ``bin_step``: what ``roi_align(..., bin_step=bin_step)`` would launch.)  The launches ``roi_align`` ('forward'), ``roi_align_add_`` ('add', with its ``pool``) or ``roi_align_backward``
    ('backward') would make for these numbers, as the launcher's own route says (include/dynamask_hip.h, dm_roi_align_plan):
    a list of up to two dicts with the keys ROI_PLAN_FIELDS (two: the order kernel in front of the tile kernel, or the two
    sampling-grid classes of the generic kernel).  Raises where the call would fail.  ``workspace`` (forward): None = what
    ``roi_align`` itself passes (the bytes the library asks for, unless ROI_WORKSPACE is cleared), else a byte count."""
    if entry == ROI_ENTRY_STRIDED:
        pool = 0 if bin_step is None else bin_step
    if workspace is None:
        workspace = int(lib().dm_roi_align_workspace_bytes(N, output_size)) if ROI_WORKSPACE and entry == 'forward' else 0
    rc, recs = roi_align_plan_raw(entry, map_sizes, B, C, N, output_size, sampling_ratio, workspace, 1 if workspace > 0 else 0, pool)
    if rc < 0:
        check(rc, 'dm_roi_align_plan')
    return recs


def roi_align_backward(grad_out, feat_shapes, rois, output_size, spatial_scales, sampling_ratio=0, finest_scale=56.0):
    _chk(grad_out, 'grad_out')
    _chk(rois, 'rois')
    grads = [torch.zeros(s, device=grad_out.device, dtype=torch.float32) for s in feat_shapes]
    B, C = feat_shapes[0][:2]
    N = rois.shape[0]
    rc = lib().dm_roi_align_bwd(_p(grad_out), _ptr_array(grads), _int_array([s[2] for s in feat_shapes]),
                                _int_array([s[3] for s in feat_shapes]), _float_array(spatial_scales),
                                len(feat_shapes), B, C, _p(rois), N, output_size, sampling_ratio, finest_scale,
                                _stream())
    check(rc, 'dm_roi_align_bwd')
    return grads


# --------------------------------------------------------------- RLE (after the path, 8f rank 2)
MAX_MASKS_PER_LAUNCH = 65535      # dm_paste_masks, dm_rle_encode_canvas, dm_paste_rle: the masks are the grid's y dimension


def _chk_mask_count(N, name):
    if N > MAX_MASKS_PER_LAUNCH:
        raise ValueError(f'{name}: {N} masks in one call, at most {MAX_MASKS_PER_LAUNCH} (split the batch)')


def _rle_collect(N, img_h, img_w, runs, start, positions, launch, capacity, sizes=None):
    """Shared tail of the encoders: read the run totals, re-run once with a larger
    buffer if the boundaries did not fit, copy exactly the used part of `positions`, build
    the COCO dicts ({'size': [h, w], 'counts': bytes}, what pycocotools' encode returns).
    ``sizes``: per-mask (h, w) canvases (paste_rle_multi) instead of one img_h x img_w."""
    import ctypes as C
    start_h = start.cpu()                        # synchronises the stream
    total = int(start_h[N])
    if total > capacity:
        positions = torch.empty((total,), device=runs.device, dtype=torch.int32)
        launch(positions, total)
        start_h = start.cpu()
    pos_h = torch.empty((max(total, 1),), dtype=torch.int32, pin_memory=True)
    if total > 0:
        pos_h[:total].copy_(positions[:total], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    base = pos_h.data_ptr()
    L = lib()
    out = []
    cap = 64
    buf = C.create_string_buffer(cap)
    for n in range(N):
        s0, s1 = int(start_h[n]), int(start_h[n + 1])
        if not 0 <= s0 <= s1 <= total:           # dm_rle_string would read past the host copy of the boundaries
            raise RuntimeError(f'RLE encoder: mask {n} has its boundaries at [{s0}, {s1}) of {total} counted in all')
        need = (s1 - s0 + 1) * 7             # <= 7 characters per count (31-bit values)
        if need > cap:
            cap = need
            buf = C.create_string_buffer(cap)
        h, w = (img_h, img_w) if sizes is None else sizes[n]
        ln = L.dm_rle_string(C.c_void_p(base + 4 * s0), s1 - s0, h * w, buf, cap)
        if ln < 0:
            raise RuntimeError('dm_rle_string: buffer too small')
        out.append({'size': [int(h), int(w)], 'counts': buf.raw[:ln]})
    return out


def rle_encode(canvas):
    """uint8/bool [N, h, w] device bitmaps -> list of COCO RLE dicts (device encoder)."""
    if canvas.dtype == torch.bool:
        canvas = canvas.view(torch.uint8)
    _chk(canvas, 'canvas', torch.uint8)
    N, h, w = canvas.shape
    if N == 0:
        return []
    _chk_mask_count(N, 'rle_encode')
    dev = canvas.device
    scratch = torch.empty((lib().dm_rle_scratch_ints(N, h, w),), device=dev, dtype=torch.int32)
    runs = torch.empty((N,), device=dev, dtype=torch.int32)
    start = torch.empty((N + 1,), device=dev, dtype=torch.int32)
    capacity = max(4096, N * 4 * (h + w))

    def launch(positions, cap):
        check(lib().dm_rle_encode_canvas(_p(canvas), N, h, w, _p(scratch), _p(runs), _p(start), _p(positions), cap,
                                         _stream()), 'dm_rle_encode_canvas')
    positions = torch.empty((capacity,), device=dev, dtype=torch.int32)
    launch(positions, capacity)
    return _rle_collect(N, h, w, runs, start, positions, launch, capacity)


def paste_rle(masks, boxes, img_h, img_w, threshold=0.5, apply_sigmoid=False):
    """Paste + threshold + RLE in one go: the [N, img_h, img_w] canvas is never written and only
    the run boundaries cross PCIe.  Same pixel arithmetic as ``paste_masks``."""
    _chk(masks, 'masks')
    _chk(boxes, 'boxes')
    N = masks.shape[0]
    if N == 0:
        return []
    _chk_mask_count(N, 'paste_rle')
    mh, mw = masks.shape[-2:]
    dev = masks.device
    img_h, img_w = int(img_h), int(img_w)
    scratch = torch.empty((lib().dm_rle_scratch_ints(N, img_h, img_w),), device=dev, dtype=torch.int32)
    runs = torch.empty((N,), device=dev, dtype=torch.int32)
    start = torch.empty((N + 1,), device=dev, dtype=torch.int32)
    capacity = max(4096, N * 4 * (img_h + img_w))

    def launch(positions, cap):
        check(lib().dm_paste_rle(_p(masks), _p(boxes), N, mh, mw, img_h, img_w, float(threshold),
                                 1 if apply_sigmoid else 0, _p(scratch), _p(runs), _p(start), _p(positions), cap,
                                 _stream()), 'dm_paste_rle')
    positions = torch.empty((capacity,), device=dev, dtype=torch.int32)
    launch(positions, capacity)
    return _rle_collect(N, img_h, img_w, runs, start, positions, launch, capacity)


def _upload(vals, dtype, device):
    """A small host table -> device without a host wait: pinned staging buffer, copy ordered on the current stream."""
    return torch.tensor(vals, dtype=dtype).pin_memory().to(device, non_blocking=True)


def _multi_canvas_table(det_counts, sizes, device):
    """Detections of B images, image after image -> (det_img int32 [N], img_tab int64 [B, 4] of (h, w, first detection,
    byte offset of the first canvas) on the device, total canvas bytes, the largest canvas of an image with detections,
    per-detection (h, w))."""
    assert len(det_counts) == len(sizes)
    rows, det_img, det_sizes = [], [], []
    first = off = max_pixels = 0
    for b, (n, (h, w)) in enumerate(zip(det_counts, sizes)):
        h, w, n = int(h), int(w), int(n)
        if n > 0 and (h <= 0 or w <= 0):
            raise ValueError(f'image {b}: canvas {h} x {w} holds no pixel')
        rows.append([h, w, first, off])
        det_img += [b] * n
        det_sizes += [(h, w)] * n
        first += n
        off += n * h * w
        if n > 0:
            max_pixels = max(max_pixels, h * w)
    return (_upload(det_img, torch.int32, device), _upload(rows, torch.int64, device), off, max_pixels, det_sizes)


def paste_masks_multi(masks, boxes, det_counts, sizes, threshold=0.5, apply_sigmoid=False):
    """``paste_masks`` for the detections of several images in one launch.  masks [N, 1, h, w] or [N, h, w], boxes
    [N, 4] in canvas pixels, image after image (``det_counts[b]`` detections of image b, canvas ``sizes[b]`` = (h, w)).
    Returns (packed uint8 buffer of all bitmaps, per-detection byte offsets, per-detection (h, w)): detection n is
    ``buf[off[n]:off[n] + h * w].view(h, w)``, the bits ``paste_masks`` gives it on its own image."""
    _chk(masks, 'masks')
    _chk(boxes, 'boxes')
    N = masks.shape[0]
    assert N == sum(int(n) for n in det_counts) and boxes.shape[0] == N
    dev = masks.device
    det_img, tab, total, max_pixels, det_sizes = _multi_canvas_table(det_counts, sizes, dev)
    out = torch.empty((max(total, 1),), device=dev, dtype=torch.uint8)
    offs, o = [], 0
    for h, w in det_sizes:
        offs.append(o)
        o += h * w
    if N > 0:
        mh, mw = masks.shape[-2:]
        check(lib().dm_paste_masks_multi(_p(masks), _p(boxes), N, mh, mw, _p(det_img), len(det_counts), _p(tab),
                                         max_pixels, float(threshold), 1 if apply_sigmoid else 0, _p(out), _stream()),
              'dm_paste_masks_multi')
    return out[:total], offs, det_sizes


def paste_rle_multi(masks, boxes, det_counts, sizes, threshold=0.5, apply_sigmoid=False, capacity=None):
    """``paste_rle`` for the detections of several images in one launch (arguments as ``paste_masks_multi``): one
    list of COCO RLE dicts, detection after detection, each with its own image's size.  One run-boundary buffer for all
    detections, one device -> host copy; ``capacity`` (boundaries; default 4 (h + w) per detection) is the first
    buffer's size, re-run once with the exact size if it was short (``_rle_collect``)."""
    _chk(masks, 'masks')
    _chk(boxes, 'boxes')
    N = masks.shape[0]
    assert N == sum(int(n) for n in det_counts) and boxes.shape[0] == N
    if N == 0:
        return []
    mh, mw = masks.shape[-2:]
    dev = masks.device
    det_img, tab, _, max_pixels, det_sizes = _multi_canvas_table(det_counts, sizes, dev)
    ns = lib().dm_rle_multi_scratch_ints(N, max_pixels)
    if ns < 0:
        raise ValueError(f'canvas of {max_pixels} pixels is too large for the RLE encoder')
    scratch = torch.empty((ns,), device=dev, dtype=torch.int32)
    runs = torch.empty((N,), device=dev, dtype=torch.int32)
    start = torch.empty((N + 1,), device=dev, dtype=torch.int32)
    if capacity is None:
        capacity = max(4096, sum(4 * (h + w) for h, w in det_sizes))
    B = len(det_counts)

    def launch(positions, cap):
        check(lib().dm_paste_rle_multi(_p(masks), _p(boxes), N, mh, mw, _p(det_img), B, _p(tab), max_pixels,
                                       float(threshold), 1 if apply_sigmoid else 0, _p(scratch), _p(runs), _p(start),
                                       _p(positions), cap, _stream()), 'dm_paste_rle_multi')
    positions = torch.empty((max(capacity, 1),), device=dev, dtype=torch.int32)
    launch(positions, capacity)
    return _rle_collect(N, 0, 0, runs, start, positions, launch, capacity, sizes=det_sizes)


# --------------------------------------------------------------- bbox branch (8f rank 4)
def fc(x, weight, bias=None, relu=False):
    """nn.Linear forward: x [N, K], weight [M, K], bias [M] -> [N, M] (fp32 MFMA, deterministic split-K)."""
    _chk(x, 'x')
    _chk(weight, 'weight')
    if bias is not None:
        _chk(bias, 'bias')
    N, K = x.shape
    M = weight.shape[0]
    assert weight.shape[1] == K
    out = torch.empty((N, M), device=x.device, dtype=torch.float32)
    ns = int(lib().dm_fc_scratch_floats(N, K, M))
    scratch = torch.empty((ns,), device=x.device, dtype=torch.float32) if ns > 0 else None
    check(lib().dm_fc_fwd(_p(x), _p(weight), _p(bias), N, K, M, 1 if relu else 0, _p(out), _p(scratch), _stream()),
          'dm_fc_fwd')
    return out


def bbox_decode(rois, cls_score, bbox_pred, num_classes, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.),
                wh_ratio_clip=16 / 1000, max_shape=None, scale=(1.0, 1.0), class_agnostic=False):
    """softmax(cls_score), delta2bbox(rois, bbox_pred) clipped to ``max_shape`` (h, w) and
    divided by ``scale`` (sx, sy).  rois [N, 5] (batch column first) or [N, 4]."""
    _chk(rois, 'rois')
    N = rois.shape[0]
    dev = rois.device
    nb = 1 if class_agnostic else num_classes
    scores = None
    if cls_score is not None:
        _chk(cls_score, 'cls_score')
        assert cls_score.shape == (N, num_classes + 1)
        scores = torch.empty_like(cls_score)
    if bbox_pred is not None:
        _chk(bbox_pred, 'bbox_pred')
        assert bbox_pred.shape == (N, 4 * nb)
    bboxes = torch.empty((N, 4 * nb), device=dev, dtype=torch.float32)
    ch, cw = (float(max_shape[0]), float(max_shape[1])) if max_shape is not None else (0.0, 0.0)
    check(lib().dm_bbox_decode(_p(rois), rois.shape[1], rois.shape[1] - 4, _p(cls_score), _p(bbox_pred), N, num_classes,
                               1 if class_agnostic else 0, _float_array(means), _float_array(stds), float(wh_ratio_clip),
                               ch, cw, float(scale[0]), float(scale[1]), _p(scores), _p(bboxes), _stream()),
          'dm_bbox_decode')
    return bboxes, scores


def nms(boxes, scores, iou_threshold, offset=0, max_num=-1):
    """mmcv.ops.nms: (dets [k, 5] in descending score order, keep indices [k] into the input).
    Suppression matrix on the device, greedy pass on the host.  ``max_num`` <= 0: no limit, as in ``nms_segmented``
    and ``multiclass_nms``."""
    import ctypes as C
    _chk(boxes, 'boxes')
    _chk(scores, 'scores')
    M = boxes.shape[0]
    if M == 0:
        return boxes.new_zeros((0, 5)), torch.zeros((0,), dtype=torch.long, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]
    sb = boxes[order].contiguous()
    words = (M + 63) // 64
    mask = torch.empty((M, words), device=boxes.device, dtype=torch.int64)
    check(lib().dm_nms_mask(_p(sb), M, float(iou_threshold), int(offset), _p(mask), _stream()), 'dm_nms_mask')
    mask_h = mask.cpu()                                   # synchronises
    keep_h = torch.empty((M,), dtype=torch.int32)
    n = lib().dm_nms_reduce(C.c_void_p(mask_h.data_ptr()), M, C.c_void_p(keep_h.data_ptr()),
                            int(max_num) if max_num > 0 else -1)
    keep_sorted = keep_h[:n].to(device=boxes.device, dtype=torch.long)
    keep = order[keep_sorted]
    dets = torch.cat([boxes[keep], scores[keep][:, None]], 1)
    return dets, keep


NMS_REDUCE_MAX_WORDS = 20480      # dm_nms_reduce_segmented keeps a segment's removed bits in LDS (160 KB)


def nms_segmented(boxes_sorted, counts, iou_threshold, offset=0, max_num=-1):
    """``nms`` over B segments at once, without a host wait.  boxes_sorted [sum M_b, 4]: the segments one after the
    other, each already score-sorted on its own; ``counts`` = host list of M_b.  The suppression bits are computed
    within a segment only (block-diagonal, one [M_b, ceil(M_b / 64)] matrix each) and the greedy pass runs on the
    device, one wave per segment, stopping at ``max_num`` kept boxes (> 0) per segment.  Returns (keep int32 [sum M_b]:
    segment b's kept rows, ascending in its sorted order, at keep[start_b : start_b + kept_b]; kept int32 [B]), both
    on the device."""
    _chk(boxes_sorted, 'boxes')
    counts = [int(m) for m in counts]
    B = len(counts)
    dev = boxes_sorted.device
    assert boxes_sorted.shape == (sum(counts), 4)
    keep = torch.empty((max(sum(counts), 1),), device=dev, dtype=torch.int32)
    kept = torch.zeros((B,), device=dev, dtype=torch.int32)
    if B == 0:
        return keep[:0], kept
    rows, start, off = [], 0, 0
    for m in counts:
        rows.append([start, m, off])
        start += m
        off += m * ((m + 63) // 64)
    max_words = max((m + 63) // 64 for m in counts)
    if max_words > NMS_REDUCE_MAX_WORDS:
        raise ValueError(f'{max(counts)} boxes in one segment: the device NMS pass holds at most '
                         f'{64 * NMS_REDUCE_MAX_WORDS}')
    tab = _upload(rows, torch.int64, dev)
    mask = torch.empty((max(off, 1),), device=dev, dtype=torch.int64)
    check(lib().dm_nms_mask_segmented(_p(boxes_sorted), B, _p(tab), max_words, float(iou_threshold), int(offset),
                                      _p(mask), off, _stream()), 'dm_nms_mask_segmented')
    check(lib().dm_nms_reduce_segmented(_p(mask), B, _p(tab), max_words, int(max_num) if max_num > 0 else -1, _p(keep),
                                        _p(kept), _stream()), 'dm_nms_reduce_segmented')
    return keep[:sum(counts)], kept


# --------------------------------------------------------------- test-time augmentation (several views of one image)
AUG_VIEW_FLOATS = _abi.load()[1]['DM_AUG_VIEW_FLOATS']           # (prototypes, constants) of dynamask_hip.h
AUG_FLIP_CODES = {'horizontal': 1, 'vertical': 2}


def aug_view_rows(img_metas):
    """The per-view parameters of the TTA kernels from V view metas (dicts with ``img_shape``, ``scale_factor``,
    ``flip`` and, when flipped, ``flip_direction``) -> host rows [V][AUG_VIEW_FLOATS] (sf x1, y1, x2, y2, img_h, img_w,
    flip code, 0).  The scale factor is taken as the reference's ``bboxes.new_tensor(scale_factor)`` takes it: fp32, a
    scalar for all four coordinates or one value each.  Raises ValueError for a flip direction other than 'horizontal' /
    'vertical' (merge_augs.py merge_aug_masks) -- before anything reaches the device."""
    import numpy as np
    rows = []
    for v, m in enumerate(img_metas):
        sf = np.asarray(m['scale_factor'], dtype=np.float32).reshape(-1)
        if sf.size == 1:
            sf = np.repeat(sf, 4)
        if sf.size != 4:
            raise ValueError(f'view {v}: scale_factor has {sf.size} values (one, or [w, h, w, h])')
        flip = 0
        if m['flip']:
            d = m.get('flip_direction', 'horizontal')
            if d not in AUG_FLIP_CODES:
                raise ValueError(f"view {v}: invalid flipping direction '{d}'")
            flip = AUG_FLIP_CODES[d]
        h, w = m['img_shape'][:2]
        rows.append([float(x) for x in sf] + [float(h), float(w), float(flip), 0.0])
    return rows


def aug_view_table(img_metas, device):
    """``aug_view_rows`` uploaded without a host wait: float32 [V, AUG_VIEW_FLOATS] on ``device``."""
    return _upload(aug_view_rows(img_metas), torch.float32, device)


def bbox_mapping_multi(boxes, view_tab):
    """mmdet ``bbox_mapping`` of boxes [n, >= 4] (original image) into every view of ``view_tab`` in one launch ->
    RoI rows [V, n, 5] (batch column 0): ``b * sf``, then the view's flip."""
    _chk(view_tab, 'view_tab')
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] < 4:
        raise ValueError('boxes: [n, >= 4] expected')
    if boxes.stride(1) != 1 or boxes.stride(0) < 4:
        boxes = boxes.contiguous()
    if not boxes.is_cuda or boxes.dtype != torch.float32:
        _chk(boxes, 'boxes')                    # (raises: no CPU fallback / wrong dtype)
    V, n = view_tab.shape[0], boxes.shape[0]
    out = torch.empty((V, n, 5), device=boxes.device, dtype=torch.float32)
    if n > 0 and V > 0:
        check(lib().dm_bbox_mapping_multi(_p(boxes), boxes.stride(0), n, V, _p(view_tab), _p(out), _stream()),
              'dm_bbox_mapping_multi')
    return out


def merge_aug_bboxes(bboxes_list, scores_list, view_tab):
    """mmdet ``merge_aug_bboxes`` in one launch: V views' boxes [n, 4C] (view coordinates) and scores [n, C + 1] ->
    (boxes mapped back to the original image and averaged [n, 4C], averaged scores [n, C + 1])."""
    _chk(view_tab, 'view_tab')
    V = view_tab.shape[0]
    if len(bboxes_list) != V or len(scores_list) != V or V == 0:
        raise ValueError(f'{len(bboxes_list)} box and {len(scores_list)} score tensors for {V} views')
    n, c4 = bboxes_list[0].shape
    cs = scores_list[0].shape[1]
    for b, sc in zip(bboxes_list, scores_list):
        _chk(b, 'bboxes')
        _chk(sc, 'scores')
        if tuple(b.shape) != (n, c4) or tuple(sc.shape) != (n, cs):
            raise ValueError('every view needs boxes and scores of the same shape')
    dev = bboxes_list[0].device
    out_b = torch.empty((n, c4), device=dev, dtype=torch.float32)
    out_s = torch.empty((n, cs), device=dev, dtype=torch.float32)
    if n > 0:
        tab = _upload([[b.data_ptr(), sc.data_ptr()] for b, sc in zip(bboxes_list, scores_list)], torch.int64, dev)
        if hazard.ENABLED[0]:
            hazard.touch('dm_merge_aug_bboxes (view tables)', reads=list(bboxes_list) + list(scores_list))
        check(lib().dm_merge_aug_bboxes(_p(tab), _p(view_tab), V, n, c4, cs, _p(out_b), _p(out_s), _stream()),
              'dm_merge_aug_bboxes')
    return out_b, out_s


def proposals_mapping_back(proposals, img_metas):
    """The first half of mmdet ``merge_aug_proposals`` for all segments in one launch (dm_proposals_mapping_back):
    ``proposals[s]`` [n_s, 5] (view coordinates, score last) with its view's meta ``img_metas[s]`` -> [sum n_s, 5], the
    segments one after the other, boxes mapped back to the original image (flip, then a true division by the scale
    factor), scores copied.  No host wait."""
    S = len(proposals)
    if len(img_metas) != S:
        raise ValueError(f'{S} proposal tensors for {len(img_metas)} metas')
    rows_tab, r0 = [], 0
    for p in proposals:
        _chk(p, 'proposals')
        if p.dim() != 2 or p.shape[1] != 5:
            raise ValueError(f'proposals: [n, 5] expected, got {list(p.shape)}')
        rows_tab.append([p.data_ptr(), p.shape[0], r0])
        r0 += p.shape[0]
    dev = proposals[0].device if S else torch.device('cuda')
    out = torch.empty((r0, 5), device=dev, dtype=torch.float32)
    if r0 > 0:
        view_tab = aug_view_table(img_metas, dev)
        tab = _upload(rows_tab, torch.int64, dev)
        if hazard.ENABLED[0]:
            hazard.touch('dm_proposals_mapping_back (segment table)', reads=list(proposals))
        check(lib().dm_proposals_mapping_back(_p(tab), _p(view_tab), S, max(r[1] for r in rows_tab), _p(out), _stream()),
              'dm_proposals_mapping_back')
    return out


def merge_aug_masks(logits_list, labels, view_tab):
    """mmdet ``merge_aug_masks`` of V views' mask LOGITS [n, K, S, S] in one launch -> probabilities [n, 1, S, S]: the
    ``labels`` [n] channel when K > 1 (the channel the paste would select), sigmoid (the paste's own), un-flipped,
    averaged over the views."""
    _chk(view_tab, 'view_tab')
    V = view_tab.shape[0]
    if len(logits_list) != V or V == 0:
        raise ValueError(f'{len(logits_list)} logit tensors for {V} views')
    n, K, S, S2 = logits_list[0].shape
    if S != S2:
        raise ValueError('square mask logits expected')
    for t in logits_list:
        _chk(t, 'logits')
        if tuple(t.shape) != (n, K, S, S):
            raise ValueError('every view needs logits of the same shape')
    dev = logits_list[0].device
    out = torch.empty((n, 1, S, S), device=dev, dtype=torch.float32)
    if n == 0:
        return out
    if K > 1:
        _chk(labels, 'labels', torch.int64)
        if labels.shape != (n,):
            raise ValueError(f'labels: [{n}] expected')
    tab = _upload([t.data_ptr() for t in logits_list], torch.int64, dev)
    if hazard.ENABLED[0]:
        hazard.touch('dm_merge_aug_masks (view table)', reads=list(logits_list))
    check(lib().dm_merge_aug_masks(_p(tab), _p(view_tab), V, n, K, S, _p(labels) if K > 1 else _p(None), _p(out),
                                   _stream()), 'dm_merge_aug_masks')
    return out


# --------------------------------------------------------------- convolutions
def packed_cout(cout):
    return lib().dm_conv_packed_cout(int(cout))


def packed_floats(cout, ksize, src_channels, precision='fp32'):
    fn = lib().dm_conv_packed_floats_bf16x3 if precision == 'bf16x3' else lib().dm_conv_packed_floats
    n = fn(int(cout), int(ksize), len(src_channels), _int_array(src_channels))
    if n < 0:
        raise ValueError('bad conv packing request')
    return int(n)


def pack_conv_weight(w, transpose_flip=False, src_channels=None, precision='fp32'):
    """OIHW -> [k*k][KQ][CoutP][4] (see include/dynamask_hip.h).  ``src_channels``:
    how the input channels split over the concat sources (default: one source).
    ``precision='bf16x3'``: the split layout of dm_conv_pack_weight_bf16x3, marked as such (``conv_layout``); conv2d
    and conv1x1_group then run the bf16x3 kernel on it."""
    _chk(w, 'weight')
    precision = _precision.checked(precision)
    cout, cin, kh, kw = w.shape
    assert kh == kw and kh in (1, 3)
    rows = cout if transpose_flip else cin
    cols = cin if transpose_flip else cout
    if src_channels is None:
        src_channels = [rows]
    assert sum(src_channels) == rows
    wp = torch.empty((packed_floats(cols, kh, src_channels, precision),), device=w.device, dtype=torch.float32)
    fn, name = ((lib().dm_conv_pack_weight_bf16x3, 'dm_conv_pack_weight_bf16x3') if precision == 'bf16x3'
                else (lib().dm_conv_pack_weight, 'dm_conv_pack_weight'))
    check(fn(_p(w), cout, cin, kh, 1 if transpose_flip else 0, len(src_channels), _int_array(src_channels), _p(wp),
             _stream()), name)
    if precision == 'bf16x3':
        wp._dm_bf16x3 = True
    return wp


def conv_layout(w_packed):
    """'bf16x3' for a weight packed by ``pack_conv_weight(precision='bf16x3')``, else 'fp32'."""
    return 'bf16x3' if getattr(w_packed, '_dm_bf16x3', False) else 'fp32'


# Per-shape routing of the bf16x3 mode (dynamask_amd/precision.py): the shapes whose bf16x3 launch measured faster than
# the exact one (profiles/r07_precision.txt, tools/precision_probe.py; DESIGN.md "Opt-in bf16x3 convolutions").  A rule
# is (ksize, min cout, max cout, max H * W); a shape that no rule covers runs the exact kernel in either mode.
#   3x3 on 14 x 14 maps: 256 couts 0.64-0.69 of the exact time at 16 / 100 / 512 RoIs, the 36-cout DCN offset
#     convolution 0.88 (its tail couts run in the 64-cout tile).  Maps of 28 x 28 and wider have no bf16x3 build (LDS).
#   1x1 on 14 x 14 maps with >= 96 couts: 0.83-0.92; FCNMaskHead's 80-cout conv_logits at 28 x 28: 0.96.  On
#     28 x 28 / 56 x 56 maps the other 1x1s are not faster (1.01-1.35: the fuse / transform convolutions of 128 and 64
#     couts, 64 -> 30; the 64-cout fuse at 56 x 56 measured 0.99-1.04 over three collections, no gain): exact.
BF16X3_ROUTES = (
    (3, 36, 1 << 30, 16 * 16),
    (1, 96, 1 << 30, 16 * 16),
    (1, 80, 80, 28 * 28),
)
# the grouped FPN-wide semantic 1x1 convolutions (conv1x1_group, one launch for all three SFM stages)
BF16X3_SEMANTIC_GROUP = [True]
# FCNMaskHead's deconv 2x2/s2 (dm_deconv2x2_fwd) on maps up to this many pixels (0: never).  Measured 256 -> 256 @14 x 512
# RoIs: 0.68-0.70 ms bf16x3 against 0.65 exact (1.04-1.06: its 4 * 256 packed columns already fill the exact 128 x 128 tile; the
# bf16x3 build's 64-cout tile needs twice the workgroups): exact.
BF16X3_DECONV_MAX_HW = [0]


def _bf16x3_3x3_built(H, W):
    """dm_conv2d_fwd's bf16x3 3x3 build stages one plane position per thread: the plane of a 128-pixel tile (launch_conv in
    csrc/conv_igemm.hip) must hold <= 256 positions.  Maps up to 6 x 6 and wide, flat ones (8 x 32, 1 x W) fail that."""
    hw = H * W
    nseg = -(-127 // hw) + 1
    rmax = -(-127 // W) + 1 + 2 * nseg
    return rmax * (W + 2) <= 256


def bf16x3_routed(cout, ksize, H, W):
    """Does the routing table send this shape to the bf16x3 kernel (and is there a build for it)?"""
    if ksize == 3 and not _bf16x3_3x3_built(H, W):
        return False
    return any(ksize == k and lo <= cout <= hi and H * W <= hw for k, lo, hi, hw in BF16X3_ROUTES)


def deconv_precision_for(H, W):
    """The kernel FCNMaskHead's deconv of an H x W map runs now (BF16X3_DECONV_MAX_HW)."""
    return 'bf16x3' if inference_precision() == 'bf16x3' and H * W <= BF16X3_DECONV_MAX_HW[0] else 'fp32'


_EXACT_DEPTH = [0]


def exact_convs(fn):
    """Decorator: the convolutions issued inside ``fn`` run exact fp32 whatever the precision mode -- the forward and
    backward of the training path's autograd Functions, whose bodies run with grad disabled."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        _EXACT_DEPTH[0] += 1
        try:
            return fn(*args, **kw)
        finally:
            _EXACT_DEPTH[0] -= 1
    return wrapped


def inference_precision():
    """The precision an inference convolution runs at now: the mode, or 'fp32' while grad is enabled or inside the
    training path (``exact_convs``)."""
    p = _precision.get_conv_precision()
    if p != 'fp32' and (torch.is_grad_enabled() or _EXACT_DEPTH[0] > 0):
        return 'fp32'
    return p


def conv_precision_for(cout, ksize, H, W):
    """'bf16x3' when the mode is on, grad is disabled and the routing table takes this shape; else 'fp32'."""
    if inference_precision() == 'bf16x3' and bf16x3_routed(cout, ksize, H, W):
        return 'bf16x3'
    return 'fp32'


class _DevicePlan:
    """The packs of ONE device: entries, the device-resident job table, and the event of the last refresh."""

    def __init__(self, device):
        self.device = device
        self.entries = []          # dicts: param (weakref), out, job fields, ver, used
        self.table = None
        self.table_ids = None
        self.old_tables = []       # previous job tables stay alive for two more refreshes: a batch launch on another
                                   # stream may still be reading one when the next is uploaded
        self.event = None          # recorded behind the last refresh; streams that read packs wait for it (get)
        self.generation = 0
        self.waited = {}           # stream id -> generation it has waited for


class PackPlan:
    """Kernel-layout weights of a training step, refreshed by ONE launch (dm_conv_pack_weight_batch) per device.

    Every optimizer step changes ~45 weight tensors, each of which the kernels read in a packed layout; packing them
    one launch at a time cost the host 1.3 ms of the 3.7 ms it needs to issue a forward pass, and the forward is the
    part of the step where the GPU waits for the host.  A pack registered here (``get``) owns a persistent output
    buffer; the first request that finds its pack stale refreshes, in one launch, every registered pack of that device
    that was used since the previous refresh (a pack nobody asked for in a whole step is left alone and refreshed on
    demand).  The job table lives on the device and is rebuilt only when the set of jobs changes.

    Streams: a refresh runs on the stream that asked for it and records an event; ``get`` makes any OTHER stream wait
    for that event before it hands out a buffer (once per stream and refresh), so a pack refreshed on the main stream
    and read by a side stream -- or the other way round -- is ordered whoever triggers the refresh."""

    def __init__(self):
        self.plans = {}            # device index -> _DevicePlan
        self.launches = 0
        self.uploads = 0

    @property
    def entries(self):
        return [e for p in self.plans.values() for e in p.entries]

    @staticmethod
    def _ver(param):
        return (param.data_ptr(), param._version, WEIGHT_EPOCH[0])

    def _plan(self, device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        p = self.plans.get(idx)
        if p is None:
            p = self.plans[idx] = _DevicePlan(torch.device('cuda', idx))
        return p

    def register(self, param, transpose_flip, src_channels, lo, hi):
        import weakref
        cout, cin_total, kh, kw = param.shape
        lo = 0 if lo is None else lo
        hi = cin_total if hi is None else hi
        cin = hi - lo
        rows = cout if transpose_flip else cin
        cols = cin if transpose_flip else cout
        src_channels = [rows] if src_channels is None else list(src_channels)
        assert sum(src_channels) == rows and kh == kw and kh in (1, 3) and len(src_channels) <= 4
        out = torch.empty((packed_floats(cols, kh, src_channels),), device=param.device, dtype=torch.float32)
        plan = self._plan(param.device)
        e = dict(param=weakref.ref(param), out=out, cout=cout, cin=cin, ks=kh, flip=1 if transpose_flip else 0,
                 srcs=src_channels, ld=cin_total, c0=lo, ver=None, used=True, plan=plan)
        plan.entries.append(e)
        return e

    def get(self, e):
        p = e['param']()
        if p is None:
            raise RuntimeError('PackPlan.get: the parameter of this pack no longer exists')
        plan = e['plan']
        e['used'] = True
        if e['ver'] != self._ver(p):
            self._refresh(plan)
            e['used'] = True          # (refresh clears the flag of what it packed; this one is in use now)
        if plan.event is not None:
            st = torch.cuda.current_stream(plan.device)
            if plan.waited.get(st.cuda_stream) != plan.generation:
                st.wait_event(plan.event)          # (a no-op for the stream that recorded it)
                plan.waited[st.cuda_stream] = plan.generation
        return e['out']

    def refresh(self, device=None):
        """Refresh the stale packs of ``device`` (default: the current device) on its current stream."""
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        plan = self.plans.get(idx)
        if plan is not None:
            self._refresh(plan)

    def _refresh(self, plan):
        live = []
        for e in plan.entries:
            p = e['param']()
            if p is not None:
                live.append((e, p))
        plan.entries = [e for e, _ in live]
        todo = [(e, p) for e, p in live if e['used'] and e['ver'] != self._ver(p)]
        if not todo:
            return
        with torch.cuda.device(plan.device):
            ids = tuple((id(e), p.data_ptr()) for e, p in todo)
            if ids != plan.table_ids and torch.cuda.is_current_stream_capturing():
                # (with the job table already on the device the refresh is one launch and is captured like any other:
                # a captured training step repacks its weights on every replay)
                raise RuntimeError('PackPlan: a kernel-layout weight is stale inside a HIP-graph capture and its job table '
                                   'is not on the device yet (the upload cannot be captured: run the path once eagerly first)')
            if ids != plan.table_ids:
                arr = (_lib.PackJob * len(todo))()      # (derived from the header at first use)
                for j, (e, p) in zip(arr, todo):
                    j.w, j.w_packed = p.data_ptr(), e['out'].data_ptr()
                    j.Cout, j.Cin, j.ksize, j.transpose_flip = e['cout'], e['cin'], e['ks'], e['flip']
                    j.num_srcs = len(e['srcs'])
                    for k, c in enumerate(e['srcs']):
                        j.src_channels[k] = c
                    j.ld, j.c0 = e['ld'], e['c0']
                host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
                if plan.table is not None:
                    plan.old_tables = (plan.old_tables + [plan.table])[-2:]
                plan.table = host.to(plan.device)
                plan.table_ids = ids
                self.uploads += 1
            if hazard.ENABLED[0]:       # the device-side job table hides what this launch reads and writes
                hazard.touch('dm_conv_pack_weight_batch', reads=[p for _, p in todo], writes=[e['out'] for e, _ in todo])
            check(lib().dm_conv_pack_weight_batch(_p(plan.table), len(todo), _stream()), 'dm_conv_pack_weight_batch')
            self.launches += 1
            plan.event = torch.cuda.current_stream(plan.device).record_event()
            plan.generation += 1
            plan.waited = {torch.cuda.current_stream(plan.device).cuda_stream: plan.generation}
        for e, p in todo:
            e['ver'] = self._ver(p)
            e['used'] = False
        # (a pack requested later in the same step sets ``used`` again and finds its version current)


PACK_PLAN = PackPlan()


_overlapped = 0


class overlapped_streams:
    """Context: launches inside run next to other work on a second stream (DynaMaskRoIHead splits
    the RoIs over two streams).  Passed to dm_conv2d_fwd as flag bit 3, a scheduling hint."""

    def __enter__(self):
        global _overlapped
        _overlapped += 1

    def __exit__(self, *exc):
        global _overlapped
        _overlapped -= 1


# DM_CONV_SPLITK=0: no split-K for small inference launches (the sums of one launch, in one order, whatever the RoI count)
CONV_SPLITK = [os.environ.get('DM_CONV_SPLITK', '1') == '1']
_SPLITK_DEPTH = [0]


class splitk_scope:
    """Inside this scope ``conv2d`` may split the K loop of a launch that would leave most of the chip idle
    (dm_conv2d_fwd_ws): entered by the inference entry points of the RoI head only -- a training forward keeps one
    association of its sums whatever the RoI count (its golden tests pin gradients behind ReLU kinks and pool ties)."""

    def __enter__(self):
        _SPLITK_DEPTH[0] += 1
        return self

    def __exit__(self, *exc):
        _SPLITK_DEPTH[0] -= 1
        return False


def conv2d(srcs, w_packed, bias, cout, ksize, relu=False, out=None, out_ch_offset=0, accumulate=False, mask=None):
    """Fused concat(srcs) -> conv(ksize, same) -> +bias -> ReLU.  ``mask`` (same shape as ``out``): outputs where it
    is <= 0 are stored as 0 -- the ReLU adjoint of a data gradient (threshold_backward: it passes at NaN), fused into the
    epilogue."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    srcs = [_chk_src(s) for s in srcs]
    _chk(w_packed, 'w_packed')
    if bias is not None:
        _chk(bias, 'bias')
    NB, _, H, W = srcs[0].shape
    for s in srcs:
        assert s.shape[0] == NB and s.shape[2] == H and s.shape[3] == W
    cin = sum(s.shape[1] for s in srcs)
    layout = conv_layout(w_packed)         # the bf16x3 layout runs the bf16x3 kernel (flag bit 4)
    assert w_packed.numel() == packed_floats(cout, ksize, [s.shape[1] for s in srcs], layout), 'weights packed for other sources'
    if out is None:
        out = torch.empty((NB, cout, H, W), device=srcs[0].device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert out.shape[0] == NB and out.shape[2] == H and out.shape[3] == W
    strides = (ctypes.c_longlong * len(srcs))(*[int(s.stride(0)) for s in srcs])
    flags = (1 if relu else 0) | (2 if accumulate else 0) | (8 if _overlapped else 0) | (16 if layout == 'bf16x3' else 0)
    if mask is not None:
        _chk(mask, 'mask')
        assert mask.shape == out.shape
        rc = lib().dm_conv2d_fwd_masked(_ptr_array(srcs), _int_array([s.shape[1] for s in srcs]), strides, len(srcs), NB, H, W,
                                        _p(w_packed), _p(bias), cout, ksize, flags, _p(out), out.shape[1], out_ch_offset,
                                        _p(mask), _stream())
        check(rc, 'dm_conv2d_fwd_masked')
        return out
    if CONV_SPLITK[0] and _SPLITK_DEPTH[0] > 0 and not accumulate:
        # the <= 100-RoI inference calls: a launch of few workgroups splits its K loop (dm_conv2d_fwd_ws)
        nws = int(lib().dm_conv2d_splitk_floats(NB, H, W, cout, ksize))
        if nws > 0:
            ws = torch.empty((nws,), device=out.device, dtype=torch.float32)
            rc = lib().dm_conv2d_fwd_ws(_ptr_array(srcs), _int_array([s.shape[1] for s in srcs]), strides, len(srcs), NB, H, W,
                                        _p(w_packed), _p(bias), cout, ksize, flags, _p(out), out.shape[1], out_ch_offset,
                                        _p(ws), nws, _stream())
            check(rc, 'dm_conv2d_fwd_ws')
            return out
    rc = lib().dm_conv2d_fwd(_ptr_array(srcs), _int_array([s.shape[1] for s in srcs]), strides, len(srcs), NB, H, W,
                             _p(w_packed), _p(bias), cout, ksize, flags, _p(out), out.shape[1], out_ch_offset, _stream())
    check(rc, 'dm_conv2d_fwd')
    return out


CONV_PLAN_FIELDS = ('KS', 'WGM', 'WGN', 'WM', 'WN', 'CK', 'TAIL', 'PREC', 'POST', 'MAXPOS', 'ksplit', 'kchunks', 'q_begin', 'Q',
                    'grid_x', 'grid_y', 'nontemporal')


def conv2d_plan_raw(src_channels, NB, H, W, cout, ksize, flags=0, out_ch_total=None, out_ch_offset=0, workspace_floats=0,
                    has_mask=False, has_addend=False, src_batch_strides=None):
    """dm_conv2d_plan: (return code, records).  The code is the number of launches or the (negative) error the call with
    these arguments would return; ``flags`` are dm_conv2d_fwd's.  Host only: no tensor, no device."""
    consts = _abi.load()[1]
    n, cap = consts['DM_CONV_PLAN_INTS'], consts['DM_CONV_PLAN_MAX_LAUNCHES']
    assert len(CONV_PLAN_FIELDS) == n
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    strides = None if src_batch_strides is None else (ctypes.c_longlong * len(src_batch_strides))(*[int(v) for v in src_batch_strides])
    rc = lib().dm_conv2d_plan(_int_array(src_channels), strides, len(src_channels), int(NB), int(H), int(W), int(cout), int(ksize),
                              int(flags), int(cout if out_ch_total is None else out_ch_total), int(out_ch_offset),
                              int(workspace_floats), 1 if has_mask else 0, 1 if has_addend else 0, rec, cap)
    return rc, [dict(zip(CONV_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def conv2d_plan(src_channels, NB, H, W, cout, ksize, relu=False, accumulate=False, overlapped=False, bf16x3=False, **kw):
    """The launches ``conv2d`` would make for this shape, as the launcher reports them (include/dynamask_hip.h,
    dm_conv2d_plan): a list of one or two dicts with the keys CONV_PLAN_FIELDS (two: a 3x3 launch whose underfull last
    round goes to a second launch).  Raises where the call would fail.  ``workspace_floats`` > 0: the dm_conv2d_fwd_ws
    call; ``has_mask`` / ``has_addend``: the masked / post-add calls."""
    flags = (1 if relu else 0) | (2 if accumulate else 0) | (8 if overlapped else 0) | (16 if bf16x3 else 0)
    rc, recs = conv2d_plan_raw(src_channels, NB, H, W, cout, ksize, flags, **kw)
    if rc < 0:
        check(rc, 'dm_conv2d_plan')
    return recs


def conv1x1_group(xs, w_packeds, biases, couts, relu=False, outs=None):
    """Up to three independent single-source 1x1 convolutions (+ bias, + ReLU) as ONE launch (dm_conv1x1_group_fwd): the
    FPN-wide semantic convolutions of the SFM stages.  Same bits as ``conv2d`` per problem.  The weights are all of one
    layout (``conv_layout``): the bf16x3 one runs the bf16x3 kernel."""
    k = len(xs)
    assert 1 <= k <= 3 and len(w_packeds) == k and len(biases) == k and len(couts) == k
    NB = xs[0].shape[0]
    for x, w in zip(xs, w_packeds):
        _chk(x, 'x')
        _chk(w, 'w_packed')
        assert x.shape[0] == NB
    layout = conv_layout(w_packeds[0])
    assert all(conv_layout(w) == layout for w in w_packeds), 'weights of one group packed in different layouts'
    for x, w, c in zip(xs, w_packeds, couts):
        assert w.numel() == packed_floats(c, 1, [x.shape[1]], layout), 'weights packed for other sources'
    if outs is None:
        outs = [torch.empty((NB, c, x.shape[2], x.shape[3]), device=x.device, dtype=torch.float32) for x, c in zip(xs, couts)]
    for o, x, c in zip(outs, xs, couts):
        _chk(o, 'out')
        assert tuple(o.shape) == (NB, c, x.shape[2], x.shape[3])
    bias_arr = (ctypes.c_void_p * k)(*[0 if b is None else _chk(b, 'bias').data_ptr() for b in biases])
    if hazard.ENABLED[0]:
        hazard.note_ptr_array(bias_arr, [b for b in biases if b is not None])
    check(lib().dm_conv1x1_group_fwd(k, _ptr_array(xs), _int_array([x.shape[1] for x in xs]), _int_array([x.shape[2] for x in xs]),
                                     _int_array([x.shape[3] for x in xs]), NB, _ptr_array(w_packeds), bias_arr, _int_array(couts),
                                     (1 if relu else 0) | (16 if layout == 'bf16x3' else 0), _ptr_array(outs), _stream()),
          'dm_conv1x1_group_fwd')
    return outs


def deform_conv(x, offset, w_packed, cout, deform_groups, relu=False, out=None):
    _chk(x, 'x')
    _chk(offset, 'offset')
    _chk(w_packed, 'w_packed')
    NB, C, H, W = x.shape
    assert offset.shape == (NB, deform_groups * 18, H, W)
    assert w_packed.numel() == packed_floats(cout, 3, [C])
    if out is None:
        out = torch.empty((NB, cout, H, W), device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (NB, cout, H, W)
    if CONV_SPLITK[0] and _SPLITK_DEPTH[0] > 0:
        nws = int(lib().dm_deform_conv_splitk_floats(NB, C, H, W, cout))
        if nws > 0:
            ws = torch.empty((nws,), device=out.device, dtype=torch.float32)
            check(lib().dm_deform_conv_fwd_ws(_p(x), _p(offset), NB, C, H, W, _p(w_packed), cout, deform_groups,
                                              (1 if relu else 0) | (8 if _overlapped else 0), _p(out), _p(ws), nws, _stream()),
                  'dm_deform_conv_fwd_ws')
            return out
    check(lib().dm_deform_conv_fwd(_p(x), _p(offset), NB, C, H, W, _p(w_packed), cout, deform_groups,
                                   (1 if relu else 0) | (8 if _overlapped else 0), _p(out), _stream()), 'dm_deform_conv_fwd')
    return out


DCN_PLAN_FIELDS = ('kernel', 'P0', 'P1', 'P2', 'P3', 'threads', 'MT', 'q_begin', 'Q', 'grid_x', 'grid_y', 'ksplit', 'kchan',
                   'lds_bytes', 'reduce')
DCN_KERNELS = ('generic', 'lds', 'c256', 'band')          # field 'kernel' of a plan record


def deform_conv_plan_raw(NB, C, H, W, cout, deform_groups, flags=0, workspace_floats=0, m2=0):
    """dm_deform_conv_plan: (return code, records).  The code is the number of launches or the (negative) error the call
    with these arguments would return; ``flags`` are dm_deform_conv_fwd's.  Host only: no tensor, no device."""
    consts = _abi.load()[1]
    n, cap = consts['DM_DCN_PLAN_INTS'], consts['DM_DCN_PLAN_MAX_LAUNCHES']
    assert len(DCN_PLAN_FIELDS) == n
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    rc = lib().dm_deform_conv_plan(int(NB), int(C), int(H), int(W), int(cout), int(deform_groups), int(flags),
                                   int(workspace_floats), int(m2), rec, cap)
    return rc, [dict(zip(DCN_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def deform_conv_plan(NB, C, H, W, cout, deform_groups, relu=False, overlapped=False, workspace_floats=0, m2=0):
    """The launches ``deform_conv`` (``m2`` > 0: ``deform_conv_tout``) would make for this shape, as the launcher's own
    route says (include/dynamask_hip.h, dm_deform_conv_plan): a list of one or two dicts with the keys DCN_PLAN_FIELDS
    (two: a launch whose underfull last round goes to a second launch).  Raises where the call would fail.
    ``workspace_floats`` > 0: the dm_deform_conv_fwd_ws call."""
    rc, recs = deform_conv_plan_raw(NB, C, H, W, cout, deform_groups, (1 if relu else 0) | (8 if overlapped else 0),
                                    workspace_floats, m2)
    if rc < 0:
        check(rc, 'dm_deform_conv_plan')
    return recs


def deform_conv_tout_supported(x, cout, m2):
    """Can ``deform_conv_tout`` take this shape (else: ``deform_conv`` + ``conv2d``)?"""
    NB, C, H, W = x.shape
    return bool(lib().dm_deform_conv_tout_supported(NB, C, H, W, cout, m2))


def pack_tout_weight(w):
    """The 1x1 weight [M2, C, 1, 1] behind a DCN, as ``deform_conv_tout`` reads it: transposed [C][M2 padded to 32], zeros
    in the padding."""
    m2, c = w.shape[0], w.shape[1]
    m2p = (m2 + 31) // 32 * 32
    out = torch.zeros((c, m2p), device=w.device, dtype=torch.float32)
    out[:, :m2] = w.detach().reshape(m2, c).t()
    return out


def deform_conv_tout(x, offset, w_packed, cout, deform_groups, w2t, b2, m2, out2, keep_dcn=False, dcn_out=None):
    """relu(DCN 3x3) -> 1x1 conv + bias + ReLU into channels [0, m2) of ``out2`` in ONE launch (dm_deform_conv_tout_fwd:
    the second GEMM runs on the DCN's accumulators in registers; same bits as ``deform_conv(relu=True)`` followed by
    ``conv2d(relu=True, out=out2)``).  ``keep_dcn``: also return relu(DCN) (else it is never written)."""
    _chk(x, 'x')
    _chk(offset, 'offset')
    _chk(w_packed, 'w_packed')
    _chk(w2t, 'w2t')
    _chk(b2, 'b2')
    _chk(out2, 'out2')
    NB, C, H, W = x.shape
    assert offset.shape == (NB, deform_groups * 18, H, W)
    assert w_packed.numel() == packed_floats(cout, 3, [C])
    assert tuple(w2t.shape) == (cout, (m2 + 31) // 32 * 32) and b2.numel() == m2
    assert out2.shape[0] == NB and tuple(out2.shape[2:]) == (H, W) and out2.shape[1] >= m2
    dcn = None
    if dcn_out is not None:                 # (a caller's buffer for relu(DCN): implies keep_dcn)
        dcn = _chk(dcn_out, 'dcn_out')
        assert tuple(dcn.shape) == (NB, cout, H, W)
    elif keep_dcn:
        dcn = torch.empty((NB, cout, H, W), device=x.device, dtype=torch.float32)
    check(lib().dm_deform_conv_tout_fwd(_p(x), _p(offset), NB, C, H, W, _p(w_packed), cout, deform_groups, _p(w2t), _p(b2), m2,
                                        _p(out2), out2.shape[1], _p(dcn), _stream()), 'dm_deform_conv_tout_fwd')
    return dcn


# ------------------------------------------------ RefineMask: dilated and any-width 3x3 convolutions (csrc/conv_dilated.hip)
# Exact fp32 in every precision mode (as the DCN kernels): the bf16x3 mode does not reach these launches.
def _dil_check(x, w_packed, cout):
    _chk(x, 'x')
    _chk(w_packed, 'w_packed')
    if conv_layout(w_packed) != 'fp32':
        raise ValueError('the dilated 3x3 kernels read the exact fp32 layout (pack_conv_weight(precision="fp32"))')
    assert w_packed.numel() == packed_floats(cout, 3, [x.shape[1]]), 'weights packed for another shape'


def _dil_out(x, cout, out):
    NB, _, H, W = x.shape
    if out is None:
        return torch.empty((NB, cout, H, W), device=x.device, dtype=torch.float32)
    _chk(out, 'out')
    assert tuple(out.shape) == (NB, cout, H, W)
    return out


def conv3x3_dil_supported(x, cout, dilation):
    """Does ``conv3x3_dil`` take this shape (dm_conv3x3_dil_supported: C % 8 == 0, 1 <= dilation <= 8, any H, W)?"""
    NB, C, H, W = x.shape
    return bool(lib().dm_conv3x3_dil_supported(NB, C, H, W, int(cout), int(dilation)))


def conv3x3_dil(x, w_packed, bias, cout, dilation, relu=False, add=False, out=None):
    """conv3x3(x, dilation = padding = ``dilation``) + bias (+ ReLU) -> [NB, cout, H, W] (dm_conv3x3_dil_fwd).  ``add``:
    ``out`` += that value (after the ReLU).  ``w_packed``: ``pack_conv_weight`` of the [cout, C, 3, 3] weight."""
    _dil_check(x, w_packed, cout)
    if bias is not None:
        _chk(bias, 'bias')
    if add and out is None:
        raise ValueError('add=True needs out')
    out = _dil_out(x, cout, out)
    NB, C, H, W = x.shape
    check(lib().dm_conv3x3_dil_fwd(_p(x), NB, C, H, W, _p(w_packed), _p(bias), cout, int(dilation),
                                   (1 if relu else 0) | (4 if add else 0), _p(out), _stream()), 'dm_conv3x3_dil_fwd')
    return out


def conv3x3_multidil_supported(x, cout, dilations):
    NB, C, H, W = x.shape
    return bool(lib().dm_conv3x3_multidil_supported(NB, C, H, W, int(cout), len(dilations), _int_array(dilations)))


# MultiBranchFusion: the three branches as ONE launch (dm_conv3x3_multidil_fwd); False: three dm_conv3x3_dil_fwd, the
# second and third adding into the first's output (the A/B baseline; same bits)
FUSED_MULTIDIL = [os.environ.get('DM_FUSED_MULTIDIL', '1') != '0']


def conv3x3_multidil(x, w_packeds, biases, cout, dilations, relu=True, out=None, fused=None):
    """sum_b act(conv3x3_{dilations[b]}(x) + biases[b]) -> [NB, cout, H, W], act = ReLU if ``relu``: MultiBranchFusion's
    branch sum (refine_mask_head.py:28-31).  ``fused`` (default FUSED_MULTIDIL): one launch, else the unfused sequence."""
    k = len(dilations)
    assert len(w_packeds) == k and len(biases) == k
    for w in w_packeds:
        _dil_check(x, w, cout)
    for b in biases:
        if b is not None:
            _chk(b, 'bias')
    out = _dil_out(x, cout, out)
    if fused is None:
        fused = FUSED_MULTIDIL[0]
    if fused:
        NB, C, H, W = x.shape
        bias_arr = (ctypes.c_void_p * k)(*[0 if b is None else b.data_ptr() for b in biases])
        if hazard.ENABLED[0]:
            hazard.note_ptr_array(bias_arr, [b for b in biases if b is not None])
        check(lib().dm_conv3x3_multidil_fwd(_p(x), NB, C, H, W, _ptr_array(w_packeds), bias_arr, cout, k, _int_array(dilations),
                                            1 if relu else 0, _p(out), _stream()), 'dm_conv3x3_multidil_fwd')
        return out
    for i, (w, b, d) in enumerate(zip(w_packeds, biases, dilations)):
        conv3x3_dil(x, w, b, cout, d, relu=relu, add=i > 0, out=out)
    return out


def sigmoid(x, out=None):
    """Elementwise logistic (dm_sigmoid_fwd; the paste kernels' expression)."""
    _chk(x, 'x')
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, 'out')
        assert out.shape == x.shape
    check(lib().dm_sigmoid_fwd(_p(x), x.numel(), _p(out), _stream()), 'dm_sigmoid_fwd')
    return out


# ------------------------------------------------ PointRend: the subdivision step (csrc/point_refine.hip)
# Exact fp32 in every precision mode: the bf16x3 mode does not reach these launches.
def _cells(t):
    """Cells per row of a [n, ...] map (also when n == 0)."""
    hw = 1
    for d in t.shape[1:]:
        hw *= int(d)
    return hw


def point_select_supported(hw, num_points, n=1):
    return bool(lib().dm_point_select_supported(int(n), int(hw), int(num_points)))


def point_select(refined, num_points, out=None):
    """The ``num_points`` cells of smallest |v| per row of the label-channel map ``refined`` [n, 1, H, W] (or [n, HW]):
    ``topk(-|v|, num_points)`` of MaskPointHead.get_roi_rel_points_test -> int32 [n, num_points], indices in ascending
    order; among equal |v| at the cut the lower index is taken (dm_point_select)."""
    _chk(refined, 'refined')
    n = refined.shape[0]
    hw = _cells(refined)
    P = int(num_points)
    if out is None:
        out = torch.empty((n, P), device=refined.device, dtype=torch.int32)
    _chk(out, 'out', torch.int32)
    assert tuple(out.shape) == (n, P)
    check(lib().dm_point_select(_p(refined), n, hw, P, _p(out), _stream()), 'dm_point_select')
    return out


def point_gather(feat, rois, coarse, idx, mh, mw, spatial_scale, out=None):
    """The point head's input [n, C + NC, P] at the cells ``idx`` [n, P] of an ``mh`` x ``mw`` grid: channels < C the
    point_sample of ``feat`` [B, C, H, W] (the image of each RoI) at the cell centres mapped into the image
    (rel_roi_point_to_rel_img_point with ``spatial_scale``), channels >= C the point_sample of the RoI's ``coarse``
    [n, NC, CH, CW] logits at the RoI-relative centres (dm_point_gather_fwd)."""
    _chk(feat, 'feat')
    _chk(rois, 'rois')
    _chk(coarse, 'coarse')
    _chk(idx, 'idx', torch.int32)
    B, C, H, W = feat.shape
    n, P = idx.shape
    NC, CH, CW = coarse.shape[1:]
    assert rois.shape == (n, 5) and coarse.shape[0] == n
    if out is None:
        out = torch.empty((n, C + NC, P), device=feat.device, dtype=torch.float32)
    _chk(out, 'out')
    assert tuple(out.shape) == (n, C + NC, P)
    check(lib().dm_point_gather_fwd(_p(feat), B, C, H, W, _p(rois), n, _p(coarse), NC, CH, CW, _p(idx), P, int(mh), int(mw),
                                    float(spatial_scale), _p(out), _stream()), 'dm_point_gather_fwd')
    return out


def point_scatter(vals, idx, refined):
    """refined[r].flatten()[idx[r, p]] = vals[r, p] in place (dm_point_scatter)."""
    _chk(vals, 'vals')
    _chk(idx, 'idx', torch.int32)
    _chk(refined, 'refined')
    n, P = idx.shape
    assert vals.numel() == n * P and refined.shape[0] == n
    check(lib().dm_point_scatter(_p(vals), _p(idx), n, P, _p(refined), _cells(refined), _stream()),
          'dm_point_scatter')
    return refined


# MaskPointHead's MLP + the scatter as ONE launch (dm_point_mlp_fwd); False: the unfused sequence -- each layer a
# dm_conv2d_fwd 1x1 on the points as a 1 x P image, dm_class_logits_fwd for the label row, dm_point_scatter (the A/B
# baseline; the same arithmetic in another association)
FUSED_POINT_MLP = [os.environ.get('DM_FUSED_POINT_MLP', '1') != '0']


def point_mlp_supported(x, num_fcs, ncl, hw):
    n, CT, P = x.shape
    return bool(lib().dm_point_mlp_supported(n, P, 256, CT - 256, 256, int(num_fcs), int(ncl), int(hw)))


def point_mlp_scatter(x, w_packeds, biases, w_logits, b_logits, labels, idx, refined, fused=None):
    """MaskPointHead.forward (coarse_pred_each_layer) on the point features ``x`` [n, 256 + NC, P] (``point_gather``):
    relu(W_l [h; coarse] + b_l) per layer, then the ``labels`` row of fc_logits, stored into ``refined`` [n, 1, H, W] at
    the cells ``idx`` [n, P] (in place).  ``w_packeds``: ``pack_conv_weight`` of each [256, 256 + NC, 1, 1] weight;
    ``w_logits`` [NCL, 256 + NC], ``b_logits`` [NCL].  ``fused`` (default FUSED_POINT_MLP): one launch, else the
    unfused sequence."""
    _chk(x, 'x')
    _chk(w_logits, 'w_logits')
    _chk(labels, 'labels', torch.int64)
    _chk(idx, 'idx', torch.int32)
    _chk(refined, 'refined')
    n, CT, P = x.shape
    k = len(w_packeds)
    assert len(biases) == k and tuple(idx.shape) == (n, P) and refined.shape[0] == n and labels.shape == (n,)
    for w in w_packeds:
        _chk(w, 'w_packed')
        if conv_layout(w) != 'fp32':
            raise ValueError('the point MLP reads the exact fp32 layout (pack_conv_weight(precision="fp32"))')
        assert w.numel() == packed_floats(256, 1, [CT]), 'weights packed for another shape'
    if b_logits is not None:
        _chk(b_logits, 'b_logits')
    hw = _cells(refined)
    if fused is None:
        fused = FUSED_POINT_MLP[0]
    if fused:
        bias_arr = (ctypes.c_void_p * k)(*[0 if b is None else _chk(b, 'bias').data_ptr() for b in biases])
        if hazard.ENABLED[0]:
            hazard.note_ptr_array(bias_arr, [b for b in biases if b is not None])
        check(lib().dm_point_mlp_fwd(_p(x), n, P, 256, CT - 256, 256, k, _ptr_array(w_packeds), bias_arr, _p(w_logits),
                                     _p(b_logits), w_logits.shape[0], _p(labels), _p(idx), 0, _p(refined), hw, _stream()),
              'dm_point_mlp_fwd')
        return refined
    if n == 0:
        return refined
    # ping-pong between two [n, 256 + NC, 1, P] buffers that both hold the coarse channels
    bufs = [x.view(n, CT, 1, P), x.clone().view(n, CT, 1, P), None]
    bufs[2] = bufs[1].clone()
    cur = bufs[0]
    for i, (w, b) in enumerate(zip(w_packeds, biases)):
        dst = bufs[1 + (i % 2)]
        conv2d([cur], w, b, 256, 1, relu=True, out=dst, out_ch_offset=0)
        cur = dst
    nl = w_logits.shape[0]
    lab = labels.clamp(0, nl - 1).contiguous()
    bl = b_logits if b_logits is not None else torch.zeros((nl,), device=x.device, dtype=torch.float32)
    vals, _ = class_logits(cur, w_logits, bl, w_logits, bl, lab)
    return point_scatter(vals, idx, refined)


# ------------------------------------------------ PointRefine: one SFM stage's point step (csrc/point_refine.hip, K24)
# Exact fp32 in every precision mode: the bf16x3 mode does not reach these launches.
def point_topk_select_supported(hw, num_points, n=1):
    return bool(lib().dm_point_topk_select_supported(int(n), int(hw), int(num_points), 1))


def point_topk_select(detail, num_points, use_sigmoid=True, out=None):
    """The ``num_points`` cells of LARGEST key per row of the detail map ``detail`` [n, 1, S, S] (or [n, HW]), key
    ``sigmoid(v)`` (``use_sigmoid``) or ``v``: ``topk`` of SFMStage.get_roi_rel_points_train -> int32 [n, num_points],
    indices ascending; among equal keys at the cut the lower index is taken (dm_point_topk_select)."""
    _chk(detail, 'detail')
    n = detail.shape[0]
    hw = _cells(detail)
    P = int(num_points)
    if out is None:
        out = torch.empty((n, P), device=detail.device, dtype=torch.int32)
    _chk(out, 'out', torch.int32)
    assert tuple(out.shape) == (n, P)
    check(lib().dm_point_topk_select(_p(detail), n, hw, P, 1 if use_sigmoid else 0, _p(out), _stream()),
          'dm_point_topk_select')
    return out


def point_feat_gather(feat, rois, coarse, idx, spatial_scale, out=None):
    """The point MLP's input [n, C + NC, P] of an SFM stage at the cells ``idx`` [n, P] of the S x S grid of ``coarse``
    [n, NC, S, S] (``idx`` None: every cell, P = S * S): channels < C the point_sample of ``feat`` [B, C, H, W] (the image
    of each RoI, ``rois[:, 0]``) at the cell centres mapped into the image (rel_roi_point_to_rel_img_point with
    ``spatial_scale``), channels >= C the exact values of ``coarse`` at the cells (dm_point_feat_gather)."""
    _chk(feat, 'feat')
    _chk(rois, 'rois')
    _chk(coarse, 'coarse')
    B, C, H, W = feat.shape
    n, NC, S = coarse.shape[0], coarse.shape[1], coarse.shape[2]
    assert coarse.shape[3] == S and tuple(rois.shape) == (n, 5)
    if idx is None:
        P = S * S
    else:
        _chk(idx, 'idx', torch.int32)
        assert idx.shape[0] == n
        P = idx.shape[1]
    if out is None:
        out = torch.empty((n, C + NC, P), device=feat.device, dtype=torch.float32)
    _chk(out, 'out')
    assert tuple(out.shape) == (n, C + NC, P)
    check(lib().dm_point_feat_gather(_p(feat), B, C, H, W, _p(rois), n, _p(coarse), NC, _p(idx), P, S, float(spatial_scale),
                                     _p(out), _stream()), 'dm_point_feat_gather')
    return out


def point_scatter_rows(vals, idx, feat):
    """feat[r, c].flatten()[idx[r, p]] = vals[r, c, p] in place (dm_point_scatter_rows)."""
    _chk(vals, 'vals')
    _chk(idx, 'idx', torch.int32)
    _chk(feat, 'feat')
    n, P = idx.shape
    C = feat.shape[1]
    assert vals.numel() == n * C * P and feat.shape[0] == n
    check(lib().dm_point_scatter_rows(_p(vals), _p(idx), n, C, P, _p(feat), _cells(feat) // max(C, 1), _stream()),
          'dm_point_scatter_rows')
    return feat


# The SFM stage's point MLP + scatter: 'fused' -- one launch (dm_point_refine_mlp); 'unfused' -- each layer a
# dm_conv2d_fwd 1x1 on the points as a 1 x P image, then dm_point_scatter_rows (when every cell is selected the last
# layer writes the stage features directly: the dense form).  DM_POINT_REFINE_MLP=fused / unfused forces one;
# default (None): the per-shape choice of point_refine_mlp_form.
POINT_REFINE_MLP = [os.environ.get('DM_POINT_REFINE_MLP') or None]


def point_refine_mlp_supported(n, C, NC, P, num_fcs, hw, has_idx=True):
    return bool(lib().dm_point_refine_mlp_supported(int(n), int(P), int(C), int(NC), int(num_fcs), int(hw),
                                                    1 if has_idx else 0))


def point_refine_mlp_form(n, C, P, hw):
    """The default form of an SFM stage's point MLP for n RoIs, C channels and P of hw cells."""
    if POINT_REFINE_MLP[0] in ('fused', 'unfused'):
        return POINT_REFINE_MLP[0]
    # measured at 16 / 100 RoIs: at C = 256 (S = 14, every cell) the dense 1x1 sequence wins (0.075 / 0.19 ms against
    # 0.125 / 0.29 ms fused), at C = 128 / 64 the fused launch does (0.26 / 0.16 ms against 0.28 / 0.18 ms at 100 RoIs).
    # The choice does not depend on n, so a batch of images computes what each image alone does.
    return 'unfused' if C >= 256 else 'fused'


def point_refine_mlp(x, C, w_packeds, biases, idx, feat, form=None):
    """SFMStage's point MLP (coarse_pred_each_layer) on the point features ``x`` [n, C + NC, P] (``point_feat_gather``):
    relu(W_l [h; coarse] + b_l) per hidden layer, then fc_logits (no ReLU), ALL C rows stored into ``feat`` [n, C, S, S]
    at the cells ``idx`` [n, P] (in place; ``idx`` None: every cell in order).  ``w_packeds`` / ``biases``: the hidden
    layers then fc_logits, each ``pack_conv_weight`` of a [C, C + NC, 1, 1] weight.  ``form``: 'fused' (one launch),
    'unfused' (the launch sequence) or None (``point_refine_mlp_form``)."""
    _chk(x, 'x')
    _chk(feat, 'feat')
    n, CT, P = x.shape
    NC = CT - C
    k = len(w_packeds) - 1
    assert k >= 1 and len(biases) == k + 1 and feat.shape[0] == n and feat.shape[1] == C
    hw = _cells(feat) // C
    if idx is not None:
        _chk(idx, 'idx', torch.int32)
        assert tuple(idx.shape) == (n, P)
    else:
        assert P == hw, 'without an index every cell is a point'
    for w in w_packeds:
        _chk(w, 'w_packed')
        if conv_layout(w) != 'fp32':
            raise ValueError('the point MLP reads the exact fp32 layout (pack_conv_weight(precision="fp32"))')
        assert w.numel() == packed_floats(C, 1, [CT]), 'weights packed for another shape'
    if form is None:
        form = point_refine_mlp_form(n, C, P, hw)
    if form == 'fused':
        bias_arr = (ctypes.c_void_p * (k + 1))(*[0 if b is None else _chk(b, 'bias').data_ptr() for b in biases])
        if hazard.ENABLED[0]:
            hazard.note_ptr_array(bias_arr, [b for b in biases if b is not None])
        check(lib().dm_point_refine_mlp(_p(x), n, P, C, NC, k, _ptr_array(w_packeds), bias_arr, _p(idx), 0, _p(feat), hw,
                                        _stream()), 'dm_point_refine_mlp')
        return feat
    if form != 'unfused':
        raise ValueError(f'point_refine_mlp: form {form!r} (fused / unfused)')
    if n == 0:
        return feat
    # ping-pong between two [n, C + NC, 1, P] buffers that both hold the coarse channels
    bufs = [x.view(n, CT, 1, P), x.clone().view(n, CT, 1, P), None]
    bufs[2] = bufs[1].clone() if k > 1 else None
    cur = bufs[0]
    for i in range(k):
        dst = bufs[1 + (i % 2)]
        conv2d([cur], w_packeds[i], biases[i], C, 1, relu=True, out=dst, out_ch_offset=0)
        cur = dst
    if idx is None:                     # dense: the points are the cells in order, fc_logits writes the features
        conv2d([cur], w_packeds[k], biases[k], C, 1, out=feat.view(n, C, 1, P))
        return feat
    vals = conv2d([cur], w_packeds[k], biases[k], C, 1)
    return point_scatter_rows(vals, idx, feat)


# ------------------------------------------------ Mask Scoring R-CNN: the IoU head's launches (csrc/conv_strided.hip)
# Exact fp32 in every precision mode: the bf16x3 mode does not reach these launches.
def conv3x3_s2_supported(x, cout, splits=0):
    """Does ``conv3x3_s2`` take this shape (dm_conv3x3_s2_supported: C % 8 == 0, any H, W; splits 0 or 1/2/4/8 <= C / 8)?"""
    NB, C, H, W = x.shape
    return bool(lib().dm_conv3x3_s2_supported(NB, C, H, W, int(cout), int(splits)))


def conv3x3_s2(x, w_packed, bias, cout, relu=False, splits=0, out=None):
    """Conv2d(C, cout, 3, stride=2, padding=1)(x) + bias (+ ReLU) -> [NB, cout, ceil(H / 2), ceil(W / 2)]
    (dm_conv3x3_s2_fwd).  ``w_packed``: ``pack_conv_weight`` of the [cout, C, 3, 3] weight (the stride-1 layout).
    ``splits``: workgroups per tile over the K loop (0: the library's choice; 1, 2, 4, 8: forced)."""
    _dil_check(x, w_packed, cout)
    if bias is not None:
        _chk(bias, 'bias')
    NB, C, H, W = x.shape
    shape = (NB, int(cout), (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    nws = int(lib().dm_conv3x3_s2_workspace_floats(NB, C, H, W, int(cout), int(splits)))
    ws = torch.empty((nws,), device=x.device, dtype=torch.float32) if nws > 0 else None
    check(lib().dm_conv3x3_s2_fwd(_p(x), NB, C, H, W, _p(w_packed), _p(bias), int(cout), int(splits), 1 if relu else 0,
                                  _p(out), _p(ws), max(nws, 0), _stream()), 'dm_conv3x3_s2_fwd')
    return out


def mask_iou_input(mask_pred, labels):
    """max_pool2d(sigmoid(mask_pred[i, labels[i]]), 2, 2) -> [n, 1, S / 2, S / 2] (dm_mask_iou_input): ``mask_pred``
    [n, C, S, S] logits (C == 1: class-agnostic, ``labels`` may be None), ``labels`` [n] int64."""
    _chk(mask_pred, 'mask_pred')
    n, C, H, W = mask_pred.shape
    if C > 1 or labels is not None:
        _chk(labels, 'labels', torch.int64)
        assert labels.shape == (n,)
    out = torch.empty((n, 1, H // 2, W // 2), device=mask_pred.device, dtype=torch.float32)
    check(lib().dm_mask_iou_input(_p(mask_pred), n, C, H, W, _p(labels), _p(out), _stream()), 'dm_mask_iou_input')
    return out


def mask_iou_scores(mask_iou_pred, labels, dets):
    """mask_iou_pred[i, labels[i]] * dets[i, -1] -> [n] (dm_mask_iou_scores; MaskIoUHead.get_mask_scores)."""
    _chk(mask_iou_pred, 'mask_iou_pred')
    _chk(labels, 'labels', torch.int64)
    _chk(dets, 'dets')
    n, nc = mask_iou_pred.shape
    assert labels.shape == (n,) and dets.dim() == 2 and dets.shape[0] == n
    out = torch.empty((n,), device=mask_iou_pred.device, dtype=torch.float32)
    check(lib().dm_mask_iou_scores(_p(mask_iou_pred), n, nc, _p(labels), _p(dets), dets.shape[1], _p(out), _stream()),
          'dm_mask_iou_scores')
    return out


def pack_deconv_weight(w, precision='fp32'):
    """``precision='bf16x3'``: dm_deconv_pack_weight_bf16x3's layout, marked as such (``conv_layout``)."""
    _chk(w, 'weight')
    precision = _precision.checked(precision)
    cin, cout, kh, kw = w.shape
    assert kh == 2 and kw == 2
    wp = torch.empty((packed_floats(4 * cout, 1, [cin], precision),), device=w.device, dtype=torch.float32)
    fn, name = ((lib().dm_deconv_pack_weight_bf16x3, 'dm_deconv_pack_weight_bf16x3') if precision == 'bf16x3'
                else (lib().dm_deconv_pack_weight, 'dm_deconv_pack_weight'))
    check(fn(_p(w), cin, cout, _p(wp), _stream()), name)
    if precision == 'bf16x3':
        wp._dm_bf16x3 = True
    return wp


def deconv2x2(x, w_packed, bias, cout, relu=False):
    """The bf16x3 layout (``pack_deconv_weight(precision='bf16x3')``) runs the bf16x3 kernel (flag bit 4)."""
    _chk(x, 'x')
    _chk(w_packed, 'w_packed')
    NB, C, H, W = x.shape
    layout = conv_layout(w_packed)
    assert w_packed.numel() == packed_floats(4 * cout, 1, [C], layout), 'weights packed for another shape'
    out = torch.empty((NB, cout, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    check(lib().dm_deconv2x2_fwd(_p(x), NB, C, H, W, _p(w_packed), _p(bias), cout,
                                 (1 if relu else 0) | (16 if layout == 'bf16x3' else 0), _p(out), _stream()), 'dm_deconv2x2_fwd')
    return out


def carafe(x, enc, up_kernel=5, group=1, scale=2):
    _chk(x, 'x')
    _chk(enc, 'enc')
    NB, C, H, W = x.shape
    assert enc.shape == (NB, up_kernel * up_kernel * group * scale * scale, H, W)
    out = torch.empty((NB, C, H * scale, W * scale), device=x.device, dtype=torch.float32)
    check(lib().dm_carafe_fwd(_p(x), _p(enc), NB, C, H, W, up_kernel, group, scale, _p(out), _stream()),
          'dm_carafe_fwd')
    return out


def _carafe_map_size(H, W, out_size):
    if out_size is None:
        return 2 * H, 2 * W
    OH, OW = out_size
    return int(OH), int(OW)


def carafe_map_supported(x_or_shape, up_kernel, group, out_size=None):
    """dm_carafe_map_supported: does ``carafe_map`` take this map (a tensor or its shape) at this ``out_size`` (default
    2H x 2W)?  Host only."""
    NB, C, H, W = x_or_shape.shape if isinstance(x_or_shape, torch.Tensor) else x_or_shape
    OH, OW = _carafe_map_size(int(H), int(W), out_size)
    return bool(lib().dm_carafe_map_supported(int(NB), int(C), int(H), int(W), int(up_kernel), int(group), OH, OW))


def carafe_map(x, enc, up_kernel=5, group=1, addend=None, out=None, out_size=None, chan_split=0):
    """``addend + carafe(x, softmax_taps(pixel_shuffle(enc)))[:, :, :OH, :OW]`` at scale 2, one launch (dm_carafe_map_fwd):
    CARAFE on a whole map with FPN_CARAFE's cropped add.  ``x`` [NB, C, H, W]; ``enc`` [NB, group * K * K * 4, H, W], the
    raw content-encoder output; ``out_size`` (OH, OW) with 2H - 1 <= OH <= 2H and 2W - 1 <= OW <= 2W (default: that of
    ``out``, else of ``addend``, else 2H x 2W); ``addend`` [NB, C, OH, OW] or None; ``out`` may be ``addend`` itself.
    ``chan_split``: workgroups per pixel tile over the group's channels (0: the library's choice; the bits do not depend
    on it)."""
    _chk(x, 'x')
    _chk(enc, 'enc')
    if x.dim() != 4 or enc.dim() != 4:
        raise ValueError(f'carafe_map: x and enc are 4-D, got {list(x.shape)} and {list(enc.shape)}')
    NB, C, H, W = x.shape
    up_kernel, group = int(up_kernel), int(group)
    if tuple(enc.shape) != (NB, up_kernel * up_kernel * group * 4, H, W):
        raise ValueError(f'enc: [{NB}, {up_kernel * up_kernel * group * 4}, {H}, {W}] expected, got {list(enc.shape)}')
    if out_size is None:
        ref = out if out is not None else addend
        out_size = tuple(ref.shape[2:]) if isinstance(ref, torch.Tensor) and ref.dim() == 4 else None
    OH, OW = _carafe_map_size(H, W, out_size)
    shape = (NB, C, OH, OW)
    if addend is not None:
        _chk(addend, 'addend')
        if tuple(addend.shape) != shape:
            raise ValueError(f'addend: {list(shape)} expected, got {list(addend.shape)}')
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != shape:
            raise ValueError(f'out: {list(shape)} expected, got {list(out.shape)}')
    check(lib().dm_carafe_map_fwd(_p(x), _p(enc), NB, C, H, W, up_kernel, group, _p(addend), OH, OW, int(chan_split), _p(out),
                                  _stream()), 'dm_carafe_map_fwd')
    return out


# ------------------------------------------------------------ bandwidth kernels
def point_sample(feat, rois, output_size, spatial_scale):
    _chk(feat, 'feat')
    _chk(rois, 'rois')
    B, C, H, W = feat.shape
    N = rois.shape[0]
    out = torch.empty((N, C, output_size, output_size), device=feat.device, dtype=torch.float32)
    check(lib().dm_point_sample_fwd(_p(feat), B, C, H, W, _p(rois), N, output_size, spatial_scale, _p(out),
                                    _stream()), 'dm_point_sample_fwd')
    return out


def class_logits(x, w_inst, b_inst, w_det, b_det, labels, sig_out=None, sig_ch_offset=0, out=None):
    _chk(x, 'x')
    for t, n in ((w_inst, 'w_inst'), (b_inst, 'b_inst'), (w_det, 'w_det'), (b_det, 'b_det')):
        _chk(t, n)
    _chk(labels, 'labels', torch.int64)
    N, C, H, W = x.shape
    nc = w_inst.shape[0]
    if out is None:
        inst = torch.empty((N, 1, H, W), device=x.device, dtype=torch.float32)
        det = torch.empty((N, 1, H, W), device=x.device, dtype=torch.float32)
    else:                                   # (inst, det): e.g. row slices of the buffers of a chunked launch sequence
        inst, det = out
        for t, nm in ((inst, 'out[0]'), (det, 'out[1]')):
            _chk(t, nm)
            assert tuple(t.shape) == (N, 1, H, W)
    sig_ct = 0
    if sig_out is not None:
        _chk(sig_out, 'sig_out')
        assert sig_out.shape[0] == N and sig_out.shape[2:] == x.shape[2:]
        sig_ct = sig_out.shape[1]
    check(lib().dm_class_logits_fwd(_p(x), N, C, H * W, _p(w_inst), _p(b_inst), _p(w_det), _p(b_det), nc,
                                    _p(labels), _p(inst), _p(det), _p(sig_out), sig_ct, sig_ch_offset, _stream()),
          'dm_class_logits_fwd')
    return inst, det


def class_logits_up2x_supported(x):
    return x.shape[3] % 2 == 0 and x.shape[2] >= 2 and x.shape[3] >= 2


def class_logits_up2x(x, w_inst, b_inst, w_det, b_det, labels, out=None):
    """``class_logits(upsample2x(x, align_corners=False, relu=True), ...)`` in one kernel, without the upsampled tensor
    (the stage before an exit).  x [N, C, H, W] -> (inst, det) [N, 1, 2H, 2W]."""
    _chk(x, 'x')
    for t, n in ((w_inst, 'w_inst'), (b_inst, 'b_inst'), (w_det, 'w_det'), (b_det, 'b_det')):
        _chk(t, n)
    _chk(labels, 'labels', torch.int64)
    N, C, H, W = x.shape
    nc = w_inst.shape[0]
    if out is None:
        inst = torch.empty((N, 1, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
        det = torch.empty((N, 1, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    else:
        inst, det = out
        for t, nm in ((inst, 'out[0]'), (det, 'out[1]')):
            _chk(t, nm)
            assert tuple(t.shape) == (N, 1, 2 * H, 2 * W)
    check(lib().dm_class_logits_up2x_fwd(_p(x), N, C, H, W, _p(w_inst), _p(b_inst), _p(w_det), _p(b_det), nc, _p(labels),
                                         _p(inst), _p(det), _stream()), 'dm_class_logits_up2x_fwd')
    return inst, det


def upsample2x(x, align_corners=False, relu=False, out=None):
    _chk(x, 'x')
    N, C, H, W = x.shape
    if out is None:
        out = torch.empty((N, C, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (N, C, 2 * H, 2 * W)
    check(lib().dm_upsample2x_bilinear_fwd(_p(x), N * C, H, W, 1 if align_corners else 0, 1 if relu else 0,
                                           _p(out), _stream()), 'dm_upsample2x_bilinear_fwd')
    return out


def boundary_merge_(coarse, fine):
    """In place on ``fine`` (as the reference, dynamask_roi_head.py:148)."""
    _chk(coarse, 'coarse')
    _chk(fine, 'fine')
    n, S = coarse.shape[0], coarse.shape[-1]
    assert fine.shape[0] == n and fine.shape[-1] == 2 * S and fine.shape[-2] == 2 * S
    check(lib().dm_boundary_merge(_p(coarse), _p(fine), n, S, _stream()), 'dm_boundary_merge')
    return fine


def boundary_merge_chain(p_s, p_2s, fine_or_final, out=None):
    """The inference tail in one launch (dm_boundary_merge_chain): ``merge(merge(p_s -> p_2s) -> fine)``.
    ``fine_or_final``: the [n, 1, 4S, 4S] fine logits (merged in place and returned), or the last stage's [n, 1, 2S, 2S]
    logits -- then the fine logits are their align_corners x2 upsample, computed inside the kernel, and the result goes
    to ``out`` (allocated if None).  ``p_2s`` is not modified."""
    _chk(p_s, 'p_s')
    _chk(p_2s, 'p_2s')
    _chk(fine_or_final, 'fine_or_final')
    n, S = p_s.shape[0], p_s.shape[-1]
    assert p_s.shape[-2] == S and tuple(p_2s.shape[-2:]) == (2 * S, 2 * S) and p_2s.shape[0] == n == fine_or_final.shape[0]
    if n == 0:
        return fine_or_final if fine_or_final.shape[-1] == 4 * S else p_s.new_zeros((0, 1, 4 * S, 4 * S))
    if fine_or_final.shape[-1] == 4 * S:
        assert out is None or out is fine_or_final
        check(lib().dm_boundary_merge_chain(_p(p_s), _p(p_2s), None, _p(fine_or_final), n, S, _stream()), 'dm_boundary_merge_chain')
        return fine_or_final
    assert tuple(fine_or_final.shape[-2:]) == (2 * S, 2 * S)
    if out is None:
        out = torch.empty((n, 1, 4 * S, 4 * S), device=p_s.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert out.shape[0] == n and tuple(out.shape[-2:]) == (4 * S, 4 * S)
    check(lib().dm_boundary_merge_chain(_p(p_s), _p(p_2s), _p(fine_or_final), _p(out), n, S, _stream()), 'dm_boundary_merge_chain')
    return out


def stage_head(sem, rois, output_size, spatial_scale, x, w_inst, b_inst, w_det, b_det, labels, sig_out=None, sig_ch_offset=0, out=None):
    """``point_sample(sem, rois, output_size, spatial_scale)`` and ``class_logits(x, ..., sig_out, sig_ch_offset, out)`` of
    one SFM stage as ONE launch (dm_stage_head_fwd) -> (sampled, inst, det)."""
    _chk(sem, 'sem')
    _chk(rois, 'rois')
    _chk(x, 'x')
    for t, n_ in ((w_inst, 'w_inst'), (b_inst, 'b_inst'), (w_det, 'w_det'), (b_det, 'b_det')):
        _chk(t, n_)
    _chk(labels, 'labels', torch.int64)
    B, Cs, H, W = sem.shape
    N, C, S, S2 = x.shape
    assert S == S2 == output_size and rois.shape[0] == N
    nc = w_inst.shape[0]
    sampled = torch.empty((N, Cs, S, S), device=x.device, dtype=torch.float32)
    if out is None:
        inst = torch.empty((N, 1, S, S), device=x.device, dtype=torch.float32)
        det = torch.empty((N, 1, S, S), device=x.device, dtype=torch.float32)
    else:
        inst, det = out
        for t, nm in ((inst, 'out[0]'), (det, 'out[1]')):
            _chk(t, nm)
            assert tuple(t.shape) == (N, 1, S, S)
    sig_ct = 0
    if sig_out is not None:
        _chk(sig_out, 'sig_out')
        assert sig_out.shape[0] == N and sig_out.shape[2:] == x.shape[2:]
        sig_ct = sig_out.shape[1]
    check(lib().dm_stage_head_fwd(_p(sem), B, Cs, H, W, _p(rois), N, S, spatial_scale, _p(sampled), _p(x), C, _p(w_inst), _p(b_inst),
                                  _p(w_det), _p(b_det), nc, _p(labels), _p(inst), _p(det), _p(sig_out), sig_ct, sig_ch_offset,
                                  _stream()), 'dm_stage_head_fwd')
    return sampled, inst, det


def gumbel_select(logits, U, temperature=0.5):
    _chk(logits, 'logits')
    _chk(U, 'U')
    N, K = logits.shape
    y = torch.empty_like(logits)
    hot = torch.empty_like(logits)
    idx = torch.empty((N,), device=logits.device, dtype=torch.int32)
    check(lib().dm_gumbel_select_fwd(_p(logits), _p(U), N, K, temperature, _p(y), _p(hot), _p(idx), _stream()),
          'dm_gumbel_select_fwd')
    return y, hot, idx


def detail_target(masks, fuse=(0.7, 0.3)):
    """fuse: two host floats, or a device tensor holding them (read by the kernel: no sync)."""
    _chk(masks, 'masks')
    N, S = masks.shape[0], masks.shape[-1]
    out = torch.empty((N, S, S), device=masks.device, dtype=torch.float32)
    if isinstance(fuse, torch.Tensor):
        fd = _chk(fuse.detach().reshape(-1), 'fuse')
        assert fd.numel() == 2
        rc = lib().dm_detail_target(_p(masks), N, S, 0.0, 0.0, _p(fd), _p(out), _stream())
    else:
        rc = lib().dm_detail_target(_p(masks), N, S, float(fuse[0]), float(fuse[1]), None, _p(out), _stream())
    check(rc, 'dm_detail_target')
    return out


def mask_loss(inst_pred, det_pred, inst_tgt, det_tgt, weight, need_grad=True):
    """Returns (sums[2], per_roi_det[N], grad_inst, grad_det) -- see the header."""
    for t, n in ((inst_pred, 'inst_pred'), (det_pred, 'det_pred'), (inst_tgt, 'inst_tgt'), (det_tgt, 'det_tgt'),
                 (weight, 'weight')):
        _chk(t, n)
    N = inst_pred.shape[0]
    HW = inst_pred.numel() // max(N, 1)
    sums = torch.zeros((2,), device=inst_pred.device, dtype=torch.float32)
    per_roi = torch.zeros((N,), device=inst_pred.device, dtype=torch.float32)
    gi = torch.empty_like(inst_pred) if need_grad else None
    gd = torch.empty_like(det_pred) if need_grad else None
    scratch = torch.empty((max(int(lib().dm_mask_loss_scratch_floats(N)), 1),), device=inst_pred.device, dtype=torch.float32)
    check(lib().dm_mask_loss_fwd_bwd(_p(inst_pred), _p(det_pred), _p(inst_tgt), _p(det_tgt), _p(weight), N, HW,
                                     _p(sums), _p(per_roi), _p(gi), _p(gd), _p(scratch), _stream()), 'dm_mask_loss_fwd_bwd')
    return sums, per_roi, gi, gd


def mask_loss_stage(inst_pred, det_pred, inst_tgt, det_tgt, mask_labels, stage, detail_weight, loss_terms, grad_ml,
                    want_inst_grad):
    """dm_mask_loss_stage: one stage of DynaCrossEntropyLoss, normalisers applied in the kernel.  ``loss_terms`` [2]
    and ``grad_ml`` [N, K] are accumulated into / written in place; returns (grad_inst | None, grad_det)."""
    for t, n in ((inst_pred, 'inst_pred'), (det_pred, 'det_pred'), (inst_tgt, 'inst_tgt'), (det_tgt, 'det_tgt'),
                 (mask_labels, 'mask_labels'), (loss_terms, 'loss_terms'), (grad_ml, 'grad_ml')):
        _chk(t, n)
    N, K = mask_labels.shape
    HW = inst_pred.numel() // max(N, 1)
    gi = torch.empty_like(inst_pred) if want_inst_grad else None
    gd = torch.empty_like(det_pred)
    scratch = torch.empty((max(int(lib().dm_mask_loss_scratch_floats(N)), 1),), device=inst_pred.device, dtype=torch.float32)
    check(lib().dm_mask_loss_stage(_p(inst_pred), _p(det_pred), _p(inst_tgt), _p(det_tgt), _p(mask_labels), K, int(stage), N,
                                   HW, float(detail_weight), _p(loss_terms), _p(grad_ml), _p(gi), _p(gd), _p(scratch),
                                   _stream()), 'dm_mask_loss_stage')
    return gi, gd


def gumbel_select_backward(y_soft, grad_y, temperature=0.5):
    _chk(y_soft, 'y_soft')
    _chk(grad_y, 'grad_y')
    N, K = y_soft.shape
    g = torch.empty_like(y_soft)
    check(lib().dm_gumbel_select_bwd(_p(y_soft), _p(grad_y), N, K, temperature, _p(g), _stream()),
          'dm_gumbel_select_bwd')
    return g


def class_balance(mask_labels):
    """(cb loss scalar tensor, d cb / d mask_labels)."""
    _chk(mask_labels, 'mask_labels')
    N, K = mask_labels.shape
    loss = torch.empty((1,), device=mask_labels.device, dtype=torch.float32)
    grad = torch.empty_like(mask_labels)
    check(lib().dm_class_balance_fwd_bwd(_p(mask_labels), N, K, _p(loss), _p(grad), _stream()),
          'dm_class_balance_fwd_bwd')
    return loss[0], grad


_BN_SCRATCH = {}


def _bn_scratch(device, C):
    """Partial-sum scratch of the split BatchNorm kernels, one buffer per (device, stream): no
    allocation on the step path (kernels that share it are ordered by their stream)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    need = lib().dm_bn_scratch_floats(C)
    buf = _BN_SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty((max(need, 1 << 15),), device=device, dtype=torch.float32)
        _BN_SCRATCH[key] = buf
    return buf


def bn_stats(x, running_mean=None, running_var=None, momentum=0.1, mean_shift=None):
    """``mean_shift`` [C]: the running mean moves towards mean + mean_shift (x lacks a per-channel bias, see the header)."""
    _chk(x, 'x')
    if mean_shift is not None:
        _chk(mean_shift, 'mean_shift')
    NB, C, H, W = x.shape
    mean = torch.empty((C,), device=x.device, dtype=torch.float32)
    var = torch.empty((C,), device=x.device, dtype=torch.float32)
    scratch = _bn_scratch(x.device, C)
    check(lib().dm_bn_stats(_p(x), NB, C, H * W, _p(mean), _p(var), _p(running_mean), _p(running_var), momentum,
                            _p(mean_shift), _p(scratch), _stream()), 'dm_bn_stats')
    return mean, var


def bn_relu_maxpool(x, mean, var, gamma, beta, eps=1e-5):
    for t, n in ((x, 'x'), (mean, 'mean'), (var, 'var'), (gamma, 'gamma'), (beta, 'beta')):
        _chk(t, n)
    NB, C, H, W = x.shape
    out = torch.empty((NB, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=x.device, dtype=torch.float32)
    check(lib().dm_bn_relu_maxpool_fwd(_p(x), NB, C, H, W, _p(mean), _p(var), _p(gamma), _p(beta), eps, _p(out),
                                       _stream()), 'dm_bn_relu_maxpool_fwd')
    return out


def bn_relu_maxpool_argmax(x, mean, var, gamma, beta, eps=1e-5):
    """Plane index of the tap each pooled output took (diagnostic; = max_pool2d(return_indices=True))."""
    for t, n in ((x, 'x'), (mean, 'mean'), (var, 'var'), (gamma, 'gamma'), (beta, 'beta')):
        _chk(t, n)
    NB, C, H, W = x.shape
    arg = torch.empty((NB, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=x.device, dtype=torch.int32)
    check(lib().dm_bn_relu_maxpool_argmax(_p(x), NB, C, H, W, _p(mean), _p(var), _p(gamma), _p(beta), eps, _p(arg),
                                          _stream()), 'dm_bn_relu_maxpool_argmax')
    return arg


MASK_PRE_OPS = ('stats', 'fwd', 'bwd')           # dm_mask_pre_plan's `op` (DM_MASK_PRE_*): bn_stats, bn_relu_maxpool, its backward
MASK_PRE_KERNELS = ('stats', 'stats_split', 'stats_finalize', 'fwd', 'fwd_rows', 'pool_scatter', 'pool_lds', 'pool_sums', 'bn_bwd',
                    'bn_bwd_split')               # field 'kernel' of a plan record
MASK_PRE_PLAN_FIELDS = ('kernel', 'P0', 'P1', 'P2', 'grid_x', 'grid_y', 'threads', 'lds_bytes', 'clear')
# every (kernel, P0, P1, P2) the three route functions can name, by op (include/dynamask_hip.h, dm_mask_pre_plan):
# stats_split (PASS, VEC), pool_sums (EVEN: 2 x 2 blocks or the element form, PRE: prefetch or not), bn_bwd_split (PASS)
MASK_PRE_BUILDS = {
    'stats': {(0, 0, 0, 0), (2, 0, 0, 0)} | {(1, p, vec, 0) for p in (0, 1) for vec in (0, 1)},
    'fwd': {(3, 0, 0, 0), (4, 0, 0, 0)},
    'bwd': {(5, 0, 0, 0), (6, 0, 0, 0), (8, 0, 0, 0), (9, 0, 0, 0), (9, 1, 0, 0)} | {(7, even, pre, 0) for even in (0, 1) for pre in (0, 1)},
}


def mask_pre_plan_raw(op, NB, C, H, W, scratch, align, cus=0):
    """dm_mask_pre_plan: (return code, records) for ``op`` (an index into MASK_PRE_OPS).  The code is the number of launches or
    the (negative) error the call with these numbers would return.  ``cus`` 0: the current device's count.  Host only."""
    consts = _abi.load()[1]
    n, cap = consts['DM_MASK_PRE_PLAN_INTS'], consts['DM_MASK_PRE_PLAN_MAX_LAUNCHES']
    assert len(MASK_PRE_PLAN_FIELDS) == n
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    rc = lib().dm_mask_pre_plan(int(op), int(NB), int(C), int(H), int(W), int(scratch), int(align), int(cus), rec, cap)
    return rc, [dict(zip(MASK_PRE_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def mask_pre_plan(op, NB, C, H, W, scratch=True, aligned=True, cus=0):
    """The launches ``bn_stats`` ('stats'), ``bn_relu_maxpool`` ('fwd') or ``bn_relu_maxpool_backward`` ('bwd') would make for
    an [NB, C, H, W] input, as the launcher's own route says (include/dynamask_hip.h, dm_mask_pre_plan): a list of dicts with
    the keys MASK_PRE_PLAN_FIELDS.  ``scratch``: the call brings one (this module's always do).  ``aligned``: True for
    16-byte aligned tensors (a fresh torch allocation), False for a float's 4 bytes (a view one float into a buffer), or the
    bytes themselves (16, 8, 4).  ``cus``: route for that many compute units instead of the device's.  Raises where the call
    would fail."""
    align = (16 if aligned else 4) if isinstance(aligned, bool) else aligned
    rc, recs = mask_pre_plan_raw(MASK_PRE_OPS.index(op), NB, C, H, W, 1 if scratch else 0, align, cus)
    if rc < 0:
        check(rc, 'dm_mask_pre_plan')
    return recs


# ------------------------------------------------------------------- backward ops
def relu_backward_(grad, out):
    _chk(grad, 'grad')
    _chk(out, 'out')
    assert grad.numel() == out.numel()
    check(lib().dm_relu_bwd(_p(grad), _p(out), grad.numel(), _stream()), 'dm_relu_bwd')
    return grad


def sigmoid_backward(sig, ga, gb, g_logit=None):
    """sig / ga / gb: [N, 1, H, W] views (possibly channel slices); returns / accumulates
    d/dlogit = (ga + gb) * sig * (1 - sig)."""
    N, _, H, W = sig.shape
    for t in (sig, ga) + ((gb,) if gb is not None else ()):
        assert t.is_cuda and t.dtype == torch.float32 and t.shape[1] == 1 and t.stride(3) == 1 and t.stride(2) == W
    acc = g_logit is not None
    if g_logit is None:
        g_logit = torch.empty((N, 1, H, W), device=sig.device, dtype=torch.float32)
    check(lib().dm_sigmoid_bwd(_p(sig), sig.stride(0), _p(ga), ga.stride(0), _p(gb), gb.stride(0) if gb is not None else 0,
                               N, H * W, _p(g_logit), 1 if acc else 0, _stream()), 'dm_sigmoid_bwd')
    return g_logit


def channel_sum(g, out=None):
    g = _chk_src(g)
    NB, C, H, W = g.shape
    acc = out is not None
    if out is None:
        out = torch.empty((C,), device=g.device, dtype=torch.float32)
    if DETERMINISTIC[0]:
        fx = _fx_like(out)
        check(lib().dm_channel_sum_fx(_p(g), g.stride(0), NB, C, H * W, _p(fx), _stream()), 'dm_channel_sum_fx')
        return _fx_finish(fx, out, acc)
    check(lib().dm_channel_sum(_p(g), g.stride(0), NB, C, H * W, _p(out), 1 if acc else 0, _stream()), 'dm_channel_sum')
    return out


CLB_SLAB = [True]      # class-logit parameter gradients without contended atomics (False: per-RoI float atomics)
WGRAD_SLAB = [True]    # weight gradients by slab reduce (no atomics); False: float atomics
_WGRAD_SCRATCH = [0]


def _wgrad_scratch_floats():
    if not _WGRAD_SCRATCH[0]:
        _WGRAD_SCRATCH[0] = int(lib().dm_conv2d_wgrad_scratch_floats())
    return _WGRAD_SCRATCH[0]


def conv2d_wgrad(dy, srcs, ksize, dw=None, db=None, want_bias=False):
    """dW [Cout, sum(Cs), k, k] of conv(cat(srcs)) given dy [NB, Cout, H, W].  ``db`` ([Cout], accumulated into) or
    ``want_bias`` (a fresh tensor): the bias gradient from the same pass over dy; returns dW, or (dW, db) with a bias."""
    dy = _chk_src(dy)
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    srcs = [_chk_src(s) for s in srcs]
    NB, Cout, H, W = dy.shape
    cin = sum(s.shape[1] for s in srcs)
    det = DETERMINISTIC[0]
    if dw is None:
        dw = (torch.empty if det else torch.zeros)((Cout, cin, ksize, ksize), device=dy.device, dtype=torch.float32)
        acc = False
    else:
        _chk(dw, 'dw')
        assert dw.shape == (Cout, cin, ksize, ksize)
        acc = True
    bias_acc = db is not None
    if db is None and want_bias:
        db = (torch.empty if det else torch.zeros)((Cout,), device=dy.device, dtype=torch.float32)
    if db is not None:
        _chk(db, 'db')
        assert db.shape == (Cout,)
    # the accumulation, chosen once: split-K partial tiles into slabs, added in a fixed order (no atomics, the same bits every
    # run in either mode); else 64-bit fixed point (deterministic) or float atomics
    mode = 'slab' if WGRAD_SLAB[0] else ('fx' if det else 'atomics')
    ldw, taps = cin * ksize * ksize, ksize * ksize
    scratch, nfl = None, 0
    if mode == 'slab':
        nfl = _wgrad_scratch_floats()
        scratch = torch.empty((nfl,), device=dy.device, dtype=torch.float32)      # from the calling stream's pool
        # a source whose slabs the scratch cannot hold would add with float atomics (dm_conv2d_wgrad_slab does not refuse it):
        # where the same bits are promised, the launcher's own route is asked, and such a call takes the fixed-point form
        def takes_slabs(i, s):
            first = conv2d_wgrad_plan(NB, Cout, s.shape[1], H, W, ksize, has_bias=db is not None and i == 0, scratch_floats=nfl,
                                      dy_bs=dy.stride(0), x_bs=s.stride(0), io_aligned8=(dy.data_ptr() | s.data_ptr()) % 8 == 0,
                                      scratch_aligned16=scratch.data_ptr() % 16 == 0)[0]
            return first['accum'] == WGRAD_MODES.index('slab')
        if det and not all(takes_slabs(i, s) for i, s in enumerate(srcs)):
            mode, scratch = 'fx', None
    if mode == 'slab' and det:
        if not acc:
            dw.zero_()
        if db is not None and not bias_acc:
            db.zero_()
    fx = _fx_like(dw) if mode == 'fx' else None
    bfx = _fx_like(db) if mode == 'fx' and db is not None else None
    name = {'slab': 'dm_conv2d_wgrad_slab', 'fx': 'dm_conv2d_wgrad_fx', 'atomics': 'dm_conv2d_wgrad'}[mode]
    base = 0
    for i, s in enumerate(srcs):
        bias_ptr = (bfx if mode == 'fx' else db) if i == 0 else None
        tail = (_p(scratch), nfl, _stream()) if mode == 'slab' else (_stream(),)
        check(getattr(lib(), name)(_p(dy), dy.stride(0), Cout, _p(s), s.stride(0), s.shape[1], NB, H, W, ksize,
                                   _p(fx if mode == 'fx' else dw), ldw, base * taps, _p(bias_ptr), *tail), name)
        base += s.shape[1]
    if mode == 'fx':
        _fx_finish(fx, dw, acc)
        if db is not None:
            _fx_finish(bfx, db, bias_acc)
    return (dw, db) if db is not None else dw


WGRAD_PLAN_FIELDS = ('kernel', 'P0', 'P1', 'P2', 'P3', 'P4', 'grid', 'threads', 'lds_bytes', 'MT', 'JT', 'splits', 'per_split',
                     'slabs', 'slab_ld', 'slab_rows', 'slab_stride', 'accum')
WGRAD_KERNELS = ('gemm', 'narrow', 'reduce')              # field 'kernel' of a plan record
WGRAD_MODES = ('atomics', 'slab', 'fx')                   # dm_conv2d_wgrad_plan's `mode`, and field 'accum' of a record


def conv2d_wgrad_plan_raw(dy_bs, cout, x_bs, cs, NB, H, W, ksize, has_bias=0, mode=0, scratch_floats=0, io_aligned8=1,
                          scratch_aligned16=1):
    """dm_conv2d_wgrad_plan: (return code, records).  The code is the number of launches or the (negative) error the call
    with these arguments would return.  Host only: no tensor, no device."""
    consts = _abi.load()[1]
    n, cap = consts['DM_WGRAD_PLAN_INTS'], consts['DM_WGRAD_PLAN_MAX_LAUNCHES']
    assert len(WGRAD_PLAN_FIELDS) == n
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    rc = lib().dm_conv2d_wgrad_plan(int(dy_bs), int(cout), int(x_bs), int(cs), int(NB), int(H), int(W), int(ksize), int(has_bias),
                                    int(mode), int(scratch_floats), int(io_aligned8), int(scratch_aligned16), rec, cap)
    return rc, [dict(zip(WGRAD_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def conv2d_wgrad_plan(NB, cout, cs, H, W, ksize, mode='slab', has_bias=False, scratch_floats=None, dy_bs=None, x_bs=None,
                      io_aligned8=True, scratch_aligned16=True):
    """The launches the weight gradient of one source of ``cs`` channels would make for this shape, as the launcher's own
    route says (include/dynamask_hip.h, dm_conv2d_wgrad_plan): a list of one or two dicts with the keys WGRAD_PLAN_FIELDS
    (two: the slab reduce follows).  ``mode``: one of WGRAD_MODES; 'slab' with ``scratch_floats`` None: the scratch
    ``conv2d_wgrad`` brings.  A 'slab' call whose first record says ``accum`` 0 adds with float atomics.  Batch strides:
    those of contiguous tensors unless given.  Raises where the call would fail."""
    if scratch_floats is None:
        scratch_floats = _wgrad_scratch_floats() if mode == 'slab' else 0
    rc, recs = conv2d_wgrad_plan_raw(cout * H * W if dy_bs is None else dy_bs, cout, cs * H * W if x_bs is None else x_bs, cs, NB,
                                     H, W, ksize, has_bias, WGRAD_MODES.index(mode), scratch_floats, io_aligned8, scratch_aligned16)
    if rc < 0:
        check(rc, 'dm_conv2d_wgrad_plan')
    return recs


BWD_OPS = ('im2col', 'coord_grad', 'col2im', 'upsample', 'point_sample', 'class_logits')       # dm_bwd_plan's `op` (DM_BWD_*)
BWD_KERNELS = ('im2col_lds', 'im2col', 'coord_grad_lds', 'coord_grad', 'col2im_lds', 'upsample_lds', 'upsample_gather',
               'upsample_ac_lds', 'upsample_scatter', 'point_sample_gather', 'point_sample_scatter', 'class_logits_wave',
               'class_logits', 'class_logits_reduce')                                         # field 'kernel' of a plan record
BWD_PLAN_FIELDS = ('kernel', 'P0', 'P1', 'P2', 'grid_x', 'grid_y', 'threads', 'lds_bytes', 'clear')
BWD_MODES = WGRAD_MODES          # class logits' `mode`; P2 of a point-sample or class-logit record: the accumulation taken
# every (kernel, P0, P1, P2) the six route functions can name, by op (include/dynamask_hip.h, dm_bwd_plan)
BWD_BUILDS = {
    'im2col': {(0, ct, 0, 0) for ct in (32, 16, 8, 4)} | {(1, 32, 0, 0)},
    'coord_grad': {(2, 4, 2, 512), (2, 2, 2, 1024), (3, 0, 0, 0)},
    'col2im': {(4, ct, 0, 0) for ct in (8, 4, 2, 1)},
    'upsample': {(5, 0, 0, 0), (6, 0, 0, 0), (7, 1024, 0, 0), (7, 256, 0, 0), (8, 0, 0, 0)},
    'point_sample': {(k, 4, 0, acc) for k in (9, 10) for acc in (0, 2)},
    'class_logits': {(11, 4, it, acc) for it in (1, 4) for acc in (0, 1, 2)} | {(12, 0, 0, acc) for acc in (0, 1, 2)} | {(13, 0, 0, 1)},
}


def backward_plan_raw(op, *numbers):
    """dm_bwd_plan: (return code, records) for ``op`` (an index into BWD_OPS) and its numbers, in the header's order.  The code
    is the number of launches or the (negative) error the call with these numbers would return.  Host only."""
    consts = _abi.load()[1]
    n, cap = consts['DM_BWD_PLAN_INTS'], consts['DM_BWD_PLAN_MAX_LAUNCHES']
    assert len(BWD_PLAN_FIELDS) == n
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    nums = (ctypes.c_longlong * len(numbers))(*[int(v) for v in numbers])
    rc = lib().dm_bwd_plan(int(op), nums, len(numbers), rec, cap)
    return rc, [dict(zip(BWD_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def backward_plan(op, *shape, align_corners=False, aligned16=True, mode=None):
    """The launches the matching call of this module would make, as its launcher's own route says (include/dynamask_hip.h,
    dm_bwd_plan): a list of dicts with the keys BWD_PLAN_FIELDS (none: an empty call; two: the class-logit reduce follows).
    ``op`` (one of BWD_OPS) and ``shape``: 'im2col' / 'coord_grad' / 'col2im': NB, C, H, W, deform_groups; 'upsample': NC, H,
    W (and ``align_corners``); 'point_sample': B, C, H, W, N, S; 'class_logits': N, C, HW, num_classes.  ``mode`` (one of
    BWD_MODES; 'point_sample': 'atomics' or 'fx'): None takes what CLB_SLAB and DETERMINISTIC make the call use.  Tensors
    count as contiguous and 16-byte aligned unless ``aligned16`` says otherwise.  Raises where the call would fail."""
    i = BWD_OPS.index(op)
    nums = tuple(shape)
    if op == 'upsample':
        nums += (1 if align_corners else 0,)
    elif op == 'point_sample':
        nums += (1 if (DETERMINISTIC[0] if mode is None else mode == 'fx') else 0,)
    elif op == 'class_logits':
        if mode is None:
            mode = 'slab' if CLB_SLAB[0] and shape[0] > 0 else ('fx' if DETERMINISTIC[0] else 'atomics')
        scratch = int(lib().dm_class_logits_bwd_scratch_floats(shape[0], shape[1])) if mode == 'slab' else 0
        nums += (BWD_MODES.index(mode), 1 if aligned16 else 0, scratch)
    rc, recs = backward_plan_raw(i, *nums)
    if rc < 0:
        check(rc, 'dm_bwd_plan')
    return recs


def upsample2x_backward(grad_out, fwd_out, in_shape, align_corners=False):
    _chk(grad_out, 'grad_out')
    if fwd_out is not None:
        _chk(fwd_out, 'fwd_out')
    N, C, H, W = in_shape
    gin = torch.empty(in_shape, device=grad_out.device, dtype=torch.float32)
    check(lib().dm_upsample2x_bilinear_bwd(_p(grad_out), _p(fwd_out), N * C, H, W, 1 if align_corners else 0, _p(gin),
                                           _stream()), 'dm_upsample2x_bilinear_bwd')
    return gin


def point_sample_backward(grad_out, feat_shape, rois, spatial_scale, grad_feat=None):
    _chk(grad_out, 'grad_out')
    _chk(rois, 'rois')
    B, C, H, W = feat_shape
    N, _, S, _ = grad_out.shape
    if DETERMINISTIC[0]:
        acc = grad_feat is not None
        if grad_feat is None:
            grad_feat = torch.empty(feat_shape, device=grad_out.device, dtype=torch.float32)
        fx = _fx_like(grad_feat)
        check(lib().dm_point_sample_bwd_fx(_p(grad_out), B, C, H, W, _p(rois), N, S, spatial_scale, _p(fx), _stream()),
              'dm_point_sample_bwd_fx')
        return _fx_finish(fx, grad_feat, acc)
    if grad_feat is None:
        grad_feat = torch.zeros(feat_shape, device=grad_out.device, dtype=torch.float32)
    check(lib().dm_point_sample_bwd(_p(grad_out), B, C, H, W, _p(rois), N, S, spatial_scale, _p(grad_feat), _stream()),
          'dm_point_sample_bwd')
    return grad_feat


def class_logits_backward(x, w_inst, w_det, labels, g_inst, g_det, grad_x, accumulate_x, gw_inst, gb_inst, gw_det, gb_det):
    for t, n in ((x, 'x'), (w_inst, 'w_inst'), (w_det, 'w_det'), (g_inst, 'g_inst'), (g_det, 'g_det'), (grad_x, 'grad_x'),
                 (gw_inst, 'gw_inst'), (gb_inst, 'gb_inst'), (gw_det, 'gw_det'), (gb_det, 'gb_det')):
        _chk(t, n)
    _chk(labels, 'labels', torch.int64)
    N, C, H, W = x.shape
    nc = w_inst.shape[0]
    if CLB_SLAB[0] and N > 0:
        # per-RoI sums to a scratch, added per class in RoI order by a second launch: no contended atomics (the RoIs of an
        # image share a few classes) and a fixed order of additions -- also what the deterministic mode uses
        scratch = torch.empty((int(lib().dm_class_logits_bwd_scratch_floats(N, C)),), device=x.device, dtype=torch.float32)
        check(lib().dm_class_logits_bwd_slab(_p(x), N, C, H * W, _p(w_inst), _p(w_det), nc, _p(labels), _p(g_inst), _p(g_det),
                                             _p(grad_x), 1 if accumulate_x else 0, _p(gw_inst), _p(gb_inst), _p(gw_det), _p(gb_det),
                                             _p(scratch), scratch.numel(), _stream()), 'dm_class_logits_bwd_slab')
        return grad_x
    if DETERMINISTIC[0]:
        outs = (gw_inst, gb_inst, gw_det, gb_det)
        fxs = [_fx_like(t) for t in outs]
        check(lib().dm_class_logits_bwd_fx(_p(x), N, C, H * W, _p(w_inst), _p(w_det), nc, _p(labels), _p(g_inst), _p(g_det),
                                           _p(grad_x), 1 if accumulate_x else 0, *[_p(f) for f in fxs], _stream()),
              'dm_class_logits_bwd_fx')
        for f, t in zip(fxs, outs):
            _fx_finish(f, t, True)
        return grad_x
    check(lib().dm_class_logits_bwd(_p(x), N, C, H * W, _p(w_inst), _p(w_det), nc, _p(labels), _p(g_inst), _p(g_det),
                                    _p(grad_x), 1 if accumulate_x else 0, _p(gw_inst), _p(gb_inst), _p(gw_det), _p(gb_det),
                                    _stream()), 'dm_class_logits_bwd')
    return grad_x


def deform_im2col(x, offset, deform_groups, out=None):
    _chk(x, 'x')
    _chk(offset, 'offset')
    NB, C, H, W = x.shape
    if out is None:
        col = torch.empty((NB, 9 * C, H, W), device=x.device, dtype=torch.float32)
    else:
        col = out
        _chk(col, 'out')
        assert tuple(col.shape) == (NB, 9 * C, H, W)
    check(lib().dm_deform_im2col(_p(x), _p(offset), NB, C, H, W, deform_groups, _p(col), _stream()), 'dm_deform_im2col')
    return col


def deform_col2im_coord(colgrad, x, offset, deform_groups):
    _chk(colgrad, 'colgrad')
    _chk(x, 'x')
    _chk(offset, 'offset')
    NB, C, H, W = x.shape
    gx = torch.empty_like(x)
    goff = torch.empty_like(offset)
    check(lib().dm_deform_col2im_coord(_p(colgrad), _p(x), _p(offset), NB, C, H, W, deform_groups, _p(gx), _p(goff),
                                       _stream()), 'dm_deform_col2im_coord')
    return gx, goff


def deform_coord_grad(colgrad, x, offset, deform_groups, out=None):
    """Offset gradient of DCNv1 from the column gradient (first half of deform_col2im_coord)."""
    _chk(colgrad, 'colgrad')
    _chk(x, 'x')
    _chk(offset, 'offset')
    NB, C, H, W = x.shape
    goff = torch.empty_like(offset) if out is None else out
    check(lib().dm_deform_coord_grad(_p(colgrad), _p(x), _p(offset), NB, C, H, W, deform_groups, _p(goff), _stream()),
          'dm_deform_coord_grad')
    return goff


def deform_col2im(colgrad, offset, x_shape, deform_groups, out=None):
    """Input gradient of DCNv1 from the column gradient (second half of deform_col2im_coord)."""
    _chk(colgrad, 'colgrad')
    _chk(offset, 'offset')
    NB, C, H, W = x_shape
    gx = torch.empty(x_shape, device=colgrad.device, dtype=torch.float32) if out is None else out
    check(lib().dm_deform_col2im(_p(colgrad), _p(offset), NB, C, H, W, deform_groups, _p(gx), _stream()), 'dm_deform_col2im')
    return gx


def dcn_weight_permute(src, cout, c, to_colmajor, dst=None, accumulate=False):
    _chk(src, 'src')
    if dst is None:
        shape = (9 * c, cout, 1, 1) if to_colmajor else (cout, c, 3, 3)
        dst = torch.empty(shape, device=src.device, dtype=torch.float32)
    check(lib().dm_dcn_weight_permute(_p(src), _p(dst), cout, c, 1 if to_colmajor else 0, 1 if accumulate else 0,
                                      _stream()), 'dm_dcn_weight_permute')
    return dst


def pack_dcn_colgrad_weight(weight):
    """DCN weight [Cout, C, 3, 3] packed for the column-gradient GEMM W^T . dY (a 1x1 conv Cout -> 9C)."""
    cout, c = weight.shape[0], weight.shape[1]
    return pack_conv_weight(dcn_weight_permute(weight.contiguous(), cout, c, True))        # [(tap,ci)][co]


def deform_conv_backward_data(x, offset, weight, grad_out, deform_groups, side=None, w_colgrad=None):
    """(grad_x, grad_offset) of DCNv1 3x3: column gradient = W^T . dY as a 1x1 conv, then the coordinate gradient and
    col2im over it (``w_colgrad``: ``pack_dcn_colgrad_weight(weight)``); ``side``: a second stream -- the coordinate
    gradient (bound by its gathers) then runs there, beside col2im (bound by LDS atomics) on the caller's stream; both
    only read the column gradient.  (Round 4's one-kernel form measured at parity -- both are bound by the LDS scatter --
    and was removed in round 5: docs/HISTORY.md.)"""
    NB, C, H, W = x.shape
    if w_colgrad is None:
        w_colgrad = pack_dcn_colgrad_weight(weight)
    colgrad = conv2d(grad_out, w_colgrad, None, 9 * C, 1)                      # W^T . dY
    if side is None:
        return deform_col2im_coord(colgrad, x, offset, deform_groups)
    main = torch.cuda.current_stream(x.device)
    goff = torch.empty_like(offset)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        deform_coord_grad(colgrad, x, offset, deform_groups, out=goff)
    gx = deform_col2im(colgrad, offset, tuple(x.shape), deform_groups)
    main.wait_stream(side)             # colgrad (main-stream memory) is released after this point
    return gx, goff


def deform_conv_backward_weight(x, offset, grad_out, deform_groups, gw_accum=None, col=None):
    """grad_weight [Cout, C, 3, 3] of DCNv1 3x3 = dY . col^T as a 1x1 weight gradient over the tap-major column
    matrix.  ``gw_accum``: tensor the gradient is ADDED to (then None is returned); ``col``: the column matrix of
    (x, offset) if the forward kept it."""
    NB, C, H, W = x.shape
    cout = grad_out.shape[1]
    if col is None:
        col = deform_im2col(x, offset, deform_groups)
    gw_cm = conv2d_wgrad(grad_out, col, 1)                                     # [co][(tap,ci)]
    del col
    if gw_accum is not None:
        dcn_weight_permute(gw_cm, cout, C, False, dst=gw_accum, accumulate=True)
        return None
    return dcn_weight_permute(gw_cm, cout, C, False)


def deform_conv_backward(x, offset, weight, grad_out, deform_groups, gw_accum=None, col=None):
    """(grad_x, grad_offset, grad_weight) of DCNv1 3x3.  The two GEMMs of the
    reference's backward run as 1x1 convs over the tap-major column matrix."""
    gx, goff = deform_conv_backward_data(x, offset, weight, grad_out, deform_groups)
    gw = deform_conv_backward_weight(x, offset, grad_out, deform_groups, gw_accum=gw_accum, col=col)
    return gx, goff, gw


def bn_relu_maxpool_backward(x, mean, var, gamma, beta, grad_out, eps=1e-5):
    for t, n in ((x, 'x'), (mean, 'mean'), (var, 'var'), (gamma, 'gamma'), (beta, 'beta'), (grad_out, 'grad_out')):
        _chk(t, n)
    NB, C, H, W = x.shape
    gx = torch.empty_like(x)
    gg = torch.empty((C,), device=x.device, dtype=torch.float32)
    gb = torch.empty((C,), device=x.device, dtype=torch.float32)
    scratch = _bn_scratch(x.device, C)
    check(lib().dm_bn_relu_maxpool_bwd(_p(x), NB, C, H, W, _p(mean), _p(var), _p(gamma), _p(beta), eps, _p(grad_out),
                                       _p(gx), _p(gg), _p(gb), _p(scratch), _stream()), 'dm_bn_relu_maxpool_bwd')
    return gx, gg, gb


def sgd_momentum_step_(params_flat, grads_flat, momentum_flat, lr, momentum=0.9, weight_decay=1e-4, grad_scale=1.0,
                       first_step=False):
    for t, n in ((params_flat, 'params'), (grads_flat, 'grads'), (momentum_flat, 'momentum')):
        _chk(t, n)
    check(lib().dm_sgd_momentum_step(_p(params_flat), _p(grads_flat), _p(momentum_flat), params_flat.numel(), lr, momentum,
                                     weight_decay, grad_scale, 1 if first_step else 0, _stream()), 'dm_sgd_momentum_step')
    WEIGHT_EPOCH[0] += 1


# ------------------------------------------------------- callers either side of the path
def mask_target_rois(boxes, gt_inds, max_w, max_h):
    _chk(boxes, 'boxes')
    _chk(gt_inds, 'gt_inds', torch.int64)
    N = boxes.shape[0]
    rois = torch.empty((N, 5), device=boxes.device, dtype=torch.float32)
    check(lib().dm_mask_target_rois(_p(boxes), _p(gt_inds), N, float(max_w), float(max_h), _p(rois), _stream()),
          'dm_mask_target_rois')
    return rois


def pack_polygons(masks, device):
    """``PolygonMasks.masks`` (list over objects of lists of float arrays x0, y0, x1, y1, ...) -> the three device
    arrays of ``polygon_mask_targets``: vertices [V, 2] float64, first vertex of each polygon [P + 1] int32, first
    polygon of each object [G + 1] int32.  One upload per image."""
    import numpy as np
    verts, poly_start, inst_start = [], [0], [0]
    for obj in masks:
        for p in obj:
            p = np.asarray(p, dtype=np.float64).reshape(-1)
            assert p.size % 2 == 0, 'a polygon is a flat (x, y) list'
            verts.append(p.reshape(-1, 2))
            poly_start.append(poly_start[-1] + p.size // 2)
        inst_start.append(len(poly_start) - 1)
    v = np.concatenate(verts, 0) if verts else np.zeros((0, 2), np.float64)
    return (torch.from_numpy(np.ascontiguousarray(v)).to(device), torch.tensor(poly_start, dtype=torch.int32, device=device),
            torch.tensor(inst_start, dtype=torch.int32, device=device))


def polygon_mask_targets(packed, boxes, gt_inds, size):
    """[N, size, size] 0 / 1 targets of the objects ``gt_inds`` in the frames of ``boxes`` (clipped to the image)."""
    verts, poly_start, inst_start = packed
    _chk(verts, 'verts', torch.float64)
    _chk(poly_start, 'poly_start', torch.int32)
    _chk(inst_start, 'inst_start', torch.int32)
    _chk(boxes, 'boxes')
    _chk(gt_inds, 'gt_inds', torch.int64)
    N = boxes.shape[0]
    out = torch.empty((N, size, size), device=boxes.device, dtype=torch.float32)
    check(lib().dm_polygon_mask_targets(_p(verts), _p(poly_start), _p(inst_start), inst_start.numel() - 1, _p(boxes), _p(gt_inds),
                                        N, size, _p(out), _stream()), 'dm_polygon_mask_targets')
    return out


def threshold_ge(x, thr):
    _chk(x, 'x')
    out = torch.empty_like(x)
    check(lib().dm_threshold_ge(_p(x), x.numel(), float(thr), _p(out), _stream()), 'dm_threshold_ge')
    return out


def paste_masks(masks, boxes, img_h, img_w, threshold=0.5, apply_sigmoid=False, out=None):
    """masks [N, 1, h, w] or [N, h, w], boxes [N, 4] -> bool [N, img_h, img_w].
    ``out``: optional contiguous uint8 [N, img_h, img_w] slab to paste into (a slice of a
    larger canvas when detections are pasted bucket by bucket).
    A NaN coordinate samples nothing: the value is 0 and the bit is ``0 >= threshold``.  (A zero-width box with a pixel
    centre exactly on it gives 0 / 0.)"""
    _chk(masks, 'masks')
    _chk(boxes, 'boxes')
    N = masks.shape[0]
    _chk_mask_count(N, 'paste_masks')
    mh, mw = masks.shape[-2:]
    if out is None:
        out = torch.empty((N, img_h, img_w), device=masks.device, dtype=torch.uint8)
    else:
        _chk(out, 'out', torch.uint8)
        assert tuple(out.shape) == (N, img_h, img_w)
    check(lib().dm_paste_masks(_p(masks), _p(boxes), N, mh, mw, int(img_h), int(img_w), float(threshold),
                               1 if apply_sigmoid else 0, _p(out), _stream()), 'dm_paste_masks')
    return out.view(torch.bool) if N > 0 else out.bool()


# ------------------------------------------------------- RoI sampling + bbox-branch training
def bbox_overlaps(bboxes1, bboxes2, mode='iou', eps=1e-6):
    """core/bbox/iou_calculators/iou2d_calculator.py:37-131 (is_aligned=False) -> [n1, n2]."""
    assert mode in ('iou', 'iof')
    n1, n2 = bboxes1.shape[0], bboxes2.shape[0]
    out = torch.empty((n1, n2), device=bboxes1.device, dtype=torch.float32)
    if n1 * n2 == 0:
        return out
    _chk(bboxes1, 'bboxes1')
    _chk(bboxes2, 'bboxes2')
    check(lib().dm_bbox_overlaps(_p(bboxes1), n1, _p(bboxes2), n2, 1 if mode == 'iof' else 0, float(eps), _p(out),
                                 _stream()), 'dm_bbox_overlaps')
    return out


def ignore_columns_(overlaps, iof, thr, boxes_major=True):
    """max_iou_assigner.py:107-118, in place: overlaps[:, n] = -1 where box n's largest IoF with an ignore region is
    > thr.  ``iof``: [N, I] (boxes vs regions, ``boxes_major``) or [I, N] (regions vs boxes)."""
    _chk(overlaps, 'overlaps')
    _chk(iof, 'iof')
    G, N = overlaps.shape
    I = iof.shape[1] if boxes_major else iof.shape[0]
    assert (iof.shape[0] if boxes_major else iof.shape[1]) == N
    check(lib().dm_ignore_columns(_p(overlaps), G, N, _p(iof), I, 1 if boxes_major else 0, float(thr), _stream()),
          'dm_ignore_columns')
    return overlaps


def max_iou_assign(overlaps, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True, gt_max_assign_all=True,
                   gt_labels=None):
    """max_iou_assigner.py:129-212 for non-empty inputs -> (gt_inds, max_overlaps, labels|None)."""
    _chk(overlaps, 'overlaps')
    k, n = overlaps.shape
    dev = overlaps.device
    lo, hi = (0.0, float(neg_iou_thr)) if isinstance(neg_iou_thr, float) else (float(neg_iou_thr[0]), float(neg_iou_thr[1]))
    gt_inds = torch.empty((n,), device=dev, dtype=torch.int64)
    max_ov = torch.empty((n,), device=dev, dtype=torch.float32)
    labels = None
    if gt_labels is not None:
        _chk(gt_labels, 'gt_labels', torch.int64)
        labels = torch.empty((n,), device=dev, dtype=torch.int64)
    scratch = torch.empty((2 * k,), device=dev, dtype=torch.float32)
    check(lib().dm_max_iou_assign(_p(overlaps), k, n, float(pos_iou_thr), lo, hi, float(min_pos_iou),
                                  1 if match_low_quality else 0, 1 if gt_max_assign_all else 0, _p(gt_labels), _p(scratch),
                                  _p(gt_inds), _p(max_ov), _p(labels), _stream()), 'dm_max_iou_assign')
    return gt_inds, max_ov, labels


def random_sample(gt_inds, bboxes, n_prepended, gt_bboxes, labels, pos_keys, neg_keys, keys_by_class_rank, num, quota_pos,
                  neg_pos_ub=-1.0):
    """dm_random_sample: key-ranked RoI sampling -> dict of [num]-row device buffers + ``counts`` [4] int32
    (positives kept, negatives kept, positive candidates, negative candidates).  No host sync."""
    _chk(gt_inds, 'gt_inds', torch.int64)
    _chk(bboxes, 'bboxes')
    _chk(pos_keys, 'pos_keys')
    _chk(neg_keys, 'neg_keys')
    M = gt_inds.shape[0]
    assert bboxes.shape == (M, 4)
    if not keys_by_class_rank:
        assert pos_keys.numel() >= M and neg_keys.numel() >= M
    G = int(gt_bboxes.shape[0])
    if G:
        _chk(gt_bboxes, 'gt_bboxes')
    if labels is not None:
        _chk(labels, 'labels', torch.int64)
        assert labels.shape[0] == M
    dev = gt_inds.device
    i64 = dict(device=dev, dtype=torch.int64)
    f32 = dict(device=dev, dtype=torch.float32)
    out = dict(pos_inds=torch.empty((num,), **i64), neg_inds=torch.empty((num,), **i64),
               counts=torch.empty((4,), device=dev, dtype=torch.int32),
               pos_bboxes=torch.empty((num, 4), **f32), neg_bboxes=torch.empty((num, 4), **f32),
               pos_gt_bboxes=torch.empty((num, 4), **f32), pos_assigned_gt_inds=torch.empty((num,), **i64),
               pos_gt_labels=torch.empty((num,), **i64) if labels is not None else None,
               pos_is_gt=torch.empty((num,), device=dev, dtype=torch.uint8))
    scratch = torch.empty((3 * M,), device=dev, dtype=torch.int32)
    check(lib().dm_random_sample(_p(gt_inds), _p(bboxes), M, int(n_prepended), _p(gt_bboxes) if G else _p(None), G,
                                 _p(labels), _p(pos_keys), _p(neg_keys), 1 if keys_by_class_rank else 0, int(num),
                                 int(quota_pos), float(neg_pos_ub), _p(scratch), _p(out['pos_inds']), _p(out['neg_inds']),
                                 _p(out['counts']), _p(out['pos_bboxes']), _p(out['neg_bboxes']), _p(out['pos_gt_bboxes']),
                                 _p(out['pos_assigned_gt_inds']), _p(out['pos_gt_labels']), _p(out['pos_is_gt']),
                                 _stream()), 'dm_random_sample')
    return out


def bbox_encode(proposals, gt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """bbox2delta, delta_xywh_bbox_coder.py:74-116."""
    _chk(proposals, 'proposals')
    _chk(gt, 'gt')
    assert proposals.shape == gt.shape
    out = torch.empty_like(proposals)
    check(lib().dm_bbox_encode(_p(proposals), _p(gt), proposals.shape[0], _float_array(means), _float_array(stds), _p(out),
                               _stream()), 'dm_bbox_encode')
    return out


def softmax_ce(cls_score, labels, weight, scale, need_grad=True):
    """-> (loss [1] = scale * sum_i w_i CE_i, acc [1] percent, grad [N, C] or None).  The prediction behind ``acc`` is the
    LOWEST index among a row's maxima: an exact tie at the top counts as correct only for the lowest tied class."""
    _chk(cls_score, 'cls_score')
    _chk(labels, 'labels', torch.int64)
    if weight is not None:
        _chk(weight, 'weight')
    N, C = cls_score.shape
    dev = cls_score.device
    out = torch.empty((2,), device=dev, dtype=torch.float32)
    grad = torch.empty_like(cls_score) if need_grad else None
    scratch = torch.empty((2 * N,), device=dev, dtype=torch.float32)
    check(lib().dm_softmax_ce_fwd_bwd(_p(cls_score), _p(labels), _p(weight), N, C, float(scale), _p(scratch), _p(out[0:1]),
                                      _p(out[1:2]), _p(grad), _stream()), 'dm_softmax_ce_fwd_bwd')
    return out[0], out[1], grad


def l1_loss_pos(bbox_pred, labels, targets, weights, num_classes, scale, need_grad=True):
    """-> (loss [1], grad [N, NB*4] or None); NB = bbox_pred.shape[1] // 4."""
    _chk(bbox_pred, 'bbox_pred')
    _chk(labels, 'labels', torch.int64)
    _chk(targets, 'targets')
    _chk(weights, 'weights')
    N = bbox_pred.shape[0]
    nb = bbox_pred.shape[1] // 4
    dev = bbox_pred.device
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    grad = torch.empty_like(bbox_pred) if need_grad else None
    scratch = torch.empty((N,), device=dev, dtype=torch.float32)
    check(lib().dm_l1_loss_fwd_bwd(_p(bbox_pred), _p(labels), _p(targets), _p(weights), N, nb, int(num_classes), float(scale),
                                   _p(scratch), _p(loss), _p(grad), _stream()), 'dm_l1_loss_fwd_bwd')
    return loss[0], grad


def sumsq(x, out=None):
    """Sum of squares of a flat fp32 buffer (fixed-order) -> device scalar [1]."""
    _chk(x, 'x')
    out = torch.empty((1,), device=x.device, dtype=torch.float32) if out is None else out
    scratch = torch.empty((int(lib().dm_sumsq_scratch_floats()),), device=x.device, dtype=torch.float32)
    check(lib().dm_sumsq(_p(x), x.numel(), _p(scratch), _p(out), _stream()), 'dm_sumsq')
    return out


def clip_scale_(x, sumsq_total, max_norm):
    """x *= min(1, max_norm / (sqrt(sumsq_total) + 1e-6)); the coefficient is taken on the device."""
    _chk(x, 'x')
    _chk(sumsq_total, 'sumsq')
    check(lib().dm_clip_scale(_p(x), x.numel(), _p(sumsq_total), float(max_norm), _stream()), 'dm_clip_scale')
    return x


def scale_(x, factor):
    """x *= factor (x: a contiguous run of fp32, e.g. a slice of a flat gradient buffer)."""
    _chk(x, 'x')
    check(lib().dm_scale(_p(x), x.numel(), float(factor), _stream()), 'dm_scale')
    return x


# ------------------------------------------------------- FCNMaskHead upsample layers: backward
def carafe_backward(x, enc, grad_out, up_kernel=5, group=1, scale=2):
    """-> (grad_x, grad_enc) of ``carafe`` (mask-head shape: scale 2, H*W <= 256)."""
    _chk(x, 'x')
    _chk(enc, 'enc')
    _chk(grad_out, 'grad_out')
    NB, C, H, W = x.shape
    assert grad_out.shape == (NB, C, H * scale, W * scale)
    gx, genc = torch.empty_like(x), torch.empty_like(enc)
    scratch = torch.empty((int(lib().dm_carafe_bwd_scratch_floats(NB, H, W, up_kernel, group)),), device=x.device,
                          dtype=torch.float32)
    check(lib().dm_carafe_bwd(_p(x), _p(enc), _p(grad_out), NB, C, H, W, up_kernel, group, scale, _p(gx), _p(genc),
                              _p(scratch), _stream()), 'dm_carafe_bwd')
    return gx, genc


def upsample2x_nearest(x):
    _chk(x, 'x')
    NB, C, H, W = x.shape
    out = torch.empty((NB, C, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    check(lib().dm_upsample2x_nearest_fwd(_p(x), NB * C, H, W, _p(out), _stream()), 'dm_upsample2x_nearest_fwd')
    return out


def upsample2x_nearest_backward(grad_out):
    _chk(grad_out, 'grad_out')
    NB, C, OH, OW = grad_out.shape
    gin = torch.empty((NB, C, OH // 2, OW // 2), device=grad_out.device, dtype=torch.float32)
    check(lib().dm_upsample2x_nearest_bwd(_p(grad_out), NB * C, OH // 2, OW // 2, _p(gin), _stream()),
          'dm_upsample2x_nearest_bwd')
    return gin


def pixel_unshuffle2x(x):
    """[N, C, 2H, 2W] -> [N, 4C, H, W] with channel (dy*2+dx)*C + c."""
    _chk(x, 'x')
    NB, C, OH, OW = x.shape
    out = torch.empty((NB, 4 * C, OH // 2, OW // 2), device=x.device, dtype=torch.float32)
    check(lib().dm_pixel_unshuffle2x(_p(x), NB, C, OH // 2, OW // 2, _p(out), _stream()), 'dm_pixel_unshuffle2x')
    return out


# ------------------------------------------------------------ Cascade Mask R-CNN (section K25 of the header)
# CascadeRoIHead: the three stages' FCNMaskHeads as one launch per layer (conv2d_group / deconv2x2_group / conv1x1_group);
# False: the three stage chains one after the other (the A/B baseline; the same bits when the K split is off)
CASCADE_GROUPED = [os.environ.get('DM_CASCADE_GROUPED', '1') != '0']


def conv2d_group_splits(count, NB, H, W, cin, cout, ksize, workspace_floats):
    """The K-split count ``conv2d_group`` takes with a workspace of ``workspace_floats`` (1: none)."""
    return int(lib().dm_conv2d_group_splits(int(count), int(NB), int(H), int(W), int(cin), int(cout), int(ksize),
                                            int(workspace_floats)))


def conv2d_group_plan_raw(count, NB, H, W, cin, cout, ksize, flags=0, workspace_floats=0):
    """dm_conv2d_group_plan: (return code, records).  The code is the number of records (one per problem of the one launch)
    or the (negative) error the dm_conv2d_group_fwd call with these arguments would return.  Host only."""
    consts = _abi.load()[1]
    n, cap = consts['DM_CONV_PLAN_INTS'], consts['DM_CONV_GROUP_PLAN_MAX']
    rec = (ctypes.c_int * (n * cap))(*([-1] * (n * cap)))
    rc = lib().dm_conv2d_group_plan(int(count), int(NB), int(H), int(W), int(cin), int(cout), int(ksize), int(flags),
                                    int(workspace_floats), rec, cap)
    return rc, [dict(zip(CONV_PLAN_FIELDS, rec[i * n:(i + 1) * n])) for i in range(max(rc, 0))]


def conv2d_group_plan(count, NB, H, W, cin, cout, ksize, relu=False, workspace_floats=0):
    """The launch ``conv2d_group`` would make for ``count`` problems of this shape, as the launcher reports it: one dict
    per problem with the keys CONV_PLAN_FIELDS (``grid_x``: the problem's share of the grid; the split is shared).
    Raises where the call would fail."""
    rc, recs = conv2d_group_plan_raw(count, NB, H, W, cin, cout, ksize, 1 if relu else 0, workspace_floats)
    if rc < 0:
        check(rc, 'dm_conv2d_group_plan')
    return recs


def conv2d_group(xs, w_packeds, biases, cout, ksize, relu=False, outs=None, split=None):
    """1 to 3 independent single-source "same" convolutions of one shape (+ bias, + ReLU) as ONE launch
    (dm_conv2d_group_fwd); several ``xs`` may be one tensor.  ``split`` (default: CONV_SPLITK): a 3x3 launch of few
    workgroups may split its K loop, with the split count decided on the grouped launch.  Exact fp32 only: weights
    packed in the bf16x3 layout raise.  Per problem the bits of ``conv2d`` (no split) or of dm_conv2d_fwd_ws with the
    same split count (``conv2d_group_splits``)."""
    k = len(xs)
    if not 1 <= k <= 3 or len(w_packeds) != k or len(biases) != k:
        raise ValueError(f'conv2d_group: 1 to 3 problems with a weight and a bias each (got {k}, {len(w_packeds)}, {len(biases)})')
    if ksize not in (1, 3):
        raise ValueError(f'conv2d_group: ksize 1 or 3 (got {ksize})')
    for x in xs:
        _chk(x, 'x')
        if x.dim() != 4 or tuple(x.shape) != tuple(xs[0].shape):
            raise ValueError('conv2d_group: every problem needs an input of the same [NB, Cin, H, W] shape')
    NB, cin, H, W = xs[0].shape
    for w in w_packeds:
        _chk(w, 'w_packed')
        if conv_layout(w) != 'fp32':
            raise ValueError('conv2d_group: the grouped launch is exact fp32 (weights packed in the bf16x3 layout)')
        if w.numel() != packed_floats(cout, ksize, [cin]):
            raise ValueError('conv2d_group: weights packed for another shape')
    if outs is None:
        outs = [torch.empty((NB, cout, H, W), device=xs[0].device, dtype=torch.float32) for _ in range(k)]
    for o in outs:
        _chk(o, 'out')
        assert tuple(o.shape) == (NB, cout, H, W)
    bias_arr = (ctypes.c_void_p * k)(*[0 if b is None else _chk(b, 'bias').data_ptr() for b in biases])
    if hazard.ENABLED[0]:
        hazard.note_ptr_array(bias_arr, [b for b in biases if b is not None])
    ws, nws = None, 0
    if (CONV_SPLITK[0] if split is None else split) and NB > 0:
        nws = int(lib().dm_conv2d_group_splitk_floats(k, NB, H, W, cin, cout, ksize))
        if nws > 0:
            ws = torch.empty((nws,), device=xs[0].device, dtype=torch.float32)
    check(lib().dm_conv2d_group_fwd(k, _ptr_array(xs), NB, H, W, cin, cout, ksize, _ptr_array(w_packeds), bias_arr,
                                    1 if relu else 0, _ptr_array(outs), _p(ws), nws, _stream()), 'dm_conv2d_group_fwd')
    return outs


def deconv2x2_group(xs, w_packeds, biases, cout, relu=False):
    """1 to 3 ``deconv2x2`` problems of one shape as ONE launch (dm_deconv2x2_group_fwd): the bits of ``deconv2x2`` each.
    Exact fp32 only."""
    k = len(xs)
    if not 1 <= k <= 3 or len(w_packeds) != k or len(biases) != k:
        raise ValueError(f'deconv2x2_group: 1 to 3 problems with a weight and a bias each (got {k})')
    for x in xs:
        _chk(x, 'x')
        if x.dim() != 4 or tuple(x.shape) != tuple(xs[0].shape):
            raise ValueError('deconv2x2_group: every problem needs an input of the same [NB, C, H, W] shape')
    NB, C, H, W = xs[0].shape
    for w in w_packeds:
        _chk(w, 'w_packed')
        if conv_layout(w) != 'fp32':
            raise ValueError('deconv2x2_group: the grouped launch is exact fp32 (weights packed in the bf16x3 layout)')
        if w.numel() != packed_floats(4 * cout, 1, [C]):
            raise ValueError('deconv2x2_group: weights packed for another shape')
    outs = [torch.empty((NB, cout, 2 * H, 2 * W), device=xs[0].device, dtype=torch.float32) for _ in range(k)]
    bias_arr = (ctypes.c_void_p * k)(*[0 if b is None else _chk(b, 'bias').data_ptr() for b in biases])
    if hazard.ENABLED[0]:
        hazard.note_ptr_array(bias_arr, [b for b in biases if b is not None])
    check(lib().dm_deconv2x2_group_fwd(k, _ptr_array(xs), NB, C, H, W, _ptr_array(w_packeds), bias_arr, cout,
                                       1 if relu else 0, _ptr_array(outs), _stream()), 'dm_deconv2x2_group_fwd')
    return outs


def image_shape_table(img_metas, device):
    """The per-image clip table of ``cascade_refine``: float32 [B, 2] = (img_shape h, w) of each meta, uploaded without
    a host wait."""
    return _upload([[float(m['img_shape'][0]), float(m['img_shape'][1])] for m in img_metas], torch.float32, device)


def cascade_refine(rois, cls_score, bbox_pred, num_classes, img_tab, score_sum, first, class_agnostic=True,
                   means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), wh_ratio_clip=16 / 1000, regress=True):
    """One cascade stage boundary in one launch (dm_cascade_refine): ``score_sum`` += ``cls_score`` (``first``: starts
    from 0, i.e. python's ``sum``), and -- ``regress`` -- the next stage's RoIs [n, 5]: ``regress_by_class`` of ``rois``
    [n, 5] by the first argmax of ``cls_score[:, :-1]``, decoded with ``means`` / ``stds`` and clipped to
    ``img_tab[rois[:, 0]]`` (``image_shape_table``).  Returns the new RoIs (None without ``regress``)."""
    _chk(cls_score, 'cls_score')
    n = cls_score.shape[0]
    if cls_score.shape != (n, num_classes + 1):
        raise ValueError(f'cls_score: [{n}, {num_classes + 1}] expected, got {list(cls_score.shape)}')
    if score_sum is not None:
        _chk(score_sum, 'score_sum')
        if score_sum.shape != cls_score.shape:
            raise ValueError('score_sum: the shape of cls_score expected')
    out = None
    if regress:
        _chk(rois, 'rois')
        _chk(bbox_pred, 'bbox_pred')
        _chk(img_tab, 'img_tab')
        if rois.shape != (n, 5):
            raise ValueError(f'rois: [{n}, 5] expected')
        if bbox_pred.shape != (n, 4 if class_agnostic else 4 * num_classes):
            raise ValueError(f'bbox_pred: [{n}, {4 if class_agnostic else 4 * num_classes}] expected')
        if img_tab.dim() != 2 or img_tab.shape[1] != 2 or img_tab.shape[0] < 1:
            raise ValueError('img_tab: [B, 2] expected')
        out = torch.empty((n, 5), device=rois.device, dtype=torch.float32)
    elif score_sum is None:
        raise ValueError('cascade_refine: nothing to do (no score sum, no regression)')
    if n == 0:
        return out
    check(lib().dm_cascade_refine(_p(rois if regress else None), _p(cls_score), _p(bbox_pred if regress else None), n,
                                  int(num_classes), 1 if class_agnostic else 0, _float_array(means), _float_array(stds),
                                  float(wh_ratio_clip), _p(img_tab if regress else None),
                                  int(img_tab.shape[0]) if regress else 0, _p(score_sum), 1 if first else 0, _p(out),
                                  _stream()), 'dm_cascade_refine')
    return out


# ------------------------------------------------------------------ Hybrid Task Cascade (dynamask_hip.h section K26)
def resize_coords(n_in, n_out):
    """The taps of ``resize_bilinear`` along one axis, on the host in fp32 as the kernel computes them: (low index,
    high index, weight of the high tap) per output -- ``F.interpolate(align_corners=True)``'s rule, source coordinate
    ``dst * (in - 1) / (out - 1)`` and 0 when ``out == 1``."""
    import numpy as np
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    lo = np.minimum(src.astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (src - lo.astype(np.float32)).astype(np.float32)


def resize_bilinear(x, size, out=None):
    """``F.interpolate(x, size=size, mode='bilinear', align_corners=True)`` of [N, C, H, W], up or down."""
    _chk(x, 'x')
    N, C, H, W = x.shape
    OH, OW = int(size[0]), int(size[1])
    if OH < 1 or OW < 1:
        raise ValueError(f'resize_bilinear: size {size}')
    if out is None:
        out = torch.empty((N, C, OH, OW), device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (N, C, OH, OW)
    check(lib().dm_resize_bilinear_fwd(_p(x), N * C, H, W, OH, OW, _p(out), _stream()), 'dm_resize_bilinear_fwd')
    return out


def conv1x1_post_add(srcs, w_packed, bias, cout, addend, relu=True, out=None):
    """``out = addend + act(conv1x1(cat(srcs)) + bias)``: the addend joins after the activation (``conv2d``'s
    ``accumulate`` adds in front of it).  ``out`` defaults to a new tensor; it may be ``addend`` (in place).  Exact fp32
    whatever the inference precision: the bits of ``conv2d(relu)`` followed by an fp32 add."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    srcs = [_chk_src(s) for s in srcs]
    _chk(w_packed, 'w_packed')
    _chk(addend, 'addend')
    if bias is not None:
        _chk(bias, 'bias')
    NB, _, H, W = srcs[0].shape
    for s in srcs:
        assert s.shape[0] == NB and s.shape[2] == H and s.shape[3] == W
    if conv_layout(w_packed) != 'fp32':
        raise ValueError('conv1x1_post_add: exact fp32 only (weights packed for bf16x3)')
    assert w_packed.numel() == packed_floats(cout, 1, [s.shape[1] for s in srcs]), 'weights packed for other sources'
    if tuple(addend.shape) != (NB, cout, H, W):
        raise ValueError(f'addend: {[NB, cout, H, W]} expected, got {list(addend.shape)}')
    if out is None:
        out = torch.empty_like(addend)
    else:
        _chk(out, 'out')
        assert out.shape == addend.shape
    strides = (ctypes.c_longlong * len(srcs))(*[int(s.stride(0)) for s in srcs])
    check(lib().dm_conv2d_post_add_fwd(_ptr_array(srcs), _int_array([s.shape[1] for s in srcs]), strides, len(srcs), NB, H,
                                       W, _p(w_packed), _p(bias), cout, 1, 1 if relu else 0, _p(addend), _p(out), cout, 0,
                                       _stream()), 'dm_conv2d_post_add_fwd')
    return out


# ------------------------------------------------------------------ FPN neck (dynamask_hip.h section K31)
def conv2d_up_add(srcs, w_packed, bias, cout, addend, iy, ix, relu=False, out=None):
    """``out[n, c, y, x] = addend[n, c, iy[y], ix[x]] + act(conv1x1(cat(srcs)) + bias)`` (dm_conv2d_up_add_fwd): FPN's
    top-down merge inside the lateral convolution.  ``addend`` [NB, cout, Hs, Ws]; ``iy`` [H] / ``ix`` [W]: device int32
    tables with values in [0, Hs) / [0, Ws) (``necks.nearest_index``; the values are not checked).  Exact fp32 whatever the
    inference precision: the bits of ``conv2d(ksize=1)`` followed by an fp32 add of the gathered addend."""
    if isinstance(srcs, torch.Tensor):
        srcs = [srcs]
    srcs = [_chk_src(s) for s in srcs]
    _chk(w_packed, 'w_packed')
    _chk(addend, 'addend')
    _chk(iy, 'iy', torch.int32)
    _chk(ix, 'ix', torch.int32)
    if bias is not None:
        _chk(bias, 'bias')
    NB, _, H, W = srcs[0].shape
    for s in srcs:
        assert s.shape[0] == NB and s.shape[2] == H and s.shape[3] == W
    if conv_layout(w_packed) != 'fp32':
        raise ValueError('conv2d_up_add: exact fp32 only (weights packed for bf16x3)')
    assert w_packed.numel() == packed_floats(cout, 1, [s.shape[1] for s in srcs]), 'weights packed for other sources'
    if addend.dim() != 4 or tuple(addend.shape[:2]) != (NB, cout) or addend.shape[2] < 1 or addend.shape[3] < 1:
        raise ValueError(f'addend: [{NB}, {cout}, Hs, Ws] expected, got {list(addend.shape)}')
    if tuple(iy.shape) != (H,) or tuple(ix.shape) != (W,):
        raise ValueError(f'iy [{H}] and ix [{W}] expected, got {list(iy.shape)} and {list(ix.shape)}')
    if out is None:
        out = torch.empty((NB, cout, H, W), device=srcs[0].device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (NB, cout, H, W)
        if out.data_ptr() == addend.data_ptr():
            raise ValueError('conv2d_up_add: out may not be the addend')
    strides = (ctypes.c_longlong * len(srcs))(*[int(s.stride(0)) for s in srcs])
    check(lib().dm_conv2d_up_add_fwd(_ptr_array(srcs), _int_array([s.shape[1] for s in srcs]), strides, len(srcs), NB, H, W,
                                     _p(w_packed), _p(bias), cout, 1, 1 if relu else 0, _p(addend), addend.shape[2],
                                     addend.shape[3], _p(iy), _p(ix), _p(out), cout, 0, _stream()), 'dm_conv2d_up_add_fwd')
    return out


def subsample2(x, out=None):
    """``x[:, :, ::2, ::2]`` as a dense tensor = ``F.max_pool2d(x, 1, stride=2)`` (dm_subsample2_fwd)."""
    _chk(x, 'x')
    N, C, H, W = x.shape
    if H < 1 or W < 1:
        raise ValueError(f'subsample2: an empty map {list(x.shape)}')
    shape = (N, C, (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_subsample2_fwd(_p(x), N * C, H, W, _p(out), _stream()), 'dm_subsample2_fwd')
    return out


def roi_align_pool(size, out_size):
    """The pooling that joins ``size`` x ``size`` RoIAlign bins to ``out_size`` x ``out_size`` features in
    ``roi_align_add_``: 1 (identity) or 2 (the exact 2 x 2 mean = ``adaptive_avg_pool2d`` size -> size / 2)."""
    if size == out_size:
        return 1
    if size == 2 * out_size:
        return 2
    raise NotImplementedError(f'semantic RoI features of {size} x {size} join RoI features of {out_size} x {out_size} only '
                              'by the identity or the 2 x 2 mean (adaptive_avg_pool2d with other windows: no kernel)')


def roi_align_add_(feats, fmap, rois, size, spatial_scale, sampling_ratio=0):
    """``feats += pool(RoIAlign_size(fmap, rois))`` in place, one launch: ``fmap`` [B, C, H, W] (one level, no level
    mapping), ``rois`` [N, 5], ``feats`` [N, C, size, size] (identity) or [N, C, size / 2, size / 2] (2 x 2 mean)."""
    _chk(feats, 'feats')
    _chk(fmap, 'fmap')
    _chk(rois, 'rois')
    B, C, H, W = fmap.shape
    N = rois.shape[0]
    if feats.dim() != 4 or feats.shape[0] != N or feats.shape[1] != C or feats.shape[2] != feats.shape[3]:
        raise ValueError(f'feats: [{N}, {C}, s, s] expected, got {list(feats.shape)}')
    pool = roi_align_pool(int(size), int(feats.shape[2]))
    if N == 0:
        return feats
    check(lib().dm_roi_align_add_fwd(_p(fmap), B, C, H, W, float(spatial_scale), _p(rois), N, int(size), int(sampling_ratio),
                                     pool, _p(feats), _stream()), 'dm_roi_align_add_fwd')
    return feats


# ------------------------------------------------ Grid R-CNN: the GridHead launches (csrc/grid_head.hip)
# Exact fp32 in every precision mode: the bf16x3 mode does not reach these launches.
# Groups of at least this many floats run the wide build of dm_group_norm_fwd (1024 threads, 16-byte loads) unless
# DM_GN_WIDE=0; the library's constant of the same name (csrc/grid_head.hip) decides, this copy is for tools and tests
# (tests/test_fcos_cpu.py holds the two equal).
GN_WIDE_MIN_L = 16385


def group_norm_supported(x, num_groups):
    N, C, H, W = x.shape
    return bool(lib().dm_group_norm_supported(N, C, int(num_groups), H, W))


def group_norm(x, weight, bias, num_groups, eps=1e-5, relu=False, out=None):
    """GroupNorm(num_groups, C, eps)(x) (+ ReLU) of x [N, C, H, W] with per-channel ``weight`` / ``bias`` [C]
    (dm_group_norm_fwd; biased variance, two-pass statistics).  ``out`` may be ``x`` itself: in place."""
    _chk(x, 'x')
    _chk(weight, 'weight')
    _chk(bias, 'bias')
    if x.dim() != 4:
        raise ValueError(f'x: [N, C, H, W] expected, got {list(x.shape)}')
    N, C, H, W = x.shape
    assert weight.shape == (C,) and bias.shape == (C,)
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, 'out')
        assert out.shape == x.shape
    check(lib().dm_group_norm_fwd(_p(x), N, C, int(num_groups), H, W, _p(weight), _p(bias), float(eps), 1 if relu else 0,
                                  _p(out), _stream()), 'dm_group_norm_fwd')
    return out


def grid_neighbors(grid_points):
    """grid_head.py:88-102: per point (= column * grid_size + row) its neighbours in the order left, up, down, right."""
    gs = int(round(grid_points ** 0.5))
    assert gs * gs == grid_points
    out = []
    for i in range(gs):
        for j in range(gs):
            nb = []
            if i > 0:
                nb.append((i - 1) * gs + j)
            if j > 0:
                nb.append(i * gs + j - 1)
            if j < gs - 1:
                nb.append(i * gs + j + 1)
            if i < gs - 1:
                nb.append((i + 1) * gs + j)
            out.append(tuple(nb))
    return out


def grid_fusion_supported(x, grid_points):
    N, C, H, W = x.shape
    return H == W and C % grid_points == 0 and bool(lib().dm_grid_fusion_supported(N, int(grid_points), C // grid_points, H))


def pack_grid_fusion_table(trans, grid_points, channels):
    """The weight table of one fusion order (dm_grid_fusion_fwd): ``trans[i][j]`` = (dw weight [c, 1, 5, 5], dw bias [c],
    1x1 weight [c, c, 1, 1], 1x1 bias [c]) of point i's j-th neighbour -> [P][4][25 c + c + c c + c] floats, the 1x1
    weight transposed to [k][o]; the slots a point has no neighbour for stay zero."""
    P, c = int(grid_points), int(channels)
    total = int(lib().dm_grid_fusion_table_floats(P, c))
    if total < 0:
        raise NotImplementedError(f'grid fusion: no kernel for {P} points of {c} channels')
    E = total // (4 * P)
    dev = trans[0][0][0].device
    table = torch.zeros((P, 4, E), device=dev, dtype=torch.float32)
    for i, slots in enumerate(trans):
        assert len(slots) <= 4
        for j, (dw_w, dw_b, w1, b1) in enumerate(slots):
            assert dw_w.shape == (c, 1, 5, 5) and dw_b.shape == (c,) and w1.shape == (c, c, 1, 1) and b1.shape == (c,)
            table[i, j] = torch.cat([dw_w.detach().reshape(-1), dw_b.detach(), w1.detach().reshape(c, c).t().reshape(-1),
                                     b1.detach()])
    return table.reshape(-1)


def grid_fusion(x, src, table, grid_points, out=None):
    """One order of GridHead's neighbour fusion in one launch (dm_grid_fusion_fwd): per point i,
    ``x_i + sum_j trans_ij(src_{neighbour j of i})`` -> [N, P c, S, S].  ``src`` is ``x`` (first order) or the first
    order's result (second order); ``out`` may be neither."""
    _chk(x, 'x')
    _chk(src, 'src')
    _chk(table, 'table')
    N, C, H, W = x.shape
    P = int(grid_points)
    assert src.shape == x.shape and H == W and C % P == 0
    assert table.numel() == int(lib().dm_grid_fusion_table_floats(P, C // P)), 'table packed for another shape'
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, 'out')
        assert out.shape == x.shape
    check(lib().dm_grid_fusion_fwd(_p(x), _p(src), N, P, C // P, H, _p(table), _p(out), _stream()), 'dm_grid_fusion_fwd')
    return out


def deconv4x4_s2_grouped_supported(x, cout, groups):
    N, C, H, W = x.shape
    g = int(groups)
    return H == W and C % g == 0 and cout % g == 0 and bool(
        lib().dm_deconv4x4_s2_grouped_supported(N, g, C // g, int(cout) // g, H))


def deconv4x4_s2_grouped(x, weight, bias, groups, out=None):
    """ConvTranspose2d(C, cout, 4, stride=2, padding=1, groups=groups)(x) (dm_deconv4x4_s2_grouped_fwd): ``weight``
    [C, cout / groups, 4, 4] in torch's layout (no packing), ``bias`` [cout] or None -> [N, cout, 2 S, 2 S]."""
    _chk(x, 'x')
    _chk(weight, 'weight')
    if bias is not None:
        _chk(bias, 'bias')
    N, C, H, W = x.shape
    g = int(groups)
    assert H == W and C % g == 0 and weight.dim() == 4 and weight.shape[0] == C and tuple(weight.shape[2:]) == (4, 4)
    co = int(weight.shape[1])
    assert bias is None or bias.shape == (g * co,)
    shape = (N, g * co, 2 * H, 2 * W)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_deconv4x4_s2_grouped_fwd(_p(x), N, g, C // g, co, H, _p(weight), _p(bias), _p(out), _stream()),
          'dm_deconv4x4_s2_grouped_fwd')
    return out


def grid_get_bboxes(heat, det_bboxes, sub_regions, out=None, return_cells=False):
    """GridHead.get_bboxes on the device (dm_grid_get_bboxes): ``heat`` [n, P, HS, HS] logits, ``det_bboxes`` [n, D >= 5]
    (score last), ``sub_regions`` the P (x1, y1, x2, y2) of calc_sub_regions -> [n, 5], NOT clipped to the image.
    ``return_cells``: also the cell of each point's maximum within its map, int32 [n, P]."""
    _chk(heat, 'heat')
    _chk(det_bboxes, 'det_bboxes')
    n, P, HS, HS2 = heat.shape
    assert HS == HS2 and det_bboxes.dim() == 2 and det_bboxes.shape[0] == n and len(sub_regions) == P
    if out is None:
        out = torch.empty((n, 5), device=heat.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (n, 5)
    cells = torch.empty((n, P), device=heat.device, dtype=torch.int32) if return_cells else None
    check(lib().dm_grid_get_bboxes(_p(heat), n, P, HS, _p(det_bboxes), det_bboxes.shape[1],
                                   _int_array([r[0] for r in sub_regions]), _int_array([r[1] for r in sub_regions]),
                                   _p(out), _p(cells), _stream()), 'dm_grid_get_bboxes')
    return (out, cells) if return_cells else out


# ------------------------------------------------ Double-Head R-CNN (section K28 of the header)
def global_avg_pool_supported(x):
    N, C, H, W = x.shape
    return bool(lib().dm_global_avg_pool_supported(N, C, H * W))


def global_avg_pool(x, out=None):
    """x [N, C, H, W] -> [N, C], the mean of every plane (dm_global_avg_pool_fwd): ``nn.AvgPool2d(H)`` on an H x H map,
    flattened.  The summation order is fixed by H * W alone: a sample's bits do not depend on the rest of the batch."""
    _chk(x, 'x')
    if x.dim() != 4:
        raise ValueError(f'x: [N, C, H, W] expected, got {list(x.shape)}')
    N, C, H, W = x.shape
    if C < 1 or H * W < 1:
        raise ValueError(f'x: an empty plane has no mean, got {list(x.shape)}')
    if out is None:
        out = torch.empty((N, C), device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert out.shape == (N, C)
    check(lib().dm_global_avg_pool_fwd(_p(x), N, C, H * W, _p(out), _stream()), 'dm_global_avg_pool_fwd')
    return out


# ------------------------------------------------ RPN post-processing (section K30 of the header, csrc/rpn.hip)
RPN_SEG_WORDS = _abi.load()[1]['DM_RPN_SEG_WORDS']
RPN_SELECT_CHUNK = _abi.load()[1]['DM_RPN_SELECT_CHUNK']


def rpn_select_supported(num_segments, max_candidates, total_candidates=None):
    total = max_candidates if total_candidates is None else total_candidates
    return bool(lib().dm_rpn_select_supported(int(num_segments), int(max_candidates), int(total)))


def rpn_decode_supported(num_segments, max_rows, num_images=1):
    return bool(lib().dm_rpn_decode_supported(int(num_segments), int(max_rows), int(num_images)))


def rpn_merge_supported(num_images, num_levels, max_rows, nms_post):
    return bool(lib().dm_rpn_merge_supported(int(num_images), int(num_levels), int(max_rows), int(nms_post)))


def _chk_seg_map(t, name, channels=None):
    """One segment's map: a dense [C, H, W] fp32 block on the device (it may be one image of a wider NCHW tensor)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError(f'{name}: a [C, H, W] float32 tensor on the device expected')
    C, H, W = t.shape
    if t.numel() and (t.stride(2) != 1 or t.stride(1) != W or t.stride(0) != H * W):
        raise ValueError(f'{name}: the [C, H, W] block must be dense')
    if channels is not None and C != channels:
        raise ValueError(f'{name}: {channels} channels expected, got {C}')
    return t


class RPNSegments:
    """The segment table of the RPN entry points: segment s = image * num_levels + level reads ``logits[s]`` [A, H, W]
    (and ``deltas[s]`` [4 A, H, W] for ``rpn_decode``).  ``nms_pre`` <= 0 keeps every candidate.  ``strides[s]`` =
    (stride_x, stride_y), ``base_rows[s]`` = the level's first row of the base-anchor table, ``images[s]`` = its image.
    Host lists: ``sizes`` (A H W), ``rows`` (K), ``row0``; ``tab`` is the device table (uploaded without a host wait).
    The tensors are kept alive here: the table holds their addresses."""

    def __init__(self, logits, nms_pre, deltas=None, strides=None, base_rows=None, images=None, num_levels=None):
        S = len(logits)
        self.logits = [_chk_seg_map(t, 'logits') for t in logits]
        self.deltas = None if deltas is None else [_chk_seg_map(d, 'deltas', 4 * t.shape[0]) for d, t in zip(deltas, logits)]
        if deltas is not None and (len(deltas) != S or any(d.shape[1:] != t.shape[1:] for d, t in zip(deltas, logits))):
            raise ValueError('deltas: one [4 A, H, W] map per segment expected')
        self.nms_pre = int(nms_pre)
        self.num_levels = int(num_levels) if num_levels is not None else max(S, 1)
        self.sizes = [int(t.numel()) for t in self.logits]
        self.rows = [min(self.nms_pre, n) if self.nms_pre > 0 else n for n in self.sizes]
        self.row0, self.key_off = [], []
        r = k = 0
        for n, m in zip(self.sizes, self.rows):
            self.row0.append(r)
            self.key_off.append(k)
            r += m
            k += n
        self.total_rows, self.total_candidates = r, k
        self.max_candidates = max(self.sizes, default=0)
        self.max_rows = max(self.rows, default=0)
        tab = []
        for s, t in enumerate(self.logits):
            A, H, W = t.shape
            sx, sy = strides[s] if strides is not None else (0, 0)
            tab.append([t.data_ptr(), self.deltas[s].data_ptr() if self.deltas is not None else 0, A, H, W, self.rows[s],
                        self.key_off[s], self.row0[s], int(base_rows[s]) if base_rows is not None else 0, int(sx), int(sy),
                        int(images[s]) if images is not None else s // self.num_levels])
        self.device = self.logits[0].device if S else None
        self.tab = _upload(tab, torch.int64, self.device) if S else None

    def __len__(self):
        return len(self.logits)


def rpn_select(segs):
    """Per segment, its ``rows`` candidates of largest ``sigmoid(logit)`` in descending order, the lower candidate
    index first among equal scores (dm_rpn_select): (idx int32 [total rows], score [total rows]); segment s at
    ``row0[s] : row0[s] + rows[s]``.  Candidate i = (h * W + w) * A + a."""
    S = len(segs)
    dev = segs.device if S else 'cuda'
    idx = torch.empty((segs.total_rows,), device=dev, dtype=torch.int32)
    score = torch.empty((segs.total_rows,), device=dev, dtype=torch.float32)
    if S == 0 or segs.total_candidates == 0:
        return idx, score
    nbytes = int(lib().dm_rpn_select_workspace_bytes(S, segs.max_candidates, segs.total_candidates, segs.total_rows))
    if nbytes < 0:
        check(-3, 'dm_rpn_select')
    ws = torch.empty(((nbytes + 7) // 8,), device=dev, dtype=torch.int64)
    check(lib().dm_rpn_select(_p(segs.tab), S, segs.max_candidates, segs.total_candidates, segs.total_rows, segs.nms_pre,
                              _p(ws), ws.numel() * 8, _p(idx), _p(score), _stream()), 'dm_rpn_select')
    return idx, score


def rpn_decode(segs, idx, base_anchors, img_tab, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), wh_ratio_clip=16 / 1000):
    """The boxes [total rows, 4] of the candidates ``idx`` (``rpn_select``'s): anchor = ``base_anchors[base_row + a]`` +
    the grid shift, decoded by its four deltas and clipped to ``img_tab[image]`` (``image_shape_table``): the bits of
    ``bbox_decode`` on the materialised anchors (dm_rpn_decode)."""
    if segs.deltas is None:
        raise ValueError('rpn_decode: the segments carry no deltas')
    _chk(idx, 'idx', torch.int32)
    _chk(base_anchors, 'base_anchors')
    _chk(img_tab, 'img_tab')
    if idx.shape != (segs.total_rows,):
        raise ValueError(f'idx: [{segs.total_rows}] expected')
    if base_anchors.dim() != 2 or base_anchors.shape[1] != 4:
        raise ValueError('base_anchors: [R, 4] expected')
    if img_tab.dim() != 2 or img_tab.shape[1] != 2 or img_tab.shape[0] < 1:
        raise ValueError('img_tab: [B, 2] expected')
    boxes = torch.empty((segs.total_rows, 4), device=idx.device, dtype=torch.float32)
    if len(segs) == 0 or segs.total_rows == 0:
        return boxes
    check(lib().dm_rpn_decode(_p(segs.tab), len(segs), segs.max_rows, _p(idx), _p(base_anchors), _p(img_tab),
                              int(img_tab.shape[0]), _float_array(means), _float_array(stds), float(wh_ratio_clip),
                              _p(boxes), _stream()), 'dm_rpn_decode')
    return boxes


def rpn_merge(segs, keep, kept, boxes, score, nms_post):
    """Per image, the first ``nms_post`` kept rows of its levels in descending score order (equal scores: the lower
    level, then the earlier rank): (out [B, nms_post, 5] = (box, score), counts int32 [B]); rows past ``counts[b]`` are
    not written (dm_rpn_merge).  ``keep`` / ``kept`` as ``nms_segmented`` returns them for ``segs.rows``."""
    S, L = len(segs), segs.num_levels
    if S % L:
        raise ValueError(f'rpn_merge: {S} segments are no multiple of {L} levels')
    B = S // L
    _chk(keep, 'keep', torch.int32)
    _chk(kept, 'kept', torch.int32)
    _chk(boxes, 'boxes')
    _chk(score, 'score')
    if kept.shape != (S,) or keep.shape != (segs.total_rows,) or boxes.shape != (segs.total_rows, 4) or \
            score.shape != (segs.total_rows,):
        raise ValueError('rpn_merge: keep / boxes / score of the segments\' rows and one kept count per segment expected')
    out = torch.empty((B, int(nms_post), 5), device=kept.device, dtype=torch.float32)
    counts = torch.empty((B,), device=kept.device, dtype=torch.int32)
    if B == 0:
        return out, counts
    check(lib().dm_rpn_merge(_p(segs.tab), B, L, segs.max_rows, _p(keep), _p(kept), _p(boxes), _p(score), int(nms_post),
                             _p(out), _p(counts), _stream()), 'dm_rpn_merge')
    return out, counts


# ------------------------------------------------------------------ ResNet stem (dynamask_hip.h section K32)
# Exact fp32 in every precision mode: the bf16x3 mode does not reach these launches.
def pack_conv7x7_weight(w):
    """[cout, C, 7, 7] -> the operand of ``conv7x7_s2``: the matrix [cout, C * 7 * 8] (a zero eighth column behind every
    kernel row, so a row is a pair of channel quads) in ``pack_conv_weight``'s 1x1 layout."""
    _chk(w, 'weight')
    if w.dim() != 4 or tuple(w.shape[2:]) != (7, 7):
        raise ValueError(f'pack_conv7x7_weight: a [cout, C, 7, 7] weight expected, got {list(w.shape)}')
    cout, C = w.shape[:2]
    wide = torch.zeros((cout, C, 7, 8), device=w.device, dtype=torch.float32)
    wide[..., :7] = w
    return pack_conv_weight(wide.view(cout, C * 56, 1, 1))


def conv7x7_s2_supported(x, cout):
    """Does ``conv7x7_s2`` take this input (dm_conv7x7_s2_supported: 3 channels, any H, W, any cout)?  ``x``: a tensor
    or its shape."""
    NB, C, H, W = x.shape if isinstance(x, torch.Tensor) else x
    return bool(lib().dm_conv7x7_s2_supported(int(NB), int(C), int(H), int(W), int(cout)))


def conv7x7_s2(x, w_packed, bias, cout, relu=False, out=None):
    """Conv2d(3, cout, 7, stride=2, padding=3)(x) + bias (+ ReLU) -> [NB, cout, ceil(H / 2), ceil(W / 2)]
    (dm_conv7x7_s2_fwd).  ``w_packed``: ``pack_conv7x7_weight`` of the [cout, 3, 7, 7] weight."""
    _chk(x, 'x')
    _chk(w_packed, 'w_packed')
    if bias is not None:
        _chk(bias, 'bias')
    NB, C, H, W = x.shape
    flags = (1 if relu else 0) | (16 if conv_layout(w_packed) == 'bf16x3' else 0)
    if not flags & 16:
        assert w_packed.numel() == packed_floats(cout, 1, [C * 56]), 'weights packed for another shape'
    shape = (NB, int(cout), (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_conv7x7_s2_fwd(_p(x), NB, C, H, W, _p(w_packed), _p(bias), int(cout), flags, _p(out), _stream()),
          'dm_conv7x7_s2_fwd')
    return out


def maxpool3x3_s2(x, out=None):
    """``F.max_pool2d(x, 3, stride=2, padding=1)`` (dm_maxpool3x3_s2_fwd), NaN and -inf as torch treats them."""
    _chk(x, 'x')
    N, C, H, W = x.shape
    if H < 1 or W < 1:
        raise ValueError(f'maxpool3x3_s2: an empty map {list(x.shape)}')
    shape = (N, C, (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_maxpool3x3_s2_fwd(_p(x), N * C, H, W, _p(out), _stream()), 'dm_maxpool3x3_s2_fwd')
    return out


# ------------------------------------------------------------------ ResNeXt's grouped 3x3 (dynamask_hip.h section K34)
# Exact fp32 in every precision mode, like the stem.
def pack_grouped_conv_weight(w, groups):
    """[C, C / groups, 3, 3] -> the operand of ``conv3x3_grouped``: [C / T][C / groups][9][T] with T =
    dm_conv3x3_grouped_couts_per_wave(C, groups) neighbouring output channels side by side (dm_conv3x3_grouped_pack's
    layout, made by a permutation on the weight's own device)."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
        raise TypeError('pack_grouped_conv_weight: a float32 tensor expected')
    groups = int(groups)
    if w.dim() != 4 or groups < 1 or w.shape[0] % groups != 0 or tuple(w.shape[1:]) != (w.shape[0] // groups, 3, 3):
        raise ValueError(f'pack_grouped_conv_weight: a [C, C / groups, 3, 3] weight expected at groups={groups}, got {list(w.shape)}')
    C, cg = w.shape[:2]
    T = lib().dm_conv3x3_grouped_couts_per_wave(int(C), groups)
    if T == 0:
        raise NotImplementedError(f'pack_grouped_conv_weight: {cg} channels per group (C={C}, groups={groups}); 4, 8, 16, 32 and 64 are built')
    return w.reshape(C // T, T, cg, 9).permute(0, 2, 3, 1).contiguous().view(-1)


def conv3x3_grouped_supported(x, groups, stride):
    """Does ``conv3x3_grouped`` take this input (dm_conv3x3_grouped_supported: 4 / 8 / 16 / 32 / 64 channels per group,
    stride 1 or 2, any H, W)?  ``x``: a tensor or its shape."""
    NB, C, H, W = x.shape if isinstance(x, torch.Tensor) else x
    return bool(lib().dm_conv3x3_grouped_supported(int(NB), int(C), int(H), int(W), int(groups), int(stride)))


def conv3x3_grouped(x, w_packed, bias, groups, stride=1, relu=False, out=None):
    """Conv2d(C, C, 3, stride, padding=1, groups=groups)(x) + bias (+ ReLU) -> [NB, C, ceil(H / stride), ceil(W / stride)]
    (dm_conv3x3_grouped_fwd).  ``w_packed``: ``pack_grouped_conv_weight`` of the [C, C / groups, 3, 3] weight."""
    _chk(x, 'x')
    _chk(w_packed, 'w_packed')
    if bias is not None:
        _chk(bias, 'bias')
    NB, C, H, W = x.shape
    groups, stride = int(groups), int(stride)
    if stride not in (1, 2):
        raise NotImplementedError(f'conv3x3_grouped: stride={stride}; 1 and 2 are built')
    flags = (1 if relu else 0) | (16 if conv_layout(w_packed) == 'bf16x3' else 0)
    if not flags & 16:
        assert w_packed.numel() == lib().dm_conv3x3_grouped_packed_floats(C, groups), 'weights packed for another shape'
        assert bias is None or bias.numel() == C
    shape = (NB, C, (H + stride - 1) // stride, (W + stride - 1) // stride)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_conv3x3_grouped_fwd(_p(x), NB, C, H, W, _p(w_packed), _p(bias), groups, stride, flags, _p(out), _stream()),
          'dm_conv3x3_grouped_fwd')
    return out


# ------------------------------------------------------------------ Res2Net's kernels (dynamask_hip.h section K35)
# Exact fp32 in every precision mode, like the stem.
def pack_conv_slices_weight(w):
    """Folded weights [G, w, w, 3, 3] of G independent w -> w 3x3 convolutions -> the operand of ``conv3x3_slices``:
    [G][ceil(w / 8)][w][9][8], 8 neighbouring output channels of a slice side by side, zeros for the output channels
    from w on (dm_conv3x3_slices_pack's layout, made by a permutation on the weight's own device)."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
        raise TypeError('pack_conv_slices_weight: a float32 tensor expected')
    if w.dim() != 5 or w.shape[0] < 1 or w.shape[1] < 1 or tuple(w.shape[2:]) != (w.shape[1], 3, 3):
        raise ValueError(f'pack_conv_slices_weight: a [G, w, w, 3, 3] weight expected, got {list(w.shape)}')
    G, c = w.shape[:2]
    T = (c + 7) // 8
    wide = torch.zeros((G, T * 8, c, 9), device=w.device, dtype=torch.float32)
    wide[:, :c] = w.reshape(G, c, c, 9)
    return wide.view(G, T, 8, c, 9).permute(0, 1, 3, 4, 2).contiguous().view(-1)


def conv3x3_slices_supported(x, w, G, stride, out_channels=None, tail=0):
    """Does ``conv3x3_slices`` take this input (dm_conv3x3_slices_supported: any w >= 1, stride 1 or 2, any H, W)?  ``x``:
    a tensor or its shape; ``out_channels``: the channels of ``out`` (default: as many as ``x`` has)."""
    NB, Cx, H, W = x.shape if isinstance(x, torch.Tensor) else x
    Co = Cx if out_channels is None else out_channels
    return bool(lib().dm_conv3x3_slices_supported(int(NB), int(w), int(G), int(H), int(W), int(stride), int(Cx), int(Co), int(tail)))


def conv3x3_slices(x, w_packed, bias, w, G, out, stride=1, relu=False, x_ch0=0, o_ch0=0, addend=None, a_ch0=0, tail=0,
                   tail_x_ch0=0, tail_o_ch0=0):
    """G independent ``Conv2d(w, w, 3, stride, padding=1) + bias (+ ReLU)`` in ONE launch (dm_conv3x3_slices_fwd): slice g
    reads the channels [x_ch0 + g w, + w) of ``x`` [NB, Cx, H, W] -- plus, with ``addend`` [NB, Ca, H, W], its channels
    [a_ch0 + g w, + w): one fp32 add before the products -- and writes the channels [o_ch0 + g w, + w) of ``out``
    [NB, Co, ceil(H / stride), ceil(W / stride)], which is returned; nothing else of ``out`` is written.  ``tail``: 1 copies
    the ``w`` channels at ``tail_x_ch0`` of ``x`` to ``tail_o_ch0`` of ``out`` (stride 1), 2 writes their
    ``AvgPool2d(3, stride, padding=1)`` there (the divisor is always 9), in the same launch.  ``w_packed``:
    ``pack_conv_slices_weight`` of the [G, w, w, 3, 3] weights; ``bias`` [G * w] or None."""
    _chk(x, 'x')
    _chk(w_packed, 'w_packed')
    _chk(out, 'out')
    if bias is not None:
        _chk(bias, 'bias')
    if addend is not None:
        _chk(addend, 'addend')
        assert addend.dim() == 4 and addend.shape[0] == x.shape[0] and tuple(addend.shape[2:]) == tuple(x.shape[2:]), \
            'addend: another batch or map than x'
    NB, Cx, H, W = x.shape
    w, G, stride = int(w), int(G), int(stride)
    if stride not in (1, 2):
        raise NotImplementedError(f'conv3x3_slices: stride={stride}; 1 and 2 are built')
    flags = (1 if relu else 0) | (16 if conv_layout(w_packed) == 'bf16x3' else 0)
    if not flags & 16:
        assert w_packed.numel() == lib().dm_conv3x3_slices_packed_floats(G, w), 'weights packed for another shape'
        assert bias is None or bias.numel() == G * w
    assert out.dim() == 4 and (out.shape[0], out.shape[2], out.shape[3]) == (NB, (H + stride - 1) // stride, (W + stride - 1) // stride), \
        'out: another batch or map than the convolution gives'
    check(lib().dm_conv3x3_slices_fwd(_p(x), Cx, int(x_ch0), _p(addend), addend.shape[1] if addend is not None else 0, int(a_ch0),
                                      NB, w, G, H, W, stride, _p(w_packed), _p(bias), flags, _p(out), out.shape[1], int(o_ch0),
                                      int(tail), int(tail_x_ch0), int(tail_o_ch0), _stream()), 'dm_conv3x3_slices_fwd')
    return out


def avgpool2x2_ceil(x, out=None):
    """``F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)`` (dm_avgpool2x2_ceil_fwd): an edge window of an
    odd map divides by the number of elements it covers."""
    _chk(x, 'x')
    N, C, H, W = x.shape
    if H < 1 or W < 1:
        raise ValueError(f'avgpool2x2_ceil: an empty map {list(x.shape)}')
    shape = (N, C, (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_avgpool2x2_ceil_fwd(_p(x), N * C, H, W, _p(out), _stream()), 'dm_avgpool2x2_ceil_fwd')
    return out


def conv3x3_s2_c3_supported(x, cout):
    """Does ``conv3x3_s2_c3`` take this input (dm_conv3x3_s2_c3_supported: 3 channels, any H, W, any cout)?  ``x``: a
    tensor or its shape."""
    NB, C, H, W = x.shape if isinstance(x, torch.Tensor) else x
    return bool(lib().dm_conv3x3_s2_c3_supported(int(NB), int(C), int(H), int(W), int(cout)))


def conv3x3_s2_c3(x, weight, bias, relu=False, out=None):
    """Conv2d(3, cout, 3, stride=2, padding=1)(x) + bias (+ ReLU) -> [NB, cout, ceil(H / 2), ceil(W / 2)]
    (dm_conv3x3_s2_c3_fwd).  ``weight``: [cout, 3, 3, 3] as torch has it (no packing)."""
    _chk(x, 'x')
    _chk(weight, 'weight')
    if bias is not None:
        _chk(bias, 'bias')
    NB, C, H, W = x.shape
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (C, 3, 3):
        raise ValueError(f'conv3x3_s2_c3: a [cout, {C}, 3, 3] weight expected, got {list(weight.shape)}')
    cout = weight.shape[0]
    assert bias is None or bias.numel() == cout
    flags = (1 if relu else 0) | (16 if conv_layout(weight) == 'bf16x3' else 0)
    shape = (NB, cout, (H + 1) // 2, (W + 1) // 2)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == shape
    check(lib().dm_conv3x3_s2_c3_fwd(_p(x), NB, C, H, W, _p(weight), _p(bias), cout, flags, _p(out), _stream()),
          'dm_conv3x3_s2_c3_fwd')
    return out


# ------------------------------------------------------------------ image pre-processing (dynamask_hip.h section K33)
PREPROCESS_MAX_IMAGES = _abi.load()[1]['DM_PREPROCESS_MAX_IMAGES']
_RESIZE_TABLES = {}        # (n_src, n_dst) -> resize_axis_table's arrays
_RESIZE_TAPS = {}          # (device, ((n_src, n_dst), ...)) -> (taps on the device, {(n_src, n_dst): first row})


def resize_axis_table(n_src, n_dst):
    """The per-axis sample table of ``preprocess_u8`` (dynamask_hip.h K33), cached per (n_src, n_dst): numpy arrays
    (i0 int32, i1 int32, c0 int16, c1 int16) of length n_dst -- the two source indices of every destination index and
    their 11-bit coefficients (c0 + c1 == 2048)."""
    import numpy as np
    n_src, n_dst = int(n_src), int(n_dst)
    if n_src < 1 or n_dst < 1:
        raise ValueError(f'resize_axis_table: n_src={n_src}, n_dst={n_dst}; at least 1 each expected')
    key = (n_src, n_dst)
    if key not in _RESIZE_TABLES:
        d = np.arange(n_dst, dtype=np.float64)
        f = ((d + 0.5) * (1.0 / (n_dst / n_src)) - 0.5).astype(np.float32)
        i = np.floor(f)
        t = (f - i).astype(np.float32)
        i = i.astype(np.int64)
        low, high = i < 0, i >= n_src - 1
        i = np.where(low, 0, np.where(high, n_src - 1, i))
        t = np.where(low | high, np.float32(0), t).astype(np.float32)
        c0 = np.rint((np.float32(1) - t).astype(np.float32) * np.float32(2048)).astype(np.int16)
        c1 = np.rint(t * np.float32(2048)).astype(np.int16)
        _RESIZE_TABLES[key] = (i.astype(np.int32), np.minimum(i + 1, n_src - 1).astype(np.int32), c0, c1)
    return _RESIZE_TABLES[key]


def _resize_taps(keys, device):
    """The tap table of one launch: the axis tables of ``keys`` (distinct (n_src, n_dst) pairs) one after the other as
    int32 [rows, 4] on the device, uploaded once per set of keys and kept, with each key's first row."""
    import numpy as np
    ck = (str(device), keys)
    if ck not in _RESIZE_TAPS:
        if len(_RESIZE_TAPS) >= 64:
            _RESIZE_TAPS.clear()
        row0, parts, r = {}, [], 0
        for k in keys:
            i0, i1, c0, c1 = resize_axis_table(*k)
            parts.append(np.stack([i0, i1, c0.astype(np.int32), c1.astype(np.int32)], 1))
            row0[k] = r
            r += k[1]
        taps = torch.from_numpy(np.concatenate(parts)).pin_memory().to(device, non_blocking=True)
        _RESIZE_TAPS[ck] = (taps, row0)
    return _RESIZE_TAPS[ck]


def preprocess_u8(images, sizes, flips, mean, stdinv, to_rgb, pad_shape, out=None):
    """B decoded images -> the batch the backbone reads, in one launch (dm_preprocess_u8_fwd): resize to ``sizes[b]`` =
    (nh, nw) with the 8-bit fixed-point bilinear scheme, flip (``flips[b]``: None / False, 'horizontal' or 'vertical'),
    ``(v - mean[c]) * stdinv[c]`` (``to_rgb``: output channel c reads source channel 2 - c), zero padding right and bottom
    to ``pad_shape`` = (Hp, Wp).  ``images[b]``: uint8 [h, w, 3] on the device, dense pixels, any row stride >= 3 w.
    Returns ``out`` [B, 3, Hp, Wp] float32, every element written."""
    B = len(images)
    if len(sizes) != B or len(flips) != B:
        raise ValueError(f'preprocess_u8: {B} images, {len(sizes)} sizes, {len(flips)} flips')
    if B == 0:
        raise ValueError('preprocess_u8: no image')
    Hp, Wp = int(pad_shape[0]), int(pad_shape[1])
    dims, keys = [], []
    for b, (im, (nh, nw), flip) in enumerate(zip(images, sizes, flips)):
        _chk_u8_image(im, f'images[{b}]')
        h, w = im.shape[:2]
        code = 0 if not flip else AUG_FLIP_CODES.get(flip)
        if code is None:
            raise ValueError(f"images[{b}]: invalid flipping direction '{flip}'")
        for k in ((w, int(nw)), (h, int(nh))):
            if k not in keys and k[1] >= 1:          # (a size below 1 has no table: the library refuses the call below)
                keys.append(k)
        dims.append([h, w, im.stride(0) if h > 1 else 3 * w, int(nh), int(nw), code, (w, int(nw)), (h, int(nh))])
    dev = images[0].device
    taps, row0 = _resize_taps(tuple(keys), dev) if keys else (torch.zeros((0, 4), device=dev, dtype=torch.int32), {})
    flat = []
    for d in dims:
        flat += d[:6] + [row0.get(d[6], 0), row0.get(d[7], 0)]
    dims_arr = _int_array(flat)
    if not lib().dm_preprocess_u8_supported(B, dims_arr, taps.shape[0], Hp, Wp):
        check(_abi.load()[1]['DM_ERR_UNSUPPORTED'], f'dm_preprocess_u8_fwd ({B} images of at most '
              f'{PREPROCESS_MAX_IMAGES}, output {Hp} x {Wp})')
    if out is None:
        out = torch.empty((B, 3, Hp, Wp), device=dev, dtype=torch.float32)
    else:
        _chk(out, 'out')
        assert tuple(out.shape) == (B, 3, Hp, Wp)
    if hazard.ENABLED[0]:
        hazard.touch('dm_preprocess_u8_fwd (image table)', reads=list(images))
    check(lib().dm_preprocess_u8_fwd(_ptr_array(images), dims_arr, B, _p(taps), taps.shape[0], _float_array(mean),
                                     _float_array(stdinv), 1 if to_rgb else 0, _p(out), Hp, Wp, _stream()),
          'dm_preprocess_u8_fwd')
    return out


def _chk_u8_image(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a tensor')
    if not t.is_cuda:
        raise RuntimeError(f'{name}: dynamask_amd operators run on the MI355X only (got a {t.device} tensor); '
                           'there is no CPU fallback')
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise TypeError(f'{name}: a uint8 [h, w, 3] image expected, got {t.dtype} {list(t.shape)}')
    if t.stride(2) != 1 or t.stride(1) != 3 or (t.shape[0] > 1 and t.stride(0) < 3 * t.shape[1]):
        raise ValueError(f'{name}: dense pixels (strides [>= 3 w, 3, 1]) expected, got {list(t.stride())}')
    return t
