// Bbox branch post-processing (the two fully connected layers and the
// two predictors of Shared2FCBBoxHead are plain GEMMs and go to the library):
//   K20  softmax over the class logits + DeltaXYWH decode + clip + rescale
//        (BBoxHead.get_bboxes, roi_heads/bbox_heads/bbox_head.py:186-217;
//         delta2bbox, core/bbox/coder/delta_xywh_bbox_coder.py:165-204)
//   K21  NMS suppression matrix for score-sorted boxes (mmcv.ops.nms, called through
//        batched_nms by multiclass_nms, core/post_processing/bbox_nms.py:5-68) -- the
//        classic 64 x 64 tile bitmask; the greedy pass over the rows is host code
//        (dm_nms_reduce), as in the reference's extension.
#include "bbox_decode.h"

namespace {

struct DecodeArgs {
  const float* rois;      // [N, roi_stride] (x1 at column roi_x0)
  int roi_stride, roi_x0;
  const float* cls_score; // [N, NC + 1] or null
  const float* bbox_pred; // [N, 4 * NB] (NB = NC, or 1 if class agnostic) or null
  int N, NC, NB;
  float mean[4], std[4];
  float max_ratio;
  float clip_w, clip_h;   // <= 0: no clipping
  float inv_sx, inv_sy;   // rescale: boxes / scale_factor (1 if none)
  float* scores;          // [N, NC + 1]
  float* bboxes;          // [N, 4 * NB]
};

__global__ __launch_bounds__(128) void bbox_decode_kernel(DecodeArgs a) {
  __shared__ float red[2];
  const int i = blockIdx.x;
  const int t = threadIdx.x;
  if (a.cls_score) {
    const float* s = a.cls_score + (size_t)i * (a.NC + 1);
    float m = -INFINITY;
    for (int c = t; c <= a.NC; c += 128) m = fmaxf(m, s[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    m = fmaxf(red[0], red[1]);
    __syncthreads();
    float sum = 0.f;
    for (int c = t; c <= a.NC; c += 128) sum += expf(s[c] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((t & 63) == 0) red[t >> 6] = sum;
    __syncthreads();
    sum = red[0] + red[1];
    for (int c = t; c <= a.NC; c += 128) a.scores[(size_t)i * (a.NC + 1) + c] = expf(s[c] - m) / sum;
  }
  const float* r = a.rois + (size_t)i * a.roi_stride + a.roi_x0;
  const float rx1 = r[0], ry1 = r[1], rx2 = r[2], ry2 = r[3];
  for (int c = t; c < a.NB; c += 128) {
    float x1 = rx1, y1 = ry1, x2 = rx2, y2 = ry2;
    if (a.bbox_pred)
      delta2bbox_one(rx1, ry1, rx2, ry2, a.bbox_pred + ((size_t)i * a.NB + c) * 4, a.mean, a.std, a.max_ratio, x1, y1, x2, y2);
    if (a.clip_w > 0.f) clip_box(x1, y1, x2, y2, a.clip_w, a.clip_h);
    float* o = a.bboxes + ((size_t)i * a.NB + c) * 4;
    o[0] = x1 * a.inv_sx;
    o[1] = y1 * a.inv_sy;
    o[2] = x2 * a.inv_sx;
    o[3] = y2 * a.inv_sy;
  }
}

// mask[i][w] bit b set <=> box j = 64*w + b (j > i) overlaps box i by more than thr.
// One 64 x 64 tile (row tile ty, column tile tx >= ty) of the M boxes at `boxes`, written into the
// row-major [M][words] matrix at `mask`; shared by the one-matrix and the segmented launch so that both
// compute the same IoU bits.
__device__ __forceinline__ void nms_mask_tile(const float* __restrict__ boxes, int M, float thr, float off,
                                              unsigned long long* __restrict__ mask, int words, int tx, int ty,
                                              float* cb) {
  const int row0 = ty * 64, col0 = tx * 64;
  const int t = threadIdx.x;
  const int ncol = min(64, M - col0);
  if (t < ncol) {
    cb[t * 4 + 0] = boxes[(size_t)(col0 + t) * 4 + 0];
    cb[t * 4 + 1] = boxes[(size_t)(col0 + t) * 4 + 1];
    cb[t * 4 + 2] = boxes[(size_t)(col0 + t) * 4 + 2];
    cb[t * 4 + 3] = boxes[(size_t)(col0 + t) * 4 + 3];
  }
  __syncthreads();
  const int i = row0 + t;
  if (i >= M) return;
  const float x1 = boxes[(size_t)i * 4 + 0], y1 = boxes[(size_t)i * 4 + 1];
  const float x2 = boxes[(size_t)i * 4 + 2], y2 = boxes[(size_t)i * 4 + 3];
  const float area = (x2 - x1 + off) * (y2 - y1 + off);
  unsigned long long bits = 0;
  const int start = (row0 == col0) ? t + 1 : 0;
  for (int j = start; j < ncol; ++j) {
    const float bx1 = cb[j * 4 + 0], by1 = cb[j * 4 + 1], bx2 = cb[j * 4 + 2], by2 = cb[j * 4 + 3];
    const float w = fmaxf(fminf(x2, bx2) - fmaxf(x1, bx1) + off, 0.f);
    const float h = fmaxf(fminf(y2, by2) - fmaxf(y1, by1) + off, 0.f);
    const float inter = w * h;
    const float barea = (bx2 - bx1 + off) * (by2 - by1 + off);
    const float iou = inter / (area + barea - inter);
    if (iou > thr) bits |= 1ull << j;
  }
  mask[(size_t)i * words + tx] = bits;
}

// grid = (col tiles, row tiles) of 64 boxes; only the upper triangle does work.
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, int M, float thr, float off,
                                                      unsigned long long* __restrict__ mask, int words) {
  __shared__ float cb[64 * 4];
  if (blockIdx.x < blockIdx.y) return;
  nms_mask_tile(boxes, M, thr, off, mask, words, blockIdx.x, blockIdx.y, cb);
}

// Segmented form: segment b = rows [start, start + M) of `boxes` (score-sorted within the segment) and its own
// [M][ceil(M / 64)] matrix at mask + mask_off -- the diagonal blocks of a block-diagonal layout, no cross-segment
// words.  seg_tab[b] = (start, M, mask_off).  grid = (max tiles, max tiles, B); tiles past a segment's own return.
__global__ __launch_bounds__(64) void nms_mask_segmented_kernel(const float* __restrict__ boxes,
                                                                const long long* __restrict__ seg_tab, float thr,
                                                                float off, unsigned long long* __restrict__ mask) {
  __shared__ float cb[64 * 4];
  const long long* sg = seg_tab + (size_t)blockIdx.z * 3;
  const int M = (int)sg[1];
  const int words = (M + 63) >> 6;
  if ((int)blockIdx.x >= words || (int)blockIdx.y >= words || blockIdx.x < blockIdx.y) return;
  nms_mask_tile(boxes + (size_t)sg[0] * 4, M, thr, off, mask + sg[2], words, blockIdx.x, blockIdx.y, cb);
}

// The greedy pass of dm_nms_reduce on the device, one wave per segment (wave64: the 64 bits of a row word are the
// 64 lanes' boxes).  The boxes are walked 64 at a time: the diagonal words of the 64 rows are loaded one per lane,
// the serial keep / suppress decisions of the 64 boxes run on the wave-uniform removed word with one lane shuffle per
// box, then the kept rows are OR-ed into the removed words of the later columns, one word per lane.  Same decisions
// as dm_nms_reduce: a box is kept unless an earlier kept box suppresses it, and the walk stops at max_keep kept boxes.
// keep[start + k] = the k-th kept box (index within the segment's sorted rows), counts[b] = number kept.
__global__ __launch_bounds__(64) void nms_reduce_segmented_kernel(const unsigned long long* __restrict__ mask,
                                                                  const long long* __restrict__ seg_tab, int max_keep,
                                                                  int* __restrict__ keep, int* __restrict__ counts) {
  extern __shared__ unsigned long long removed[];
  const long long* sg = seg_tab + (size_t)blockIdx.x * 3;
  const int M = (int)sg[1];
  const int words = (M + 63) >> 6;
  const unsigned long long* m = mask + sg[2];
  int* kp = keep + sg[0];
  const int lane = threadIdx.x;
  for (int w = lane; w < words; w += 64) removed[w] = 0ull;
  __syncthreads();
  int n = 0;
  bool stop = false;
  for (int c = 0; c < words && !stop; ++c) {
    const int i0 = c * 64;
    const int rows = min(64, M - i0);
    const unsigned long long diag = lane < rows ? m[(size_t)(i0 + lane) * words + c] : 0ull;
    unsigned long long r = removed[c];
    unsigned long long kept = 0ull;
    for (int e = 0; e < rows; ++e) {
      const unsigned long long de = __shfl(diag, e, 64);
      if ((r >> e) & 1ull) continue;
      if (max_keep >= 0 && n >= max_keep) { stop = true; break; }
      if (lane == 0) kp[n] = i0 + e;
      ++n;
      kept |= 1ull << e;
      r |= de;
    }
    if (stop) break;
    for (int w = c + 1 + lane; w < words; w += 64) {
      unsigned long long acc = removed[w];
      unsigned long long k = kept;
      while (k) {
        const int e = __ffsll((long long)k) - 1;
        k &= k - 1;
        acc |= m[(size_t)(i0 + e) * words + w];
      }
      removed[w] = acc;
    }
    __syncthreads();
  }
  if (lane == 0) counts[blockIdx.x] = n;
}

// ----- test-time augmentation (BBoxTestMixin.aug_test_bboxes / MaskTestMixin.aug_test_mask) -----
// View v's parameters: view_tab[v * DM_AUG_VIEW_FLOATS + k], k = 0..3 the scale factor of x1, y1, x2, y2, 4 img_h,
// 5 img_w (of the view), 6 the flip code (DM_AUG_FLIP_*).  Same fp32 operations in the reference's order.

// bbox_mapping: [n, 4] boxes (row stride `stride`) -> out [V][n][5] RoI rows (batch column 0): b * sf, then the flip.
__global__ __launch_bounds__(256) void bbox_mapping_multi_kernel(const float* __restrict__ boxes, int stride, int n, int V,
                                                                 const float* __restrict__ view_tab,
                                                                 float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * V) return;
  const int v = (int)(t / n), i = (int)(t - (long long)v * n);
  const float* vt = view_tab + (size_t)v * DM_AUG_VIEW_FLOATS;
  const float* b = boxes + (size_t)i * stride;
  float x1 = b[0] * vt[0], y1 = b[1] * vt[1], x2 = b[2] * vt[2], y2 = b[3] * vt[3];
  const int flip = (int)vt[6];
  if (flip == DM_AUG_FLIP_HORIZONTAL) {
    const float a = vt[5] - x2, c = vt[5] - x1;
    x1 = a; x2 = c;
  } else if (flip == DM_AUG_FLIP_VERTICAL) {
    const float a = vt[4] - y2, c = vt[4] - y1;
    y1 = a; y2 = c;
  }
  float* o = out + (size_t)t * 5;
  o[0] = 0.f; o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
}

// merge_aug_bboxes: views' [n, C4] boxes (bbox_mapping_back: flip, then / sf) and [n, CS] scores, averaged: the sum in
// view order (starting from view 0's value), then / V.  ptr_tab[v] = (boxes, scores) of view v.  grid = (column
// blocks, n); column j < C4 is a box coordinate, C4 + k the score k.
__global__ __launch_bounds__(256) void merge_aug_bboxes_kernel(const long long* __restrict__ ptr_tab,
                                                               const float* __restrict__ view_tab, int V, int n, int C4,
                                                               int CS, float* __restrict__ out_boxes,
                                                               float* __restrict__ out_scores) {
#pragma clang fp contract(off)
  const int i = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= C4 + CS) return;
  float acc = 0.f;
  if (j < C4) {
    const int kk = j & 3, base = j - kk;
    for (int v = 0; v < V; ++v) {
      const float* vt = view_tab + (size_t)v * DM_AUG_VIEW_FLOATS;
      const float* b = reinterpret_cast<const float*>(ptr_tab[2 * v]) + (size_t)i * C4;
      const int flip = (int)vt[6];
      float x = b[j];
      if (flip == DM_AUG_FLIP_HORIZONTAL && (kk & 1) == 0) x = vt[5] - b[base + (kk ^ 2)];
      else if (flip == DM_AUG_FLIP_VERTICAL && (kk & 1) == 1) x = vt[4] - b[base + (kk ^ 2)];
      x = x / vt[kk];
      acc = v == 0 ? x : acc + x;
    }
    out_boxes[(size_t)i * C4 + j] = acc / (float)V;
  } else {
    const int k = j - C4;
    for (int v = 0; v < V; ++v) {
      const float x = reinterpret_cast<const float*>(ptr_tab[2 * v + 1])[(size_t)i * CS + k];
      acc = v == 0 ? x : acc + x;
    }
    out_scores[(size_t)i * CS + k] = acc / (float)V;
  }
}

// merge_aug_proposals' first half (merge_augs.py:27-38): every (image, view) segment's [n, 5] proposals mapped back to the
// original image (bbox_mapping_back: the flip against the view's img_shape, then a true division by the scale factor)
// and written at the segment's rows of the concatenated [total, 5] buffer, the score copied.  seg_tab[s] = (address of
// the proposals, n, first output row); view_tab[s] = the segment's view row.  grid = (row blocks, S).
__global__ __launch_bounds__(256) void proposals_mapping_back_kernel(const long long* __restrict__ seg_tab,
                                                                     const float* __restrict__ view_tab,
                                                                     float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long* sg = seg_tab + (size_t)blockIdx.y * 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int)sg[1]) return;
  const float* vt = view_tab + (size_t)blockIdx.y * DM_AUG_VIEW_FLOATS;
  const float* b = reinterpret_cast<const float*>(sg[0]) + (size_t)i * 5;
  float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  const int flip = (int)vt[6];
  if (flip == DM_AUG_FLIP_HORIZONTAL) {
    const float p = vt[5] - x2, q = vt[5] - x1;
    x1 = p; x2 = q;
  } else if (flip == DM_AUG_FLIP_VERTICAL) {
    const float p = vt[4] - y2, q = vt[4] - y1;
    y1 = p; y2 = q;
  }
  float* o = out + ((size_t)sg[2] + i) * 5;
  o[0] = x1 / vt[0]; o[1] = y1 / vt[1]; o[2] = x2 / vt[2]; o[3] = y2 / vt[3];
  o[4] = b[4];
}

// ----- Cascade R-CNN stage step (CascadeRoIHead.simple_test, cascade_roi_head.py:307-315) -----
// One wave per RoI row i of stage s:
//   sum[i, :]  = (s == 0 ? 0 : sum[i, :]) + cls[i, :]       (sum(ms_scores): ((0 + s0) + s1) + s2 in fp32)
//   label      = cls[i, :NC].argmax()                        (the first maximum; NaN counts as the maximum, as torch's)
//   out[i, :]  = [rois[i, 0], delta2bbox(rois[i, 1:], pred[i, label | 0]) clipped to img_tab[rois[i, 0]]]
// (regress_by_class, bbox_head.py:306-334).  out == NULL: the score sum only (the last stage).
struct CascadeArgs {
  const float* rois;       // [n, 5]
  const float* cls;        // [n, NC + 1]
  const float* pred;       // [n, 4] (class agnostic) or [n, 4 * NC]
  int n, NC, agnostic;
  float mean[4], std[4];
  float max_ratio;
  const float* img_tab;    // [B, 2] (h, w) per image
  int B;
  float* sum;              // [n, NC + 1] or null
  int first;
  float* out;              // [n, 5] or null
};

__device__ __forceinline__ bool argmax_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(64) void cascade_refine_kernel(CascadeArgs a) {
  const int i = blockIdx.x;
  const int t = threadIdx.x;
  const float* s = a.cls + (size_t)i * (a.NC + 1);
  if (a.sum) {
    float* o = a.sum + (size_t)i * (a.NC + 1);
    for (int c = t; c <= a.NC; c += 64) o[c] = (a.first ? 0.f : o[c]) + s[c];
  }
  if (!a.out) return;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = t; c < a.NC; c += 64) {
    const float v = s[c];
    if (argmax_better(v, c, bv, bi)) { bv = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (t != 0) return;
  const float* r = a.rois + (size_t)i * 5;
  const float b = r[0];
  const float rx1 = r[1], ry1 = r[2], rx2 = r[3], ry2 = r[4];
  const int label = bi < a.NC ? bi : 0;
  const float* d = a.pred + (size_t)i * (a.agnostic ? 4 : 4 * a.NC) + (a.agnostic ? 0 : 4 * label);
  float x1, y1, x2, y2;
  delta2bbox_one(rx1, ry1, rx2, ry2, d, a.mean, a.std, a.max_ratio, x1, y1, x2, y2);
  const int img = min(max((int)b, 0), a.B - 1);
  const float ch = a.img_tab[2 * img], cw = a.img_tab[2 * img + 1];
  if (cw > 0.f) clip_box(x1, y1, x2, y2, cw, ch);
  float* o = a.out + (size_t)i * 5;
  o[0] = b; o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
}

}  // namespace

extern "C" int dm_bbox_decode(const float* rois, int roi_stride, int roi_x0, const float* cls_score,
                              const float* bbox_pred, int N, int num_classes, int class_agnostic, const float* means,
                              const float* stds, float wh_ratio_clip, float clip_h, float clip_w, float scale_x,
                              float scale_y, float* scores, float* bboxes, dm_stream_t stream) {
  if (N < 0 || num_classes <= 0 || roi_stride < 4 || roi_x0 < 0 || roi_x0 + 4 > roi_stride) return DM_ERR_INVALID_ARG;
  if (N == 0) return DM_OK;
  if (!rois || !bboxes || !means || !stds || (cls_score && !scores)) return DM_ERR_INVALID_ARG;
  if (!(wh_ratio_clip > 0.f) || !(scale_x > 0.f) || !(scale_y > 0.f)) return DM_ERR_INVALID_ARG;
  DecodeArgs a;
  a.rois = rois; a.roi_stride = roi_stride; a.roi_x0 = roi_x0; a.cls_score = cls_score; a.bbox_pred = bbox_pred;
  a.N = N; a.NC = num_classes; a.NB = class_agnostic ? 1 : num_classes;
  for (int k = 0; k < 4; ++k) { a.mean[k] = means[k]; a.std[k] = stds[k]; }
  a.max_ratio = fabsf(logf(wh_ratio_clip));
  a.clip_w = clip_w; a.clip_h = clip_h;
  a.inv_sx = 1.0f / scale_x; a.inv_sy = 1.0f / scale_y;
  a.scores = scores; a.bboxes = bboxes;
  DM_LAUNCH(bbox_decode_kernel, dim3(N), dim3(128), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}

extern "C" int dm_nms_mask(const float* boxes_sorted, int M, float iou_threshold, int offset, unsigned long long* mask,
                           dm_stream_t stream) {
  if (M < 0) return DM_ERR_INVALID_ARG;
  if (M == 0) return DM_OK;
  if (!boxes_sorted || !mask) return DM_ERR_INVALID_ARG;
  const int words = dm_ceil_div(M, 64);
  hipError_t e = hipMemsetAsync(mask, 0, (size_t)M * words * sizeof(unsigned long long), (hipStream_t)stream);
  if (e != hipSuccess) return DM_ERR_LAUNCH;
  DM_LAUNCH(nms_mask_kernel, dim3(words, words), dim3(64), 0, (hipStream_t)stream, boxes_sorted, M, iou_threshold,
            offset ? 1.f : 0.f, mask, words);
  return dm_check_launch();
}

extern "C" int dm_nms_mask_segmented(const float* boxes_sorted, int B, const long long* seg_tab, int max_words,
                                     float iou_threshold, int offset, unsigned long long* mask, long long mask_words,
                                     dm_stream_t stream) {
  if (B < 0 || max_words < 0 || mask_words < 0 || max_words > 65535) return DM_ERR_INVALID_ARG;
  if (B == 0 || max_words == 0) return DM_OK;
  if (!boxes_sorted || !seg_tab || !mask || B > 65535) return DM_ERR_INVALID_ARG;
  hipError_t e = hipMemsetAsync(mask, 0, (size_t)mask_words * sizeof(unsigned long long), (hipStream_t)stream);
  if (e != hipSuccess) return DM_ERR_LAUNCH;
  DM_LAUNCH(nms_mask_segmented_kernel, dim3(max_words, max_words, B), dim3(64), 0, (hipStream_t)stream, boxes_sorted,
            seg_tab, iou_threshold, offset ? 1.f : 0.f, mask);
  return dm_check_launch();
}

extern "C" int dm_nms_reduce_segmented(const unsigned long long* mask, int B, const long long* seg_tab, int max_words,
                                       int max_keep, int* keep, int* counts, dm_stream_t stream) {
  static bool lds_raised[DM_MAX_DEVICES] = {false};
  if (B < 0 || max_words < 0) return DM_ERR_INVALID_ARG;
  if (B == 0) return DM_OK;
  if (!seg_tab || !counts || (max_words > 0 && (!mask || !keep))) return DM_ERR_INVALID_ARG;
  const size_t lds = (size_t)max(max_words, 1) * sizeof(unsigned long long);
  if (lds > 160 * 1024) return DM_ERR_UNSUPPORTED;
  if (lds > 64 * 1024) {
    const int rc = dm_ensure_lds_limit((const void*)nms_reduce_segmented_kernel, 160 * 1024, lds_raised);
    if (rc != DM_OK) return rc;
  }
  DM_LAUNCH(nms_reduce_segmented_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, mask, seg_tab, max_keep, keep,
            counts);
  return dm_check_launch();
}

// Greedy pass over the suppression matrix (host code, like the reference extension's
// CPU tail): walks the boxes in score order, keeps a box unless an earlier kept box
// suppresses it.  Returns the number kept (indices into the sorted order, ascending).
extern "C" int dm_nms_reduce(const unsigned long long* mask_host, int M, int* keep, int max_keep) {
  if (M < 0 || (M > 0 && (!mask_host || !keep))) return 0;
  const int words = (M + 63) / 64;
  unsigned long long removed[1024];
  unsigned long long* rem = removed;
  unsigned long long* heap = nullptr;
  if (words > 1024) {
    heap = new unsigned long long[words];
    rem = heap;
  }
  for (int w = 0; w < words; ++w) rem[w] = 0;
  int n = 0;
  for (int i = 0; i < M; ++i) {
    if (rem[i >> 6] & (1ull << (i & 63))) continue;
    if (max_keep >= 0 && n >= max_keep) break;
    keep[n++] = i;
    const unsigned long long* row = mask_host + (size_t)i * words;
    for (int w = i >> 6; w < words; ++w) rem[w] |= row[w];
  }
  delete[] heap;
  return n;
}

extern "C" int dm_bbox_mapping_multi(const float* boxes, int box_stride, int n, int V, const float* view_tab, float* out_rois,
                                     dm_stream_t stream) {
  if (n < 0 || V < 0 || box_stride < 4) return DM_ERR_INVALID_ARG;
  if (n == 0 || V == 0) return DM_OK;
  if (!boxes || !view_tab || !out_rois) return DM_ERR_INVALID_ARG;
  const long long total = (long long)n * V;
  if (total > 0x7fffffffLL) return DM_ERR_INVALID_ARG;
  DM_LAUNCH(bbox_mapping_multi_kernel, dim3(dm_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, boxes, box_stride,
            n, V, view_tab, out_rois);
  return dm_check_launch();
}

extern "C" int dm_merge_aug_bboxes(const long long* ptr_tab, const float* view_tab, int V, int n, int box_cols,
                                   int score_cols, float* out_boxes, float* out_scores, dm_stream_t stream) {
  if (n < 0 || V < 0 || box_cols < 0 || score_cols < 0 || (box_cols & 3)) return DM_ERR_INVALID_ARG;
  if (n == 0 || box_cols + score_cols == 0) return DM_OK;
  if (V == 0 || n > 65535 || !ptr_tab || !view_tab || (box_cols && !out_boxes) || (score_cols && !out_scores))
    return DM_ERR_INVALID_ARG;
  DM_LAUNCH(merge_aug_bboxes_kernel, dim3(dm_ceil_div(box_cols + score_cols, 256), n), dim3(256), 0, (hipStream_t)stream,
            ptr_tab, view_tab, V, n, box_cols, score_cols, out_boxes, out_scores);
  return dm_check_launch();
}

extern "C" int dm_proposals_mapping_back(const long long* seg_tab, const float* view_tab, int num_segments, int max_rows,
                                         float* out, dm_stream_t stream) {
  if (num_segments < 0 || max_rows < 0) return DM_ERR_INVALID_ARG;
  if (num_segments == 0 || max_rows == 0) return DM_OK;
  if (!seg_tab || !view_tab || !out || num_segments > 65535) return DM_ERR_INVALID_ARG;
  DM_LAUNCH(proposals_mapping_back_kernel, dim3(dm_ceil_div(max_rows, 256), num_segments), dim3(256), 0,
            (hipStream_t)stream, seg_tab, view_tab, out);
  return dm_check_launch();
}

extern "C" int dm_cascade_refine(const float* rois, const float* cls_score, const float* bbox_pred, int n, int num_classes,
                                 int class_agnostic, const float* means, const float* stds, float wh_ratio_clip,
                                 const float* img_shapes, int num_images, float* score_sum, int first_stage, float* out_rois,
                                 dm_stream_t stream) {
  if (n < 0 || num_classes <= 0) return DM_ERR_INVALID_ARG;
  if (!score_sum && !out_rois) return DM_ERR_INVALID_ARG;
  if (out_rois && (!rois || !bbox_pred || !img_shapes || num_images < 1 || !means || !stds || !(wh_ratio_clip > 0.f)))
    return DM_ERR_INVALID_ARG;
  if (out_rois && out_rois == rois) return DM_ERR_INVALID_ARG;
  if (n == 0) return DM_OK;
  if (!cls_score) return DM_ERR_INVALID_ARG;
  CascadeArgs a;
  a.rois = rois; a.cls = cls_score; a.pred = bbox_pred; a.n = n; a.NC = num_classes; a.agnostic = class_agnostic ? 1 : 0;
  for (int k = 0; k < 4; ++k) {
    a.mean[k] = means ? means[k] : 0.f;
    a.std[k] = stds ? stds[k] : 1.f;
  }
  a.max_ratio = out_rois ? fabsf(logf(wh_ratio_clip)) : 0.f;
  a.img_tab = img_shapes; a.B = num_images;
  a.sum = score_sum; a.first = first_stage ? 1 : 0;
  a.out = out_rois;
  DM_LAUNCH(cascade_refine_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}
