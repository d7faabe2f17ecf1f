// delta2bbox and the clip of one box: shared by bbox.hip (dm_bbox_decode, dm_cascade_refine) and rpn.hip (dm_rpn_decode)
// so that every decode of the library has the same bits.
#pragma once
#include "common.h"

namespace {

// delta2bbox of one box (delta_xywh_bbox_coder.py:165-204): the decode of bbox_decode_kernel and cascade_refine_kernel,
// one device function so that a cascade stage's boxes have the bits of dm_bbox_decode's.  The fused multiply-adds are
// spelled out and nothing else is contracted: left to the compiler, the pairs it fuses depend on the code around the call
// (bbox_decode_kernel computes the centre once per row, outside its loop, and fuses pw * dx into the centre; inlined in
// a kernel without that loop, (rx1 + rx2) * 0.5f was fused instead).  These are the operations bbox_decode_kernel has
// always compiled to.
__device__ __forceinline__ void delta2bbox_one(float rx1, float ry1, float rx2, float ry2, const float* __restrict__ d,
                                               const float (&mean)[4], const float (&std)[4], float max_ratio, float& x1,
                                               float& y1, float& x2, float& y2) {
#pragma clang fp contract(off)
  const float dx = __builtin_fmaf(d[0], std[0], mean[0]);
  const float dy = __builtin_fmaf(d[1], std[1], mean[1]);
  float dw = __builtin_fmaf(d[2], std[2], mean[2]);
  float dh = __builtin_fmaf(d[3], std[3], mean[3]);
  dw = fminf(fmaxf(dw, -max_ratio), max_ratio);
  dh = fminf(fmaxf(dh, -max_ratio), max_ratio);
  const float px = (rx1 + rx2) * 0.5f, py = (ry1 + ry2) * 0.5f;
  const float pw = rx2 - rx1, ph = ry2 - ry1;
  const float gw = pw * expf(dw), gh = ph * expf(dh);
  const float gx = __builtin_fmaf(pw, dx, px), gy = __builtin_fmaf(ph, dy, py);
  x1 = __builtin_fmaf(-0.5f, gw, gx);
  y1 = __builtin_fmaf(-0.5f, gh, gy);
  x2 = __builtin_fmaf(0.5f, gw, gx);
  y2 = __builtin_fmaf(0.5f, gh, gy);
}

__device__ __forceinline__ void clip_box(float& x1, float& y1, float& x2, float& y2, float clip_w, float clip_h) {
  x1 = fminf(fmaxf(x1, 0.f), clip_w);
  x2 = fminf(fmaxf(x2, 0.f), clip_w);
  y1 = fminf(fmaxf(y1, 0.f), clip_h);
  y2 = fminf(fmaxf(y2, 0.f), clip_h);
}

}  // namespace
