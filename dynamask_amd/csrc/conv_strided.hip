// Mask Scoring R-CNN inference (mmdet/models/roi_heads/mask_heads/maskiou_head.py, mask_scoring_roi_head.py:58-90):
//
//   dm_conv3x3_s2_fwd     the last of MaskIoUHead's convs: 3x3, stride 2, padding 1, + bias (+ ReLU) over a batch of
//                         small maps (RoIs), out [NB, Cout, ceil(H / 2), ceil(W / 2)].  Exact fp32 on
//                         v_mfma_f32_32x32x2_f32.
//   dm_mask_iou_input     max_pool2x2(sigmoid(mask_pred[i, label_i])): the IoU head's second input (maskiou_head.py:80-81),
//                         one launch; it becomes the second source of the first conv (dm_conv2d_fwd), no torch.cat.
//   dm_mask_iou_scores    mask_iou_pred[i, label_i] * det_bboxes[i, -1] (MaskIoUHead.get_mask_scores), one launch.
//
// GEMM view, weight operand (dm_conv_pack_weight(ksize 3, one source) -> [tap][KQ][CoutP][4], so a layer's _Packed cache
// is shared), workgroup, K walk, tap loop and MFMA order are conv_dilated.hip's: the shared code is mfma_tile.h.
// This kernel's own part is the pixel tile.  At the shapes that matter (7 x 7 outputs of 16 .. 100 RoIs: 784 .. 4 900
// pixels) a tile of one RoI would fill 49 of 64 pixel slots, and a plain tiling gives less than one round over the
// 256 CUs.  So a workgroup's 64 output pixels are 64 CONSECUTIVE pixels of the flattened [NB, Ho, Wo] grid, across RoI boundaries,
// and its B operand is gathered im2col-style: per K chunk (8 channels) every (tap, pixel) slot loads the two channel
// quads of its input position (stride 2, or zero outside the map) into LDS, [tap][quad][pixel].  An input position is
// read by up to four output pixels of a tile (the windows overlap by one row / column); those loads hit the L2.
// And the K loop (C / 8 chunks) is split over `splits` workgroups per tile (1, 2, 4 or 8; auto: the smallest that puts
// two workgroups on every CU, as many as its LDS and registers let reside): each split stores its bare sums to a workspace [split][NB][Cout][Ho Wo], and a
// second kernel adds them in split order ((s0 + s1) + s2 ...) and then the bias: the same bits every run.
//
// Each wave computes WM x 32 couts x 32 pixels.  TM = 64 (WM = 1, maps of <= 64 couts) or 128 (WM = 2).
// LDS: A 9 x 2 x TM float4 (36 KiB at TM = 128) + B 9 x 2 x 64 float4 (18 KiB): 54 KiB per workgroup.
#include "mfma_tile.h"

namespace {

constexpr int S2_TN = 64;                                  // output pixels per workgroup
constexpr int S2_SLOTS = 9 * S2_TN;                        // (tap, pixel) gather slots per chunk
constexpr int S2_SPT = (S2_SLOTS + DM_CONV_NT - 1) / DM_CONV_NT;   // 3 per thread
constexpr int S2_MAXSPLIT = 8;

constexpr int S2_RELU = 1;

struct S2Args {
  const float* x;
  int NB, C, H, W, Ho, Wo;
  const float* wq;
  const float* bias;
  int Cout, CoutP, KQ, MT;
  int ntiles, splits, nchunks;
  long long npix;            // NB * Ho * Wo
  int flags;
  float* out;                // splits == 1: the result
  float* ws;                 // splits > 1: bare sums [split][NB][Cout][Ho * Wo]
};

template <int WM>
__global__ __launch_bounds__(DM_CONV_NT) void conv3x3_s2_kernel(S2Args a) {
  constexpr int TM = 2 * WM * 32;
  using WT = dm_wtile<TM, DM_CONV_NQ, DM_CONV_NT>;
  __shared__ dm_f32x4 ldsA[WT::F4];
  __shared__ dm_f32x4 ldsB[9 * DM_CONV_NQ * S2_TN];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = wave >> 1;
  const int wave_n = wave & 1;
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  // block -> (split, pixel tile, cout tile); the MT cout tiles of a pixel tile are neighbours in launch order
  const int b = (int)blockIdx.x;
  const int m_tile = b % a.MT;
  const int rest = b / a.MT;
  const int n_tile = rest % a.ntiles;
  const int split = rest / a.ntiles;
  const int m0 = m_tile * TM;
  const long long p0 = (long long)n_tile * S2_TN;
  const int HoWo = a.Ho * a.Wo;
  const size_t HW = (size_t)a.H * a.W;

  // gather slots of this thread: slot g = tid + k * 256 -> (tap g / 64, pixel g % 64); its input offset or -1 (padding)
  long long st_off[S2_SPT];
#pragma unroll
  for (int k = 0; k < S2_SPT; ++k) {
    const int g = tid + k * DM_CONV_NT;
    st_off[k] = -1;
    if (g < S2_SLOTS) {
      const int tap = g / S2_TN, p = g % S2_TN;
      const long long P = p0 + p;
      if (P < a.npix) {
        const long long n = P / HoWo;
        const int r = (int)(P - n * HoWo);
        const int oy = r / a.Wo, ox = r - (r / a.Wo) * a.Wo;
        const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) st_off[k] = n * (long long)a.C * (long long)HW + (long long)iy * a.W + ix;
      }
    }
  }

  dm_f32x16 acc[WM][1];
  dm_acc_clear(acc);

  dm_f32x4 ra[WT::PER_T];
  dm_f32x4 rb[S2_SPT * DM_CONV_NQ];
  auto prefetch = [&](int c0) {
    WT::fetch(ra, a.wq, c0 / 4, a.KQ, a.CoutP, m0, tid);
    const float* sp = a.x + (size_t)c0 * HW;
#pragma unroll
    for (int k = 0; k < S2_SPT; ++k) dm_fetch_quads<DM_CONV_NQ>(rb + k * DM_CONV_NQ, sp, st_off[k], HW);
  };
  auto commit = [&]() {
    WT::commit(ldsA, ra, tid);
#pragma unroll
    for (int k = 0; k < S2_SPT; ++k) {
      const int g = tid + k * DM_CONV_NT;
      if (g < S2_SLOTS) {
        const int tap = g / S2_TN, p = g % S2_TN;
#pragma unroll
        for (int qd = 0; qd < DM_CONV_NQ; ++qd) ldsB[(tap * DM_CONV_NQ + qd) * S2_TN + p] = rb[k * DM_CONV_NQ + qd];
      }
    }
  };

  // this split's chunks [k_lo, k_hi) of the nchunks (every split has at least one: splits <= nchunks)
  const int k_lo = (int)((long long)split * a.nchunks / a.splits);
  const int k_hi = (int)((long long)(split + 1) * a.nchunks / a.splits);
  const int pix = wave_n * 32 + l31;
  const int b_lane[1] = {hi * S2_TN + pix};       // B image [tap][quad][pixel]
  prefetch(k_lo * DM_CONV_CK);
#pragma unroll 1
  for (int kc = k_lo; kc < k_hi; ++kc) {
    commit();
    __syncthreads();
    if (kc + 1 < k_hi) prefetch((kc + 1) * DM_CONV_CK);
    dm_nine_taps<WT>(acc, ldsA, ldsB, hi, l31, wave_m * WM, b_lane, [](int tap) { return tap * DM_CONV_NQ * S2_TN; });
    __syncthreads();
  }

  // ---- epilogue: every store is guarded (pixel < npix, cout < Cout)
  const long long P = p0 + pix;
  if (P >= a.npix) return;
  const long long n = P / HoWo;
  const int r_pix = (int)(P - n * HoWo);
  const int co_wave = m0 + wave_m * WM * 32;
  const bool relu = (a.flags & S2_RELU) != 0;
  const size_t plane_stride = (size_t)a.NB * a.Cout * HoWo;
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co_wave + i * 32 + dm_dtile_row(r, hi);
      if (co >= a.Cout) continue;
      const size_t o = ((size_t)n * a.Cout + co) * HoWo + r_pix;
      if (a.splits == 1) {
        float v = acc[i][0][r] + (a.bias ? a.bias[co] : 0.f);
        if (relu) v = dm_relu(v);
        a.out[o] = v;
      } else {
        a.ws[(size_t)split * plane_stride + o] = acc[i][0][r];
      }
    }
}

// out[e] = act(((ws[0][e] + ws[1][e]) + ...) + bias[co]): the splits in index order, then the bias
__global__ __launch_bounds__(256) void conv3x3_s2_reduce_kernel(const float* __restrict__ ws, int splits, long long total,
                                                                int Cout, int HoWo, const float* __restrict__ bias, int relu,
                                                                float* __restrict__ out) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    float v = ws[e];
    for (int s = 1; s < splits; ++s) v += ws[(size_t)s * total + e];
    if (bias) v += bias[(e / HoWo) % Cout];
    if (relu) v = dm_relu(v);
    out[e] = v;
  }
}

// ------------------------------------------------------------------------------------------------ IoU-head input
// out[i, 0, y, x] = max over the 2 x 2 window (row-major) of sigmoid(pred[i, c_i, 2y + dy, 2x + dx]), c_i = label_i clamped
// to [0, C - 1] (0 when C == 1).  The max is torch's max_pool2d rule: a later element replaces the running max when it is
// larger or NaN.
__global__ __launch_bounds__(256) void mask_iou_input_kernel(const float* __restrict__ pred, long long n, int C, int H, int W,
                                                             const long long* __restrict__ labels, int Ho, int Wo,
                                                             float* __restrict__ out) {
  const long long per = (long long)Ho * Wo, total = n * per;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long i = e / per;
    const int r = (int)(e - i * per);
    const int oy = r / Wo, ox = r - (r / Wo) * Wo;
    long long c = 0;
    if (C > 1) {
      c = labels[i];
      c = c < 0 ? 0 : (c > C - 1 ? C - 1 : c);
    }
    const float* p = pred + ((size_t)i * C + (size_t)c) * H * W + (size_t)(2 * oy) * W + 2 * ox;
    float m = dm_sigmoid(p[0]);
    const float rest3[3] = {dm_sigmoid(p[1]), dm_sigmoid(p[W]), dm_sigmoid(p[W + 1])};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (rest3[k] > m || __builtin_isnan(rest3[k])) m = rest3[k];
    out[e] = m;
  }
}

// scores[i] = iou[i, c_i] * dets[i, D - 1], c_i = label_i clamped to [0, NC - 1]
__global__ __launch_bounds__(256) void mask_iou_scores_kernel(const float* __restrict__ iou, int n, int NC,
                                                              const long long* __restrict__ labels,
                                                              const float* __restrict__ dets, int D, float* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  long long c = labels[i];
  c = c < 0 ? 0 : (c > NC - 1 ? NC - 1 : c);
  out[i] = iou[(size_t)i * NC + (size_t)c] * dets[(size_t)i * D + D - 1];
}

// ------------------------------------------------------------------------------------------------ host side
long long s2_tiles(int NB, int H, int W) {
  return ((long long)NB * ((H + 1) / 2) * ((W + 1) / 2) + S2_TN - 1) / S2_TN;
}

// the split count a request resolves to: `splits` itself, or (0) the smallest of 1, 2, 4, 8 (<= C / 8) that puts two
// workgroups on every CU (two reside per CU: 54 KiB of LDS, <= 256 registers); -1: not supported
int s2_resolve(int NB, int C, int H, int W, int Cout, int splits) {
  if (!dm_conv3x3_shape_ok(NB, C, H, W, Cout)) return -1;
  const int nchunks = C / DM_CONV_CK;
  const long long base = s2_tiles(NB, H, W) * dm_cout_tiles(Cout);
  int s = splits;
  if (s == 0) {
    s = 1;
    while (s < S2_MAXSPLIT && 2 * s <= nchunks && base * s < 2LL * dm_num_cus()) s *= 2;
  } else if (!(s == 1 || s == 2 || s == 4 || s == 8) || s > nchunks) {
    return -1;
  }
  if (base * s > 0x7fffffffLL) return -1;
  return s;
}

// the workspace of a resolved split count: nothing for one split, else a plane of bare sums per split
long long s2_ws_floats(int s, int NB, int H, int W, int Cout) {
  return s == 1 ? 0 : (long long)s * NB * Cout * ((H + 1) / 2) * ((W + 1) / 2);
}

}  // namespace

extern "C" int dm_conv3x3_s2_supported(int NB, int C, int H, int W, int Cout, int splits) {
  return s2_resolve(NB, C, H, W, Cout, splits) > 0 ? 1 : 0;
}

extern "C" long long dm_conv3x3_s2_workspace_floats(int NB, int C, int H, int W, int Cout, int splits) {
  const int s = s2_resolve(NB, C, H, W, Cout, splits);
  return s < 0 ? -1 : s2_ws_floats(s, NB, H, W, Cout);
}

extern "C" int dm_conv3x3_s2_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                                 int Cout, int splits, int flags, float* out, float* workspace, long long workspace_floats,
                                 dm_stream_t stream) {
  if (!x || !w_packed || !out) return DM_ERR_INVALID_ARG;
  const int fc = dm_flags_check(flags, S2_RELU);
  if (fc != DM_OK) return fc;
  const int s = s2_resolve(NB, C, H, W, Cout, splits);
  if (s < 0) return DM_ERR_UNSUPPORTED;
  if (s > 1 && (!workspace || workspace_floats < s2_ws_floats(s, NB, H, W, Cout))) return DM_ERR_INVALID_ARG;
  S2Args a = {};
  a.x = x; a.NB = NB; a.C = C; a.H = H; a.W = W;
  a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
  a.wq = w_packed; a.bias = bias;
  a.Cout = Cout; a.CoutP = dm_conv_packed_cout(Cout); a.KQ = C / 4; a.MT = dm_cout_tiles(Cout);
  a.ntiles = (int)s2_tiles(NB, H, W); a.splits = s; a.nchunks = C / DM_CONV_CK;
  a.npix = (long long)NB * a.Ho * a.Wo;
  a.flags = flags; a.out = out; a.ws = s > 1 ? workspace : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((long long)a.MT * a.ntiles * s)), block(DM_CONV_NT);
  if (Cout <= 64) DM_LAUNCH((conv3x3_s2_kernel<1>), grid, block, 0, st, a);
  else DM_LAUNCH((conv3x3_s2_kernel<2>), grid, block, 0, st, a);
  int rc = dm_check_launch();
  if (rc != DM_OK || s == 1) return rc;
  const long long total = (long long)NB * Cout * a.Ho * a.Wo;
  DM_LAUNCH(conv3x3_s2_reduce_kernel, dim3(dm_grid_1d(total, 4096)), dim3(256), 0, st, workspace, s, total, Cout,
            a.Ho * a.Wo, bias, (flags & S2_RELU) ? 1 : 0, out);
  return dm_check_launch();
}

extern "C" int dm_mask_iou_input_supported(int n, int C, int H, int W) {
  return (n >= 0 && C >= 1 && H >= 2 && W >= 2) ? 1 : 0;
}

extern "C" int dm_mask_iou_input(const float* mask_pred, int n, int C, int H, int W, const long long* labels, float* out,
                                 dm_stream_t stream) {
  if (!dm_mask_iou_input_supported(n, C, H, W)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!mask_pred || !out || (C > 1 && !labels)) return DM_ERR_INVALID_ARG;
  const int Ho = H / 2, Wo = W / 2;
  const long long total = (long long)n * Ho * Wo;
  DM_LAUNCH(mask_iou_input_kernel, dim3(dm_grid_1d(total, 4096)), dim3(256), 0, (hipStream_t)stream, mask_pred,
            (long long)n, C, H, W, labels, Ho, Wo, out);
  return dm_check_launch();
}

extern "C" int dm_mask_iou_scores(const float* mask_iou_pred, int n, int NC, const long long* labels, const float* dets,
                                  int D, float* out, dm_stream_t stream) {
  if (n < 0 || NC < 1 || D < 1) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!mask_iou_pred || !labels || !dets || !out) return DM_ERR_INVALID_ARG;
  DM_LAUNCH(mask_iou_scores_kernel, dim3((unsigned)((n + 255LL) / 256)), dim3(256), 0, (hipStream_t)stream, mask_iou_pred, n,
            NC, labels, dets, D, out);
  return dm_check_launch();
}
