// PointRend inference: the subdivision step of PointRendRoIHead._mask_point_forward_test
// (mmdet/models/roi_heads/point_rend_roi_head.py:96-128) on the label channel of the refined map.
//
//   dm_point_select      per RoI, the P cells of smallest |v| of an [n, HW] map (MaskPointHead.get_roi_rel_points_test:
//                        topk(-|logit[label]|)), indices in ascending order; at the cut the lower flat index wins.
//                        One 1024-thread workgroup per RoI: a radix select on the 31 magnitude bits (four 8-bit passes
//                        over the map, histogram in LDS), then one pass in index order that compacts the selection.
//                        The map (up to 224^2 = 50 176 floats, 196 KiB) does not fit the LDS: every pass reads it from
//                        the L2 / memory.
//   dm_point_gather_fwd  per (RoI, selected cell): the cell centre (get_roi_rel_points_test's fp32 chain), the C-channel
//                        point_sample of the RoI's image of the feature map at rel_roi_point_to_rel_img_point of it, and
//                        the NC-channel point_sample of the RoI's coarse logits at the RoI-relative point -> one
//                        [n, C + NC, P] buffer (the point head's input, fine channels first).
//   dm_point_mlp_fwd     MaskPointHead.forward (mask_point_head.py:85-104) on that buffer: nfc layers
//                        relu(W [F, C + NC] x [h; coarse] + b) (F == C: each layer's output takes the place of the fine
//                        channels), then the label row of fc_logits, written straight into the refined map at the
//                        selected cells (the scatter_ of :121-124).  Exact fp32 MFMA (v_mfma_f32_32x32x2_f32).
//   dm_point_scatter     map[r, idx[r, p]] = vals[r, p]: the scatter of the unfused sequence.
//
// point_sample is mmcv's: grid_sample(bilinear, zeros, align_corners=False) of points * 2 - 1.  The sample below
// repeats the fp32 operations of PyTorch's CPU grid sampler (unnormalize (g + 1) * size / 2 - 0.5, weights from the
// floor distances, corners added nw, ne, sw, se), with every product and sum rounded on its own (no contraction).
#include "mfma_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------ selection
constexpr int SEL_NT = 1024;
constexpr int SEL_NW = SEL_NT / DM_WAVE;      // 16 waves
constexpr unsigned MAG = 0x7fffffffu;          // |v| as an unsigned key: the bit pattern orders like the magnitude
constexpr long long SEL_MAX_HW = 1LL << 24;

// The selection key of a map value: the P SMALLEST keys are taken.  SEL_MAG: |v| (PointRend's least certain cells).
// SEL_DESC_RAW / SEL_DESC_SIGMOID: v / dm_sigmoid(v) (the library's logistic) in descending order (PointRefine's topk of
// the detail map): the order-preserving unsigned image of the float, complemented.
enum { SEL_MAG = 0, SEL_DESC_RAW = 1, SEL_DESC_SIGMOID = 2 };

template <int MODE>
__device__ __forceinline__ unsigned sel_key(const float* __restrict__ row, int i) {
  if constexpr (MODE == SEL_MAG) {
    return reinterpret_cast<const unsigned*>(row)[i] & MAG;
  } else {
    const float v = MODE == SEL_DESC_SIGMOID ? dm_sigmoid(row[i]) : row[i];
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;                  // -0 and +0 are one key, as they compare: the lower index wins the tie
    const unsigned up = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ~up;
  }
}

template <int MODE>
__global__ __launch_bounds__(SEL_NT) void point_select_kernel(const float* __restrict__ map, int HW, int P,
                                                              int* __restrict__ idx) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_digit, s_k;
  __shared__ unsigned wcnt[2][SEL_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* keys = map + (size_t)blockIdx.x * HW;
  int* out = idx + (size_t)blockIdx.x * P;

  // radix select: after the four passes T = prefix is the key of the P-th smallest, k the number of keys == T to take
  unsigned prefix = 0, mask = 0, k = (unsigned)P;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < HW; i += SEL_NT) {
      const unsigned key = sel_key<MODE>(keys, i);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wave == 0) {
      unsigned h[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = hist[4 * lane + j];
        s += h[j];
      }
      unsigned incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
      }
      const unsigned excl = incl - s;
      if (excl < k && k <= incl) {        // exactly one lane: the digit holding the k-th key
        unsigned c = excl;
        int dsel = 4 * lane + 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (c + h[j] >= k) {
            dsel = 4 * lane + j;
            break;
          }
          c += h[j];
        }
        s_digit = (unsigned)dsel;
        s_k = k - c;
      }
    }
    __syncthreads();
    prefix |= s_digit << shift;
    mask |= 255u << shift;
    k = s_k;
    __syncthreads();
  }

  // compaction in index order: key < T, or key == T among the first k such indices
  const unsigned T = prefix;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned base_eq = 0, base_sel = 0;
#pragma unroll 1
  for (int t0 = 0; t0 < HW; t0 += SEL_NT) {
    const int i = t0 + tid;
    const unsigned key = i < HW ? sel_key<MODE>(keys, i) : 0xffffffffu;
    const bool lt = key < T, eq = key == T;
    const unsigned long long beq = __ballot(eq);
    if (lane == 0) wcnt[0][wave] = (unsigned)__popcll(beq);
    __syncthreads();
    unsigned eq_rank = base_eq + (unsigned)__popcll(beq & below), tot_eq = 0;
#pragma unroll
    for (int w = 0; w < SEL_NW; ++w) {
      const unsigned c = wcnt[0][w];
      if (w < wave) eq_rank += c;
      tot_eq += c;
    }
    const bool sel = lt || (eq && eq_rank < k);
    const unsigned long long bsel = __ballot(sel);
    if (lane == 0) wcnt[1][wave] = (unsigned)__popcll(bsel);
    __syncthreads();
    unsigned pos = base_sel + (unsigned)__popcll(bsel & below), tot_sel = 0;
#pragma unroll
    for (int w = 0; w < SEL_NW; ++w) {
      const unsigned c = wcnt[1][w];
      if (w < wave) pos += c;
      tot_sel += c;
    }
    if (sel && pos < (unsigned)P) out[pos] = i;
    base_eq += tot_eq;
    base_sel += tot_sel;
    __syncthreads();                      // wcnt is rewritten by the next tile
    if (base_sel >= (unsigned)P) break;   // (uniform)
  }
}

// ------------------------------------------------------------------------------------------------ gather
constexpr int GAT_NT = 256;
constexpr int GAT_CG = 8;                     // channels per thread

// mmcv point_sample of one channel plane [H, W] at the normalised point (rx, ry) in [0, 1]^2
__device__ __forceinline__ float grid_sample_zeros(const float* __restrict__ plane, int H, int W, float rx, float ry) {
  const float gx = __fsub_rn(__fmul_rn(rx, 2.f), 1.f), gy = __fsub_rn(__fmul_rn(ry, 2.f), 1.f);
  const float ix = __fsub_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f * (float)W), 0.5f);
  const float iy = __fsub_rn(__fmul_rn(__fadd_rn(gy, 1.f), 0.5f * (float)H), 0.5f);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float w = __fsub_rn(ix, x0), e = __fsub_rn(1.f, w);
  const float nn = __fsub_rn(iy, y0), s = __fsub_rn(1.f, nn);
  const float wnw = __fmul_rn(s, e), wne = __fmul_rn(s, w), wsw = __fmul_rn(nn, e), wse = __fmul_rn(nn, w);
  // corners inside the plane (a point far outside -- a huge box -- never reaches the int conversion)
  const bool x0in = x0 >= 0.f && x0 < (float)W, x1in = x0 + 1.f >= 0.f && x0 + 1.f < (float)W;
  const bool y0in = y0 >= 0.f && y0 < (float)H, y1in = y0 + 1.f >= 0.f && y0 + 1.f < (float)H;
  const int xi = (x0in || x1in) ? (int)x0 : 0, yi = (y0in || y1in) ? (int)y0 : 0;
  const float vnw = (x0in && y0in) ? plane[(long long)yi * W + xi] : 0.f;
  const float vne = (x1in && y0in) ? plane[(long long)yi * W + xi + 1] : 0.f;
  const float vsw = (x0in && y1in) ? plane[(long long)(yi + 1) * W + xi] : 0.f;
  const float vse = (x1in && y1in) ? plane[(long long)(yi + 1) * W + xi + 1] : 0.f;
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(vnw, wnw), __fmul_rn(vne, wne)), __fmul_rn(vsw, wsw)), __fmul_rn(vse, wse));
}

struct GatherArgs {
  const float* feat;
  int B, C, H, W;
  const float* rois;
  int n;
  const float* coarse;
  int NC, CH, CW;
  const int* idx;
  int P, MH, MW;
  float spatial_scale;
  float* out;
};

__global__ __launch_bounds__(GAT_NT) void point_gather_kernel(GatherArgs a) {
  const long long gp = (long long)blockIdx.x * GAT_NT + threadIdx.x;
  if (gp >= (long long)a.n * a.P) return;
  const int roi = (int)(gp / a.P), p = (int)(gp - (long long)roi * a.P);
  const int flat = a.idx[gp];
  const int col = flat % a.MW, row = flat / a.MW;
  // get_roi_rel_points_test: w_step = 1.0 / W (Python double) meets the fp32 tensor as an fp32 scalar
  const float w_step = (float)(1.0 / (double)a.MW), h_step = (float)(1.0 / (double)a.MH);
  const float px = __fadd_rn(0.5f * w_step, __fmul_rn((float)col, w_step));
  const float py = __fadd_rn(0.5f * h_step, __fmul_rn((float)row, h_step));
  const int CT = a.C + a.NC;
  float* o = a.out + (size_t)roi * CT * a.P + p;
  const int c0 = blockIdx.y * GAT_CG;
  if (c0 < a.C) {
    const float* r = a.rois + (size_t)roi * 5;
    const float bf = r[0];
    const int b = (int)bf;
    if (!(bf >= 0.f) || b >= a.B) {       // a RoI of no image of the batch: zeros
#pragma unroll
      for (int c = 0; c < GAT_CG; ++c) o[(size_t)(c0 + c) * a.P] = 0.f;
      return;
    }
    // rel_roi_point_to_rel_img_point: abs = rel * (x2 - x1) + x1, then abs / (W, H) of the map * spatial_scale
    const float ax = __fadd_rn(__fmul_rn(px, __fsub_rn(r[3], r[1])), r[1]);
    const float ay = __fadd_rn(__fmul_rn(py, __fsub_rn(r[4], r[2])), r[2]);
    const float rx = __fmul_rn(__fdiv_rn(ax, (float)a.W), a.spatial_scale);
    const float ry = __fmul_rn(__fdiv_rn(ay, (float)a.H), a.spatial_scale);
    const size_t HWf = (size_t)a.H * a.W;
    const float* f = a.feat + ((size_t)b * a.C + c0) * HWf;
#pragma unroll
    for (int c = 0; c < GAT_CG; ++c) o[(size_t)(c0 + c) * a.P] = grid_sample_zeros(f + c * HWf, a.H, a.W, rx, ry);
  } else {
    const int k0 = c0 - a.C;
    const size_t HWc = (size_t)a.CH * a.CW;
    const float* f = a.coarse + ((size_t)roi * a.NC + k0) * HWc;
#pragma unroll
    for (int c = 0; c < GAT_CG; ++c) o[(size_t)(c0 + c) * a.P] = grid_sample_zeros(f + c * HWc, a.CH, a.CW, px, py);
  }
}

// ------------------------------------------------------------------------------------------------ point MLP
// Workgroup, activation image and hidden layers are mfma_tile.h's point MLP: wave w computes output channels [64 w,
// 64 w + 64) of a layer for the 64 points as 2 x 2 tiles of 32 x 32.  KQ = (C + NC) / 4 quads (86 KB at 336 channels);
// a layer writes its F = C outputs over the first C channels, the NC coarse channels stay (weights: 1 MB for three
// layers).  This kernel's own is the last layer: the label row of fc_logits as a dot product per point.
constexpr int MLP_F = 256;
constexpr int MLP_MAXFC = 4;
constexpr int MLP_MAXNC = 96;

struct MlpArgs {
  const float* x;
  int n, P, C, NC, KQ, CoutP, nfc, tiles;
  const float* w[MLP_MAXFC];
  const float* b[MLP_MAXFC];
  const float* wl;
  const float* bl;
  int NCL;
  const long long* labels;
  const int* idx;
  float* refined;
  int HW;
};

__global__ __launch_bounds__(DM_MLP_NT) void point_mlp_kernel(MlpArgs a) {
  extern __shared__ dm_f32x4 lds[];            // [KQ][64] activations, then red[4][64], then the logits row
  float* red = reinterpret_cast<float*>(lds + a.KQ * DM_MLP_TP);
  float* wrow = red + 4 * DM_MLP_TP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int roi = blockIdx.x / a.tiles, p0 = (blockIdx.x - roi * a.tiles) * DM_MLP_TP;
  const int np = min(DM_MLP_TP, a.P - p0);
  const int CT = a.C + a.NC;
  const float* xr = a.x + (size_t)roi * CT * a.P + p0;

  dm_mlp_stage(lds, xr, a.KQ, a.P, np, tid);
  int lab = (int)a.labels[roi];
  lab = lab < 0 ? 0 : (lab >= a.NCL ? a.NCL - 1 : lab);
  for (int k = tid; k < CT; k += DM_MLP_NT) wrow[k] = a.wl[(size_t)lab * CT + k];
  __syncthreads();

  const int co_w = wave * 64;
#pragma unroll 1
  for (int L = 0; L < a.nfc; ++L) {
    dm_f32x16 acc[2][2];
    dm_mlp_gemm(acc, a.w[L], a.CoutP, a.KQ, lds, co_w, 0, hi, l31);
    dm_mlp_relu_store(acc, a.b[L], lds, co_w, 0, hi, l31);
  }

  // the label row of fc_logits: four partial sums per point over quarters of the quads, added in order
  {
    const int p = tid & (DM_MLP_TP - 1), part = tid >> 6;
    const int qper = (a.KQ + 3) / 4, qa = part * qper, qb = min(a.KQ, qa + qper);
    float s = 0.f;
    for (int q = qa; q < qb; ++q) {
      const dm_f32x4 v = lds[q * DM_MLP_TP + p];
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(wrow[4 * q + j], v[j], s);
    }
    red[part * DM_MLP_TP + p] = s;
  }
  __syncthreads();
  if (tid < np) {
    const float v = ((red[tid] + red[DM_MLP_TP + tid]) + red[2 * DM_MLP_TP + tid]) + red[3 * DM_MLP_TP + tid] + (a.bl ? a.bl[lab] : 0.f);
    const int cell = a.idx[(size_t)roi * a.P + p0 + tid];
    if (cell >= 0 && cell < a.HW) a.refined[(size_t)roi * a.HW + cell] = v;
  }
}

size_t mlp_lds_bytes(int KQ, int CT) { return (size_t)KQ * DM_MLP_TP * 16 + 4 * DM_MLP_TP * 4 + (size_t)CT * 4; }

// ------------------------------------------------------------------------------------------------ scatter
__global__ void point_scatter_kernel(const float* __restrict__ vals, const int* __restrict__ idx, long long total, int P,
                                     float* __restrict__ map, int HW) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const long long roi = g / P;
  const int cell = idx[g];
  if (cell >= 0 && cell < HW) map[roi * HW + cell] = vals[g];
}

}  // namespace

extern "C" int dm_point_select_supported(int n, int HW, int P) {
  return (n >= 0 && HW >= 1 && (long long)HW <= SEL_MAX_HW && P >= 1 && P <= HW) ? 1 : 0;
}

extern "C" int dm_point_select(const float* map, int n, int HW, int P, int* idx, dm_stream_t stream) {
  if (!dm_point_select_supported(n, HW, P)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!map || !idx) return DM_ERR_INVALID_ARG;
  DM_LAUNCH(point_select_kernel<SEL_MAG>, dim3(n), dim3(SEL_NT), 0, (hipStream_t)stream, map, HW, P, idx);
  return dm_check_launch();
}

extern "C" int dm_point_gather_supported(int B, int C, int H, int W, int n, int NC, int CH, int CW, int P, int MH, int MW) {
  if (B < 1 || C < GAT_CG || C % GAT_CG != 0 || H < 1 || W < 1 || n < 0) return 0;
  if (NC < GAT_CG || NC % GAT_CG != 0 || CH < 1 || CW < 1 || MH < 1 || MW < 1) return 0;
  if (P < 1 || (long long)P > (long long)MH * MW || (long long)MH * MW > 0x7fffffffLL) return 0;
  return dm_ceil_div((long long)n * P, GAT_NT) <= 0x7fffffffLL ? 1 : 0;
}

extern "C" int dm_point_gather_fwd(const float* feat, int B, int C, int H, int W, const float* rois, int n,
                                   const float* coarse, int NC, int CH, int CW, const int* idx, int P, int MH, int MW,
                                   float spatial_scale, float* out, dm_stream_t stream) {
  if (!dm_point_gather_supported(B, C, H, W, n, NC, CH, CW, P, MH, MW)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!feat || !rois || !coarse || !idx || !out) return DM_ERR_INVALID_ARG;
  GatherArgs a = {feat, B, C, H, W, rois, n, coarse, NC, CH, CW, idx, P, MH, MW, spatial_scale, out};
  const dim3 grid((unsigned)dm_ceil_div((long long)n * P, GAT_NT), (unsigned)((C + NC) / GAT_CG));
  DM_LAUNCH(point_gather_kernel, grid, dim3(GAT_NT), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}

extern "C" int dm_point_mlp_supported(int n, int P, int C, int NC, int F, int num_fcs, int NCL, int HW) {
  if (n < 0 || P < 1 || P > HW || C != MLP_F || F != MLP_F || NC < 8 || NC % 8 != 0 || NC > MLP_MAXNC) return 0;
  if (num_fcs < 1 || num_fcs > MLP_MAXFC || NCL < 1) return 0;
  return (long long)n * dm_ceil_div(P, DM_MLP_TP) <= 0x7fffffffLL ? 1 : 0;
}

extern "C" int dm_point_mlp_fwd(const float* x, int n, int P, int C, int NC, int F, int num_fcs,
                                const float* const* w_packed, const float* const* bias, const float* w_logits,
                                const float* b_logits, int NCL, const long long* labels, const int* idx, int flags,
                                float* refined, int HW, dm_stream_t stream) {
  const int fc = dm_flags_check(flags, 0);
  if (fc != DM_OK) return fc;
  if (!dm_point_mlp_supported(n, P, C, NC, F, num_fcs, NCL, HW)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!x || !w_packed || !w_logits || !labels || !idx || !refined) return DM_ERR_INVALID_ARG;
  MlpArgs a = {};
  a.x = x; a.n = n; a.P = P; a.C = C; a.NC = NC; a.KQ = (C + NC) / 4; a.CoutP = dm_conv_packed_cout(F);
  a.nfc = num_fcs; a.tiles = dm_ceil_div(P, DM_MLP_TP);
  for (int L = 0; L < num_fcs; ++L) {
    if (!w_packed[L]) return DM_ERR_INVALID_ARG;
    a.w[L] = w_packed[L];
    a.b[L] = bias ? bias[L] : nullptr;
  }
  a.wl = w_logits; a.bl = b_logits; a.NCL = NCL; a.labels = labels; a.idx = idx; a.refined = refined; a.HW = HW;
  const int lds = (int)mlp_lds_bytes(a.KQ, C + NC);
  static bool raised[DM_MAX_DEVICES] = {false};
  const int rc = dm_ensure_lds_limit((const void*)point_mlp_kernel, lds, raised);
  if (rc != DM_OK) return rc;
  DM_LAUNCH(point_mlp_kernel, dim3((unsigned)((long long)n * a.tiles)), dim3(DM_MLP_NT), lds, (hipStream_t)stream, a);
  return dm_check_launch();
}

extern "C" int dm_point_scatter(const float* vals, const int* idx, int n, int P, float* map, int HW, dm_stream_t stream) {
  if (n < 0 || P < 1 || P > HW) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!vals || !idx || !map) return DM_ERR_INVALID_ARG;
  const long long total = (long long)n * P;
  DM_LAUNCH(point_scatter_kernel, dim3((unsigned)dm_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, vals, idx,
            total, P, map, HW);
  return dm_check_launch();
}

// =====================================================================================================================
// PointRefine inference (header section K24): one SFMStage of mmdet/models/roi_heads/mask_heads/mask_point_refine.py
// (:95-132) on the stage features f [n, C, S, S]:
//
//   dm_point_topk_select   per RoI, the P cells of LARGEST detail value (topk of sigmoid(detail[label]), or of the raw
//                          logit without mask_use_sigmoid), indices ascending, the lower flat index first among equal
//                          keys at the cut: point_select_kernel with the descending keys.
//   dm_point_feat_gather   the MLP input [n, C + NC, P] in one launch: C channels point_sample'd from the RoI's image of
//                          the stage's semantic map (dm_point_gather_fwd's expressions), NC channels copied
//                          exactly from the RoI's [NC, S * S] coarse logit map at the selected cell (torch.gather).
//   dm_point_refine_mlp    num_fcs layers relu(W [C, C + NC] x [h; coarse] + b), then fc_logits [C, C + NC] (no ReLU),
//                          ALL C rows written into f at the selected cells (the scatter_ of :126-127).  Exact fp32 MFMA.
//   dm_point_scatter_rows  f[r, c, idx[r, p]] = vals[r, c, p]: the scatter of the unfused sequence.
// A NULL index array means "every cell in order" (P == S * S: the select is skipped, the MLP is per point).

namespace {

// ------------------------------------------------------------------------------------------------ gather
struct FeatGatherArgs {
  const float* feat;
  int B, C, H, W;
  const float* rois;
  int n;
  const float* coarse;
  int NC;
  const int* idx;
  int P, S;
  float spatial_scale;
  float* out;
};

__global__ __launch_bounds__(GAT_NT) void point_feat_gather_kernel(FeatGatherArgs a) {
  const long long gp = (long long)blockIdx.x * GAT_NT + threadIdx.x;
  if (gp >= (long long)a.n * a.P) return;
  const int roi = (int)(gp / a.P), p = (int)(gp - (long long)roi * a.P);
  const int HW = a.S * a.S;
  const int flat = a.idx ? a.idx[gp] : p;
  const int CT = a.C + a.NC;
  float* o = a.out + (size_t)roi * CT * a.P + p;
  const int c0 = blockIdx.y * GAT_CG;
  if (c0 < a.C) {
    const int col = flat % a.S, row = flat / a.S;
    // get_roi_rel_points_train: w_step = 1.0 / S (Python double) meets the fp32 tensor as an fp32 scalar
    const float step = (float)(1.0 / (double)a.S);
    const float px = __fadd_rn(0.5f * step, __fmul_rn((float)col, step));
    const float py = __fadd_rn(0.5f * step, __fmul_rn((float)row, step));
    const float* r = a.rois + (size_t)roi * 5;
    const float bf = r[0];
    const int b = (int)bf;
    if (!(bf >= 0.f) || b >= a.B) {       // a RoI of no image of the batch: zeros
#pragma unroll
      for (int c = 0; c < GAT_CG; ++c) o[(size_t)(c0 + c) * a.P] = 0.f;
      return;
    }
    const float ax = __fadd_rn(__fmul_rn(px, __fsub_rn(r[3], r[1])), r[1]);
    const float ay = __fadd_rn(__fmul_rn(py, __fsub_rn(r[4], r[2])), r[2]);
    const float rx = __fmul_rn(__fdiv_rn(ax, (float)a.W), a.spatial_scale);
    const float ry = __fmul_rn(__fdiv_rn(ay, (float)a.H), a.spatial_scale);
    const size_t HWf = (size_t)a.H * a.W;
    const float* f = a.feat + ((size_t)b * a.C + c0) * HWf;
#pragma unroll
    for (int c = 0; c < GAT_CG; ++c) o[(size_t)(c0 + c) * a.P] = grid_sample_zeros(f + c * HWf, a.H, a.W, rx, ry);
  } else {
    const int k0 = c0 - a.C;
    const float* f = a.coarse + ((size_t)roi * a.NC + k0) * HW + flat;
#pragma unroll
    for (int c = 0; c < GAT_CG; ++c) o[(size_t)(c0 + c) * a.P] = f[(size_t)c * HW];
  }
}

// ------------------------------------------------------------------------------------------------ point MLP
// mfma_tile.h's point MLP again.  The C output channels x 64 points of a layer are C / 32 x 2 tiles of 32 x 32:
// C = 256 -- a wave owns two channel tiles x both point tiles (dm_point_mlp_fwd's split); C = 128 -- one channel tile x
// both point tiles; C = 64 -- one channel tile x one point tile.  KQ = (C + NC) / 4: 104 KB at C = 256, NC = 160.
// fc_logits is one more layer of the same shape whose outputs (+ bias, no ReLU) go to f at the selected cells.
constexpr int RMLP_MAXNC = 160;
constexpr int RMLP_MAXFC = 4;

struct RefineMlpArgs {
  const float* x;
  int n, P, NC, KQ, CoutP, nfc, tiles;
  const float* w[RMLP_MAXFC + 1];              // the hidden layers, then fc_logits
  const float* b[RMLP_MAXFC + 1];
  const int* idx;
  float* feat;
  int HW;
};

template <int C>
__global__ __launch_bounds__(DM_MLP_NT) void point_refine_mlp_kernel(RefineMlpArgs a) {
  constexpr int NT32 = C / 32 * 2;              // 32 x 32 tiles of a layer
  constexpr int TW = NT32 / 4;                  // per wave
  constexpr int NJ = TW >= 2 ? 2 : 1;           // point tiles per wave
  constexpr int NI = TW / NJ;                   // channel tiles per wave
  static_assert(NI * NJ * 4 == NT32, "tile split");
  extern __shared__ dm_f32x4 lds[];             // [KQ][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int roi = blockIdx.x / a.tiles, p0 = (blockIdx.x - roi * a.tiles) * DM_MLP_TP;
  const int np = min(DM_MLP_TP, a.P - p0);
  const int CT = C + a.NC;
  const float* xr = a.x + (size_t)roi * CT * a.P + p0;

  dm_mlp_stage(lds, xr, a.KQ, a.P, np, tid);
  __syncthreads();

  const int ci0 = NJ == 2 ? wave * NI : (wave >> 1);     // first channel tile of the wave
  const int pj0 = NJ == 2 ? 0 : (wave & 1);              // first point tile of the wave
  const int co_w = ci0 * 32;
#pragma unroll 1
  for (int L = 0; L <= a.nfc; ++L) {
    dm_f32x16 acc[NI][NJ];
    dm_mlp_gemm(acc, a.w[L], a.CoutP, a.KQ, lds, co_w, pj0, hi, l31);
    const float* bias = a.b[L];
    if (L < a.nfc) {
      dm_mlp_relu_store(acc, bias, lds, co_w, pj0, hi, l31);
    } else {
      // fc_logits: every output row into the stage features at the point's cell
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int p = (pj0 + j) * 32 + l31;
        if (p >= np) continue;
        const int cell = a.idx ? a.idx[(size_t)roi * a.P + p0 + p] : p0 + p;
        if (cell < 0 || cell >= a.HW) continue;
        float* dst = a.feat + (size_t)roi * C * a.HW + cell;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int co = co_w + i * 32 + dm_dtile_row(4 * g, hi);
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(size_t)(co + r) * a.HW] = acc[i][j][4 * g + r] + (bias ? bias[co + r] : 0.f);
          }
      }
    }
  }
}

size_t refine_mlp_lds_bytes(int C, int NC) { return (size_t)((C + NC) / 4) * DM_MLP_TP * 16; }

template <int C>
int launch_refine_mlp(const RefineMlpArgs& a, dm_stream_t stream) {
  // the LDS limit is raised once per device to what the widest accepted NC needs
  static bool raised[DM_MAX_DEVICES] = {false};
  const int rc = dm_ensure_lds_limit((const void*)point_refine_mlp_kernel<C>, (int)refine_mlp_lds_bytes(C, RMLP_MAXNC), raised);
  if (rc != DM_OK) return rc;
  DM_LAUNCH(point_refine_mlp_kernel<C>, dim3((unsigned)((long long)a.n * a.tiles)), dim3(DM_MLP_NT),
            (int)refine_mlp_lds_bytes(C, a.NC), (hipStream_t)stream, a);
  return dm_check_launch();
}

// ------------------------------------------------------------------------------------------------ scatter (rows)
__global__ void point_scatter_rows_kernel(const float* __restrict__ vals, const int* __restrict__ idx, long long total,
                                          int C, int P, float* __restrict__ map, int HW) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // over [n, C, P]
  if (g >= total) return;
  const long long rc = g / P;
  const int p = (int)(g - rc * P);
  const long long roi = rc / C;
  const int cell = idx[roi * P + p];
  if (cell >= 0 && cell < HW) map[rc * HW + cell] = vals[g];
}

}  // namespace

extern "C" int dm_point_topk_select_supported(int n, int HW, int P, int mode) {
  return (mode == 0 || mode == 1) && dm_point_select_supported(n, HW, P) ? 1 : 0;
}

extern "C" int dm_point_topk_select(const float* map, int n, int HW, int P, int mode, int* idx, dm_stream_t stream) {
  if (!dm_point_topk_select_supported(n, HW, P, mode)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!map || !idx) return DM_ERR_INVALID_ARG;
  if (mode == 1)
    DM_LAUNCH(point_select_kernel<SEL_DESC_SIGMOID>, dim3(n), dim3(SEL_NT), 0, (hipStream_t)stream, map, HW, P, idx);
  else
    DM_LAUNCH(point_select_kernel<SEL_DESC_RAW>, dim3(n), dim3(SEL_NT), 0, (hipStream_t)stream, map, HW, P, idx);
  return dm_check_launch();
}

extern "C" int dm_point_feat_gather_supported(int B, int C, int H, int W, int n, int NC, int P, int S, int has_idx) {
  if (B < 1 || C < GAT_CG || C % GAT_CG != 0 || H < 1 || W < 1 || n < 0) return 0;
  if (NC < GAT_CG || NC % GAT_CG != 0 || S < 1 || (long long)S * S > 0x7fffffffLL) return 0;
  if (P < 1 || (long long)P > (long long)S * S || (!has_idx && (long long)P != (long long)S * S)) return 0;
  if ((C + NC) / GAT_CG > 65535) return 0;
  return dm_ceil_div((long long)n * P, GAT_NT) <= 0x7fffffffLL ? 1 : 0;
}

extern "C" int dm_point_feat_gather(const float* feat, int B, int C, int H, int W, const float* rois, int n,
                                    const float* coarse, int NC, const int* idx, int P, int S, float spatial_scale,
                                    float* out, dm_stream_t stream) {
  if (!dm_point_feat_gather_supported(B, C, H, W, n, NC, P, S, idx ? 1 : 0)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!feat || !rois || !coarse || !out) return DM_ERR_INVALID_ARG;
  FeatGatherArgs a = {feat, B, C, H, W, rois, n, coarse, NC, idx, P, S, spatial_scale, out};
  const dim3 grid((unsigned)dm_ceil_div((long long)n * P, GAT_NT), (unsigned)((C + NC) / GAT_CG));
  DM_LAUNCH(point_feat_gather_kernel, grid, dim3(GAT_NT), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}

extern "C" int dm_point_refine_mlp_supported(int n, int P, int C, int NC, int num_fcs, int HW, int has_idx) {
  if (n < 0 || P < 1 || P > HW || (!has_idx && P != HW)) return 0;
  if (C != 64 && C != 128 && C != 256) return 0;
  if (NC < 8 || NC > RMLP_MAXNC || (C + NC) % 8 != 0 || num_fcs < 1 || num_fcs > RMLP_MAXFC) return 0;
  return (long long)n * dm_ceil_div(P, DM_MLP_TP) <= 0x7fffffffLL ? 1 : 0;
}

extern "C" int dm_point_refine_mlp(const float* x, int n, int P, int C, int NC, int num_fcs, const float* const* w_packed,
                                   const float* const* bias, const int* idx, int flags, float* feat, int HW,
                                   dm_stream_t stream) {
  const int fc = dm_flags_check(flags, 0);
  if (fc != DM_OK) return fc;
  if (!dm_point_refine_mlp_supported(n, P, C, NC, num_fcs, HW, idx ? 1 : 0)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!x || !w_packed || !feat) return DM_ERR_INVALID_ARG;
  RefineMlpArgs a = {};
  a.x = x; a.n = n; a.P = P; a.NC = NC; a.KQ = (C + NC) / 4; a.CoutP = dm_conv_packed_cout(C);
  a.nfc = num_fcs; a.tiles = dm_ceil_div(P, DM_MLP_TP);
  for (int L = 0; L <= num_fcs; ++L) {
    if (!w_packed[L]) return DM_ERR_INVALID_ARG;
    a.w[L] = w_packed[L];
    a.b[L] = bias ? bias[L] : nullptr;
  }
  a.idx = idx; a.feat = feat; a.HW = HW;
  if (C == 64) return launch_refine_mlp<64>(a, stream);
  if (C == 128) return launch_refine_mlp<128>(a, stream);
  return launch_refine_mlp<256>(a, stream);
}

extern "C" int dm_point_scatter_rows(const float* vals, const int* idx, int n, int C, int P, float* map, int HW,
                                     dm_stream_t stream) {
  if (n < 0 || C < 1 || P < 1 || P > HW) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!vals || !idx || !map) return DM_ERR_INVALID_ARG;
  const long long total = (long long)n * C * P;
  if ((total + 255) / 256 > 0x7fffffffLL) return DM_ERR_UNSUPPORTED;
  DM_LAUNCH(point_scatter_rows_kernel, dim3((unsigned)dm_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, vals,
            idx, total, C, P, map, HW);
  return dm_check_launch();
}
