// 3x3 convolution with a dilation d (1 <= d <= 8), stride 1, padding d ("same"), as an implicit GEMM on the fp32-input
// MFMA units of gfx950 (v_mfma_f32_32x32x2_f32: exact fp32 fma chain), for maps of any width.  It serves RefineMask
// (mmdet/models/roi_heads/mask_heads/refine_mask_head.py): the four 3x3 semantic_convs on the whole stride-4 FPN map
// (d = 1, 336 x 200 at 1333 x 800, 512 x 256 on Cityscapes) and the three dilated branches of MultiBranchFusion
// (d = 1, 3, 5 on 14^2 / 28^2 / 56^2 RoI maps).
//
// GEMM view and operand layout are conv_igemm.hip's (Out[co, pixel] = bias[co] + sum_k W[k, co] X[k, pixel], k = (tap,
// channel), channels in quads, one ds_read_b128 per operand feeds four MFMAs; the 32x32 D layout puts the pixel on the
// lane), and so is the weight layout: dm_conv_pack_weight(ksize 3, one source) -> [tap][KQ][CoutP][4].  What differs is
// the pixel tile.  conv_igemm.hip stages a plane of WHOLE rows (flat pixel runs plus a halo of one), which stops fitting
// its LDS from ~168 px of width on and cannot take a halo wider than one.  Here a workgroup's 128 pixels are a 2-D block
// of TH x TW = 8 x 16 pixels of ONE image (or RoI), and its LDS plane is that block plus a halo of d on every side:
// (8 + 2d) x (16 + 2d) positions, at most 24 x 32 = 768 at d = 8, whatever the map's width.  A tap (ky, kx) of
// dilation d reads the plane at offset (ky d) Pw + kx d (Pw = 16 + 2d): the dilation is a runtime value.
//
// Workgroup and K walk are mfma_tile.h's (which also holds the weight operand and the B register staging); each
// wave computes 32 WM couts x 64 pixels.  TM = 64 (WM = 1, maps of <= 64 couts) or 128 (WM = 2).
// LDS: A 9 x 2 x TM float4 (36 KiB at TM = 128) + B 2 x 768 float4 (24 KiB): 60 KiB per workgroup.
//
// NBR = 3 (dm_conv3x3_multidil_fwd): MultiBranchFusion's  sum_b relu(conv_{d_b}(x) + bias_b)  in one launch.  The branches
// run one after the other over the same tile (each stages its own plane, halo d_b); after branch b's K loop its
// accumulators go through bias + ReLU into a running sum in registers, then are cleared for the next branch.  The sum is
// formed as ((t_1 + t_2) + t_3), the order in which the unfused sequence (three dm_conv3x3_dil_fwd, the second and third
// with the "add into out" bit) adds: the fused and the unfused launches give the same bits.
#include "mfma_tile.h"

namespace {

constexpr int DIL_TH = 8, DIL_TW = 16;        // pixel block of a workgroup
constexpr int DIL_TN = DIL_TH * DIL_TW;       // 128
constexpr int DIL_MAXD = 8;
constexpr int DIL_PLANE_MAX = (DIL_TH + 2 * DIL_MAXD) * (DIL_TW + 2 * DIL_MAXD);   // 768
constexpr int DIL_MAXPOS = (DIL_PLANE_MAX + DM_CONV_NT - 1) / DM_CONV_NT;          // 3

// epilogue flags of the two entry points (dynamask_hip.h)
constexpr int DIL_RELU = 1;
constexpr int DIL_ADD = 4;

struct DilArgs {
  const float* x;
  int NB, C, H, W;
  const float* wq[3];
  const float* bias[3];
  int d[3];
  int nbr;
  int Cout, CoutP, KQ, MT;
  int tiles_x, tiles_y, ntiles;
  int flags;
  float* out;
};

template <int WM, int NBR>
__global__ __launch_bounds__(DM_CONV_NT) void conv3x3_dil_kernel(DilArgs a) {
  constexpr int TM = 2 * WM * 32;
  constexpr int WN = 2;
  using WT = dm_wtile<TM, DM_CONV_NQ, DM_CONV_NT>;
  __shared__ dm_f32x4 ldsA[WT::F4];
  __shared__ dm_f32x4 ldsB[DM_CONV_NQ * DIL_PLANE_MAX];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = wave >> 1;
  const int wave_n = wave & 1;
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  // XCD-aware order (conv_igemm.hip): the MT cout tiles of one pixel tile -- same input -- are 8 apart in launch order
  int m_tile, n_tile;
  {
    const int b = (int)blockIdx.x, gx = (int)gridDim.x, grp = 8 * a.MT;
    const int full = (gx / grp) * grp;
    if (b < full) {
      const int g = b / grp, r = b - g * grp;
      m_tile = r / 8;
      n_tile = g * 8 + (r & 7);
    } else {
      const int r = b - full;
      m_tile = r % a.MT;
      n_tile = full / a.MT + r / a.MT;
    }
  }
  const int m0 = m_tile * TM;
  const int per_img = a.tiles_x * a.tiles_y;
  const int n = n_tile / per_img;
  const int rem = n_tile - n * per_img;
  const int y0 = (rem / a.tiles_x) * DIL_TH;
  const int x0 = (rem % a.tiles_x) * DIL_TW;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const float* xn = a.x + (size_t)n * a.C * HW;

  // this lane's pixel of each of its WN column blocks
  int ty[WN], tx[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int p = (wave_n * WN + j) * 32 + l31;
    ty[j] = p / DIL_TW;
    tx[j] = p % DIL_TW;
  }

  dm_f32x16 acc[WM][WN];
  dm_f32x16 sum[NBR > 1 ? WM : 1][NBR > 1 ? WN : 1];
  const int co_wave = m0 + wave_m * WM * 32;

#pragma unroll 1
  for (int b = 0; b < NBR; ++b) {
    const int d = a.d[b];
    const int Pw = DIL_TW + 2 * d;
    const int plane = (DIL_TH + 2 * d) * Pw;
    const float* wq = a.wq[b];

    dm_acc_clear(acc);

    // B staging: thread -> plane positions tid + k * 256; its source pixel (or -1: halo outside the map)
    int st_off[DIL_MAXPOS];
#pragma unroll
    for (int k = 0; k < DIL_MAXPOS; ++k) {
      const int pos = tid + k * DM_CONV_NT;
      st_off[k] = -1;
      if (pos < plane) {
        const int py = pos / Pw, px = pos - (pos / Pw) * Pw;
        const int gy = y0 - d + py, gx = x0 - d + px;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) st_off[k] = gy * W + gx;
      }
    }
    int lane_base[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) lane_base[j] = ty[j] * Pw + tx[j] + hi * plane;

    dm_f32x4 ra[WT::PER_T];
    dm_f32x4 rb[DIL_MAXPOS * DM_CONV_NQ];
    auto prefetch = [&](int c0) {
      WT::fetch(ra, wq, c0 / 4, a.KQ, a.CoutP, m0, tid);
      const float* sp = xn + (size_t)c0 * HW;
#pragma unroll
      for (int k = 0; k < DIL_MAXPOS; ++k) dm_fetch_quads<DM_CONV_NQ>(rb + k * DM_CONV_NQ, sp, st_off[k], HW);
    };
    auto commit = [&]() {
      WT::commit(ldsA, ra, tid);
#pragma unroll
      for (int k = 0; k < DIL_MAXPOS; ++k) {
        const int pos = tid + k * DM_CONV_NT;
        if (pos < plane) {
#pragma unroll
          for (int qd = 0; qd < DM_CONV_NQ; ++qd) ldsB[qd * plane + pos] = rb[k * DM_CONV_NQ + qd];
        }
      }
    };

    prefetch(0);
#pragma unroll 1
    for (int c0 = 0; c0 < a.C; c0 += DM_CONV_CK) {
      commit();
      __syncthreads();
      if (c0 + DM_CONV_CK < a.C) prefetch(c0 + DM_CONV_CK);
      // The nine taps, fragments double-buffered one tap ahead: mfma_tile.h's dm_nine_taps written out, the one block this
      // kernel does not share.  Routed through that function (or only its MFMA step through dm_mfma_quad) the compiler
      // issues this kernel's LDS reads later (waits of lgkmcnt 1 / 0 where this form has 3 / 1) and the 256 x 512 map
      // and the 64-cout RoI maps measure 0.3 .. 0.6 % slower.  A change to the loop goes into both.
      auto load_frag = [&](int tap, dm_f32x4* av, dm_f32x4* bv) {
        const int tapoff = (tap / 3) * d * Pw + (tap % 3) * d;
#pragma unroll
        for (int i = 0; i < WM; ++i) av[i] = ldsA[(tap * DM_CONV_NQ + hi) * TM + (wave_m * WM + i) * 32 + l31];
#pragma unroll
        for (int j = 0; j < WN; ++j) bv[j] = ldsB[lane_base[j] + tapoff];
      };
      dm_f32x4 av[2][WM], bv[2][WN];
      load_frag(0, av[0], bv[0]);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int cur = tap & 1;
        if (tap + 1 < 9) load_frag(tap + 1, av[cur ^ 1], bv[cur ^ 1]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i][e], bv[cur][j][e], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }

    if (NBR > 1) {
      // bias + ReLU of this branch into the running sum (the first branch initialises it: no "0 + t")
      const float* bias = a.bias[b];
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = min(co_wave + i * 32 + dm_dtile_row(r, hi), a.Cout - 1);
          const float bv_ = bias ? bias[co] : 0.f;
#pragma unroll
          for (int j = 0; j < WN; ++j) {
            float t = acc[i][j][r] + bv_;
            if (a.flags & DIL_RELU) t = dm_relu(t);
            if (b == 0) sum[NBR > 1 ? i : 0][NBR > 1 ? j : 0][r] = t;
            else sum[NBR > 1 ? i : 0][NBR > 1 ? j : 0][r] += t;
          }
        }
    }
  }

  // ---- epilogue: every store is guarded (pixel inside the map, cout < Cout)
  const bool relu = (a.flags & DIL_RELU) != 0, add = (a.flags & DIL_ADD) != 0;
  float* on = a.out + (size_t)n * a.Cout * HW;
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co_wave + i * 32 + dm_dtile_row(r, hi);
      if (co >= a.Cout) continue;
      const float bv_ = (NBR == 1 && a.bias[0]) ? a.bias[0][co] : 0.f;
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        const int y = y0 + ty[j], x = x0 + tx[j];
        if (y >= H || x >= W) continue;
        float v;
        if (NBR == 1) {
          v = acc[i][j][r] + bv_;
          if (relu) v = dm_relu(v);
        } else {
          v = sum[NBR > 1 ? i : 0][NBR > 1 ? j : 0][r];
        }
        float* op = on + (size_t)co * HW + (size_t)y * W + x;
        if (add) v = *op + v;
        *op = v;
      }
    }
}

__global__ void sigmoid_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = dm_sigmoid(x[i]);
}

bool dil_shape_ok(int NB, int C, int H, int W, int Cout) {
  if (!dm_conv3x3_shape_ok(NB, C, H, W, Cout)) return false;
  const long long tiles = (long long)NB * dm_ceil_div(H, DIL_TH) * dm_ceil_div(W, DIL_TW);
  return tiles * dm_cout_tiles(Cout) <= 0x7fffffffLL;
}

int run_dil(DilArgs& a, hipStream_t st) {
  a.CoutP = dm_conv_packed_cout(a.Cout);
  a.KQ = a.C / 4;
  a.tiles_x = dm_ceil_div(a.W, DIL_TW);
  a.tiles_y = dm_ceil_div(a.H, DIL_TH);
  a.ntiles = a.NB * a.tiles_x * a.tiles_y;
  const bool narrow = a.Cout <= 64;
  a.MT = dm_cout_tiles(a.Cout);
  const dim3 grid((unsigned)((long long)a.MT * a.ntiles)), block(DM_CONV_NT);
  if (a.nbr == 1) {
    if (narrow) DM_LAUNCH((conv3x3_dil_kernel<1, 1>), grid, block, 0, st, a);
    else DM_LAUNCH((conv3x3_dil_kernel<2, 1>), grid, block, 0, st, a);
  } else {
    if (narrow) DM_LAUNCH((conv3x3_dil_kernel<1, 3>), grid, block, 0, st, a);
    else DM_LAUNCH((conv3x3_dil_kernel<2, 3>), grid, block, 0, st, a);
  }
  return dm_check_launch();
}

}  // namespace

extern "C" int dm_conv3x3_dil_supported(int NB, int C, int H, int W, int Cout, int dilation) {
  return (dil_shape_ok(NB, C, H, W, Cout) && dilation >= 1 && dilation <= DIL_MAXD) ? 1 : 0;
}

extern "C" int dm_conv3x3_dil_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                                  int Cout, int dilation, int flags, float* out, dm_stream_t stream) {
  if (!x || !w_packed || !out) return DM_ERR_INVALID_ARG;
  const int fc = dm_flags_check(flags, DIL_RELU | DIL_ADD);   // (bit 1, dm_conv2d_fwd's add-before-ReLU, is not one)
  if (fc != DM_OK) return fc;
  if (!dm_conv3x3_dil_supported(NB, C, H, W, Cout, dilation)) return DM_ERR_UNSUPPORTED;
  DilArgs a = {};
  a.x = x; a.NB = NB; a.C = C; a.H = H; a.W = W;
  a.wq[0] = w_packed; a.bias[0] = bias; a.d[0] = dilation; a.nbr = 1;
  a.Cout = Cout; a.flags = flags; a.out = out;
  return run_dil(a, (hipStream_t)stream);
}

extern "C" int dm_conv3x3_multidil_supported(int NB, int C, int H, int W, int Cout, int num_branches, const int* dilations) {
  if (num_branches != 3 || !dilations || !dil_shape_ok(NB, C, H, W, Cout)) return 0;
  for (int b = 0; b < 3; ++b)
    if (dilations[b] < 1 || dilations[b] > DIL_MAXD) return 0;
  return 1;
}

extern "C" int dm_conv3x3_multidil_fwd(const float* x, int NB, int C, int H, int W, const float* const* w_packed,
                                       const float* const* bias, int Cout, int num_branches, const int* dilations, int flags,
                                       float* out, dm_stream_t stream) {
  if (!x || !w_packed || !out || !dilations) return DM_ERR_INVALID_ARG;
  const int fc = dm_flags_check(flags, DIL_RELU | DIL_ADD);   // (bit 1, dm_conv2d_fwd's add-before-ReLU, is not one)
  if (fc != DM_OK) return fc;
  if (!dm_conv3x3_multidil_supported(NB, C, H, W, Cout, num_branches, dilations)) return DM_ERR_UNSUPPORTED;
  DilArgs a = {};
  a.x = x; a.NB = NB; a.C = C; a.H = H; a.W = W;
  for (int b = 0; b < 3; ++b) {
    if (!w_packed[b]) return DM_ERR_INVALID_ARG;
    a.wq[b] = w_packed[b];
    a.bias[b] = bias ? bias[b] : nullptr;
    a.d[b] = dilations[b];
  }
  a.nbr = 3;
  a.Cout = Cout; a.flags = flags; a.out = out;
  return run_dil(a, (hipStream_t)stream);
}

extern "C" int dm_sigmoid_fwd(const float* x, long long n, float* out, dm_stream_t stream) {
  if (n < 0 || (n > 0 && (!x || !out))) return DM_ERR_INVALID_ARG;
  if (n == 0) return DM_OK;
  DM_LAUNCH(sigmoid_kernel, dim3(dm_grid_1d(n, 4096)), dim3(256), 0, (hipStream_t)stream, x, n, out);
  return dm_check_launch();
}
