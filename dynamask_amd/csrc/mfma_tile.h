// The fp32 MFMA tile code shared by conv_dilated.hip, conv_strided.hip and point_refine.hip (v_mfma_f32_32x32x2_f32: an
// exact fp32 fma chain, so the ORDER of the MFMAs below is part of every result's bits: it is written here, once).
// Operands come in channel quads: one float4 per lane (lane half hi = lane >> 5 takes quad q0 + hi of a pair of quads)
// feeds four MFMAs.  The 32x32 D tile puts the column (pixel / point) on the lane and 16 rows (couts) in the registers.
#pragma once
#include "common.h"

// row of acc[r] in a 32x32 D tile for lane half hi; rows 4g .. 4g + 3 (r = 4g ..) are consecutive
__device__ __forceinline__ int dm_dtile_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

template <int NI, int NJ>
__device__ __forceinline__ void dm_acc_clear(dm_f32x16 (&acc)[NI][NJ]) {
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// one pair of quads into NI x NJ tiles: element e outermost (the fma chain of a tile is e = 0, 1, 2, 3 of every step)
template <int NI, int NJ>
__device__ __forceinline__ void dm_mfma_quad(dm_f32x16 (&acc)[NI][NJ], const dm_f32x4 (&av)[NI], const dm_f32x4 (&bv)[NJ]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ 3x3 convolutions
// Workgroup of the 3x3 kernels: 256 threads, 4 waves as 2 (couts) x 2 (pixels); K walked in chunks of 8 channels (a pair
// of quads): the next chunk's global loads go into registers before the MFMAs of the current one, into LDS after them.
constexpr int DM_CONV_NT = 256;
constexpr int DM_CONV_CK = 8;
constexpr int DM_CONV_NQ = DM_CONV_CK / 4;

// The A operand of a chunk: the [9 taps][NQ][TM couts] float4 image of dm_conv_pack_weight(ksize 3)'s
// [tap][KQ][CoutP][4] at couts m0 .. m0 + TM (zeros from CoutP on), staged by NT threads.
template <int TM, int NQ, int NT>
struct dm_wtile {
  static constexpr int F4 = 9 * NQ * TM;
  static constexpr int PER_T = (F4 + NT - 1) / NT;

  // the image of the chunk that starts at quad q0, into registers
  static __device__ __forceinline__ void fetch(dm_f32x4 (&ra)[PER_T], const float* wq, int q0, int KQ, int CoutP, int m0, int tid) {
    const float* abase = wq + (size_t)q0 * CoutP * 4;
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
      const int idx = tid + i * NT;
      const int m = idx % TM, tq = idx / TM;
      const int tap = tq / NQ, q = tq % NQ;
      dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < F4 && m0 + m < CoutP)
        v = *reinterpret_cast<const dm_f32x4*>(abase + (((size_t)tap * KQ + q) * CoutP + m0 + m) * 4);
      ra[i] = v;
    }
  }
  static __device__ __forceinline__ void commit(dm_f32x4* ldsA, const dm_f32x4 (&ra)[PER_T], int tid) {
#pragma unroll
    for (int i = 0; i < PER_T; ++i)
      if (F4 % NT == 0 || tid + i * NT < F4) ldsA[tid + i * NT] = ra[i];
  }
  // a tap's fragments of the NI cout tiles (of 32) from tile `tile0` on, for lane half hi and row l31 of a tile
  template <int NI>
  static __device__ __forceinline__ void frag(dm_f32x4 (&av)[NI], const dm_f32x4* ldsA, int tap, int hi, int tile0, int l31) {
#pragma unroll
    for (int i = 0; i < NI; ++i) av[i] = ldsA[(tap * NQ + hi) * TM + (tile0 + i) * 32 + l31];
  }
};

// B register staging: NQ quads of channels (plane stride HW) at base + off, or zeros when off < 0 (padding)
template <int NQ>
__device__ __forceinline__ void dm_fetch_quads(dm_f32x4* rb, const float* base, long long off, size_t HW) {
  if (off >= 0) {
    const float* gp = base + off;
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd)
#pragma unroll
      for (int e = 0; e < 4; ++e) rb[qd][e] = gp[(size_t)(qd * 4 + e) * HW];
  } else {
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) rb[qd] = dm_f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// The nine taps of one staged chunk, fragments double-buffered one tap ahead.  This lane's B fragment of pixel tile j
// is ldsB[b_lane[j] + b_tap(tap)]: the kernel's own image of its pixel tile (what the kernels differ in).
// conv_strided.hip runs this; conv_dilated.hip holds the same loop written out (it measures slower through here).
template <typename WT, int NI, int NJ, typename BTap>
__device__ __forceinline__ void dm_nine_taps(dm_f32x16 (&acc)[NI][NJ], const dm_f32x4* ldsA, const dm_f32x4* ldsB, int hi,
                                             int l31, int tile0, const int (&b_lane)[NJ], BTap b_tap) {
  auto load_frag = [&](int tap, dm_f32x4 (&av)[NI], dm_f32x4 (&bv)[NJ]) {
    const int tapoff = b_tap(tap);
    WT::template frag<NI>(av, ldsA, tap, hi, tile0, l31);
#pragma unroll
    for (int j = 0; j < NJ; ++j) bv[j] = ldsB[b_lane[j] + tapoff];
  };
  dm_f32x4 av[2][NI], bv[2][NJ];
  load_frag(0, av[0], bv[0]);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int cur = tap & 1;
    if (tap + 1 < 9) load_frag(tap + 1, av[cur ^ 1], bv[cur ^ 1]);
    dm_mfma_quad(acc, av[cur], bv[cur]);
  }
}

// ------------------------------------------------------------------------------------------------ point MLPs
// Workgroup of the point MLPs: 64 points of one RoI, 256 threads = 4 waves.  The activations live in the LDS as
// [KQ][64 points][4 channels]; a layer reads all of them, then (after a barrier) its outputs replace the first channels.
// The weights are dm_conv_pack_weight's 1x1 layout [KQ][CoutP][4], read straight from the L2 (shared by every
// workgroup): one float4 per lane feeds four MFMAs, the next pair of quads' float4s are in flight while the current
// pair's MFMAs run.  A wave owns NI channel tiles from channel co_w on x NJ point tiles from tile pj0 on.
constexpr int DM_MLP_TP = 64;
constexpr int DM_MLP_NT = 256;

// x [.., P] channel-major, np valid points -> the activation image (zeros for the points past np)
__device__ __forceinline__ void dm_mlp_stage(dm_f32x4* lds, const float* xr, int KQ, int P, int np, int tid) {
  for (int e = tid; e < KQ * DM_MLP_TP; e += DM_MLP_NT) {
    const int q = e / DM_MLP_TP, p = e - q * DM_MLP_TP;
    dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < np) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = xr[(size_t)(4 * q + j) * P + p];
    }
    lds[e] = v;
  }
}

// acc = W [rows co_w ..] x activations: cleared, then every pair of quads in order
template <int NI, int NJ>
__device__ __forceinline__ void dm_mlp_gemm(dm_f32x16 (&acc)[NI][NJ], const float* w, int CoutP, int KQ, const dm_f32x4* lds,
                                            int co_w, int pj0, int hi, int l31) {
  dm_acc_clear(acc);
  const dm_f32x4* wq = reinterpret_cast<const dm_f32x4*>(w) + co_w + l31;
  dm_f32x4 av[NI], an[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) av[i] = wq[(size_t)hi * CoutP + i * 32];
#pragma unroll 1
  for (int q0 = 0; q0 < KQ; q0 += 2) {
    const int qn = q0 + 2 < KQ ? q0 + 2 : q0;
#pragma unroll
    for (int i = 0; i < NI; ++i) an[i] = wq[(size_t)(qn + hi) * CoutP + i * 32];
    dm_f32x4 bv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bv[j] = lds[(q0 + hi) * DM_MLP_TP + (pj0 + j) * 32 + l31];
    dm_mfma_quad(acc, av, bv);
#pragma unroll
    for (int i = 0; i < NI; ++i) av[i] = an[i];
  }
}

// a hidden layer's end: relu(acc + bias) over the layer's input, between two barriers
template <int NI, int NJ>
__device__ __forceinline__ void dm_mlp_relu_store(const dm_f32x16 (&acc)[NI][NJ], const float* bias, dm_f32x4* lds, int co_w,
                                                  int pj0, int hi, int l31) {
  __syncthreads();                             // every wave has read this layer's input
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = co_w + i * 32 + dm_dtile_row(4 * g, hi);     // rows co .. co + 3 of D, quad co / 4
      dm_f32x4 bq = {0.f, 0.f, 0.f, 0.f};
      if (bias) bq = *reinterpret_cast<const dm_f32x4*>(bias + co);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        dm_f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = dm_relu(acc[i][j][4 * g + r] + bq[r]);
        lds[(co / 4) * DM_MLP_TP + (pj0 + j) * 32 + l31] = v;
      }
    }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ host side
// cout tiles of a 3x3 launch: TM = 64 for maps of <= 64 couts, else 128
static inline int dm_cout_tiles(int Cout) { return dm_ceil_div(dm_conv_packed_cout(Cout), Cout <= 64 ? 64 : 128); }

static inline bool dm_conv3x3_shape_ok(int NB, int C, int H, int W, int Cout) {
  return NB >= 1 && C >= DM_CONV_CK && C % DM_CONV_CK == 0 && H >= 1 && W >= 1 && Cout >= 1;
}

// The flag word of these exact-fp32 entry points: bit 4 (bf16x3) is not served, bit 3 (dm_conv2d_fwd's scheduling hint)
// is accepted and ignored, any other bit outside `accepted` is an error.
static inline int dm_flags_check(int flags, int accepted) {
  if (flags & 16) return DM_ERR_UNSUPPORTED;
  if (flags & ~(accepted | 8)) return DM_ERR_INVALID_ARG;
  return DM_OK;
}

// blocks of 256 threads of a grid-stride launch over `total` elements
static inline int dm_grid_1d(long long total, int cap) { return (int)(total / 256 + 1 < cap ? total / 256 + 1 : cap); }
