// K8: deformable convolution v1 (3x3, stride 1, pad 1, dilation 1, groups 1, no
// bias), forward.  Arithmetic spec: mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu
// :84-115 (bilinear) and :190-243 (im2col) of the reference tree; the reference
// materialises the [C*9, N*H*W] column matrix in HBM and calls a library GEMM
// (deform_conv_cuda.cpp:198-237).  Here the deformable im2col is the PRODUCER
// of the MFMA B operand: a workgroup owns TN flat pixels x (up to 256) output
// channels, gathers the bilinear-sampled columns of 8 input channels and feeds
// them to v_mfma_f32_32x32x2_f32 through LDS.  The column matrix never exists
// in HBM, and since one workgroup covers every output channel (C <= 256) each
// sample is gathered exactly once.
//
// Same software pipeline and quad K-ordering as conv_igemm.hip: the gather of
// chunk c+1 (4 loads per sample, issued into registers) overlaps the 144 MFMAs
// per wave of chunk c; LDS images  A: [tap][quad][TM][4]  B: [quad][tap][TN][4].
//
// The 4 tap offsets + 4 bilinear weights of a (kernel tap, pixel) pair depend
// only on the deformable group, so each thread keeps them in registers for its
// (tap, pixel) pairs and reuses them for all C/deform_groups channels.
#include "common.h"

namespace {

struct DcnArgs {
  const float* x;
  const float* offset;
  int NB, C, H, W, HW, Q;
  const float* wp;  // [9][KQ][CoutP][4]
  int Cout, CoutP, KQ, dg, relu;
  int q_begin = 0;   // first flat pixel of this launch (Q is its end)
  float* out;
  int MT;
  // split-K (round 4, the <= 100-RoI inference calls): blockIdx.y = split, which walks channels [split * kchan, + kchan)
  // and stores bare sums to ws + split * ws_stride ([NB][Cout][HW]); dcn_splitk_reduce_kernel adds the splits in order
  float* ws = nullptr;
  long long ws_stride = 0, ws_floats = 0;
  int ksplit = 1, kchan = 0;
  // the 1x1 convolution behind the DCN, chained in the epilogue of the band kernel (round 6, dm_deform_conv_tout_fwd):
  // out2[m] = relu(b2[m] + sum_k w2[m][k] * relu(dcn[k])), w2t = [Cout][w2_ld] (transposed; w2_ld = M2 rounded up to 32);
  // store_out = 0: the DCN output itself is not written
  const float* w2t = nullptr;
  const float* b2 = nullptr;
  float* out2 = nullptr;
  int M2 = 0, w2_ld = 0, out2_ct = 0, store_out = 1;
};

// One bilinear sample from its two row pairs.  Spelled as an explicit fma chain so that every kernel
// variant rounds the same way (left to the compiler, the two gathers contracted differently and
// results differed in the last bit depending on which variant a launch size selected).
typedef float dm_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float dcn_bilinear(float wt0, float wt1, float wb0, float wb1, float ta, float tb, float ba, float bb) {
  return __builtin_fmaf(wb1, bb, __builtin_fmaf(wb0, ba, __builtin_fmaf(wt1, tb, wt0 * ta)));
}

template <int WGM, int WGN, int WM, int WN>
__global__ __launch_bounds__(WGM* WGN * 64) void deform_conv_kernel(DcnArgs a) {
  constexpr int CK = 8;
  constexpr int TM = WGM * WM * 32;
  constexpr int TN = WGN * WN * 32;
  constexpr int NT = WGM * WGN * 64;
  constexpr int TG = NT / TN;                 // thread groups sharing a pixel column
  constexpr int MAXT = (9 + TG - 1) / TG;     // taps owned per thread
  constexpr int A_F4 = 9 * 2 * TM;
  constexpr int A_PER_T = (A_F4 + NT - 1) / NT;
  static_assert(NT % TN == 0, "threads must tile the pixel columns");

  extern __shared__ __attribute__((aligned(16))) float lds[];
  // split-K: this workgroup's channel range and destination (see DcnArgs)
  const int kc_begin = (a.ksplit > 1) ? (int)blockIdx.y * a.kchan : 0;
  const int kc_end = (a.ksplit > 1) ? min(a.C, kc_begin + a.kchan) : a.C;
  float* const e_out = (a.ksplit > 1) ? a.ws + (size_t)blockIdx.y * a.ws_stride : a.out;
  const int e_relu = (a.ksplit > 1) ? 0 : a.relu;
  dm_f32x4* ldsA = reinterpret_cast<dm_f32x4*>(lds);           // [9][2][TM]
  dm_f32x4* ldsB = reinterpret_cast<dm_f32x4*>(lds) + A_F4;    // [2][9][TN]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wave_m = wave / WGN, wave_n = wave % WGN;
  const int hi = lane >> 5, l31 = lane & 31;
  // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own
  // L2), so the MT cout tiles of one pixel tile -- which read the same input -- are placed
  // 8 apart in launch order: same XCD, back to back.  The ragged tail keeps the plain order.
  int m_tile, n_tile;
  {
    const int b = blockIdx.x, grp = 8 * a.MT;
    const int full = (gridDim.x / grp) * grp;
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
  const int q0 = a.q_begin + n_tile * TN;
  const int HW = a.HW, W = a.W, H = a.H;

  // MFMA-side columns of this lane
  int col_n[WN], col_p[WN];
  bool col_ok[WN];
#pragma unroll
  for (int wn = 0; wn < WN; ++wn) {
    int q = q0 + (wave_n * WN + wn) * 32 + l31;
    col_ok[wn] = q < a.Q;
    q = min(q, a.Q - 1);
    col_n[wn] = q / HW;
    col_p[wn] = q - col_n[wn] * HW;
  }

  // gather-side column of this thread
  const int gj = tid % TN;
  const int tg = tid / TN;
  int gq = q0 + gj;
  const bool g_ok = gq < a.Q;
  gq = min(gq, a.Q - 1);
  const int gn = gq / HW;
  const int gp = gq - gn * HW;
  const int gy = gp / W, gx = gp - gy * W;

  // Per owned (tap, pixel): the 2x2 bilinear footprint as two 8-byte row pairs.
  // pair base column cb = clamp(w_low, 0, W-2); a tap that falls outside the
  // image keeps weight 0 (spec: deform_conv_cuda_kernel.cu:84-115), so the pair
  // loads stay in bounds and the products equal the reference's w1..w4 * v1..v4.
  int ot[MAXT], ob[MAXT];
  float wt0[MAXT], wt1[MAXT], wb0[MAXT], wb1[MAXT];
  int cur_group = -1;
  const int cpg = a.C / a.dg;

  auto load_params = [&](int group) {
    const float* offp = a.offset + ((size_t)gn * a.dg + group) * 18 * HW + gp;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int tap = tg + t * TG;
      ot[t] = ob[t] = 0;
      wt0[t] = wt1[t] = wb0[t] = wb1[t] = 0.f;
      if (tap < 9 && g_ok) {
        const int ki = tap / 3, kj = tap - ki * 3;
        const float off_h = offp[(size_t)(2 * tap) * HW];
        const float off_w = offp[(size_t)(2 * tap + 1) * HW];
        const float h_im = (float)(gy - 1 + ki) + off_h;
        const float w_im = (float)(gx - 1 + kj) + off_w;
        if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
          const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
          const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
          const float hh = 1.f - lh, hw = 1.f - lw;
          const float wr_t = (h_low >= 0) ? hh : 0.f;
          const float wr_b = (h_low + 1 <= H - 1) ? lh : 0.f;
          const int rt = min(max(h_low, 0), H - 1), rbm = min(max(h_low + 1, 0), H - 1);
          const int cb = min(max(w_low, 0), W - 2);
          const float wc0 = (cb == w_low ? hw : 0.f) + (cb == w_low + 1 ? lw : 0.f);
          const float wc1 = (cb + 1 == w_low ? hw : 0.f) + (cb + 1 == w_low + 1 ? lw : 0.f);
          ot[t] = rt * W + cb;
          ob[t] = rbm * W + cb;
          wt0[t] = wr_t * wc0; wt1[t] = wr_t * wc1;
          wb0[t] = wr_b * wc0; wb1[t] = wr_b * wc1;
        }
      }
    }
  };

  dm_f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  struct __attribute__((packed, aligned(4))) F2 { float a, b; };
  dm_f32x4 ra[A_PER_T];       // next chunk's weights
  dm_f32x4 raw[MAXT * 4];     // raw row pairs of ONE channel quad of the next chunk (in flight)
  dm_f32x4 rb0[MAXT];         // combined quad 0 of the next chunk

  auto prefetch_a = [&](int c0) {
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int idx = tid + i * NT;
      dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < A_F4) {
        const int m = idx % TM;
        const int tq = idx / TM;
        const int qd = tq & 1;
        const int tap = tq >> 1;
        if (m0 + m < a.CoutP)
          v = *reinterpret_cast<const dm_f32x4*>(a.wp + (((size_t)tap * a.KQ + (c0 >> 2) + qd) * a.CoutP + m0 + m) * 4);
      }
      ra[i] = v;
    }
  };
  auto issue_quad = [&](int c0, int qd) {   // 2 x 8-byte loads per sample, nothing waits on them here
    const float* xp = a.x + ((size_t)gn * a.C + c0 + qd * 4) * HW;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* xc = xp + (size_t)e * HW;
        const F2 top = *reinterpret_cast<const F2*>(xc + ot[t]);
        const F2 bot = *reinterpret_cast<const F2*>(xc + ob[t]);
        dm_f32x4 v = {top.a, top.b, bot.a, bot.b};
        raw[t * 4 + e] = v;
      }
    }
  };
  auto combine = [&](int t) {
    dm_f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const dm_f32x4 l = raw[t * 4 + e];
      v[e] = dcn_bilinear(wt0[t], wt1[t], wb0[t], wb1[t], l[0], l[1], l[2], l[3]);
    }
    return v;
  };
  auto commit = [&]() {   // A registers + both B quads -> LDS (quad 1 is combined here)
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int idx = tid + i * NT;
      if (idx < A_F4) ldsA[idx] = ra[i];
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int tap = tg + t * TG;
      if (tap < 9) {
        ldsB[(0 * 9 + tap) * TN + gj] = rb0[t];
        ldsB[(1 * 9 + tap) * TN + gj] = combine(t);
      }
    }
  };
  // operand fragments double-buffered in registers (see conv_igemm.hip)
  auto load_frag = [&](int tap, dm_f32x4* av, dm_f32x4* bv) {
#pragma unroll
    for (int i = 0; i < WM; ++i) av[i] = ldsA[(tap * 2 + hi) * TM + (wave_m * WM + i) * 32 + l31];
#pragma unroll
    for (int j = 0; j < WN; ++j) bv[j] = ldsB[(hi * 9 + tap) * TN + (wave_n * WN + j) * 32 + l31];
  };
  auto mfma_taps = [&](int t0, int t1) {
    dm_f32x4 av[2][WM], bv[2][WN];
    load_frag(t0, av[0], bv[0]);
#pragma unroll
    for (int tap = t0; tap < t1; ++tap) {
      const int cur = (tap - t0) & 1;
      if (tap + 1 < t1) load_frag(tap + 1, av[cur ^ 1], bv[cur ^ 1]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int j = 0; j < WN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i][e], bv[cur][j][e], acc[i][j], 0, 0, 0);
    }
  };

  // prologue: chunk 0 entirely in registers
  cur_group = kc_begin / cpg;
  load_params(cur_group);
  prefetch_a(kc_begin);
  issue_quad(kc_begin, 0);
#pragma unroll
  for (int t = 0; t < MAXT; ++t) rb0[t] = combine(t);
  issue_quad(kc_begin, 1);

  for (int c0 = kc_begin; c0 < kc_end; c0 += CK) {
    commit();
    __syncthreads();
    const int cn = c0 + CK;
    const bool more = cn < kc_end;
    if (more) {
      const int group = cn / cpg;    // CK divides cpg (checked on the host)
      if (group != cur_group) {
        cur_group = group;
        load_params(group);
      }
      prefetch_a(cn);
      issue_quad(cn, 0);             // in flight under taps 0..3
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_taps(0, 4);
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int t = 0; t < MAXT; ++t) rb0[t] = combine(t);
      issue_quad(cn, 1);             // in flight under taps 4..8, combined at commit()
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_taps(4, 9);
    __syncthreads();
  }

  // epilogue with hoisted addresses (one base per pixel column, one per-lane channel offset; see conv_igemm.hip)
  {
    float* pj[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) pj[j] = e_out + (size_t)col_n[j] * a.Cout * HW + col_p[j];
    const int co_lane = m0 + wave_m * WM * 32 + 4 * hi;
    const size_t off_lane = (size_t)co_lane * HW;
    const bool relu = e_relu != 0;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = i * 32 + (r & 3) + 8 * (r >> 2);
        if (co_lane + k < a.Cout) {
          const size_t o = off_lane + (size_t)k * HW;
#pragma unroll
          for (int j = 0; j < WN; ++j) {
            if (col_ok[j]) {
              float v = acc[i][j][r];
              if (relu) v = dm_relu(v);
              pj[j][o] = v;
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Variant for small maps (128 <= H*W <= 256, i.e. the 14x14 stage): 128 couts x 128 pixels per
// workgroup like the plain conv kernel.  What kept the kernel above at 128 x 64 is the register
// cost of gathering from global memory (the raw row pairs of the next chunk live in VGPRs under
// the MFMAs).  Here the 8 channels of the (at most two) images a pixel tile touches are
// staged in LDS per chunk and the bilinear gather reads LDS:
// short latency, so a tap's B operand is produced just in time, three taps ahead of its MFMAs.
// The staged layout is [image][channel quad][pixel] float4 (the conv kernel's B layout): a sample's corner is ONE
// 16-byte read for the four channels of the thread's quad -- four reads per tap.  (Round 2 kept whole planes and read
// every corner pair of every channel with a ds_read2_b32: 8 reads and ~20 register moves per tap; tools/micro/mfma_mix.hip
// prices 8 such reads next to 16 MFMAs at a third of the MFMAs' own time.)
//
// The K loop is a sequence of steps of 3 taps (3 steps per chunk of 8 channels).  Step s does the
// MFMAs of its 3 taps from ring slot s & 1 of the A (weights) and B (gathered pixels) images while
// it fills slot (s + 1) & 1 for the next step: B by the gather, A from registers loaded one step
// earlier.  The channel quads are double buffered by chunk; those of chunk c + 1 are loaded
// in step 0 of chunk c, stored in step 1, and first read by the gather of step 2.  One barrier per
// step, no phase without MFMAs.
__global__ __launch_bounds__(256, 2) void deform_conv_lds_kernel(DcnArgs a) {
  constexpr int TM = 128, TN = 128, NT = 256;
  constexpr int AS_F4 = 3 * 2 * TM;               // one A slot: [tap of the step][quad][cout] float4
  constexpr int BS_F4 = 3 * 2 * TN;               // one B slot: [tap of the step][quad][pixel] float4
  constexpr int A_PER_T = AS_F4 / NT;             // 3
  constexpr int X_PER_T = 4;                      // float4 per thread for 2 images x 8 planes (H*W <= 256)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // split-K: this workgroup's channel range and destination (see DcnArgs)
  const int kc_begin = (a.ksplit > 1) ? (int)blockIdx.y * a.kchan : 0;
  const int kc_end = (a.ksplit > 1) ? min(a.C, kc_begin + a.kchan) : a.C;
  float* const e_out = (a.ksplit > 1) ? a.ws + (size_t)blockIdx.y * a.ws_stride : a.out;
  const int e_relu = (a.ksplit > 1) ? 0 : a.relu;
  dm_f32x4* ldsA = reinterpret_cast<dm_f32x4*>(lds);                 // [2][AS_F4]
  dm_f32x4* ldsB = ldsA + 2 * AS_F4;                                 // [2][BS_F4]
  dm_f32x4* ldsX = ldsB + 2 * BS_F4;                                 // [2 buffers][2 image slots][2 quads][H*W] float4

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_m = wave >> 1, wave_n = wave & 1;
  const int hi = lane >> 5, l31 = lane & 31;
  int m_tile, n_tile;
  {
    const int b = blockIdx.x, grp = 8 * a.MT;
    const int full = (gridDim.x / grp) * grp;
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
  const int m0 = m_tile * TM, q0 = a.q_begin + n_tile * TN;
  const int HW = a.HW, W = a.W, H = a.H;
  const int n0 = q0 / HW;                          // first image of the tile; the tile touches n0 and n0 + 1 at most
  const int xbuf = 2 * 2 * HW;                     // float4 per staging buffer

  int col_n[2], col_p[2];
  bool col_ok[2];
#pragma unroll
  for (int wn = 0; wn < 2; ++wn) {
    int q = q0 + (wave_n * 2 + wn) * 32 + l31;
    col_ok[wn] = q < a.Q;
    q = min(q, a.Q - 1);
    col_n[wn] = q / HW;
    col_p[wn] = q - col_n[wn] * HW;
  }

  // gather role: pixel gj of the tile, channel quad gh of the chunk
  const int gj = tid & 127, gh = tid >> 7;
  int gq = q0 + gj;
  const bool g_ok = gq < a.Q;
  gq = min(gq, a.Q - 1);
  const int gn = gq / HW, gp = gq - gn * HW;
  const int gy = gp / W, gx = gp - gy * W;
  const int xbase = ((gn - n0) * 2 + gh) * HW;               // this thread's quad inside a staging buffer

  int otb[9];                                      // top | bottom << 16: offsets inside a plane (< 256)
  float wt0[9], wt1[9], wb0[9], wb1[9];
  const int cpg = a.C / a.dg;
  auto load_params = [&](int group) {
    const float* offp = a.offset + ((size_t)gn * a.dg + group) * 18 * HW + gp;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      otb[tap] = 0;
      wt0[tap] = wt1[tap] = wb0[tap] = wb1[tap] = 0.f;
      if (g_ok) {
        const int ki = tap / 3, kj = tap - ki * 3;
        const float h_im = (float)(gy - 1 + ki) + offp[(size_t)(2 * tap) * HW];
        const float w_im = (float)(gx - 1 + kj) + offp[(size_t)(2 * tap + 1) * HW];
        if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
          const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
          const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
          const float hh = 1.f - lh, hw = 1.f - lw;
          const float wr_t = (h_low >= 0) ? hh : 0.f;
          const float wr_b = (h_low + 1 <= H - 1) ? lh : 0.f;
          const int rt = min(max(h_low, 0), H - 1), rbm = min(max(h_low + 1, 0), H - 1);
          const int cb = min(max(w_low, 0), W - 2);
          const float wc0 = (cb == w_low ? hw : 0.f) + (cb == w_low + 1 ? lw : 0.f);
          const float wc1 = (cb + 1 == w_low ? hw : 0.f) + (cb + 1 == w_low + 1 ? lw : 0.f);
          otb[tap] = (rt * W + cb) | ((rbm * W + cb) << 16);
          wt0[tap] = wr_t * wc0; wt1[tap] = wr_t * wc1;
          wb0[tap] = wr_b * wc0; wb1[tap] = wr_b * wc1;
        }
      }
    }
  };

  dm_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  dm_f32x4 ra[A_PER_T], rx[X_PER_T];
  // staging slot i of this thread: (image slot, quad, pixel) = its place in a staging buffer; x_off = float offset of
  // the quad's first channel at that pixel, relative to (image n0, channel c0).  Slots past the staging buffer or past
  // the last image load an address that exists (slot 0 / the last image) and are not stored / never gathered from.
  int x_off[X_PER_T];
#pragma unroll
  for (int i = 0; i < X_PER_T; ++i) {
    const int idx = tid + i * NT;
    const int img = idx / (2 * HW), r = idx - img * 2 * HW;
    const int quad = r / HW, px = r - quad * HW;
    const int ii = (idx < 4 * HW) ? img : 0, qq = (idx < 4 * HW) ? quad : 0, pp = (idx < 4 * HW) ? px : 0;
    x_off[i] = ((min(n0 + ii, a.NB - 1) - n0) * a.C + qq * 4) * HW + pp;
  }
  // weights of taps 3g .. 3g+2, channels c0 .. c0+7
  auto load_a = [&](int c0, int g) {
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int idx = tid + i * NT;
      const int m = idx % TM, tq = idx / TM;       // tq = (tap of the step) * 2 + quad
      // (rows past CoutP: the last row again -- their products land in accumulator rows the epilogue never stores;
      // an unconditional load keeps exec-mask branches out of the loop)
      const int mm = min(m0 + m, a.CoutP - 1);
      ra[i] = *reinterpret_cast<const dm_f32x4*>(a.wp + (((size_t)(3 * g + (tq >> 1)) * a.KQ + (c0 >> 2) + (tq & 1)) * a.CoutP + mm) * 4);
    }
  };
  auto store_a = [&](int slot) {
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) ldsA[slot * AS_F4 + tid + i * NT] = ra[i];
  };
  auto load_x = [&](int c0) {                     // lanes = consecutive pixels: coalesced dword loads, as the conv kernel's B staging
    const float* xc = a.x + ((size_t)n0 * a.C + c0) * HW;
#pragma unroll
    for (int i = 0; i < X_PER_T; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) rx[i][e] = xc[x_off[i] + e * HW];
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < X_PER_T; ++i) {
      const int idx = tid + i * NT;
      if (idx < 4 * HW) ldsX[buf * xbuf + idx] = rx[i];
    }
  };
  auto gather3 = [&](int t0, int slot, int buf) {   // taps t0 .. t0+2 of the chunk in staging buffer buf -> B slot
    const dm_f32x4* xq = ldsX + buf * xbuf + xbase;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int tap = t0 + u;
      const dm_f32x4* pt = xq + (otb[tap] & 0xffff);
      const dm_f32x4* pb = xq + (otb[tap] >> 16);
      const dm_f32x4 tl = pt[0], tr = pt[1], bl = pb[0], br = pb[1];
      dm_f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = dcn_bilinear(wt0[tap], wt1[tap], wb0[tap], wb1[tap], tl[e], tr[e], bl[e], br[e]);
      ldsB[slot * BS_F4 + (u * 2 + gh) * TN + gj] = v;
    }
  };
  // One step: the MFMAs of 3 taps from ring slot ``slot``; if ``fill``, the gather of taps t0 .. t0+2 (staging buffer
  // ``gbuf``) into the other slot, one tap inside each MFMA cluster: the four corner reads are issued with the
  // cluster's operand reads, the fma chain and the 16-byte write sit in the middle of the cluster -- their LDS latency
  // passes under MFMAs of the same wave instead of in front of them (round 2 gathered all three taps, then ran the 48 MFMAs).
  auto step = [&](int slot, bool fill, int t0, int gbuf) {
    const dm_f32x4* xq = ldsX + gbuf * xbuf + xbase;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      dm_f32x4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = ldsA[slot * AS_F4 + (u * 2 + hi) * TM + (wave_m * 2 + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = ldsB[slot * BS_F4 + (u * 2 + hi) * TN + (wave_n * 2 + j) * 32 + l31];
      const int tap = t0 + u;
      dm_f32x4 tl, tr, bl, br;
      if (fill) {
        const dm_f32x4* pt = xq + (otb[tap] & 0xffff);
        const dm_f32x4* pb = xq + (otb[tap] >> 16);
        tl = pt[0]; tr = pt[1]; bl = pb[0]; br = pb[1];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (fill) {
        dm_f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = dcn_bilinear(wt0[tap], wt1[tap], wb0[tap], wb1[tap], tl[e], tr[e], bl[e], br[e]);
        ldsB[(slot ^ 1) * BS_F4 + (u * 2 + gh) * TN + gj] = v;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 2; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // prologue: planes of chunk 0, weights and gathered pixels of step 0, loads of step 1 in flight
  int cur_group = kc_begin / cpg;
  load_params(cur_group);
  load_x(kc_begin);
  load_a(kc_begin, 0);
  store_x(0);
  store_a(0);
  load_a(kc_begin, 1);
  __syncthreads();
  gather3(0, 0, 0);
  __syncthreads();
  int slot = 0;                                   // ring slot of the current step
  for (int c0 = kc_begin, buf = 0; c0 < kc_end; c0 += 8, buf ^= 1) {
    const int cn = c0 + 8;
    const bool more = cn < kc_end;
    // step 0: MFMAs of taps 0..2; fills taps 3..5
    if (more) load_x(cn);
    store_a(slot ^ 1);
    load_a(c0, 2);
    step(slot, true, 3, buf);
    __syncthreads();
    slot ^= 1;
    // step 1: MFMAs of taps 3..5; fills taps 6..8; the quads of the next chunk go to the other buffer
    store_a(slot ^ 1);
    if (more) {
      load_a(cn, 0);
      store_x(buf ^ 1);
    }
    step(slot, true, 6, buf);
    __syncthreads();
    slot ^= 1;
    // step 2: MFMAs of taps 6..8; fills taps 0..2 of the next chunk
    if (more) {
      const int group = cn / cpg;
      if (group != cur_group) {
        cur_group = group;
        load_params(group);
      }
      store_a(slot ^ 1);
      load_a(cn, 1);
    }
    step(slot, more, 0, buf ^ 1);
    __syncthreads();
    slot ^= 1;
  }

  {
    float* pj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) pj[j] = e_out + (size_t)col_n[j] * a.Cout * HW + col_p[j];
    const int co_lane = m0 + wave_m * 64 + 4 * hi;
    const size_t off_lane = (size_t)co_lane * HW;
    const bool relu = e_relu != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = i * 32 + (r & 3) + 8 * (r >> 2);
        if (co_lane + k < a.Cout) {
          const size_t o = off_lane + (size_t)k * HW;
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (col_ok[j]) {
              float v = acc[i][j][r];
              if (relu) v = dm_relu(v);
              pj[j][o] = v;
            }
        }
      }
  }
}

// ---------------------------------------------------------------------------
// The small-map kernel for 256 output channels: a workgroup owns ALL 256 couts of 64 flat pixels, so a sample is gathered
// once (the 128 x 128 kernel above gathers it twice, once in each of the two cout workgroups of a pixel tile), and the
// gather is the part of the non-MFMA instruction budget that bounds that kernel (tools/micro/mfma_mix.hip).  Still four
// waves and two workgroups per CU (the 8-wave 256 x 128 tile of docs/experiments/r05_dcn256.patch ran alone on its CU and
// lost in the two-stream step).  Wave w owns couts 64 w .. 64 w + 63 over all 64 pixels (2 x 2 blocks of 32 x 32), so a
// weight fragment is used by exactly one wave: it is not staged through LDS but read from the packed weights (L2 hits:
// 512 contiguous bytes per half-wave) straight into the registers the MFMAs read, one step ahead, into two register
// sets that alternate by step.  No A ring, none of its writes.
// B is the scheme of the kernel above: planes staged per chunk as [image][quad][pixel] float4, double buffered; a
// two-slot ring of 3-tap steps, one barrier per step.  The 384 quad-items of a step (3 taps x 2 quads x 64 pixels) are
// dealt over 256 threads as one whole item (tap 3 s + rb, rb = tid >> 7) plus one HALF item of the step's third tap
// (channels 2 rb, 2 rb + 1 of the quad: 8-byte corner reads, 8-byte write); a thread keeps the parameters of 6 taps.
// Same products in the same order, same fma chain: the same bits as every other variant.
__global__ __launch_bounds__(256, 2) void deform_conv_c256_kernel(DcnArgs a) {
  constexpr int TN = 64, NT = 256;
  constexpr int BS_F4 = 3 * 2 * TN;               // one B slot: [tap of the step][quad][pixel] float4
  constexpr int X_PER_T = 4;                      // float4 per thread for 2 images x 8 planes (H*W <= 256)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  dm_f32x4* ldsB = reinterpret_cast<dm_f32x4*>(lds);                 // [2][BS_F4]
  dm_f32x4* ldsX = ldsB + 2 * BS_F4;                                 // [2 buffers][2 image slots][2 quads][H*W] float4

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int q0 = a.q_begin + (int)blockIdx.x * TN;
  const int HW = a.HW, W = a.W, H = a.H;
  const int n0 = q0 / HW;                          // first image of the tile; the tile touches n0 and n0 + 1 at most
  const int xbuf = 2 * 2 * HW;                     // float4 per staging buffer

  // gather role: pixel gj of the tile, channel quad gh of the chunk; rb picks the whole item's tap and the half item's channels
  const int gj = tid & 63, gh = (tid >> 6) & 1, rb = tid >> 7;
  int gq = q0 + gj;
  const bool g_ok = gq < a.Q;
  gq = min(gq, a.Q - 1);
  const int gn = gq / HW, gp = gq - gn * HW;
  const int gy = gp / W, gx = gp - gy * W;
  const int xbase = ((gn - n0) * 2 + gh) * HW;               // this thread's quad inside a staging buffer

  // [step s][0: tap 3s + rb (whole item), 1: tap 3s + 2 (half item)]
  int otb[3][2];                                   // top | bottom << 16: offsets inside a plane (< 256)
  float wt0[3][2], wt1[3][2], wb0[3][2], wb1[3][2];
  const int cpg = a.C / a.dg;
  auto load_params = [&](int group) {
    const float* offp = a.offset + ((size_t)gn * a.dg + group) * 18 * HW + gp;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        otb[s][r] = 0;
        wt0[s][r] = wt1[s][r] = wb0[s][r] = wb1[s][r] = 0.f;
        if (g_ok) {
          const int ki = s, kj = r ? 2 : rb, tap = 3 * s + kj;
          const float h_im = (float)(gy - 1 + ki) + offp[(size_t)(2 * tap) * HW];
          const float w_im = (float)(gx - 1 + kj) + offp[(size_t)(2 * tap + 1) * HW];
          if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
            const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
            const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
            const float hh = 1.f - lh, hw = 1.f - lw;
            const float wr_t = (h_low >= 0) ? hh : 0.f;
            const float wr_b = (h_low + 1 <= H - 1) ? lh : 0.f;
            const int rt = min(max(h_low, 0), H - 1), rbm = min(max(h_low + 1, 0), H - 1);
            const int cb = min(max(w_low, 0), W - 2);
            const float wc0 = (cb == w_low ? hw : 0.f) + (cb == w_low + 1 ? lw : 0.f);
            const float wc1 = (cb + 1 == w_low ? hw : 0.f) + (cb + 1 == w_low + 1 ? lw : 0.f);
            otb[s][r] = (rt * W + cb) | ((rbm * W + cb) << 16);
            wt0[s][r] = wr_t * wc0; wt1[s][r] = wr_t * wc1;
            wb0[s][r] = wr_b * wc0; wb1[s][r] = wr_b * wc1;
          }
        }
      }
  };

  dm_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  dm_f32x4 rx[X_PER_T];
  // Global loads go through buffer descriptors: the lane's part of an address is one 32-bit register that never changes,
  // the chunk / tap part is scalar.  (With flat 64-bit addresses the compiler keeps a register pair per tap and row block
  // alive through the loop, and the kernel spills.)
  const __amdgpu_buffer_rsrc_t xsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x) + (size_t)n0 * a.C * HW, 0, min(2, a.NB - n0) * a.C * HW * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, 9 * a.KQ * a.CoutP * 16, 0x00020000);
  unsigned x_off[X_PER_T];                         // bytes; places as in deform_conv_lds_kernel
#pragma unroll
  for (int i = 0; i < X_PER_T; ++i) {
    const int idx = tid + i * NT;
    const int img = idx / (2 * HW), r = idx - img * 2 * HW;
    const int quad = r / HW, px = r - quad * HW;
    const int ii = (idx < 4 * HW) ? img : 0, qq = (idx < 4 * HW) ? quad : 0, pp = (idx < 4 * HW) ? px : 0;
    x_off[i] = 4u * (unsigned)(((min(n0 + ii, a.NB - 1) - n0) * a.C + qq * 4) * HW + pp);
  }
  // A: lane (l31, hi) holds, per tap, the float4 of channel quad 2 * (chunk) + hi of cout rows 64 w + 32 i + l31
  // (rows past CoutP: the last row again -- never stored; an unconditional load keeps exec-mask branches out of the loop)
  unsigned a_off[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) a_off[i] = 16u * (unsigned)(hi * a.CoutP + min(wave * 64 + i * 32 + l31, a.CoutP - 1));   // bytes
  const int a_quad = a.CoutP * 16, a_tap = a.KQ * a_quad;      // bytes per channel quad / per tap of the packed weights
  auto load_a1 = [&](dm_f32x4 (&dst)[6], int c0, int g, int u) {   // weights of tap 3g + u, channels c0 .. c0+7
    const int so = (3 * g + u) * a_tap + (c0 >> 2) * a_quad;
#pragma unroll
    for (int i = 0; i < 2; ++i) dst[u * 2 + i] = __builtin_bit_cast(dm_f32x4, __builtin_amdgcn_raw_buffer_load_b128(wsrc, a_off[i], so, 0));
  };
  auto load_x = [&](int c0) {                     // lanes = consecutive pixels: coalesced dword loads
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int so = (c0 + e) * HW * 4;
#pragma unroll
      for (int i = 0; i < X_PER_T; ++i) rx[i][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xsrc, x_off[i], so, 0));
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < X_PER_T; ++i) {
      const int idx = tid + i * NT;
      if (idx < 4 * HW) ldsX[buf * xbuf + idx] = rx[i];
    }
  };
  // the whole item of step s: tap 3s + rb, four channels; the half item: tap 3s + 2, channels 2 rb and 2 rb + 1
  auto whole_read = [&](const dm_f32x4* xq, int s, dm_f32x4& tl, dm_f32x4& tr, dm_f32x4& bl, dm_f32x4& br) {
    const dm_f32x4* pt = xq + (otb[s][0] & 0xffff);
    const dm_f32x4* pb = xq + (otb[s][0] >> 16);
    tl = pt[0]; tr = pt[1]; bl = pb[0]; br = pb[1];
  };
  auto whole_write = [&](int slot, int s, const dm_f32x4& tl, const dm_f32x4& tr, const dm_f32x4& bl, const dm_f32x4& br) {
    dm_f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = dcn_bilinear(wt0[s][0], wt1[s][0], wb0[s][0], wb1[s][0], tl[e], tr[e], bl[e], br[e]);
    ldsB[slot * BS_F4 + (rb * 2 + gh) * TN + gj] = v;
  };
  auto half_read = [&](const dm_f32x4* xq, int s, dm_f32x2& tl, dm_f32x2& tr, dm_f32x2& bl, dm_f32x2& br) {
    const dm_f32x2* pt = reinterpret_cast<const dm_f32x2*>(xq + (otb[s][1] & 0xffff)) + rb;
    const dm_f32x2* pb = reinterpret_cast<const dm_f32x2*>(xq + (otb[s][1] >> 16)) + rb;
    tl = pt[0]; tr = pt[2]; bl = pb[0]; br = pb[2];
  };
  auto half_write = [&](int slot, int s, const dm_f32x2& tl, const dm_f32x2& tr, const dm_f32x2& bl, const dm_f32x2& br) {
    dm_f32x2 v;
#pragma unroll
    for (int e = 0; e < 2; ++e) v[e] = dcn_bilinear(wt0[s][1], wt1[s][1], wb0[s][1], wb1[s][1], tl[e], tr[e], bl[e], br[e]);
    reinterpret_cast<dm_f32x2*>(&ldsB[slot * BS_F4 + (2 * 2 + gh) * TN + gj])[rb] = v;
  };
  // One step: the MFMAs of 3 taps, A from register set ``cur``, B from ring slot ``slot``.  If ``fill``, step ``sn``'s
  // items are gathered from staging buffer ``gbuf`` into the other slot (the whole item inside the first tap's MFMA
  // cluster, the half item inside the second's); if ``pre``, the weights of step (pc0, pg) are loaded into ``nxt``, one
  // tap's two float4 in front of each cluster.
  auto step = [&](const dm_f32x4 (&cur)[6], dm_f32x4 (&nxt)[6], int slot, bool fill, int sn, int gbuf, bool pre, int pc0, int pg) {
    const dm_f32x4* xq = ldsX + gbuf * xbuf + xbase;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      dm_f32x4 bv[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = ldsB[slot * BS_F4 + (u * 2 + hi) * TN + j * 32 + l31];
      dm_f32x4 tl, tr, bl, br;
      dm_f32x2 htl, htr, hbl, hbr;
      if (fill && u == 0) whole_read(xq, sn, tl, tr, bl, br);
      if (fill && u == 1) half_read(xq, sn, htl, htr, hbl, hbr);
      if (pre) load_a1(nxt, pc0, pg, u);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u * 2 + i][e], bv[j][e], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (fill && u == 0) whole_write(slot ^ 1, sn, tl, tr, bl, br);
      if (fill && u == 1) half_write(slot ^ 1, sn, htl, htr, hbl, hbr);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 2; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u * 2 + i][e], bv[j][e], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // One chunk of 8 channels.  On entry ``p`` holds (or has in flight) the weights of its step 0 and ring slot ``slot``
  // its gathered taps 0..2; on exit ``q`` and slot ^ 1 hold those of the next chunk: the caller swaps p and q.
  int cur_group = 0;
  auto chunk = [&](dm_f32x4 (&p)[6], dm_f32x4 (&q)[6], int c0, int buf, int slot) {
    const int cn = c0 + 8;
    const bool more = cn < a.C;
    // step 0: MFMAs of taps 0..2; fills taps 3..5
    if (more) load_x(cn);
    step(p, q, slot, true, 1, buf, true, c0, 1);
    __syncthreads();
    // step 1: MFMAs of taps 3..5; fills taps 6..8; the quads of the next chunk go to the other buffer
    if (more) store_x(buf ^ 1);
    step(q, p, slot ^ 1, true, 2, buf, true, c0, 2);
    __syncthreads();
    // step 2: MFMAs of taps 6..8; fills taps 0..2 of the next chunk
    if (more) {
      const int group = cn / cpg;
      if (group != cur_group) {
        cur_group = group;
        load_params(group);
      }
    }
    step(p, q, slot, more, 0, buf ^ 1, more, cn, 0);
    __syncthreads();
  };

  // prologue: planes of chunk 0, weights and gathered pixels of step 0
  dm_f32x4 a0[6], a1[6];
  load_params(0);
  load_x(0);
#pragma unroll
  for (int u = 0; u < 3; ++u) load_a1(a0, 0, 0, u);
  store_x(0);
  __syncthreads();
  {
    const dm_f32x4* xq = ldsX + xbase;
    dm_f32x4 tl, tr, bl, br;
    dm_f32x2 htl, htr, hbl, hbr;
    whole_read(xq, 0, tl, tr, bl, br);
    half_read(xq, 0, htl, htr, hbl, hbr);
    whole_write(0, 0, tl, tr, bl, br);
    half_write(0, 0, htl, htr, hbl, hbr);
  }
  __syncthreads();
  // (a chunk is three steps: the ring slot and the register set of step 0 both alternate from chunk to chunk)
  for (int c0 = 0; c0 < a.C; c0 += 16) {
    chunk(a0, a1, c0, 0, 0);
    if (c0 + 8 < a.C) chunk(a1, a0, c0 + 8, 1, 1);
  }

  {
    float* pj[2];
    bool col_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int q = q0 + j * 32 + l31;
      col_ok[j] = q < a.Q;
      q = min(q, a.Q - 1);
      const int n = q / HW;
      pj[j] = a.out + (size_t)n * a.Cout * HW + (q - n * HW);
    }
    const int co_lane = wave * 64 + 4 * hi;
    const size_t off_lane = (size_t)co_lane * HW;
    const bool relu = a.relu != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = i * 32 + (r & 3) + 8 * (r >> 2);
        if (co_lane + k < a.Cout) {
          const size_t o = off_lane + (size_t)k * HW;
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (col_ok[j]) {
              float v = acc[i][j][r];
              if (relu) v = dm_relu(v);
              pj[j][o] = v;
            }
        }
      }
  }
}

// ---------------------------------------------------------------------------
// Variant for the large maps (28 x 28, 56 x 56): the bilinear gather runs IN the wave that consumes it.
// What holds the kernel at the top to a third of the MFMA rate at 64 channels is the path of a sample:
// two 8-byte global loads (texture path, L2 hits), a combine, a 16-byte LDS write, and an LDS read back by
// every cout wave -- with 64 couts a sample feeds 128 flop.  Here a workgroup owns 128 pixels of ONE image
// and all couts; a wave owns 32 of those pixels and ALL cout tiles, so the B operand of an MFMA
// (lane = pixel, lane half = channel quad) is exactly what the lane itself can gather: four 16-byte LDS reads per tap from a
// band of the chunk's 8 channels, staged as [quad][pixel] float4 (BR rows around the tile's rows; a 128-pixel tile spans <= 4 rows of
// a 56-wide map, offsets of +-6 rows stay inside), one fma chain, and the value goes straight into WM
// MFMAs.  No B image in LDS, no texture-path gathers; a sample outside the band (rare: large offsets) is
// loaded from global memory by the lanes concerned.  Per chunk: A (weights) and the band are loaded into
// registers under the MFMAs of the previous chunk and stored to LDS between two barriers.
// Same products, same K order (chunk of 8 -> tap -> element -> quad) and the same fma chain as the kernels
// above: results do not depend on which variant a shape takes.
constexpr int DCN_NEAR_ROWS = 5;

template <int WM, int WGM, int XR>
__global__ __launch_bounds__(256, 2) void deform_conv_band_kernel(DcnArgs a, int tiles_per_img, int BR) {
  // WGM waves share a pixel column (each with WM of the cout tiles: 128 couts = 2 x 2 -- four tiles in one wave spill)
  constexpr int TM = WM * WGM * 32, TN = (4 / WGM) * 32, NT = 256;
  constexpr int A_F4 = 9 * 2 * TM;                       // float4 of one chunk's weights: [tap][quad][cout]
  constexpr int A_PER_T = (A_F4 + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // split-K: this workgroup's channel range and destination (see DcnArgs)
  const int kc_begin = (a.ksplit > 1) ? (int)blockIdx.y * a.kchan : 0;
  const int kc_end = (a.ksplit > 1) ? min(a.C, kc_begin + a.kchan) : a.C;
  float* const e_out = (a.ksplit > 1) ? a.ws + (size_t)blockIdx.y * a.ws_stride : a.out;
  const int e_relu = (a.ksplit > 1) ? 0 : a.relu;
  dm_f32x4* ldsA = reinterpret_cast<dm_f32x4*>(lds);
  dm_f32x4* ldsX = reinterpret_cast<dm_f32x4*>(lds) + A_F4;      // [2 quads][BR * W] float4: the 4 channels of a quad at a band pixel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int wave_m = wave % WGM, wave_n = wave / WGM;
  const int HW = a.HW, W = a.W, H = a.H;
  const int PS = BR * W, PS4 = PS >> 2;                  // W % 4 == 0 (host)
  const int n = blockIdx.x / tiles_per_img, tile = blockIdx.x - n * tiles_per_img;
  const int p0 = tile * TN;
  const int p_end = min(p0 + TN, HW);
  const int y_first = p0 / W, y_last = (p_end - 1) / W;
  const int band_y0 = min(max(y_first - (BR - (y_last - y_first + 1)) / 2, 0), H - BR);     // H >= BR (host)
  int gp = p0 + wave_n * 32 + l31;
  const bool g_ok = gp < HW;
  gp = min(gp, HW - 1);
  const int gy = gp / W, gx = gp - gy * W;

  int otb[9];                          // top | bottom << 16.  In band: offsets inside a band plane; else: inside the image plane (H * W < 65536, host)
  float wt0[9], wt1[9], wb0[9], wb1[9];
  unsigned oob = 0, any_oob = 0;       // taps of this lane / of any lane of the wave that leave the band
  const int cpg = a.C / a.dg;
  auto load_params = [&](int group) {
    const float* offp = a.offset + ((size_t)n * a.dg + group) * 18 * HW + gp;
    oob = 0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      otb[tap] = 0;
      wt0[tap] = wt1[tap] = wb0[tap] = wb1[tap] = 0.f;
      if (g_ok) {
        const int ki = tap / 3, kj = tap - ki * 3;
        const float h_im = (float)(gy - 1 + ki) + offp[(size_t)(2 * tap) * HW];
        const float w_im = (float)(gx - 1 + kj) + offp[(size_t)(2 * tap + 1) * HW];
        if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
          const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
          const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
          const float hh = 1.f - lh, hw = 1.f - lw;
          const float wr_t = (h_low >= 0) ? hh : 0.f;
          const float wr_b = (h_low + 1 <= H - 1) ? lh : 0.f;
          const int rt = min(max(h_low, 0), H - 1), rbm = min(max(h_low + 1, 0), H - 1);
          const int cb = min(max(w_low, 0), W - 2);
          const float wc0 = (cb == w_low ? hw : 0.f) + (cb == w_low + 1 ? lw : 0.f);
          const float wc1 = (cb + 1 == w_low ? hw : 0.f) + (cb + 1 == w_low + 1 ? lw : 0.f);
          if (rt >= gy - DCN_NEAR_ROWS && rbm <= gy + DCN_NEAR_ROWS) {     // inside the band of every tiling (host checks the pad)
            otb[tap] = ((rt - band_y0) * W + cb) | (((rbm - band_y0) * W + cb) << 16);
            wt0[tap] = wr_t * wc0; wt1[tap] = wr_t * wc1;
            wb0[tap] = wr_b * wc0; wb1[tap] = wr_b * wc1;
          } else {
            oob |= 1u << tap;          // weight 0 here; the sample is added by the slow pass of every chunk
          }
        }
      }
    }
    any_oob = 0;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
      if (__ballot((oob >> tap) & 1u) != 0ull) any_oob |= 1u << tap;
  };

  dm_f32x16 acc[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  dm_f32x4 ra[A_PER_T], rx[XR];        // XR * 256 float4 cover the 8 band planes (host)
  // weights: slot offsets fixed per thread (rows past CoutP and slots past the chunk repeat a row that exists: their products
  // land in accumulator rows that are never stored / their LDS slots are never written) -- no exec-mask branch per load
  unsigned a_off[A_PER_T];
#pragma unroll
  for (int i = 0; i < A_PER_T; ++i) {
    const int idx = min(tid + i * NT, A_F4 - 1);
    const int m = idx % TM, tq = idx / TM;               // tq = tap * 2 + quad
    a_off[i] = (unsigned)((((size_t)(tq >> 1) * a.KQ + (tq & 1)) * a.CoutP + min(m, a.CoutP - 1)) * 4);
  }
  auto load_a = [&](int c0) {
    const float* wb = a.wp + (size_t)(c0 >> 2) * a.CoutP * 4;
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) ra[i] = *reinterpret_cast<const dm_f32x4*>(wb + a_off[i]);
  };
  // staging slot i of this thread = (quad, band pixel) = idx / PS, idx % PS (two quads: one compare); the loads of a slot
  // are the quad's four channels at that pixel.  Slots past the band load slot 0 and are not stored.
  auto load_x = [&](int c0) {          // lanes = consecutive band pixels: coalesced dword loads, four channels per slot
    const float* xb = a.x + ((size_t)n * a.C + c0) * HW + (size_t)band_y0 * W;
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int idx = tid + i * NT;
      const int off = (idx < PS) ? idx : (idx < 2 * PS ? 4 * HW + idx - PS : 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) rx[i][e] = xb[off + e * HW];
    }
  };
  auto store_ax = [&]() {
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      const int idx = tid + i * NT;
      if (idx < A_F4) ldsA[idx] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const int idx = tid + i * NT;
      if (idx < 2 * PS) ldsX[idx] = rx[i];
    }
  };
  struct __attribute__((packed, aligned(4))) F2 { float a, b; };      // (the slow pass's global row pairs)

  int cur_group = kc_begin / cpg;
  load_params(cur_group);
  load_a(kc_begin);
  load_x(kc_begin);
  for (int c0 = kc_begin; c0 < kc_end; c0 += 8) {
    __syncthreads();                   // the previous chunk's operand reads are done
    store_ax();
    __syncthreads();
    const int cn = c0 + 8;
    if (cn < kc_end) {
      load_a(cn);
      load_x(cn);
    }
    const unsigned any_oob_s = __builtin_amdgcn_readfirstlane(any_oob);
    const dm_f32x4* pq = ldsX + hi * PS;                                    // this lane half's channel quad
    const float* gl = a.x + ((size_t)n * a.C + c0 + 4 * hi) * HW;          // the same channels in global memory
    // Nine taps: the four corners of a tap are four 16-byte reads for the quad's four channels (round 2 kept channel
    // planes: two ds_read2_b32 per sample, 72 reads per chunk and wave against 36).  Software-pipelined by one tap: the
    // four values of a tap are formed first, then the next tap's corners and weight fragments are issued and run under
    // this tap's 4 * WM MFMAs.
    // (the weight fragments are double-buffered where the registers allow: with four cout tiles per wave a second set
    // spills, and they are read behind the tap's MFMAs instead -- their latency passes under the next tap's fma chains)
    constexpr int AB = (WM < 4) ? 2 : 1;
    dm_f32x4 av[AB][WM];
    dm_f32x4 tl, tr, bl, br;
    auto issue_x = [&](int tap) {
      const dm_f32x4* pt = pq + (otb[tap] & 0xffff);
      const dm_f32x4* pb = pq + (otb[tap] >> 16);
      tl = pt[0]; tr = pt[1]; bl = pb[0]; br = pb[1];
    };
    auto issue_a = [&](int tap) {
#pragma unroll
      for (int i = 0; i < WM; ++i) av[tap % AB][i] = ldsA[(tap * 2 + hi) * TM + (wave_m * WM + i) * 32 + l31];
    };
    issue_x(0);
    issue_a(0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = dcn_bilinear(wt0[tap], wt1[tap], wb0[tap], wb1[tap], tl[e], tr[e], bl[e], br[e]);
      __builtin_amdgcn_sched_barrier(0);
      if (tap + 1 < 9) {
        issue_x(tap + 1);
        if (AB == 2) issue_a(tap + 1);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < WM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tap % AB][i][e], v[e], acc[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (AB == 1 && tap + 1 < 9) issue_a(tap + 1);
    }
    if (any_oob_s) {
      // Slow pass: taps that leave the band for some lane of this wave.  The lanes concerned recompute the tap
      // from the offsets and gather from global memory; the others contribute 0.  (Kept out of the loop above:
      // with the two sources in one place the compiler selects between the POINTERS and every sample becomes a
      // flat load, and a branch per tap keeps it from overlapping one tap's LDS reads with another's MFMAs.)
      const float* offp = a.offset + ((size_t)n * a.dg + cur_group) * 18 * HW + gp;
#pragma unroll 1
      for (int tap = 0; tap < 9; ++tap) {
        if (!((any_oob_s >> tap) & 1u)) continue;
        const bool mine = (oob >> tap) & 1u;
        float w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f;
        int g_t = 0, g_b = 0;
        if (mine) {
          const int ki = tap / 3, kj = tap - ki * 3;
          const float h_im = (float)(gy - 1 + ki) + offp[(size_t)(2 * tap) * HW];
          const float w_im = (float)(gx - 1 + kj) + offp[(size_t)(2 * tap + 1) * HW];
          const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
          const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
          const float hh = 1.f - lh, hw = 1.f - lw;
          const float wr_t = (h_low >= 0) ? hh : 0.f;
          const float wr_b = (h_low + 1 <= H - 1) ? lh : 0.f;
          const int rt = min(max(h_low, 0), H - 1), rbm = min(max(h_low + 1, 0), H - 1);
          const int cb = min(max(w_low, 0), W - 2);
          const float wc0 = (cb == w_low ? hw : 0.f) + (cb == w_low + 1 ? lw : 0.f);
          const float wc1 = (cb + 1 == w_low ? hw : 0.f) + (cb + 1 == w_low + 1 ? lw : 0.f);
          g_t = rt * W + cb;
          g_b = rbm * W + cb;
          w00 = wr_t * wc0; w01 = wr_t * wc1;
          w10 = wr_b * wc0; w11 = wr_b * wc1;
        }
        dm_f32x4 av[WM];
#pragma unroll
        for (int i = 0; i < WM; ++i) av[i] = ldsA[(tap * 2 + hi) * TM + (wave_m * WM + i) * 32 + l31];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float* gc = gl + (size_t)e * HW;
          const F2 top = *reinterpret_cast<const F2*>(gc + g_t);
          const F2 bot = *reinterpret_cast<const F2*>(gc + g_b);
          const float g = dcn_bilinear(w00, w01, w10, w11, top.a, top.b, bot.a, bot.b);
#pragma unroll
          for (int i = 0; i < WM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], g, acc[i], 0, 0, 0);
        }
      }
    }
    if (cn < kc_end) {
      const int group = cn / cpg;      // 8 divides cpg (host)
      if (group != cur_group) {
        cur_group = group;
        load_params(group);
      }
    }
  }
  // The 1x1 convolution + ReLU that follows the DCN in an SFM stage (fuse_transform_out, dynamask_head.py:117-121), chained
  // here while the DCN's 32 pixels x all couts are still in this wave's accumulators: the MFMA D layout IS a B operand --
  // register r of tile i holds dcn[k = i*32 + (r&3) + 8*(r>>2) + 4*hi][pixel = lane & 31], i.e. for the k pair (kb, kb + 4)
  // lanes 0-31 / 32-63 carry exactly B[k][n] of a 32x32x2 step -- so the second GEMM needs no LDS round trip for its
  // input, only its weights (staged transposed: lane = cout).  Walking i, r upward adds the products in the order
  // (0,4),(1,5),(2,6),(3,7),(8,12),... -- the order the 1x1 kernel of conv_igemm.hip uses (quad pairs of a 16-channel
  // chunk): the result has the bits of the two launches it replaces.  The DCN output is then never written (inference).
  if (WGM == 1 && a.w2t) {
    // MT2: the cout tiles of the 1x1 this build has room for (host: ceil(M2 / 32) <= MT2).  The rows of w2t are w2_ld =
    // roundup(M2, 32) floats, fewer than MT2 * 32 when M2 needs fewer tiles (128 channels, M2 <= 32): the staging and the
    // row stride follow w2_ld, and the tiles past M2 are skipped (a wave-uniform branch).
    constexpr int MT2 = (WM + 1) / 2;
    const int ld2 = a.w2_ld;
    __syncthreads();                           // every wave is done with the last chunk's operands in LDS
    {
      const dm_f32x4* src = reinterpret_cast<const dm_f32x4*>(a.w2t);
      dm_f32x4* dst = reinterpret_cast<dm_f32x4*>(lds);
      for (int idx = tid; idx < a.Cout * (ld2 / 4); idx += NT) dst[idx] = src[idx];
    }
    __syncthreads();
    const float* w2t = lds;
    dm_f32x16 acc2[MT2];
#pragma unroll
    for (int t = 0; t < MT2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[t][r] = 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kb = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float b = dm_relu(acc[i][r]);
#pragma unroll
        for (int t = 0; t < MT2; ++t)
          if (t * 32 < ld2) acc2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2t[kb * ld2 + t * 32 + l31], b, acc2[t], 0, 0, 0);
      }
    const int p = p0 + wave_n * 32 + l31;
    if (p < HW) {
      float* po2 = a.out2 + (size_t)n * a.out2_ct * HW + p;
#pragma unroll
      for (int t = 0; t < MT2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (co < a.M2) po2[(size_t)co * HW] = dm_relu(acc2[t][r] + a.b2[co]);
        }
    }
    if (!a.store_out) return;
  }
  // epilogue: lane = pixel column, registers walk the couts
  {
    const int p = p0 + wave_n * 32 + l31;
    if (p < HW) {
      float* po = e_out + (size_t)n * a.Cout * HW + p;
      const bool relu = e_relu != 0;
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = (wave_m * WM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (co < a.Cout) {
            float v = acc[i][r];
            if (relu) v = dm_relu(v);
            po[(size_t)co * HW] = v;
          }
        }
    }
  }
}

// out = relu?(sum over the splits, in index order) of a split-K launch (ws: [splits][NB * Cout * HW])
__global__ __launch_bounds__(256) void dcn_splitk_reduce_kernel(const float* __restrict__ ws, int splits, long long stride,
                                                               long long total, int relu, float* __restrict__ out) {
  // (total, stride: multiples of 4 floats, ws / out 16-byte aligned -- checked by dcn_finish_split, which otherwise passes v4 = 0
  // through the sign of ``splits``)
  const bool v4 = splits > 0;
  splits = v4 ? splits : -splits;
  if (v4) {
    const float4* ws4 = reinterpret_cast<const float4*>(ws);
    float4* out4 = reinterpret_cast<float4*>(out);
    const long long total4 = total >> 2, stride4 = stride >> 2;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total4; e += (long long)gridDim.x * blockDim.x) {
      float4 v = ws4[e];
      for (int s_ = 1; s_ < splits; ++s_) {
        const float4 w = ws4[(size_t)s_ * stride4 + e];
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
      }
      if (relu) { v.x = dm_relu(v.x); v.y = dm_relu(v.y); v.z = dm_relu(v.z); v.w = dm_relu(v.w); }
      out4[e] = v;
    }
    return;
  }
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    float v = ws[e];
    for (int s_ = 1; s_ < splits; ++s_) v += ws[(size_t)s_ * stride + e];
    out[e] = relu ? dm_relu(v) : v;
  }
}

// ---- host side: validate, route, emit ---------------------------------------------------------------------------------
// dcn_route decides everything about the launches of a call from numbers alone (no pointer, no HIP call); dcn_emit enqueues
// exactly what the route says; dm_deform_conv_plan reports the same value.  Every variant runs 4-wave workgroups, two per
// CU (8-wave tiles run alone on their CU and lose: 128 x 128 from global memory 1.81 vs 1.59 ms at 256 channels, 256 x 128
// from LDS -1 % in the two-stream step), so a launch has 2 x CUs slots per round.  Same products in the same order in every
// variant: results do not depend on the route (except by the association of the channel sums where the K loop is split).

enum { DCN_GENERIC = 0, DCN_LDS = 1, DCN_C256 = 2, DCN_BAND = 3 };      // DcnLaunch::kernel, as the header numbers them
constexpr int DCN_BAND_ROWS = 16;                                       // rows of the band kernel's LDS band

struct DcnCall {            // what a route depends on
  int NB, C, H, W, Cout, dg, flags;
  long long ws_floats;      // the caller's workspace (0: none)
  int M2;                   // > 0: the chained 1x1 of dm_deform_conv_tout_fwd
  int cus;
  bool seam;                // an underfull last round may go to a second launch (DM_DCN_TAIL, flag bit 3)
};

// One launch: the ints of dm_deform_conv_plan's record, in its order (the record's last int is DcnRoute::reduce)
struct DcnLaunch {
  int kernel, p[4], threads, MT, q_begin, Q, grid_x, grid_y, ksplit, kchan, lds_bytes;
};

struct DcnRoute {
  int rc = DM_OK;
  int count = 0;            // launches (0: NB = 0)
  DcnLaunch launch[DM_DCN_PLAN_MAX_LAUNCHES];
  bool reduce = false;      // launch[0] split its K loop: dcn_splitk_reduce_kernel follows
};

// Split-K for launch l of l.grid_x workgroups (a caller-owned workspace): a workgroup
// walks its chunks of 8 channels one after the other at ~3.5 us each whatever the RoI count (tools/small_n.py: dcn14 105-115 us
// for 32 chunks at 8-16 RoIs); S splits save (1 - 1/S) of that and cost a second launch that reads S and writes one copy of
// the output.  Sets l.ksplit / kchan / grid_y; l.ksplit stays 1 when it does not pay.
static void dcn_choose_split(const DcnCall& c, bool lds_tiles, DcnLaunch& l) {
  const long long wgs = l.grid_x, slots = 2LL * c.cus;
  if (c.ws_floats <= 0 || wgs <= 0) return;
  const int chunks = c.C / 8;
  const long long per = (long long)c.NB * c.Cout * (c.H * c.W);
  int S = 1;
  if (c.NB <= 24) {
    // a handful of RoIs: the cost model (13 % / 3 % on the full head at 8 / 16 RoIs)
    long long Smax = min(min(8LL, slots / wgs), (long long)chunks / 2);
    if (per > 0) Smax = min(Smax, c.ws_floats / per);
    const double chain_us = chunks * 3.5, out_mb = (double)per * 4e-6;
    double best = 8.0;
    for (int s_ = 2; s_ <= Smax; ++s_) {
      const double g = chain_us * (1.0 - 1.0 / s_) - (5.0 + (s_ + 1) * out_mb * 0.25);
      if (g > best) { best = g; S = s_; }
    }
  } else if (lds_tiles && wgs < slots && chunks >= 12 && per > 0 && c.ws_floats / per >= 3) {
    // 25 .. 128 RoIs of 14 x 14 on the 128 x 128 LDS kernel (round 5, tools/small_n.py with forced splits): the launch is
    // less than one round of workgroups, each walking 32 chunks alone on its CU -- three splits: 32 / 50 / 64 / 100 RoIs
    // 0.179 / 0.198 / 0.200 / 0.332 -> 0.157 / 0.138 / 0.197 / 0.248 ms (two: 0.177 / 0.181 / 0.183 / 0.279).  The band
    // kernels of the 28 x 28 / 56 x 56 stages gain <= 8 % or lose (56 x 56: 0.283 -> 0.346 at 100 RoIs): not split.
    S = 3;
  }
  if (S >= 2) {
    const int per_split = dm_ceil_div(chunks, S);
    l.kchan = per_split * 8;
    l.ksplit = l.grid_y = dm_ceil_div(chunks, per_split);
  }
}

// deform_conv_kernel<WGM, WGN, WM, WN> on the flat pixels [q_begin, Q): 32 WGM WM couts x 32 WGN WN pixels per workgroup
static DcnLaunch dcn_generic(int WGM, int WGN, int WM, int WN, int CoutP, int q_begin, int Q) {
  const int TM = WGM * WM * 32, TN = WGN * WN * 32, MT = dm_ceil_div(CoutP, TM);
  return {DCN_GENERIC, {WGM, WGN, WM, WN}, WGM * WGN * 64, MT, q_begin, Q, MT * dm_ceil_div(Q - q_begin, TN), 1, 1, 0,
          16 * (9 * 2 * TM + 2 * 9 * TN)};
}

// Large maps: the consuming wave gathers from an LDS band of 16 rows.  The 8 band planes of a chunk must fit the 7 float4 per
// thread of the widest staging build (W <= 56), and the rows a 128-pixel tile can span plus DCN_NEAR_ROWS each side the
// band.  Every launch size of an eligible shape takes this kernel (rows must not depend on the batch); which build
// <WM, WGM, XR> of it, this says too.  false: not a band map.
static bool dcn_band_build(const DcnCall& c, int& WM, int& WGM, int& XR) {
  if (c.W <= 0 || c.H < DCN_BAND_ROWS || (c.W & 3) != 0 || 8 * DCN_BAND_ROWS * c.W / 4 > 7 * 256 || c.Cout <= 32) return false;
  const int max_rows = (c.W - 1 + 128 + c.W - 1) / c.W;                     // rows a 128-pixel tile can span
  const long long HW = (long long)c.H * c.W;
  const int CoutP = dm_conv_packed_cout(c.Cout);
  if ((DCN_BAND_ROWS - max_rows) / 2 < DCN_NEAR_ROWS || HW <= 256 || HW >= 65536 || (CoutP != 64 && CoutP != 128)) return false;
  const bool narrow = 8 * DCN_BAND_ROWS * c.W / 4 <= 4 * 256;               // band planes fit 4 float4 per thread
  // a handful of RoIs (real inference): the launch is bound by the time of one workgroup -- one cout tile per
  // wave, the waves sharing a pixel column (2-4 x the workgroups, 1/2-1/4 of the K-loop time each; same bits)
  bool few = (long long)c.NB * dm_ceil_div(HW, 128) * 4 < (long long)c.cus * 3;
  // ... unless the caller brought a workspace: a workgroup's time is its number of chunks times a load round trip
  // (~3.5 us) whatever it computes per chunk, so the full layout (every cout of 128 pixels: one gather per sample, four
  // times the MFMAs per round trip) with the K loop split (dcn_choose_split's cost model, <= 24 RoIs) beats it:
  // 16 / 24 detections 0.5845 / 0.733 -> 0.578 / 0.712 ms (profiles/r06_infer_notes.txt (6))
  if (c.ws_floats > 0 && c.NB <= 24) few = false;
  XR = narrow ? 4 : 7;
  if (few) { WM = 1; WGM = CoutP / 32; }
  else if (CoutP == 128 && !narrow) { WM = 2; WGM = 2; }                    // two waves share a pixel column
  else { WM = CoutP / 32; WGM = 1; }                                        // a wave holds every cout of its 32 pixels
  return true;
}

// Small maps (14 x 14): the planes of two images fit in LDS beside the operand rings (deform_conv_lds_kernel, .._c256_kernel)
static bool dcn_lds_map(int HW) { return HW >= 128 && HW <= 256 && (HW & 3) == 0; }

// A handful of RoIs: launches that leave most of the chip idle are bound by the time of one workgroup, and 64 x 64 tiles
// give four times the workgroups of the 128 x 128 LDS kernel (14 x 14, 8 RoIs: 0.208 -> 0.108 ms, 32 RoIs: 0.213 -> 0.168 ms;
// from 64 RoIs on the big tiles win); same for the 128 x 64 tiles (28 x 28, 8 RoIs: 0.081 -> 0.056 ms)
static bool dcn_small_launch(const DcnCall& c, int CoutP, int Q) {
  return (long long)dm_ceil_div(CoutP, 128) * dm_ceil_div(Q, 128) * 20 <= (long long)c.cus * 9;
}

// Rounds (see conv_igemm.hip): r.launch[0] covers the batch in tiles of tile_px pixels, two workgroups per CU.  From one
// full round on, the pixels of a nearly empty last round go to a second launch with 64 x 64 tiles (same bits): 512 RoIs
// 1.24 -> 1.19 ms.  Only for small remainders (the 64 x 64 build is slower per pixel: at 0.5 of a round the split loses).
static void dcn_seam(const DcnCall& c, int CoutP, int tile_px, DcnRoute& r) {
  DcnLaunch& m = r.launch[0];
  const int slots = 2 * c.cus, full_rounds = m.grid_x / slots, rem = m.grid_x - full_rounds * slots;
  if (!(full_rounds >= 1 && rem > 0 && rem * 20 <= 3 * slots)) return;
  const int n_main = full_rounds * slots / m.MT, Q = m.Q;
  m.grid_x = m.MT * n_main;
  m.Q = n_main * tile_px;
  r.launch[r.count++] = dcn_generic(2, 2, 1, 1, CoutP, m.Q, Q);
}

static DcnRoute dcn_route(const DcnCall& c) {
  DcnRoute r;
  auto refuse = [&r](int rc) { r.rc = rc; return r; };
  if (c.flags & 16) return refuse(DM_ERR_UNSUPPORTED);      // (flag bit 4, the bf16x3 mode of dm_conv2d_fwd: the DCN stays exact fp32)
  int WM = 0, WGM = 0, XR = 0;
  if (c.M2 > 0) {
    // the chained 1x1 answers for its shape before its arguments: only the band build in which a wave holds every cout of
    // its pixels can chain it, and its weights ([Cout][32-padded M2]) must fit the LDS the kernel has
    if (c.NB == 0) return r;
    if (c.Cout != c.C || !dcn_band_build(c, WM, WGM, XR) || WGM != 1 || c.Cout != WM * 32 || dm_ceil_div(c.M2, 32) > (WM + 1) / 2)
      return refuse(DM_ERR_UNSUPPORTED);
  }
  if (c.NB < 0 || c.C <= 0 || c.H <= 0 || c.W <= 0 || c.Cout <= 0 || c.dg <= 0 || c.C % c.dg != 0) return refuse(DM_ERR_INVALID_ARG);
  if ((long long)c.NB * c.H * c.W > 0x7fffffffLL) return refuse(DM_ERR_INVALID_ARG);
  if ((c.C / c.dg) % 8 != 0) return refuse(DM_ERR_UNSUPPORTED);   // channel chunk must not straddle a deformable group
  if (c.W < 2) return refuse(DM_ERR_UNSUPPORTED);                 // the gather loads row pairs
  if (c.NB == 0) return r;
  const int HW = c.H * c.W, Q = c.NB * HW, CoutP = dm_conv_packed_cout(c.Cout);
  DcnLaunch& l = r.launch[0];
  r.count = 1;
  if (dcn_band_build(c, WM, WGM, XR)) {
    // 128 / WGM pixels per workgroup, tiles per image; operand rings + the 8 band planes.  (The chained 1x1 never splits: the
    // second GEMM needs the complete channel sums -- its call has no workspace.)
    l = {DCN_BAND, {WM, WGM, XR, 0}, 256, 1, 0, Q, c.NB * dm_ceil_div(HW, (4 / WGM) * 32), 1, 1, 0,
         16 * (9 * 2 * WM * WGM * 32) + 4 * 8 * DCN_BAND_ROWS * c.W};
    dcn_choose_split(c, false, l);
  } else if (c.Cout > 64 && dcn_lds_map(HW) && (c.ws_floats > 0 || !dcn_small_launch(c, CoutP, Q))) {
    // 128 couts x 128 pixels: A ring + B ring (2 x 3 taps x 2 quads x 128 float4 each) + 2 plane buffers of 2 images x 8
    // channels.  With a workspace this kernel takes the small launches too: its K loop split (up to 8 ways at <= 24 RoIs, 3
    // above) fills the chip faster than 64 x 64 tiles (round 6: the 16- / 32-detection inference calls 0.652 / 0.949 ->
    // 0.626 / 0.918 ms; the 14 x 14 DCN was their largest launch, 90 us at 16 RoIs).
    const int MT = dm_ceil_div(CoutP, 128);
    l = {DCN_LDS, {0, 0, 0, 0}, 256, MT, 0, Q, MT * dm_ceil_div(Q, 128), 1, 1, 0, 16 * (2 * 2 * 3 * 2 * 128) + 4 * 2 * 2 * 8 * HW};
    dcn_choose_split(c, true, l);
    if (l.ksplit == 1) {
      // 256 couts: one workgroup per 64 pixels holds every cout (deform_conv_c256_kernel: each sample gathered once; the
      // waves own different couts and read their weights straight from L2).  B ring (2 x 3 taps x 2 quads x 64 float4) + the
      // plane buffers: 37 KB at 14 x 14, 44 KB at H*W = 256.  Launches that split their K loop stay on the LDS kernel.
      if (CoutP == 256) l = {DCN_C256, {0, 0, 0, 0}, 256, 1, 0, Q, dm_ceil_div(Q, 64), 1, 1, 0, 16 * (2 * 3 * 2 * 64) + 4 * 2 * 2 * 8 * HW};
      if (c.seam) dcn_seam(c, CoutP, CoutP == 256 ? 64 : 128, r);
    }
  } else {
    // gather from global memory: a wave holds 64 accumulator registers, so 128 couts x 64 px (2.57 -> 2.28 ms at 64 channels,
    // 56 x 56, for the 64 x 64 tiles), or 32 x 128
    l = c.Cout > 64 ? (dcn_small_launch(c, CoutP, Q) ? dcn_generic(2, 2, 1, 1, CoutP, 0, Q) : dcn_generic(2, 2, 2, 1, CoutP, 0, Q))
                    : c.Cout > 32 ? dcn_generic(2, 2, 1, 1, CoutP, 0, Q) : dcn_generic(1, 4, 1, 1, CoutP, 0, Q);
    dcn_choose_split(c, false, l);
  }
  r.reduce = l.ksplit > 1;
  return r;
}

static DcnCall dcn_call(int NB, int C, int H, int W, int Cout, int dg, int flags, long long ws_floats, int M2) {
  // (flag bit 3, the caller overlaps launches on a second stream: no seam -- measured 259 vs 251 img/s)
  static const int tail_mode = getenv("DM_DCN_TAIL") ? atoi(getenv("DM_DCN_TAIL")) : 1;
  return {NB, C, H, W, Cout, dg, flags, ws_floats > 0 ? ws_floats : 0, M2, dm_num_cus(), tail_mode && !(flags & 8)};
}

constexpr int dcn_build(int kernel, int p0, int p1, int p2, int p3) { return (((kernel * 8 + p0) * 8 + p1) * 8 + p2) * 8 + p3; }
#define DCN_GENERIC_CASE(A, B, C, D) \
  case dcn_build(DCN_GENERIC, A, B, C, D): DM_LAUNCH((deform_conv_kernel<A, B, C, D>), grid, block, lds, st, a); break
#define DCN_BAND_CASE(A, B, C) \
  case dcn_build(DCN_BAND, A, B, C, 0): DM_LAUNCH((deform_conv_band_kernel<A, B, C>), grid, block, lds, st, a, tiles, DCN_BAND_ROWS); break

// The one place a DCN forward kernel is enqueued: the launches of route r, each with its slice of the arguments
static int dcn_emit(const DcnRoute& r, DcnArgs a, hipStream_t st) {
  for (int i = 0; i < r.count; ++i) {
    const DcnLaunch& l = r.launch[i];
    a.MT = l.MT; a.q_begin = l.q_begin; a.Q = l.Q; a.ksplit = l.ksplit; a.kchan = l.kchan;
    a.ws_stride = l.ksplit > 1 ? (long long)a.NB * a.Cout * a.HW : 0;
    if (l.kernel == DCN_LDS) {
      // the one build above 64 KB of LDS: raised once per device, to what the largest map it takes (H*W = 256) needs
      static bool raised[DM_MAX_DEVICES] = {false};
      if (dm_ensure_lds_limit(reinterpret_cast<const void*>(&deform_conv_lds_kernel), 16 * 2 * 2 * 3 * 2 * 128 + 4 * 2 * 2 * 8 * 256,
                              raised) != DM_OK)
        return DM_ERR_LAUNCH;
    }
    const dim3 grid((unsigned)l.grid_x, (unsigned)l.grid_y), block((unsigned)l.threads);
    const size_t lds = (size_t)l.lds_bytes;
    const int tiles = l.grid_x / a.NB;                                    // (band kernel: tiles per image)
    switch (dcn_build(l.kernel, l.p[0], l.p[1], l.p[2], l.p[3])) {
      DCN_GENERIC_CASE(2, 2, 1, 1);
      case dcn_build(DCN_LDS, 0, 0, 0, 0): DM_LAUNCH(deform_conv_lds_kernel, grid, block, lds, st, a); break;
      case dcn_build(DCN_C256, 0, 0, 0, 0): DM_LAUNCH(deform_conv_c256_kernel, grid, block, lds, st, a); break;
      DCN_BAND_CASE(1, 2, 4); DCN_BAND_CASE(1, 2, 7); DCN_BAND_CASE(2, 1, 4); DCN_BAND_CASE(2, 1, 7);
      DCN_BAND_CASE(1, 4, 4); DCN_BAND_CASE(1, 4, 7); DCN_BAND_CASE(4, 1, 4); DCN_BAND_CASE(2, 2, 7);
      DCN_GENERIC_CASE(2, 2, 2, 1); DCN_GENERIC_CASE(1, 4, 1, 1);
      default: return DM_ERR_UNSUPPORTED;                                 // (a route that names no build: a bug in dcn_route)
    }
    const int rc = dm_check_launch();
    if (rc != DM_OK) return rc;
  }
  if (!r.reduce) return DM_OK;
  // out = relu?(the splits of launch[0], added in index order); four per thread where everything is 16-byte aligned
  const long long total = a.ws_stride;
  const bool v4 = (total & 3) == 0 && ((((uintptr_t)a.ws) | ((uintptr_t)a.out)) & 15) == 0;
  DM_LAUNCH(dcn_splitk_reduce_kernel, dim3((unsigned)min((long long)4096, ((v4 ? total / 4 : total) + 255) / 256)), dim3(256), 0, st, a.ws,
            v4 ? a.ksplit : -a.ksplit, a.ws_stride, total, a.relu, a.out);
  return dm_check_launch();
}

// a: DcnArgs() or, for the chained 1x1, its members filled in (dm_deform_conv_tout_fwd)
static int deform_conv_fwd_impl(DcnArgs a, const float* x, const float* offset, int NB, int C, int H, int W, const float* w_packed,
                                int Cout, int deform_groups, int relu, float* out, float* ws, long long ws_floats, dm_stream_t stream) {
  const bool null_arg = !x || !offset || !w_packed || !out;
  if (null_arg && a.M2 == 0) return DM_ERR_INVALID_ARG;       // (the chained call answers for its shape first: dcn_route)
  const DcnRoute r = dcn_route(dcn_call(NB, C, H, W, Cout, deform_groups, relu, ws ? ws_floats : 0, a.M2));
  if (r.rc != DM_OK || r.count == 0) return r.rc;
  if (null_arg) return DM_ERR_INVALID_ARG;
  a.x = x; a.offset = offset; a.NB = NB; a.C = C; a.H = H; a.W = W; a.HW = H * W; a.Q = NB * H * W;
  a.wp = w_packed; a.Cout = Cout; a.CoutP = dm_conv_packed_cout(Cout); a.KQ = (C + 7) / 8 * 2; a.dg = deform_groups;
  a.relu = relu & 1; a.out = out;
  a.ws = (ws && ws_floats > 0) ? ws : nullptr;
  a.ws_floats = a.ws ? ws_floats : 0;
  return dcn_emit(r, a, (hipStream_t)stream);
}

}  // namespace

extern "C" int dm_deform_conv_fwd(const float* x, const float* offset, int NB, int C, int H, int W,
                                  const float* w_packed, int Cout, int deform_groups, int relu, float* out,
                                  dm_stream_t stream) {
  return deform_conv_fwd_impl(DcnArgs(), x, offset, NB, C, H, W, w_packed, Cout, deform_groups, relu, out, nullptr, 0, stream);
}

// (ABI 21) dm_deform_conv_fwd with a caller-owned workspace: dcn_route may split the channel loop (dcn_choose_split).
// dm_deform_conv_splitk_floats: an upper bound on what a split of this shape uses, which the route honours (0: no launch of
// this shape splits; tests/test_dcn_plan_cpu.py holds the route to both).
extern "C" long long dm_deform_conv_splitk_floats(int NB, int C, int H, int W, int Cout) {
  if (NB <= 0 || C < 32 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  const long long wgs = (long long)dm_ceil_div(Cout, 128) * dm_ceil_div((long long)NB * H * W, 128);
  if (wgs * 2 > 2LL * dm_num_cus() && !(H * W <= 256 && wgs < 2LL * dm_num_cus())) return 0;      // (14 x 14: up to one round)
  return 8LL * NB * Cout * H * W;
}

extern "C" int dm_deform_conv_fwd_ws(const float* x, const float* offset, int NB, int C, int H, int W,
                                     const float* w_packed, int Cout, int deform_groups, int relu, float* out,
                                     float* workspace, long long workspace_floats, dm_stream_t stream) {
  return deform_conv_fwd_impl(DcnArgs(), x, offset, NB, C, H, W, w_packed, Cout, deform_groups, relu, out, workspace, workspace_floats, stream);
}

// (added to ABI 28) What the three entry points here would launch for these host arguments: dcn_route's own value, the one
// dcn_emit enqueues (the header has the record layout).  Nothing below touches HIP but dm_num_cus().
extern "C" int dm_deform_conv_plan(int NB, int C, int H, int W, int Cout, int deform_groups, int relu, long long workspace_floats,
                                   int M2, int* records, int max_records) {
  if (!records || max_records < DM_DCN_PLAN_MAX_LAUNCHES || workspace_floats < 0 || M2 < 0) return DM_ERR_INVALID_ARG;
  if (M2 > 0 && workspace_floats > 0) return DM_ERR_INVALID_ARG;          // (the chained call takes no workspace)
  const DcnRoute r = dcn_route(dcn_call(NB, C, H, W, Cout, deform_groups, M2 > 0 ? 1 : relu, workspace_floats, M2));
  if (r.rc != DM_OK) return r.rc;
  for (int l = 0; l < r.count; ++l) {
    const DcnLaunch& m = r.launch[l];
    const int rec[DM_DCN_PLAN_INTS] = {m.kernel, m.p[0], m.p[1], m.p[2], m.p[3], m.threads, m.MT, m.q_begin, m.Q, m.grid_x, m.grid_y,
                                       m.ksplit, m.kchan, m.lds_bytes, r.reduce ? 1 : 0};
    for (int i = 0; i < DM_DCN_PLAN_INTS; ++i) records[l * DM_DCN_PLAN_INTS + i] = rec[i];
  }
  return r.count;
}

// Does this shape take the band build that can chain the 1x1 (a wave = 32 pixels x all couts)?  Route it and see.
extern "C" int dm_deform_conv_tout_supported(int NB, int C, int H, int W, int Cout, int M2) {
  if (M2 <= 0) return 0;
  const DcnRoute r = dcn_route(dcn_call(NB, C, H, W, Cout, 1, 1, 0, M2));
  return (r.rc == DM_OK && r.count == 1) ? 1 : 0;
}

// (ABI 27) DCN 3x3 + ReLU + the 1x1 convolution + bias + ReLU behind it in ONE launch (the header has the contract).
// DM_ERR_UNSUPPORTED where dm_deform_conv_tout_supported() says 0 -- the caller then launches the two operators.
extern "C" int dm_deform_conv_tout_fwd(const float* x, const float* offset, int NB, int C, int H, int W, const float* w_packed,
                                       int Cout, int deform_groups, const float* w2t, const float* b2, int M2, float* out2,
                                       int out2_ch_total, float* out_dcn, dm_stream_t stream) {
  if (!w2t || !b2 || !out2 || M2 <= 0 || M2 > out2_ch_total) return DM_ERR_INVALID_ARG;
  DcnArgs a;
  a.w2t = w2t; a.b2 = b2; a.out2 = out2; a.M2 = M2; a.w2_ld = dm_ceil_div(M2, 32) * 32; a.out2_ct = out2_ch_total;
  // (out_dcn == NULL is the "do not store" request: the kernel gets out2 as a stand-in and store_out = 0)
  a.store_out = (out_dcn && out_dcn != out2) ? 1 : 0;
  return deform_conv_fwd_impl(a, x, offset, NB, C, H, W, w_packed, Cout, deform_groups, 1, out_dcn ? out_dcn : out2, nullptr, 0, stream);
}
