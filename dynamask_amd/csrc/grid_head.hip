// Grid R-CNN inference (mmdet/models/roi_heads/mask_heads/grid_head.py:151-187, :294-359), section K27 of dynamask_hip.h:
//
//   dm_group_norm_fwd            GroupNorm (+ ReLU) of [N, C, H, W]: the eight ConvModules' `gn` and GridHead.norm1.
//   dm_grid_fusion_fwd           one order of the neighbour fusion: out_i = x_i + sum_j (W1_ij dw5x5_ij(src_j) + b1_ij), all
//                                points and neighbours of all RoIs in one launch.
//   dm_deconv4x4_s2_grouped_fwd  ConvTranspose2d(kernel 4, stride 2, padding 1, groups) + bias: deconv1 and deconv2.
//   dm_grid_get_bboxes           GridHead.get_bboxes: sigmoid, first maximum per point, the vote of the boundary points.
//
// All exact fp32 on the VALU (the head's 218 GFLOP are its eight 3x3 convolutions, which run on the MFMA kernels of
// conv_strided.hip / conv_igemm.hip; these four launches are 9 GFLOP together), one fixed summation order, no atomics:
// the same bits on every run, and a RoI's result does not depend on the other RoIs of the call.
#include "common.h"

namespace {

constexpr int GH_NT = 256;

// the sum of v over the workgroup's 256 threads, in one fixed order (lanes by shuffle, then the four waves in index
// order), returned to every thread.  `red` holds 4 floats; two barriers per call.
__device__ __forceinline__ float gh_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                       // (the previous call's reads of red are over)
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------ GroupNorm
// One workgroup per (sample, group): the group is L = (C / G) * H * W consecutive floats.  Two passes for the statistics,
// both on values shifted by the group's first element x0 (a constant group gives mean = x0 and every difference exactly
// 0): s = sum(x - x0), m = s / L; var = sum(((x - x0) - m)^2) / L (biased); y = ((x - x0) - m) * rsqrt(var + eps) * gamma
// + beta.  The group is re-read from the cache (3 KB .. 49 KB) instead of being held: one code path for every L.  In
// place (y == x) is safe: a workgroup writes only its own group, each element by the thread that last read it.
__global__ __launch_bounds__(GH_NT) void group_norm_kernel(const float* x, int C, int G, int HW, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, int relu, float* y) {
  __shared__ float red[4];
  const int cpg = C / G;
  const int L = cpg * HW;
  const size_t base = (size_t)blockIdx.x * L;          // blockIdx.x = n * G + g: groups are consecutive in NCHW
  const int g = (int)(blockIdx.x % (unsigned)G);
  const float* xg = x + base;
  const float x0 = xg[0];
  float s = 0.f;
  for (int i = threadIdx.x; i < L; i += GH_NT) s += xg[i] - x0;
  const float m = gh_block_sum(s, red) / (float)L;
  float q = 0.f;
  for (int i = threadIdx.x; i < L; i += GH_NT) {
    const float d = (xg[i] - x0) - m;
    q += d * d;
  }
  const float var = gh_block_sum(q, red) / (float)L;
  const float rstd = 1.f / sqrtf(var + eps);
  float* yg = y + base;
  for (int i = threadIdx.x; i < L; i += GH_NT) {
    const int c = g * cpg + i / HW;
    float v = ((xg[i] - x0) - m) * rstd * gamma[c] + beta[c];
    if (relu) v = dm_relu(v);
    yg[i] = v;
  }
}

// The wide build, for the groups of a dense head's towers (FCOSHead on a 1333 x 800 image: 8 x 100 x 168 floats = 525 KB at
// stride 8): the same three passes and the same expressions, by 1024 threads instead of 256 and with 16-byte loads and
// stores.  A group starts wherever (n G + g) L floats lead -- 4-byte aligned only when L is odd -- so it is walked as a
// scalar head (up to the first 16-byte boundary of x), an aligned middle of float4s and a scalar tail; the stores are
// float4s where y's group has x's offset from a 16-byte boundary (in place: always), four scalars each otherwise.
// Thread t owns the middle's vectors t, t + 1024, ... and head / tail element t; it adds its vectors' components into four
// accumulators in that order, then ((a0 + a1) + (a2 + a3)) + its head / tail element; the 64 lanes by shuffle, the 16 waves
// in index order: one fixed order for a given L and offset of the group from a 16-byte boundary, both fixed by the shape and
// the group's place in the tensor -- the same bits on every run, and a sample's bits do not depend on the samples beside
// it.  The channel of an element is carried along (quotient and remainder by H W advance by constants): one division per
// thread.  In place is safe for the same reason as above.
constexpr int GW_NT = 1024;
constexpr int GW_WAVES = GW_NT / 64;

__device__ __forceinline__ float gw_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                       // (the previous call's reads of red are over)
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < GW_WAVES; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(GW_NT) void group_norm_wide_kernel(const float* x, int C, int G, int HW, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int relu, float* y) {
  __shared__ float red[GW_WAVES];
  const int cpg = C / G;
  const int L = cpg * HW;
  const size_t base = (size_t)blockIdx.x * L;
  const int g = (int)(blockIdx.x % (unsigned)G);
  const float* xg = x + base;
  float* yg = y + base;
  const int tid = threadIdx.x;
  // head: the elements in front of x's first 16-byte boundary (0 .. 3; L > 3 here), nv aligned vectors, then the tail
  const int head = (int)(((16u - (unsigned)((uintptr_t)xg & 15u)) & 15u) >> 2);
  const int nv = (L - head) >> 2;
  const int tail0 = head + 4 * nv;                     // first tail element; L - tail0 in 0 .. 3
  const dm_f32x4* xv = reinterpret_cast<const dm_f32x4*>(xg + head);
  const int ei = tid < 4 ? tid : tail0 + (tid - 4);    // threads 0 .. 3: head elements; 4 .. 7: tail elements
  const bool edge = tid < 4 ? tid < head : (tid < 8 && ei < L);
  const float x0 = xg[0];

  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
  for (int v = tid; v < nv; v += GW_NT) {
    const dm_f32x4 t = xv[v];
    a0 += t.x - x0; a1 += t.y - x0; a2 += t.z - x0; a3 += t.w - x0;
  }
  float s = (a0 + a1) + (a2 + a3);
  if (edge) s += xg[ei] - x0;
  const float m = gw_block_sum(s, red) / (float)L;

  a0 = a1 = a2 = a3 = 0.f;
#pragma unroll 4
  for (int v = tid; v < nv; v += GW_NT) {
    const dm_f32x4 t = xv[v];
    const float d0 = (t.x - x0) - m, d1 = (t.y - x0) - m, d2 = (t.z - x0) - m, d3 = (t.w - x0) - m;
    a0 += d0 * d0; a1 += d1 * d1; a2 += d2 * d2; a3 += d3 * d3;
  }
  float q = (a0 + a1) + (a2 + a3);
  if (edge) {
    const float d = (xg[ei] - x0) - m;
    q += d * d;
  }
  const float var = gw_block_sum(q, red) / (float)L;
  const float rstd = 1.f / sqrtf(var + eps);

  if (edge) {
    const int c = g * cpg + ei / HW;
    float v = ((xg[ei] - x0) - m) * rstd * gamma[c] + beta[c];
    if (relu) v = dm_relu(v);
    yg[ei] = v;
  }
  const bool vec_store = (((uintptr_t)yg ^ (uintptr_t)xg) & 15u) == 0;       // (uniform over the workgroup)
  dm_f32x4* yv = reinterpret_cast<dm_f32x4*>(yg + head);
  // element i = head + 4 v + j lies in channel g cpg + i / HW: (qc, rc) = divmod(i, HW) of the vector's first element
  const int step = 4 * GW_NT, dq = step / HW, dr = step - dq * HW;
  int i0 = head + 4 * tid;
  int qc = i0 / HW, rc = i0 - qc * HW;
  for (int v = tid; v < nv; v += GW_NT) {
    const dm_f32x4 t = xv[v];
    const float in[4] = {t.x, t.y, t.z, t.w};
    float o[4];
    int qj = qc, rj = rc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = g * cpg + qj;
      float r = ((in[j] - x0) - m) * rstd * gamma[c] + beta[c];
      if (relu) r = dm_relu(r);
      o[j] = r;
      if (++rj == HW) { rj = 0; ++qj; }
    }
    if (vec_store) {
      dm_f32x4 w;
      w.x = o[0]; w.y = o[1]; w.z = o[2]; w.w = o[3];
      yv[v] = w;
    } else {
      float* yo = yg + head + 4 * (size_t)v;
      yo[0] = o[0]; yo[1] = o[1]; yo[2] = o[2]; yo[3] = o[3];
    }
    qc += dq; rc += dr;
    if (rc >= HW) { rc -= HW; ++qc; }
  }
}

// ------------------------------------------------------------------------------------------------ neighbour fusion
// One workgroup per (RoI, point i).  Per neighbour slot j (the reference's order: left, up, down, right): the source
// point's c x S x S slice goes to LDS, the depthwise 5x5 (+ its bias) of it to LDS, then the 1x1: lane = pixel
// (S * S <= 64), wave w owns the OPW output channels [w * OPW, (w + 1) * OPW), its weights are wave-uniform (the table
// holds W1 transposed, [k][o]).  t = (sum_k W1[o, k] d[k]) + b1[o], k ascending; total = ((x_i + t_0) + t_1) + ...
// Table, per (point, slot): [dw weight c x 25][dw bias c][W1^T c x c][b1 c]  (GF_EDGE(c) floats; empty slots unused).
struct FusionArgs {
  int P, c, S;
  int nb[16][4];           // neighbour point of (point, slot), -1: none
};

__host__ __device__ constexpr int gf_edge(int c) { return c * 25 + c + c * c + c; }

template <int OPW>
__global__ __launch_bounds__(GH_NT) void grid_fusion_kernel(const float* __restrict__ x, const float* __restrict__ src,
                                                           const float* __restrict__ table, float* __restrict__ out,
                                                           FusionArgs a) {
  constexpr int C = 4 * OPW;
  constexpr int MAXSS = 64;
  __shared__ float s_src[C * MAXSS];
  __shared__ float s_d[C * MAXSS];
  const int S = a.S, SS = S * S;
  const int n = (int)blockIdx.x / a.P, i = (int)blockIdx.x % a.P;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t roi = (size_t)n * a.P * C * SS;
  const bool live = lane < SS;

  float total[OPW];
#pragma unroll
  for (int oo = 0; oo < OPW; ++oo)
    total[oo] = live ? x[roi + ((size_t)i * C + wave * OPW + oo) * SS + lane] : 0.f;

  for (int j = 0; j < 4; ++j) {
    const int p = a.nb[i][j];
    if (p < 0) continue;                                     // (uniform over the workgroup)
    const float* e = table + (size_t)(i * 4 + j) * gf_edge(C);
    const float* dw_w = e;
    const float* dw_b = e + C * 25;
    const float* w1t = dw_b + C;
    const float* b1 = w1t + C * C;
    __syncthreads();                                         // the previous slot's reads of s_src / s_d are over
    const float* sp = src + roi + (size_t)p * C * SS;
    for (int el = tid; el < C * SS; el += GH_NT) s_src[el] = sp[el];
    __syncthreads();
    for (int el = tid; el < C * SS; el += GH_NT) {
      const int k = el / SS, pix = el - k * SS;
      const int y = pix / S, xx = pix - y * S;
      float acc = 0.f;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy) {
        const int iy = y + dy - 2;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
          const int ix = xx + dx - 2;
          if (iy >= 0 && iy < S && ix >= 0 && ix < S) acc += dw_w[k * 25 + dy * 5 + dx] * s_src[k * SS + iy * S + ix];
        }
      }
      s_d[el] = acc + dw_b[k];
    }
    __syncthreads();
    float t[OPW];
#pragma unroll
    for (int oo = 0; oo < OPW; ++oo) t[oo] = 0.f;
    if (live) {
      for (int k = 0; k < C; ++k) {
        const float d = s_d[k * SS + lane];
        const float* wr = w1t + k * C + wave * OPW;
#pragma unroll
        for (int oo = 0; oo < OPW; ++oo) t[oo] += wr[oo] * d;
      }
#pragma unroll
      for (int oo = 0; oo < OPW; ++oo) total[oo] += t[oo] + b1[wave * OPW + oo];
    }
  }
  if (live) {
#pragma unroll
    for (int oo = 0; oo < OPW; ++oo) out[roi + ((size_t)i * C + wave * OPW + oo) * SS + lane] = total[oo];
  }
}

// ------------------------------------------------------------------------------------------------ grouped deconv 4x4 / s2
// out[n, g co + o, 2m + a, 2l + b] = bias + sum_k sum over the 2 x 2 taps of phase (a, b) of
// x[n, g ci + k, iy, ix] w[g ci + k, o, ky, kx], where along an axis phase 0 reads (k 1, i m) and (k 3, i m - 1), phase 1
// reads (k 2, i m) and (k 0, i m + 1); taps outside the map are zero (the border rows and columns have fewer taps).
// One workgroup per (sample, group, tile of OT output channels): the group's ci planes sit in LDS with a zero border,
// a thread owns one input position (m, l) -- the 2 x 2 output block above it -- and OPT output channels, whose sixteen
// taps per input channel are wave-uniform.  WOVER: the four waves split the tile's channels (OT = 4 OPT) and every wave
// walks all positions; else every wave owns all OT = OPT channels and the 256 threads split the positions.
// (the pointers are plain __restrict__ parameters, not members of a struct: the weight loads, whose addresses are
// wave-uniform, then compile to scalar loads)
template <int OPT, bool WOVER>
__global__ __launch_bounds__(GH_NT) void deconv4x4_s2_grouped_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ out,
                                                                    int G, int ci, int co, int S) {
  extern __shared__ float s_x[];                 // [ci][(S + 2) * (S + 2)], zero border
  const int Sp = S + 2, plane = Sp * Sp, SS = S * S;
  const int ng = (int)blockIdx.x, g = ng % G;
  const size_t n = (size_t)(ng / G);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* xg = x + (n * G + g) * (size_t)ci * SS;
  for (int el = tid; el < ci * plane; el += GH_NT) {
    const int k = el / plane, r = el - k * plane;
    const int py = r / Sp, px = r - py * Sp;
    float v = 0.f;
    if (py >= 1 && py <= S && px >= 1 && px <= S) v = xg[(size_t)k * SS + (py - 1) * S + (px - 1)];
    s_x[el] = v;
  }
  __syncthreads();
  const int o0 = (int)blockIdx.y * (WOVER ? 4 * OPT : OPT) + (WOVER ? wave * OPT : 0);
  const int So = 2 * S;
  for (int pos = WOVER ? (tid & 63) : tid; pos < SS; pos += WOVER ? 64 : GH_NT) {
    const int m = pos / S, l = pos - m * S;
    float acc[OPT][4];
#pragma unroll
    for (int oo = 0; oo < OPT; ++oo)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[oo][q] = 0.f;
    const float* xc = s_x + (m + 1) * Sp + (l + 1);            // the centre of the 3 x 3 neighbourhood, channel 0
    for (int k = 0; k < ci; ++k) {
      const float* xp = xc + k * plane;
      const float v00 = xp[-Sp - 1], v01 = xp[-Sp], v02 = xp[-Sp + 1];
      const float v10 = xp[-1], v11 = xp[0], v12 = xp[1];
      const float v20 = xp[Sp - 1], v21 = xp[Sp], v22 = xp[Sp + 1];
      const float* wk = w + ((size_t)(g * ci + k) * co + o0) * 16;
#pragma unroll
      for (int oo = 0; oo < OPT; ++oo) {
        const float* t = wk + oo * 16;                         // t[ky * 4 + kx]
        // phase (0, 0): rows (k 1, m), (k 3, m - 1) x columns (k 1, l), (k 3, l - 1); one FMA per tap, in this order
        float p = acc[oo][0];
        p = fmaf(t[5], v11, p); p = fmaf(t[7], v10, p); p = fmaf(t[13], v01, p); p = fmaf(t[15], v00, p);
        acc[oo][0] = p;
        // phase (0, 1): columns (k 2, l), (k 0, l + 1)
        p = acc[oo][1];
        p = fmaf(t[6], v11, p); p = fmaf(t[4], v12, p); p = fmaf(t[14], v01, p); p = fmaf(t[12], v02, p);
        acc[oo][1] = p;
        // phase (1, 0): rows (k 2, m), (k 0, m + 1)
        p = acc[oo][2];
        p = fmaf(t[9], v11, p); p = fmaf(t[11], v10, p); p = fmaf(t[1], v21, p); p = fmaf(t[3], v20, p);
        acc[oo][2] = p;
        // phase (1, 1)
        p = acc[oo][3];
        p = fmaf(t[10], v11, p); p = fmaf(t[8], v12, p); p = fmaf(t[2], v21, p); p = fmaf(t[0], v22, p);
        acc[oo][3] = p;
      }
    }
#pragma unroll
    for (int oo = 0; oo < OPT; ++oo) {
      const int o = o0 + oo;
      const float b = bias ? bias[g * co + o] : 0.f;
      float* op = out + ((n * G + g) * (size_t)co + o) * So * So + (size_t)(2 * m) * So + 2 * l;
      op[0] = acc[oo][0] + b;
      op[1] = acc[oo][1] + b;
      op[So] = acc[oo][2] + b;
      op[So + 1] = acc[oo][3] + b;
    }
  }
}

// ------------------------------------------------------------------------------------------------ get_bboxes
// One workgroup per RoI.  Per point: s = sigmoid(heat) (dm_sigmoid), its maximum and the FIRST cell that holds it (torch's
// max over the sigmoid values: saturated cells tie, a NaN is the maximum); then grid_head.py:313-355 in fp32, one
// rounding per operation (no contraction): the sub-region offsets, the box expanded by half its size, the score-weighted
// vote of the boundary points.  The box is NOT clipped to the image (Quirk Q21: the reference clamps a copy).
struct BoxArgs {
  const float* heat;
  const float* det;
  float* out;
  int* cells;              // [n, P]: the maximum's cell within the point's map (tests, debugging), or NULL
  int P, gs, HS, D;
  int sub_x[16], sub_y[16];
};

__device__ __forceinline__ bool gb_better(float v, int i, float bv, int bi) {
  const bool vn = __builtin_isnan(v), bn = __builtin_isnan(bv);
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(GH_NT) void grid_get_bboxes_kernel(BoxArgs a) {
#pragma clang fp contract(off)
  __shared__ float r_v[GH_NT];
  __shared__ int r_i[GH_NT];
  __shared__ float sc[16], px[16], py[16];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const int cells = a.HS * a.HS;
  for (int p = 0; p < a.P; ++p) {
    const float* h = a.heat + (n * a.P + p) * (size_t)cells;
    float bv = -1.f;                       // below every sigmoid value
    int bi = 0x7fffffff;
    for (int i = tid; i < cells; i += GH_NT) {
      const float v = dm_sigmoid(h[i]);
      if (gb_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    r_v[tid] = bv;
    r_i[tid] = bi;
    __syncthreads();
    for (int s = GH_NT / 2; s >= 1; s >>= 1) {
      if (tid < s && gb_better(r_v[tid + s], r_i[tid + s], r_v[tid], r_i[tid])) {
        r_v[tid] = r_v[tid + s];
        r_i[tid] = r_i[tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int pos = r_i[0];
      sc[p] = r_v[0];
      if (a.cells) a.cells[n * a.P + p] = pos;
      px[p] = (float)(pos % a.HS + a.sub_x[p]);
      py[p] = (float)(pos / a.HS + a.sub_y[p]);
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const float* d = a.det + n * a.D;
  const float bx1 = d[0], by1 = d[1], bx2 = d[2], by2 = d[3];
  const float widths = bx2 - bx1, heights = by2 - by1;
  const float x1 = bx1 - widths / 2.f, y1 = by1 - heights / 2.f;
  const float fw = (float)a.HS;
  const int gs = a.gs;
  float res[4];
  for (int side = 0; side < 4; ++side) {
    float num = 0.f, den = 0.f;
    for (int i = 0; i < gs; ++i) {
      // x1: the points of column 0; y1: of row 0; x2: of the last column; y2: of the last row (point = column * gs + row)
      const int p = side == 0 ? i : side == 1 ? i * gs : side == 2 ? a.P - gs + i : (i + 1) * gs - 1;
      const bool horiz = (side & 1) == 0;
      const float coord = horiz ? (px[p] + 0.5f) / fw * widths + x1 : (py[p] + 0.5f) / fw * heights + y1;
      const float term = coord * sc[p];
      num = i == 0 ? term : num + term;
      den = i == 0 ? sc[p] : den + sc[p];
    }
    res[side] = num / den;
  }
  float* o = a.out + n * 5;
  o[0] = res[0]; o[1] = res[1]; o[2] = res[2]; o[3] = res[3];
  o[4] = d[a.D - 1];
}

bool fusion_ok(int P, int c, int S) { return (P == 4 || P == 9) && (c == 8 || c == 64) && (S == 3 || S == 7); }

// The deconvolution keeps a group's ci input planes of (S + 2)^2 floats in dynamic LDS.  The largest supported shape takes
// exactly the 64 KiB a launch gets without hipFuncSetAttribute(MaxDynamicSharedMemorySize): a larger ci or S has to raise
// that limit (or tile the planes) before it is admitted here.
constexpr int DECONV_MAX_CI = 64, DECONV_MAX_S = 14;
constexpr size_t DECONV_LDS_LIMIT = 65536;
constexpr size_t deconv_lds_bytes(int ci, int S) { return (size_t)ci * (S + 2) * (S + 2) * sizeof(float); }
static_assert(deconv_lds_bytes(DECONV_MAX_CI, DECONV_MAX_S) <= DECONV_LDS_LIMIT, "deconv planes exceed the default dynamic LDS");

bool deconv_ok(int G, int ci, int co, int S) {
  return (G == 4 || G == 9) && (ci == 8 || ci == 64) && (co == 1 || co == 8 || co == 64) && (S == 1 || S == 3 || S == 7 || S == 14) &&
         ci <= DECONV_MAX_CI && S <= DECONV_MAX_S;
}

// The wide build takes the groups of at least GN_WIDE_MIN_L floats.  Above 16384 on purpose: every group the Grid head
// launches (768 .. 12544 floats) keeps group_norm_kernel and its bits.  The value is the smallest measured length from which
// the wide build is faster at one and at four samples (tools/fcos_infer_bench.py; the table is in DESIGN.md).
// DM_GN_WIDE=0: group_norm_kernel for every L (the A/B baseline of that tool); read once, re-read by dm_reload_env_knobs.
constexpr int GN_WIDE_MIN_L = 16385;
int g_gn_wide = -1;

int gn_wide() {
  if (g_gn_wide < 0) dm_gn_reload_knobs();      // (a race between two host threads repeats an idempotent load)
  return g_gn_wide;
}

}  // namespace

void dm_gn_reload_knobs() {
  const char* e = getenv("DM_GN_WIDE");
  g_gn_wide = (e && *e && atoi(e) == 0) ? 0 : 1;
}

extern "C" int dm_group_norm_supported(long long N, int C, int G, int H, int W) {
  if (N < 0 || C < 1 || G < 1 || H < 1 || W < 1 || C % G != 0) return 0;
  if ((long long)(C / G) * H * W > (1LL << 24)) return 0;             // the group's element count as int (and as float)
  if (N * G > 0x7fffffffLL) return 0;
  return 1;
}

extern "C" int dm_group_norm_fwd(const float* x, long long N, int C, int G, int H, int W, const float* gamma, const float* beta,
                                 float eps, int relu, float* y, dm_stream_t stream) {
  if (!dm_group_norm_supported(N, C, G, H, W)) return DM_ERR_UNSUPPORTED;
  if (relu & ~1) return DM_ERR_INVALID_ARG;
  if (N == 0) return DM_OK;
  if (!x || !y || !gamma || !beta || !(eps > 0.f)) return DM_ERR_INVALID_ARG;
  if ((long long)(C / G) * H * W >= GN_WIDE_MIN_L && gn_wide())
    DM_LAUNCH(group_norm_wide_kernel, dim3((unsigned)(N * G)), dim3(GW_NT), 0, (hipStream_t)stream, x, C, G, H * W, gamma, beta,
              eps, relu, y);
  else
    DM_LAUNCH(group_norm_kernel, dim3((unsigned)(N * G)), dim3(GH_NT), 0, (hipStream_t)stream, x, C, G, H * W, gamma, beta, eps,
              relu, y);
  return dm_check_launch();
}

extern "C" int dm_grid_fusion_supported(int N, int P, int c, int S) {
  return (N >= 0 && fusion_ok(P, c, S) && (long long)N * P <= 0x7fffffffLL) ? 1 : 0;
}

extern "C" long long dm_grid_fusion_table_floats(int P, int c) {
  if (!(P == 4 || P == 9) || !(c == 8 || c == 64)) return -1;
  return (long long)P * 4 * gf_edge(c);
}

extern "C" int dm_grid_fusion_fwd(const float* x, const float* src, int N, int P, int c, int S, const float* table, float* out,
                                  dm_stream_t stream) {
  if (!dm_grid_fusion_supported(N, P, c, S)) return DM_ERR_UNSUPPORTED;
  if (N == 0) return DM_OK;
  if (!x || !src || !table || !out || out == x || out == src) return DM_ERR_INVALID_ARG;
  FusionArgs a = {};
  a.P = P; a.c = c; a.S = S;
  // grid_head.py:88-102: point = column * gs + row; the slots in the reference's order left, up, down, right
  const int gs = P == 4 ? 2 : 3;
  for (int col = 0; col < gs; ++col)
    for (int row = 0; row < gs; ++row) {
      int* nb = a.nb[col * gs + row];
      int k = 0;
      if (col > 0) nb[k++] = (col - 1) * gs + row;
      if (row > 0) nb[k++] = col * gs + row - 1;
      if (row < gs - 1) nb[k++] = col * gs + row + 1;
      if (col < gs - 1) nb[k++] = (col + 1) * gs + row;
      while (k < 4) nb[k++] = -1;
    }
  const dim3 grid((unsigned)(N * P)), block(GH_NT);
  if (c == 64) DM_LAUNCH((grid_fusion_kernel<16>), grid, block, 0, (hipStream_t)stream, x, src, table, out, a);
  else DM_LAUNCH((grid_fusion_kernel<2>), grid, block, 0, (hipStream_t)stream, x, src, table, out, a);
  return dm_check_launch();
}

extern "C" int dm_deconv4x4_s2_grouped_supported(int N, int G, int ci, int co, int S) {
  return (N >= 0 && deconv_ok(G, ci, co, S) && (long long)N * G <= 0x7fffffffLL) ? 1 : 0;
}

extern "C" int dm_deconv4x4_s2_grouped_fwd(const float* x, int N, int G, int ci, int co, int S, const float* w, const float* bias,
                                           float* out, dm_stream_t stream) {
  if (!dm_deconv4x4_s2_grouped_supported(N, G, ci, co, S)) return DM_ERR_UNSUPPORTED;
  if (N == 0) return DM_OK;
  if (!x || !w || !out || out == x) return DM_ERR_INVALID_ARG;
  const size_t lds = deconv_lds_bytes(ci, S);          // <= DECONV_LDS_LIMIT: deconv_ok
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(GH_NT);
  if (co == 64) DM_LAUNCH((deconv4x4_s2_grouped_kernel<16, true>), dim3((unsigned)(N * G), 1), block, lds, st, x, w, bias, out, G, ci, co, S);
  else if (co == 8) DM_LAUNCH((deconv4x4_s2_grouped_kernel<2, true>), dim3((unsigned)(N * G), 1), block, lds, st, x, w, bias, out, G, ci, co, S);
  else DM_LAUNCH((deconv4x4_s2_grouped_kernel<1, false>), dim3((unsigned)(N * G), 1), block, lds, st, x, w, bias, out, G, ci, co, S);
  return dm_check_launch();
}

extern "C" int dm_grid_get_bboxes_supported(int n, int P, int HS, int D) {
  return (n >= 0 && (P == 4 || P == 9) && HS >= 1 && HS <= 1024 && D >= 5) ? 1 : 0;
}

extern "C" int dm_grid_get_bboxes(const float* heat, int n, int P, int HS, const float* det, int D, const int* sub_x,
                                  const int* sub_y, float* out, int* cells, dm_stream_t stream) {
  if (!dm_grid_get_bboxes_supported(n, P, HS, D)) return DM_ERR_UNSUPPORTED;
  if (n == 0) return DM_OK;
  if (!heat || !det || !sub_x || !sub_y || !out || out == det) return DM_ERR_INVALID_ARG;
  BoxArgs a = {};
  a.heat = heat; a.det = det; a.out = out; a.cells = cells;
  a.P = P; a.gs = P == 4 ? 2 : 3; a.HS = HS; a.D = D;
  for (int p = 0; p < P; ++p) { a.sub_x[p] = sub_x[p]; a.sub_y[p] = sub_y[p]; }
  DM_LAUNCH(grid_get_bboxes_kernel, dim3((unsigned)n), dim3(GH_NT), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}
