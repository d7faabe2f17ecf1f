// ResNet stem inference (mmdet/models/backbones/resnet.py:559-571, :628-631):
//
//   dm_conv7x7_s2_fwd      conv1: 7x7, stride 2, padding 3, from 3 channels, + bias (the folded bn1) (+ ReLU), out
//                          [NB, Cout, ceil(H / 2), ceil(W / 2)].  Exact fp32 on v_mfma_f32_32x32x2_f32.
//   dm_maxpool3x3_s2_fwd   MaxPool2d(3, stride 2, padding 1), torch's NaN rule, padding taps take no part.
//   dm_conv3x3_s2_c3_fwd   the first convolution of the deep stem (resnet.py:525-545, Res2Net): 3x3, stride 2, padding 1,
//                          from 3 channels, + bias (+ ReLU).  Exact fp32, a direct vector kernel (below).
//
// GEMM view of the convolution: K is the 147 products (c, ky, kx) laid out as 21 ROWS (c, ky) of 8 kx SLOTS, slot 7 a zero
// weight: K = 168 = 42 quads, the weight operand dm_conv_pack_weight's 1x1 layout [42][CoutP][4] of that [Cout, 168]
// matrix (ops.pack_conv7x7_weight).  A step of the tile core (dm_mfma_quad: a pair of quads) is then one row: lane half 0
// takes kx 0..3, half 1 takes kx 4..7, and a lane's four B values are four NEIGHBOURS of the staged input row -- LDS reads
// at compile-time offsets from one per-lane base.  (147 padded to 152 would be 19 steps instead of 21, with a table lookup
// per read.)  The fma chain of an output is row 0 .. 20, in a row kx 0, 4, 1, 5, 2, 6, 3, (7): the same for every output,
// whatever NB, the map's size, the tile or the padding -- a tap in the padding is a product with a staged zero, and slot 7
// multiplies a literal zero (not a staged value: 0 * Inf would make a NaN torch does not make).
//
// Workgroup: 256 threads = 4 waves as 2 (32 couts each) x 2 (64 pixels each), an output tile of 8 x 16 pixels of one image
// by 64 couts.  The tile's input patch, (2 * 8 + 5) x (2 * 16 + 5) x 3 values, and all 42 quads of its 64 couts' weights
// are staged in LDS once, one barrier: patch 3 x 21 x 38 floats (9.4 KiB, a zero column pads the pitch) + weights
// 42 x 64 float4 (42 KiB).
#include "mfma_tile.h"

namespace {

constexpr int S7_TH = 8, S7_TW = 16;               // output tile
constexpr int S7_PH = 2 * S7_TH + 5;               // 21 input rows
constexpr int S7_PW = 2 * S7_TW + 5;               // 37 input columns
constexpr int S7_PITCH = S7_PW + 1;                // + the column kx slot 7 points at (a zero; its product is not formed)
constexpr int S7_C = 3;
constexpr int S7_ROWS = S7_C * 7;                  // K rows (c, ky)
constexpr int S7_KQ = 2 * S7_ROWS;                 // 42 quads
constexpr int S7_TM = 64;                          // couts per workgroup
constexpr int S7_NT = 256;
constexpr int S7_RELU = 1;

struct S7Args {
  const float* x;
  int NB, H, W, Ho, Wo;
  const float* wq;
  const float* bias;
  int Cout, CoutP, MT, tiles_x, tiles_y;
  int flags;
  float* out;
};

__global__ __launch_bounds__(S7_NT) void conv7x7_s2_kernel(S7Args a) {
  __shared__ dm_f32x4 ldsA[S7_KQ * S7_TM];
  __shared__ float patch[S7_C * S7_PH * S7_PITCH];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = wave >> 1;
  const int wave_n = wave & 1;
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  // block -> (image, tile row, tile column, cout tile); the MT cout tiles of a pixel tile are neighbours in launch order
  int b = (int)blockIdx.x;
  const int m0 = (b % a.MT) * S7_TM;
  b /= a.MT;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  const int n = b / a.tiles_y;
  const int oy0 = ty * S7_TH, ox0 = tx * S7_TW;
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;

  for (int idx = tid; idx < S7_KQ * S7_TM; idx += S7_NT) {
    const int q = idx / S7_TM, m = idx % S7_TM;
    dm_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m0 + m < a.CoutP) v = *reinterpret_cast<const dm_f32x4*>(a.wq + ((size_t)q * a.CoutP + m0 + m) * 4);
    ldsA[idx] = v;
  }
  const float* xn = a.x + (size_t)n * S7_C * a.H * a.W;
  for (int idx = tid; idx < S7_C * S7_PH * S7_PITCH; idx += S7_NT) {
    const int col = idx % S7_PITCH, cr = idx / S7_PITCH;
    const int r = cr % S7_PH, c = cr / S7_PH;
    const int iy = iy0 + r, ix = ix0 + col;
    float v = 0.f;
    if (col < S7_PW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = xn[((size_t)c * a.H + iy) * a.W + ix];
    patch[idx] = v;
  }
  __syncthreads();

  // pixel tile j of this wave: output rows wave_n * 4 + 2 j + (l31 >> 4), column l31 & 15 of the 8 x 16 tile
  dm_f32x16 acc[1][2];
  dm_acc_clear(acc);
  int pbase[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) pbase[j] = 2 * (wave_n * 4 + 2 * j + (l31 >> 4)) * S7_PITCH + 2 * (l31 & 15) + 4 * hi;
  const dm_f32x4* aw = ldsA + hi * S7_TM + wave_m * 32 + l31;
#pragma unroll 1
  for (int c = 0; c < S7_C; ++c) {
    const float* pc = patch + c * S7_PH * S7_PITCH;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      dm_f32x4 av[1], bv[2];
      av[0] = aw[(c * 7 + ky) * 2 * S7_TM];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float* p = pc + ky * S7_PITCH + pbase[j];
        bv[j][0] = p[0];
        bv[j][1] = p[1];
        bv[j][2] = p[2];
        bv[j][3] = hi ? 0.f : p[3];
      }
      dm_mfma_quad(acc, av, bv);
    }
  }

  // ---- epilogue: every store is guarded (row < Ho, column < Wo, cout < Cout)
  const int ox = ox0 + (l31 & 15);
  if (ox >= a.Wo) return;
  const bool relu = (a.flags & S7_RELU) != 0;
  const size_t HoWo = (size_t)a.Ho * a.Wo;
  const int co_wave = m0 + wave_m * 32;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int oy = oy0 + wave_n * 4 + 2 * j + (l31 >> 4);
    if (oy >= a.Ho) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co_wave + dm_dtile_row(r, hi);
      if (co >= a.Cout) continue;
      float v = acc[0][j][r] + (a.bias ? a.bias[co] : 0.f);
      if (relu) v = dm_relu(v);
      a.out[((size_t)n * a.Cout + co) * HoWo + (size_t)oy * a.Wo + ox] = v;
    }
  }
}

// workgroups of a launch, or -1 when they do not fit a grid (H, W, Cout <= S7_MAXDIM keep every factor small)
constexpr int S7_MAXDIM = 1 << 24;
long long s7_blocks(int NB, int H, int W, int Cout) {
  const long long ty = dm_ceil_div((H + 1) / 2, S7_TH), tx = dm_ceil_div((W + 1) / 2, S7_TW);
  const long long per_image = ty * tx;                                   // < 2^40
  if (per_image > 0x7fffffffLL) return -1;
  const long long pixel_tiles = (long long)NB * per_image;               // < 2^62
  if (pixel_tiles > 0x7fffffffLL) return -1;
  const long long blocks = pixel_tiles * dm_ceil_div(dm_conv_packed_cout(Cout), S7_TM);
  return blocks > 0x7fffffffLL ? -1 : blocks;
}

// ------------------------------------------------------------------------------------------------ max-pool
// A thread makes four neighbouring outputs of a row from the nine columns 2 ox0 - 1 .. 2 ox0 + 7 of three input rows: two
// float4 loads and a scalar per row where the rows are 16-byte aligned (VEC: W % 4 == 0 and an aligned base), scalar
// loads otherwise and at the right edge.  A tap outside the map enters as -inf, which dm_pool_takes never takes: the
// same as leaving it out.  Per output the taps are met in torch's order, rows outermost.
template <bool VEC>
__global__ __launch_bounds__(256) void maxpool3x3_s2_kernel(const float* __restrict__ in, long long total, int H, int W, int Ho,
                                                            int Wo, int WoG, float* __restrict__ out) {
  const float ninf = -__builtin_inff();
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long row = e / WoG;             // nc * Ho + oy
    const int ox0 = 4 * (int)(e - row * WoG);
    const long long nc = row / Ho;
    const int oy = (int)(row - nc * Ho);
    float best[4] = {ninf, ninf, ninf, ninf};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= H) continue;
      const float* p = in + ((size_t)nc * H + iy) * W + 2 * ox0;       // column 2 ox0 of the row
      float v[9];
      v[0] = ox0 > 0 ? p[-1] : ninf;
      if (VEC && 2 * ox0 + 8 <= W) {
        const dm_f32x4 lo = *reinterpret_cast<const dm_f32x4*>(p), hi4 = *reinterpret_cast<const dm_f32x4*>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[1 + i] = lo[i];
          v[5 + i] = hi4[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[1 + i] = 2 * ox0 + i < W ? p[i] : ninf;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          if (dm_pool_takes(v[2 * k + dx], best[k])) best[k] = v[2 * k + dx];
    }
    float* o = out + (size_t)row * Wo + ox0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ox0 + k < Wo) o[k] = best[k];
  }
}

// ------------------------------------------------------------------------------------------------ deep stem, first conv
// 27 products per output: a thread owns ONE output pixel (consecutive lanes are consecutive pixels of the image's flat
// map, so loads and stores run along rows), reads its own 27 taps into registers -- a tap outside the map is a zero
// operand, and no other pixel's value enters --, and makes S3_CT output channels from them, four fma chains at a time.
// The weights [Cout, 27] are torch's own layout, read through wave-uniform addresses.  The chain of an output: c = 0 .. 2,
// ky = 0 .. 2, kx = 0 .. 2 from zero, the bias added last.
constexpr int S3_CT = 32;                          // couts per workgroup
constexpr int S3_MAXDIM = 1 << 24;

__global__ __launch_bounds__(256) void conv3x3_s2_c3_kernel(const float* __restrict__ x, int H, int W, int Ho, int Wo,
                                                            const float* __restrict__ w, const float* __restrict__ bias, int Cout,
                                                            int co_tiles, unsigned px_tiles, int relu, float* __restrict__ out) {
  // block -> (image, pixel tile, cout tile); the cout tiles of a pixel tile are neighbours in launch order
  unsigned b = blockIdx.x;
  const int co0 = (int)(b % co_tiles) * S3_CT;
  b /= co_tiles;
  const unsigned pt = b % px_tiles;
  const unsigned n = b / px_tiles;
  const long long HoWo = (long long)Ho * Wo;
  const long long e = (long long)pt * 256 + threadIdx.x;
  if (e >= HoWo) return;
  const int oy = (int)(e / Wo), ox = (int)(e - (long long)oy * Wo);
  float v[27];
  const float* xn = x + (size_t)n * 3 * H * W;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
        v[(c * 3 + ky) * 3 + kx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xn[((size_t)c * H + iy) * W + ix] : 0.f;
      }
  float* on = out + (size_t)n * Cout * HoWo + e;
#pragma unroll 1
  for (int j0 = 0; j0 < S3_CT && co0 + j0 < Cout; j0 += 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* wj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wj[j] = w + (size_t)min(co0 + j0 + j, Cout - 1) * 27;     // (a cout past the last: not stored)
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(v[t], wj[j][t], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co0 + j0 + j;
      if (co >= Cout) break;
      float r = acc[j] + (bias ? bias[co] : 0.f);
      if (relu) r = dm_relu(r);
      on[(size_t)co * HoWo] = r;
    }
  }
}

// workgroups of a launch, or -1 when they do not fit a grid
long long s3_blocks(int NB, int H, int W, int Cout) {
  const long long px = ((long long)((H + 1) / 2) * ((W + 1) / 2) + 255) / 256;            // < 2^40
  if (px > 0x7fffffffLL) return -1;
  const long long per_image = px * dm_ceil_div(Cout, S3_CT);                               // < 2^51
  if (per_image > 0x7fffffffLL) return -1;
  const long long blocks = per_image * NB;
  return blocks > 0x7fffffffLL ? -1 : blocks;
}

}  // namespace

extern "C" int dm_conv3x3_s2_c3_supported(int NB, int C, int H, int W, int Cout) {
  if (NB < 1 || C != 3 || H < 1 || W < 1 || Cout < 1 || H > S3_MAXDIM || W > S3_MAXDIM || Cout > S3_MAXDIM) return 0;
  return s3_blocks(NB, H, W, Cout) > 0 ? 1 : 0;
}

extern "C" int dm_conv3x3_s2_c3_fwd(const float* x, int NB, int C, int H, int W, const float* w, const float* bias, int Cout,
                                    int flags, float* out, dm_stream_t stream) {
  if (!x || !w || !out) return DM_ERR_INVALID_ARG;
  const int fc = dm_flags_check(flags, S7_RELU);
  if (fc != DM_OK) return fc;
  if (!dm_conv3x3_s2_c3_supported(NB, C, H, W, Cout)) return DM_ERR_UNSUPPORTED;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int co_tiles = dm_ceil_div(Cout, S3_CT);
  const unsigned px_tiles = (unsigned)(((long long)Ho * Wo + 255) / 256);
  DM_LAUNCH(conv3x3_s2_c3_kernel, dim3((unsigned)s3_blocks(NB, H, W, Cout)), dim3(256), 0, (hipStream_t)stream, x, H, W, Ho,
            Wo, w, bias, Cout, co_tiles, px_tiles, (flags & S7_RELU) ? 1 : 0, out);
  return dm_check_launch();
}

extern "C" int dm_conv7x7_s2_supported(int NB, int C, int H, int W, int Cout) {
  if (NB < 1 || C != S7_C || H < 1 || W < 1 || Cout < 1 || H > S7_MAXDIM || W > S7_MAXDIM || Cout > S7_MAXDIM) return 0;
  return s7_blocks(NB, H, W, Cout) > 0 ? 1 : 0;
}

extern "C" int dm_conv7x7_s2_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                                 int Cout, int flags, float* out, dm_stream_t stream) {
  if (!x || !w_packed || !out) return DM_ERR_INVALID_ARG;
  const int fc = dm_flags_check(flags, S7_RELU);
  if (fc != DM_OK) return fc;
  if (!dm_conv7x7_s2_supported(NB, C, H, W, Cout)) return DM_ERR_UNSUPPORTED;
  S7Args a = {};
  a.x = x; a.NB = NB; a.H = H; a.W = W;
  a.Ho = (H + 1) / 2; a.Wo = (W + 1) / 2;
  a.wq = w_packed; a.bias = bias;
  a.Cout = Cout; a.CoutP = dm_conv_packed_cout(Cout); a.MT = dm_ceil_div(a.CoutP, S7_TM);
  a.tiles_y = dm_ceil_div(a.Ho, S7_TH); a.tiles_x = dm_ceil_div(a.Wo, S7_TW);
  a.flags = flags; a.out = out;
  DM_LAUNCH(conv7x7_s2_kernel, dim3((unsigned)s7_blocks(NB, H, W, Cout)), dim3(S7_NT), 0, (hipStream_t)stream, a);
  return dm_check_launch();
}

extern "C" int dm_maxpool3x3_s2_supported(long long NC, int H, int W) {
  return (NC >= 0 && H >= 1 && W >= 1 && NC <= (1LL << 40) / ((long long)H * W)) ? 1 : 0;
}

extern "C" int dm_maxpool3x3_s2_fwd(const float* in, long long NC, int H, int W, float* out, dm_stream_t stream) {
  if (!dm_maxpool3x3_s2_supported(NC, H, W)) return DM_ERR_UNSUPPORTED;
  if (NC == 0) return DM_OK;
  if (!in || !out) return DM_ERR_INVALID_ARG;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, WoG = (Wo + 3) / 4;
  const long long total = NC * Ho * WoG;
  const dim3 grid((unsigned)min((long long)dm_ceil_div(total, 256), 65536LL));
  const bool vec = W % 4 == 0 && ((uintptr_t)in & 15) == 0;
  if (vec) DM_LAUNCH(maxpool3x3_s2_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, total, H, W, Ho, Wo, WoG, out);
  else DM_LAUNCH(maxpool3x3_s2_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, total, H, W, Ho, Wo, WoG, out);
  return dm_check_launch();
}
