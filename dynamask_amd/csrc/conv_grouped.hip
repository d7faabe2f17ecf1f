// Grouped 3x3 convolution, stride 1 and 2 (conv2 of every ResNeXt block: mmdet/models/backbones/resnext.py:54-63):
//
//   dm_conv3x3_grouped_fwd   out = act(Conv2d(C, C, 3, stride, padding = 1, groups)(x) + bias), exact fp32.
//
// A grouped 3x3 does `groups` times less arithmetic than the dense one on the same bytes, and the fp32 MFMA rate is the
// fp32 vector rate: the launch is a stream of the map with 9 * C / groups fmas per output, so it is ONE direct vector
// kernel, built per (CG = C / groups, stride).  A workgroup owns ONE group of ONE image on one tile of output pixels: it
// reads that group's CG input channels and nothing else (group isolation is by construction, not by a zero product), and
// every weight it multiplies by is the same for all lanes of a wave -- the weights are read through uniform addresses
// (scalar loads of the constant cache), never staged.
//
// Workgroup: 256 threads = 4 waves.  A wave makes 8 rows x 32 columns of output pixels for COT output channels: lane ->
// (row lane >> 3, the 4 neighbouring columns 4 * (lane & 7) ..), COT x 4 accumulators.  The 4 waves are WCO waves along
// the group's output channels (WCO * COT == CG) times 4 / WCO along the rows:
//
//     CG      COT  WCO   output tile (rows x columns)
//     4        4    1    32 x 32
//     8        4    2    16 x 32
//     16       4    4     8 x 32
//     32       8    4     8 x 32
//     64      16    4     8 x 32
//
// K (the group's CG input channels) is walked in chunks of CK channels: the chunk's input patch, (S * (TH - 1) + 3) rows
// of S * 31 + 3 columns per channel (pitch 36 / 68 floats: a lane's window starts 16-byte aligned), is staged in LDS with
// zeros outside the map, one barrier pair per chunk; CK is the largest of 2 / 4 / 8 / 16 (<= CG) whose patch fits 40 KiB.
// A lane reads its 3 x 6 (stride 1) or 3 x 9 (stride 2) window of a channel once and makes 36 * COT fmas from it.
//
// The fma chain of an output: input channel 0 .. CG - 1 of its group, in a channel ky = 0 .. 2, in a row kx = 0 .. 2, from
// a zero accumulator, the bias added last.  It does not depend on NB, H, W, the tile or the output's position (a tap in
// the padding multiplies a staged zero), so an image's bits do not depend on the other images of the call.
//
// Weights: dm_conv3x3_grouped_pack's [C / COT][CG][9][COT] -- the COT output channels of a wave side by side for each
// (input channel, tap), 9 * COT contiguous floats per input channel.
#include "mfma_tile.h"

namespace {

constexpr int GC_NT = 256;
constexpr int GC_TW = 32;                          // output columns of a tile
constexpr int GC_WROWS = 8;                        // output rows of a wave
constexpr int GC_RELU = 1;
constexpr int GC_LDS_BYTES = 40 * 1024;
constexpr int GC_MAXDIM = 1 << 24;

constexpr int gc_cot(int cg) { return cg >= 64 ? 16 : cg >= 32 ? 8 : 4; }
constexpr int gc_wco(int cg) { return cg / gc_cot(cg); }
constexpr int gc_th(int cg) { return (4 / gc_wco(cg)) * GC_WROWS; }
constexpr int gc_ph(int cg, int s) { return s * (gc_th(cg) - 1) + 3; }
constexpr int gc_pw(int s) { return s * (GC_TW - 1) + 3; }
constexpr int gc_pitch(int s) { return (gc_pw(s) + 3) / 4 * 4; }
constexpr int gc_ck(int cg, int s) {
  int ck = 2;
  while (ck * 2 <= cg && ck * 2 <= 16 && ck * 2 * gc_ph(cg, s) * gc_pitch(s) * 4 <= GC_LDS_BYTES) ck *= 2;
  return ck;
}

bool gc_cg_ok(int cg) { return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64; }

struct GCArgs {
  const float* x;
  const float* wq;
  const float* bias;
  float* out;
  int C, H, W, Ho, Wo, groups, tiles_x, tiles_y, flags, vec;
};

template <int CG, int S>
__global__ __launch_bounds__(GC_NT) void conv3x3_grouped_kernel(GCArgs a) {
  constexpr int COT = gc_cot(CG), WCO = gc_wco(CG), TH = gc_th(CG);
  constexpr int PH = gc_ph(CG, S), PW = gc_pw(S), PITCH = gc_pitch(S), CK = gc_ck(CG, S);
  constexpr int NX = 3 * S + 3;                    // columns of a lane's window: 6 / 9
  static_assert(COT * WCO == CG && CG % CK == 0 && CK * PH * PITCH * 4 <= GC_LDS_BYTES, "tile geometry");
  __shared__ __attribute__((aligned(16))) float patch[CK * PH * PITCH];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: the weight addresses below are scalar
  const int wco = wave % WCO, wsp = wave / WCO;

  // block -> (image, group, tile row, tile column): the tiles of a group's map are neighbours in launch order
  int b = (int)blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  b /= a.tiles_y;
  const int g = b % a.groups;
  const int n = b / a.groups;
  const int oy0 = ty * TH, ox0 = tx * GC_TW;
  const int iy0 = S * oy0 - 1, ix0 = S * ox0 - 1;
  const int ly = wsp * GC_WROWS + (lane >> 3), lx4 = (lane & 7) * 4;

  const float* xg = a.x + ((size_t)n * a.C + (size_t)g * CG) * a.H * a.W;
  const float* wv = a.wq + (size_t)(g * WCO + wco) * CG * 9 * COT;

  float acc[COT][4];
#pragma unroll
  for (int j = 0; j < COT; ++j)
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[j][p] = 0.f;

#pragma unroll 1
  for (int c0 = 0; c0 < CG; c0 += CK) {
    if (c0) __syncthreads();                       // every wave has read the previous chunk
    for (int idx = tid; idx < CK * PH * PITCH; idx += GC_NT) {
      const int col = idx % PITCH, cr = idx / PITCH;
      const int r = cr % PH, c = cr / PH;
      const int iy = iy0 + r, ix = ix0 + col;
      float v = 0.f;
      if (col < PW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = xg[((size_t)(c0 + c) * a.H + iy) * a.W + ix];
      patch[idx] = v;
    }
    __syncthreads();

#pragma unroll 1
    for (int c = 0; c < CK; ++c) {
      float xin[3][NX];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float* pr = patch + (c * PH + S * ly + ky) * PITCH + S * lx4;
        const dm_f32x4 v0 = *reinterpret_cast<const dm_f32x4*>(pr);
#pragma unroll
        for (int i = 0; i < 4; ++i) xin[ky][i] = v0[i];
        if constexpr (S == 1) {
          xin[ky][4] = pr[4];
          xin[ky][5] = pr[5];
        } else {
          const dm_f32x4 v1 = *reinterpret_cast<const dm_f32x4*>(pr + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) xin[ky][4 + i] = v1[i];
          xin[ky][NX - 1] = pr[8];
        }
      }
      const float* wc = wv + (size_t)(c0 + c) * 9 * COT;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int j = 0; j < COT; ++j) {
            const float w = wc[(ky * 3 + kx) * COT + j];
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[j][p] = __builtin_fmaf(xin[ky][S * p + kx], w, acc[j][p]);
          }
    }
  }

  // ---- epilogue: every store is guarded (row < Ho, column < Wo)
  const int oy = oy0 + ly, ox = ox0 + lx4;
  if (oy >= a.Ho || ox >= a.Wo) return;
  const bool relu = (a.flags & GC_RELU) != 0;
  const int co0 = g * CG + wco * COT;
#pragma unroll
  for (int j = 0; j < COT; ++j) {
    const float bj = a.bias ? a.bias[co0 + j] : 0.f;
    float* o = a.out + (((size_t)n * a.C + co0 + j) * a.Ho + oy) * a.Wo + ox;
    dm_f32x4 v;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      v[p] = acc[j][p] + bj;
      if (relu) v[p] = dm_relu(v[p]);
    }
    if (a.vec) {                                   // Wo % 4 == 0: ox < Wo is ox + 3 < Wo, and the row is 16-byte aligned
      *reinterpret_cast<dm_f32x4*>(o) = v;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (ox + p < a.Wo) o[p] = v[p];
    }
  }
}

// workgroups of a launch, or -1 when they do not fit a grid
long long gc_blocks(int NB, int cg, int H, int W, int groups, int stride) {
  const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const long long per_map = (long long)dm_ceil_div(Ho, gc_th(cg)) * dm_ceil_div(Wo, GC_TW);       // < 2^43
  if (per_map > 0x7fffffffLL) return -1;
  const long long per_image = per_map * groups;                                             // < 2^55
  if (per_image > 0x7fffffffLL) return -1;
  const long long blocks = per_image * NB;
  return blocks > 0x7fffffffLL ? -1 : blocks;
}

bool gc_shape_ok(int NB, int C, int H, int W, int groups, int stride) {
  if (NB < 0 || groups < 1 || C < 1 || C % groups != 0 || !gc_cg_ok(C / groups)) return false;
  if (H < 1 || W < 1 || H > GC_MAXDIM || W > GC_MAXDIM || C > GC_MAXDIM || (stride != 1 && stride != 2)) return false;
  return NB == 0 || gc_blocks(NB, C / groups, H, W, groups, stride) > 0;
}

template <int CG>
void gc_launch(int stride, unsigned blocks, hipStream_t stream, GCArgs& a) {
  a.tiles_y = dm_ceil_div(a.Ho, gc_th(CG));
  if (stride == 1) DM_LAUNCH((conv3x3_grouped_kernel<CG, 1>), dim3(blocks), dim3(GC_NT), 0, stream, a);
  else DM_LAUNCH((conv3x3_grouped_kernel<CG, 2>), dim3(blocks), dim3(GC_NT), 0, stream, a);
}

}  // namespace

extern "C" int dm_conv3x3_grouped_couts_per_wave(int C, int groups) {
  if (groups < 1 || C < 1 || C % groups != 0 || !gc_cg_ok(C / groups)) return 0;
  return gc_cot(C / groups);
}

extern "C" long long dm_conv3x3_grouped_packed_floats(int C, int groups) {
  if (!dm_conv3x3_grouped_couts_per_wave(C, groups)) return -1;
  return (long long)C * (C / groups) * 9;
}

// host memory to host memory: w [C, CG, 3, 3] -> [C / COT][CG][9][COT]
extern "C" int dm_conv3x3_grouped_pack(const float* w, int C, int groups, float* w_packed) {
  const int cot = dm_conv3x3_grouped_couts_per_wave(C, groups);
  if (!cot) return DM_ERR_UNSUPPORTED;
  if (!w || !w_packed) return DM_ERR_INVALID_ARG;
  const int cg = C / groups;
  for (int co = 0; co < C; ++co)
    for (int ci = 0; ci < cg; ++ci)
      for (int tap = 0; tap < 9; ++tap)
        w_packed[(((size_t)(co / cot) * cg + ci) * 9 + tap) * cot + co % cot] = w[((size_t)co * cg + ci) * 9 + tap];
  return DM_OK;
}

extern "C" int dm_conv3x3_grouped_supported(int NB, int C, int H, int W, int groups, int stride) {
  return (NB >= 1 && gc_shape_ok(NB, C, H, W, groups, stride)) ? 1 : 0;
}

extern "C" int dm_conv3x3_grouped_fwd(const float* x, int NB, int C, int H, int W, const float* w_packed, const float* bias,
                                      int groups, int stride, int flags, float* out, dm_stream_t stream) {
  const int fc = dm_flags_check(flags, GC_RELU);
  if (fc != DM_OK) return fc;
  if (!gc_shape_ok(NB, C, H, W, groups, stride)) return DM_ERR_UNSUPPORTED;
  if (NB == 0) return DM_OK;
  if (!x || !w_packed || !out) return DM_ERR_INVALID_ARG;
  GCArgs a = {};
  a.x = x; a.wq = w_packed; a.bias = bias; a.out = out;
  a.C = C; a.H = H; a.W = W; a.groups = groups;
  a.Ho = (H + stride - 1) / stride; a.Wo = (W + stride - 1) / stride;
  a.tiles_x = dm_ceil_div(a.Wo, GC_TW);
  a.flags = flags;
  a.vec = (a.Wo % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  const int cg = C / groups;
  const unsigned blocks = (unsigned)gc_blocks(NB, cg, H, W, groups, stride);
  switch (cg) {
    case 4: gc_launch<4>(stride, blocks, (hipStream_t)stream, a); break;
    case 8: gc_launch<8>(stride, blocks, (hipStream_t)stream, a); break;
    case 16: gc_launch<16>(stride, blocks, (hipStream_t)stream, a); break;
    case 32: gc_launch<32>(stride, blocks, (hipStream_t)stream, a); break;
    default: gc_launch<64>(stride, blocks, (hipStream_t)stream, a); break;
  }
  return dm_check_launch();
}
