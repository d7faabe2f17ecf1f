// Sliced 3x3 convolution, stride 1 and 2 (the hierarchical 3x3 convolutions that stand where conv2 stood in every
// Res2Net block: mmdet/models/backbones/res2net.py:117-133):
//
//   dm_conv3x3_slices_fwd   G independent act(Conv2d(w, w, 3, stride, padding = 1)(x_g [+ addend_g]) + bias_g), exact fp32,
//                           slice g reading w channels of a wider x (and of a wider addend) and writing w channels of a
//                           wider out; plus an optional tail that copies or 3x3-average-pools one more w-channel slice.
//
// The slices are 26 / 52 / 104 / 208 channels wide in the reference's configs -- no multiple of 8 --, so this is ONE
// direct fp32 vector kernel in the style of conv_grouped.hip, with the slice width a run-time value: any w >= 1 runs.  A
// workgroup owns ONE slice of ONE image on one tile of output pixels and one tile of output channels: it reads that
// slice's w input channels and nothing else (isolation is by construction: no product with a foreign channel is formed,
// and K is not padded at all -- the channel loop ends at w), and every weight it multiplies by is the same for all lanes
// of a wave: the weights are read through uniform addresses, never staged.
//
// Workgroup: 256 threads = 4 waves.  A wave makes 8 rows x 32 columns of output pixels for CS_COT = 8 output channels:
// lane -> (row lane >> 3, the 4 neighbouring columns 4 * (lane & 7) ..), 8 x 4 accumulators.  Two builds per stride:
//
//     WCO   waves along the output channels   cout tile   output tile (rows x columns)     taken for
//      1                  1                       8           32 x 32                       w <= 8
//      4                  4                      32            8 x 32                       w > 8
//
// The cout tiles cover w rounded up to 8: the weights of the couts from w on are zeros in the packed layout and their
// results are never stored.  K (the slice's w input channels) is walked in chunks of up to CK channels (8; 2 in the
// 32-row build at stride 2, whose patch is 65 rows; the last chunk is shorter when CK does not divide w): the chunk's
// input patch, (S * (TH - 1) + 3) rows of S * 31 + 3 columns per
// channel (pitch 36 / 68 floats: a lane's window starts 16-byte aligned), is staged in LDS with zeros outside the map, one
// barrier pair per chunk.  With an addend the staged value is x + addend, ONE fp32 add per element (torch's
// `sp + spx[i]`); the padding stays zero.  A lane reads its 3 x 6 (stride 1) or 3 x 9 (stride 2) window of a channel once
// and makes 36 * 8 fmas from it.
//
// The fma chain of an output: input channel 0 .. w - 1 of its slice, in a channel ky = 0 .. 2, in a row kx = 0 .. 2, from
// a zero accumulator, the bias added last.  It does not depend on NB, G, H, W, the tile or the output's position (a tap in
// the padding multiplies a staged zero), so an image's bits do not depend on the other images of the call.
//
// The tail rides in the same grid, behind the convolution's workgroups: one thread per output pixel of the w tail
// channels.  Mode 1 copies; mode 2 is AvgPool2d(3, stride, padding = 1): the window's elements inside the map are added
// row-major from zero and the sum is divided ONCE by 9, whatever the window covers (count_include_pad).
//
// Weights: dm_conv3x3_slices_pack's [G][ceil(w / 8)][w][9][8] -- the 8 output channels of a wave side by side for each
// (input channel, tap), zeros for the output channels from w on.
#include "mfma_tile.h"

namespace {

constexpr int CS_NT = 256;
constexpr int CS_TW = 32;                          // output columns of a tile
constexpr int CS_WROWS = 8;                        // output rows of a wave
constexpr int CS_COT = 8;                          // output channels of a wave
constexpr int CS_CK = 8;                           // input channels of a staged chunk, at most
constexpr int CS_LDS_BYTES = 40 * 1024;
constexpr int CS_RELU = 1;
constexpr int CS_MAXDIM = 1 << 24;

constexpr int cs_th(int wco) { return (4 / wco) * CS_WROWS; }
constexpr int cs_ph(int wco, int s) { return s * (cs_th(wco) - 1) + 3; }
constexpr int cs_pw(int s) { return s * (CS_TW - 1) + 3; }
constexpr int cs_pitch(int s) { return (cs_pw(s) + 3) / 4 * 4; }
constexpr int cs_ck(int wco, int s) {              // the largest of 8 / 4 / 2 / 1 whose patch fits CS_LDS_BYTES
  int ck = CS_CK;
  while (ck > 1 && ck * cs_ph(wco, s) * cs_pitch(s) * 4 > CS_LDS_BYTES) ck /= 2;
  return ck;
}

inline int cs_wco(int w) { return w <= CS_COT ? 1 : 4; }
inline int cs_cot_tiles(int w) { return dm_ceil_div(w, CS_COT); }

struct CSArgs {
  const float* x;
  const float* addend;
  const float* wq;
  const float* bias;
  float* out;
  int Cx, x_ch0, Ca, a_ch0, Co, o_ch0;
  int w, G, H, W, Ho, Wo, stride;
  int tiles_x, tiles_y, co_tiles, flags, vec;
  int tail, tail_x_ch0, tail_o_ch0;
  unsigned conv_blocks, tail_per_image;
};

// one thread per output pixel of the tail's w channels of one image
__device__ __forceinline__ void cs_tail(const CSArgs& a, unsigned tb) {
  const unsigned n = tb / a.tail_per_image;
  const long long e = (long long)(tb - n * a.tail_per_image) * CS_NT + threadIdx.x;
  const long long HoWo = (long long)a.Ho * a.Wo;
  if (e >= (long long)a.w * HoWo) return;
  const int c = (int)(e / HoWo);
  const int p = (int)(e - (long long)c * HoWo);
  const int oy = p / a.Wo, ox = p - oy * a.Wo;
  const float* src = a.x + ((size_t)n * a.Cx + a.tail_x_ch0 + c) * a.H * a.W;
  float* dst = a.out + ((size_t)n * a.Co + a.tail_o_ch0 + c) * HoWo;
  if (a.tail == 1) {                               // stride 1: Ho == H, Wo == W
    dst[p] = src[p];
    return;
  }
  float sum = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = a.stride * oy - 1 + ky;
    if (iy < 0 || iy >= a.H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = a.stride * ox - 1 + kx;
      if (ix >= 0 && ix < a.W) sum += src[(size_t)iy * a.W + ix];
    }
  }
  dst[p] = sum / 9.f;
}

template <int WCO, int S>
__global__ __launch_bounds__(CS_NT) void conv3x3_slices_kernel(CSArgs a) {
  constexpr int COT = CS_COT, TH = cs_th(WCO), CK = cs_ck(WCO, S);
  constexpr int PH = cs_ph(WCO, S), PW = cs_pw(S), PITCH = cs_pitch(S);
  constexpr int NX = 3 * S + 3;                    // columns of a lane's window: 6 / 9
  static_assert(CK >= 1 && CK * PH * PITCH * 4 <= CS_LDS_BYTES, "the patch fits LDS");
  __shared__ __attribute__((aligned(16))) float patch[CK * PH * PITCH];

  if (blockIdx.x >= a.conv_blocks) {               // block-uniform: the tail's workgroups meet no barrier
    cs_tail(a, blockIdx.x - a.conv_blocks);
    return;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: the weight addresses below are scalar
  const int wco = wave % WCO, wsp = wave / WCO;

  // block -> (image, slice, cout tile, tile row, tile column): the tiles of a slice's map are neighbours in launch order
  int b = (int)blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  b /= a.tiles_y;
  const int ct = b % a.co_tiles;
  b /= a.co_tiles;
  const int g = b % a.G;
  const int n = b / a.G;
  const int oy0 = ty * TH, ox0 = tx * CS_TW;
  const int iy0 = S * oy0 - 1, ix0 = S * ox0 - 1;
  const int ly = wsp * CS_WROWS + (lane >> 3), lx4 = (lane & 7) * 4;
  const int w = a.w;
  const int cot = ct * WCO + wco;                  // this wave's tile of 8 couts of the slice
  const bool live = cot * COT < w;                 // (w <= 24 at WCO 4: a wave past the slice's couts only helps staging)

  const size_t HW = (size_t)a.H * a.W;
  const float* xg = a.x + ((size_t)n * a.Cx + a.x_ch0 + (size_t)g * w) * HW;
  const float* ag = a.addend ? a.addend + ((size_t)n * a.Ca + a.a_ch0 + (size_t)g * w) * HW : nullptr;
  const float* wv = a.wq + ((size_t)g * ((w + COT - 1) / COT) + (live ? cot : 0)) * w * 9 * COT;

  float acc[COT][4];
#pragma unroll
  for (int j = 0; j < COT; ++j)
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[j][p] = 0.f;

#pragma unroll 1
  for (int c0 = 0; c0 < w; c0 += CK) {
    const int ck = w - c0 < CK ? w - c0 : CK;      // channels of this chunk: the loop never leaves the slice
    if (c0) __syncthreads();                       // every wave has read the previous chunk
    for (int idx = tid; idx < ck * PH * PITCH; idx += CS_NT) {
      const int col = idx % PITCH, cr = idx / PITCH;
      const int r = cr % PH, c = cr / PH;
      const int iy = iy0 + r, ix = ix0 + col;
      float v = 0.f;
      if (col < PW && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
        const size_t off = ((size_t)(c0 + c) * a.H + iy) * a.W + ix;
        v = xg[off];
        if (ag) v = v + ag[off];
      }
      patch[idx] = v;
    }
    __syncthreads();
    if (!live) continue;

#pragma unroll 1
    for (int c = 0; c < ck; ++c) {
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
            const float wt = wc[(ky * 3 + kx) * COT + j];
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[j][p] = __builtin_fmaf(xin[ky][S * p + kx], wt, acc[j][p]);
          }
    }
  }

  // ---- epilogue: every store is guarded (row < Ho, column < Wo, cout < w)
  const int oy = oy0 + ly, ox = ox0 + lx4;
  if (!live || oy >= a.Ho || ox >= a.Wo) return;
  const bool relu = (a.flags & CS_RELU) != 0;
#pragma unroll
  for (int j = 0; j < COT; ++j) {
    const int cs = cot * COT + j;                  // cout inside the slice
    if (cs >= w) break;
    const float bj = a.bias ? a.bias[g * w + cs] : 0.f;
    float* o = a.out + (((size_t)n * a.Co + a.o_ch0 + (size_t)g * w + cs) * a.Ho + oy) * a.Wo + ox;
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

// workgroups of the convolution and of the tail, or false when they do not fit a grid together
bool cs_blocks(int NB, int w, int G, int H, int W, int stride, int tail, long long* conv, long long* tail_per_image) {
  const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const int wco = cs_wco(w);
  const long long per_map = (long long)dm_ceil_div(Ho, cs_th(wco)) * dm_ceil_div(Wo, CS_TW);      // < 2^43
  if (per_map > 0x7fffffffLL) return false;
  const long long per_image = per_map * G;                                                      // < 2^55 + checked
  if (per_image > 0x7fffffffLL) return false;
  const long long per_image_co = per_image * dm_ceil_div(cs_cot_tiles(w), wco);                 // < 2^31 * 2^22
  if (per_image_co > 0x7fffffffLL) return false;
  *conv = per_image_co * NB;
  if (*conv > 0x7fffffffLL) return false;
  *tail_per_image = 0;
  if (tail) {
    if ((long long)Ho * Wo > 0x7fffffffLL) return false;
    const long long outs = (long long)w * Ho * Wo;                                              // < 2^55
    if (outs / CS_NT + 1 > 0x7fffffffLL) return false;
    *tail_per_image = (outs + CS_NT - 1) / CS_NT;
  }
  return *conv + *tail_per_image * NB <= 0x7fffffffLL;
}

bool cs_shape_ok(int NB, int w, int G, int H, int W, int stride, int Cx, int Co, int tail) {
  if (NB < 0 || w < 1 || G < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return false;
  if (w > CS_MAXDIM || G > CS_MAXDIM || H > CS_MAXDIM || W > CS_MAXDIM || Cx > CS_MAXDIM || Co > CS_MAXDIM) return false;
  if (tail < 0 || tail > 2 || (tail == 1 && stride != 1)) return false;
  // the slices fit x, the slices and the tail's channels fit out, at all (the offsets are dm_conv3x3_slices_fwd's checks)
  if (Cx < (long long)w * G || Co < (long long)w * (G + (tail ? 1 : 0))) return false;
  long long conv, tpi;
  return NB == 0 || cs_blocks(NB, w, G, H, W, stride, tail, &conv, &tpi);
}

// does [ch0, ch0 + n) lie inside [0, C)?
bool cs_inside(int ch0, long long n, int C) { return ch0 >= 0 && (long long)ch0 + n <= C; }

}  // namespace

extern "C" long long dm_conv3x3_slices_packed_floats(int G, int w) {
  if (G < 1 || w < 1 || w > CS_MAXDIM || G > CS_MAXDIM) return -1;
  return (long long)G * cs_cot_tiles(w) * w * 9 * CS_COT;
}

// host memory to host memory: w_folded [G, w, w, 3, 3] -> [G][ceil(w / 8)][w][9][8], zeros for the couts from w on
extern "C" int dm_conv3x3_slices_pack(const float* wf, int G, int w, float* w_packed) {
  if (dm_conv3x3_slices_packed_floats(G, w) < 0) return DM_ERR_UNSUPPORTED;
  if (!wf || !w_packed) return DM_ERR_INVALID_ARG;
  const int T = cs_cot_tiles(w);
  for (int g = 0; g < G; ++g)
    for (int t = 0; t < T; ++t)
      for (int ci = 0; ci < w; ++ci)
        for (int tap = 0; tap < 9; ++tap)
          for (int j = 0; j < CS_COT; ++j) {
            const int co = t * CS_COT + j;
            w_packed[((((size_t)g * T + t) * w + ci) * 9 + tap) * CS_COT + j] =
                co < w ? wf[(((size_t)g * w + co) * w + ci) * 9 + tap] : 0.f;
          }
  return DM_OK;
}

extern "C" int dm_conv3x3_slices_supported(int NB, int w, int G, int H, int W, int stride, int Cx, int Co, int tail) {
  return (NB >= 1 && cs_shape_ok(NB, w, G, H, W, stride, Cx, Co, tail)) ? 1 : 0;
}

extern "C" int dm_conv3x3_slices_fwd(const float* x, int Cx, int x_ch0, const float* addend, int Ca, int a_ch0, int NB,
                                     int w, int G, int H, int W, int stride, const float* w_packed, const float* bias,
                                     int flags, float* out, int Co, int o_ch0, int tail, int tail_x_ch0, int tail_o_ch0,
                                     dm_stream_t stream) {
  const int fc = dm_flags_check(flags, CS_RELU);
  if (fc != DM_OK) return fc;
  if (stride != 1 && stride != 2) return DM_ERR_INVALID_ARG;
  if (!cs_shape_ok(NB, w, G, H, W, stride, Cx, Co, tail)) return DM_ERR_UNSUPPORTED;
  const long long span = (long long)w * G;
  if (!cs_inside(x_ch0, span, Cx) || !cs_inside(o_ch0, span, Co)) return DM_ERR_INVALID_ARG;
  if (addend && !cs_inside(a_ch0, span, Ca)) return DM_ERR_INVALID_ARG;
  if (tail) {
    if (!cs_inside(tail_x_ch0, w, Cx) || !cs_inside(tail_o_ch0, w, Co)) return DM_ERR_INVALID_ARG;
    // the tail's output channels may not be a slice's: both would be written
    if (tail_o_ch0 < o_ch0 + span && o_ch0 < tail_o_ch0 + w) return DM_ERR_INVALID_ARG;
  }
  if (NB == 0) return DM_OK;
  if (!x || !w_packed || !out) return DM_ERR_INVALID_ARG;
  long long conv, tpi;
  cs_blocks(NB, w, G, H, W, stride, tail, &conv, &tpi);
  CSArgs a = {};
  a.x = x; a.addend = addend; a.wq = w_packed; a.bias = bias; a.out = out;
  a.Cx = Cx; a.x_ch0 = x_ch0; a.Ca = Ca; a.a_ch0 = a_ch0; a.Co = Co; a.o_ch0 = o_ch0;
  a.w = w; a.G = G; a.H = H; a.W = W; a.stride = stride;
  a.Ho = (H + stride - 1) / stride; a.Wo = (W + stride - 1) / stride;
  const int wco = cs_wco(w);
  a.tiles_x = dm_ceil_div(a.Wo, CS_TW); a.tiles_y = dm_ceil_div(a.Ho, cs_th(wco));
  a.co_tiles = dm_ceil_div(cs_cot_tiles(w), wco);
  a.flags = flags;
  a.vec = (a.Wo % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  a.tail = tail; a.tail_x_ch0 = tail_x_ch0; a.tail_o_ch0 = tail_o_ch0;
  a.conv_blocks = (unsigned)conv; a.tail_per_image = (unsigned)tpi;
  const dim3 grid((unsigned)(conv + tpi * NB));
  hipStream_t s = (hipStream_t)stream;
  if (wco == 1) {
    if (stride == 1) DM_LAUNCH((conv3x3_slices_kernel<1, 1>), grid, dim3(CS_NT), 0, s, a);
    else DM_LAUNCH((conv3x3_slices_kernel<1, 2>), grid, dim3(CS_NT), 0, s, a);
  } else {
    if (stride == 1) DM_LAUNCH((conv3x3_slices_kernel<4, 1>), grid, dim3(CS_NT), 0, s, a);
    else DM_LAUNCH((conv3x3_slices_kernel<4, 2>), grid, dim3(CS_NT), 0, s, a);
  }
  return dm_check_launch();
}
