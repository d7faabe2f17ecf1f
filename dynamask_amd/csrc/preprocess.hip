// K33  Image pre-processing in front of the backbone: the reference's test pipeline Resize(keep_ratio) -> RandomFlip ->
// Normalize(to_rgb) -> Pad(size_divisor) -> ImageToTensor -> collate (mmdet/datasets/pipelines/transforms.py,
// formating.py; done there by cv2 on the host) as ONE launch over B decoded uint8 HWC images: out [B, 3, Hp, Wp] fp32,
// written completely (the padding's zeros too), no resized image in memory.
//
// The resize is 8-bit fixed-point bilinear: 11-bit coefficients per axis (host tables, dynamask_hip.h), the horizontal
// pass in int32, the vertical pass with the two >> 16 products and the rounding >> 2.  Integer up to the byte, then
// (float(v) - mean) * stdinv in fp32.  A streaming kernel: one thread per output column, PRE_ROWS rows per workgroup (the
// column's taps stay in registers, the row's taps are wave-uniform), each channel plane stored along x.
#include "common.h"

namespace {

constexpr int PRE_NT = 256;
constexpr int PRE_ROWS = 4;

struct PreImage {
  const unsigned char* src;   // [h][row_stride] bytes, 3 per pixel
  int h, w, row_stride;
  int nh, nw, flip;
  int x_row0, y_row0;         // first rows of the image's column / row taps in the tap table
};

struct PreArgs {
  PreImage img[DM_PREPROCESS_MAX_IMAGES];
  const int* taps;            // [tap_rows][4] = (i0, i1, c0, c1)
  float mean[3], stdinv[3];
  int to_rgb;
  float* out;
  int Hp, Wp;
};

__global__ __launch_bounds__(PRE_NT) void preprocess_u8_kernel(PreArgs a) {
#pragma clang fp contract(off)
  const PreImage& im = a.img[blockIdx.z];
  const int x = blockIdx.x * PRE_NT + threadIdx.x;
  if (x >= a.Wp) return;
  const bool in_x = x < im.nw;
  int x0 = 0, x1 = 0, a0 = 0, a1 = 0;
  if (in_x) {
    const int xs = im.flip == DM_AUG_FLIP_HORIZONTAL ? im.nw - 1 - x : x;
    const int4 t = *reinterpret_cast<const int4*>(a.taps + 4 * (size_t)(im.x_row0 + xs));
    x0 = 3 * min(max(t.x, 0), im.w - 1);
    x1 = 3 * min(max(t.y, 0), im.w - 1);
    a0 = t.z; a1 = t.w;
  }
  const size_t plane = (size_t)a.Hp * a.Wp;
  float* o = a.out + (size_t)blockIdx.z * 3 * plane + x;
  const int y_end = min((int)(blockIdx.y + 1) * PRE_ROWS, a.Hp);
  for (int y = blockIdx.y * PRE_ROWS; y < y_end; ++y) {
    float v[3] = {0.f, 0.f, 0.f};
    if (in_x && y < im.nh) {
      const int ys = im.flip == DM_AUG_FLIP_VERTICAL ? im.nh - 1 - y : y;
      const int* ty = a.taps + 4 * (size_t)(im.y_row0 + ys);
      const int y0 = min(max(ty[0], 0), im.h - 1), y1 = min(max(ty[1], 0), im.h - 1);
      const int b0 = ty[2], b1 = ty[3];
      const unsigned char* top = im.src + (size_t)y0 * im.row_stride;
      const unsigned char* bot = im.src + (size_t)y1 * im.row_stride;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sc = a.to_rgb ? 2 - c : c;
        const int rt = (int)top[x0 + sc] * a0 + (int)top[x1 + sc] * a1;
        const int rb = (int)bot[x0 + sc] * a0 + (int)bot[x1 + sc] * a1;
        int p = (((b0 * (rt >> 4)) >> 16) + ((b1 * (rb >> 4)) >> 16) + 2) >> 2;
        p = min(max(p, 0), 255);
        v[c] = ((float)p - a.mean[c]) * a.stdinv[c];
      }
    }
    float* oy = o + (size_t)y * a.Wp;
    oy[0] = v[0];
    oy[plane] = v[1];
    oy[2 * plane] = v[2];
  }
}

}  // namespace

extern "C" int dm_preprocess_u8_supported(int B, const int* dims, long long tap_rows, int Hp, int Wp) {
  if (B < 0 || B > DM_PREPROCESS_MAX_IMAGES || Hp < 1 || Wp < 1 || Hp > (1 << 24) || Wp > (1 << 24) || tap_rows < 0) return 0;
  if (B > 0 && !dims) return 0;
  if (dm_ceil_div(Hp, PRE_ROWS) > 65535) return 0;
  for (int b = 0; b < B; ++b) {
    const int* d = dims + (size_t)b * DM_PREPROCESS_DIMS;
    const int h = d[0], w = d[1], nh = d[3], nw = d[4], flip = d[5];
    const long long stride = d[2], xr = d[6], yr = d[7];
    if (h < 1 || w < 1 || nh < 1 || nw < 1 || nh > Hp || nw > Wp || w > (1 << 24) || h > (1 << 24)) return 0;
    if (stride < 3LL * w) return 0;
    if (flip != DM_AUG_FLIP_NONE && flip != DM_AUG_FLIP_HORIZONTAL && flip != DM_AUG_FLIP_VERTICAL) return 0;
    if (xr < 0 || yr < 0 || xr + nw > tap_rows || yr + nh > tap_rows) return 0;
  }
  return 1;
}

extern "C" int dm_preprocess_u8_fwd(const uint8_t* const* srcs, const int* dims, int B, const int32_t* taps,
                                    long long tap_rows, const float* mean, const float* stdinv, int to_rgb, float* out,
                                    int Hp, int Wp, dm_stream_t stream) {
  if (!dm_preprocess_u8_supported(B, dims, tap_rows, Hp, Wp)) return DM_ERR_UNSUPPORTED;
  if (B == 0) return DM_OK;
  if (!srcs || !taps || !mean || !stdinv || !out || ((uintptr_t)taps & 15)) return DM_ERR_INVALID_ARG;
  PreArgs a = {};
  for (int b = 0; b < B; ++b) {
    const int* d = dims + (size_t)b * DM_PREPROCESS_DIMS;
    if (!srcs[b]) return DM_ERR_INVALID_ARG;
    PreImage& im = a.img[b];
    im.src = srcs[b];
    im.h = d[0]; im.w = d[1]; im.row_stride = d[2];
    im.nh = d[3]; im.nw = d[4]; im.flip = d[5];
    im.x_row0 = d[6]; im.y_row0 = d[7];
  }
  a.taps = taps;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdinv[c] = stdinv[c]; }
  a.to_rgb = to_rgb ? 1 : 0;
  a.out = out; a.Hp = Hp; a.Wp = Wp;
  DM_LAUNCH(preprocess_u8_kernel, dim3(dm_ceil_div(Wp, PRE_NT), dm_ceil_div(Hp, PRE_ROWS), B), dim3(PRE_NT), 0,
            (hipStream_t)stream, a);
  return dm_check_launch();
}
