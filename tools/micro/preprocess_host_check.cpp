// Host side of the image pre-processing launcher (csrc/preprocess.hip) under AddressSanitizer, no device needed: the
// support check at its limits and the argument validation with bad arguments -- every call returns before anything is
// enqueued.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Iinclude -Idynamask_amd/csrc \
//       dynamask_amd/csrc/preprocess.hip tools/micro/preprocess_host_check.cpp -o preprocess_host_check && ./preprocess_host_check
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "dynamask_hip.h"

static int failures = 0;
#define EXPECT(expr, want)                                                        \
  do {                                                                            \
    const long long got_ = (long long)(expr);                                     \
    if (got_ != (long long)(want)) {                                              \
      printf("FAIL %s = %lld, expected %lld\n", #expr, got_, (long long)(want));  \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

// one image's row of `dims`
static void row(std::vector<int>& d, int h, int w, int stride, int nh, int nw, int flip, int xr, int yr) {
  const int v[DM_PREPROCESS_DIMS] = {h, w, stride, nh, nw, flip, xr, yr};
  d.insert(d.end(), v, v + DM_PREPROCESS_DIMS);
}

static int one(int h, int w, int stride, int nh, int nw, int flip, int xr, int yr, long long tap_rows, int Hp, int Wp) {
  std::vector<int> d;          // exactly one row: a read past it is a finding
  row(d, h, w, stride, nh, nw, flip, xr, yr);
  return dm_preprocess_u8_supported(1, d.data(), tap_rows, Hp, Wp);
}

int main() {
  // dm_preprocess_u8_supported
  EXPECT(one(1, 1, 3, 1, 1, DM_AUG_FLIP_NONE, 0, 1, 2, 32, 32), 1);
  EXPECT(one(750, 1250, 3750, 800, 1333, DM_AUG_FLIP_HORIZONTAL, 0, 1333, 2133, 800, 1344), 1);
  EXPECT(one(37, 53, 240, 50, 72, DM_AUG_FLIP_VERTICAL, 0, 72, 122, 64, 96), 1);
  EXPECT(one(0, 53, 240, 50, 72, 0, 0, 72, 122, 64, 96), 0);               // sizes below 1
  EXPECT(one(37, 0, 240, 50, 72, 0, 0, 72, 122, 64, 96), 0);
  EXPECT(one(37, 53, 240, 0, 72, 0, 0, 72, 122, 64, 96), 0);               // n_dst < 1
  EXPECT(one(37, 53, 240, 50, -1, 0, 0, 72, 122, 64, 96), 0);
  EXPECT(one(37, 53, 158, 50, 72, 0, 0, 72, 122, 64, 96), 0);              // row stride below 3 w
  EXPECT(one(37, 53, 159, 50, 72, 0, 0, 72, 122, 64, 96), 1);
  EXPECT(one(37, 53, 240, 65, 72, 0, 0, 72, 137, 64, 96), 0);              // does not fit the padded output
  EXPECT(one(37, 53, 240, 50, 97, 0, 0, 97, 147, 64, 96), 0);
  EXPECT(one(37, 53, 240, 50, 72, 3, 0, 72, 122, 64, 96), 0);              // no such flip
  EXPECT(one(37, 53, 240, 50, 72, -1, 0, 72, 122, 64, 96), 0);
  EXPECT(one(37, 53, 240, 50, 72, 0, -1, 72, 122, 64, 96), 0);             // taps outside the table
  EXPECT(one(37, 53, 240, 50, 72, 0, 51, 72, 122, 64, 96), 0);
  EXPECT(one(37, 53, 240, 50, 72, 0, 0, 73, 122, 64, 96), 0);
  EXPECT(one(37, 53, 240, 50, 72, 0, 0, 72, -1, 64, 96), 0);
  EXPECT(one(37, 53, 240, 50, 72, 0, 0x7fffffff, 0x7fffffff, 122, 64, 96), 0);
  EXPECT(one(37, 53, 240, 50, 72, 0, 0, 72, 122, 0, 96), 0);               // the output
  EXPECT(one(37, 53, 240, 50, 72, 0, 0, 72, 122, 64, (1 << 24) + 1), 0);
  EXPECT(one(37, 53, 240, 50, 72, 0, 0, 72, 122, 4 * 65535 + 1, 96), 0);   // rows beyond the grid
  EXPECT(one(37, 53, 240, 50, 72, 0, 0, 72, 122, 4 * 65535, 96), 1);
  EXPECT(one((1 << 24) + 1, 53, 240, 50, 72, 0, 0, 72, 122, 64, 96), 0);
  EXPECT(dm_preprocess_u8_supported(0, nullptr, 0, 32, 32), 1);            // no image: nothing to read
  EXPECT(dm_preprocess_u8_supported(1, nullptr, 0, 32, 32), 0);
  EXPECT(dm_preprocess_u8_supported(-1, nullptr, 0, 32, 32), 0);
  {
    std::vector<int> d;
    for (int b = 0; b < DM_PREPROCESS_MAX_IMAGES + 1; ++b) row(d, 4, 4, 12, 4, 4, 0, 0, 0);
    EXPECT(dm_preprocess_u8_supported(DM_PREPROCESS_MAX_IMAGES, d.data(), 4, 32, 32), 1);
    EXPECT(dm_preprocess_u8_supported(DM_PREPROCESS_MAX_IMAGES + 1, d.data(), 4, 32, 32), 0);
  }
  // dm_preprocess_u8_fwd: the support check first, then the pointers
  std::vector<int> d;
  row(d, 4, 4, 12, 4, 4, 0, 0, 0);
  alignas(16) int32_t taps[4 * 4] = {0};
  uint8_t img[48] = {0};
  const uint8_t* srcs[1] = {img};
  const uint8_t* none[1] = {nullptr};
  float mean[3] = {0}, stdinv[3] = {1, 1, 1}, out[3 * 32 * 32];
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 0, taps, 4, mean, stdinv, 1, out, 32, 32, nullptr), DM_OK);      // nothing to do
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps, 3, mean, stdinv, 1, out, 32, 32, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps, 4, mean, stdinv, 1, out, 2, 32, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), DM_PREPROCESS_MAX_IMAGES + 1, taps, 4, mean, stdinv, 1, out, 32, 32, nullptr),
         DM_ERR_UNSUPPORTED);
  EXPECT(dm_preprocess_u8_fwd(nullptr, d.data(), 1, taps, 4, mean, stdinv, 1, out, 32, 32, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_preprocess_u8_fwd(none, d.data(), 1, taps, 4, mean, stdinv, 1, out, 32, 32, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, nullptr, 4, mean, stdinv, 1, out, 32, 32, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps + 1, 3, mean, stdinv, 1, out, 32, 32, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps + 1, 4, mean, stdinv, 1, out, 32, 32, nullptr), DM_ERR_INVALID_ARG);   // misaligned
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps, 4, nullptr, stdinv, 1, out, 32, 32, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps, 4, mean, nullptr, 1, out, 32, 32, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_preprocess_u8_fwd(srcs, d.data(), 1, taps, 4, mean, stdinv, 1, nullptr, 32, 32, nullptr), DM_ERR_INVALID_ARG);
  printf(failures ? "%d check(s) failed\n" : "preprocess host checks: all passed\n", failures);
  return failures ? 1 : 0;
}
