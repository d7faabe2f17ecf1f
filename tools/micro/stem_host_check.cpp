// Host side of the stem launchers (csrc/stem.hip) under AddressSanitizer, no device needed: the support checks at their
// limits and the argument validation with bad arguments -- every call returns before anything is enqueued.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address -Iinclude -Idynamask_amd/csrc \
//       dynamask_amd/csrc/stem.hip tools/micro/stem_host_check.cpp -o stem_host_check && ./stem_host_check
#include <stdio.h>

#include "dynamask_hip.h"

// the one symbol stem.hip takes from another file of the library (csrc/conv_igemm.hip), restated for this program alone
extern "C" int dm_conv_packed_cout(int Cout) { return (Cout + 31) / 32 * 32; }

static int failures = 0;
#define EXPECT(expr, want)                                                        \
  do {                                                                            \
    const long long got_ = (long long)(expr);                                     \
    if (got_ != (long long)(want)) {                                              \
      printf("FAIL %s = %lld, expected %lld\n", #expr, got_, (long long)(want));  \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

int main() {
  float x[3 * 8 * 8] = {0}, w[42 * 64 * 4] = {0}, out[64 * 4 * 4] = {0};
  // dm_conv7x7_s2_supported
  EXPECT(dm_conv7x7_s2_supported(1, 3, 1, 1, 1), 1);
  EXPECT(dm_conv7x7_s2_supported(4, 3, 800, 1344, 64), 1);
  EXPECT(dm_conv7x7_s2_supported(2, 3, 37, 53, 24), 1);
  EXPECT(dm_conv7x7_s2_supported(0, 3, 8, 8, 64), 0);
  EXPECT(dm_conv7x7_s2_supported(-1, 3, 8, 8, 64), 0);
  EXPECT(dm_conv7x7_s2_supported(1, 3, 0, 8, 64), 0);
  EXPECT(dm_conv7x7_s2_supported(1, 3, 8, -8, 64), 0);
  EXPECT(dm_conv7x7_s2_supported(1, 3, 8, 8, 0), 0);
  for (int C = -1; C <= 9; ++C) EXPECT(dm_conv7x7_s2_supported(1, C, 8, 8, 64), C == 3 ? 1 : 0);
  EXPECT(dm_conv7x7_s2_supported(1, 3, 16, 32, 64 * 65536), 1);
  EXPECT(dm_conv7x7_s2_supported(32768, 3, 16, 32, 64 * 65536), 0);            // 2^31 workgroups
  EXPECT(dm_conv7x7_s2_supported(0x7fffffff, 3, 0x7fffffff, 0x7fffffff, 0x7fffffff), 0);
  // dm_conv7x7_s2_fwd: null pointers, flags, shapes -- in that order
  EXPECT(dm_conv7x7_s2_fwd(nullptr, 1, 3, 8, 8, w, nullptr, 64, 0, out, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, nullptr, nullptr, 64, 0, out, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, 64, 0, nullptr, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, 64, 16, out, nullptr), DM_ERR_UNSUPPORTED);      // bf16x3
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, 64, 17, out, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, 64, 2, out, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, 64, 4, out, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, 64, -1 & ~16, out, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 5, 8, 8, w, nullptr, 64, 0, out, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_conv7x7_s2_fwd(x, 0, 3, 8, 8, w, nullptr, 64, 1, out, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 0, w, nullptr, 64, 1, out, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_conv7x7_s2_fwd(x, 1, 3, 8, 8, w, nullptr, -64, 1, out, nullptr), DM_ERR_UNSUPPORTED);
  // dm_maxpool3x3_s2_*
  EXPECT(dm_maxpool3x3_s2_supported(0, 1, 1), 1);
  EXPECT(dm_maxpool3x3_s2_supported(4 * 64, 400, 672), 1);
  EXPECT(dm_maxpool3x3_s2_supported(-1, 4, 4), 0);
  EXPECT(dm_maxpool3x3_s2_supported(1, 0, 4), 0);
  EXPECT(dm_maxpool3x3_s2_supported(1, 4, -1), 0);
  EXPECT(dm_maxpool3x3_s2_supported(1LL << 40, 1, 1), 1);
  EXPECT(dm_maxpool3x3_s2_supported((1LL << 40) + 1, 1, 1), 0);
  EXPECT(dm_maxpool3x3_s2_supported(1LL << 62, 0x7fffffff, 0x7fffffff), 0);
  EXPECT(dm_maxpool3x3_s2_fwd(x, 0, 8, 8, out, nullptr), DM_OK);               // nothing to do
  EXPECT(dm_maxpool3x3_s2_fwd(nullptr, 0, 8, 8, nullptr, nullptr), DM_OK);
  EXPECT(dm_maxpool3x3_s2_fwd(nullptr, 3, 8, 8, out, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_maxpool3x3_s2_fwd(x, 3, 8, 8, nullptr, nullptr), DM_ERR_INVALID_ARG);
  EXPECT(dm_maxpool3x3_s2_fwd(x, -3, 8, 8, out, nullptr), DM_ERR_UNSUPPORTED);
  EXPECT(dm_maxpool3x3_s2_fwd(x, 3, 0, 8, out, nullptr), DM_ERR_UNSUPPORTED);
  printf(failures ? "%d check(s) failed\n" : "stem host checks: all passed\n", failures);
  return failures ? 1 : 0;
}
