// Shared helpers for the gfx950 kernels of libdynamask_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "dynamask_hip.h"

#define DM_WAVE 64

static inline int dm_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// hipGetLastError() is sticky per thread: a benign error left behind by another
// library's HIP call (torch probing peer access, an event query returning
// "not ready") would otherwise be blamed on our launch.  Clear it first.
#define DM_LAUNCH(...)        \
  do {                        \
    (void)hipGetLastError();  \
    hipLaunchKernelGGL(__VA_ARGS__); \
  } while (0)

// Post-launch check: the launch itself is asynchronous; configuration errors
// (bad grid, too much LDS) surface here.
static inline int dm_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DM_OK : DM_ERR_LAUNCH;
}

// dm_reload_env_knobs (roi_align.hip) also re-reads DM_GN_WIDE, which lives with the GroupNorm launcher (grid_head.hip).
void dm_gn_reload_knobs();

// Per-device facts.  One process may drive several devices (a rehearsal of ranks on one box, a
// single-process multi-GPU caller): compute-unit counts and "this kernel's LDS limit has been
// raised" flags are properties of a device, not of the process, so they are kept per device.
// (A benign race between two host threads only repeats an idempotent call.)
#define DM_MAX_DEVICES 64

static inline int dm_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= DM_MAX_DEVICES) dev = 0;
  return dev;
}

// Compute units of the current device (MI355X: 256).
static inline int dm_num_cus() {
  static int cus[DM_MAX_DEVICES] = {0};
  const int dev = dm_current_device();
  if (cus[dev] == 0) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}

// Raise a kernel's dynamic-LDS limit once per device.  `flags` is a static array of
// DM_MAX_DEVICES bools owned by the call site (one per kernel).
static inline int dm_ensure_lds_limit(const void* kernel, int bytes, bool* flags) {
  const int dev = dm_current_device();
  if (!flags[dev]) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return DM_ERR_LAUNCH;
    flags[dev] = true;
  }
  return DM_OK;
}

// ---- order-independent accumulation (deterministic mode; dynamask_hip.h "Deterministic accumulation") ----
// The *_fx entry points add into 64-bit fixed-point cells (value * 2^36, two's complement through the u64 atomic)
// instead of float cells: integer addition is associative, so the sum does not depend on the order in which
// workgroups arrive.  The contract (resolution, ranges, poison) is in dynamask_hip.h, "Fixed-point accumulators".
#define DM_FX_ONE 68719476736.0 /* 2^36 */
#define DM_FIX_ADDEND_MAX 134217728.f /* 2^27: what dm_fix36_mul / dm_fix36_abs16 convert without saturating */
// g * w -> the same 2^-36 fixed point in eight fp32 / integer instructions (the fp64 route -- a double multiply and
// __double2ll_rn, for which there is no hardware convert -- is ~11 and the DCN col2im is bound by exactly these: 5.3e8
// vector instructions per launch, its VALU pipe 100 % busy).  The caller passes w16 = w * 2^4 and w36 = w * 2^36 (exact
// scalings, shared by the channels of a sample): t = g * w16 and p = g * w36 are the same rounded product at two scales;
// hi = rne(t) is bits 63..32 (+ a borrow), p - hi * 2^32 is exact in fp32 (|.| <= 2^31, a multiple of p's ulp) and its
// integer part is the signed low word.  Finite g * w with |g * w| < 2^27; the fraction below 2^-36 is truncated.
__device__ __forceinline__ unsigned long long dm_fix36_mul(float g, float w16, float w36) {
  const float hi_f = __builtin_rintf(g * w16);
  const float rem = __builtin_fmaf(hi_f, -4294967296.0f, g * w36);
  const int lo = (int)rem;
  const int hi = (int)hi_f + (lo >> 31);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}

// |value| * 2^36 from t16 = value * 2^4 in four instructions: the high word is trunc(|t16|), the low word its fraction
// * 2^32 (exact for a non-negative number: a subset of its mantissa bits; a negative one has no such split -- 1 - 2^-40
// is not a float -- which is why the sign goes into the choice of ds_add_u64 / ds_sub_u64 instead: dm_fix36_accumulate).
// |value| < 2^27; the fraction below 2^-36 is truncated towards zero, as in dm_fix36_mul.
__device__ __forceinline__ unsigned long long dm_fix36_abs16(float t16) {
  const float m = __builtin_fabsf(t16);
  const unsigned hi = (unsigned)m;
  const unsigned lo = (unsigned)(__builtin_amdgcn_fractf(m) * 4294967296.0f);
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}
__device__ __forceinline__ void dm_fix36_accumulate(unsigned long long* cell, float t16) {
  const unsigned long long mag = dm_fix36_abs16(t16);
  if (t16 < 0.f) atomicSub(cell, mag);
  else atomicAdd(cell, mag);
}

// An addend an fx cell cannot hold (NaN, Inf, |v| >= DM_FX_ADDEND_MAX = 2^25) POISONS the cell: a signed maximum with
// LLONG_MAX.  The maximum absorbs (adding a marker does not: four markers of 2^62 sum to 0 mod 2^64 and the cell read
// as clean): whatever the cell held and however many bad addends arrive it is LLONG_MAX afterwards, and in-range addends
// that follow (|their sum| < 2^61) leave it at |q| >= 2^61, which dm_fx_to_float reads as NaN.
#define DM_FX_ADDEND_MAX 33554432.f    /* 2^25: |v| * 2^36 < 2^61, below the poison threshold */
#define DM_FX_POISON 0x7fffffffffffffffLL
#define DM_FX_POISON_MIN (1LL << 61)   /* |cell| >= this: poisoned */
__device__ __forceinline__ void dm_fx_poison(unsigned long long* cell) {
  atomicMax(reinterpret_cast<long long*>(cell), DM_FX_POISON);
}
// a sum that is already in the cells' format (the LDS tiles' flush)
__device__ __forceinline__ void dm_fx_add_q(unsigned long long* cell, long long q, bool bad) {
  if (bad || q >= DM_FX_POISON_MIN || q <= -DM_FX_POISON_MIN) dm_fx_poison(cell);
  else atomicAdd(cell, (unsigned long long)q);
}
__device__ __forceinline__ void dm_fx_add(unsigned long long* cell, float v) {
  if (__builtin_fabsf(v) < DM_FX_ADDEND_MAX) atomicAdd(cell, (unsigned long long)__double2ll_rn((double)v * DM_FX_ONE));
  else dm_fx_poison(cell);
}
// accumulate v into cell idx of an accumulator that is float (fx = false) or 64-bit fixed point (fx = true)
__device__ __forceinline__ void dm_acc_add(float* base, size_t idx, float v, bool fx) {
  if (fx) dm_fx_add(reinterpret_cast<unsigned long long*>(base) + idx, v);
  else atomicAdd(base + idx, v);
}

// The logistic function of the paste kernels' apply_sigmoid (paste_masks_kernel, PasteSrc) and of the TTA mask merge
// (dm_merge_aug_masks): one expression, so that a merged probability is bit for bit what the paste computes from the logit.
__device__ __forceinline__ float dm_sigmoid(float t) { return 1.f / (1.f + expf(-t)); }

// ReLU as torch.relu computes it: NaN stays NaN (fmaxf(v, 0.f) returns its non-NaN operand, so it erased a NaN born in
// the accumulation), -0 stays -0, every other value is fmaxf's.  A compare and a select: as many instructions as the
// two v_max_f32 it replaces.  Every fused ReLU of the library is this one expression (the fused launches promise the bits
// of the unfused sequences).
__device__ __forceinline__ float dm_relu(float v) { return v < 0.f ? 0.f : v; }

// The ReLU looking backward, autograd's threshold_backward: the gradient g is zeroed where the forward output y <= 0, so it
// passes at y = NaN (the forward's NaN is already in every product g meets further down).
__device__ __forceinline__ float dm_relu_mask(float y, float g) { return y <= 0.f ? 0.f : g; }

// Running maximum of a pooling window in torch's max_pool2d order: a later element replaces the maximum when it is larger
// or NaN, and a NaN stays (the rule of dm_mask_iou_input, csrc/conv_strided.hip).
__device__ __forceinline__ bool dm_pool_takes(float v, float best) { return v > best || v != v; }

typedef float dm_f32x16 __attribute__((ext_vector_type(16)));
typedef float dm_f32x4 __attribute__((ext_vector_type(4)));
