// Shared host-side helpers for libfdet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/fdet.h"

namespace fdet {

inline char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FDET_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return FDET_OK;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) with its result checked (a kernel that needs more than 64 KB of LDS
// fails at launch with an unhelpful error otherwise)
inline int set_lds_attr(const void* kern, size_t lds, const char* what) {
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FDET_ELAUNCH, "%s: cannot reserve %zu bytes of LDS", what, lds);
  }
  return FDET_OK;
}
// environment switch read once per call site (launch paths are hot on the launch-bound demo path)
#define FDET_ENV_ONCE(NAME) ([]() -> const char* { static const char* v_ = getenv(NAME); return v_; }())

// compute units of the current device, asked once per process (256 where the query fails)
inline int num_cus() {
  static int ncu = 0;
  if (ncu == 0) {
    int dev = 0, v = 0;
    ncu = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return ncu;
}

// record of the kernels a stem call launched (fdet_stem_last_route, fdet_stem.hip); the first launch of a call sets the fields
enum { STEM_VALU_K10 = FDET_STEM_VALU_K10, STEM_VALU_K3_GENERIC = FDET_STEM_VALU_K3_GENERIC, STEM_VALU_K3_SCALAR = FDET_STEM_VALU_K3_SCALAR,
       STEM_MFMA = FDET_STEM_MFMA, STEM_X3_SINGLE = FDET_STEM_X3_SINGLE, STEM_X3_PIPE = FDET_STEM_X3_PIPE,
       STEM_K3_MATRIX = FDET_STEM_K3_MATRIX, STEM_K3_PS_FWD = FDET_STEM_K3_PS_FWD, STEM_PASS_FWD = 1, STEM_PASS_WGRAD = 2 };
void stem_note_route(int family, int pass, bool p16, bool u8, bool ps, int grid, int items);
void stem_clear_route();

constexpr int WAVE = 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;   // valid in lane 0
}
__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// x / 255 for an integer 0 <= x <= 255, bit-identical to the IEEE division: q = x * fl(1/255) is off by an ulp for 126 of the
// 256 values, one residual correction (two FMAs) makes all 256 exact (tests/test_gpu_detect.py::test_u8_norm_bit_exact covers
// every value).  fdet_u8_to_f32_norm (fdet_detect.hip) and fdet_aug_finish (fdet_augment.hip) share it.
__device__ __forceinline__ float u8_over_255(float x) {
  const float r = 1.0f / 255.0f;
  const float q = x * r;
  const float rem = __builtin_fmaf(-q, 255.0f, x);
  return __builtin_fmaf(rem, r, q);
}

}  // namespace fdet

#define FDET_REQUIRE(cond, ...) \
  do { if (!(cond)) return fdet::fail(FDET_EINVAL, __VA_ARGS__); } while (0)
