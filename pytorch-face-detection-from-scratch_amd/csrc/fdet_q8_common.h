// The one statement of the int8 (Q8) activation layout and of every float step of the int8 contract of include/fdet.h
// ("Int8 inference"): the numpy restatements under tests/ (q8_cpu_ref.py and its siblings) say the same in numpy and the GPU
// tests demand equality, so a change here changes every int8 kernel at once.  Device code is __forceinline__; nothing here is
// a kernel or an entry point.
//
// Activation layout: int8 [N][H+2][W+2][C], channel innermost, a one-pixel halo of zeros round every image.  Symmetric
// quantisation never produces -128, so the halo byte 0 is the real zero and a conv needs no bounds test.  Producers write
// real pixels only: a buffer that keeps its shape keeps its halo.
#pragma once
#include "fdet_common.h"

namespace fdet {
namespace q8 {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int ROWS = 4;               // map rows per conv work item (one wave): 4 rows x 16 columns
constexpr int MAX_C = 256;
constexpr int MAX_HW = 4096;
constexpr size_t LDS_MAX = 160 * 1024;

// c_mult: 64 for the square entries (fdet_q8_*), 16 for the mixed-width ones (fdet_q8x_*)
__host__ __device__ constexpr bool act_shape_ok(int C, int H, int W, int c_mult) {
  return C >= c_mult && C <= MAX_C && C % c_mult == 0 && H >= 1 && W >= 1 && H <= MAX_HW && W <= MAX_HW;
}

// bytes of N images, 0 when the shape has no layout or the tensor passes 2^31 - 1 bytes (32-bit offsets inside the kernels)
inline size_t act_bytes(int N, int C, int H, int W, int c_mult) {
  if (N < 1 || !act_shape_ok(C, H, W, c_mult)) return 0;
  const unsigned long long b = (unsigned long long)N * (H + 2) * (W + 2) * C;
  return b < (1ull << 31) ? (size_t)b : 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// clamp(rintf(t), -127, 127): round half to even, -128 never produced
__device__ __forceinline__ int round_q(float t) {
  return (int)fminf(fmaxf(rintf(t), -127.0f), 127.0f);
}

// fdet_q8_quantize's rounding of one product: a NaN product (NaN input, or 0 * inf under a denormal scale) -> 0
__device__ __forceinline__ int round_q_nan0(float t) { return t == t ? round_q(t) : 0; }

__device__ __forceinline__ int pack4(int a, int b, int c, int d) {
  return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | (int)((unsigned)(d & 255) << 24);
}

__device__ __forceinline__ int byte_of(int w, int r) {
  return (int)(signed char)((unsigned)w >> (8 * r));
}

__device__ __forceinline__ float lrelu(float v, float slope) { return v >= 0.0f ? v : v * slope; }

// bytewise signed max of two packed dwords
__device__ __forceinline__ int max4(int a, int b) {
  return pack4(max(byte_of(a, 0), byte_of(b, 0)), max(byte_of(a, 1), byte_of(b, 1)), max(byte_of(a, 2), byte_of(b, 2)),
               max(byte_of(a, 3), byte_of(b, 3)));
}

// The requantising epilogue of a conv on four channels of one pixel: multiplier, LeakyReLU, skip code times skip_mul, round.
__device__ __forceinline__ void requant4(int (&q)[4], v4i acc, v4f m, float slope, bool has_skip, int sk, float skip_mul) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = lrelu((float)acc[r] * m[r], slope);
    if (has_skip) v = v + (float)byte_of(sk, r) * skip_mul;
    q[r] = round_q(v);
  }
}

// The nine taps of a 3x3 conv on one 64-channel chunk: a work item's ROWS rows x 16 columns x 16 NT output channels from its
// 18 preloaded pixel fragments b[padded row][kx] (row j, tap ky -> b[j + ky]), each used by up to three (row, tap) pairs.
// Weights come from LDS: tile t of tap `tap` at w + tap * tap_stride + t * 1024 (w already points at the lane's 16 bytes).
//   A (weights): lane l holds 16 consecutive ci bytes of row co = 16 t + (l & 15), starting at ci = 16 (l >> 4)
//   B (pixels):  lane l holds the same 16 ci of pixel column (l & 15)
//   D:           lane l holds co = 16 t + 4 (l >> 4) + r (r = 0..3) of pixel (l & 15): four channels = one dword store
// Both operands take their k from the same 16-byte channel run, so the sum does not depend on how the instruction orders k
// inside a lane's fragment; the one-hot tests (tests/test_gpu_q8.py) check rows, columns and taps.
template <int NT>
__device__ __forceinline__ void taps9(v4i (&acc)[ROWS][NT], const v4i (&b)[ROWS + 2][3], const unsigned char* w, int tap_stride) {
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - 3 * (tap / 3);
    v4i a[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const v4i*>(w + (size_t)tap * tap_stride + t * 1024);
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[j][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b[j + ky][kx], acc[j][t], 0, 0, 0);
  }
}

// The integer stems stage the frame codes 0..255 as x - 128 (the MFMA multiplies signed by signed), so
//     sum x * w = sum (x - 128) * w + 128 * sum_k w[co][k]
// and the last term joins the bias.  stem_offset: that constant and the multiplier of four consecutive channels, from
// wsum = the channels' weight sums in the accumulators' own layout (the caller's MFMAs against a B of ones).  Wrapping adds:
// the exact sum fits where the contract's acc does.  A kernel whose lane holds 16 channels calls both once per dword.
__device__ __forceinline__ void stem_offset(unsigned (&cst)[4], float (&m)[4], const int* bias, const float* mul, v4i wsum) {
  const v4f mv = *reinterpret_cast<const v4f*>(mul);
  const v4i bv = *reinterpret_cast<const v4i*>(bias);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = mv[r];
    cst[r] = (unsigned)bv[r] + 128u * (unsigned)wsum[r];
  }
}

// the packed dword of four channels of one stem output pixel
__device__ __forceinline__ int stem_requant(v4i acc, const unsigned (&cst)[4], const float (&m)[4]) {
  int q[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = round_q((float)(int)((unsigned)acc[r] + cst[r]) * m[r]);
  return pack4(q[0], q[1], q[2], q[3]);
}

}  // namespace q8
}  // namespace fdet
