// What the two integer 3x3 / stride 2 / pad 1 stem kernels share (k_stem3_q8 in fdet_stem_q8.hip: 64 output channels per
// workgroup; k_stem3_q8x in fdet_q8_ssd.hip: 16): the launch geometry, the staging of the input rows in LDS as x - 128, the
// tap offsets of a lane's B operand and its gather.  Device code only; the channel tiling and the epilogue are each kernel's.
#pragma once
#include "fdet_common.h"

namespace fdet {
namespace s3 {

constexpr int ROWS = 4;                             // output rows per workgroup: one per wave
constexpr int SEG = 256;                            // output columns per workgroup: 16 MFMA column tiles
constexpr int IN_ROWS = 2 * ROWS + 1;               // input rows under ROWS output rows
constexpr int RS = 2 * SEG + 16;                    // bytes of one staged input row: image columns 2 ox0 - 4 .. 2 ox0 + 2 SEG + 11
constexpr int LDS = 3 * IN_ROWS * RS;               // 14,256 bytes
constexpr long long MAX_ITEMS = 1ll << 20;          // workgroups per launch (larger batches: consecutive launches)

struct Args {
  const unsigned char* frames;
  const signed char* w;                              // [F][32]
  const int* bias;
  const float* mul;
  signed char* q;
  int N, F, H, W, Ho, Wo;
  int segs, row_groups;
  int dwords;                                        // 1: W % 4 == 0 and a 4-byte aligned frame pointer, rows are read as dwords
};

struct Item {
  int n, ox0, oy0, ntiles;
};

// workgroup blockIdx.x -> (image, group of ROWS output rows, segment of SEG output columns)
__device__ __forceinline__ Item item_of(const Args& a, int item) {
  const int per_img = a.segs * a.row_groups;
  const int n = item / per_img;
  const int rem = item - n * per_img;
  const int rg = rem / a.segs;
  const int ox0 = (rem - rg * a.segs) * SEG;
  return Item{n, ox0, rg * ROWS, (min(SEG, a.Wo - ox0) + 15) >> 4};
}

// The 9 input rows x 3 channels under the workgroup's output rows.  LDS row (ci, iy) holds input row 2 oy0 - 1 + iy of channel
// ci; its byte i is image column 2 ox0 - 4 + i, stored as x - 128 (the byte x ^ 0x80), everything outside the image as -128
// (the code 0 that the contract's zero padding stands for).  No barrier here: the caller has one before the first gather.
__device__ __forceinline__ void stage_rows(const Args& a, const Item& it, unsigned char* rows) {
  const int nd = ((32 * it.ntiles + 3) >> 2) + 1;          // dwords of a staged row that the tiles read (bytes 3 .. 32 ntiles + 3)
  const int c0 = 2 * it.ox0 - 4;                            // image column of byte 0 (a multiple of 4)
  const int y0 = 2 * it.oy0 - 1;
  for (int u = threadIdx.x; u < 3 * IN_ROWS * nd; u += 256) {
    const int lr = u / nd, d = u - lr * nd;
    const int ci = lr / IN_ROWS, iy = lr - ci * IN_ROWS;
    const int y = y0 + iy, c = c0 + 4 * d;
    unsigned v = 0;                                         // outside the image: code 0
    if (y >= 0 && y < a.H && c + 3 >= 0 && c < a.W) {
      const unsigned char* src = a.frames + ((size_t)(it.n * 3 + ci) * a.H + y) * a.W;
      if (a.dwords) {                                       // c and W are multiples of 4: the dword is inside the row as a whole
        v = *reinterpret_cast<const unsigned*>(src + c);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (c + b >= 0 && c + b < a.W) v |= (unsigned)src[c + b] << (8 * b);
      }
    }
    *reinterpret_cast<unsigned*>(rows + lr * RS + 4 * d) = v ^ 0x80808080u;          // x - 128 as a signed byte
  }
}

// B operand of lane (lp = lane & 15, lk = lane >> 4) of wave j: tap k = 8 lk + e -> LDS row (ci, 2 j + ky), byte
// 2 (ox - ox0) + kx + 3; taps 27..31 read tap 26 again (weight zero)
__device__ __forceinline__ void tap_offsets(int (&off)[8], int lk, int lp, int j) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = min(8 * lk + e, 26);
    const int ci = k / 9, ky = (k - 9 * ci) / 3, kx = k - 9 * ci - 3 * ky;
    off[e] = (ci * IN_ROWS + 2 * j + ky) * RS + kx + 3 + 2 * lp;
  }
}

__device__ __forceinline__ long gather(const unsigned char* rows, const int (&off)[8], int tile) {
  unsigned lo = 0, hi = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo |= (unsigned)rows[off[e] + 32 * tile] << (8 * e);
    hi |= (unsigned)rows[off[e + 4] + 32 * tile] << (8 * e);
  }
  return (long)(((unsigned long)hi << 32) | lo);
}

// clamp(rintf(t), -127, 127): round half to even, -128 never produced (fdet_q8.hip's q8_round)
__device__ __forceinline__ int round_q(float t) {
  return (int)fminf(fmaxf(rintf(t), -127.0f), 127.0f);
}

__device__ __forceinline__ int pack4(int a, int b, int c, int d) {
  return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | (int)((unsigned)(d & 255) << 24);
}

// Launches `kern` over image chunks: grid (chunk images x segments x row groups, channel blocks).  The entry has validated the
// arguments.
template <typename Kern>
inline int launch(Kern kern, int channel_blocks, const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul,
                  int8_t* q, int N, int F, int H, int W, hipStream_t stream, const char* what) {
  const int Ho = H / 2, Wo = W / 2;
  const int segs = (Wo + SEG - 1) / SEG, row_groups = (Ho + ROWS - 1) / ROWS;
  const long long per_img = (long long)segs * row_groups;
  const int chunk = (int)std::max(1ll, MAX_ITEMS / per_img);
  for (int n0 = 0; n0 < N; n0 += chunk) {
    Args a{};
    a.frames = frames + (size_t)n0 * 3 * H * W;
    a.w = reinterpret_cast<const signed char*>(w_q);
    a.bias = b_q;
    a.mul = mul;
    a.q = reinterpret_cast<signed char*>(q) + (size_t)n0 * (Ho + 2) * (Wo + 2) * F;
    a.N = std::min(chunk, N - n0); a.F = F; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.segs = segs; a.row_groups = row_groups;
    a.dwords = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(a.frames) & 3) == 0;
    const dim3 grid((unsigned)(a.N * per_img), (unsigned)channel_blocks);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, a);
    if (int rc = check_launch(what)) return rc;
  }
  return FDET_OK;
}

}  // namespace s3
}  // namespace fdet
