// Int8 inference: the Resnet stem (3x3, stride 2, pad 1, 3 -> F channels) from the uint8 frames straight into the int8
// trunk's layout, in integer arithmetic on the integer matrix cores (v_mfma_i32_16x16x32_i8).  The arithmetic is the contract
// of include/fdet.h ("Int8 inference", fdet_stem3_fwd_q8_u8); tests/q8_resnet_cpu_ref.py restates it in numpy and the GPU
// tests demand equality.
//
// K = 27 taps (k = (ci*3+ky)*3+kx, padded to 32 with zero weights), so the kernel is a gather in front of one MFMA step:
//   A (weights): lane l holds the 8 taps k = 8 (l >> 4) .. + 7 of one output channel (row l & 15 of its 16-channel tile)
//   B (pixels):  lane l holds the same 8 taps of output pixel (l & 15) of one output row, gathered from LDS
//   D:           lane l holds rows 4 (l >> 4) + r (r = 0..3) of pixel (l & 15)
// Row m of tile t is channel 16 (m >> 2) + 4 t + (m & 3) of the block's 64: a lane's 4 tiles x 4 rows are then the 16
// consecutive channels 16 (l >> 4) .. + 15 of its pixel, one 16-byte store into the channel-innermost output.
//
// The MFMA multiplies signed by signed and the frame codes are 0..255, so the input rows are staged in LDS as x - 128 (the
// byte x ^ 0x80), and everything outside the image as -128 (the code 0 that the contract's zero padding stands for).  All 27
// taps are then always present and
//     sum x * w = sum (x - 128) * w + 128 * sum_k w[co][k]
// where the last term is a per-channel constant that joins the bias.  Every step is an exact int32 sum, so the bytes are the
// contract's.  Both operands take tap k from the same byte of the same lane group, so the sum does not depend on how the
// instruction orders k inside a fragment; the one-hot tests (tests/test_gpu_q8_resnet.py) check taps, lanes and channels.
#include "fdet_common.h"

namespace {
using namespace fdet;

typedef int s3_v4i __attribute__((ext_vector_type(4)));
typedef float s3_v4f __attribute__((ext_vector_type(4)));

constexpr int S3_ROWS = 4;                          // output rows per workgroup: one per wave
constexpr int S3_SEG = 256;                         // output columns per workgroup: 16 MFMA column tiles
constexpr int S3_IN_ROWS = 2 * S3_ROWS + 1;         // input rows under S3_ROWS output rows
constexpr int S3_RS = 2 * S3_SEG + 16;              // bytes of one staged input row: image columns 2 ox0 - 4 .. 2 ox0 + 2 SEG + 11
constexpr int S3_LDS = 3 * S3_IN_ROWS * S3_RS;      // 14,256 bytes
constexpr int S3_MAX_HW = 4096;
constexpr int S3_MAX_F = 256;
constexpr long long S3_MAX_ITEMS = 1ll << 20;       // workgroups per launch (larger batches: consecutive launches)

struct Stem3Args {
  const unsigned char* frames;
  const signed char* w;                              // [F][32]
  const int* bias;
  const float* mul;
  signed char* q;
  int N, F, H, W, Ho, Wo;
  int segs, row_groups;
  int dwords;                                        // 1: W % 4 == 0 and a 4-byte aligned frame pointer, rows are read as dwords
};

__host__ __device__ inline bool s3_shape_ok(int Cin, int F, int H, int W) {
  return Cin == 3 && F >= 64 && F <= S3_MAX_F && (F & 63) == 0 && H >= 2 && W >= 2 && H <= S3_MAX_HW && W <= S3_MAX_HW &&
         !(H & 1) && !(W & 1);
}

// bytes of the output tensor, 0 when N images of this shape are not accepted (as fdet_q8_act_bytes: under 2^31 bytes)
inline size_t s3_out_bytes(int N, int Cin, int F, int H, int W) {
  if (N < 1 || !s3_shape_ok(Cin, F, H, W)) return 0;
  const unsigned long long b = (unsigned long long)N * (H / 2 + 2) * (W / 2 + 2) * F;
  return b < (1ull << 31) ? (size_t)b : 0;
}

// clamp(rintf(t), -127, 127): round half to even, -128 never produced (fdet_q8.hip's q8_round)
__device__ __forceinline__ int s3_round(float t) {
  return (int)fminf(fmaxf(rintf(t), -127.0f), 127.0f);
}

__device__ __forceinline__ int s3_pack4(int a, int b, int c, int d) {
  return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | (int)((unsigned)(d & 255) << 24);
}

// Workgroup = 4 waves on (image, group of 4 output rows, segment of 256 output columns) and the 64 output channels
// blockIdx.y * 64 .. + 63.  It stages the 9 input rows x 3 channels under its rows once; wave j then walks the column tiles of
// output row j.  LDS row (ci, iy) holds input row 2 oy0 - 1 + iy of channel ci; its byte i is image column 2 ox0 - 4 + i.
__global__ __launch_bounds__(256) void k_stem3_q8(const Stem3Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[S3_LDS];
  const int item = blockIdx.x;
  const int per_img = a.segs * a.row_groups;
  const int n = item / per_img;
  const int rem = item - n * per_img;
  const int rg = rem / a.segs;
  const int ox0 = (rem - rg * a.segs) * S3_SEG;
  const int oy0 = rg * S3_ROWS;
  const int ntiles = (min(S3_SEG, a.Wo - ox0) + 15) >> 4;
  const int nd = ((32 * ntiles + 3) >> 2) + 1;              // dwords of a staged row that the tiles read (bytes 3 .. 32 ntiles + 3)
  const int c0 = 2 * ox0 - 4;                               // image column of byte 0 (a multiple of 4)
  const int y0 = 2 * oy0 - 1;
  for (int u = threadIdx.x; u < 3 * S3_IN_ROWS * nd; u += 256) {
    const int lr = u / nd, d = u - lr * nd;
    const int ci = lr / S3_IN_ROWS, iy = lr - ci * S3_IN_ROWS;
    const int y = y0 + iy, c = c0 + 4 * d;
    unsigned v = 0;                                         // outside the image: code 0
    if (y >= 0 && y < a.H && c + 3 >= 0 && c < a.W) {
      const unsigned char* src = a.frames + ((size_t)(n * 3 + ci) * a.H + y) * a.W;
      if (a.dwords) {                                       // c and W are multiples of 4: the dword is inside the row as a whole
        v = *reinterpret_cast<const unsigned*>(src + c);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (c + b >= 0 && c + b < a.W) v |= (unsigned)src[c + b] << (8 * b);
      }
    }
    *reinterpret_cast<unsigned*>(rows + lr * S3_RS + 4 * d) = v ^ 0x80808080u;          // x - 128 as a signed byte
  }
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int co0 = blockIdx.y * 64;
  // A: tile t, row lp -> channel co0 + 16 (lp >> 2) + 4 t + (lp & 3), its taps 8 lk .. + 7 (bytes 27..31 of a row are zero)
  long wa[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    wa[t] = *reinterpret_cast<const long*>(a.w + (size_t)(co0 + 16 * (lp >> 2) + 4 * t + (lp & 3)) * 32 + 8 * lk);
  // the lane's 16 output channels co0 + 16 lk .. + 15 (dword t, byte r = channel 4 t + r): multiplier and the constant
  // bias + 128 * sum of the channel's weights -- the MFMA against a B of ones is that sum, in the accumulators' own layout
  // (wrapping adds: the exact sum fits where the contract's acc does)
  float m[4][4];
  unsigned cst[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int co = co0 + 16 * lk + 4 * t;
    const s3_v4f mv = *reinterpret_cast<const s3_v4f*>(a.mul + co);
    const s3_v4i bv = *reinterpret_cast<const s3_v4i*>(a.bias + co);
    const s3_v4i z = {0, 0, 0, 0};
    const s3_v4i ws = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa[t], 0x0101010101010101l, z, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[t][r] = mv[r];
      cst[t][r] = (unsigned)bv[r] + 128u * (unsigned)ws[r];
    }
  }
  // B: tap k = 8 lk + e -> LDS row (ci, 2 j + ky), byte 2 (ox - ox0) + kx + 3; taps 27..31 read tap 26 again (weight zero)
  int off[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = min(8 * lk + e, 26);
    const int ci = k / 9, ky = (k - 9 * ci) / 3, kx = k - 9 * ci - 3 * ky;
    off[e] = (ci * S3_IN_ROWS + 2 * j + ky) * S3_RS + kx + 3 + 2 * lp;
  }
  __syncthreads();
  const int oy = oy0 + j;
  if (oy >= a.Ho) return;                                   // (after the only barrier)
  signed char* qrow = a.q + ((size_t)(n * (a.Ho + 2) + oy + 1) * (a.Wo + 2) + ox0 + 1) * a.F + co0 + 16 * lk;
  for (int tile = 0; tile < ntiles; ++tile) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo |= (unsigned)rows[off[e] + 32 * tile] << (8 * e);
      hi |= (unsigned)rows[off[e + 4] + 32 * tile] << (8 * e);
    }
    const long b = (long)(((unsigned long)hi << 32) | lo);
    int o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const s3_v4i z = {0, 0, 0, 0};
      const s3_v4i acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa[t], b, z, 0, 0, 0);
      int qv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) qv[r] = s3_round((float)(int)((unsigned)acc[r] + cst[t][r]) * m[t][r]);
      o[t] = s3_pack4(qv[0], qv[1], qv[2], qv[3]);
    }
    const int px = 16 * tile + lp;
    if (ox0 + px < a.Wo) {
      const s3_v4i ov = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<s3_v4i*>(qrow + (size_t)px * a.F) = ov;
    }
  }
}

inline bool s3_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int fdet_stem3_fwd_q8_ok(int N, int Cin, int F, int H, int W) { return s3_out_bytes(N, Cin, F, H, W) > 0 ? 1 : 0; }

extern "C" int fdet_stem3_fwd_q8_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                                    int N, int Cin, int F, int H, int W, void* stream) {
  FDET_REQUIRE(frames && w_q && b_q && mul && q, "stem3_fwd_q8: null argument");
  FDET_REQUIRE(s3_out_bytes(N, Cin, F, H, W) > 0,
               "stem3_fwd_q8: unsupported shape N=%d Cin=%d F=%d %dx%d (3 channels, F %% 64 == 0, F <= %d, even H and W in 2..%d, "
               "output under 2^31 bytes)", N, Cin, F, H, W, S3_MAX_F, S3_MAX_HW);
  FDET_REQUIRE(s3_aligned16(w_q) && s3_aligned16(b_q) && s3_aligned16(mul) && s3_aligned16(q),
               "stem3_fwd_q8: w_q, b_q, mul and q must be 16-byte aligned");
  const int Ho = H / 2, Wo = W / 2;
  const int segs = (Wo + S3_SEG - 1) / S3_SEG, row_groups = (Ho + S3_ROWS - 1) / S3_ROWS;
  const long long per_img = (long long)segs * row_groups;
  const int chunk = (int)std::max(1ll, S3_MAX_ITEMS / per_img);
  for (int n0 = 0; n0 < N; n0 += chunk) {
    Stem3Args a{};
    a.frames = frames + (size_t)n0 * 3 * H * W;
    a.w = reinterpret_cast<const signed char*>(w_q);
    a.bias = b_q;
    a.mul = mul;
    a.q = reinterpret_cast<signed char*>(q) + (size_t)n0 * (Ho + 2) * (Wo + 2) * F;
    a.N = std::min(chunk, N - n0); a.F = F; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.segs = segs; a.row_groups = row_groups;
    a.dwords = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(a.frames) & 3) == 0;
    const dim3 grid((unsigned)(a.N * per_img), (unsigned)(F / 64));
    hipLaunchKernelGGL(k_stem3_q8, grid, dim3(256), 0, (hipStream_t)stream, a);
    if (int rc = check_launch("fdet_stem3_fwd_q8_u8")) return rc;
  }
  return FDET_OK;
}
