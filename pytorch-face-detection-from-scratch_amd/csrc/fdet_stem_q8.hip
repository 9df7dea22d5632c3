// Int8 inference: the Resnet stem (3x3, stride 2, pad 1, 3 -> F channels) from the uint8 frames straight into the int8
// trunk's layout, in integer arithmetic on the integer matrix cores (v_mfma_i32_16x16x32_i8).  The arithmetic is the contract
// of include/fdet.h ("Int8 inference", fdet_stem3_fwd_q8_u8, and fdet_stem3_fwd_q8x_u8 for F a multiple of 16);
// tests/q8_resnet_cpu_ref.py restates it in numpy and the GPU tests demand equality.  The second half of the file is the
// PoolResnet stem (10x10, stride 8, pad 2) in the same arithmetic, fdet_stem10_fwd_q8_u8.  The offset and the requantising
// line of all three kernels are q8::stem_offset and q8::stem_requant (fdet_q8_common.h).
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
#include "fdet_q8_common.h"

namespace {
using namespace fdet;

using q8::v4i;
using q8::v4f;

// What the two 3x3 stem kernels share (k_stem3_q8: 64 output channels per workgroup; k_stem3_q8x: 16): the launch geometry,
// the staging of the input rows in LDS as x - 128, the tap offsets of a lane's B operand and its gather.
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

// F a multiple of f_mult: 64 for k_stem3_q8, 16 for k_stem3_q8x
__host__ __device__ inline bool s3_shape_ok(int Cin, int F, int H, int W, int f_mult) {
  return Cin == 3 && q8::act_shape_ok(F, H, W, f_mult) && H >= 2 && W >= 2 && !(H & 1) && !(W & 1);
}

// bytes of the output tensor, 0 when N images of this shape are not accepted (as fdet_q8_act_bytes: under 2^31 bytes)
inline size_t s3_out_bytes(int N, int Cin, int F, int H, int W, int f_mult) {
  return s3_shape_ok(Cin, F, H, W, f_mult) ? q8::act_bytes(N, F, H / 2, W / 2, f_mult) : 0;
}

// Workgroup = 4 waves on (image, group of 4 output rows, segment of 256 output columns) and the 64 output channels
// blockIdx.y * 64 .. + 63.  It stages the 9 input rows x 3 channels under its rows once; wave j then walks the column tiles of
// output row j.  LDS row (ci, iy) holds input row 2 oy0 - 1 + iy of channel ci; its byte i is image column 2 ox0 - 4 + i.
__global__ __launch_bounds__(256) void k_stem3_q8(const s3::Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[s3::LDS];
  const s3::Item it = s3::item_of(a, blockIdx.x);
  const int n = it.n, ox0 = it.ox0, oy0 = it.oy0, ntiles = it.ntiles;
  s3::stage_rows(a, it, rows);
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int co0 = blockIdx.y * 64;
  // A: tile t, row lp -> channel co0 + 16 (lp >> 2) + 4 t + (lp & 3), its taps 8 lk .. + 7 (bytes 27..31 of a row are zero)
  long wa[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    wa[t] = *reinterpret_cast<const long*>(a.w + (size_t)(co0 + 16 * (lp >> 2) + 4 * t + (lp & 3)) * 32 + 8 * lk);
  // the lane's 16 output channels co0 + 16 lk .. + 15 (dword t, byte r = channel 4 t + r): q8::stem_offset, the weight sums
  // from the MFMA against a B of ones
  float m[4][4];
  unsigned cst[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int co = co0 + 16 * lk + 4 * t;
    const v4i z = {0, 0, 0, 0};
    q8::stem_offset(cst[t], m[t], a.bias + co, a.mul + co, __builtin_amdgcn_mfma_i32_16x16x32_i8(wa[t], 0x0101010101010101l, z, 0, 0, 0));
  }
  int off[8];
  s3::tap_offsets(off, lk, lp, j);
  __syncthreads();
  const int oy = oy0 + j;
  if (oy >= a.Ho) return;                                   // (after the only barrier)
  signed char* qrow = a.q + ((size_t)(n * (a.Ho + 2) + oy + 1) * (a.Wo + 2) + ox0 + 1) * a.F + co0 + 16 * lk;
  for (int tile = 0; tile < ntiles; ++tile) {
    const long b = s3::gather(rows, off, tile);
    int o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const v4i z = {0, 0, 0, 0};
      o[t] = q8::stem_requant(__builtin_amdgcn_mfma_i32_16x16x32_i8(wa[t], b, z, 0, 0, 0), cst[t], m[t]);
    }
    const int px = 16 * tile + lp;
    if (ox0 + px < a.Wo) {
      const v4i ov = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<v4i*>(qrow + (size_t)px * a.F) = ov;
    }
  }
}

// The same stem for F a multiple of 16 (the SSD detector's 16 filters): k_stem3_q8's arithmetic with ONE 16-channel tile per
// workgroup: row m of the tile is channel co0 + m, so a lane ends up with the four channels co0 + 4 (l >> 4) + r of its
// pixel, one dword store.  F % 64 == 0 goes to k_stem3_q8.
__global__ __launch_bounds__(256) void k_stem3_q8x(const s3::Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[s3::LDS];
  const s3::Item it = s3::item_of(a, blockIdx.x);
  const int n = it.n, ox0 = it.ox0, oy0 = it.oy0, ntiles = it.ntiles;
  s3::stage_rows(a, it, rows);
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int co0 = blockIdx.y * 16;
  // A: row lp -> channel co0 + lp, its taps 8 lk .. + 7 (bytes 27..31 of a row are zero)
  const long wa = *reinterpret_cast<const long*>(a.w + (size_t)(co0 + lp) * 32 + 8 * lk);
  // the lane's four output channels co0 + 4 lk + r: q8::stem_offset, the weight sums from the MFMA against a B of ones
  float m[4];
  unsigned cst[4];
  const v4i z = {0, 0, 0, 0};
  q8::stem_offset(cst, m, a.bias + co0 + 4 * lk, a.mul + co0 + 4 * lk,
                  __builtin_amdgcn_mfma_i32_16x16x32_i8(wa, 0x0101010101010101l, z, 0, 0, 0));
  int off[8];
  s3::tap_offsets(off, lk, lp, j);
  __syncthreads();
  const int oy = oy0 + j;
  if (oy >= a.Ho) return;                                   // (after the only barrier)
  signed char* qrow = a.q + ((size_t)(n * (a.Ho + 2) + oy + 1) * (a.Wo + 2) + ox0 + 1) * a.F + co0 + 4 * lk;
  for (int tile = 0; tile < ntiles; ++tile) {
    const long b = s3::gather(rows, off, tile);
    const int o = q8::stem_requant(__builtin_amdgcn_mfma_i32_16x16x32_i8(wa, b, z, 0, 0, 0), cst, m);
    const int px = 16 * tile + lp;
    if (ox0 + px < a.Wo) *reinterpret_cast<int*>(qrow + (size_t)px * a.F) = o;
  }
}

}  // namespace

extern "C" int fdet_stem3_fwd_q8_ok(int N, int Cin, int F, int H, int W) { return s3_out_bytes(N, Cin, F, H, W, 64) > 0 ? 1 : 0; }

extern "C" int fdet_stem3_fwd_q8_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                                    int N, int Cin, int F, int H, int W, void* stream) {
  FDET_REQUIRE(frames && w_q && b_q && mul && q, "stem3_fwd_q8: null argument");
  FDET_REQUIRE(s3_out_bytes(N, Cin, F, H, W, 64) > 0,
               "stem3_fwd_q8: unsupported shape N=%d Cin=%d F=%d %dx%d (3 channels, F %% 64 == 0, F <= %d, even H and W in 2..%d, "
               "output under 2^31 bytes)", N, Cin, F, H, W, q8::MAX_C, q8::MAX_HW);
  FDET_REQUIRE(q8::aligned16(w_q) && q8::aligned16(b_q) && q8::aligned16(mul) && q8::aligned16(q),
               "stem3_fwd_q8: w_q, b_q, mul and q must be 16-byte aligned");
  return s3::launch(k_stem3_q8, F / 64, frames, w_q, b_q, mul, q, N, F, H, W, (hipStream_t)stream, "fdet_stem3_fwd_q8_u8");
}

extern "C" int fdet_stem3_fwd_q8x_ok(int N, int Cin, int F, int H, int W) { return s3_out_bytes(N, Cin, F, H, W, 16) > 0 ? 1 : 0; }

extern "C" int fdet_stem3_fwd_q8x_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                                     int N, int Cin, int F, int H, int W, void* stream) {
  FDET_REQUIRE(frames && w_q && b_q && mul && q, "stem3_fwd_q8x: null argument");
  FDET_REQUIRE(s3_out_bytes(N, Cin, F, H, W, 16) > 0,
               "stem3_fwd_q8x: unsupported shape N=%d Cin=%d F=%d %dx%d (3 channels, F %% 16 == 0, F <= %d, even H and W in 2..%d, "
               "output under 2^31 bytes)", N, Cin, F, H, W, q8::MAX_C, q8::MAX_HW);
  FDET_REQUIRE(q8::aligned16(w_q) && q8::aligned16(b_q) && q8::aligned16(mul) && q8::aligned16(q),
               "stem3_fwd_q8x: w_q, b_q, mul and q must be 16-byte aligned");
  if ((F & 63) == 0) return fdet_stem3_fwd_q8_u8(frames, w_q, b_q, mul, q, N, Cin, F, H, W, stream);   // the same contract
  return s3::launch(k_stem3_q8x, F / 16, frames, w_q, b_q, mul, q, N, F, H, W, (hipStream_t)stream, "fdet_stem3_fwd_q8x_u8");
}

namespace {
// ------------------------------------------------------------------------------------------------------------------------
// The PoolResnet stem (10x10, stride 8, pad 2, 3 -> F channels) in the same integer arithmetic (fdet_stem10_fwd_q8_u8;
// tests/q8_pool_stem_cpu_ref.py restates it), on v_mfma_i32_16x16x64_i8.
//
// K is ordered as rows kr = ci * 10 + ky (30 of them, padded to 32) of 16 kx slots each, slots 10..15 and rows 30, 31 with
// zero weights: K = 512 = 8 MFMA steps for 300 real taps.  In step s the lane group g = lane >> 4 takes row
// kr = 4 s + {0, 2, 1, 3}[g], for both operands:
//   A (weights): lane l holds the 16 bytes wpk[co][kr][0..15] of one output channel (row l & 15 of its tile, permuted as in
//                k_stem3_q8 so that a lane ends up with 16 consecutive channels of its pixel: one 16-byte store)
//   B (pixels):  lane l holds 16 CONTIGUOUS staged bytes of input row (ci, 8 oy + ky - 2), from column 8 ox - 2, of output
//                pixel ox = l & 15 of the tile: no per-tap gather; whatever lies in slots 10..15 meets a zero weight
// LDS byte i of a staged row is image column 8 ox0 - 2 + i, so every window starts at a multiple of 8 bytes and is read as two
// aligned 8-byte loads.  The row pitch is 576 = 64 (mod 128) bytes: lane groups 0 / 1 (and 2 / 3), which share a 32-lane half
// of an 8-byte LDS read, take rows two apart (26 apart across a channel boundary, an odd multiple of two as well), that is
// 128 bytes apart modulo the 256-byte bank row, and each group's 16 windows cover 128 contiguous bytes: no conflicts.
// Rows are staged as x - 128 with -128 outside the image, and 128 * sum_k w[co][k] joins the bias, exactly as above.
constexpr int S10_ROWS = 4;                           // output rows per workgroup: one per wave
constexpr int S10_SEG = 64;                           // output columns per workgroup: 4 MFMA column tiles
constexpr int S10_IN_ROWS = 8 * S10_ROWS + 2;         // input rows under S10_ROWS output rows
constexpr int S10_RS = 576;                           // LDS row pitch: >= 8 * S10_SEG + 8 and = 64 (mod 128)
constexpr int S10_LDS = 3 * S10_IN_ROWS * S10_RS;     // 58,752 bytes
constexpr long long S10_MAX_ITEMS = 1ll << 20;
static_assert(S10_RS >= 8 * S10_SEG + 8 && S10_RS % 128 == 64 && ((S10_IN_ROWS - 8) / 2) % 2 == 1, "stem10 LDS pitch");

struct Stem10Args {
  const unsigned char* frames;
  const signed char* w;                                // [F][32][16]
  const int* bias;
  const float* mul;
  signed char* q;
  int N, F, H, W, Ho, Wo;
  int segs, row_groups;
  int align;                                           // how a row is read: 16 (W % 16 == 0 and a 16-byte aligned frame pointer: one
                                                       // 16-byte and one 4-byte load per 16 staged bytes), 4 (W % 4 == 0, 4-byte
                                                       // aligned: dwords), 1 (bytes)
};

__host__ __device__ inline bool s10_shape_ok(int Cin, int F, int H, int W) {
  return Cin == 3 && q8::act_shape_ok(F, H, W, 64) && H >= 6 && W >= 6;
}

inline size_t s10_out_bytes(int N, int Cin, int F, int H, int W) {
  return s10_shape_ok(Cin, F, H, W) ? q8::act_bytes(N, F, (H - 6) / 8 + 1, (W - 6) / 8 + 1, 64) : 0;
}

// Workgroup = 4 waves on (image, group of 4 output rows, segment of 64 output columns) and the 64 output channels
// blockIdx.y * 64 .. + 63.  It stages the 34 input rows x 3 channels under its rows once; wave j then walks the column tiles of
// output row j with the 64 channels' weights (8 steps x 4 tiles) in registers.  LDS row (ci, iy) holds input row
// 8 oy0 - 2 + iy of channel ci.
__global__ __launch_bounds__(256) void k_stem10_q8(const Stem10Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char rows[S10_LDS];
  const int item = blockIdx.x;
  const int per_img = a.segs * a.row_groups;
  const int n = item / per_img;
  const int rem = item - n * per_img;
  const int rg = rem / a.segs;
  const int ox0 = (rem - rg * a.segs) * S10_SEG;
  const int oy0 = rg * S10_ROWS;
  const int ntiles = (min(S10_SEG, a.Wo - ox0) + 15) >> 4;
  const int nd = 32 * ntiles + 2;                           // dwords of a staged row that the tiles read (bytes 0 .. 128 ntiles + 7)
  const int nr = 8 * min(S10_ROWS, a.Ho - oy0) + 2;         // input rows that the block's output rows read
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int co0 = blockIdx.y * 64;
  const int kperm = ((lk & 1) << 1) | (lk >> 1);            // {0, 2, 1, 3}[lk]
  // A: step s, tile t, row lp -> channel co0 + 16 (lp >> 2) + 4 t + (lp & 3), its K row 4 s + kperm (issued first: these 32
  // loads are in flight while the rows are staged)
  v4i wa[8][4];
#pragma unroll
  for (int s = 0; s < 8; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t)
      wa[s][t] = *reinterpret_cast<const v4i*>(a.w + (size_t)(co0 + 16 * (lp >> 2) + 4 * t + (lp & 3)) * 512 + (4 * s + kperm) * 16);
  const int c0 = 8 * ox0 - 4;                               // dword path: staged dword d is image columns c0 + 4 d + 2 .. + 5
  const int y0 = 8 * oy0 - 2;
  if (a.align == 16) {
    // 16 staged bytes (image columns c - 2 .. c + 13, c = 8 ox0 + 16 k) from the aligned 16 bytes at c and the dword before
    // them.  Four items per thread and pass: the eight loads are unconditional, from addresses clamped into the image, and are
    // all in flight before the first one is used; what lies outside the image is replaced by the code 0 afterwards.
    const int nc = 8 * ntiles + 1;                          // 16-byte chunks of a staged row (bytes 0 .. 128 ntiles + 15 <= S10_RS)
    const int total = 3 * nr * nc;
    for (int u0 = threadIdx.x; u0 < total; u0 += 1024) {
      v4i dv[4];
      unsigned pv[4];
      int dst[4];
      bool okd[4], okp[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = min(u0 + 256 * i, total - 1);
        const int lr = u / nc, k = u - lr * nc;
        const int ci = lr / nr, iy = lr - ci * nr;
        const int y = y0 + iy, c = 8 * ox0 + 16 * k;
        const bool row = y >= 0 && y < a.H;
        const unsigned char* src = a.frames + ((size_t)(n * 3 + ci) * a.H + min(max(y, 0), a.H - 1)) * a.W;
        okd[i] = row && c < a.W;
        okp[i] = row && c >= 4 && c - 4 < a.W;
        dv[i] = *reinterpret_cast<const v4i*>(src + min(c, a.W - 16));
        pv[i] = *reinterpret_cast<const unsigned*>(src + min(max(c - 4, 0), a.W - 4));
        dst[i] = (ci * S10_IN_ROWS + iy) * S10_RS + 16 * k;
      }
      __builtin_amdgcn_sched_barrier(0);                      // (the loads stay ahead of the stores)
#pragma unroll
      for (int i = 0; i < 4; ++i) {                           // (an item past the end is the last item again: the same bytes)
        const unsigned p = okp[i] ? pv[i] : 0u;
        const unsigned d0 = okd[i] ? (unsigned)dv[i][0] : 0u, d1 = okd[i] ? (unsigned)dv[i][1] : 0u;
        const unsigned d2 = okd[i] ? (unsigned)dv[i][2] : 0u, d3 = okd[i] ? (unsigned)dv[i][3] : 0u;
        const v4i o = {(int)(((p >> 16) | (d0 << 16)) ^ 0x80808080u), (int)(((d0 >> 16) | (d1 << 16)) ^ 0x80808080u),
                          (int)(((d1 >> 16) | (d2 << 16)) ^ 0x80808080u), (int)(((d2 >> 16) | (d3 << 16)) ^ 0x80808080u)};
        *reinterpret_cast<v4i*>(rows + dst[i]) = o;
      }
    }
  } else {
    for (int u = threadIdx.x; u < 3 * nr * nd; u += 256) {
      const int lr = u / nd, d = u - lr * nd;
      const int ci = lr / nr, iy = lr - ci * nr;
      const int y = y0 + iy;
      unsigned v = 0;                                       // outside the image: code 0
      if (y >= 0 && y < a.H) {
        const unsigned char* src = a.frames + ((size_t)(n * 3 + ci) * a.H + y) * a.W;
        const int c = c0 + 4 * d;                           // (a multiple of 4)
        if (a.align == 4) {                                 // W is a multiple of 4: an aligned dword is inside the row as a whole
          const unsigned lo = c >= 0 && c < a.W ? *reinterpret_cast<const unsigned*>(src + c) : 0u;
          const unsigned hi = c + 4 < a.W ? *reinterpret_cast<const unsigned*>(src + c + 4) : 0u;
          v = (lo >> 16) | (hi << 16);
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (c + 2 + b >= 0 && c + 2 + b < a.W) v |= (unsigned)src[c + 2 + b] << (8 * b);
        }
      }
      *reinterpret_cast<unsigned*>(rows + (ci * S10_IN_ROWS + iy) * S10_RS + 4 * d) = v ^ 0x80808080u;   // x - 128 as a signed byte
    }
  }
  // the lane's 16 output channels co0 + 16 lk .. + 15: q8::stem_offset, the weight sums from the MFMAs against a B of ones
  float m[4][4];
  unsigned cst[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int co = co0 + 16 * lk + 4 * t;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    v4i ws = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 8; ++s) ws = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[s][t], ones, ws, 0, 0, 0);
    q8::stem_offset(cst[t], m[t], a.bias + co, a.mul + co, ws);
  }
  // B: step s -> LDS row (ci, 8 j + ky) of K row min(4 s + kperm, 29) (rows 30 and 31 have zero weights), bytes 8 lp .. + 15
  int off[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int kr = min(4 * s + kperm, 29);
    const int ci = kr / 10, ky = kr - 10 * ci;
    off[s] = (ci * S10_IN_ROWS + 8 * j + ky) * S10_RS + 8 * lp;
  }
  __syncthreads();
  const int oy = oy0 + j;
  if (oy >= a.Ho) return;                                   // (after the only barrier)
  signed char* qrow = a.q + ((size_t)(n * (a.Ho + 2) + oy + 1) * (a.Wo + 2) + ox0 + 1) * a.F + co0 + 16 * lk;
  for (int tile = 0; tile < ntiles; ++tile) {
    v4i acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4i{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const long b0 = *reinterpret_cast<const long*>(rows + off[s] + 128 * tile);
      const long b1 = *reinterpret_cast<const long*>(rows + off[s] + 128 * tile + 8);
      const v4i b = {(int)b0, (int)(b0 >> 32), (int)b1, (int)(b1 >> 32)};
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[s][t], b, acc[t], 0, 0, 0);
    }
    int o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = q8::stem_requant(acc[t], cst[t], m[t]);
    const int px = 16 * tile + lp;
    if (ox0 + px < a.Wo) {
      const v4i ov = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<v4i*>(qrow + (size_t)px * a.F) = ov;
    }
  }
}

}  // namespace

extern "C" int fdet_stem10_fwd_q8_ok(int N, int Cin, int F, int H, int W) { return s10_out_bytes(N, Cin, F, H, W) > 0 ? 1 : 0; }

extern "C" int fdet_stem10_fwd_q8_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                                     int N, int Cin, int F, int H, int W, void* stream) {
  FDET_REQUIRE(frames && w_q && b_q && mul && q, "stem10_fwd_q8: null argument");
  FDET_REQUIRE(s10_out_bytes(N, Cin, F, H, W) > 0,
               "stem10_fwd_q8: unsupported shape N=%d Cin=%d F=%d %dx%d (3 channels, F %% 64 == 0, F <= %d, H and W in 6..%d, "
               "output under 2^31 bytes)", N, Cin, F, H, W, q8::MAX_C, q8::MAX_HW);
  FDET_REQUIRE(q8::aligned16(w_q) && q8::aligned16(b_q) && q8::aligned16(mul) && q8::aligned16(q),
               "stem10_fwd_q8: w_q, b_q, mul and q must be 16-byte aligned");
  const int Ho = (H - 6) / 8 + 1, Wo = (W - 6) / 8 + 1;
  const int segs = (Wo + S10_SEG - 1) / S10_SEG, row_groups = (Ho + S10_ROWS - 1) / S10_ROWS;
  const long long per_img = (long long)segs * row_groups;
  const int chunk = (int)std::max(1ll, S10_MAX_ITEMS / per_img);
  for (int n0 = 0; n0 < N; n0 += chunk) {
    Stem10Args a{};
    a.frames = frames + (size_t)n0 * 3 * H * W;
    a.w = reinterpret_cast<const signed char*>(w_q);
    a.bias = b_q;
    a.mul = mul;
    a.q = reinterpret_cast<signed char*>(q) + (size_t)n0 * (Ho + 2) * (Wo + 2) * F;
    a.N = std::min(chunk, N - n0); a.F = F; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
    a.segs = segs; a.row_groups = row_groups;
    const uintptr_t fa = reinterpret_cast<uintptr_t>(a.frames);
    a.align = (W & 15) == 0 && (fa & 15) == 0 ? 16 : (W & 3) == 0 && (fa & 3) == 0 ? 4 : 1;
    const dim3 grid((unsigned)(a.N * per_img), (unsigned)(F / 64));
    hipLaunchKernelGGL(k_stem10_q8, grid, dim3(256), 0, (hipStream_t)stream, a);
    if (int rc = check_launch("fdet_stem10_fwd_q8_u8")) return rc;
  }
  return FDET_OK;
}
