// Int8 post-training-quantised inference of the PoolResnet residual trunk (gfx950): 3x3 convolutions on the integer matrix
// cores (v_mfma_i32_16x16x64_i8) with the requantising epilogue in registers, and the converters between fp32 NCHW and the
// int8 activation layout.  The arithmetic is the contract of include/fdet.h ("Int8 inference"); tests/q8_cpu_ref.py restates
// it in numpy and the GPU tests demand equality.
//
// Activation layout (Q8): int8 [N][H+2][W+2][C], channel innermost, a one-pixel halo of zeros round every image.  Symmetric
// quantisation never produces -128, so the halo byte 0 is the real zero and the conv needs no bounds test.  Producers write
// real pixels only: a buffer that keeps its shape keeps its halo.
//
// Conv as a GEMM per tap and 64-channel chunk: D[co][pixel] += W[co][ci] * X[ci][pixel], K = 64 = one MFMA step.
//   A (weights): lane l holds 16 consecutive ci bytes of row co = 16t + (l & 15), starting at ci = 16 (l >> 4)
//   B (pixels):  lane l holds the same 16 ci of pixel column (l & 15)
//   D:           lane l holds co = 16t + 4 (l >> 4) + r (r = 0..3) of pixel (l & 15): four channels = one dword store
// Both operands take their k from the same 16-byte channel run, so the sum does not depend on how the instruction orders k
// inside a lane's fragment; the one-hot tests (tests/test_gpu_q8.py) check rows, columns and taps.
#include "fdet_common.h"

namespace {
using namespace fdet;

typedef int q8_v4i __attribute__((ext_vector_type(4)));
typedef float q8_v4f __attribute__((ext_vector_type(4)));

constexpr int Q8_ROWS = 4;            // map rows per work item (one wave): 4 rows x 16 columns x 64 output channels
constexpr int Q8_MAX_C = 256;
constexpr int Q8_MAX_HW = 4096;
constexpr size_t Q8_LDS_MAX = 160 * 1024;

struct Q8Geo {
  int N, C, H, W, HP, WP;
};

__host__ __device__ inline bool q8_shape_ok(int C, int H, int W) {
  return C >= 64 && C <= Q8_MAX_C && (C & 63) == 0 && H >= 1 && W >= 1 && H <= Q8_MAX_HW && W <= Q8_MAX_HW;
}

// bytes of N images, 0 when the shape has no layout or the tensor passes 2^31 - 1 bytes (32-bit offsets inside the kernels)
inline size_t q8_bytes(int N, int C, int H, int W) {
  if (N < 1 || !q8_shape_ok(C, H, W)) return 0;
  const unsigned long long b = (unsigned long long)N * (H + 2) * (W + 2) * C;
  return b < (1ull << 31) ? (size_t)b : 0;
}

// clamp(rintf(t), -127, 127): round half to even, -128 never produced
__device__ __forceinline__ int q8_round(float t) {
  return (int)fminf(fmaxf(rintf(t), -127.0f), 127.0f);
}

__device__ __forceinline__ int q8_pack4(int a, int b, int c, int d) {
  return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | (int)((unsigned)(d & 255) << 24);
}

__device__ __forceinline__ int q8_byte(int w, int r) {
  return (int)(signed char)((unsigned)w >> (8 * r));
}

// fp32 NCHW -> Q8.  One block per (image, row, 32 columns) and all channels: thread (column, channel group) reads four
// channel planes (32 lanes = 128 contiguous bytes each), packs a dword into an LDS tile [column][C/4 (+1: banks)], and the
// tile -- contiguous in the channel-innermost output -- goes out in consecutive dwords.
constexpr int Q8_QT = 32;
__global__ __launch_bounds__(256) void k_q8_quantize(const float* __restrict__ x, signed char* __restrict__ q, Q8Geo g, float inv_s,
                                                      int tiles_x) {
  __shared__ int tile[Q8_QT * (Q8_MAX_C / 4 + 1)];
  const int C4 = g.C >> 2;
  const int tx = blockIdx.x % tiles_x;
  const int r = blockIdx.x / tiles_x;
  const int yy = r % g.H, n = r / g.H;
  const int x0 = tx * Q8_QT;
  const int npx = min(Q8_QT, g.W - x0);
  const int col = threadIdx.x & (Q8_QT - 1);
  const size_t plane = (size_t)g.H * g.W;
  if (col < npx) {
    const float* src = x + (size_t)n * g.C * plane + (size_t)yy * g.W + x0 + col;
    for (int c4 = threadIdx.x / Q8_QT; c4 < C4; c4 += 256 / Q8_QT) {
      int v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float t = src[(size_t)(4 * c4 + k) * plane] * inv_s;
        v[k] = t == t ? q8_round(t) : 0;                   // a NaN product (NaN input, or 0 * inf under a denormal scale) -> 0
      }
      tile[col * (C4 + 1) + c4] = q8_pack4(v[0], v[1], v[2], v[3]);
    }
  }
  __syncthreads();
  int* dst = reinterpret_cast<int*>(q + ((size_t)(n * g.HP + yy + 1) * g.WP + x0 + 1) * g.C);
  for (int i = threadIdx.x; i < npx * C4; i += 256) dst[i] = tile[(i / C4) * (C4 + 1) + i % C4];
}

// Q8 -> fp32 NCHW.  One thread per (n, group of 4 channels, y, x), x fastest: one dword read at a stride of C bytes between
// lanes, four coalesced stores (the tensor it reads is the small 15x15 one; no LDS transpose here).
__global__ __launch_bounds__(256) void k_q8_dequantize(const signed char* __restrict__ q, float* __restrict__ x, Q8Geo g, float s,
                                                        int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xx = i % g.W;
  int r = i / g.W;
  const int yy = r % g.H;
  r /= g.H;
  const int c4 = r % (g.C >> 2);
  const int n = r / (g.C >> 2);
  const size_t plane = (size_t)g.H * g.W;
  const int w = *reinterpret_cast<const int*>(q + ((size_t)(n * g.HP + yy + 1) * g.WP + xx + 1) * g.C + 4 * c4);
  float* dst = x + ((size_t)n * g.C + 4 * c4) * plane + (size_t)yy * g.W + xx;
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[k * plane] = (float)q8_byte(w, k) * s;
}

// 3x3 conv, pad 1, on Q8 tensors.  Block = 4 waves that share the 64 output channels blockIdx.y * 64 .. + 63, whose packed
// weights ([tap][C/64][64 co][64 ci] = 36 KB per 64 input channels) the block keeps in LDS; every wave then walks work items
// of 4 rows x 16 columns of one image.  Lanes whose pixel lies outside the map read a clamped (valid) pixel and store nothing.
template <bool POOL>
__global__ __launch_bounds__(256) void k_q8_conv3x3(const signed char* __restrict__ x, const signed char* __restrict__ wpk,
                                                     const int* __restrict__ bias, const float* __restrict__ mul,
                                                     const signed char* __restrict__ skip, float skip_mul,
                                                     signed char* __restrict__ y, Q8Geo g, int tiles_x, int row_groups, int items,
                                                     float slope) {
  extern __shared__ __attribute__((aligned(16))) unsigned char q8_lds[];
  const int KC = g.C >> 6;
  const int co0 = blockIdx.y * 64;
  const int steps = 9 * KC;
  for (int s0 = 0; s0 < steps; s0 += 9) {                  // 16-byte units, 256 per (tap, chunk); nine loads in flight per thread
    q8_v4i v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
      v[k] = *reinterpret_cast<const q8_v4i*>(wpk + ((size_t)(s0 + k) * g.C + co0) * 64 + threadIdx.x * 16);
#pragma unroll
    for (int k = 0; k < 9; ++k) reinterpret_cast<q8_v4i*>(q8_lds)[(s0 + k) * 256 + threadIdx.x] = v[k];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int per_img = tiles_x * row_groups;
  const unsigned char* wl = q8_lds + lp * 64 + lk * 16;
  for (int item = blockIdx.x * 4 + wave; item < items; item += gridDim.x * 4) {
    const int n = item / per_img;
    const int rem = item - n * per_img;
    const int rg = rem / tiles_x;
    const int px = (rem - rg * tiles_x) * 16 + lp;
    const int pxc = min(px, g.W - 1);
    const int y0 = rg * Q8_ROWS;
    q8_v4i acc[Q8_ROWS][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const q8_v4i b = *reinterpret_cast<const q8_v4i*>(bias + co0 + 16 * t + 4 * lk);
#pragma unroll
      for (int j = 0; j < Q8_ROWS; ++j) acc[j][t] = b;
    }
    // the item reads padded rows y0 .. y0 + 5 (row j, tap ky -> padded row y0 + j + ky) at columns px .. px + 2: 18 fragments
    // per 64-channel chunk, all issued before the first MFMA needs one, each used by up to three (row, tap) pairs.  Padded
    // rows past H + 1 belong to rows of the item below the map only: clamped, their results are never stored.
    const signed char* xr[Q8_ROWS + 2];
#pragma unroll
    for (int r = 0; r < Q8_ROWS + 2; ++r)
      xr[r] = x + ((size_t)(n * g.HP + min(y0 + r, g.H + 1)) * g.WP + pxc) * g.C + lk * 16;
    for (int kc = 0; kc < KC; ++kc) {
      q8_v4i b[Q8_ROWS + 2][3];
#pragma unroll
      for (int r = 0; r < Q8_ROWS + 2; ++r)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) b[r][kx] = *reinterpret_cast<const q8_v4i*>(xr[r] + (size_t)kx * g.C + kc * 64);
      __builtin_amdgcn_sched_barrier(0);                   // keep the 18 loads ahead of the MFMAs (the scheduler sinks them)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * (tap / 3);
        q8_v4i a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = *reinterpret_cast<const q8_v4i*>(wl + (size_t)(tap * KC + kc) * 4096 + t * 1024);
#pragma unroll
        for (int j = 0; j < Q8_ROWS; ++j)
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[j][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b[j + ky][kx], acc[j][t], 0, 0, 0);
      }
    }
    // epilogue: multiplier, LeakyReLU, skip, requantise (, 2x2 max), four channels of one pixel per dword
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int co = co0 + 16 * t + 4 * lk;
      const q8_v4f m = *reinterpret_cast<const q8_v4f*>(mul + co);
      int q[Q8_ROWS][4];
#pragma unroll
      for (int j = 0; j < Q8_ROWS; ++j) {
        int sk = 0;
        if (skip != nullptr)
          sk = *reinterpret_cast<const int*>(skip + ((size_t)(n * g.HP + min(y0 + j, g.H - 1) + 1) * g.WP + pxc + 1) * g.C + co);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = (float)acc[j][t][r] * m[r];
          v = v >= 0.0f ? v : v * slope;
          if (skip != nullptr) v = v + (float)q8_byte(sk, r) * skip_mul;
          q[j][r] = q8_round(v);
        }
      }
      if (POOL) {
        const int Ho = g.H >> 1, Wo = g.W >> 1;
#pragma unroll
        for (int j = 0; j < Q8_ROWS; j += 2) {
          int o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = max(q[j][r], q[j + 1][r]);
            o[r] = max(v, __shfl_xor(v, 1, 64));
          }
          if (!(lp & 1) && px < g.W && y0 + j < g.H)
            *reinterpret_cast<int*>(y + ((size_t)(n * (Ho + 2) + ((y0 + j) >> 1) + 1) * (Wo + 2) + (px >> 1) + 1) * g.C + co) =
                q8_pack4(o[0], o[1], o[2], o[3]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < Q8_ROWS; ++j)
          if (px < g.W && y0 + j < g.H)
            *reinterpret_cast<int*>(y + ((size_t)(n * g.HP + y0 + j + 1) * g.WP + px + 1) * g.C + co) =
                q8_pack4(q[j][0], q[j][1], q[j][2], q[j][3]);
      }
    }
  }
}

inline bool q8_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------------
// The un-pooled tail of the trunk in ONE launch: nblocks residual blocks (2 * nblocks convs of 64 channels) on maps of at
// most 16 x 16.  A workgroup of four waves owns one image for the whole chain and keeps in LDS
//     two weight buffers  [tap][co][64] of one layer each, 36,864 bytes: layer L computes from buffer L & 1 while the
//                         threads hold layer L + 1 in registers (nine 16-byte loads each) and store it into the other
//                         buffer behind the layer's MFMAs,
//     two haloed planes   h and a, (H+2)(W+2) x 64 bytes each (at most 20,736): h is a copy of the image with its halo of
//                         zeros, a is zero-filled once; only real pixels are written, so the halo stays the padding,
//     biases, multipliers of every layer (16 KB), read from memory once per workgroup: inside the layer loop the only global
//                         loads are the next layer's weights, and nothing waits for them before the layer's MFMAs are done.
// The first conv of a block reads h and writes a; the second reads a and overwrites h in place -- a lane reads its own skip
// dword before it writes that dword, and no other lane touches it -- so one barrier per conv is all the ordering there is.
// A wave computes the 64 output channels of 4 rows x 16 columns exactly as k_q8_conv3x3 does (same fragments, same
// epilogue, operands from LDS): at most four row groups, one per wave.
constexpr int Q8C_MAXB = 16;                        // blocks per launch
constexpr int Q8C_MAXHW = 16;                       // one MFMA column tile per map row
constexpr int Q8C_WBYTES = 9 * 64 * 64;             // one layer's packed weights
constexpr int Q8C_PLANE = (Q8C_MAXHW + 2) * (Q8C_MAXHW + 2) * 64;
constexpr int Q8C_PARAMS = 2 * Q8C_MAXB * 64 * 4;                // one layer-major array of biases, one of multipliers
constexpr int Q8C_LDS = 2 * Q8C_WBYTES + 2 * Q8C_PLANE + 2 * Q8C_PARAMS;          // 131,584

struct Q8ChainArgs {
  const signed char* x;
  const signed char* w[2 * Q8C_MAXB];              // per conv, in execution order
  const int* bias[2 * Q8C_MAXB];
  const float* mul[2 * Q8C_MAXB];
  signed char* out[Q8C_MAXB];                       // per block: Q8 output, or nullptr
  float skip_mul[Q8C_MAXB];
  float* out_f32;
  float out_scale, slope;
  int nlayers, N, H, W;
};

__host__ __device__ inline bool q8_chain_shape_ok(int C, int H, int W) {
  return C == 64 && H >= 1 && W >= 1 && H <= Q8C_MAXHW && W <= Q8C_MAXHW;
}

__global__ __launch_bounds__(256) void k_q8_chain(const Q8ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char q8_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int H = a.H, W = a.W, HP = H + 2, WP = W + 2;
  const int plane = HP * WP * 64;                   // bytes; a multiple of 64
  unsigned char* const ph = q8_lds + 2 * Q8C_WBYTES;
  unsigned char* const pa = ph + Q8C_PLANE;
  const int row_groups = (H + Q8_ROWS - 1) / Q8_ROWS;           // <= 4: one per wave
  const int pxc = min(lp, W - 1);
  const int y0 = wave * Q8_ROWS;
  const bool live = wave < row_groups;
  const bool px_ok = lp < W;
  int* const lbias = reinterpret_cast<int*>(pa + Q8C_PLANE);                  // [layer][64]
  float* const lmul = reinterpret_cast<float*>(pa + Q8C_PLANE + Q8C_PARAMS);  // [layer][64]
  for (int i = tid; i < plane / 16; i += 256) reinterpret_cast<q8_v4i*>(pa)[i] = q8_v4i{0, 0, 0, 0};
  for (int i = tid; i < a.nlayers * 16; i += 256) {
    reinterpret_cast<q8_v4i*>(lbias)[i] = reinterpret_cast<const q8_v4i*>(a.bias[i >> 4])[i & 15];
    reinterpret_cast<q8_v4f*>(lmul)[i] = reinterpret_cast<const q8_v4f*>(a.mul[i >> 4])[i & 15];
  }
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    // layer 0's weights and the image.  Buffer 0 and h were last read two barriers ago (the last layer of the previous
    // image is odd: it reads buffer 1 and the a plane, and touches h only in its own dwords)
    {
      q8_v4i v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = reinterpret_cast<const q8_v4i*>(a.w[0])[k * 256 + tid];
      const q8_v4i* src = reinterpret_cast<const q8_v4i*>(a.x + (size_t)n * plane);
      for (int i = tid; i < plane / 16; i += 256) reinterpret_cast<q8_v4i*>(ph)[i] = src[i];
#pragma unroll
      for (int k = 0; k < 9; ++k) reinterpret_cast<q8_v4i*>(q8_lds)[k * 256 + tid] = v[k];
    }
    __syncthreads();
    for (int L = 0; L < a.nlayers; ++L) {
      const bool second = L & 1;
      const bool more = L + 1 < a.nlayers;
      q8_v4i nw[9];
      if (more) {
        const q8_v4i* wn = reinterpret_cast<const q8_v4i*>(a.w[L + 1]);
#pragma unroll
        for (int k = 0; k < 9; ++k) nw[k] = wn[k * 256 + tid];
      }
      if (live) {
        const unsigned char* src = second ? pa : ph;
        const unsigned char* wl = q8_lds + (L & 1) * Q8C_WBYTES + lp * 64 + lk * 16;
        const int* bias = lbias + L * 64;
        const float* mul = lmul + L * 64;
        q8_v4i acc[Q8_ROWS][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const q8_v4i b = *reinterpret_cast<const q8_v4i*>(bias + 16 * t + 4 * lk);
#pragma unroll
          for (int j = 0; j < Q8_ROWS; ++j) acc[j][t] = b;
        }
        // padded rows y0 .. y0 + 5 at columns px .. px + 2; rows past H + 1 belong to rows below the map only (clamped, never
        // stored), columns past W to lanes that store nothing
        q8_v4i b[Q8_ROWS + 2][3];
#pragma unroll
        for (int r = 0; r < Q8_ROWS + 2; ++r) {
          const unsigned char* xr = src + (min(y0 + r, H + 1) * WP + pxc) * 64 + lk * 16;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) b[r][kx] = *reinterpret_cast<const q8_v4i*>(xr + kx * 64);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap - 3 * (tap / 3);
          q8_v4i af[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) af[t] = *reinterpret_cast<const q8_v4i*>(wl + tap * 4096 + t * 1024);
#pragma unroll
          for (int j = 0; j < Q8_ROWS; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[j][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[t], b[j + ky][kx], acc[j][t], 0, 0, 0);
        }
        // epilogue of k_q8_conv3x3, into the other plane (first conv) or over the skip dword (second conv)
        const int blk = L >> 1;
        const float skip_mul = a.skip_mul[blk];
        signed char* const gout = second ? a.out[blk] : nullptr;
        float* const fout = L + 1 == a.nlayers ? a.out_f32 : nullptr;
        unsigned char* dst = second ? ph : pa;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int co = 16 * t + 4 * lk;
          const q8_v4f m = *reinterpret_cast<const q8_v4f*>(mul + co);
#pragma unroll
          for (int j = 0; j < Q8_ROWS; ++j) {
            const int yy = y0 + j;
            const int off = ((min(yy, H - 1) + 1) * WP + pxc + 1) * 64 + co;
            int sk = 0;
            if (second) sk = *reinterpret_cast<const int*>(ph + off);
            int q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float v = (float)acc[j][t][r] * m[r];
              v = v >= 0.0f ? v : v * a.slope;
              if (second) v = v + (float)q8_byte(sk, r) * skip_mul;
              q[r] = q8_round(v);
            }
            if (px_ok && yy < H) {
              const int pk = q8_pack4(q[0], q[1], q[2], q[3]);
              *reinterpret_cast<int*>(dst + off) = pk;
              if (gout != nullptr) *reinterpret_cast<int*>(gout + (size_t)n * plane + off) = pk;
              if (fout != nullptr) {
                float* d = fout + (((size_t)n * 64 + co) * H + yy) * W + lp;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[(size_t)r * H * W] = (float)q[r] * a.out_scale;
              }
            }
          }
        }
      }
      if (more) {
        q8_v4i* wd = reinterpret_cast<q8_v4i*>(q8_lds + ((L + 1) & 1) * Q8C_WBYTES);
#pragma unroll
        for (int k = 0; k < 9; ++k) wd[k * 256 + tid] = nw[k];
      }
      __syncthreads();
    }
  }
}


}  // namespace

extern "C" int fdet_q8_supported(int C, int H, int W) { return q8_shape_ok(C, H, W) ? 1 : 0; }

extern "C" size_t fdet_q8_act_bytes(int N, int C, int H, int W) { return q8_bytes(N, C, H, W); }

extern "C" int fdet_q8_quantize(const float* x, float scale, int8_t* q, int N, int C, int H, int W, void* stream) {
  FDET_REQUIRE(x && q && q8_bytes(N, C, H, W) > 0, "q8_quantize: unsupported shape N=%d C=%d H=%d W=%d (C %% 64 == 0, C <= 256)", N, C, H, W);
  FDET_REQUIRE(scale > 0.0f && scale <= 3.0e38f, "q8_quantize: scale must be positive and finite");
  FDET_REQUIRE((reinterpret_cast<uintptr_t>(q) & 3) == 0, "q8_quantize: the int8 tensor must be 4-byte aligned");
  const int tiles_x = (W + Q8_QT - 1) / Q8_QT;
  const long long blocks = (long long)N * H * tiles_x;
  FDET_REQUIRE(blocks < (1ll << 31), "q8_quantize: tensor too large");
  const Q8Geo g{N, C, H, W, H + 2, W + 2};
  hipLaunchKernelGGL(k_q8_quantize, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x,
                     reinterpret_cast<signed char*>(q), g, 1.0f / scale, tiles_x);
  return check_launch("fdet_q8_quantize");
}

extern "C" int fdet_q8_dequantize(const int8_t* q, float scale, float* x, int N, int C, int H, int W, void* stream) {
  FDET_REQUIRE(x && q && q8_bytes(N, C, H, W) > 0, "q8_dequantize: unsupported shape N=%d C=%d H=%d W=%d (C %% 64 == 0, C <= 256)", N, C, H, W);
  FDET_REQUIRE(scale > 0.0f && scale <= 3.0e38f, "q8_dequantize: scale must be positive and finite");
  FDET_REQUIRE((reinterpret_cast<uintptr_t>(q) & 3) == 0, "q8_dequantize: the int8 tensor must be 4-byte aligned");
  const long long total = (long long)N * (C / 4) * H * W;
  FDET_REQUIRE(total < (1ll << 31), "q8_dequantize: tensor too large");
  const Q8Geo g{N, C, H, W, H + 2, W + 2};
  hipLaunchKernelGGL(k_q8_dequantize, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const signed char*>(q), x, g, scale, (int)total);
  return check_launch("fdet_q8_dequantize");
}

extern "C" int fdet_q8_conv3x3(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, const int8_t* skip,
                               float skip_mul, int8_t* y, int N, int C, int H, int W, int pool, float slope, void* stream) {
  FDET_REQUIRE(x && wpk && bias && mul && y && q8_bytes(N, C, H, W) > 0,
               "q8_conv3x3: unsupported shape N=%d C=%d H=%d W=%d (C %% 64 == 0, C <= 256)", N, C, H, W);
  FDET_REQUIRE(pool == 0 || pool == 1, "q8_conv3x3: pool must be 0 or 1");
  FDET_REQUIRE(!pool || (!(H & 1) && !(W & 1)), "q8_conv3x3: the pooled form needs even H and W, got %dx%d", H, W);
  FDET_REQUIRE(q8_aligned16(x) && q8_aligned16(wpk) && q8_aligned16(bias) && q8_aligned16(mul) && q8_aligned16(y) &&
               q8_aligned16(skip), "q8_conv3x3: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y && skip != y, "q8_conv3x3: the output may not alias an input");
  const size_t lds = (size_t)9 * (C / 64) * 4096;
  FDET_REQUIRE(lds <= Q8_LDS_MAX, "q8_conv3x3: %d channels do not fit the LDS", C);
  const int tiles_x = (W + 15) / 16, row_groups = (H + Q8_ROWS - 1) / Q8_ROWS;
  const long long items = (long long)N * tiles_x * row_groups;
  FDET_REQUIRE(items < (1ll << 31), "q8_conv3x3: tensor too large");
  const Q8Geo g{N, C, H, W, H + 2, W + 2};
  // blocks resident on a CU next to each other (two by registers, fewer where the LDS says so), shared between the
  // output-channel chunks
  const int per_cu = (int)(Q8_LDS_MAX / lds) < 2 ? (int)(Q8_LDS_MAX / lds) : 2;
  long long gx = (items + 3) / 4;
  const long long cap = ((long long)num_cus() * per_cu + C / 64 - 1) / (C / 64);
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned)gx, (unsigned)(C / 64));
  const void* kern = pool ? (const void*)k_q8_conv3x3<true> : (const void*)k_q8_conv3x3<false>;
  if (lds > 64 * 1024) {
    const int rc = set_lds_attr(kern, lds, "fdet_q8_conv3x3");
    if (rc != FDET_OK) return rc;
  }
  const signed char* xs = reinterpret_cast<const signed char*>(x);
  const signed char* ws = reinterpret_cast<const signed char*>(wpk);
  const signed char* ss = reinterpret_cast<const signed char*>(skip);
  signed char* ys = reinterpret_cast<signed char*>(y);
  if (pool)
    hipLaunchKernelGGL(k_q8_conv3x3<true>, grid, dim3(256), lds, (hipStream_t)stream, xs, ws, bias, mul, ss, skip_mul, ys, g, tiles_x,
                       row_groups, (int)items, slope);
  else
    hipLaunchKernelGGL(k_q8_conv3x3<false>, grid, dim3(256), lds, (hipStream_t)stream, xs, ws, bias, mul, ss, skip_mul, ys, g, tiles_x,
                       row_groups, (int)items, slope);
  return check_launch("fdet_q8_conv3x3");
}

extern "C" int fdet_q8_chain_supported(int C, int H, int W) { return q8_chain_shape_ok(C, H, W) ? 1 : 0; }

extern "C" int fdet_q8_chain(const int8_t* x, const int8_t* const* h_wpk1, const int32_t* const* h_b1, const float* const* h_mul1,
                             const int8_t* const* h_wpk2, const int32_t* const* h_b2, const float* const* h_mul2,
                             const float* h_skip_mul, int8_t* const* h_out, float* out_f32, float out_scale, int nblocks, int N,
                             int C, int H, int W, float slope, void* stream) {
  FDET_REQUIRE(q8_chain_shape_ok(C, H, W) && N >= 1 && q8_bytes(N, C, H, W) > 0,
               "q8_chain: unsupported shape N=%d C=%d H=%d W=%d (C == 64, 1 <= H, W <= %d)", N, C, H, W, Q8C_MAXHW);
  FDET_REQUIRE(nblocks >= 1 && nblocks <= Q8C_MAXB, "q8_chain: nblocks must be 1..%d, got %d", Q8C_MAXB, nblocks);
  FDET_REQUIRE(x && h_wpk1 && h_b1 && h_mul1 && h_wpk2 && h_b2 && h_mul2 && h_skip_mul, "q8_chain: null argument");
  FDET_REQUIRE((h_out && h_out[nblocks - 1]) || out_f32, "q8_chain: the last block needs an output (h_out[nblocks - 1] or out_f32)");
  FDET_REQUIRE(out_f32 == nullptr || (out_scale > 0.0f && out_scale <= 3.0e38f), "q8_chain: out_scale must be positive and finite");
  Q8ChainArgs a{};
  a.x = reinterpret_cast<const signed char*>(x);
  bool ok = q8_aligned16(x) && q8_aligned16(out_f32);
  for (int k = 0; k < nblocks; ++k) {
    FDET_REQUIRE(h_wpk1[k] && h_b1[k] && h_mul1[k] && h_wpk2[k] && h_b2[k] && h_mul2[k], "q8_chain: null tensor in block %d", k);
    a.w[2 * k] = reinterpret_cast<const signed char*>(h_wpk1[k]);
    a.w[2 * k + 1] = reinterpret_cast<const signed char*>(h_wpk2[k]);
    a.bias[2 * k] = h_b1[k];
    a.bias[2 * k + 1] = h_b2[k];
    a.mul[2 * k] = h_mul1[k];
    a.mul[2 * k + 1] = h_mul2[k];
    a.skip_mul[k] = h_skip_mul[k];
    a.out[k] = h_out ? reinterpret_cast<signed char*>(h_out[k]) : nullptr;
    FDET_REQUIRE(a.out[k] == nullptr || a.out[k] != a.x, "q8_chain: an output may not alias x");
    ok = ok && q8_aligned16(h_wpk1[k]) && q8_aligned16(h_wpk2[k]) && q8_aligned16(h_b1[k]) && q8_aligned16(h_b2[k]) &&
         q8_aligned16(h_mul1[k]) && q8_aligned16(h_mul2[k]) && q8_aligned16(a.out[k]);
  }
  FDET_REQUIRE(ok, "q8_chain: every tensor must be 16-byte aligned");
  a.out_f32 = out_f32;
  a.out_scale = out_scale;
  a.slope = slope;
  a.nlayers = 2 * nblocks;
  a.N = N; a.H = H; a.W = W;
  const int rc = set_lds_attr((const void*)k_q8_chain, Q8C_LDS, "fdet_q8_chain");
  if (rc != FDET_OK) return rc;
  const int grid = N < num_cus() ? N : num_cus();      // one workgroup per CU (LDS), one image at a time
  hipLaunchKernelGGL(k_q8_chain, dim3((unsigned)grid), dim3(256), Q8C_LDS, (hipStream_t)stream, a);
  return check_launch("fdet_q8_chain");
}
