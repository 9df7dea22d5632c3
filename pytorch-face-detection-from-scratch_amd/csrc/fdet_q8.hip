// Int8 post-training-quantised inference (gfx950): 3x3 and 1x1 convolutions on the integer matrix cores
// (v_mfma_i32_16x16x64_i8) with the requantising epilogue in registers, the LDS-resident chain of un-pooled residual blocks,
// the Linear(C,5) head, and the converters between fp32 NCHW and the int8 activation layout.  The arithmetic is the contract of
// include/fdet.h ("Int8 inference" and "Int8 inference: mixed widths"); tests/q8_cpu_ref.py and tests/q8_ssd_cpu_ref.py
// restate it in numpy and the GPU tests demand equality.  The layout, the rounding, the epilogue and the nine-tap fragment walk
// are fdet_q8_common.h's.
//
// One conv kernel family serves the square entry (fdet_q8_conv3x3: C -> C, C a multiple of 64) and the mixed-width ones
// (fdet_q8x_conv3x3, fdet_q8x_pointwise: any multiples of 16 up to 256, as the SSD trunk has them).
// Packed weights: K flattened tap-major, channel-minor (k = tap * Cin + ci), zero-padded to a multiple of 64 and
// laid out as [K/64][Cout][64].  One v_mfma_i32_16x16x64_i8 step takes k = 64 s .. 64 s + 63; lane group g = lane >> 4 holds
// the 16 bytes k = 64 s + 16 g .. + 15 of both operands, and with Cin a multiple of 16 these never straddle a tap: Cin = 16
// puts four taps into one step (3 steps, three zero slots), Cin = 32 two (5 steps, one zero slot), Cin a multiple of 64 is
// the per-tap, per-chunk walk of q8::taps9 ([tap][Cin/64][Cout][64]: the square entry's packed order).  A lane group whose
// slot is past the last tap reads the last tap's last 16 channels (a valid address) against zero weights.
//   A (weights): lane l holds the slot's 16 bytes of row co = 16 t + (l & 15)
//   B (pixels):  lane l holds the same slot of pixel column (l & 15), at the slot's tap offset
//   D:           lane l holds co = 16 t + 4 (l >> 4) + r (r = 0..3) of pixel (l & 15): four channels = one dword store
// A block computes NT 16-channel tiles (1, 2 or 4: Cout = 16 or 32 compute no channel that is thrown away) and keeps their
// weights in LDS; a wave walks work items of 4 rows x 16 columns.
#include "fdet_common.h"
#include "fdet_q8_common.h"

namespace {
using namespace fdet;
using q8::v4i;
using q8::v4f;

struct Q8Geo {
  int N, C, H, W, HP, WP;
};

// fp32 NCHW -> Q8.  One block per (image, row, 32 columns) and all channels: thread (column, channel group) reads four
// channel planes (32 lanes = 128 contiguous bytes each), packs a dword into an LDS tile [column][C/4 (+1: banks)], and the
// tile -- contiguous in the channel-innermost output -- goes out in consecutive dwords.
constexpr int Q8_QT = 32;
__global__ __launch_bounds__(256) void k_q8_quantize(const float* __restrict__ x, signed char* __restrict__ q, Q8Geo g, float inv_s,
                                                      int tiles_x) {
  __shared__ int tile[Q8_QT * (q8::MAX_C / 4 + 1)];
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
        v[k] = q8::round_q_nan0(t);
      }
      tile[col * (C4 + 1) + c4] = q8::pack4(v[0], v[1], v[2], v[3]);
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
  for (int k = 0; k < 4; ++k) dst[k * plane] = (float)q8::byte_of(w, k) * s;
}

struct Q8ConvGeo {
  int N, Cin, Cout, H, W, HP, WP;
};

// 3x3 conv (ntaps == 9) or 1x1 conv at the centre tap (ntaps == 1), Cin -> Cout, on Q8 tensors.  Block = 4 waves that share
// the 16 NT output channels blockIdx.y * 16 NT .. and keep their packed weights in LDS ([K/64][16 NT][64]); every wave walks
// work items of 4 rows x 16 columns of one image.  Lanes whose pixel lies outside the map read a clamped (valid) pixel and
// store nothing.  WIDE (Cin a multiple of 64, 3x3): q8::taps9 -- 18 loads per 64-channel chunk, each used by up to three
// (row, tap) pairs.  Otherwise one load per (row, step) at the lane group's own tap.
template <int NT, bool POOL, bool WIDE>
__global__ __launch_bounds__(256) void k_q8_conv(const signed char* __restrict__ x, const signed char* __restrict__ wpk,
                                                  const int* __restrict__ bias, const float* __restrict__ mul,
                                                  const signed char* __restrict__ skip, float skip_mul,
                                                  signed char* __restrict__ y, Q8ConvGeo g, int KS, int ntaps, int tiles_x, int row_groups,
                                                  int items, float slope) {
  extern __shared__ __attribute__((aligned(16))) unsigned char q8_lds[];
  constexpr int CB = 16 * NT;                              // output channels of the block
  const int co0 = blockIdx.y * CB;
  if (WIDE && NT == 4) {
    // 256 16-byte units per step and KS a multiple of 9: nine loads in flight per thread, then nine LDS stores
    for (int s0 = 0; s0 < KS; s0 += 9) {
      v4i v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k)
        v[k] = *reinterpret_cast<const v4i*>(wpk + ((size_t)(s0 + k) * g.Cout + co0) * 64 + threadIdx.x * 16);
#pragma unroll
      for (int k = 0; k < 9; ++k) reinterpret_cast<v4i*>(q8_lds)[(s0 + k) * 256 + threadIdx.x] = v[k];
    }
  } else {
    for (int u = threadIdx.x; u < KS * CB * 4; u += 256) {   // 16-byte units: CB * 4 per step, contiguous in wpk
      const int s = u / (CB * 4), r = u - s * (CB * 4);
      reinterpret_cast<v4i*>(q8_lds)[u] = *reinterpret_cast<const v4i*>(wpk + ((size_t)s * g.Cout + co0) * 64 + (size_t)r * 16);
    }
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
    const int y0 = rg * q8::ROWS;
    v4i acc[q8::ROWS][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const v4i b = *reinterpret_cast<const v4i*>(bias + co0 + 16 * t + 4 * lk);
#pragma unroll
      for (int j = 0; j < q8::ROWS; ++j) acc[j][t] = b;
    }
    // padded rows y0 .. y0 + 5 (row j, tap ky -> padded row y0 + j + ky) at columns px .. px + 2.  Padded rows past H + 1
    // belong to rows of the item below the map only: clamped, their results are never stored.
    const signed char* xr[q8::ROWS + 2];
#pragma unroll
    for (int r = 0; r < q8::ROWS + 2; ++r)
      xr[r] = x + ((size_t)(n * g.HP + min(y0 + r, g.H + 1)) * g.WP + pxc) * g.Cin + (WIDE ? lk * 16 : 0);
    if (WIDE) {
      const int KC = g.Cin >> 6;
      for (int kc = 0; kc < KC; ++kc) {
        v4i b[q8::ROWS + 2][3];
#pragma unroll
        for (int r = 0; r < q8::ROWS + 2; ++r)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) b[r][kx] = *reinterpret_cast<const v4i*>(xr[r] + (size_t)kx * g.Cin + kc * 64);
        __builtin_amdgcn_sched_barrier(0);                 // keep the 18 loads ahead of the MFMAs (the scheduler sinks them)
        q8::taps9<NT>(acc, b, wl + (size_t)kc * (CB * 64), KC * (CB * 64));
      }
    } else {
      const int K = ntaps * g.Cin;
      // the four pixel fragments of step s: the lane group's slot k = 64 s + 16 lk, its tap and first channel; a slot past K
      // has zero weights and reads the last real slot's bytes
      auto fetch = [&](int s, v4i(&b)[q8::ROWS]) {
        const int k = min(64 * s + 16 * lk, K - 16);
        const int tap = ntaps == 9 ? k / g.Cin : 4;
        const int ci = ntaps == 9 ? k - tap * g.Cin : k;
        const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
        for (int j = 0; j < q8::ROWS; ++j) {
          // (a select over the six row pointers: ky is not known at compile time)
          const int r = j + ky;
          const signed char* p = r == 0 ? xr[0] : r == 1 ? xr[1] : r == 2 ? xr[2] : r == 3 ? xr[3] : r == 4 ? xr[4] : xr[5];
          b[j] = *reinterpret_cast<const v4i*>(p + (size_t)kx * g.Cin + ci);
        }
      };
      v4i b[q8::ROWS], bn[q8::ROWS];
      fetch(0, b);
#pragma unroll
      for (int j = 0; j < q8::ROWS; ++j) bn[j] = b[j];
      for (int s = 0; s < KS; ++s) {
        if (s + 1 < KS) fetch(s + 1, bn);                  // the next step's loads fly behind this step's MFMAs
        v4i a[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const v4i*>(wl + (size_t)s * (CB * 64) + t * 1024);
#pragma unroll
        for (int j = 0; j < q8::ROWS; ++j)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[j][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b[j], acc[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < q8::ROWS; ++j) b[j] = bn[j];
      }
    }
    // epilogue: multiplier, LeakyReLU, skip, requantise (, 2x2 floor max), four channels of one pixel per dword
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int co = co0 + 16 * t + 4 * lk;
      const v4f m = *reinterpret_cast<const v4f*>(mul + co);
      int q[q8::ROWS][4];
#pragma unroll
      for (int j = 0; j < q8::ROWS; ++j) {
        int sk = 0;
        if (skip != nullptr)
          sk = *reinterpret_cast<const int*>(skip + ((size_t)(n * g.HP + min(y0 + j, g.H - 1) + 1) * g.WP + pxc + 1) * g.Cout + co);
        q8::requant4(q[j], acc[j][t], m, slope, skip != nullptr, sk, skip_mul);
      }
      if (POOL) {
        // floor pool: a window needs both of its rows and both of its columns inside the map, so an odd last row or column
        // takes part in none.  On the even maps that fdet_q8_conv3x3 demands this selects the lanes that px < W && y0 + j < H
        // selects (px and y0 + j are even here).
        const int Ho = g.H >> 1, Wo = g.W >> 1;
#pragma unroll
        for (int j = 0; j < q8::ROWS; j += 2) {
          int o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = max(q[j][r], q[j + 1][r]);
            o[r] = max(v, __shfl_xor(v, 1, 64));
          }
          if (!(lp & 1) && px + 1 < g.W && y0 + j + 1 < g.H)
            *reinterpret_cast<int*>(y + ((size_t)(n * (Ho + 2) + ((y0 + j) >> 1) + 1) * (Wo + 2) + (px >> 1) + 1) * g.Cout + co) =
                q8::pack4(o[0], o[1], o[2], o[3]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < q8::ROWS; ++j)
          if (px < g.W && y0 + j < g.H)
            *reinterpret_cast<int*>(y + ((size_t)(n * g.HP + y0 + j + 1) * g.WP + px + 1) * g.Cout + co) =
                q8::pack4(q[j][0], q[j][1], q[j][2], q[j][3]);
      }
    }
  }
}

// per_cu: the blocks resident on a CU next to each other that the grid is capped by (shared between the output-channel
// chunks), or 0 to ask the runtime what registers and this launch's LDS allow (once per kernel and step count).
template <int NT, bool POOL, bool WIDE>
int q8_launch(const signed char* x, const signed char* w, const int* bias, const float* mul, const signed char* skip, float skip_mul,
              signed char* y, const Q8ConvGeo& g, int KS, int ntaps, float slope, int per_cu, hipStream_t stream, const char* what) {
  const size_t lds = (size_t)KS * NT * 1024;
  if (lds > q8::LDS_MAX) return fail(FDET_EINVAL, "%s: %d -> %d channels do not fit the LDS", what, g.Cin, g.Cout);
  const int tiles_x = (g.W + 15) / 16, row_groups = (g.H + q8::ROWS - 1) / q8::ROWS;
  const long long items = (long long)g.N * tiles_x * row_groups;
  if (items >= (1ll << 31)) return fail(FDET_EINVAL, "%s: tensor too large", what);
  const int chunks = g.Cout / (16 * NT);
  const void* kern = (const void*)k_q8_conv<NT, POOL, WIDE>;
  if (lds > 64 * 1024) {
    const int rc = set_lds_attr(kern, lds, what);
    if (rc != FDET_OK) return rc;
  }
  static int resident[q8::MAX_C * 9 / 64 + 1] = {};
  if (per_cu == 0 && (per_cu = resident[KS]) == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      per_cu = 1;
    }
    resident[KS] = per_cu;
  }
  long long gx = (items + 3) / 4;
  const long long cap = ((long long)num_cus() * per_cu + chunks - 1) / chunks;
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL((k_q8_conv<NT, POOL, WIDE>), dim3((unsigned)gx, (unsigned)chunks), dim3(256), lds, stream, x, w, bias, mul, skip,
                     skip_mul, y, g, KS, ntaps, tiles_x, row_groups, (int)items, slope);
  return check_launch(what);
}

template <int NT>
int q8_dispatch(const signed char* x, const signed char* w, const int* bias, const float* mul, const signed char* skip, float skip_mul,
                signed char* y, const Q8ConvGeo& g, int KS, int ntaps, int pool, float slope, int per_cu, hipStream_t stream,
                const char* what) {
  const bool wide = ntaps == 9 && (g.Cin & 63) == 0;
  if (pool)
    return wide ? q8_launch<NT, true, true>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, per_cu, stream, what)
                : q8_launch<NT, true, false>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, per_cu, stream, what);
  return wide ? q8_launch<NT, false, true>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, per_cu, stream, what)
              : q8_launch<NT, false, false>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, per_cu, stream, what);
}

// The one launcher of fdet_q8_conv3x3, fdet_q8x_conv3x3 and fdet_q8x_pointwise; the entry has validated the arguments.
int q8_conv(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, const int8_t* skip, float skip_mul, int8_t* y,
            int N, int Cin, int Cout, int H, int W, int ntaps, int pool, float slope, int per_cu, void* stream, const char* what) {
  const Q8ConvGeo g{N, Cin, Cout, H, W, H + 2, W + 2};
  const int KS = (ntaps * Cin + 63) / 64;
  const signed char* xs = reinterpret_cast<const signed char*>(x);
  const signed char* ws = reinterpret_cast<const signed char*>(wpk);
  const signed char* ss = reinterpret_cast<const signed char*>(skip);
  signed char* ys = reinterpret_cast<signed char*>(y);
  hipStream_t st = (hipStream_t)stream;
  if ((Cout & 63) == 0) return q8_dispatch<4>(xs, ws, bias, mul, ss, skip_mul, ys, g, KS, ntaps, pool, slope, per_cu, st, what);
  if ((Cout & 31) == 0) return q8_dispatch<2>(xs, ws, bias, mul, ss, skip_mul, ys, g, KS, ntaps, pool, slope, per_cu, st, what);
  return q8_dispatch<1>(xs, ws, bias, mul, ss, skip_mul, ys, g, KS, ntaps, pool, slope, per_cu, st, what);
}

// Linear(C,5) at every position of a Q8 map: one thread per pixel, the five weight rows are the same for every lane.
__global__ __launch_bounds__(256) void k_q8x_head(const signed char* __restrict__ x, const signed char* __restrict__ w,
                                                   const int* __restrict__ bias, const float* __restrict__ m, float* __restrict__ z,
                                                   int N, int C, int H, int W, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xx = i % W;
  const int r = i / W;
  const int yy = r % H, n = r / H;
  const signed char* p = x + ((size_t)(n * (H + 2) + yy + 1) * (W + 2) + xx + 1) * C;
  int acc[5];
#pragma unroll
  for (int o = 0; o < 5; ++o) acc[o] = bias[o];
  for (int c = 0; c < C; c += 16) {
    const v4i v = *reinterpret_cast<const v4i*>(p + c);
#pragma unroll
    for (int o = 0; o < 5; ++o) {
      const v4i wv = *reinterpret_cast<const v4i*>(w + (size_t)o * C + c);
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[o] += q8::byte_of(v[d], b) * q8::byte_of(wv[d], b);
    }
  }
  const size_t plane = (size_t)H * W;
  float* dst = z + (size_t)n * 5 * plane + (size_t)yy * W + xx;
#pragma unroll
  for (int o = 0; o < 5; ++o) dst[o * plane] = (float)acc[o] * m[o];
}

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
// A wave computes the 64 output channels of 4 rows x 16 columns exactly as k_q8_conv does (the same q8::taps9 and
// q8::requant4, operands from LDS): at most four row groups, one per wave.
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
  const int row_groups = (H + q8::ROWS - 1) / q8::ROWS;           // <= 4: one per wave
  const int pxc = min(lp, W - 1);
  const int y0 = wave * q8::ROWS;
  const bool live = wave < row_groups;
  const bool px_ok = lp < W;
  int* const lbias = reinterpret_cast<int*>(pa + Q8C_PLANE);                  // [layer][64]
  float* const lmul = reinterpret_cast<float*>(pa + Q8C_PLANE + Q8C_PARAMS);  // [layer][64]
  for (int i = tid; i < plane / 16; i += 256) reinterpret_cast<v4i*>(pa)[i] = v4i{0, 0, 0, 0};
  for (int i = tid; i < a.nlayers * 16; i += 256) {
    reinterpret_cast<v4i*>(lbias)[i] = reinterpret_cast<const v4i*>(a.bias[i >> 4])[i & 15];
    reinterpret_cast<v4f*>(lmul)[i] = reinterpret_cast<const v4f*>(a.mul[i >> 4])[i & 15];
  }
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    // layer 0's weights and the image.  Buffer 0 and h were last read two barriers ago (the last layer of the previous
    // image is odd: it reads buffer 1 and the a plane, and touches h only in its own dwords)
    {
      v4i v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = reinterpret_cast<const v4i*>(a.w[0])[k * 256 + tid];
      const v4i* src = reinterpret_cast<const v4i*>(a.x + (size_t)n * plane);
      for (int i = tid; i < plane / 16; i += 256) reinterpret_cast<v4i*>(ph)[i] = src[i];
#pragma unroll
      for (int k = 0; k < 9; ++k) reinterpret_cast<v4i*>(q8_lds)[k * 256 + tid] = v[k];
    }
    __syncthreads();
    for (int L = 0; L < a.nlayers; ++L) {
      const bool second = L & 1;
      const bool more = L + 1 < a.nlayers;
      v4i nw[9];
      if (more) {
        const v4i* wn = reinterpret_cast<const v4i*>(a.w[L + 1]);
#pragma unroll
        for (int k = 0; k < 9; ++k) nw[k] = wn[k * 256 + tid];
      }
      if (live) {
        const unsigned char* src = second ? pa : ph;
        const unsigned char* wl = q8_lds + (L & 1) * Q8C_WBYTES + lp * 64 + lk * 16;
        const int* bias = lbias + L * 64;
        const float* mul = lmul + L * 64;
        v4i acc[q8::ROWS][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const v4i b = *reinterpret_cast<const v4i*>(bias + 16 * t + 4 * lk);
#pragma unroll
          for (int j = 0; j < q8::ROWS; ++j) acc[j][t] = b;
        }
        // padded rows y0 .. y0 + 5 at columns px .. px + 2; rows past H + 1 belong to rows below the map only (clamped, never
        // stored), columns past W to lanes that store nothing
        v4i b[q8::ROWS + 2][3];
#pragma unroll
        for (int r = 0; r < q8::ROWS + 2; ++r) {
          const unsigned char* xr = src + (min(y0 + r, H + 1) * WP + pxc) * 64 + lk * 16;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) b[r][kx] = *reinterpret_cast<const v4i*>(xr + kx * 64);
        }
        q8::taps9<4>(acc, b, wl, 4096);
        // epilogue of k_q8_conv, into the other plane (first conv) or over the skip dword (second conv)
        const int blk = L >> 1;
        const float skip_mul = a.skip_mul[blk];
        signed char* const gout = second ? a.out[blk] : nullptr;
        float* const fout = L + 1 == a.nlayers ? a.out_f32 : nullptr;
        unsigned char* dst = second ? ph : pa;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int co = 16 * t + 4 * lk;
          const v4f m = *reinterpret_cast<const v4f*>(mul + co);
#pragma unroll
          for (int j = 0; j < q8::ROWS; ++j) {
            const int yy = y0 + j;
            const int off = ((min(yy, H - 1) + 1) * WP + pxc + 1) * 64 + co;
            int sk = 0;
            if (second) sk = *reinterpret_cast<const int*>(ph + off);
            int q[4];
            q8::requant4(q, acc[j][t], m, a.slope, second, sk, skip_mul);
            if (px_ok && yy < H) {
              const int pk = q8::pack4(q[0], q[1], q[2], q[3]);
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
        v4i* wd = reinterpret_cast<v4i*>(q8_lds + ((L + 1) & 1) * Q8C_WBYTES);
#pragma unroll
        for (int k = 0; k < 9; ++k) wd[k * 256 + tid] = nw[k];
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int fdet_q8_supported(int C, int H, int W) { return q8::act_shape_ok(C, H, W, 64) ? 1 : 0; }

extern "C" size_t fdet_q8_act_bytes(int N, int C, int H, int W) { return q8::act_bytes(N, C, H, W, 64); }

extern "C" int fdet_q8_quantize(const float* x, float scale, int8_t* q, int N, int C, int H, int W, void* stream) {
  FDET_REQUIRE(x && q && q8::act_bytes(N, C, H, W, 64) > 0, "q8_quantize: unsupported shape N=%d C=%d H=%d W=%d (C %% 64 == 0, C <= 256)", N, C,
               H, W);
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
  FDET_REQUIRE(x && q && q8::act_bytes(N, C, H, W, 64) > 0, "q8_dequantize: unsupported shape N=%d C=%d H=%d W=%d (C %% 64 == 0, C <= 256)", N,
               C, H, W);
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
  FDET_REQUIRE(x && wpk && bias && mul && y && q8::act_bytes(N, C, H, W, 64) > 0,
               "q8_conv3x3: unsupported shape N=%d C=%d H=%d W=%d (C %% 64 == 0, C <= 256)", N, C, H, W);
  FDET_REQUIRE(pool == 0 || pool == 1, "q8_conv3x3: pool must be 0 or 1");
  FDET_REQUIRE(!pool || (!(H & 1) && !(W & 1)), "q8_conv3x3: the pooled form needs even H and W, got %dx%d", H, W);
  FDET_REQUIRE(q8::aligned16(x) && q8::aligned16(wpk) && q8::aligned16(bias) && q8::aligned16(mul) && q8::aligned16(y) &&
               q8::aligned16(skip), "q8_conv3x3: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y && skip != y, "q8_conv3x3: the output may not alias an input");
  const size_t lds = (size_t)9 * (C / 64) * 4096;
  FDET_REQUIRE(lds <= q8::LDS_MAX, "q8_conv3x3: %d channels do not fit the LDS", C);
  // blocks resident on a CU next to each other: two by registers, fewer where the LDS says so
  const int per_cu = (int)(q8::LDS_MAX / lds) < 2 ? (int)(q8::LDS_MAX / lds) : 2;
  return q8_conv(x, wpk, bias, mul, skip, skip_mul, y, N, C, C, H, W, 9, pool, slope, per_cu, stream, "fdet_q8_conv3x3");
}

extern "C" int fdet_q8_chain_supported(int C, int H, int W) { return q8_chain_shape_ok(C, H, W) ? 1 : 0; }

extern "C" int fdet_q8_chain(const int8_t* x, const int8_t* const* h_wpk1, const int32_t* const* h_b1, const float* const* h_mul1,
                             const int8_t* const* h_wpk2, const int32_t* const* h_b2, const float* const* h_mul2,
                             const float* h_skip_mul, int8_t* const* h_out, float* out_f32, float out_scale, int nblocks, int N,
                             int C, int H, int W, float slope, void* stream) {
  FDET_REQUIRE(q8_chain_shape_ok(C, H, W) && N >= 1 && q8::act_bytes(N, C, H, W, 64) > 0,
               "q8_chain: unsupported shape N=%d C=%d H=%d W=%d (C == 64, 1 <= H, W <= %d)", N, C, H, W, Q8C_MAXHW);
  FDET_REQUIRE(nblocks >= 1 && nblocks <= Q8C_MAXB, "q8_chain: nblocks must be 1..%d, got %d", Q8C_MAXB, nblocks);
  FDET_REQUIRE(x && h_wpk1 && h_b1 && h_mul1 && h_wpk2 && h_b2 && h_mul2 && h_skip_mul, "q8_chain: null argument");
  FDET_REQUIRE((h_out && h_out[nblocks - 1]) || out_f32, "q8_chain: the last block needs an output (h_out[nblocks - 1] or out_f32)");
  FDET_REQUIRE(out_f32 == nullptr || (out_scale > 0.0f && out_scale <= 3.0e38f), "q8_chain: out_scale must be positive and finite");
  Q8ChainArgs a{};
  a.x = reinterpret_cast<const signed char*>(x);
  bool ok = q8::aligned16(x) && q8::aligned16(out_f32);
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
    ok = ok && q8::aligned16(h_wpk1[k]) && q8::aligned16(h_wpk2[k]) && q8::aligned16(h_b1[k]) && q8::aligned16(h_b2[k]) &&
         q8::aligned16(h_mul1[k]) && q8::aligned16(h_mul2[k]) && q8::aligned16(a.out[k]);
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

extern "C" int fdet_q8x_supported(int C, int H, int W) { return q8::act_shape_ok(C, H, W, 16) ? 1 : 0; }

extern "C" size_t fdet_q8x_act_bytes(int N, int C, int H, int W) { return q8::act_bytes(N, C, H, W, 16); }

extern "C" int fdet_q8x_conv3x3_ok(int N, int Cin, int Cout, int H, int W, int pool) {
  if (pool != 0 && pool != 1) return 0;
  if (q8::act_bytes(N, Cin, H, W, 16) == 0 || q8::act_bytes(N, Cout, H, W, 16) == 0) return 0;
  if (pool && (H < 2 || W < 2)) return 0;
  return 1;
}

extern "C" int fdet_q8x_conv3x3(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, const int8_t* skip,
                                float skip_mul, int8_t* y, int N, int Cin, int Cout, int H, int W, int pool, float slope,
                                void* stream) {
  FDET_REQUIRE(x && wpk && bias && mul && y, "q8x_conv3x3: null argument");
  FDET_REQUIRE(pool == 0 || pool == 1, "q8x_conv3x3: pool must be 0 or 1");
  FDET_REQUIRE(fdet_q8x_conv3x3_ok(N, Cin, Cout, H, W, pool),
               "q8x_conv3x3: unsupported shape N=%d Cin=%d Cout=%d H=%d W=%d pool=%d (channels: multiples of 16 up to %d, "
               "1 <= H, W <= %d, at least 2 x 2 when pooled, tensors under 2^31 bytes)", N, Cin, Cout, H, W, pool, q8::MAX_C, q8::MAX_HW);
  FDET_REQUIRE(q8::aligned16(x) && q8::aligned16(wpk) && q8::aligned16(bias) && q8::aligned16(mul) && q8::aligned16(y) &&
               q8::aligned16(skip), "q8x_conv3x3: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y && skip != y, "q8x_conv3x3: the output may not alias an input");
  return q8_conv(x, wpk, bias, mul, skip, skip_mul, y, N, Cin, Cout, H, W, 9, pool, slope, 0, stream, "fdet_q8x_conv3x3");
}

extern "C" int fdet_q8x_pointwise_ok(int N, int Cin, int Cout, int H, int W) {
  return q8::act_bytes(N, Cin, H, W, 16) > 0 && q8::act_bytes(N, Cout, H, W, 16) > 0 ? 1 : 0;
}

extern "C" int fdet_q8x_pointwise(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, int8_t* y, int N, int Cin,
                                  int Cout, int H, int W, void* stream) {
  FDET_REQUIRE(x && wpk && bias && mul && y, "q8x_pointwise: null argument");
  FDET_REQUIRE(fdet_q8x_pointwise_ok(N, Cin, Cout, H, W),
               "q8x_pointwise: unsupported shape N=%d Cin=%d Cout=%d H=%d W=%d (channels: multiples of 16 up to %d, 1 <= H, W <= %d, "
               "tensors under 2^31 bytes)", N, Cin, Cout, H, W, q8::MAX_C, q8::MAX_HW);
  FDET_REQUIRE(q8::aligned16(x) && q8::aligned16(wpk) && q8::aligned16(bias) && q8::aligned16(mul) && q8::aligned16(y),
               "q8x_pointwise: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y, "q8x_pointwise: the output may not alias the input");
  // identity activation: slope 1 (t * 1.0f is t)
  return q8_conv(x, wpk, bias, mul, nullptr, 0.0f, y, N, Cin, Cout, H, W, 1, 0, 1.0f, 0, stream, "fdet_q8x_pointwise");
}

extern "C" int fdet_q8x_head_ok(int N, int C, int H, int W) {
  if (q8::act_bytes(N, C, H, W, 16) == 0) return 0;
  return (unsigned long long)N * 5 * H * W * 4 < (1ull << 31) ? 1 : 0;
}

extern "C" int fdet_q8x_head_f32(const int8_t* x, const int8_t* w_q, const int32_t* b_q, const float* m, float* z, int N, int C, int H,
                                 int W, void* stream) {
  FDET_REQUIRE(x && w_q && b_q && m && z, "q8x_head_f32: null argument");
  FDET_REQUIRE(fdet_q8x_head_ok(N, C, H, W),
               "q8x_head_f32: unsupported shape N=%d C=%d H=%d W=%d (C a multiple of 16 up to %d, 1 <= H, W <= %d, tensors under 2^31 "
               "bytes)", N, C, H, W, q8::MAX_C, q8::MAX_HW);
  FDET_REQUIRE(q8::aligned16(x) && q8::aligned16(w_q) && q8::aligned16(b_q) && q8::aligned16(m) && q8::aligned16(z),
               "q8x_head_f32: every tensor must be 16-byte aligned");
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(k_q8x_head, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const signed char*>(x), reinterpret_cast<const signed char*>(w_q), b_q, m, z, N, C, H, W, (int)total);
  return check_launch("fdet_q8x_head_f32");
}
