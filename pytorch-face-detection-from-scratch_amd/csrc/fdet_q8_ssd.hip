// Int8 inference of the SSD detector (gfx950): the mixed-width integer convs that fdet_q8.hip does not cover.  The trunk of
// SSD(filters = 16) has 16, 32, 64, 128 and 256 channels, blocks whose width changes (each with a 1x1 skip conv), a floor
// pool 15 -> 7 and four Linear(C,5) heads, and its stem has 16 filters.  The arithmetic is the contract of include/fdet.h
// ("Int8 inference: mixed widths"); tests/q8_ssd_cpu_ref.py restates it in numpy and the GPU tests demand equality.
//
// Activation layout: the Q8 layout of fdet_q8.hip, int8 [N][H+2][W+2][C] with a halo of zeros, for C any multiple of 16 up
// to 256.  Packed weights: K flattened tap-major, channel-minor (k = tap * Cin + ci), zero-padded to a multiple of 64 and
// laid out as [K/64][Cout][64].  One v_mfma_i32_16x16x64_i8 step takes k = 64 s .. 64 s + 63; lane group g = lane >> 4 holds
// the 16 bytes k = 64 s + 16 g .. + 15 of both operands, and with Cin a multiple of 16 these never straddle a tap: Cin = 16
// puts four taps into one step (3 steps, three zero slots), Cin = 32 two (5 steps, one zero slot), Cin a multiple of 64 is
// the per-tap, per-chunk walk of k_q8_conv3x3, whose packed order this is.  A lane group whose slot is past the last tap
// reads the last tap's last 16 channels (a valid address) against zero weights.
//   A (weights): lane l holds the slot's 16 bytes of row co = 16 t + (l & 15)
//   B (pixels):  lane l holds the same slot of pixel column (l & 15), at the slot's tap offset
//   D:           lane l holds co = 16 t + 4 (l >> 4) + r (r = 0..3) of pixel (l & 15): four channels = one dword store
// A block computes NT 16-channel tiles (1, 2 or 4: Cout = 16 or 32 compute no channel that is thrown away) and keeps their
// weights in LDS; a wave walks work items of 4 rows x 16 columns.
#include "fdet_common.h"
#include "fdet_stem3_q8.h"

namespace {
using namespace fdet;

typedef int qx_v4i __attribute__((ext_vector_type(4)));
typedef float qx_v4f __attribute__((ext_vector_type(4)));

constexpr int QX_ROWS = 4;
constexpr int QX_MAX_C = 256;
constexpr int QX_MAX_HW = 4096;
constexpr size_t QX_LDS_MAX = 160 * 1024;

struct QxGeo {
  int N, Cin, Cout, H, W, HP, WP;
};

__host__ __device__ inline bool qx_c_ok(int C) { return C >= 16 && C <= QX_MAX_C && (C & 15) == 0; }

__host__ __device__ inline bool qx_shape_ok(int C, int H, int W) {
  return qx_c_ok(C) && H >= 1 && W >= 1 && H <= QX_MAX_HW && W <= QX_MAX_HW;
}

// bytes of N images, 0 when the shape has no layout or the tensor passes 2^31 - 1 bytes (32-bit offsets inside the kernels)
inline size_t qx_bytes(int N, int C, int H, int W) {
  if (N < 1 || !qx_shape_ok(C, H, W)) return 0;
  const unsigned long long b = (unsigned long long)N * (H + 2) * (W + 2) * C;
  return b < (1ull << 31) ? (size_t)b : 0;
}

// clamp(rintf(t), -127, 127): round half to even, -128 never produced (fdet_q8.hip's q8_round)
__device__ __forceinline__ int qx_round(float t) {
  return (int)fminf(fmaxf(rintf(t), -127.0f), 127.0f);
}

__device__ __forceinline__ int qx_pack4(int a, int b, int c, int d) {
  return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16) | (int)((unsigned)(d & 255) << 24);
}

__device__ __forceinline__ int qx_byte(int w, int r) {
  return (int)(signed char)((unsigned)w >> (8 * r));
}

// 3x3 conv (ntaps == 9) or 1x1 conv at the centre tap (ntaps == 1), Cin -> Cout, on Q8 tensors.  Block = 4 waves that share
// the 16 NT output channels blockIdx.y * 16 NT .. and keep their packed weights in LDS ([K/64][16 NT][64]); every wave walks
// work items of 4 rows x 16 columns of one image.  Lanes whose pixel lies outside the map read a clamped (valid) pixel and
// store nothing.  WIDE (Cin a multiple of 64, 3x3): the fragment walk of k_q8_conv3x3 -- 18 loads per 64-channel chunk, each
// used by up to three (row, tap) pairs.  Otherwise one load per (row, step) at the lane group's own tap.
template <int NT, bool POOL, bool WIDE>
__global__ __launch_bounds__(256) void k_q8x_conv(const signed char* __restrict__ x, const signed char* __restrict__ wpk,
                                                   const int* __restrict__ bias, const float* __restrict__ mul,
                                                   const signed char* __restrict__ skip, float skip_mul,
                                                   signed char* __restrict__ y, QxGeo g, int KS, int ntaps, int tiles_x, int row_groups,
                                                   int items, float slope) {
  extern __shared__ __attribute__((aligned(16))) unsigned char qx_lds[];
  constexpr int CB = 16 * NT;                              // output channels of the block
  const int co0 = blockIdx.y * CB;
  for (int u = threadIdx.x; u < KS * CB * 4; u += 256) {   // 16-byte units: CB * 4 per step, contiguous in wpk
    const int s = u / (CB * 4), r = u - s * (CB * 4);
    reinterpret_cast<qx_v4i*>(qx_lds)[u] = *reinterpret_cast<const qx_v4i*>(wpk + ((size_t)s * g.Cout + co0) * 64 + (size_t)r * 16);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  const int per_img = tiles_x * row_groups;
  const unsigned char* wl = qx_lds + lp * 64 + lk * 16;
  for (int item = blockIdx.x * 4 + wave; item < items; item += gridDim.x * 4) {
    const int n = item / per_img;
    const int rem = item - n * per_img;
    const int rg = rem / tiles_x;
    const int px = (rem - rg * tiles_x) * 16 + lp;
    const int pxc = min(px, g.W - 1);
    const int y0 = rg * QX_ROWS;
    qx_v4i acc[QX_ROWS][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const qx_v4i b = *reinterpret_cast<const qx_v4i*>(bias + co0 + 16 * t + 4 * lk);
#pragma unroll
      for (int j = 0; j < QX_ROWS; ++j) acc[j][t] = b;
    }
    // padded rows y0 .. y0 + 5 (row j, tap ky -> padded row y0 + j + ky) at columns px .. px + 2.  Padded rows past H + 1
    // belong to rows of the item below the map only: clamped, their results are never stored.
    const signed char* xr[QX_ROWS + 2];
#pragma unroll
    for (int r = 0; r < QX_ROWS + 2; ++r) xr[r] = x + ((size_t)(n * g.HP + min(y0 + r, g.H + 1)) * g.WP + pxc) * g.Cin;
    if (WIDE) {
      const int KC = g.Cin >> 6;
      for (int kc = 0; kc < KC; ++kc) {
        qx_v4i b[QX_ROWS + 2][3];
#pragma unroll
        for (int r = 0; r < QX_ROWS + 2; ++r)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) b[r][kx] = *reinterpret_cast<const qx_v4i*>(xr[r] + (size_t)kx * g.Cin + kc * 64 + lk * 16);
        __builtin_amdgcn_sched_barrier(0);                 // keep the 18 loads ahead of the MFMAs
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int ky = tap / 3, kx = tap - 3 * (tap / 3);
          qx_v4i a[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const qx_v4i*>(wl + (size_t)(tap * KC + kc) * (CB * 64) + t * 1024);
#pragma unroll
          for (int j = 0; j < QX_ROWS; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[j][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b[j + ky][kx], acc[j][t], 0, 0, 0);
        }
      }
    } else {
      const int K = ntaps * g.Cin;
      // the four pixel fragments of step s: the lane group's slot k = 64 s + 16 lk, its tap and first channel; a slot past K
      // has zero weights and reads the last real slot's bytes
      auto fetch = [&](int s, qx_v4i(&b)[QX_ROWS]) {
        const int k = min(64 * s + 16 * lk, K - 16);
        const int tap = ntaps == 9 ? k / g.Cin : 4;
        const int ci = ntaps == 9 ? k - tap * g.Cin : k;
        const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
        for (int j = 0; j < QX_ROWS; ++j) {
          // (a select over the six row pointers: ky is not known at compile time)
          const int r = j + ky;
          const signed char* p = r == 0 ? xr[0] : r == 1 ? xr[1] : r == 2 ? xr[2] : r == 3 ? xr[3] : r == 4 ? xr[4] : xr[5];
          b[j] = *reinterpret_cast<const qx_v4i*>(p + (size_t)kx * g.Cin + ci);
        }
      };
      qx_v4i b[QX_ROWS], bn[QX_ROWS];
      fetch(0, b);
#pragma unroll
      for (int j = 0; j < QX_ROWS; ++j) bn[j] = b[j];
      for (int s = 0; s < KS; ++s) {
        if (s + 1 < KS) fetch(s + 1, bn);                  // the next step's loads fly behind this step's MFMAs
        qx_v4i a[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const qx_v4i*>(wl + (size_t)s * (CB * 64) + t * 1024);
#pragma unroll
        for (int j = 0; j < QX_ROWS; ++j)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[j][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b[j], acc[j][t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < QX_ROWS; ++j) b[j] = bn[j];
      }
    }
    // epilogue of k_q8_conv3x3: multiplier, LeakyReLU, skip, requantise (, 2x2 floor max), four channels of one pixel per dword
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int co = co0 + 16 * t + 4 * lk;
      const qx_v4f m = *reinterpret_cast<const qx_v4f*>(mul + co);
      int q[QX_ROWS][4];
#pragma unroll
      for (int j = 0; j < QX_ROWS; ++j) {
        int sk = 0;
        if (skip != nullptr)
          sk = *reinterpret_cast<const int*>(skip + ((size_t)(n * g.HP + min(y0 + j, g.H - 1) + 1) * g.WP + pxc + 1) * g.Cout + co);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = (float)acc[j][t][r] * m[r];
          v = v >= 0.0f ? v : v * slope;
          if (skip != nullptr) v = v + (float)qx_byte(sk, r) * skip_mul;
          q[j][r] = qx_round(v);
        }
      }
      if (POOL) {
        // floor pool: a window needs both of its rows and both of its columns inside the map, so an odd last row or column
        // takes part in none
        const int Ho = g.H >> 1, Wo = g.W >> 1;
#pragma unroll
        for (int j = 0; j < QX_ROWS; j += 2) {
          int o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = max(q[j][r], q[j + 1][r]);
            o[r] = max(v, __shfl_xor(v, 1, 64));
          }
          if (!(lp & 1) && px + 1 < g.W && y0 + j + 1 < g.H)
            *reinterpret_cast<int*>(y + ((size_t)(n * (Ho + 2) + ((y0 + j) >> 1) + 1) * (Wo + 2) + (px >> 1) + 1) * g.Cout + co) =
                qx_pack4(o[0], o[1], o[2], o[3]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < QX_ROWS; ++j)
          if (px < g.W && y0 + j < g.H)
            *reinterpret_cast<int*>(y + ((size_t)(n * g.HP + y0 + j + 1) * g.WP + px + 1) * g.Cout + co) =
                qx_pack4(q[j][0], q[j][1], q[j][2], q[j][3]);
      }
    }
  }
}

inline bool qx_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int NT, bool POOL, bool WIDE>
int qx_launch(const signed char* x, const signed char* w, const int* bias, const float* mul, const signed char* skip, float skip_mul,
              signed char* y, const QxGeo& g, int KS, int ntaps, float slope, hipStream_t stream, const char* what) {
  const size_t lds = (size_t)KS * NT * 1024;
  if (lds > QX_LDS_MAX) return fail(FDET_EINVAL, "%s: %d -> %d channels do not fit the LDS", what, g.Cin, g.Cout);
  const int tiles_x = (g.W + 15) / 16, row_groups = (g.H + QX_ROWS - 1) / QX_ROWS;
  const long long items = (long long)g.N * tiles_x * row_groups;
  if (items >= (1ll << 31)) return fail(FDET_EINVAL, "%s: tensor too large", what);
  const int chunks = g.Cout / (16 * NT);
  const void* kern = (const void*)k_q8x_conv<NT, POOL, WIDE>;
  if (lds > 64 * 1024) {
    const int rc = set_lds_attr(kern, lds, what);
    if (rc != FDET_OK) return rc;
  }
  // blocks resident on a CU next to each other (what registers and this launch's LDS allow: asked once per kernel and step
  // count), shared between the output-channel chunks
  static int resident[QX_MAX_C * 9 / 64 + 1] = {};
  int per_cu = resident[KS];
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      per_cu = 1;
    }
    resident[KS] = per_cu;
  }
  long long gx = (items + 3) / 4;
  const long long cap = ((long long)num_cus() * per_cu + chunks - 1) / chunks;
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL((k_q8x_conv<NT, POOL, WIDE>), dim3((unsigned)gx, (unsigned)chunks), dim3(256), lds, stream, x, w, bias, mul, skip,
                     skip_mul, y, g, KS, ntaps, tiles_x, row_groups, (int)items, slope);
  return check_launch(what);
}

template <int NT>
int qx_dispatch(const signed char* x, const signed char* w, const int* bias, const float* mul, const signed char* skip, float skip_mul,
                signed char* y, const QxGeo& g, int KS, int ntaps, int pool, float slope, hipStream_t stream, const char* what) {
  const bool wide = ntaps == 9 && (g.Cin & 63) == 0;
  if (pool)
    return wide ? qx_launch<NT, true, true>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, stream, what)
                : qx_launch<NT, true, false>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, stream, what);
  return wide ? qx_launch<NT, false, true>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, stream, what)
              : qx_launch<NT, false, false>(x, w, bias, mul, skip, skip_mul, y, g, KS, ntaps, slope, stream, what);
}

int qx_conv(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, const int8_t* skip, float skip_mul, int8_t* y,
            int N, int Cin, int Cout, int H, int W, int ntaps, int pool, float slope, void* stream, const char* what) {
  const QxGeo g{N, Cin, Cout, H, W, H + 2, W + 2};
  const int KS = (ntaps * Cin + 63) / 64;
  const signed char* xs = reinterpret_cast<const signed char*>(x);
  const signed char* ws = reinterpret_cast<const signed char*>(wpk);
  const signed char* ss = reinterpret_cast<const signed char*>(skip);
  signed char* ys = reinterpret_cast<signed char*>(y);
  hipStream_t st = (hipStream_t)stream;
  if ((Cout & 63) == 0) return qx_dispatch<4>(xs, ws, bias, mul, ss, skip_mul, ys, g, KS, ntaps, pool, slope, st, what);
  if ((Cout & 31) == 0) return qx_dispatch<2>(xs, ws, bias, mul, ss, skip_mul, ys, g, KS, ntaps, pool, slope, st, what);
  return qx_dispatch<1>(xs, ws, bias, mul, ss, skip_mul, ys, g, KS, ntaps, pool, slope, st, what);
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
    const qx_v4i v = *reinterpret_cast<const qx_v4i*>(p + c);
#pragma unroll
    for (int o = 0; o < 5; ++o) {
      const qx_v4i wv = *reinterpret_cast<const qx_v4i*>(w + (size_t)o * C + c);
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[o] += qx_byte(v[d], b) * qx_byte(wv[d], b);
    }
  }
  const size_t plane = (size_t)H * W;
  float* dst = z + (size_t)n * 5 * plane + (size_t)yy * W + xx;
#pragma unroll
  for (int o = 0; o < 5; ++o) dst[o * plane] = (float)acc[o] * m[o];
}

// ---------------------------------------------------------------------------------------------------------------------
// The 3x3 / stride 2 / pad 1 stem on uint8 frames for F a multiple of 16: k_stem3_q8's arithmetic (fdet_stem_q8.hip: rows
// staged as x - 128, 128 * sum(w_q[co]) folded into the bias, one v_mfma_i32_16x16x32_i8 step over the 27 taps; geometry,
// staging, tap offsets and gather are the shared code of fdet_stem3_q8.h) with ONE 16-channel tile per workgroup: row m of the
// tile is channel co0 + m, so a lane ends up with the four channels co0 + 4 (l >> 4) + r of its pixel, one dword store.
// F % 64 == 0 goes to the existing entry.
__host__ __device__ inline bool sx_shape_ok(int Cin, int F, int H, int W) {
  return Cin == 3 && qx_c_ok(F) && H >= 2 && W >= 2 && H <= QX_MAX_HW && W <= QX_MAX_HW && !(H & 1) && !(W & 1);
}

inline size_t sx_out_bytes(int N, int Cin, int F, int H, int W) {
  if (N < 1 || !sx_shape_ok(Cin, F, H, W)) return 0;
  const unsigned long long b = (unsigned long long)N * (H / 2 + 2) * (W / 2 + 2) * F;
  return b < (1ull << 31) ? (size_t)b : 0;
}

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
  // the lane's four output channels co0 + 4 lk + r: multiplier and the constant bias + 128 * sum of the channel's weights
  // (the MFMA against a B of ones is that sum, in the accumulators' own layout; wrapping adds)
  const qx_v4f mv = *reinterpret_cast<const qx_v4f*>(a.mul + co0 + 4 * lk);
  const qx_v4i bv = *reinterpret_cast<const qx_v4i*>(a.bias + co0 + 4 * lk);
  unsigned cst[4];
  {
    const qx_v4i z = {0, 0, 0, 0};
    const qx_v4i ws = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa, 0x0101010101010101l, z, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) cst[r] = (unsigned)bv[r] + 128u * (unsigned)ws[r];
  }
  int off[8];
  s3::tap_offsets(off, lk, lp, j);
  __syncthreads();
  const int oy = oy0 + j;
  if (oy >= a.Ho) return;                                   // (after the only barrier)
  signed char* qrow = a.q + ((size_t)(n * (a.Ho + 2) + oy + 1) * (a.Wo + 2) + ox0 + 1) * a.F + co0 + 4 * lk;
  for (int tile = 0; tile < ntiles; ++tile) {
    const long b = s3::gather(rows, off, tile);
    const qx_v4i z = {0, 0, 0, 0};
    const qx_v4i acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(wa, b, z, 0, 0, 0);
    int qv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) qv[r] = qx_round((float)(int)((unsigned)acc[r] + cst[r]) * mv[r]);
    const int px = 16 * tile + lp;
    if (ox0 + px < a.Wo) *reinterpret_cast<int*>(qrow + (size_t)px * a.F) = qx_pack4(qv[0], qv[1], qv[2], qv[3]);
  }
}

}  // namespace

extern "C" int fdet_q8x_supported(int C, int H, int W) { return qx_shape_ok(C, H, W) ? 1 : 0; }

extern "C" size_t fdet_q8x_act_bytes(int N, int C, int H, int W) { return qx_bytes(N, C, H, W); }

extern "C" int fdet_q8x_conv3x3_ok(int N, int Cin, int Cout, int H, int W, int pool) {
  if (pool != 0 && pool != 1) return 0;
  if (qx_bytes(N, Cin, H, W) == 0 || qx_bytes(N, Cout, H, W) == 0) return 0;
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
               "1 <= H, W <= %d, at least 2 x 2 when pooled, tensors under 2^31 bytes)", N, Cin, Cout, H, W, pool, QX_MAX_C, QX_MAX_HW);
  FDET_REQUIRE(qx_aligned16(x) && qx_aligned16(wpk) && qx_aligned16(bias) && qx_aligned16(mul) && qx_aligned16(y) && qx_aligned16(skip),
               "q8x_conv3x3: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y && skip != y, "q8x_conv3x3: the output may not alias an input");
  return qx_conv(x, wpk, bias, mul, skip, skip_mul, y, N, Cin, Cout, H, W, 9, pool, slope, stream, "fdet_q8x_conv3x3");
}

extern "C" int fdet_q8x_pointwise_ok(int N, int Cin, int Cout, int H, int W) {
  return qx_bytes(N, Cin, H, W) > 0 && qx_bytes(N, Cout, H, W) > 0 ? 1 : 0;
}

extern "C" int fdet_q8x_pointwise(const int8_t* x, const int8_t* wpk, const int32_t* bias, const float* mul, int8_t* y, int N, int Cin,
                                  int Cout, int H, int W, void* stream) {
  FDET_REQUIRE(x && wpk && bias && mul && y, "q8x_pointwise: null argument");
  FDET_REQUIRE(fdet_q8x_pointwise_ok(N, Cin, Cout, H, W),
               "q8x_pointwise: unsupported shape N=%d Cin=%d Cout=%d H=%d W=%d (channels: multiples of 16 up to %d, 1 <= H, W <= %d, "
               "tensors under 2^31 bytes)", N, Cin, Cout, H, W, QX_MAX_C, QX_MAX_HW);
  FDET_REQUIRE(qx_aligned16(x) && qx_aligned16(wpk) && qx_aligned16(bias) && qx_aligned16(mul) && qx_aligned16(y),
               "q8x_pointwise: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y, "q8x_pointwise: the output may not alias the input");
  // identity activation: slope 1 (t * 1.0f is t)
  return qx_conv(x, wpk, bias, mul, nullptr, 0.0f, y, N, Cin, Cout, H, W, 1, 0, 1.0f, stream, "fdet_q8x_pointwise");
}

extern "C" int fdet_q8x_head_ok(int N, int C, int H, int W) {
  if (qx_bytes(N, C, H, W) == 0) return 0;
  return (unsigned long long)N * 5 * H * W * 4 < (1ull << 31) ? 1 : 0;
}

extern "C" int fdet_q8x_head_f32(const int8_t* x, const int8_t* w_q, const int32_t* b_q, const float* m, float* z, int N, int C, int H,
                                 int W, void* stream) {
  FDET_REQUIRE(x && w_q && b_q && m && z, "q8x_head_f32: null argument");
  FDET_REQUIRE(fdet_q8x_head_ok(N, C, H, W),
               "q8x_head_f32: unsupported shape N=%d C=%d H=%d W=%d (C a multiple of 16 up to %d, 1 <= H, W <= %d, tensors under 2^31 "
               "bytes)", N, C, H, W, QX_MAX_C, QX_MAX_HW);
  FDET_REQUIRE(qx_aligned16(x) && qx_aligned16(w_q) && qx_aligned16(b_q) && qx_aligned16(m) && qx_aligned16(z),
               "q8x_head_f32: every tensor must be 16-byte aligned");
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(k_q8x_head, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const signed char*>(x), reinterpret_cast<const signed char*>(w_q), b_q, m, z, N, C, H, W, (int)total);
  return check_launch("fdet_q8x_head_f32");
}

extern "C" int fdet_stem3_fwd_q8x_ok(int N, int Cin, int F, int H, int W) { return sx_out_bytes(N, Cin, F, H, W) > 0 ? 1 : 0; }

extern "C" int fdet_stem3_fwd_q8x_u8(const unsigned char* frames, const int8_t* w_q, const int32_t* b_q, const float* mul, int8_t* q,
                                     int N, int Cin, int F, int H, int W, void* stream) {
  FDET_REQUIRE(frames && w_q && b_q && mul && q, "stem3_fwd_q8x: null argument");
  FDET_REQUIRE(sx_out_bytes(N, Cin, F, H, W) > 0,
               "stem3_fwd_q8x: unsupported shape N=%d Cin=%d F=%d %dx%d (3 channels, F %% 16 == 0, F <= %d, even H and W in 2..%d, "
               "output under 2^31 bytes)", N, Cin, F, H, W, QX_MAX_C, QX_MAX_HW);
  FDET_REQUIRE(qx_aligned16(w_q) && qx_aligned16(b_q) && qx_aligned16(mul) && qx_aligned16(q),
               "stem3_fwd_q8x: w_q, b_q, mul and q must be 16-byte aligned");
  if ((F & 63) == 0) return fdet_stem3_fwd_q8_u8(frames, w_q, b_q, mul, q, N, Cin, F, H, W, stream);   // the same contract
  return s3::launch(k_stem3_q8x, F / 16, frames, w_q, b_q, mul, q, N, F, H, W, (hipStream_t)stream, "fdet_stem3_fwd_q8x_u8");
}
