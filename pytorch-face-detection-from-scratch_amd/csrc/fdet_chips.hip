// Face chips cut on the device and the sharpest chip of each track.  The rules, step by step, are stated
// with the declarations in include/fdet.h; tests/chips_cpu_ref.py restates them sequentially in numpy, and the two agree
// byte for byte: every value is an integer, so no order of addition changes a result.
//
//   fdet_chip_extract      one workgroup of 256 threads per chip.  The window is square and so is the chip, so ONE per-axis tap
//                          table (first window index and tap count per chip column, or first index and fraction when the chip
//                          is larger than the window) serves columns and rows; it goes into LDS once.  Two walks:
//     thread per pixel       S <= 8 * C (at most 10 taps per axis): thread p owns chip pixel p, p + 256, ..; neighbouring lanes
//                            own neighbouring chip columns and read source columns at most 8 pixels apart.
//     wave per pixel         S > 8 * C: a wave owns a chip pixel and its lanes run along the source columns of the pixel's tap
//                            rectangle (row-major where a row has fewer than 64 taps), then add up with an integer wave
//                            reduction.
//                          Each pixel's luma goes into an LDS plane of C * C bytes beside the store to the chip; after a barrier the
//                          squared Laplacian is summed over the plane (wave reduction, four partials) and thread 0 writes the
//                          fdet_chip_info.  All LDS is dynamic: 65536 + 2048 + 32 bytes at C = 256, which is why the entry point
//                          raises the kernel's dynamic-LDS limit on every call (it is a per-device setting).
//   fdet_chip_best_update  k_best_max: one thread per chip, one 64-bit atomicMax per candidate on scratch[seq * G + id - 1] with the
//                          key (1 << 60) | (sharp << 20) | (0xFFFFF - chip index): the largest sharp wins, then the lowest index.
//                          k_best_apply: one workgroup per chip; the one that finds its own key replaces the entry (strictly
//                          sharper, or empty) and copies the chip's bytes.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

constexpr int CT = 256;                      // threads per workgroup
constexpr int NW = CT / WAVE;
constexpr int WIDE = 8;                      // S > WIDE * C: a wave per chip pixel
static_assert(sizeof(fdet_chip_info) == 40 && sizeof(fdet_chip_best) == 40, "record layout");
static_assert(FDET_CHIP_MAX_CHIPS == (1 << 20), "the chip index takes the low 20 bits of a key");

__host__ __device__ inline size_t luma_bytes(int C) { return ((size_t)C * C + 15) & ~(size_t)15; }
inline size_t extract_lds(int C) { return luma_bytes(C) + (size_t)C * 8 + NW * 8; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// chip -> (image, row): the last image whose first chip is <= m (images without rows are stepped over)
__device__ __forceinline__ void find_chip(const int32_t* __restrict__ off, int n, int m, int& image, int& row) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  image = lo;
  row = m - off[lo];
}

// (num + den / 2) / den for num < 2^35 + den and a quotient <= 255: an fp32 estimate, then exact correction
__device__ __forceinline__ int round_div(unsigned long long sum, unsigned long long den) {
  const unsigned long long num = sum + (den >> 1);
  long long q = (long long)((float)num / (float)den);
  while (q > 0 && (unsigned long long)q * den > num) --q;
  while ((unsigned long long)(q + 1) * den <= num) ++q;
  return (int)q;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// rule 3 for chip column (or row) u.  area (S >= C): first window index and tap count; else i0 (may be -1) and f
__device__ __forceinline__ int2 axis_taps(int u, int S, int C) {
  if (S >= C) {
    const int a = (u * S) / C, b = ((u + 1) * S + C - 1) / C;       // u * S <= 256 * 8192
    return make_int2(a, b - a);
  }
  const int t = (2 * u + 1) * S - C;
  const int i0 = t >= 0 ? t / (2 * C) : -1;                        // t >= S - C > -2C: floor is -1
  return make_int2(i0, t - i0 * 2 * C);
}

// window index and weight of tap k of an axis entry e at chip column u
__device__ __forceinline__ void tap(int2 e, int u, int k, int S, int C, bool area, int& i, int& w) {
  if (area) {
    i = e.x + k;
    w = min((i + 1) * C, (u + 1) * S) - max(i * C, u * S);
  } else {
    i = clampi(e.x + k, 0, S - 1);
    w = k ? e.y : 2 * C - e.y;
  }
}

__global__ void __launch_bounds__(CT)
k_chip_extract(const uint8_t* __restrict__ bank, const fdet_aug_image* __restrict__ table, int n_images,
               const float* __restrict__ rows, const int32_t* __restrict__ counts, const int32_t* __restrict__ chip_offset, int K,
               int C, int margin256, int planar, uint8_t* __restrict__ chips, fdet_chip_info* __restrict__ info) {
  extern __shared__ __align__(16) unsigned char lds[];
  uint8_t* const luma = lds;
  int2* const tab = reinterpret_cast<int2*>(lds + luma_bytes(C));
  unsigned long long* const part = reinterpret_cast<unsigned long long*>(lds + luma_bytes(C) + (size_t)C * 8);

  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int CC = C * C;
  uint8_t* const chip = chips + (size_t)m * CC * 3;
  int image, row;
  find_chip(chip_offset, n_images, m, image, row);

  // ---- steps 1 + 2, the same in every thread ------------------------------------------------------------------------------
  bool ok = row >= 0 && row < K && row < counts[image];              // the host checked its copies; this keeps the reads inside
  int W = 0, H = 0, X1 = 0, Y1 = 0, X2 = 0, Y2 = 0, S = 0, wx0 = 0, wy0 = 0;
  const uint8_t* src = bank;
  if (ok) {
    const fdet_aug_image im = table[image];
    W = im.w; H = im.h;
    src = bank + im.offset;
    const float* d = rows + ((size_t)image * K + row) * 5;
    const float sc = d[0], x = d[1], y = d[2], w = d[3], h = d[4];
    const float big = 3.402823466e38f, lim = (float)FDET_TRACK_MAX_COORD;
    const float fx1 = rintf(x), fy1 = rintf(y), fx2 = rintf(x + w), fy2 = rintf(y + h);
    // every comparison is false for a NaN
    ok = W > 0 && H > 0 && fabsf(sc) <= big && fabsf(x) <= big && fabsf(y) <= big && fabsf(w) <= big && fabsf(h) <= big &&
         fabsf(fx1) <= lim && fabsf(fy1) <= lim && fabsf(fx2) <= lim && fabsf(fy2) <= lim;
    if (ok) {
      X1 = (int)fx1; Y1 = (int)fy1; X2 = (int)fx2; Y2 = (int)fy2;
      ok = X2 - X1 >= 1 && Y2 - Y1 >= 1 && X2 > 0 && X1 < W && Y2 > 0 && Y1 < H;
    }
    if (ok) {
      const int side = max(X2 - X1, Y2 - Y1);
      S = side + 2 * ((side * margin256 + 128) >> 8);               // side <= 32768, margin256 <= 256
      ok = S <= FDET_CHIP_MAX_SIDE;
      wx0 = (X1 + X2 - S) >> 1;
      wy0 = (Y1 + Y2 - S) >> 1;
    }
  }
  if (!ok) {                                                         // block-uniform
    for (int i = tid; i < CC * 3; i += CT) chip[i] = 0;
    if (tid == 0) {
      fdet_chip_info z;
      z.image = image; z.row = row; z.wx0 = 0; z.wy0 = 0; z.S = 0; z.inside256 = 0; z.flags = 0; z.reserved = 0; z.sharp = 0;
      info[m] = z;
    }
    return;
  }

  // ---- step 3: one tap table for both axes ---------------------------------------------------------------------------------
  const bool area = S >= C;
  for (int u = tid; u < C; u += CT) tab[u] = axis_taps(u, S, C);
  __syncthreads();

  // ---- step 4 -----------------------------------------------------------------------------------------------------------------
  const long long D = area ? S : 2 * C;
  const unsigned long long DD = (unsigned long long)(D * D);
  const int64_t rb = (int64_t)W * 3;
  auto store = [&](int v, int u, const unsigned long long (&sum)[3]) {
    const int r = round_div(sum[0], DD), g = round_div(sum[1], DD), b = round_div(sum[2], DD);
    const int p = v * C + u;
    if (planar) {
      chip[p] = (uint8_t)r; chip[CC + p] = (uint8_t)g; chip[2 * CC + p] = (uint8_t)b;
    } else {
      chip[p * 3] = (uint8_t)r; chip[p * 3 + 1] = (uint8_t)g; chip[p * 3 + 2] = (uint8_t)b;
    }
    luma[p] = (uint8_t)((77 * r + 150 * g + 29 * b + 128) >> 8);
  };
  if (S <= WIDE * C) {                                               // block-uniform
    for (int p = tid; p < CC; p += CT) {
      const int v = p / C, u = p - v * C;
      const int2 ey = tab[v], ex = tab[u];
      const int ny = area ? ey.y : 2, nx = area ? ex.y : 2;
      unsigned long long sum[3] = {0ull, 0ull, 0ull};
      for (int ky = 0; ky < ny; ++ky) {
        int iy, wy;
        tap(ey, v, ky, S, C, area, iy, wy);
        const uint8_t* line = src + (int64_t)clampi(wy0 + iy, 0, H - 1) * rb;
        unsigned r0 = 0, r1 = 0, r2 = 0;                             // <= D * 255 < 2^22
        for (int kx = 0; kx < nx; ++kx) {
          int ix, wx;
          tap(ex, u, kx, S, C, area, ix, wx);
          const uint8_t* q = line + (int64_t)clampi(wx0 + ix, 0, W - 1) * 3;
          r0 += (unsigned)wx * q[0]; r1 += (unsigned)wx * q[1]; r2 += (unsigned)wx * q[2];
        }
        sum[0] += (unsigned long long)wy * r0; sum[1] += (unsigned long long)wy * r1; sum[2] += (unsigned long long)wy * r2;
      }
      store(v, u, sum);
    }
  } else {                                                           // area averaging of many taps: a wave per chip pixel
    for (int p = wid; p < CC; p += NW) {
      const int v = p / C, u = p - v * C;
      const int2 ey = tab[v], ex = tab[u];
      const int ny = ey.y, nx = ex.y;
      unsigned long long sum[3] = {0ull, 0ull, 0ull};
      if (nx >= WAVE) {
        for (int ky = 0; ky < ny; ++ky) {
          int iy, wy;
          tap(ey, v, ky, S, C, true, iy, wy);
          const uint8_t* line = src + (int64_t)clampi(wy0 + iy, 0, H - 1) * rb;
          unsigned r0 = 0, r1 = 0, r2 = 0;
          for (int kx = lane; kx < nx; kx += WAVE) {
            int ix, wx;
            tap(ex, u, kx, S, C, true, ix, wx);
            const uint8_t* q = line + (int64_t)clampi(wx0 + ix, 0, W - 1) * 3;
            r0 += (unsigned)wx * q[0]; r1 += (unsigned)wx * q[1]; r2 += (unsigned)wx * q[2];
          }
          sum[0] += (unsigned long long)wy * r0; sum[1] += (unsigned long long)wy * r1; sum[2] += (unsigned long long)wy * r2;
        }
      } else {
        for (int i = lane; i < nx * ny; i += WAVE) {                 // nx * ny < 64 * 1026
          const int ky = i / nx, kx = i - ky * nx;
          int iy, wy, ix, wx;
          tap(ey, v, ky, S, C, true, iy, wy);
          tap(ex, u, kx, S, C, true, ix, wx);
          const uint8_t* q = src + (int64_t)clampi(wy0 + iy, 0, H - 1) * rb + (int64_t)clampi(wx0 + ix, 0, W - 1) * 3;
          const unsigned long long ww = (unsigned long long)((unsigned)wy * (unsigned)wx);     // <= D * D <= 2^26
          sum[0] += ww * q[0]; sum[1] += ww * q[1]; sum[2] += ww * q[2];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) sum[c] = wave_sum_u64(sum[c]);
      if (lane == 0) store(v, u, sum);
    }
  }
  __syncthreads();

  // ---- step 6: sharpness of the chip as written ---------------------------------------------------------------------------
  unsigned long long sh = 0ull;
  const int CI = C - 2;
  for (int p = tid; p < CI * CI; p += CT) {
    const int v = 1 + p / CI, u = 1 + p % CI;
    const int c = v * C + u;
    const int lap = 4 * (int)luma[c] - (int)luma[c - C] - (int)luma[c + C] - (int)luma[c - 1] - (int)luma[c + 1];
    sh += (unsigned long long)(lap * lap);
  }
  sh = wave_sum_u64(sh);
  if (lane == 0) part[wid] = sh;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0ull;
#pragma unroll
    for (int w = 0; w < NW; ++w) total += part[w];
    // ---- step 5 ---------------------------------------------------------------------------------------------------------------
    const long long ix = max(0, min(wx0 + S, W) - max(wx0, 0)), iy = max(0, min(wy0 + S, H) - max(wy0, 0));
    fdet_chip_info o;
    o.image = image; o.row = row; o.wx0 = wx0; o.wy0 = wy0; o.S = S;
    o.inside256 = (int32_t)((ix * iy * 256) / ((long long)S * S));
    o.flags = 1; o.reserved = 0;
    o.sharp = (int64_t)total;
    info[m] = o;
  }
}

// ---- the best-shot gallery ----------------------------------------------------------------------------------------------------
struct Cand {
  int entry;                 // seq * G + id - 1; -1: not a candidate, or its id is beyond G
  int seq, frame;
  unsigned long long key;
};

// rule 1 for chip i; `over` = a candidate whose id is beyond G
__device__ __forceinline__ Cand candidate(const fdet_chip_info& f, int i, const int32_t* __restrict__ ids, int K,
                                          const int32_t* __restrict__ seq_offset, int n_seq, const int32_t* __restrict__ frame_base,
                                          int G, int min_side, int min_inside256, bool& over) {
  Cand c{-1, 0, 0, 0ull};
  over = false;
  const int T = seq_offset[n_seq];
  if (!(f.flags & 1) || f.image < 0 || f.image >= T || f.row < 0 || f.row >= K) return c;      // the reads below stay inside
  if (f.S < min_side || f.inside256 < min_inside256 || f.sharp < 0 || f.sharp >= (1ll << 40)) return c;
  const int id = ids[(size_t)f.image * K + f.row];
  if (id < 1) return c;
  if (id > G) { over = true; return c; }
  int lo = 0, hi = n_seq - 1;                                        // the last sequence whose first frame is <= image
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seq_offset[mid] <= f.image) lo = mid; else hi = mid - 1;
  }
  c.seq = lo;
  c.frame = frame_base[lo] + f.image - seq_offset[lo];
  c.entry = lo * G + id - 1;
  c.key = (1ull << 60) | ((unsigned long long)f.sharp << 20) | (unsigned long long)(0xFFFFF - i);
  return c;
}

__global__ void __launch_bounds__(CT)
k_best_max(const fdet_chip_info* __restrict__ info, int M, const int32_t* __restrict__ ids, int K,
           const int32_t* __restrict__ seq_offset, int n_seq, const int32_t* __restrict__ frame_base, int G, int min_side,
           int min_inside256, fdet_chip_best* __restrict__ gallery, unsigned long long* __restrict__ scratch,
           unsigned long long* __restrict__ overflow) {
  const int i = blockIdx.x * CT + threadIdx.x;
  if (i >= M) return;
  bool over;
  const Cand c = candidate(info[i], i, ids, K, seq_offset, n_seq, frame_base, G, min_side, min_inside256, over);
  if (over) atomicAdd(overflow, 1ull);
  if (c.entry < 0) return;
  atomicMax(&scratch[c.entry], c.key);
  atomicAdd(&gallery[c.entry].seen, 1);                              // rule 4; no other launch touches this word
}

__global__ void __launch_bounds__(CT)
k_best_apply(const uint8_t* __restrict__ chips, const fdet_chip_info* __restrict__ info, int C, const int32_t* __restrict__ ids, int K,
             const int32_t* __restrict__ seq_offset, int n_seq, const int32_t* __restrict__ frame_base, int G, int min_side,
             int min_inside256, fdet_chip_best* __restrict__ gallery, uint8_t* __restrict__ gallery_chips,
             const unsigned long long* __restrict__ scratch) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const fdet_chip_info f = info[i];
  bool over;
  const Cand c = candidate(f, i, ids, K, seq_offset, n_seq, frame_base, G, min_side, min_inside256, over);
  if (c.entry < 0 || scratch[c.entry] != c.key) return;              // block-uniform: one winner per entry
  fdet_chip_best* const e = gallery + c.entry;
  const bool replace = e->id == 0 || f.sharp > e->sharp;
  __syncthreads();                                                   // every thread has read the entry
  if (!replace) return;
  const size_t bytes = (size_t)C * C * 3;
  const uint8_t* s = chips + (size_t)i * bytes;
  uint8_t* d = gallery_chips + (size_t)c.entry * bytes;
  if (((uintptr_t)s | (uintptr_t)d | bytes) % 4 == 0) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
    for (size_t k = tid; k < bytes / 4; k += CT) d4[k] = s4[k];
  } else {
    for (size_t k = tid; k < bytes; k += CT) d[k] = s[k];
  }
  if (tid == 0) {
    e->id = c.entry - c.seq * G + 1;
    e->frame = c.frame;
    e->image_wx0 = f.wx0; e->image_wy0 = f.wy0; e->S = f.S; e->inside256 = f.inside256;
    e->reserved = 0;
    e->sharp = f.sharp;
  }
}

}  // namespace

extern "C" int fdet_chip_extract(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                                 const float* rows, const int32_t* counts, const int32_t* h_counts, const int32_t* chip_offset,
                                 const int32_t* h_chip_offset, int K, int C, int margin256, int planar, uint8_t* chips,
                                 fdet_chip_info* info, void* stream) {
  const char* what = "fdet_chip_extract";
  FDET_REQUIRE(C >= FDET_CHIP_MIN_SIZE && C <= FDET_CHIP_MAX_SIZE, "%s: C=%d outside %d..%d", what, C, FDET_CHIP_MIN_SIZE,
               FDET_CHIP_MAX_SIZE);
  FDET_REQUIRE(margin256 >= 0 && margin256 <= 256, "%s: margin256=%d outside 0..256", what, margin256);
  FDET_REQUIRE(planar == 0 || planar == 1, "%s: planar=%d must be 0 or 1", what, planar);
  FDET_REQUIRE(n_images >= 1 && K >= 0, "%s: bad sizes n_images=%d K=%d", what, n_images, K);
  FDET_REQUIRE(bank && table && h_table && counts && h_counts && chip_offset && h_chip_offset && (K == 0 || rows),
               "%s: null pointer (rows may be NULL only with K = 0)", what);
  FDET_REQUIRE(h_chip_offset[0] == 0, "%s: chip_offset[0]=%d must be 0", what, h_chip_offset[0]);
  int64_t total = 0;
  for (int i = 0; i < n_images; ++i) {
    const fdet_aug_image& S = h_table[i];
    FDET_REQUIRE(S.offset >= 0 && S.h > 0 && S.w > 0 && (int64_t)S.h * S.w < 0x7fffffffLL, "%s: bad table row %d (offset %lld, %dx%d)",
                 what, i, (long long)S.offset, S.h, S.w);
    FDET_REQUIRE(h_counts[i] >= 0 && h_counts[i] <= K, "%s: counts[%d]=%d outside 0..K=%d", what, i, h_counts[i], K);
    total += h_counts[i];
    FDET_REQUIRE(total <= FDET_CHIP_MAX_CHIPS, "%s: more than %d chips in one call", what, FDET_CHIP_MAX_CHIPS);
    FDET_REQUIRE(h_chip_offset[i + 1] == (int32_t)total, "%s: chip_offset[%d]=%d is not the prefix sum of counts (%lld)", what, i + 1,
                 h_chip_offset[i + 1], (long long)total);
  }
  if (total == 0) return FDET_OK;
  FDET_REQUIRE(chips && info, "%s: null pointer", what);
  const size_t lds = extract_lds(C);
  if (int rc = set_lds_attr((const void*)k_chip_extract, lds, what)) return rc;      // per device: set on every call
  hipLaunchKernelGGL(k_chip_extract, dim3((unsigned)total), dim3(CT), lds, (hipStream_t)stream, bank, table, n_images, rows, counts,
                     chip_offset, K, C, margin256, planar, chips, info);
  return check_launch(what);
}

extern "C" size_t fdet_chip_gallery_bytes(int n_seq, int G) {
  return (n_seq < 1 || G < 1) ? 0 : (size_t)n_seq * (size_t)G * sizeof(fdet_chip_best);
}

extern "C" int fdet_chip_best_update(const uint8_t* chips, const fdet_chip_info* info, int M, int C, const int32_t* ids, int K,
                                     const int32_t* seq_offset, const int32_t* h_seq_offset, int n_seq, const int32_t* frame_base,
                                     int G, int min_side, int min_inside256, void* gallery, uint8_t* gallery_chips,
                                     uint64_t* scratch, uint64_t* overflow, void* stream) {
  const char* what = "fdet_chip_best_update";
  FDET_REQUIRE(G >= 1 && n_seq >= 1 && K >= 0, "%s: bad sizes G=%d n_seq=%d K=%d", what, G, n_seq, K);
  FDET_REQUIRE((int64_t)n_seq * G <= 0x7fffffffLL, "%s: n_seq * G = %lld entries", what, (long long)n_seq * G);
  FDET_REQUIRE(M >= 0 && M <= FDET_CHIP_MAX_CHIPS, "%s: M=%d outside 0..%d", what, M, FDET_CHIP_MAX_CHIPS);
  FDET_REQUIRE(C >= FDET_CHIP_MIN_SIZE && C <= FDET_CHIP_MAX_SIZE, "%s: C=%d outside %d..%d", what, C, FDET_CHIP_MIN_SIZE,
               FDET_CHIP_MAX_SIZE);
  FDET_REQUIRE(min_side >= 0, "%s: min_side=%d must be >= 0", what, min_side);
  FDET_REQUIRE(min_inside256 >= 0 && min_inside256 <= 256, "%s: min_inside256=%d outside 0..256", what, min_inside256);
  FDET_REQUIRE(seq_offset && h_seq_offset && frame_base && gallery && gallery_chips && scratch && overflow, "%s: null pointer", what);
  FDET_REQUIRE(M == 0 || (chips && info && ids), "%s: null pointer", what);
  FDET_REQUIRE(h_seq_offset[0] == 0, "%s: seq_offset[0]=%d must be 0", what, h_seq_offset[0]);
  for (int s = 0; s < n_seq; ++s)
    FDET_REQUIRE(h_seq_offset[s + 1] >= h_seq_offset[s], "%s: seq_offset[%d]=%d < seq_offset[%d]=%d", what, s + 1, h_seq_offset[s + 1],
                 s, h_seq_offset[s]);
  if (M == 0) return FDET_OK;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)n_seq * G * sizeof(uint64_t), st);
  if (e != hipSuccess) return fail(FDET_ELAUNCH, "%s: clearing scratch: %s", what, hipGetErrorString(e));
  hipLaunchKernelGGL(k_best_max, dim3((unsigned)((M + CT - 1) / CT)), dim3(CT), 0, st, info, M, ids, K, seq_offset, n_seq, frame_base, G,
                     min_side, min_inside256, reinterpret_cast<fdet_chip_best*>(gallery),
                     reinterpret_cast<unsigned long long*>(scratch), reinterpret_cast<unsigned long long*>(overflow));
  hipLaunchKernelGGL(k_best_apply, dim3((unsigned)M), dim3(CT), 0, st, chips, info, C, ids, K, seq_offset, n_seq, frame_base, G, min_side,
                     min_inside256, reinterpret_cast<fdet_chip_best*>(gallery), gallery_chips,
                     reinterpret_cast<const unsigned long long*>(scratch));
  return check_launch(what);
}
