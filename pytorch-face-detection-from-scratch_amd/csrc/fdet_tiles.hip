// Tiled full-resolution detection: the two ends around the batched network.
//
//   fdet_tile_gather  axis-aligned windows of the device image bank (HWC uint8 RGB) -> model-sized planar uint8 frames
//                     [T,3,Ho,Wo], the input forward_frames hands to the stem unchanged.  The sample is the one
//                     fdet_aug_warp takes when only a crop is set (fp64 coordinates, fp32 bilinear weights, taps clamped
//                     to the window, one rint + clamp), operation for operation, so the two kernels agree byte for byte.
//                     Unlike the warp, which must serve rotation and issues twelve single-byte global loads per pixel, a
//                     block stages the source rectangle its 128 x 8 output tile taps into LDS with 16-byte global loads
//                     (each source row is fetched once for all the output rows that tap it) and samples from LDS.
//   fdet_tile_merge   every window's detections mapped back to source pixels, an optional cut-face rule at interior window
//                     sides, and ONE greedy NMS per source image over the union (the semantics of fdet_nms), one workgroup
//                     per image, candidates in LDS, no host synchronisation.
//
// tests/tiles_cpu_ref.py restates both in numpy.  Built with -ffp-contract=off like every file here.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

// ------------------------------------------------------------------------------------------------------------------
// gather: block (32, 8), one thread per 4 consecutive output pixels of a row, all three channels
// ------------------------------------------------------------------------------------------------------------------
constexpr int GT_PX = 4, GT_BX = 32, GT_BY = 8;
constexpr int GT_W = GT_BX * GT_PX, GT_H = GT_BY;
constexpr int GT_LDS = 32 * 1024;        // source rectangle of one output tile; larger ones (downscales beyond ~3x) sample
                                         // global memory directly, as the warp does

// the four output pixels of one thread: base[o0 + x * 3 + c] / base[o1 + x * 3 + c] is channel c of source column x in the
// upper / lower tap row (base: the LDS stage or the image in global memory)
template <typename Off>
__device__ __forceinline__ void gather_px(const uint8_t* base, Off o0, Off o1, float fy, const fdet_tile& Tl, double rw, int ox0,
                                          int Wo, uint8_t (&res)[3][GT_PX]) {
  const int xlo = Tl.x0, xhi = Tl.x0 + Tl.w - 1;
#pragma unroll
  for (int i = 0; i < GT_PX; ++i) {
    const int ox = min(ox0 + i, Wo - 1);            // tail lanes recompute the last pixel; only valid pixels are stored
    const double u = (double)ox;
    const double sx = (u + 0.5) * rw + (double)Tl.x0 - 0.5;
    const double fx0 = floor(sx);
    const float fx = (float)(sx - fx0);
    const int ix = (int)fx0;
    const int x0 = min(max(ix, xlo), xhi), x1 = min(max(ix + 1, xlo), xhi);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = (float)base[o0 + x0 * 3 + c], v01 = (float)base[o0 + x1 * 3 + c];
      const float v10 = (float)base[o1 + x0 * 3 + c], v11 = (float)base[o1 + x1 * 3 + c];
      const float top = (1.f - fx) * v00 + fx * v01;
      const float bot = (1.f - fx) * v10 + fx * v11;
      const float val = (1.f - fy) * top + fy * bot;
      res[c][i] = (uint8_t)fminf(fmaxf(rintf(val), 0.f), 255.f);
    }
  }
}

__global__ void __launch_bounds__(256)
k_tile_gather(const uint8_t* __restrict__ bank, int64_t bank_bytes, const fdet_aug_image* __restrict__ table,
              const fdet_tile* __restrict__ tiles, int Ho, int Wo, uint8_t* __restrict__ frames) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[GT_LDS];
  const int b = blockIdx.z;
  const fdet_tile Tl = tiles[b];
  const fdet_aug_image img = table[Tl.image];
  const uint8_t* src = bank + img.offset;
  const int tx0 = blockIdx.x * GT_W, ty0 = blockIdx.y * GT_H;
  const int tid = threadIdx.y * GT_BX + threadIdx.x;
  const int oy = ty0 + threadIdx.y, ox0 = tx0 + threadIdx.x * GT_PX;
  // fp64 coordinates, the warp's own expressions (fdet_augment.hip:k_aug_warp); they are monotone in the output index,
  // so the taps of the tile lie between those of its first and last pixel
  const double rw = (double)Tl.w / (double)Wo, rh = (double)Tl.h / (double)Ho;
  const int xlo = Tl.x0, xhi = Tl.x0 + Tl.w - 1, ylo = Tl.y0, yhi = Tl.y0 + Tl.h - 1;
  const int oxl = min(tx0 + GT_W, Wo) - 1, oyl = min(ty0 + GT_H, Ho) - 1;
  const double sxa = ((double)tx0 + 0.5) * rw + (double)Tl.x0 - 0.5, sxb = ((double)oxl + 0.5) * rw + (double)Tl.x0 - 0.5;
  const double sya = ((double)ty0 + 0.5) * rh + (double)Tl.y0 - 0.5, syb = ((double)oyl + 0.5) * rh + (double)Tl.y0 - 0.5;
  const int fxlo = min(max((int)floor(sxa), xlo), xhi), fxhi = min(max((int)floor(sxb) + 1, xlo), xhi);
  const int fylo = min(max((int)floor(sya), ylo), yhi), fyhi = min(max((int)floor(syb) + 1, ylo), yhi);
  const int ncols = fxhi - fxlo + 1, nrows = fyhi - fylo + 1;
  // a staged row keeps its global 16-byte phase, so every global load and every LDS store is a whole aligned 16 bytes
  const int pitch = (ncols * 3 + 15 + 15) & ~15;
  const bool staged = (int64_t)pitch * nrows <= GT_LDS;       // block-uniform
  const int64_t row_bytes = (int64_t)img.w * 3;
  if (staged) {
    const int vpr = pitch >> 4;
    const int phase = (int)((uintptr_t)bank & 15);
    for (int idx = tid; idx < nrows * vpr; idx += 256) {
      const int r = idx / vpr, v = idx - r * vpr;
      const int64_t g = img.offset + (int64_t)(fylo + r) * row_bytes + (int64_t)fxlo * 3;     // byte offset in the bank
      const int m = (int)((g + phase) & 15);
      if (v * 16 >= m + ncols * 3) continue;
      const int64_t a = g - m + (int64_t)v * 16;
      uint4 q;
      if (a >= 0 && a + 16 <= bank_bytes) {
        q = *reinterpret_cast<const uint4*>(bank + a);
      } else {                                                // the 16 bytes straddle an end of the bank: byte loads
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < 16; ++j)
          if (a + j >= 0 && a + j < bank_bytes) w[j >> 2] |= (uint32_t)bank[a + j] << (8 * (j & 3));
        q = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *reinterpret_cast<uint4*>(stage + r * pitch + v * 16) = q;
    }
    __syncthreads();
  }
  if (oy >= Ho || ox0 >= Wo) return;
  const double sy = ((double)oy + 0.5) * rh + (double)Tl.y0 - 0.5;
  const double fy0 = floor(sy);
  const float fy = (float)(sy - fy0);
  const int iy = (int)fy0;
  const int y0 = min(max(iy, ylo), yhi), y1 = min(max(iy + 1, ylo), yhi);
  uint8_t res[3][GT_PX];
  if (staged) {
    const int phase = (int)((uintptr_t)bank & 15);
    const int m0 = (int)((img.offset + (int64_t)y0 * row_bytes + (int64_t)fxlo * 3 + phase) & 15);
    const int m1 = (int)((img.offset + (int64_t)y1 * row_bytes + (int64_t)fxlo * 3 + phase) & 15);
    gather_px(stage, (y0 - fylo) * pitch + m0 - fxlo * 3, (y1 - fylo) * pitch + m1 - fxlo * 3, fy, Tl, rw, ox0, Wo, res);
  } else {
    gather_px(src, (int64_t)y0 * row_bytes, (int64_t)y1 * row_bytes, fy, Tl, rw, ox0, Wo, res);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint8_t* row = frames + (((int64_t)b * 3 + c) * Ho + oy) * Wo;
    if ((Wo % GT_PX) == 0) {                         // ox0 + 3 < Wo and 4-byte aligned
      const uint32_t w = (uint32_t)res[c][0] | ((uint32_t)res[c][1] << 8) | ((uint32_t)res[c][2] << 16) | ((uint32_t)res[c][3] << 24);
      *reinterpret_cast<uint32_t*>(row + ox0) = w;
    } else {
#pragma unroll
      for (int i = 0; i < GT_PX; ++i)
        if (ox0 + i < Wo) row[ox0 + i] = res[c][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// merge: one workgroup per source image; 33 bytes of LDS per candidate, as fdet_nms
// ------------------------------------------------------------------------------------------------------------------
constexpr int MERGE_CAP = 4864;

struct MergeLds {
  float* x1; float* y1; float* x2; float* y2; float* key;
  int* src;              // candidate -> row of `rows` (tile * K + r)
  int* order;            // sorted position -> candidate
  int* keep;             // visiting order -> candidate
  unsigned char* dead;   // by sorted position
  int* ctl;              // [0] running count, [1..4] per-wave counts, [5] kept
};

__host__ __device__ inline size_t merge_lds_bytes(int cap) { return (size_t)cap * 32 + (size_t)((cap + 15) / 16) * 16 + 64; }

__device__ __forceinline__ MergeLds merge_carve(char* smem, int cap) {
  MergeLds L;
  float* f = reinterpret_cast<float*>(smem);
  L.x1 = f; L.y1 = f + cap; L.x2 = f + 2 * cap; L.y2 = f + 3 * cap; L.key = f + 4 * cap;
  L.src = reinterpret_cast<int*>(f + 5 * cap);
  L.order = reinterpret_cast<int*>(f + 6 * cap);
  L.keep = reinterpret_cast<int*>(f + 7 * cap);
  L.dead = reinterpret_cast<unsigned char*>(f + 8 * cap);
  L.ctl = reinterpret_cast<int*>(smem + merge_lds_bytes(cap) - 64);
  return L;
}

// one detection row in frame pixels -> source pixels: fp32, separate multiply and add, then half-to-even
__device__ __forceinline__ void to_source(const float* d, const fdet_tile& Tl, float kx, float ky, float& x, float& y, float& w,
                                          float& h) {
  x = rintf((float)Tl.x0 + d[1] * kx);
  y = rintf((float)Tl.y0 + d[2] * ky);
  w = rintf(d[3] * kx);
  h = rintf(d[4] * ky);
}

__global__ void __launch_bounds__(256)
k_tile_merge(const float* __restrict__ rows, const int32_t* __restrict__ counts, const fdet_tile* __restrict__ tiles,
             const int32_t* __restrict__ tile_offset, int T, int K, int Ho, int Wo, const fdet_aug_image* __restrict__ table,
             float margin, double thr, int cap, int Kout, float* __restrict__ out, int32_t* __restrict__ out_counts,
             unsigned long long* __restrict__ rejected) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MergeLds L = merge_carve(smem, cap);
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int t0 = tile_offset[n], t1 = tile_offset[n + 1];
  const fdet_aug_image img = table[n];
  bool bad = t0 < 0 || t1 < t0 || t1 > T;
  if (tid == 0) L.ctl[0] = 0;
  __syncthreads();
  // 1 + 2: ordered compaction of the tiles' rows (tile order, then row) that pass the cut-face rule
  for (int t = t0; t < t1 && !bad; ++t) {
    const fdet_tile Tl = tiles[t];
    const int c = counts[t];
    if (c < 0 || c > K || Tl.image != n) { bad = true; break; }        // uniform: every thread read the same words
    const float kx = (float)Tl.w / (float)Wo, ky = (float)Tl.h / (float)Ho;
    const bool cl = Tl.x0 > 0, cr = Tl.x0 + Tl.w < img.w, ct = Tl.y0 > 0, cb = Tl.y0 + Tl.h < img.h;   // interior sides
    for (int r0 = 0; r0 < c; r0 += 256) {
      const int r = r0 + tid;
      const float* d = rows + ((size_t)t * K + min(r, c - 1)) * 5;
      bool hit = r < c;
      if (hit && margin > 0.f) {
        const float bx2 = d[1] + d[3], by2 = d[2] + d[4];
        if ((cl && d[1] < margin) || (cr && bx2 > (float)Wo - margin) || (ct && d[2] < margin) || (cb && by2 > (float)Ho - margin))
          hit = false;
      }
      const unsigned long long bal = __ballot(hit);
      const int before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) L.ctl[1 + wid] = __popcll(bal);
      __syncthreads();
      int base = L.ctl[0];
      for (int w = 0; w < wid; ++w) base += L.ctl[1 + w];
      const int k = base + before;
      if (hit && k < cap) {
        float x, y, w, h;
        to_source(d, Tl, kx, ky, x, y, w, h);
        L.key[k] = d[0] != d[0] ? -INFINITY : d[0];      // a NaN score is ordered as -inf (visited last), as fdet_eval_match does
        L.x1[k] = x; L.y1[k] = y; L.x2[k] = x + w; L.y2[k] = y + h;
        L.src[k] = t * K + r;
      }
      __syncthreads();
      if (tid == 0) L.ctl[0] += L.ctl[1] + L.ctl[2] + L.ctl[3] + L.ctl[4];
      __syncthreads();
    }
  }
  const int C = L.ctl[0];
  bad = bad || C > MERGE_CAP || C > cap;
  int nk = 0;
  if (!bad) {
    // 3: greedy NMS (torchvision 0.11.2 nms_kernel.cpp as restated by fdet_nms): stable descending rank, fp32 overlap
    for (int i = tid; i < C; i += 256) {
      const float si = L.key[i];
      int rk = 0;
      for (int j = 0; j < C; ++j) { const float sj = L.key[j]; rk += (sj > si) || (sj == si && j < i); }
      L.order[rk] = i;
    }
    for (int i = tid; i < C; i += 256) L.dead[i] = 0;
    if (tid == 0) L.ctl[5] = 0;
    __syncthreads();
    for (int a = 0; a < C; ++a) {
      if (L.dead[a]) continue;                       // uniform: written before the last barrier
      const int i = L.order[a];
      if (tid == 0) { L.keep[L.ctl[5]] = i; L.ctl[5] += 1; }
      const float ix1 = L.x1[i], iy1 = L.y1[i], ix2 = L.x2[i], iy2 = L.y2[i];
      const float ia = (ix2 - ix1) * (iy2 - iy1);
      for (int bq = a + 1 + tid; bq < C; bq += 256) {
        if (L.dead[bq]) continue;
        const int j = L.order[bq];
        const float jx1 = L.x1[j], jy1 = L.y1[j], jx2 = L.x2[j], jy2 = L.y2[j];
        const float ja = (jx2 - jx1) * (jy2 - jy1);
        const float w = fmaxf(0.f, fminf(ix2, jx2) - fmaxf(ix1, jx1));
        const float h = fmaxf(0.f, fminf(iy2, jy2) - fmaxf(iy1, jy1));
        const float inter = w * h;
        const float ovr = inter / (ia + ja - inter);                 // 0/0 = NaN -> not suppressed
        if ((double)ovr > thr) L.dead[bq] = 1;
      }
      __syncthreads();
    }
    __syncthreads();
    nk = L.ctl[5];
    bad = nk > Kout;
  }
  // 4: an image over a limit is rejected as a whole
  if (bad) nk = 0;
  float* o = out + (size_t)n * Kout * 5;
  for (int k = tid; k < Kout; k += 256) {
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (k < nk) {
      const int s = L.src[L.keep[k]];
      const int t = s / K;
      const fdet_tile Tl = tiles[t];
      const float* d = rows + (size_t)s * 5;
      v[0] = d[0];
      to_source(d, Tl, (float)Tl.w / (float)Wo, (float)Tl.h / (float)Ho, v[1], v[2], v[3], v[4]);
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) o[(size_t)k * 5 + e] = v[e];
  }
  if (tid == 0) {
    out_counts[n] = nk;
    if (bad) atomicAdd(rejected, 1ull);
  }
}

}  // namespace

extern "C" int fdet_tile_gather(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                                const fdet_tile* tiles, const fdet_tile* h_tiles, int T, int Ho, int Wo, uint8_t* frames,
                                void* stream) {
  FDET_REQUIRE(bank && table && h_table && tiles && h_tiles && frames, "tile_gather: null pointer");
  FDET_REQUIRE(n_images > 0 && T > 0 && T <= 65535 && Ho > 0 && Wo > 0 && (Ho + GT_H - 1) / GT_H <= 65535,
               "tile_gather: bad sizes n_images=%d T=%d %dx%d (at most 65535 windows per call)", n_images, T, Ho, Wo);
  FDET_REQUIRE((Wo % 4) != 0 || ((uintptr_t)frames % 4) == 0, "tile_gather: frames must be 4-byte aligned");
  int64_t bank_bytes = 0;                                    // the bytes the referenced images prove readable
  for (int t = 0; t < T; ++t) {
    const fdet_tile& W = h_tiles[t];
    FDET_REQUIRE(W.image >= 0 && W.image < n_images, "tile_gather: tiles[%d].image=%d outside the table of %d", t, W.image,
                 n_images);
    const fdet_aug_image& I = h_table[W.image];
    FDET_REQUIRE(I.offset >= 0 && I.h > 0 && I.w > 0, "tile_gather: bad table row %d (offset %lld, %dx%d)", W.image,
                 (long long)I.offset, I.h, I.w);
    FDET_REQUIRE(W.w > 0 && W.h > 0 && W.x0 >= 0 && W.y0 >= 0 && (int64_t)W.x0 + W.w <= I.w && (int64_t)W.y0 + W.h <= I.h,
                 "tile_gather: tiles[%d] window (%d,%d,%d,%d) outside the %dx%d source", t, W.x0, W.y0, W.w, W.h, I.w, I.h);
    const int64_t end = I.offset + (int64_t)I.h * I.w * 3;
    bank_bytes = end > bank_bytes ? end : bank_bytes;
  }
  const dim3 grid((Wo + GT_W - 1) / GT_W, (Ho + GT_H - 1) / GT_H, T);
  hipLaunchKernelGGL(k_tile_gather, grid, dim3(GT_BX, GT_BY), 0, (hipStream_t)stream, bank, bank_bytes, table, tiles, Ho, Wo,
                     frames);
  return check_launch("fdet_tile_gather");
}

extern "C" int fdet_tile_merge(const float* rows, const int32_t* counts, const fdet_tile* tiles, const int32_t* tile_offset,
                               int n_images, int T, int K, int Ho, int Wo, const fdet_aug_image* table, float edge_margin,
                               double iou_threshold, int Kout, float* out, int32_t* out_counts, uint64_t* rejected,
                               void* stream) {
  FDET_REQUIRE(rows && counts && tiles && tile_offset && table && out && out_counts && rejected, "tile_merge: null pointer");
  FDET_REQUIRE(n_images > 0 && T > 0 && K > 0 && Ho > 0 && Wo > 0 && Kout > 0 && (int64_t)T * K <= 0x7fffffffLL,
               "tile_merge: bad sizes n_images=%d T=%d K=%d %dx%d Kout=%d", n_images, T, K, Ho, Wo, Kout);
  FDET_REQUIRE(edge_margin >= 0.f, "tile_merge: edge_margin=%g must be >= 0", (double)edge_margin);
  const int64_t most = (int64_t)T * K;
  const int cap = most < MERGE_CAP ? (int)most : MERGE_CAP;
  const size_t lds = merge_lds_bytes(cap);
  if (lds > 64 * 1024)
    if (int rc = set_lds_attr(reinterpret_cast<const void*>(k_tile_merge), lds, "fdet_tile_merge")) return rc;
  hipLaunchKernelGGL(k_tile_merge, dim3(n_images), dim3(256), lds, (hipStream_t)stream, rows, counts, tiles, tile_offset, T, K,
                     Ho, Wo, table, edge_margin, iou_threshold, cap, Kout, out, out_counts,
                     reinterpret_cast<unsigned long long*>(rejected));
  return check_launch("fdet_tile_merge");
}
