// Rendering detections into a second image bank: PIL-exact outlines and pixelation.
//
//   fdet_render_boxes   dst image i = src image i (device-to-device copies, one per run of images that are consecutive in
//                       both banks: one for a whole bank), then two launches whose work items are boxes, not pixels of the
//                       bank:
//     k_render_pixelate  RP_SPLIT workgroups per (image, box).  A workgroup lists the earlier boxes of its image that
//                        overlap its own in LDS (usually none after the merge), walks the box's cells, sums each cell over
//                        the SOURCE image and writes the rounded mean to the pixels no earlier box covers.  Workgroups
//                        write disjoint pixels and read only the source, so no order of execution changes a byte.
//     k_render_outline   one workgroup per (image, box) paints the four bands of the outline.  All outlines share one colour,
//                        so workgroups that overlap write equal bytes.
//   The (image, box) of a workgroup comes from the prefix sum of `counts` (k_render_prefix, into ws).
//
// Pixels are 3 bytes at arbitrary byte offsets (odd widths, banks with lead bytes), so both kernels move single bytes, one
// pixel per lane along a row: the three byte accesses of a wave cover one contiguous run of 192 bytes.  Only box pixels are
// touched; the bulk of the bytes moves in the copy.
//
// tests/render_cpu_ref.py restates the rules in numpy; every comparison is equality of bytes.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_SPLIT = 8;          // workgroups that share the cells of one box
constexpr int RP_LIST = 512;         // overlapping earlier boxes kept in LDS; beyond, ownership re-reads the rows
constexpr int RP_WIDE = 64;          // cells at least this wide are walked by the whole workgroup, smaller ones by one wave

struct Rect { int x0, y0, x1, y1; };

// rule 2: fp32 corners truncated toward zero, inclusive at both ends; false = the box is skipped
__device__ __forceinline__ bool box_rect(const float* __restrict__ row, Rect& r, float& w, float& h) {
  const float x = row[1], y = row[2];
  w = row[3];
  h = row[4];
  const float lim = 16777216.f;
  const float xe = x + w, ye = y + h;
  // written so that a NaN or an infinity anywhere fails
  if (!(fabsf(x) <= lim && fabsf(y) <= lim && fabsf(xe) <= lim && fabsf(ye) <= lim && w >= 1.f && h >= 1.f))
    return false;
  r.x0 = (int)x;
  r.y0 = (int)y;
  r.x1 = (int)xe;
  r.y1 = (int)ye;
  // w, h >= 1 leave a rectangle of zero width or height only where truncation toward zero folds a start in (-1, 0) and an
  // end in [0, 1) onto pixel 0; PIL paints such rectangles by another rule, so they are skipped too
  return r.x1 > r.x0 && r.y1 > r.y0;
}

// work item -> (image, box): the last image whose first item is <= item (images without boxes are stepped over)
__device__ __forceinline__ bool find_item(const int32_t* __restrict__ prefix, int n, int item, int& image, int& box) {
  if (item >= prefix[n]) return false;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= item) lo = mid; else hi = mid - 1;
  }
  image = lo;
  box = item - prefix[lo];
  return true;
}

// exclusive prefix sum of counts clamped to 0..K (the host has refused counts outside; the clamp keeps a caller whose two
// copies differ inside the rows)
__global__ void __launch_bounds__(RP_THREADS)
k_render_prefix(const int32_t* __restrict__ counts, int n, int K, int32_t* __restrict__ prefix) {
  __shared__ int s[RP_THREADS];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += RP_THREADS) {
    const int i = base + tid;
    const int v = i < n ? min(max(counts[i], 0), K) : 0;
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < RP_THREADS; off <<= 1) {
      const int add = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    const int c = carry;
    if (i < n) prefix[i] = c + s[tid] - v;
    __syncthreads();
    if (tid == RP_THREADS - 1) carry = c + s[tid];
    __syncthreads();
  }
  if (tid == 0) prefix[n] = carry;
}

struct Owner {
  const Rect* list;          // LDS
  int n_list;                // > RP_LIST: the list overflowed, read the rows
  const float* rows;         // the image's rows
  int box;
};

// does a box of lower index cover (x, y)?
__device__ __forceinline__ bool covered(const Owner& o, int x, int y) {
  if (o.n_list <= RP_LIST) {
    for (int e = 0; e < o.n_list; ++e) {
      const Rect q = o.list[e];
      if (x >= q.x0 && x <= q.x1 && y >= q.y0 && y <= q.y1) return true;
    }
    return false;
  }
  for (int j = 0; j < o.box; ++j) {
    Rect q;
    float w, h;
    if (box_rect(o.rows + (size_t)j * 5, q, w, h) && x >= q.x0 && x <= q.x1 && y >= q.y0 && y <= q.y1) return true;
  }
  return false;
}

// channel sums of the source pixels of the cell [cx0,cx1] x [cy0,cy1] taken row-major at positions first, first + stride, ..
// by this lane, added up over the lanes of its wave (every lane returns the wave's totals).  Row-major positions, not one
// row per step: a cell narrower than the wave still keeps all its lanes busy.
__device__ __forceinline__ void cell_sums(const uint8_t* __restrict__ src, int64_t row_bytes, int cx0, int cx1, int cy0, int cy1,
                                          int first, int stride, unsigned long long (&sum)[3]) {
  sum[0] = sum[1] = sum[2] = 0ull;
  const int cw = cx1 - cx0 + 1, total = cw * (cy1 - cy0 + 1);     // an image holds fewer than 2^31 pixels
  for (int i = first; i < total; i += stride) {
    const int dy = i / cw;
    const uint8_t* p = src + (int64_t)(cy0 + dy) * row_bytes + (int64_t)(cx0 + i - dy * cw) * 3;
    sum[0] += p[0];
    sum[1] += p[1];
    sum[2] += p[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    unsigned long long v = sum[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    sum[c] = v;
  }
}

__global__ void __launch_bounds__(RP_THREADS)
k_render_pixelate(const uint8_t* __restrict__ src_bank, const fdet_aug_image* __restrict__ src_table,
                  const float* __restrict__ rows, const int32_t* __restrict__ prefix, int n, int K, int blocks,
                  uint8_t* __restrict__ dst_bank, const fdet_aug_image* __restrict__ dst_table) {
  __shared__ Rect list[RP_LIST];
  __shared__ int n_list;
  __shared__ unsigned long long part[RP_THREADS / WAVE][3];
  int image, box;
  if (!find_item(prefix, n, blockIdx.x, image, box)) return;                   // block-uniform
  const float* irows = rows + (size_t)image * K * 5;
  Rect r;
  float bw, bh;
  if (!box_rect(irows + (size_t)box * 5, r, bw, bh)) return;
  const fdet_aug_image si = src_table[image], di = dst_table[image];
  const int W = si.w, H = si.h;
  // the box clipped to the image; nothing of it inside: nothing to do
  const int vx0 = max(r.x0, 0), vy0 = max(r.y0, 0), vx1 = min(r.x1, W - 1), vy1 = min(r.y1, H - 1);
  if (vx0 > vx1 || vy0 > vy1) return;
  const int m = max(r.x1 - r.x0 + 1, r.y1 - r.y0 + 1);
  const int cell = (int)max((long long)1, ((long long)m + blocks - 1) / blocks);
  if (cell == 1) return;                             // every mean is its own pixel: the copy already holds it
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
  if (tid == 0) n_list = 0;
  __syncthreads();
  for (int j = tid; j < box; j += RP_THREADS) {
    Rect q;
    float w, h;
    if (box_rect(irows + (size_t)j * 5, q, w, h) && q.x0 <= vx1 && q.x1 >= vx0 && q.y0 <= vy1 && q.y1 >= vy0) {
      const int k = atomicAdd(&n_list, 1);           // the list is a set: its order changes nothing
      if (k < RP_LIST) list[k] = q;
    }
  }
  __syncthreads();
  const Owner own{list, n_list, irows, box};
  const uint8_t* src = src_bank + si.offset;
  uint8_t* dst = dst_bank + di.offset;
  const int64_t row_bytes = (int64_t)W * 3;
  // the cells that reach into the image
  const int ci0 = (vx0 - r.x0) / cell, ci1 = (vx1 - r.x0) / cell, cj0 = (vy0 - r.y0) / cell, cj1 = (vy1 - r.y0) / cell;
  const int ncx = ci1 - ci0 + 1;
  const long long ncells = (long long)ncx * (cj1 - cj0 + 1);
  const bool wide = cell >= RP_WIDE;                 // block-uniform
  const int nw = RP_THREADS / WAVE;
  // wide: the workgroup takes cell blockIdx.y, blockIdx.y + RP_SPLIT, ..; else each wave takes its own cells
  const long long c0 = wide ? blockIdx.y : (long long)blockIdx.y * nw + wid;
  const long long cstep = wide ? RP_SPLIT : (long long)RP_SPLIT * nw;
  for (long long c = c0; c < ncells; c += cstep) {              // wide: c is block-uniform, so the barriers below are too
    const int ci = ci0 + (int)(c % ncx), cj = cj0 + (int)(c / ncx);
    const int cx0 = max(r.x0 + ci * cell, vx0), cx1 = min(r.x0 + ci * cell + cell - 1, vx1);
    const int cy0 = max(r.y0 + cj * cell, vy0), cy1 = min(r.y0 + cj * cell + cell - 1, vy1);
    unsigned long long sum[3];
    const int first = wide ? tid : lane, stride = wide ? RP_THREADS : WAVE;
    cell_sums(src, row_bytes, cx0, cx1, cy0, cy1, first, stride, sum);
    if (wide) {
      if (lane == 0) { part[wid][0] = sum[0]; part[wid][1] = sum[1]; part[wid][2] = sum[2]; }
      __syncthreads();
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        sum[ch] = 0ull;
        for (int w = 0; w < nw; ++w) sum[ch] += part[w][ch];
      }
      __syncthreads();
    }
    const int cw = cx1 - cx0 + 1, total = cw * (cy1 - cy0 + 1);
    const unsigned long long cnt = (unsigned long long)total;
    const uint8_t v0 = (uint8_t)((sum[0] + cnt / 2) / cnt), v1 = (uint8_t)((sum[1] + cnt / 2) / cnt),
                  v2 = (uint8_t)((sum[2] + cnt / 2) / cnt);
    for (int i = first; i < total; i += stride) {
      const int dy = i / cw, x = cx0 + i - dy * cw, y = cy0 + dy;
      if (covered(own, x, y)) continue;
      uint8_t* p = dst + (int64_t)y * row_bytes + (int64_t)x * 3;
      p[0] = v0;
      p[1] = v1;
      p[2] = v2;
    }
  }
}

// one band [bx0,bx1] x [by0,by1] (already inside the image; empty when a low end exceeds its high end)
__device__ __forceinline__ void paint_band(uint8_t* __restrict__ dst, int64_t row_bytes, int bx0, int by0, int bx1, int by1, int tid,
                                           uint8_t cr, uint8_t cg, uint8_t cb) {
  if (bx0 > bx1 || by0 > by1) return;
  const int bwid = bx1 - bx0 + 1;
  const long long total = (long long)bwid * (by1 - by0 + 1);
  for (long long i = tid; i < total; i += RP_THREADS) {
    const int y = by0 + (int)(i / bwid), x = bx0 + (int)(i % bwid);
    uint8_t* p = dst + (int64_t)y * row_bytes + (int64_t)x * 3;
    p[0] = cr; p[1] = cg; p[2] = cb;
  }
}

__global__ void __launch_bounds__(RP_THREADS)
k_render_outline(const float* __restrict__ rows, const int32_t* __restrict__ prefix, int n, int K, uint8_t* __restrict__ dst_bank,
                 const fdet_aug_image* __restrict__ dst_table, uint8_t cr, uint8_t cg, uint8_t cb) {
  int image, box;
  if (!find_item(prefix, n, blockIdx.x, image, box)) return;
  Rect r;
  float bw, bh;
  if (!box_rect(rows + ((size_t)image * K + box) * 5, r, bw, bh)) return;
  const int t = (bw <= 15.f || bh <= 15.f) ? 1 : 3;              // the reference's rule (datasets/utils.py:198-201)
  const fdet_aug_image di = dst_table[image];
  const int W = di.w, H = di.h;
  uint8_t* dst = dst_bank + di.offset;
  const int64_t row_bytes = (int64_t)W * 3;
  const int tid = threadIdx.x;
  const int cx0 = max(r.x0, 0), cx1 = min(r.x1, W - 1);
  // the rectangle minus the rectangle shrunk by t: rows y0..y0+t-1 and y1-t+1..y1 whole, columns x0..x0+t-1 and x1-t+1..x1
  // of the rows between.  Where 2t exceeds the extent the inner rectangle is empty and the bands cover the whole rectangle.
  const int top1 = min(r.y0 + t - 1, r.y1);
  const int bot0 = max(r.y1 - t + 1, top1 + 1);
  paint_band(dst, row_bytes, cx0, max(r.y0, 0), cx1, min(top1, H - 1), tid, cr, cg, cb);
  paint_band(dst, row_bytes, cx0, max(bot0, 0), cx1, min(r.y1, H - 1), tid, cr, cg, cb);
  const int my0 = max(top1 + 1, 0), my1 = min(bot0 - 1, H - 1);
  const int left1 = min(r.x0 + t - 1, r.x1);
  const int right0 = max(r.x1 - t + 1, left1 + 1);
  paint_band(dst, row_bytes, cx0, my0, min(left1, W - 1), my1, tid, cr, cg, cb);
  paint_band(dst, row_bytes, max(right0, 0), my0, cx1, my1, tid, cr, cg, cb);
}

}  // namespace

extern "C" int fdet_render_boxes(const uint8_t* src, const fdet_aug_image* src_table, const fdet_aug_image* h_src_table,
                                 const float* rows, const int32_t* counts, const int32_t* h_counts, int n_images, int K,
                                 uint8_t* dst, const fdet_aug_image* dst_table, const fdet_aug_image* h_dst_table, int outline,
                                 int pixelate, int blocks, int red, int green, int blue, int32_t* ws, void* stream) {
  const char* what = "fdet_render_boxes";
  FDET_REQUIRE(src && src_table && h_src_table && counts && h_counts && dst && dst_table && h_dst_table && ws, "%s: null pointer",
               what);
  FDET_REQUIRE(n_images > 0 && K >= 0 && (K == 0 || rows), "%s: bad sizes n_images=%d K=%d (rows may be NULL only with K = 0)", what,
               n_images, K);
  FDET_REQUIRE(blocks >= 1, "%s: blocks=%d must be >= 1", what, blocks);
  FDET_REQUIRE((outline == 0 || outline == 1) && (pixelate == 0 || pixelate == 1), "%s: outline=%d and pixelate=%d must be 0 or 1", what,
               outline, pixelate);
  FDET_REQUIRE(red >= 0 && red <= 255 && green >= 0 && green <= 255 && blue >= 0 && blue <= 255, "%s: colour (%d,%d,%d) outside 0..255",
               what, red, green, blue);
  int64_t s_lo = INT64_MAX, s_hi = 0, d_lo = INT64_MAX, d_hi = 0, total = 0;
  for (int i = 0; i < n_images; ++i) {
    const fdet_aug_image &S = h_src_table[i], &D = h_dst_table[i];
    FDET_REQUIRE(S.offset >= 0 && S.h > 0 && S.w > 0 && (int64_t)S.h * S.w < 0x7fffffffLL, "%s: bad source table row %d (offset %lld, %dx%d)",
                 what, i, (long long)S.offset, S.h, S.w);
    FDET_REQUIRE(D.offset >= 0 && D.h == S.h && D.w == S.w, "%s: destination table row %d (offset %lld, %dx%d) does not match the source's %dx%d",
                 what, i, (long long)D.offset, D.h, D.w, S.h, S.w);
    FDET_REQUIRE(h_counts[i] >= 0 && h_counts[i] <= K, "%s: counts[%d]=%d outside 0..K=%d", what, i, h_counts[i], K);
    const int64_t bytes = (int64_t)S.h * S.w * 3;
    s_lo = S.offset < s_lo ? S.offset : s_lo;
    s_hi = S.offset + bytes > s_hi ? S.offset + bytes : s_hi;
    d_lo = D.offset < d_lo ? D.offset : d_lo;
    d_hi = D.offset + bytes > d_hi ? D.offset + bytes : d_hi;
    total += h_counts[i];
  }
  FDET_REQUIRE(total <= 0x7fffffffLL, "%s: %lld boxes in one call", what, (long long)total);
  // the byte ranges the two tables span must be disjoint
  const uintptr_t sa = (uintptr_t)src + (uintptr_t)s_lo, sb = (uintptr_t)src + (uintptr_t)s_hi;
  const uintptr_t da = (uintptr_t)dst + (uintptr_t)d_lo, db = (uintptr_t)dst + (uintptr_t)d_hi;
  FDET_REQUIRE(sb <= da || db <= sa, "%s: source and destination overlap", what);
  // rule 1: one copy per run of images that follow each other in both banks
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n_images;) {
    int64_t bytes = (int64_t)h_src_table[i].h * h_src_table[i].w * 3;
    int j = i + 1;
    while (j < n_images && h_src_table[j].offset == h_src_table[i].offset + bytes && h_dst_table[j].offset == h_dst_table[i].offset + bytes) {
      bytes += (int64_t)h_src_table[j].h * h_src_table[j].w * 3;
      ++j;
    }
    const hipError_t e = hipMemcpyAsync(dst + h_dst_table[i].offset, src + h_src_table[i].offset, (size_t)bytes, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(FDET_ELAUNCH, "%s: copy of images %d..%d: %s", what, i, j - 1, hipGetErrorString(e));
    i = j;
  }
  if (total == 0 || (!outline && !pixelate)) return FDET_OK;
  hipLaunchKernelGGL(k_render_prefix, dim3(1), dim3(RP_THREADS), 0, st, counts, n_images, K, ws);
  if (pixelate)
    hipLaunchKernelGGL(k_render_pixelate, dim3((unsigned)total, RP_SPLIT), dim3(RP_THREADS), 0, st, src, src_table, rows, ws, n_images, K,
                       blocks, dst, dst_table);
  if (outline)
    hipLaunchKernelGGL(k_render_outline, dim3((unsigned)total), dim3(RP_THREADS), 0, st, rows, ws, n_images, K, dst, dst_table,
                       (uint8_t)red, (uint8_t)green, (uint8_t)blue);
  return check_launch(what);
}
