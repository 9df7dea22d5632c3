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
//   fdet_render_boxes_blur  the same with Gaussian blur as PIL computes it: six integer box-blur passes per
//                       box, three along the rows and three along the columns of the box's region R, each rounded to uint8.
//     k_blur_plan        one workgroup: byte offset of every box's intermediate (3 |R| bytes) in the workspace, by a prefix
//                        sum over the boxes; a box whose intermediate ends past the workspace is counted in `rejected` and
//                        left out
//     k_blur_rows        BL_SPLIT workgroups per (image, box).  A workgroup packs as many (row, channel) lines of R as fit
//                        into BL_CAP bytes of LDS, and runs each pass as ONE prefix sum over the packed lines (a difference of
//                        two prefix values inside a line does not see the lines before it); every lane then computes its
//                        pixels from prefix reads alone.  The third pass's bytes go to the intermediate.
//     k_blur_cols        the same over (column, channel) lines of the intermediate; the last pass writes the pixels no
//                        earlier box covers (the ownership list of k_render_pixelate).
//
// tests/render_cpu_ref.py and tests/render_blur_cpu_ref.py restate the rules in numpy; every comparison is equality of bytes.
#include "fdet_common.h"
#include <cmath>
#include <cstdint>

using namespace fdet;

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_SPLIT = 8;          // workgroups that share the cells of one box
constexpr int RP_LIST = 512;         // overlapping earlier boxes kept in LDS; beyond, ownership re-reads the rows
constexpr int RP_WIDE = 64;          // cells at least this wide are walked by the whole workgroup, smaller ones by one wave

struct Rect { int x0, y0, x1, y1; };

// rule 2: fp32 corners truncated toward zero, inclusive at both ends; false = the box is skipped
__host__ __device__ __forceinline__ bool box_rect(const float* __restrict__ row, Rect& r, float& w, float& h) {
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

// the earlier boxes of the image that overlap [vx0,vx1] x [vy0,vy1], listed in LDS by the whole workgroup (barriers inside)
__device__ __forceinline__ Owner list_earlier(const float* __restrict__ irows, int box, int vx0, int vy0, int vx1, int vy1, Rect* list,
                                              int* n_list) {
  const int tid = threadIdx.x;
  if (tid == 0) *n_list = 0;
  __syncthreads();
  for (int j = tid; j < box; j += RP_THREADS) {
    Rect q;
    float w, h;
    if (box_rect(irows + (size_t)j * 5, q, w, h) && q.x0 <= vx1 && q.x1 >= vx0 && q.y0 <= vy1 && q.y1 >= vy0) {
      const int k = atomicAdd(n_list, 1);            // the list is a set: its order changes nothing
      if (k < RP_LIST) list[k] = q;
    }
  }
  __syncthreads();
  return Owner{list, *n_list, irows, box};
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
  const Owner own = list_earlier(irows, box, vx0, vy0, vx1, vy1, list, &n_list);
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

// ---- Gaussian blur (rule 3b) ------------------------------------------------------------------------------------------
constexpr int BL_THREADS = RP_THREADS;      // list_earlier strides by RP_THREADS
constexpr int BL_CAP = FDET_BLUR_MAX_LINE;  // bytes of LDS a chunk of lines fills; one line must fit
constexpr int BL_SPLIT = 16;                // workgroups that share the chunks of one box

// the prefix array is padded by one word per 32: a thread's run of up to 32 consecutive prefix writes then falls into
// banks other than its neighbours' runs
__device__ __forceinline__ int pp(int k) { return k + (k >> 5); }

struct alignas(16) BlurLds {
  uint32_t P[BL_CAP + BL_CAP / 32 + 2];     // P[pp(k)] = v[0] + .. + v[k-1] over the packed lines
  uint8_t v[BL_CAP];                        // `units` lines of length n, one after the other
  uint32_t wsum[BL_THREADS / WAVE];
};

struct BlurBox {
  int vx0, vy0, vx1, vy1;                   // R
  unsigned r, ww, fw;
};

// rule 3b.1-2 for one row of the boxes: false = skipped or nothing inside the image
__host__ __device__ __forceinline__ bool blur_region(const float* __restrict__ row, int W, int H, Rect& r, BlurBox& b) {
  float w, h;
  if (!box_rect(row, r, w, h)) return false;
  b.vx0 = r.x0 > 0 ? r.x0 : 0;
  b.vy0 = r.y0 > 0 ? r.y0 : 0;
  b.vx1 = r.x1 < W - 1 ? r.x1 : W - 1;
  b.vy1 = r.y1 < H - 1 ? r.y1 : H - 1;
  return b.vx0 <= b.vx1 && b.vy0 <= b.vy1;
}

__device__ __forceinline__ void blur_params(const int32_t* __restrict__ tab, int n_tab, const Rect& r, BlurBox& b) {
  const long long S = max((long long)r.x1 - r.x0 + 1, (long long)r.y1 - r.y0 + 1);
  const int32_t* e = tab + 3 * (size_t)min(S, (long long)n_tab - 1);
  b.r = (unsigned)max(e[0], 0);             // the host has refused negative entries; a caller whose copies differ stays in range
  b.ww = (unsigned)e[1];
  b.fw = (unsigned)e[2];
}

// byte offsets of the boxes' intermediates: offs[item] >= 0, or -1 for a box with nothing to do or rejected
__global__ void __launch_bounds__(BL_THREADS)
k_blur_plan(const float* __restrict__ rows, const int32_t* __restrict__ prefix, int n, int K, const fdet_aug_image* __restrict__ src_table,
            int total, long long cap, long long* __restrict__ offs, unsigned long long* __restrict__ rejected) {
  __shared__ unsigned long long s[BL_THREADS];
  __shared__ unsigned long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0ull;
  __syncthreads();
  int n_bad = 0;
  for (int base = 0; base < total; base += BL_THREADS) {
    const int item = base + tid;
    unsigned long long size = 0ull;
    bool bad = false;
    int image, box;
    if (item < total && find_item(prefix, n, item, image, box)) {
      const fdet_aug_image si = src_table[image];
      Rect r;
      BlurBox b;
      if (blur_region(rows + ((size_t)image * K + box) * 5, si.w, si.h, r, b)) {
        const long long rw = b.vx1 - b.vx0 + 1, rh = b.vy1 - b.vy0 + 1;
        if (rw > BL_CAP || rh > BL_CAP) bad = true;
        else size = (unsigned long long)(3 * rw * rh);
      }
    }
    s[tid] = size;
    __syncthreads();
    for (int off = 1; off < BL_THREADS; off <<= 1) {
      const unsigned long long add = tid >= off ? s[tid - off] : 0ull;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    const unsigned long long c = carry;
    const unsigned long long start = c + s[tid] - size;
    if (size && start + size > (unsigned long long)cap) bad = true;
    if (item < total) offs[item] = (size && !bad) ? (long long)start : -1ll;
    n_bad += __syncthreads_count(bad);
    if (tid == BL_THREADS - 1) carry = c + s[tid];
    __syncthreads();
  }
  if (tid == 0 && n_bad) rejected[0] += (unsigned long long)n_bad;          // the only writer: no atomic
}

// rule 3b.3, three times, over the m = units * n bytes of L.v (lines of length n); the result replaces L.v.  All threads of
// the workgroup call it; L.v must be complete (a barrier after the load), and it ends with a barrier.
__device__ __forceinline__ void blur_passes(BlurLds& L, int m, int n, unsigned r, unsigned ww, unsigned fw) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int E = 4 * ((m + 4 * BL_THREADS - 1) / (4 * BL_THREADS));          // bytes per thread, whole words; E * BL_THREADS <= BL_CAP
  const int k0 = tid * E;
  const uint32_t* vw = reinterpret_cast<const uint32_t*>(L.v);
  const int rc = (int)min(r, (unsigned)n);                                  // for indices: every tap beyond n is the edge
  for (int pass = 0; pass < 3; ++pass) {
    uint32_t tot = 0;
    for (int q = 0; q < E; q += 4) {
      const int k = k0 + q;
      if (k < m) {
        uint32_t w = vw[k >> 2];
        if (m - k < 4) w &= (1u << (8 * (m - k))) - 1u;                     // the bytes past m are not part of any line
        tot += (w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24);
      }
    }
    uint32_t inc = tot;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const uint32_t t = __shfl_up(inc, off, WAVE);
      if (lane >= off) inc += t;
    }
    if (lane == WAVE - 1) L.wsum[wid] = inc;
    __syncthreads();
    uint32_t run = inc - tot;
    for (int w = 0; w < wid; ++w) run += L.wsum[w];
    if (tid == 0) L.P[0] = 0u;
    for (int q = 0; q < E; q += 4) {
      const int k = k0 + q;
      if (k < m) {
        const uint32_t w = vw[k >> 2];
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (k + b < m) {
            run += (w >> (8 * b)) & 0xffu;
            L.P[pp(k + b + 1)] = run;
          }
      }
    }
    __syncthreads();
    // unsigned arithmetic modulo 2^32: with the validated table the true value is below 2^32, so nothing is lost
    for (int idx = tid; idx < m; idx += BL_THREADS) {
      const int u = idx / n, i = idx - u * n, b0 = u * n;
      const int lo = max(i - rc, 0), hi = min(i + rc, n - 1);
      uint32_t sum = L.P[pp(b0 + hi + 1)] - L.P[pp(b0 + lo)];
      const uint32_t nl = r > (unsigned)i ? r - (unsigned)i : 0u;
      const uint32_t nr = r + (unsigned)i > (unsigned)(n - 1) ? r + (unsigned)i - (unsigned)(n - 1) : 0u;
      if (nl | nr) {
        const uint32_t v0 = L.P[pp(b0 + 1)] - L.P[pp(b0)], vl = L.P[pp(b0 + n)] - L.P[pp(b0 + n - 1)];
        sum += nl * v0 + nr * vl;
      }
      uint32_t acc = ww * sum + (1u << 23);
      if (fw) {
        const int ja = max(i - rc - 1, 0), jb = min(i + rc + 1, n - 1);
        acc += fw * ((L.P[pp(b0 + ja + 1)] - L.P[pp(b0 + ja)]) + (L.P[pp(b0 + jb + 1)] - L.P[pp(b0 + jb)]));
      }
      L.v[idx] = (uint8_t)(acc >> 24);
    }
    __syncthreads();
  }
}

// the three row passes of a box: lines are (row, channel) of R in the source, unit 3 * row + channel
__global__ void __launch_bounds__(BL_THREADS)
k_blur_rows(const uint8_t* __restrict__ src_bank, const fdet_aug_image* __restrict__ src_table, const float* __restrict__ rows,
            const int32_t* __restrict__ prefix, int n_images, int K, const long long* __restrict__ offs,
            const int32_t* __restrict__ blur_tab, int n_tab, uint8_t* __restrict__ inter) {
  __shared__ BlurLds L;
  int image, box;
  if (!find_item(prefix, n_images, blockIdx.x, image, box)) return;          // block-uniform, as every return below
  const long long off = offs[blockIdx.x];
  if (off < 0) return;
  const fdet_aug_image si = src_table[image];
  Rect r;
  BlurBox b;
  if (!blur_region(rows + ((size_t)image * K + box) * 5, si.w, si.h, r, b)) return;
  blur_params(blur_tab, n_tab, r, b);
  const int n = b.vx1 - b.vx0 + 1, units = 3 * (b.vy1 - b.vy0 + 1);        // n, rows <= BL_CAP: k_blur_plan has checked
  const int U = BL_CAP / n, chunks = (units + U - 1) / U, nb = 3 * n;
  const int64_t row_bytes = (int64_t)si.w * 3;
  const uint8_t* src = src_bank + si.offset + (int64_t)b.vy0 * row_bytes + (int64_t)b.vx0 * 3;
  uint8_t* mid = inter + off;
  const int tid = threadIdx.x;
  for (int chunk = blockIdx.y; chunk < chunks; chunk += BL_SPLIT) {
    const int gu0 = chunk * U, Uh = min(U, units - gu0);
    // the rows the chunk's units lie in, walked byte by byte: consecutive lanes, consecutive bytes
    const int r0 = gu0 / 3, nq = ((gu0 + Uh - 1) / 3 - r0 + 1) * nb;
    for (int q = tid; q < nq; q += BL_THREADS) {
      const int rr = q / nb, bb = q - rr * nb, i = bb / 3, u = (r0 + rr) * 3 + (bb - 3 * i) - gu0;
      if (u >= 0 && u < Uh) L.v[u * n + i] = src[(int64_t)(r0 + rr) * row_bytes + bb];
    }
    __syncthreads();
    blur_passes(L, Uh * n, n, b.r, b.ww, b.fw);
    for (int q = tid; q < nq; q += BL_THREADS) {
      const int rr = q / nb, bb = q - rr * nb, i = bb / 3, u = (r0 + rr) * 3 + (bb - 3 * i) - gu0;
      if (u >= 0 && u < Uh) mid[(int64_t)(r0 + rr) * nb + bb] = L.v[u * n + i];
    }
    __syncthreads();
  }
}

// the three column passes: lines are (column, channel) of the intermediate, unit 3 * column + channel = the byte's offset in
// its row; the result goes to the pixels of R that no earlier box covers
__global__ void __launch_bounds__(BL_THREADS)
k_blur_cols(const fdet_aug_image* __restrict__ src_table, const float* __restrict__ rows, const int32_t* __restrict__ prefix, int n_images,
            int K, const long long* __restrict__ offs, const int32_t* __restrict__ blur_tab, int n_tab, const uint8_t* __restrict__ inter,
            uint8_t* __restrict__ dst_bank, const fdet_aug_image* __restrict__ dst_table) {
  __shared__ BlurLds L;
  __shared__ Rect list[RP_LIST];
  __shared__ int n_list;
  int image, box;
  if (!find_item(prefix, n_images, blockIdx.x, image, box)) return;
  const long long off = offs[blockIdx.x];
  if (off < 0) return;
  const fdet_aug_image si = src_table[image], di = dst_table[image];
  const float* irows = rows + (size_t)image * K * 5;
  Rect r;
  BlurBox b;
  if (!blur_region(irows + (size_t)box * 5, si.w, si.h, r, b)) return;
  blur_params(blur_tab, n_tab, r, b);
  const int n = b.vy1 - b.vy0 + 1, units = 3 * (b.vx1 - b.vx0 + 1);
  const int U = BL_CAP / n, chunks = (units + U - 1) / U;
  if ((int)blockIdx.y >= chunks) return;
  const Owner own = list_earlier(irows, box, b.vx0, b.vy0, b.vx1, b.vy1, list, &n_list);
  const int64_t row_bytes = (int64_t)si.w * 3;
  const uint8_t* mid = inter + off;
  uint8_t* dst = dst_bank + di.offset + (int64_t)b.vy0 * row_bytes + (int64_t)b.vx0 * 3;
  const int tid = threadIdx.x;
  for (int chunk = blockIdx.y; chunk < chunks; chunk += BL_SPLIT) {
    const int gu0 = chunk * U, Uh = min(U, units - gu0), m = Uh * n;
    for (int q = tid; q < m; q += BL_THREADS) {
      const int i = q / Uh, u = q - i * Uh;
      L.v[u * n + i] = mid[(int64_t)i * units + gu0 + u];
    }
    __syncthreads();
    blur_passes(L, m, n, b.r, b.ww, b.fw);
    for (int q = tid; q < m; q += BL_THREADS) {
      const int i = q / Uh, u = q - i * Uh;
      if (!covered(own, b.vx0 + (gu0 + u) / 3, b.vy0 + i)) dst[(int64_t)i * row_bytes + gu0 + u] = L.v[u * n + i];
    }
    __syncthreads();
  }
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

namespace {

struct BlurArgs {
  int blur;
  const int32_t *tab, *h_tab;
  int n_tab;
  size_t ws_bytes;
  uint64_t* rejected;
};

// ws: prefix int32 [n_images + 1] | offsets int64 [total boxes] (8-byte aligned) | the boxes' intermediates
size_t blur_header_bytes(int n_images, int64_t total) { return align8(sizeof(int32_t) * ((size_t)n_images + 1)) + sizeof(int64_t) * (size_t)total; }

int render_impl(const char* what, const uint8_t* src, const fdet_aug_image* src_table, const fdet_aug_image* h_src_table, const float* rows,
                const int32_t* counts, const int32_t* h_counts, int n_images, int K, uint8_t* dst, const fdet_aug_image* dst_table,
                const fdet_aug_image* h_dst_table, int outline, int pixelate, int blocks, int red, int green, int blue, void* ws,
                const BlurArgs& B, void* stream) {
  FDET_REQUIRE(src && src_table && h_src_table && counts && h_counts && dst && dst_table && h_dst_table && ws, "%s: null pointer",
               what);
  FDET_REQUIRE(n_images > 0 && K >= 0 && (K == 0 || rows), "%s: bad sizes n_images=%d K=%d (rows may be NULL only with K = 0)", what,
               n_images, K);
  FDET_REQUIRE(blocks >= 1, "%s: blocks=%d must be >= 1", what, blocks);
  FDET_REQUIRE((outline == 0 || outline == 1) && (pixelate == 0 || pixelate == 1), "%s: outline=%d and pixelate=%d must be 0 or 1", what,
               outline, pixelate);
  FDET_REQUIRE(B.blur == 0 || B.blur == 1, "%s: blur=%d must be 0 or 1", what, B.blur);
  FDET_REQUIRE(!(B.blur && pixelate), "%s: blur and pixelate exclude each other", what);
  FDET_REQUIRE(red >= 0 && red <= 255 && green >= 0 && green <= 255 && blue >= 0 && blue <= 255, "%s: colour (%d,%d,%d) outside 0..255",
               what, red, green, blue);
  if (B.blur) {
    FDET_REQUIRE(B.tab && B.h_tab && B.rejected, "%s: null pointer (blur table or rejected)", what);
    FDET_REQUIRE(B.n_tab >= 1, "%s: n_tab=%d must be >= 1", what, B.n_tab);
    for (int e = 0; e < B.n_tab; ++e) {
      const int64_t r = B.h_tab[3 * (size_t)e], ww = B.h_tab[3 * (size_t)e + 1], fw = B.h_tab[3 * (size_t)e + 2];
      FDET_REQUIRE(r >= 0 && ww >= 0 && fw >= 0 && (2 * r + 1) * ww + 2 * fw <= (int64_t)1 << 24,
                   "%s: blur table entry %d (r=%lld, ww=%lld, fw=%lld): negative, or weights (2r+1)*ww + 2*fw above 2^24", what, e, (long long)r,
                   (long long)ww, (long long)fw);
    }
  }
  int64_t s_lo = INT64_MAX, s_hi = 0, d_lo = INT64_MAX, d_hi = 0, total = 0;
  for (int i = 0; i < n_images; ++i) {
    const fdet_aug_image &S = h_src_table[i], &D = h_dst_table[i];
    FDET_REQUIRE(S.offset >= 0 && S.h > 0 && S.w > 0 && (int64_t)S.h * S.w < 0x7fffffffLL, "%s: bad source table row %d (offset %lld, %dx%d)",
                 what, i, (long long)S.offset, S.h, S.w);
    FDET_REQUIRE(D.offset >= 0 && D.h == S.h && D.w == S.w, "%s: destination table row %d (offset %lld, %dx%d) does not match the source's %dx%d",
                 what, i, (long long)D.offset, D.h, D.w, S.h, S.w);
    FDET_REQUIRE(h_counts[i] >= 0 && h_counts[i] <= K, "%s: counts[%d]=%d outside 0..K=%d", what, i, h_counts[i], K);
    FDET_REQUIRE(!B.blur || (S.h <= FDET_BLUR_MAX_LINE && S.w <= FDET_BLUR_MAX_LINE), "%s: image %d is %dx%d, blur takes lines of at most %d pixels",
                 what, i, S.h, S.w, FDET_BLUR_MAX_LINE);
    const int64_t bytes = (int64_t)S.h * S.w * 3;
    s_lo = S.offset < s_lo ? S.offset : s_lo;
    s_hi = S.offset + bytes > s_hi ? S.offset + bytes : s_hi;
    d_lo = D.offset < d_lo ? D.offset : d_lo;
    d_hi = D.offset + bytes > d_hi ? D.offset + bytes : d_hi;
    total += h_counts[i];
  }
  FDET_REQUIRE(total <= 0x7fffffffLL, "%s: %lld boxes in one call", what, (long long)total);
  const size_t header = B.blur ? blur_header_bytes(n_images, total) : sizeof(int32_t) * ((size_t)n_images + 1);
  FDET_REQUIRE(B.ws_bytes >= header, "%s: workspace of %zu bytes, %zu needed before the boxes' intermediates", what, B.ws_bytes, header);
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
  if (total == 0 || (!outline && !pixelate && !B.blur)) return FDET_OK;
  int32_t* prefix = static_cast<int32_t*>(ws);
  hipLaunchKernelGGL(k_render_prefix, dim3(1), dim3(RP_THREADS), 0, st, counts, n_images, K, prefix);
  if (pixelate)
    hipLaunchKernelGGL(k_render_pixelate, dim3((unsigned)total, RP_SPLIT), dim3(RP_THREADS), 0, st, src, src_table, rows, prefix, n_images, K,
                       blocks, dst, dst_table);
  if (B.blur) {
    uint8_t* base = static_cast<uint8_t*>(ws);
    long long* offs = reinterpret_cast<long long*>(base + align8(sizeof(int32_t) * ((size_t)n_images + 1)));
    uint8_t* inter = base + header;
    hipLaunchKernelGGL(k_blur_plan, dim3(1), dim3(BL_THREADS), 0, st, rows, prefix, n_images, K, src_table, (int)total,
                       (long long)(B.ws_bytes - header), offs, reinterpret_cast<unsigned long long*>(B.rejected));
    hipLaunchKernelGGL(k_blur_rows, dim3((unsigned)total, BL_SPLIT), dim3(BL_THREADS), 0, st, src, src_table, rows, prefix, n_images, K, offs,
                       B.tab, B.n_tab, inter);
    hipLaunchKernelGGL(k_blur_cols, dim3((unsigned)total, BL_SPLIT), dim3(BL_THREADS), 0, st, src_table, rows, prefix, n_images, K, offs,
                       B.tab, B.n_tab, inter, dst, dst_table);
  }
  if (outline)
    hipLaunchKernelGGL(k_render_outline, dim3((unsigned)total), dim3(RP_THREADS), 0, st, rows, prefix, n_images, K, dst, dst_table,
                       (uint8_t)red, (uint8_t)green, (uint8_t)blue);
  return check_launch(what);
}

}  // namespace

extern "C" int fdet_render_boxes(const uint8_t* src, const fdet_aug_image* src_table, const fdet_aug_image* h_src_table,
                                 const float* rows, const int32_t* counts, const int32_t* h_counts, int n_images, int K,
                                 uint8_t* dst, const fdet_aug_image* dst_table, const fdet_aug_image* h_dst_table, int outline,
                                 int pixelate, int blocks, int red, int green, int blue, int32_t* ws, void* stream) {
  const BlurArgs none{0, nullptr, nullptr, 0, SIZE_MAX, nullptr};
  return render_impl("fdet_render_boxes", src, src_table, h_src_table, rows, counts, h_counts, n_images, K, dst, dst_table, h_dst_table,
                     outline, pixelate, blocks, red, green, blue, ws, none, stream);
}

extern "C" size_t fdet_render_blur_ws_bytes(const fdet_aug_image* h_src_table, const float* h_rows, const int32_t* h_counts, int n_images,
                                            int K) {
  if (!h_src_table || !h_counts || n_images <= 0 || K < 0 || (K > 0 && !h_rows)) return 0;
  int64_t total = 0;
  size_t bytes = 0;
  for (int i = 0; i < n_images; ++i) {
    if (h_counts[i] < 0 || h_counts[i] > K) return 0;
    total += h_counts[i];
    for (int k = 0; k < h_counts[i]; ++k) {
      Rect r;
      BlurBox b;
      if (blur_region(h_rows + ((size_t)i * K + k) * 5, h_src_table[i].w, h_src_table[i].h, r, b))
        bytes += (size_t)3 * (size_t)(b.vx1 - b.vx0 + 1) * (size_t)(b.vy1 - b.vy0 + 1);
    }
  }
  return blur_header_bytes(n_images, total) + bytes;
}

extern "C" int fdet_render_boxes_blur(const uint8_t* src, const fdet_aug_image* src_table, const fdet_aug_image* h_src_table,
                                      const float* rows, const int32_t* counts, const int32_t* h_counts, int n_images, int K,
                                      uint8_t* dst, const fdet_aug_image* dst_table, const fdet_aug_image* h_dst_table, int outline,
                                      int pixelate, int blur, int blocks, const int32_t* blur_tab, const int32_t* h_blur_tab, int n_tab,
                                      int red, int green, int blue, void* ws, size_t ws_bytes, uint64_t* rejected, void* stream) {
  const BlurArgs B{blur, blur_tab, h_blur_tab, n_tab, ws_bytes, rejected};
  return render_impl("fdet_render_boxes_blur", src, src_table, h_src_table, rows, counts, h_counts, n_images, K, dst, dst_table,
                     h_dst_table, outline, pixelate, blocks, red, green, blue, ws, B, stream);
}
