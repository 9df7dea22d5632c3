// The box primitives of the post-processing kernels: ordered compaction, stable descending rank, the NaN-last key, the
// fp32 overlap, the greedy sweep and the LDS carve of the candidate arrays.  Each is a rule that a restatement test checks
// bit for bit, and each is stated here once: fdet_detect.hip (YOLO decode / NMS / reduce, step metrics), fdet_ssd.hip (SSD
// reduce, the tie count of the SSD loss), fdet_tiles.hip (tile merge, with and without box voting), fdet_eval.hip and
// fdet_eval_wider.hip (rank and key) all call these, and fdet_track_refine.hip the ordered compaction.  The tracker, the
// chip and the render kernels follow integer rules of their own, and the WIDER evaluator's fp64 "+1" overlap is a different
// rule: they are not here.
//
// Every file that includes this is built with -ffp-contract=off: the results are compared BIT-EXACTLY with the
// reference's CPU arithmetic (separate mul and add, IEEE division), so no FMA contraction is allowed in these functions.
#pragma once
#include "fdet_common.h"
#include <cmath>

namespace fdet {

constexpr int BOX_THREADS = 256;       // every kernel here is one 256-thread workgroup (4 waves) per image

// --------------------------------------------------------------------------------------------------------------------
// LDS carve of the candidate arrays: 28 bytes per candidate, 32 with a keep list, one dead flag each (padded to 16), and
// 64 bytes of control words.  A greedy NMS over K candidates with its keep list spends 33 bytes per candidate.
// --------------------------------------------------------------------------------------------------------------------
struct BoxLds {
  float *x1, *y1, *x2, *y2;
  float* key;            // the score the candidates are ordered by
  float* area;           // plane 5 as the NMS kernels use it: (x2 - x1) * (y2 - y1), filled by box_greedy_nms
  int* src;              // plane 5 as the tile merge uses it (candidate -> input row); its `area` is null
  int* order;            // sorted position -> candidate index
  int* keep;             // visiting order -> candidate index; null without a keep list
  unsigned char* dead;   // by sorted position
  int* ctl;              // [0] running count, [1..4] per-wave counts (compact_slot), [5] kept (box_greedy_nms)
};

__host__ __device__ inline size_t box_lds_bytes(int cap, bool keep) {
  return (size_t)cap * (keep ? 32 : 28) + (size_t)((cap + 15) / 16) * 16 + 64;
}

// Seven planes, the dead flags, the control words, then the keep list if there is one (behind the control words: fdet_nms
// measures 6 % slower on the MI355X with the keep list in front of the dead flags).
// area_plane: plane 5 holds precomputed areas (else it is `src` and the sweep computes areas from the corners: the tile
// merge, at 160 576 of 163 840 bytes for 4864 candidates, has no LDS left for both).  The two forms give identical bits.
__device__ __forceinline__ BoxLds box_carve(char* smem, int cap, bool keep, bool area_plane) {
  BoxLds L;
  float* f = reinterpret_cast<float*>(smem);
  L.x1 = f; L.y1 = f + cap; L.x2 = f + 2 * cap; L.y2 = f + 3 * cap; L.key = f + 4 * cap;
  L.area = area_plane ? f + 5 * cap : nullptr;
  L.src = area_plane ? nullptr : reinterpret_cast<int*>(f + 5 * cap);
  L.order = reinterpret_cast<int*>(f + 6 * cap);
  L.dead = reinterpret_cast<unsigned char*>(f + 7 * cap);
  L.ctl = reinterpret_cast<int*>(smem + box_lds_bytes(cap, false) - 64);
  L.keep = keep ? L.ctl + 16 : nullptr;
  return L;
}

// --------------------------------------------------------------------------------------------------------------------
// Ordered block compaction, one 256-wide chunk per call: the slot of this thread's element among the hits of the whole
// sweep, in element order (chunk, then thread).  Every thread of the block calls it once per chunk, uniformly.
// ctl[0] (the hits of the earlier chunks) must be 0, and visible, before the first call; it holds the total once a
// barrier has followed the last call.  A thread without a hit gets a slot it must not use.
// Two barriers per chunk: the slot of the block's last thread, plus its own hit, is the new total; it stores it after the
// second barrier, by which time every thread has read the old one, and the next call's per-wave counts are written only
// after that barrier too.
// --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int compact_slot(bool hit, int* ctl /*LDS [5]*/) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned long long bal = __ballot(hit);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) ctl[1 + wid] = __popcll(bal);
  __syncthreads();
  int slot = ctl[0] + before;
  for (int w = 0; w < wid; ++w) slot += ctl[1 + w];
  __syncthreads();
  if (tid == BOX_THREADS - 1) ctl[0] = slot + (hit ? 1 : 0);
  return slot;
}

// --------------------------------------------------------------------------------------------------------------------
// Stable descending order by rank counting: rank_i = #{j : s_j > s_i or (s_j == s_i and j < i)}, the position of element i
// in torch.sort(descending=True, stable=True) (lowest index first on equal keys).  The > is strict and the tie term is
// separate, so that equal keys get distinct ranks; keys must not be NaN for the ranks to be a permutation.
// --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int box_rank(const float* key /*LDS [K]*/, int K, int i) {
  const float si = key[i];
  int r = 0;
  for (int j = 0; j < K; ++j) { const float sj = key[j]; r += (sj > si) || (sj == si && j < i); }
  return r;
}

// The key of a score where a NaN must sort last and -0 must tie with +0 (the evaluators, the tile merge).  fdet_nms,
// fdet_reduce_bounding_boxes and the SSD reducer rank the raw score, as torchvision does: they do not call this.
__device__ __forceinline__ float nan_last_key(float s) { return (s == s) ? s + 0.0f : -INFINITY; }

// --------------------------------------------------------------------------------------------------------------------
// fp32 overlap of two corner boxes with their areas (x2 - x1) * (y2 - y1), in the order of operations of torchvision
// 0.11.2's nms_kernel.cpp (box_iou of the same release computes the same value): clamp each extent at 0, one multiply,
// then inter / (a + b - inter) with an IEEE division.  0/0 = NaN, which compares false with every threshold: two empty
// boxes never suppress or match each other.
// --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float box_overlap(float ax1, float ay1, float ax2, float ay2, float aa, float bx1, float by1,
                                             float bx2, float by2, float ba) {
  const float w = fmaxf(0.f, fminf(ax2, bx2) - fmaxf(ax1, bx1));
  const float h = fmaxf(0.f, fminf(ay2, by2) - fmaxf(ay1, by1));
  const float inter = w * h;
  return inter / (aa + ba - inter);
}

// --------------------------------------------------------------------------------------------------------------------
// Greedy NMS over the K candidates in L (torchvision 0.11.2 nms_kernel.cpp): candidates are visited in stable descending
// key order, a survivor suppresses every later one whose fp32 overlap, widened to double, is > thr (strict).  One barrier
// per keeper.  The candidates must be visible to the block on entry (a barrier since they were written).
//
// What happens to a keeper and to what it suppresses is the caller's, passed as an inlined hook object:
//   begin()                          once, before the first barrier (set up LDS of its own)
//   visit(i)                         candidate i survived and is about to sweep the later ones
//   suppress(j, jx1, jy1, jx2, jy2)  by the thread that marks candidate j dead; j dies here and nowhere else
//   settle(i, ix1, iy1, ix2, iy2)    after the barrier that ends keeper i's sweep; candidate i is never read again
// Hooks record keepers in L.keep[L.ctl[5]++]; the count is returned.
// --------------------------------------------------------------------------------------------------------------------
template <typename Hook>
__device__ __forceinline__ int box_greedy_nms(const BoxLds& L, int K, double thr, Hook& hook) {
  const int tid = threadIdx.x;
  for (int i = tid; i < K; i += BOX_THREADS) {
    L.order[box_rank(L.key, K, i)] = i;
    if (L.area) L.area[i] = (L.x2[i] - L.x1[i]) * (L.y2[i] - L.y1[i]);
  }
  for (int i = tid; i < K; i += BOX_THREADS) L.dead[i] = 0;
  if (tid == 0) L.ctl[5] = 0;
  hook.begin();
  __syncthreads();
  for (int a = 0; a < K; ++a) {
    if (L.dead[a]) continue;                 // uniform: written before the last barrier
    const int i = L.order[a];
    hook.visit(i);
    const float ix1 = L.x1[i], iy1 = L.y1[i], ix2 = L.x2[i], iy2 = L.y2[i];
    const float ia = L.area ? L.area[i] : (ix2 - ix1) * (iy2 - iy1);
    for (int b = a + 1 + tid; b < K; b += BOX_THREADS) {
      if (L.dead[b]) continue;
      const int j = L.order[b];
      const float jx1 = L.x1[j], jy1 = L.y1[j], jx2 = L.x2[j], jy2 = L.y2[j];
      const float ja = L.area ? L.area[j] : (jx2 - jx1) * (jy2 - jy1);
      if ((double)box_overlap(ix1, iy1, ix2, iy2, ia, jx1, jy1, jx2, jy2, ja) > thr) {
        L.dead[b] = 1;
        hook.suppress(j, jx1, jy1, jx2, jy2);
      }
    }
    __syncthreads();
    hook.settle(i, ix1, iy1, ix2, iy2);
  }
  __syncthreads();
  return L.ctl[5];
}

// The hook of plain NMS: every survivor is kept, in visiting order.
struct KeepEvery {
  const BoxLds& L;
  __device__ __forceinline__ void begin() const {}
  __device__ __forceinline__ void visit(int i) const {
    if (threadIdx.x == 0) { L.keep[L.ctl[5]] = i; L.ctl[5] += 1; }
  }
  __device__ __forceinline__ void suppress(int, float, float, float, float) const {}
  __device__ __forceinline__ void settle(int, float, float, float, float) const {}
};

}  // namespace fdet
