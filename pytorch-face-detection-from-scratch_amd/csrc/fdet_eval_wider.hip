// WIDER Face protocol evaluation of one batch (gfx950): Easy / Medium / Hard style subsets with ignored boxes, inclusive
// (+1) pixel overlap in source pixels, min-max normalised scores cut at n_bins thresholds.  Declared in include/fdet.h
// (fdet_eval_wider); tests/wider_cpu_ref.py restates it as the protocol's sequential loop.
//
// One workgroup per image.  The candidate of a detection (arg-max overlap over ALL boxes, ignored ones included) does not
// depend on the subset or on what was recalled before, so the protocol's serial walk is not needed:
//   1. every detection gets its rank (as in fdet_eval_match), its candidate, whether the overlap reaches the threshold,
//      the candidate's subset mask and the bin of its normalised score;
//   2. winner[box] = min rank over the detections that reach the threshold on it (LDS atomicMin): the detection that
//      recalls the box first, the same for every subset that keeps the box;
//   3. per subset: a detection whose candidate is reached but not kept vanishes, every other one is a proposal, a winner
//      on a kept box is a hit; both are counted per bin in LDS and the non-zero bins added to the global histograms.
// The cumulative sums of the two histograms over bins <= t are the protocol's (proposals, recalled boxes) at threshold t.
//
// Overlaps are fp64 with a fixed operation order; contraction is off for the whole file (and in the Makefile).
#include "fdet_boxes.h"
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

using namespace fdet;

namespace {

constexpr int WIDER_THREADS = 256;
constexpr uint32_t NO_BIN = 0xFFFFu;

// LDS: score, rank, candidate, (bin | mask << 16) per detection slot; the winner table; the proposal and hit bins
__host__ __device__ inline size_t wider_lds_bytes(int Kmax, int max_gt, int n_bins) {
  return ((size_t)Kmax * 4 + (size_t)max_gt + (size_t)n_bins * 2) * 4;
}

// the smallest t in 0..n_bins-1 with n >= 1.0 - (double)(t+1)/n_bins, or NO_BIN.  The right side does not increase with t
// (division and subtraction round monotonically), so the exact expression can be bisected.
__device__ __forceinline__ uint32_t wider_bin(double n, int n_bins) {
  const double nb = (double)n_bins;
  if (!(n >= 1.0 - (double)n_bins / nb)) return NO_BIN;      // below the last threshold, or NaN
  int lo = 0, hi = n_bins - 1;                                // invariant: the predicate holds at hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (n >= 1.0 - (double)(mid + 1) / nb) hi = mid; else lo = mid + 1;
  }
  return (uint32_t)lo;
}

__global__ void __launch_bounds__(WIDER_THREADS)
k_eval_wider(const float* __restrict__ pred, const int32_t* __restrict__ pred_counts, int Kmax,
             const float* __restrict__ pred_scale, const float* __restrict__ gt_rows,
             const int32_t* __restrict__ gt_offset, int gt_cap, const uint32_t* __restrict__ gt_subsets, int n_subsets,
             int max_gt, double iou_threshold, const double* __restrict__ score_norm, int n_bins,
             uint32_t* __restrict__ proposals, uint32_t* __restrict__ hits, unsigned long long* __restrict__ counters) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* sc = reinterpret_cast<float*>(smem);
  uint32_t* rk = reinterpret_cast<uint32_t*>(sc + Kmax);
  int32_t* bi = reinterpret_cast<int32_t*>(rk + Kmax);       // (candidate << 1) | reached, or -1 without a candidate
  uint32_t* bm = reinterpret_cast<uint32_t*>(bi + Kmax);     // bin | candidate's subset mask << 16
  uint32_t* winner = bm + Kmax;
  uint32_t* hpr = winner + max_gt;
  uint32_t* hhi = hpr + n_bins;
  __shared__ uint32_t kept[FDET_EVAL_WIDER_MAX_SUBSETS];

  const int n = blockIdx.x, tid = threadIdx.x;
  const int K = pred_counts[n];
  const int g0 = gt_offset[n], g1 = gt_offset[n + 1];
  const int G = g1 - g0;
  // an image this launch cannot hold is counted and left out altogether (never evaluated on a part of its rows)
  if (K < 0 || K > Kmax || g0 < 0 || G < 0 || g1 > gt_cap || G > max_gt) {
    if (tid == 0) atomicAdd(&counters[n_subsets + FDET_EVAL_WIDER_N_REJECTED], 1ull);
    return;
  }
  const float* P = pred + (size_t)n * Kmax * 5;
  const float sx = pred_scale ? pred_scale[n * 2] : 1.f, sy = pred_scale ? pred_scale[n * 2 + 1] : 1.f;
  const double smin = score_norm ? score_norm[0] : 0.0, srange = score_norm ? score_norm[1] : 1.0;
  const uint32_t all = n_subsets >= 32 ? 0xFFFFFFFFu : ((1u << n_subsets) - 1u);
  for (int d = tid; d < K; d += WIDER_THREADS) sc[d] = nan_last_key(P[d * 5]);
  for (int g = tid; g < G; g += WIDER_THREADS) winner[g] = 0xFFFFFFFFu;
  if (tid < FDET_EVAL_WIDER_MAX_SUBSETS) kept[tid] = 0u;
  __syncthreads();

  {                                                    // boxes kept per subset
    uint32_t c[FDET_EVAL_WIDER_MAX_SUBSETS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int g = tid; g < G; g += WIDER_THREADS) {
      const uint32_t m = gt_subsets[g0 + g] & all;
#pragma unroll
      for (int s = 0; s < FDET_EVAL_WIDER_MAX_SUBSETS; ++s) c[s] += (m >> s) & 1u;
    }
#pragma unroll
    for (int s = 0; s < FDET_EVAL_WIDER_MAX_SUBSETS; ++s)
      if (c[s]) atomicAdd(&kept[s], c[s]);
  }

  for (int d = tid; d < K; d += WIDER_THREADS) {
    const uint32_t r = (uint32_t)box_rank(sc, K, d);
    // source pixels: four fp32 multiplies, everything after them in fp64
    const float fx = P[d * 5 + 1] * sx, fy = P[d * 5 + 2] * sy, fw = P[d * 5 + 3] * sx, fh = P[d * 5 + 4] * sy;
    const double dx1 = (double)fx, dy1 = (double)fy, dx2 = dx1 + (double)fw, dy2 = dy1 + (double)fh;
    const double ad = (dx2 - dx1 + 1.0) * (dy2 - dy1 + 1.0);
    double best = -INFINITY;
    int bidx = -1;
    for (int g = 0; g < G; ++g) {
      const float* ga = gt_rows + (size_t)(g0 + g) * 5;
      const double gx1 = (double)ga[1], gy1 = (double)ga[2], gx2 = gx1 + (double)ga[3], gy2 = gy1 + (double)ga[4];
      const double ag = (gx2 - gx1 + 1.0) * (gy2 - gy1 + 1.0);
      const double iw = (dx2 < gx2 ? dx2 : gx2) - (dx1 > gx1 ? dx1 : gx1) + 1.0;
      const double ih = (dy2 < gy2 ? dy2 : gy2) - (dy1 > gy1 ? dy1 : gy1) + 1.0;
      double ov = 0.0;
      if (iw > 0.0 && ih > 0.0) {
        const double inter = iw * ih;
        ov = inter / (ad + ag - inter);
      }
      if (ov > best) { best = ov; bidx = g; }          // strict: lowest row on ties, a NaN never wins
    }
    const bool reached = bidx >= 0 && best >= iou_threshold;
    const uint32_t mask = bidx >= 0 ? (gt_subsets[g0 + bidx] & all) : 0u;
    const double nrm = ((double)P[d * 5] - smin) / srange;
    rk[d] = r;
    bi[d] = bidx >= 0 ? ((bidx << 1) | (reached ? 1 : 0)) : -1;
    bm[d] = wider_bin(nrm, n_bins) | (mask << 16);
    if (reached) atomicMin(&winner[bidx], r);
  }

  for (int s = 0; s < n_subsets; ++s) {
    for (int b = tid; b < 2 * n_bins; b += WIDER_THREADS) hpr[b] = 0u;     // hpr and hhi are contiguous
    __syncthreads();                                   // (also orders rk/bi/bm and the winners on the first pass)
    for (int d = tid; d < K; d += WIDER_THREADS) {
      const uint32_t bin = bm[d] & 0xFFFFu;
      if (bin == NO_BIN) continue;
      const int c = bi[d];
      const bool reached = c >= 0 && (c & 1);
      const bool keep = (bm[d] >> (16 + s)) & 1u;
      if (reached && !keep) continue;                  // landed on an ignored box: neither a proposal nor a miss
      atomicAdd(&hpr[bin], 1u);
      if (reached && winner[c >> 1] == rk[d]) atomicAdd(&hhi[bin], 1u);
    }
    __syncthreads();
    for (int b = tid; b < 2 * n_bins; b += WIDER_THREADS) {
      const uint32_t c = hpr[b];
      if (c) atomicAdd(b < n_bins ? &proposals[(size_t)s * n_bins + b] : &hits[(size_t)s * n_bins + (b - n_bins)], c);
    }
    __syncthreads();                                   // the flush reads before the next pass clears
  }
  if (tid < n_subsets && kept[tid]) atomicAdd(&counters[tid], (unsigned long long)kept[tid]);
  if (tid == 0) {
    atomicAdd(&counters[n_subsets + FDET_EVAL_WIDER_N_IMAGES], 1ull);
    atomicAdd(&counters[n_subsets + FDET_EVAL_WIDER_N_DET], (unsigned long long)K);
  }
}

}  // namespace

extern "C" int fdet_eval_wider(const float* pred, const int32_t* pred_counts, int B, int Kmax, const float* pred_scale,
                               const float* gt_rows, const int32_t* gt_offset, int gt_cap, const uint32_t* gt_subsets,
                               int n_subsets, int max_gt, double iou_threshold, const double* score_norm, int n_bins,
                               uint32_t* proposals, uint32_t* hits, uint64_t* counters, void* stream) {
  FDET_REQUIRE(n_subsets >= 1 && n_subsets <= FDET_EVAL_WIDER_MAX_SUBSETS, "eval_wider: n_subsets=%d, 1..%d are supported",
               n_subsets, FDET_EVAL_WIDER_MAX_SUBSETS);
  FDET_REQUIRE(Kmax >= 1 && Kmax <= FDET_EVAL_MAX_DET,
               "eval_wider: Kmax=%d detections per image, 1..%d are supported (16 bytes of LDS each)", Kmax, FDET_EVAL_MAX_DET);
  FDET_REQUIRE(max_gt >= 1 && max_gt <= FDET_EVAL_MAX_GT,
               "eval_wider: max_gt=%d boxes per image, 1..%d are supported", max_gt, FDET_EVAL_MAX_GT);
  FDET_REQUIRE(n_bins >= 1 && n_bins <= FDET_EVAL_MAX_BINS, "eval_wider: n_bins=%d, 1..%d are supported", n_bins,
               FDET_EVAL_MAX_BINS);
  FDET_REQUIRE(B > 0 && gt_cap > 0, "eval_wider: B=%d and gt_cap=%d must be positive", B, gt_cap);
  FDET_REQUIRE(iou_threshold == iou_threshold, "eval_wider: iou_threshold is NaN");
  FDET_REQUIRE(pred && pred_counts && gt_rows && gt_offset && gt_subsets && proposals && hits && counters,
               "eval_wider: null argument");
  const size_t lds = wider_lds_bytes(Kmax, max_gt, n_bins);
  if (lds > 48 * 1024)
    if (int rc = set_lds_attr((const void*)k_eval_wider, lds, "eval_wider")) return rc;
  hipLaunchKernelGGL(k_eval_wider, dim3(B), dim3(WIDER_THREADS), lds, (hipStream_t)stream, pred, pred_counts, Kmax,
                     pred_scale, gt_rows, gt_offset, gt_cap, gt_subsets, n_subsets, max_gt, iou_threshold, score_norm,
                     n_bins, proposals, hits, reinterpret_cast<unsigned long long*>(counters));
  return check_launch("fdet_eval_wider");
}
