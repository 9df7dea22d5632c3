// Dataset-level detection evaluation (gfx950): PASCAL VOC / WIDER Face matching of one batch, accumulated into
// per-(IoU threshold, score bin) true/false-positive histograms.  Declared in include/fdet.h (fdet_eval_match).
//
// One workgroup per image.  The rule -- detections in descending score, each one's candidate is the ground-truth box of
// highest IoU among ALL boxes of the image, true positive iff IoU >= threshold and the candidate is not yet claimed --
// has a candidate that does not depend on what was claimed, so no sequential sweep is needed:
//   1. every detection gets its rank (number of detections that precede it: higher score, or equal score and lower row)
//      and its arg-max box (fp32 box_iou of k_metrics, strict > so the lowest index wins ties and NaN never wins);
//   2. per threshold: winner[box] = min rank over the detections that claim it (LDS atomicMin); a detection is a true
//      positive iff it is that winner; the workgroup's tp/fp bins are counted in LDS and the non-zero ones added to the
//      global histograms with vector atomics.
#include "fdet_boxes.h"
#include <cfloat>
#include <cmath>

using namespace fdet;

namespace {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_MAX_T = FDET_EVAL_MAX_THRESHOLDS;

struct EvalThresholds { float v[EVAL_MAX_T]; };

// LDS: score, rank, best box, best IoU per detection slot; the winner table; the tp and fp bins of one threshold
__host__ __device__ inline size_t eval_lds_bytes(int Kmax, int max_gt, int n_bins) {
  return ((size_t)Kmax * 4 + (size_t)max_gt + (size_t)n_bins * 2) * 4;
}

__device__ __forceinline__ int eval_bin(float s, int n_bins) {
  const float v = s * (float)n_bins;
  if (!(v >= 0.f)) return 0;                         // negative (and -inf, which NaN was mapped to)
  if (v >= (float)n_bins) return n_bins - 1;
  return (int)floorf(v);
}

__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_match(const float* __restrict__ pred, const int32_t* __restrict__ pred_counts, int Kmax,
             const float* __restrict__ gt_rows, const int32_t* __restrict__ gt_offset, int gt_cap, int max_gt,
             EvalThresholds thr, int T, int n_bins, uint32_t* __restrict__ tp, uint32_t* __restrict__ fp,
             unsigned long long* __restrict__ counters, int32_t* __restrict__ match) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* sc = reinterpret_cast<float*>(smem);
  uint32_t* rk = reinterpret_cast<uint32_t*>(sc + Kmax);
  int32_t* bi = reinterpret_cast<int32_t*>(rk + Kmax);
  float* io = reinterpret_cast<float*>(bi + Kmax);
  uint32_t* winner = reinterpret_cast<uint32_t*>(io + Kmax);
  uint32_t* htp = winner + max_gt;
  uint32_t* hfp = htp + n_bins;

  const int n = blockIdx.x, tid = threadIdx.x;
  const int K = pred_counts[n];
  const int g0 = gt_offset[n], g1 = gt_offset[n + 1];
  const int G = g1 - g0;
  int32_t* mrow = match ? match + (size_t)n * Kmax : nullptr;
  // an image this launch cannot hold is counted and left out altogether (never evaluated on a part of its rows)
  if (K < 0 || K > Kmax || g0 < 0 || G < 0 || g1 > gt_cap || G > max_gt) {
    if (mrow) for (int d = tid; d < Kmax; d += EVAL_THREADS) mrow[d] = -1;
    if (tid == 0) atomicAdd(&counters[FDET_EVAL_N_REJECTED], 1ull);
    return;
  }
  const float* P = pred + (size_t)n * Kmax * 5;
  for (int d = tid; d < K; d += EVAL_THREADS) sc[d] = nan_last_key(P[d * 5]);
  for (int b = tid; b < 2 * n_bins; b += EVAL_THREADS) htp[b] = 0u;      // htp and hfp are contiguous
  __syncthreads();

  for (int d = tid; d < K; d += EVAL_THREADS) {
    const uint32_t r = (uint32_t)box_rank(sc, K, d);
    const float px1 = P[d * 5 + 1], py1 = P[d * 5 + 2], px2 = P[d * 5 + 3] + px1, py2 = P[d * 5 + 4] + py1;
    const float a2 = (px2 - px1) * (py2 - py1);
    float best = -INFINITY;
    int bidx = -1;
    for (int g = 0; g < G; ++g) {
      const float* ga = gt_rows + (size_t)(g0 + g) * 5;
      const float gx1 = ga[1], gy1 = ga[2], gx2 = ga[3] + ga[1], gy2 = ga[4] + ga[2];
      const float a1 = (gx2 - gx1) * (gy2 - gy1);
      const float iou = box_overlap(gx1, gy1, gx2, gy2, a1, px1, py1, px2, py2, a2);
      if (iou > best) { best = iou; bidx = g; }
    }
    rk[d] = r;
    bi[d] = bidx;
    io[d] = best;
  }

  for (int t = 0; t < T; ++t) {
    const float th = thr.v[t];
    for (int g = tid; g < G; g += EVAL_THREADS) winner[g] = 0xFFFFFFFFu;
    __syncthreads();                                   // (also orders rk/bi/io and the zeroed bins on the first pass)
    for (int d = tid; d < K; d += EVAL_THREADS)
      if (bi[d] >= 0 && io[d] >= th) atomicMin(&winner[bi[d]], rk[d]);
    __syncthreads();
    for (int d = tid; d < K; d += EVAL_THREADS) {
      const int b = bi[d];
      const bool hit = b >= 0 && io[d] >= th && winner[b] == rk[d];
      atomicAdd(hit ? &htp[eval_bin(sc[d], n_bins)] : &hfp[eval_bin(sc[d], n_bins)], 1u);
      if (t == 0 && mrow) mrow[d] = hit ? g0 + b : -1;
    }
    __syncthreads();
    for (int b = tid; b < 2 * n_bins; b += EVAL_THREADS) {
      const uint32_t c = htp[b];
      if (c) {
        atomicAdd(b < n_bins ? &tp[(size_t)t * n_bins + b] : &fp[(size_t)t * n_bins + (b - n_bins)], c);
        htp[b] = 0u;
      }
    }
    // the next pass's first barrier orders these clears before its bin adds
  }
  if (mrow) for (int d = K + tid; d < Kmax; d += EVAL_THREADS) mrow[d] = -1;
  if (tid == 0) {
    atomicAdd(&counters[FDET_EVAL_N_GT], (unsigned long long)G);
    atomicAdd(&counters[FDET_EVAL_N_IMAGES], 1ull);
    atomicAdd(&counters[FDET_EVAL_N_DET], (unsigned long long)K);
  }
}

}  // namespace

extern "C" int fdet_eval_match(const float* pred, const int32_t* pred_counts, int B, int Kmax, const float* gt_rows,
                               const int32_t* gt_offset, int gt_cap, int max_gt, const float* iou_thresholds, int T,
                               int n_bins, uint32_t* tp, uint32_t* fp, uint64_t* counters, int32_t* match,
                               void* stream) {
  FDET_REQUIRE(pred && pred_counts && gt_rows && gt_offset && iou_thresholds && tp && fp && counters,
               "eval_match: null argument");
  FDET_REQUIRE(B > 0 && gt_cap > 0, "eval_match: B=%d and gt_cap=%d must be positive", B, gt_cap);
  FDET_REQUIRE(T >= 1 && T <= EVAL_MAX_T, "eval_match: T=%d IoU thresholds, 1..%d are supported", T, EVAL_MAX_T);
  FDET_REQUIRE(Kmax >= 1 && Kmax <= FDET_EVAL_MAX_DET,
               "eval_match: Kmax=%d detections per image, 1..%d are supported (16 bytes of LDS each)", Kmax, FDET_EVAL_MAX_DET);
  FDET_REQUIRE(max_gt >= 1 && max_gt <= FDET_EVAL_MAX_GT,
               "eval_match: max_gt=%d boxes per image, 1..%d are supported", max_gt, FDET_EVAL_MAX_GT);
  FDET_REQUIRE(n_bins >= 1 && n_bins <= FDET_EVAL_MAX_BINS, "eval_match: n_bins=%d, 1..%d are supported", n_bins,
               FDET_EVAL_MAX_BINS);
  EvalThresholds thr;
  for (int t = 0; t < EVAL_MAX_T; ++t) thr.v[t] = t < T ? iou_thresholds[t] : 2.f;
  const size_t lds = eval_lds_bytes(Kmax, max_gt, n_bins);
  if (lds > 48 * 1024)
    if (int rc = set_lds_attr((const void*)k_eval_match, lds, "eval_match")) return rc;
  hipLaunchKernelGGL(k_eval_match, dim3(B), dim3(EVAL_THREADS), lds, (hipStream_t)stream, pred, pred_counts, Kmax,
                     gt_rows, gt_offset, gt_cap, max_gt, thr, T, n_bins, tp, fp,
                     reinterpret_cast<unsigned long long*>(counters), match);
  return check_launch("fdet_eval_match");
}
