// SSD detection math (BASELINE.json config 4: "anchor match + hard-neg mining")
//   multi-scale target encode   datasets/WIDERFace/dataset_ssd.py:36-76,134-139
//   ssd_loss + hard negative mining (+ autograd)   losses/SSDLoss.py:7-86, models/ModelMetaSSD.py:127-129
//   ReduceSSDBoundingBoxes      datasets/utils.py:8-92
//   head pack                   models/SSD.py:206-240
// Priors are ordered (scale, i, j); P = sum ps^2 (4774 for 60/30/15/7).
// Built with -ffp-contract=off: the reducer's boxes and keep lists are compared BIT-EXACTLY with the reference's CPU
// arithmetic (separate mul and add, IEEE division), so no FMA contraction is allowed in this file.
#include "fdet_boxes.h"
#include <cfloat>
#include <cmath>

using namespace fdet;

constexpr int SSD_MAXS = 8;
struct SsdScales { int n; int ps[SSD_MAXS]; int start[SSD_MAXS + 1]; };

__global__ void __launch_bounds__(256)
k_ssd_encode(const float* __restrict__ boxes, const int32_t* __restrict__ offs, const SsdScales sc, float fw, float fh,
             float* __restrict__ out) {
  const int n = blockIdx.x, P = sc.start[sc.n];
  float* o = out + (size_t)n * P * 5;
  for (int t = threadIdx.x; t < P * 5; t += blockDim.x) o[t] = 0.f;
  __syncthreads();
  if (threadIdx.x < sc.n) {                                          // one thread per scale: later boxes overwrite
    const int ps = sc.ps[threadIdx.x];
    const float xps = (float)(1.0 / ps);                             // python float 1/ps, used as an fp32 scalar
    const float dconf = (float)(0.001 * ps);
    for (int k = offs[n]; k < offs[n + 1]; ++k) {
      const float* b = boxes + (size_t)k * 5;
      const float xn = b[1] / fw, yn = b[2] / fh, wn = b[3] / fw, hn = b[4] / fh;   // :44-45
      int i = (int)floor((double)(xn / xps)), j = (int)floor((double)(yn / xps));  // :54
      float v1 = xn - (float)((double)i * (1.0 / ps));               // :65
      float v2 = yn - (float)((double)j * (1.0 / ps));
      v1 = v1 / xps; v2 = v2 / xps;                                  // :69-70
      i = min(max(i, 0), ps - 1); j = min(max(j, 0), ps - 1);        // :75-76
      float* d = o + (size_t)(sc.start[threadIdx.x] + i * ps + j) * 5;
      d[0] = b[0] - dconf; d[1] = v1; d[2] = v2; d[3] = wn; d[4] = hn;
    }
  }
}

// one workgroup per image: mining mask, loss partials, un-normalised gradients
__global__ void __launch_bounds__(256)
k_ssd_loss_image(const float* __restrict__ pred, const float* __restrict__ tgt, int P, int ratio,
                 float* __restrict__ grad, unsigned char* __restrict__ mask_out, double* __restrict__ part /*[B][3]*/) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_loss = reinterpret_cast<float*>(smem);                    // -log(conf); -inf for positives
  __shared__ double s_red[3][4];
  __shared__ int s_npos;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* pr = pred + (size_t)n * P * 5;
  const float* tg = tgt + (size_t)n * P * 5;
  if (tid == 0) s_npos = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < P; i += 256) {
    const bool pos = tg[(size_t)i * 5] > 0.f;                        // SSDLoss.py:39
    cnt += pos;
    s_loss[i] = pos ? -INFINITY : -logf(pr[(size_t)i * 5]);          // :45, :68
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) atomicAdd(&s_npos, cnt);
  __syncthreads();
  const int npos = s_npos;
  const long long nneg = (long long)npos * ratio;                    // :43
  // ---- the nneg largest losses among the negatives (descending sort, ties: lower index first;
  //      :46-52) by radix select on the order-preserving integer image of the floats: four 8-bit
  //      passes find the threshold key T, then keys > T are in and keys == T fill the rest in index order
  const int P_neg = P - npos;
  const long long kk = nneg < (long long)P_neg ? nneg : (long long)P_neg;   // negatives to keep
  __shared__ int s_hist[256];
  __shared__ unsigned s_prefix, s_mask;
  __shared__ int s_want, s_tie[5];                                   // s_tie: the control words of compact_slot
  auto key_of = [&](int i) -> unsigned {
    const unsigned b = __float_as_uint(s_loss[i]);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);               // monotone: larger float -> larger key
  };
  if (tid == 0) { s_prefix = 0u; s_mask = 0u; s_want = (int)kk; s_tie[0] = 0; }
  __syncthreads();
  if (kk > 0 && kk < P_neg) {
    for (int pass = 3; pass >= 0; --pass) {
      for (int t = tid; t < 256; t += 256) s_hist[t] = 0;
      __syncthreads();
      const unsigned prefix = s_prefix, msk = s_mask;
      for (int i = tid; i < P; i += 256) {
        if (s_loss[i] == -INFINITY && tg[(size_t)i * 5] > 0.f) continue;         // positives are not candidates
        const unsigned k = key_of(i);
        if ((k & msk) == prefix) atomicAdd(&s_hist[(k >> (8 * pass)) & 255u], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int want = s_want, b = 255;
        for (; b > 0; --b) { if (s_hist[b] >= want) break; want -= s_hist[b]; }
        s_want = want;                                               // rank inside the chosen bin (1-based count still to take)
        s_prefix = prefix | ((unsigned)b << (8 * pass));
        s_mask = msk | (0xFFu << (8 * pass));
      }
      __syncthreads();
    }
  }
  const unsigned Tkey = s_prefix;                                    // threshold key (valid when 0 < kk < P_neg)
  const int ties_to_take = s_want;                                   // how many keys == T are kept (lowest indices)
  __syncthreads();
  double bce = 0.0, sl1 = 0.0;
  for (int i0 = 0; i0 < P; i0 += 256) {
    const int i = i0 + tid;
    const bool inb = i < P;
    const float label = inb ? tg[(size_t)i * 5] : 0.f;
    const bool pos = inb && label > 0.f;
    bool sel = pos;
    bool tie = false;
    if (inb && !pos) {
      if (kk >= P_neg) sel = kk > 0;
      else if (kk > 0) { const unsigned k = key_of(i); sel = k > Tkey; tie = k == Tkey; }
    }
    // ordered count of the ties (index order = thread order inside the sweep): the lowest indices are taken
    const int tie_rank = compact_slot(tie, s_tie);
    if (tie) sel = tie_rank < ties_to_take;
    if (!inb) continue;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, g4 = 0.f;
    if (sel) {
      const float c0 = pr[(size_t)i * 5];
      const float lo = 1e-7f, hi = 1.f - 1e-7f;                      // 10**-7 as an fp32 scalar (:13-14)
      const float c = fminf(fmaxf(c0, lo), hi);
      const float lr = rintf(label);                                 // :72
      bce += (double)(-1.f * (lr * logf(c) + (1.f - lr) * logf(1.f - c)));
      if (c0 >= lo && c0 <= hi) g0 = -(lr / c) + (1.f - lr) / (1.f - c);
    }
    if (pos) {
      const float* pl = pr + (size_t)i * 5 + 1;
      const float* gl = tg + (size_t)i * 5 + 1;
      float gg[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = pl[k] - gl[k], ad = fabsf(d);
        sl1 += ad < 1.f ? (double)(0.5f * d * d) : (double)(ad - 0.5f);           // F.smooth_l1_loss, beta = 1
        gg[k] = ad < 1.f ? d : (d > 0.f ? 1.f : -1.f);
      }
      g1 = gg[0]; g2 = gg[1]; g3 = gg[2]; g4 = gg[3];
    }
    if (grad) {
      float* go = grad + ((size_t)n * P + i) * 5;
      go[0] = g0; go[1] = g1; go[2] = g2; go[3] = g3; go[4] = g4;
    }
    if (mask_out) mask_out[(size_t)n * P + i] = sel ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) { bce += __shfl_down(bce, off, 64); sl1 += __shfl_down(sl1, off, 64); }
  if (lane == 0) { s_red[0][wid] = bce; s_red[1][wid] = sl1; }
  __syncthreads();
  if (tid == 0) {
    part[(size_t)n * 3 + 0] = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
    part[(size_t)n * 3 + 1] = ((s_red[1][0] + s_red[1][1]) + s_red[1][2]) + s_red[1][3];
    part[(size_t)n * 3 + 2] = (double)npos;
  }
}

__global__ void __launch_bounds__(64)
k_ssd_loss_total(const double* __restrict__ part, int B, float* __restrict__ loss, float* __restrict__ inv_npos) {
  if (threadIdx.x == 0) {
    double bce = 0.0, sl1 = 0.0, np = 0.0;
    for (int n = 0; n < B; ++n) { bce += part[n * 3]; sl1 += part[n * 3 + 1]; np += part[n * 3 + 2]; }
    loss[0] = (float)((sl1 + bce) / np);                             // :86 (0/0 = NaN as in the reference)
    // no positive in the batch: nothing was selected, every unscaled gradient is 0 and autograd leaves it 0
    // (the 1/0 of :86 never reaches an unselected element), so the scale must not turn 0 into 0 * inf = NaN
    inv_npos[0] = np > 0.0 ? (float)(1.0 / np) : 0.f;
  }
}

// data-parallel form: the three batch sums (BCE, smooth-L1, positive priors) of THIS shard, fixed order, fp64
__global__ void __launch_bounds__(64)
k_ssd_loss_sums(const double* __restrict__ part, int B, double* __restrict__ sums) {
  if (threadIdx.x == 0) {
    double bce = 0.0, sl1 = 0.0, np = 0.0;
    for (int n = 0; n < B; ++n) { bce += part[n * 3]; sl1 += part[n * 3 + 1]; np += part[n * 3 + 2]; }
    sums[0] = bce; sums[1] = sl1; sums[2] = np;
  }
}
__global__ void __launch_bounds__(64)
k_ssd_loss_finish(const double* __restrict__ sums, float* __restrict__ loss, float* __restrict__ inv_npos) {
  if (threadIdx.x == 0) {
    loss[0] = (float)((sums[1] + sums[0]) / sums[2]);                  // :86 with the batch-wide sums
    inv_npos[0] = sums[2] > 0.0 ? (float)(1.0 / sums[2]) : 0.f;         // as k_ssd_loss_total: zero gradients stay zero
  }
}

__global__ void __launch_bounds__(256)
k_ssd_scale_grad(float* __restrict__ grad, size_t n, const float* __restrict__ inv_npos) {
  const float s = inv_npos[0];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) grad[i] *= s;
}

// one workgroup per image: decode with priors -> threshold -> round -> greedy NMS -> xywh
__global__ void __launch_bounds__(256)
k_ssd_reduce(const float* __restrict__ x, const SsdScales sc, int with_priors, const float* __restrict__ priors, float pt,
             double thr, float fw, float fh, float* __restrict__ out, int32_t* __restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = blockIdx.x, P = sc.start[sc.n];
  const BoxLds L = box_carve(smem, P, true, true);
  const float* m = x + (size_t)n * P * 5;
  const int tid = threadIdx.x;
  if (tid == 0) L.ctl[0] = 0;
  __syncthreads();
  for (int c0 = 0; c0 < P; c0 += 256) {                               // ordered compaction (utils.py:54-59)
    const int c = c0 + tid;
    const bool hit = (c < P) && (m[(size_t)c * 5] > pt);
    const int k = compact_slot(hit, L.ctl);
    if (hit) {
      int s_ = 0;
      while (s_ + 1 < sc.n && c >= sc.start[s_ + 1]) ++s_;
      const int ps = sc.ps[s_], loc = c - sc.start[s_];
      const int i = loc / ps, j = loc - i * ps;
      const float* r = m + (size_t)c * 5;
      float v1 = r[1], v2 = r[2], v3 = r[3], v4 = r[4];
      if (with_priors) {                                             // :63-68
        const float mult = (float)(1.0 / ps);
        v1 = v1 * mult; v2 = v2 * mult;
        if (priors) {                                                // a caller-supplied (P,4) prior table (:31-32): added to all of x, y, w, h
          const float* pr = priors + (size_t)c * 4;
          v1 = v1 + pr[0]; v2 = v2 + pr[1]; v3 = v3 + pr[2]; v4 = v4 + pr[3];
        } else {                                                     // calculate_priors (:36-48): (i / ps, j / ps, 0, 0)
          v1 = v1 + (float)i * mult; v2 = v2 + (float)j * mult;
        }
      }
      const float X = v1 * fw, Y = v2 * fh, Wd = v3 * fw, Hd = v4 * fh;           // :69-70 (width, height as named there)
      const float X2 = Wd + X, Y2 = Hd + Y;                          // :79-80
      L.key[k] = r[0];
      L.x1[k] = rintf(X); L.y1[k] = rintf(Y); L.x2[k] = rintf(X2); L.y2[k] = rintf(Y2);   // :84
    }
  }
  __syncthreads();
  KeepEvery every{L};
  const int nk = box_greedy_nms(L, L.ctl[0], thr, every);
  for (int k = tid; k < nk; k += blockDim.x) {
    const int i = L.keep[k];
    float* o = out + ((size_t)n * P + k) * 5;
    o[0] = L.key[i]; o[1] = L.x1[i]; o[2] = L.y1[i];
    o[3] = L.x2[i] - L.x1[i];                                        // :73-74
    o[4] = L.y2[i] - L.y1[i];
  }
  if (tid == 0) out_counts[n] = nk;
}

static int ssd_scales(const int* h_ps, int ns, SsdScales& sc) {
  if (!h_ps || ns < 1 || ns > SSD_MAXS) return fail(FDET_EINVAL, "ssd: 1..%d patch sizes (got %d)", SSD_MAXS, ns);
  sc.n = ns; sc.start[0] = 0;
  for (int s = 0; s < ns; ++s) {
    if (h_ps[s] < 1 || h_ps[s] > 1024) return fail(FDET_EINVAL, "ssd: bad patch size %d", h_ps[s]);
    sc.ps[s] = h_ps[s]; sc.start[s + 1] = sc.start[s] + h_ps[s] * h_ps[s];
  }
  return FDET_OK;
}

extern "C" int fdet_ssd_num_priors(const int* h_patch_sizes, int nscales) {
  SsdScales sc{};
  if (ssd_scales(h_patch_sizes, nscales, sc)) return -1;
  return sc.start[sc.n];
}

extern "C" int fdet_ssd_encode_targets(const float* boxes, const int32_t* box_offsets, int B, const int* h_patch_sizes,
                                       int nscales, float img_w, float img_h, float* out, void* stream) {
  FDET_REQUIRE(boxes && box_offsets && out && B > 0 && img_w > 0 && img_h > 0, "ssd_encode_targets: bad arguments");
  SsdScales sc{};
  if (int rc = ssd_scales(h_patch_sizes, nscales, sc)) return rc;
  hipLaunchKernelGGL(k_ssd_encode, dim3(B), dim3(256), 0, (hipStream_t)stream, boxes, box_offsets, sc, img_w, img_h, out);
  return check_launch("fdet_ssd_encode_targets");
}

extern "C" size_t fdet_ssd_loss_ws_bytes(int B) { return B > 0 ? (size_t)B * 3 * sizeof(double) + 16 : 0; }

extern "C" int fdet_ssd_loss_fwd_bwd(const float* pred, const float* target, int B, int P, int neg_pos_ratio, float* loss,
                                     float* grad, uint8_t* mask, void* ws, size_t ws_bytes, void* stream) {
  FDET_REQUIRE(pred && target && loss && ws && B > 0 && P > 0 && neg_pos_ratio >= 0, "ssd_loss_fwd_bwd: bad arguments");
  FDET_REQUIRE((size_t)P * 4 <= 150 * 1024, "ssd_loss_fwd_bwd: P=%d priors exceed the LDS tile", P);
  if (ws_bytes < fdet_ssd_loss_ws_bytes(B)) return fail(FDET_EWORKSPACE, "ssd_loss_fwd_bwd: workspace %zu < %zu bytes", ws_bytes, fdet_ssd_loss_ws_bytes(B));
  double* part = (double*)ws;
  float* inv = (float*)(part + (size_t)B * 3);
  const size_t lds = (size_t)P * 4;
  if (lds > 64 * 1024)
    if (int rc = set_lds_attr((const void*)k_ssd_loss_image, lds, "ssd_loss_fwd_bwd")) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ssd_loss_image, dim3(B), dim3(256), lds, st, pred, target, P, neg_pos_ratio, grad, mask, part);
  if (int rc = check_launch("fdet_ssd_loss_fwd_bwd")) return rc;
  hipLaunchKernelGGL(k_ssd_loss_total, dim3(1), dim3(64), 0, st, part, B, loss, inv);
  if (grad) {
    const size_t n = (size_t)B * P * 5;
    size_t blocks = (n + 255) / 256; if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_ssd_scale_grad, dim3((unsigned)blocks), dim3(256), 0, st, grad, n, inv);
  }
  return check_launch("fdet_ssd_loss_fwd_bwd(total)");
}

extern "C" int fdet_ssd_loss_parts(const float* pred, const float* target, int B, int P, int neg_pos_ratio, float* grad,
                                   uint8_t* mask, double* sums, void* ws, size_t ws_bytes, void* stream) {
  FDET_REQUIRE(pred && target && sums && ws && B > 0 && P > 0 && neg_pos_ratio >= 0, "ssd_loss_parts: bad arguments");
  FDET_REQUIRE((size_t)P * 4 <= 150 * 1024, "ssd_loss_parts: P=%d priors exceed the LDS tile", P);
  if (ws_bytes < fdet_ssd_loss_ws_bytes(B)) return fail(FDET_EWORKSPACE, "ssd_loss_parts: workspace %zu < %zu bytes", ws_bytes, fdet_ssd_loss_ws_bytes(B));
  double* part = (double*)ws;
  const size_t lds = (size_t)P * 4;
  if (lds > 64 * 1024)
    if (int rc = set_lds_attr((const void*)k_ssd_loss_image, lds, "ssd_loss_parts")) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ssd_loss_image, dim3(B), dim3(256), lds, st, pred, target, P, neg_pos_ratio, grad, mask, part);
  if (int rc = check_launch("fdet_ssd_loss_parts")) return rc;
  hipLaunchKernelGGL(k_ssd_loss_sums, dim3(1), dim3(64), 0, st, part, B, sums);
  return check_launch("fdet_ssd_loss_parts(sums)");
}

extern "C" int fdet_ssd_loss_finish(const double* sums, float* loss, float* grad, size_t n_grad, void* ws, size_t ws_bytes,
                                    void* stream) {
  FDET_REQUIRE(sums && loss && ws && ws_bytes >= 16, "ssd_loss_finish: bad arguments (workspace of at least 16 bytes)");
  float* inv = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ssd_loss_finish, dim3(1), dim3(64), 0, st, sums, loss, inv);
  if (grad && n_grad) {
    size_t blocks = (n_grad + 255) / 256; if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_ssd_scale_grad, dim3((unsigned)blocks), dim3(256), 0, st, grad, n_grad, inv);
  }
  return check_launch("fdet_ssd_loss_finish");
}

// priors: NULL = the reference's calculate_priors(); else a device (P,4) table (ReduceSSDBoundingBoxes(priors=...), utils.py:31-32)
extern "C" int fdet_ssd_reduce_bounding_boxes_priors(const float* x, int B, const int* h_patch_sizes, int nscales, int with_priors,
                                                     const float* priors, float prob_threshold, double iou_threshold, float img_w,
                                                     float img_h, float* out, int32_t* out_counts, void* stream);
extern "C" int fdet_ssd_reduce_bounding_boxes(const float* x, int B, const int* h_patch_sizes, int nscales, int with_priors,
                                              float prob_threshold, double iou_threshold, float img_w, float img_h,
                                              float* out, int32_t* out_counts, void* stream) {
  return fdet_ssd_reduce_bounding_boxes_priors(x, B, h_patch_sizes, nscales, with_priors, nullptr, prob_threshold, iou_threshold, img_w,
                                               img_h, out, out_counts, stream);
}
extern "C" int fdet_ssd_reduce_bounding_boxes_priors(const float* x, int B, const int* h_patch_sizes, int nscales, int with_priors,
                                                     const float* priors, float prob_threshold, double iou_threshold, float img_w,
                                                     float img_h, float* out, int32_t* out_counts, void* stream) {
  FDET_REQUIRE(x && out && out_counts && B > 0, "ssd_reduce_bounding_boxes: bad arguments");
  SsdScales sc{};
  if (int rc = ssd_scales(h_patch_sizes, nscales, sc)) return rc;
  const int P = sc.start[sc.n];
  const size_t lds = box_lds_bytes(P, true);
  FDET_REQUIRE(lds <= 160 * 1024, "ssd_reduce_bounding_boxes: %d priors need %zu bytes of LDS (> 160 KB)", P, lds);
  if (lds > 64 * 1024)
    if (int rc = set_lds_attr((const void*)k_ssd_reduce, lds, "ssd_reduce_bounding_boxes")) return rc;
  hipLaunchKernelGGL(k_ssd_reduce, dim3(B), dim3(256), lds, (hipStream_t)stream, x, sc, with_priors, priors, prob_threshold,
                     iou_threshold, img_w, img_h, out, out_counts);
  return check_launch("fdet_ssd_reduce_bounding_boxes");
}

// SSD heads: z [N,CP,ps,ps] (channels 0..4 = Linear(C,5) on the NHWC map, models/SSD.py:233-238) ->
// rows prior_start + i*ps + j of y [N,P,5]: sigmoid on the score (:240), apply_priors (:206-218).
__global__ void __launch_bounds__(256)
k_ssd_head_pack_fwd(const float* __restrict__ z, int N, int CP, int ps, int prior_start, int P, float* __restrict__ y) {
  const int cells = ps * ps;
  const float mult = (float)(1.0 / ps);
  for (int t = blockIdx.x * 256 + threadIdx.x; t < N * cells; t += gridDim.x * 256) {
    const int n = t / cells, c = t - n * cells;
    const int i = c / ps, j = c - i * ps;
    const float* zp = z + (size_t)n * CP * cells + c;
    float* o = y + ((size_t)n * P + prior_start + c) * 5;
    o[0] = 1.f / (1.f + expf(-zp[0]));
    o[1] = zp[cells] * mult + (float)i * mult;
    o[2] = zp[2 * cells] * mult + (float)j * mult;
    o[3] = zp[3 * cells];
    o[4] = zp[4 * cells];
  }
}
__global__ void __launch_bounds__(256)
k_ssd_head_pack_bwd(const float* __restrict__ dy, const float* __restrict__ y, int N, int CP, int ps, int prior_start,
                    int P, float* __restrict__ dz) {
  const int cells = ps * ps;
  const float mult = (float)(1.0 / ps);
  for (int t = blockIdx.x * 256 + threadIdx.x; t < N * cells; t += gridDim.x * 256) {
    const int n = t / cells, c = t - n * cells;
    const float* g = dy + ((size_t)n * P + prior_start + c) * 5;
    const float s = y[((size_t)n * P + prior_start + c) * 5];
    float* d = dz + (size_t)n * CP * cells + c;
    d[0] = g[0] * (s * (1.f - s));
    d[cells] = g[1] * mult;
    d[2 * cells] = g[2] * mult;
    d[3 * cells] = g[3];
    d[4 * cells] = g[4];
    for (int k = 5; k < CP; ++k) d[(size_t)k * cells] = 0.f;
  }
}

extern "C" int fdet_ssd_head_pack_fwd(const float* z, int N, int CP, int ps, int prior_start, int P, float* y, void* stream) {
  FDET_REQUIRE(z && y && N > 0 && CP >= 5 && ps > 0 && prior_start >= 0 && prior_start + ps * ps <= P, "ssd_head_pack_fwd: bad arguments");
  const int total = N * ps * ps;
  hipLaunchKernelGGL(k_ssd_head_pack_fwd, dim3(min((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, z, N, CP, ps, prior_start, P, y);
  return check_launch("fdet_ssd_head_pack_fwd");
}
extern "C" int fdet_ssd_head_pack_bwd(const float* dy, const float* y, int N, int CP, int ps, int prior_start, int P, float* dz,
                                      void* stream) {
  FDET_REQUIRE(dy && y && dz && N > 0 && CP >= 5 && ps > 0 && prior_start >= 0 && prior_start + ps * ps <= P, "ssd_head_pack_bwd: bad arguments");
  const int total = N * ps * ps;
  hipLaunchKernelGGL(k_ssd_head_pack_bwd, dim3(min((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, dy, y, N, CP, ps, prior_start, P, dz);
  return check_launch("fdet_ssd_head_pack_bwd");
}
