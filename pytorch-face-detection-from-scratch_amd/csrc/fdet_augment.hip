// On-device WIDER-Face training augmentation (datasets/WIDERFace/datamodule.py:105-134 of the reference: the albumentations
// training_transform / default_transform pipelines), on a ragged batch of HWC uint8 RGB images resident in device memory.
//
//   fdet_aug_warp    RandomResizedCrop + Resize + HorizontalFlip + Rotate(reflect-101) composed into ONE bilinear sample of the
//                    source per output pixel, then brightness/contrast (v*alpha + beta) and Gaussian noise on the interpolated
//                    fp32 value, one rint + clamp -> uint8 CHW intermediate (B,3,Ho,Wo)
//   fdet_aug_finish  GlassBlur (fast mode, one iteration, max_delta 1; the sigma=0.1 blurs are the identity on uint8) and
//                    MotionBlur (k x k line kernel, reflect-101) from an LDS tile with a 3-pixel halo -> final uint8 frame and
//                    its fp32 /255 image (bit-identical to fdet_u8_to_f32_norm)
//   fdet_aug_boxes   the same geometric chain on [conf,x,y,w,h] boxes, min_area filter, half-even rounding, per-image compaction
//                    into the flat rows + box_offset layout of fdet_encode_targets / fdet_ssd_encode_targets
//
// All per-image randomness is sampled on the host (fdet_amd/datasets/augment.py) except the per-pixel draws (noise, glass
// offsets), which come from a stateless hash of (seed, image key, tag, y, x): the result does not depend on launch geometry or
// on an image's position in the batch.  DESIGN.md "On-device augmentation" states the semantics; tests/aug_cpu_ref.py restates
// every kernel in numpy.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

constexpr uint32_t TAG_GLASS = 6;   // noise uses tags 2c, 2c+1 for channel c

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// murmur3's finaliser chained over the five words; tests/aug_cpu_ref.py:aug_hash restates it bit-exactly
__device__ __forceinline__ uint32_t aug_hash(uint32_t seed, uint32_t key, uint32_t tag, uint32_t y, uint32_t x) {
  uint32_t h = fmix32(seed ^ 0x9e3779b9u);
  h = fmix32(h ^ key);
  h = fmix32(h ^ tag);
  h = fmix32(h ^ y);
  return fmix32(h ^ x);
}

// standard normal by Box-Muller: u1 in (0,1], u2 in [0,1), 24 bits each
__device__ __forceinline__ float aug_normal(uint32_t seed, uint32_t key, int c, int y, int x) {
  const uint32_t h1 = aug_hash(seed, key, 2u * c, (uint32_t)y, (uint32_t)x);
  const uint32_t h2 = aug_hash(seed, key, 2u * c + 1u, (uint32_t)y, (uint32_t)x);
  const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(h2 >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// continuous reflect-101 of an index-space coordinate into [0, n-1]
__device__ __forceinline__ double reflect101d(double t, int n) {
  if (n == 1) return 0.0;
  const double p = 2.0 * (double)(n - 1);
  t = fabs(t);
  t = fmod(t, p);
  return t > (double)(n - 1) ? p - t : t;
}

// integer reflect-101 (cv2 BORDER_REFLECT_101) into [0, n-1]
__device__ __forceinline__ int reflect101i(int t, int n) {
  if (n == 1) return 0;
  while (t < 0 || t >= n) {
    if (t < 0) t = -t;
    if (t >= n) t = 2 * (n - 1) - t;
  }
  return t;
}

// ------------------------------------------------------------------------------------------------------------------
// (a) warp: one thread per 4 consecutive output pixels of a row, all three channels
// ------------------------------------------------------------------------------------------------------------------
constexpr int WARP_PX = 4;

__global__ void __launch_bounds__(256)
k_aug_warp(const uint8_t* __restrict__ bank, const fdet_aug_image* __restrict__ table, const fdet_aug_params* __restrict__ params,
           int Ho, int Wo, uint32_t seed, uint8_t* __restrict__ mid) {
  const int b = blockIdx.z;
  const int oy = blockIdx.y * blockDim.y + threadIdx.y;
  const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * WARP_PX;
  if (oy >= Ho || ox0 >= Wo) return;
  const fdet_aug_params& P = params[b];
  const fdet_aug_image img = table[P.image];
  const uint8_t* src = bank + img.offset;
  const int flags = P.flags;
  // Source coordinates in fp64 (a few operations per pixel in an HBM-bound kernel): an fp32 coordinate near x = 2000 carries
  // ~1e-4 px of rounding, enough to flip the final rounding of textured pixels; in fp64 the coordinate chain is the
  // restatement's own (tests/aug_cpu_ref.py:warp_values, same operation order) and only the interpolation is fp32.
  const double rw = (double)P.crop_w / (double)Wo, rh = (double)P.crop_h / (double)Ho;
  const int xlo = P.crop_x0, xhi = P.crop_x0 + P.crop_w - 1, ylo = P.crop_y0, yhi = P.crop_y0 + P.crop_h - 1;
  uint8_t res[3][WARP_PX];
#pragma unroll
  for (int i = 0; i < WARP_PX; ++i) {
    const int ox = min(ox0 + i, Wo - 1);          // tail lanes recompute the last pixel; only valid pixels are stored
    double u = (double)ox, v = (double)oy;
    if (flags & FDET_AUG_ROTATE) {                 // inverse rotation about (Wo/2, Ho/2) of the pixel centre
      const double c = (double)P.cos_a, s = (double)P.sin_a;
      const double dx = ((double)ox + 0.5) - (double)Wo / 2.0, dy = ((double)oy + 0.5) - (double)Ho / 2.0;
      u = reflect101d((double)Wo / 2.0 + (c * dx - s * dy) - 0.5, Wo);
      v = reflect101d((double)Ho / 2.0 + (s * dx + c * dy) - 0.5, Ho);
    }
    if (flags & FDET_AUG_FLIP) u = (double)(Wo - 1) - u;
    const double sx = (u + 0.5) * rw + (double)P.crop_x0 - 0.5;
    const double sy = (v + 0.5) * rh + (double)P.crop_y0 - 0.5;
    const double fx0 = floor(sx), fy0 = floor(sy);
    const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
    const int ix = (int)fx0, iy = (int)fy0;
    const int x0 = min(max(ix, xlo), xhi), x1 = min(max(ix + 1, xlo), xhi);
    const int y0 = min(max(iy, ylo), yhi), y1 = min(max(iy + 1, ylo), yhi);
    const uint8_t* r0 = src + ((int64_t)y0 * img.w) * 3;
    const uint8_t* r1 = src + ((int64_t)y1 * img.w) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = (float)r0[x0 * 3 + c], v01 = (float)r0[x1 * 3 + c];
      const float v10 = (float)r1[x0 * 3 + c], v11 = (float)r1[x1 * 3 + c];
      const float top = (1.f - fx) * v00 + fx * v01;
      const float bot = (1.f - fx) * v10 + fx * v11;
      float val = (1.f - fy) * top + fy * bot;
      if (flags & FDET_AUG_BRIGHTNESS) val = val * P.alpha + P.beta;
      if (flags & FDET_AUG_NOISE) val = val + P.sigma * aug_normal(seed, P.key, c, oy, ox);
      res[c][i] = (uint8_t)fminf(fmaxf(rintf(val), 0.f), 255.f);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint8_t* row = mid + (((int64_t)b * 3 + c) * Ho + oy) * Wo;
    if ((Wo % WARP_PX) == 0) {                     // ox0 + 3 < Wo and 4-byte aligned
      const uint32_t w = (uint32_t)res[c][0] | ((uint32_t)res[c][1] << 8) | ((uint32_t)res[c][2] << 16) | ((uint32_t)res[c][3] << 24);
      *reinterpret_cast<uint32_t*>(row + ox0) = w;
    } else {
#pragma unroll
      for (int i = 0; i < WARP_PX; ++i)
        if (ox0 + i < Wo) row[ox0 + i] = res[c][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// (b) glass + motion blur: 64 x 16 output tile per block, 16 x 16 threads of 4 pixels each, LDS tile with a 3-pixel halo
// ------------------------------------------------------------------------------------------------------------------
constexpr int FT_W = 64, FT_H = 16, HALO = 3;
constexpr int LT_W = FT_W + 2 * HALO, LT_H = FT_H + 2 * HALO;

// the glass-blurred value's source pixel for output pixel (qy, qx): albumentations 1.1.0 glass_blur(mode="fast"), one
// iteration: rows h = H-1..2, columns w = W-1..2, k = iw*len(hs) + ih; x1[p_k] = x0[p_k + d_k], then x1[p_k + d_k] = x0[p_k]
// (the largest k wins).  d in {-1,0}^2, so the writers of q are among q, q+(1,0), q+(0,1), q+(1,1).
__device__ __forceinline__ void glass_source(int qy, int qx, int H, int W, uint32_t seed, uint32_t key, int& sy, int& sx) {
  sy = qy;
  sx = qx;
  if (H < 3 || W < 3) return;
  long long best = -1;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const int ph = qy + a, pw = qx + bb;
      if (ph < 2 || ph > H - 1 || pw < 2 || pw > W - 1) continue;
      const uint32_t h = aug_hash(seed, key, TAG_GLASS, (uint32_t)ph, (uint32_t)pw);
      const int dy = -(int)(h & 1u), dx = -(int)((h >> 1) & 1u);
      if (a == 0 && bb == 0 && best < 0) {            // gather at q itself (overridden by any scatter)
        sy = qy + dy;
        sx = qx + dx;
      }
      if (ph + dy == qy && pw + dx == qx) {           // scatter from p into q
        const long long k = (long long)(W - 1 - pw) * (H - 2) + (H - 1 - ph);
        if (k > best) { best = k; sy = ph; sx = pw; }
      }
    }
  }
}

__global__ void __launch_bounds__(256)
k_aug_finish(const uint8_t* __restrict__ mid, const fdet_aug_params* __restrict__ params, int Ho, int Wo, uint32_t seed,
             uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
  __shared__ uint8_t tile[3][LT_H][LT_W];
  __shared__ float wts[49];
  const int b = blockIdx.z;
  const fdet_aug_params& P = params[b];
  const int flags = P.flags;
  const bool glass = (flags & FDET_AUG_GLASS) != 0, motion = (flags & FDET_AUG_MOTION) != 0;
  const int k = motion ? P.motion_k : 1;
  const int tx0 = blockIdx.x * FT_W, ty0 = blockIdx.y * FT_H;
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  const uint8_t* img = mid + (int64_t)b * 3 * Ho * Wo;
  const int64_t plane = (int64_t)Ho * Wo;
  if (!glass && !motion && (Wo % 4) == 0) {          // block-uniform: the frame is the intermediate, no tile needed
    const int oy = ty0 + threadIdx.y, ox0 = tx0 + threadIdx.x * 4;
    if (oy >= Ho || ox0 >= Wo) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t o = (int64_t)c * plane + (int64_t)oy * Wo + ox0;
      const uint32_t w = *reinterpret_cast<const uint32_t*>(img + o);
      const int64_t oo = (int64_t)b * 3 * plane + o;
      *reinterpret_cast<uint32_t*>(out_u8 + oo) = w;
      float4 f;
      f.x = u8_over_255((float)(w & 255u));
      f.y = u8_over_255((float)((w >> 8) & 255u));
      f.z = u8_over_255((float)((w >> 16) & 255u));
      f.w = u8_over_255((float)(w >> 24));
      *reinterpret_cast<float4*>(out_f32 + oo) = f;
    }
    return;
  }
  if (tid < 49) wts[tid] = tid < k * k ? P.motion_w[tid] : 0.f;
  for (int i = tid; i < LT_H * LT_W; i += 256) {
    const int ly = i / LT_W, lx = i - ly * LT_W;
    const int gy = reflect101i(ty0 + ly - HALO, Ho), gx = reflect101i(tx0 + lx - HALO, Wo);
    int sy = gy, sx = gx;
    if (glass) glass_source(gy, gx, Ho, Wo, seed, P.key, sy, sx);
    const int64_t o = (int64_t)sy * Wo + sx;
#pragma unroll
    for (int c = 0; c < 3; ++c) tile[c][ly][lx] = img[c * plane + o];
  }
  __syncthreads();
  const int oy = ty0 + threadIdx.y, ox0 = tx0 + threadIdx.x * 4;
  if (oy >= Ho || ox0 >= Wo) return;
  const int r = k / 2;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint8_t q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ly = threadIdx.y + HALO, lx = threadIdx.x * 4 + i + HALO;
      if (!motion) {
        q[i] = tile[c][ly][lx];
      } else {
        float acc = 0.f;
        for (int dy = 0; dy < k; ++dy)
          for (int dx = 0; dx < k; ++dx) acc = acc + wts[dy * k + dx] * (float)tile[c][ly + dy - r][lx + dx - r];
        q[i] = (uint8_t)fminf(fmaxf(rintf(acc), 0.f), 255.f);
      }
    }
    const int64_t o = ((int64_t)b * 3 + c) * plane + (int64_t)oy * Wo + ox0;
    if ((Wo % 4) == 0) {                              // ox0 + 3 < Wo; 4-byte aligned u8 and 16-byte aligned f32
      *reinterpret_cast<uint32_t*>(out_u8 + o) =
          (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
      float4 f;
      f.x = u8_over_255((float)q[0]);
      f.y = u8_over_255((float)q[1]);
      f.z = u8_over_255((float)q[2]);
      f.w = u8_over_255((float)q[3]);
      *reinterpret_cast<float4*>(out_f32 + o) = f;
    } else {
      for (int i = 0; i < 4; ++i)
        if (ox0 + i < Wo) {
          out_u8[o + i] = q[i];
          out_f32[o + i] = u8_over_255((float)q[i]);
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// (c) boxes: one block; thread t owns a contiguous run of images, counts survivors, block scan, then writes
// ------------------------------------------------------------------------------------------------------------------
constexpr int BOX_THREADS = 1024;

// transforms one [conf,x,y,w,h] row; false when it is dropped.  fp32 with no contraction: tests/aug_cpu_ref.py restates the
// same operation sequence in numpy float32, so rows compare exactly.
__device__ __forceinline__ bool box_transform(const float* in, const fdet_aug_params& P, const fdet_aug_image& img, int Ho, int Wo,
                                              float* out) {
  const float W = (float)img.w, H = (float)img.h;
  float x1 = fminf(fmaxf(in[1], 0.f), W), y1 = fminf(fmaxf(in[2], 0.f), H);
  float x2 = fminf(fmaxf(in[1] + in[3], 0.f), W), y2 = fminf(fmaxf(in[2] + in[4], 0.f), H);
  const float cw = (float)P.crop_w, ch = (float)P.crop_h;
  x1 = fminf(fmaxf(x1 - (float)P.crop_x0, 0.f), cw);
  x2 = fminf(fmaxf(x2 - (float)P.crop_x0, 0.f), cw);
  y1 = fminf(fmaxf(y1 - (float)P.crop_y0, 0.f), ch);
  y2 = fminf(fmaxf(y2 - (float)P.crop_y0, 0.f), ch);
  const float sxs = (float)Wo / cw, sys = (float)Ho / ch;
  x1 = x1 * sxs; x2 = x2 * sxs; y1 = y1 * sys; y2 = y2 * sys;
  if (P.flags & FDET_AUG_FLIP) {
    const float a = (float)Wo - x2, bq = (float)Wo - x1;
    x1 = a; x2 = bq;
  }
  if (P.flags & FDET_AUG_ROTATE) {                   // forward rotation of the corners, axis-aligned envelope, clip
    const float cx = 0.5f * (float)Wo, cy = 0.5f * (float)Ho, c = P.cos_a, s = P.sin_a;
    const float xs[4] = {x1, x2, x1, x2}, ys[4] = {y1, y1, y2, y2};
    float lx = 3.0e38f, ly = 3.0e38f, hx = -3.0e38f, hy = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dx = xs[i] - cx, dy = ys[i] - cy;
      const float rx = (c * dx + s * dy) + cx, ry = (c * dy - s * dx) + cy;
      lx = fminf(lx, rx); hx = fmaxf(hx, rx); ly = fminf(ly, ry); hy = fmaxf(hy, ry);
    }
    x1 = fminf(fmaxf(lx, 0.f), (float)Wo); x2 = fminf(fmaxf(hx, 0.f), (float)Wo);
    y1 = fminf(fmaxf(ly, 0.f), (float)Ho); y2 = fminf(fmaxf(hy, 0.f), (float)Ho);
  }
  const float w = x2 - x1, h = y2 - y1;
  if (!(w > 0.f) || !(h > 0.f) || w * h < 10.f) return false;
  out[0] = 1.f; out[1] = rintf(x1); out[2] = rintf(y1); out[3] = rintf(w); out[4] = rintf(h);
  return true;
}

__global__ void __launch_bounds__(BOX_THREADS)
k_aug_boxes(const float* __restrict__ boxes, const int32_t* __restrict__ box_offset, const fdet_aug_image* __restrict__ table,
            const fdet_aug_params* __restrict__ params, int B, int Ho, int Wo, int max_rows, float* __restrict__ rows,
            int32_t* __restrict__ out_offset) {
  __shared__ int scan[BOX_THREADS];
  const int t = threadIdx.x;
  const int per = (B + BOX_THREADS - 1) / BOX_THREADS;
  const int n0 = min(t * per, B), n1 = min(n0 + per, B);
  int cnt = 0;
  float tmp[5];
  for (int n = n0; n < n1; ++n) {
    const fdet_aug_params& P = params[n];
    const fdet_aug_image img = table[P.image];
    for (int j = box_offset[P.image]; j < box_offset[P.image + 1]; ++j)
      cnt += box_transform(boxes + (int64_t)j * 5, P, img, Ho, Wo, tmp) ? 1 : 0;
  }
  scan[t] = cnt;
  __syncthreads();
  for (int off = 1; off < BOX_THREADS; off <<= 1) {   // inclusive Hillis-Steele scan
    const int v = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  int pos = scan[t] - cnt;
  for (int n = n0; n < n1; ++n) {
    out_offset[n] = pos;
    const fdet_aug_params& P = params[n];
    const fdet_aug_image img = table[P.image];
    for (int j = box_offset[P.image]; j < box_offset[P.image + 1]; ++j) {
      if (!box_transform(boxes + (int64_t)j * 5, P, img, Ho, Wo, tmp)) continue;
      if (pos < max_rows)
        for (int e = 0; e < 5; ++e) rows[(int64_t)pos * 5 + e] = tmp[e];
      ++pos;
    }
  }
  if (t == BOX_THREADS - 1) out_offset[B] = scan[t];
}

int check_params(const fdet_aug_image* h_table, int n_images, const fdet_aug_params* h_params, int B, const char* what) {
  for (int b = 0; b < B; ++b) {
    const fdet_aug_params& P = h_params[b];
    FDET_REQUIRE(P.image >= 0 && P.image < n_images, "%s: params[%d].image=%d outside the table of %d", what, b, P.image, n_images);
    const fdet_aug_image& I = h_table[P.image];
    FDET_REQUIRE(I.offset >= 0 && I.h > 0 && I.w > 0, "%s: bad table row %d (offset %lld, %dx%d)", what, P.image,
                 (long long)I.offset, I.h, I.w);
    FDET_REQUIRE(P.crop_w > 0 && P.crop_h > 0 && P.crop_x0 >= 0 && P.crop_y0 >= 0 && P.crop_x0 + P.crop_w <= I.w &&
                     P.crop_y0 + P.crop_h <= I.h,
                 "%s: params[%d] crop (%d,%d,%d,%d) outside the %dx%d source", what, b, P.crop_x0, P.crop_y0, P.crop_w,
                 P.crop_h, I.w, I.h);
  }
  return FDET_OK;
}

int check_motion(const fdet_aug_params* h_params, int B, const char* what) {
  for (int b = 0; b < B; ++b) {
    const int k = h_params[b].motion_k;
    FDET_REQUIRE(k == 1 || k == 3 || k == 5 || k == 7, "%s: params[%d].motion_k=%d not in {1,3,5,7}", what, b, k);
    FDET_REQUIRE(k > 1 || !(h_params[b].flags & FDET_AUG_MOTION), "%s: params[%d] has motion blur on with k=1", what, b);
  }
  return FDET_OK;
}

}  // namespace

extern "C" int fdet_aug_warp(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                             const fdet_aug_params* params, const fdet_aug_params* h_params, int B, int Ho, int Wo, uint32_t seed,
                             uint8_t* mid, void* stream) {
  FDET_REQUIRE(bank && table && h_table && params && h_params && mid, "aug_warp: null pointer");
  FDET_REQUIRE(n_images > 0 && B > 0 && Ho > 0 && Wo > 0 && Ho <= 65535 * 4, "aug_warp: bad sizes n_images=%d B=%d %dx%d",
               n_images, B, Ho, Wo);
  FDET_REQUIRE(B <= 65535, "aug_warp: batch %d too large", B);
  FDET_REQUIRE((Wo % 4) != 0 || ((uintptr_t)mid % 4) == 0, "aug_warp: mid must be 4-byte aligned");
  int rc = check_params(h_table, n_images, h_params, B, "aug_warp");
  if (rc) return rc;
  const dim3 block(64, 4);
  const int wq = (Wo + WARP_PX - 1) / WARP_PX;
  const dim3 grid((wq + 63) / 64, (Ho + 3) / 4, B);
  hipLaunchKernelGGL(k_aug_warp, grid, block, 0, (hipStream_t)stream, bank, table, params, Ho, Wo, seed, mid);
  return check_launch("fdet_aug_warp");
}

extern "C" int fdet_aug_finish(const uint8_t* mid, const fdet_aug_params* params, const fdet_aug_params* h_params, int B, int Ho,
                               int Wo, uint32_t seed, uint8_t* out_u8, float* out_f32, void* stream) {
  FDET_REQUIRE(mid && params && h_params && out_u8 && out_f32, "aug_finish: null pointer");
  FDET_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && B <= 65535 && (Ho + FT_H - 1) / FT_H <= 65535, "aug_finish: bad sizes B=%d %dx%d",
               B, Ho, Wo);
  FDET_REQUIRE((Wo % 4) != 0 || (((uintptr_t)mid % 4) == 0 && ((uintptr_t)out_u8 % 4) == 0 && ((uintptr_t)out_f32 % 16) == 0),
               "aug_finish: mid / out_u8 must be 4-byte and out_f32 16-byte aligned");
  int rc = check_motion(h_params, B, "aug_finish");
  if (rc) return rc;
  const dim3 grid((Wo + FT_W - 1) / FT_W, (Ho + FT_H - 1) / FT_H, B);
  hipLaunchKernelGGL(k_aug_finish, grid, dim3(16, 16), 0, (hipStream_t)stream, mid, params, Ho, Wo, seed, out_u8, out_f32);
  return check_launch("fdet_aug_finish");
}

extern "C" int fdet_aug_boxes(const float* boxes, const int32_t* box_offset, const fdet_aug_image* table,
                              const fdet_aug_image* h_table, int n_images, const fdet_aug_params* params,
                              const fdet_aug_params* h_params, int B, int Ho, int Wo, int max_rows, float* rows,
                              int32_t* out_offset, void* stream) {
  FDET_REQUIRE(boxes && box_offset && table && h_table && params && h_params && rows && out_offset, "aug_boxes: null pointer");
  FDET_REQUIRE(n_images > 0 && B > 0 && Ho > 0 && Wo > 0 && max_rows >= 0, "aug_boxes: bad sizes n_images=%d B=%d %dx%d max_rows=%d",
               n_images, B, Ho, Wo, max_rows);
  int rc = check_params(h_table, n_images, h_params, B, "aug_boxes");
  if (rc) return rc;
  hipLaunchKernelGGL(k_aug_boxes, dim3(1), dim3(BOX_THREADS), 0, (hipStream_t)stream, boxes, box_offset, table, params, B, Ho, Wo,
                     max_rows, rows, out_offset);
  return check_launch("fdet_aug_boxes");
}
