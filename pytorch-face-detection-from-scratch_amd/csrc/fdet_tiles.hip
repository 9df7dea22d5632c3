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
//   fdet_tile_gather_flags / fdet_tile_merge_vote   the same two kernels for test-time augmentation: a
//                     per-window mirror flag (the gather reads its taps in reversed column order, the merge un-mirrors
//                     the rows first) and box voting (each kept box becomes the score-weighted integer mean of the boxes
//                     it suppressed).  Both are template instances; the plain entries compile to what they were.
//
// tests/tiles_cpu_ref.py and tests/tta_cpu_ref.py restate them in numpy.  Built with -ffp-contract=off like every file here.
#include "fdet_boxes.h"
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
                                          int Wo, bool mir, uint8_t (&res)[3][GT_PX]) {
  const int xlo = Tl.x0, xhi = Tl.x0 + Tl.w - 1;
#pragma unroll
  for (int i = 0; i < GT_PX; ++i) {
    const int ox = min(ox0 + i, Wo - 1);            // tail lanes recompute the last pixel; only valid pixels are stored
    const double u = (double)(mir ? Wo - 1 - ox : ox);     // a mirrored frame takes column Wo-1-ox's sample, same arithmetic
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

// FLAGS: flags[b] bit 0 = frame b is written mirrored left to right (fdet_tile_gather_flags); stores stay in output order,
// the block stages the source rectangle of the mirrored column range and every pixel reads the mirrored column's taps
template <bool FLAGS>
__global__ void __launch_bounds__(256)
k_tile_gather(const uint8_t* __restrict__ bank, int64_t bank_bytes, const fdet_aug_image* __restrict__ table,
              const fdet_tile* __restrict__ tiles, const uint8_t* __restrict__ flags, int Ho, int Wo,
              uint8_t* __restrict__ frames) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[GT_LDS];
  const int b = blockIdx.z;
  const fdet_tile Tl = tiles[b];
  const bool mir = FLAGS && (flags[b] & 1);                  // block-uniform
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
  const int ua = mir ? Wo - 1 - oxl : tx0, ub = mir ? Wo - 1 - tx0 : oxl;       // first and last sampled column
  const double sxa = ((double)ua + 0.5) * rw + (double)Tl.x0 - 0.5, sxb = ((double)ub + 0.5) * rw + (double)Tl.x0 - 0.5;
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
    gather_px(stage, (y0 - fylo) * pitch + m0 - fxlo * 3, (y1 - fylo) * pitch + m1 - fxlo * 3, fy, Tl, rw, ox0, Wo, mir, res);
  } else {
    gather_px(src, (int64_t)y0 * row_bytes, (int64_t)y1 * row_bytes, fy, Tl, rw, ox0, Wo, mir, res);
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
// merge: one workgroup per source image; 33 bytes of LDS per candidate, the carve of fdet_nms (fdet_boxes.h) with plane 5
// holding src: candidate -> row of `rows` (tile * K + r), so that the sweep computes the areas from the corners
// ------------------------------------------------------------------------------------------------------------------
constexpr int MERGE_CAP = 4864;

// one detection row in frame pixels -> source pixels: fp32, separate multiply and add, then half-to-even
__device__ __forceinline__ void to_source(const float* d, const fdet_tile& Tl, float kx, float ky, float& x, float& y, float& w,
                                          float& h) {
  x = rintf((float)Tl.x0 + d[1] * kx);
  y = rintf((float)Tl.y0 + d[2] * ky);
  w = rintf(d[3] * kx);
  h = rintf(d[4] * ky);
}

// what fdet_tile_merge_vote adds to fdet_tile_merge
struct MergeTta {
  const uint8_t* flags;    // [T] bit 0 = the tile's frame was mirrored; nullptr = none
  int32_t* out_votes;      // [n_images, Kout]
  int min_votes, vote;
};
// LDS behind the candidates: two sets of {Q, sum q*x1, sum q*y1, sum q*x2, sum q*y2, suppressed} int64, used alternately by
// successive keepers so that one barrier per keeper stays enough
constexpr int VOTE_ACC = 6, VOTE_LDS = 128;

// step 0: the row of a mirrored frame in the pixels of the unmirrored frame; two fp32 subtractions in this order
__device__ __forceinline__ void load_row(const float* d, bool mir, int Wo, float (&r)[5]) {
#pragma unroll
  for (int e = 0; e < 5; ++e) r[e] = d[e];
  if (mir) r[1] = ((float)Wo - r[1]) - r[3];
}

// the integer weight of a member: 2^20 * min(score, 1), 0 for a score that is NaN (key -inf) or <= 0 and for a box with a
// corner that is not finite or beyond 2^24 (whose integer value an fp32 no longer holds)
__device__ __forceinline__ long long vote_weight(float key, float x1, float y1, float x2, float y2) {
  const float lim = 16777216.f;
  if (!(key > 0.f) || !(fabsf(x1) <= lim && fabsf(y1) <= lim && fabsf(x2) <= lim && fabsf(y2) <= lim)) return 0;
  return llrint((double)fminf(key, 1.f) * 1048576.0);
}

// what box voting does per suppression and per keeper in the shared sweep (box_greedy_nms of fdet_boxes.h)
struct VoteHook {
  const BoxLds& L;
  unsigned long long* acc;                           // the two accumulator sets
  const MergeTta& A;
  int par = 0;
  unsigned long long* S = nullptr;                   // the accumulator set of this keeper
  float* mine = nullptr;                             // the plane that lane e of wave 0 writes in settle: x, y, w or h

  __device__ __forceinline__ void begin() {
    if (threadIdx.x < 2 * VOTE_ACC) acc[threadIdx.x] = 0ull;
    const int e = threadIdx.x & 3;                   // chosen once: a per-keeper choice costs 4 % on the vote=1 path
    mine = e == 0 ? L.x1 : e == 1 ? L.y1 : e == 2 ? L.x2 : L.y2;
  }
  __device__ __forceinline__ void visit(int) { S = acc + par * VOTE_ACC; }
  // j dies here and nowhere else: the current keeper owns it.  Integer sums in LDS, so the order of the additions cannot
  // change them
  __device__ __forceinline__ void suppress(int j, float jx1, float jy1, float jx2, float jy2) const {
    atomicAdd(&S[5], 1ull);
    const long long q = A.vote ? vote_weight(L.key[j], jx1, jy1, jx2, jy2) : 0;
    if (q) {
      atomicAdd(&S[0], (unsigned long long)q);
      atomicAdd(&S[1], (unsigned long long)(q * (long long)jx1));
      atomicAdd(&S[2], (unsigned long long)(q * (long long)jy1));
      atomicAdd(&S[3], (unsigned long long)(q * (long long)jx2));
      atomicAdd(&S[4], (unsigned long long)(q * (long long)jy2));
    }
  }
  // 4: lanes 0..3 of wave 0 turn the sums into x, y, w, h.  Candidate i is never read again by the sweep, so its box
  // slots take the voted box and its key slot the member count (bit 31: voted); the other waves go on meanwhile
  __device__ __forceinline__ void settle(int i, float ix1, float iy1, float ix2, float iy2) {
    if (threadIdx.x < 4) {
      const int e = threadIdx.x, ax = e & 1;
      const unsigned long long sq = S[0], sl = S[1 + ax], sh = S[3 + ax], sn = S[5];
      __builtin_amdgcn_wave_barrier();           // the four lanes' reads are issued before lane 0's clears
      if (e == 0) {
#pragma unroll
        for (int k = 0; k < VOTE_ACC; ++k) S[k] = 0ull;
      }
      const long long members = (long long)sn + 1;
      const long long qi = A.vote ? vote_weight(L.key[i], ix1, iy1, ix2, iy2) : 0;
      const long long Q = (long long)sq + qi;
      const long long slo = (long long)sl + (qi ? qi * (long long)(ax ? iy1 : ix1) : 0);
      const long long shi = (long long)sh + (qi ? qi * (long long)(ax ? iy2 : ix2) : 0);
      if (Q > 0) {
        const double lo = rint((double)slo / (double)Q);
        const float v = e < 2 ? (float)lo : (float)(rint((double)shi / (double)Q) - lo);
        mine[i] = v;
      }
      if (e == 0) {
        // lanes 0..3 read L.key[i] (vote_weight above) before this store by program order inside one wave; a read
        // of the key moved below this line, or into another wave, would see the member count instead
        L.key[i] = __int_as_float((int)members | (Q > 0 ? (int)0x80000000 : 0));
        if (members >= A.min_votes) { L.keep[L.ctl[5]] = i; L.ctl[5] += 1; }       // 5: the others only suppressed
      }
    }
    par ^= 1;                                        // two sets, used alternately: one barrier per keeper stays enough
  }
};

template <bool TTA>
__global__ void __launch_bounds__(256)
k_tile_merge(const float* __restrict__ rows, const int32_t* __restrict__ counts, const fdet_tile* __restrict__ tiles,
             const int32_t* __restrict__ tile_offset, int T, int K, int Ho, int Wo, const fdet_aug_image* __restrict__ table,
             float margin, double thr, int cap, int Kout, float* __restrict__ out, int32_t* __restrict__ out_counts,
             unsigned long long* __restrict__ rejected, MergeTta A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const BoxLds L = box_carve(smem, cap, true, false);
  unsigned long long* const acc = reinterpret_cast<unsigned long long*>(smem + box_lds_bytes(cap, true));  // TTA only
  const int n = blockIdx.x, tid = threadIdx.x;
  const int t0 = tile_offset[n], t1 = tile_offset[n + 1];
  const fdet_aug_image img = table[n];
  bool bad = t0 < 0 || t1 < t0 || t1 > T;
  if (tid == 0) L.ctl[0] = 0;
  __syncthreads();
  // 1 + 2: ordered compaction of the tiles' rows (tile order, then row) that pass the cut-face rule
  for (int t = t0; t < t1 && !bad; ++t) {
    const fdet_tile Tl = tiles[t];
    const bool mir = TTA && A.flags && (A.flags[t] & 1);
    const int c = counts[t];
    if (c < 0 || c > K || Tl.image != n) { bad = true; break; }        // uniform: every thread read the same words
    const float kx = (float)Tl.w / (float)Wo, ky = (float)Tl.h / (float)Ho;
    const bool cl = Tl.x0 > 0, cr = Tl.x0 + Tl.w < img.w, ct = Tl.y0 > 0, cb = Tl.y0 + Tl.h < img.h;   // interior sides
    for (int r0 = 0; r0 < c; r0 += 256) {
      const int r = r0 + tid;
      float d[5];
      load_row(rows + ((size_t)t * K + min(r, c - 1)) * 5, mir, Wo, d);
      bool hit = r < c;
      if (hit && margin > 0.f) {
        const float bx2 = d[1] + d[3], by2 = d[2] + d[4];
        if ((cl && d[1] < margin) || (cr && bx2 > (float)Wo - margin) || (ct && d[2] < margin) || (cb && by2 > (float)Ho - margin))
          hit = false;
      }
      const int k = compact_slot(hit, L.ctl);
      if (hit && k < cap) {
        float x, y, w, h;
        to_source(d, Tl, kx, ky, x, y, w, h);
        // a NaN score is ordered as -inf (visited last), as fdet_eval_match does.  The shared key also turns -0 into +0:
        // the key never reaches an output (v[0] below is read from the row again) and -0 compares equal to +0 in the rank,
        // in vote_weight's `key > 0` and in its fminf, so no result changes with it
        L.key[k] = nan_last_key(d[0]);
        L.x1[k] = x; L.y1[k] = y; L.x2[k] = x + w; L.y2[k] = y + h;
        L.src[k] = t * K + r;
      }
    }
  }
  __syncthreads();                                   // the candidates and the total are visible
  const int C = L.ctl[0];
  bad = bad || C > MERGE_CAP || C > cap;
  int nk = 0;
  if (!bad) {
    // 3: greedy NMS (torchvision 0.11.2 nms_kernel.cpp, the sweep of fdet_nms): stable descending rank, fp32 overlap
    if (TTA) {
      VoteHook vote{L, acc, A};
      nk = box_greedy_nms(L, C, thr, vote);
    } else {
      KeepEvery every{L};
      nk = box_greedy_nms(L, C, thr, every);
    }
    bad = nk > Kout;
  }
  // 4: an image over a limit is rejected as a whole
  if (bad) nk = 0;
  float* o = out + (size_t)n * Kout * 5;
  for (int k = tid; k < Kout; k += 256) {
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int votes = 0;
    if (k < nk) {
      const int i = L.keep[k];
      const int s = L.src[i];
      const int t = s / K;
      const fdet_tile Tl = tiles[t];
      float d[5];
      load_row(rows + (size_t)s * 5, TTA && A.flags && (A.flags[t] & 1), Wo, d);
      v[0] = d[0];
      const int bits = TTA ? __float_as_int(L.key[i]) : 0;
      votes = bits & 0x7fffffff;
      if (bits < 0) { v[1] = L.x1[i]; v[2] = L.y1[i]; v[3] = L.x2[i]; v[4] = L.y2[i]; }
      else to_source(d, Tl, (float)Tl.w / (float)Wo, (float)Tl.h / (float)Ho, v[1], v[2], v[3], v[4]);
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) o[(size_t)k * 5 + e] = v[e];
    if (TTA) A.out_votes[(size_t)n * Kout + k] = votes;
  }
  if (tid == 0) {
    out_counts[n] = nk;
    if (bad) atomicAdd(rejected, 1ull);
  }
}

}  // namespace

// both gather entries: h_flags == nullptr is fdet_tile_gather
static int tile_gather_launch(const char* what, const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table,
                              int n_images, const fdet_tile* tiles, const fdet_tile* h_tiles, const uint8_t* flags,
                              const uint8_t* h_flags, int T, int Ho, int Wo, uint8_t* frames, void* stream) {
  FDET_REQUIRE(bank && table && h_table && tiles && h_tiles && frames, "%s: null pointer", what);
  FDET_REQUIRE(n_images > 0 && T > 0 && T <= 65535 && Ho > 0 && Wo > 0 && (Ho + GT_H - 1) / GT_H <= 65535,
               "%s: bad sizes n_images=%d T=%d %dx%d (at most 65535 windows per call)", what, n_images, T, Ho, Wo);
  FDET_REQUIRE((Wo % 4) != 0 || ((uintptr_t)frames % 4) == 0, "%s: frames must be 4-byte aligned", what);
  int64_t bank_bytes = 0;                                    // the bytes the referenced images prove readable
  for (int t = 0; t < T; ++t) {
    const fdet_tile& W = h_tiles[t];
    FDET_REQUIRE(W.image >= 0 && W.image < n_images, "%s: tiles[%d].image=%d outside the table of %d", what, t, W.image,
                 n_images);
    const fdet_aug_image& I = h_table[W.image];
    FDET_REQUIRE(I.offset >= 0 && I.h > 0 && I.w > 0, "%s: bad table row %d (offset %lld, %dx%d)", what, W.image,
                 (long long)I.offset, I.h, I.w);
    FDET_REQUIRE(W.w > 0 && W.h > 0 && W.x0 >= 0 && W.y0 >= 0 && (int64_t)W.x0 + W.w <= I.w && (int64_t)W.y0 + W.h <= I.h,
                 "%s: tiles[%d] window (%d,%d,%d,%d) outside the %dx%d source", what, t, W.x0, W.y0, W.w, W.h, I.w, I.h);
    FDET_REQUIRE(!h_flags || (h_flags[t] & ~1u) == 0, "%s: flags[%d]=%u, only bit 0 (mirror) is defined", what, t,
                 (unsigned)(h_flags ? h_flags[t] : 0));
    const int64_t end = I.offset + (int64_t)I.h * I.w * 3;
    bank_bytes = end > bank_bytes ? end : bank_bytes;
  }
  const dim3 grid((Wo + GT_W - 1) / GT_W, (Ho + GT_H - 1) / GT_H, T);
  if (h_flags)
    hipLaunchKernelGGL(k_tile_gather<true>, grid, dim3(GT_BX, GT_BY), 0, (hipStream_t)stream, bank, bank_bytes, table, tiles,
                       flags, Ho, Wo, frames);
  else
    hipLaunchKernelGGL(k_tile_gather<false>, grid, dim3(GT_BX, GT_BY), 0, (hipStream_t)stream, bank, bank_bytes, table, tiles,
                       flags, Ho, Wo, frames);
  return check_launch(what);
}

extern "C" int fdet_tile_gather(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table, int n_images,
                                const fdet_tile* tiles, const fdet_tile* h_tiles, int T, int Ho, int Wo, uint8_t* frames,
                                void* stream) {
  return tile_gather_launch("fdet_tile_gather", bank, table, h_table, n_images, tiles, h_tiles, nullptr, nullptr, T, Ho, Wo, frames,
                            stream);
}

extern "C" int fdet_tile_gather_flags(const uint8_t* bank, const fdet_aug_image* table, const fdet_aug_image* h_table,
                                      int n_images, const fdet_tile* tiles, const fdet_tile* h_tiles, const uint8_t* flags,
                                      const uint8_t* h_flags, int T, int Ho, int Wo, uint8_t* frames, void* stream) {
  FDET_REQUIRE(flags && h_flags, "fdet_tile_gather_flags: null pointer");
  return tile_gather_launch("fdet_tile_gather_flags", bank, table, h_table, n_images, tiles, h_tiles, flags, h_flags, T, Ho, Wo,
                            frames, stream);
}

// both merge entries: tta == nullptr is fdet_tile_merge
static int tile_merge_launch(const char* what, const float* rows, const int32_t* counts, const fdet_tile* tiles,
                             const int32_t* tile_offset, int n_images, int T, int K, int Ho, int Wo, const fdet_aug_image* table,
                             float edge_margin, double iou_threshold, int Kout, float* out, int32_t* out_counts,
                             uint64_t* rejected, const MergeTta* tta, void* stream) {
  FDET_REQUIRE(rows && counts && tiles && tile_offset && table && out && out_counts && rejected, "%s: null pointer", what);
  FDET_REQUIRE(n_images > 0 && T > 0 && K > 0 && Ho > 0 && Wo > 0 && Kout > 0 && (int64_t)T * K <= 0x7fffffffLL,
               "%s: bad sizes n_images=%d T=%d K=%d %dx%d Kout=%d", what, n_images, T, K, Ho, Wo, Kout);
  FDET_REQUIRE(edge_margin >= 0.f, "%s: edge_margin=%g must be >= 0", what, (double)edge_margin);
  const int64_t most = (int64_t)T * K;
  const int cap = most < MERGE_CAP ? (int)most : MERGE_CAP;
  const size_t lds = box_lds_bytes(cap, true) + (tta ? VOTE_LDS : 0);
  const void* kern = tta ? reinterpret_cast<const void*>(k_tile_merge<true>) : reinterpret_cast<const void*>(k_tile_merge<false>);
  if (lds > 64 * 1024)
    if (int rc = set_lds_attr(kern, lds, what)) return rc;
  auto* rej = reinterpret_cast<unsigned long long*>(rejected);
  if (tta)
    hipLaunchKernelGGL(k_tile_merge<true>, dim3(n_images), dim3(256), lds, (hipStream_t)stream, rows, counts, tiles, tile_offset,
                       T, K, Ho, Wo, table, edge_margin, iou_threshold, cap, Kout, out, out_counts, rej, *tta);
  else
    hipLaunchKernelGGL(k_tile_merge<false>, dim3(n_images), dim3(256), lds, (hipStream_t)stream, rows, counts, tiles, tile_offset,
                       T, K, Ho, Wo, table, edge_margin, iou_threshold, cap, Kout, out, out_counts, rej, MergeTta{});
  return check_launch(what);
}

extern "C" int fdet_tile_merge(const float* rows, const int32_t* counts, const fdet_tile* tiles, const int32_t* tile_offset,
                               int n_images, int T, int K, int Ho, int Wo, const fdet_aug_image* table, float edge_margin,
                               double iou_threshold, int Kout, float* out, int32_t* out_counts, uint64_t* rejected,
                               void* stream) {
  return tile_merge_launch("fdet_tile_merge", rows, counts, tiles, tile_offset, n_images, T, K, Ho, Wo, table, edge_margin,
                           iou_threshold, Kout, out, out_counts, rejected, nullptr, stream);
}

extern "C" int fdet_tile_merge_vote(const float* rows, const int32_t* counts, const fdet_tile* tiles, const uint8_t* flags,
                                    const int32_t* tile_offset, int n_images, int T, int K, int Ho, int Wo,
                                    const fdet_aug_image* table, float edge_margin, double iou_threshold, int min_votes, int vote,
                                    int Kout, float* out, int32_t* out_votes, int32_t* out_counts, uint64_t* rejected,
                                    void* stream) {
  FDET_REQUIRE(out_votes, "fdet_tile_merge_vote: null pointer");
  FDET_REQUIRE(min_votes >= 1 && (vote == 0 || vote == 1), "fdet_tile_merge_vote: min_votes=%d must be >= 1 and vote=%d 0 or 1",
               min_votes, vote);
  const MergeTta tta{flags, out_votes, min_votes, vote};
  return tile_merge_launch("fdet_tile_merge_vote", rows, counts, tiles, tile_offset, n_images, T, K, Ho, Wo, table, edge_margin,
                           iou_threshold, Kout, out, out_counts, rejected, &tta, stream);
}
