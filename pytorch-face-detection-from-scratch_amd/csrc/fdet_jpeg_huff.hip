// Huffman decoding of baseline JPEG scans on the device (the rules are spelled out in include/fdet.h and
// restated in Python by tests/jpeg_huff_cpu_ref.py).  The host unstuffs the scan into one byte run per restart interval
// (fdet_jpeg_scan_prepare in fdet_jpeg.hip); here
//
//   fdet_jpeg_huffman_sync   k_huff_sync   one self-synchronisation pass: a thread per subsequence of sub_bits bits
//   fdet_jpeg_huffman_emit   k_huff_scan   exclusive scan of the subsequences' block counts per segment
//                            k_huff_emit   the parse again from the true entry states, coefficients stored de-zigzagged
//                            k_huff_dcsum  DC differences -> DC values per (segment, component), modulo 2^16
//
// A workgroup takes 256 consecutive subsequences of ONE image, so that the image's six decode tables sit in LDS once; the
// grid is the sum of the images' workgroups and a workgroup finds its image by a search over their wg_first.  Lanes read
// their own bits from global memory through a 64-bit window; lanes diverge by the nature of the problem.  No thread waits for another: a pass is one launch, and the caller decides how many to enqueue.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

__constant__ uint8_t kNaturalD[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int HUFF_THREADS = 256;
constexpr uint32_t END = FDET_JPEG_HUFF_END;

// The bits of one segment.  `words` 32-bit words may be read (the segment's bytes rounded up to 16); what lies behind reads 0.
struct Bits {
  const uint32_t* w;
  uint32_t words;
  uint32_t cur;        // index of the word in the high half of `win`
  uint64_t win;
  __device__ __forceinline__ uint32_t word(uint32_t i) const { return i < words ? __builtin_bswap32(w[i]) : 0u; }
  __device__ __forceinline__ void seek(uint32_t p) {
    cur = p >> 5;
    win = ((uint64_t)word(cur) << 32) | word(cur + 1);
  }
  __device__ __forceinline__ uint32_t peek32(uint32_t p) {     // bits p .. p + 31, most significant first
    const uint32_t i = p >> 5;
    if (i != cur) {
      if (i == cur + 1) { win = (win << 32) | word(i + 1); cur = i; }
      else seek(p);
    }
    return (uint32_t)((win << (p & 31)) >> 32);
  }
};

struct Geom {
  int ncomp, hs, vs, bpm;       // blocks per MCU
  int mcus_x, mcus_y;
};

__device__ __forceinline__ int comp_of(const Geom& G, int blk) {
  const int luma = G.hs * G.vs;
  return G.ncomp == 1 ? 0 : blk < luma ? 0 : blk == luma ? 1 : 2;
}

// Where the parse of one subsequence stores: EMIT only.
struct Sink {
  int16_t* coef;
  uint64_t coef_count;
  int64_t plane[3];
  int first_mcu;
  uint32_t seg_blocks;
  bool check_tail;              // not the image's last segment: the host decoder looks at what follows its blocks
  uint32_t n;                   // scan-order index (within the segment) of the block being parsed
  int64_t base;                 // its first coefficient, -1: outside (nothing is stored)
};

__device__ __forceinline__ void sink_open(Sink& S, const Geom& G) {
  S.base = -1;
  if (S.n >= S.seg_blocks) return;
  const int64_t mcu = (int64_t)S.first_mcu + S.n / (uint32_t)G.bpm;
  const int b = (int)(S.n % (uint32_t)G.bpm);
  if (mcu >= (int64_t)G.mcus_x * G.mcus_y) return;
  const int my = (int)(mcu / G.mcus_x), mx = (int)(mcu - (int64_t)my * G.mcus_x);
  const int c = comp_of(G, b);
  const int hs = c == 0 ? G.hs : 1, vs = c == 0 ? G.vs : 1;
  const int r = c == 0 ? b : 0;
  const int v = r / hs, h = r - v * hs;
  const int64_t idx = (c == 0 ? S.plane[0] : c == 1 ? S.plane[1] : S.plane[2]) + ((int64_t)(my * vs + v) * ((int64_t)G.mcus_x * hs) + (mx * hs + h)) * 64;
  if (idx < 0 || (uint64_t)(idx + 64) > S.coef_count) return;
  S.base = idx;
}

// Parse the symbols that start in [p, limit) of a segment of `nbits` bits.  -> the exit position, or END in `p`.
template <bool EMIT>
__device__ __forceinline__ void parse(Bits& R, const fdet_jpeg_huff_tables* T, const Geom& G, uint32_t& p, uint32_t limit,
                                      uint32_t nbits, int& blk, int& z, uint32_t& count, uint32_t& events, Sink& S) {
  bool ended = false;
  const uint32_t stop = limit < nbits ? limit : nbits;
  // every iteration consumes at least one bit, so the loop runs at most sub_bits times
  while (p < stop) {
    if (EMIT && S.n >= S.seg_blocks) break;              // what follows the segment's blocks is padding
    const uint32_t rem = nbits - p;
    const uint32_t bits = R.peek32(p);
    const int c = comp_of(G, blk);
    const fdet_jpeg_huff_table& H = z == 0 ? T->dc[c] : T->ac[c];
    const uint32_t look = bits >> 23;                    // 9 bits: 0..511
    uint32_t nb = H.look_nbits[look];
    int sym = H.look_sym[look];
    if (nb == 0 || nb > 9) {
      nb = 0;
      for (uint32_t l = 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(bits >> (32 - l));
        if (code <= H.maxcode[l]) {
          const int32_t idx = H.valoffset[l] + code;
          if (idx >= 0 && idx < H.nvals && idx < 256) { nb = l; sym = H.vals[idx]; }
          break;
        }
      }
      if (nb == 0) { events |= FDET_JPEG_HUFF_NOCODE; p += 1; continue; }
    }
    if (nb > rem) { ended = true; break; }
    if (z == 0) {
      uint32_t s = (uint32_t)sym;
      if (s > 16) { events |= FDET_JPEG_HUFF_DCCAT; s = 0; }
      if (nb + s > rem) { ended = true; break; }
      if (EMIT && S.base >= 0) {
        int32_t d = 0;
        if (s) {
          const uint32_t v = (uint32_t)(((uint64_t)bits << nb) >> (32 - s)) & (uint32_t)((1ull << s) - 1);
          d = v < (1u << (s - 1)) ? (int32_t)v - (int32_t)((1ull << s) - 1) : (int32_t)v;
        }
        S.coef[S.base] = (int16_t)d;
      }
      p += nb + s;
      z = 1;
      continue;
    }
    const int r = sym >> 4;
    const uint32_t s = (uint32_t)sym & 15u;
    bool close = false;
    if (s) {
      const int k = z + r;
      if (k > 63) {
        events |= FDET_JPEG_HUFF_RUN;
        p += nb;
        close = true;
      } else {
        if (nb + s > rem) { ended = true; break; }
        if (EMIT && S.base >= 0) {
          const uint32_t v = (uint32_t)(((uint64_t)bits << nb) >> (32 - s)) & ((1u << s) - 1);
          const int32_t d = v < (1u << (s - 1)) ? (int32_t)v - (int32_t)((1u << s) - 1) : (int32_t)v;
          S.coef[S.base + kNaturalD[k & 63]] = (int16_t)d;
        }
        p += nb + s;
        z = k + 1;
        close = z > 63;
      }
    } else {
      p += nb;
      if (r == 15) { z += 16; close = z > 63; }
      else close = true;
    }
    if (close) {
      count += 1;
      blk = blk + 1 >= G.bpm ? 0 : blk + 1;
      z = 0;
      if (EMIT) {
        S.n += 1;
        if (S.n == S.seg_blocks && S.check_tail && nbits - p > 64u) events |= FDET_JPEG_HUFF_TRAILING;
        sink_open(S, G);
      }
    }
  }
  if (ended || p < limit) p = END;
}

__device__ __forceinline__ void load_tables(fdet_jpeg_huff_tables* lds, const fdet_jpeg_huff_tables* g) {
  static_assert(sizeof(fdet_jpeg_huff_tables) % 8 == 0, "tables are copied in 8-byte words");
  const uint64_t* src = reinterpret_cast<const uint64_t*>(g);
  uint64_t* dst = reinterpret_cast<uint64_t*>(lds);
  for (int i = threadIdx.x; i < (int)(sizeof(fdet_jpeg_huff_tables) / 8); i += HUFF_THREADS) dst[i] = src[i];
  __syncthreads();
}

// The segment of subsequence g of an image: the last one whose sub_first <= g (the image's segments are consecutive).
__device__ __forceinline__ int find_segment(const fdet_jpeg_huff_segment* segs, int first, int count, int g) {
  int lo = 0, hi = count - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[first + mid].sub_first <= g) lo = mid;
    else hi = mid - 1;
  }
  return first + lo;
}

struct Sub {
  bool active;
  int g, seg, k;                // global subsequence, its segment, its index within the segment
  uint32_t nbits, begin, limit; // the segment's bits, this subsequence's first bit and the boundary behind it
  Geom G;
  Bits R;
};

// The image of workgroup `wg`: the last one whose wg_first <= wg.
__device__ __forceinline__ int find_image(const fdet_jpeg_huff_image* images, int n_images, int wg) {
  int lo = 0, hi = n_images - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[mid].wg_first <= wg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ Sub locate(const uint8_t* scan, const fdet_jpeg_huff_image& I, const fdet_jpeg_huff_segment* segs,
                                      int sub_bits, int wg) {
  Sub U;
  U.G.ncomp = I.ncomp; U.G.hs = I.hs; U.G.vs = I.vs;
  U.G.bpm = I.ncomp == 1 ? 1 : I.hs * I.vs + 2;
  U.G.mcus_x = I.mcus_x; U.G.mcus_y = I.mcus_y;
  const int t = wg * HUFF_THREADS + threadIdx.x;
  U.active = wg >= 0 && t < I.sub_count;
  U.g = I.sub_first + (U.active ? t : 0);
  U.seg = find_segment(segs, I.seg_first, I.seg_count, U.g);
  const fdet_jpeg_huff_segment& S = segs[U.seg];
  U.k = U.g - S.sub_first;
  if (U.k < 0 || U.k >= S.sub_count) U.active = false;
  U.nbits = (uint32_t)S.byte_len * 8u;
  U.begin = (uint32_t)U.k * (uint32_t)sub_bits;
  U.limit = U.begin + (uint32_t)sub_bits;
  U.R.w = reinterpret_cast<const uint32_t*>(scan + S.byte_offset);
  U.R.words = (uint32_t)((S.byte_len + 15) >> 4) * 4u;
  return U;
}

__device__ __forceinline__ bool unpack(uint32_t st, const Geom& G, uint32_t& off, int& blk, int& z) {
  off = st & 31u;
  blk = (int)((st >> 8) & 15u);
  z = (int)((st >> 16) & 63u);
  if (blk >= G.bpm) blk = 0;
  return st != END;
}

__global__ void __launch_bounds__(HUFF_THREADS)
k_huff_sync(const uint8_t* __restrict__ scan, const fdet_jpeg_huff_tables* __restrict__ tables,
            const fdet_jpeg_huff_image* __restrict__ images, int n_images, const fdet_jpeg_huff_segment* __restrict__ segs,
            int sub_bits, uint64_t* state, uint32_t* __restrict__ changed) {
  __shared__ __attribute__((aligned(16))) fdet_jpeg_huff_tables T;
  const int img = find_image(images, n_images, (int)blockIdx.x);
  const fdet_jpeg_huff_image I = images[img];
  const int wg = (int)blockIdx.x - I.wg_first;
  if (wg < 0 || wg * HUFF_THREADS >= I.sub_count) return;               // uniform: the whole workgroup leaves
  load_tables(&T, tables + img);
  Sub U = locate(scan, I, segs, sub_bits, wg);
  if (!U.active) return;
  const uint32_t entry = U.k == 0 ? 0u : (uint32_t)state[3 * (int64_t)(U.g - 1)];
  if (state[3 * (int64_t)U.g + 2] == (uint64_t)entry + 1) return;
  uint32_t off, count = 0, events = 0;
  int blk, z;
  uint32_t p = END;
  if (unpack(entry, U.G, off, blk, z)) {
    p = U.begin + off;
    U.R.seek(p < U.nbits ? p : 0);
    Sink none;
    parse<false>(U.R, &T, U.G, p, U.limit, U.nbits, blk, z, count, events, none);
  }
  const uint32_t exit_state = p == END ? END : ((p - U.limit) & 31u) | ((uint32_t)blk << 8) | ((uint32_t)z << 16);
  state[3 * (int64_t)U.g] = exit_state;
  state[3 * (int64_t)U.g + 1] = count;
  state[3 * (int64_t)U.g + 2] = (uint64_t)entry + 1;
  changed[img] = 1u;
}

// grid: segments.  first_block[g] = blocks completed by the segment's subsequences in front of g.
__global__ void __launch_bounds__(HUFF_THREADS)
k_huff_scan(const fdet_jpeg_huff_image* __restrict__ images, const fdet_jpeg_huff_segment* __restrict__ segs,
            const uint64_t* __restrict__ state, uint32_t* __restrict__ first_block, uint32_t* __restrict__ flags) {
  __shared__ uint32_t part[HUFF_THREADS];
  const fdet_jpeg_huff_segment S = segs[blockIdx.x];
  const fdet_jpeg_huff_image& I = images[S.image];
  const int tid = threadIdx.x;
  const int per = (S.sub_count + HUFF_THREADS - 1) / HUFF_THREADS;      // a contiguous run per thread
  const int a = min(tid * per, S.sub_count), b = min(a + per, S.sub_count);
  uint32_t sum = 0;
  for (int k = a; k < b; ++k) sum += (uint32_t)state[3 * (int64_t)(S.sub_first + k) + 1];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < HUFF_THREADS; d <<= 1) {                          // inclusive scan of the runs' sums
    const uint32_t v = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  for (int k = a; k < b; ++k) {
    first_block[S.sub_first + k] = run;
    run += (uint32_t)state[3 * (int64_t)(S.sub_first + k) + 1];
  }
  const uint32_t bpm = I.ncomp == 1 ? 1u : (uint32_t)(I.hs * I.vs + 2);
  if (tid == HUFF_THREADS - 1 && part[tid] < (uint32_t)S.mcu_count * bpm) atomicOr(&flags[S.image], FDET_JPEG_HUFF_EXHAUSTED);
}

__global__ void __launch_bounds__(HUFF_THREADS)
k_huff_emit(const uint8_t* __restrict__ scan, const fdet_jpeg_huff_tables* __restrict__ tables,
            const fdet_jpeg_huff_image* __restrict__ images, int n_images, const fdet_jpeg_huff_segment* __restrict__ segs,
            int sub_bits, const uint64_t* __restrict__ state, const uint32_t* __restrict__ first_block,
            int16_t* __restrict__ coef, uint64_t coef_count, uint32_t* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) fdet_jpeg_huff_tables T;
  const int img = find_image(images, n_images, (int)blockIdx.x);
  const fdet_jpeg_huff_image I = images[img];
  const int wg = (int)blockIdx.x - I.wg_first;
  if (wg < 0 || wg * HUFF_THREADS >= I.sub_count) return;
  load_tables(&T, tables + img);
  Sub U = locate(scan, I, segs, sub_bits, wg);
  if (!U.active) return;
  const uint32_t entry = U.k == 0 ? 0u : (uint32_t)state[3 * (int64_t)(U.g - 1)];
  uint32_t off, count = 0, events = 0;
  int blk, z;
  if (!unpack(entry, U.G, off, blk, z)) return;
  const fdet_jpeg_huff_segment& S = segs[U.seg];
  Sink K;
  K.coef = coef;
  K.coef_count = coef_count;
  K.plane[0] = I.coef_offset[0]; K.plane[1] = I.coef_offset[1]; K.plane[2] = I.coef_offset[2];
  K.first_mcu = S.first_mcu;
  K.seg_blocks = (uint32_t)S.mcu_count * (uint32_t)U.G.bpm;
  K.check_tail = U.seg != I.seg_first + I.seg_count - 1;
  K.n = first_block[U.g];
  sink_open(K, U.G);
  uint32_t p = U.begin + off;
  U.R.seek(p < U.nbits ? p : 0);
  parse<true>(U.R, &T, U.G, p, U.limit, U.nbits, blk, z, count, events, K);
  if (events) atomicOr(&flags[img], events);
}

// grid (segments, components).  The c-th component's blocks of a segment in scan order: element j lies in MCU first_mcu +
// j / (hs_c * vs_c) at (v, h) = divmod(j mod (hs_c * vs_c), hs_c).  A contiguous run of elements per thread, the runs'
// sums scanned through LDS.
__global__ void __launch_bounds__(HUFF_THREADS)
k_huff_dcsum(const fdet_jpeg_huff_image* __restrict__ images, const fdet_jpeg_huff_segment* __restrict__ segs,
             int16_t* __restrict__ coef, uint64_t coef_count) {
  __shared__ uint32_t part[HUFF_THREADS];
  const fdet_jpeg_huff_segment S = segs[blockIdx.x];
  const fdet_jpeg_huff_image& I = images[S.image];
  const int c = blockIdx.y;
  if (c >= I.ncomp) return;
  const int hs = c == 0 ? I.hs : 1, vs = c == 0 ? I.vs : 1;
  const int per_mcu = hs * vs;
  const int64_t n = (int64_t)S.mcu_count * per_mcu;
  const int64_t mcus = (int64_t)I.mcus_x * I.mcus_y;
  const int64_t plane = I.coef_offset[c];
  const int64_t bw = (int64_t)I.mcus_x * hs;
  auto address = [&](int64_t j) -> int64_t {
    const int64_t mcu = S.first_mcu + j / per_mcu;
    if (mcu < 0 || mcu >= mcus) return -1;
    const int r = (int)(j % per_mcu);
    const int v = r / hs, h = r - v * hs;
    const int64_t my = mcu / I.mcus_x, mx = mcu - my * I.mcus_x;
    const int64_t idx = plane + ((my * vs + v) * bw + mx * hs + h) * 64;
    return (idx < 0 || (uint64_t)(idx + 64) > coef_count) ? -1 : idx;
  };
  const int tid = threadIdx.x;
  const int64_t per = (n + HUFF_THREADS - 1) / HUFF_THREADS;
  const int64_t a = min((int64_t)tid * per, n), b = min(a + per, n);
  uint32_t sum = 0;
  for (int64_t j = a; j < b; ++j) {
    const int64_t idx = address(j);
    if (idx >= 0) sum += (uint32_t)(uint16_t)coef[idx];
  }
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < HUFF_THREADS; d <<= 1) {
    const uint32_t v = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  for (int64_t j = a; j < b; ++j) {
    const int64_t idx = address(j);
    if (idx >= 0) {
      run += (uint32_t)(uint16_t)coef[idx];
      coef[idx] = (int16_t)(uint16_t)(run & 0xffffu);
    }
  }
}

// Everything the kernels index with, checked on the host copies.  -> the workgroups of all images.
int validate(const char* who, const void* scan, size_t scan_bytes, const fdet_jpeg_huff_image* h_images, int n_images,
             const fdet_jpeg_huff_segment* h_segs, int n_segs, int sub_bits, size_t n_subs, size_t coef_count, bool planes,
             int64_t* max_wgs) {
  FDET_REQUIRE(sub_bits >= 64 && sub_bits % 32 == 0 && sub_bits <= (1 << 20),
               "%s: sub_bits=%d must be a multiple of 32 between 64 and 2^20", who, sub_bits);
  FDET_REQUIRE(n_images > 0 && n_images <= 65535 && n_segs >= n_images && n_subs > 0 && n_subs <= 0x7fffffffu && scan_bytes > 0,
               "%s: bad sizes n_images=%d (1..65535) n_segs=%d n_subs=%zu scan_bytes=%zu", who, n_images, n_segs, n_subs,
               scan_bytes);
  FDET_REQUIRE(((uintptr_t)scan % 16) == 0, "%s: scan must be 16-byte aligned", who);
  int seg_at = 0;
  int64_t sub_at = 0, wgs = 0;
  for (int i = 0; i < n_images; ++i) {
    const fdet_jpeg_huff_image& I = h_images[i];
    FDET_REQUIRE((I.ncomp == 1 && I.hs == 1 && I.vs == 1) ||
                     (I.ncomp == 3 && ((I.hs == 1 && I.vs == 1) || (I.hs == 2 && I.vs == 1) || (I.hs == 2 && I.vs == 2))),
                 "%s: image %d: %d components with luma sampling %dx%d is outside the supported set", who, i, I.ncomp, I.hs, I.vs);
    FDET_REQUIRE(I.mcus_x > 0 && I.mcus_y > 0 && I.mcus_x <= 8192 && I.mcus_y <= 8192, "%s: image %d: bad MCU grid %dx%d", who, i,
                 I.mcus_x, I.mcus_y);
    const int64_t mcus = (int64_t)I.mcus_x * I.mcus_y;
    FDET_REQUIRE(I.seg_first == seg_at && I.seg_count > 0 && (int64_t)seg_at + I.seg_count <= n_segs && I.sub_first == sub_at &&
                     I.wg_first == wgs,
                 "%s: image %d: its segments / subsequences / workgroups do not follow those of the image before", who, i);
    if (planes) {
      for (int c = 0; c < I.ncomp; ++c) {
        const int64_t nb = mcus * (c == 0 ? I.hs * I.vs : 1);
        FDET_REQUIRE(I.coef_offset[c] >= 0 && (I.coef_offset[c] % 8) == 0 &&
                         (uint64_t)(I.coef_offset[c] + nb * 64) <= (uint64_t)coef_count,
                     "%s: image %d: coefficient plane %d at %lld (+%lld) is misaligned or past the %zu given", who, i, c,
                     (long long)I.coef_offset[c], (long long)(nb * 64), coef_count);
      }
    }
    int64_t mcu_at = 0, subs = 0;
    for (int s = seg_at; s < seg_at + I.seg_count; ++s) {
      const fdet_jpeg_huff_segment& S = h_segs[s];
      FDET_REQUIRE(S.byte_offset >= 0 && (S.byte_offset % 16) == 0 && S.byte_len >= 0 && S.byte_len < (1 << 27) &&
                       (uint64_t)(S.byte_offset + ((S.byte_len + 15) & ~15)) <= (uint64_t)scan_bytes,
                   "%s: segment %d: %d bytes at %lld are misaligned or outside the scan buffer of %zu bytes", who, s, S.byte_len,
                   (long long)S.byte_offset, scan_bytes);
      const int64_t want = S.byte_len == 0 ? 1 : ((int64_t)S.byte_len * 8 + sub_bits - 1) / sub_bits;
      FDET_REQUIRE(S.image == i && S.first_mcu == mcu_at && S.mcu_count > 0 && S.sub_first == sub_at + subs && S.sub_count == want,
                   "%s: segment %d: image, MCU range or subsequence range do not follow from its bytes and its neighbours", who, s);
      mcu_at += S.mcu_count;
      subs += want;
    }
    FDET_REQUIRE(mcu_at == mcus && I.sub_count == subs && (uint64_t)(sub_at + subs) <= (uint64_t)n_subs,
                 "%s: image %d: its segments cover %lld of %lld MCUs, or its %lld subsequences leave the state buffer", who, i,
                 (long long)mcu_at, (long long)mcus, (long long)subs);
    seg_at += I.seg_count;
    sub_at += subs;
    wgs += (subs + HUFF_THREADS - 1) / HUFF_THREADS;
  }
  FDET_REQUIRE(seg_at == n_segs, "%s: %d segments given, the images own %d", who, n_segs, seg_at);
  FDET_REQUIRE(wgs <= 0x7fffffffLL, "%s: %lld workgroups are more than one launch takes", who, (long long)wgs);
  *max_wgs = wgs;
  return FDET_OK;
}

}  // namespace

extern "C" int fdet_jpeg_huffman_sync(const uint8_t* scan, size_t scan_bytes, const fdet_jpeg_huff_tables* tables,
                                      const fdet_jpeg_huff_image* images, const fdet_jpeg_huff_image* h_images, int n_images,
                                      const fdet_jpeg_huff_segment* segs, const fdet_jpeg_huff_segment* h_segs, int n_segs,
                                      int sub_bits, uint64_t* state, size_t n_subs, uint32_t* changed, void* stream) {
  FDET_REQUIRE(scan && tables && images && h_images && segs && h_segs && state && changed, "jpeg_huffman_sync: null pointer");
  FDET_REQUIRE(((uintptr_t)state % 8) == 0 && ((uintptr_t)tables % 8) == 0, "jpeg_huffman_sync: state and tables must be 8-byte aligned");
  int64_t wgs = 0;
  if (int rc = validate("jpeg_huffman_sync", scan, scan_bytes, h_images, n_images, h_segs, n_segs, sub_bits, n_subs, 0, false, &wgs))
    return rc;
  hipLaunchKernelGGL(k_huff_sync, dim3((unsigned)wgs), dim3(HUFF_THREADS), 0, (hipStream_t)stream, scan, tables, images,
                     n_images, segs, sub_bits, state, changed);
  return check_launch("fdet_jpeg_huffman_sync");
}

extern "C" int fdet_jpeg_huffman_emit(const uint8_t* scan, size_t scan_bytes, const fdet_jpeg_huff_tables* tables,
                                      const fdet_jpeg_huff_image* images, const fdet_jpeg_huff_image* h_images, int n_images,
                                      const fdet_jpeg_huff_segment* segs, const fdet_jpeg_huff_segment* h_segs, int n_segs,
                                      int sub_bits, const uint64_t* state, size_t n_subs, uint32_t* first_block, int16_t* coef,
                                      size_t coef_count, uint32_t* flags, void* stream) {
  FDET_REQUIRE(scan && tables && images && h_images && segs && h_segs && state && first_block && coef && flags,
               "jpeg_huffman_emit: null pointer");
  FDET_REQUIRE(((uintptr_t)state % 8) == 0 && ((uintptr_t)tables % 8) == 0 && ((uintptr_t)coef % 16) == 0 && coef_count > 0,
               "jpeg_huffman_emit: state and tables must be 8-byte aligned, coef 16-byte aligned and not empty");
  int64_t wgs = 0;
  if (int rc = validate("jpeg_huffman_emit", scan, scan_bytes, h_images, n_images, h_segs, n_segs, sub_bits, n_subs, coef_count,
                        true, &wgs))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_huff_scan, dim3((unsigned)n_segs), dim3(HUFF_THREADS), 0, st, images, segs, state, first_block, flags);
  if (int rc = check_launch("fdet_jpeg_huffman_emit (scan)")) return rc;
  if (hipMemsetAsync(coef, 0, coef_count * sizeof(int16_t), st) != hipSuccess)
    return fail(FDET_ELAUNCH, "fdet_jpeg_huffman_emit: hipMemsetAsync failed");
  hipLaunchKernelGGL(k_huff_emit, dim3((unsigned)wgs), dim3(HUFF_THREADS), 0, st, scan, tables, images, n_images, segs, sub_bits,
                     state, first_block, coef, (uint64_t)coef_count, flags);
  if (int rc = check_launch("fdet_jpeg_huffman_emit (emit)")) return rc;
  hipLaunchKernelGGL(k_huff_dcsum, dim3((unsigned)n_segs, 3u), dim3(HUFF_THREADS), 0, st, images, segs, coef, (uint64_t)coef_count);
  return check_launch("fdet_jpeg_huffman_emit (dcsum)");
}
