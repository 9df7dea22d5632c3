// Baseline JPEG encode out of the device image bank: the mirror image of fdet_jpeg.hip with the entropy coder
// on the device as well, so that only the compressed scan crosses to the host.
//
//   host    fdet_jpeg_quant_tables   Annex K tables scaled by the quality (jcparam.c jpeg_set_quality)
//           fdet_jpeg_write_header   SOI APP0 DQT DQT SOF0 DHT x4 SOS, as jcmarker.c writes them at the defaults
//   device  fdet_jpeg_enc_plan       k_enc_fdct: RGB -> YCbCr, edge padding, chroma downsampling, jfdctint.c's forward DCT, quantisation
//                                                -> int16 coefficients, zigzag order, blocks in scan order, dummy blocks included
//                                    k_enc_bits: one thread per block: the exact bit length of its Huffman code
//                                    k_enc_scan: per image, exclusive scan of the lengths -> bit offsets and the image's total
//           fdet_jpeg_enc_emit       k_enc_emit: one thread per block writes its bits at its offset
//
// Every step is integer arithmetic in libjpeg (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jchuff.c), restated operation for
// operation: the file equals libjpeg-turbo's.  tests/jpeg_enc_cpu_ref.py restates it in numpy.  The two host functions make no
// HIP call and keep no mutable global state.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

// ------------------------------------------------------------------------------------------------------------------
// tables
// ------------------------------------------------------------------------------------------------------------------
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3 typical Huffman tables: bits[l - 1] = number of codes of length l, then the symbols in code order
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
     0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
     0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
     0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
     0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
     0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
     0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};

// The encoder's view of the four tables: entry = code << 5 | length (length 0: the symbol has no code).  Words 0..15 and
// 16..31 the two DC tables by category, 32..287 and 288..543 the two AC tables by run << 4 | category.
constexpr int ENC_WORDS = 32 + 2 * 256;
struct EncTab { uint32_t w[ENC_WORDS]; };

constexpr EncTab make_enc_tab() {
  EncTab T{};
  for (int t = 0; t < 2; ++t) {
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < kDcBits[t][l - 1]; ++i) T.w[16 * t + kDcVals[p++]] = (code++ << 5) | (uint32_t)l;
      code <<= 1;
    }
    code = 0;
    p = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < kAcBits[t][l - 1]; ++i) T.w[32 + 256 * t + kAcVals[t][p++]] = (code++ << 5) | (uint32_t)l;
      code <<= 1;
    }
  }
  return T;
}
__constant__ EncTab kEncTab = make_enc_tab();

struct ZigTab { uint8_t v[64]; };                        // natural index -> zigzag position
constexpr ZigTab make_zig_of() {
  ZigTab T{};
  for (int k = 0; k < 64; ++k) T.v[kZigzag[k]] = (uint8_t)k;
  return T;
}
__constant__ ZigTab kZigOf = make_zig_of();


void quant_tables(int quality, uint16_t* out) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      const int v = ((t ? kBaseChroma[k] : kBaseLuma[k]) * scale + 50) / 100;
      out[64 * t + k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

// natural order; travels to k_enc_fdct by value.  recip = 2^32 / d + 1 with d = 8 q, the quantiser's divisor: for every n < 2^16
// and d <= 2040, (n * recip) >> 32 == n / d (the error term n * (recip * d - 2^32) stays below 2^32), which the kernel uses
// in place of an integer division.
struct QTabs { uint16_t q[2][64]; uint32_t recip[2][64]; };

inline void fill_recip(QTabs& Q) {
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) Q.recip[t][k] = (uint32_t)((1ull << 32) / ((uint64_t)Q.q[t][k] << 3)) + 1u;
}

inline bool sub_ok(int s) { return s == FDET_JPEG_SUB_444 || s == FDET_JPEG_SUB_422 || s == FDET_JPEG_SUB_420; }

// ------------------------------------------------------------------------------------------------------------------
// device: colour conversion + padding + downsampling + forward DCT + quantisation
// ------------------------------------------------------------------------------------------------------------------
constexpr int FIX_SHIFT = 16;
constexpr int fixc(double x) { return (int)(x * 65536.0 + 0.5); }

// component c of the pixel at p (jccolor.c rgb_ycc_convert)
__device__ __forceinline__ int ycc_of(const uint8_t* __restrict__ p, int c) {
  const int r = p[0], g = p[1], b = p[2];
  if (c == 0) return (fixc(0.29900) * r + fixc(0.58700) * g + fixc(0.11400) * b + 32768) >> FIX_SHIFT;
  if (c == 1) return (-fixc(0.16874) * r - fixc(0.33126) * g + fixc(0.50000) * b + (128 << 16) + 32767) >> FIX_SHIFT;
  return (fixc(0.50000) * r - fixc(0.41869) * g - fixc(0.08131) * b + (128 << 16) + 32767) >> FIX_SHIFT;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one 8-point pass.  FIRST: the row pass (outputs scaled up by 2^PASS1_BITS); else the column pass.
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&o)[8]) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) { o[0] = (t10 + t11) << 2; o[4] = (t10 - t11) << 2; }
  else { o[0] = descale(t10 + t11, 2); o[4] = descale(t10 - t11, 2); }
  int z1 = (t12 + t13) * 4433;
  o[2] = descale(z1 + t13 * 6270, N);
  o[6] = descale(z1 - t12 * 15137, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o[7] = descale(m4 + z1 + z3, N);
  o[5] = descale(m5 + z2 + z4, N);
  o[3] = descale(m6 + z2 + z3, N);
  o[1] = descale(m7 + z1 + z4, N);
}

constexpr int ENC_WAVES = 4;           // waves per workgroup, eight 8x8 blocks per wave
constexpr int MID_PITCH = 72;          // int32 per block between the passes: 64 + 8, so that the column reads of a wave's 8
                                       // blocks fall on 64 different banks
constexpr int OUT_PITCH = 72;          // int16 per block of quantised coefficients on their way to zigzag order

struct BlockPos { int comp, bx, by; bool dummy; };

// Block `blk` of an image in scan order -> its component and block coordinates in that component's grid.  A dummy luma block
// (outside the real_bw x real_bh blocks the image covers) takes the coordinates of the nearest real block before it in its
// MCU: it repeats that block's DC.  The first block of an MCU is always real.
__device__ __forceinline__ BlockPos block_pos(int blk, int hs, int vs, int mcus_x, int real_bw, int real_bh) {
  const int per = hs * vs + 2;
  const int m = blk / per, k = blk - m * per;
  const int my = m / mcus_x, mx = m - my * mcus_x;
  BlockPos P;
  if (k >= hs * vs) { P.comp = k - hs * vs + 1; P.bx = mx; P.by = my; P.dummy = false; return P; }
  int kk = k;
  while (kk > 0 && !(mx * hs + (kk % hs) < real_bw && my * vs + (kk / hs) < real_bh)) --kk;
  P.comp = 0; P.bx = mx * hs + (kk % hs); P.by = my * vs + (kk / hs); P.dummy = kk != k;
  return P;
}

// grid (groups of 4 x 8 blocks, image).  Lane l of a wave: block l >> 3 of its eight, sample row l & 7.  It builds its 8 samples
// from the bank (the bytes sit at any alignment), runs the row pass in registers, transposes through LDS, runs column l & 7,
// quantises, scatters to zigzag order in LDS, and stores 8 coefficients with one 16-byte store (a wave writes 1 KiB contiguously).
__global__ void __launch_bounds__(256)
k_enc_fdct(const uint8_t* __restrict__ bank, const fdet_jpeg_enc_desc* __restrict__ descs, QTabs Q, int hs, int vs,
           int16_t* __restrict__ coef) {
  __shared__ __attribute__((aligned(16))) int32_t mid[ENC_WAVES][8 * MID_PITCH];
  __shared__ __attribute__((aligned(16))) int16_t outz[ENC_WAVES][8 * OUT_PITCH];
  __shared__ uint8_t zig_of[64];                         // natural index -> zigzag position
  const fdet_jpeg_enc_desc* D = descs + blockIdx.y;
  const int W = D->width, H = D->height, nb = D->n_blocks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = lane >> 3, j = lane & 7;
  if (threadIdx.x < 64) zig_of[threadIdx.x] = kZigOf.v[threadIdx.x];
  const int blk_raw = (blockIdx.x * ENC_WAVES + wave) * 8 + b;
  const bool active = blk_raw < nb;
  const int blk = active ? blk_raw : nb - 1;             // idle lanes redo the last block (every lane reaches the barriers)
  const BlockPos P = block_pos(blk, hs, vs, D->mcus_x, (W + 7) >> 3, (H + 7) >> 3);
  const uint8_t* img = bank + D->bank_offset;
  int d[8], o[8];
  const int sy = P.by * 8 + j, sx = P.bx * 8;
  if (P.comp == 0 || hs == 1) {
    const uint8_t* row = img + (int64_t)min(sy, H - 1) * W * 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = ycc_of(row + min(sx + i, W - 1) * 3, P.comp) - 128;
  } else if (vs == 1) {                                  // h2v1: (a + b + bias) >> 1, bias 0, 1, 0, 1, ... by output column
    const uint8_t* row = img + (int64_t)min(sy, H - 1) * W * 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int x0 = min(2 * (sx + i), W - 1), x1 = min(2 * (sx + i) + 1, W - 1);
      d[i] = ((ycc_of(row + x0 * 3, P.comp) + ycc_of(row + x1 * 3, P.comp) + (i & 1)) >> 1) - 128;
    }
  } else {                                               // h2v2: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ...
    const int rd = min(sy, ((H + 1) >> 1) - 1);          // rows past the last downsampled row repeat THAT row
    const uint8_t* r0 = img + (int64_t)min(2 * rd, H - 1) * W * 3;
    const uint8_t* r1 = img + (int64_t)min(2 * rd + 1, H - 1) * W * 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int x0 = min(2 * (sx + i), W - 1) * 3, x1 = min(2 * (sx + i) + 1, W - 1) * 3;
      d[i] = ((ycc_of(r0 + x0, P.comp) + ycc_of(r0 + x1, P.comp) + ycc_of(r1 + x0, P.comp) + ycc_of(r1 + x1, P.comp) + 1 + (i & 1)) >> 2) - 128;
    }
  }
  fdct8<true>(d, o);                                     // pass 1: sample row j
  int32_t* M = &mid[wave][b * MID_PITCH];
  *reinterpret_cast<int4*>(M + j * 8) = make_int4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<int4*>(M + j * 8 + 4) = make_int4(o[4], o[5], o[6], o[7]);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) d[r] = M[r * 8 + j];
  fdct8<false>(d, o);                                    // pass 2: column j; o[r] is the coefficient at row r, column j
  const uint16_t* q = Q.q[P.comp ? 1 : 0];
  const uint32_t* qr = Q.recip[P.comp ? 1 : 0];
  int16_t* Z = &outz[wave][b * OUT_PITCH];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = r * 8 + j;
    const int div = (int)q[n] << 3;                      // the FDCT leaves its output scaled up by 8
    const int a = o[r] < 0 ? -o[r] : o[r];
    int v = (int)__umulhi((unsigned)(a + (div >> 1)), qr[n]);       // (a + div / 2) / div: |a| < 2^14 here
    v = o[r] < 0 ? -v : v;
    if (P.dummy && n != 0) v = 0;
    Z[zig_of[n]] = (int16_t)v;
  }
  __syncthreads();
  if (active)
    *reinterpret_cast<uint4*>(coef + (D->block_base + blk) * 64 + j * 8) = *reinterpret_cast<const uint4*>(Z + j * 8);
}

// ------------------------------------------------------------------------------------------------------------------
// device: entropy coding.  One walk over a block's 64 coefficients serves both phases: COUNT sums the code lengths, EMIT
// writes the same bits.
// ------------------------------------------------------------------------------------------------------------------
// Bits of an image's stream, most significant first.  The buffer was zero-filled; a block ORs the words it shares with its
// neighbours (its first word when it starts inside one, its last partial word) and stores the words it owns.
struct BitWriter {
  uint32_t* words;         // the image's stream
  uint32_t at;             // index of the word `acc` is filling
  uint64_t acc;            // the low `fill` bits are that word's bits so far
  int fill;
  bool shared;             // the word being filled has bits of the block before this one

  __device__ __forceinline__ void put(uint32_t code, int n) {
    acc = (acc << n) | code;
    fill += n;
    if (fill >= 32) {
      const uint32_t w = __builtin_bswap32((uint32_t)(acc >> (fill - 32)));
      if (shared) atomicOr(words + at, w);
      else words[at] = w;
      shared = false;
      ++at;
      fill -= 32;
      acc &= (1ull << fill) - 1ull;
    }
  }
  __device__ __forceinline__ void finish() {
    if (fill > 0) atomicOr(words + at, __builtin_bswap32((uint32_t)(acc << (32 - fill))));
  }
};

struct BitCounter {
  uint32_t bits;
  __device__ __forceinline__ void put(uint32_t, int n) { bits += (uint32_t)n; }
};

template <class SINK>
__device__ __forceinline__ void put_value(SINK& S, const uint32_t* __restrict__ tab, int sym_base, int run, int v) {
  const int a = v < 0 ? -v : v;
  const int n = a ? 32 - __builtin_clz((unsigned)a) : 0;
  const uint32_t e = tab[sym_base + ((run << 4) | n)];
  S.put(e >> 5, (int)(e & 31u));
  if (n) S.put((uint32_t)(v < 0 ? v + (1 << n) - 1 : v) & ((1u << n) - 1u), n);
}

// zz: the block's 64 coefficients in zigzag order (16-byte aligned); pred: the DC it is predicted from; ct: 0 luma, 1 chroma
template <class SINK>
__device__ __forceinline__ void code_block(SINK& S, const uint32_t* __restrict__ tab, const int16_t* __restrict__ zz, int pred, int ct) {
  const int dc_base = 16 * ct, ac_base = 32 + 256 * ct;
  int run = 0;
#pragma unroll 1
  for (int g = 0; g < 8; ++g) {
    const uint4 raw = *reinterpret_cast<const uint4*>(zz + g * 8);
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = (int)(int16_t)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
      if (g == 0 && i == 0) {
        put_value(S, tab, dc_base, 0, v - pred);
      } else if (v == 0) {
        ++run;
      } else {
        while (run > 15) {
          const uint32_t e = tab[ac_base + 0xF0];
          S.put(e >> 5, (int)(e & 31u));
          run -= 16;
        }
        put_value(S, tab, ac_base, run, v);
        run = 0;
      }
    }
  }
  if (run) {
    const uint32_t e = tab[ac_base];
    S.put(e >> 5, (int)(e & 31u));
  }
}

// The block a block's DC is predicted from: the previous block of its component in scan order; -1 for the first.
__device__ __forceinline__ int pred_block(int blk, int hs, int vs, int& ct) {
  const int nl = hs * vs, per = nl + 2;
  const int m = blk / per, k = blk - m * per;
  ct = k >= nl;
  if (k > 0 && k < nl) return blk - 1;
  if (m == 0) return -1;
  return k == 0 ? blk - 3 : blk - per;                   // the last luma block of the MCU before / the same chroma block there
}

__device__ __forceinline__ void load_enc_tab(uint32_t* tab) {
  for (int i = threadIdx.x; i < ENC_WORDS; i += blockDim.x) tab[i] = kEncTab.w[i];
  __syncthreads();
}

// grid (256 blocks of the image, image): bits[block] = the length of its code
__global__ void __launch_bounds__(256)
k_enc_bits(const fdet_jpeg_enc_desc* __restrict__ descs, int hs, int vs, const int16_t* __restrict__ coef, uint32_t* __restrict__ bits) {
  __shared__ uint32_t tab[ENC_WORDS];
  load_enc_tab(tab);
  const fdet_jpeg_enc_desc* D = descs + blockIdx.y;
  const int blk = blockIdx.x * 256 + threadIdx.x;
  if (blk >= D->n_blocks) return;
  const int16_t* base = coef + D->block_base * 64;
  int ct;
  const int pb = pred_block(blk, hs, vs, ct);
  const int pred = pb < 0 ? 0 : (int)base[(int64_t)pb * 64];
  BitCounter S{0u};
  code_block(S, tab, base + (int64_t)blk * 64, pred, ct);
  bits[D->block_base + blk] = S.bits;
}

// grid (image): one workgroup walks the image's blocks 256 at a time with a running carry.
__global__ void __launch_bounds__(256)
k_enc_scan(const fdet_jpeg_enc_desc* __restrict__ descs, const uint32_t* __restrict__ bits, uint32_t* __restrict__ start,
           uint32_t* __restrict__ total) {
  __shared__ uint32_t part[256];
  const fdet_jpeg_enc_desc* D = descs + blockIdx.x;
  const int nb = D->n_blocks;
  const int64_t base = D->block_base;
  uint32_t carry = 0;
  for (int at = 0; at < nb; at += 256) {
    const int i = at + (int)threadIdx.x;
    const uint32_t v = i < nb ? bits[base + i] : 0u;
    part[threadIdx.x] = v;
    __syncthreads();
    uint32_t s = v;
    for (int off = 1; off < 256; off <<= 1) {            // inclusive scan, Hillis-Steele
      const uint32_t add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
      __syncthreads();
      s += add;
      part[threadIdx.x] = s;
      __syncthreads();
    }
    if (i < nb) start[base + i] = carry + s - v;
    carry += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

// grid (256 blocks of the image, image): every block writes its code at its bit offset; the image's last block adds the
// 1-bits that pad the stream to a byte.
__global__ void __launch_bounds__(256)
k_enc_emit(const fdet_jpeg_enc_desc* __restrict__ descs, int hs, int vs, const int16_t* __restrict__ coef,
           const uint32_t* __restrict__ start, uint8_t* __restrict__ scan) {
  __shared__ uint32_t tab[ENC_WORDS];
  load_enc_tab(tab);
  const fdet_jpeg_enc_desc* D = descs + blockIdx.y;
  const int blk = blockIdx.x * 256 + threadIdx.x;
  if (blk >= D->n_blocks) return;
  const int16_t* base = coef + D->block_base * 64;
  int ct;
  const int pb = pred_block(blk, hs, vs, ct);
  const int pred = pb < 0 ? 0 : (int)base[(int64_t)pb * 64];
  const uint32_t s = start[D->block_base + blk];
  BitWriter S{reinterpret_cast<uint32_t*>(scan + D->scan_offset), s >> 5, 0ull, (int)(s & 31u), (s & 31u) != 0u};
  code_block(S, tab, base + (int64_t)blk * 64, pred, ct);
  if (blk == D->n_blocks - 1) {
    const int used = (int)((S.at * 32u + (uint32_t)S.fill) & 7u);
    if (used) S.put((1u << (8 - used)) - 1u, 8 - used);
  }
  S.finish();
}

// ------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------
struct Layout { size_t bits, start, total, end; };

inline Layout layout(int64_t B, int n) {
  Layout L;
  L.bits = (size_t)B * 128;
  L.start = L.bits + (size_t)B * 4;
  L.total = L.start + (size_t)B * 4;
  L.end = L.total + (size_t)n * 4;
  return L;
}

constexpr int64_t MAX_TOTAL_BLOCKS = (int64_t)1 << 34;

// The descriptors of a call: sizes, MCU grids and the dense block numbering.  -> the call's block total in *B, the largest image in *most.
int check_descs(const char* who, const fdet_jpeg_enc_desc* h, int n, int subsampling, int64_t* B, int* most) {
  FDET_REQUIRE(n > 0 && n <= 65535, "%s: n_images=%d outside 1..65535", who, n);
  FDET_REQUIRE(sub_ok(subsampling), "%s: subsampling=%d is not FDET_JPEG_SUB_444 | _422 | _420", who, subsampling);
  const int hs = subsampling == FDET_JPEG_SUB_444 ? 1 : 2, vs = subsampling == FDET_JPEG_SUB_420 ? 2 : 1;
  int64_t at = 0;
  int mx = 0;
  for (int i = 0; i < n; ++i) {
    const fdet_jpeg_enc_desc& I = h[i];
    FDET_REQUIRE(I.width >= 1 && I.height >= 1 && I.width <= 65535 && I.height <= 65535, "%s: image %d: bad size %dx%d (1..65535)",
                 who, i, I.width, I.height);
    FDET_REQUIRE(I.mcus_x == (I.width + 8 * hs - 1) / (8 * hs) && I.mcus_y == (I.height + 8 * vs - 1) / (8 * vs),
                 "%s: image %d: an MCU grid of %dx%d is not that of %dx%d pixels", who, i, I.mcus_x, I.mcus_y, I.width, I.height);
    const int64_t nb = (int64_t)I.mcus_x * I.mcus_y * (hs * vs + 2);
    FDET_REQUIRE(nb <= FDET_JPEG_ENC_MAX_BLOCKS && I.n_blocks == (int32_t)nb, "%s: image %d: n_blocks=%d, its grid has %lld (at most %d)",
                 who, i, I.n_blocks, (long long)nb, FDET_JPEG_ENC_MAX_BLOCKS);
    FDET_REQUIRE(I.block_base == at, "%s: image %d: block_base=%lld does not continue the image before it (%lld)", who, i,
                 (long long)I.block_base, (long long)at);
    at += nb;
    mx = I.n_blocks > mx ? I.n_blocks : mx;
  }
  *B = at;
  *most = mx;
  return FDET_OK;
}

struct Out {
  uint8_t* p;
  size_t n;
  void u8(int v) { p[n++] = (uint8_t)v; }
  void u16(int v) { u8(v >> 8); u8(v & 255); }
};

}  // namespace

extern "C" int fdet_jpeg_quant_tables(int quality, uint16_t* out) {
  FDET_REQUIRE(out, "jpeg_quant_tables: null pointer");
  FDET_REQUIRE(quality >= 1 && quality <= 100, "jpeg_quant_tables: quality=%d outside 1..100", quality);
  quant_tables(quality, out);
  return FDET_OK;
}

extern "C" int fdet_jpeg_write_header(int width, int height, int quality, int subsampling, uint8_t* out, size_t capacity, size_t* n) {
  FDET_REQUIRE(out && n, "jpeg_write_header: null pointer");
  FDET_REQUIRE(width >= 1 && height >= 1 && width <= 65535 && height <= 65535, "jpeg_write_header: bad size %dx%d (1..65535)", width,
               height);
  FDET_REQUIRE(quality >= 1 && quality <= 100, "jpeg_write_header: quality=%d outside 1..100", quality);
  FDET_REQUIRE(sub_ok(subsampling), "jpeg_write_header: subsampling=%d is not FDET_JPEG_SUB_444 | _422 | _420", subsampling);
  *n = FDET_JPEG_ENC_HEADER_BYTES;
  if (capacity < FDET_JPEG_ENC_HEADER_BYTES)
    return fail(FDET_EWORKSPACE, "jpeg_write_header: the header takes %d bytes, the buffer holds %zu", FDET_JPEG_ENC_HEADER_BYTES, capacity);
  uint16_t qt[128];
  quant_tables(quality, qt);
  Out O{out, 0};
  O.u16(0xFFD8);
  O.u16(0xFFE0); O.u16(16);                              // APP0: JFIF 1.01, no units, density 1x1, no thumbnail
  O.u8('J'); O.u8('F'); O.u8('I'); O.u8('F'); O.u8(0);
  O.u8(1); O.u8(1); O.u8(0); O.u16(1); O.u16(1); O.u8(0); O.u8(0);
  for (int t = 0; t < 2; ++t) {
    O.u16(0xFFDB); O.u16(67); O.u8(t);
    for (int k = 0; k < 64; ++k) O.u8(qt[64 * t + kZigzag[k]]);
  }
  O.u16(0xFFC0); O.u16(17); O.u8(8); O.u16(height); O.u16(width); O.u8(3);
  const int hs = subsampling == FDET_JPEG_SUB_444 ? 1 : 2, vs = subsampling == FDET_JPEG_SUB_420 ? 2 : 1;
  O.u8(1); O.u8(hs << 4 | vs); O.u8(0);
  O.u8(2); O.u8(0x11); O.u8(1);
  O.u8(3); O.u8(0x11); O.u8(1);
  for (int t = 0; t < 2; ++t) {                          // DC t, AC t
    O.u16(0xFFC4); O.u16(2 + 1 + 16 + 12); O.u8(t);
    for (int l = 0; l < 16; ++l) O.u8(kDcBits[t][l]);
    for (int k = 0; k < 12; ++k) O.u8(kDcVals[k]);
    O.u16(0xFFC4); O.u16(2 + 1 + 16 + 162); O.u8(0x10 | t);
    for (int l = 0; l < 16; ++l) O.u8(kAcBits[t][l]);
    for (int k = 0; k < 162; ++k) O.u8(kAcVals[t][k]);
  }
  O.u16(0xFFDA); O.u16(12); O.u8(3);
  O.u8(1); O.u8(0x00); O.u8(2); O.u8(0x11); O.u8(3); O.u8(0x11);
  O.u8(0); O.u8(63); O.u8(0);
  if (O.n != FDET_JPEG_ENC_HEADER_BYTES) return fail(FDET_EINVAL, "jpeg_write_header: wrote %zu bytes, not %d", O.n, FDET_JPEG_ENC_HEADER_BYTES);
  return FDET_OK;
}

extern "C" size_t fdet_jpeg_enc_ws_bytes(int64_t total_blocks, int n_images) {
  if (total_blocks < 1 || total_blocks > MAX_TOTAL_BLOCKS || n_images < 1 || n_images > 65535) return 0;
  return layout(total_blocks, n_images).end;
}

extern "C" int fdet_jpeg_enc_plan(const uint8_t* bank, size_t bank_bytes, const fdet_jpeg_enc_desc* descs,
                                  const fdet_jpeg_enc_desc* h_descs, int n_images, int quality, int subsampling, uint8_t* workspace,
                                  size_t workspace_bytes, void* stream) {
  FDET_REQUIRE(bank && descs && h_descs && workspace, "jpeg_enc_plan: null pointer");
  FDET_REQUIRE(quality >= 1 && quality <= 100, "jpeg_enc_plan: quality=%d outside 1..100", quality);
  FDET_REQUIRE(((uintptr_t)workspace % 16) == 0, "jpeg_enc_plan: the workspace must be 16-byte aligned");
  int64_t B = 0;
  int most = 0;
  if (int rc = check_descs("jpeg_enc_plan", h_descs, n_images, subsampling, &B, &most)) return rc;
  for (int i = 0; i < n_images; ++i) {
    const fdet_jpeg_enc_desc& I = h_descs[i];
    const int64_t nbytes = (int64_t)I.width * I.height * 3;
    FDET_REQUIRE(I.bank_offset >= 0 && (uint64_t)I.bank_offset + (uint64_t)nbytes <= (uint64_t)bank_bytes,
                 "jpeg_enc_plan: image %d: %lld bytes at offset %lld run past the bank of %zu bytes", i, (long long)nbytes,
                 (long long)I.bank_offset, bank_bytes);
  }
  const Layout L = layout(B, n_images);
  if (B > MAX_TOTAL_BLOCKS || workspace_bytes < L.end)
    return fail(FDET_EWORKSPACE, "jpeg_enc_plan: %lld blocks of %d images need a workspace of %zu bytes, %zu given", (long long)B,
                n_images, L.end, workspace_bytes);
  const int hs = subsampling == FDET_JPEG_SUB_444 ? 1 : 2, vs = subsampling == FDET_JPEG_SUB_420 ? 2 : 1;
  QTabs Q;
  quant_tables(quality, &Q.q[0][0]);
  fill_recip(Q);
  int16_t* coef = reinterpret_cast<int16_t*>(workspace);
  uint32_t* bits = reinterpret_cast<uint32_t*>(workspace + L.bits);
  uint32_t* start = reinterpret_cast<uint32_t*>(workspace + L.start);
  uint32_t* total = reinterpret_cast<uint32_t*>(workspace + L.total);
  const dim3 g1((unsigned)((most + ENC_WAVES * 8 - 1) / (ENC_WAVES * 8)), (unsigned)n_images);
  hipLaunchKernelGGL(k_enc_fdct, g1, dim3(256), 0, (hipStream_t)stream, bank, descs, Q, hs, vs, coef);
  if (int rc = check_launch("fdet_jpeg_enc_plan (fdct)")) return rc;
  const dim3 g2((unsigned)((most + 255) / 256), (unsigned)n_images);
  hipLaunchKernelGGL(k_enc_bits, g2, dim3(256), 0, (hipStream_t)stream, descs, hs, vs, (const int16_t*)coef, bits);
  if (int rc = check_launch("fdet_jpeg_enc_plan (bits)")) return rc;
  hipLaunchKernelGGL(k_enc_scan, dim3((unsigned)n_images), dim3(256), 0, (hipStream_t)stream, descs, (const uint32_t*)bits, start, total);
  return check_launch("fdet_jpeg_enc_plan (scan)");
}

extern "C" int fdet_jpeg_enc_emit(const fdet_jpeg_enc_desc* descs, const fdet_jpeg_enc_desc* h_descs, const uint32_t* h_totals,
                                  int n_images, int subsampling, const uint8_t* workspace, size_t workspace_bytes, uint8_t* scan,
                                  size_t scan_bytes, void* stream) {
  FDET_REQUIRE(descs && h_descs && h_totals && workspace && scan, "jpeg_enc_emit: null pointer");
  FDET_REQUIRE(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)scan % 4) == 0,
               "jpeg_enc_emit: the workspace must be 16-byte aligned, the scan buffer 4-byte aligned");
  int64_t B = 0;
  int most = 0;
  if (int rc = check_descs("jpeg_enc_emit", h_descs, n_images, subsampling, &B, &most)) return rc;
  const Layout L = layout(B, n_images);
  if (workspace_bytes < L.end)
    return fail(FDET_EWORKSPACE, "jpeg_enc_emit: %lld blocks of %d images take a workspace of %zu bytes, %zu given", (long long)B,
                n_images, L.end, workspace_bytes);
  uint64_t at = 0;
  for (int i = 0; i < n_images; ++i) {
    const fdet_jpeg_enc_desc& I = h_descs[i];
    FDET_REQUIRE(h_totals[i] >= 1 && (uint64_t)h_totals[i] <= (uint64_t)I.n_blocks * FDET_JPEG_ENC_MAX_BLOCK_BITS,
                 "jpeg_enc_emit: image %d: a total of %u bits is outside what its %d blocks can take", i, h_totals[i], I.n_blocks);
    const uint64_t span = (((uint64_t)h_totals[i] + 7) / 8 + 3) / 4 * 4;
    FDET_REQUIRE(I.scan_offset >= 0 && (I.scan_offset % 4) == 0 && (uint64_t)I.scan_offset >= at &&
                     (uint64_t)I.scan_offset + span <= (uint64_t)scan_bytes,
                 "jpeg_enc_emit: image %d: %llu bytes at scan offset %lld are misaligned, overlap the image before or run past the %zu given",
                 i, (unsigned long long)span, (long long)I.scan_offset, scan_bytes);
    at = (uint64_t)I.scan_offset + span;
  }
  const int hs = subsampling == FDET_JPEG_SUB_444 ? 1 : 2, vs = subsampling == FDET_JPEG_SUB_420 ? 2 : 1;
  const int16_t* coef = reinterpret_cast<const int16_t*>(workspace);
  const uint32_t* start = reinterpret_cast<const uint32_t*>(workspace + L.start);
  const dim3 g((unsigned)((most + 255) / 256), (unsigned)n_images);
  hipLaunchKernelGGL(k_enc_emit, g, dim3(256), 0, (hipStream_t)stream, descs, hs, vs, coef, start, scan);
  return check_launch("fdet_jpeg_enc_emit");
}
