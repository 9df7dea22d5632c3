// PoolResnet stem (Conv2d(3,F,10,stride 8,pad 2)) in bf16x3 arithmetic (x = hi + lo bf16 split,
// three MFMA passes, fp32 accumulation): forward.
//
// One band = one output row (n, oy).  MFMA K = one (ci, ky) input row segment of 16 taps:
//   t = kx + 2 in [0,16)  (taps outside [2,12) carry zero weights)
// so a lane's B fragment for output column ox and k-half h is the 8 consecutive input pixels
// 8*ox + 8*h + j - 4 ... stored row-major with a 4-element zero pad: LDS index 8*ox + 8*h + j --
// one aligned 16-byte read, consecutive lanes -> consecutive chunks (no de-interleave needed, the
// stride-8 of the conv turns into the natural 8-element fragment granularity).
// Weights live in registers for the whole kernel (30 rows x (hi,lo) x 4 VGPRs = 240 per lane).
#include "fdet_common.h"
#include "fdet_ps.h"
#include "fdet_q8_common.h"
#include <algorithm>
#include <cstdlib>
#include <utility>

using namespace fdet;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int KS = 10, ST = 8, PD = 2, CIN = 3;
constexpr int NROW = CIN * KS;             // 30 (ci, ky) rows = MFMA K steps
constexpr int RL = 8 * 64 + 16;            // row length in elements (chunks: 66)
constexpr int RC = RL / 8;
constexpr int NSLOT = 15;                  // float4 staging slots per thread: 30 rows x 128 lanes / 256

struct StemX3Args {
  const float* x; const float* w; const float* bias; float* y;
  int N, F, H, W, Ho, Wo, nrows;
  // PS output (fdet_ps.h) of the pipelined kernel: y is then the image-0 pointer of a PS tensor (F == 64)
  int ps_hp, ps_wp, ps_plane, ps_img;
  // Q8 output of the pipelined kernel: y is an int8 [N][Ho+2][Wo+2][64] tensor (fdet.h "Int8 inference"), ps_hp / ps_wp its
  // padded extent, ps_img its image size in 16-byte units, q_inv = 1.0f / scale
  float q_inv;
};

__global__ void __launch_bounds__(256, 1)
k_stem_fwd_x3(const StemX3Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* Xh = reinterpret_cast<__bf16*>(smem);         // [30][RL]
  __bf16* Xl = Xh + NROW * RL;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int m = wid & 1, nt = wid >> 1;
  const int cob = blockIdx.y;
  const int co = cob * 64 + m * 32 + l31;
  const int jmax = a.W / 4;

  {
    f32x4* z = reinterpret_cast<f32x4*>(smem);
    for (int t = tid; t < NROW * RL * 4 / 16; t += 256) z[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // A fragments: row rr = ci*10 + ky, element j <-> tap t = 8*half + j, kx = t - 2
  bf16x8 ah[NROW], al[NROW];
#pragma unroll
  for (int rr = 0; rr < NROW; ++rr) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kx = 8 * half + j - 2;
      const float f = (co < a.F && kx >= 0 && kx < KS) ? a.w[((size_t)co * CIN * KS + rr) * KS + kx] : 0.f;
      const __bf16 h = (__bf16)f;
      ah[rr][j] = h;
      al[rr][j] = (__bf16)(f - (float)h);
    }
  }
  const bf16x8* Bh = reinterpret_cast<const bf16x8*>(Xh) + nt * 32 + l31 + half;
  const bf16x8* Bl = reinterpret_cast<const bf16x8*>(Xl) + nt * 32 + l31 + half;

  f32x4 px[NSLOT];
#define SX3_LOAD(ROW_N, ROW_OY)                                                                 \
  {                                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < NSLOT; ++s_) {                                      \
      const int it = s_ * 256 + tid;                                                            \
      const int rr = it >> 7, j = it & 127;                                                     \
      const int ci = rr / KS, ky = rr - ci * KS;                                                \
      const int iy = (ROW_OY) * ST - PD + ky;                                                   \
      const bool ok = j < jmax && iy >= 0 && iy < a.H;                                          \
      px[s_] = ok ? *reinterpret_cast<const f32x4*>(a.x + (((size_t)(ROW_N) * CIN + ci) * a.H + iy) * a.W + j * 4) \
                  : f32x4{0.f, 0.f, 0.f, 0.f};                                                  \
    }                                                                                           \
  }
#define SX3_STORE()                                                                             \
  {                                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < NSLOT; ++s_) {                                      \
      const int it = s_ * 256 + tid;                                                            \
      const int rr = it >> 7, j = it & 127;                                                     \
      if (j < jmax) {                                                                           \
        bf16x4 h4, l4;                                                                          \
        _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_) {                                      \
          const __bf16 h = (__bf16)px[s_][c_];                                                  \
          h4[c_] = h; l4[c_] = (__bf16)(px[s_][c_] - (float)h);                                 \
        }                                                                                       \
        *reinterpret_cast<bf16x4*>(Xh + rr * RL + 4 + 4 * j) = h4;                              \
        *reinterpret_cast<bf16x4*>(Xl + rr * RL + 4 + 4 * j) = l4;                              \
      }                                                                                         \
    }                                                                                           \
  }

  int row = blockIdx.x;
  if (row < a.nrows) { const int n = row / a.Ho, oy = row - n * a.Ho; SX3_LOAD(n, oy) }
  for (; row < a.nrows; row += gridDim.x) {
    const int n = row / a.Ho, oy = row - n * a.Ho;
    __syncthreads();
    SX3_STORE()
    __syncthreads();
    const int nrow = row + gridDim.x;
    if (nrow < a.nrows) { const int n2 = nrow / a.Ho, oy2 = nrow - n2 * a.Ho; SX3_LOAD(n2, oy2) }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    bf16x8 bh[2], bl[2];
    bh[0] = Bh[0]; bl[0] = Bl[0];
#pragma unroll
    for (int rr = 0; rr < NROW; ++rr) {
      const int cur = rr & 1, nxt = cur ^ 1;
      if (rr + 1 < NROW) { bh[nxt] = Bh[(rr + 1) * RC]; bl[nxt] = Bl[(rr + 1) * RC]; }
      __builtin_amdgcn_sched_barrier(0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], bl[cur], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rr], bh[cur], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], bh[cur], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    const int ox = nt * 32 + l31;
    if (ox < a.Wo) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c2 = cob * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (c2 < a.F) a.y[(((size_t)n * a.F + c2) * a.Ho + oy) * a.Wo + ox] = acc[r] + a.bias[c2];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Pipelined forward (same tiles, arithmetic and results): TWO LDS tiles and contiguous output rows
// per workgroup.  While the 90 MFMAs of output row b run on tile b & 1, the hi/lo split + LDS writes
// of row b+1 (its 30 input rows already in registers) ride one float4 per MFMA k-step, and the
// global loads of row b+3 follow four steps behind the job that freed their register: asm buffer
// loads (branch-free: padded / out-of-image elements are out-of-range offsets that return zero)
// into two register sets, one in accumulation registers, one in arch VGPRs, waited for with a
// counted vmcnt one whole row later (the 16 output stores of a row count in that queue too).
// See the pipelined weight gradient (fdet_wgrad3x3_x3.hip) for why the staging must not be a
// burst: a wave issues in order, and a burst of loads / LDS writes keeps it from issuing MFMAs.
// ---------------------------------------------------------------------------------------
// compile-time loop: the body sees its index as a constant expression, so register arrays indexed by it
// are promoted to registers before any unrolling decision (asm outputs into a stack array would be
// stored to scratch right behind the asm load, before the data has landed)
template <int... I, class F>
__device__ __forceinline__ void sx_static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void sx_static_for(F&& f) { sx_static_for_impl(std::make_integer_sequence<int, N>{}, f); }
#define SX_LAMBDA(I) [&](auto I) __attribute__((always_inline))

typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
template <bool AG>
__device__ __forceinline__ void sx_aload(f32x4& d, unsigned off, const u32x4s& rs) {
  if constexpr (AG) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=a"(d) : "v"(off), "s"(rs));
  else asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(d) : "v"(off), "s"(rs));
}
template <bool AG>
__device__ __forceinline__ void sx_apass(f32x4& d) {
  if constexpr (AG) asm volatile("" : "+a"(d)); else asm volatile("" : "+v"(d));
}
// the same for ONE dword (four uint8 pixels; U8 instantiations)
template <bool AG>
__device__ __forceinline__ void sx_aload1(unsigned& d, unsigned off, const u32x4s& rs) {
  if constexpr (AG) asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=a"(d) : "v"(off), "s"(rs));
  else asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(d) : "v"(off), "s"(rs));
}
template <bool AG>
__device__ __forceinline__ void sx_apass1(unsigned& d) {
  if constexpr (AG) asm volatile("" : "+a"(d)); else asm volatile("" : "+v"(d));
}
__device__ __forceinline__ void sx_split_pair(float f0, float f1, unsigned& hi, unsigned& lo) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t h = {(__bf16)f0, (__bf16)f1};
  hi = __builtin_bit_cast(unsigned, h);
  const f32x2_t hf = {__builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
  const f32x2_t l = f32x2_t{f0, f1} - hf;
  const bf16x2_t lb = {(__bf16)l[0], (__bf16)l[1]};
  lo = __builtin_bit_cast(unsigned, lb);
}

__device__ __forceinline__ unsigned sx_hi_pair(float f0, float f1) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t h = {(__bf16)f0, (__bf16)f1};
  return __builtin_bit_cast(unsigned, h);
}

// P16 (precision16, PS output only): one MFMA pass on bf16(x) x bf16(w); the lo halves are neither computed nor staged and
// only the hi plane of the output is written.
// U8 (inference, PS output only): the input is the uint8 frame itself -- `x / 255` (models/PoolResnet.py:95) happens in the
// staging job through a 256-entry table of (bf16 hi | bf16 lo) pairs of p / 255 in LDS, i.e. the values the fp32 path splits
// out of fdet_u8_to_f32_norm's output, bit for bit; a slot loads one dword (4 pixels) instead of a float4, and the fp32 image
// (2.76 MB per frame written and read back) never exists.
// Q8 (int8 inference, with PSO and U8, not P16): the epilogue quantises the fp32 value acc + bias that the fp32-output form
// stores -- q = clamp(rintf(v * q_inv), -127, 127), NaN -> 0, as fdet_q8_quantize -- and writes the int8 trunk's layout
// [N][Ho+2][Wo+2][64], real pixels only: after one v_permlane32_swap a lane holds the 8 consecutive channels of one group of
// its pixel as two dwords, one 8-byte store per group pair.
template <bool PSO, bool P16 = false, bool U8 = false, bool Q8 = false>
__global__ void __launch_bounds__(256, 1)
k_stem_fwd_x3_pipe(const StemX3Args a) {
  static_assert(PSO || !P16, "precision16 stem: PS output only");
  static_assert(PSO || !U8, "uint8 stem: PS output only");
  static_assert(!Q8 || (PSO && U8 && !P16), "Q8 stem: the uint8-frame bf16x3 form only");
  constexpr int NST = Q8 ? 2 : PSO ? (P16 ? 2 : 4) : 16;   // output stores per row (they sit in the memory queue of the counted waits)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = NROW * RL * 2;                   // bf16 elements per tile: hi rows, then lo rows
  __bf16* const base = reinterpret_cast<__bf16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int m = wid & 1, nt = wid >> 1;
  const int cob = blockIdx.y;
  const int co = cob * 64 + m * 32 + l31;
  const int jmax = a.W / 4;
  float* const sbias = reinterpret_cast<float*>(smem + 2 * TILE * 2);      // 64 floats behind the tiles
  {
    f32x4* z = reinterpret_cast<f32x4*>(smem);
    for (int t = tid; t < 2 * TILE * 2 / 16; t += 256) z[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tid < 64) sbias[tid] = cob * 64 + tid < a.F ? a.bias[cob * 64 + tid] : 0.f;
  }
  unsigned* const lut = reinterpret_cast<unsigned*>(smem + 2 * TILE * 2 + 256);   // U8: [256] (hi | lo << 16) of p / 255
  if (U8) {
    const float f = (float)tid / 255.0f;                 // IEEE division, as torch's `x / 255.0`
    unsigned h_, l_;
    sx_split_pair(f, 0.f, h_, l_);
    lut[tid] = (h_ & 0xffffu) | (l_ << 16);
  }
  bf16x8 ah[NROW], al[NROW];
#pragma unroll
  for (int rr = 0; rr < NROW; ++rr) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kx = 8 * half + j - 2;
      const float f = (co < a.F && kx >= 0 && kx < KS) ? a.w[((size_t)co * CIN * KS + rr) * KS + kx] : 0.f;
      const __bf16 h = (__bf16)f;
      ah[rr][j] = h;
      if (!P16) al[rr][j] = (__bf16)(f - (float)h);
    }
  }
  const unsigned long long pa = (unsigned long long)a.x;
  const u32x4s rx = {(unsigned)pa, (unsigned)(pa >> 32), (unsigned)(a.N * CIN * a.H * a.W) * (U8 ? 1u : 4u), 0x00020000u};
  // staging slot s of a thread: input row rr = (s*256 + tid) >> 7, float4 j = (s*256 + tid) & 127 -> rr = 2s + (tid >> 7)
  const int j4 = tid & 127, rsub = tid >> 7;
  const bool lane_ok = j4 < jmax;
  f32x4 p0[U8 ? 1 : NSLOT], p1[U8 ? 1 : NSLOT];
  unsigned q0[U8 ? NSLOT : 1], q1[U8 ? NSLOT : 1];           // U8: one dword (four pixels) per slot
  // load slot SL of output row (RN, ROY) into register SL of set S; ROY < 0: nothing (zeros)
#define SXP_LOAD1(S, SL, RN, ROY)                                                               \
  {                                                                                             \
    const int irow_ = 2 * (SL) + rsub;                                                          \
    const int ci = irow_ / KS, ky = irow_ - ci * KS;                                            \
    const int iy = (ROY) * ST - PD + ky;                                                        \
    const bool ok = lane_ok & ((ROY) >= 0) & (iy >= 0) & (iy < a.H);                           \
    unsigned off = ((unsigned)(((RN) * CIN + ci) * a.H + iy) * a.W + j4 * 4) * (U8 ? 1u : 4u); \
    if constexpr (Q8) {                                                                         \
      /* the same offset as a multiply and a separate add: fused into a 64-bit multiply-add, its addend pair's unused high */ \
      /* register was one that an in-flight load of the other set writes (tools/audit_asm_loads.py reports the read)     */ \
      off = (unsigned)(((RN) * CIN + ci) * a.H + iy) * a.W;                                     \
      asm volatile("" : "+v"(off));                                                             \
      off += j4 * 4;                                                                            \
    }                                                                                           \
    if constexpr (U8) sx_aload1<S == 0>(q##S[SL], ok ? off : 0x80000000u, rx);                  \
    else sx_aload<S == 0>(p##S[SL], ok ? off : 0x80000000u, rx);                                \
  }
#define SXP_WAIT(S, NKEEP)                                                                      \
  {                                                                                             \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NKEEP));                                           \
    if constexpr (U8) { sx_static_for<NSLOT>(SX_LAMBDA(s_) { sx_apass1<S == 0>(q##S[s_]); }); } \
    else { sx_static_for<NSLOT>(SX_LAMBDA(s_) { sx_apass<S == 0>(p##S[s_]); }); }               \
  }
  // lanes past the row's width hold zeros and write them into the row's (zero) right pad
#define SXP_JOB(S, SL, TB)                                                                      \
  {                                                                                             \
    __bf16* d_ = base + (TB) * TILE + (2 * (SL) + rsub) * RL + 4 + 4 * j4;                      \
    unsigned h0, l0, h1, l1;                                                                    \
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));                               \
    if constexpr (U8) {                                                                         \
      const unsigned w_ = q##S[SL];                  /* a lane past the row's width loaded 0: table entry 0 is (0, 0) */ \
      const unsigned t0 = lut[w_ & 255u], t1 = lut[(w_ >> 8) & 255u], t2 = lut[(w_ >> 16) & 255u], t3 = lut[w_ >> 24]; \
      h0 = __builtin_amdgcn_perm(t1, t0, 0x05040100u); h1 = __builtin_amdgcn_perm(t3, t2, 0x05040100u);       \
      *reinterpret_cast<u32x2_t*>(d_) = u32x2_t{h0, h1};                                        \
      if (!P16) {                                                                               \
        l0 = __builtin_amdgcn_perm(t1, t0, 0x07060302u); l1 = __builtin_amdgcn_perm(t3, t2, 0x07060302u);     \
        *reinterpret_cast<u32x2_t*>(d_ + NROW * RL) = u32x2_t{l0, l1};                          \
      }                                                                                         \
    } else if (P16) {                                                                           \
      h0 = sx_hi_pair(p##S[SL][0], p##S[SL][1]); h1 = sx_hi_pair(p##S[SL][2], p##S[SL][3]);     \
      *reinterpret_cast<u32x2_t*>(d_) = u32x2_t{h0, h1};                                        \
    } else {                                                                                    \
      sx_split_pair(p##S[SL][0], p##S[SL][1], h0, l0); sx_split_pair(p##S[SL][2], p##S[SL][3], h1, l1); \
      *reinterpret_cast<u32x2_t*>(d_) = u32x2_t{h0, h1};                                        \
      *reinterpret_cast<u32x2_t*>(d_ + NROW * RL) = u32x2_t{l0, l1};                            \
    }                                                                                           \
  }
  const int bpw = (a.nrows + (int)gridDim.x - 1) / (int)gridDim.x;
  int row = blockIdx.x * bpw;
  const int last = min(row + bpw, a.nrows);
#define SXP_NOY(R_, N_, OY_) const int N_ = (R_) / a.Ho; const int OY_ = (R_) < last ? (R_) - N_ * a.Ho : -1;
  {
    SXP_NOY(row, n_, oy_)
    sx_static_for<NSLOT>(SX_LAMBDA(s) { SXP_LOAD1(0, s, n_, oy_) });
  }
  SXP_WAIT(0, 0)
  __syncthreads();                                       // zero fill done
  sx_static_for<NSLOT>(SX_LAMBDA(s) { SXP_JOB(0, s, 0) });
  {
    SXP_NOY(row + 1, n_, oy_)
    sx_static_for<NSLOT>(SX_LAMBDA(s) { SXP_LOAD1(1, s, n_, oy_) });
  }
  {
    SXP_NOY(row + 2, n_, oy_)
    sx_static_for<NSLOT>(SX_LAMBDA(s) { SXP_LOAD1(0, s, n_, oy_) });
  }
  SXP_WAIT(1, NSLOT)                                     // first band: no stores queued behind set 1 yet, its counted wait would let it pass
  __syncthreads();
  const int ox = nt * 32 + l31;
  // one output row on tile PAR; jobs of the next row from set S = PAR ^ 1 into tile S.  In the memory queue at
  // the wait, oldest first: set S loads, the previous row's 16 stores, set PAR loads  ->  keep 16 + NSLOT.
#define SXP_BAND(PAR, S)                                                                        \
  {                                                                                             \
    const int n = row / a.Ho, oy = row - n * a.Ho;                                              \
    SXP_NOY(row + 3, n3_, oy3_)                                                                 \
    const bf16x8* Bh = reinterpret_cast<const bf16x8*>(base + (PAR) * TILE) + nt * 32 + l31 + half; \
    const bf16x8* Bl = Bh + NROW * RC;                                                          \
    f32x16 acc;                                                                                 \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[r] = 0.f;                                \
    bf16x8 bh[2], bl[2];                                                                        \
    bh[0] = Bh[0]; if (!P16) bl[0] = Bl[0];                                                     \
    SXP_WAIT(S, NST + NSLOT)                                                                    \
    sx_static_for<NROW>(SX_LAMBDA(rr_) {                                                        \
      constexpr int rr = rr_;                                                                   \
      constexpr int cur = rr & 1, nxt = cur ^ 1;                                                \
      if (rr + 1 < NROW) { bh[nxt] = Bh[(rr + 1) * RC]; if (!P16) bl[nxt] = Bl[(rr + 1) * RC]; } \
      if (!P16) {                                                                               \
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], bl[cur], acc, 0, 0, 0);           \
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rr], bh[cur], acc, 0, 0, 0);           \
      }                                                                                         \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rr], bh[cur], acc, 0, 0, 0);             \
      if constexpr (rr < NSLOT) SXP_JOB(S, rr, S)                                               \
      if constexpr (rr >= 4 && rr - 4 < NSLOT) SXP_LOAD1(S, rr - 4, n3_, oy3_)                  \
      __builtin_amdgcn_sched_barrier(0);                                                        \
    });                                                                                         \
    if constexpr (Q8) {                                                                         \
      /* lane = position, registers = channels 32m + 8g + 4half + i: dword A = channels 16gp + 4half + i, dword B = those */ \
      /* + 8; the swap gives half 0 (A, A of half 1) and half 1 (B of half 0, B): channels 8G .. 8G + 7 of the pixel    */ \
      _Pragma("unroll") for (int gp = 0; gp < 2; ++gp) {                                        \
        unsigned da = 0u, db = 0u;                                                              \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                         \
          const float ta = (acc[8 * gp + i] + sbias[m * 32 + 16 * gp + 4 * half + i]) * a.q_inv; \
          const float tb = (acc[8 * gp + 4 + i] + sbias[m * 32 + 16 * gp + 8 + 4 * half + i]) * a.q_inv; \
          da |= (unsigned)(q8::round_q_nan0(ta) & 255) << (8 * i);                              \
          db |= (unsigned)(q8::round_q_nan0(tb) & 255) << (8 * i);                              \
        }                                                                                       \
        auto r1 = __builtin_amdgcn_permlane32_swap(da, db, false, false);                       \
        const int G = 4 * m + 2 * gp + half;                                                    \
        const unsigned off = (ox < a.Wo && row < last) ? (unsigned)((n * a.ps_hp + oy + 1) * a.ps_wp + ox + 1) * 64u + 8u * G : 0x80000000u; \
        typedef unsigned sx_u32x2 __attribute__((ext_vector_type(2)));                          \
        __builtin_amdgcn_raw_buffer_store_b64(sx_u32x2{r1[0], r1[1]}, ry, off, 0, 0);           \
      }                                                                                         \
    } else if constexpr (PSO) {                                                                 \
      /* PS output: lane = position, registers = channels 32m + 8g + 4half + i; a v_permlane32_swap pair leaves a */ \
      /* lane with the 8 channels of one unit (as fdet_conv3x3_ps.hip): two 16-byte stores per group pair          */ \
      _Pragma("unroll") for (int gp = 0; gp < 2; ++gp) {                                        \
        float za[4], zb[4];                                                                     \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                         \
          za[i] = acc[8 * gp + i] + sbias[m * 32 + 16 * gp + 4 * half + i];                     \
          zb[i] = acc[8 * gp + 4 + i] + sbias[m * 32 + 16 * gp + 8 + 4 * half + i];             \
        }                                                                                       \
        unsigned ha[2], la[2], hb[2], lb[2];                                                    \
        if (P16) { ps_hi4(za, ha); ps_hi4(zb, hb); } else { ps_split4(za, ha, la); ps_split4(zb, hb, lb); } \
        _Pragma("unroll") for (int k = 0; k < 2; ++k) {                                         \
          auto r1 = __builtin_amdgcn_permlane32_swap(ha[k], hb[k], false, false);               \
          ha[k] = r1[0]; hb[k] = r1[1];                                                         \
          if (!P16) {                                                                           \
            auto r2 = __builtin_amdgcn_permlane32_swap(la[k], lb[k], false, false);             \
            la[k] = r2[0]; lb[k] = r2[1];                                                       \
          }                                                                                     \
        }                                                                                       \
        const int G = 4 * m + 2 * gp + half;                                                    \
        const unsigned off = (ox < a.Wo && row < last) ? (unsigned)(n * a.ps_img + (G * a.ps_hp + oy) * a.ps_wp + ox + 1) * 16u : 0x80000000u; \
        typedef unsigned sx_u32x4 __attribute__((ext_vector_type(4)));                          \
        __builtin_amdgcn_raw_buffer_store_b128(sx_u32x4{ha[0], ha[1], hb[0], hb[1]}, ry, off, 0, 0); \
        if (!P16) __builtin_amdgcn_raw_buffer_store_b128(sx_u32x4{la[0], la[1], lb[0], lb[1]}, ry, off, a.ps_plane * 16, 0); \
      }                                                                                         \
    } else {                                                                                    \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                            \
      const int c2 = cob * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;                     \
      const bool ok = ox < a.Wo && c2 < a.F && row < last;                                      \
      const unsigned off = ok ? ((unsigned)((n * a.F + c2) * a.Ho + oy) * a.Wo + ox) * 4u : 0x80000000u; \
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[r] + sbias[m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half]), ry, off, 0, 0); \
    }                                                                                           \
    }                                                                                           \
    __syncthreads();                                                                            \
    row += 1;                                                                                   \
  }
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, PSO ? a.N * a.ps_img * 16 : a.N * a.F * a.Ho * a.Wo * 4, 0x00020000);
  // rows are walked in PAIRS with no exit between the two band bodies (an odd count ends on a dummy row: zeros in,
  // nothing stored): with a mid-loop exit hipcc merged the two bodies' tails behind a run-time flag, and the asm-load
  // audit (tools/audit_asm_loads.py), which cannot follow that flag, reported paths no wave takes
  const int last2 = row + ((last - row + 1) & ~1);
  while (row < last2) {
    SXP_BAND(0, 1)
    SXP_BAND(1, 0)
  }
  SXP_WAIT(0, 0)
  SXP_WAIT(1, 0)
#undef SXP_BAND
#undef SXP_NOY
#undef SXP_JOB
#undef SXP_WAIT
#undef SXP_LOAD1
}

// ---------------------------------------------------------------------------------------
// weight gradient, bf16x3:  dW[co][ci,ky,kx] = sum_ox dy[co][ox] * x[ci][8oy+ky-2][8ox+kx-2]
// MFMA K = 16 output columns.  B needs 8 consecutive ox for one tap = a stride-8 walk over the
// input row, so the row is staged DE-INTERLEAVED by column phase: plane (row, ix % 8), element
// ix / 8 (+8 zero front pad).  Taps kx = 2..9 read phase kx-2 at element ox (aligned chunk);
// taps kx = 0,1 read phase 6,7 at element ox-1 (one-element funnel shift of two chunks).
// N tiles: 0..7 hold the 240 aligned taps (row*8 + kx-2), 8..9 the 60 shifted ones (row*2 + kx).
// ---------------------------------------------------------------------------------------
constexpr int PC = 11;                     // chunks per plane (88 elements: 8 pad + 61 + slack), odd
constexpr int PE = PC * 8;
constexpr int NPLANE = NROW * 8;           // 240
constexpr int DL = 72;                     // dy row length (elements), DL/8 odd
constexpr int WSLOT = 4;                   // staging slots: 30 rows x 30 groups of 16 pixels / 256 threads
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct StemWgX3Args {
  const float* x; const float* dy; float* ws; float* wsb;
  int N, F, H, W, Ho, Wo, nrows;
};

__device__ __forceinline__ bf16x8 shift7(const bf16x8& c0, const bf16x8& c1) {      // elements 7..14 of (c0|c1)
  const u32x4 a = __builtin_bit_cast(u32x4, c0), b = __builtin_bit_cast(u32x4, c1);
  u32x4 o;
  o[0] = __builtin_amdgcn_alignbyte(b[0], a[3], 2);
  o[1] = __builtin_amdgcn_alignbyte(b[1], b[0], 2);
  o[2] = __builtin_amdgcn_alignbyte(b[2], b[1], 2);
  o[3] = __builtin_amdgcn_alignbyte(b[3], b[2], 2);
  return __builtin_bit_cast(bf16x8, o);
}

__global__ void __launch_bounds__(256, 1)
k_stem_wgrad_x3(const StemWgX3Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* Ph = reinterpret_cast<__bf16*>(smem);         // [240 planes][PE]
  __bf16* Pl = Ph + NPLANE * PE;
  __bf16* Dh = Pl + NPLANE * PE;                        // [64 co][DL]
  __bf16* Dl = Dh + 64 * DL;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int m = wid & 1, ng = wid >> 1;                 // co tile, N-tile group (tiles 5*ng .. 5*ng+4)
  const int cob = blockIdx.y;
  const int gmax = a.W / 16, dmax = a.Wo / 4;

  {
    f32x4* z = reinterpret_cast<f32x4*>(smem);
    for (int t = tid; t < (NPLANE * PE + 64 * DL) * 4 / 16; t += 256) z[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // per-lane chunk base of each of this wave's 5 N tiles
  int pbase[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int tile = ng * 5 + t;
    int plane, extra;
    if (tile < 8) {                                     // aligned taps: kk = row*8 + (kx-2)
      const int kk = min(tile * 32 + l31, NROW * 8 - 1);
      plane = kk; extra = 1;                            // +1 chunk: the 8-element front pad
    } else {                                            // shifted taps: kk2 = row*2 + kx, phase 6 + kx
      const int kk2 = min((tile - 8) * 32 + l31, NROW * 2 - 1);
      plane = (kk2 >> 1) * 8 + 6 + (kk2 & 1); extra = 0;
    }
    pbase[t] = plane * PC + extra + half;
  }
  const bf16x8* Bh = reinterpret_cast<const bf16x8*>(Ph);
  const bf16x8* Bl = reinterpret_cast<const bf16x8*>(Pl);
  const bf16x8* Ah = reinterpret_cast<const bf16x8*>(Dh + (m * 32 + l31) * DL) + half;
  const bf16x8* Al = reinterpret_cast<const bf16x8*>(Dl + (m * 32 + l31) * DL) + half;

  f32x16 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bpart[4] = {0.f, 0.f, 0.f, 0.f};

  f32x4 px[WSLOT][4], pd[4];
#define SWX3_LOAD(ROW_N, ROW_OY)                                                                \
  {                                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < WSLOT; ++s_) {                                      \
      const int it = s_ * 256 + tid;                                                            \
      const int rr = it >> 5, g_ = it & 31;                                                     \
      const int rc = min(rr, NROW - 1);                                                         \
      const int ci = rc / KS, ky = rc - ci * KS;                                                \
      const int iy = (ROW_OY) * ST - PD + ky;                                                   \
      const bool ok = rr < NROW && g_ < gmax && iy >= 0 && iy < a.H;                            \
      const float* src = a.x + (((size_t)(ROW_N) * CIN + ci) * a.H + max(iy, 0)) * a.W + g_ * 16; \
      _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_)                                          \
        px[s_][q_] = ok ? *reinterpret_cast<const f32x4*>(src + q_ * 4) : f32x4{0.f, 0.f, 0.f, 0.f}; \
    }                                                                                           \
    _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                                          \
      const int it = s_ * 256 + tid;                                                            \
      const int c = it >> 4, j = it & 15;                                                       \
      const int cg = cob * 64 + c;                                                              \
      pd[s_] = (j < dmax && cg < a.F)                                                           \
                   ? *reinterpret_cast<const f32x4*>(a.dy + (((size_t)(ROW_N) * a.F + cg) * a.Ho + (ROW_OY)) * a.Wo + j * 4) \
                   : f32x4{0.f, 0.f, 0.f, 0.f};                                                 \
    }                                                                                           \
  }
  // pixel ix = 16g + i  ->  plane row*8 + (i & 7), element 8 + 2g + (i >> 3): (i, i+8) pack into one dword
#define SWX3_STORE()                                                                            \
  {                                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < WSLOT; ++s_) {                                      \
      const int it = s_ * 256 + tid;                                                            \
      const int rr = it >> 5, g_ = it & 31;                                                     \
      if (rr < NROW && g_ < gmax) {                                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) {                                      \
          const float f0 = px[s_][i_ >> 2][i_ & 3], f1 = px[s_][2 + (i_ >> 2)][i_ & 3];        \
          const __bf16 h0 = (__bf16)f0, h1 = (__bf16)f1;                                        \
          const int e_ = (rr * 8 + i_) * PE + 8 + 2 * g_;                                       \
          *reinterpret_cast<bf16x2*>(Ph + e_) = bf16x2{h0, h1};                                 \
          *reinterpret_cast<bf16x2*>(Pl + e_) = bf16x2{(__bf16)(f0 - (float)h0), (__bf16)(f1 - (float)h1)}; \
        }                                                                                       \
      }                                                                                         \
    }                                                                                           \
    _Pragma("unroll") for (int s_ = 0; s_ < 4; ++s_) {                                          \
      const int it = s_ * 256 + tid;                                                            \
      const int c = it >> 4, j = it & 15;                                                       \
      if (j < dmax) {                                                                           \
        bf16x4 h4, l4;                                                                          \
        _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_) {                                      \
          const __bf16 h = (__bf16)pd[s_][c_];                                                  \
          h4[c_] = h; l4[c_] = (__bf16)(pd[s_][c_] - (float)h);                                 \
          bpart[s_] += pd[s_][c_];                                                              \
        }                                                                                       \
        *reinterpret_cast<bf16x4*>(Dh + c * DL + 4 * j) = h4;                                   \
        *reinterpret_cast<bf16x4*>(Dl + c * DL + 4 * j) = l4;                                   \
      }                                                                                         \
    }                                                                                           \
  }

  int row = blockIdx.x;
  if (row < a.nrows) { const int n = row / a.Ho, oy = row - n * a.Ho; SWX3_LOAD(n, oy) }
  const int nks = (a.Wo + 15) / 16;
  for (; row < a.nrows; row += gridDim.x) {
    __syncthreads();
    SWX3_STORE()
    __syncthreads();
    const int nrow = row + gridDim.x;
    if (nrow < a.nrows) { const int n2 = nrow / a.Ho, oy2 = nrow - n2 * a.Ho; SWX3_LOAD(n2, oy2) }
#pragma unroll 1
    for (int ks = 0; ks < nks; ++ks) {
      const bf16x8 ah = Ah[2 * ks], al = Al[2 * ks];
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        bf16x8 bh, bl;
        if (ng * 5 + t < 8) {
          bh = Bh[pbase[t] + 2 * ks]; bl = Bl[pbase[t] + 2 * ks];
        } else {
          bh = shift7(Bh[pbase[t] + 2 * ks], Bh[pbase[t] + 2 * ks + 1]);
          bl = shift7(Bl[pbase[t] + 2 * ks], Bl[pbase[t] + 2 * ks + 1]);
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
      }
    }
  }
  // slab ws[blk][co][320]: column k' = tile*32 + lane (decoded by the reduce kernel)
  const int FP = gridDim.y * 64;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int kp = (ng * 5 + t) * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c2 = cob * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      a.ws[((size_t)blockIdx.x * FP + c2) * 320 + kp] = acc[t][r];
    }
  }
#pragma unroll
  for (int s_ = 0; s_ < 4; ++s_) {
    float v = bpart[s_];
    v += __shfl_xor(v, 8, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 1, 16);
    const int c = (s_ * 256 + tid) >> 4;
    if ((tid & 15) == 0) a.wsb[(size_t)blockIdx.x * FP + cob * 64 + c] = v;
  }
}

// ---------------------------------------------------------------------------------------
// Pipelined weight gradient (same planes and slab layout): planes of 9 chunks (8 pad + 60 + slack) so that TWO
// plane tiles fit LDS beside ONE dy tile; contiguous output rows per workgroup.  While the 60 MFMAs of row b
// run on plane tile b & 1, the 32 pixel-pair split jobs of row b+1 ride two per (k-step, N tile) slot into the
// other tile, the asm buffer loads of row b+2 follow four slots behind the jobs that freed their registers (ONE x
// register set, counted waits per group of four slots), and the small dy tile of row b+1 -- loaded at the start of
// row b -- is staged between the rows.  Every wave takes four aligned-tap N tiles and one
// funnel-shifted one (tiles {0..3, 8} / {4..7, 9}), so there is a single code path.
// ---------------------------------------------------------------------------------------
constexpr int PCP = 9, PEP = PCP * 8;      // plane pitch of the pipelined kernel
constexpr int TILEP = NPLANE * PEP * 2;    // bf16 elements per plane tile (hi planes, then lo planes)

// P16 (precision16): one MFMA pass on bf16(dy) x bf16(x); the lo planes are neither computed nor staged.
template <bool P16>
__global__ void __launch_bounds__(256, 1)
k_stem_wgrad_x3_pipe(const StemWgX3Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* const base = reinterpret_cast<__bf16*>(smem);       // two plane tiles
  __bf16* Dh = base + 2 * TILEP;                              // [64 co][DL]
  __bf16* Dl = Dh + 64 * DL;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int m = wid & 1, ng = wid >> 1;
  const int cob = blockIdx.y;
  const int gmax = a.W / 16, dmax = a.Wo / 4;
  {
    f32x4* z = reinterpret_cast<f32x4*>(smem);
    for (int t = tid; t < (2 * TILEP + 2 * 64 * DL + 8 * PEP) * 2 / 16; t += 256) z[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // N tile t of this wave: t < 4 -> aligned taps tile ng*4 + t (kk = row*8 + kx-2); t == 4 -> shifted taps tile 8 + ng
  int pbase[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    int plane, extra;
    if (t < 4) { const int kk = min((ng * 4 + t) * 32 + l31, NROW * 8 - 1); plane = kk; extra = 1; }
    else { const int kk2 = min(ng * 32 + l31, NROW * 2 - 1); plane = (kk2 >> 1) * 8 + 6 + (kk2 & 1); extra = 0; }
    pbase[t] = plane * PCP + extra + half;
  }
  const bf16x8* Ah = reinterpret_cast<const bf16x8*>(Dh + (m * 32 + l31) * DL) + half;
  const bf16x8* Al = reinterpret_cast<const bf16x8*>(Dl + (m * 32 + l31) * DL) + half;
  f32x16 acc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bpart[4] = {0.f, 0.f, 0.f, 0.f};
  // staging geometry of this thread (threads without a pixel group write their zeros into 8 junk planes)
  int xw_off[WSLOT]; unsigned x_goff[WSLOT]; bool x_ok[WSLOT];
#pragma unroll
  for (int s_ = 0; s_ < WSLOT; ++s_) {
    const int it = s_ * 256 + tid;
    const int rr = it >> 5, g_ = it & 31;
    x_ok[s_] = rr < NROW && g_ < gmax;
    xw_off[s_] = x_ok[s_] ? (rr * 8) * PEP + 8 + 2 * g_ : -1;
    x_goff[s_] = (unsigned)(g_ * 16) * 4u;
  }
  __bf16* const junk = Dl + 64 * DL + 2 * (tid & 31);
  unsigned d_goff[4]; bool d_ok[4]; int dw_off[4];
#pragma unroll
  for (int s_ = 0; s_ < 4; ++s_) {
    const int it = s_ * 256 + tid;
    const int c = it >> 4, j = it & 15;
    const int cg = cob * 64 + c;
    d_ok[s_] = j < dmax && cg < a.F;
    d_goff[s_] = ((unsigned)cg * a.Ho * a.Wo + j * 4) * 4u;
    dw_off[s_] = c * DL + 4 * j;
  }
  const unsigned long long pa_x = (unsigned long long)a.x, pa_d = (unsigned long long)a.dy;
  const u32x4s rsx = {(unsigned)pa_x, (unsigned)(pa_x >> 32), (unsigned)(a.N * CIN * a.H * a.W) * 4u, 0x00020000u};
  const u32x4s rsd = {(unsigned)pa_d, (unsigned)(pa_d >> 32), (unsigned)(a.N * a.F * a.Ho * a.Wo) * 4u, 0x00020000u};
  f32x4 px0[WSLOT][4], pd[4];       // ONE x register set (a slot is re-loaded right behind the jobs that read it) and the dy set
  const int bpw = (a.nrows + (int)gridDim.x - 1) / (int)gridDim.x;
  int row = blockIdx.x * bpw;
  const int last = min(row + bpw, a.nrows);
#define SWP_NOY(R_, N_, OY_) const int N_ = (R_) / a.Ho; const int OY_ = (R_) < last ? (R_) - N_ * a.Ho : -1;
#define SWP_LOAD_X1(S, SL, Q, N_, OY_)                                                            \
  {                                                                                               \
    const int rr_ = ((SL) * 256 + tid) >> 5;                                                      \
    const int rc_ = min(rr_, NROW - 1);                                                           \
    const int ci_ = rc_ / KS, ky_ = rc_ - ci_ * KS;                                               \
    const int iy_ = (OY_) * ST - PD + ky_;                                                        \
    const bool ok_ = x_ok[SL] & ((OY_) >= 0) & (iy_ >= 0) & (iy_ < a.H);                          \
    const unsigned off_ = ((unsigned)(((N_) * CIN + ci_) * a.H + iy_) * a.W) * 4u + x_goff[SL] + (Q) * 16; \
    sx_aload<false>(px##S[SL][Q], ok_ ? off_ : 0x80000000u, rsx);                                \
  }
#define SWP_LOAD_D1(SL, N_, OY_)                                                                  \
  {                                                                                               \
    const unsigned off_ = ((unsigned)(((N_) * a.F) * a.Ho + (OY_)) * a.Wo) * 4u + d_goff[SL];     \
    sx_aload<false>(pd[SL], (d_ok[SL] & ((OY_) >= 0)) ? off_ : 0x80000000u, rsd);                 \
  }
#define SWP_PASS_X(S) sx_static_for<WSLOT * 4>(SX_LAMBDA(l_) { sx_apass<false>(px##S[l_ / 4][l_ % 4]); });
#define SWP_PASS_XS(SL) sx_static_for<4>(SX_LAMBDA(q_) { sx_apass<false>(px0[SL][q_]); });
#define SWP_PASS_D() sx_static_for<4>(SX_LAMBDA(s_) { sx_apass<false>(pd[s_]); });
  // pixel-pair job (SL, I): pixels i and i+8 of the thread's 16-pixel group -> plane row*8 + i of tile TB
#define SWP_JOB(S, SL, I, TB)                                                                     \
  {                                                                                               \
    unsigned hi_, lo_;                                                                            \
    __bf16* d_ = (xw_off[SL] >= 0 ? base + (TB) * TILEP + xw_off[SL] : junk) + (I) * PEP;         \
    if (P16) {                                                                                    \
      hi_ = sx_hi_pair(px##S[SL][(I) >> 2][(I) & 3], px##S[SL][2 + ((I) >> 2)][(I) & 3]);         \
      *reinterpret_cast<unsigned*>(d_) = hi_;                                                     \
    } else {                                                                                      \
      sx_split_pair(px##S[SL][(I) >> 2][(I) & 3], px##S[SL][2 + ((I) >> 2)][(I) & 3], hi_, lo_);  \
      *reinterpret_cast<unsigned*>(d_) = hi_;                                                     \
      *reinterpret_cast<unsigned*>(d_ + (xw_off[SL] >= 0 ? NPLANE * PEP : 0)) = lo_;              \
    }                                                                                             \
  }
  // dy tile (lanes past the row hold zeros and write them into the row's zero pad)
#define SWP_STAGE_D()                                                                             \
  sx_static_for<4>(SX_LAMBDA(s_) {                                                                \
    unsigned h0, l0, h1, l1;                                                                      \
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));                                 \
    if (P16) {                                                                                    \
      h0 = sx_hi_pair(pd[s_][0], pd[s_][1]); h1 = sx_hi_pair(pd[s_][2], pd[s_][3]);               \
      *reinterpret_cast<u32x2_t*>(Dh + dw_off[s_]) = u32x2_t{h0, h1};                             \
    } else {                                                                                      \
      sx_split_pair(pd[s_][0], pd[s_][1], h0, l0); sx_split_pair(pd[s_][2], pd[s_][3], h1, l1);   \
      *reinterpret_cast<u32x2_t*>(Dh + dw_off[s_]) = u32x2_t{h0, h1};                             \
      *reinterpret_cast<u32x2_t*>(Dl + dw_off[s_]) = u32x2_t{l0, l1};                             \
    }                                                                                             \
    bpart[s_] += (pd[s_][0] + pd[s_][1]) + (pd[s_][2] + pd[s_][3]);                               \
  });
  {
    SWP_NOY(row, n_, oy_)
    sx_static_for<4>(SX_LAMBDA(s_) { SWP_LOAD_D1(s_, n_, oy_) });
    sx_static_for<WSLOT * 4>(SX_LAMBDA(l_) { SWP_LOAD_X1(0, l_ / 4, l_ % 4, n_, oy_) });
  }
  asm volatile("s_waitcnt vmcnt(0)");
  SWP_PASS_X(0)
  SWP_PASS_D()
  __syncthreads();                                       // zero fill done
  sx_static_for<WSLOT * 8>(SX_LAMBDA(j_) { SWP_JOB(0, j_ / 8, j_ % 8, 0) });
  SWP_STAGE_D()
  {
    SWP_NOY(row + 1, n_, oy_)
    sx_static_for<WSLOT * 4>(SX_LAMBDA(l_) { SWP_LOAD_X1(0, l_ / 4, l_ % 4, n_, oy_) });
  }
  __syncthreads();
  // one row on plane tile PAR.  Slot u = 5 ks + t.  In the memory queue at the top of a row, oldest first:
  // [x of the next row: 16, issued under the previous row][dy of the next row: 4, issued first thing in this row];
  // the jobs of slot group s (slots 4s..4s+3) read x loads 4s..4s+3, behind which sit 12 - 4s older-row loads,
  // the 4 dy loads and the max(0, 4s - 4) re-loads already issued in this row.
#define SWP_ROW(PAR)                                                                              \
  {                                                                                               \
    SWP_NOY(row + 2, n2_, oy2_)                                                                   \
    SWP_NOY(row + 1, n1_, oy1_)                                                                   \
    const bf16x8* Bh = reinterpret_cast<const bf16x8*>(base + (PAR) * TILEP);                     \
    const bf16x8* Bl = reinterpret_cast<const bf16x8*>(base + (PAR) * TILEP + NPLANE * PEP);      \
    bf16x8 fa[2][2], fb[2][4];                                                                    \
    fa[0][0] = Ah[0]; if (!P16) fa[0][1] = Al[0];                                                 \
    fb[0][0] = Bh[pbase[0]]; if (!P16) fb[0][1] = Bl[pbase[0]];                                   \
    sx_static_for<4>(SX_LAMBDA(s_) { SWP_LOAD_D1(s_, n1_, oy1_) });                               \
    sx_static_for<20>(SX_LAMBDA(u_) {                                                             \
      constexpr int u = u_;                                                                       \
      constexpr int ks = u / 5, t = u % 5;                                                        \
      constexpr int F = u & 1, FA = ks & 1;                                                       \
      if constexpr (u < 16 && u % 4 == 0) {                                                       \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(u == 0 ? 16 : 12));                              \
        SWP_PASS_XS(u / 4)                                                                        \
      }                                                                                           \
      bf16x8 bh, bl;                                                                              \
      if constexpr (t == 4) { bh = shift7(fb[F][0], fb[F][2]); if (!P16) bl = shift7(fb[F][1], fb[F][3]); } \
      else { bh = fb[F][0]; if (!P16) bl = fb[F][1]; }                                            \
      if (!P16) {                                                                                 \
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[FA][0], bl, acc[t], 0, 0, 0);         \
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[FA][1], bh, acc[t], 0, 0, 0);         \
      }                                                                                           \
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[FA][0], bh, acc[t], 0, 0, 0);           \
      if constexpr (u + 1 < 20) {                                                                 \
        constexpr int ks1 = (u + 1) / 5, t1 = (u + 1) % 5;                                        \
        if constexpr (t1 == 0) { fa[ks1 & 1][0] = Ah[2 * ks1]; if (!P16) fa[ks1 & 1][1] = Al[2 * ks1]; } \
        fb[F ^ 1][0] = Bh[pbase[t1] + 2 * ks1]; if (!P16) fb[F ^ 1][1] = Bl[pbase[t1] + 2 * ks1]; \
        if constexpr (t1 == 4) { fb[F ^ 1][2] = Bh[pbase[t1] + 2 * ks1 + 1]; if (!P16) fb[F ^ 1][3] = Bl[pbase[t1] + 2 * ks1 + 1]; } \
      }                                                                                           \
      if constexpr (u < 16) { SWP_JOB(0, u / 4, (u % 4) * 2, (PAR) ^ 1) SWP_JOB(0, u / 4, (u % 4) * 2 + 1, (PAR) ^ 1) } \
      if constexpr (u >= 4) SWP_LOAD_X1(0, (u - 4) / 4, (u - 4) % 4, n2_, oy2_)                   \
      __builtin_amdgcn_sched_barrier(0);                                                          \
    });                                                                                           \
    __syncthreads();                                                                              \
    asm volatile("s_waitcnt vmcnt(16)");                                                          \
    SWP_PASS_D()                                                                                  \
    SWP_STAGE_D()                                                                                 \
    __syncthreads();                                                                              \
    row += 1;                                                                                     \
  }
  // ONE loop body, the plane-tile parity is a run-time scalar: with two unrolled bodies (parity 0 / 1) hipcc gave them
  // different register assignments and bridged the back edge with copies of the x register set -- copies of registers
  // whose asm loads may still be in flight (tools/audit_asm_loads.py, count-aware since round 2, flagged 56 of them;
  // the round-1 audit's 150-line window had hidden them).  A copy taken before the data lands keeps the stale value.
  for (int par = 0; row < last; par ^= 1) SWP_ROW(par)
  asm volatile("s_waitcnt vmcnt(0)");
  SWP_PASS_X(0) SWP_PASS_D()
#undef SWP_ROW
#undef SWP_STAGE_D
#undef SWP_JOB
#undef SWP_PASS_D
#undef SWP_PASS_X
#undef SWP_PASS_XS
#undef SWP_LOAD_D1
#undef SWP_LOAD_X1
#undef SWP_NOY
  const int FP = gridDim.y * 64;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int kp = (t < 4 ? ng * 4 + t : 8 + ng) * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c2 = cob * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      a.ws[((size_t)blockIdx.x * FP + c2) * 320 + kp] = acc[t][r];
    }
  }
#pragma unroll
  for (int s_ = 0; s_ < 4; ++s_) {
    float v = bpart[s_];
    v += __shfl_xor(v, 8, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 1, 16);
    const int c = (s_ * 256 + tid) >> 4;
    if ((tid & 15) == 0) a.wsb[(size_t)blockIdx.x * FP + cob * 64 + c] = v;
  }
}

// dW[f][ci,ky,kx] = sum_b ws[b][f][k'] with k' -> tap decode; db[f] = sum_b wsb[b][f]  (fixed order)
__global__ void __launch_bounds__(1024)
k_stem_x3_reduce(const float* __restrict__ ws, const float* __restrict__ wsb, int nblk, int F, int FP,
                 float* __restrict__ dW, float* __restrict__ db) {
  // 64 slab columns x 16 slab phases per workgroup (slabs are 82 KB apart: more phases = fewer dependent round trips)
  __shared__ float part[1024];
  const int f = blockIdx.y;
  const int kq = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int kp = blockIdx.x * 64 + kq;
  float s = 0.f;
  if (kp < 320)
    for (int b = ph; b < nblk; b += 16) s += ws[((size_t)b * FP + f) * 320 + kp];
  part[threadIdx.x] = s;
  __syncthreads();
  if (ph == 0 && kp < 320) {
    int rr = -1, kx = 0;
    if (kp < 256) { if (kp < NROW * 8) { rr = kp >> 3; kx = (kp & 7) + 2; } }
    else { const int k2 = kp - 256; if (k2 < NROW * 2) { rr = k2 >> 1; kx = k2 & 1; } }
    if (rr >= 0) {
      float tot = 0.f;
#pragma unroll
      for (int p = 0; p < 16; ++p) tot += part[p * 64 + kq];
      dW[((size_t)f * NROW + rr) * KS + kx] = tot;
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    float t = 0.f;
    for (int b = threadIdx.x; b < nblk; b += 1024) t += wsb[(size_t)b * FP + f];
    part[threadIdx.x] = t;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
      if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) db[f] = part[0];
  }
}

}  // namespace

namespace fdet {

int stem_x3_fwd(const float* x, const float* w, const float* bias, float* y, int N, int F, int H, int W,
                hipStream_t st) {
  StemX3Args a{};
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.N = N; a.F = F; a.H = H; a.W = W;
  a.Ho = (H + 4 - 10) / 8 + 1; a.Wo = (W + 4 - 10) / 8 + 1; a.nrows = N * a.Ho;
  const int FP = (F + 63) / 64 * 64;
  const int nblk = a.nrows < 256 ? a.nrows : 256;
  const size_t lds = (size_t)NROW * RL * 2 * 2;
  const char* e = FDET_ENV_ONCE("FDET_STEM_PIPE");
  // pipelined kernel: 32-bit byte offsets into x and y (FDET_STEM_PIPE=0 keeps the single-tile kernel)
  if (!(e && e[0] == '0') && (size_t)N * CIN * H * W < ((size_t)1 << 29) && (size_t)N * F * a.Ho * a.Wo < ((size_t)1 << 29)) {
    if (hipFuncSetAttribute((const void*)k_stem_fwd_x3_pipe<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * lds + 256)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FDET_ELAUNCH, "stem_fwd(bf16x3): cannot reserve %zu bytes of LDS", 2 * lds + 256);
    }
    stem_note_route(STEM_X3_PIPE, STEM_PASS_FWD, false, false, false, nblk, a.nrows);
    hipLaunchKernelGGL(k_stem_fwd_x3_pipe<false>, dim3(nblk, FP / 64), dim3(256), 2 * lds + 256, st, a);
    return check_launch("fdet_stem_fwd(bf16x3 pipelined)");
  }
  { if (int rc_ = set_lds_attr((const void*)k_stem_fwd_x3, (size_t)(lds), __func__)) return rc_; }
  stem_note_route(STEM_X3_SINGLE, STEM_PASS_FWD, false, false, false, nblk, a.nrows);
  hipLaunchKernelGGL(k_stem_fwd_x3, dim3(nblk, FP / 64), dim3(256), lds, st, a);
  return check_launch("fdet_stem_fwd(bf16x3)");
}

// Images per launch of the pipelined kernels: their buffer descriptors take 32-bit byte offsets (x, dy < 2^29 floats;
// the PS output < 2^31 bytes), so a larger batch runs as consecutive launches over image chunks.  0: not one image fits.
int stem_x3_chunk(int F, int H, int W, int ps_img) {
  const int Ho = (H + 4 - 10) / 8 + 1, Wo = (W + 4 - 10) / 8 + 1;
  const size_t lim = ((size_t)1 << 29) - 1;
  size_t c = lim / ((size_t)CIN * H * W);
  c = std::min(c, lim / ((size_t)F * Ho * Wo));
  if (ps_img > 0) c = std::min(c, (((size_t)1 << 31) - 1) / ((size_t)ps_img * 16));
  return (int)std::min<size_t>(c, (size_t)1 << 30);
}

bool stem_x3_fwd_ps_ok(int N, int F, int H, int W) {
  PsGeo g;
  const int Ho = (H + 4 - 10) / 8 + 1, Wo = (W + 4 - 10) / 8 + 1;
  return F == 64 && N > 0 && H >= 10 && ps_geo(N, F, Ho, Wo, g) && stem_x3_chunk(F, H, W, g.img) >= 1;
}

// the same forward with a pre-split (PS) output: y_ps = image-0 pointer of a PS tensor (N, 64, Ho, Wo); chunks of
// stem_x3_chunk images, each launch on its slice of x and of the PS images (rows never cross images: same arithmetic)
int stem_x3_fwd_ps(const void* xin, const float* w, const float* bias, void* y_ps, int N, int F, int H, int W, hipStream_t st, bool p16,
                   bool u8) {
  const int Ho = (H + 4 - 10) / 8 + 1, Wo = (W + 4 - 10) / 8 + 1;
  PsGeo g;
  if (!stem_x3_fwd_ps_ok(N, F, H, W) || !ps_geo(N, F, Ho, Wo, g))
    return fail(FDET_EINVAL, "stem_fwd_ps: unsupported shape (F=%d, output %dx%d, N=%d)", F, Ho, Wo, N);
  const int chunk = stem_x3_chunk(F, H, W, g.img);
  const size_t lds = (size_t)NROW * RL * 2 * 2;
  const size_t ldsb = 2 * lds + 256 + 1024;                // tiles, bias, the uint8 table
  const void* kern = u8 ? (p16 ? (const void*)k_stem_fwd_x3_pipe<true, true, true> : (const void*)k_stem_fwd_x3_pipe<true, false, true>)
                        : (p16 ? (const void*)k_stem_fwd_x3_pipe<true, true> : (const void*)k_stem_fwd_x3_pipe<true, false>);
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb) != hipSuccess) {
    (void)hipGetLastError();
    return fail(FDET_ELAUNCH, "stem_fwd_ps: cannot reserve %zu bytes of LDS", ldsb);
  }
  const size_t in_img = (size_t)CIN * H * W * (u8 ? 1 : 4);          // bytes per input image
  for (int n0 = 0; n0 < N; n0 += chunk) {
    StemX3Args a{};
    a.x = reinterpret_cast<const float*>(reinterpret_cast<const char*>(xin) + (size_t)n0 * in_img);   // u8: uint8 frames [N][3][H][W], 4-byte aligned rows (W % 4 == 0)
    a.w = w; a.bias = bias; a.y = reinterpret_cast<float*>(reinterpret_cast<char*>(y_ps) + (size_t)n0 * g.img * 16);
    a.N = std::min(chunk, N - n0); a.F = F; a.H = H; a.W = W;
    a.Ho = Ho; a.Wo = Wo; a.nrows = a.N * Ho;
    a.ps_hp = g.HP; a.ps_wp = g.WP; a.ps_plane = g.plane; a.ps_img = g.img;
    const int nblk = a.nrows < 256 ? a.nrows : 256;
    stem_note_route(STEM_X3_PIPE, STEM_PASS_FWD, p16, u8, true, nblk, a.nrows);
    if (u8 && p16) hipLaunchKernelGGL((k_stem_fwd_x3_pipe<true, true, true>), dim3(nblk, 1), dim3(256), ldsb, st, a);
    else if (u8) hipLaunchKernelGGL((k_stem_fwd_x3_pipe<true, false, true>), dim3(nblk, 1), dim3(256), ldsb, st, a);
    else if (p16) hipLaunchKernelGGL((k_stem_fwd_x3_pipe<true, true>), dim3(nblk, 1), dim3(256), ldsb, st, a);
    else hipLaunchKernelGGL((k_stem_fwd_x3_pipe<true, false>), dim3(nblk, 1), dim3(256), ldsb, st, a);
    if (int rc = check_launch("fdet_stem_fwd_ps")) return rc;
  }
  return 0;
}

// Int8 inference: the uint8-frame stem with the quantised output (k_stem_fwd_x3_pipe<.., Q8>).  q: int8 [N][Ho+2][Wo+2][64];
// chunks as stem_x3_fwd_ps (the tensor is under 2^31 bytes, so its 32-bit offsets hold whatever the chunk)
bool stem_x3_fwd_q8_ok(int N, int F, int H, int W) {
  if (!stem_x3_fwd_ps_ok(N, F, H, W)) return false;
  const int Ho = (H + 4 - 10) / 8 + 1, Wo = (W + 4 - 10) / 8 + 1;
  return (unsigned long long)N * (Ho + 2) * (Wo + 2) * 64 < (1ull << 31);
}

int stem_x3_fwd_q8(const unsigned char* frames, const float* w, const float* bias, float q_inv, signed char* q, int N, int F, int H,
                   int W, hipStream_t st) {
  if (!stem_x3_fwd_q8_ok(N, F, H, W)) return fail(FDET_EINVAL, "stem_fwd_q8: unsupported shape (F=%d, %dx%d, N=%d)", F, H, W, N);
  const int Ho = (H + 4 - 10) / 8 + 1, Wo = (W + 4 - 10) / 8 + 1;
  const int img = (Ho + 2) * (Wo + 2) * 4;                 // 16-byte units per output image
  const int chunk = stem_x3_chunk(F, H, W, img);
  const size_t ldsb = (size_t)NROW * RL * 2 * 2 * 2 + 256 + 1024;      // tiles, bias, the uint8 table
  { if (int rc_ = set_lds_attr((const void*)k_stem_fwd_x3_pipe<true, false, true, true>, ldsb, __func__)) return rc_; }
  for (int n0 = 0; n0 < N; n0 += chunk) {
    StemX3Args a{};
    a.x = reinterpret_cast<const float*>(frames + (size_t)n0 * CIN * H * W);
    a.w = w; a.bias = bias; a.y = reinterpret_cast<float*>(q + (size_t)n0 * img * 16);
    a.N = std::min(chunk, N - n0); a.F = F; a.H = H; a.W = W;
    a.Ho = Ho; a.Wo = Wo; a.nrows = a.N * Ho;
    a.ps_hp = Ho + 2; a.ps_wp = Wo + 2; a.ps_img = img; a.q_inv = q_inv;
    const int nblk = a.nrows < 256 ? a.nrows : 256;
    stem_note_route(STEM_X3_PIPE, STEM_PASS_FWD, false, true, false, nblk, a.nrows);
    hipLaunchKernelGGL((k_stem_fwd_x3_pipe<true, false, true, true>), dim3(nblk, 1), dim3(256), ldsb, st, a);
    if (int rc = check_launch("fdet_stem_fwd_q8_u8")) return rc;
  }
  return 0;
}

// the pipelined weight gradient covers this shape (any N: chunks of stem_x3_chunk images); precision16 has no other kernel
bool stem_x3_wgrad_pipe_ok(int N, int F, int H, int W) {
  const char* e = FDET_ENV_ONCE("FDET_STEM_PIPE");
  const int Wo = (W + 4 - 10) / 8 + 1;
  return !(e && e[0] == '0') && N > 0 && F > 0 && H >= 10 && Wo <= 60 && Wo > 48 && stem_x3_chunk(F, H, W, 0) >= 1;
}

// workspace of stem_x3_wgrad: per-workgroup partials [slabs][FP][320] then [slabs][FP]; one slab per workgroup of every chunk
size_t stem_x3_wgrad_ws_floats(int N, int F, int H, int W) {
  const int Ho = (H + 4 - 10) / 8 + 1;
  const int FP = (F + 63) / 64 * 64;
  const int chunk = std::max(1, stem_x3_chunk(F, H, W, 0));
  size_t slabs = 0;
  for (int n0 = 0; n0 < N; n0 += chunk) slabs += (size_t)std::min(std::min(chunk, N - n0) * Ho, 256);
  return slabs * FP * 320 + slabs * FP;
}

int stem_x3_wgrad(const float* x, const float* dy, float* dW, float* db, float* ws, int N, int F, int H, int W,
                  hipStream_t st, bool p16) {
  const int Ho = (H + 4 - 10) / 8 + 1, Wo = (W + 4 - 10) / 8 + 1;
  const int FP = (F + 63) / 64 * 64;
  const size_t lds = ((size_t)NPLANE * PE * 2 + 64 * DL * 2) * 2;
  StemWgX3Args a{};
  a.F = F; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
  int slabs = 0;
  if (stem_x3_wgrad_pipe_ok(N, F, H, W)) {
    // pipelined: two plane tiles of 9-chunk planes, exactly four 16-column k-steps (48 < Wo <= 60), 32-bit byte offsets:
    // a chunk's workgroups write consecutive slabs of one workspace, and one reduction sums the slabs of all chunks
    const size_t lds2 = ((size_t)2 * TILEP + 2 * 64 * DL + 8 * PEP) * 2;
    const void* kern = p16 ? (const void*)k_stem_wgrad_x3_pipe<true> : (const void*)k_stem_wgrad_x3_pipe<false>;
    { if (int rc_ = set_lds_attr(kern, (size_t)(lds2), __func__)) return rc_; }
    const int chunk = stem_x3_chunk(F, H, W, 0);
    const size_t tot = stem_x3_wgrad_ws_floats(N, F, H, W) / ((size_t)FP * 321);
    for (int n0 = 0; n0 < N; n0 += chunk) {
      a.N = std::min(chunk, N - n0); a.nrows = a.N * Ho;
      a.x = x + (size_t)n0 * CIN * H * W; a.dy = dy + (size_t)n0 * F * Ho * Wo;
      const int nblk = a.nrows < 256 ? a.nrows : 256;
      a.ws = ws + (size_t)slabs * FP * 320; a.wsb = ws + tot * FP * 320 + (size_t)slabs * FP;
      stem_note_route(STEM_X3_PIPE, STEM_PASS_WGRAD, p16, false, false, nblk, a.nrows);
      if (p16) hipLaunchKernelGGL(k_stem_wgrad_x3_pipe<true>, dim3(nblk, FP / 64), dim3(256), lds2, st, a);
      else hipLaunchKernelGGL(k_stem_wgrad_x3_pipe<false>, dim3(nblk, FP / 64), dim3(256), lds2, st, a);
      if (int rc = check_launch("fdet_stem_wgrad(bf16x3)")) return rc;
      slabs += nblk;
    }
    a.ws = ws; a.wsb = ws + tot * FP * 320;
  } else {
    if (p16) return fail(FDET_EINVAL, "stem_wgrad (precision16): only the pipelined kernel's shapes (48 < Wo <= 60) are built");
    a.x = x; a.dy = dy; a.N = N; a.nrows = N * Ho;
    slabs = a.nrows < 256 ? a.nrows : 256;
    a.ws = ws; a.wsb = ws + (size_t)slabs * FP * 320;
    { if (int rc_ = set_lds_attr((const void*)k_stem_wgrad_x3, (size_t)(lds), __func__)) return rc_; }
    stem_note_route(STEM_X3_SINGLE, STEM_PASS_WGRAD, false, false, false, slabs, a.nrows);
    hipLaunchKernelGGL(k_stem_wgrad_x3, dim3(slabs, FP / 64), dim3(256), lds, st, a);
    if (int rc = check_launch("fdet_stem_wgrad(bf16x3)")) return rc;
  }
  hipLaunchKernelGGL(k_stem_x3_reduce, dim3(5, F), dim3(1024), 0, st, a.ws, a.wsb, slabs, F, FP, dW, db);
  return check_launch("fdet_stem_wgrad(bf16x3 reduce)");
}

}  // namespace fdet
