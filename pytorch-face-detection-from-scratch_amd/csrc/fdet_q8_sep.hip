// Int8 inference of the SeparableCNN residual block (gfx950): pw1 1x1 -> LeakyReLU -> depthwise 3x3 -> LeakyReLU -> pw2 1x1
// -> + skip (-> 2x2 max) as ONE kernel, the two pointwise convs on the integer matrix cores (v_mfma_i32_16x16x64_i8).  The
// arithmetic is the contract of include/fdet.h ("Int8 inference: the separable block"); tests/q8_sep_cpu_ref.py restates it
// in numpy and the GPU tests demand equality.
//
// One workgroup (4 waves) owns one image x one tile of R rows x CW columns and keeps in LDS
//     P   the block's parameters: w1 [C][C], w2 [C][C], wd [9][C] (int8), mul1, mul2, mul3 [C] (fp32): 2 C^2 + 21 C bytes
//     X   the x tile with a one-position halo, (R+2)(CW+2) positions of C bytes, as it lies in memory (channel innermost:
//         a lane's MFMA B operand is 16 contiguous bytes); positions past the padded image are zero-filled
//     A   a plane of the same shape: a_q on every haloed position (GEMM 1), and after the depthwise pass the block's output
//         codes on the tile's own positions (GEMM 2's epilogue): its ring still holds a_q of the halo positions
//     B   b_q on the tile's own R x CW positions
// GEMM 1 runs over every haloed position: pw1 has no bias and lrelu(0) = 0, so the Q8 halo of zeros gives a_q = 0 outside
// the image and the depthwise pass tests no bounds.  The pointwise GEMMs take 16 positions per MFMA column tile from the flat
// position list of a plane; weights are the A operand (lane l: 16 consecutive ci of row co = 16 t + (l & 15) from
// ci = 64 kc + 16 (l >> 4)) and stay in registers for a whole phase; D gives lane l the channels 16 t + 4 (l >> 4) + r of
// position (l & 15): one dword.  The depthwise conv is vector ALU on bytes: a thread owns four channels (one dword) and walks
// positions, nine dword reads and 36 multiply-adds each, int32 accumulators (|acc| <= 9 * 127 * 127).
// The chain (fdet_q8_sepchain) is the same device code looped over blocks with the whole map as the one tile: X and A swap
// roles from block to block (the output written into A is the next block's x, its ring the zeros GEMM 1 produced from the
// halo), and the parameters of up to Q8S_WIN blocks are staged at once.
#include "fdet_common.h"
#include "fdet_q8_common.h"

namespace {
using namespace fdet;

using q8::v4i;
using q8::v4f;

constexpr int Q8S_THREADS = 256;
constexpr size_t Q8S_LDS_PLAN = 80 * 1024;         // the planner's budget: two workgroups per CU
constexpr int Q8SC_MAXB = 16;                      // blocks per chain launch
constexpr int Q8SC_MAXHW = 16;
constexpr int Q8S_WIN = 10;                        // blocks whose parameters the chain keeps in LDS at once

__host__ __device__ inline bool q8s_shape_ok(int C, int H, int W) {
  return (C == 64 || C == 128) && q8::act_shape_ok(C, H, W, 64);
}

__host__ __device__ inline int q8s_param_bytes(int C) { return 2 * C * C + 21 * C; }

__host__ __device__ inline size_t q8s_tile_lds(int C, int R, int CW) {
  return (size_t)q8s_param_bytes(C) + (size_t)C * (2ull * (R + 2) * (CW + 2) + (size_t)R * CW);
}

inline size_t q8s_bytes(int N, int C, int H, int W) { return q8s_shape_ok(C, H, W) ? q8::act_bytes(N, C, H, W, 64) : 0; }

// one block's parameters, global -> LDS in the order of the header comment (every piece a multiple of 16 bytes)
struct Q8SepParams {
  const signed char* w1;
  const signed char* wd;
  const signed char* w2;
  const float* mul1;
  const float* mul2;
  const float* mul3;
};

template <int KC>
__device__ __forceinline__ void q8s_stage_params(unsigned char* dst, const Q8SepParams& p) {
  constexpr int C = 64 * KC;
  constexpr int UW = C * C / 16, UD = 9 * C / 16, UM = C / 4;
  v4i* d = reinterpret_cast<v4i*>(dst);
  for (int i = threadIdx.x; i < 2 * UW + UD + 3 * UM; i += Q8S_THREADS) {
    const v4i* s;
    int j = i;
    if (j < UW) s = reinterpret_cast<const v4i*>(p.w1);
    else if ((j -= UW) < UW) s = reinterpret_cast<const v4i*>(p.w2);
    else if ((j -= UW) < UD) s = reinterpret_cast<const v4i*>(p.wd);
    else if ((j -= UD) < UM) s = reinterpret_cast<const v4i*>(p.mul1);
    else if ((j -= UM) < UM) s = reinterpret_cast<const v4i*>(p.mul2);
    else { j -= UM; s = reinterpret_cast<const v4i*>(p.mul3); }
    d[i] = s[j];
  }
}

// One pointwise GEMM over `npos` consecutive positions of `src` (C bytes each).  EPI(pos, co, acc) takes the four int32
// sums of channels co .. co + 3 of a position below npos.
template <int KC, class Epi>
__device__ __forceinline__ void q8s_pointwise(const unsigned char* src, const unsigned char* w, int npos, Epi epi) {
  constexpr int C = 64 * KC, T = C / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lp = lane & 15, lk = lane >> 4;
  v4i wf[T][KC];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) wf[t][kc] = *reinterpret_cast<const v4i*>(w + (16 * t + lp) * C + kc * 64 + lk * 16);
  const int groups = (npos + 15) >> 4;
  for (int g = wave; g < groups; g += Q8S_THREADS / 64) {
    const int pos = g * 16 + lp;
    const unsigned char* xr = src + min(pos, npos - 1) * C + lk * 16;
    v4i b[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) b[kc] = *reinterpret_cast<const v4i*>(xr + kc * 64);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      v4i acc = {0, 0, 0, 0};
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[t][kc], b[kc], acc, 0, 0, 0);
      if (pos < npos) epi(pos, 16 * t + 4 * lk, acc);
    }
  }
}

// The block on one tile: X (haloed x) -> A's own positions (the output codes).  A and B are scratch planes.  Ends with a
// barrier; the caller has put a barrier between its writes to X / the parameters and this call.
template <int KC>
__device__ __forceinline__ void q8s_block(const unsigned char* X, unsigned char* A, unsigned char* B, const unsigned char* P, int R,
                                          int CW, float skip_mul, float slope) {
  constexpr int C = 64 * KC;
  const int CWP = CW + 2;
  const unsigned char* w1 = P;
  const unsigned char* w2 = P + C * C;
  const unsigned char* wd = P + 2 * C * C;
  const float* mul1 = reinterpret_cast<const float*>(P + 2 * C * C + 9 * C);
  const float* mul2 = mul1 + C;
  const float* mul3 = mul2 + C;
  // GEMM 1 on every haloed position
  q8s_pointwise<KC>(X, w1, (R + 2) * CWP, [&](int pos, int co, v4i acc) {
    const v4f m = *reinterpret_cast<const v4f*>(mul1 + co);
    int q[4];
    q8::requant4(q, acc, m, slope, false, 0, 0.0f);
    *reinterpret_cast<int*>(A + pos * C + co) = q8::pack4(q[0], q[1], q[2], q[3]);
  });
  __syncthreads();
  // depthwise 3x3: a thread owns channels 4 g .. 4 g + 3
  {
    constexpr int G = C / 4;
    const int g = threadIdx.x % G;
    int wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const int*>(wd + k * C + 4 * g);
    const v4f m = *reinterpret_cast<const v4f*>(mul2 + 4 * g);
    for (int p = threadIdx.x / G; p < R * CW; p += Q8S_THREADS / G) {
      const int r = p / CW, c = p - r * CW;
      const unsigned char* ap = A + (r * CWP + c) * C + 4 * g;
      int acc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int v = *reinterpret_cast<const int*>(ap + (ky * CWP + kx) * C);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] += q8::byte_of(v, j) * q8::byte_of(wt[ky * 3 + kx], j);
        }
      int q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = q8::round_q(q8::lrelu((float)acc[j] * m[j], slope));
      *reinterpret_cast<int*>(B + p * C + 4 * g) = q8::pack4(q[0], q[1], q[2], q[3]);
    }
  }
  __syncthreads();
  // GEMM 2 on the tile's own positions, + skip, into A (whose own positions the depthwise pass has finished reading)
  q8s_pointwise<KC>(B, w2, R * CW, [&](int pos, int co, v4i acc) {
    const int r = pos / CW, c = pos - r * CW;
    const int off = ((r + 1) * CWP + c + 1) * C + co;
    const v4f m = *reinterpret_cast<const v4f*>(mul3 + co);
    const int sk = *reinterpret_cast<const int*>(X + off);
    int q[4];
    q8::requant4(q, acc, m, 1.0f, true, sk, skip_mul);     // no activation: slope 1 (t * 1.0f is t)
    *reinterpret_cast<int*>(A + off) = q8::pack4(q[0], q[1], q[2], q[3]);
  });
  __syncthreads();
}

struct Q8SepGeo {
  int N, H, W, R, CW, bands, segs;
};

template <int KC, bool POOL>
__global__ __launch_bounds__(Q8S_THREADS) void k_q8_sepblock(const signed char* __restrict__ x, Q8SepParams prm, float skip_mul,
                                                             signed char* __restrict__ y, Q8SepGeo g, float slope) {
  constexpr int C = 64 * KC, U = C / 16;           // 16-byte units per position
  extern __shared__ __attribute__((aligned(16))) unsigned char q8s_lds[];
  const int R = g.R, CW = g.CW, CWP = CW + 2;
  const int plane = (R + 2) * CWP * C;
  unsigned char* const P = q8s_lds;
  unsigned char* const X = P + q8s_param_bytes(C);
  unsigned char* const A = X + plane;
  unsigned char* const B = A + plane;
  int tile = blockIdx.x;
  const int seg = tile % g.segs;
  tile /= g.segs;
  const int band = tile % g.bands;
  const int n = tile / g.bands;
  const int y0 = band * R, x0 = seg * CW;          // the tile's first own pixel = the padded coordinate of its halo corner
  const int HP = g.H + 2, WP = g.W + 2;
  q8s_stage_params<KC>(P, prm);
  {
    const int urow = CWP * U;
    const signed char* src = x + ((size_t)n * HP + y0) * WP * C + (size_t)x0 * C;
    for (int i = threadIdx.x; i < (R + 2) * urow; i += Q8S_THREADS) {
      const int r = i / urow, u = i - r * urow;
      v4i v = {0, 0, 0, 0};
      if (y0 + r < HP && x0 + u / U < WP) v = *reinterpret_cast<const v4i*>(src + (size_t)r * WP * C + (size_t)u * 16);
      reinterpret_cast<v4i*>(X)[i] = v;
    }
  }
  __syncthreads();
  q8s_block<KC>(X, A, B, P, R, CW, skip_mul, slope);
  const int rows = min(R, g.H - y0), cols = min(CW, g.W - x0);      // the tile's real pixels
  if (POOL) {
    const int Ho = g.H >> 1, Wo = g.W >> 1;
    const int pr = rows >> 1, pc = cols >> 1, G = C / 4;
    signed char* dst = y + (((size_t)n * (Ho + 2) + (y0 >> 1) + 1) * (Wo + 2) + (x0 >> 1) + 1) * C;
    for (int i = threadIdx.x; i < pr * pc * G; i += Q8S_THREADS) {
      const int d = i % G;
      const int p = i / G;
      const int r = p / pc, c = p - r * pc;
      const unsigned char* s = A + ((2 * r + 1) * CWP + 2 * c + 1) * C + 4 * d;
      const int top = q8::max4(*reinterpret_cast<const int*>(s), *reinterpret_cast<const int*>(s + C));
      const int bot = q8::max4(*reinterpret_cast<const int*>(s + CWP * C), *reinterpret_cast<const int*>(s + CWP * C + C));
      *reinterpret_cast<int*>(dst + ((size_t)r * (Wo + 2) + c) * C + 4 * d) = q8::max4(top, bot);
    }
  } else {
    signed char* dst = y + (((size_t)n * HP + y0 + 1) * WP + x0 + 1) * C;
    const int urow = cols * U;
    for (int i = threadIdx.x; i < rows * urow; i += Q8S_THREADS) {
      const int r = i / urow, u = i - r * urow;
      *reinterpret_cast<v4i*>(dst + (size_t)r * WP * C + (size_t)u * 16) =
          *reinterpret_cast<const v4i*>(A + ((r + 1) * CWP + 1) * C + u * 16);
    }
  }
}

struct Q8SepChainArgs {
  const signed char* x;
  Q8SepParams prm[Q8SC_MAXB];
  signed char* out[Q8SC_MAXB];                      // per block: Q8 output, or nullptr
  float skip_mul[Q8SC_MAXB];
  float* out_f32;
  float out_scale, slope;
  int nblocks, N, H, W;
};

__host__ __device__ inline bool q8s_chain_shape_ok(int C, int H, int W) {
  return C == 64 && H >= 1 && W >= 1 && H <= Q8SC_MAXHW && W <= Q8SC_MAXHW;
}

inline size_t q8s_chain_lds(int nblocks, int H, int W) {
  const int win = nblocks < Q8S_WIN ? nblocks : Q8S_WIN;
  return (size_t)win * q8s_param_bytes(64) + 64 * (2 * (size_t)(H + 2) * (W + 2) + (size_t)H * W);
}

__global__ __launch_bounds__(Q8S_THREADS) void k_q8_sepchain(const Q8SepChainArgs a) {
  constexpr int C = 64, PB = 2 * C * C + 21 * C;
  extern __shared__ __attribute__((aligned(16))) unsigned char q8s_lds[];
  const int H = a.H, W = a.W, WP = W + 2;
  const int plane = (H + 2) * WP * C;
  const int win = min(a.nblocks, Q8S_WIN);
  unsigned char* const P = q8s_lds;
  unsigned char* X = P + win * PB;
  unsigned char* A = X + plane;
  unsigned char* const B = A + plane;
  const bool resident = a.nblocks <= Q8S_WIN;       // every block's parameters fit: staged once per workgroup
  if (resident)
    for (int k = 0; k < a.nblocks; ++k) q8s_stage_params<1>(P + k * PB, a.prm[k]);
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    const v4i* src = reinterpret_cast<const v4i*>(a.x + (size_t)n * plane);
    for (int i = threadIdx.x; i < plane / 16; i += Q8S_THREADS) reinterpret_cast<v4i*>(X)[i] = src[i];
    for (int k0 = 0; k0 < a.nblocks; k0 += Q8S_WIN) {
      const int cnt = min(Q8S_WIN, a.nblocks - k0);
      if (!resident)                                // (the previous window's last reads ended at the barrier that closes q8s_block)
        for (int k = 0; k < cnt; ++k) q8s_stage_params<1>(P + k * PB, a.prm[k0 + k]);
      __syncthreads();
      for (int k = k0; k < k0 + cnt; ++k) {
        q8s_block<1>(X, A, B, P + (k - k0) * PB, H, W, a.skip_mul[k], a.slope);
        // the output is A's interior, its ring the zeros of GEMM 1 on the halo: A is the next block's x.  The copies below
        // only read it; the next block writes the old X, which nobody reads any more.
        if (a.out[k] != nullptr) {
          signed char* dst = a.out[k] + (size_t)n * plane;
          const int urow = W * (C / 16);
          for (int i = threadIdx.x; i < H * urow; i += Q8S_THREADS) {
            const int r = i / urow, u = i - r * urow;
            const int off = ((r + 1) * WP + 1) * C + u * 16;
            *reinterpret_cast<v4i*>(dst + off) = *reinterpret_cast<const v4i*>(A + off);
          }
        }
        if (k + 1 == a.nblocks && a.out_f32 != nullptr) {
          const int hw = H * W;
          float* dst = a.out_f32 + (size_t)n * C * hw;
          for (int i = threadIdx.x; i < (C / 4) * hw; i += Q8S_THREADS) {
            const int c4 = i / hw, p = i - c4 * hw;
            const int yy = p / W, xx = p - yy * W;
            const int v = *reinterpret_cast<const int*>(A + ((yy + 1) * WP + xx + 1) * C + 4 * c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(size_t)(4 * c4 + j) * hw + p] = (float)q8::byte_of(v, j) * a.out_scale;
          }
        }
        unsigned char* t = X;
        X = A;
        A = t;
      }
    }
    __syncthreads();                                // the copies out of the last output end before the next image lands
  }
}

// The planner: among the tilings (bands x segments of equal size, rounded up; even when pooled) whose LDS fits the budget,
// the fewest GEMM-1 MFMA column tiles (16 haloed positions each) over the map; ties go to the fewer tiles.
bool q8s_plan(int C, int H, int W, int pool, int* rows, int* cols, size_t* lds) {
  if (!q8s_shape_ok(C, H, W) || (pool && ((H | W) & 1))) return false;
  const long long avail = ((long long)Q8S_LDS_PLAN - q8s_param_bytes(C)) / C;    // position-sized units for the three planes
  long long best = -1, best_tiles = 0;
  for (int nb = 1; nb <= H; ++nb) {
    int R = (H + nb - 1) / nb;
    if (pool && (R & 1)) ++R;
    if ((H + R - 1) / R != nb) continue;            // the same R as a smaller band count
    // 2 (R+2)(CW+2) + R CW <= avail
    long long cwmax = (avail - 4ll * (R + 2)) / (3ll * R + 4);
    if (cwmax > W) cwmax = W;
    if (pool) cwmax &= ~1ll;
    if (cwmax < (pool ? 2 : 1)) continue;
    const int ns = (int)((W + cwmax - 1) / cwmax);
    int CW = (W + ns - 1) / ns;
    if (pool && (CW & 1)) ++CW;                     // (<= cwmax: cwmax is even)
    const int segs = (W + CW - 1) / CW;
    const long long tiles = (long long)nb * segs;
    const long long cost = tiles * (((long long)(R + 2) * (CW + 2) + 15) / 16);
    if (best < 0 || cost < best || (cost == best && tiles < best_tiles)) {
      best = cost;
      best_tiles = tiles;
      *rows = R;
      *cols = CW;
    }
  }
  if (best < 0) return false;
  *lds = q8s_tile_lds(C, *rows, *cols);
  return true;
}

template <int KC>
int q8s_launch(const signed char* x, const Q8SepParams& prm, float skip_mul, signed char* y, const Q8SepGeo& g, int pool, size_t lds,
               float slope, hipStream_t stream) {
  const void* kern = pool ? (const void*)k_q8_sepblock<KC, true> : (const void*)k_q8_sepblock<KC, false>;
  if (lds > 64 * 1024) {
    const int rc = set_lds_attr(kern, lds, "fdet_q8_sepblock");
    if (rc != FDET_OK) return rc;
  }
  const dim3 grid((unsigned)(g.N * g.bands * g.segs));
  if (pool)
    hipLaunchKernelGGL((k_q8_sepblock<KC, true>), grid, dim3(Q8S_THREADS), lds, stream, x, prm, skip_mul, y, g, slope);
  else
    hipLaunchKernelGGL((k_q8_sepblock<KC, false>), grid, dim3(Q8S_THREADS), lds, stream, x, prm, skip_mul, y, g, slope);
  return check_launch("fdet_q8_sepblock");
}

}  // namespace

extern "C" int fdet_q8_sepblock_supported(int C, int H, int W) { return q8s_shape_ok(C, H, W) ? 1 : 0; }

extern "C" int fdet_q8_sepblock_plan(int C, int H, int W, int pool, int* rows, int* cols, size_t* lds_bytes) {
  int r = 0, c = 0;
  size_t l = 0;
  if (!rows || !cols || !lds_bytes || !q8s_plan(C, H, W, pool ? 1 : 0, &r, &c, &l)) return 0;
  *rows = r;
  *cols = c;
  *lds_bytes = l;
  return 1;
}

extern "C" int fdet_q8_sepblock(const int8_t* x, const int8_t* w1, const float* mul1, const int8_t* wd, const float* mul2,
                                const int8_t* w2, const float* mul3, float skip_mul, int8_t* y, int N, int C, int H, int W, int pool,
                                int tile_rows, int tile_cols, float slope, void* stream) {
  FDET_REQUIRE(x && w1 && mul1 && wd && mul2 && w2 && mul3 && y && q8s_bytes(N, C, H, W) > 0,
               "q8_sepblock: unsupported shape N=%d C=%d H=%d W=%d (C 64 or 128, 1 <= H, W <= %d, under 2 GiB)", N, C, H, W, q8::MAX_HW);
  FDET_REQUIRE(pool == 0 || pool == 1, "q8_sepblock: pool must be 0 or 1");
  FDET_REQUIRE(!pool || (!(H & 1) && !(W & 1)), "q8_sepblock: the pooled form needs even H and W, got %dx%d", H, W);
  FDET_REQUIRE(q8::aligned16(x) && q8::aligned16(w1) && q8::aligned16(mul1) && q8::aligned16(wd) && q8::aligned16(mul2) &&
               q8::aligned16(w2) && q8::aligned16(mul3) && q8::aligned16(y), "q8_sepblock: every tensor must be 16-byte aligned");
  FDET_REQUIRE(x != y, "q8_sepblock: the output may not alias the input");
  FDET_REQUIRE((tile_rows == 0) == (tile_cols == 0) && tile_rows >= 0 && tile_cols >= 0,
               "q8_sepblock: tile_rows and tile_cols are both 0 (the planner) or both positive, got %d, %d", tile_rows, tile_cols);
  int R = tile_rows, CW = tile_cols;
  size_t lds = 0;
  if (R == 0) {
    FDET_REQUIRE(q8s_plan(C, H, W, pool, &R, &CW, &lds), "q8_sepblock: no tiling for C=%d %dx%d", C, H, W);
  } else {
    FDET_REQUIRE(R <= q8::MAX_HW && CW <= q8::MAX_HW && (!pool || (!(R & 1) && !(CW & 1))),
                 "q8_sepblock: a forced tile is at most %d a side and even when pooled, got %dx%d", q8::MAX_HW, R, CW);
    lds = q8s_tile_lds(C, R, CW);
    FDET_REQUIRE(lds <= q8::LDS_MAX, "q8_sepblock: a %dx%d tile of %d channels needs %zu bytes of LDS (at most %zu)", R, CW, C, lds,
                 q8::LDS_MAX);
  }
  Q8SepGeo g{N, H, W, R, CW, (H + R - 1) / R, (W + CW - 1) / CW};
  FDET_REQUIRE((long long)N * g.bands * g.segs < (1ll << 31), "q8_sepblock: too many tiles");
  const Q8SepParams prm{reinterpret_cast<const signed char*>(w1), reinterpret_cast<const signed char*>(wd),
                        reinterpret_cast<const signed char*>(w2), mul1, mul2, mul3};
  const signed char* xs = reinterpret_cast<const signed char*>(x);
  signed char* ys = reinterpret_cast<signed char*>(y);
  return C == 64 ? q8s_launch<1>(xs, prm, skip_mul, ys, g, pool, lds, slope, (hipStream_t)stream)
                 : q8s_launch<2>(xs, prm, skip_mul, ys, g, pool, lds, slope, (hipStream_t)stream);
}

extern "C" int fdet_q8_sepchain_supported(int C, int H, int W) { return q8s_chain_shape_ok(C, H, W) ? 1 : 0; }

extern "C" int fdet_q8_sepchain(const int8_t* x, const int8_t* const* h_w1, const float* const* h_mul1, const int8_t* const* h_wd,
                                const float* const* h_mul2, const int8_t* const* h_w2, const float* const* h_mul3,
                                const float* h_skip_mul, int8_t* const* h_out, float* out_f32, float out_scale, int nblocks, int N,
                                int C, int H, int W, float slope, void* stream) {
  FDET_REQUIRE(q8s_chain_shape_ok(C, H, W) && N >= 1 && q8s_bytes(N, C, H, W) > 0,
               "q8_sepchain: unsupported shape N=%d C=%d H=%d W=%d (C == 64, 1 <= H, W <= %d)", N, C, H, W, Q8SC_MAXHW);
  FDET_REQUIRE(nblocks >= 1 && nblocks <= Q8SC_MAXB, "q8_sepchain: nblocks must be 1..%d, got %d", Q8SC_MAXB, nblocks);
  FDET_REQUIRE(x && h_w1 && h_mul1 && h_wd && h_mul2 && h_w2 && h_mul3 && h_skip_mul, "q8_sepchain: null argument");
  FDET_REQUIRE((h_out && h_out[nblocks - 1]) || out_f32, "q8_sepchain: the last block needs an output (h_out[nblocks - 1] or out_f32)");
  FDET_REQUIRE(out_f32 == nullptr || (out_scale > 0.0f && out_scale <= 3.0e38f), "q8_sepchain: out_scale must be positive and finite");
  Q8SepChainArgs a{};
  a.x = reinterpret_cast<const signed char*>(x);
  bool ok = q8::aligned16(x) && q8::aligned16(out_f32);
  for (int k = 0; k < nblocks; ++k) {
    FDET_REQUIRE(h_w1[k] && h_mul1[k] && h_wd[k] && h_mul2[k] && h_w2[k] && h_mul3[k], "q8_sepchain: null tensor in block %d", k);
    a.prm[k] = Q8SepParams{reinterpret_cast<const signed char*>(h_w1[k]), reinterpret_cast<const signed char*>(h_wd[k]),
                           reinterpret_cast<const signed char*>(h_w2[k]), h_mul1[k], h_mul2[k], h_mul3[k]};
    a.skip_mul[k] = h_skip_mul[k];
    a.out[k] = h_out ? reinterpret_cast<signed char*>(h_out[k]) : nullptr;
    FDET_REQUIRE(a.out[k] == nullptr || a.out[k] != a.x, "q8_sepchain: an output may not alias x");
    ok = ok && q8::aligned16(h_w1[k]) && q8::aligned16(h_mul1[k]) && q8::aligned16(h_wd[k]) && q8::aligned16(h_mul2[k]) &&
         q8::aligned16(h_w2[k]) && q8::aligned16(h_mul3[k]) && q8::aligned16(a.out[k]);
  }
  FDET_REQUIRE(ok, "q8_sepchain: every tensor must be 16-byte aligned");
  a.out_f32 = out_f32;
  a.out_scale = out_scale;
  a.slope = slope;
  a.nblocks = nblocks;
  a.N = N; a.H = H; a.W = W;
  const size_t lds = q8s_chain_lds(nblocks, H, W);
  FDET_REQUIRE(lds <= q8::LDS_MAX, "q8_sepchain: %zu bytes of LDS", lds);
  if (lds > 64 * 1024) {
    const int rc = set_lds_attr((const void*)k_q8_sepchain, lds, "fdet_q8_sepchain");
    if (rc != FDET_OK) return rc;
  }
  const int per_cu = (int)(q8::LDS_MAX / lds) < 2 ? 1 : 2;
  const int grid = N < num_cus() * per_cu ? N : num_cus() * per_cu;
  hipLaunchKernelGGL(k_q8_sepchain, dim3((unsigned)grid), dim3(Q8S_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("fdet_q8_sepchain");
}
