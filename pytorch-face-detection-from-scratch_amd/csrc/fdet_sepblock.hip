// The depthwise-separable residual block of models/SeparableCNN.py:40-51 as ONE kernel (fp32 NCHW in and out):
//
//   a = lrelu(W1 x)   b = lrelu(dw3x3(a))   c = W2 b   e = c * drop_scale[n,c] + x   out = maxpool2x2(e) | e
//
// Both 1x1 convs are GEMMs on the bf16 matrix cores with the bf16x3 split (fp32-grade, see fdet_pointwise_x3.hip, whose
// forward weight panels this kernel reads); the depthwise 3x3 and both LeakyReLUs run in LDS between them, so that
// eval reads x once and writes out once.  None of the three convs has a bias, which makes zero padding exact: a halo
// position outside the image holds x = 0, hence a = lrelu(W1 0) = 0, which is the zero the depthwise conv pads with.
//
// One workgroup (4 waves) = one image x one tile of R rows x CW columns (the whole map when it fits).
//   phase A   x of the tile plus a one-position halo (clipped to the image) -> bf16 hi/lo units in LDS, all F channels
//   per group g of 32 channels (the M tile of GEMM 1 = two K chunks of GEMM 2):
//     B1  GEMM 1: a_g = lrelu(W1[32g..32g+31, :] x) over the haloed positions -> fp32 LDS plane [32][R+2][CW+2]
//                 (cells outside the image are zeroed once and never written)
//     B2  b_g = lrelu(dw(a_g)) over the tile's own positions -> bf16 hi/lo units in LDS
//     B3  GEMM 2: acc[F][R*CW] += W2[:, 32g..32g+31] b_g    (accumulators stay in registers over all groups)
//   phase C   e = acc * scale + x; stored directly, or pooled through LDS (x's units are dead by then) with one
//             routing byte per window in the format fdet_pool_route_bwd reads.
// LDS = 4 F' GP + 128 (R+2)(CW+2) + 128 PO bytes (F' = F rounded to 16, GP / PO = haloed / own positions rounded to 32);
// the host picks, among the (R, CW) that fit, the tile with the smallest halo overhead (fdet_sepblock_plan).
// Training additionally stores a and b (the two post-activation intermediates the composed backward reads) and the
// routing bytes; c and e are never written: backward needs neither (no activation follows the second GEMM).
#include "fdet_conv3x3_x3.h"
#include <algorithm>
#include <cstdint>

using namespace fdet;

namespace {

constexpr int SEP_THR = 256;
constexpr size_t SEP_LDS_MAX = 160 * 1024;

struct SepPlan {
  int R, CW, nbands, nseg, TH, TW, GPS, POS, KC, MG;   // tile, grid, haloed plane, position strides, K chunks, channel groups
  size_t lds;
};

struct SepArgs {
  const float* x;            // [N,F,H,W]
  const bf16x8* w1_hi;       // forward panel of fdet_pack_pointwise_weights_bf16x3: unit (c16*2 + h)*CoP + co
  const bf16x8* w1_lo;
  const bf16x8* w2_hi;
  const bf16x8* w2_lo;
  const float* wd;           // [F][9]
  const float* scale;        // [N,F] or null
  float* out;                // [N,F,H/pool,W/pool]
  float* a_save;             // [N,F,H,W] or null
  float* b_save;             // [N,F,H,W] or null
  unsigned char* route;      // [N,F,H/2,W/2] or null
  int N, F, H, W, pool, CoP;
  SepPlan p;
  float slope;
};

__device__ __forceinline__ float lrelu(float v, float s) { return v > 0.f ? v : v * s; }

template <int MT, int NT2>
__global__ void __launch_bounds__(SEP_THR)
k_sepblock_fwd(const SepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const SepPlan& pl = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int F = a.F, H = a.H, W = a.W;
  // tile of this workgroup
  int t = blockIdx.x;
  const int seg = t % pl.nseg; t /= pl.nseg;
  const int band = t % pl.nbands;
  const int img = t / pl.nbands;
  const int r0 = band * pl.R, c0 = seg * pl.CW;
  const int Rt = min(pl.R, H - r0), Ct = min(pl.CW, W - c0);
  const int gy0 = max(r0 - 1, 0), gy1 = min(r0 + Rt + 1, H), gx0 = max(c0 - 1, 0), gx1 = min(c0 + Ct + 1, W);
  const int GW = gx1 - gx0, GP = (gy1 - gy0) * GW, PO = Rt * Ct;
  const int GPS = pl.GPS, POS = pl.POS, TW = pl.TW, AST = pl.TH * pl.TW;
  const int nt1 = (GP + 31) >> 5, nt2 = (PO + 31) >> 5;

  bf16x8* x_hi = reinterpret_cast<bf16x8*>(smem);                  // [2 KC][GPS]
  bf16x8* x_lo = x_hi + 2 * pl.KC * GPS;
  float* a_g = reinterpret_cast<float*>(x_lo + 2 * pl.KC * GPS);   // [32][TH][TW]
  bf16x8* b_hi = reinterpret_cast<bf16x8*>(a_g + 32 * AST);        // [4][POS]
  bf16x8* b_lo = b_hi + 4 * POS;
  float* e_lds = reinterpret_cast<float*>(smem);                   // phase C (pooled): [F][PO], over the dead x units

  const size_t plane = (size_t)H * W;
  const float* __restrict__ xi = a.x + (size_t)img * F * plane;

  // ---- phase A: x -> hi/lo units; a_g cleared
  for (int it = tid; it < 2 * pl.KC * GPS; it += SEP_THR) {
    const int j8 = it / GPS, q = it - j8 * GPS;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = 0.f;
    if (q < GP) {
      const int gy = q / GW, gx = q - gy * GW;
      const float* __restrict__ src = xi + (size_t)(gy0 + gy) * W + gx0 + gx;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ch = j8 * 8 + j;
        if (ch < F) f[j] = src[(size_t)ch * plane];
      }
    }
    bf16x8 hi, lo;
    split8(f, hi, lo);
    x_hi[it] = hi;
    x_lo[it] = lo;
  }
  for (int it = tid; it < 32 * AST; it += SEP_THR) a_g[it] = 0.f;

  f32x16 acc[MT][NT2];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  __syncthreads();

  for (int g = 0; g < pl.MG; ++g) {
    // ---- B1: a_g = lrelu(W1[group g] x) over the haloed positions; wave w takes position tiles w, w+4, ...
    for (int nt = wid; nt < nt1; nt += 4) {
      f32x16 c1;
#pragma unroll
      for (int r = 0; r < 16; ++r) c1[r] = 0.f;
      for (int c = 0; c < pl.KC; ++c) {
        const size_t wu = (size_t)(c * 2 + half) * a.CoP + g * 32 + l31;
        const int bu = (c * 2 + half) * GPS + nt * 32 + l31;
        const bf16x8 ah = a.w1_hi[wu], al = a.w1_lo[wu];
        const bf16x8 bh = x_hi[bu], bl = x_lo[bu];
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c1, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c1, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c1, 0, 0, 0);
      }
      const int q = nt * 32 + l31;
      if (q < GP) {
        const int gy = q / GW, gx = q - gy * GW;
        const int y = gy0 + gy, xx = gx0 + gx;
        const int cell = (y - r0 + 1) * TW + (xx - c0 + 1);
        const bool own = a.a_save && y >= r0 && y < r0 + Rt && xx >= c0 && xx < c0 + Ct;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int chl = (r & 3) + 8 * (r >> 2) + 4 * half;
          const float v = lrelu(c1[r], a.slope);
          a_g[chl * AST + cell] = v;
          const int ch = g * 32 + chl;
          if (own && ch < F) a.a_save[((size_t)img * F + ch) * plane + (size_t)y * W + xx] = v;
        }
      }
    }
    __syncthreads();
    // ---- B2: b_g = lrelu(dw3x3(a_g)) over the tile's own positions -> hi/lo units (8 channels of one position each)
    for (int it = tid; it < 4 * POS; it += SEP_THR) {
      const int j8 = it / POS, p = it - j8 * POS;
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = 0.f;
      if (p < PO) {
        const int iy = p / Ct, ix = p - iy * Ct;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int chl = j8 * 8 + j, ch = g * 32 + chl;
          if (ch < F) {
            const float* __restrict__ wq = a.wd + (size_t)ch * 9;
            const float* __restrict__ ap = a_g + chl * AST + iy * TW + ix;
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) s = fmaf(wq[dy * 3 + dx], ap[dy * TW + dx], s);
            s = lrelu(s, a.slope);
            f[j] = s;
            if (a.b_save) a.b_save[((size_t)img * F + ch) * plane + (size_t)(r0 + iy) * W + c0 + ix] = s;
          }
        }
      }
      bf16x8 hi, lo;
      split8(f, hi, lo);
      b_hi[it] = hi;
      b_lo[it] = lo;
    }
    __syncthreads();
    // ---- B3: acc += W2[:, group g] b_g; wave w owns the output position tiles w, w+4, ...
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const int c = 2 * g + kc;
      if (c < pl.KC) {
        bf16x8 bh[NT2], bl[NT2];
#pragma unroll
        for (int n = 0; n < NT2; ++n) {
          const int nt = wid + 4 * n;
          const int bu = (kc * 2 + half) * POS + min(nt, nt2 - 1) * 32 + l31;
          bh[n] = b_hi[bu]; bl[n] = b_lo[bu];
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (m * 32 < F) {
            const size_t wu = (size_t)(c * 2 + half) * a.CoP + m * 32 + l31;
            const bf16x8 ah = a.w2_hi[wu], al = a.w2_lo[wu];
#pragma unroll
            for (int n = 0; n < NT2; ++n) {
              if (wid + 4 * n < nt2) {
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[n], acc[m][n], 0, 0, 0);
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[n], acc[m][n], 0, 0, 0);
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[n], acc[m][n], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    // (the next group's B1 writes a_g, which B2 is done with; its B2 writes b_g only after the barrier behind B1)
  }

  // ---- phase C: e = c * scale + x
  const float* __restrict__ sc = a.scale ? a.scale + (size_t)img * F : nullptr;
  if (a.pool == 2) __syncthreads();                       // every wave is done with x's units and b_g
#pragma unroll
  for (int n = 0; n < NT2; ++n) {
    const int p = (wid + 4 * n) * 32 + l31;
    if (wid + 4 * n < nt2 && p < PO) {
      const int iy = p / Ct, ix = p - iy * Ct;
      const size_t off = (size_t)(r0 + iy) * W + c0 + ix;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ch = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (ch < F) {
            const float e = acc[m][n][r] * (sc ? sc[ch] : 1.f) + xi[(size_t)ch * plane + off];
            if (a.pool == 2) e_lds[ch * PO + p] = e;
            else a.out[((size_t)img * F + ch) * plane + off] = e;
          }
        }
    }
  }
  if (a.pool != 2) return;
  __syncthreads();
  // 2x2 max pool (first maximum in scan order wins, NaN is a maximum: ATen) + routing byte: bits 4-5 = argmax, bits 0-3 set
  // (fdet_pool_route_bwd multiplies by lrelu' of the element before the dropout, which is 1 here: no activation follows W2)
  const int Hp = H >> 1, Wp = W >> 1, Rp = Rt >> 1, Cp = Ct >> 1;
  for (int it = tid; it < F * Rp * Cp; it += SEP_THR) {
    const int px = it % Cp, r = it / Cp, py = r % Rp, ch = r / Rp;
    const float* __restrict__ ep = e_lds + ch * PO + (2 * py) * Ct + 2 * px;
    const float v[4] = {ep[0], ep[1], ep[Ct], ep[Ct + 1]};
    float m = -INFINITY; int arg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (v[k] > m || v[k] != v[k]) { m = v[k]; arg = k; }
    const size_t o = (((size_t)img * F + ch) * Hp + (r0 >> 1) + py) * Wp + (c0 >> 1) + px;
    a.out[o] = m;
    if (a.route) a.route[o] = (unsigned char)(0x0F | (arg << 4));
  }
}

// out = g * scale[n,c] * lrelu'(act)   (scale / act may be null: factor 1); in place allowed
__global__ void __launch_bounds__(256)
k_sep_gate(const float* __restrict__ g, const float* __restrict__ act, const float* __restrict__ scale, float* __restrict__ out,
           size_t total, int P, float slope) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    float v = g[t];
    if (scale) v *= scale[t / P];
    if (act) v *= (act[t] > 0.f ? 1.f : slope);
    out[t] = v;
  }
}

__global__ void __launch_bounds__(256)
k_sep_lrelu(const float* __restrict__ z, float* __restrict__ y, size_t total, float slope) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) y[t] = lrelu(z[t], slope);
}

int round32(int v) { return (v + 31) / 32 * 32; }

// the tile with the least halo work among those that fit `budget` bytes of LDS and the accumulator tiles; false: none
bool sep_plan(int F, int H, int W, int pool, size_t budget, SepPlan& best) {
  if (F < 8 || F % 8 || F > 128 || H < 1 || W < 1 || (pool != 1 && pool != 2)) return false;
  if (pool == 2 && ((H | W) & 1)) return false;
  const int KC = (F + 15) / 16, MG = (F + 31) / 32;
  const int MT = MG > 2 ? 4 : MG, NT2 = MT == 4 ? 2 : 4;
  const int step = pool;
  double best_cost = 1e30;
  bool found = false;
  for (int nseg = 1; nseg <= W; ++nseg) {
    int CW = (W + nseg - 1) / nseg;
    if (pool == 2 && (CW & 1)) ++CW;
    if ((W + CW - 1) / CW != nseg) continue;
    for (int R = (pool == 2 ? 2 : 1); R <= H; R += step) {
      const int nb = (H + R - 1) / R;
      SepPlan p;
      p.R = R; p.CW = CW; p.nbands = nb; p.nseg = nseg; p.TH = R + 2; p.TW = CW + 2;
      p.GPS = round32(std::min(R + 2, H) * std::min(CW + 2, W));
      p.POS = round32(R * CW);
      p.KC = KC; p.MG = MG;
      if (p.POS > 32 * 4 * NT2) continue;
      p.lds = (size_t)4 * 16 * KC * p.GPS + (size_t)128 * p.TH * p.TW + (size_t)128 * p.POS;
      if (pool == 2 && (size_t)4 * F * R * CW > (size_t)4 * 16 * KC * p.GPS) continue;   // (never: GP >= PO)
      if (p.lds > budget) continue;
      // cost: GEMM 1 positions actually computed per own position (rounded tiles included), small tiles penalised a little
      const double cost = (double)nb * nseg * p.GPS / ((double)H * W) + 0.02 * nb * nseg;
      if (cost < best_cost) { best_cost = cost; best = p; found = true; }
    }
  }
  return found;
}

template <int MT, int NT2>
int sep_launch(const SepArgs& a, hipStream_t st) {
  if (int rc = set_lds_attr((const void*)k_sepblock_fwd<MT, NT2>, a.p.lds, "fdet_sepblock_fwd")) return rc;
  const unsigned grid = (unsigned)((size_t)a.N * a.p.nbands * a.p.nseg);
  hipLaunchKernelGGL((k_sepblock_fwd<MT, NT2>), dim3(grid), dim3(SEP_THR), a.p.lds, st, a);
  return check_launch("fdet_sepblock_fwd");
}

}  // namespace

extern "C" int fdet_sepblock_plan(int F, int H, int W, int pool, int* out, int n) {
  SepPlan p;
  const bool ok = sep_plan(F, H, W, pool, SEP_LDS_MAX, p);
  const int v[6] = {ok ? p.R : 0, ok ? p.CW : 0, ok ? p.nbands : 0, ok ? p.nseg : 0, ok ? (int)p.lds : 0, ok ? p.GPS : 0};
  for (int i = 0; out && i < n && i < 6; ++i) out[i] = v[i];
  return ok ? 1 : 0;
}

extern "C" int fdet_sepblock_fwd(const float* x, const void* w1_pk, const float* wd, const void* w2_pk, const float* drop_scale,
                                 float* out, float* a_save, float* b_save, unsigned char* route, int N, int F, int H, int W,
                                 int pool, float slope, void* stream) {
  FDET_REQUIRE(x && w1_pk && wd && w2_pk && out && N > 0, "sepblock_fwd: bad arguments");
  FDET_REQUIRE((a_save == nullptr) == (b_save == nullptr), "sepblock_fwd: a_save and b_save go together");
  FDET_REQUIRE(!route || (pool == 2 && a_save), "sepblock_fwd: routing bytes belong to a pooled training pass");
  SepArgs a;
  FDET_REQUIRE(sep_plan(F, H, W, pool, SEP_LDS_MAX, a.p),
               "sepblock_fwd: no tiling for F=%d H=%d W=%d pool=%d (F %% 8 == 0, 8 <= F <= 128; even maps when pooling)", F, H, W, pool);
  FDET_REQUIRE((size_t)N * a.p.nbands * a.p.nseg < ((size_t)1 << 31), "sepblock_fwd: too many tiles");
  a.x = x; a.wd = wd; a.scale = drop_scale; a.out = out; a.a_save = a_save; a.b_save = b_save; a.route = route;
  a.N = N; a.F = F; a.H = H; a.W = W; a.pool = pool; a.slope = slope;
  a.CoP = (F + 31) / 32 * 32;
  const size_t units = (size_t)((F + 15) / 16) * 2 * a.CoP;
  a.w1_hi = reinterpret_cast<const bf16x8*>(w1_pk); a.w1_lo = a.w1_hi + units;
  a.w2_hi = reinterpret_cast<const bf16x8*>(w2_pk); a.w2_lo = a.w2_hi + units;
  hipStream_t st = (hipStream_t)stream;
  if (a.p.MG > 2) return sep_launch<4, 2>(a, st);
  if (a.p.MG == 2) return sep_launch<2, 4>(a, st);
  return sep_launch<1, 4>(a, st);
}

extern "C" int fdet_sepblock_gate_bwd(const float* g, const float* act, const float* drop_scale, float* out, int N, int F, int P,
                                      float slope, void* stream) {
  FDET_REQUIRE(g && out && N > 0 && F > 0 && P > 0, "sepblock_gate_bwd: bad arguments");
  const size_t total = (size_t)N * F * P;
  size_t blocks = (total + 255) / 256; if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_sep_gate, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, act, drop_scale, out, total, P, slope);
  return check_launch("fdet_sepblock_gate_bwd");
}

extern "C" int fdet_sepblock_lrelu(const float* z, float* y, size_t n, float slope, void* stream) {
  FDET_REQUIRE(z && y && n > 0, "sepblock_lrelu: bad arguments");
  size_t blocks = (n + 255) / 256; if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_sep_lrelu, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, y, n, slope);
  return check_launch("fdet_sepblock_lrelu");
}
