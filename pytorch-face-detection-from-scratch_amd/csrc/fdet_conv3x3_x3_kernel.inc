// 3x3 convolutions (forward and data gradient) on the bf16 matrix cores with fp32-level accuracy:
// every fp32 operand x is split into two bf16 values  x = hi + lo  (hi = bf16(x), lo = bf16(x-hi))
// and a product is evaluated as  a_hi*b_lo + a_lo*b_hi + a_hi*b_hi  with fp32 accumulation
// ("bf16x3").  The dropped a_lo*b_lo term is 2^-16 relative, so results stay within ~1e-5 of the
// fp32 FMA chain (tests: 1e-4) while v_mfma_f32_32x32x16_bf16 delivers 16x the K per clock of the
// f32 MFMA: three passes are ~5x faster, which moves the 3x3 convs from MFMA-bound to HBM-bound.
//
// Implicit GEMM over "flattened padded rows": the batch is one tall virtual image (image n owns
// virtual rows n(H+1)+1 .. n(H+1)+H, row n(H+1) is a shared zero row); a tile is a band of R
// virtual rows x one column segment of CW columns, laid out in LDS with row pitch WP (multiple of
// 4): slot 0 = left halo, slots 1..CW = data, slot CW+1 = right halo.  An output position
// q = row*WP + col reads tap (ky,kx) at q + ky*WP + kx -- a constant offset per tap.
//   M = 32 positions per MFMA tile (A operand = activations), N = 32 output channels (B operand =
//   weights), K = 16 input channels at ONE tap.  LDS is channel-innermost:
//     activations: four arrays {hi,lo} x {k-half} of [position][8 x bf16]   (16 B per position)
//     weights:     {hi,lo} x [tap][k-half][co][8 x bf16]                    (pre-split panels in HBM)
//   so every fragment is one aligned ds_read_b128 and consecutive lanes read consecutive slots.
// With positions on the accumulator ROWS a lane holds 4 consecutive positions of one channel:
// the epilogue loads/stores 16 bytes per lane (NCHW rows are contiguous) -- 4x fewer memory
// instructions than a channel-per-register epilogue, which was store-issue bound.
//
// Persistent workgroups (one per CU, 4 waves, 512-register budget, ~155 KB LDS): a workgroup walks
// tiles t, t+G, ...; LDS is double buffered per 16-channel chunk and the pipeline runs ACROSS
// tiles: while chunk s is in the MFMA loop the global loads of chunk s+1 (possibly the next tile's
// first chunk) are in flight, and their fp32 -> (hi,lo) split + LDS writes are interleaved with
// the MFMAs of the later taps.  One barrier per chunk.
// This file is included by fdet_conv3x3_x3_tu.hip with X3_MODE defined (one translation unit
// per epilogue mode keeps each kernel's register allocation independent and the build parallel).
// X3_P16 = 1 instantiates the precision16 form instead: one bf16 pass (P16 below).
#include "fdet_conv3x3_x3.h"
#ifndef X3_P16
#define X3_P16 0
#endif

namespace {

// NV consecutive floats; ALIGNED: 16-byte aligned address (VW == 4 geometries), else 4-byte aligned
template <int NV, bool ALIGNED>
__device__ __forceinline__ f32x4 ldv(const float* __restrict__ p) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (ALIGNED && NV == 4) v = *reinterpret_cast<const f32x4*>(p);
  else __builtin_memcpy(&v, p, 4 * NV);
  return v;
}
template <int NV, bool ALIGNED>
__device__ __forceinline__ void stv(float* __restrict__ p, const f32x4& v) {
  if (ALIGNED && NV == 4) *reinterpret_cast<f32x4*>(p) = v;
  else __builtin_memcpy(p, &v, 4 * NV);
}

#ifdef FDET_X3_STAMPS
// diagnostic build only (tools/probe): per-workgroup s_memtime stamps of thread 0, 16 slots each
#define X3_STAMP(i) { __builtin_amdgcn_sched_barrier(0); if (p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 32 + (i)] = ((i) == 14 || (i) == 15) ? (long long)__builtin_amdgcn_s_memrealtime() : (long long)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#else
#define X3_STAMP(i) {}
#endif

template <int CTRL>
__device__ __forceinline__ float dpp_quad(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// 4x4 transpose of 16-byte elements across each quad of lanes: slot k of lane j <-> slot j of lane k
// (slot g = registers 4g..4g+3).  b0/b1 = bits 0/1 of the lane index.
__device__ __forceinline__ void quad_transpose(f32x16& a, bool b0, bool b1) {
#pragma unroll
  for (int k = 0; k < 4; k += 2)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float lo = a[4 * k + i], hi = a[4 * (k + 1) + i];
      const float recv = dpp_quad<0xB1>(b0 ? lo : hi);          // quad_perm [1,0,3,2]
      a[4 * k + i] = b0 ? recv : lo;
      a[4 * (k + 1) + i] = b0 ? hi : recv;
    }
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float lo = a[4 * k + i], hi = a[4 * (k + 2) + i];
      const float recv = dpp_quad<0x4E>(b1 ? lo : hi);          // quad_perm [2,3,0,1]
      a[4 * k + i] = b1 ? recv : lo;
      a[4 * (k + 2) + i] = b1 ? hi : recv;
    }
}

// Epilogue of one tile.  The MFMA leaves acc[n][m][4g+i] = position qwave + 32n + 8g + 4*half + i,
// channel cob*MB + 32m + l31 in lane (l31, half): 16 bytes per lane, but 32 different channels (cache
// lines) per instruction.  A quad transpose turns that into: slot k of lane l31 = channel
// cob*MB + 32m + (l31 & ~3) + k, positions qwave + 32n + 8*(l31&3) + 4*half + i -- the 8 lanes
// {quad} x {half} of one instruction cover 32 consecutive positions (128 B) of ONE channel.
// Memory phases are batched explicitly (all loads of rows [N0,N1), then all stores): a load -> use ->
// store chain per 16 bytes would expose one HBM round trip each.
template <int MT, int NT, int VW, int MODE, int N0, int N1, bool P16>
__device__ __forceinline__ void epilogue_rows(const X3Args& p, f32x16 (&acc)[NT][MT], int v0, int x0, int cw, int cob,
                                              int qwave, int l31, int half) {
  const ConvArgs& a = p.c;
  const float* __restrict__ g_bias = a.bias;
  const float* __restrict__ g_skip = a.skip;
  const float* __restrict__ g_scale = a.scale;
  const float* __restrict__ g_act = a.act;
  float* __restrict__ g_full = a.y_full;
  float* __restrict__ g_out = a.y_out;
  constexpr int MB = MT * 32;
  constexpr bool AL = VW == 4;
  constexpr bool GEN = MODE == EPI_GENERIC;
  const int H1 = a.H + 1, HW = a.H * a.W;
  const int qlimit = a.R * a.WP;
  const bool fwd = GEN ? !a.dgrad : (MODE == EPI_FWD_FULL || MODE == EPI_FWD_BOTH || MODE == EPI_FWD_OUT);
  // stream A: fwd -> skip (needed for y_out), dgrad -> act ;  stream B: dgrad -> add
  const float* __restrict__ sa = fwd ? ((GEN ? (g_out && g_skip) : MODE != EPI_FWD_FULL) ? g_skip : nullptr)
                                     : ((GEN ? g_act != nullptr : MODE == EPI_DGRAD_ACT) ? g_act : nullptr);
  const float* __restrict__ sb = fwd ? nullptr : ((GEN ? g_skip != nullptr : MODE == EPI_DGRAD_ADD) ? g_skip : nullptr);
  const bool use_scale = GEN ? (fwd && g_out && g_scale) : MODE == EPI_FWD_BOTH;
  const bool use_bias = GEN ? (fwd && g_bias) : fwd;
  const bool st_full = GEN ? (g_full != nullptr) : MODE != EPI_FWD_OUT;
  const bool st_out = GEN ? (fwd && g_out) : (MODE == EPI_FWD_BOTH || MODE == EPI_FWD_OUT);
  const int j = l31 & 3, cb = l31 & ~3;
  const bool b0 = j & 1, b1 = j & 2;
  int nv[NT], idx0[NT], img[NT];
#pragma unroll
  for (int n = N0; n < N1; ++n) {
    const int q4 = qwave + n * 32 + 8 * j + 4 * half;
    const int tr = fdiv(q4, p.magic_wp), ox = q4 - tr * a.WP;
    const int v = v0 + tr;
    const int im = fdiv(v, a.magic_h1), oy = v - im * H1 - 1;
    int c = cw - ox;
    c = c > 4 ? 4 : c;
    const bool ok = q4 < qlimit && v < a.VR && oy >= 0 && c > 0;
    nv[n] = ok ? c : 0;
    img[n] = ok ? im : 0;
    idx0[n] = ok ? ((im * a.Cout) * a.H + oy) * a.W + x0 + ox : 0;      // 0: a safe address for the loads
#pragma unroll
    for (int m = 0; m < MT; ++m) quad_transpose(acc[n][m], b0, b1);       // every lane takes part (DPP)
  }
  int co[MT][4];
  float bz[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cob * MB + m * 32 + cb + k;
      co[m][k] = c >= a.Cout ? -1 : c;                    // (fast modes: only the data gradients meet Cout % 32 == 16, the SSD trunk's 32 -> 16)
      bz[m][k] = (use_bias && co[m][k] >= 0) ? g_bias[co[m][k]] : 0.f;
    }
  // ---- loads
  f32x4 ta[N1 - N0][MT][4], tb[GEN ? N1 - N0 : 1][MT][4];
  float sc[N1 - N0][MT][4];
#define X3_LD_ROWS(NV_)                                                                            \
  _Pragma("unroll") for (int m = 0; m < MT; ++m) _Pragma("unroll") for (int k = 0; k < 4; ++k) {   \
    const int c_ = co[m][k] < 0 ? 0 : co[m][k];                                                    \
    if (sa) ta[n - N0][m][k] = ldv<NV_, AL>(sa + idx0[n] + c_ * HW);                               \
    if (sb) (GEN ? tb[n - N0][m][k] : ta[n - N0][m][k]) = ldv<NV_, AL>(sb + idx0[n] + c_ * HW);    \
  }
#pragma unroll
  for (int n = N0; n < N1; ++n) {
    if (VW == 4) { X3_LD_ROWS(4) }                       // straight line: nv is 0 (safe address) or 4
    else if (nv[n] == 4) { X3_LD_ROWS(4) }
    else if (nv[n] == 3) { X3_LD_ROWS(3) }
    else if (nv[n] == 2) { X3_LD_ROWS(2) }
    else if (nv[n] == 1) { X3_LD_ROWS(1) }
    if (use_scale) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) sc[n - N0][m][k] = g_scale[img[n] * a.Cout + (co[m][k] < 0 ? 0 : co[m][k])];
    }
  }
#undef X3_LD_ROWS
  // ---- arithmetic, in place and for every lane (acc <- value for y_full / dx, ta <- value for y_out):
  //      all load results are consumed before the first store is issued
#pragma unroll
  for (int n = N0; n < N1; ++n)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float z = acc[n][m][4 * k + i];
          if (fwd) {
            const float t = z + bz[m][k];
            z = t > 0.f ? t : t * a.slope;
            const float o = (use_scale ? z * sc[n - N0][m][k] : z) + (sa ? ta[n - N0][m][k][i] : 0.f);
            ta[n - N0][m][k][i] = o;
          } else {
            if (sa) z *= (ta[n - N0][m][k][i] > 0.f) ? 1.f : a.slope;
            if (sb) z += (GEN ? tb[n - N0][m][k][i] : ta[n - N0][m][k][i]);
          }
          acc[n][m][4 * k + i] = z;
        }
  // ---- stores
#define X3_ST_ROWS(NV_)                                                                            \
  _Pragma("unroll") for (int m = 0; m < MT; ++m) _Pragma("unroll") for (int k = 0; k < 4; ++k) {   \
    if (co[m][k] < 0) continue;                                                                    \
    const int idx_ = idx0[n] + co[m][k] * HW;                                                      \
    const f32x4 z_ = {acc[n][m][4 * k], acc[n][m][4 * k + 1], acc[n][m][4 * k + 2], acc[n][m][4 * k + 3]}; \
    if (st_full) stv<NV_, AL>(g_full + idx_, st16<P16>(z_));                                       \
    if (st_out) stv<NV_, AL>(g_out + idx_, st16<P16>(ta[n - N0][m][k]));                           \
  }
#pragma unroll
  for (int n = N0; n < N1; ++n) {
    if (nv[n] == 4) { X3_ST_ROWS(4) }
    else if (VW != 4 && nv[n] == 3) { X3_ST_ROWS(3) }
    else if (VW != 4 && nv[n] == 2) { X3_ST_ROWS(2) }
    else if (VW != 4 && nv[n] == 1) { X3_ST_ROWS(1) }
  }
#undef X3_ST_ROWS
}

template <int MT, int NT, int VW, int MODE, bool P16>
__device__ __forceinline__ void epilogue_x3(const X3Args& p, f32x16 (&acc)[NT][MT], int v0, int x0, int cw, int cob,
                                            int qwave, int l31, int half) {
  if (MODE != EPI_GENERIC) {                              // two 32-position row blocks per memory batch
    epilogue_rows<MT, NT, VW, MODE, 0, (NT > 2 ? 2 : NT), P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
    if (NT > 2) epilogue_rows<MT, NT, VW, MODE, (NT > 2 ? 2 : 0), (NT > 2 ? 4 : 1), P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
  } else {                                                // slow path: one 32-position row block at a time
    epilogue_rows<MT, NT, VW, MODE, 0, 1, P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
    if (NT > 1) epilogue_rows<MT, NT, VW, MODE, (NT > 1 ? 1 : 0), (NT > 1 ? 2 : 1), P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
    if (NT > 2) {
      epilogue_rows<MT, NT, VW, MODE, (NT > 2 ? 2 : 0), (NT > 2 ? 3 : 1), P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
      epilogue_rows<MT, NT, VW, MODE, (NT > 2 ? 3 : 0), (NT > 2 ? 4 : 1), P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
    }
  }
}

// NW waves per workgroup (4: one per SIMD, 512 registers; 8: two per SIMD, 256 registers each -- the
// partner wave's VALU / LDS / memory instructions fill the gaps of this wave's MFMA stream)
// P16 (precision16): one bf16 pass -- operands rounded to bf16 (hi only: no lo staging, the panels' lo half is not read),
// one MFMA per (n, m) tile, fp32 accumulation and epilogue, stored values rounded to bf16.
template <int MT, int NT, int VW, bool SEG, int NW, int MODE, bool P16 = false>
__global__ void __launch_bounds__(NW * 64, 1)
k_conv3x3_x3(const X3Args p) {
  constexpr int NTHR = NW * 64;
  constexpr int NBS = nbs_of(NW, NT, VW);
  constexpr int MB = MT * 32;
  constexpr int A_UNITS = 9 * 2 * MB;                 // 16-byte units per weight array per chunk
  constexpr int NAU = P16 ? A_UNITS : 2 * A_UNITS;    // weight units staged per chunk: hi and lo (P16: hi only)
  constexpr int NA = (NAU + NTHR - 1) / NTHR;
  constexpr int NJOBS = NA + NBS * VW + (SEG ? 1 : 0);
  using VT = typename Vec<VW>::T;
  const ConvArgs& a = p.c;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int PT = p.PT, WP = a.WP;
  const int buf_units = 2 * A_UNITS + 4 * PT;         // 16-byte units per buffer
  bf16x8* lds = reinterpret_cast<bf16x8*>(smem);
  // staging writes are branch-free (so that the scheduler can weave them between MFMAs): a write that
  // must not happen lands in this thread's junk unit behind the two buffers
  const int junk = 2 * buf_units + threadIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int H1 = a.H + 1;
  const int HW = a.H * a.W;
  const int G = gridDim.x;
  X3_STAMP(0)
  X3_STAMP(15)
  if (a.stagger > 0) {
    // de-synchronise the workgroups: without it every CU is in its MFMA phase, then every CU in its
    // load / store burst, and HBM and the matrix cores take turns idling chip-wide
    const long long t0 = (long long)__builtin_amdgcn_s_memtime();
    const long long wait = (long long)a.stagger * ((blockIdx.x * 5) & 7) / 8;
    while ((long long)__builtin_amdgcn_s_memtime() - t0 < wait) __builtin_amdgcn_s_sleep(16);
  }

  {  // zero both buffers once: halo / pad slots of the activation arrays are never written
    f32x4* z = reinterpret_cast<f32x4*>(smem);
    for (int t = tid; t < 2 * buf_units + NTHR; t += NTHR) z[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging geometry that does not depend on the tile: slot -> (k-half, tile row, column group)
  int b_tr[NBS], b_col[NBS], b_xo[NBS], b_dst[NBS];
#pragma unroll
  for (int s = 0; s < NBS; ++s) {
    const int it = s * NTHR + tid;
    b_tr[s] = -1; b_col[s] = 0; b_xo[s] = 0; b_dst[s] = 0;
    if (it < 2 * p.items_half) {
      const int h = it >= p.items_half ? 1 : 0;
      const int pp = it - h * p.items_half;
      const int tr = fdiv(pp, p.magic_wv), xg = pp - tr * p.WV;
      b_tr[s] = tr;
      b_col[s] = xg * VW;
      b_xo[s] = 8 * h * HW + xg * VW;
      b_dst[s] = h * PT + tr * WP + 1 + xg * VW;      // unit index inside the hi array pair; lo = +2*PT
    }
  }
  // halo columns of a column segment (SEG): thread -> (k-half, side, tile row)
  int h_tr = -1, h_side = 0, h_xo = 0, h_dst = 0;
  if (SEG && tid < 4 * (a.R + 2)) {
    const int h = tid & 1;
    h_side = (tid >> 1) & 1;
    h_tr = tid >> 2;
    h_xo = 8 * h * HW;
    h_dst = h * PT + h_tr * WP;
  }

  const int a_chunk_units = 9 * 2 * a.CoP;            // units per chunk per array in HBM
  const int nch = a.Cin / CK16;

  // per-tile state: current tile (MFMA + epilogue) and next stage (loads)
  int v0 = 0, x0 = 0, cw = a.W, cob = 0;
  int n_cob = 0, n_cw = a.W;                           // next stage's tile
  int b_src[NBS];
  bool b_ok[NBS];
  int h_src = 0;
  bool h_ok = false;

  // geometry of tile T for the staging loads
#define X3_TILE_GEO(T, V0, X0, CWC, COB)                                                           \
  {                                                                                                \
    const int T_ = (T);                                                                            \
    COB = T_ % p.ncob;                                                                             \
    const int r_ = T_ / p.ncob;                                                                    \
    const int seg_ = SEG ? r_ % p.NSEG : 0;                                                        \
    const int band_ = SEG ? r_ / p.NSEG : r_;                                                      \
    V0 = band_ * a.R;                                                                              \
    X0 = seg_ * p.CW;                                                                              \
    CWC = min(p.CW, a.W - X0);                                                                     \
  }
#define X3_STAGE_GEO(V0, X0, CWC)                                                                  \
  {                                                                                                \
    _Pragma("unroll") for (int s_ = 0; s_ < NBS; ++s_) {                                           \
      const int v_ = (V0) - 1 + b_tr[s_];                                                          \
      const int n_ = fdiv(max(v_, 0), a.magic_h1), yy_ = v_ - n_ * H1 - 1;                         \
      b_ok[s_] = b_tr[s_] >= 0 && v_ >= 0 && v_ < a.VR && yy_ >= 0 && b_col[s_] < (CWC);          \
      b_src[s_] = b_xo[s_] + (b_ok[s_] ? ((n_ * a.Cin) * a.H + yy_) * a.W + (X0) : 0);            \
    }                                                                                              \
    if (SEG) {                                                                                     \
      const int v_ = (V0) - 1 + h_tr;                                                              \
      const int n_ = fdiv(max(v_, 0), a.magic_h1), yy_ = v_ - n_ * H1 - 1;                         \
      const int col_ = h_side ? (X0) + (CWC) : (X0) - 1;                                           \
      h_ok = h_tr >= 0 && v_ >= 0 && v_ < a.VR && yy_ >= 0 && col_ >= 0 && col_ < a.W;            \
      h_src = h_xo + (h_ok ? ((n_ * a.Cin) * a.H + yy_) * a.W + col_ : 0);                         \
    }                                                                                              \
  }

  bf16x8 pa[NA];
  VT pb[NBS][8];
  float ph[8];
#define X3_ISSUE_LOADS(C16, COB)                                                                   \
  {                                                                                                \
    _Pragma("unroll") for (int s_ = 0; s_ < NA; ++s_) {                                            \
      const int u_ = min(tid + s_ * NTHR, NAU - 1);                                                \
      const int lo_ = u_ >= A_UNITS ? 1 : 0;                                                       \
      const int r_ = u_ - lo_ * A_UNITS;                                                           \
      const int th_ = r_ / MB, co_ = r_ - th_ * MB;                                                \
      const bf16x8* src_ = (lo_ ? p.a_lo : p.a_hi) + (size_t)(C16) * a_chunk_units + th_ * a.CoP + (COB) * MB + co_; \
      pa[s_] = *src_;                                                                              \
    }                                                                                              \
    const float* xs_ = a.x + (size_t)(C16) * CK16 * HW;                                            \
    _Pragma("unroll") for (int s_ = 0; s_ < NBS; ++s_) {                                           \
      const float* q_ = xs_ + b_src[s_];                                                           \
      _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) pb[s_][j_] = *reinterpret_cast<const VT*>(q_ + j_ * HW); \
    }                                                                                              \
    if (SEG) {                                                                                     \
      const float* q_ = xs_ + h_src;                                                               \
      _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) ph[j_] = q_[j_ * HW];                       \
    }                                                                                              \
  }
  // staging job J of the chunk held in pa/pb/ph -> LDS buffer at unit offset NB (weights: copy;
  // activations: split).  LIVE = false sends everything to the junk unit.
#define X3_JOB(J, NB, LIVE)                                                                        \
  {                                                                                                \
    if ((J) < NA) {                                                                                \
      const int u_ = tid + (J) * NTHR;                                                             \
      lds[((LIVE) && u_ < NAU) ? (NB) + u_ : junk] = pa[(J) < NA ? (J) : 0];                       \
    } else if ((J) < NA + NBS * VW) {                                                              \
      const int s_ = ((J) - NA) / VW < NBS ? ((J) - NA) / VW : 0, i_ = ((J) - NA) % VW;            \
      const bool w_ = (LIVE) && b_tr[s_] >= 0 && b_col[s_] + i_ < n_cw;                            \
      float f_[8];                                                                                 \
      _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) f_[j_] = b_ok[s_] ? vget<VW>(pb[s_][j_], i_) : 0.f; \
      bf16x8 hi_, lo_;                                                                             \
      if (P16) { _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) hi_[j_] = (__bf16)f_[j_]; }      \
      else split8(f_, hi_, lo_);                                                                   \
      const int d_ = (NB) + 2 * A_UNITS + b_dst[s_] + i_;                                          \
      lds[w_ ? d_ : junk] = hi_;                                                                   \
      if (!P16) lds[w_ ? d_ + 2 * PT : junk] = lo_;                                                \
    } else if (SEG) {                                                                              \
      const bool w_ = (LIVE) && h_tr >= 0;                                                         \
      float f_[8];                                                                                 \
      _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) f_[j_] = h_ok ? ph[j_] : 0.f;               \
      bf16x8 hi_, lo_;                                                                             \
      if (P16) { _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) hi_[j_] = (__bf16)f_[j_]; }      \
      else split8(f_, hi_, lo_);                                                                   \
      const int d_ = (NB) + 2 * A_UNITS + h_dst + (h_side ? n_cw + 1 : 0);                         \
      lds[w_ ? d_ : junk] = hi_;                                                                   \
      if (!P16) lds[w_ ? d_ + 2 * PT : junk] = lo_;                                                \
    }                                                                                              \
  }

  f32x16 acc[NT][MT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][m][r] = 0.f;

  int tapoff[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) tapoff[t] = (t / 3) * WP + (t % 3);

  const int qwave = wid * NT * 32;
  const int w_off = half * MB + l31;                           // + tap*2*MB + m*32 ; lo: + A_UNITS
  const int x_off = 2 * A_UNITS + half * PT + qwave + l31;     // + tapoff + n*32   ; lo: + 2*PT

  int tile = blockIdx.x;
  int n_v0, n_x0;
  X3_TILE_GEO(tile, n_v0, n_x0, n_cw, n_cob)
  X3_STAGE_GEO(n_v0, n_x0, n_cw)
  X3_ISSUE_LOADS(0, n_cob)
  __syncthreads();                       // zero fill complete
#pragma unroll
  for (int j = 0; j < NJOBS; ++j) X3_JOB(j, 0, true)
  __syncthreads();
  X3_STAMP(1)

  int stage = 0;
  int tcount = 0;
  while (tile < p.ntiles) {
    v0 = n_v0; x0 = n_x0; cw = n_cw; cob = n_cob;
    for (int c = 0; c < nch; ++c, ++stage) {
      const bf16x8* buf = lds + (stage & 1) * buf_units;
      const int nb_off = ((stage & 1) ^ 1) * buf_units;
      // ---- next stage: this tile's next chunk, or the first chunk of the workgroup's next tile
      bool has_next = true;
      int nc = c + 1;
      if (nc == nch) {
        nc = 0;
        const int nt = tile + G;
        has_next = nt < p.ntiles;
        if (has_next) {
          X3_TILE_GEO(nt, n_v0, n_x0, n_cw, n_cob)
          X3_STAGE_GEO(n_v0, n_x0, n_cw)
        }
      }
      if (tcount == 1 && c == 1) X3_STAMP(16)
      if (has_next) X3_ISSUE_LOADS(nc, n_cob)
      if (tcount == 1 && c == 1) X3_STAMP(17)

      const bf16x8* Ww = buf + w_off;
      const bf16x8* Xw = buf + x_off;
      // fragments of tap t+1 are fetched before the MFMAs of tap t
      bf16x8 wh[2][MT], wl[2][MT], xh[2][NT], xl[2][NT];
#pragma unroll
      for (int m = 0; m < MT; ++m) { wh[0][m] = Ww[m * 32]; if (!P16) wl[0][m] = Ww[A_UNITS + m * 32]; }
#pragma unroll
      for (int n = 0; n < NT; ++n) { xh[0][n] = Xw[tapoff[0] + n * 32]; if (!P16) xl[0][n] = Xw[2 * PT + tapoff[0] + n * 32]; }
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        if (t + 1 < 9) {
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            wh[nxt][m] = Ww[(t + 1) * 2 * MB + m * 32];
            if (!P16) wl[nxt][m] = Ww[A_UNITS + (t + 1) * 2 * MB + m * 32];
          }
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            xh[nxt][n] = Xw[tapoff[t + 1] + n * 32];
            if (!P16) xl[nxt][n] = Xw[2 * PT + tapoff[t + 1] + n * 32];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t >= TW0) {
          // staging jobs of the next stage share this tap's MFMA shadow
#pragma unroll
          for (int j = 0; j < NJOBS; ++j)
            if (TW0 + (j * (9 - TW0)) / NJOBS == t) X3_JOB(j, nb_off, has_next)
        }
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            if (!P16) {
              acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[cur][n], wl[cur][m], acc[n][m], 0, 0, 0);
              acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[cur][n], wh[cur][m], acc[n][m], 0, 0, 0);
            }
            acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[cur][n], wh[cur][m], acc[n][m], 0, 0, 0);
          }
        if (t >= TW0) {
          // weave: per MFMA a few VALU (split) and now and then one LDS write
#pragma unroll
          for (int i = 0; i < (P16 ? 1 : 3) * MT * NT; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            if ((i & 1) == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (tcount == 1 && c == 1 && (t == 2 || t == 5 || t == 8)) X3_STAMP(18 + t / 3)
      }
      __syncthreads();
      if (tcount == 1 && c == 1) X3_STAMP(21)
      if (tcount == 0 && c < 4) X3_STAMP(2 + c)
    }
    if (tcount == 1) X3_STAMP(7)

    // ---- epilogue of this tile
    epilogue_x3<MT, NT, VW, MODE, P16>(p, acc, v0, x0, cw, cob, qwave, l31, half);
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][m][r] = 0.f;
    if (tcount == 0) X3_STAMP(6)
    if (tcount == 1) X3_STAMP(8)
    tile += G;
    ++tcount;
  }
#ifdef FDET_X3_STAMPS
  X3_STAMP(11)
  __builtin_amdgcn_s_waitcnt(0);         // stores issued AND acknowledged
  X3_STAMP(12)
  X3_STAMP(14)
  if (p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 32 + 13] = tcount;
#endif
}


template <int MT, int NT, int VW, bool SEG, int NW>
int launch_x3(const X3Args& p, size_t lds, int grid, hipStream_t st) {
  (void)hipFuncSetAttribute((const void*)k_conv3x3_x3<MT, NT, VW, SEG, NW, X3_MODE, X3_P16 != 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((k_conv3x3_x3<MT, NT, VW, SEG, NW, X3_MODE, X3_P16 != 0>), dim3(grid), dim3(NW * 64), lds, st, p);
  return check_launch(X3_P16 ? "fdet_conv3x3_bf16" : "fdet_conv3x3_bf16x3");
}

}  // namespace

#define X3_CAT2(a, b) a##b
#define X3_CAT(a, b) X3_CAT2(a, b)
#if X3_P16
#define X3_LAUNCH_NAME X3_CAT(X3_CAT(fdet_x3_launch_m, X3_MODE_ID), _bf16)
#else
#define X3_LAUNCH_NAME X3_CAT(fdet_x3_launch_m, X3_MODE_ID)
#endif
int X3_LAUNCH_NAME(const X3Args& p, int MT, int NW, int NT, int VW, bool seg, size_t lds, int grid, hipStream_t st) {
#define X3_CASE(M_, W_, N_, V_) \
  if (MT == M_ && NW == W_ && NT == N_ && VW == V_) return seg ? launch_x3<M_, N_, V_, true, W_>(p, lds, grid, st) : launch_x3<M_, N_, V_, false, W_>(p, lds, grid, st);
#define X3_CASE_NOSEG(M_, W_, N_, V_) \
  if (MT == M_ && NW == W_ && NT == N_ && VW == V_) return launch_x3<M_, N_, V_, false, W_>(p, lds, grid, st);
#define X3_CASES(M_, W_, N_) X3_CASE(M_, W_, N_, 4) X3_CASE_NOSEG(M_, W_, N_, 2) X3_CASE_NOSEG(M_, W_, N_, 1)
  X3_CONFIGS
#undef X3_CASES
#undef X3_CASE
#undef X3_CASE_NOSEG
  return fail(FDET_EINVAL, "conv3x3_bf16x3: internal: no kernel for tile <%d,%d,%d,%d>", MT, NW, NT, VW);
}
