// Offline refinement of the tracker's output over whole sequences: fdet_track_refine back-fills a track
// before its first detection, interpolates the gaps between detections, stitches the fragments of one face into one id
// and drops short chains.  The rule, step by step, is stated with the declaration in include/fdet.h;
// tests/track_refine_cpu_ref.py restates it on Python ints, and the two agree byte for byte.
//
// One workgroup of 256 threads per sequence, five passes, every table indexed by id - (lowest id of the sequence) in LDS
// (7 tables x 4096 words = 112 KB):
//   1. validate: counts, emitted ids, the span of the ids (LDS atomicMin / atomicMax: order-independent);
//   2. anchors, frame by frame: the emitted rows stamp their ids, then the emitted rows with misses == 0 and the rows of
//      det_ids whose id carries no stamp are compacted in row order (compact_slot of fdet_boxes.h) into the frame's 128
//      anchor records in the workspace.  Each record is linked behind its track's previous one, so a track, and after pass 3
//      a chain, is a list of records in time order; first / last record and the count of every track stay in LDS;
//   3. stitch, track by track in ascending id: the threads share the chains found so far, each keeps its best candidate
//      (exact cross-multiplied comparison, lower chain id on a tie), a wave and a block reduction pick the chain; joining is
//      linking the two lists;
//   4. length filter: a short chain's members lose their chain;
//   5. emission, frame by frame, with the previous and the next anchor record of every chain in LDS (the forward sweep
//      keeps both: a record knows its successor).  The chains of a frame set one bit each in two 4096-bit masks (kinds
//      0..2, kind 3) with atomicOr; a coasted row is chosen per chain with an atomicMax that its winner resets.  A prefix
//      sum over the masks' 64 words gives every row its place in ascending chain id, and each thread writes its rows.
// The only floating-point operations are those of step 1 of fdet_track_update on an anchor's row and the one double
// multiply of the stitching threshold.  Built with -ffp-contract=off like every file here.
#include "fdet_boxes.h"
#include <climits>
#include <cstdint>

using namespace fdet;

namespace {

constexpr int NS = FDET_TRACK_SLOTS, NR = FDET_TRACK_REFINE_ROWS, NI = FDET_TRACK_REFINE_MAX_IDS, NTHR = BOX_THREADS;
constexpr int MAX_T = 1 << 24;                 // a record index t * 128 + slot stays an int
static_assert(NTHR == NR && NTHR == 2 * NS && NI % 64 == 0 && NI / 64 == WAVE, "one thread per output row, one lane per mask word");

// an anchor: the track it belongs to (id - lo), its box, its score (bits), the record that follows it in its chain (-1 =
// none) and the row it came from (p < 128: emitted row p; 128 + j: row j of det_rows)
struct Rec {
  int idx, x1, y1, x2, y2, score, next, src;
};
static_assert(sizeof(Rec) == 32, "record layout");

constexpr size_t LDS_INTS = 7 * (size_t)NI + 2 * 2 * 64 + 2 * 64 + 8 + 8 + 4 * 4;
constexpr size_t LDS_BYTES = LDS_INTS * 4;

// step 1 of fdet_track_update on one row: its corners, or false
__device__ __forceinline__ bool corners(const float* v, int& X1, int& Y1, int& X2, int& Y2) {
  const float sc = v[0], x = v[1], y = v[2], w = v[3], h = v[4];
  const float lim = (float)FDET_TRACK_MAX_COORD;
  const float fx1 = rintf(x), fy1 = rintf(y), fx2 = rintf(x + w), fy2 = rintf(y + h);
  bool ok = fabsf(sc) <= 3.402823466e38f && fabsf(w) <= 3.402823466e38f && fabsf(h) <= 3.402823466e38f && fabsf(fx1) <= lim &&
            fabsf(fy1) <= lim && fabsf(fx2) <= lim && fabsf(fy2) <= lim;
  if (!ok) return false;
  X1 = (int)fx1; Y1 = (int)fy1; X2 = (int)fx2; Y2 = (int)fy2;
  return X2 - X1 >= 1 && Y2 - Y1 >= 1;
}

// a stitching candidate; inter == 0 means none
struct Cand {
  unsigned long long inter, uni;
  int chain;
};

// a is the better candidate: larger IoU exactly, then the lower chain
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
  const unsigned long long l = a.inter * b.uni, r = b.inter * a.uni;      // sides <= 2^15: inter <= 2^30, uni <= 2^31
  return l > r || (l == r && a.chain < b.chain);
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {      // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ __forceinline__ void put_row(float* __restrict__ out_rows, int32_t* __restrict__ out_ids, int32_t* __restrict__ out_misses,
                                        int32_t* __restrict__ out_kind, size_t t, int rank, float s, float x, float y, float w, float h,
                                        int id, int misses, int kind) {
  if (rank >= NR) return;
  const size_t o = t * NR + rank;
  out_rows[o * 5 + 0] = s; out_rows[o * 5 + 1] = x; out_rows[o * 5 + 2] = y; out_rows[o * 5 + 3] = w; out_rows[o * 5 + 4] = h;
  out_ids[o] = id;
  out_misses[o] = misses;
  out_kind[o] = kind;
}

__global__ void __launch_bounds__(NTHR)
k_track_refine(const float* __restrict__ det_rows, const int32_t* __restrict__ det_ids, int K, const float* __restrict__ trk_rows,
               const int32_t* __restrict__ trk_ids, const int32_t* __restrict__ trk_misses, const int32_t* __restrict__ trk_counts,
               const int32_t* __restrict__ seq_offset, int T, int lookback, int grow256, int stitch_gap, double stitch_iou,
               int min_length, float* __restrict__ out_rows, int32_t* __restrict__ out_ids, int32_t* __restrict__ out_misses,
               int32_t* __restrict__ out_kind, int32_t* __restrict__ out_counts, Rec* __restrict__ recs, int32_t* __restrict__ nrec,
               unsigned long long* __restrict__ rejected) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  int* const firstRec = smem;                  // track -> its first anchor record, -1 = none
  int* const lastRec = smem + NI;              // track, later chain -> its last anchor record
  int* const cnt = smem + 2 * NI;              // track, later chain -> anchors; -1 = dropped by the length filter
  int* const chainOf = smem + 3 * NI;          // track -> chain (the lowest id - lo of the chain), -1 = dropped
  int* const curRec = smem + 4 * NI;           // pass 5: chain -> its last anchor before this frame; pass 2: the stamps
  int* const nxtRec = smem + 5 * NI;           // pass 5: chain -> its first anchor at or after this frame
  int* const aux = smem + 6 * NI;              // pass 3: the chains so far; pass 5: chain -> its best coasted row + 1
  unsigned long long* const m012 = reinterpret_cast<unsigned long long*>(smem + 7 * NI);      // chains with a row of kind 0..2
  unsigned long long* const mB = m012 + 64;    // chains with a back-filled row
  int* const pre012 = reinterpret_cast<int*>(mB + 64);
  int* const preB = pre012 + 64;
  int* const ctl = preB + 64;                  // compact_slot's five words
  int* const misc = ctl + 8;                   // lo, hi, rows of kind 0..2, rows of kind 3
  int* const red = misc + 8;                   // per wave: a candidate's inter, uni (as ints: both < 2^32) and chain

  const int seq = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int t0 = seq_offset[seq], t1 = seq_offset[seq + 1];
  if (t0 < 0 || t1 < t0 || t1 > T) {           // the host validated its copy; no frame can be addressed from these
    if (tid == 0) atomicAdd(rejected, 1ull);
    return;
  }
  const int n = t1 - t0;
  if (n == 0) return;

  // ---- pass 1: validation and the span of the ids ---------------------------------------------------------------------
  if (tid == 0) { misc[0] = INT_MAX; misc[1] = 0; }
  __syncthreads();
  bool bad = false;
  for (int t = t0 + tid; t < t1; t += NTHR) {
    const int c = trk_counts[t];
    if (c < 0 || c > NS) bad = true;
  }
  bad = __syncthreads_or(bad);
  int lo = INT_MAX, hi = 0;
  if (!bad) {
    for (size_t i = tid; i < (size_t)n * NS; i += NTHR) {
      const size_t t = (size_t)t0 + i / NS;
      if ((int)(i % NS) < trk_counts[t]) {
        const int id = trk_ids[(size_t)t0 * NS + i];
        if (id <= 0) bad = true;
        else { lo = min(lo, id); hi = max(hi, id); }
      }
    }
    for (size_t i = tid; i < (size_t)n * K; i += NTHR) {
      const int id = det_ids[(size_t)t0 * K + i];
      if (id > 0) { lo = min(lo, id); hi = max(hi, id); }
    }
    atomicMin(&misc[0], lo);
    atomicMax(&misc[1], hi);
    bad = __syncthreads_or(bad);
  }
  lo = misc[0]; hi = misc[1];
  const int span = hi >= lo ? hi - lo + 1 : 0;           // lo >= 1: no overflow
  if (span > NI) bad = true;

  // ---- pass 2: the anchors of every frame, linked per track -----------------------------------------------------------
  if (!bad) {
    for (int i = tid; i < span; i += NTHR) { firstRec[i] = -1; lastRec[i] = -1; cnt[i] = 0; chainOf[i] = i; curRec[i] = 0; }
    __syncthreads();
    int* const stamp = curRec;
    for (int t = t0; t < t1; ++t) {
      const int c = trk_counts[t], mark = t - t0 + 1;
      int myIdx = -1, myMiss = 1;
      if (tid < c) {
        myIdx = trk_ids[(size_t)t * NS + tid] - lo;
        myMiss = trk_misses[(size_t)t * NS + tid];
        if ((unsigned)myIdx < (unsigned)span) stamp[myIdx] = mark; else myIdx = -1;
      }
      if (tid == 0) ctl[0] = 0;
      __syncthreads();
      for (int j0 = -NTHR; j0 < K; j0 += NTHR) {         // the first chunk is the emitted rows, the others are det_rows
        const int j = j0 + tid;
        bool hit = false;
        int idx = -1, X1 = 0, Y1 = 0, X2 = 0, Y2 = 0, src = 0;
        float sc = 0.f;
        const float* row = nullptr;
        if (j0 < 0) {
          if (myIdx >= 0 && myMiss == 0) { idx = myIdx; src = tid; row = trk_rows + ((size_t)t * NS + tid) * 5; }
        } else if (j < K) {
          const int id = det_ids[(size_t)t * K + j];
          if (id > 0 && (unsigned)(id - lo) < (unsigned)span && stamp[id - lo] != mark) {
            idx = id - lo; src = NS + j; row = det_rows + ((size_t)t * K + j) * 5;
          }
        }
        if (row) {
          float v[5];
#pragma unroll
          for (int e = 0; e < 5; ++e) v[e] = row[e];
          sc = v[0];
          hit = corners(v, X1, Y1, X2, Y2);
          if (!hit) bad = true;                          // an anchor's row must be a valid box
        }
        const int slot = compact_slot(hit, ctl);
        if (hit && slot < NS) {
          const int r = t * NS + slot;
          recs[r] = Rec{idx, X1, Y1, X2, Y2, __float_as_int(sc), -1, src};
          const int prev = lastRec[idx];                 // one anchor per track and frame: nobody else touches these words
          if (prev >= 0) recs[prev].next = r; else firstRec[idx] = r;
          lastRec[idx] = r;
          atomicAdd(&cnt[idx], 1);
        }
      }
      __syncthreads();
      const int total = ctl[0];                          // uniform
      if (total > NS) bad = true;
      if (tid == 0) nrec[t] = min(total, NS);
      __syncthreads();                                   // ctl[0] was read before it is reset; the records are visible
    }
    bad = __syncthreads_or(bad);
  }

  if (bad) {                                   // the whole sequence: outputs zeroed
    const size_t m = (size_t)n * NR, b = (size_t)t0 * NR;
    for (size_t i = tid; i < m * 5; i += NTHR) out_rows[b * 5 + i] = 0.f;
    for (size_t i = tid; i < m; i += NTHR) { out_ids[b + i] = 0; out_misses[b + i] = 0; out_kind[b + i] = 0; }
    for (size_t i = tid; i < (size_t)n; i += NTHR) out_counts[t0 + i] = 0;
    if (tid == 0) atomicAdd(rejected, 1ull);
    return;
  }

  // ---- pass 3: stitch, tracks in ascending id -------------------------------------------------------------------------
  if (stitch_gap >= 0) {
    int* const list = aux;
    int nCh = 0;                               // uniform
    for (int idx = 0; idx < span; ++idx) {
      const int fr = firstRec[idx];
      if (fr < 0) continue;                    // uniform
      const int f = fr / NS;
      const int f0 = recs[fr].x1, f1 = recs[fr].y1, f2 = recs[fr].x2, f3 = recs[fr].y2;
      const unsigned long long areaF = (unsigned long long)(f2 - f0) * (unsigned long long)(f3 - f1);
      Cand best{0ull, 1ull, INT_MAX};
      for (int k = tid; k < nCh; k += NTHR) {
        const int h = list[k], lr = lastRec[h], L = lr / NS;
        if (!(L < f && f - L - 1 <= stitch_gap)) continue;
        const int a0 = recs[lr].x1, a1 = recs[lr].y1, a2 = recs[lr].x2, a3 = recs[lr].y2;
        const int iw = min(a2, f2) - max(a0, f0), ih = min(a3, f3) - max(a1, f1);
        if (iw <= 0 || ih <= 0) continue;
        const unsigned long long inter = (unsigned long long)iw * (unsigned long long)ih;
        const unsigned long long uni = (unsigned long long)(a2 - a0) * (unsigned long long)(a3 - a1) + areaF - inter;
        if (!((double)inter > stitch_iou * (double)uni)) continue;
        const Cand c{inter, uni, h};
        if (better(c, best)) best = c;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        Cand o;
        o.inter = (unsigned)__shfl_xor((int)(unsigned)best.inter, off, 64);
        o.uni = (unsigned)__shfl_xor((int)(unsigned)best.uni, off, 64);
        o.chain = __shfl_xor(best.chain, off, 64);
        if (better(o, best)) best = o;
      }
      if (lane == 0) { red[wid * 3] = (int)(unsigned)best.inter; red[wid * 3 + 1] = (int)(unsigned)best.uni; red[wid * 3 + 2] = best.chain; }
      __syncthreads();
      best = Cand{(unsigned)red[0], (unsigned)red[1], red[2]};
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const Cand o{(unsigned)red[w * 3], (unsigned)red[w * 3 + 1], red[w * 3 + 2]};
        if (better(o, best)) best = o;
      }
      if (best.inter > 0) {                    // uniform
        if (tid == 0) {
          const int h = best.chain;
          chainOf[idx] = h;
          recs[lastRec[h]].next = fr;
          lastRec[h] = lastRec[idx];
          cnt[h] += cnt[idx];
        }
      } else {
        if (tid == 0) list[nCh] = idx;
        nCh += 1;
      }
      __syncthreads();
    }
  }

  // ---- pass 4: the length filter, and the tables of the sweep --------------------------------------------------------
  __syncthreads();
  for (int i = tid; i < span; i += NTHR)
    if (chainOf[i] == i && firstRec[i] >= 0 && cnt[i] < min_length) cnt[i] = -1;
  __syncthreads();
  for (int i = tid; i < span; i += NTHR) {     // a member reads its own word and its chain's count only
    const int c = chainOf[i];
    if (cnt[c] == -1) chainOf[i] = -1;
  }
  __syncthreads();
  for (int i = tid; i < span; i += NTHR) {
    nxtRec[i] = (chainOf[i] == i) ? firstRec[i] : -1;    // an id without anchors is its own chain with nothing to come
    curRec[i] = -1;
    aux[i] = 0;
  }
  if (tid < 64) { m012[tid] = 0ull; mB[tid] = 0ull; }
  __syncthreads();
  int* const coast = aux;

  // ---- pass 5: emission, frame by frame --------------------------------------------------------------------------------
  for (int t = t0; t < t1; ++t) {
    const int c = trk_counts[t], na = nrec[t];
    // the frame's anchors: thread s owns record s
    int aC = -1;
    Rec ar{0, 0, 0, 0, 0, 0, -1, 0};
    if (tid < na) {
      ar = recs[(size_t)t * NS + tid];
      aC = chainOf[ar.idx];
      if (aC >= 0) atomicOr(&m012[aC >> 6], 1ull << (aC & 63));
    }
    // the frame's coasted rows: thread 128 + p owns emitted row p; the member track with the highest id wins its chain
    int cC = -1, cPack = 0, cMiss = 0;
    const int p = tid - NS;
    if (p >= 0 && p < c) {
      cMiss = trk_misses[(size_t)t * NS + p];
      const int idx = trk_ids[(size_t)t * NS + p] - lo;
      if (cMiss != 0 && (unsigned)idx < (unsigned)span) {
        cC = chainOf[idx];
        if (cC >= 0) { cPack = ((idx << 7) | p) + 1; atomicMax(&coast[cC], cPack); }
      }
    }
    // chains inside a gap or before their first anchor
    for (int i = tid; i < span; i += NTHR) {
      const int nr = nxtRec[i];
      if (nr < 0) continue;
      const int fn = nr / NS;
      if (fn <= t) continue;
      if (curRec[i] >= 0) atomicOr(&m012[i >> 6], 1ull << (i & 63));
      else if (fn - t <= lookback) atomicOr(&mB[i >> 6], 1ull << (i & 63));
    }
    __syncthreads();
    // a coasted row stands where its chain has neither an anchor nor an interpolated row, and before a back-filled one
    const bool cMax = cC >= 0 && coast[cC] == cPack;
    bool cWin = false;
    if (cMax && !((m012[cC >> 6] >> (cC & 63)) & 1ull)) {              // only this thread can set that bit now
      cWin = true;
      atomicOr(&m012[cC >> 6], 1ull << (cC & 63));
      atomicAnd(&mB[cC >> 6], ~(1ull << (cC & 63)));
    }
    __syncthreads();
    if (wid == 0) {                            // exclusive prefix sums over the masks' words
      const int a = __popcll(m012[lane]), b = __popcll(mB[lane]);
      int sa = a, sb = b;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int ua = __shfl_up(sa, off, 64), ub = __shfl_up(sb, off, 64);
        if (lane >= off) { sa += ua; sb += ub; }
      }
      pre012[lane] = sa - a;
      preB[lane] = sb - b;
      if (lane == 63) { misc[2] = sa; misc[3] = sb; }
    }
    __syncthreads();
    const int n012 = misc[2], nB = misc[3], total = n012 + nB, nOut = min(total, NR);
    if (aC >= 0) {
      const int rank = pre012[aC >> 6] + __popcll(m012[aC >> 6] & ((1ull << (aC & 63)) - 1ull));
      const float* row = ar.src < NS ? trk_rows + ((size_t)t * NS + ar.src) * 5 : det_rows + ((size_t)t * K + (ar.src - NS)) * 5;
      put_row(out_rows, out_ids, out_misses, out_kind, (size_t)t, rank, row[0], row[1], row[2], row[3], row[4], lo + aC, 0, 0);
    }
    if (cWin) {
      const int rank = pre012[cC >> 6] + __popcll(m012[cC >> 6] & ((1ull << (cC & 63)) - 1ull));
      const float* row = trk_rows + ((size_t)t * NS + p) * 5;
      put_row(out_rows, out_ids, out_misses, out_kind, (size_t)t, rank, row[0], row[1], row[2], row[3], row[4], lo + cC, cMiss, 1);
    }
    if (cMax) coast[cC] = 0;                   // every comparison with it came before the last two barriers
    for (int i = tid; i < span; i += NTHR) {
      const int nr = nxtRec[i];
      if (nr < 0) continue;
      const int fn = nr / NS;
      if (fn <= t) continue;
      const int cr = curRec[i];
      const unsigned long long bit = 1ull << (i & 63);
      if (cr >= 0) {                           // step 4
        const int a = cr / NS;
        const Rec A = recs[cr], B = recs[nr];
        const long long d = fn - a, k = t - a;
        const int x1 = A.x1 + (int)floor_div(2ll * (B.x1 - A.x1) * k + d, 2 * d), y1 = A.y1 + (int)floor_div(2ll * (B.y1 - A.y1) * k + d, 2 * d);
        const int x2 = A.x2 + (int)floor_div(2ll * (B.x2 - A.x2) * k + d, 2 * d), y2 = A.y2 + (int)floor_div(2ll * (B.y2 - A.y2) * k + d, 2 * d);
        const int rank = pre012[i >> 6] + __popcll(m012[i >> 6] & (bit - 1ull));
        put_row(out_rows, out_ids, out_misses, out_kind, (size_t)t, rank, __int_as_float(A.score), (float)x1, (float)y1,
                (float)(x2 - x1), (float)(y2 - y1), lo + i, (int)k, 2);
      } else if (mB[i >> 6] & bit) {           // step 5
        const Rec F = recs[nr];
        const long long gm = (long long)grow256 * (fn - t);
        const int gx = (int)min((gm * (F.x2 - F.x1) + 256) >> 9, (long long)FDET_TRACK_MAX_COORD);
        const int gy = (int)min((gm * (F.y2 - F.y1) + 256) >> 9, (long long)FDET_TRACK_MAX_COORD);
        const int rank = n012 + preB[i >> 6] + __popcll(mB[i >> 6] & (bit - 1ull));
        put_row(out_rows, out_ids, out_misses, out_kind, (size_t)t, rank, __int_as_float(F.score), (float)(F.x1 - gx),
                (float)(F.y1 - gy), (float)(F.x2 - F.x1 + 2 * gx), (float)(F.y2 - F.y1 + 2 * gy), lo + i, fn - t, 3);
      }
    }
    if (tid >= nOut) {                         // one thread per row past the count
      const size_t o = (size_t)t * NR + tid;
#pragma unroll
      for (int e = 0; e < 5; ++e) out_rows[o * 5 + e] = 0.f;
      out_ids[o] = 0; out_misses[o] = 0; out_kind[o] = 0;
    }
    if (tid == 0) {
      out_counts[t] = nOut;
      if (total > NR) atomicAdd(rejected + 1, (unsigned long long)(total - NR));
    }
    __syncthreads();
    if (aC >= 0) { curRec[aC] = t * NS + tid; nxtRec[aC] = ar.next; }
    if (tid < 64) { m012[tid] = 0ull; mB[tid] = 0ull; }
    __syncthreads();
  }
}

}  // namespace

extern "C" size_t fdet_track_refine_ws_bytes(int n_seq, int T) {
  if (n_seq < 1 || T < 1 || T > MAX_T) return 0;
  return (size_t)T * ((size_t)NS * sizeof(Rec) + sizeof(int32_t));
}

extern "C" int fdet_track_refine(const float* det_rows, const int32_t* det_ids, int K, const float* trk_rows, const int32_t* trk_ids,
                                 const int32_t* trk_misses, const int32_t* trk_counts, const int32_t* seq_offset,
                                 const int32_t* h_seq_offset, int n_seq, int T, int lookback, int grow256, int stitch_gap,
                                 double stitch_iou, int min_length, float* out_rows, int32_t* out_ids, int32_t* out_misses,
                                 int32_t* out_kind, int32_t* out_counts, void* ws, size_t ws_bytes, uint64_t* rejected, void* stream) {
  const char* what = "fdet_track_refine";
  FDET_REQUIRE(n_seq >= 1 && T >= 0 && T <= MAX_T && K >= 0, "%s: bad sizes n_seq=%d T=%d K=%d", what, n_seq, T, K);
  FDET_REQUIRE(lookback >= 0 && lookback <= 1024, "%s: lookback=%d must be in 0..1024", what, lookback);
  FDET_REQUIRE(grow256 >= 0 && grow256 <= 256, "%s: grow256=%d must be in 0..256", what, grow256);
  FDET_REQUIRE(stitch_gap <= 65535, "%s: stitch_gap=%d must be at most 65535 (negative: no stitching)", what, stitch_gap);
  FDET_REQUIRE(stitch_iou >= 0.0 && stitch_iou < 1.0, "%s: stitch_iou=%g must be in [0, 1)", what, stitch_iou);
  FDET_REQUIRE(min_length >= 1, "%s: min_length=%d must be >= 1", what, min_length);
  FDET_REQUIRE(seq_offset && h_seq_offset && rejected, "%s: null pointer", what);
  FDET_REQUIRE(T == 0 || (trk_rows && trk_ids && trk_misses && trk_counts && out_rows && out_ids && out_misses && out_kind &&
                          out_counts && ws),
               "%s: null pointer", what);
  FDET_REQUIRE(T == 0 || K == 0 || (det_rows && det_ids), "%s: null pointer", what);
  FDET_REQUIRE(h_seq_offset[0] == 0 && h_seq_offset[n_seq] == T, "%s: seq_offset must run from 0 to T=%d, got %d..%d", what, T,
               h_seq_offset[0], h_seq_offset[n_seq]);
  for (int s = 0; s < n_seq; ++s)
    FDET_REQUIRE(h_seq_offset[s + 1] >= h_seq_offset[s], "%s: seq_offset[%d]=%d < seq_offset[%d]=%d", what, s + 1,
                 h_seq_offset[s + 1], s, h_seq_offset[s]);
  FDET_REQUIRE(ws_bytes >= fdet_track_refine_ws_bytes(n_seq, T), "%s: workspace of %zu bytes, %zu needed", what, ws_bytes,
               fdet_track_refine_ws_bytes(n_seq, T));
  if (T == 0) return FDET_OK;
  FDET_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0, "%s: workspace must be 4-byte aligned", what);
  if (int rc = set_lds_attr(reinterpret_cast<const void*>(k_track_refine), LDS_BYTES, what)) return rc;
  Rec* const recs = reinterpret_cast<Rec*>(ws);
  int32_t* const nrec = reinterpret_cast<int32_t*>(recs + (size_t)T * NS);
  hipLaunchKernelGGL(k_track_refine, dim3(n_seq), dim3(NTHR), LDS_BYTES, (hipStream_t)stream, det_rows, det_ids, K, trk_rows, trk_ids,
                     trk_misses, trk_counts, seq_offset, T, lookback, grow256, stitch_gap, stitch_iou, min_length, out_rows, out_ids,
                     out_misses, out_kind, out_counts, recs, nrec, reinterpret_cast<unsigned long long*>(rejected));
  return check_launch(what);
}
