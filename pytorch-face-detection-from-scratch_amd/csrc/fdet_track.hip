// Face tracking across frame sequences: fdet_track_update associates the detections of consecutive frames
// with a fixed table of tracks per sequence.  The rule, step by step, is stated with the declaration in include/fdet.h;
// tests/track_cpu_ref.py restates it sequentially in numpy, and the two agree byte for byte.
//
// One workgroup of 256 threads per sequence walks the sequence's frames in order with the state in LDS (16 B header + 128
// tracks x 48 B = 6160 B, field-major so that lane s touches bank s) and writes it back once, after the last frame, so a
// sequence that is rejected half-way leaves its state as it was.  Per frame:
//   * the valid rows are compacted in row order into LDS (wave ballots + per-wave counts, as fdet_tile_merge does); the
//     counts of the frame after next and the first 256 rows of the next frame are loaded while this frame is worked on, so
//     the walk does not wait for a global load per frame;
//   * the greedy matching of step 4 is found by locally dominant pairs: thread d owns compacted detection d and caches its
//     best unmatched track (largest IoU, lowest slot), thread 128 + s owns slot s and caches its best unmatched
//     detection (largest IoU, lowest row).  A pair that is the best of both its ends is what the greedy sweep would take
//     before any other pair touching either end, so all such pairs of a round are matched at once; the order of step 4 is a
//     strict total order on pairs, under which this gives exactly the greedy matching.  While an eligible pair is left the
//     best one of all is such a pair, so every round but the last matches something.  A typical frame takes two rounds
//     (all faces, then nothing) of two barriers each.  The live and the matched slots are 64-bit
//     masks, so the loop over a detection's candidate tracks is a scalar bit scan with no dependent LDS read;
//   * updates, frees, births (ranks by ballot: the k-th birth in row order takes the k-th free slot in slot order, which
//     is what taking the lowest free slot one birth at a time gives) and the emission are one thread per slot.
// fdet_track_update_motion is the same kernel with MOTION = true: the two velocity words of a track (F_VX, F_VY) are fields of
// the LDS state like the others, the prediction (step 0) and the damping (step 6') are done by the slot's own thread where
// it computes P and where it counts the miss, the velocity update (step 5') where it blends, and the growth (step 9') where
// it emits.  Each touches only words of its own slot, so the motion steps add no barrier; with MOTION = false they are
// compiled out and the kernel is fdet_track_update's as before.
// The only floating-point operations are the fp32 sums x + w, y + h of the validity test and the one double multiply of the
// eligibility test.  Built with -ffp-contract=off like every file here.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

constexpr int NS = FDET_TRACK_SLOTS, ND = FDET_TRACK_MAX_DETS, NTHR = 256;
constexpr int STATE_INTS = 4 + NS * 12;                       // fdet_track_seq + NS fdet_track, in int32 words
static_assert(sizeof(fdet_track) == 48 && sizeof(fdet_track_seq) == 16, "state layout");
static_assert(NTHR == ND && 2 * NS == NTHR && NS == 2 * WAVE, "one thread per detection, the upper two waves own the slots");

// words of fdet_track
enum { F_ID, F_X1, F_Y1, F_X2, F_Y2, F_HITS, F_MISS, F_BORN, F_SCORE, F_R0, F_R1, F_R2, NF };
enum { F_VX = F_R0, F_VY = F_R1 };           // fdet_track_update_motion: the velocity in 1/256 pixel per frame

// the best partner found so far for a track or a detection; inter == 0 means none (an eligible pair has inter > 0).
// Corners within +-FDET_TRACK_MAX_COORD (the tracks' too: a weighted mean of detections' corners) keep a side <= 2^15, an area
// and inter <= 2^30 and uni <= 2^31, so the rule's int64 values fit 32 unsigned bits here and a cross product 64.
struct Pair {
  unsigned inter, uni;
  int other;
};

__device__ __forceinline__ Pair no_pair() { return Pair{0u, 1u, -1}; }

// a.inter / a.uni > b.inter / b.uni, exactly
__device__ __forceinline__ bool larger(const Pair& a, const Pair& b) {
  return (unsigned long long)a.inter * b.uni > (unsigned long long)b.inter * a.uni;
}

// step 3 for a track box p and a detection box d; `areas` = areaT + areaD.  Not eligible -> no_pair()
__device__ __forceinline__ Pair overlap(int p0, int p1, int p2, int p3, int d0, int d1, int d2, int d3, unsigned areas, double thr,
                                        int other) {
  const int iw = min(p2, d2) - max(p0, d0), ih = min(p3, d3) - max(p1, d1);
  if (iw <= 0 || ih <= 0) return no_pair();
  const unsigned inter = (unsigned)iw * (unsigned)ih, uni = areas - inter;
  if (!((double)inter > thr * (double)uni)) return no_pair();
  return Pair{inter, uni, other};
}

// a value every lane holds alike, moved to scalar registers
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// the parameters of the motion steps; fdet_track_update passes zeros and reads none
struct Motion {
  int beta256, damp256, vmax256, grow256;
};

template <bool MOTION>
__global__ void __launch_bounds__(NTHR)
k_track_update(const float* __restrict__ rows, const int32_t* __restrict__ counts, const int32_t* __restrict__ seq_offset, int T,
               int K, double thr, int alpha256, int max_misses, int min_hits, int emit_misses, float birth_score,
               int32_t* __restrict__ state, float* __restrict__ out_rows, int32_t* __restrict__ out_ids,
               int32_t* __restrict__ out_misses, int32_t* __restrict__ out_counts, int32_t* __restrict__ det_ids,
               unsigned long long* __restrict__ rejected, Motion mo) {
  __shared__ int tf[NF][NS];                 // the tracks, field-major
  __shared__ int hdr[4];                     // next_id, frame, dropped, reserved
  __shared__ int tP[4][NS];                  // step 2: the tracks' boxes in pixels
  __shared__ int tDet[NS];                   // slot -> matched detection, -1 = none
  __shared__ int freeList[NS];
  __shared__ unsigned long long lmask[2], taken[2];     // live / matched slots, one bit per slot
  __shared__ int dB[4][ND];                  // step 1: X1, Y1, X2, Y2 of the valid rows, compacted in row order
  __shared__ int dRow[ND];
  __shared__ float dSc[ND];
  __shared__ int tBest[NS];                  // slot -> the detection it likes best, -1 = none or matched
  __shared__ int dMat[ND];                   // detection -> matched slot, -1 = none
  __shared__ int ctl[20];                    // per-wave counts: [0..7] valid rows (two sets, by chunk parity), [8..11] births,
                                             // [12..13] free slots, [16..17] emitted

  const int seq = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  // threads 128..255 own the slots: slot sl, in the waves swid = 0 | 1.  The detections are owned from thread 0 up, so the
  // per-slot and the per-detection work of a frame with up to 128 detections lie in different waves
  const bool isSlot = tid >= NS;
  const int sl = tid - NS, swid = wid - 2;
  const int t0 = seq_offset[seq], t1 = seq_offset[seq + 1];
  if (t0 < 0 || t1 < t0 || t1 > T) {         // the host validated its copy; no frame can be addressed from these
    if (tid == 0) atomicAdd(rejected, 1ull);
    return;
  }
  int32_t* const g = state + (size_t)seq * STATE_INTS;
  if (tid < 4) hdr[tid] = g[tid];
  for (int i = tid; i < NS * NF; i += NTHR) tf[i % NF][i / NF] = g[4 + i];
  __syncthreads();

  // counts two frames ahead and the first 256 rows one frame ahead are loaded while the current frame is worked on
  int cCur = 0, cNext = 0;
  float pr[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (t0 < t1) {
    cCur = counts[t0];
    if (t0 + 1 < t1) cNext = counts[t0 + 1];
    if (cCur >= 0 && cCur <= K && tid < cCur) {
      const float* d = rows + ((size_t)t0 * K + tid) * 5;
#pragma unroll
      for (int e = 0; e < 5; ++e) pr[e] = d[e];
    }
  }
  bool bad = false;
  for (int t = t0; t < t1; ++t) {
    const int c = cCur;                      // uniform: every thread read the same word
    if (c < 0 || c > K) { bad = true; break; }
    const float* const fr = rows + (size_t)t * K * 5;
    int32_t* const did = det_ids + (size_t)t * K;
    int cNN = 0;
    float nx[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (t + 2 < t1) cNN = counts[t + 2];
    if (t + 1 < t1 && cNext >= 0 && cNext <= K && tid < cNext) {      // only rows below the count are ever read
      const float* d = fr + ((size_t)K + tid) * 5;
#pragma unroll
      for (int e = 0; e < 5; ++e) nx[e] = d[e];
    }

    // ---- step 1: valid rows, compacted in row order -----------------------------------------------------------------
    int nD = 0;                              // uniform
    for (int r0 = 0, set = 0; r0 < c; r0 += NTHR, set ^= 4) {
      const int r = r0 + tid;
      bool ok = false;
      int X1 = 0, Y1 = 0, X2 = 0, Y2 = 0;
      float sc = 0.f;
      if (r < c) {
        float v[5];
        if (r0 == 0) {
#pragma unroll
          for (int e = 0; e < 5; ++e) v[e] = pr[e];
        } else {
          const float* d = fr + (size_t)r * 5;
#pragma unroll
          for (int e = 0; e < 5; ++e) v[e] = d[e];
        }
        sc = v[0];
        const float x = v[1], y = v[2], w = v[3], h = v[4];
        const float lim = (float)FDET_TRACK_MAX_COORD;
        const float fx1 = rintf(x), fy1 = rintf(y), fx2 = rintf(x + w), fy2 = rintf(y + h);
        // every comparison is false for a NaN; an infinite x, y, w or h makes a corner infinite or NaN
        ok = fabsf(sc) <= 3.402823466e38f && fabsf(w) <= 3.402823466e38f && fabsf(h) <= 3.402823466e38f &&
             fabsf(fx1) <= lim && fabsf(fy1) <= lim && fabsf(fx2) <= lim && fabsf(fy2) <= lim;
        if (ok) {
          X1 = (int)fx1; Y1 = (int)fy1; X2 = (int)fx2; Y2 = (int)fy2;
          ok = X2 - X1 >= 1 && Y2 - Y1 >= 1;
        }
        if (!ok) did[r] = 0;
      }
      const unsigned long long bal = __ballot(ok);
      if (lane == 0) ctl[set + wid] = __popcll(bal);
      __syncthreads();                       // the set written two chunks ago was read before the barrier in between
      int k = nD + __popcll(bal & below);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int n = ctl[set + w];
        nD += n;
        if (w < wid) k += n;
      }
      if (ok && k < ND) {
        dB[0][k] = X1; dB[1][k] = Y1; dB[2][k] = X2; dB[3][k] = Y2;
        dRow[k] = r;
        dSc[k] = sc;
      }
    }
    for (int j = c + tid; j < K; j += NTHR) did[j] = 0;
    if (nD > ND) { bad = true; break; }      // uniform

    // ---- step 2: live tracks in pixels; the live slots as two 64-bit masks -----------------------------------------
    bool live = false;
    int q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    if (isSlot) {
      live = tf[F_ID][sl] != 0;
      if (live) {
        int c[4] = {tf[F_X1][sl], tf[F_Y1][sl], tf[F_X2][sl], tf[F_Y2][sl]};
        if (MOTION) {                        // step 0: both corners of an axis move, or the axis stops
          constexpr int M = FDET_TRACK_MAX_COORD;
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const int s = (tf[F_VX + a][sl] + 8) >> 4;        // |v256| <= 2^18, |q| < 2^19: 32 bits hold every value
            const int qa = c[a] + s, qb = c[2 + a] + s;
            const int pa = (qa + 8) >> 4, pb = (qb + 8) >> 4;
            if (pa >= -M && pa <= M && pb >= -M && pb <= M) {
              c[a] = qa; c[2 + a] = qb;
              tf[F_X1 + a][sl] = qa; tf[F_X2 + a][sl] = qb;
            } else {
              tf[F_VX + a][sl] = 0;
            }
          }
        }
        q0 = (c[0] + 8) >> 4; q1 = (c[1] + 8) >> 4; q2 = (c[2] + 8) >> 4; q3 = (c[3] + 8) >> 4;
        tP[0][sl] = q0; tP[1][sl] = q1; tP[2][sl] = q2; tP[3][sl] = q3;
      }
      tDet[sl] = -1;
    }
    dMat[tid] = -1;
    {
      const unsigned long long bal = __ballot(live);
      if (lane == 0 && isSlot) { lmask[swid] = bal; taken[swid] = 0ull; }
    }
    __syncthreads();                         // also: the detections of step 1 are in LDS
    const unsigned long long live0 = uniform64(lmask[0]), live1 = uniform64(lmask[1]);

    // ---- steps 3 + 4: greedy matching by locally dominant pairs ------------------------------------------------------
    // Thread d owns detection d and caches its best unmatched track; thread 128 + s owns slot s and caches its best
    // unmatched detection (with up to 128 detections the two loops run in different waves, side by side).  A pair that is the best of both its ends is matched, all such pairs of a round at once; a
    // cache is recomputed only when its partner was taken by another.
    const bool isDet = tid < nD;
    int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    float mySc = 0.f;
    if (isDet) { b0 = dB[0][tid]; b1 = dB[1][tid]; b2 = dB[2][tid]; b3 = dB[3][tid]; mySc = dSc[tid]; }
    const unsigned areaD = (unsigned)(b2 - b0) * (unsigned)(b3 - b1);
    int myMatch = -1;
    if ((live0 | live1) != 0ull && nD > 0) { // uniform
      const unsigned areaT = (unsigned)(q2 - q0) * (unsigned)(q3 - q1);
      Pair bestD = no_pair(), bestT = no_pair();       // this thread's detection -> a slot; this thread's slot -> a detection
      bool staleD = isDet, staleT = live;
      for (;;) {
        if (staleD) {                        // larger IoU, then lower slot: slots ascending, strict comparison
          bestD = no_pair();
          const unsigned long long free0 = live0 & ~uniform64(taken[0]), free1 = live1 & ~uniform64(taken[1]);
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            for (unsigned long long m = half ? free1 : free0; m; m &= m - 1) {      // a scalar loop: the slot is no LDS read
              const int s = half * 64 + __builtin_ctzll(m);
              const int p0 = tP[0][s], p1 = tP[1][s], p2 = tP[2][s], p3 = tP[3][s];  // the same words for every lane
              const Pair c = overlap(p0, p1, p2, p3, b0, b1, b2, b3, (unsigned)(p2 - p0) * (unsigned)(p3 - p1) + areaD, thr, s);
              if (larger(c, bestD)) bestD = c;
            }
          }
          staleD = false;
        }
        if (staleT) {                        // larger IoU, then lower row: rows ascending, strict comparison
          bestT = no_pair();
          for (int d = 0; d < nD; ++d) {
            if (dMat[d] >= 0) continue;
            const int e0 = dB[0][d], e1 = dB[1][d], e2 = dB[2][d], e3 = dB[3][d];
            const Pair c = overlap(q0, q1, q2, q3, e0, e1, e2, e3, areaT + (unsigned)(e2 - e0) * (unsigned)(e3 - e1), thr, d);
            if (larger(c, bestT)) bestT = c;
          }
          staleT = false;
        }
        if (live) tBest[sl] = tDet[sl] < 0 ? bestT.other : -1;
        __syncthreads();
        const bool hit = isDet && myMatch < 0 && bestD.inter > 0 && tBest[bestD.other] == tid;
        if (hit) {
          myMatch = bestD.other;
          tDet[myMatch] = tid;
          dMat[tid] = myMatch;
          atomicOr(&taken[myMatch >> 6], 1ull << (myMatch & 63));
        }
        if (!__syncthreads_or(hit)) break;   // no pair is the best of both its ends: no eligible pair is left
        if (isDet && myMatch < 0 && bestD.inter > 0 && tDet[bestD.other] >= 0) staleD = true;
        if (live && tDet[sl] < 0 && bestT.inter > 0 && dMat[bestT.other] >= 0) staleT = true;
      }
    }

    // ---- steps 5 + 6: one thread per live slot ------------------------------------------------------------------------
    if (live) {
      const int d = tDet[sl];
      if (d >= 0) {
        if (MOTION) {                        // step 5': from the predicted corners, before they are blended
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const long long r = 16ll * (dB[a][d] + dB[2 + a][d]) - ((long long)tf[F_X1 + a][sl] + tf[F_X2 + a][sl]);
            const long long v = (long long)tf[F_VX + a][sl] + (((long long)mo.beta256 * 8 * r + 128) >> 8);
            tf[F_VX + a][sl] = (int)min(max(v, -(long long)mo.vmax256), (long long)mo.vmax256);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long q = (long long)tf[F_X1 + e][sl], D = (long long)dB[e][d];
          tf[F_X1 + e][sl] = (int)(((long long)alpha256 * 16 * D + (long long)(256 - alpha256) * q + 128) >> 8);
        }
        tf[F_HITS][sl] += 1;
        tf[F_MISS][sl] = 0;
        tf[F_SCORE][sl] = __float_as_int(dSc[d]);
      } else {
        const int m = tf[F_MISS][sl] + 1;
        tf[F_MISS][sl] = m;
        if (m > max_misses) {
#pragma unroll
          for (int e = 0; e < NF; ++e) tf[e][sl] = 0;
        } else if (MOTION) {                 // step 6'
          tf[F_VX][sl] = (tf[F_VX][sl] * mo.damp256 + 128) >> 8;
          tf[F_VY][sl] = (tf[F_VY][sl] * mo.damp256 + 128) >> 8;
        }
      }
    }
    __syncthreads();

    // ---- steps 7 + 8: births in row order into the free slots in slot order ----------------------------------------
    const bool birth = isDet && myMatch < 0 && mySc >= birth_score;
    const bool freeS = isSlot && tf[F_ID][sl] == 0;
    const unsigned long long balB = __ballot(birth), balF = __ballot(freeS);
    if (lane == 0) {
      ctl[8 + wid] = __popcll(balB);
      if (isSlot) ctl[12 + swid] = __popcll(balF);
    }
    __syncthreads();
    if (freeS) freeList[(swid ? ctl[12] : 0) + __popcll(balF & below)] = sl;
    const int nFree = ctl[12] + ctl[13], nB = ctl[8] + ctl[9] + ctl[10] + ctl[11];
    int bRank = __popcll(balB & below);
    for (int w = 0; w < wid; ++w) bRank += ctl[8 + w];
    __syncthreads();
    int myId = 0;
    if (myMatch >= 0) myId = tf[F_ID][myMatch];
    if (birth && bRank < nFree) {
      const int s = freeList[bRank];
      myId = hdr[0] + bRank + 1;
      tf[F_ID][s] = myId;
      tf[F_X1][s] = 16 * b0; tf[F_Y1][s] = 16 * b1; tf[F_X2][s] = 16 * b2; tf[F_Y2][s] = 16 * b3;
      tf[F_HITS][s] = 1;
      tf[F_MISS][s] = 0;
      tf[F_BORN][s] = hdr[1];
      tf[F_SCORE][s] = __float_as_int(mySc);
      tf[F_R0][s] = 0; tf[F_R1][s] = 0; tf[F_R2][s] = 0;
    }
    if (isDet) did[dRow[tid]] = myId;
    __syncthreads();
    if (tid == 0) {
      const int nb = min(nB, nFree);
      hdr[0] += nb;
      hdr[2] += nB - nb;
      hdr[1] += 1;                           // step 9's frame += 1; nothing below reads it
    }

    // ---- step 9: emit in slot order -------------------------------------------------------------------------------------
    {
      const bool em = isSlot && tf[F_ID][sl] != 0 && tf[F_HITS][sl] >= min_hits && tf[F_MISS][sl] <= emit_misses;
      const unsigned long long bal = __ballot(em);
      if (lane == 0 && isSlot) ctl[16 + swid] = __popcll(bal);
      __syncthreads();
      const int nE = ctl[16] + ctl[17];
      float* const o = out_rows + (size_t)t * NS * 5;
      int32_t* const oi = out_ids + (size_t)t * NS;
      int32_t* const om = out_misses + (size_t)t * NS;
      if (em) {
        const int p = (swid ? ctl[16] : 0) + __popcll(bal & below);
        const int p0 = (tf[F_X1][sl] + 8) >> 4, p1 = (tf[F_Y1][sl] + 8) >> 4;
        const int p2 = (tf[F_X2][sl] + 8) >> 4, p3 = (tf[F_Y2][sl] + 8) >> 4;
        int gx = 0, gy = 0;
        if (MOTION) {                        // step 9': misses = 0 gives 0; misses has no bound, so 64 bits
          const long long gm = (long long)mo.grow256 * tf[F_MISS][sl];
          gx = (int)min((gm * (p2 - p0) + 256) >> 9, (long long)FDET_TRACK_MAX_COORD);
          gy = (int)min((gm * (p3 - p1) + 256) >> 9, (long long)FDET_TRACK_MAX_COORD);
        }
        o[p * 5 + 0] = __int_as_float(tf[F_SCORE][sl]);
        o[p * 5 + 1] = (float)(p0 - gx); o[p * 5 + 2] = (float)(p1 - gy);
        o[p * 5 + 3] = (float)(p2 - p0 + 2 * gx); o[p * 5 + 4] = (float)(p3 - p1 + 2 * gy);
        oi[p] = tf[F_ID][sl];
        om[p] = tf[F_MISS][sl];
      }
      if (isSlot && sl >= nE) {
#pragma unroll
        for (int e = 0; e < 5; ++e) o[sl * 5 + e] = 0.f;
        oi[sl] = 0;
        om[sl] = 0;
      }
      if (tid == 0) out_counts[t] = nE;
    }
    __syncthreads();
    cCur = cNext;
    cNext = cNN;
#pragma unroll
    for (int e = 0; e < 5; ++e) pr[e] = nx[e];
  }

  if (bad) {                                 // the whole sequence: outputs zeroed, state left as it was
    __syncthreads();                         // this block's earlier stores to the same words come first
    const size_t n = (size_t)(t1 - t0);
    float* const o = out_rows + (size_t)t0 * NS * 5;
    for (size_t i = tid; i < n * NS * 5; i += NTHR) o[i] = 0.f;
    for (size_t i = tid; i < n * NS; i += NTHR) { out_ids[(size_t)t0 * NS + i] = 0; out_misses[(size_t)t0 * NS + i] = 0; }
    for (size_t i = tid; i < n * (size_t)K; i += NTHR) det_ids[(size_t)t0 * K + i] = 0;
    for (size_t i = tid; i < n; i += NTHR) out_counts[t0 + i] = 0;
    if (tid == 0) atomicAdd(rejected, 1ull);
    return;
  }
  if (tid < 4) g[tid] = hdr[tid];
  for (int i = tid; i < NS * NF; i += NTHR) g[4 + i] = tf[i % NF][i / NF];
}

}  // namespace

extern "C" size_t fdet_track_state_bytes(int n_seq) {
  return n_seq < 1 ? 0 : (size_t)n_seq * (sizeof(fdet_track_seq) + (size_t)NS * sizeof(fdet_track));
}

namespace {

int track_update(const char* what, bool motion, Motion mo, const float* rows, const int32_t* counts, const int32_t* seq_offset,
                 const int32_t* h_seq_offset, int n_seq, int T, int K, double iou_threshold, int alpha256, int max_misses,
                 int min_hits, int emit_misses, float birth_score, void* state, float* out_rows, int32_t* out_ids,
                 int32_t* out_misses, int32_t* out_counts, int32_t* det_ids, uint64_t* rejected, void* stream) {
  FDET_REQUIRE(n_seq >= 1 && T >= 0 && K >= 0, "%s: bad sizes n_seq=%d T=%d K=%d", what, n_seq, T, K);
  FDET_REQUIRE(alpha256 >= 1 && alpha256 <= 256, "%s: alpha256=%d must be in 1..256", what, alpha256);
  FDET_REQUIRE(max_misses >= 0 && min_hits >= 1 && emit_misses >= 0 && emit_misses <= max_misses,
               "%s: max_misses=%d must be >= 0, min_hits=%d >= 1 and emit_misses=%d in 0..max_misses", what, max_misses, min_hits,
               emit_misses);
  FDET_REQUIRE(iou_threshold >= 0.0 && iou_threshold < 1.0, "%s: iou_threshold=%g must be in [0, 1)", what, iou_threshold);
  FDET_REQUIRE(seq_offset && h_seq_offset && state && rejected, "%s: null pointer", what);
  FDET_REQUIRE(T == 0 || (counts && out_rows && out_ids && out_misses && out_counts), "%s: null pointer", what);
  FDET_REQUIRE(T == 0 || K == 0 || (rows && det_ids), "%s: null pointer", what);
  FDET_REQUIRE(h_seq_offset[0] == 0 && h_seq_offset[n_seq] == T, "%s: seq_offset must run from 0 to T=%d, got %d..%d", what, T,
               h_seq_offset[0], h_seq_offset[n_seq]);
  for (int s = 0; s < n_seq; ++s)
    FDET_REQUIRE(h_seq_offset[s + 1] >= h_seq_offset[s], "%s: seq_offset[%d]=%d < seq_offset[%d]=%d", what, s + 1,
                 h_seq_offset[s + 1], s, h_seq_offset[s]);
  if (T == 0) return FDET_OK;                // no frame: every state stays as it is
  hipLaunchKernelGGL(motion ? k_track_update<true> : k_track_update<false>, dim3(n_seq), dim3(NTHR), 0, (hipStream_t)stream, rows,
                     counts, seq_offset, T, K, iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score,
                     reinterpret_cast<int32_t*>(state), out_rows, out_ids, out_misses, out_counts, det_ids,
                     reinterpret_cast<unsigned long long*>(rejected), mo);
  return check_launch(what);
}

}  // namespace

extern "C" int fdet_track_update(const float* rows, const int32_t* counts, const int32_t* seq_offset, const int32_t* h_seq_offset,
                                 int n_seq, int T, int K, double iou_threshold, int alpha256, int max_misses, int min_hits,
                                 int emit_misses, float birth_score, void* state, float* out_rows, int32_t* out_ids,
                                 int32_t* out_misses, int32_t* out_counts, int32_t* det_ids, uint64_t* rejected, void* stream) {
  return track_update("fdet_track_update", false, Motion{0, 0, 0, 0}, rows, counts, seq_offset, h_seq_offset, n_seq, T, K,
                      iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score, state, out_rows, out_ids, out_misses,
                      out_counts, det_ids, rejected, stream);
}

extern "C" int fdet_track_update_motion(const float* rows, const int32_t* counts, const int32_t* seq_offset,
                                        const int32_t* h_seq_offset, int n_seq, int T, int K, double iou_threshold, int alpha256,
                                        int max_misses, int min_hits, int emit_misses, float birth_score, int beta256, int damp256,
                                        int max_speed, int grow256, void* state, float* out_rows, int32_t* out_ids,
                                        int32_t* out_misses, int32_t* out_counts, int32_t* det_ids, uint64_t* rejected,
                                        void* stream) {
  const char* what = "fdet_track_update_motion";
  FDET_REQUIRE(beta256 >= 0 && beta256 <= 256 && damp256 >= 0 && damp256 <= 256 && grow256 >= 0 && grow256 <= 256,
               "%s: beta256=%d, damp256=%d and grow256=%d must be in 0..256", what, beta256, damp256, grow256);
  FDET_REQUIRE(max_speed >= 0 && max_speed <= 1024, "%s: max_speed=%d must be in 0..1024", what, max_speed);
  return track_update(what, true, Motion{beta256, damp256, 256 * max_speed, grow256}, rows, counts, seq_offset, h_seq_offset, n_seq,
                      T, K, iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score, state, out_rows, out_ids,
                      out_misses, out_counts, det_ids, rejected, stream);
}
