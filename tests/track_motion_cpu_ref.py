"""Sequential restatement of fdet_track_update_motion on Python ints, written from the rule in include/fdet.h:
the nine steps of tests/track_cpu_ref.py plus the prediction (0), the velocity update (5'), the damping (6') and the growth of
a coasting track's emitted box (9').  The state is the same 48-byte fdet_track; the velocities are reserved[0] and
reserved[1].  Also the generator of the moving-face sequence the host and the GPU tests share.
"""
from fractions import Fraction

import numpy as np

import track_cpu_ref as R

M = R.MAX_COORD
AXES = (("x1q", "x2q"), ("y1q", "y2q"))


def _frame(st, rows, count, iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score, beta256, damp256, max_speed,
           grow256):
    """One frame of one sequence on the state record `st` (modified in place) -> (out_rows, out_ids, out_misses, n, det_ids)
    or None when the frame has more than MAX_DETS valid rows."""
    K = rows.shape[0]
    seq, tracks = st["seq"], st["tracks"]
    det_ids = np.zeros(K, np.int32)
    dets = []
    for j in range(count):
        box = R.valid_box(rows[j])
        if box is not None:
            dets.append((j, box, np.float32(rows[j, 0])))
    if len(dets) > R.MAX_DETS:
        return None
    live = [s for s in range(R.SLOTS) if tracks[s]["id"] != 0]
    # step 0
    for s in live:
        tr = tracks[s]
        for a, (lo, hi) in enumerate(AXES):
            sh = (int(tr["reserved"][a]) + 8) >> 4
            qa, qb = int(tr[lo]) + sh, int(tr[hi]) + sh
            if abs((qa + 8) >> 4) <= M and abs((qb + 8) >> 4) <= M:
                tr[lo], tr[hi] = qa, qb
            else:
                tr["reserved"][a] = 0
    # steps 3 + 4, on the predicted, un-grown boxes
    pairs = []
    for s in live:
        P = R.pixel_box(tracks[s])
        for k, (j, D, _) in enumerate(dets):
            inter, uni = R.overlap(P, D)
            if float(inter) > float(iou_threshold) * float(uni):
                pairs.append((Fraction(-inter, uni), s, k))
    pairs.sort()
    t_match, d_match = {}, {}
    for _, s, k in pairs:
        if s not in t_match and k not in d_match:
            t_match[s], d_match[k] = k, s
    # steps 5' + 5, 6 + 6'
    vmax = 256 * max_speed
    for s in live:
        tr = tracks[s]
        if s in t_match:
            _, D, score = dets[t_match[s]]
            for a, (lo, hi) in enumerate(AXES):
                r = 16 * (D[a] + D[2 + a]) - (int(tr[lo]) + int(tr[hi]))
                v = int(tr["reserved"][a]) + ((beta256 * 8 * r + 128) >> 8)
                tr["reserved"][a] = min(max(v, -vmax), vmax)
            for e, key in enumerate(R.CORNERS):
                tr[key] = (alpha256 * 16 * D[e] + (256 - alpha256) * int(tr[key]) + 128) >> 8
            tr["hits"] += 1
            tr["misses"] = 0
            tr["score"] = score
            det_ids[dets[t_match[s]][0]] = tr["id"]
        else:
            tr["misses"] += 1
            if tr["misses"] > max_misses:
                tracks[s] = np.zeros((), R.TRACK_DTYPE)
            else:
                for a in range(2):
                    tr["reserved"][a] = (int(tr["reserved"][a]) * damp256 + 128) >> 8
    # step 7
    for k, (j, D, score) in enumerate(dets):
        if k in d_match or not (score >= np.float32(birth_score)):
            continue
        free = [s for s in range(R.SLOTS) if tracks[s]["id"] == 0]
        if not free:
            seq["dropped"] += 1
            continue
        seq["next_id"] += 1
        tr = tracks[free[0]]
        tr["id"] = seq["next_id"]
        for e, key in enumerate(R.CORNERS):
            tr[key] = 16 * D[e]
        tr["hits"], tr["misses"], tr["born"], tr["score"] = 1, 0, seq["frame"], score
        tr["reserved"] = 0
        det_ids[j] = tr["id"]
    # steps 9 + 9'
    out_rows = np.zeros((R.SLOTS, 5), np.float32)
    out_ids = np.zeros(R.SLOTS, np.int32)
    out_misses = np.zeros(R.SLOTS, np.int32)
    n = 0
    for s in range(R.SLOTS):
        tr = tracks[s]
        if tr["id"] != 0 and tr["hits"] >= min_hits and tr["misses"] <= emit_misses:
            P = R.pixel_box(tr)
            m = int(tr["misses"])
            gx = gy = 0
            if m > 0:
                gx = min((grow256 * m * (P[2] - P[0]) + 256) >> 9, M)
                gy = min((grow256 * m * (P[3] - P[1]) + 256) >> 9, M)
            out_rows[n] = (tr["score"], P[0] - gx, P[1] - gy, P[2] - P[0] + 2 * gx, P[3] - P[1] + 2 * gy)
            out_ids[n], out_misses[n] = tr["id"], m
            n += 1
    seq["frame"] += 1
    return out_rows, out_ids, out_misses, n, det_ids


def track_update_motion(rows, counts, seq_offset, state, iou_threshold=0.3, alpha256=128, max_misses=5, min_hits=2,
                        emit_misses=None, birth_score=0.0, beta256=128, damp256=256, max_speed=64, grow256=0):
    """track_cpu_ref.track_update's arguments and results, with the four motion parameters."""
    assert 0 <= beta256 <= 256 and 0 <= damp256 <= 256 and 0 <= grow256 <= 256 and 0 <= max_speed <= 1024
    rows = np.asarray(rows, np.float32)
    counts = np.asarray(counts, np.int64)
    T, K = rows.shape[0], rows.shape[1]
    emit_misses = max_misses if emit_misses is None else emit_misses
    out_rows = np.zeros((T, R.SLOTS, 5), np.float32)
    out_ids = np.zeros((T, R.SLOTS), np.int32)
    out_misses = np.zeros((T, R.SLOTS), np.int32)
    out_counts = np.zeros(T, np.int32)
    det_ids = np.zeros((T, K), np.int32)
    rejected = 0
    for s in range(len(seq_offset) - 1):
        t0, t1 = int(seq_offset[s]), int(seq_offset[s + 1])
        st = state[s:s + 1].copy()
        res = []
        for t in range(t0, t1):
            r = None
            if 0 <= counts[t] <= K:
                r = _frame(st[0], rows[t], int(counts[t]), iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score,
                           beta256, damp256, max_speed, grow256)
            if r is None:
                res = None
                break
            res.append(r)
        if res is None:                                     # rejected as a whole: state untouched, velocities included
            rejected += 1
            continue
        state[s] = st[0]
        for t, r in zip(range(t0, t1), res):
            out_rows[t], out_ids[t], out_misses[t], out_counts[t], det_ids[t] = r
    return out_rows, out_ids, out_misses, out_counts, det_ids, rejected


NEUTRAL = dict(beta256=0, damp256=256, max_speed=64, grow256=0)

# the sequence of the exact-prediction and the anonymisation tests: a 16 x 16 face at +6 px/frame in x and +2 in y,
# detected in frames 0..4 and 8..11, missed in 5..7
MOVING_T, MOVING_MISSED, MOVING_START, MOVING_V, MOVING_SIZE = 12, (5, 6, 7), (10, 20), (6, 2), 16
MOVING_PARAMS = dict(iou_threshold=0.3, alpha256=256, max_misses=5, min_hits=1, emit_misses=5, birth_score=0.0)
MOVING_MOTION = dict(beta256=256, damp256=256, max_speed=64, grow256=0)


def moving_face(K=4, score=0.9):
    """(rows (12,K,5) fp32, counts (12,), true (12,4) int [x, y, w, h] of the face in every frame)."""
    t = np.arange(MOVING_T)
    true = np.stack([MOVING_START[0] + MOVING_V[0] * t, MOVING_START[1] + MOVING_V[1] * t, np.full(MOVING_T, MOVING_SIZE),
                     np.full(MOVING_T, MOVING_SIZE)], 1)
    rows = np.zeros((MOVING_T, K, 5), np.float32)
    counts = np.ones(MOVING_T, np.int32)
    counts[list(MOVING_MISSED)] = 0
    for i in range(MOVING_T):
        if counts[i]:
            rows[i, 0] = (score, *true[i])
    return rows, counts, true
