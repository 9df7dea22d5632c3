"""Sequential restatement of fdet_track_refine on Python ints, written from the numbered rule in include/fdet.h:
anchors, stitching, the length filter, interpolation, back-fill, one row per frame and chain, order and room.  One sequence at
a time, one chain at a time; the box arithmetic is on Python ints (exact at any size) and reuses step 1 and step 3 of
tests/track_cpu_ref.py.  Besides the five outputs and the two counters it returns what it did, so that a test can tell that
its inputs exercised every step.
"""
import numpy as np

import track_cpu_ref as R

ROWS, MAX_IDS, M = 256, 4096, R.MAX_COORD
NAMES = ("out_rows", "out_ids", "out_misses", "out_kind", "out_counts")
STAT_KEYS = ("kind0", "kind1", "kind2", "kind3", "stitches", "dropped_chains", "backfill_clipped", "backfill_unclipped")


def interpolate(A, B, a, b, t):
    """Step 4: the box at frame a < t < b between the anchors (a, A) and (b, B), round half up per corner."""
    return tuple(A[c] + (2 * (B[c] - A[c]) * (t - a) + (b - a)) // (2 * (b - a)) for c in range(4))


def grow(F, m, grow256):
    """Step 9' of fdet_track_update_motion: [x, y, w, h] of the corner box F grown for m frames."""
    gx = min((grow256 * m * (F[2] - F[0]) + 256) >> 9, M)
    gy = min((grow256 * m * (F[3] - F[1]) + 256) >> 9, M)
    return F[0] - gx, F[1] - gy, F[2] - F[0] + 2 * gx, F[3] - F[1] + 2 * gy


def _sequence(det_rows, det_ids, trk_rows, trk_ids, trk_misses, trk_counts, t0, t1, lookback, grow256, stitch_gap, stitch_iou,
              min_length, stats):
    """The frames t0..t1-1 of one sequence -> {t: [(row (5,) fp32, id, misses, kind), ...] in output order, untruncated}, or
    None when the sequence is rejected."""
    K = det_rows.shape[1]
    ids = set()
    for t in range(t0, t1):
        c = int(trk_counts[t])
        if not 0 <= c <= R.SLOTS:
            return None
        for p in range(c):
            if int(trk_ids[t, p]) <= 0:
                return None
            ids.add(int(trk_ids[t, p]))
        ids.update(int(i) for i in det_ids[t] if i > 0)
    if ids and max(ids) - min(ids) + 1 > MAX_IDS:
        return None
    # step 1: anchors (t, box, score, row) per track in time order, coasted rows per track and frame
    anchors, coasted = {}, {}
    for t in range(t0, t1):
        c = int(trk_counts[t])
        emitted = set(int(i) for i in trk_ids[t, :c])
        found = []
        for p in range(c):
            i = int(trk_ids[t, p])
            if int(trk_misses[t, p]) == 0:
                found.append((i, trk_rows[t, p]))
            else:
                coasted.setdefault(i, {})[t] = (trk_rows[t, p].copy(), int(trk_misses[t, p]))
        for j in range(K):
            i = int(det_ids[t, j])
            if i > 0 and i not in emitted:
                found.append((i, det_rows[t, j]))
        if len(found) > R.SLOTS:
            return None
        for i, row in found:
            box = R.valid_box(row)
            if box is None:
                return None
            anchors.setdefault(i, []).append((t, box, np.float32(row[0]), row.copy()))
    # step 2: chains in ascending track id; chain id -> its anchors in time order, member tracks
    chains, members = {}, {}
    for j in sorted(anchors):
        f, F = anchors[j][0][0], anchors[j][0][1]
        best = None
        if stitch_gap >= 0:
            for cid in sorted(chains):
                L, A = chains[cid][-1][0], chains[cid][-1][1]
                if L < f and f - L - 1 <= stitch_gap:
                    inter, uni = R.overlap(A, F)
                    if float(inter) > float(stitch_iou) * float(uni) and (best is None or inter * best[1] > best[0] * uni):
                        best = (inter, uni, cid)
        if best is None:
            chains[j], members[j] = list(anchors[j]), [j]
        else:
            chains[best[2]].extend(anchors[j])
            members[best[2]].append(j)
            stats["stitches"] += 1
    # step 3
    for cid in [c for c in chains if len(chains[c]) < min_length]:
        for j in members[cid]:
            coasted.pop(j, None)
        del chains[cid], members[cid]
        stats["dropped_chains"] += 1
    for cid, an in chains.items():                          # what the back-fill of this chain meets
        if lookback > 0:
            stats["backfill_clipped" if an[0][0] - lookback < t0 else "backfill_unclipped"] += 1
    passthrough = sorted(i for i in coasted if i not in anchors)
    # steps 4..7, frame by frame
    out = {}
    for t in range(t0, t1):
        first, last = {}, []
        for cid in sorted(set(chains) | set(passthrough)):
            if cid in chains:
                an = chains[cid]
                at = [k for k, x in enumerate(an) if x[0] == t]
                own = [coasted[j][t] + (j,) for j in members[cid] if t in coasted.get(j, {})]
                if at:
                    first[cid] = (an[at[0]][3], 0, 0)
                elif an[0][0] < t < an[-1][0]:
                    k = max(k for k, x in enumerate(an) if x[0] < t)
                    (a, A, score, _), (b, B, _, _) = an[k], an[k + 1]
                    P = interpolate(A, B, a, b, t)
                    first[cid] = (np.array([score, P[0], P[1], P[2] - P[0], P[3] - P[1]], np.float32), t - a, 2)
                elif own:
                    row, misses, _ = max(own, key=lambda x: x[2])
                    first[cid] = (row, misses, 1)
                elif an[0][0] - lookback <= t < an[0][0]:
                    f, F, score = an[0][0], an[0][1], an[0][2]
                    last.append((np.array([score, *grow(F, f - t, grow256)], np.float32), cid, f - t, 3))
            elif t in coasted[cid]:
                first[cid] = (coasted[cid][t][0], coasted[cid][t][1], 1)
        out[t] = [(first[c][0], c, first[c][1], first[c][2]) for c in sorted(first)] + last
    return out


def track_refine(det_rows, det_ids, trk_rows, trk_ids, trk_misses, trk_counts, seq_offset, lookback=5, grow256=0, stitch_gap=10,
                 stitch_iou=0.1, min_length=1):
    """-> (out_rows (T,256,5) fp32, out_ids, out_misses, out_kind (T,256) int32, out_counts (T,) int32, [rejected sequences,
    rows without room], stats: rows written of each kind, stitches, dropped chains, chains whose back-fill was / was not cut
    off by the start of their sequence)."""
    assert 0 <= lookback <= 1024 and 0 <= grow256 <= 256 and stitch_gap <= 65535 and 0.0 <= stitch_iou < 1.0 and min_length >= 1
    det_rows, trk_rows = np.asarray(det_rows, np.float32), np.asarray(trk_rows, np.float32)
    T = trk_rows.shape[0]
    out_rows = np.zeros((T, ROWS, 5), np.float32)
    out_ids, out_misses, out_kind = (np.zeros((T, ROWS), np.int32) for _ in range(3))
    out_counts = np.zeros(T, np.int32)
    rejected = [0, 0]
    stats = dict.fromkeys(STAT_KEYS, 0)
    for s in range(len(seq_offset) - 1):
        t0, t1 = int(seq_offset[s]), int(seq_offset[s + 1])
        mine = dict.fromkeys(STAT_KEYS, 0)
        res = _sequence(det_rows, det_ids, trk_rows, trk_ids, trk_misses, trk_counts, t0, t1, lookback, grow256, stitch_gap,
                        stitch_iou, min_length, mine)
        if res is None:
            rejected[0] += 1
            continue
        for k in STAT_KEYS:
            stats[k] += mine[k]
        for t, rows in res.items():
            rejected[1] += max(0, len(rows) - ROWS)
            rows = rows[:ROWS]
            out_counts[t] = len(rows)
            for n, (row, cid, misses, kind) in enumerate(rows):
                out_rows[t, n], out_ids[t, n], out_misses[t, n], out_kind[t, n] = row, cid, misses, kind
                stats[f"kind{kind}"] += 1
    return out_rows, out_ids, out_misses, out_kind, out_counts, rejected, stats
