"""Sequential numpy restatement of fdet_track_update, written from the numbered rule in include/fdet.h.

One frame at a time, one track at a time, on Python ints (exact at any size), int64 and float64; the only fp32 operations
are the sums x + w and y + h of step 1 and the comparison with birth_score of step 7, as the rule says.  The state is the
C structs: per sequence one fdet_track_seq and FDET_TRACK_SLOTS fdet_track.

Also the seeded generator of synthetic sequences the host and the GPU tests share.
"""
from fractions import Fraction

import numpy as np

SLOTS, MAX_DETS, MAX_COORD = 128, 256, 16384
TRACK_DTYPE = np.dtype([("id", "<i4"), ("x1q", "<i4"), ("y1q", "<i4"), ("x2q", "<i4"), ("y2q", "<i4"), ("hits", "<i4"),
                        ("misses", "<i4"), ("born", "<i4"), ("score", "<f4"), ("reserved", "<i4", (3,))])
SEQ_DTYPE = np.dtype([("next_id", "<i4"), ("frame", "<i4"), ("dropped", "<i4"), ("reserved", "<i4")])
STATE_DTYPE = np.dtype([("seq", SEQ_DTYPE), ("tracks", TRACK_DTYPE, (SLOTS,))])
assert TRACK_DTYPE.itemsize == 48 and SEQ_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == 6160
CORNERS = ("x1q", "y1q", "x2q", "y2q")


def fresh_state(n_seq):
    return np.zeros(n_seq, dtype=STATE_DTYPE)


def valid_box(row):
    """Step 1 for one row [score,x,y,w,h] (fp32): (X1, Y1, X2, Y2) as Python ints, or None."""
    s, x, y, w, h = (np.float32(v) for v in row)
    if not all(np.isfinite(v) for v in (s, x, y, w, h)):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        c = [np.rint(x), np.rint(y), np.rint(np.float32(x + w)), np.rint(np.float32(y + h))]      # fp32 sums, half to even
    if not all(np.isfinite(v) and abs(float(v)) <= MAX_COORD for v in c):
        return None
    X1, Y1, X2, Y2 = (int(v) for v in c)
    if X2 - X1 < 1 or Y2 - Y1 < 1:
        return None
    return X1, Y1, X2, Y2


def pixel_box(tr):
    """Step 2: floor((q + 8) / 16) per corner."""
    return tuple((int(tr[k]) + 8) >> 4 for k in CORNERS)


def overlap(P, D):
    """Step 3: (inter, uni) as Python ints."""
    iw = min(P[2], D[2]) - max(P[0], D[0])
    ih = min(P[3], D[3]) - max(P[1], D[1])
    inter = iw * ih if iw > 0 and ih > 0 else 0
    uni = (P[2] - P[0]) * (P[3] - P[1]) + (D[2] - D[0]) * (D[3] - D[1]) - inter
    return inter, uni


def _frame(st, rows, count, iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score):
    """One frame of one sequence on the state record `st` (modified in place) -> (out_rows, out_ids, out_misses, n, det_ids)
    or None when the frame has more than MAX_DETS valid rows."""
    K = rows.shape[0]
    seq, tracks = st["seq"], st["tracks"]
    det_ids = np.zeros(K, np.int32)
    dets = []                                               # (row index, box, score) of the valid rows, in row order
    for j in range(count):
        box = valid_box(rows[j])
        if box is not None:
            dets.append((j, box, np.float32(rows[j, 0])))
    if len(dets) > MAX_DETS:
        return None
    live = [s for s in range(SLOTS) if tracks[s]["id"] != 0]
    # steps 3 + 4: every eligible pair, ordered once by (IoU descending, slot, row), then one sweep
    pairs = []
    for s in live:
        P = pixel_box(tracks[s])
        for k, (j, D, _) in enumerate(dets):
            inter, uni = overlap(P, D)
            if float(inter) > float(iou_threshold) * float(uni):
                pairs.append((Fraction(-inter, uni), s, k))
    pairs.sort()
    t_match, d_match = {}, {}
    for _, s, k in pairs:
        if s not in t_match and k not in d_match:
            t_match[s], d_match[k] = k, s
    # steps 5 + 6
    for s in live:
        tr = tracks[s]
        if s in t_match:
            _, D, score = dets[t_match[s]]
            for e, key in enumerate(CORNERS):
                tr[key] = (alpha256 * 16 * D[e] + (256 - alpha256) * int(tr[key]) + 128) >> 8
            tr["hits"] += 1
            tr["misses"] = 0
            tr["score"] = score
            det_ids[dets[t_match[s]][0]] = tr["id"]
        else:
            tr["misses"] += 1
            if tr["misses"] > max_misses:
                tracks[s] = np.zeros((), TRACK_DTYPE)
    # step 7
    for k, (j, D, score) in enumerate(dets):
        if k in d_match or not (score >= np.float32(birth_score)):
            continue
        free = [s for s in range(SLOTS) if tracks[s]["id"] == 0]
        if not free:
            seq["dropped"] += 1
            continue
        seq["next_id"] += 1
        tr = tracks[free[0]]
        tr["id"] = seq["next_id"]
        for e, key in enumerate(CORNERS):
            tr[key] = 16 * D[e]
        tr["hits"], tr["misses"], tr["born"], tr["score"] = 1, 0, seq["frame"], score
        det_ids[j] = tr["id"]
    # step 9
    out_rows = np.zeros((SLOTS, 5), np.float32)
    out_ids = np.zeros(SLOTS, np.int32)
    out_misses = np.zeros(SLOTS, np.int32)
    n = 0
    for s in range(SLOTS):
        tr = tracks[s]
        if tr["id"] != 0 and tr["hits"] >= min_hits and tr["misses"] <= emit_misses:
            P = pixel_box(tr)
            out_rows[n] = (tr["score"], P[0], P[1], P[2] - P[0], P[3] - P[1])
            out_ids[n], out_misses[n] = tr["id"], tr["misses"]
            n += 1
    seq["frame"] += 1
    return out_rows, out_ids, out_misses, n, det_ids


def track_update(rows, counts, seq_offset, state, iou_threshold=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=None,
                 birth_score=0.0):
    """rows (T,K,5) fp32, counts (T,), seq_offset (n_seq+1,), state (n_seq,) STATE_DTYPE, modified in place ->
    (out_rows (T,128,5) fp32, out_ids (T,128) int32, out_misses (T,128) int32, out_counts (T,) int32, det_ids (T,K) int32,
    rejected)."""
    rows = np.asarray(rows, np.float32)
    counts = np.asarray(counts, np.int64)
    T, K = rows.shape[0], rows.shape[1]
    emit_misses = max_misses if emit_misses is None else emit_misses
    out_rows = np.zeros((T, SLOTS, 5), np.float32)
    out_ids = np.zeros((T, SLOTS), np.int32)
    out_misses = np.zeros((T, SLOTS), np.int32)
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
                r = _frame(st[0], rows[t], int(counts[t]), iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score)
            if r is None:
                res = None
                break
            res.append(r)
        if res is None:                                     # rejected as a whole: state untouched, outputs zero
            rejected += 1
            continue
        state[s] = st[0]
        for t, r in zip(range(t0, t1), res):
            out_rows[t], out_ids[t], out_misses[t], out_counts[t], det_ids[t] = r
    return out_rows, out_ids, out_misses, out_counts, det_ids, rejected


def synthetic_sequence(T, K, seed, faces=4, size=(640, 480), dropout=0.2, false_positives=0.5, negative=False):
    """(rows (T,K,5) fp32, counts (T,) int32): `faces` boxes that move a few pixels per frame (the first two cross each
    other), each missed with probability `dropout`, plus Poisson(false_positives) false positives per frame, shuffled.
    negative: the scene is shifted so that part of the boxes have negative x and y.  Coordinates carry fractions."""
    g = np.random.default_rng(seed)
    W, H = size
    pos = np.stack([g.uniform(0.1 * W, 0.8 * W, faces), g.uniform(0.1 * H, 0.8 * H, faces)], 1)
    vel = g.uniform(-4, 4, (faces, 2))
    wh = g.uniform(24, 90, (faces, 2))
    if faces >= 2:                                          # two faces on one line, moving through each other
        pos[0], pos[1] = (0.2 * W, 0.5 * H), (0.2 * W + 6.0 * min(T, 30), 0.5 * H + 3)
        vel[0], vel[1] = (6.0, 0.0), (-6.0, 0.0)
        wh[0] = wh[1] = (60, 60)
    shift = np.array([0.3 * W, 0.3 * H]) if negative else np.zeros(2)
    rows = np.zeros((T, K, 5), np.float32)
    counts = np.zeros(T, np.int32)
    for t in range(T):
        out = []
        for f in range(faces):
            if g.random() >= dropout:
                xy = pos[f] - shift + g.normal(0, 1.0, 2)
                out.append((g.uniform(0.5, 1.0), xy[0], xy[1], wh[f, 0] + g.normal(0, 1.0), wh[f, 1] + g.normal(0, 1.0)))
        for _ in range(g.poisson(false_positives)):
            out.append((g.uniform(0.3, 0.7), g.uniform(-shift[0], W - shift[0]), g.uniform(-shift[1], H - shift[1]),
                        g.uniform(10, 60), g.uniform(10, 60)))
        out = [out[i] for i in g.permutation(len(out))][:K]
        counts[t] = len(out)
        if out:
            rows[t, :len(out)] = np.asarray(out, np.float32)
        pos += vel
    return rows, counts
