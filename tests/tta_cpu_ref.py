"""numpy restatement of the test-time augmentation of tiled detection (fdet_amd/tiling.py plan_tta, csrc/fdet_tiles.hip
fdet_tile_gather_flags / fdet_tile_merge_vote), written from the rule in include/fdet.h and DESIGN.md 5f: the doubled plan,
the mirrored gather as tiles_cpu_ref's gather plus a column reversal, and the merge as the plain sequential loop with
ownership, float32 un-mirror and mapping in the stated order and the vote sums in Python integers, so rows compare exactly.
Not a test module: tests import it.
"""
import numpy as np

import tiles_cpu_ref as R

f32 = np.float32
MAX_CANDIDATES = R.MAX_CANDIDATES
LIMIT = f32(2.0 ** 24)


# ---------------------------------------------------------------------------------------------------------------- plan
def plan_tta(sizes, tile_sizes=(480,), overlap=0.25, include_whole=True, flip=False):
    """-> (list of (image, x0, y0, w, h), offsets, flags)"""
    recs, offs = R.plan(sizes, tile_sizes, overlap, include_whole)
    if not flip:
        return recs, offs, [0] * len(recs)
    out, flags, new = [], [], [0]
    for i in range(len(offs) - 1):
        mine = recs[offs[i]:offs[i + 1]]
        out += mine + mine
        flags += [0] * len(mine) + [1] * len(mine)
        new.append(len(out))
    return out, new, flags


# -------------------------------------------------------------------------------------------------------------- gather
def gather(img, win, Ho, Wo, flag=0):
    fr = R.gather(img, win, Ho, Wo)
    return fr[:, :, ::-1].copy() if flag & 1 else fr


# --------------------------------------------------------------------------------------------------------------- merge
def unmirror(d, Wo):
    """step 0: x <- ((float)Wo - x) - w, two float32 subtractions in that order"""
    d = np.array(d, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        d[1] = f32(f32(f32(Wo) - d[1]) - d[3])
    return d


def unmirror_rows(rows, flags, Wo):
    """every row of the flagged tiles un-mirrored (what a test feeds fdet_tile_merge with)"""
    rows = np.array(rows, f32)
    for t, fl in enumerate(flags):
        if int(fl) & 1:
            rows[t, :, 1] = (f32(Wo) - rows[t, :, 1]) - rows[t, :, 3]
    return rows


def weight(key, x1, y1, x2, y2):
    """q = llrint((double)min(score, 1.0f) * 2^20); 0 for a NaN (key -inf) or non-positive score and for a box with a corner
    that is not finite or beyond 2^24"""
    if not key > 0:
        return 0
    for c in (x1, y1, x2, y2):
        if not (np.isfinite(c) and abs(c) <= LIMIT):
            return 0
    return int(np.rint(np.float64(min(f32(key), f32(1.0))) * 1048576.0))


def _candidates(rows, counts, wins, flags, Ho, Wo, img_hw, margin):
    cand = []
    for t, win in enumerate(wins):
        for r in range(int(counts[t])):
            d = unmirror(rows[t, r], Wo) if int(flags[t]) & 1 else np.asarray(rows[t, r], f32)
            if R.cut_by_window(d, win, img_hw, Ho, Wo, margin):
                continue
            s = f32(d[0])
            cand.append((f32(-np.inf) if np.isnan(s) else s, s) + R.to_source(d, win, Ho, Wo))
    return cand


def merge_vote_image(rows, counts, wins, flags, Ho, Wo, img_hw, margin, thr, K, Kout, vote, min_votes):
    """One image -> ((k,5) float32 survivors in visiting order, (k,) votes, rejected)."""
    none = (np.zeros((0, 5), f32), np.zeros(0, np.int32), True)
    if any(int(c) < 0 or int(c) > K for c in counts):
        return none
    cand = _candidates(rows, counts, wins, flags, Ho, Wo, img_hw, margin)
    if len(cand) > MAX_CANDIDATES:
        return none
    order = sorted(range(len(cand)), key=lambda i: (-cand[i][0], i))
    c = np.array([cand[i] for i in order], f32).reshape(-1, 6)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x1, y1 = c[:, 2], c[:, 3]
        x2, y2 = x1 + c[:, 4], y1 + c[:, 5]
        area = (x2 - x1) * (y2 - y1)
        dead = np.zeros(len(order), bool)
        kept, votes = [], []
        for a in range(len(order)):
            if dead[a]:
                continue
            w = np.maximum(f32(0), np.minimum(x2[a], x2[a + 1:]) - np.maximum(x1[a], x1[a + 1:]))
            h = np.maximum(f32(0), np.minimum(y2[a], y2[a + 1:]) - np.maximum(y1[a], y1[a + 1:]))
            inter = w * h
            ovr = inter / (area[a] + area[a + 1:] - inter)
            kill = ~dead[a + 1:] & (ovr.astype(np.float64) > thr)      # owned by a: the first keeper that suppresses them
            dead[a + 1:] |= kill
            members = [a] + (a + 1 + np.nonzero(kill)[0]).tolist()
            row = np.array(cand[order[a]][1:], f32)
            if vote:
                Q = S1 = S2 = S3 = S4 = 0                               # Python integers: exact
                for m in members:
                    q = weight(c[m, 0], x1[m], y1[m], x2[m], y2[m])
                    if q:
                        Q += q
                        S1 += q * int(x1[m])
                        S2 += q * int(y1[m])
                        S3 += q * int(x2[m])
                        S4 += q * int(y2[m])
                if Q > 0:
                    X1, Y1, X2, Y2 = (np.rint(np.float64(S) / np.float64(Q)) for S in (S1, S2, S3, S4))
                    row = np.array([row[0], f32(X1), f32(Y1), f32(X2 - X1), f32(Y2 - Y1)], f32)
            if len(members) >= min_votes:
                kept.append(row)
                votes.append(len(members))
    if len(kept) > Kout:
        return none
    return np.array(kept, f32).reshape(-1, 5), np.array(votes, np.int32), False


def merge_vote(rows, counts, tiles, flags, tile_offset, sizes, Ho, Wo, margin, thr, Kout, vote=1, min_votes=1):
    """All images: tiles = list of (image, x0, y0, w, h); flags per tile (None = zeros); sizes (n,2) (h,w).
    -> (out (n,Kout,5), out_votes (n,Kout), out_counts (n,), rejected)"""
    rows, counts = np.asarray(rows, f32), np.asarray(counts)
    flags = np.zeros(len(rows), np.uint8) if flags is None else np.asarray(flags)
    n, K = len(tile_offset) - 1, rows.shape[1]
    out, ov, cnt, rej = np.zeros((n, Kout, 5), f32), np.zeros((n, Kout), np.int32), np.zeros(n, np.int32), 0
    for i in range(n):
        a, b = int(tile_offset[i]), int(tile_offset[i + 1])
        wins = [tuple(int(v) for v in tiles[t])[1:] for t in range(a, b)]
        kept, votes, bad = merge_vote_image(rows[a:b], counts[a:b], wins, flags[a:b], Ho, Wo, tuple(int(v) for v in sizes[i]), margin,
                                            thr, K, Kout, vote, min_votes)
        if bad:
            rej += 1
            continue
        out[i, :len(kept)] = kept
        ov[i, :len(kept)] = votes
        cnt[i] = len(kept)
    return out, ov, cnt, rej
