"""Sequential restatement of fdet_chip_extract and fdet_chip_best_update (include/fdet.h) on Python ints and
numpy int64.  Every value is an integer, so the device must agree with this byte for byte.

The resampling of one axis is a weight matrix [C,S] (rule 3).  The clamped gather of rule 4 is folded into it: window
index i reads image column clamp(w0 + i, 0, W-1), so the weights of the window indices that land on one image column add
up, which gives a matrix [C,W]; a chip channel is then  Ay @ plane @ Ax.T  in int64.  A window of S = 8192 on a 40x50
image costs no more than a small one."""
import numpy as np

MIN_SIZE, MAX_SIZE, MAX_SIDE, MAX_CHIPS, MAX_COORD = 8, 256, 8192, 1 << 20, 16384
INFO_DTYPE = np.dtype([("image", "<i4"), ("row", "<i4"), ("wx0", "<i4"), ("wy0", "<i4"), ("S", "<i4"), ("inside256", "<i4"),
                       ("flags", "<i4"), ("reserved", "<i4"), ("sharp", "<i8")])
BEST_DTYPE = np.dtype([("id", "<i4"), ("frame", "<i4"), ("image_wx0", "<i4"), ("image_wy0", "<i4"), ("S", "<i4"),
                       ("inside256", "<i4"), ("seen", "<i4"), ("reserved", "<i4"), ("sharp", "<i8")])
assert INFO_DTYPE.itemsize == 40 and BEST_DTYPE.itemsize == 40


def axis_taps(u, S, C):
    """Rule 3 for chip column u: [(window index, weight), ..] and D."""
    if S >= C:
        taps = []
        for i in range((u * S) // C, S):
            w = min((i + 1) * C, (u + 1) * S) - max(i * C, u * S)
            if w <= 0:
                break
            taps.append((i, w))
        return taps, S
    t = (2 * u + 1) * S - C
    i0 = t // (2 * C)                                        # floor division, may be -1
    f = t - i0 * 2 * C
    return [(min(max(i0, 0), S - 1), 2 * C - f), (min(max(i0 + 1, 0), S - 1), f)], 2 * C


def axis_weights(S, C):
    """-> ([C,S] int64 weight matrix, D).  Taps that clamp onto one index add up."""
    Wm = np.zeros((C, S), np.int64)
    if S >= C:                                               # the same as axis_taps, for all u and i at once
        i = np.arange(S, dtype=np.int64)[None, :]
        u = np.arange(C, dtype=np.int64)[:, None]
        Wm[:] = np.maximum(np.minimum((i + 1) * C, (u + 1) * S) - np.maximum(i * C, u * S), 0)
        return Wm, S
    for u in range(C):
        for i, w in axis_taps(u, S, C)[0]:
            Wm[u, i] += w
    return Wm, 2 * C


def image_weights(S, C, w0, W):
    """-> ([C,W] int64, D): axis_weights with rule 4's clamped gather folded in."""
    Wm, D = axis_weights(S, C)
    cols = np.clip(w0 + np.arange(S, dtype=np.int64), 0, W - 1)
    A = np.zeros((W, C), np.int64)
    np.add.at(A, cols, Wm.T)
    return A.T.copy(), D


def window(row, W, H, margin256):
    """Rules 1 + 2 -> (wx0, wy0, S), or None for an invalid row."""
    v = np.asarray(row, np.float32)
    if not np.isfinite(v).all():
        return None
    with np.errstate(over="ignore"):
        c = [np.rint(v[1]), np.rint(v[2]), np.rint(np.float32(v[1] + v[3])), np.rint(np.float32(v[2] + v[4]))]
    if not all(np.isfinite(q) and abs(float(q)) <= MAX_COORD for q in c):
        return None
    X1, Y1, X2, Y2 = (int(q) for q in c)
    if X2 - X1 < 1 or Y2 - Y1 < 1 or not (X2 > 0 and X1 < W and Y2 > 0 and Y1 < H):
        return None
    side = max(X2 - X1, Y2 - Y1)
    S = side + 2 * ((side * margin256 + 128) >> 8)
    if S > MAX_SIDE:
        return None
    return (X1 + X2 - S) >> 1, (Y1 + Y2 - S) >> 1, S


def luma(chip):
    c = chip.astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def sharpness(chip):
    """Rule 6 on an (C,C,3) uint8 chip -> Python int."""
    L = luma(chip)
    lap = 4 * L[1:-1, 1:-1] - L[:-2, 1:-1] - L[2:, 1:-1] - L[1:-1, :-2] - L[1:-1, 2:]
    return int((lap * lap).sum())


def cut(image, wx0, wy0, S, C):
    """Rules 3 + 4: the (C,C,3) uint8 chip of the window of an (H,W,3) uint8 image."""
    H, W = image.shape[:2]
    Ay, D = image_weights(S, C, wy0, H)
    Ax, _ = image_weights(S, C, wx0, W)
    out = np.zeros((C, C, 3), np.uint8)
    for ch in range(3):
        acc = Ay @ image[:, :, ch].astype(np.int64) @ Ax.T
        out[:, :, ch] = (acc + (D * D) // 2) // (D * D)
    return out


def extract(images, rows, counts, C, margin256, planar=0):
    """images: list of (H,W,3) uint8; rows (n,K,5); counts (n,) -> (chips (M,C,C,3) | (M,3,C,C) uint8, info (M,) records,
    offset (n+1,) int32)."""
    rows = np.asarray(rows, np.float32)
    counts = np.asarray(counts, np.int64)
    n = len(images)
    assert MIN_SIZE <= C <= MAX_SIZE and 0 <= margin256 <= 256 and rows.shape[0] == n and (counts >= 0).all() and (counts <= rows.shape[1]).all()
    offset = np.zeros(n + 1, np.int32)
    offset[1:] = np.cumsum(counts)
    M = int(offset[-1])
    chips = np.zeros((M, C, C, 3), np.uint8)
    info = np.zeros(M, INFO_DTYPE)
    for i in range(n):
        H, W = images[i].shape[:2]
        for j in range(int(counts[i])):
            m = int(offset[i]) + j
            info[m]["image"], info[m]["row"] = i, j
            win = window(rows[i, j], W, H, margin256)
            if win is None:
                continue
            wx0, wy0, S = win
            chips[m] = cut(images[i], wx0, wy0, S, C)
            inside = max(0, min(wx0 + S, W) - max(wx0, 0)) * max(0, min(wy0 + S, H) - max(wy0, 0))
            info[m]["wx0"], info[m]["wy0"], info[m]["S"] = wx0, wy0, S
            info[m]["inside256"] = (inside * 256) // (S * S)
            info[m]["flags"] = 1
            info[m]["sharp"] = sharpness(chips[m])
    if planar:
        chips = np.ascontiguousarray(chips.transpose(0, 3, 1, 2))
    return chips, info, offset


def fresh_gallery(n_seq, G, C):
    return np.zeros((n_seq, G), BEST_DTYPE), np.zeros((n_seq, G, C * C * 3), np.uint8)


def best_update(chips, info, ids, seq_offset, frame_base, gallery, gallery_chips, min_side=0, min_inside256=0):
    """fdet_chip_best_update, one chip after the other; gallery (n_seq,G) records and gallery_chips (n_seq,G,C*C*3) are
    modified in place -> the number of candidates whose id is beyond G."""
    n_seq, G = gallery.shape
    ids = np.asarray(ids, np.int32)
    K = ids.shape[1]
    overflow = 0
    cand = {}                                                # (seq, id) -> chip indices, ascending
    for i in range(len(info)):
        f = info[i]
        if not f["flags"] & 1:
            continue
        t = int(f["image"])
        k = int(ids[t, int(f["row"])]) if K else 0
        if k < 1 or f["S"] < min_side or f["inside256"] < min_inside256:
            continue
        if k > G:
            overflow += 1
            continue
        s = max(q for q in range(n_seq) if seq_offset[q] <= t)            # the last sequence that starts at or before t
        cand.setdefault((s, k), []).append(i)
    for (s, k), members in cand.items():
        win = members[0]
        for i in members[1:]:
            if info[i]["sharp"] > info[win]["sharp"]:        # strictly: ties stay with the lower index
                win = i
        e = gallery[s, k - 1]
        if e["id"] == 0 or info[win]["sharp"] > e["sharp"]:
            f = info[win]
            e["id"], e["frame"] = k, int(frame_base[s]) + int(f["image"]) - int(seq_offset[s])
            e["image_wx0"], e["image_wy0"], e["S"], e["inside256"], e["sharp"] = f["wx0"], f["wy0"], f["S"], f["inside256"], f["sharp"]
            gallery_chips[s, k - 1] = chips[win].reshape(-1)
        e["seen"] += len(members)
    return overflow
