"""numpy restatement of tiled detection (fdet_amd/tiling.py, csrc/fdet_tiles.hip), written from the rules of DESIGN.md 5c:
the tile plan as a closed form and a literal loop, the gather through the warp restatement of tests/aug_cpu_ref.py (a window
is a crop), and the cross-window merge as the plain sequential loop in float32 with the kernel's operation order, so rows
compare exactly.  The reference project has no counterpart.  Not a test module: tests import it.
"""
import math

import numpy as np

import aug_cpu_ref as R

f32 = np.float32
MAX_CANDIDATES = 4864


# ---------------------------------------------------------------------------------------------------------------- plan
def stride_of(t, overlap):
    return max(1, t - int(math.floor(overlap * t + 0.5)))


def origins(L, t, stride):
    if L <= t:
        return [0]
    out, k = [], 0
    while k * stride < L - t:
        out.append(k * stride)
        k += 1
    out.append(L - t)
    return out


def n_origins(L, t, stride):
    """closed form: 1 for L <= t, else ceil((L - t) / stride) + 1"""
    return 1 if L <= t else (L - t + stride - 1) // stride + 1


def plan(sizes, tile_sizes=(480,), overlap=0.25, include_whole=True):
    """-> (list of (image, x0, y0, w, h), offsets)"""
    recs, offs = [], [0]
    for i, (h, w) in enumerate(np.asarray(sizes).reshape(-1, 2).tolist()):
        mine = [(i, 0, 0, w, h)] if include_whole else []
        for t in tile_sizes:
            s = stride_of(t, overlap)
            for y0 in origins(h, t, s):
                for x0 in origins(w, t, s):
                    rec = (i, x0, y0, min(t, w), min(t, h))
                    if rec == (i, 0, 0, w, h) and rec in mine:
                        continue
                    mine.append(rec)
        recs += mine
        offs.append(len(recs))
    return recs, offs


# -------------------------------------------------------------------------------------------------------------- gather
def gather_values(img, win, Ho, Wo):
    """float64 (3,Ho,Wo) value before the rint/clamp: the warp with only a crop set.  img (H,W,3) uint8, win (x0,y0,w,h)."""
    P = {"flags": 0, "crop_x0": win[0], "crop_y0": win[1], "crop_w": win[2], "crop_h": win[3]}
    return R.warp_values(img, P, Ho, Wo, 0)


def gather(img, win, Ho, Wo):
    return R.to_u8(gather_values(img, win, Ho, Wo))


# --------------------------------------------------------------------------------------------------------------- merge
def to_source(d, win, Ho, Wo):
    """[score,x,y,w,h] in frame pixels of window (x0,y0,w,h) -> source pixels, float32, half-to-even."""
    kx, ky = f32(win[2]) / f32(Wo), f32(win[3]) / f32(Ho)
    x = np.rint(f32(win[0]) + f32(d[1]) * kx)
    y = np.rint(f32(win[1]) + f32(d[2]) * ky)
    w = np.rint(f32(d[3]) * kx)
    h = np.rint(f32(d[4]) * ky)
    return f32(x), f32(y), f32(w), f32(h)


def cut_by_window(d, win, img_hw, Ho, Wo, margin):
    """the edge rule: within `margin` frame pixels of a window side that is not a side of the image"""
    if not margin > 0:
        return False
    x0, y0, ww, wh = win
    m = f32(margin)
    x, y = f32(d[1]), f32(d[2])
    x2, y2 = f32(x + f32(d[3])), f32(y + f32(d[4]))
    return bool((x0 > 0 and x < m) or (x0 + ww < img_hw[1] and x2 > f32(Wo) - m) or
                (y0 > 0 and y < m) or (y0 + wh < img_hw[0] and y2 > f32(Ho) - m))


def _iou(a, b):
    """float32 overlap of two (x1,y1,x2,y2) boxes as torchvision 0.11.2's nms_kernel.cpp computes it"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        aa = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
        ab = f32(f32(b[2] - b[0]) * f32(b[3] - b[1]))
        w = max(f32(0), f32(min(a[2], b[2]) - max(a[0], b[0])))
        h = max(f32(0), f32(min(a[3], b[3]) - max(a[1], b[1])))
        inter = f32(w * h)
        return f32(inter / f32(f32(aa + ab) - inter))


def _candidates(rows, counts, wins, Ho, Wo, img_hw, margin):
    """candidates of one image in (tile, row) order: (key, score, x, y, w, h)"""
    cand = []
    for t, win in enumerate(wins):
        for r in range(int(counts[t])):
            d = rows[t, r]
            if cut_by_window(d, win, img_hw, Ho, Wo, margin):
                continue
            s = f32(d[0])
            cand.append((f32(-np.inf) if np.isnan(s) else s, s) + to_source(d, win, Ho, Wo))
    return cand


def merge_image(rows, counts, wins, Ho, Wo, img_hw, margin, thr, K, Kout):
    """One image: rows (t,K,5) / counts (t,) of its windows `wins` -> ((k,5) float32 survivors in visiting order, rejected)."""
    none = np.zeros((0, 5), f32)
    if any(int(c) < 0 or int(c) > K for c in counts):
        return none, True
    cand = _candidates(rows, counts, wins, Ho, Wo, img_hw, margin)
    if len(cand) > MAX_CANDIDATES:
        return none, True
    order = sorted(range(len(cand)), key=lambda i: (-cand[i][0], i))      # stable descending; ties by (tile, row)
    c = np.array([cand[i] for i in order], f32).reshape(-1, 6)             # in visiting order
    x1, y1 = c[:, 2], c[:, 3]
    x2, y2 = x1 + c[:, 4], y1 + c[:, 5]                                    # float32 sums
    area = (x2 - x1) * (y2 - y1)
    dead = np.zeros(len(order), bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a in range(len(order)):
            if dead[a]:
                continue
            keep.append(order[a])
            w = np.maximum(f32(0), np.minimum(x2[a], x2[a + 1:]) - np.maximum(x1[a], x1[a + 1:]))
            h = np.maximum(f32(0), np.minimum(y2[a], y2[a + 1:]) - np.maximum(y1[a], y1[a + 1:]))
            inter = w * h
            ovr = inter / (area[a] + area[a + 1:] - inter)                 # float32 throughout; 0/0 = NaN
            dead[a + 1:] |= ovr.astype(np.float64) > thr                    # NaN > thr is False
    if len(keep) > Kout:
        return none, True
    return np.array([cand[i][1:] for i in keep], f32).reshape(-1, 5), False


def merge_image_bruteforce(rows, counts, wins, Ho, Wo, img_hw, margin, thr, K, Kout):
    """The same result the O(n^2) way: a candidate survives iff no SURVIVING candidate earlier in the order overlaps it by
    more than thr, decided by recursion on the order instead of the running dead flags."""
    none = np.zeros((0, 5), f32)
    if any(int(c) < 0 or int(c) > K for c in counts):
        return none, True
    cand = _candidates(rows, counts, wins, Ho, Wo, img_hw, margin)
    if len(cand) > MAX_CANDIDATES:
        return none, True
    n = len(cand)
    keys = np.array([c[0] for c in cand], np.float64)
    order = np.lexsort((np.arange(n), -keys))
    xyxy = [(c[2], c[3], f32(c[2] + c[4]), f32(c[3] + c[5])) for c in cand]
    alive = np.zeros(n, bool)
    for a in range(n):
        alive[a] = not any(alive[b] and float(_iou(xyxy[order[b]], xyxy[order[a]])) > thr for b in range(a))
    keep = [order[a] for a in range(n) if alive[a]]
    if len(keep) > Kout:
        return none, True
    return np.array([cand[i][1:] for i in keep], f32).reshape(-1, 5), False


def merge(rows, counts, tiles, tile_offset, sizes, Ho, Wo, margin, thr, Kout, one=merge_image):
    """All images: tiles = list of (image, x0, y0, w, h); sizes (n,2) (h,w).  -> (out (n,Kout,5), out_counts (n,), rejected)"""
    rows, counts = np.asarray(rows, f32), np.asarray(counts)
    n, K = len(tile_offset) - 1, rows.shape[1]
    out, cnt, rej = np.zeros((n, Kout, 5), f32), np.zeros(n, np.int32), 0
    for i in range(n):
        a, b = int(tile_offset[i]), int(tile_offset[i + 1])
        wins = [tuple(int(v) for v in tiles[t])[1:] for t in range(a, b)]
        kept, bad = one(rows[a:b], counts[a:b], wins, Ho, Wo, tuple(int(v) for v in sizes[i]), margin, thr, K, Kout)
        if bad:
            rej += 1
            continue
        out[i, :len(kept)] = kept
        cnt[i] = len(kept)
    return out, cnt, rej
