"""numpy float64 restatement of the WIDER Face protocol evaluation (fdet_eval_wider + WiderEvaluator.compute) as the
SEQUENTIAL loop the protocol's published tools run per image: walk the detections in descending score, keep
`recall_list[g]` in {0, 1, -1}, record `pred_recall[h]` and `proposal_list[h]`, then read both off at the last detection
above each of the n_bins thresholds.  A test helper like eval_cpu_ref.py; not part of the package; needs no GPU and,
but for `write_mats`, no scipy."""
import os

import numpy as np

F = np.float32
D = np.float64


def visiting_order(scores):
    s = np.asarray(scores, F)
    s = np.where(np.isnan(s), F(-np.inf), s) + F(0)
    return np.lexsort((np.arange(len(s)), -s.astype(D)))               # descending score, ties by ascending row


def _lt(a, b):
    return np.where(a < b, a, b)                                        # min(a, b) = a < b ? a : b


def _gt(a, b):
    return np.where(a > b, a, b)


def overlap_matrix(det, gt, scale=(1.0, 1.0)):
    """(K,4) x (G,4) [x,y,w,h] -> (K,G) float64 overlaps with inclusive (+1) pixel coordinates.  Detections are scaled to
    source pixels by four fp32 multiplies first; every later operation is a float64 one in the kernel's order."""
    det, gt = np.asarray(det, F).reshape(-1, 4), np.asarray(gt, F).reshape(-1, 4)
    sx, sy = F(scale[0]), F(scale[1])
    fx, fy, fw, fh = (det[:, 0] * sx).astype(F), (det[:, 1] * sy).astype(F), (det[:, 2] * sx).astype(F), (det[:, 3] * sy).astype(F)
    dx1, dy1 = fx.astype(D)[:, None], fy.astype(D)[:, None]
    dx2, dy2 = dx1 + fw.astype(D)[:, None], dy1 + fh.astype(D)[:, None]
    gx1, gy1 = gt[None, :, 0].astype(D), gt[None, :, 1].astype(D)
    gx2, gy2 = gx1 + gt[None, :, 2].astype(D), gy1 + gt[None, :, 3].astype(D)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ad = (dx2 - dx1 + 1.0) * (dy2 - dy1 + 1.0)
        ag = (gx2 - gx1 + 1.0) * (gy2 - gy1 + 1.0)
        iw = _lt(dx2, gx2) - _gt(dx1, gx1) + 1.0
        ih = _lt(dy2, gy2) - _gt(dy1, gy1) + 1.0
        inter = iw * ih
        ov = inter / (ad + ag - inter)
    return np.where((iw > 0) & (ih > 0), ov, 0.0)


def thresholds(n_bins):
    return np.array([1.0 - D(t + 1) / D(n_bins) for t in range(n_bins)], D)


def normalise(scores, norm):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (np.asarray(scores, F).astype(D) - D(norm[0])) / D(norm[1])


def image_eval(det_rows, gt_rows, keep, iou_threshold, n_bins, norm=(0.0, 1.0), scale=(1.0, 1.0)):
    """One image, one subset.  det_rows (K,5) [score,x,y,w,h]; gt_rows (G,5) [conf,x,y,w,h]: ALL boxes; keep (G,) bool.
    -> (n_bins,2) int64: per threshold t the number of proposals and of recalled boxes among the detections up to the last
    one with normalised score >= 1-(t+1)/n_bins (the protocol's img_pr_info)."""
    det_rows, gt_rows = np.asarray(det_rows, F).reshape(-1, 5), np.asarray(gt_rows, F).reshape(-1, 5)
    K, G = len(det_rows), len(gt_rows)
    out = np.zeros((n_bins, 2), np.int64)
    if K == 0:
        return out
    order = visiting_order(det_rows[:, 0])
    det = det_rows[order]
    M = overlap_matrix(det[:, 1:], gt_rows[:, 1:], scale)
    M = np.where(np.isnan(M), -np.inf, M)
    recall_list = np.zeros(G, np.int64)
    proposal_list = np.ones(K, np.int64)
    pred_recall = np.zeros(K, np.int64)
    for h in range(K):
        if G:
            g = int(np.argmax(M[h]))                                    # first maximum: lowest row on ties
            if M[h, g] > -np.inf and M[h, g] >= iou_threshold:
                if not keep[g]:
                    recall_list[g] = -1
                    proposal_list[h] = -1
                elif recall_list[g] == 0:
                    recall_list[g] = 1
        pred_recall[h] = int((recall_list == 1).sum())
    n = normalise(det[:, 0], norm)
    n_prop = np.cumsum(proposal_list == 1)                              # #(proposal_list[:r+1] == 1)
    with np.errstate(invalid="ignore"):
        ge = n[None, :] >= thresholds(n_bins)[:, None]                  # (n_bins, K)
    some = ge.any(1)
    last = K - 1 - np.argmax(ge[:, ::-1], 1)                            # the LAST detection at or above the threshold
    out[some, 0] = n_prop[last[some]]
    out[some, 1] = pred_recall[last[some]]
    return out


def evaluate(pred, counts, gt_rows, gt_offset, masks, n_subsets, iou_threshold=0.5, n_bins=1000, norm=(0.0, 1.0), scale=None):
    """A batch in the kernel's layout -> (proposals (S,n_bins), hits (S,n_bins), n_faces (S,)): the per-threshold sums of
    `image_eval` over the images, differenced over t so that they compare with the kernel's histograms."""
    pred = np.asarray(pred, F)
    B = pred.shape[0]
    cum = np.zeros((n_subsets, n_bins, 2), np.int64)
    n_faces = np.zeros(n_subsets, np.int64)
    for i in range(B):
        K, g0, g1 = int(counts[i]), int(gt_offset[i]), int(gt_offset[i + 1])
        sc = (1.0, 1.0) if scale is None else scale[i]
        for s in range(n_subsets):
            keep = ((np.asarray(masks[g0:g1], np.uint32) >> np.uint32(s)) & np.uint32(1)).astype(bool)
            n_faces[s] += int(keep.sum())
            cum[s] += image_eval(pred[i, :K], gt_rows[g0:g1], keep, iou_threshold, n_bins, norm, sc)
    hist = np.diff(cum, axis=1, prepend=0)
    return hist[:, :, 0], hist[:, :, 1], n_faces


def voc_ap(recall, precision):
    """voc_ap of the VOC / WIDER evaluation tools (all-point interpolation), float64, written as their loop."""
    mrec = np.concatenate(([0.0], np.asarray(recall, D), [1.0]))
    mpre = np.concatenate(([0.0], np.asarray(precision, D), [0.0]))
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap


def curve(proposals, hits, n_faces):
    """One subset's histograms -> (precision, recall, ap): cumulative over the thresholds; no proposal -> precision 0."""
    cp, ch = np.cumsum(proposals).astype(D), np.cumsum(hits).astype(D)
    precision = np.where(cp > 0, ch / np.where(cp > 0, cp, 1.0), 0.0)
    if n_faces == 0:
        return precision, np.full(len(cp), np.nan), float("nan")
    recall = ch / D(n_faces)
    return precision, recall, voc_ap(recall, precision)


def score_min_max(pred, counts):
    """(min, max) of the protocol's norm_score: min starts at 1, max at 0; NaN scores are not looked at."""
    lo, hi = D(1.0), D(0.0)
    for i in range(len(counts)):
        s = np.asarray(pred[i, :int(counts[i]), 0], F).astype(D)
        s = s[~np.isnan(s)]
        if len(s):
            lo, hi = min(lo, s.min()), max(hi, s.max())
    return float(lo), float(hi)


def score_range(pred, counts):
    """(min, max - min): what fdet_eval_wider takes as score_norm."""
    lo, hi = score_min_max(pred, counts)
    return lo, hi - lo


def random_batch(rng, B, Kmax, max_det, max_gt, n_subsets, size=480, empty_det=(), empty_gt=(), all_ignored=(), big=None, scale=None):
    """Random batch in the kernel's layout with subset masks.  Scores quantised to two decimals (ties straddle the
    thresholds); half of an image's detections are jittered copies of its boxes, a few are exact copies listed twice
    (duplicates on a recalled face); rows unsorted; about a third of the boxes are ignored in each subset.
    `scale` (B,2): the detections are stored divided by it, so that scaled back they sit on the boxes again."""
    pred = np.zeros((B, Kmax, 5), F)
    counts = np.zeros(B, np.int32)
    gts, ms, offs = [], [], [0]
    for n in range(B):
        G = 0 if n in empty_gt else int(rng.integers(1, max_gt + 1))
        if big is not None and n == big[0]:
            G = big[1]
        K = 0 if n in empty_det else int(rng.integers(max(1, min(8, max_det)), max_det + 1))
        gt = np.round(np.c_[rng.uniform(0, size - 80, (G, 2)), rng.uniform(10, 80, (G, 2))])
        det = np.round(np.c_[rng.uniform(0, size - 80, (K, 2)), rng.uniform(10, 80, (K, 2))])
        if G and K:
            h = K // 2
            src = rng.integers(0, G, h)
            det[:h] = gt[src] + rng.integers(-6, 7, (h, 4))
            q = h // 4
            det[:q] = gt[src[:q]]                                       # exact copies ...
            det[q:2 * q] = gt[src[:q]]                                  # ... twice: the second is a duplicate
            det[:, 2:] = np.maximum(det[:, 2:], 1)
        pred[n, :K, 0] = np.round(rng.uniform(0, 1, K), 2)
        pred[n, :K, 1:] = det if scale is None else det / np.asarray(scale[n], np.float64)[[0, 1, 0, 1]]
        pred[n, K:] = rng.uniform(0, 1, (Kmax - K, 5))                  # slots past the count hold garbage
        counts[n] = K
        m = np.zeros(G, np.uint32)
        for s in range(n_subsets):
            m |= (rng.uniform(size=G) < 0.67).astype(np.uint32) << np.uint32(s)
        if n in all_ignored:
            m[:] = 0
        m |= rng.integers(0, 2, G).astype(np.uint32) << np.uint32(n_subsets + 3)   # bits the kernel must not read
        gts.append(np.c_[np.ones(G), gt].astype(F).reshape(-1, 5))
        ms.append(m)
        offs.append(offs[-1] + G)
    rows = np.concatenate(gts + [np.zeros((3, 5), F)], 0).astype(F)     # cap > total
    masks = np.concatenate(ms + [np.full(3, 0xFFFFFFFF, np.uint32)])
    return pred, counts, rows, np.asarray(offs, np.int32), masks


def exercised(pred, counts, gt_rows, gt_offset, masks, n_subsets, iou_threshold=0.5, scale=None):
    """What a batch exercises, by the restatement alone: detections swallowed by an ignored box, duplicate detections on
    a recalled box, and pairs of equal scores inside one image."""
    ignored = dup = ties = 0
    for i in range(len(counts)):
        K, g0, g1 = int(counts[i]), int(gt_offset[i]), int(gt_offset[i + 1])
        if K == 0:
            continue
        sc = np.asarray(pred[i, :K, 0], F)
        ties += K - len(np.unique(sc[~np.isnan(sc)]))
        if g1 == g0:
            continue
        order = visiting_order(sc)
        M = overlap_matrix(pred[i, :K, 1:][order], gt_rows[g0:g1, 1:], (1.0, 1.0) if scale is None else scale[i])
        M = np.where(np.isnan(M), -np.inf, M)
        g = np.argmax(M, 1)
        reach = M[np.arange(K), g] >= iou_threshold
        for s in range(n_subsets):
            keep = ((np.asarray(masks[g0:g1], np.uint32) >> np.uint32(s)) & np.uint32(1)).astype(bool)
            ignored += int((reach & ~keep[g]).sum())
            hit = g[reach & keep[g]]
            dup += len(hit) - len(np.unique(hit))
    return {"ignored_hits": ignored, "duplicates": dup, "ties": ties}


def write_mats(gt_dir, names, boxes, keeps):
    """The four files in the nested cell layout of the protocol's own: event_list {E,1}, file_list {E,1}{N,1},
    face_bbx_list {E,1}{N,1} (n,4) doubles, gt_list {E,1}{N,1} (k,1) 1-based indices.  keeps: {subset: per-image index lists}."""
    from scipy.io import savemat
    events = sorted({n.split("/")[0] for n in names})
    cell = lambda n: np.empty((n, 1), dtype=object)                      # noqa: E731
    ev, fl, bb = cell(len(events)), cell(len(events)), cell(len(events))
    gl = {k: cell(len(events)) for k in keeps}
    for e, event in enumerate(events):
        mine = [i for i, n in enumerate(names) if n.split("/")[0] == event]
        ev[e, 0] = np.array([event])
        fl[e, 0], bb[e, 0] = cell(len(mine)), cell(len(mine))
        for k in keeps:
            gl[k][e, 0] = cell(len(mine))
        for j, i in enumerate(mine):
            fl[e, 0][j, 0] = np.array([os.path.splitext(names[i].split("/")[1])[0]])
            bb[e, 0][j, 0] = np.asarray(boxes[i], np.float64).reshape(-1, 4)
            for k in keeps:
                gl[k][e, 0][j, 0] = (np.asarray(keeps[k][i], np.float64).reshape(-1, 1) + 1)
    os.makedirs(gt_dir, exist_ok=True)
    savemat(os.path.join(gt_dir, "wider_face_val.mat"), {"event_list": ev, "file_list": fl, "face_bbx_list": bb})
    for k in keeps:
        savemat(os.path.join(gt_dir, f"wider_{k}_val.mat"), {"gt_list": gl[k]})
