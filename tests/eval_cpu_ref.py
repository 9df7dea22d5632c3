"""numpy restatement of the detection evaluator (fdet_eval_match + DetectionEvaluator.compute): the SEQUENTIAL greedy
PASCAL VOC / WIDER Face matching loop, fp32 IoU in the operation order of the kernel, the score-bin formula, the tp/fp
histograms and the all-point interpolated AP.  A test helper like aug_cpu_ref.py; not part of the package."""
import numpy as np

F = np.float32


def iou_matrix(det, gt):
    """(K,4) x (G,4) [x,y,w,h] -> (K,G) fp32 box_iou on x, y, x+w, y+h (every operation rounded to fp32, no fusing)."""
    det, gt = np.asarray(det, F).reshape(-1, 4), np.asarray(gt, F).reshape(-1, 4)
    px1, py1 = det[:, None, 0], det[:, None, 1]
    px2, py2 = det[:, None, 2] + px1, det[:, None, 3] + py1
    gx1, gy1 = gt[None, :, 0], gt[None, :, 1]
    gx2, gy2 = gt[None, :, 2] + gx1, gt[None, :, 3] + gy1
    a1 = (gx2 - gx1) * (gy2 - gy1)
    a2 = (px2 - px1) * (py2 - py1)
    w = np.fmax(np.fmin(gx2, px2) - np.fmax(gx1, px1), F(0))
    h = np.fmax(np.fmin(gy2, py2) - np.fmax(gy1, py1), F(0))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / (a1 + a2 - inter)).astype(F)


def score_bin(scores, n_bins):
    s = np.asarray(scores, F)
    s = np.where(np.isnan(s), F(-np.inf), s)
    with np.errstate(invalid="ignore"):
        v = (s * F(n_bins)).astype(F)
    out = np.zeros(s.shape, np.int64)
    mid = (v >= 0) & (v < F(n_bins))
    out[mid] = np.floor(v[mid]).astype(np.int64)
    out[v >= F(n_bins)] = n_bins - 1
    return out


def visiting_order(scores):
    s = np.asarray(scores, F)
    s = np.where(np.isnan(s), F(-np.inf), s) + F(0)
    return np.lexsort((np.arange(len(s)), -s.astype(np.float64)))      # descending score, ties by ascending row


def match_image(det_rows, gt_rows, iou_thresholds):
    """det_rows (K,5) [score,x,y,w,h], gt_rows (G,5) [conf,x,y,w,h] -> tp (T,K) bool, match (T,K) box index or -1.
    The sequential loop: a detection's candidate is the box of highest IoU among ALL boxes; TP iff IoU >= threshold and
    the candidate is unclaimed."""
    det_rows = np.asarray(det_rows, F).reshape(-1, 5)
    gt_rows = np.asarray(gt_rows, F).reshape(-1, 5)
    K, G = len(det_rows), len(gt_rows)
    thr = np.asarray(iou_thresholds, F)
    tp = np.zeros((len(thr), K), bool)
    match = np.full((len(thr), K), -1, np.int64)
    if K == 0 or G == 0:
        return tp, match
    M = iou_matrix(det_rows[:, 1:], gt_rows[:, 1:])
    M = np.where(np.isnan(M), F(-np.inf), M)
    order = visiting_order(det_rows[:, 0])
    for t, th in enumerate(thr):
        used = np.zeros(G, bool)
        for d in order:
            g = int(np.argmax(M[d]))                        # first maximum: lowest index on ties
            if M[d, g] > F(-np.inf) and M[d, g] >= th and not used[g]:
                used[g] = True
                tp[t, d] = True
                match[t, d] = g
    return tp, match


def evaluate(pred, counts, gt_rows, gt_offset, iou_thresholds, n_bins):
    """A batch in the kernel's layout -> (tp hist (T,n_bins), fp hist, n_gt, match (B,Kmax) of the first threshold with
    indices into gt_rows)."""
    pred = np.asarray(pred, F)
    B, Kmax, _ = pred.shape
    T = len(iou_thresholds)
    htp, hfp = np.zeros((T, n_bins), np.int64), np.zeros((T, n_bins), np.int64)
    match = np.full((B, Kmax), -1, np.int64)
    n_gt = 0
    for n in range(B):
        K, g0, g1 = int(counts[n]), int(gt_offset[n]), int(gt_offset[n + 1])
        n_gt += g1 - g0
        tp, m = match_image(pred[n, :K], gt_rows[g0:g1], iou_thresholds)
        bins = score_bin(pred[n, :K, 0], n_bins)
        for t in range(T):
            np.add.at(htp[t], bins[tp[t]], 1)
            np.add.at(hfp[t], bins[~tp[t]], 1)
        match[n, :K] = np.where(m[0] >= 0, m[0] + g0, -1)
    return htp, hfp, n_gt, match


def voc_ap(recall, precision):
    """voc_ap of the VOC / WIDER evaluation tools (all-point interpolation), float64, written as their loop."""
    mrec = np.concatenate(([0.0], np.asarray(recall, np.float64), [1.0]))
    mpre = np.concatenate(([0.0], np.asarray(precision, np.float64), [0.0]))
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap


def ap_from_hist(htp, hfp, n_gt):
    """AP of one threshold's binned curve: cumulative counts from the highest bin down, empty leading bins dropped."""
    if n_gt == 0:
        return float("nan")
    ctp = np.cumsum(htp[::-1]).astype(np.float64)
    cfp = np.cumsum(hfp[::-1]).astype(np.float64)
    keep = (ctp + cfp) > 0
    return voc_ap(ctp[keep] / n_gt, ctp[keep] / (ctp[keep] + cfp[keep]))


def ap_exact(scores, is_tp, n_gt):
    """Brute-force AP over the exactly sorted detection list of a whole set (one curve point per detection)."""
    if n_gt == 0:
        return float("nan")
    order = visiting_order(scores)
    tp = np.cumsum(np.asarray(is_tp, bool)[order]).astype(np.float64)
    fp = np.cumsum(~np.asarray(is_tp, bool)[order]).astype(np.float64)
    return voc_ap(tp / n_gt, tp / (tp + fp))


def random_batch(rng, B, Kmax, max_det, max_gt, size=480, empty_det=(), empty_gt=(), big=None):
    """Random batch in the kernel's layout.  Scores quantised to two decimals (ties); half of an image's detections are
    jittered copies of its boxes (IoUs on both sides of every threshold); rows unsorted.  `big`: (image, G) forces one
    image to G boxes."""
    pred = np.zeros((B, Kmax, 5), F)
    counts = np.zeros(B, np.int32)
    gts, offs = [], [0]
    for n in range(B):
        G = 0 if n in empty_gt else int(rng.integers(0, max_gt + 1))
        if big is not None and n == big[0]:
            G = big[1]
        K = 0 if n in empty_det else int(rng.integers(0, max_det + 1))
        gt = np.round(np.c_[rng.uniform(0, size - 80, (G, 2)), rng.uniform(10, 80, (G, 2))])
        det = np.round(np.c_[rng.uniform(0, size - 80, (K, 2)), rng.uniform(10, 80, (K, 2))])
        if G and K:
            h = K // 2
            det[:h] = gt[rng.integers(0, G, h)] + rng.integers(-6, 7, (h, 4))
            det[:, 2:] = np.maximum(det[:, 2:], 1)
        pred[n, :K, 0] = np.round(rng.uniform(0, 1, K), 2)
        pred[n, :K, 1:] = det
        pred[n, K:] = rng.uniform(0, 1, (Kmax - K, 5))          # slots past the count hold garbage that must be ignored
        counts[n] = K
        gts.append(np.c_[np.ones(G), gt].astype(F).reshape(-1, 5))
        offs.append(offs[-1] + G)
    rows = np.concatenate(gts, 0) if offs[-1] else np.zeros((0, 5), F)
    rows = np.concatenate([rows, np.zeros((max(1, 3), 5), F)], 0)      # cap > total, as DeviceBatches allocates
    return pred, counts, rows.astype(F), np.asarray(offs, np.int32)
