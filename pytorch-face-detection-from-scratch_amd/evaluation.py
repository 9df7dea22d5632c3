"""Dataset-level detection evaluation: precision/recall curve and average precision over a whole validation set.

The reference's only quality numbers are the step metrics of `ModelMeta.step` (one batch, one score threshold, ground
truth decoded back from the target grid).  `DetectionEvaluator` keeps score-binned true/false-positive histograms on
the device, fed by one HIP kernel per batch (csrc/fdet_eval.hip, `hotpath.eval_match`) from what the package already has
there: the `(rows, counts)` pair of a reducer's `forward_batch` and the true boxes of `DeviceBatches` (`GtBoxes`).

    ev = DetectionEvaluator(iou_thresholds=(0.5,))
    for x, y, gt in val_batches:
        ev.evaluate_batch(model, model(x), gt)          # no host synchronisation
    r = ev.compute()                                    # one device-to-host copy; r.ap, r.best_f1, r.at(0.5)

Matching is the PASCAL VOC / WIDER Face rule (include/fdet.h, fdet_eval_match); scores are binned into `n_bins` equal
bins of [0, 1] (1000: the number of score thresholds of the WIDER protocol) and the curve has one point per bin edge.
DESIGN.md 5b says how this differs from the official WIDER tool.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hotpath as hp


def voc_ap(recall: np.ndarray, precision: np.ndarray) -> float:
    """All-point interpolated AP of the VOC / WIDER tools: precision made monotone from the right, summed over the recall
    steps.  `recall` ascending, float64."""
    mrec = np.concatenate(([0.0], np.asarray(recall, np.float64), [1.0]))
    mpre = np.concatenate(([0.0], np.asarray(precision, np.float64), [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


class EvalResult:
    """Host-side result of `DetectionEvaluator.compute()`.  Index b of `precision[t]` / `recall[t]` is the operating point
    "keep detections with score >= b / n_bins"."""

    def __init__(self, tp: np.ndarray, fp: np.ndarray, n_gt: int, n_images: int, n_det: int, iou_thresholds: np.ndarray):
        self.tp, self.fp = tp.astype(np.int64), fp.astype(np.int64)
        self.n_gt, self.n_images, self.n_det = int(n_gt), int(n_images), int(n_det)
        self.iou_thresholds = np.asarray(iou_thresholds)
        self.n_bins = tp.shape[1]
        self.cum_tp = np.cumsum(self.tp[:, ::-1], axis=1)[:, ::-1].astype(np.float64)       # from the highest bin down
        self.cum_fp = np.cumsum(self.fp[:, ::-1], axis=1)[:, ::-1].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.precision = self.cum_tp / (self.cum_tp + self.cum_fp)                      # NaN where nothing is kept
            self.recall = self.cum_tp / float(self.n_gt) if self.n_gt else np.full_like(self.cum_tp, np.nan)
            self.f1 = 2 * self.precision * self.recall / (self.precision + self.recall)
        self.ap_per_threshold = np.full(len(self.iou_thresholds), np.nan)
        if self.n_gt:
            for t in range(len(self.iou_thresholds)):
                keep = (self.cum_tp[t] + self.cum_fp[t]) > 0                                # bins above the top score
                self.ap_per_threshold[t] = voc_ap(self.recall[t][keep][::-1], self.precision[t][keep][::-1])
        self.ap = float(self.ap_per_threshold[0])
        self.mean_ap = float(np.mean(self.ap_per_threshold))
        f = np.where(np.isnan(self.f1[0]), -1.0, self.f1[0])
        self.best_bin = int(self.n_bins - 1 - np.argmax(f[::-1]))          # ties: the highest score threshold
        self.best_f1 = float(f[self.best_bin]) if f[self.best_bin] >= 0 else float("nan")
        self.best_threshold = self.best_bin / self.n_bins

    def at(self, score_threshold: float, t: int = 0) -> dict:
        """Precision / recall / F1 of "score >= score_threshold" at IoU threshold number `t`: exact when the threshold is a
        multiple of 1/n_bins (as compared in fp32: the bin of a score is floorf(score * n_bins)), otherwise the bin edge at
        or below it."""
        b = min(self.n_bins - 1, max(0, int(np.floor(np.float32(score_threshold) * np.float32(self.n_bins)))))
        return {"bin": b, "tp": int(self.cum_tp[t, b]), "fp": int(self.cum_fp[t, b]), "precision": float(self.precision[t, b]),
                "recall": float(self.recall[t, b]), "f1": float(self.f1[t, b])}

    def to_json(self) -> dict:
        nan = lambda a: [None if x != x else float(x) for x in a]      # noqa: E731  (JSON has no NaN)
        return {"iou_thresholds": [float(t) for t in self.iou_thresholds], "n_bins": self.n_bins, "n_gt": self.n_gt,
                "n_images": self.n_images, "n_detections": self.n_det, "ap": nan(self.ap_per_threshold),
                "mean_ap": None if self.mean_ap != self.mean_ap else self.mean_ap,
                "best_f1": None if self.best_f1 != self.best_f1 else self.best_f1, "best_threshold": self.best_threshold,
                "precision": [nan(p) for p in self.precision], "recall": [nan(r) for r in self.recall],
                "tp": self.tp.tolist(), "fp": self.fp.tolist()}


def _pack_gt(gt, device):
    """GtBoxes | (rows, box_offset) | list of per-image (n,5) tensors -> (rows (cap,5) f32, box_offset (B+1,) int32)."""
    if hasattr(gt, "rows") and hasattr(gt, "box_offset"):
        return gt.rows, gt.box_offset
    if isinstance(gt, tuple) and len(gt) == 2 and all(isinstance(g, torch.Tensor) for g in gt) and gt[1].dtype == torch.int32:
        return gt
    mats = [np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float32).reshape(-1, 5) for b in gt]
    offs = np.zeros(len(mats) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([m.shape[0] for m in mats])
    cap = max(int(offs[-1]), 1)
    packed = np.zeros((cap * 5 + len(offs),), dtype=np.float32)      # rows and offsets in one buffer: one copy
    if offs[-1]:
        packed[:cap * 5] = np.concatenate(mats, 0).reshape(-1)
    packed[cap * 5:] = offs.view(np.float32)
    d = torch.from_numpy(packed).pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" \
        else torch.from_numpy(packed)
    return d[:cap * 5].view(cap, 5), d[cap * 5:].view(torch.int32)


class DetectionEvaluator:
    """Accumulates a validation set's detections against its true boxes; `compute()` gives the curve and AP.

    iou_thresholds: up to 10 IoU thresholds (AP is reported per threshold; `ap` is the first, `mean_ap` their mean);
    n_bins: score bins over [0, 1]; score_floor: the probability threshold of the reducers `evaluate_batch` builds (a PR
    curve needs the low-score detections the model's own operating threshold drops)."""

    def __init__(self, iou_thresholds: Sequence[float] = (0.5,), n_bins: int = 1000, device="cuda", score_floor: float = 0.01):
        self.state = hp.EvalState(iou_thresholds, n_bins, device)
        self.score_floor = float(score_floor)
        self._reducers: dict = {}

    iou_thresholds = property(lambda self: self.state.iou_thresholds)
    n_bins = property(lambda self: self.state.n_bins)
    device = property(lambda self: self.state.device)

    def reset(self) -> None:
        self.state.zero_()

    def update(self, pred_rows: torch.Tensor, pred_counts: torch.Tensor, gt, max_gt: Optional[int] = None,
               want_match: bool = False):
        """Add one batch: (pred_rows (B,Kmax,5), pred_counts (B,)) from `forward_batch`, `gt` a GtBoxes, a
        (rows, box_offset) pair or a list of per-image (n,5) [conf,x,y,w,h] tensors.  One kernel launch, no host
        synchronisation."""
        rows, offs = _pack_gt(gt, pred_rows.device)
        return hp.eval_match(pred_rows, pred_counts.to(torch.int32), rows, offs, self.state, max_gt, want_match)

    def reducer_for(self, model):
        """The evaluator's own reducer for `model`: the model's geometry and NMS IoU threshold, probability_threshold =
        score_floor.  `model.reduce_bounding_boxes` is left alone."""
        from .datasets.utils import ReduceBoundingBoxes, ReduceSSDBoundingBoxes
        own = model.reduce_bounding_boxes
        key = (id(model), float(own.iou_threshold))
        red = self._reducers.get(key)
        if red is None:
            if isinstance(own, ReduceSSDBoundingBoxes):
                red = ReduceSSDBoundingBoxes(probability_threshold=self.score_floor, iou_threshold=own.iou_threshold,
                                             input_shape=own.input_shape, patch_sizes=own.patch_sizes, priors=own.priors,
                                             with_priors=own.with_priors)
            elif isinstance(own, ReduceBoundingBoxes):
                red = ReduceBoundingBoxes(probability_threshold=self.score_floor, iou_threshold=own.iou_threshold,
                                          input_shape=own.input_shape, num_of_patches=own.num_of_patches)
            else:
                raise TypeError(f"no evaluation reducer for {type(own).__name__}")
            self._reducers[key] = red
        return red

    @torch.no_grad()
    def evaluate_batch(self, model, y_hat: torch.Tensor, gt, want_match: bool = False):
        """Reduce the head output `y_hat` of `model` at `score_floor` and add the batch.  No host synchronisation."""
        rows, counts = self.reducer_for(model).forward_batch(y_hat.detach())
        return self.update(rows, counts, gt, want_match=want_match)

    def merge(self, other: "DetectionEvaluator") -> "DetectionEvaluator":
        """Add `other`'s state (same thresholds and bins) to this one's."""
        a, b = self.state, other.state
        if a.n_bins != b.n_bins or not np.array_equal(a.iou_thresholds, b.iou_thresholds):
            raise ValueError("merge: evaluators with different IoU thresholds or bins")
        a.hist += b.hist.to(a.device)                      # int32 wrap-around == uint32 addition
        a.counters += b.counters.to(a.device)
        return self

    def all_reduce(self, group=None) -> "DetectionEvaluator":
        """Sum the integer state over the ranks of `group` (torch.distributed), so every rank computes the curve of the whole
        validation set.  The histograms travel as int64; a bin that does not fit uint32 afterwards raises."""
        import torch.distributed as dist
        s = self.state
        wide = torch.cat([(s.hist.reshape(-1).to(torch.int64) & 0xFFFFFFFF), s.counters])
        dist.all_reduce(wide, op=dist.ReduceOp.SUM, group=group)
        h = wide[:-4]
        if int(h.max()) > 0xFFFFFFFF:
            raise OverflowError("all_reduce: a histogram bin exceeds 32 bits")
        s.hist.copy_(torch.where(h > 0x7FFFFFFF, h - (1 << 32), h).to(torch.int32).view_as(s.hist))
        s.counters.copy_(wide[-4:])
        return self

    def compute(self) -> EvalResult:
        """One device-to-host copy, then float64 on the host: cumulative TP/FP from the highest bin down, precision and recall
        per bin edge, all-point interpolated AP per IoU threshold, best F1.  With no ground truth AP is NaN."""
        s = self.state
        flat = torch.cat([s.hist.reshape(-1).to(torch.int64) & 0xFFFFFFFF, s.counters]).cpu().numpy()
        c = flat[-4:]
        if c[hp.EVAL_N_REJECTED]:
            raise hp.N.FdetError(f"evaluation: {int(c[hp.EVAL_N_REJECTED])} image(s) exceeded what the kernel launch was sized "
                                 f"for (detections > Kmax, boxes > max_gt or offsets outside the rows): pass max_gt to update()")
        h = flat[:-4].reshape(2, s.T, s.n_bins)
        return EvalResult(h[0], h[1], c[hp.EVAL_N_GT], c[hp.EVAL_N_IMAGES], c[hp.EVAL_N_DET], s.iou_thresholds)
