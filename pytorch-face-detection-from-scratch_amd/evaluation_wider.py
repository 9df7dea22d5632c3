"""WIDER Face protocol evaluation: Easy / Medium / Hard average precision over a whole validation set.

`evaluation.DetectionEvaluator` applies the PASCAL VOC rule to every box.  The WIDER protocol is a different rule (boxes
outside a subset are ignored rather than missed, no uniqueness rule, inclusive pixel overlaps in source pixels, scores
min-max normalised over the data set and cut at 1000 thresholds); `WiderEvaluator` runs it on the device, all subsets in
one kernel launch per batch (csrc/fdet_eval_wider.hip, `hotpath.eval_wider`; the rule is spelled out in include/fdet.h).

    subsets, boxes = WiderSubsets.from_mat("wider_face_split", names)      # the four .mat files of the protocol
    gt = DeviceBoxes(boxes, "cuda")
    ev = WiderEvaluator()
    for idx in batches_of_bank_indices:
        rows, counts = detector.detect(bank, idx)                          # source pixels
        ev.update(rows, counts, subsets.batch(gt, idx))
    r = ev.compute()                                                        # r.ap["easy"], r.ap["medium"], r.ap["hard"]

DESIGN.md 5d says what is and what is not pinned against the protocol's published tools.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hotpath as hp
from .evaluation import voc_ap

MAT_FILES = {"easy": "wider_easy_val.mat", "medium": "wider_medium_val.mat", "hard": "wider_hard_val.mat"}


def image_key(name) -> str:
    """`.../<event>/<image>.jpg` -> `<event>/<image>`: the name the protocol's files use."""
    parts = str(name).replace("\\", "/").split("/")
    stem = os.path.splitext(parts[-1])[0]
    return f"{parts[-2]}/{stem}" if len(parts) > 1 and parts[-2] not in ("", ".") else stem


class WiderGt:
    """One batch of protocol ground truth on the device: rows (cap,5) [conf,x,y,w,h] of ALL boxes in source pixels,
    box_offset (B+1,) int32, subsets (cap,) int32 holding the uint32 subset masks."""

    def __init__(self, rows: torch.Tensor, box_offset: torch.Tensor, subsets: torch.Tensor, max_per_image: Optional[int] = None):
        self.rows, self.box_offset, self.subsets, self.max_per_image = rows, box_offset, subsets, max_per_image


class WiderSubsets:
    """Per image of a bank, a uint32 mask per ground-truth row: bit s set = the box is kept in subset s."""

    def __init__(self, masks: Sequence, subset_names: Sequence[str]):
        self.masks = [np.ascontiguousarray(np.asarray(m).reshape(-1), dtype=np.uint32) for m in masks]
        self.subset_names = tuple(subset_names)
        if not 1 <= len(self.subset_names) <= hp.EVAL_WIDER_MAX_SUBSETS:
            raise ValueError(f"{len(self.subset_names)} subsets, 1..{hp.EVAL_WIDER_MAX_SUBSETS} are supported")
        self._dev = {}
        self._offs = None

    def __len__(self) -> int:
        return len(self.masks)

    @classmethod
    def from_masks(cls, masks: Sequence, subset_names: Sequence[str] = ("easy", "medium", "hard")) -> "WiderSubsets":
        return cls(masks, subset_names)

    @classmethod
    def all_kept(cls, boxes: Sequence, subset_names: Sequence[str] = ("all",)) -> "WiderSubsets":
        """Every box kept in every subset (one subset by default): the protocol's rule without ignored boxes."""
        bits = (1 << len(subset_names)) - 1
        return cls([np.full(np.asarray(b).reshape(-1, 5).shape[0], bits, np.uint32) for b in boxes], subset_names)

    @classmethod
    def from_mat(cls, gt_dir, names: Sequence, subset_names: Sequence[str] = ("easy", "medium", "hard")):
        """Read `wider_face_val.mat` (event_list, file_list, face_bbx_list) and the subsets' `gt_list` files under `gt_dir`
        and map them to the images `names` (paths or `<event>/<image>` strings, in bank order).
        -> (WiderSubsets, per-image (n,5) float32 [1,x,y,w,h] boxes: the FULL face_bbx_list the 1-based gt_list indexes)."""
        from scipy.io import loadmat
        gt_dir = str(gt_dir)
        face = loadmat(os.path.join(gt_dir, "wider_face_val.mat"))
        subs = []
        for s in subset_names:
            if s not in MAT_FILES:
                raise ValueError(f"no .mat file is known for subset {s!r} (known: {sorted(MAT_FILES)})")
            subs.append(loadmat(os.path.join(gt_dir, MAT_FILES[s]))["gt_list"])
        table = {}
        for e in range(len(face["event_list"])):
            event = str(np.asarray(face["event_list"][e][0]).reshape(-1)[0])
            files, bbx = face["file_list"][e][0], face["face_bbx_list"][e][0]
            for j in range(len(files)):
                key = f"{event}/{str(np.asarray(files[j][0]).reshape(-1)[0])}"
                b = np.asarray(bbx[j][0], np.float64).reshape(-1, 4)
                mask = np.zeros(len(b), np.uint32)
                for s, gl in enumerate(subs):
                    keep = np.asarray(gl[e][0][j][0]).reshape(-1).astype(np.int64) - 1          # 1-based
                    if len(keep) and (keep.min() < 0 or keep.max() >= len(b)):
                        raise ValueError(f"{key}: gt_list of {subset_names[s]!r} indexes outside its {len(b)} boxes")
                    mask[keep] |= np.uint32(1 << s)
                table[key] = (np.concatenate([np.ones((len(b), 1)), b], 1).astype(np.float32), mask)
        boxes, masks = [], []
        for n in names:
            k = image_key(n)
            if k not in table:
                raise KeyError(f"{k}: not in {os.path.join(gt_dir, 'wider_face_val.mat')}")
            boxes.append(table[k][0])
            masks.append(table[k][1])
        return cls(masks, subset_names), boxes

    def flat(self, device) -> torch.Tensor:
        """The masks of all images, concatenated in bank order, on `device` (int32 bit patterns)."""
        device = torch.device(device)
        if device not in self._dev:
            m = np.concatenate(self.masks) if sum(len(m) for m in self.masks) else np.zeros(0, np.uint32)
            m = np.concatenate([m, np.zeros(1 if len(m) == 0 else 0, np.uint32)])              # DeviceBoxes pads an empty set
            self._dev[device] = torch.from_numpy(m.view(np.int32).copy()).to(device)
        return self._dev[device]

    def batch(self, boxes, indices) -> WiderGt:
        """The ground truth of the images `indices` of a `DeviceBoxes` over the same bank.  One host read of the offsets per
        `DeviceBoxes`."""
        if boxes.n != len(self):
            raise ValueError(f"masks cover {len(self)} images, the boxes {boxes.n}")
        idx = np.asarray(indices, dtype=np.int64)
        if self._offs is None or self._offs[0] is not boxes:          # read once per DeviceBoxes
            offs = boxes.offset.cpu().numpy().astype(np.int64)
            if int(offs[-1]) != sum(len(m) for m in self.masks):
                raise ValueError("masks and boxes disagree on the number of rows")
            self._offs = (boxes, offs)
        offs = self._offs[1]
        cnt = offs[idx + 1] - offs[idx]
        new = np.zeros(len(idx) + 1, dtype=np.int32)
        new[1:] = np.cumsum(cnt)
        total = int(new[-1])
        dev = boxes.rows.device
        if total == 0:
            rows = torch.zeros(1, 5, dtype=torch.float32, device=dev)
            sub = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            src = torch.from_numpy(np.repeat(offs[idx] - new[:-1], cnt) + np.arange(total, dtype=np.int64)).to(dev)
            rows = boxes.rows.index_select(0, src)
            sub = self.flat(dev).index_select(0, src)
        return WiderGt(rows, torch.from_numpy(new).to(dev), sub, max(int(cnt.max()) if len(cnt) else 0, 1))


class WiderResult:
    """Host-side result of `WiderEvaluator.compute()`.  Index t of `precision[name]` / `recall[name]` is the operating point
    "normalised score >= 1 - (t+1)/n_bins".  A point without a proposal has precision 0: its recall is its neighbour's
    (no proposal, no hit), so it adds no area under the interpolated curve."""

    def __init__(self, proposals: np.ndarray, hits: np.ndarray, n_faces, n_images: int, n_det: int, subset_names, score_norm):
        self.subset_names = tuple(subset_names)
        self.proposals, self.hits = proposals.astype(np.int64), hits.astype(np.int64)
        self.n_bins = int(proposals.shape[1])
        self.n_images, self.n_det = int(n_images), int(n_det)
        self.score_min, self.score_range = float(score_norm[0]), float(score_norm[1])
        self.n_faces, self.precision, self.recall, self.ap = {}, {}, {}, {}
        for s, name in enumerate(self.subset_names):
            cp = np.cumsum(self.proposals[s]).astype(np.float64)
            ch = np.cumsum(self.hits[s]).astype(np.float64)
            nf = int(n_faces[s])
            self.n_faces[name] = nf
            self.precision[name] = np.where(cp > 0, ch / np.where(cp > 0, cp, 1.0), 0.0)
            self.recall[name] = ch / float(nf) if nf else np.full(self.n_bins, np.nan)
            self.ap[name] = voc_ap(self.recall[name], self.precision[name]) if nf else float("nan")

    def to_json(self) -> dict:
        nan = lambda a: [None if x != x else float(x) for x in a]      # noqa: E731  (JSON has no NaN)
        return {"subsets": list(self.subset_names), "n_bins": self.n_bins, "n_images": self.n_images, "n_detections": self.n_det,
                "score_min": self.score_min, "score_range": self.score_range,
                "n_faces": {k: self.n_faces[k] for k in self.subset_names},
                "ap": {k: (None if self.ap[k] != self.ap[k] else self.ap[k]) for k in self.subset_names},
                "precision": {k: nan(self.precision[k]) for k in self.subset_names},
                "recall": {k: nan(self.recall[k]) for k in self.subset_names},
                "proposals": self.proposals.tolist(), "hits": self.hits.tolist()}


def _unpack_gt(gt):
    if isinstance(gt, WiderGt):
        return gt.rows, gt.box_offset, gt.subsets, gt.max_per_image
    if isinstance(gt, (tuple, list)) and len(gt) == 3 and all(isinstance(g, torch.Tensor) for g in gt):
        return gt[0], gt[1], gt[2], None
    raise TypeError("gt must be a WiderGt (WiderSubsets.batch) or a (rows, box_offset, subsets) triple of device tensors")


class WiderEvaluator:
    """Accumulates a validation set's detections against the protocol's ground truth; `compute()` gives the AP per subset.

    normalize=True (the protocol): scores are min-max normalised over the whole set, which is only known at the end, so
    `update` keeps the batch on the device (rows cloned) and `compute()` launches the kernel once per kept batch with the
    (min, max - min) pair a device reduction found (min starts at 1, max at 0, as the protocol's norm_score does).
    normalize=False: raw scores are cut at the thresholds, the kernel runs in `update`, nothing is kept."""

    def __init__(self, subset_names: Sequence[str] = ("easy", "medium", "hard"), iou_threshold: float = 0.5, n_bins: int = 1000,
                 normalize: bool = True, device="cuda"):
        self.subset_names = tuple(subset_names)
        self.normalize = bool(normalize)
        self.state = hp.WiderState(len(self.subset_names), iou_threshold, n_bins, device)
        self._kept: List[tuple] = []
        self._lo = self._hi = None
        self._final = None                                   # the (min, range) the state was filled with, once it is

    iou_threshold = property(lambda self: self.state.iou_threshold)
    n_bins = property(lambda self: self.state.n_bins)
    device = property(lambda self: self.state.device)

    def reset(self) -> None:
        self.state.zero_()
        self._kept, self._lo, self._hi, self._final = [], None, None, None

    def update(self, pred_rows: torch.Tensor, pred_counts: torch.Tensor, gt, scale: Optional[torch.Tensor] = None,
               max_gt: Optional[int] = None) -> None:
        """Add one batch: (pred_rows (B,Kmax,5), pred_counts (B,)) from `forward_batch` / `TiledDetector.detect`; `gt` from
        `WiderSubsets.batch`; `scale` (B,2) fp32 (sx, sy) takes the detections to source pixels (None: they are).  No host
        synchronisation."""
        rows, offs, sub, mpi = _unpack_gt(gt)
        max_gt = mpi if max_gt is None else max_gt
        counts = pred_counts.to(torch.int32)
        self._final = None
        if not self.normalize:
            hp.eval_wider(pred_rows, counts, rows, offs, sub, self.state, scale, None, max_gt)
            return
        pred_rows = pred_rows.detach().clone()
        s = pred_rows[:, :, 0].to(torch.float64)
        valid = (torch.arange(s.shape[1], device=s.device)[None, :] < counts[:, None]) & ~torch.isnan(s)
        one, zero = torch.ones((), dtype=torch.float64, device=s.device), torch.zeros((), dtype=torch.float64, device=s.device)
        lo = torch.minimum(torch.where(valid, s, one).amin(), one)
        hi = torch.maximum(torch.where(valid, s, zero).amax(), zero)
        self._lo = lo if self._lo is None else torch.minimum(self._lo, lo)
        self._hi = hi if self._hi is None else torch.maximum(self._hi, hi)
        self._kept.append((pred_rows, counts.clone(), rows, offs, sub, None if scale is None else scale.clone(), max_gt))

    def _fill(self, lo: float, hi: float) -> None:
        """Run the kernel over the kept batches with the normalisation (lo, hi - lo)."""
        if hi == lo:
            raise hp.N.FdetError(f"WIDER evaluation: every score equals {lo}: min-max normalisation divides by zero")
        norm = torch.tensor([lo, hi - lo], dtype=torch.float64, device=self.device)
        self.state.zero_()
        for pred, counts, rows, offs, sub, scale, max_gt in self._kept:
            hp.eval_wider(pred, counts, rows, offs, sub, self.state, scale, norm, max_gt)
        self._final = (lo, hi - lo)

    def _range(self):
        if self._lo is None:
            return 1.0, 0.0
        lo, hi = torch.stack([self._lo, self._hi]).cpu().tolist()
        return lo, hi

    def merge(self, other: "WiderEvaluator") -> "WiderEvaluator":
        """Add `other`'s state (same subsets, threshold, bins and mode) to this one's."""
        a, b = self.state, other.state
        if (self.subset_names, a.n_bins, a.iou_threshold, self.normalize) != (other.subset_names, b.n_bins, b.iou_threshold, other.normalize):
            raise ValueError("merge: evaluators with different subsets, IoU threshold, bins or normalisation")
        self._final = None
        if not self.normalize:
            a.hist += b.hist.to(a.device)                    # int32 wrap-around == uint32 addition
            a.counters += b.counters.to(a.device)
            return self
        mv = lambda t: None if t is None else t.to(a.device)      # noqa: E731
        self._kept += [tuple(mv(t) if isinstance(t, torch.Tensor) else t for t in k) for k in other._kept]
        if other._lo is not None:
            self._lo = mv(other._lo) if self._lo is None else torch.minimum(self._lo, mv(other._lo))
            self._hi = mv(other._hi) if self._hi is None else torch.maximum(self._hi, mv(other._hi))
        return self

    def all_reduce(self, group=None) -> "WiderEvaluator":
        """Sum the integer state over the ranks of `group` (torch.distributed).  With normalize=True the score range is
        reduced first (MIN / MAX), every rank runs the kernel over its own batches with the common range, then the
        histograms are summed; `compute()` afterwards gives the whole validation set's result on every rank."""
        import torch.distributed as dist
        s = self.state
        if self.normalize:
            lo, hi = self._range()
            r = torch.tensor([lo, -hi], dtype=torch.float64, device=s.device)
            dist.all_reduce(r, op=dist.ReduceOp.MIN, group=group)
            lo, hi = float(r[0]), -float(r[1])
            if self._kept:
                self._fill(lo, hi)
            else:
                s.zero_()
            self._final = (lo, hi - lo)
        nc = s.counters.numel()
        wide = torch.cat([(s.hist.reshape(-1).to(torch.int64) & 0xFFFFFFFF), s.counters])
        dist.all_reduce(wide, op=dist.ReduceOp.SUM, group=group)
        h = wide[:-nc]
        if int(h.max()) > 0xFFFFFFFF:
            raise OverflowError("all_reduce: a histogram bin exceeds 32 bits")
        s.hist.copy_(torch.where(h > 0x7FFFFFFF, h - (1 << 32), h).to(torch.int32).view_as(s.hist))
        s.counters.copy_(wide[-nc:])
        return self

    def compute(self) -> WiderResult:
        """With normalize=True: one small device-to-host copy for the score range, one kernel launch per kept batch.  Then
        one copy of the integers and float64 on the host: cumulative proposals and hits over the thresholds, precision =
        hits / proposals (no proposal: 0), recall = hits / kept faces, AP by `evaluation.voc_ap`.  A subset without a kept
        face has AP NaN.  A rejected image raises."""
        s = self.state
        norm = (0.0, 1.0)
        if self.normalize:
            if self._final is None:
                lo, hi = self._range()
                if self._kept:
                    self._fill(lo, hi)
                else:
                    s.zero_()
                    self._final = (0.0, 1.0)
            norm = self._final
        nc = s.counters.numel()
        flat = torch.cat([s.hist.reshape(-1).to(torch.int64) & 0xFFFFFFFF, s.counters]).cpu().numpy()
        c = flat[-nc:]
        S = s.n_subsets
        if c[S + hp.EVAL_WIDER_N_REJECTED]:
            raise hp.N.FdetError(f"WIDER evaluation: {int(c[S + hp.EVAL_WIDER_N_REJECTED])} image(s) exceeded what the kernel launch "
                                 f"was sized for (detections > Kmax, boxes > max_gt or offsets outside the rows): pass max_gt to update()")
        h = flat[:-nc].reshape(2, S, s.n_bins)
        return WiderResult(h[0], h[1], c[:S], c[S + hp.EVAL_WIDER_N_IMAGES], c[S + hp.EVAL_WIDER_N_DET], self.subset_names, norm)


# ---- the protocol's prediction directory -------------------------------------------------------------------------------
def _fmt(v: float) -> str:
    return f"{float(v):.9g}"                                  # 9 significant digits: every float32 reads back as itself


def write_wider_pred_dir(root, names: Sequence, rows, counts) -> None:
    """names: n image names (`<event>/<image>[.ext]`); rows (n,K,5) [score,x,y,w,h]; counts (n,) -> `root/<event>/<image>.txt`
    holding the image name, the number of boxes, then one `x y w h score` line per box in descending score (ties in row
    order), every number printed with 9 significant digits (`%.9g`), which a float32 survives exactly."""
    rows = np.asarray(rows.detach().cpu() if isinstance(rows, torch.Tensor) else rows, np.float32)
    counts = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    for i, name in enumerate(names):
        key = image_key(name)
        path = os.path.join(str(root), key + ".txt")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        det = rows[i, :int(counts[i])]
        s = np.where(np.isnan(det[:, 0]), -np.inf, det[:, 0]).astype(np.float64)
        det = det[np.lexsort((np.arange(len(s)), -s))]
        with open(path, "w") as f:
            f.write(f"{key.split('/')[-1]}\n{len(det)}\n")
            for sc, x, y, w, h in det.tolist():
                f.write(f"{_fmt(x)} {_fmt(y)} {_fmt(w)} {_fmt(h)} {_fmt(sc)}\n")


def read_wider_pred_dir(root):
    """-> (names `<event>/<image>` sorted, rows (n,K,5) float32 [score,x,y,w,h] zero-padded, counts (n,) int32)."""
    root = str(root)
    names, dets = [], []
    for dirpath, dirnames, filenames in os.walk(root):
        dirnames.sort()
        for fn in sorted(filenames):
            if not fn.endswith(".txt"):
                continue
            with open(os.path.join(dirpath, fn)) as f:
                lines = [ln.strip() for ln in f if ln.strip()]
            k = int(lines[1])
            if len(lines) < 2 + k:
                raise ValueError(f"{os.path.join(dirpath, fn)}: {k} boxes announced, {len(lines) - 2} lines found")
            v = np.array([[float(t) for t in ln.split()[:5]] for ln in lines[2:2 + k]], np.float64).reshape(-1, 5)
            rel = os.path.relpath(dirpath, root)
            names.append(fn[:-4] if rel == "." else f"{rel.replace(os.sep, '/')}/{fn[:-4]}")
            dets.append(np.concatenate([v[:, 4:5], v[:, :4]], 1).astype(np.float32))
    order = np.argsort(names, kind="stable") if names else []
    names, dets = [names[i] for i in order], [dets[i] for i in order]
    K = max([len(d) for d in dets] + [1])
    rows = np.zeros((len(dets), K, 5), np.float32)
    for i, d in enumerate(dets):
        rows[i, :len(d)] = d
    return names, rows, np.array([len(d) for d in dets], np.int32)
