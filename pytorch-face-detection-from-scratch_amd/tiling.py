"""Tiled full-resolution detection from a device image bank.

Every other inference entry point squeezes the whole image into the model's input (480x480) and returns boxes in model
coordinates; the YOLO heads emit at most one box per grid cell.  `TiledDetector` runs the same network on overlapping
windows of the source image (and, by default, on the whole image as today), maps each window's boxes back to source pixels
and merges them with one NMS per source image.  The windows are cut out of the bank by `fdet_tile_gather` and merged by
`fdet_tile_merge` (csrc/fdet_tiles.hip); the network and the reducers in between are the existing ones, unchanged.

    bank = bank_from_files(paths, "cuda")
    det = TiledDetector(model.eval(), tile_sizes=(480,), overlap=0.25)
    rows, counts = det.detect(bank, range(len(bank)))           # (n, max_out, 5) [score,x,y,w,h] in SOURCE pixels, (n,)

With a `DetectionEvaluator` the pair gives the AP on unresized images:

    ev = DetectionEvaluator()
    det = TiledDetector(model, reducer=ev.reducer_for(model))   # the low-score detections a PR curve needs
    rows, counts = det.detect(bank, idx)
    ev.update(rows, counts, boxes_for(device_boxes, idx))       # source-pixel boxes as ground truth

Test-time augmentation: `TiledDetector(..., flip=True, vote=True)` runs every window a second time
mirrored left to right (`fdet_tile_gather_flags`) and merges with box voting (`fdet_tile_merge_vote`): each kept box
becomes the score-weighted mean of the boxes it suppressed.  Both are off by default.

Rules, limits and measurements: DESIGN.md 5c.  The reference project has no counterpart.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

TILE_DTYPE = np.dtype([("image", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4")])     # fdet_tile
assert TILE_DTYPE.itemsize == 20


@dataclass
class TilePlan:
    tiles: np.ndarray            # (T,) TILE_DTYPE records, image-major
    tile_offset: np.ndarray      # (n+1,) int32: image i owns tiles tile_offset[i]..tile_offset[i+1]-1

    def __len__(self) -> int:
        return len(self.tiles)


def tile_stride(t: int, overlap: float) -> int:
    """max(1, t - floor(overlap * t + 0.5))."""
    return max(1, int(t) - int(math.floor(float(overlap) * int(t) + 0.5)))


def axis_origins(L: int, t: int, stride: int) -> list:
    """Window origins along an axis of length L for tile side t: [0] when L <= t; else k * stride for
    k = 0..ceil((L - t) / stride), the last one replaced by L - t (it ends flush with the image)."""
    if L <= t:
        return [0]
    k_last = -((t - L) // stride)                   # ceil((L - t) / stride) in integers
    o = [k * stride for k in range(k_last)]
    o.append(L - t)
    return o


def plan_tiles(sizes, tile_sizes: Sequence[int] = (480,), overlap: float = 0.25, include_whole: bool = True) -> TilePlan:
    """The windows of every image, exactly by this rule:

    * `sizes`: (n,2) integers (h, w).  `overlap` in [0, 1).  For each image, in order:
    * with `include_whole`, the window (x0, y0, w, h) = (0, 0, w, h) comes first;
    * then, for each tile side t of `tile_sizes` in the given order: the window size is (min(t, w), min(t, h)); the stride is
      max(1, t - floor(overlap * t + 0.5)); along an axis of length L > t the origins are k * stride for
      k = 0..ceil((L - t) / stride), the last one replaced by L - t; an axis with L <= t has the single origin 0; windows are
      emitted row-major (y outer, x inner);
    * a window equal to the whole image is emitted once per image only (the first time it comes up).

    -> TilePlan(tiles (T,) records {image, x0, y0, w, h} int32 with image = the row of `sizes`, tile_offset (n+1,) int32).
    Integer arithmetic apart from overlap * t; the same input gives the same plan."""
    sz = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if not 0.0 <= float(overlap) < 1.0:
        raise ValueError(f"plan_tiles: overlap={overlap} must be in [0, 1)")
    ts = [int(t) for t in tile_sizes]
    if any(t < 1 for t in ts):
        raise ValueError(f"plan_tiles: tile sides must be positive, got {tile_sizes}")
    if not ts and not include_whole:
        raise ValueError("plan_tiles: no tile side and no whole-image window")
    recs, offs = [], [0]
    for i, (h, w) in enumerate(sz.tolist()):
        if h < 1 or w < 1:
            raise ValueError(f"plan_tiles: image {i} has size {h}x{w}")
        whole_done = False
        if include_whole:
            recs.append((i, 0, 0, w, h))
            whole_done = True
        for t in ts:
            s = tile_stride(t, overlap)
            ww, wh = min(t, w), min(t, h)
            for y0 in axis_origins(h, t, s):
                for x0 in axis_origins(w, t, s):
                    if ww == w and wh == h:
                        if whole_done:
                            continue
                        whole_done = True
                    recs.append((i, x0, y0, ww, wh))
        offs.append(len(recs))
    tiles = np.array(recs, dtype=TILE_DTYPE) if recs else np.zeros(0, dtype=TILE_DTYPE)
    return TilePlan(np.ascontiguousarray(tiles), np.asarray(offs, dtype=np.int32))


# The mirrored frames of `flip=True` come from fdet_tile_gather_flags because it was measured faster than fdet_tile_gather +
# flip(-1) of the flagged frames by more than the min-max spread of either (tools/tta_throughput.py, profiles/r11_tta.json,
# DESIGN 5f); False takes gather + flip, which gives the same bytes.
FLAGGED_GATHER_MEASURED_FASTER = True


def plan_tta(sizes, tile_sizes: Sequence[int] = (480,), overlap: float = 0.25, include_whole: bool = True, flip: bool = False):
    """-> (TilePlan, flags (T,) uint8).  flip=False: `plan_tiles`' plan and zeros.  flip=True: every image owns its
    `plan_tiles` windows in that order with flag 0, followed by the same windows again with flag 1 (bit 0: the frame is
    mirrored left to right)."""
    p = plan_tiles(sizes, tile_sizes, overlap, include_whole)
    if not flip:
        return p, np.zeros(len(p), np.uint8)
    off = p.tile_offset.astype(np.int64)
    n = len(off) - 1
    tiles = np.concatenate([p.tiles[off[i]:off[i + 1]] for i in range(n) for _ in (0, 1)]) if n else p.tiles
    flags = np.concatenate([np.full(off[i + 1] - off[i], f, np.uint8) for i in range(n) for f in (0, 1)]) if n else np.zeros(0, np.uint8)
    return TilePlan(np.ascontiguousarray(tiles), (2 * off).astype(np.int32)), np.ascontiguousarray(flags)


def boxes_for(boxes, indices):
    """The (rows, box_offset) ground-truth pair `DetectionEvaluator.update` takes, for the images `indices` of a
    `DeviceBoxes` (source-pixel boxes of a whole bank).  One host read of the offsets."""
    import torch
    idx = np.asarray(indices, dtype=np.int64)
    offs = boxes.offset.cpu().numpy().astype(np.int64)
    cnt = offs[idx + 1] - offs[idx]
    new = np.zeros(len(idx) + 1, dtype=np.int32)
    new[1:] = np.cumsum(cnt)
    total = int(new[-1])
    if total == 0:
        rows = torch.zeros(1, 5, dtype=torch.float32, device=boxes.rows.device)
    else:
        src = np.repeat(offs[idx] - new[:-1], cnt) + np.arange(total, dtype=np.int64)
        rows = boxes.rows.index_select(0, torch.from_numpy(src).to(boxes.rows.device))
    return rows, torch.from_numpy(new).to(boxes.rows.device)


class TiledDetector:
    """Detect at the source resolution: windows of the bank's images -> the network -> one merge per image.

    model: PoolResnet / Resnet / MobilenetV3Backbone (through `forward_frames`) or SSD (through its forward), in eval mode.
    tile_sizes / overlap / include_whole: `plan_tiles`.  edge_margin (frame pixels): drop a detection closer than this to a
    window side that is not a side of the image (a face cut by the window); 0 = off.  reducer: None takes
    `model.reduce_bounding_boxes` as it is; `evaluator.reducer_for(model)` keeps the low-score detections.  merge_iou: the
    cross-window NMS threshold, None = the reducer's.  max_frames: frames per network call.  max_out: most boxes per image
    (4864 is what `DetectionEvaluator.update` takes).
    flip: every window a second time, mirrored left to right (twice the frames).  vote: each kept box becomes the
    score-weighted mean of the boxes it suppressed, and a kept box with fewer than min_votes members (itself included) is left
    out; the member counts of the last `detect` are `last_votes` ((n, max_out) int32, None without flip / vote)."""

    def __init__(self, model, tile_sizes: Sequence[int] = (480,), overlap: float = 0.25, include_whole: bool = True,
                 edge_margin: float = 0.0, merge_iou: Optional[float] = None, reducer=None, max_frames: int = 256,
                 max_out: int = 4864, flip: bool = False, vote: bool = False, min_votes: int = 1):
        if not 1 <= int(max_frames) <= 65535:
            raise ValueError(f"TiledDetector: max_frames={max_frames}, 1..65535 are supported")
        if int(max_out) < 1:
            raise ValueError("TiledDetector: max_out must be positive")
        if float(edge_margin) < 0:
            raise ValueError("TiledDetector: edge_margin must be >= 0")
        if int(min_votes) < 1:
            raise ValueError("TiledDetector: min_votes must be >= 1")
        if int(min_votes) > 1 and not vote:
            raise ValueError("TiledDetector: min_votes > 1 needs vote=True")
        self.model = model
        self.tile_sizes = tuple(int(t) for t in tile_sizes)
        self.overlap = float(overlap)
        self.include_whole = bool(include_whole)
        self.edge_margin = float(edge_margin)
        self.reducer = reducer
        self.merge_iou = merge_iou
        self.max_frames = int(max_frames)
        self.max_out = int(max_out)
        self.flip, self.vote, self.min_votes = bool(flip), bool(vote), int(min_votes)
        self.last_votes = None
        plan_tiles(np.array([[1, 1]]), self.tile_sizes, self.overlap, self.include_whole)      # validates the arguments

    def plan(self, sizes) -> TilePlan:
        return plan_tiles(sizes, self.tile_sizes, self.overlap, self.include_whole)

    def plan_tta(self, sizes):
        return plan_tta(sizes, self.tile_sizes, self.overlap, self.include_whole, self.flip)

    def _maps(self, frames):
        from . import hotpath as hp
        m = self.model
        if hasattr(m, "forward_frames"):
            return m.forward_frames(frames)
        # SSD: the preprocessing of its forward(x, predict=1), then the stack
        return m(hp.resize_bilinear_norm(frames, tuple(m.input_shape[1:])))

    def detect(self, bank, indices):
        """-> (rows (n, max_out, 5) [score,x,y,w,h] in source pixels, counts (n,) int32), on the bank's device, for the images
        `indices` of `bank`.  Raises FdetError when an image exceeds a limit of fdet_tile_merge / fdet_tile_merge_vote (more
        than 4864 candidates in its windows, which `flip` doubles; more than max_out survivors): nothing is ever truncated.
        The only host read is that counter."""
        import torch
        from . import hotpath as hp
        from ._native import FdetError
        if self.model.training:
            raise ValueError("TiledDetector: call model.eval() first (inference only)")
        idx = np.asarray(list(indices) if not isinstance(indices, np.ndarray) else indices, dtype=np.int64).reshape(-1)
        if idx.size == 0:
            raise ValueError("TiledDetector.detect: no image")
        if idx.min() < 0 or idx.max() >= len(bank):
            raise IndexError(f"TiledDetector.detect: indices outside the bank of {len(bank)} images")
        dev = bank.device
        table = np.ascontiguousarray(bank.table[idx])                    # the chosen images, renumbered 0..n-1
        tta = self.flip or self.vote                                     # the two TTA entries instead of the plain ones
        sizes = np.stack([table["h"], table["w"]], 1)
        plan, flags = self.plan_tta(sizes) if tta else (self.plan(sizes), None)
        T = len(plan)
        reducer = self.reducer if self.reducer is not None else self.model.reduce_bounding_boxes
        iou = float(reducer.iou_threshold if self.merge_iou is None else self.merge_iou)
        Ho, Wo = int(self.model.input_shape[1]), int(self.model.input_shape[2])
        packed = np.concatenate([table.view(np.uint8).reshape(-1), plan.tiles.view(np.uint8).reshape(-1),
                                 plan.tile_offset.view(np.uint8).reshape(-1)] + ([flags] if tta else []))
        d = torch.from_numpy(packed).pin_memory().to(dev, non_blocking=True)      # one copy: 16- and 4-byte aligned parts
        nt, ntl = table.nbytes, plan.tiles.nbytes
        no = plan.tile_offset.nbytes
        d_table, d_tiles, d_off = d[:nt], d[nt:nt + ntl], d[nt + ntl:nt + ntl + no].view(torch.int32)
        d_flags = d[nt + ntl + no:] if tta else None
        rows = counts = None
        with torch.no_grad():
            for a in range(0, T, self.max_frames):
                b = min(a + self.max_frames, T)
                if self.flip and FLAGGED_GATHER_MEASURED_FASTER:
                    frames = hp.tile_gather_flags(bank.data, d_table, table, d_tiles[a * 20:b * 20], plan.tiles[a:b],
                                                  d_flags[a:b], flags[a:b], (Ho, Wo))
                else:
                    frames = hp.tile_gather(bank.data, d_table, table, d_tiles[a * 20:b * 20], plan.tiles[a:b], (Ho, Wo))
                    sel = np.nonzero(flags[a:b])[0] if self.flip else ()
                    if len(sel):                             # one more read and write of the flagged frames only
                        sel = torch.from_numpy(sel).to(dev)
                        frames.index_copy_(0, sel, frames.index_select(0, sel).flip(-1))
                r, c = reducer.forward_batch(self._maps(frames))
                if rows is None:
                    rows = torch.empty(T, r.shape[1], 5, dtype=torch.float32, device=dev)
                    counts = torch.empty(T, dtype=torch.int32, device=dev)
                rows[a:b] = r
                counts[a:b] = c
            if tta:
                out, self.last_votes, out_counts, rejected = hp.tile_merge_vote(
                    rows, counts, d_tiles, d_flags, d_off, d_table, (Ho, Wo), self.edge_margin, iou, self.max_out, self.vote,
                    self.min_votes)
            else:
                self.last_votes = None
                out, out_counts, rejected = hp.tile_merge(rows, counts, d_tiles, d_off, d_table, (Ho, Wo), self.edge_margin, iou,
                                                          self.max_out)
        n_rej = int(rejected.item())
        if n_rej:
            entry = "fdet_tile_merge_vote" if tta else "fdet_tile_merge"
            hint = "use fewer windows or flip=False (the mirrored pass doubles the candidates)" if self.flip else "use fewer windows"
            raise FdetError(f"TiledDetector.detect: {n_rej} image(s) exceed a limit of {entry} (more than "
                            f"{hp.TILE_MAX_CANDIDATES} candidates in one image's windows, or more than max_out={self.max_out} "
                            f"merged boxes); raise the reducer's probability threshold or {hint}")
        return out, out_counts

    def detect_split(self, bank, indices):
        """`detect` as the reference-shaped tuple of per-image (k,5) tensors."""
        from .models.BaseModel import split_rows
        return split_rows(*self.detect(bank, indices))
