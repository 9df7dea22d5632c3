"""Tensor-level wrappers over the C-ABI (include/fdet.h).  Each function validates shapes on
the host (a kernel launched on mismatched shapes can fault the GPU), allocates the outputs
with torch, and enqueues the HIP kernels on torch's current stream.  GPU tensors only.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import _native as N
from ._native import check, lib, ptr, stream

I32 = torch.int32
F32 = torch.float32


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != F32:
        t = t.float()
    return t.contiguous()


# ------------------------------------------------------------------------------------------
# detection math
# ------------------------------------------------------------------------------------------
def encode_targets(boxes: Sequence[torch.Tensor], img_size: Tuple[int, int], num_of_patches: int,
                   device=None) -> torch.Tensor:
    """Batched WIDERFaceDataset.convert_bbx_to_feature_map (dataset.py:32-64).
    `boxes`: list of (n_i,5) tensors [conf,x,y,w,h] -> (B,5,S,S) on the GPU."""
    B = len(boxes)
    device = device or torch.device("cuda", torch.cuda.current_device())
    counts = [int(b.shape[0]) if b.numel() else 0 for b in boxes]
    offs = torch.zeros(B + 1, dtype=I32)
    offs[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0).to(I32)
    rows = [b.reshape(-1, 5).to(F32).cpu() for b in boxes if b.numel()]
    flat = torch.cat(rows, 0) if rows else torch.zeros(1, 5)
    flat_d = flat.contiguous().to(device)
    offs_d = offs.to(device)
    S = int(num_of_patches)
    out = torch.empty(B, 5, S, S, dtype=F32, device=device)
    if B:
        check(lib().fdet_encode_targets(ptr(flat_d), ptr(offs_d, I32), B, S, float(img_size[0]), float(img_size[1]),
                                        ptr(out), stream()), "fdet_encode_targets")
    return out


def _device_rows(rows: torch.Tensor, box_offset: torch.Tensor):
    if not (rows.is_cuda and box_offset.is_cuda):
        raise N.FdetError("device-input target encode: rows and box_offset must be GPU tensors")
    if rows.dtype != F32 or rows.dim() != 2 or rows.shape[1] != 5 or rows.shape[0] < 1:
        raise ValueError(f"rows must be a (cap>=1,5) float32 tensor, got {tuple(rows.shape)} {rows.dtype}")
    if box_offset.dtype != I32 or box_offset.dim() != 1 or box_offset.numel() < 2:
        raise ValueError("box_offset must be a (B+1,) int32 tensor")
    return rows.contiguous(), box_offset.contiguous(), box_offset.numel() - 1


def encode_targets_device(rows: torch.Tensor, box_offset: torch.Tensor, img_size: Tuple[int, int],
                          num_of_patches: int) -> torch.Tensor:
    """encode_targets on rows already on the device: rows (cap,5) [conf,x,y,w,h], box_offset (B+1,) int32 (image n owns
    rows box_offset[n]..box_offset[n+1]-1, box_offset[B] <= cap) -> (B,5,S,S).  No host round trip, no synchronisation."""
    rows, box_offset, B = _device_rows(rows, box_offset)
    S = int(num_of_patches)
    out = torch.empty(B, 5, S, S, dtype=F32, device=rows.device)
    check(lib().fdet_encode_targets(ptr(rows), ptr(box_offset, I32), B, S, float(img_size[0]), float(img_size[1]),
                                    ptr(out), stream()), "fdet_encode_targets")
    return out


def yolo_loss_fwd_bwd(pred: torch.Tensor, gt: torch.Tensor, want_grad: bool = True, grad_scale: float = 1.0):
    """(B,5,S,S) x2 -> (loss_per_image (B,), loss_sum (1,), grad (B,5,S,S) or None)."""
    pred, gt = _f32(pred), _f32(gt)
    if pred.dim() != 4 or pred.shape[1] != 5 or pred.shape[2] != pred.shape[3] or pred.shape != gt.shape:
        raise ValueError(f"yolo_loss: expected matching (B,5,S,S) maps, got {tuple(pred.shape)} / {tuple(gt.shape)}")
    B, _, S, _ = pred.shape
    lpi = torch.empty(B, dtype=F32, device=pred.device)
    lsum = torch.empty(1, dtype=F32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    check(lib().fdet_yolo_loss_fwd_bwd(ptr(pred), ptr(gt), B, S, ptr(lpi), ptr(lsum), ptr(grad), float(grad_scale),
                                       stream()), "fdet_yolo_loss_fwd_bwd")
    return lpi, lsum, grad


def decode(maps: torch.Tensor, prob_threshold: float, img_w: float, img_h: float):
    maps = _f32(maps)
    B, C, S, S2 = maps.shape
    if C != 5 or S != S2:
        raise ValueError(f"decode: expected (B,5,S,S), got {tuple(maps.shape)}")
    scores = torch.zeros(B, S * S, dtype=F32, device=maps.device)
    boxes = torch.zeros(B, S * S, 4, dtype=F32, device=maps.device)
    counts = torch.zeros(B, dtype=I32, device=maps.device)
    check(lib().fdet_decode(ptr(maps), B, S, float(prob_threshold), float(img_w), float(img_h), ptr(scores),
                            ptr(boxes), ptr(counts, I32), stream()), "fdet_decode")
    return scores, boxes, counts


def nms_batched(boxes: torch.Tensor, scores: torch.Tensor, counts: torch.Tensor, iou_threshold: float):
    boxes, scores = _f32(boxes), _f32(scores)
    B, K, four = boxes.shape
    if four != 4 or scores.shape != (B, K) or counts.shape != (B,):
        raise ValueError("nms_batched: expected boxes (B,K,4), scores (B,K), counts (B,)")
    counts = counts.to(I32).contiguous()
    keep = torch.zeros(B, K, dtype=I32, device=boxes.device)
    kc = torch.zeros(B, dtype=I32, device=boxes.device)
    check(lib().fdet_nms(ptr(boxes), ptr(scores), ptr(counts, I32), B, K, float(iou_threshold), ptr(keep, I32),
                         ptr(kc, I32), stream()), "fdet_nms")
    return keep, kc


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """Drop-in for torchvision.ops.nms (keyword names as the reference passes them,
    datasets/utils.py:164): (K,4) xyxy, (K,) -> int64 kept indices by descending score."""
    K = boxes.shape[0]
    if K == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    if K > 4864:
        raise N.FdetError(f"nms: K={K} > 4864 candidates per image is not supported by fdet_nms")
    cnt = torch.tensor([K], dtype=I32, device=boxes.device)
    keep, kc = nms_batched(boxes.reshape(1, K, 4), scores.reshape(1, K), cnt, iou_threshold)
    return keep[0, : int(kc[0])].to(torch.int64)


def reduce_bounding_boxes(maps: torch.Tensor, prob_threshold: float, iou_threshold: float, img_w: float,
                          img_h: float):
    """Batched ReduceBoundingBoxes.forward: (B,5,S,S) -> (out (B,S*S,5), counts (B,))."""
    maps = _f32(maps)
    B, C, S, S2 = maps.shape
    if C != 5 or S != S2:
        raise ValueError(f"reduce_bounding_boxes: expected (B,5,S,S), got {tuple(maps.shape)}")
    out = torch.zeros(B, S * S, 5, dtype=F32, device=maps.device)
    counts = torch.zeros(B, dtype=I32, device=maps.device)
    check(lib().fdet_reduce_bounding_boxes(ptr(maps), B, S, float(prob_threshold), float(iou_threshold),
                                           float(img_w), float(img_h), ptr(out), ptr(counts, I32), stream()),
          "fdet_reduce_bounding_boxes")
    return out, counts


def step_metrics(gt: torch.Tensor, gt_counts: torch.Tensor, pred: torch.Tensor, pred_counts: torch.Tensor):
    B, K, five = gt.shape
    if five != 5 or pred.shape != gt.shape:
        raise ValueError("step_metrics: expected gt/pred (B,K,5)")
    per = torch.empty(B, 3, dtype=F32, device=gt.device)
    tot = torch.empty(3, dtype=F32, device=gt.device)
    check(lib().fdet_step_metrics(ptr(_f32(gt)), ptr(gt_counts.to(I32).contiguous(), I32), ptr(_f32(pred)),
                                  ptr(pred_counts.to(I32).contiguous(), I32), B, K, ptr(per), ptr(tot), stream()),
          "fdet_step_metrics")
    return per, tot


# ------------------------------------------------------------------------------------------
# dataset-level evaluation (csrc/fdet_eval.hip)
# ------------------------------------------------------------------------------------------
EVAL_MAX_THRESHOLDS, EVAL_MAX_DET, EVAL_MAX_GT, EVAL_MAX_BINS = 10, 4864, 4096, 4096      # FDET_EVAL_* of include/fdet.h
EVAL_N_GT, EVAL_N_IMAGES, EVAL_N_DET, EVAL_N_REJECTED = 0, 1, 2, 3


class EvalState:
    """The accumulators of fdet_eval_match: `hist` (2,T,n_bins) int32 holding the uint32 bit patterns of the tp (hist[0])
    and fp (hist[1]) histograms, `counters` (4,) int64 [ground-truth boxes, images, detections, rejected images].  Lives
    on `device`; a CPU state is good for merging / reducing what was copied off a GPU, not for eval_match."""

    def __init__(self, iou_thresholds=(0.5,), n_bins: int = 1000, device="cuda"):
        import ctypes
        import numpy as np
        thr = [float(t) for t in iou_thresholds]
        if not 1 <= len(thr) <= EVAL_MAX_THRESHOLDS:
            raise ValueError(f"eval: {len(thr)} IoU thresholds, 1..{EVAL_MAX_THRESHOLDS} are supported")
        if not 1 <= int(n_bins) <= EVAL_MAX_BINS:
            raise ValueError(f"eval: n_bins={n_bins}, 1..{EVAL_MAX_BINS} are supported")
        self.iou_thresholds = np.asarray(thr, dtype=np.float32)            # the values the kernel compares with
        self._thr_c = (ctypes.c_float * len(thr))(*self.iou_thresholds.tolist())
        self.n_bins = int(n_bins)
        self.device = torch.device(device)
        self.hist = torch.zeros(2, len(thr), self.n_bins, dtype=I32, device=self.device)
        self.counters = torch.zeros(4, dtype=torch.int64, device=self.device)

    @property
    def T(self) -> int:
        return len(self.iou_thresholds)

    def zero_(self) -> None:
        self.hist.zero_()
        self.counters.zero_()


def _eval_common_args(name: str, pred, pred_counts, gt_rows, gt_offset, max_gt):
    """The shape and dtype checks that eval_match and eval_wider share, `name` being the entry the messages speak for
    -> (B, Kmax, cap, max_gt), max_gt defaulting to min(cap, EVAL_MAX_GT)."""
    if pred.dim() != 3 or pred.shape[2] != 5 or pred.dtype != F32 or pred.shape[0] < 1:
        raise ValueError(f"{name}: pred must be a (B>=1,Kmax,5) float32 tensor, got {tuple(pred.shape)} {pred.dtype}")
    B, Kmax = int(pred.shape[0]), int(pred.shape[1])
    if not 1 <= Kmax <= EVAL_MAX_DET:
        raise ValueError(f"{name}: Kmax={Kmax} detections per image, 1..{EVAL_MAX_DET} are supported")
    if tuple(pred_counts.shape) != (B,) or pred_counts.dtype != I32:
        raise ValueError(f"{name}: pred_counts must be a ({B},) int32 tensor, got {tuple(pred_counts.shape)} {pred_counts.dtype}")
    if gt_rows.dim() != 2 or gt_rows.shape[1] != 5 or gt_rows.dtype != F32 or gt_rows.shape[0] < 1:
        raise ValueError(f"{name}: gt_rows must be a (cap>=1,5) float32 tensor, got {tuple(gt_rows.shape)} {gt_rows.dtype}")
    cap = int(gt_rows.shape[0])
    if tuple(gt_offset.shape) != (B + 1,) or gt_offset.dtype != I32:
        raise ValueError(f"{name}: gt_offset must be a ({B + 1},) int32 tensor, got {tuple(gt_offset.shape)} {gt_offset.dtype}")
    max_gt = min(cap, EVAL_MAX_GT) if max_gt is None else int(max_gt)
    if not 1 <= max_gt <= EVAL_MAX_GT:
        raise ValueError(f"{name}: max_gt={max_gt} boxes per image, 1..{EVAL_MAX_GT} are supported")
    return B, Kmax, cap, max_gt


def eval_match(pred: torch.Tensor, pred_counts: torch.Tensor, gt_rows: torch.Tensor, gt_offset: torch.Tensor,
               state: EvalState, max_gt: Optional[int] = None, want_match: bool = False):
    """Match one batch and add it to `state` (fdet_eval_match): pred (B,Kmax,5) [score,x,y,w,h] with pred_counts (B,) as
    `forward_batch` of either reducer returns them, gt_rows (cap,5) [conf,x,y,w,h] with gt_offset (B+1,) int32 as
    GtBoxes holds them.  `max_gt`: the most boxes one image can have (default min(cap, 4096)).  One launch, no host
    synchronisation.  -> match (B,Kmax) int32 for the first threshold with `want_match`, else None."""
    if not isinstance(state, EvalState):
        raise ValueError("eval_match: state must be an EvalState")
    B, Kmax, cap, max_gt = _eval_common_args("eval_match", pred, pred_counts, gt_rows, gt_offset, max_gt)
    pred, pred_counts, gt_rows, gt_offset = pred.contiguous(), pred_counts.contiguous(), gt_rows.contiguous(), gt_offset.contiguous()
    match = torch.empty(B, Kmax, dtype=I32, device=pred.device) if want_match else None
    check(lib().fdet_eval_match(ptr(pred), ptr(pred_counts, I32), B, Kmax, ptr(gt_rows), ptr(gt_offset, I32), cap, max_gt,
                                state._thr_c, state.T, state.n_bins, ptr(state.hist[0], I32), ptr(state.hist[1], I32),
                                ptr(state.counters, torch.int64), ptr(match, I32), stream()), "fdet_eval_match")
    return match


# ------------------------------------------------------------------------------------------
# WIDER Face protocol evaluation (csrc/fdet_eval_wider.hip)
# ------------------------------------------------------------------------------------------
EVAL_WIDER_MAX_SUBSETS = 8                                    # FDET_EVAL_WIDER_* of include/fdet.h
EVAL_WIDER_N_IMAGES, EVAL_WIDER_N_DET, EVAL_WIDER_N_REJECTED, EVAL_WIDER_N_COUNTERS = 0, 1, 2, 3


class WiderState:
    """The accumulators of fdet_eval_wider: `hist` (2,S,n_bins) int32 holding the uint32 bit patterns of the proposal
    (hist[0]) and hit (hist[1]) histograms, `counters` (S+3,) int64 [kept boxes per subset, images, detections, rejected
    images]."""

    def __init__(self, n_subsets: int = 3, iou_threshold: float = 0.5, n_bins: int = 1000, device="cuda"):
        if not 1 <= int(n_subsets) <= EVAL_WIDER_MAX_SUBSETS:
            raise ValueError(f"eval_wider: {n_subsets} subsets, 1..{EVAL_WIDER_MAX_SUBSETS} are supported")
        if not 1 <= int(n_bins) <= EVAL_MAX_BINS:
            raise ValueError(f"eval_wider: n_bins={n_bins}, 1..{EVAL_MAX_BINS} are supported")
        self.n_subsets, self.n_bins, self.iou_threshold = int(n_subsets), int(n_bins), float(iou_threshold)
        self.device = torch.device(device)
        self.hist = torch.zeros(2, self.n_subsets, self.n_bins, dtype=I32, device=self.device)
        self.counters = torch.zeros(self.n_subsets + EVAL_WIDER_N_COUNTERS, dtype=torch.int64, device=self.device)

    def zero_(self) -> None:
        self.hist.zero_()
        self.counters.zero_()


def eval_wider(pred: torch.Tensor, pred_counts: torch.Tensor, gt_rows: torch.Tensor, gt_offset: torch.Tensor,
               gt_subsets: torch.Tensor, state: WiderState, pred_scale: Optional[torch.Tensor] = None,
               score_norm: Optional[torch.Tensor] = None, max_gt: Optional[int] = None) -> None:
    """Add one batch to `state` (fdet_eval_wider): pred / pred_counts / gt_rows / gt_offset as for `eval_match`, with ALL
    boxes of the images in source pixels; gt_subsets (cap,) int32 holding the uint32 subset masks; pred_scale (B,2) fp32
    (sx, sy) or None; score_norm (2,) float64 [min, max - min] on the device or None.  One launch, no host
    synchronisation."""
    if not isinstance(state, WiderState):
        raise ValueError("eval_wider: state must be a WiderState")
    B, Kmax, cap, max_gt = _eval_common_args("eval_wider", pred, pred_counts, gt_rows, gt_offset, max_gt)
    if tuple(gt_subsets.shape) != (cap,) or gt_subsets.dtype != I32:
        raise ValueError(f"eval_wider: gt_subsets must be a ({cap},) int32 tensor, got {tuple(gt_subsets.shape)} {gt_subsets.dtype}")
    if pred_scale is not None and (tuple(pred_scale.shape) != (B, 2) or pred_scale.dtype != F32):
        raise ValueError(f"eval_wider: pred_scale must be a ({B},2) float32 tensor, got {tuple(pred_scale.shape)} {pred_scale.dtype}")
    if score_norm is not None and (tuple(score_norm.shape) != (2,) or score_norm.dtype != torch.float64):
        raise ValueError("eval_wider: score_norm must be a (2,) float64 tensor")
    pred, pred_counts, gt_rows, gt_offset, gt_subsets = (t.contiguous() for t in (pred, pred_counts, gt_rows, gt_offset, gt_subsets))
    check(lib().fdet_eval_wider(ptr(pred), ptr(pred_counts, I32), B, Kmax,
                                ptr(None if pred_scale is None else pred_scale.contiguous()), ptr(gt_rows),
                                ptr(gt_offset, I32), cap, ptr(gt_subsets, I32), state.n_subsets, max_gt, state.iou_threshold,
                                ptr(score_norm, torch.float64), state.n_bins, ptr(state.hist[0], I32), ptr(state.hist[1], I32),
                                ptr(state.counters, torch.int64), stream()), "fdet_eval_wider")


# ------------------------------------------------------------------------------------------
# tiled full-resolution detection (csrc/fdet_tiles.hip)
# ------------------------------------------------------------------------------------------
TILE_MAX_CANDIDATES = 4864                                   # FDET_TILE_MAX_CANDIDATES of include/fdet.h


def _tile_records(h_tiles):
    import numpy as np
    if not isinstance(h_tiles, np.ndarray) or h_tiles.dtype.itemsize != 20 or h_tiles.ndim != 1 or not h_tiles.flags.c_contiguous:
        raise ValueError("tiles: expected a contiguous (T,) numpy record array of fdet_tile {image,x0,y0,w,h} int32")
    return h_tiles


def tile_gather(bank_data: torch.Tensor, d_table: torch.Tensor, h_table, d_tiles: torch.Tensor, h_tiles, out_hw,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Windows of a device image bank -> (T,3,Ho,Wo) planar uint8 frames (fdet_tile_gather).  bank_data: the bank's byte
    buffer; d_table / h_table: its fdet_aug_image table on the device (uint8 view) and as the numpy record array;
    d_tiles / h_tiles: the windows likewise (tiling.TILE_DTYPE).  Bad windows raise FdetError before anything is written."""
    h_tiles = _tile_records(h_tiles)
    T, n_images = len(h_tiles), len(h_table)
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    if d_tiles.numel() != T * 20 or d_table.numel() != n_images * 16:
        raise ValueError("tile_gather: device and host copies of the tiles / table differ in size")
    if out is None:
        out = torch.empty(T, 3, Ho, Wo, dtype=torch.uint8, device=bank_data.device)
    elif tuple(out.shape) != (T, 3, Ho, Wo):
        raise ValueError(f"tile_gather: out must be ({T},3,{Ho},{Wo}), got {tuple(out.shape)}")
    U8 = torch.uint8
    check(lib().fdet_tile_gather(ptr(bank_data, U8), ptr(d_table, U8), h_table.ctypes.data, n_images, ptr(d_tiles, U8),
                                 h_tiles.ctypes.data, T, Ho, Wo, ptr(out, U8), stream()), "fdet_tile_gather")
    return out


def tile_merge(rows: torch.Tensor, counts: torch.Tensor, d_tiles: torch.Tensor, tile_offset: torch.Tensor, d_table: torch.Tensor,
               frame_hw, edge_margin: float, iou_threshold: float, max_out: int, rejected: Optional[torch.Tensor] = None):
    """fdet_tile_merge: rows (T,K,5) [score,x,y,w,h] in frame pixels + counts (T,) int32 of the T windows d_tiles,
    tile_offset (n+1,) int32, d_table the n images' table -> (out (n,max_out,5) in source pixels, out_counts (n,) int32,
    rejected (1,) int64 counter, += 1 per image over a limit).  One launch, no host synchronisation."""
    if rows.dim() != 3 or rows.shape[2] != 5 or rows.dtype != F32:
        raise ValueError(f"tile_merge: rows must be (T,K,5) float32, got {tuple(rows.shape)} {rows.dtype}")
    T, K = int(rows.shape[0]), int(rows.shape[1])
    n = int(tile_offset.numel()) - 1
    if tuple(counts.shape) != (T,) or counts.dtype != I32 or tile_offset.dtype != I32 or n < 1:
        raise ValueError("tile_merge: counts must be (T,) int32 and tile_offset (n+1,) int32")
    if d_tiles.numel() != T * 20 or d_table.numel() != n * 16:
        raise ValueError("tile_merge: tiles / table do not match T / n")
    if int(max_out) < 1:
        raise ValueError("tile_merge: max_out must be positive")
    dev = rows.device
    out = torch.empty(n, int(max_out), 5, dtype=F32, device=dev)
    out_counts = torch.empty(n, dtype=I32, device=dev)
    if rejected is None:
        rejected = torch.zeros(1, dtype=torch.int64, device=dev)
    U8 = torch.uint8
    check(lib().fdet_tile_merge(ptr(rows.contiguous()), ptr(counts.contiguous(), I32), ptr(d_tiles, U8),
                                ptr(tile_offset.contiguous(), I32), n, T, K, int(frame_hw[0]), int(frame_hw[1]), ptr(d_table, U8),
                                float(edge_margin), float(iou_threshold), int(max_out), ptr(out), ptr(out_counts, I32),
                                ptr(rejected, torch.int64), stream()), "fdet_tile_merge")
    return out, out_counts, rejected


def render_blur_ws_bytes(h_table, h_rows, h_counts) -> int:
    """fdet_render_blur_ws_bytes: the workspace `render_boxes_blur` needs for these host copies of the image table, the
    rows (n,K,5) fp32 and the counts (n,) int32."""
    n, K = int(h_rows.shape[0]), int(h_rows.shape[1])
    size = int(lib().fdet_render_blur_ws_bytes(h_table.ctypes.data, h_rows.ctypes.data if K else None, h_counts.ctypes.data, n, K))
    if size == 0:
        raise ValueError("render_blur_ws_bytes: bad arguments (a count outside 0..K)")
    return size


def render_boxes_blur(src, rows: torch.Tensor, counts: torch.Tensor, h_counts, out, d_tab: torch.Tensor, h_tab, outline: bool = False,
                      blocks: int = 8, color=(0, 0, 255), blur: bool = True, pixelate: bool = False, ws: Optional[torch.Tensor] = None,
                      rejected: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fdet_render_boxes_blur: the images of the bank `src` into the bank `out` (same sizes, its own buffer) with the first
    counts[i] boxes of rows[i] blurred by the table d_tab / h_tab ((n_tab,3) int32 (r, ww, fw), device and host) and
    outlined.  ws: uint8 device scratch (None: sized here from a host copy of `rows`).  -> rejected (1,) int64 counter,
    += 1 per box the workspace does not hold; the caller must read it as an error."""
    import numpy as np
    n, K = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    U8 = torch.uint8
    if not isinstance(h_tab, np.ndarray) or h_tab.dtype != np.int32 or h_tab.ndim != 2 or h_tab.shape[1] != 3 or not h_tab.flags.c_contiguous:
        raise ValueError("render_boxes_blur: h_tab must be a contiguous (n_tab,3) numpy int32 array")
    if tuple(d_tab.shape) != h_tab.shape or d_tab.dtype != I32:
        raise ValueError("render_boxes_blur: d_tab must be the device copy of h_tab")
    if ws is None:
        h_rows = np.ascontiguousarray(rows.cpu().numpy())
        ws = torch.empty(render_blur_ws_bytes(src.table, h_rows, h_counts), dtype=U8, device=dev)
    if rejected is None:
        rejected = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().fdet_render_boxes_blur(ptr(src.data, U8), ptr(src.d_table, U8), src.table.ctypes.data, ptr(rows) if K else None,
                                       ptr(counts, I32), h_counts.ctypes.data, n, K, ptr(out.data, U8), ptr(out.d_table, U8),
                                       out.table.ctypes.data, int(bool(outline)), int(bool(pixelate)), int(bool(blur)), int(blocks),
                                       ptr(d_tab, I32), h_tab.ctypes.data, int(h_tab.shape[0]), int(color[0]), int(color[1]), int(color[2]),
                                       ptr(ws, U8), int(ws.numel()), ptr(rejected, torch.int64), stream()), "fdet_render_boxes_blur")
    return rejected


def _tile_flags(h_flags, T):
    import numpy as np
    if not isinstance(h_flags, np.ndarray) or h_flags.dtype != np.uint8 or h_flags.shape != (T,) or not h_flags.flags.c_contiguous:
        raise ValueError(f"flags: expected a contiguous ({T},) numpy uint8 array")
    return h_flags


def tile_gather_flags(bank_data: torch.Tensor, d_table: torch.Tensor, h_table, d_tiles: torch.Tensor, h_tiles, d_flags: torch.Tensor,
                      h_flags, out_hw, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`tile_gather` with a mirror flag per window (fdet_tile_gather_flags): d_flags / h_flags are (T,) uint8 on the device
    and as a numpy array; bit 0 set writes the frame mirrored left to right, byte-equal to `flip(-1)` of the unflagged frame.
    A flag with another bit set raises FdetError before anything is written."""
    h_tiles = _tile_records(h_tiles)
    T, n_images = len(h_tiles), len(h_table)
    h_flags = _tile_flags(h_flags, T)
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    U8 = torch.uint8
    if d_tiles.numel() != T * 20 or d_table.numel() != n_images * 16 or d_flags.numel() != T or d_flags.dtype != U8:
        raise ValueError("tile_gather_flags: device and host copies of the tiles / table / flags differ in size")
    if out is None:
        out = torch.empty(T, 3, Ho, Wo, dtype=U8, device=bank_data.device)
    elif tuple(out.shape) != (T, 3, Ho, Wo):
        raise ValueError(f"tile_gather_flags: out must be ({T},3,{Ho},{Wo}), got {tuple(out.shape)}")
    check(lib().fdet_tile_gather_flags(ptr(bank_data, U8), ptr(d_table, U8), h_table.ctypes.data, n_images, ptr(d_tiles, U8),
                                       h_tiles.ctypes.data, ptr(d_flags, U8), h_flags.ctypes.data, T, Ho, Wo, ptr(out, U8),
                                       stream()), "fdet_tile_gather_flags")
    return out


def tile_merge_vote(rows: torch.Tensor, counts: torch.Tensor, d_tiles: torch.Tensor, d_flags: Optional[torch.Tensor],
                    tile_offset: torch.Tensor, d_table: torch.Tensor, frame_hw, edge_margin: float, iou_threshold: float,
                    max_out: int, vote: bool = True, min_votes: int = 1, rejected: Optional[torch.Tensor] = None):
    """fdet_tile_merge_vote: `tile_merge` that first un-mirrors the rows of the windows flagged in d_flags ((T,) uint8 on
    the device, None = no window is mirrored) and, with `vote`, writes each kept box as the score-weighted mean of the boxes
    it suppressed; `vote=False` writes the kept boxes themselves.  Kept boxes with fewer than min_votes members are left out.
    -> (out (n,max_out,5), out_votes (n,max_out) int32, out_counts (n,) int32, rejected (1,) int64)."""
    if rows.dim() != 3 or rows.shape[2] != 5 or rows.dtype != F32:
        raise ValueError(f"tile_merge_vote: rows must be (T,K,5) float32, got {tuple(rows.shape)} {rows.dtype}")
    T, K = int(rows.shape[0]), int(rows.shape[1])
    n = int(tile_offset.numel()) - 1
    if tuple(counts.shape) != (T,) or counts.dtype != I32 or tile_offset.dtype != I32 or n < 1:
        raise ValueError("tile_merge_vote: counts must be (T,) int32 and tile_offset (n+1,) int32")
    if d_tiles.numel() != T * 20 or d_table.numel() != n * 16:
        raise ValueError("tile_merge_vote: tiles / table do not match T / n")
    U8 = torch.uint8
    if d_flags is not None and (d_flags.numel() != T or d_flags.dtype != U8):
        raise ValueError("tile_merge_vote: flags must be (T,) uint8")
    if int(max_out) < 1 or int(min_votes) < 1:
        raise ValueError("tile_merge_vote: max_out and min_votes must be positive")
    dev = rows.device
    out = torch.empty(n, int(max_out), 5, dtype=F32, device=dev)
    out_votes = torch.empty(n, int(max_out), dtype=I32, device=dev)
    out_counts = torch.empty(n, dtype=I32, device=dev)
    if rejected is None:
        rejected = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().fdet_tile_merge_vote(ptr(rows.contiguous()), ptr(counts.contiguous(), I32), ptr(d_tiles, U8),
                                     ptr(None if d_flags is None else d_flags.contiguous(), U8), ptr(tile_offset.contiguous(), I32),
                                     n, T, K, int(frame_hw[0]), int(frame_hw[1]), ptr(d_table, U8), float(edge_margin),
                                     float(iou_threshold), int(min_votes), int(bool(vote)), int(max_out), ptr(out),
                                     ptr(out_votes, I32), ptr(out_counts, I32), ptr(rejected, torch.int64), stream()),
          "fdet_tile_merge_vote")
    return out, out_votes, out_counts, rejected


# ------------------------------------------------------------------------------------------
# Tracking across frame sequences (csrc/fdet_track.hip, csrc/fdet_track_refine.hip; tracking.py drives this)
# ------------------------------------------------------------------------------------------
TRACK_SLOTS, TRACK_MAX_DETS, TRACK_MAX_COORD = 128, 256, 16384      # FDET_TRACK_* of include/fdet.h
TRACK_STATE_BYTES = 16 + TRACK_SLOTS * 48                           # per sequence


def track_state_bytes(n_seq: int) -> int:
    return int(lib().fdet_track_state_bytes(int(n_seq)))


def track_update(rows: torch.Tensor, counts: torch.Tensor, seq_offset: torch.Tensor, h_seq_offset, state: torch.Tensor,
                 iou_threshold: float, alpha256: int, max_misses: int, min_hits: int, emit_misses: int, birth_score: float,
                 rejected: Optional[torch.Tensor] = None):
    """fdet_track_update: rows (T,K,5) [score,x,y,w,h] + counts (T,) int32 of T frames; seq_offset (n_seq+1,) int32 on the
    device and h_seq_offset, the same values as a numpy int32 array: sequence s owns frames seq_offset[s]..seq_offset[s+1]-1
    in time order; state: (n_seq * 6160,) uint8 on the device, updated in place (zeros = fresh) ->
    (out_rows (T,128,5), out_ids (T,128) int32, out_misses (T,128) int32, out_counts (T,) int32, det_ids (T,K) int32,
    rejected (1,) int64 counter, += 1 per rejected sequence).  One launch, no host synchronisation."""
    return _track_update("fdet_track_update", (), rows, counts, seq_offset, h_seq_offset, state, iou_threshold, alpha256, max_misses,
                         min_hits, emit_misses, birth_score, rejected)


def _track_update(entry, motion, rows, counts, seq_offset, h_seq_offset, state, iou_threshold, alpha256, max_misses, min_hits,
                  emit_misses, birth_score, rejected):
    """The two tracker entries: `motion` holds the integers fdet_track_update_motion takes after birth_score, or nothing."""
    import numpy as np
    if rows.dim() != 3 or rows.shape[2] != 5 or rows.dtype != F32:
        raise ValueError(f"track_update: rows must be (T,K,5) float32, got {tuple(rows.shape)} {rows.dtype}")
    T, K = int(rows.shape[0]), int(rows.shape[1])
    if not isinstance(h_seq_offset, np.ndarray) or h_seq_offset.dtype != np.int32 or h_seq_offset.ndim != 1 or \
            not h_seq_offset.flags.c_contiguous or h_seq_offset.size < 2:
        raise ValueError("track_update: h_seq_offset must be a contiguous (n_seq+1,) numpy int32 array")
    n = int(h_seq_offset.size) - 1
    if tuple(counts.shape) != (T,) or counts.dtype != I32 or tuple(seq_offset.shape) != (n + 1,) or seq_offset.dtype != I32:
        raise ValueError("track_update: counts must be (T,) int32 and seq_offset (n_seq+1,) int32")
    if state.dtype != torch.uint8 or state.numel() != n * TRACK_STATE_BYTES:
        raise ValueError(f"track_update: state must be {n * TRACK_STATE_BYTES} uint8 for {n} sequence(s), got {state.numel()}")
    dev = rows.device
    out_rows = torch.empty(T, TRACK_SLOTS, 5, dtype=F32, device=dev)
    out_ids = torch.empty(T, TRACK_SLOTS, dtype=I32, device=dev)
    out_misses = torch.empty(T, TRACK_SLOTS, dtype=I32, device=dev)
    out_counts = torch.empty(T, dtype=I32, device=dev)
    det_ids = torch.empty(T, K, dtype=I32, device=dev)
    if rejected is None:
        rejected = torch.zeros(1, dtype=torch.int64, device=dev)

    def p(t, dtype=F32):                                     # an empty tensor has no storage to point at
        return ptr(t, dtype) if t.numel() else None

    check(getattr(lib(), entry)(p(rows.contiguous()), p(counts.contiguous(), I32), ptr(seq_offset.contiguous(), I32),
                                h_seq_offset.ctypes.data, n, T, K, float(iou_threshold), int(alpha256), int(max_misses),
                                int(min_hits), int(emit_misses), float(birth_score), *motion,
                                ptr(state, torch.uint8), p(out_rows), p(out_ids, I32), p(out_misses, I32), p(out_counts, I32),
                                p(det_ids, I32), ptr(rejected, torch.int64), stream()), entry)
    return out_rows, out_ids, out_misses, out_counts, det_ids, rejected


def track_update_motion(rows: torch.Tensor, counts: torch.Tensor, seq_offset: torch.Tensor, h_seq_offset, state: torch.Tensor,
                        iou_threshold: float, alpha256: int, max_misses: int, min_hits: int, emit_misses: int, birth_score: float,
                        beta256: int, damp256: int, max_speed: int, grow256: int, rejected: Optional[torch.Tensor] = None):
    """fdet_track_update_motion: `track_update` with the constant-velocity motion model.  beta256 (0..256): gain of the
    velocity update; damp256 (0..256): what a missed track keeps of its velocity per frame; max_speed (0..1024): pixels per
    frame; grow256 (0..256): growth of the emitted box per missed frame.  The same arguments, state and results otherwise;
    the velocities live in reserved[0..1] of each track, and a state is driven by one of the two entries from fresh on."""
    return _track_update("fdet_track_update_motion", (int(beta256), int(damp256), int(max_speed), int(grow256)), rows, counts,
                         seq_offset, h_seq_offset, state, iou_threshold, alpha256, max_misses, min_hits, emit_misses, birth_score,
                         rejected)


TRACK_REFINE_ROWS, TRACK_REFINE_MAX_IDS = 256, 4096                 # FDET_TRACK_REFINE_* of include/fdet.h


def track_refine(det_rows: torch.Tensor, det_ids: torch.Tensor, trk_rows: torch.Tensor, trk_ids: torch.Tensor,
                 trk_misses: torch.Tensor, trk_counts: torch.Tensor, seq_offset: torch.Tensor, h_seq_offset, lookback: int,
                 grow256: int, stitch_gap: int, stitch_iou: float, min_length: int, rejected: Optional[torch.Tensor] = None):
    """fdet_track_refine over whole sequences: det_rows (T,K,5) the rows given to `track_update`, det_ids (T,K) int32 what it
    returned for them, trk_rows (T,128,5) / trk_ids / trk_misses (T,128) int32 / trk_counts (T,) int32 its outputs; seq_offset
    and h_seq_offset as there ->
    (out_rows (T,256,5), out_ids, out_misses, out_kind (T,256) int32, out_counts (T,) int32, rejected (2,) int64: [0] += 1 per
    rejected sequence, [1] += rows that found no room).  One launch, no host synchronisation."""
    import numpy as np
    if det_rows.dim() != 3 or det_rows.shape[2] != 5 or det_rows.dtype != F32:
        raise ValueError(f"track_refine: det_rows must be (T,K,5) float32, got {tuple(det_rows.shape)} {det_rows.dtype}")
    T, K = int(det_rows.shape[0]), int(det_rows.shape[1])
    if not isinstance(h_seq_offset, np.ndarray) or h_seq_offset.dtype != np.int32 or h_seq_offset.ndim != 1 or \
            not h_seq_offset.flags.c_contiguous or h_seq_offset.size < 2:
        raise ValueError("track_refine: h_seq_offset must be a contiguous (n_seq+1,) numpy int32 array")
    n = int(h_seq_offset.size) - 1
    if tuple(det_ids.shape) != (T, K) or det_ids.dtype != I32:
        raise ValueError(f"track_refine: det_ids must be ({T},{K}) int32, got {tuple(det_ids.shape)} {det_ids.dtype}")
    if tuple(trk_rows.shape) != (T, TRACK_SLOTS, 5) or trk_rows.dtype != F32:
        raise ValueError(f"track_refine: trk_rows must be ({T},{TRACK_SLOTS},5) float32, got {tuple(trk_rows.shape)} {trk_rows.dtype}")
    for name, t in (("trk_ids", trk_ids), ("trk_misses", trk_misses)):
        if tuple(t.shape) != (T, TRACK_SLOTS) or t.dtype != I32:
            raise ValueError(f"track_refine: {name} must be ({T},{TRACK_SLOTS}) int32, got {tuple(t.shape)} {t.dtype}")
    if tuple(trk_counts.shape) != (T,) or trk_counts.dtype != I32 or tuple(seq_offset.shape) != (n + 1,) or seq_offset.dtype != I32:
        raise ValueError("track_refine: trk_counts must be (T,) int32 and seq_offset (n_seq+1,) int32")
    dev = det_rows.device
    out_rows = torch.empty(T, TRACK_REFINE_ROWS, 5, dtype=F32, device=dev)
    out_ids = torch.empty(T, TRACK_REFINE_ROWS, dtype=I32, device=dev)
    out_misses = torch.empty(T, TRACK_REFINE_ROWS, dtype=I32, device=dev)
    out_kind = torch.empty(T, TRACK_REFINE_ROWS, dtype=I32, device=dev)
    out_counts = torch.empty(T, dtype=I32, device=dev)
    if rejected is None:
        rejected = torch.zeros(2, dtype=torch.int64, device=dev)
    if rejected.dtype != torch.int64 or rejected.numel() != 2:
        raise ValueError("track_refine: rejected must hold 2 int64")
    ws_bytes = int(lib().fdet_track_refine_ws_bytes(n, T))
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=I32, device=dev)

    def p(t, dtype=F32):                                     # an empty tensor has no storage to point at
        return ptr(t, dtype) if t.numel() else None

    check(lib().fdet_track_refine(p(det_rows.contiguous()), p(det_ids.contiguous(), I32), K, p(trk_rows.contiguous()),
                                  p(trk_ids.contiguous(), I32), p(trk_misses.contiguous(), I32), p(trk_counts.contiguous(), I32),
                                  ptr(seq_offset.contiguous(), I32), h_seq_offset.ctypes.data, n, T, int(lookback), int(grow256),
                                  int(stitch_gap), float(stitch_iou), int(min_length), p(out_rows), p(out_ids, I32),
                                  p(out_misses, I32), p(out_kind, I32), p(out_counts, I32), ptr(ws, I32), ws_bytes,
                                  ptr(rejected, torch.int64), stream()), "fdet_track_refine")
    return out_rows, out_ids, out_misses, out_kind, out_counts, rejected


# ------------------------------------------------------------------------------------------
# Face chips and the best-shot gallery (csrc/fdet_chips.hip; chips.py drives these)
# ------------------------------------------------------------------------------------------
CHIP_MIN_SIZE, CHIP_MAX_SIZE, CHIP_MAX_SIDE, CHIP_MAX_CHIPS = 8, 256, 8192, 1 << 20      # FDET_CHIP_* of include/fdet.h
CHIP_INFO_BYTES = CHIP_BEST_BYTES = 40                                # fdet_chip_info, fdet_chip_best


def chip_extract(bank_data: torch.Tensor, d_table: torch.Tensor, h_table, rows: torch.Tensor, counts: torch.Tensor, h_counts,
                 size: int, margin256: int, planar: bool = False):
    """fdet_chip_extract: one size x size chip per row j < counts[i] of rows (n,K,5) [score,x,y,w,h], cut from image i of the
    bank (bank_data / d_table / h_table as `tile_gather` takes them).  h_counts: the values of counts as a contiguous (n,)
    numpy int32 array -> (chips (M,size,size,3) uint8, or (M,3,size,size) when planar; info (M * 40,) uint8, M fdet_chip_info;
    h_chip_offset (n+1,) numpy int32, chip h_chip_offset[i] + j is row j of image i).  One launch, no host synchronisation."""
    import numpy as np
    n = len(h_table)
    if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != 5 or rows.dtype != F32:
        raise ValueError(f"chip_extract: rows must be ({n},K,5) float32, got {tuple(rows.shape)} {rows.dtype}")
    K, C = int(rows.shape[1]), int(size)
    if tuple(counts.shape) != (n,) or counts.dtype != I32:
        raise ValueError(f"chip_extract: counts must be ({n},) int32, got {tuple(counts.shape)} {counts.dtype}")
    if not isinstance(h_counts, np.ndarray) or h_counts.dtype != np.int32 or h_counts.shape != (n,) or not h_counts.flags.c_contiguous:
        raise ValueError(f"chip_extract: h_counts must be a contiguous ({n},) numpy int32 array")
    if d_table.numel() != n * 16:
        raise ValueError("chip_extract: device and host copies of the table differ in size")
    h_off = np.zeros(n + 1, np.int64)
    np.cumsum(np.clip(h_counts.astype(np.int64), 0, max(K, 0)), out=h_off[1:])          # a count outside 0..K is refused below
    M = int(h_off[-1])
    if M > CHIP_MAX_CHIPS:
        raise ValueError(f"chip_extract: {M} chips in one call, at most {CHIP_MAX_CHIPS}")
    h_off = np.ascontiguousarray(h_off.astype(np.int32))
    dev, U8 = bank_data.device, torch.uint8
    d_off = torch.from_numpy(h_off).to(dev)
    chips = torch.empty((M, 3, C, C) if planar else (M, C, C, 3), dtype=U8, device=dev)
    info = torch.empty(M * CHIP_INFO_BYTES, dtype=U8, device=dev)

    def p(t, dtype=U8):                                      # an empty tensor has no storage to point at
        return ptr(t, dtype) if t.numel() else None

    check(lib().fdet_chip_extract(ptr(bank_data, U8), ptr(d_table, U8), h_table.ctypes.data, n, p(rows.contiguous(), F32),
                                  ptr(counts.contiguous(), I32), h_counts.ctypes.data, ptr(d_off, I32), h_off.ctypes.data, K, C,
                                  int(margin256), int(bool(planar)), p(chips), p(info), stream()), "fdet_chip_extract")
    return chips, info, h_off


def chip_gallery_bytes(n_seq: int, capacity: int) -> int:
    return int(lib().fdet_chip_gallery_bytes(int(n_seq), int(capacity)))


def chip_best_update(chips: torch.Tensor, info: torch.Tensor, ids: torch.Tensor, seq_offset: torch.Tensor, h_seq_offset,
                     frame_base: torch.Tensor, capacity: int, min_side: int, min_inside256: int, gallery: torch.Tensor,
                     gallery_chips: torch.Tensor, scratch: torch.Tensor, overflow: torch.Tensor) -> None:
    """fdet_chip_best_update: chips (M,...) uint8 and info (M * 40,) uint8 as `chip_extract` returns them; ids (n,K) int32
    row-aligned with the rows the chips were cut from; seq_offset (n_seq+1,) int32 on the device and h_seq_offset, the same
    values as a numpy int32 array; frame_base (n_seq,) int32.  Updated in place: gallery (n_seq * capacity * 40,) uint8
    (zeros = empty), gallery_chips (n_seq, capacity, size*size*3) uint8, overflow (1,) int64 counter; scratch (n_seq *
    capacity,) int64 is cleared by the call.  Two launches, no host synchronisation."""
    import numpy as np
    if not isinstance(h_seq_offset, np.ndarray) or h_seq_offset.dtype != np.int32 or h_seq_offset.ndim != 1 or \
            not h_seq_offset.flags.c_contiguous or h_seq_offset.size < 2:
        raise ValueError("chip_best_update: h_seq_offset must be a contiguous (n_seq+1,) numpy int32 array")
    n_seq, G = int(h_seq_offset.size) - 1, int(capacity)
    M = int(chips.shape[0])
    if chips.dim() != 4 or chips.dtype != torch.uint8 or chips.shape[1:].numel() % 3 or info.dtype != torch.uint8 or \
            info.numel() != M * CHIP_INFO_BYTES:
        raise ValueError(f"chip_best_update: chips must be (M,C,C,3) or (M,3,C,C) uint8 and info M * {CHIP_INFO_BYTES} uint8")
    C = int(max(chips.shape[1:]))
    if chips.shape[1:].numel() != C * C * 3:
        raise ValueError(f"chip_best_update: chips of shape {tuple(chips.shape)} are not square RGB chips")
    if ids.dim() != 2 or ids.dtype != I32:
        raise ValueError(f"chip_best_update: ids must be (n_images,K) int32, got {tuple(ids.shape)} {ids.dtype}")
    if int(ids.shape[0]) != int(h_seq_offset[-1]):
        raise ValueError(f"chip_best_update: ids holds {int(ids.shape[0])} frames, seq_offset ends at {int(h_seq_offset[-1])}")
    if tuple(seq_offset.shape) != (n_seq + 1,) or seq_offset.dtype != I32 or tuple(frame_base.shape) != (n_seq,) or frame_base.dtype != I32:
        raise ValueError("chip_best_update: seq_offset must be (n_seq+1,) int32 and frame_base (n_seq,) int32")
    if G < 1 or gallery.dtype != torch.uint8 or gallery.numel() != n_seq * G * CHIP_BEST_BYTES or gallery_chips.dtype != torch.uint8 or \
            gallery_chips.numel() != n_seq * G * C * C * 3:
        raise ValueError(f"chip_best_update: gallery must be {n_seq} x {G} x {CHIP_BEST_BYTES} uint8 and gallery_chips {n_seq} x {G} x {C * C * 3}")
    if scratch.dtype != torch.int64 or scratch.numel() != n_seq * G or overflow.dtype != torch.int64 or overflow.numel() != 1:
        raise ValueError(f"chip_best_update: scratch must be {n_seq * G} int64 and overflow one int64")
    U8, I64 = torch.uint8, torch.int64

    def p(t, dtype=U8):
        return ptr(t, dtype) if t.numel() else None

    check(lib().fdet_chip_best_update(p(chips.contiguous()), p(info), M, C, p(ids.contiguous(), I32), int(ids.shape[1]),
                                      ptr(seq_offset.contiguous(), I32), h_seq_offset.ctypes.data, n_seq, ptr(frame_base, I32), G,
                                      int(min_side), int(min_inside256), ptr(gallery, U8), ptr(gallery_chips, U8),
                                      ptr(scratch, I64), ptr(overflow, I64), stream()), "fdet_chip_best_update")


# ------------------------------------------------------------------------------------------
# Baseline JPEG decode (csrc/fdet_jpeg.hip; datasets/jpeg.py drives these)
# ------------------------------------------------------------------------------------------
JPEG_UNSUPPORTED, JPEG_ECORRUPT = -4, -5                     # FDET_JPEG_* of include/fdet.h


def _jpeg_dtypes():
    import numpy as np
    info = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("restart_interval", "<i4"), ("hs", "<i4", (3,)),
                     ("vs", "<i4", (3,)), ("blocks_w", "<i4", (3,)), ("blocks_h", "<i4", (3,)), ("mcus_x", "<i4"),
                     ("mcus_y", "<i4"), ("coef_count", "<i8"), ("qt", "<u2", (3, 64))], align=True)          # fdet_jpeg_info_t
    desc = np.dtype([("bank_offset", "<i8"), ("coef_offset", "<i8", (3,)), ("plane_offset", "<i8", (3,)), ("width", "<i4"),
                     ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("blocks_w", "<i4", (3,)),
                     ("blocks_h", "<i4", (3,)), ("reserved", "<i4"), ("qt", "<u2", (3, 64))], align=True)    # fdet_jpeg_desc
    assert info.itemsize == 464 and desc.itemsize == 488
    return info, desc


JPEG_INFO_DTYPE, JPEG_DESC_DTYPE = _jpeg_dtypes()


def jpeg_info(data: bytes):
    """fdet_jpeg_info on the bytes of one file (host only, thread-safe) -> (rc, info record | None, message).  rc 0: a
    baseline JPEG of the supported subset; JPEG_UNSUPPORTED: a JPEG another decoder must take; JPEG_ECORRUPT / -1: broken."""
    import numpy as np
    L = lib()
    out = np.zeros(1, dtype=JPEG_INFO_DTYPE)
    rc = L.fdet_jpeg_info(data, len(data), out.ctypes.data)
    if rc != 0:
        return rc, None, L.fdet_last_error().decode(errors="replace")       # the message is thread-local: read it here
    return 0, out[0], ""


def jpeg_entropy_decode(data: bytes, coef_ptr: int, capacity: int):
    """fdet_jpeg_entropy_decode (host only, thread-safe; ctypes releases the GIL): the scan of `data` -> `capacity` int16
    coefficients at host address `coef_ptr`.  -> (rc, message)."""
    L = lib()
    rc = L.fdet_jpeg_entropy_decode(data, len(data), coef_ptr, capacity)
    return rc, ("" if rc == 0 else L.fdet_last_error().decode(errors="replace"))


def jpeg_reconstruct(coef: torch.Tensor, d_descs: torch.Tensor, h_descs, workspace: torch.Tensor, bank_data: torch.Tensor) -> None:
    """fdet_jpeg_reconstruct: device int16 coefficients + one fdet_jpeg_desc per image (device uint8 view and the numpy record
    array) -> RGB written into the bank's byte buffer, on the current stream.  Bad descriptors raise before anything runs."""
    import numpy as np
    if not isinstance(h_descs, np.ndarray) or h_descs.dtype != JPEG_DESC_DTYPE or h_descs.ndim != 1 or not h_descs.flags.c_contiguous:
        raise ValueError("jpeg_reconstruct: h_descs must be a contiguous (n,) record array of JPEG_DESC_DTYPE")
    if d_descs.numel() != len(h_descs) * JPEG_DESC_DTYPE.itemsize:
        raise ValueError("jpeg_reconstruct: device and host copies of the descriptors differ in size")
    U8 = torch.uint8
    check(lib().fdet_jpeg_reconstruct(ptr(coef, torch.int16), coef.numel(), ptr(d_descs, U8), h_descs.ctypes.data, len(h_descs),
                                      ptr(workspace, U8), workspace.numel(), ptr(bank_data, U8), bank_data.numel(), stream()),
          "fdet_jpeg_reconstruct")


# ------------------------------------------------------------------------------------------
# Huffman decoding of JPEG scans on the device (csrc/fdet_jpeg_huff.hip; datasets/jpeg.py huffman="device" drives these)
# ------------------------------------------------------------------------------------------
JPEG_HUFF_HOST = 1                                           # FDET_JPEG_HUFF_* of include/fdet.h
JPEG_HUFF_END = 0x80000000
JPEG_HUFF_NOCODE, JPEG_HUFF_RUN, JPEG_HUFF_DCCAT, JPEG_HUFF_EXHAUSTED, JPEG_HUFF_TRAILING = 1, 2, 4, 8, 16


def _jpeg_huff_dtypes():
    import numpy as np
    table = np.dtype([("look_nbits", "u1", (512,)), ("look_sym", "u1", (512,)), ("maxcode", "<i4", (18,)),
                      ("valoffset", "<i4", (18,)), ("vals", "u1", (256,)), ("nvals", "<i4"), ("reserved", "<i4")], align=True)
    tables = np.dtype([("dc", table, (3,)), ("ac", table, (3,))], align=True)                                # fdet_jpeg_huff_tables
    seg = np.dtype([("byte_offset", "<i8"), ("byte_len", "<i4"), ("first_mcu", "<i4"), ("mcu_count", "<i4"), ("image", "<i4"),
                    ("sub_first", "<i4"), ("sub_count", "<i4")], align=True)                                 # fdet_jpeg_huff_segment
    image = np.dtype([("coef_offset", "<i8", (3,)), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("mcus_x", "<i4"),
                      ("mcus_y", "<i4"), ("seg_first", "<i4"), ("seg_count", "<i4"), ("sub_first", "<i4"), ("sub_count", "<i4"),
                      ("wg_first", "<i4"), ("reserved", "<i4", (2,))], align=True)                                                # fdet_jpeg_huff_image
    assert table.itemsize == 1432 and tables.itemsize == 8592 and seg.itemsize == 32 and image.itemsize == 72
    return tables, seg, image


JPEG_HUFF_TABLES_DTYPE, JPEG_HUFF_SEG_DTYPE, JPEG_HUFF_IMAGE_DTYPE = _jpeg_huff_dtypes()


def jpeg_scan_prepare(data: bytes, scan_ptr: int, scan_capacity: int, segs_ptr: int, seg_capacity: int, tables_ptr: int):
    """fdet_jpeg_scan_prepare (host only, thread-safe; ctypes releases the GIL): the file `data` -> its unstuffed segments
    at host address `scan_ptr`, `seg_capacity` fdet_jpeg_huff_segment records at `segs_ptr` and one fdet_jpeg_huff_tables at
    `tables_ptr`.  -> (rc, scan bytes used, segments, message); rc JPEG_HUFF_HOST: decode this image on the host."""
    import ctypes
    L = lib()
    used, nseg = ctypes.c_size_t(0), ctypes.c_int(0)
    rc = L.fdet_jpeg_scan_prepare(data, len(data), scan_ptr, scan_capacity, ctypes.addressof(used), segs_ptr, seg_capacity,
                                  ctypes.addressof(nseg), tables_ptr)
    if rc == 0:
        return 0, int(used.value), int(nseg.value), ""
    return rc, 0, 0, ("decode on the host" if rc == JPEG_HUFF_HOST else L.fdet_last_error().decode(errors="replace"))


def jpeg_scan_prepare_arrays(data: bytes, seg_capacity=None, scan_capacity=None):
    """jpeg_scan_prepare into fresh numpy arrays -> (rc, scan uint8 (used,), segments (n,) of JPEG_HUFF_SEG_DTYPE, tables
    (1,) of JPEG_HUFF_TABLES_DTYPE, message).  The capacities default to what always suffices."""
    import numpy as np
    rc, info, msg = jpeg_info(data)
    if rc != 0:
        return rc, None, None, None, msg
    mcus = int(info["mcus_x"]) * int(info["mcus_y"])
    ri = int(info["restart_interval"]) or mcus
    nseg = -(-mcus // ri) if seg_capacity is None else int(seg_capacity)
    cap = (len(data) + 15) // 16 * 16 + 16 * nseg if scan_capacity is None else int(scan_capacity)
    scan = np.zeros(max(cap, 1), np.uint8)
    segs = np.zeros(max(nseg, 1), JPEG_HUFF_SEG_DTYPE)
    tables = np.zeros(1, JPEG_HUFF_TABLES_DTYPE)
    rc, used, n, msg = jpeg_scan_prepare(data, scan.ctypes.data, cap, segs.ctypes.data, nseg, tables.ctypes.data)
    if rc != 0:
        return rc, None, None, None, msg
    return 0, scan[:used], segs[:n], tables, ""


def jpeg_huff_layout(images, segs, sub_bits: int) -> int:
    """Fill the subsequence ranges (segments: sub_first, sub_count; images: sub_first, sub_count, wg_first) that follow from
    the segments' byte_len and `sub_bits`, in place.  `images` must already hold seg_first / seg_count.  -> subsequences."""
    import numpy as np
    bits = segs["byte_len"].astype(np.int64) * 8
    cnt = np.maximum(1, -(-bits // int(sub_bits)))
    first = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    if total > 0x7fffffff:
        raise N.FdetError(f"jpeg_huff_layout: {total} subsequences are more than one launch takes")
    segs["sub_count"], segs["sub_first"] = cnt, first
    ends = np.concatenate([first, [total]])
    images["sub_first"] = ends[images["seg_first"]]
    images["sub_count"] = ends[images["seg_first"] + images["seg_count"]] - images["sub_first"]
    wgs = -(-images["sub_count"].astype(np.int64) // 256)
    images["wg_first"] = np.cumsum(wgs) - wgs
    return total


def _jpeg_huff_args(who, scan, d_tables, d_images, h_images, d_segs, h_segs, state):
    import numpy as np
    for name, h, dt, d in (("h_images", h_images, JPEG_HUFF_IMAGE_DTYPE, d_images), ("h_segs", h_segs, JPEG_HUFF_SEG_DTYPE, d_segs)):
        if not isinstance(h, np.ndarray) or h.dtype != dt or h.ndim != 1 or not h.flags.c_contiguous:
            raise ValueError(f"{who}: {name} must be a contiguous (n,) record array of its dtype")
        if d.numel() != len(h) * dt.itemsize:
            raise ValueError(f"{who}: device and host copies of {name} differ in size")
    if d_tables.numel() != len(h_images) * JPEG_HUFF_TABLES_DTYPE.itemsize:
        raise ValueError(f"{who}: one fdet_jpeg_huff_tables per image is expected")
    if state.numel() % 3:
        raise ValueError(f"{who}: state holds three words per subsequence")


def jpeg_huffman_sync(scan: torch.Tensor, d_tables: torch.Tensor, d_images: torch.Tensor, h_images, d_segs: torch.Tensor, h_segs,
                      sub_bits: int, state: torch.Tensor, changed: torch.Tensor) -> None:
    """fdet_jpeg_huffman_sync: ONE synchronisation pass on the current stream.  scan / d_tables / d_images / d_segs device
    uint8, state device int64 (3 words per subsequence, zero-filled before the first pass), changed device int32 (one word
    per image, zero-filled by the caller).  Bad descriptors raise before anything runs."""
    _jpeg_huff_args("jpeg_huffman_sync", scan, d_tables, d_images, h_images, d_segs, h_segs, state)
    if changed.numel() < len(h_images):
        raise ValueError("jpeg_huffman_sync: one `changed` word per image is expected")
    U8 = torch.uint8
    check(lib().fdet_jpeg_huffman_sync(ptr(scan, U8), scan.numel(), ptr(d_tables, U8), ptr(d_images, U8), h_images.ctypes.data,
                                       len(h_images), ptr(d_segs, U8), h_segs.ctypes.data, len(h_segs), int(sub_bits),
                                       ptr(state, torch.int64), state.numel() // 3, ptr(changed, I32), stream()),
          "fdet_jpeg_huffman_sync")


def jpeg_huffman_emit(scan: torch.Tensor, d_tables: torch.Tensor, d_images: torch.Tensor, h_images, d_segs: torch.Tensor, h_segs,
                      sub_bits: int, state: torch.Tensor, first_block: torch.Tensor, coef: torch.Tensor, flags: torch.Tensor) -> None:
    """fdet_jpeg_huffman_emit on the current stream: converged states -> the int16 coefficient planes of `coef` (zeroed here),
    byte for byte fdet_jpeg_entropy_decode's; flags device int32, one word per image, zero-filled by the caller."""
    _jpeg_huff_args("jpeg_huffman_emit", scan, d_tables, d_images, h_images, d_segs, h_segs, state)
    if flags.numel() < len(h_images) or first_block.numel() < state.numel() // 3:
        raise ValueError("jpeg_huffman_emit: one flag word per image and one first_block word per subsequence are expected")
    U8 = torch.uint8
    check(lib().fdet_jpeg_huffman_emit(ptr(scan, U8), scan.numel(), ptr(d_tables, U8), ptr(d_images, U8), h_images.ctypes.data,
                                       len(h_images), ptr(d_segs, U8), h_segs.ctypes.data, len(h_segs), int(sub_bits),
                                       ptr(state, torch.int64), state.numel() // 3, ptr(first_block, I32), ptr(coef, torch.int16),
                                       coef.numel(), ptr(flags, I32), stream()),
          "fdet_jpeg_huffman_emit")


# ------------------------------------------------------------------------------------------
# Baseline JPEG encode (csrc/fdet_jpeg_enc.hip; datasets/jpeg.py DeviceJpegEncoder drives these)
# ------------------------------------------------------------------------------------------
JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}     # FDET_JPEG_SUB_*: PIL's numbering
JPEG_ENC_MAX_BLOCK_BITS = 11 + 16 + 63 * (16 + 10)
JPEG_ENC_MAX_BLOCKS = 1 << 20
JPEG_ENC_HEADER_BYTES = 623


def _jpeg_enc_dtype():
    import numpy as np
    d = np.dtype([("bank_offset", "<i8"), ("block_base", "<i8"), ("scan_offset", "<i8"), ("width", "<i4"), ("height", "<i4"),
                  ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("n_blocks", "<i4"), ("reserved", "<i4")], align=True)   # fdet_jpeg_enc_desc
    assert d.itemsize == 48
    return d


JPEG_ENC_DESC_DTYPE = _jpeg_enc_dtype()


def jpeg_quant_tables(quality: int):
    """fdet_jpeg_quant_tables (host only) -> uint16 (2, 64): luminance and chrominance table of `quality`, natural order."""
    import numpy as np
    out = np.zeros((2, 64), dtype=np.uint16)
    check(lib().fdet_jpeg_quant_tables(int(quality), out.ctypes.data), "fdet_jpeg_quant_tables")
    return out


def jpeg_write_header(width: int, height: int, quality: int, subsampling: int) -> bytes:
    """fdet_jpeg_write_header (host only, thread-safe) -> the bytes of a file in front of its scan (SOI .. SOS)."""
    import ctypes
    buf = ctypes.create_string_buffer(JPEG_ENC_HEADER_BYTES)
    n = ctypes.c_size_t(0)
    check(lib().fdet_jpeg_write_header(int(width), int(height), int(quality), int(subsampling), buf, JPEG_ENC_HEADER_BYTES,
                                       ctypes.byref(n)), "fdet_jpeg_write_header")
    return buf.raw[:n.value]


def jpeg_enc_ws_bytes(total_blocks: int, n_images: int) -> int:
    n = int(lib().fdet_jpeg_enc_ws_bytes(int(total_blocks), int(n_images)))
    if n == 0:
        raise N.FdetError(f"fdet_jpeg_enc_ws_bytes: no plan over {total_blocks} blocks of {n_images} images")
    return n


def _jpeg_enc_descs(who: str, d_descs: torch.Tensor, h_descs) -> None:
    import numpy as np
    if not isinstance(h_descs, np.ndarray) or h_descs.dtype != JPEG_ENC_DESC_DTYPE or h_descs.ndim != 1 or not h_descs.flags.c_contiguous:
        raise ValueError(f"{who}: h_descs must be a contiguous (n,) record array of JPEG_ENC_DESC_DTYPE")
    if d_descs.numel() != len(h_descs) * JPEG_ENC_DESC_DTYPE.itemsize:
        raise ValueError(f"{who}: device and host copies of the descriptors differ in size")


def jpeg_enc_plan(bank_data: torch.Tensor, d_descs: torch.Tensor, h_descs, quality: int, subsampling: int,
                  workspace: torch.Tensor) -> None:
    """fdet_jpeg_enc_plan: the images the descriptors name -> coefficients, block bit lengths, bit offsets and per-image bit
    totals in `workspace` (layout: include/fdet.h), on the current stream.  Bad descriptors raise before anything runs."""
    _jpeg_enc_descs("jpeg_enc_plan", d_descs, h_descs)
    U8 = torch.uint8
    check(lib().fdet_jpeg_enc_plan(ptr(bank_data, U8), bank_data.numel(), ptr(d_descs, U8), h_descs.ctypes.data, len(h_descs),
                                   int(quality), int(subsampling), ptr(workspace, U8), workspace.numel(), stream()),
          "fdet_jpeg_enc_plan")


def jpeg_enc_emit(d_descs: torch.Tensor, h_descs, h_totals, subsampling: int, workspace: torch.Tensor, scan: torch.Tensor) -> None:
    """fdet_jpeg_enc_emit: the planned blocks' bits -> `scan` (device uint8, zero-filled by the caller on the current stream),
    image i at h_descs[i]["scan_offset"].  h_totals: the plan's per-image bit totals, read back by the caller (uint32 (n,))."""
    import numpy as np
    _jpeg_enc_descs("jpeg_enc_emit", d_descs, h_descs)
    if not isinstance(h_totals, np.ndarray) or h_totals.dtype != np.uint32 or h_totals.shape != (len(h_descs),) or not h_totals.flags.c_contiguous:
        raise ValueError("jpeg_enc_emit: h_totals must be a contiguous (n,) uint32 array")
    U8 = torch.uint8
    check(lib().fdet_jpeg_enc_emit(ptr(d_descs, U8), h_descs.ctypes.data, h_totals.ctypes.data, len(h_descs), int(subsampling),
                                   ptr(workspace, U8), workspace.numel(), ptr(scan, U8), scan.numel(), stream()),
          "fdet_jpeg_enc_emit")


# ------------------------------------------------------------------------------------------
# SSD detection math (datasets/WIDERFace/dataset_ssd.py, losses/SSDLoss.py, datasets/utils.py:8-92)
# ------------------------------------------------------------------------------------------
SSD_PATCH_SIZES = (60, 30, 15, 7)


def _ps_array(patch_sizes):
    import ctypes
    ps = [int(p) for p in patch_sizes]
    return (ctypes.c_int * len(ps))(*ps), len(ps)


def ssd_num_priors(patch_sizes=SSD_PATCH_SIZES) -> int:
    arr, n = _ps_array(patch_sizes)
    P = int(lib().fdet_ssd_num_priors(arr, n))
    if P < 0:
        raise N.FdetError("ssd_num_priors: bad patch sizes")
    return P


def ssd_encode_targets(boxes: Sequence[torch.Tensor], img_size: Tuple[int, int], patch_sizes=SSD_PATCH_SIZES,
                       device=None) -> torch.Tensor:
    """Batched multi-scale SSD target encode: list of (n_i,5) [conf,x,y,w,h] -> (B,P,5) on the GPU."""
    B = len(boxes)
    device = device or torch.device("cuda", torch.cuda.current_device())
    counts = [int(b.shape[0]) if b.numel() else 0 for b in boxes]
    offs = torch.zeros(B + 1, dtype=I32)
    offs[1:] = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0).to(I32)
    rows = [b.reshape(-1, 5).to(F32).cpu() for b in boxes if b.numel()]
    flat = (torch.cat(rows, 0) if rows else torch.zeros(1, 5)).contiguous().to(device)
    arr, ns = _ps_array(patch_sizes)
    out = torch.empty(B, ssd_num_priors(patch_sizes), 5, dtype=F32, device=device)
    if B:
        check(lib().fdet_ssd_encode_targets(ptr(flat), ptr(offs.to(device), I32), B, arr, ns, float(img_size[0]),
                                            float(img_size[1]), ptr(out), stream()), "fdet_ssd_encode_targets")
    return out


def ssd_encode_targets_device(rows: torch.Tensor, box_offset: torch.Tensor, img_size: Tuple[int, int],
                              patch_sizes=SSD_PATCH_SIZES) -> torch.Tensor:
    """ssd_encode_targets on rows already on the device (layout of encode_targets_device) -> (B,P,5)."""
    rows, box_offset, B = _device_rows(rows, box_offset)
    arr, ns = _ps_array(patch_sizes)
    out = torch.empty(B, ssd_num_priors(patch_sizes), 5, dtype=F32, device=rows.device)
    check(lib().fdet_ssd_encode_targets(ptr(rows), ptr(box_offset, I32), B, arr, ns, float(img_size[0]),
                                        float(img_size[1]), ptr(out), stream()), "fdet_ssd_encode_targets")
    return out


def ssd_loss_fwd_bwd(pred: torch.Tensor, target: torch.Tensor, neg_pos_ratio: int = 10, want_grad: bool = True,
                     want_mask: bool = False):
    """ssd_loss(pred[:,:,0], pred[:,:,1:], target[:,:,0], target[:,:,1:], ratio): (loss (1,), grad or None, mask or None)."""
    pred, target = _f32(pred), _f32(target)
    if pred.dim() != 3 or pred.shape[2] != 5 or pred.shape != target.shape:
        raise ValueError(f"ssd_loss: expected matching (B,P,5) tensors, got {tuple(pred.shape)} / {tuple(target.shape)}")
    B, P, _ = pred.shape
    loss = torch.empty(1, dtype=F32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    mask = torch.empty(B, P, dtype=torch.uint8, device=pred.device) if want_mask else None
    ws = torch.empty(int(lib().fdet_ssd_loss_ws_bytes(B)) // 8 + 1, dtype=torch.float64, device=pred.device)
    check(lib().fdet_ssd_loss_fwd_bwd(ptr(pred), ptr(target), B, P, int(neg_pos_ratio), ptr(loss), ptr(grad),
                                      ptr(mask, torch.uint8), ptr(ws, torch.float64), ws.numel() * 8, stream()),
          "fdet_ssd_loss_fwd_bwd")
    return loss, grad, mask


def ssd_loss_parts(pred: torch.Tensor, target: torch.Tensor, neg_pos_ratio: int = 10, want_grad: bool = True):
    """Data-parallel half of ssd_loss: (sums (3,) f64 = [BCE, smooth-L1, positives] of THIS shard, UNSCALED grad or None)."""
    pred, target = _f32(pred), _f32(target)
    if pred.dim() != 3 or pred.shape[2] != 5 or pred.shape != target.shape:
        raise ValueError(f"ssd_loss: expected matching (B,P,5) tensors, got {tuple(pred.shape)} / {tuple(target.shape)}")
    B, P, _ = pred.shape
    sums = torch.empty(3, dtype=torch.float64, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    ws = torch.empty(int(lib().fdet_ssd_loss_ws_bytes(B)) // 8 + 1, dtype=torch.float64, device=pred.device)
    check(lib().fdet_ssd_loss_parts(ptr(pred), ptr(target), B, P, int(neg_pos_ratio), ptr(grad), None, ptr(sums, torch.float64),
                                    ptr(ws, torch.float64), ws.numel() * 8, stream()), "fdet_ssd_loss_parts")
    return sums, grad


def ssd_loss_finish(sums: torch.Tensor, grad: Optional[torch.Tensor]) -> torch.Tensor:
    """loss (1,) from the batch-wide sums (after the caller's SUM all-reduce); scales `grad` in place by 1 / positives."""
    if sums.dtype != torch.float64 or sums.numel() != 3:
        raise ValueError("ssd_loss_finish: sums must be the (3,) float64 tensor of ssd_loss_parts")
    loss = torch.empty(1, dtype=F32, device=sums.device)
    ws = torch.empty(4, dtype=F32, device=sums.device)
    check(lib().fdet_ssd_loss_finish(ptr(sums, torch.float64), ptr(loss), ptr(grad), grad.numel() if grad is not None else 0,
                                     ptr(ws), 16, stream()), "fdet_ssd_loss_finish")
    return loss


def ssd_reduce_bounding_boxes(x: torch.Tensor, prob_threshold: float, iou_threshold: float, img_w: float, img_h: float,
                              patch_sizes=SSD_PATCH_SIZES, with_priors: bool = True, priors: torch.Tensor = None):
    """Batched ReduceSSDBoundingBoxes.forward: (B,P,5) -> (rows (B,P,5), counts (B,)).  priors: optional (P,4) table
    (datasets/utils.py:31-32), None = the reference's calculate_priors()."""
    x = _f32(x)
    B, P, five = x.shape
    if five != 5 or P != ssd_num_priors(patch_sizes):
        raise ValueError(f"ssd_reduce_bounding_boxes: expected (B,{ssd_num_priors(patch_sizes)},5), got {tuple(x.shape)}")
    arr, ns = _ps_array(patch_sizes)
    out = torch.zeros(B, P, 5, dtype=F32, device=x.device)
    counts = torch.zeros(B, dtype=I32, device=x.device)
    if priors is not None:
        priors = _f32(priors.to(x.device))
        if tuple(priors.shape) != (P, 4):
            raise ValueError(f"ssd_reduce_bounding_boxes: priors must be ({P},4), got {tuple(priors.shape)}")
    check(lib().fdet_ssd_reduce_bounding_boxes_priors(ptr(x), B, arr, ns, int(bool(with_priors)), ptr(priors), float(prob_threshold),
                                                      float(iou_threshold), float(img_w), float(img_h), ptr(out),
                                                      ptr(counts, I32), stream()), "fdet_ssd_reduce_bounding_boxes")
    return out, counts


def ssd_head_pack_fwd(z: torch.Tensor, ps: int, prior_start: int, y: torch.Tensor) -> None:
    Nn, CP, H, W = z.shape
    if H != ps or W != ps or y.dim() != 3 or y.shape[0] != Nn or y.shape[2] != 5:
        raise ValueError("ssd_head_pack_fwd: shape mismatch")
    check(lib().fdet_ssd_head_pack_fwd(ptr(z), Nn, CP, ps, int(prior_start), y.shape[1], ptr(y), stream()), "fdet_ssd_head_pack_fwd")


def ssd_head_pack_bwd(dy: torch.Tensor, y: torch.Tensor, ps: int, prior_start: int, dz: torch.Tensor) -> None:
    Nn, CP, H, W = dz.shape
    if H != ps or W != ps or dy.shape != y.shape or y.shape[0] != Nn or y.shape[2] != 5:
        raise ValueError("ssd_head_pack_bwd: shape mismatch")
    check(lib().fdet_ssd_head_pack_bwd(ptr(dy), ptr(y), Nn, CP, ps, int(prior_start), y.shape[1], ptr(dz), stream()), "fdet_ssd_head_pack_bwd")


def u8_to_f32_norm(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.dtype != torch.uint8:
        raise TypeError("u8_to_f32_norm expects uint8")
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=F32, device=x.device)
    elif tuple(out.shape) != tuple(x.shape):
        raise ValueError("u8_to_f32_norm: out shape differs")
    check(lib().fdet_u8_to_f32_norm(ptr(x, torch.uint8), ptr(out), x.numel(), stream()), "fdet_u8_to_f32_norm")
    return out


def resize_bilinear_norm(x: torch.Tensor, size: Tuple[int, int], divisor: float = 255.0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Resize(size)(x) / 255.0` on the device (torchvision 0.11.2 tensor semantics: bilinear,
    align_corners=False, no antialias).  uint8 input goes through the uint8 round trip (round half
    even) before the division; float input is interpolated and divided.  (N,C,H,W) or (C,H,W)."""
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError(f"resize_bilinear_norm: expected (N,C,H,W) or (C,H,W), got {tuple(x.shape)}")
    x = x.contiguous()
    Nn, C, Hs, Ws = x.shape
    Hd, Wd = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty(Nn, C, Hd, Wd, dtype=F32, device=x.device)
    else:
        _chk4(out, (Nn, C, Hd, Wd), "out")
    if x.dtype == torch.uint8:
        if divisor != 255.0:
            raise ValueError("resize_bilinear_norm: the uint8 path always divides by 255")
        check(lib().fdet_resize_bilinear_u8_norm(ptr(x, torch.uint8), ptr(out), Nn, C, Hs, Ws, Hd, Wd, stream()),
              "fdet_resize_bilinear_u8_norm")
    else:
        check(lib().fdet_resize_bilinear_f32_norm(ptr(_f32(x)), ptr(out), Nn, C, Hs, Ws, Hd, Wd, float(divisor), stream()),
              "fdet_resize_bilinear_f32_norm")
    return out


# ------------------------------------------------------------------------------------------
# optimiser / dropout
# ------------------------------------------------------------------------------------------
def adam_step(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int,
              lr: float = 1e-4, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
              grad_scale: float = 1.0) -> None:
    n = param.numel()
    if not (grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == n):
        raise ValueError("adam_step: buffer sizes differ")
    check(lib().fdet_adam_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), n, int(step), float(lr),
                               float(beta1), float(beta2), float(eps), float(grad_scale), stream()), "fdet_adam_step")


def dropout_scales(out: torch.Tensor, p: float, seed: int, offset: int) -> torch.Tensor:
    check(lib().fdet_dropout_scales(ptr(out), out.numel(), float(p), int(seed) & (2**64 - 1),
                                    int(offset) & (2**64 - 1), stream()), "fdet_dropout_scales")
    return out


def dropout_scales_layers(n: int, channels: Sequence[int], p: Sequence[float], seed: int, base: int, first_image: int,
                          device) -> List[torch.Tensor]:
    """Dropout2d scales of every dropout layer in one launch (fdet_dropout_scales_layers): returns one dense
    (n, channels[k]) tensor per layer (views into one buffer).  The counter is indexed by the global image number
    `first_image + i`, so data-parallel ranks draw what a single process draws for the concatenated batch."""
    import ctypes
    L = len(channels)
    if L != len(p) or not (1 <= L <= 32):
        raise ValueError("dropout_scales_layers: 1..32 layers, one p per layer")
    ls = int(sum(channels))
    buf = torch.empty(max(n * ls, 1), dtype=F32, device=device)
    ch = (ctypes.c_int * L)(*[int(c) for c in channels])
    pp = (ctypes.c_float * L)(*[float(v) for v in p])
    m64 = 2**64 - 1
    check(lib().fdet_dropout_scales_layers(ptr(buf), int(n), L, ch, pp, int(seed) & m64, int(base) & m64,
                                           int(first_image) & m64, stream()), "fdet_dropout_scales_layers")
    out, off = [], 0
    for c in channels:
        out.append(buf[off:off + n * c].view(n, c))
        off += n * c
    return out


# ------------------------------------------------------------------------------------------
# conv stack primitives (shapes are validated here; the kernels trust them)
# ------------------------------------------------------------------------------------------
def _chk4(t: torch.Tensor, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def packed_sizes(cout: int, cin: int) -> Tuple[int, int]:
    cop, cip = (cout + 31) // 32 * 32, (cin + 31) // 32 * 32
    return cin * 9 * cop, cout * 9 * cip


def x3_supported(cout: int, cin: int) -> bool:
    """bf16x3 conv kernels need channel counts that are multiples of 16."""
    return cout % 16 == 0 and cin % 16 == 0


def pack_conv3x3_weights(w: torch.Tensor, wpk_fwd: Optional[torch.Tensor], wpk_bwd: Optional[torch.Tensor],
                         x3: bool = False) -> None:
    """x3=True packs the bf16 hi/lo panels of the bf16x3 kernels (same buffer sizes)."""
    cout, cin, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise ValueError("pack_conv3x3_weights: 3x3 kernels only")
    nf, nb = packed_sizes(cout, cin)
    if wpk_fwd is not None and wpk_fwd.numel() != nf:
        raise ValueError(f"wpk_fwd must hold {nf} floats")
    if wpk_bwd is not None and wpk_bwd.numel() != nb:
        raise ValueError(f"wpk_bwd must hold {nb} floats")
    fn = lib().fdet_pack_conv3x3_weights_bf16x3 if x3 else lib().fdet_pack_conv3x3_weights
    check(fn(ptr(w), cout, cin, ptr(wpk_fwd), ptr(wpk_bwd), stream()), "fdet_pack_conv3x3_weights")


def pack_conv3x3_weights_batched(ws, wpk_fwds, wpk_bwds) -> None:
    """bf16x3 panels of len(ws) same-shape layers in one launch."""
    cout, cin, kh, kw = ws[0].shape
    if (kh, kw) != (3, 3):
        raise ValueError("pack_conv3x3_weights_batched: 3x3 kernels only")
    nf, nb = packed_sizes(cout, cin)
    for w, f_, b_ in zip(ws, wpk_fwds, wpk_bwds):
        _chk4(w, (cout, cin, 3, 3), "w")
        if f_.numel() != nf or b_.numel() != nb:
            raise ValueError("pack_conv3x3_weights_batched: packed buffer size does not match (Cout,Cin)")
    import ctypes
    arr = ctypes.c_void_p * len(ws)
    check(lib().fdet_pack_conv3x3_weights_bf16x3_batched(arr(*[ptr(w) for w in ws]), len(ws), cout, cin,
                                                         arr(*[ptr(t) for t in wpk_fwds]), arr(*[ptr(t) for t in wpk_bwds]),
                                                         stream()), "fdet_pack_conv3x3_weights_bf16x3_batched")


def _p16_fn(name: str, x3: bool, p16: bool):
    """The C entry of a conv op: `<name>_bf16` (precision16: one bf16 MFMA pass, bf16-rounded stores; include/fdet.h),
    `<name>_bf16x3`, or the exact-fp32 `<name>`.  precision16 exists only beside the bf16x3 kernels."""
    if p16:
        if not x3:
            raise ValueError(f"{name}: precision16 (p16=True) runs on the bf16 matrix-core kernels only (x3=True)")
        return getattr(lib(), name + "_bf16")
    return getattr(lib(), name + "_bf16x3") if x3 else getattr(lib(), name)


def conv3x3_fwd(x, wpk, bias, cout: int, y_full=None, skip=None, drop_scale=None, y_out=None, slope: float = 0.2,
                x3: bool = False, p16: bool = False):
    Nn, cin, H, W = x.shape
    if wpk.numel() != packed_sizes(cout, cin)[0]:
        raise ValueError("conv3x3_fwd: packed weight size does not match (Cout,Cin)")
    for t, nm in ((y_full, "y_full"), (skip, "skip"), (y_out, "y_out")):
        if t is not None:
            _chk4(t, (Nn, cout, H, W), nm)
    if bias is not None:
        _chk4(bias, (cout,), "bias")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, cout), "drop_scale")
    fn = _p16_fn("fdet_conv3x3_fwd", x3, p16)
    check(fn(ptr(x), ptr(wpk), ptr(bias), ptr(y_full), ptr(skip), ptr(drop_scale), ptr(y_out),
             Nn, cin, cout, H, W, 1, float(slope), stream()), "fdet_conv3x3_fwd")


def conv3x3_dgrad(dz, wpk_bwd, cin: int, dx, act=None, add=None, slope: float = 0.2, x3: bool = False, p16: bool = False):
    Nn, cout, H, W = dz.shape
    if wpk_bwd.numel() != packed_sizes(cout, cin)[1]:
        raise ValueError("conv3x3_dgrad: packed weight size does not match (Cout,Cin)")
    _chk4(dx, (Nn, cin, H, W), "dx")
    for t, nm in ((act, "act"), (add, "add")):
        if t is not None:
            _chk4(t, (Nn, cin, H, W), nm)
    fn = _p16_fn("fdet_conv3x3_dgrad", x3, p16)
    check(fn(ptr(dz), ptr(wpk_bwd), ptr(act), ptr(add), ptr(dx), Nn, cin, cout, H, W, float(slope), stream()),
          "fdet_conv3x3_dgrad")


X3_ROUTE_FIELDS = ("family", "vw", "mt", "mode", "seg", "p16")
X3_FAMILIES = {2: "al", 3: "sb", 4: "general"}


def conv3x3_x3_last_route() -> dict:
    """Kernel route of the last bf16x3 / precision16 conv3x3 forward, data-gradient or pooled launch on this thread
    (fdet_conv3x3_x3_last_route): family ("al", "sb", "general"; None after a refused call), vector width VW, MT,
    epilogue mode (EPI_*), column-segmented rows and precision16."""
    import ctypes
    out = (ctypes.c_int * len(X3_ROUTE_FIELDS))()
    check(lib().fdet_conv3x3_x3_last_route(out, len(out)), "fdet_conv3x3_x3_last_route")
    r = dict(zip(X3_ROUTE_FIELDS, list(out)))
    r["family"] = X3_FAMILIES.get(r["family"])
    return r


WGRAD_PLAN_FIELDS = ("ok", "pipe", "lpr32", "pk4", "pack", "vw", "mtc", "nseg")


def conv3x3_wgrad_x3_plan(Nn, cin, cout, H, W, L: int = 1) -> dict:
    """The bf16x3 / precision16 weight-gradient plan of L same-shape layers (fdet_conv3x3_wgrad_bf16x3_plan; launches
    nothing): ok, pipe, lpr32, pk4, pack (reserved, always 0), vw, mtc, nseg."""
    import ctypes
    out = (ctypes.c_int * len(WGRAD_PLAN_FIELDS))()
    check(lib().fdet_conv3x3_wgrad_bf16x3_plan(int(Nn), int(cin), int(cout), int(H), int(W), int(L), out, len(out)),
          "fdet_conv3x3_wgrad_bf16x3_plan")
    return dict(zip(WGRAD_PLAN_FIELDS, list(out)))


def pool_fusion_supported(cout: int, cin: int, H: int, W: int, N: int = 1) -> bool:
    """Pooled residual blocks whose tail runs inside the conv epilogues (fdet_conv3x3_fwd_pool_bf16x3): the library's own
    plan check (fdet_conv3x3_pool_fusion_ok), batch-size limits included when N is given."""
    return bool(lib().fdet_conv3x3_pool_fusion_ok(int(N), int(cin), int(cout), int(H), int(W)))


def conv3x3_fwd_pool(x, wpk, bias, skip, drop_scale, out_pooled, route, slope: float = 0.2, p16: bool = False):
    """out_pooled = maxpool2x2(lrelu(conv(x)+bias)*drop_scale + skip); route: uint8 routing bytes or None (eval).
    p16: precision16 (fdet_conv3x3_fwd_pool_bf16)."""
    Nn, cin, H, W = x.shape
    cout = bias.shape[0]
    if wpk.numel() != packed_sizes(cout, cin)[0]:
        raise ValueError("conv3x3_fwd_pool: packed weight size does not match (Cout,Cin)")
    _chk4(skip, (Nn, cout, H, W), "skip")
    _chk4(out_pooled, (Nn, cout, H // 2, W // 2), "out_pooled")
    if route is not None:
        _chk4(route, (Nn, cout, H // 2, W // 2), "route")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, cout), "drop_scale")
    fn = _p16_fn("fdet_conv3x3_fwd_pool", True, p16)
    check(fn(ptr(x), ptr(wpk), ptr(bias), ptr(skip), ptr(drop_scale), ptr(out_pooled), ptr(route, torch.uint8), Nn, cin, cout,
             H, W, float(slope), stream()), fn.__name__)


def conv3x3_dgrad_unpool(dz, wpk_bwd, cin: int, dout_pooled, route, dx, slope: float = 0.2, p16: bool = False):
    """dx = conv^T(dz) + unpool(dout_pooled) through the routing bytes of the forward pass.
    p16: precision16 (fdet_conv3x3_dgrad_unpool_bf16)."""
    Nn, cout, H, W = dz.shape
    if wpk_bwd.numel() != packed_sizes(cout, cin)[1]:
        raise ValueError("conv3x3_dgrad_unpool: packed weight size does not match (Cout,Cin)")
    _chk4(dx, (Nn, cin, H, W), "dx")
    _chk4(dout_pooled, (Nn, cin, H // 2, W // 2), "dout_pooled")
    _chk4(route, (Nn, cin, H // 2, W // 2), "route")
    fn = _p16_fn("fdet_conv3x3_dgrad_unpool", True, p16)
    check(fn(ptr(dz), ptr(wpk_bwd), ptr(dout_pooled), ptr(route, torch.uint8), ptr(dx), Nn, cin, cout, H, W, float(slope),
             stream()), fn.__name__)


def pool_route_bwd(dout_pooled, route, drop_scale, dz2, slope: float = 0.2):
    """dz2 = unpool(dout_pooled) * drop_scale * lrelu'(c), from the routing bytes alone."""
    Nn, F_, H, W = dz2.shape
    _chk4(dout_pooled, (Nn, F_, H // 2, W // 2), "dout_pooled")
    _chk4(route, (Nn, F_, H // 2, W // 2), "route")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, F_), "drop_scale")
    check(lib().fdet_pool_route_bwd(ptr(dout_pooled), ptr(route, torch.uint8), ptr(drop_scale), ptr(dz2), Nn, F_, H, W,
                                    float(slope), stream()), "fdet_pool_route_bwd")


# ---- pointwise (1x1 conv / per-position Linear) GEMMs, bf16x3 ------------------------------------------------------
def pointwise_pack(w: torch.Tensor):
    """w (Cout,Cin[,1,1]) -> (forward panel, backward panel) for pointwise_fwd / pointwise_dgrad."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    w2 = _f32(w.reshape(cout, cin))
    n = int(lib().fdet_pointwise_packed_bytes(cout, cin)) // 4
    f_ = torch.empty(n, dtype=F32, device=w.device)
    b_ = torch.empty(n, dtype=F32, device=w.device)
    check(lib().fdet_pack_pointwise_weights_bf16x3(ptr(w2), cout, cin, ptr(f_), ptr(b_), stream()), "fdet_pack_pointwise_weights_bf16x3")
    return f_, b_


def pointwise_fwd(x, wpk_fwd, bias, y, slope: float = 1.0, p16: bool = False):
    """y (N,Cout,H,W) = lrelu_slope(W x + bias) for x (N,Cin,H,W).  p16: precision16 (fdet_pointwise_fwd_bf16)."""
    Nn, cin = x.shape[0], x.shape[1]
    cout = y.shape[1]
    P = x.numel() // (Nn * cin)
    if y.shape[0] != Nn or y.numel() != Nn * cout * P:
        raise ValueError("pointwise_fwd: x / y shapes disagree")
    if bias is not None:
        _chk4(bias, (cout,), "bias")
    if wpk_fwd.numel() * 4 < int(lib().fdet_pointwise_packed_bytes(cout, cin)):
        raise ValueError("pointwise_fwd: packed weight buffer too small for (Cout,Cin)")
    fn = lib().fdet_pointwise_fwd_bf16 if p16 else lib().fdet_pointwise_fwd_bf16x3
    check(fn(ptr(x), ptr(wpk_fwd), ptr(bias), ptr(y), Nn, cin, cout, P, float(slope), stream()), fn.__name__)


def pointwise_dgrad(dz, wpk_bwd, dx, add=None, p16: bool = False):
    """dx (N,Cin,H,W) = W^T dz (+ add).  p16: precision16 (fdet_pointwise_dgrad_bf16)."""
    Nn, cout = dz.shape[0], dz.shape[1]
    cin = dx.shape[1]
    P = dz.numel() // (Nn * cout)
    if dx.shape[0] != Nn or dx.numel() != Nn * cin * P or (add is not None and tuple(add.shape) != tuple(dx.shape)):
        raise ValueError("pointwise_dgrad: shapes disagree")
    if wpk_bwd.numel() * 4 < int(lib().fdet_pointwise_packed_bytes(cout, cin)):
        raise ValueError("pointwise_dgrad: packed weight buffer too small for (Cout,Cin)")
    fn = lib().fdet_pointwise_dgrad_bf16 if p16 else lib().fdet_pointwise_dgrad_bf16x3
    check(fn(ptr(dz), ptr(wpk_bwd), ptr(add), ptr(dx), Nn, cin, cout, P, stream()), fn.__name__)


def pointwise_wgrad(x, dz, dW, db=None, p16: bool = False):
    """dW (Cout,Cin[,1,1]) = sum dz x^T, db (Cout,) = sum dz.  p16: precision16 (fdet_pointwise_wgrad_bf16: bf16-rounded
    operands, fp32 sums; the same workspace)."""
    Nn, cin = x.shape[0], x.shape[1]
    cout = dz.shape[1]
    P = x.numel() // (Nn * cin)
    if dz.shape[0] != Nn or dz.numel() != Nn * cout * P or dW.numel() != cout * cin or (db is not None and db.numel() != cout):
        raise ValueError("pointwise_wgrad: shapes disagree")
    nb = int(lib().fdet_pointwise_wgrad_ws_bytes(Nn, cin, cout, P))
    ws = torch.empty(nb // 4 + 4, dtype=F32, device=x.device)
    fn = lib().fdet_pointwise_wgrad_bf16 if p16 else lib().fdet_pointwise_wgrad_bf16x3
    check(fn(ptr(x), ptr(dz), ptr(dW), ptr(db), ptr(ws), ws.numel() * 4, Nn, cin, cout, P, stream()), fn.__name__)


def conv3x3_wgrad_ws_bytes(Nn, cin, cout, H, W) -> int:
    """Workspace that serves BOTH precisions of conv3x3_wgrad."""
    return max(int(lib().fdet_conv3x3_wgrad_ws_bytes(Nn, cin, cout, H, W)),
               int(lib().fdet_conv3x3_wgrad_bf16x3_ws_bytes(Nn, cin, cout, H, W)))


def wgrad_x3_supported(Nn, cin, cout, H, W) -> bool:
    return int(lib().fdet_conv3x3_wgrad_bf16x3_ws_bytes(Nn, cin, cout, H, W)) > 0


def conv3x3_wgrad(x, dz, dW, db, ws, x3: bool = False, p16: bool = False):
    """p16: precision16 (fdet_conv3x3_wgrad_bf16: bf16-rounded operands, fp32 sums; the bf16x3 workspace size)."""
    Nn, cin, H, W = x.shape
    cout = dz.shape[1]
    _chk4(dz, (Nn, cout, H, W), "dz")
    _chk4(dW, (cout, cin, 3, 3), "dW")
    _chk4(db, (cout,), "db")
    fn = _p16_fn("fdet_conv3x3_wgrad", x3, p16)
    check(fn(ptr(x), ptr(dz), ptr(dW), ptr(db), ptr(ws, ws.dtype), ws.numel() * ws.element_size(),
             Nn, cin, cout, H, W, stream()), "fdet_conv3x3_wgrad")


def conv3x3_wgrad_batched_ws_bytes(L, Nn, cin, cout, H, W) -> int:
    return int(lib().fdet_conv3x3_wgrad_bf16x3_batched_ws_bytes(L, Nn, cin, cout, H, W))


def conv3x3_wgrad_batched(xs, dzs, dWs, dbs, ws, p16: bool = False):
    """bf16x3 weight gradients of L <= 16 same-shape layers in one launch (+ one reduce); p16: precision16
    (fdet_conv3x3_wgrad_bf16_batched, same workspace)."""
    L = len(xs)
    if not (1 <= L <= 16 and len(dzs) == len(dWs) == len(dbs) == L):
        raise ValueError("conv3x3_wgrad_batched: 1..16 layers, equal list lengths")
    Nn, cin, H, W = xs[0].shape
    cout = dzs[0].shape[1]
    for x, dz, dW, db in zip(xs, dzs, dWs, dbs):
        _chk4(x, (Nn, cin, H, W), "x")
        _chk4(dz, (Nn, cout, H, W), "dz")
        _chk4(dW, (cout, cin, 3, 3), "dW")
        _chk4(db, (cout,), "db")
    import ctypes
    arr = ctypes.c_void_p * L
    hx, hdz = arr(*[ptr(t) for t in xs]), arr(*[ptr(t) for t in dzs])
    hdW, hdb = arr(*[ptr(t) for t in dWs]), arr(*[ptr(t) for t in dbs])
    fn = lib().fdet_conv3x3_wgrad_bf16_batched if p16 else lib().fdet_conv3x3_wgrad_bf16x3_batched
    check(fn(hx, hdz, hdW, hdb, L, ptr(ws, ws.dtype), ws.numel() * ws.element_size(), Nn, cin, cout, H, W, stream()),
          fn.__name__)


def _ptr_array(ts, dtype=F32):
    """HOST array of device pointers (None entries -> NULL); None -> NULL array."""
    import ctypes
    if ts is None:
        return None
    return (ctypes.c_void_p * len(ts))(*[ptr(t, dtype) for t in ts])


def block_chain_supported(F_: int, H: int, W: int) -> bool:
    return bool(lib().fdet_block_chain_supported(int(F_), int(H), int(W)))


def block_chain_ok(N: int, F_: int, H: int, W: int, ps: bool = False) -> bool:
    """The chain kernels run N images of this map (fdet_block_chain_ok: the entry points' own check, batch size included);
    ps: the PS flavour."""
    return bool(lib().fdet_block_chain_ok(int(N), int(F_), int(H), int(W), int(ps)))


def block_chain_fwd(x, wpk1, b1, wpk2, b2, scales, a_out, c_out, outs, slope: float = 0.2):
    """Run len(wpk1) un-pooled residual blocks in one launch (fdet_block_chain_fwd_bf16x3).
    Lists of per-block tensors; `scales`, `a_out`, `c_out` may be None; `outs` entries may be None
    except the last."""
    nb = len(wpk1)
    Nn, F_, H, W = x.shape
    if not (len(b1) == len(wpk2) == len(b2) == len(outs) == nb) or outs[-1] is None:
        raise ValueError("block_chain_fwd: inconsistent per-block lists")
    for lst, nm in ((a_out, "a_out"), (c_out, "c_out"), (outs, "outs")):
        for t in (lst or []):
            if t is not None:
                _chk4(t, (Nn, F_, H, W), nm)
    for t in (scales or []):
        if t is not None:
            _chk4(t, (Nn, F_), "scale")
    nf = packed_sizes(F_, F_)[0]
    for t in list(wpk1) + list(wpk2):
        if t.numel() != nf:
            raise ValueError("block_chain_fwd: packed weight size does not match the channel count")
    for t in list(b1) + list(b2):
        _chk4(t, (F_,), "bias")
    check(lib().fdet_block_chain_fwd_bf16x3(ptr(x), _ptr_array(wpk1), _ptr_array(b1), _ptr_array(wpk2), _ptr_array(b2),
                                            _ptr_array(scales), _ptr_array(a_out), _ptr_array(c_out), _ptr_array(outs),
                                            nb, Nn, F_, H, W, float(slope), stream()), "fdet_block_chain_fwd_bf16x3")


def block_chain_bwd(dout, wpk1b, wpk2b, scales, a_saved, c_saved, dz1, dz2, dx, slope: float = 0.2):
    """Data-gradient chain of the same blocks (fdet_block_chain_bwd_bf16x3): fills dz1[k], dz2[k], dx."""
    nb = len(wpk1b)
    Nn, F_, H, W = dout.shape
    if not (len(wpk2b) == len(a_saved) == len(c_saved) == len(dz1) == len(dz2) == nb):
        raise ValueError("block_chain_bwd: inconsistent per-block lists")
    for lst, nm in ((a_saved, "a"), (c_saved, "c"), (dz1, "dz1"), (dz2, "dz2"), ([dx], "dx")):
        for t in lst:
            _chk4(t, (Nn, F_, H, W), nm)
    for t in (scales or []):
        if t is not None:
            _chk4(t, (Nn, F_), "scale")
    nbk = packed_sizes(F_, F_)[1]
    for t in list(wpk1b) + list(wpk2b):
        if t.numel() != nbk:
            raise ValueError("block_chain_bwd: packed weight size does not match the channel count")
    check(lib().fdet_block_chain_bwd_bf16x3(ptr(dout), _ptr_array(wpk1b), _ptr_array(wpk2b), _ptr_array(scales),
                                            _ptr_array(a_saved), _ptr_array(c_saved), _ptr_array(dz1), _ptr_array(dz2),
                                            ptr(dx), nb, Nn, F_, H, W, float(slope), stream()), "fdet_block_chain_bwd_bf16x3")


def block_tail_fwd(c, x, drop_scale, out, pool: int):
    Nn, F_, H, W = c.shape
    _chk4(x, c.shape, "x")
    _chk4(out, (Nn, F_, H // pool, W // pool), "out")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, F_), "drop_scale")
    check(lib().fdet_block_tail_fwd(ptr(c), ptr(x), ptr(drop_scale), ptr(out), Nn, F_, H, W, pool, stream()),
          "fdet_block_tail_fwd")


def block_tail_bwd(dout, c, x, drop_scale, dz2, de, pool: int, slope: float = 0.2):
    Nn, F_, H, W = c.shape
    _chk4(dout, (Nn, F_, H // pool, W // pool), "dout")
    _chk4(dz2, c.shape, "dz2")
    if pool == 2:
        _chk4(x, c.shape, "x")
        _chk4(de, c.shape, "de")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, F_), "drop_scale")
    check(lib().fdet_block_tail_bwd(ptr(dout), ptr(c), ptr(x), ptr(drop_scale), ptr(dz2), ptr(de), Nn, F_, H, W, pool,
                                    float(slope), stream()), "fdet_block_tail_bwd")


def stem_ws_bytes(Nn, cin, F_, H, W, k, stride, pad) -> int:
    return int(lib().fdet_stem_ws_bytes(Nn, cin, F_, H, W, k, stride, pad))


def stem_x3_supported(cin, W, k, stride, pad) -> bool:
    return cin == 3 and (k, stride, pad) == (10, 8, 2) and W % 4 == 0 and W <= 512 and ((W + 2 * pad - k) // stride + 1) % 4 == 0


def stem_fwd(x, w, bias, y, ws, k, stride, pad, x3: bool = False):
    Nn, cin, H, W = x.shape
    F_ = w.shape[0]
    _chk4(w, (F_, cin, k, k), "w")
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    _chk4(y, (Nn, F_, Ho, Wo), "y")
    fn = lib().fdet_stem_fwd_bf16x3 if x3 else lib().fdet_stem_fwd
    check(fn(ptr(x), ptr(w), ptr(bias), ptr(y), ptr(ws, ws.dtype), ws.numel() * ws.element_size(),
             Nn, cin, F_, H, W, k, stride, pad, stream()), "fdet_stem_fwd")


def stem_k3_wgrad_x3_supported(cin, F_, H, W, k, stride, pad) -> bool:
    """The Resnet stem (3 channels, k3 s2 p1) has a matrix-core (bf16x3) weight gradient for this shape (fdet_stem_k3.hip)."""
    Wo = (W + 2 * pad - k) // stride + 1
    return cin == 3 and (k, stride, pad) == (3, 2, 1) and F_ % 8 == 0 and H % 2 == 0 and W % 4 == 0 and Wo % 16 == 0 and Wo <= 320


def stem_k3_fwd_ps_supported(cin, F_, H, W, k, stride, pad) -> bool:
    return cin == 3 and (k, stride, pad) == (3, 2, 1) and F_ % 8 == 0 and H % 2 == 0 and W % 2 == 0


def stem_fwd_ps_ok(N, cin, F_, H, W, k, stride, pad, p16: bool = False, u8: bool = False) -> bool:
    """fdet_stem_fwd_ps (p16: _p16; u8: the uint8-frame form) accepts N images of this shape (fdet_stem_fwd_ps_ok)."""
    return bool(lib().fdet_stem_fwd_ps_ok(int(N), int(cin), int(F_), int(H), int(W), int(k), int(stride), int(pad), int(p16), int(u8)))


def stem_wgrad_x3_ok(N, cin, F_, H, W, k, stride, pad, p16: bool = False) -> bool:
    """The matrix-core stem weight gradient (bf16x3, or precision16 with p16) accepts N images of this shape
    (fdet_stem_wgrad_x3_ok)."""
    return bool(lib().fdet_stem_wgrad_x3_ok(int(N), int(cin), int(F_), int(H), int(W), int(k), int(stride), int(pad), int(p16)))


STEM_ROUTE_FIELDS = ("family", "pass", "p16", "u8", "ps", "launches", "grid", "items")
STEM_FAMILIES = {1: "valu_k10", 2: "valu_k3_generic", 3: "valu_k3_scalar", 4: "mfma", 5: "x3_single", 6: "x3_pipe", 7: "k3_matrix",
                 8: "k3_ps_fwd"}
STEM_PASSES = {1: "fwd", 2: "wgrad"}


def stem_last_route() -> dict:
    """What the last stem forward / weight-gradient call on this thread launched (fdet_stem_last_route): kernel family
    (None after a refused call), pass ("fwd" / "wgrad"), precision16, uint8 input, PS output, launches of the main kernel
    (image chunks), and gridDim.x and work items of the first launch."""
    import ctypes
    out = (ctypes.c_int * len(STEM_ROUTE_FIELDS))()
    check(lib().fdet_stem_last_route(out, len(out)), "fdet_stem_last_route")
    r = dict(zip(STEM_ROUTE_FIELDS, list(out)))
    r["family"] = STEM_FAMILIES.get(r["family"])
    r["pass"] = STEM_PASSES.get(r["pass"])
    return r


def stem_wgrad(x, dy, dW, db, ws, k, stride, pad, x3: bool = False, p16: bool = False):
    Nn, cin, H, W = x.shape
    F_ = dW.shape[0]
    _chk4(dW, (F_, cin, k, k), "dW")
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    _chk4(dy, (Nn, F_, Ho, Wo), "dy")
    fn = lib().fdet_stem_wgrad_bf16 if (x3 and p16) else (lib().fdet_stem_wgrad_bf16x3 if x3 else lib().fdet_stem_wgrad)
    check(fn(ptr(x), ptr(dy), ptr(dW), ptr(db), ptr(ws, ws.dtype), ws.numel() * ws.element_size(),
             Nn, cin, F_, H, W, k, stride, pad, stream()), "fdet_stem_wgrad")


def head_fwd(x, drop_scale, w, bias, y, k, pad):
    Nn, F_, H, W = x.shape
    _chk4(w, (5, F_, k, k), "w")
    So, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    _chk4(y, (Nn, 5, So, Wo), "y")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, F_), "drop_scale")
    check(lib().fdet_head_fwd(ptr(x), ptr(drop_scale), ptr(w), ptr(bias), ptr(y), Nn, F_, H, W, k, pad, stream()),
          "fdet_head_fwd")


def head_bwd_ws_bytes(Nn, F_, H, W, k, pad) -> int:
    return int(lib().fdet_head_bwd_ws_bytes(Nn, F_, H, W, k, pad))


def head_bwd(x, drop_scale, w, y, dy, dx, dW, db, ws, k, pad):
    Nn, F_, H, W = x.shape
    _chk4(w, (5, F_, k, k), "w")
    _chk4(dW, (5, F_, k, k), "dW")
    _chk4(dx, x.shape, "dx")
    _chk4(dy, y.shape, "dy")
    check(lib().fdet_head_bwd(ptr(x), ptr(drop_scale), ptr(w), ptr(y), ptr(dy), ptr(dx), ptr(dW), ptr(db),
                              ptr(ws, ws.dtype), ws.numel() * ws.element_size(), Nn, F_, H, W, k, pad, stream()),
          "fdet_head_bwd")


def head_loss_fused_supported(F_, H, W, k, pad) -> bool:
    return bool(lib().fdet_head_loss_fused_supported(int(F_), int(H), int(W), int(k), int(pad)))


def head_loss_fused_ws_bytes(Nn, F_, H, W, k, pad) -> int:
    return int(lib().fdet_head_loss_fused_ws_bytes(Nn, F_, H, W, k, pad))


def head_loss_fused(x, drop_scale, w, bias, gt, y, lpi, lsum, dx, dW, db, ws, k, pad):
    """Training head + yolo_loss + their gradients in one launch sequence (fdet_head_loss_fused): fills y (N,5,S,S),
    lpi (N,), lsum (1,), dx like x, dW (5,F,k,k), db (5,).  ws: zero-initialised workspace of head_loss_fused_ws_bytes()."""
    Nn, F_, H, W = x.shape
    _chk4(w, (5, F_, k, k), "w")
    _chk4(dW, (5, F_, k, k), "dW")
    _chk4(dx, x.shape, "dx")
    _chk4(gt, y.shape, "gt")
    if drop_scale is not None:
        _chk4(drop_scale, (Nn, F_), "drop_scale")
    check(lib().fdet_head_loss_fused(ptr(x), ptr(drop_scale), ptr(w), ptr(bias), ptr(gt), ptr(y), ptr(lpi), ptr(lsum), ptr(dx),
                                     ptr(dW), ptr(db), ptr(ws, ws.dtype), ws.numel() * ws.element_size(), Nn, F_, H, W, k, pad,
                                     stream()), "fdet_head_loss_fused")


# ---- MobileNetV3 backbone (inference, bf16, NHWC activations) -------------------------------------------------------
BF16 = torch.bfloat16
MB_ACT = {"none": 0, "relu": 1, "hswish": 2}


def mb_stem(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """x (N,3,H,W) f32 in [0,1] or uint8 (the /255 fused) -> (N,H/2,W/2,16) bf16; w (16,27) f32 BN-folded."""
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 2 or x.shape[3] % 2 or x.dtype not in (F32, torch.uint8):
        raise ValueError(f"mb_stem: expected (N,3,H,W) f32/uint8 with even H, W; got {tuple(x.shape)} {x.dtype}")
    _chk4(w, (16, 27), "stem weight"); _chk4(bias, (16,), "stem bias")
    Nn, _, H, W = x.shape
    y = torch.empty(Nn, H // 2, W // 2, 16, dtype=BF16, device=x.device)
    check(lib().fdet_mb_stem(ptr(x, x.dtype), int(x.dtype == torch.uint8), ptr(w), ptr(bias), ptr(y, BF16), Nn, H, W, stream()),
          "fdet_mb_stem")
    return y


def mb_depthwise(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, K: int, stride: int, act: int, want_pool: bool):
    """x (N,H,W,C) bf16 -> (y (N,Ho,Wo,C) bf16, per-image partial channel sums (N,slots,C) f32 or None); w (K*K,C) f32."""
    if x.dim() != 4 or x.dtype != BF16:
        raise ValueError("mb_depthwise: expected (N,H,W,C) bf16")
    Nn, H, W, C = x.shape
    _chk4(w, (K * K, C), "depthwise weight"); _chk4(bias, (C,), "depthwise bias")
    Ho, Wo = -(-H // stride), -(-W // stride)
    y = torch.empty(Nn, Ho, Wo, C, dtype=BF16, device=x.device)
    pool = None
    if want_pool:
        slots = int(lib().fdet_mb_depthwise_pool_slots(Nn, H, W, C, K, stride))
        if slots <= 0:
            raise ValueError("mb_depthwise: unsupported shape")
        pool = torch.empty(Nn, slots, C, dtype=F32, device=x.device)
    check(lib().fdet_mb_depthwise(ptr(x, BF16), ptr(w), ptr(bias), ptr(y, BF16), ptr(pool), Nn, H, W, C, K, stride, act, stream()),
          "fdet_mb_depthwise")
    return y, pool


def mb_se_gate(pool: torch.Tensor, HW: int, w1, b1, w2, b2) -> torch.Tensor:
    """gate (N,C) = hardsigmoid(W2 relu(W1 mean + b1) + b2), mean = sum of the pool rows / HW; pool (N,slots,C) as
    mb_depthwise returns it (or (N,C)); w1 (R,C), w2 (C,R)."""
    if pool.dim() == 2:
        pool = pool.unsqueeze(1)
    Nn, slots, C = pool.shape
    R = w1.shape[0]
    _chk4(w1, (R, C), "se reduce weight"); _chk4(b1, (R,), "se reduce bias")
    _chk4(w2, (C, R), "se expand weight"); _chk4(b2, (C,), "se expand bias")
    gate = torch.empty(Nn, C, dtype=F32, device=pool.device)
    check(lib().fdet_mb_se_gate(ptr(pool), slots, HW, ptr(w1), ptr(b1), ptr(w2), ptr(b2), Nn, C, R, ptr(gate), stream()), "fdet_mb_se_gate")
    return gate


def mb_pointwise_pack(w: torch.Tensor, bias: torch.Tensor):
    """BN-folded (Cout,Cin) f32 weight + (Cout,) bias -> (bf16 panel [ceil32(Cout)][ceil16(Cin)], f32 bias [ceil32(Cout)])."""
    cout, cin = w.shape
    cop, cip = -(-cout // 32) * 32, -(-cin // 16) * 16
    wp = torch.zeros(cop, cip, dtype=BF16, device=w.device)
    wp[:cout, :cin] = w.to(BF16)
    bp = torch.zeros(cop, dtype=F32, device=w.device)
    bp[:cout] = bias
    return wp, bp


def mb_pointwise(x: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor, cout: int, act: int, gate=None, res=None) -> torch.Tensor:
    """y (N,H,W,Cout) bf16 = act(W (x * gate) + bias) (+ res) for x (N,H,W,Cin) bf16."""
    if x.dim() != 4 or x.dtype != BF16:
        raise ValueError("mb_pointwise: expected (N,H,W,C) bf16")
    Nn, H, W, cin = x.shape
    if tuple(wp.shape) != (-(-cout // 32) * 32, -(-cin // 16) * 16) or wp.dtype != BF16 or bp.numel() != wp.shape[0]:
        raise ValueError(f"mb_pointwise: weight panel {tuple(wp.shape)} does not fit Cout={cout}, Cin={cin}")
    if gate is not None:
        _chk4(gate, (Nn, cin), "gate")
    y = torch.empty(Nn, H, W, cout, dtype=BF16, device=x.device)
    if res is not None and (tuple(res.shape) != tuple(y.shape) or res.dtype != BF16):
        raise ValueError("mb_pointwise: residual must match the output")
    check(lib().fdet_mb_pointwise(ptr(x, BF16), ptr(wp, BF16), ptr(bp), ptr(gate), ptr(res, BF16), ptr(y, BF16), Nn, H * W, cin,
                                  cout, act, stream()), "fdet_mb_pointwise")
    return y


def mb_head_pack(w: torch.Tensor) -> torch.Tensor:
    """Conv2d(C,5,3,p1) weight (5,C,3,3) f32 -> bf16 (2,64,C): row tap*5 + ch (rows 45..63 zero), split into
    hi = bf16(w), lo = bf16(w - hi)."""
    C = w.shape[1]
    wt = torch.zeros(64, C, dtype=F32, device=w.device)
    wt[:45] = w.float().permute(2, 3, 0, 1).reshape(45, C)       # (ky, kx, ch) -> tap*5 + ch
    hi = wt.to(BF16)
    lo = (wt - hi.float()).to(BF16)
    return torch.stack([hi, lo]).contiguous()


def mb_head(f: torch.Tensor, w2: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """f (N,S,S,C) bf16 -> sigmoid(Conv2d(C,5,3,p1)) as (N,5,S,S) f32; w2 = mb_head_pack(weight)."""
    if f.dim() != 4 or f.dtype != BF16 or f.shape[1] != f.shape[2] or f.shape[3] % 16:
        raise ValueError("mb_head: expected (N,S,S,C) bf16 with C % 16 == 0")
    Nn, S, _, C = f.shape
    if tuple(w2.shape) != (2, 64, C) or w2.dtype != BF16:
        raise ValueError(f"mb_head: expected the packed weight (2,64,{C}) bf16, got {tuple(w2.shape)} {w2.dtype}")
    _chk4(bias, (5,), "head bias")
    y = torch.empty(Nn, 5, S, S, dtype=F32, device=f.device)
    nb = int(lib().fdet_mb_head_ws_bytes(Nn, S))
    ws = torch.empty(nb // 4, dtype=F32, device=f.device)
    check(lib().fdet_mb_head(ptr(f, BF16), ptr(w2, BF16), ptr(bias), ptr(y), ptr(ws), nb, Nn, S, C, stream()), "fdet_mb_head")
    return y


# ------------------------------------------------------------------------------------------
# int8 inference (csrc/fdet_q8.hip; include/fdet.h "Int8 inference")
# ------------------------------------------------------------------------------------------
I8 = torch.int8


def q8_supported(C: int, H: int, W: int) -> bool:
    return bool(lib().fdet_q8_supported(int(C), int(H), int(W)))


def q8_act_bytes(Nn: int, C: int, H: int, W: int) -> int:
    return int(lib().fdet_q8_act_bytes(int(Nn), int(C), int(H), int(W)))


class Q8Tensor:
    """An int8 feature map in the kernels' layout [N][H+2][W+2][C] with its halo of zeros.  The storage is zero-filled when
    the tensor is made and whenever `reshape_` gives it another shape; producers write real pixels only, so reuse at the
    same shape costs nothing."""

    def __init__(self, Nn: int, C: int, H: int, W: int, device, storage: Optional[torch.Tensor] = None):
        nbytes = q8_act_bytes(Nn, C, H, W)
        if nbytes == 0:
            raise N.FdetError(f"Q8Tensor: unsupported shape ({Nn},{C},{H},{W}) (C % 64 == 0, C <= 256, under 2 GiB)")
        if storage is None:
            storage = torch.zeros(nbytes, dtype=I8, device=device)
        elif storage.dtype != I8 or storage.dim() != 1 or not storage.is_cuda or storage.numel() < nbytes:
            raise ValueError("Q8Tensor: storage must be a flat int8 GPU tensor of at least fdet_q8_act_bytes bytes")
        else:
            storage.zero_()
        self.storage = storage
        self.shape = (int(Nn), int(C), int(H), int(W))

    def reshape_(self, Nn: int, C: int, H: int, W: int) -> "Q8Tensor":
        """The same allocation as a map of another shape (it must fit): the halo moves, so the storage is zero-filled."""
        if (Nn, C, H, W) != self.shape:
            nbytes = q8_act_bytes(Nn, C, H, W)
            if nbytes == 0 or nbytes > self.storage.numel():
                raise ValueError(f"Q8Tensor.reshape_: ({Nn},{C},{H},{W}) does not fit this allocation")
            self.storage.zero_()
            self.shape = (int(Nn), int(C), int(H), int(W))
        return self

    @property
    def data(self) -> int:
        return ptr(self.storage, I8)

    @property
    def device(self):
        return self.storage.device

    def nchw(self) -> torch.Tensor:
        """The real pixels as an (N,C,H,W) int8 tensor (a torch copy: tests and trace())."""
        Nn, C, H, W = self.shape
        v = self.storage[:Nn * (H + 2) * (W + 2) * C].view(Nn, H + 2, W + 2, C)
        return v[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).contiguous()


def _q8_same(t, shape, name):
    if not isinstance(t, Q8Tensor) or t.shape != tuple(shape):
        raise ValueError(f"{name}: expected a Q8Tensor of shape {tuple(shape)}, got {getattr(t, 'shape', type(t))}")


def q8_quantize(x: torch.Tensor, scale: float, out: Optional[Q8Tensor] = None) -> Q8Tensor:
    """fp32 (N,C,H,W) -> Q8Tensor: q = clamp(rintf(x * (1.0f / scale)), -127, 127), NaN -> 0."""
    if x.dim() != 4:
        raise ValueError("q8_quantize: expected an (N,C,H,W) tensor")
    Nn, C, H, W = x.shape
    q = out if out is not None else Q8Tensor(Nn, C, H, W, x.device)
    _q8_same(q, (Nn, C, H, W), "q8_quantize: out")
    check(lib().fdet_q8_quantize(ptr(x), float(scale), q.data, Nn, C, H, W, stream()), "fdet_q8_quantize")
    return q


def q8_dequantize(q: Q8Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Q8Tensor -> fp32 (N,C,H,W) = float(q) * scale."""
    Nn, C, H, W = q.shape
    x = out if out is not None else torch.empty(Nn, C, H, W, dtype=F32, device=q.device)
    _chk4(x, q.shape, "q8_dequantize: out")
    check(lib().fdet_q8_dequantize(q.data, float(scale), ptr(x), Nn, C, H, W, stream()), "fdet_q8_dequantize")
    return x


def q8_pack_weights(w_q: torch.Tensor) -> torch.Tensor:
    """int8 [Cout,Cin,3,3] -> the conv's [tap][Cin/64][Cout][64] order (one-time work, a torch permutation)."""
    if w_q.dtype != I8 or w_q.dim() != 4 or tuple(w_q.shape[2:]) != (3, 3) or w_q.shape[0] != w_q.shape[1] or w_q.shape[1] % 64:
        raise ValueError("q8_pack_weights: expected int8 weights [C,C,3,3] with C % 64 == 0")
    co, ci = w_q.shape[:2]
    return w_q.permute(2, 3, 1, 0).reshape(9, ci // 64, 64, co).permute(0, 1, 3, 2).contiguous().reshape(-1)


def q8_conv3x3(x: Q8Tensor, wpk: torch.Tensor, bias: torch.Tensor, mul: torch.Tensor, y: Q8Tensor, skip: Optional[Q8Tensor] = None,
               skip_mul: float = 0.0, pool: bool = False, slope: float = 0.2) -> Q8Tensor:
    """y = requantise(LeakyReLU((bias + conv3x3(x)) * mul) [+ skip * skip_mul]) [2x2 max-pooled] on the integer matrix cores."""
    if not isinstance(x, Q8Tensor):
        raise ValueError("q8_conv3x3: x must be a Q8Tensor")
    Nn, C, H, W = x.shape
    if pool and (H % 2 or W % 2):
        raise ValueError(f"q8_conv3x3: cannot 2x2-pool an odd {H}x{W} map")
    _q8_same(y, (Nn, C, H // 2, W // 2) if pool else (Nn, C, H, W), "q8_conv3x3: y")
    if skip is not None:
        _q8_same(skip, x.shape, "q8_conv3x3: skip")
    if wpk.numel() != 9 * C * C:
        raise ValueError("q8_conv3x3: packed weight size does not match the channel count")
    _chk4(bias, (C,), "bias")
    _chk4(mul, (C,), "mul")
    check(lib().fdet_q8_conv3x3(x.data, ptr(wpk, I8), ptr(bias, torch.int32), ptr(mul), skip.data if skip is not None else None,
                                float(skip_mul), y.data, Nn, C, H, W, int(bool(pool)), float(slope), stream()), "fdet_q8_conv3x3")
    return y


def q8_chain_supported(C: int, H: int, W: int) -> bool:
    """fdet_q8_chain runs maps of this shape: 64 channels, 1 <= H, W <= 16."""
    return bool(lib().fdet_q8_chain_supported(int(C), int(H), int(W)))


Q8_CHAIN_MAX_BLOCKS = 16


class Q8ChainWeights:
    """The host pointer arrays of fdet_q8_chain, built once: convs1 / convs2 = per block (wpk, bias, mul) of its first and
    second conv (device tensors, kept alive here), skip_muls = per block the skip multiplier."""

    def __init__(self, convs1: Sequence, convs2: Sequence, skip_muls: Sequence[float], C: int = 64):
        import ctypes
        nb = len(skip_muls)
        if not (1 <= nb <= Q8_CHAIN_MAX_BLOCKS) or len(convs1) != nb or len(convs2) != nb:
            raise ValueError(f"q8_chain: 1..{Q8_CHAIN_MAX_BLOCKS} blocks with two convs each, got {len(convs1)}, {len(convs2)}, {nb}")
        for wpk, bias, mul in list(convs1) + list(convs2):
            if wpk.numel() != 9 * C * C:
                raise ValueError("q8_chain: packed weight size does not match the channel count")
            _chk4(bias, (C,), "bias")
            _chk4(mul, (C,), "mul")
        self.C, self.nblocks = int(C), nb
        self.tensors = (list(convs1), list(convs2))
        self.arrays = tuple(_ptr_array([c[i] for c in cs], dt) for cs in (convs1, convs2)
                            for i, dt in ((0, I8), (1, torch.int32), (2, F32)))
        self.skip_mul = (ctypes.c_float * nb)(*[float(v) for v in skip_muls])


def q8_chain(x: Q8Tensor, weights: Q8ChainWeights, outs: Optional[Sequence[Optional[Q8Tensor]]] = None,
             out_f32: Optional[torch.Tensor] = None, out_scale: float = 1.0, slope: float = 0.2) -> None:
    """The blocks of `weights` on x in one launch (fdet_q8_chain).  outs: per block a Q8Tensor of x's shape or None;
    out_f32: fp32 (N,C,H,W) = float(last block) * out_scale.  One of outs[-1] and out_f32 is needed."""
    if not isinstance(x, Q8Tensor):
        raise ValueError("q8_chain: x must be a Q8Tensor")
    if not isinstance(weights, Q8ChainWeights):
        raise ValueError("q8_chain: weights must be a Q8ChainWeights")
    Nn, C, H, W = x.shape
    nb = weights.nblocks
    if C != weights.C:
        raise ValueError(f"q8_chain: the weights are for {weights.C} channels, x has {C}")
    h_out = None
    if outs is not None:
        if len(outs) != nb:
            raise ValueError(f"q8_chain: outs needs {nb} entries (None where a block's output is not wanted)")
        import ctypes
        for t in outs:
            if t is not None:
                _q8_same(t, x.shape, "q8_chain: out")
        h_out = (ctypes.c_void_p * nb)(*[None if t is None else t.data for t in outs])
    if out_f32 is not None:
        _chk4(out_f32, x.shape, "q8_chain: out_f32")
    if out_f32 is None and (outs is None or outs[-1] is None):
        raise ValueError("q8_chain: the last block needs an output (outs[-1] or out_f32)")
    w1, b1, m1, w2, b2, m2 = weights.arrays
    check(lib().fdet_q8_chain(x.data, w1, b1, m1, w2, b2, m2, weights.skip_mul, h_out, ptr(out_f32), float(out_scale), nb,
                              Nn, C, H, W, float(slope), stream()), "fdet_q8_chain")


def stem_fwd_q8_ok(N_, cin, F_, H, W, k, stride, pad) -> bool:
    """fdet_stem_fwd_q8_u8 accepts N images of this shape (fdet_stem_fwd_q8_ok)."""
    return bool(lib().fdet_stem_fwd_q8_ok(int(N_), int(cin), int(F_), int(H), int(W), int(k), int(stride), int(pad)))


def stem_fwd_q8_u8(frames: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, scale: float, out: Q8Tensor, k: int = 10,
                   stride: int = 8, pad: int = 2) -> Q8Tensor:
    """uint8 frames (N,3,H,W) -> the stem's output quantised with `scale`, in `out` (real pixels only): the bytes of
    u8_to_f32_norm -> stem_fwd(x3=True) -> q8_quantize."""
    if frames.dim() != 4 or frames.dtype != torch.uint8:
        raise ValueError("stem_fwd_q8_u8: expected uint8 frames (N,3,H,W)")
    Nn, cin, H, W = frames.shape
    F_ = w.shape[0]
    _chk4(w, (F_, cin, k, k), "w")
    _chk4(bias, (F_,), "bias")
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    _q8_same(out, (Nn, F_, Ho, Wo), "stem_fwd_q8_u8: out")
    check(lib().fdet_stem_fwd_q8_u8(ptr(frames, torch.uint8), ptr(w), ptr(bias), float(scale), out.data, Nn, cin, F_, H, W, k,
                                    stride, pad, stream()), "fdet_stem_fwd_q8_u8")
    return out


def stem3_fwd_q8_ok(N_, cin, F_, H, W) -> bool:
    """fdet_stem3_fwd_q8_u8 accepts N images of this shape (fdet_stem3_fwd_q8_ok): 3 channels, F a multiple of 64 up to 256,
    even H and W in 2..4096."""
    return bool(lib().fdet_stem3_fwd_q8_ok(int(N_), int(cin), int(F_), int(H), int(W)))


def q8_pack_stem_weights(w_q: torch.Tensor) -> torch.Tensor:
    """int8 [F,3,3,3] -> the integer stem's [F][32]: k = (ci*3+ky)*3+kx, bytes 27..31 zero (one-time work, a torch reshape)."""
    if w_q.dtype != I8 or w_q.dim() != 4 or tuple(w_q.shape[1:]) != (3, 3, 3) or w_q.shape[0] % 64:
        raise ValueError("q8_pack_stem_weights: expected int8 weights [F,3,3,3] with F % 64 == 0")
    out = torch.zeros(w_q.shape[0], 32, dtype=I8, device=w_q.device)
    out[:, :27] = w_q.reshape(w_q.shape[0], 27)
    return out.reshape(-1)


def stem3_fwd_q8_u8(frames: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, mul: torch.Tensor, out: Q8Tensor) -> Q8Tensor:
    """uint8 frames (N,3,H,W) -> the 3x3 / stride 2 / pad 1 stem in integer arithmetic, requantised into `out` (real pixels
    only): clamp(rintf(float(bias + sum x_u8 * w_q) * mul), -127, 127) on the integer matrix cores (fdet_stem3_fwd_q8_u8)."""
    if frames.dim() != 4 or frames.dtype != torch.uint8:
        raise ValueError("stem3_fwd_q8_u8: expected uint8 frames (N,3,H,W)")
    Nn, cin, H, W = frames.shape
    F_ = bias.shape[0]
    if wpk.numel() != 32 * F_:
        raise ValueError("stem3_fwd_q8_u8: packed weight size does not match the channel count (q8_pack_stem_weights)")
    _chk4(bias, (F_,), "bias")
    _chk4(mul, (F_,), "mul")
    if H % 2 or W % 2:
        raise ValueError(f"stem3_fwd_q8_u8: H and W must be even, got {H}x{W}")
    _q8_same(out, (Nn, F_, H // 2, W // 2), "stem3_fwd_q8_u8: out")
    check(lib().fdet_stem3_fwd_q8_u8(ptr(frames, torch.uint8), ptr(wpk, I8), ptr(bias, torch.int32), ptr(mul), out.data, Nn, cin,
                                     F_, H, W, stream()), "fdet_stem3_fwd_q8_u8")
    return out


def stem10_fwd_q8_ok(N_, cin, F_, H, W) -> bool:
    """fdet_stem10_fwd_q8_u8 accepts N images of this shape (fdet_stem10_fwd_q8_ok): 3 channels, F a multiple of 64 up to
    256, H and W in 6..4096, the output under 2 GiB."""
    return bool(lib().fdet_stem10_fwd_q8_ok(int(N_), int(cin), int(F_), int(H), int(W)))


def q8_pack_stem10_weights(w_q: torch.Tensor) -> torch.Tensor:
    """int8 [F,3,10,10] -> the integer stem's [F][32][16]: row ci*10+ky (rows 30, 31 zero), slot kx (slots 10..15 zero);
    one-time work, a torch reshape and pad."""
    if w_q.dtype != I8 or w_q.dim() != 4 or tuple(w_q.shape[1:]) != (3, 10, 10) or w_q.shape[0] % 64:
        raise ValueError("q8_pack_stem10_weights: expected int8 weights [F,3,10,10] with F % 64 == 0")
    out = torch.zeros(w_q.shape[0], 32, 16, dtype=I8, device=w_q.device)
    out[:, :30, :10] = w_q.reshape(w_q.shape[0], 30, 10)
    return out.reshape(-1)


def stem10_fwd_q8_u8(frames: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, mul: torch.Tensor, out: Q8Tensor) -> Q8Tensor:
    """uint8 frames (N,3,H,W) -> the 10x10 / stride 8 / pad 2 stem in integer arithmetic, requantised into `out` (real pixels
    only): clamp(rintf(float(bias + sum x_u8 * w_q) * mul), -127, 127) on the integer matrix cores (fdet_stem10_fwd_q8_u8)."""
    if frames.dim() != 4 or frames.dtype != torch.uint8:
        raise ValueError("stem10_fwd_q8_u8: expected uint8 frames (N,3,H,W)")
    Nn, cin, H, W = frames.shape
    F_ = bias.shape[0]
    if wpk.numel() != 512 * F_:
        raise ValueError("stem10_fwd_q8_u8: packed weight size does not match the channel count (q8_pack_stem10_weights)")
    _chk4(bias, (F_,), "bias")
    _chk4(mul, (F_,), "mul")
    if H < 6 or W < 6:
        raise ValueError(f"stem10_fwd_q8_u8: H and W must be at least 6, got {H}x{W}")
    _q8_same(out, (Nn, F_, (H - 6) // 8 + 1, (W - 6) // 8 + 1), "stem10_fwd_q8_u8: out")
    check(lib().fdet_stem10_fwd_q8_u8(ptr(frames, torch.uint8), ptr(wpk, I8), ptr(bias, torch.int32), ptr(mul), out.data, Nn, cin,
                                      F_, H, W, stream()), "fdet_stem10_fwd_q8_u8")
    return out


# ------------------------------------------------------------------------------------------
# int8 inference of the separable block (csrc/fdet_q8_sep.hip; include/fdet.h "Int8 inference: the separable block")
# ------------------------------------------------------------------------------------------
def q8_sepblock_supported(C: int, H: int, W: int) -> bool:
    """fdet_q8_sepblock runs maps of this shape: 64 or 128 channels, 1 <= H, W <= 4096."""
    return bool(lib().fdet_q8_sepblock_supported(int(C), int(H), int(W)))


def q8_sepblock_plan(C: int, H: int, W: int, pool: bool = False):
    """(tile rows, tile columns, LDS bytes) the planner of fdet_q8_sepblock chooses, or None."""
    import ctypes
    r, c, l = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    ok = lib().fdet_q8_sepblock_plan(int(C), int(H), int(W), int(bool(pool)), ctypes.byref(r), ctypes.byref(c), ctypes.byref(l))
    return (r.value, c.value, l.value) if ok else None


def q8_pack_sep_pw(w_q: torch.Tensor) -> torch.Tensor:
    """int8 pointwise weights [Cout,Cin,1,1] (or [Cout,Cin]) -> the kernel's [Cout][Cin] rows."""
    if w_q.dtype != I8 or w_q.dim() not in (2, 4) or w_q.shape[0] != w_q.shape[1] or w_q.numel() != w_q.shape[0] ** 2:
        raise ValueError("q8_pack_sep_pw: expected int8 weights [C,C,1,1]")
    return w_q.reshape(w_q.shape[0], w_q.shape[0]).contiguous().reshape(-1)


def q8_pack_sep_dw(w_q: torch.Tensor) -> torch.Tensor:
    """int8 depthwise weights [C,1,3,3] -> the kernel's [9 taps ky*3+kx][C]."""
    if w_q.dtype != I8 or w_q.dim() != 4 or tuple(w_q.shape[1:]) != (1, 3, 3):
        raise ValueError("q8_pack_sep_dw: expected int8 weights [C,1,3,3]")
    return w_q.reshape(w_q.shape[0], 9).t().contiguous().reshape(-1)


def _q8_sep_check(C, w1, mul1, wd, mul2, w2, mul3, name):
    if w1.numel() != C * C or w2.numel() != C * C or wd.numel() != 9 * C:
        raise ValueError(f"{name}: packed weight sizes do not match the channel count (q8_pack_sep_pw / q8_pack_sep_dw)")
    for m in (mul1, mul2, mul3):
        _chk4(m, (C,), "mul")


def q8_sepblock(x: Q8Tensor, w1: torch.Tensor, mul1: torch.Tensor, wd: torch.Tensor, mul2: torch.Tensor, w2: torch.Tensor,
                mul3: torch.Tensor, skip_mul: float, y: Q8Tensor, pool: bool = False, tile=(0, 0), slope: float = 0.2) -> Q8Tensor:
    """One separable block in one launch (fdet_q8_sepblock): pw1 -> lrelu -> dw3x3 -> lrelu -> pw2 -> + x * skip_mul
    [-> 2x2 max], requantised after each stage.  tile=(rows, columns) forces a tiling; (0, 0) is the planner's."""
    if not isinstance(x, Q8Tensor):
        raise ValueError("q8_sepblock: x must be a Q8Tensor")
    Nn, C, H, W = x.shape
    if pool and (H % 2 or W % 2):
        raise ValueError(f"q8_sepblock: cannot 2x2-pool an odd {H}x{W} map")
    _q8_same(y, (Nn, C, H // 2, W // 2) if pool else (Nn, C, H, W), "q8_sepblock: y")
    _q8_sep_check(C, w1, mul1, wd, mul2, w2, mul3, "q8_sepblock")
    check(lib().fdet_q8_sepblock(x.data, ptr(w1, I8), ptr(mul1), ptr(wd, I8), ptr(mul2), ptr(w2, I8), ptr(mul3), float(skip_mul),
                                 y.data, Nn, C, H, W, int(bool(pool)), int(tile[0]), int(tile[1]), float(slope), stream()),
          "fdet_q8_sepblock")
    return y


def q8_sepchain_supported(C: int, H: int, W: int) -> bool:
    """fdet_q8_sepchain runs maps of this shape: 64 channels, 1 <= H, W <= 16."""
    return bool(lib().fdet_q8_sepchain_supported(int(C), int(H), int(W)))


class Q8SepChainWeights:
    """The host pointer arrays of fdet_q8_sepchain, built once: blocks = per block (w1, mul1, wd, mul2, w2, mul3) (device
    tensors, kept alive here), skip_muls = per block the skip multiplier."""

    def __init__(self, blocks: Sequence, skip_muls: Sequence[float], C: int = 64):
        import ctypes
        nb = len(skip_muls)
        if not (1 <= nb <= Q8_CHAIN_MAX_BLOCKS) or len(blocks) != nb:
            raise ValueError(f"q8_sepchain: 1..{Q8_CHAIN_MAX_BLOCKS} blocks, got {len(blocks)} with {nb} skip multipliers")
        for b in blocks:
            _q8_sep_check(C, *b, "q8_sepchain")
        self.C, self.nblocks = int(C), nb
        self.tensors = [tuple(b) for b in blocks]
        self.arrays = tuple(_ptr_array([b[i] for b in blocks], I8 if i in (0, 2, 4) else F32) for i in range(6))
        self.skip_mul = (ctypes.c_float * nb)(*[float(v) for v in skip_muls])


def q8_sepchain(x: Q8Tensor, weights: Q8SepChainWeights, outs: Optional[Sequence[Optional[Q8Tensor]]] = None,
                out_f32: Optional[torch.Tensor] = None, out_scale: float = 1.0, slope: float = 0.2) -> None:
    """The blocks of `weights` on x in one launch (fdet_q8_sepchain).  outs: per block a Q8Tensor of x's shape or None;
    out_f32: fp32 (N,C,H,W) = float(last block) * out_scale.  One of outs[-1] and out_f32 is needed."""
    if not isinstance(x, Q8Tensor):
        raise ValueError("q8_sepchain: x must be a Q8Tensor")
    if not isinstance(weights, Q8SepChainWeights):
        raise ValueError("q8_sepchain: weights must be a Q8SepChainWeights")
    Nn, C, H, W = x.shape
    nb = weights.nblocks
    if C != weights.C:
        raise ValueError(f"q8_sepchain: the weights are for {weights.C} channels, x has {C}")
    h_out = None
    if outs is not None:
        if len(outs) != nb:
            raise ValueError(f"q8_sepchain: outs needs {nb} entries (None where a block's output is not wanted)")
        import ctypes
        for t in outs:
            if t is not None:
                _q8_same(t, x.shape, "q8_sepchain: out")
        h_out = (ctypes.c_void_p * nb)(*[None if t is None else t.data for t in outs])
    if out_f32 is not None:
        _chk4(out_f32, x.shape, "q8_sepchain: out_f32")
    if out_f32 is None and (outs is None or outs[-1] is None):
        raise ValueError("q8_sepchain: the last block needs an output (outs[-1] or out_f32)")
    w1, m1, wd, m2, w2, m3 = weights.arrays
    check(lib().fdet_q8_sepchain(x.data, w1, m1, wd, m2, w2, m3, weights.skip_mul, h_out, ptr(out_f32), float(out_scale), nb,
                                 Nn, C, H, W, float(slope), stream()), "fdet_q8_sepchain")


# ------------------------------------------------------------------------------------------
# int8 inference, mixed widths: the SSD detector (csrc/fdet_q8.hip, csrc/fdet_stem_q8.hip; include/fdet.h "Int8 inference:
# mixed widths")
# ------------------------------------------------------------------------------------------
def q8x_supported(C: int, H: int, W: int) -> bool:
    """Q8 tensors of this shape exist for the q8x entries: C a multiple of 16 up to 256, 1 <= H, W <= 4096."""
    return bool(lib().fdet_q8x_supported(int(C), int(H), int(W)))


def q8x_act_bytes(Nn: int, C: int, H: int, W: int) -> int:
    return int(lib().fdet_q8x_act_bytes(int(Nn), int(C), int(H), int(W)))


class Q8XTensor(Q8Tensor):
    """A Q8Tensor whose channel count is any multiple of 16 up to 256 (fdet_q8x_act_bytes): the same layout, zero-filled
    when it is made."""

    def __init__(self, Nn: int, C: int, H: int, W: int, device):
        nbytes = q8x_act_bytes(Nn, C, H, W)
        if nbytes == 0:
            raise N.FdetError(f"Q8XTensor: unsupported shape ({Nn},{C},{H},{W}) (C % 16 == 0, C <= 256, under 2 GiB)")
        self.storage = torch.zeros(nbytes, dtype=I8, device=device)
        self.shape = (int(Nn), int(C), int(H), int(W))

    def reshape_(self, Nn: int, C: int, H: int, W: int):
        raise N.FdetError("Q8XTensor: make a new tensor for another shape")


def q8x_pack_weights(w_q: torch.Tensor) -> torch.Tensor:
    """int8 [Cout,Cin,kh,kw] (3x3 or 1x1) -> [K/64][Cout][64] with k = tap * Cin + ci, K zero-padded to a multiple of 64 (one-time
    work: a torch permutation and zero bytes)."""
    if w_q.dtype != I8 or w_q.dim() != 4 or tuple(w_q.shape[2:]) not in ((3, 3), (1, 1)) or w_q.shape[0] % 16 or w_q.shape[1] % 16:
        raise ValueError("q8x_pack_weights: expected int8 weights [Cout,Cin,3,3] or [Cout,Cin,1,1] with Cout and Cin multiples of 16")
    co, ci = w_q.shape[:2]
    K = ci * w_q.shape[2] * w_q.shape[3]
    KP = (K + 63) // 64 * 64
    flat = torch.zeros(co, KP, dtype=I8, device=w_q.device)
    flat[:, :K] = w_q.permute(0, 2, 3, 1).reshape(co, K)
    return flat.reshape(co, KP // 64, 64).permute(1, 0, 2).contiguous().reshape(-1)


def _q8x_weights_ok(wpk, bias, mul, cin, cout, taps, name):
    if wpk.numel() != (taps * cin + 63) // 64 * 64 * cout:
        raise ValueError(f"{name}: packed weight size does not match the channel counts (q8x_pack_weights)")
    _chk4(bias, (cout,), "bias")
    _chk4(mul, (cout,), "mul")


def q8x_conv3x3(x: Q8Tensor, wpk: torch.Tensor, bias: torch.Tensor, mul: torch.Tensor, y: Q8Tensor, skip: Optional[Q8Tensor] = None,
                skip_mul: float = 0.0, pool: bool = False, slope: float = 0.2) -> Q8Tensor:
    """y = requantise(LeakyReLU((bias + conv3x3(x)) * mul) [+ skip * skip_mul]) [2x2 floor-max-pooled], Cin -> Cout
    (fdet_q8x_conv3x3); Cout is y's channel count."""
    if not isinstance(x, Q8Tensor) or not isinstance(y, Q8Tensor):
        raise ValueError("q8x_conv3x3: x and y must be Q8 tensors")
    Nn, Cin, H, W = x.shape
    Cout = y.shape[1]
    _q8_same(y, (Nn, Cout, H // 2, W // 2) if pool else (Nn, Cout, H, W), "q8x_conv3x3: y")
    if skip is not None:
        _q8_same(skip, (Nn, Cout, H, W), "q8x_conv3x3: skip")
    _q8x_weights_ok(wpk, bias, mul, Cin, Cout, 9, "q8x_conv3x3")
    check(lib().fdet_q8x_conv3x3(x.data, ptr(wpk, I8), ptr(bias, torch.int32), ptr(mul), skip.data if skip is not None else None,
                                 float(skip_mul), y.data, Nn, Cin, Cout, H, W, int(bool(pool)), float(slope), stream()),
          "fdet_q8x_conv3x3")
    return y


def q8x_pointwise(x: Q8Tensor, wpk: torch.Tensor, bias: torch.Tensor, mul: torch.Tensor, y: Q8Tensor) -> Q8Tensor:
    """y = requantise((bias + conv1x1(x)) * mul), Cin -> Cout, identity activation (fdet_q8x_pointwise)."""
    if not isinstance(x, Q8Tensor) or not isinstance(y, Q8Tensor):
        raise ValueError("q8x_pointwise: x and y must be Q8 tensors")
    Nn, Cin, H, W = x.shape
    Cout = y.shape[1]
    _q8_same(y, (Nn, Cout, H, W), "q8x_pointwise: y")
    _q8x_weights_ok(wpk, bias, mul, Cin, Cout, 1, "q8x_pointwise")
    check(lib().fdet_q8x_pointwise(x.data, ptr(wpk, I8), ptr(bias, torch.int32), ptr(mul), y.data, Nn, Cin, Cout, H, W, stream()),
          "fdet_q8x_pointwise")
    return y


def q8x_head_f32(x: Q8Tensor, w_q: torch.Tensor, b_q: torch.Tensor, m: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """z (N,5,H,W) fp32 = float(b_q + sum_c x[c] * w_q[o][c]) * m[o] at every position (fdet_q8x_head_f32)."""
    if not isinstance(x, Q8Tensor):
        raise ValueError("q8x_head_f32: x must be a Q8 tensor")
    Nn, C, H, W = x.shape
    _chk4(w_q, (5, C), "w_q")
    _chk4(b_q, (5,), "b_q")
    _chk4(m, (5,), "m")
    _chk4(z, (Nn, 5, H, W), "z")
    check(lib().fdet_q8x_head_f32(x.data, ptr(w_q, I8), ptr(b_q, torch.int32), ptr(m), ptr(z), Nn, C, H, W, stream()),
          "fdet_q8x_head_f32")
    return z


def stem3_fwd_q8x_ok(N_, cin, F_, H, W) -> bool:
    """fdet_stem3_fwd_q8x_u8 accepts N images of this shape: 3 channels, F a multiple of 16 up to 256, even H and W up to 4096."""
    return bool(lib().fdet_stem3_fwd_q8x_ok(int(N_), int(cin), int(F_), int(H), int(W)))


def q8x_pack_stem_weights(w_q: torch.Tensor) -> torch.Tensor:
    """int8 [F,3,3,3] -> the integer stem's [F][32] (q8_pack_stem_weights for F a multiple of 16)."""
    if w_q.dtype != I8 or w_q.dim() != 4 or tuple(w_q.shape[1:]) != (3, 3, 3) or w_q.shape[0] % 16:
        raise ValueError("q8x_pack_stem_weights: expected int8 weights [F,3,3,3] with F % 16 == 0")
    out = torch.zeros(w_q.shape[0], 32, dtype=I8, device=w_q.device)
    out[:, :27] = w_q.reshape(w_q.shape[0], 27)
    return out.reshape(-1)


def stem3_fwd_q8x_u8(frames: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, mul: torch.Tensor, out: Q8Tensor) -> Q8Tensor:
    """stem3_fwd_q8_u8 for F a multiple of 16 (fdet_stem3_fwd_q8x_u8)."""
    if frames.dim() != 4 or frames.dtype != torch.uint8:
        raise ValueError("stem3_fwd_q8x_u8: expected uint8 frames (N,3,H,W)")
    Nn, cin, H, W = frames.shape
    F_ = bias.shape[0]
    if wpk.numel() != 32 * F_:
        raise ValueError("stem3_fwd_q8x_u8: packed weight size does not match the channel count (q8x_pack_stem_weights)")
    _chk4(bias, (F_,), "bias")
    _chk4(mul, (F_,), "mul")
    if H % 2 or W % 2:
        raise ValueError(f"stem3_fwd_q8x_u8: H and W must be even, got {H}x{W}")
    _q8_same(out, (Nn, F_, H // 2, W // 2), "stem3_fwd_q8x_u8: out")
    check(lib().fdet_stem3_fwd_q8x_u8(ptr(frames, torch.uint8), ptr(wpk, I8), ptr(bias, torch.int32), ptr(mul), out.data, Nn, cin,
                                      F_, H, W, stream()), "fdet_stem3_fwd_q8x_u8")
    return out
