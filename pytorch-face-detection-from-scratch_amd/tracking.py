"""Track faces across frame sequences on the device: identity from frame to frame, and bridging of the detector's gaps.

    tr = FaceTracker(max_misses=3, min_hits=1)
    rows, counts = model.reduce_bounding_boxes.forward_batch(model.forward_frames(frames))     # or TiledDetector.detect
    res = tr.update(rows, counts)                   # the frames of one call are consecutive; the state is carried on
    res.ids[t, :res.counts[t]]                      # the same face keeps its id from frame to frame

A per-frame anonymiser shows a face in every frame the detector misses it.  The tracker goes on emitting a missed track
for `emit_misses` frames at its last box, so rendering the tracker's rows instead of the detector's closes those gaps:

    anon = render_detections(bank, res.rows, res.counts, anonymize="pixelate", outline=False)

`fdet_track_update` (csrc/fdet_track.hip) does the association in one launch per call, one workgroup per sequence, with
exact integer arithmetic; include/fdet.h states the rule step by step, tests/track_cpu_ref.py restates it in numpy and
DESIGN.md 5h gives the limits and the measurements.  The reference project has no counterpart.

A missed track stays where it was, which bridges a gap only for a face that stands still.  `motion="constant_velocity"`
(`fdet_track_update_motion`) gives every track a velocity, estimated from its matches by an integer alpha-beta filter, moves
the box by it in every frame, matched or not, and can grow the emitted box while the track coasts:

    tr = FaceTracker(max_misses=3, min_hits=1, motion="constant_velocity", coast_grow=0.1)

The tracker cannot know what comes later.  On a finished recording `refine_tracks` (`fdet_track_refine`,
csrc/fdet_track_refine.hip) looks at whole sequences after the fact: it back-fills a track before its first detection,
interpolates the gaps between its detections, stitches the fragments of a face that was lost into one id and drops short
chains; `TrackLog` collects what a video tracked in several `update` calls needs for it:

    log = TrackLog()
    log.append(rows, tr.update(rows, counts))       # per call
    refined = log.refine(lookback=5, min_length=3).tracks
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import hotpath as hp
from ._native import FdetError

TRACK_DTYPE = np.dtype([("id", "<i4"), ("x1q", "<i4"), ("y1q", "<i4"), ("x2q", "<i4"), ("y2q", "<i4"), ("hits", "<i4"),
                        ("misses", "<i4"), ("born", "<i4"), ("score", "<f4"), ("reserved", "<i4", (3,))])     # fdet_track
SEQ_DTYPE = np.dtype([("next_id", "<i4"), ("frame", "<i4"), ("dropped", "<i4"), ("reserved", "<i4")])         # fdet_track_seq
STATE_DTYPE = np.dtype([("seq", SEQ_DTYPE), ("tracks", TRACK_DTYPE, (hp.TRACK_SLOTS,))])
# the same 48 bytes as a tracker with a motion model keeps them: reserved[0], reserved[1] are the velocity in 1/256 pixel per frame
MOTION_TRACK_DTYPE = np.dtype([(n, "<i4") for n in ("id", "x1q", "y1q", "x2q", "y2q", "hits", "misses", "born")] +
                              [("score", "<f4"), ("vx256", "<i4"), ("vy256", "<i4"), ("reserved", "<i4")])
MOTION_STATE_DTYPE = np.dtype([("seq", SEQ_DTYPE), ("tracks", MOTION_TRACK_DTYPE, (hp.TRACK_SLOTS,))])
assert MOTION_TRACK_DTYPE.itemsize == 48 and MOTION_STATE_DTYPE.itemsize == hp.TRACK_STATE_BYTES
MOTION_MODELS = (None, "constant_velocity")
assert TRACK_DTYPE.itemsize == 48 and SEQ_DTYPE.itemsize == 16 and STATE_DTYPE.itemsize == hp.TRACK_STATE_BYTES

TrackResult = namedtuple("TrackResult", "rows counts ids misses det_ids")
TrackResult.__doc__ = """rows (T,128,5) fp32 [score,x,y,w,h] and counts (T,) int32: the tracks emitted per frame, in the
shape `render_detections` takes; ids / misses (T,128) int32: each emitted track's id and the frames since it was last
detected (0 = detected in this frame); det_ids (T,K) int32: the id each input row was matched to or born as, 0 = none."""


def alpha_to_256(alpha: float) -> int:
    """round(alpha * 256), which must lie in 1..256."""
    a = int(round(float(alpha) * 256))
    if not 1 <= a <= 256:
        raise ValueError(f"FaceTracker: alpha={alpha} gives alpha256={a}, 1..256 are supported (alpha in (0, 1])")
    return a


def unit_to_256(name: str, value: float) -> int:
    """rint(value * 256), which must lie in 0..256."""
    v = int(np.rint(float(value) * 256))
    if not 0 <= v <= 256:
        raise ValueError(f"FaceTracker: {name}={value} gives {v}/256, 0..256 are supported ({name} in [0, 1])")
    return v


class FaceTracker:
    """n_seq independent sequences (cameras, files), each with 128 track slots.  iou_threshold: least overlap of a track and a
    detection that may be matched, in [0, 1).  alpha: weight of the new detection in a matched track's box (1 = take the
    detection, smaller = smoother).  max_misses: a track that goes unmatched for more frames than this dies.  min_hits: a
    track is emitted from its min_hits-th detection on (2 keeps one-frame false positives out).  emit_misses: an unmatched
    track is emitted for this many frames (None = max_misses, 0 = never).  birth_score: least score that starts a track.

    motion: None (a missed track stays where it was; `fdet_track_update`) or "constant_velocity" (`fdet_track_update_motion`,
    fixed at construction: a state is driven by one entry from fresh on).  With it every track carries a velocity and its box
    moves by it each frame before matching, so a moving face is still covered, and still matched, after a gap.  beta in
    [0, 1]: gain of the velocity update from a match's centre residual (1 with alpha = 1 predicts exact constant motion from
    the third frame on, 0 never moves anything).  damping in [0, 1]: what a missed track keeps of its velocity per frame.
    max_speed: bound on the velocity in whole pixels per frame, 0..1024.  coast_grow in [0, 1]: the emitted box of a track
    missed for m frames grows by coast_grow * m / 2 of its width and height on every side; the state and the matching never
    grow.  beta = 0.5, damping = 1.0 and max_speed = 64 are guesses: nobody has measured them on real video.  They are
    ignored without a motion model."""

    def __init__(self, n_seq: int = 1, iou_threshold: float = 0.3, alpha: float = 0.5, max_misses: int = 5, min_hits: int = 2,
                 emit_misses: Optional[int] = None, birth_score: float = 0.0, device="cuda", motion: Optional[str] = None,
                 beta: float = 0.5, damping: float = 1.0, max_speed: int = 64, coast_grow: float = 0.0):
        self.n_seq = int(n_seq)
        if self.n_seq < 1:
            raise ValueError(f"FaceTracker: n_seq={n_seq} must be >= 1")
        self.iou_threshold = float(iou_threshold)
        if not 0.0 <= self.iou_threshold < 1.0:
            raise ValueError(f"FaceTracker: iou_threshold={iou_threshold} must be in [0, 1)")
        self.alpha256 = alpha_to_256(alpha)
        self.max_misses, self.min_hits = int(max_misses), int(min_hits)
        self.emit_misses = self.max_misses if emit_misses is None else int(emit_misses)
        if self.max_misses < 0 or self.min_hits < 1 or not 0 <= self.emit_misses <= self.max_misses:
            raise ValueError(f"FaceTracker: max_misses={max_misses} must be >= 0, min_hits={min_hits} >= 1 and "
                             f"emit_misses={emit_misses} in 0..max_misses")
        self.birth_score = float(birth_score)
        if motion not in MOTION_MODELS:
            raise ValueError(f"FaceTracker: motion={motion!r} must be one of {MOTION_MODELS}")
        self.motion = motion
        self.beta256, self.damp256 = unit_to_256("beta", beta), unit_to_256("damping", damping)
        self.grow256 = unit_to_256("coast_grow", coast_grow)
        self.max_speed = int(max_speed)
        if self.max_speed != max_speed or not 0 <= self.max_speed <= 1024:
            raise ValueError(f"FaceTracker: max_speed={max_speed} must be a whole number of pixels per frame in 0..1024")
        self.device = torch.device(device)
        self.state = torch.zeros(self.n_seq * hp.TRACK_STATE_BYTES, dtype=torch.uint8, device=self.device)

    def reset(self) -> None:
        """Forget every track; ids start again from 1."""
        self.state.zero_()

    def snapshot(self) -> np.ndarray:
        """Host copy of the state: (n_seq,) records {seq: fdet_track_seq, tracks: (128,) fdet_track}.  With a motion model
        the same bytes are viewed as MOTION_STATE_DTYPE, whose tracks name the velocities vx256, vy256."""
        return self.state.cpu().numpy().view(STATE_DTYPE if self.motion is None else MOTION_STATE_DTYPE).copy()

    @property
    def dropped(self) -> int:
        """Detections that found no free slot so far, over all sequences (a host read)."""
        return int(self.snapshot()["seq"]["dropped"].astype(np.int64).sum())

    def update(self, rows: torch.Tensor, counts: torch.Tensor, seq_offset=None) -> TrackResult:
        """rows (T,K,5) [score,x,y,w,h] and counts (T,) int32 on the tracker's device, as the reducers' `forward_batch` and
        `TiledDetector.detect` return them, one row per frame.  seq_offset: n_seq + 1 integers, sequence s owns frames
        seq_offset[s]..seq_offset[s+1]-1 in time order (a sequence may own none); None with n_seq == 1: all T frames.
        Raises FdetError when a sequence is rejected (a count outside 0..K, or more than 256 valid rows in a frame): the
        state of such a sequence is as it was before the call, the others have advanced.  That counter is the only host
        read."""
        T = int(rows.shape[0])
        if seq_offset is None:
            if self.n_seq != 1:
                raise ValueError(f"FaceTracker.update: seq_offset is needed with n_seq={self.n_seq}")
            seq_offset = (0, T)
        h_off = np.ascontiguousarray(np.asarray(seq_offset.cpu() if isinstance(seq_offset, torch.Tensor) else seq_offset,
                                                dtype=np.int64).reshape(-1).astype(np.int32))
        if h_off.size != self.n_seq + 1:
            raise ValueError(f"FaceTracker.update: seq_offset must hold n_seq + 1 = {self.n_seq + 1} values, got {h_off.size}")
        d_off = torch.from_numpy(h_off).to(self.device)
        args = (rows, counts, d_off, h_off, self.state, self.iou_threshold, self.alpha256, self.max_misses, self.min_hits,
                self.emit_misses, self.birth_score)
        if self.motion is None:
            out_rows, out_ids, out_misses, out_counts, det_ids, rejected = hp.track_update(*args)
        else:
            out_rows, out_ids, out_misses, out_counts, det_ids, rejected = hp.track_update_motion(
                *args, self.beta256, self.damp256, self.max_speed, self.grow256)
        n_rej = int(rejected.item())
        if n_rej:
            raise FdetError(f"FaceTracker.update: {n_rej} sequence(s) rejected by fdet_track_update{'' if self.motion is None else '_motion'} (a count outside 0..K={int(rows.shape[1])}, "
                            f"or more than {hp.TRACK_MAX_DETS} valid detections in one frame); their state is unchanged")
        return TrackResult(out_rows, out_counts, out_ids, out_misses, det_ids)


class RefinedTracks(namedtuple("RefinedTracks", "rows counts ids misses kind")):
    """rows (T,256,5) fp32 [score,x,y,w,h] and counts (T,) int32 in the shape `render_detections` takes; ids / misses / kind
    (T,256) int32: each row's chain id, the frames since (kind 3: until) the detection it stands on, and what it is:
    0 = detected, 1 = coasted by the online tracker, 2 = interpolated between two detections, 3 = back-filled before the
    first.  `overflow`: rows that found no room in a frame's 256 (not an error)."""
    overflow = 0


KIND_DETECTED, KIND_COASTED, KIND_INTERPOLATED, KIND_BACKFILLED = 0, 1, 2, 3


def _host_offsets(what: str, seq_offset, n_seq: Optional[int], T: int) -> np.ndarray:
    if seq_offset is None:
        if n_seq not in (None, 1):
            raise ValueError(f"{what}: seq_offset is needed with n_seq={n_seq}")
        seq_offset = (0, T)
    h_off = np.ascontiguousarray(np.asarray(seq_offset.cpu() if isinstance(seq_offset, torch.Tensor) else seq_offset,
                                            dtype=np.int64).reshape(-1).astype(np.int32))
    if h_off.size < 2 or (n_seq is not None and h_off.size != n_seq + 1):
        raise ValueError(f"{what}: seq_offset must hold n_seq + 1 values, got {h_off.size}")
    return h_off


def refine_tracks(det_rows: torch.Tensor, result: TrackResult, seq_offset=None, lookback: int = 5, coast_grow: float = 0.0,
                  stitch_gap: int = 10, stitch_iou: float = 0.1, min_length: int = 1) -> RefinedTracks:
    """The second, offline pass over WHOLE sequences (`fdet_track_refine`, include/fdet.h states the rule): det_rows are the
    rows that were given to `FaceTracker.update` and `result` is what it returned, every sequence of seq_offset with ALL its
    frames in time order (see `TrackLog` for a video tracked in several calls).  A track is back-filled for `lookback` frames
    before its first detection (standing still, growing by coast_grow per frame as a coasting track does), the gaps between
    its detections are interpolated whatever their length, a track born within `stitch_gap` frames after another's last
    detection and overlapping it by more than `stitch_iou` takes that one's id (stitch_gap < 0: never), and a chain with fewer
    than `min_length` detections is dropped, coasted rows and all.  The detections before a track's min_hits-th come back too.
    Raises FdetError on a rejected sequence (a count outside 0..128, an id <= 0, ids spanning more than 4096 in one sequence);
    that counter is the only host read.  lookback = 5, stitch_gap = 10, stitch_iou = 0.1 and min_length = 1 are guesses:
    nobody has measured them on real video."""
    T = int(det_rows.shape[0])
    h_off = _host_offsets("refine_tracks", seq_offset, None, T)
    d_off = torch.from_numpy(h_off).to(det_rows.device)
    out_rows, out_ids, out_misses, out_kind, out_counts, rejected = hp.track_refine(
        det_rows, result.det_ids, result.rows, result.ids, result.misses, result.counts, d_off, h_off, int(lookback),
        unit_to_256("coast_grow", coast_grow), int(stitch_gap), float(stitch_iou), int(min_length))
    n_rej, overflow = (int(v) for v in rejected.cpu().tolist())
    if n_rej:
        raise FdetError(f"refine_tracks: {n_rej} sequence(s) rejected by fdet_track_refine (a count outside 0..{hp.TRACK_SLOTS}, an "
                        f"emitted id <= 0, ids spanning more than {hp.TRACK_REFINE_MAX_IDS}, or rows that fdet_track_update does "
                        "not produce)")
    res = RefinedTracks(out_rows, out_counts, out_ids, out_misses, out_kind)
    res.overflow = overflow
    return res


RefinedLog = namedtuple("RefinedLog", "tracks seq_offset position")
RefinedLog.__doc__ = """tracks: the RefinedTracks of every logged frame, sequence-major (all frames of sequence 0 in time order,
then sequence 1, ...); seq_offset (n_seq+1,) int32 numpy: sequence s owns frames seq_offset[s]..seq_offset[s+1]-1 of it;
position (T,) int64 numpy: position[i] is the place of output frame i in the order of appending (the frames of the first
`append` from 0, those of the second after them, ...)."""


class TrackLog:
    """Keeps what `FaceTracker.update` saw and returned, call by call, for `refine_tracks` over the whole video:

        log = TrackLog()
        for rows, counts in chunks:
            log.append(rows, tracker.update(rows, counts))
        refined = log.refine(lookback=5, min_length=3)

    The tensors stay on the device.  The result does not depend on how the video was cut into calls."""

    def __init__(self, n_seq: int = 1):
        self.n_seq = int(n_seq)
        if self.n_seq < 1:
            raise ValueError(f"TrackLog: n_seq={n_seq} must be >= 1")
        self._chunks = []

    def __len__(self) -> int:
        return sum(int(c[0].shape[0]) for c in self._chunks)

    def append(self, det_rows: torch.Tensor, result: TrackResult, seq_offset=None) -> None:
        """det_rows, seq_offset: what was given to `update`; result: what it returned."""
        T = int(det_rows.shape[0])
        if int(result.rows.shape[0]) != T or tuple(result.det_ids.shape) != tuple(det_rows.shape[:2]):
            raise ValueError("TrackLog.append: result does not belong to det_rows")
        h_off = _host_offsets("TrackLog.append", seq_offset, self.n_seq, T).astype(np.int64)
        if h_off[0] != 0 or h_off[-1] != T or (np.diff(h_off) < 0).any():
            raise ValueError(f"TrackLog.append: seq_offset must run from 0 to T={T} without going back")
        self._chunks.append((det_rows, result, h_off))

    def refine(self, **kw) -> RefinedLog:
        """Gathers every sequence's frames into time order and runs `refine_tracks` (its keyword arguments) once."""
        if not self._chunks:
            raise ValueError("TrackLog.refine: nothing was appended")
        base = np.concatenate([[0], np.cumsum([int(c[0].shape[0]) for c in self._chunks])]).astype(np.int64)
        position = [np.arange(base[i] + c[2][s], base[i] + c[2][s + 1]) for s in range(self.n_seq)
                    for i, c in enumerate(self._chunks)]
        position = np.concatenate(position).astype(np.int64)
        lengths = [sum(int(c[2][s + 1] - c[2][s]) for c in self._chunks) for s in range(self.n_seq)]
        seq_offset = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        dev = self._chunks[0][0].device
        K = max(int(c[0].shape[1]) for c in self._chunks)

        def padded(t):                                       # calls may differ in K: rows past a call's K carry no id
            return t if int(t.shape[1]) == K else torch.nn.functional.pad(t, (0, 0) * (t.dim() - 2) + (0, K - int(t.shape[1])))

        order = torch.from_numpy(position).to(dev)
        det_rows = torch.cat([padded(c[0]) for c in self._chunks]).index_select(0, order)
        result = TrackResult(*(torch.cat([padded(getattr(c[1], f)) if f == "det_ids" else getattr(c[1], f) for c in self._chunks])
                               .index_select(0, order) for f in TrackResult._fields))
        return RefinedLog(refine_tracks(det_rows, result, seq_offset, **kw), seq_offset, position)
