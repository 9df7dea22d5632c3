"""Cut face chips on the device and keep the sharpest chip of each track.

    rows, counts = TiledDetector(model).detect(bank, idx)
    cs = extract_chips(bank, rows, counts, idx, size=112, margin=0.25)       # one 112x112 crop per box, on the device
    cs.chips[cs.offset[i] + j]                                               # the chip of row j of image i, (112,112,3) uint8
    save_images(cs.as_bank(), [f"faces/{k}.png" for k in range(len(cs))])

    best = BestShots(size=112)                                               # one good picture per person of a video
    for bank in chunks:
        res = tracker.update(*det.detect(bank, range(len(bank))))
        best.update(bank, res)
    best.save("gallery")                                                     # gallery/seq0_track<id>.png

A chip is a square window around the box, widened by `margin` of its longer side on every side, resampled to size x size:
exact area averaging when the window is larger than the chip, integer bilinear interpolation when it is smaller, edge
replication where the window leaves the image.  `planar=True` gives (M,3,size,size), the layout `forward_frames` takes.
`fdet_chip_extract` / `fdet_chip_best_update` (csrc/fdet_chips.hip) do the work in integers; include/fdet.h states the
rules step by step, tests/chips_cpu_ref.py restates them in numpy and DESIGN.md 5i gives the limits.  The only host read
of `extract_chips` is `counts` (n int32), which sizes the output.  The reference project has no counterpart.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import hotpath as hp
from .datasets.augment import IMAGE_DTYPE, DeviceImageBank

INFO_DTYPE = np.dtype([("image", "<i4"), ("row", "<i4"), ("wx0", "<i4"), ("wy0", "<i4"), ("S", "<i4"), ("inside256", "<i4"),
                       ("flags", "<i4"), ("reserved", "<i4"), ("sharp", "<i8")])                              # fdet_chip_info
BEST_DTYPE = np.dtype([("id", "<i4"), ("frame", "<i4"), ("image_wx0", "<i4"), ("image_wy0", "<i4"), ("S", "<i4"),
                       ("inside256", "<i4"), ("seen", "<i4"), ("reserved", "<i4"), ("sharp", "<i8")])         # fdet_chip_best
assert INFO_DTYPE.itemsize == hp.CHIP_INFO_BYTES and BEST_DTYPE.itemsize == hp.CHIP_BEST_BYTES


def margin_to_256(margin: float) -> int:
    """round(margin * 256), which must lie in 0..256."""
    m = int(round(float(margin) * 256))
    if not 0 <= m <= 256:
        raise ValueError(f"chips: margin={margin} gives margin256={m}, 0..256 are supported (margin in [0, 1])")
    return m


def check_size(size: int) -> int:
    c = int(size)
    if not hp.CHIP_MIN_SIZE <= c <= hp.CHIP_MAX_SIZE:
        raise ValueError(f"chips: size={size} outside {hp.CHIP_MIN_SIZE}..{hp.CHIP_MAX_SIZE}")
    return c


class ChipSet(namedtuple("ChipSet", "chips info offset")):
    """chips (M,size,size,3) uint8 on the device, or (M,3,size,size) with planar=True; info (M * 40,) uint8 on the device,
    M fdet_chip_info records (`records()` reads them back); offset (n+1,) numpy int32: chip offset[i] + j is row j of image
    i.  An invalid row (not finite, empty, outside its image, window side above 8192) has an all-zero chip and flags = 0."""
    __slots__ = ()

    def __len__(self) -> int:
        return int(self.chips.shape[0])

    @property
    def planar(self) -> bool:
        return int(self.chips.shape[1]) == 3

    def records(self) -> np.ndarray:
        """Host copy of info: (M,) records {image,row,wx0,wy0,S,inside256,flags,reserved,sharp}."""
        return self.info.cpu().numpy().view(INFO_DTYPE).copy()

    def as_bank(self) -> DeviceImageBank:
        """The chips as an image bank over the same memory (HWC chips only), e.g. for `render.save_images`."""
        if self.planar:
            raise ValueError("ChipSet.as_bank: planar chips are not in the bank's HWC layout; extract with planar=False")
        M, C = len(self), int(self.chips.shape[1])
        table = np.zeros(M, dtype=IMAGE_DTYPE)
        table["offset"] = np.arange(M, dtype=np.int64) * (C * C * 3)
        table["h"], table["w"] = C, C
        return DeviceImageBank(self.chips.reshape(-1), table)


def extract_chips(bank: DeviceImageBank, rows: torch.Tensor, counts: torch.Tensor, indices=None, size: int = 112,
                  margin: float = 0.25, planar: bool = False) -> ChipSet:
    """One size x size chip per row j < counts[i] of rows (n,K,5) fp32 [score,x,y,w,h] in source pixels, cut from the images
    `indices` of `bank` (all of them when None); rows and counts (n,) int32 are on the bank's device and row-aligned with
    `indices`, as the reducers, `TiledDetector.detect` and `TrackResult` hold them.  `bank` is never written."""
    C, m256 = check_size(size), margin_to_256(margin)
    src = bank if indices is None else bank.subset(np.asarray(list(indices), dtype=np.int64).reshape(-1))
    n = len(src)
    if n == 0:
        raise ValueError("extract_chips: no image")
    if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != 5 or rows.dtype != torch.float32:
        raise ValueError(f"extract_chips: rows must be ({n},K,5) float32, got {tuple(rows.shape)} {rows.dtype}")
    if tuple(counts.shape) != (n,) or counts.dtype != torch.int32:
        raise ValueError(f"extract_chips: counts must be ({n},) int32, got {tuple(counts.shape)} {counts.dtype}")
    counts = counts.contiguous()
    h_counts = np.ascontiguousarray(counts.cpu().numpy())
    chips, info, offset = hp.chip_extract(src.data, src.d_table, src.table, rows, counts, h_counts, C, m256, planar)
    return ChipSet(chips, info, offset)


class BestShots:
    """The sharpest chip of every track of n_seq sequences, kept on the device from call to call.  capacity: track ids
    1..capacity of each sequence have an entry; detections of later ids are counted in `overflow`.  size, margin: the
    chips' (see `extract_chips`).  min_side: least window side in source pixels, min_inside: least share of the window
    that lies inside the image (0..1), for a detection to compete.  Sharpness is the sum of the squared 4-neighbour
    Laplacian of the chip's luma; the first of equally sharp chips is kept."""

    def __init__(self, n_seq: int = 1, capacity: int = 1024, size: int = 112, margin: float = 0.25, min_side: int = 0,
                 min_inside: float = 0.0, device="cuda"):
        self.n_seq, self.capacity = int(n_seq), int(capacity)
        if self.n_seq < 1 or self.capacity < 1:
            raise ValueError(f"BestShots: n_seq={n_seq} and capacity={capacity} must be >= 1")
        self.size, self.margin256 = check_size(size), margin_to_256(margin)
        self.margin = self.margin256 / 256
        self.min_side = int(min_side)
        if self.min_side < 0:
            raise ValueError(f"BestShots: min_side={min_side} must be >= 0")
        self.min_inside256 = int(round(float(min_inside) * 256))
        if not 0 <= self.min_inside256 <= 256:
            raise ValueError(f"BestShots: min_inside={min_inside} must be in [0, 1]")
        self.device = torch.device(device)
        E = self.n_seq * self.capacity
        self.state = torch.zeros(E * hp.CHIP_BEST_BYTES, dtype=torch.uint8, device=self.device)
        self.chips = torch.zeros(self.n_seq, self.capacity, self.size * self.size * 3, dtype=torch.uint8, device=self.device)
        self._scratch = torch.zeros(E, dtype=torch.int64, device=self.device)
        self._overflow = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.frame_base = np.zeros(self.n_seq, np.int32)

    def reset(self) -> None:
        """Forget every entry; frames count again from 0."""
        self.state.zero_()
        self.chips.zero_()
        self._overflow.zero_()
        self.frame_base[:] = 0

    @property
    def overflow(self) -> int:
        """Detections whose track id was beyond `capacity` so far (a host read)."""
        return int(self._overflow.item())

    def update(self, bank: DeviceImageBank, res, seq_offset=None, indices=None) -> ChipSet:
        """res: the `TrackResult` of the frames `indices` of `bank` (all when None), consecutive in time per sequence, with
        seq_offset as `FaceTracker.update` took it.  Cuts a chip per emitted track and lets those the detector saw in their
        frame (misses == 0) compete; a bridged box never does.  -> the chips of this call."""
        T = int(res.rows.shape[0])
        if seq_offset is None:
            if self.n_seq != 1:
                raise ValueError(f"BestShots.update: seq_offset is needed with n_seq={self.n_seq}")
            seq_offset = (0, T)
        h_off = np.ascontiguousarray(np.asarray(seq_offset.cpu() if isinstance(seq_offset, torch.Tensor) else seq_offset,
                                                dtype=np.int64).reshape(-1).astype(np.int32))
        if h_off.size != self.n_seq + 1:
            raise ValueError(f"BestShots.update: seq_offset must hold n_seq + 1 = {self.n_seq + 1} values, got {h_off.size}")
        if h_off[0] != 0 or h_off[-1] != T or (np.diff(h_off) < 0).any():
            raise ValueError(f"BestShots.update: seq_offset must rise from 0 to the {T} frames of res, got {h_off.tolist()}")
        cs = extract_chips(bank, res.rows, res.counts, indices, self.size, self.margin, planar=False)
        ids = torch.where(res.misses == 0, res.ids, torch.zeros_like(res.ids))
        hp.chip_best_update(cs.chips, cs.info, ids, torch.from_numpy(h_off).to(self.device), h_off,
                            torch.from_numpy(self.frame_base.copy()).to(self.device), self.capacity, self.min_side,
                            self.min_inside256, self.state, self.chips, self._scratch, self._overflow)
        self.frame_base += np.diff(h_off).astype(np.int32)
        return cs

    def snapshot(self) -> np.ndarray:
        """Host copy of the gallery: (n_seq, capacity) records {id,frame,image_wx0,image_wy0,S,inside256,seen,reserved,sharp}."""
        return self.state.cpu().numpy().view(BEST_DTYPE).reshape(self.n_seq, self.capacity).copy()

    def gallery(self):
        """-> (records (E,) with a leading `seq` field, chips (E,size,size,3) uint8) of the non-empty entries, on the host, in
        (sequence, id) order."""
        snap = self.snapshot()
        s_idx, k_idx = np.nonzero(snap["id"])
        rec = np.zeros(len(s_idx), dtype=np.dtype([("seq", "<i4")] + [(n, BEST_DTYPE[n]) for n in BEST_DTYPE.names]))
        rec["seq"] = s_idx
        for n in BEST_DTYPE.names:
            rec[n] = snap[n][s_idx, k_idx]
        if len(s_idx) == 0:
            return rec, np.zeros((0, self.size, self.size, 3), np.uint8)
        sel = torch.from_numpy(s_idx * self.capacity + k_idx).to(self.device)
        chips = self.chips.reshape(self.n_seq * self.capacity, -1)[sel].cpu().numpy()
        return rec, chips.reshape(-1, self.size, self.size, 3)

    def save(self, directory, fmt: str = "png", encoder: str = "pil", quality: int = 75) -> list:
        """Write every non-empty entry to directory/seq<s>_track<id>.<fmt>; -> the paths.  encoder="device" with a JPEG `fmt`:
        the entries are encoded on the device (`render.save_images(encoder="device")`), the same files."""
        if encoder == "device" and fmt.lower() in ("jpg", "jpeg"):
            from .render import save_images
            snap = self.snapshot()
            s_idx, k_idx = np.nonzero(snap["id"])
            os.makedirs(os.fspath(directory), exist_ok=True)
            paths = [os.path.join(os.fspath(directory), f"seq{int(s)}_track{int(snap['id'][s, k])}.{fmt}") for s, k in zip(s_idx, k_idx)]
            if paths:
                table = np.zeros(len(paths), dtype=IMAGE_DTYPE)
                table["offset"] = (s_idx * self.capacity + k_idx).astype(np.int64) * (self.size * self.size * 3)
                table["h"] = table["w"] = self.size
                save_images(DeviceImageBank(self.chips.reshape(-1), table), paths, encoder="device", quality=quality)
            return paths
        from PIL import Image
        rec, chips = self.gallery()
        os.makedirs(os.fspath(directory), exist_ok=True)
        settings = {} if int(quality) == 75 or fmt.lower() not in ("jpg", "jpeg") else {"quality": int(quality)}
        paths = []
        for r, c in zip(rec, chips):
            paths.append(os.path.join(os.fspath(directory), f"seq{int(r['seq'])}_track{int(r['id'])}.{fmt}"))
            Image.fromarray(c).save(paths[-1], **settings)
        return paths
