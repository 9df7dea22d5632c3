"""Render detections into a second device image bank: outlines as PIL draws them, and pixelation for anonymisation.

    rows, counts = TiledDetector(model).detect(bank, idx)
    drawn = render_detections(bank, rows, counts, idx)                                   # blue outlines, reference widths
    anon = render_detections(bank, rows, counts, idx, outline=False, anonymize="pixelate")
    save_images(drawn, [f"out/{i}.png" for i in range(len(drawn))])

The pixels never leave the device between the detector and the rendered bank: `fdet_render_boxes` (csrc/fdet_render.hip)
copies the chosen images device to device and works on the boxes alone.  The only host read is `counts` (n int32), which
sizes the launches and is validated before anything is written (`anonymize="blur"` also reads `rows` back, to size its
workspace).  Rules, limits and measurements: DESIGN.md 5g and 5r; tests/render_cpu_ref.py and tests/render_blur_cpu_ref.py
restate the rules in numpy.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Sequence

import numpy as np
import torch

from ._native import FdetError, check, lib, ptr, stream
from .datasets.augment import IMAGE_DTYPE, DeviceImageBank

ANONYMIZERS = (None, "pixelate", "blur")
BLUR_MAX_LINE = 8192                  # FDET_BLUR_MAX_LINE: the longest image side `anonymize="blur"` takes


def blur_params(radius) -> np.ndarray:
    """Gaussian radii (any shape) -> (...,3) int64 (r, ww, fw): the box radius of PIL's three-pass approximation
    (BoxBlur.c `_gaussian_blur_radius`) and the fixed-point weights of one pass (`ImagingHorizontalBoxBlur`), in float32
    operation by operation as C evaluates them: only the square root is taken in double, and the division behind `ww` is
    a float32 division."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        radius = np.asarray(radius, f32)
        s2 = radius * radius / f32(3)
        L = np.sqrt(12.0 * s2.astype(np.float64) + 1.0).astype(f32)
        l = np.floor((L.astype(np.float64) - 1.0) / 2.0).astype(f32)
        a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * s2)
        a = a / (f32(6) * (s2 - (l + f32(1)) * (l + f32(1))))
        fr = l + a
        ww = (f32(1 << 24) / (fr * f32(2) + f32(1))).astype(np.int64)
    if not np.isfinite(fr).all() or (fr < 0).any():
        raise ValueError("blur_params: a radius that is negative or not finite")
    r = fr.astype(np.int64)
    return np.stack([r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2], axis=-1)


def check_blur_table(tab: np.ndarray) -> None:
    """The bound `fdet_render_boxes_blur` validates: with it a pass never leaves unsigned 32-bit arithmetic."""
    t = np.asarray(tab).astype(np.int64).reshape(-1, 3)
    if len(t) < 1 or (t < 0).any() or ((2 * t[:, 0] + 1) * t[:, 1] + 2 * t[:, 2] > 1 << 24).any():
        raise ValueError("blur table: an entry (r, ww, fw) is negative or has weights (2r+1)*ww + 2*fw above 2^24")


_BLUR_TABLES: dict = {}


def blur_table(blocks: int = 8, radius: Optional[float] = None, n: int = 2 * BLUR_MAX_LINE + 2, device=None):
    """-> (n,3) int32 (r, ww, fw): entry S holds PIL's parameters for GaussianBlur(radius(S)), with
    radius(S) = float32(S) / float32(blocks), or the fixed `radius` in every entry when one is given.  A box whose longer side
    S reaches past the table takes entry n-1.  device=None: the numpy table; else (device tensor, numpy table), cached per
    (blocks, radius, n, device)."""
    if int(blocks) < 1 or int(n) < 1:
        raise ValueError(f"blur_table: blocks={blocks} and n={n} must be >= 1")
    if radius is not None and not 0 <= float(radius) <= 4096:
        raise ValueError(f"blur_table: radius={radius} must be in 0..4096")
    key = (int(blocks), None if radius is None else float(np.float32(radius)), int(n), None if device is None else str(torch.device(device)))
    hit = _BLUR_TABLES.get(key)
    if hit is None:
        S = np.arange(int(n), dtype=np.float32)
        rad = S / np.float32(blocks) if radius is None else np.full(int(n), radius, np.float32)
        tab = blur_params(rad)
        check_blur_table(tab)
        tab = np.ascontiguousarray(tab.astype(np.int32))
        tab.setflags(write=False)
        hit = tab if device is None else (torch.from_numpy(tab.copy()).to(device), tab)
        _BLUR_TABLES[key] = hit
    return hit


def render_detections(bank: DeviceImageBank, rows: torch.Tensor, counts: torch.Tensor, indices=None, outline: bool = True,
                      anonymize: Optional[str] = None, blocks: int = 8, color=(0, 0, 255),
                      blur_radius: Optional[float] = None, ws: Optional[torch.Tensor] = None) -> DeviceImageBank:
    """-> a new bank over its own buffer holding the images `indices` of `bank` (all of them when None), renumbered
    0..len(indices)-1, with the first counts[i] boxes of rows[i] rendered into image i.  rows (n,K,5) fp32 [score,x,y,w,h] in
    source pixels and counts (n,) int32 on the bank's device, row-aligned with `indices`, as `TiledDetector.detect` returns
    them.  anonymize="pixelate": every box becomes at most `blocks` x `blocks` flat cells (the mean of the source pixels of
    each cell); anonymize="blur": every box becomes what `im.crop(box).filter(GaussianBlur(radius))` pasted back gives, byte for
    byte, with radius = the box's longer side / `blocks`, or the fixed `blur_radius` (this mode reads `rows`
    back to size its workspace unless the caller passes one, `ws`, a uint8 tensor of `hotpath.render_blur_ws_bytes` bytes
        to reuse between calls; a box `ws` does not hold raises FdetError; images of at most 8192 pixels a side); outline: a
    `color` outline of the reference's width on top.  `bank` is never written."""
    if anonymize not in ANONYMIZERS:
        raise ValueError(f"render_detections: anonymize must be None, 'pixelate' or 'blur', got {anonymize!r}")
    if blur_radius is not None and anonymize != "blur":
        raise ValueError("render_detections: blur_radius needs anonymize='blur'")
    if int(blocks) < 1:
        raise ValueError(f"render_detections: blocks={blocks} must be >= 1")
    col = tuple(int(c) for c in color)
    if len(col) != 3 or any(not 0 <= c <= 255 for c in col):
        raise ValueError(f"render_detections: color must be three values in 0..255, got {color!r}")
    src = bank if indices is None else bank.subset(np.asarray(list(indices), dtype=np.int64).reshape(-1))
    n = len(src)
    if n == 0:
        raise ValueError("render_detections: no image")
    if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != 5 or rows.dtype != torch.float32:
        raise ValueError(f"render_detections: rows must be ({n},K,5) float32, got {tuple(rows.shape)} {rows.dtype}")
    if tuple(counts.shape) != (n,) or counts.dtype != torch.int32:
        raise ValueError(f"render_detections: counts must be ({n},) int32, got {tuple(counts.shape)} {counts.dtype}")
    table = np.zeros(n, dtype=IMAGE_DTYPE)
    sizes = src.table["h"].astype(np.int64) * src.table["w"] * 3
    table["offset"][1:] = np.cumsum(sizes)[:-1]
    table["h"], table["w"] = src.table["h"], src.table["w"]
    dev = bank.device
    out = DeviceImageBank(torch.empty(int(sizes.sum()), dtype=torch.uint8, device=dev), table)
    rows, counts = rows.contiguous(), counts.contiguous()
    h_counts = np.ascontiguousarray(counts.cpu().numpy())
    if ws is not None and anonymize != "blur":
        raise ValueError("render_detections: ws needs anonymize='blur'")
    U8, I32 = torch.uint8, torch.int32
    K = int(rows.shape[1])
    if anonymize == "blur":
        from .hotpath import render_boxes_blur
        d_tab, h_tab = blur_table(blocks, blur_radius, 2 * int(max(src.table["h"].max(), src.table["w"].max())) + 2, dev)
        rejected = render_boxes_blur(src, rows, counts, h_counts, out, d_tab, h_tab, outline=outline, blocks=blocks, color=col, ws=ws)
        n_rej = int(rejected.item())
        if n_rej:
            raise FdetError(f"render_detections: {n_rej} box(es) rejected by fdet_render_boxes_blur (the workspace does not hold them)")
        return out
    ws = torch.empty(n + 1, dtype=torch.int32, device=dev)
    check(lib().fdet_render_boxes(ptr(src.data, U8), ptr(src.d_table, U8), src.table.ctypes.data, ptr(rows) if K else None,
                                  ptr(counts, I32), h_counts.ctypes.data, n, K, ptr(out.data, U8), ptr(out.d_table, U8),
                                  out.table.ctypes.data, int(bool(outline)), int(anonymize == "pixelate"), int(blocks), col[0],
                                  col[1], col[2], ptr(ws, I32), stream()), "fdet_render_boxes")
    return out


ENCODERS = ("pil", "device")
JPEG_SUFFIXES = (".jpg", ".jpeg")


def save_images(bank: DeviceImageBank, paths: Sequence, threads: int = 16, encoder: str = "pil", quality: int = 75,
                subsampling: str = "4:2:0") -> None:
    """Write image i of `bank` to paths[i] with PIL, PNG or JPEG by the suffix, on at most 16 threads.  Parent directories
    are created.  encoder="device": the paths with a .jpg / .jpeg suffix are encoded on the device (datasets/jpeg.py
    DeviceJpegEncoder: only the compressed scans cross to the host) with `quality` and `subsampling`; the files are the ones
    PIL writes with those settings, byte for byte, and the defaults are PIL's.  Every other suffix still goes to PIL, and
    encoder="pil" hands `quality` and `subsampling` to PIL for its JPEG files when they are not the defaults."""
    if encoder not in ENCODERS:
        raise ValueError(f"save_images: encoder must be 'pil' or 'device', got {encoder!r}")
    paths = [os.fspath(p) for p in paths]
    if len(paths) != len(bank):
        raise ValueError(f"save_images: {len(paths)} paths for a bank of {len(bank)} images")
    for d in sorted({os.path.dirname(p) for p in paths}):
        if d:
            os.makedirs(d, exist_ok=True)
    rest = list(range(len(paths)))
    if encoder == "device":
        from .datasets.jpeg import DeviceJpegEncoder
        jpeg = [i for i in rest if os.path.splitext(paths[i])[1].lower() in JPEG_SUFFIXES]
        rest = [i for i in rest if os.path.splitext(paths[i])[1].lower() not in JPEG_SUFFIXES]
        if jpeg:
            DeviceJpegEncoder(bank.device, quality, subsampling).encode_to_files(bank, [paths[i] for i in jpeg], threads, indices=jpeg)
    if not rest:
        return
    from PIL import Image
    arrays = bank.to_arrays() if len(rest) == len(paths) else bank.to_arrays(rest)

    settings = {}                                            # PIL's own defaults unless the caller chose others
    if (int(quality), subsampling) != (75, "4:2:0"):
        settings = {"quality": int(quality), "subsampling": subsampling}

    def save(job):
        jpeg = os.path.splitext(job[1])[1].lower() in JPEG_SUFFIXES
        Image.fromarray(job[0]).save(job[1], **(settings if jpeg else {}))

    with ThreadPoolExecutor(max_workers=max(1, min(16, int(threads), len(rest)))) as ex:
        list(ex.map(save, zip(arrays, [paths[i] for i in rest])))
