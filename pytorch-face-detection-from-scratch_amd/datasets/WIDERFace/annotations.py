"""WIDER Face annotation files and image loading for the device image bank (host code).

`read_wider_annotations` parses `wider_face_split/wider_face_{split}_bbx_gt.txt` the way the reference's
`WIDERFaceDataModule.get_targets` does (datasets/WIDERFace/datamodule.py:69-103): an image line (ends in "jpg"), a count
line, then one `x y w h blur expression illumination invalid occlusion pose` line per face, of which the first four
numbers are kept as a row [1, x, y, w, h].  An image without faces carries the placeholder line `0 0 0 0 0 0 0 0 0 0`,
which the reference keeps as a box of zero size; `keep_placeholder=False` drops it (what an evaluation wants: a box of
zero area can never be matched).  `bank_from_files` decodes the images into a `DeviceImageBank`: with PIL (the default) or,
`decoder="device"`, with the hybrid JPEG decoder of datasets/jpeg.py, which gives the same bytes.
"""
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np


def read_wider_annotations(root, split: str = "val", max_faces: Optional[int] = None,
                           keep_placeholder: bool = True) -> Tuple[List[Path], List[np.ndarray]]:
    """-> (image paths `root/WIDER_{split}/images/<line>`, per-image (n,5) float32 boxes [1,x,y,w,h]).  `max_faces=2`
    reproduces the reference's filter (images with fewer than 3 rows, the placeholder row counting as one)."""
    root = Path(root)
    lines = (root / "wider_face_split" / f"wider_face_{split}_bbx_gt.txt").read_text().split("\n")
    paths: List[Path] = []
    boxes: List[list] = []
    counts: List[int] = []
    for line in lines:
        line = line.strip()
        if not line:
            continue
        if line.endswith("jpg"):
            paths.append(root / f"WIDER_{split}" / "images" / line)
            boxes.append([])
            counts.append(0)
            continue
        if not paths:
            raise ValueError(f"annotation file starts with {line!r}, not with an image line")
        fields = line.split()
        if len(fields) == 1:
            counts[-1] = int(fields[0])
        elif len(fields) >= 4:
            boxes[-1].append([1.0] + [float(f) for f in fields[:4]])
        else:
            raise ValueError(f"cannot parse annotation line {line!r}")
    out_p, out_b = [], []
    for p, b, c in zip(paths, boxes, counts):
        if max_faces is not None and len(b) > max_faces:
            continue
        if c == 0 and not keep_placeholder:
            b = []
        out_p.append(p)
        out_b.append(np.asarray(b, dtype=np.float32).reshape(-1, 5))
    return out_p, out_b


def _decode(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def bank_from_files(paths: Sequence, device, workers: int = 16, decoder: str = "pil", huffman: str = "host"):
    """Decode `paths` on at most 16 threads into a DeviceImageBank on `device` (RGB, HWC uint8).  A once-per-run cost: the
    bank stays resident.  decoder="pil" decodes on the host with PIL; decoder="device" Huffman-decodes on the host and
    reconstructs on the device (datasets/jpeg.py DeviceJpegDecoder; files outside its JPEG subset still go through PIL);
    with huffman="device" the Huffman decoding runs on the device too and only the file bytes cross to it.  All give the
    same bank, byte for byte."""
    if decoder not in ("pil", "device"):
        raise ValueError(f"decoder must be 'pil' or 'device', got {decoder!r}")
    if huffman not in ("host", "device"):
        raise ValueError(f"huffman must be 'host' or 'device', got {huffman!r}")
    if huffman == "device" and decoder != "device":
        raise ValueError("huffman='device' needs decoder='device'")
    if decoder == "device":
        from ..jpeg import DeviceJpegDecoder
        return DeviceJpegDecoder(device, workers=workers, huffman=huffman).decode_files(paths)
    from ..augment import DeviceImageBank
    workers = max(1, min(16, int(workers), len(paths) or 1))
    with ThreadPoolExecutor(max_workers=workers) as ex:
        images = list(ex.map(_decode, paths))
    return DeviceImageBank.from_arrays(images, device)
