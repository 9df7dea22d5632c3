"""Baseline JPEG files -> DeviceImageBank without a host-side pixel decode.

The hybrid split GPU JPEG decoders use (csrc/fdet_jpeg.hip): the host parses the markers and Huffman-decodes
the scan on a thread pool (`fdet_jpeg_entropy_decode`, plain C++ that ctypes calls with the GIL released) into a pinned
int16 staging buffer; one asynchronous copy and one `fdet_jpeg_reconstruct` launch per chunk do the arithmetic
(dequantisation, inverse DCT, chroma upsampling, colour conversion) on the device and write RGB straight into the bank's
buffer.  The result is byte-identical to `bank_from_files` with PIL (libjpeg-turbo's default decode).

    bank = DeviceJpegDecoder("cuda").decode_files(paths)

A file outside the supported subset (progressive, CMYK, ... : `hotpath.JPEG_UNSUPPORTED`) or that is no JPEG at all (png,
bmp) is decoded with PIL and copied into its slot; `decoder.fallbacks` lists those indices.  A corrupt or truncated JPEG
raises `FdetError` naming the file.
"""
from __future__ import annotations

import io
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import hotpath as hp
from .._native import FdetError
from .augment import IMAGE_DTYPE, DeviceImageBank

MAX_WORKERS = 16
MAX_IMAGES_PER_LAUNCH = 65535                                # fdet_jpeg_reconstruct's grid limit


def _align(v: int, a: int) -> int:
    return (v + a - 1) // a * a


class DeviceJpegDecoder:
    """decode_bytes / decode_files -> DeviceImageBank.  `workers` host threads (at most 16) entropy-decode into one of two
    pinned staging buffers of at most `chunk_bytes` of coefficients while the previous chunk copies and reconstructs."""

    def __init__(self, device, workers: int = 16, chunk_bytes: int = 256 << 20):
        self.device = torch.device(device)
        self.workers = max(1, min(MAX_WORKERS, int(workers)))
        self.chunk_bytes = max(128, int(chunk_bytes))
        self.fallbacks: List[int] = []
        self.chunks = 0                                      # reconstruct launches of the last call

    # -- host stages ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _pil_decode(data: bytes, name: str) -> np.ndarray:
        try:
            from PIL import Image
        except ImportError as e:
            raise FdetError(f"{name}: outside the device decoder's JPEG subset, and PIL is not importable to decode it") from e
        try:
            with Image.open(io.BytesIO(data)) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
        except Exception as e:                               # PIL raises OSError / SyntaxError / ValueError on bad files
            raise FdetError(f"{name}: cannot be decoded ({e})") from e

    def _probe(self, job):
        """-> (info record | None, fallback array | None) of one file."""
        data, name = job
        if len(data) < 2 or data[0] != 0xFF or data[1] != 0xD8:          # not a JPEG at all
            return None, self._pil_decode(data, name)
        rc, info, msg = hp.jpeg_info(data)
        if rc == 0:
            return info, None
        if rc == hp.JPEG_UNSUPPORTED:
            return None, self._pil_decode(data, name)
        raise FdetError(f"{name}: {msg} (code {rc})")

    # -- public --------------------------------------------------------------------------------------------------------
    def decode_files(self, paths: Sequence, lead_bytes: int = 0) -> DeviceImageBank:
        paths = list(paths)

        def read(p):
            with open(p, "rb") as f:
                return f.read()
        with ThreadPoolExecutor(max_workers=max(1, min(self.workers, len(paths) or 1))) as ex:
            blobs = list(ex.map(read, paths))
        return self.decode_bytes(blobs, lead_bytes, names=[str(p) for p in paths])

    def decode_bytes(self, blobs: Sequence[bytes], lead_bytes: int = 0, names: Optional[Sequence[str]] = None) -> DeviceImageBank:
        n = len(blobs)
        names = list(names) if names is not None else [f"image {i}" for i in range(n)]
        dev = self.device
        self.fallbacks, self.chunks = [], 0
        pool = ThreadPoolExecutor(max_workers=max(1, min(self.workers, n or 1)))
        try:
            probed = list(pool.map(self._probe, zip(blobs, names)))
            # the table DeviceImageBank.from_arrays builds
            table = np.zeros(n, dtype=IMAGE_DTYPE)
            off = int(lead_bytes)
            for i, (info, arr) in enumerate(probed):
                h, w = (int(info["height"]), int(info["width"])) if info is not None else arr.shape[:2]
                table[i] = (off, h, w)
                off += h * w * 3
            data = torch.empty(max(off, 1), dtype=torch.uint8, device=dev)
            if lead_bytes:
                data[:lead_bytes].zero_()
            with torch.cuda.device(dev):
                self._decode_into(pool, blobs, names, probed, table, data)
        finally:
            pool.shutdown(wait=True)
        return DeviceImageBank(data, table)

    # -- chunks --------------------------------------------------------------------------------------------------------
    def _plan(self, probed, table):
        """Chunks of device-decoded images: lists of (index, info), each within chunk_bytes of coefficients (an image larger
        than that is a chunk of its own) and the launch's image limit."""
        cap = self.chunk_bytes // 2
        chunks, cur, fill = [], [], 0
        for i, (info, _arr) in enumerate(probed):
            if info is None:
                continue
            need = _align(int(info["coef_count"]), 8)
            if cur and (fill + need > cap or len(cur) >= MAX_IMAGES_PER_LAUNCH):
                chunks.append(cur)
                cur, fill = [], 0
            cur.append((i, info))
            fill += need
        if cur:
            chunks.append(cur)
        return chunks

    @staticmethod
    def _describe(chunk, table):
        descs = np.zeros(len(chunk), dtype=hp.JPEG_DESC_DTYPE)
        coef_at, plane_at, spans = 0, 0, []
        for k, (i, info) in enumerate(chunk):
            d = descs[k]
            nc = int(info["ncomp"])
            d["bank_offset"] = table[i]["offset"]
            d["width"], d["height"], d["ncomp"] = info["width"], info["height"], nc
            d["hs"], d["vs"] = info["hs"][0], info["vs"][0]
            d["blocks_w"], d["blocks_h"], d["qt"] = info["blocks_w"], info["blocks_h"], info["qt"]
            start = coef_at
            for c in range(nc):
                nb = int(info["blocks_w"][c]) * int(info["blocks_h"][c])
                d["coef_offset"][c] = coef_at
                d["plane_offset"][c] = plane_at
                coef_at += nb * 64
                plane_at += nb * 64
            spans.append((start, int(info["coef_count"])))
            coef_at = _align(coef_at, 8)
        return descs, spans, coef_at, plane_at

    def _decode_into(self, pool, blobs, names, probed, table, data) -> None:
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        for i, (info, arr) in enumerate(probed):             # the files another decoder took
            if info is None:
                self.fallbacks.append(i)
                o = int(table[i]["offset"])
                data[o:o + arr.size].copy_(torch.from_numpy(arr.reshape(-1)))
        chunks = self._plan(probed, table)
        if not chunks:
            return
        plans = [self._describe(ch, table) for ch in chunks]
        cap = max(p[2] for p in plans)
        ws_cap = max(p[3] for p in plans)
        n_stage = min(2, len(chunks))
        stage = [torch.empty(cap, dtype=torch.int16).pin_memory() for _ in range(n_stage)]
        busy = [None] * n_stage                              # event per staging buffer: its copy and launch are done
        hold = [None] * n_stage                              # the pinned descriptors of the launch that uses the buffer
        d_coef = torch.empty(cap, dtype=torch.int16, device=dev)
        workspace = torch.empty(max(ws_cap, 8), dtype=torch.uint8, device=dev)
        try:
            for k, (chunk, (descs, spans, used, _ws)) in enumerate(zip(chunks, plans)):
                s = k % n_stage
                if busy[s] is not None:
                    busy[s].synchronize()                    # the copy out of this buffer two chunks ago has finished
                base = stage[s].data_ptr()

                def work(job, base=base):
                    (i, _info), (start, count) = job
                    rc, msg = hp.jpeg_entropy_decode(blobs[i], base + 2 * start, count)
                    return i, rc, msg
                for i, rc, msg in pool.map(work, zip(chunk, spans)):
                    if rc != 0:
                        raise FdetError(f"{names[i]}: {msg} (code {rc})")
                d_coef[:used].copy_(stage[s][:used], non_blocking=True)
                h_descs = torch.from_numpy(descs.view(np.uint8)).pin_memory()
                d_descs = h_descs.to(dev, non_blocking=True)
                hp.jpeg_reconstruct(d_coef, d_descs, descs, workspace, data)
                ev = torch.cuda.Event()
                ev.record(stream)
                busy[s], hold[s] = ev, (h_descs, d_descs)
                self.chunks += 1
        finally:
            stream.synchronize()                             # nothing of this call is in flight when its buffers go
