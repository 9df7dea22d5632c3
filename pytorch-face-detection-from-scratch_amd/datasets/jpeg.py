"""Baseline JPEG files -> DeviceImageBank without a host-side pixel decode.

The hybrid split GPU JPEG decoders use (csrc/fdet_jpeg.hip): the host parses the markers and Huffman-decodes
the scan on a thread pool (`fdet_jpeg_entropy_decode`, plain C++ that ctypes calls with the GIL released) into a pinned
int16 staging buffer; one asynchronous copy and one `fdet_jpeg_reconstruct` launch per chunk do the arithmetic
(dequantisation, inverse DCT, chroma upsampling, colour conversion) on the device and write RGB straight into the bank's
buffer.  The result is byte-identical to `bank_from_files` with PIL (libjpeg-turbo's default decode).

    bank = DeviceJpegDecoder("cuda").decode_files(paths)

With `huffman="device"` (csrc/fdet_jpeg_huff.hip) the Huffman decoding runs on the device as well: the worker
threads only unstuff the scans and build the decode tables (`fdet_jpeg_scan_prepare`), the file bytes cross to the device,
self-synchronising passes find the symbol boundaries and an emit launch writes the same int16 planes there.  An image the
device path cannot vouch for is decoded by the host path after all (`decoder.huffman_fallbacks`); the bank is the same.

    bank = DeviceJpegDecoder("cuda", huffman="device").decode_files(paths)

The other direction is `DeviceJpegEncoder` (csrc/fdet_jpeg_enc.hip): colour conversion, downsampling, forward
DCT, quantisation AND the Huffman coding run on the device, so that only the compressed scan crosses to the host, which adds
the header, stuffs the FF bytes and writes the file -- byte for byte what PIL's `Image.save(..., "JPEG")` writes.

    files = DeviceJpegEncoder("cuda", quality=75, subsampling="4:2:0").encode(bank)      # List[bytes]

A file outside the supported subset (progressive, CMYK, ... : `hotpath.JPEG_UNSUPPORTED`) or that is no JPEG at all (png,
bmp) is decoded with PIL and copied into its slot; `decoder.fallbacks` lists those indices.  A corrupt or truncated JPEG
raises `FdetError` naming the file.
"""
from __future__ import annotations

import io
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import hotpath as hp
from .._native import FdetError
from .augment import IMAGE_DTYPE, DeviceImageBank

MAX_WORKERS = 16
MAX_IMAGES_PER_LAUNCH = 65535                                # fdet_jpeg_reconstruct's grid limit
DEFAULT_SUB_BITS = 1024                                      # huffman="device": bits per subsequence
SYNC_ROUND = 4                                               # sync passes enqueued between two looks at `changed`


def _align(v: int, a: int) -> int:
    return (v + a - 1) // a * a


class DeviceJpegDecoder:
    """decode_bytes / decode_files -> DeviceImageBank.  `workers` host threads (at most 16) entropy-decode into one of two
    pinned staging buffers of at most `chunk_bytes` of coefficients while the previous chunk copies and reconstructs.
    huffman="device": the threads run fdet_jpeg_scan_prepare instead and the device decodes the scans, in subsequences of
    `sub_bits` bits (a multiple of 32, at least 64) and at most `max_sync_passes` synchronisation passes per chunk (None: as
    many as the longest segment can need); `huffman_fallbacks` lists the images the host decoded after all, `sync_passes`
    the passes enqueued."""

    def __init__(self, device, workers: int = 16, chunk_bytes: int = 256 << 20, huffman: str = "host",
                 sub_bits: int = DEFAULT_SUB_BITS, max_sync_passes: Optional[int] = None):
        if huffman not in ("host", "device"):
            raise ValueError(f"DeviceJpegDecoder: huffman must be 'host' or 'device', got {huffman!r}")
        sub_bits = int(sub_bits)
        if sub_bits < 64 or sub_bits % 32:
            raise ValueError(f"DeviceJpegDecoder: sub_bits={sub_bits} must be a multiple of 32 and at least 64")
        if max_sync_passes is not None and int(max_sync_passes) < 1:
            raise ValueError(f"DeviceJpegDecoder: max_sync_passes={max_sync_passes} must be at least 1")
        self.device = torch.device(device)
        self.workers = max(1, min(MAX_WORKERS, int(workers)))
        self.chunk_bytes = max(128, int(chunk_bytes))
        self.huffman = huffman
        self.sub_bits = sub_bits
        self.max_sync_passes = None if max_sync_passes is None else int(max_sync_passes)
        self.fallbacks: List[int] = []
        self.chunks = 0                                      # reconstruct launches of the last call
        self.huffman_fallbacks: List[int] = []               # huffman="device": images the host Huffman-decoded after all
        self.sync_passes = 0                                 # synchronisation passes enqueued by the last call
        self.scan_bytes = 0                                  # bytes of scans, tables and descriptors the last call copied across
        self.timings = None                                  # a dict to fill with per-stage seconds (tools/jpeg_throughput.py)
        self._bufs = {}

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
        self.huffman_fallbacks, self.sync_passes, self.scan_bytes = [], 0, 0
        for i, (info, arr) in enumerate(probed):             # the files another decoder took
            if info is None:
                self.fallbacks.append(i)
                o = int(table[i]["offset"])
                data[o:o + arr.size].copy_(torch.from_numpy(arr.reshape(-1)))
        chunks = self._plan(probed, table)
        if not chunks:
            return
        plans = [self._describe(ch, table) for ch in chunks]
        if self.huffman == "device":
            return self._decode_chunks_device_huffman(pool, blobs, names, chunks, plans, data)
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


    # -- huffman="device" ---------------------------------------------------------------------------------------------
    def _buf(self, key, numel, dtype, pinned=False):
        """A grow-only buffer kept across calls -> its first `numel` elements."""
        t = self._bufs.get(key)
        if t is None or t.numel() < numel:
            cap = max(int(numel), 16)
            t = torch.empty(cap, dtype=dtype).pin_memory() if pinned else torch.empty(cap, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t[:numel]

    def _clock(self, key, t0):
        if self.timings is not None:
            self.timings[key] = self.timings.get(key, 0.0) + time.perf_counter() - t0

    def huffman_stage(self, pool, blobs, names, chunk, descs):
        """fdet_jpeg_scan_prepare of one chunk on the worker threads into pinned staging, the subsequence layout, and the
        asynchronous copies -> (d_scan, d_tables, d_images, images, d_segs, segs, subsequences, positions prepare sent to
        the host): the arguments of hotpath.jpeg_huffman_sync / jpeg_huffman_emit."""
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        n = len(chunk)
        t0 = time.perf_counter()
        images = np.zeros(n, dtype=hp.JPEG_HUFF_IMAGE_DTYPE)
        nsegs = np.zeros(n, dtype=np.int64)
        for k, (i, info) in enumerate(chunk):
            mcus = int(info["mcus_x"]) * int(info["mcus_y"])
            nsegs[k] = -(-mcus // (int(info["restart_interval"]) or mcus))
            im = images[k]
            im["coef_offset"], im["ncomp"] = descs[k]["coef_offset"], info["ncomp"]
            im["hs"], im["vs"], im["mcus_x"], im["mcus_y"] = info["hs"][0], info["vs"][0], info["mcus_x"], info["mcus_y"]
        caps = np.array([_align(len(blobs[i]), 16) for i, _ in chunk], dtype=np.int64) + 16 * nsegs
        base = np.cumsum(caps) - caps
        images["seg_count"] = nsegs
        images["seg_first"] = np.cumsum(nsegs) - nsegs
        S = int(nsegs.sum())
        h_scan = self._buf("h_scan", int(caps.sum()), torch.uint8, pinned=True)
        h_segs_t = self._buf("h_segs", S * hp.JPEG_HUFF_SEG_DTYPE.itemsize, torch.uint8, pinned=True)
        h_tab = self._buf("h_tables", n * hp.JPEG_HUFF_TABLES_DTYPE.itemsize, torch.uint8, pinned=True)
        segs = h_segs_t.numpy().view(hp.JPEG_HUFF_SEG_DTYPE)
        p_scan, p_segs, p_tab = h_scan.data_ptr(), h_segs_t.data_ptr(), h_tab.data_ptr()

        def work(k):
            i = chunk[k][0]
            rc, used, got, msg = hp.jpeg_scan_prepare(blobs[i], p_scan + int(base[k]), int(caps[k]),
                                                      p_segs + int(images["seg_first"][k]) * hp.JPEG_HUFF_SEG_DTYPE.itemsize,
                                                      int(nsegs[k]),
                                                      p_tab + k * hp.JPEG_HUFF_TABLES_DTYPE.itemsize)
            return k, rc, got, msg
        host = set()
        for k, rc, got, msg in pool.map(work, range(n)):
            a = int(images["seg_first"][k])
            if rc == hp.JPEG_HUFF_HOST or (rc == 0 and got != int(nsegs[k])):
                # an empty scan over all the MCUs: valid for the kernels, flagged EXHAUSTED by the emit, decoded below
                host.add(k)
                segs[a:a + int(nsegs[k])] = 0
                segs["mcu_count"][a:a + int(nsegs[k])] = 0
                images["seg_count"][k] = 1
                segs["mcu_count"][a] = int(images["mcus_x"][k]) * int(images["mcus_y"][k])
            elif rc != 0:
                raise FdetError(f"{names[chunk[k][0]]}: {msg} (code {rc})")
            segs["byte_offset"][a:a + int(nsegs[k])] += int(base[k])
            segs["image"][a:a + int(nsegs[k])] = k
        if host:                                             # their unused segment records leave the array
            keep = segs["mcu_count"] > 0
            segs = np.ascontiguousarray(segs[keep])
            images["seg_first"] = np.cumsum(images["seg_count"]) - images["seg_count"]
        n_subs = hp.jpeg_huff_layout(images, segs, self.sub_bits)
        if host:                                             # the compacted records, back into the pinned buffer
            h_segs_t = h_segs_t[:segs.nbytes]
            h_segs_t.numpy()[:] = segs.view(np.uint8)
            segs = h_segs_t.numpy().view(hp.JPEG_HUFF_SEG_DTYPE)
        self._clock("prepare", t0)
        t0 = time.perf_counter()
        h_images_t = self._buf("h_images", images.nbytes, torch.uint8, pinned=True)
        h_images_t.numpy()[:] = images.view(np.uint8)
        d_scan = self._buf("d_scan", h_scan.numel(), torch.uint8)
        d_segs = self._buf("d_segs", h_segs_t.numel(), torch.uint8)
        d_tab = self._buf("d_tables", h_tab.numel(), torch.uint8)
        d_images = self._buf("d_images", h_images_t.numel(), torch.uint8)
        for d, h in ((d_scan, h_scan), (d_segs, h_segs_t), (d_tab, h_tab), (d_images, h_images_t)):
            d.copy_(h, non_blocking=True)
        self.scan_bytes += h_scan.numel() + h_segs_t.numel() + h_tab.numel() + h_images_t.numel()
        if self.timings is not None:
            stream.synchronize()
            self._clock("copy", t0)
        return d_scan, d_tab, d_images, images, d_segs, segs, n_subs, host

    def huffman_chunk(self, pool, blobs, names, chunk, descs, coef_count: int, d_coef: torch.Tensor):
        """The scans of one chunk (chunk: [(index, info)], descs: its fdet_jpeg_desc records) -> coefficient planes in
        d_coef[:coef_count] on the current stream.  -> the positions within the chunk whose planes the host has still to
        decode (prepare said so, the emit parse flagged them, or they were still changing at the pass cap)."""
        stream = torch.cuda.current_stream(self.device)
        n = len(chunk)
        d_scan, d_tab, d_images, images, d_segs, segs, n_subs, host = self.huffman_stage(pool, blobs, names, chunk, descs)
        state = self._buf("state", 3 * n_subs, torch.int64)
        first_block = self._buf("first_block", n_subs, torch.int32)
        words = self._buf("words", (SYNC_ROUND + 1) * n, torch.int32)       # `changed` of a round's passes, then the flags
        h_words = self._buf("h_words", (SYNC_ROUND + 1) * n, torch.int32, pinned=True)
        state.zero_()
        # sync passes in rounds: one small copy and one synchronise per round
        t0 = time.perf_counter()
        cap = self.max_sync_passes if self.max_sync_passes is not None else int(segs["sub_count"].max()) + 1
        done, quiet = 0, np.zeros(n, dtype=bool)
        while done < cap and not quiet.all():
            r = min(SYNC_ROUND, cap - done)
            words[:r * n].zero_()
            for j in range(r):
                hp.jpeg_huffman_sync(d_scan, d_tab, d_images, images, d_segs, segs, self.sub_bits, state, words[j * n:(j + 1) * n])
            h_words[:r * n].copy_(words[:r * n], non_blocking=True)
            stream.synchronize()
            done += r
            quiet = (h_words[:r * n].numpy().reshape(r, n) == 0).any(axis=0)   # a pass that changed nothing: the fixed point
        self.sync_passes += done
        self._clock("sync", t0)
        t0 = time.perf_counter()
        flags = words[SYNC_ROUND * n:]
        flags.zero_()
        hp.jpeg_huffman_emit(d_scan, d_tab, d_images, images, d_segs, segs, self.sub_bits, state, first_block, d_coef[:coef_count],
                             flags)
        h_flags = h_words[SYNC_ROUND * n:]
        h_flags.copy_(flags, non_blocking=True)
        stream.synchronize()
        self._clock("emit", t0)
        bad = (h_flags.numpy() != 0) | ~quiet
        for k in host:
            bad[k] = True
        return [int(k) for k in np.nonzero(bad)[0]]

    def coefficient_planes(self, blobs: Sequence[bytes]):
        """The device Huffman decoder alone, for inspection: files of the supported subset, as ONE chunk -> (per image the
        int16 tensor fdet_jpeg_entropy_decode would fill, [positions whose planes the host would still have to decode])."""
        n = len(blobs)
        probed = []
        for i, b in enumerate(blobs):
            rc, info, msg = hp.jpeg_info(b)
            if rc != 0:
                raise FdetError(f"image {i}: {msg} (code {rc})")
            probed.append((i, info))
        descs, spans, used, _ws = self._describe(probed, np.zeros(n, dtype=IMAGE_DTYPE))
        self.sync_passes, self.scan_bytes = 0, 0
        with torch.cuda.device(self.device):
            d_coef = torch.full((used,), 0x5555, dtype=torch.int16, device=self.device)
            pool = ThreadPoolExecutor(max_workers=max(1, min(self.workers, n)))
            try:
                todo = self.huffman_chunk(pool, blobs, [f"image {i}" for i in range(n)], probed, descs, used, d_coef)
            finally:
                pool.shutdown(wait=True)
                torch.cuda.current_stream(self.device).synchronize()
        return [d_coef[a:a + c] for a, c in spans], todo

    def _decode_chunks_device_huffman(self, pool, blobs, names, chunks, plans, data) -> None:
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        cap = max(p[2] for p in plans)
        ws_cap = max(p[3] for p in plans)
        d_coef = self._buf("d_coef", cap, torch.int16)
        workspace = self._buf("workspace", max(ws_cap, 8), torch.uint8)
        try:
            for chunk, (descs, spans, used, _ws) in zip(chunks, plans):
                todo = self.huffman_chunk(pool, blobs, names, chunk, descs, used, d_coef)
                if todo:                                     # the host path of huffman="host", image by image, into the same planes
                    need = max(spans[k][1] for k in todo)
                    for k in todo:
                        stream.synchronize()                 # the copy out of the staging buffer has finished
                        stage = self._buf("h_coef", need, torch.int16, pinned=True)
                        i = chunk[k][0]
                        start, count = spans[k]
                        rc, msg = hp.jpeg_entropy_decode(blobs[i], stage.data_ptr(), count)
                        if rc != 0:
                            raise FdetError(f"{names[i]}: {msg} (code {rc})")
                        d_coef[start:start + count].copy_(stage[:count], non_blocking=True)
                        self.huffman_fallbacks.append(i)
                t0 = time.perf_counter()
                h_descs = self._buf("h_descs", descs.nbytes, torch.uint8, pinned=True)
                h_descs.numpy()[:] = descs.view(np.uint8)
                d_descs = self._buf("d_descs", descs.nbytes, torch.uint8)
                d_descs.copy_(h_descs, non_blocking=True)
                hp.jpeg_reconstruct(d_coef[:used], d_descs, descs, workspace, data)
                self.chunks += 1
                if self.timings is not None:
                    stream.synchronize()
                    self._clock("reconstruct", t0)
        finally:
            stream.synchronize()                             # nothing of this call is in flight when its buffers go


class DeviceJpegEncoder:
    """encode / encode_to_files: the images of a DeviceImageBank -> baseline JPEG files equal to PIL's
    `Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=subsampling)` byte for byte (libjpeg-turbo at its defaults:
    standard Huffman tables, no restart markers, JFIF header only).  Two launches per chunk of images: the plan (coefficients
    and every block's exact bit length and offset; its per-image bit totals come back with one copy and one synchronise and
    size the scan buffer) and the emit.  A chunk's plan workspace stays within `chunk_bytes` (an image larger than that is a
    chunk of its own); the scans reach the host through one of two pinned staging buffers, each guarded by an event, so that
    the host assembles the files of one chunk while the device works on the next."""

    def __init__(self, device, quality: int = 75, subsampling: str = "4:2:0", chunk_bytes: int = 256 << 20):
        self.device = torch.device(device)
        self.quality = int(quality)
        if not 1 <= self.quality <= 100:
            raise ValueError(f"DeviceJpegEncoder: quality={quality} outside 1..100")
        if subsampling not in hp.JPEG_SUBSAMPLINGS:
            raise ValueError(f"DeviceJpegEncoder: subsampling must be one of {sorted(hp.JPEG_SUBSAMPLINGS)}, got {subsampling!r}")
        self.subsampling = subsampling
        self.sub = hp.JPEG_SUBSAMPLINGS[subsampling]
        self.chunk_bytes = max(1, int(chunk_bytes))
        self.chunks = 0                                      # plan / emit launch pairs of the last call
        self.scan_bytes = 0                                  # compressed bytes the last call copied to the host

    # -- geometry ------------------------------------------------------------------------------------------------------
    def _descs(self, bank: DeviceImageBank, idx: np.ndarray) -> np.ndarray:
        hs, vs = (1, 1) if self.sub == 0 else (2, 1) if self.sub == 1 else (2, 2)
        t = bank.table[idx]
        d = np.zeros(len(idx), dtype=hp.JPEG_ENC_DESC_DTYPE)
        d["bank_offset"], d["width"], d["height"] = t["offset"], t["w"], t["h"]
        d["mcus_x"] = (t["w"].astype(np.int64) + 8 * hs - 1) // (8 * hs)
        d["mcus_y"] = (t["h"].astype(np.int64) + 8 * vs - 1) // (8 * vs)
        nb = d["mcus_x"].astype(np.int64) * d["mcus_y"] * (hs * vs + 2)
        if nb.size and int(nb.max()) > hp.JPEG_ENC_MAX_BLOCKS:
            k = int(nb.argmax())
            raise FdetError(f"DeviceJpegEncoder: image {int(idx[k])} ({int(t['w'][k])}x{int(t['h'][k])}) has {int(nb[k])} blocks, "
                            f"more than the {hp.JPEG_ENC_MAX_BLOCKS} one image may have")
        d["n_blocks"] = nb
        return d

    def _chunks(self, descs: np.ndarray):
        """-> [(first, last)) ranges of `descs`, each within chunk_bytes of plan workspace and the launch's image limit."""
        out, first, fill = [], 0, 0
        for k in range(len(descs)):
            need = int(descs["n_blocks"][k]) * 136 + 4
            if k > first and (fill + need > self.chunk_bytes or k - first >= MAX_IMAGES_PER_LAUNCH):
                out.append((first, k))
                first, fill = k, 0
            fill += need
        if len(descs) > first:
            out.append((first, len(descs)))
        return out

    def _index(self, bank: DeviceImageBank, indices) -> np.ndarray:
        a, b = bank.device, self.device                      # "cuda" names the current device: equal to any "cuda:k" here
        if a.type != b.type or (a.index is not None and b.index is not None and a.index != b.index):
            raise FdetError(f"DeviceJpegEncoder: the bank lives on {bank.device}, the encoder on {self.device}")
        idx = np.arange(len(bank)) if indices is None else np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(bank)):
            raise IndexError(f"DeviceJpegEncoder: indices outside the bank of {len(bank)} images")
        return idx

    def _plan_chunk(self, bank: DeviceImageBank, descs: np.ndarray):
        """Phase 1 of one chunk (descs: its records, block_base filled here) -> (d_descs, workspace, totals uint32 (n,))."""
        dev = bank.device
        n = len(descs)
        nb = descs["n_blocks"].astype(np.int64)
        descs["block_base"] = np.cumsum(nb) - nb
        B = int(nb.sum())
        workspace = torch.empty(hp.jpeg_enc_ws_bytes(B, n), dtype=torch.uint8, device=dev)
        h = torch.from_numpy(descs.view(np.uint8)).pin_memory()
        d_descs = h.to(dev, non_blocking=True)
        hp.jpeg_enc_plan(bank.data, d_descs, descs, self.quality, self.sub, workspace)
        h_totals = torch.empty(n * 4, dtype=torch.uint8).pin_memory()
        h_totals.copy_(workspace[136 * B:136 * B + 4 * n], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()         # the one synchronise of a chunk: its totals size the scan buffer
        return d_descs, workspace, h_totals.numpy().view(np.uint32).copy()

    # -- public --------------------------------------------------------------------------------------------------------
    def plan_arrays(self, bank: DeviceImageBank, indices=None):
        """The plan phase alone, for inspection -> per image (coef int16 (n_blocks, 64) in zigzag order, blocks in scan
        order; bits uint32 (n_blocks,); start uint32 (n_blocks,); total bits)."""
        idx = self._index(bank, indices)
        descs = self._descs(bank, idx)
        out = []
        with torch.cuda.device(bank.device):
            for first, last in self._chunks(descs):
                part = descs[first:last].copy()
                _d, ws, totals = self._plan_chunk(bank, part)
                B = int(part["n_blocks"].sum())
                host = ws.cpu().numpy()
                coef = host[:128 * B].view(np.int16).reshape(B, 64)
                bits = host[128 * B:132 * B].view(np.uint32)
                start = host[132 * B:136 * B].view(np.uint32)
                for k in range(len(part)):
                    a, b = int(part["block_base"][k]), int(part["block_base"][k]) + int(part["n_blocks"][k])
                    out.append((coef[a:b].copy(), bits[a:b].copy(), start[a:b].copy(), int(totals[k])))
        return out

    def encode(self, bank: DeviceImageBank, indices=None) -> List[bytes]:
        """-> one complete JPEG file per image of `indices` (all of the bank when None), in that order."""
        idx = self._index(bank, indices)
        self.chunks, self.scan_bytes = 0, 0
        if idx.size == 0:
            return []
        dev = bank.device
        descs = self._descs(bank, idx)
        headers = {}
        out: List[bytes] = []

        def assemble(job):
            part, nbytes, staged, ev, _hold = job
            ev.synchronize()                                 # the scans of this chunk are in its staging buffer
            host = staged.numpy()
            for k in range(len(part)):
                w, h = int(part["width"][k]), int(part["height"][k])
                if (w, h) not in headers:
                    headers[(w, h)] = hp.jpeg_write_header(w, h, self.quality, self.sub)
                o = int(part["scan_offset"][k])
                out.append(headers[(w, h)] + host[o:o + int(nbytes[k])].tobytes().replace(b"\xff", b"\xff\x00") + b"\xff\xd9")

        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            stage = [None, None]                             # pinned staging, grown on demand
            pending = None                                   # the chunk whose files the host has still to assemble
            try:
                for c, (first, last) in enumerate(self._chunks(descs)):
                    part = descs[first:last].copy()
                    d_descs, workspace, totals = self._plan_chunk(bank, part)
                    limit = part["n_blocks"].astype(np.int64) * hp.JPEG_ENC_MAX_BLOCK_BITS
                    if (totals < 1).any() or (totals.astype(np.int64) > limit).any():
                        raise FdetError("DeviceJpegEncoder: the plan returned a bit total outside what its blocks can take")
                    nbytes = (totals.astype(np.int64) + 7) // 8
                    spans = (nbytes + 3) // 4 * 4            # every image's stream starts on a 4-byte boundary
                    part["scan_offset"] = np.cumsum(spans) - spans
                    size = int(spans.sum())
                    scan = torch.empty(size, dtype=torch.uint8, device=dev)
                    scan.zero_()                             # a memset on the stream: the emit ORs into shared words
                    h = torch.from_numpy(part.view(np.uint8)).pin_memory()
                    d_descs2 = h.to(dev, non_blocking=True)
                    hp.jpeg_enc_emit(d_descs2, part, totals, self.sub, workspace, scan)
                    s = c % 2
                    if stage[s] is None or stage[s].numel() < size:
                        stage[s] = torch.empty(size, dtype=torch.uint8).pin_memory()
                    stage[s][:size].copy_(scan, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    self.chunks += 1
                    self.scan_bytes += int(nbytes.sum())
                    if pending is not None:                  # assembled while the device emits and copies this chunk
                        assemble(pending)
                    pending = (part, nbytes, stage[s], ev, (h, d_descs, d_descs2))     # the descriptors live as long as the launch
                if pending is not None:
                    assemble(pending)
            finally:
                stream.synchronize()                         # nothing of this call is in flight when its buffers go
        return out

    def encode_to_files(self, bank: DeviceImageBank, paths: Sequence, threads: int = 16, indices=None) -> None:
        """encode(bank, indices), file i written to paths[i] on at most 16 threads.  Parent directories are created."""
        import os
        paths = [os.fspath(p) for p in paths]
        idx = self._index(bank, indices)
        if len(paths) != len(idx):
            raise ValueError(f"encode_to_files: {len(paths)} paths for {len(idx)} images")
        for d in sorted({os.path.dirname(p) for p in paths}):
            if d:
                os.makedirs(d, exist_ok=True)
        files = self.encode(bank, idx)

        def write(job):
            with open(job[1], "wb") as f:
                f.write(job[0])
        with ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, int(threads), len(paths) or 1))) as ex:
            list(ex.map(write, zip(files, paths)))
