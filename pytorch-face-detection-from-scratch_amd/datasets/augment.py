"""On-device WIDER-Face training augmentation.

The reference trains on `WIDERFaceDataModule.training_transform()` (datasets/WIDERFace/datamodule.py:105-124), an
albumentations pipeline run per image on the CPU in DataLoader workers, and validates on `default_transform()` (:126-134,
Resize alone).  Here the decoded images stay resident on the device (`DeviceImageBank`), the per-image random parameters
are drawn on the host (`DeviceTransform.sample`, replayable from `(seed, step)`), and three HIP kernels
(csrc/fdet_augment.hip) produce the batch: the composed warp + photometric ops, GlassBlur + MotionBlur with the /255
normalisation, and the box transform + min-area filter + rounding compacted into the layout the target encoders take.

    bank = DeviceImageBank.from_arrays(images_hwc_u8, "cuda")
    batches = DeviceBatches(bank, boxes, 64, training_transform((480, 480), seed=0), num_of_patches=10)
    fit(model_meta, batches, epochs=70)           # x and y are device fp32: fit() takes its "direct" path

Semantics, rounding, the RNG and where this departs from albumentations: DESIGN.md "On-device augmentation".
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import hotpath as hp
from .._native import check, lib, ptr, stream

IMAGE_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")], align=True)         # fdet_aug_image
PARAMS_DTYPE = np.dtype([("image", "<i4"), ("flags", "<i4"), ("crop_x0", "<i4"), ("crop_y0", "<i4"), ("crop_w", "<i4"),
                         ("crop_h", "<i4"), ("angle", "<f4"), ("cos_a", "<f4"), ("sin_a", "<f4"), ("alpha", "<f4"),
                         ("beta", "<f4"), ("sigma", "<f4"), ("key", "<u4"), ("motion_k", "<i4"), ("motion_w", "<f4", (49,)),
                         ("reserved", "<i4")], align=True)                                # fdet_aug_params
assert IMAGE_DTYPE.itemsize == 16 and PARAMS_DTYPE.itemsize == 256

FLIP, ROTATE, BRIGHTNESS, NOISE, GLASS, MOTION, CROP, CROP_FALLBACK = 1, 2, 4, 8, 16, 32, 64, 128


def bresenham(k: int, xs: int, ys: int, xe: int, ye: int) -> np.ndarray:
    """k x k uint8 kernel with the 8-connected line (xs,ys)-(xe,ye) drawn with ones (cv2.line, thickness 1)."""
    ker = np.zeros((k, k), dtype=np.uint8)
    dx, dy = abs(xe - xs), -abs(ye - ys)
    sx, sy = (1 if xs < xe else -1), (1 if ys < ye else -1)
    err, x, y = dx + dy, xs, ys
    while True:
        ker[y, x] = 1
        if x == xe and y == ye:
            return ker
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy


def image_keys(indices, step: int) -> np.ndarray:
    """Per-image key of the pixel hash: a function of (dataset index, step), not of the position in the batch."""
    idx = np.asarray(indices, dtype=np.uint64)
    return ((idx * np.uint64(0x9E3779B1)) ^ (np.uint64(step & 0xFFFFFFFF) * np.uint64(0x85EBCA77))).astype(np.uint64) & np.uint64(0xFFFFFFFF)


class DeviceImageBank:
    """Ragged HWC uint8 RGB images packed into one device byte buffer, with a {offset (64-bit), h, w} table."""

    def __init__(self, data: torch.Tensor, table: np.ndarray):
        self.data = data
        self.table = np.ascontiguousarray(table, dtype=IMAGE_DTYPE)
        self.device = data.device
        self.d_table = torch.from_numpy(self.table.view(np.uint8).copy()).to(self.device)

    @classmethod
    def from_arrays(cls, images: Sequence[np.ndarray], device, lead_bytes: int = 0,
                    chunk_bytes: int = 256 << 20) -> "DeviceImageBank":
        """Pack `images` (each (H,W,3) uint8, as np.array(PIL.Image) gives) into one device buffer.  The host copy goes through
        one pinned staging buffer per chunk.  `lead_bytes` leaves that many (zeroed) bytes before the first image."""
        device = torch.device(device)
        table = np.zeros(len(images), dtype=IMAGE_DTYPE)
        off = int(lead_bytes)
        for i, im in enumerate(images):
            a = np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"image {i}: expected (H,W,3) uint8, got {a.shape} {a.dtype}")
            table[i] = (off, a.shape[0], a.shape[1])
            off += a.size
        data = torch.empty(max(off, 1), dtype=torch.uint8, device=device)
        if lead_bytes:
            data[:lead_bytes].zero_()
        stage = torch.empty(min(max(off - lead_bytes, 1), chunk_bytes), dtype=torch.uint8).pin_memory()
        sn = stage.numpy()
        i, n = 0, len(images)
        while i < n:
            start, fill = int(table[i]["offset"]), 0
            while i < n and (fill == 0 or fill + images[i].size <= stage.numel()):
                a = np.ascontiguousarray(images[i]).reshape(-1)
                if a.size > stage.numel():                      # an image larger than the staging buffer: straight copy
                    data[start:start + a.size].copy_(torch.from_numpy(a))
                    i += 1
                    start += a.size
                    continue
                sn[fill:fill + a.size] = a
                fill += a.size
                i += 1
            if fill:
                data[start:start + fill].copy_(stage[:fill], non_blocking=True)
                torch.cuda.current_stream(device).synchronize()  # the staging buffer is refilled next
        return cls(data, table)

    def to_arrays(self, indices=None, chunk_bytes: int = 256 << 20) -> List[np.ndarray]:
        """The inverse of `from_arrays`: the images `indices` (all when None) as (H,W,3) uint8 arrays of their own, through
        one pinned staging buffer per chunk (images that follow each other in the bank share a copy)."""
        idx = np.arange(len(self)) if indices is None else np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"to_arrays: indices outside the bank of {len(self)} images")
        t = self.table[idx]
        sizes = t["h"].astype(np.int64) * t["w"] * 3
        if idx.size == 0:
            return []
        stage = torch.empty(int(min(max(int(sizes.sum()), 1), max(int(chunk_bytes), int(sizes.max())))), dtype=torch.uint8).pin_memory()
        sn = stage.numpy()
        out: List[np.ndarray] = []
        i, n = 0, len(idx)
        while i < n:
            first, fill = i, 0
            while i < n and fill + int(sizes[i]) <= stage.numel():
                run_off, run_fill, run_bytes = int(t["offset"][i]), fill, 0
                while (i < n and fill + int(sizes[i]) <= stage.numel()
                       and int(t["offset"][i]) == run_off + run_bytes):           # the run goes on in the bank
                    run_bytes += int(sizes[i])
                    fill += int(sizes[i])
                    i += 1
                stage[run_fill:run_fill + run_bytes].copy_(self.data[run_off:run_off + run_bytes], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()                 # the staging buffer is refilled next
            pos = 0
            for k in range(first, i):
                out.append(sn[pos:pos + int(sizes[k])].reshape(int(t["h"][k]), int(t["w"][k]), 3).copy())
                pos += int(sizes[k])
        return out

    def __len__(self) -> int:
        return len(self.table)

    @property
    def sizes(self) -> np.ndarray:
        """(N,2) int array of (H, W)."""
        return np.stack([self.table["h"], self.table["w"]], 1).astype(np.int64)

    @property
    def nbytes(self) -> int:
        return int((self.table["h"].astype(np.int64) * self.table["w"] * 3).sum())

    def subset(self, indices) -> "DeviceImageBank":
        """A bank over the same device buffer holding only `indices` (renumbered 0..len-1)."""
        return DeviceImageBank(self.data, self.table[np.asarray(indices, dtype=np.int64)])


class DeviceBoxes:
    """Per-image (n_i,5) [conf,x,y,w,h] source-pixel boxes of a bank, flat on the device: rows [total,5], offsets [N+1]."""

    def __init__(self, boxes: Sequence, device):
        device = torch.device(device)
        mats = [np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float32).reshape(-1, 5) for b in boxes]
        counts = np.array([m.shape[0] for m in mats], dtype=np.int64)
        offs = np.zeros(len(mats) + 1, dtype=np.int32)
        offs[1:] = np.cumsum(counts)
        flat = np.concatenate(mats, 0) if counts.sum() else np.zeros((1, 5), np.float32)
        self.rows = torch.from_numpy(np.ascontiguousarray(flat)).to(device)
        self.offset = torch.from_numpy(offs).to(device)
        self.max_per_image = int(counts.max()) if len(counts) else 0
        self.n = len(mats)


class GtBoxes:
    """Device-side view of a batch's boxes (the `gt_bbx` list of my_collate, datamodule.py:162-167): rows [cap,5] and
    box_offset [B+1] stay on the device; the per-image (n,5) tensors are split off only when indexed (one host sync)."""

    def __init__(self, rows: torch.Tensor, box_offset: torch.Tensor):
        self.rows, self.box_offset = rows, box_offset
        self._offs: Optional[List[int]] = None

    @property
    def materialized(self) -> bool:
        return self._offs is not None

    def __len__(self) -> int:
        return self.box_offset.numel() - 1

    def __getitem__(self, i: int) -> torch.Tensor:
        if self._offs is None:
            self._offs = self.box_offset.cpu().tolist()
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self.rows[self._offs[i]:self._offs[i + 1]]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class DeviceTransform:
    """The albumentations Compose of the datamodule as probabilities and ranges; `sample` draws the per-image parameters on
    the host, calling the object runs the kernels."""

    def __init__(self, input_shape, seed: int = 0, p_crop=0.0, crop_scale=(0.08, 1.0), crop_ratio=(3 / 4, 4 / 3),
                 p_flip=0.0, p_brightness=0.0, brightness=0.2, contrast=0.2, p_rotate=0.0, rotate_limit=20.0,
                 p_noise=0.0, var_limit=(0.0, 400.0), p_glass=0.0, p_motion=0.0, motion_sizes=(3, 5, 7)):
        shp = tuple(int(s) for s in input_shape)
        self.out_hw = shp[1:3] if len(shp) == 3 and shp[0] == 3 else shp[:2]
        self.seed = int(seed) & 0xFFFFFFFF
        self.p_crop, self.crop_scale, self.crop_ratio = p_crop, crop_scale, crop_ratio
        self.p_flip, self.p_brightness, self.brightness, self.contrast = p_flip, p_brightness, brightness, contrast
        self.p_rotate, self.rotate_limit = p_rotate, rotate_limit
        self.p_noise, self.var_limit = p_noise, var_limit
        self.p_glass, self.p_motion, self.motion_sizes = p_glass, p_motion, tuple(motion_sizes)

    def sample(self, sizes, step: int) -> np.ndarray:
        """Parameters of a batch whose images have `sizes` (B,2) = (H, W), drawn from Generator(PCG64([seed, step])).
        Every draw is taken whether its op fires or not, so the stream is a function of (seed, step, B) alone."""
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        B = len(sizes)
        H, W = sizes[:, 0], sizes[:, 1]
        g = np.random.Generator(np.random.PCG64([self.seed, int(step)]))
        P = np.zeros(B, dtype=PARAMS_DTYPE)
        flags = np.zeros(B, dtype=np.int64)
        # RandomResizedCrop (torchvision / albumentations rule): 10 attempts, then a ratio-clamped centre crop
        on = g.random(B) < self.p_crop
        area = (H * W).astype(np.float64)[:, None]
        lr = (math.log(self.crop_ratio[0]), math.log(self.crop_ratio[1]))
        ta = g.uniform(self.crop_scale[0], self.crop_scale[1], (B, 10)) * area
        ar = np.exp(g.uniform(lr[0], lr[1], (B, 10)))
        cw = np.rint(np.sqrt(ta * ar)).astype(np.int64)
        ch = np.rint(np.sqrt(ta / ar)).astype(np.int64)
        ok = (cw > 0) & (cw <= W[:, None]) & (ch > 0) & (ch <= H[:, None])
        first = ok.argmax(1)
        r = np.arange(B)
        aw, ah = cw[r, first], ch[r, first]
        ui, uj = g.random(B), g.random(B)
        ai = np.floor(ui * (H - ah + 1)).astype(np.int64)
        aj = np.floor(uj * (W - aw + 1)).astype(np.int64)
        in_ratio = W / H
        fw = np.where(in_ratio < min(self.crop_ratio), W,
                      np.where(in_ratio > max(self.crop_ratio), np.rint(H * max(self.crop_ratio)), W)).astype(np.int64)
        fh = np.where(in_ratio < min(self.crop_ratio), np.rint(W / min(self.crop_ratio)),
                      H).astype(np.int64)
        fw, fh = np.clip(fw, 1, W), np.clip(fh, 1, H)
        hit = ok.any(1)
        cw_ = np.where(hit, aw, fw)
        ch_ = np.where(hit, ah, fh)
        x0 = np.where(hit, np.minimum(aj, W - aw), (W - fw) // 2)
        y0 = np.where(hit, np.minimum(ai, H - ah), (H - fh) // 2)
        P["crop_x0"] = np.where(on, x0, 0)
        P["crop_y0"] = np.where(on, y0, 0)
        P["crop_w"] = np.where(on, cw_, W)
        P["crop_h"] = np.where(on, ch_, H)
        flags |= np.where(on, CROP, 0) | np.where(on & ~hit, CROP_FALLBACK, 0)
        flags |= np.where(g.random(B) < self.p_flip, FLIP, 0)
        # RandomBrightnessContrast(brightness_by_max=True): v*alpha + 255*beta
        bc = g.random(B) < self.p_brightness
        alpha = 1.0 + g.uniform(-self.contrast, self.contrast, B)
        beta = 255.0 * g.uniform(-self.brightness, self.brightness, B)
        flags |= np.where(bc, BRIGHTNESS, 0)
        P["alpha"] = np.where(bc, alpha, 1.0)
        P["beta"] = np.where(bc, beta, 0.0)
        rot = g.random(B) < self.p_rotate
        ang = g.uniform(-self.rotate_limit, self.rotate_limit, B)
        flags |= np.where(rot, ROTATE, 0)
        ang = np.where(rot, ang, 0.0)
        P["angle"] = ang
        P["cos_a"] = np.cos(np.deg2rad(ang))
        P["sin_a"] = np.sin(np.deg2rad(ang))
        noise = g.random(B) < self.p_noise
        var = g.uniform(self.var_limit[0], self.var_limit[1], B)
        flags |= np.where(noise, NOISE, 0)
        P["sigma"] = np.where(noise, np.sqrt(var), 0.0)
        flags |= np.where(g.random(B) < self.p_glass, GLASS, 0)
        # MotionBlur: k from motion_sizes, a line between two random kernel points, normalised by its sum
        mot = g.random(B) < self.p_motion
        ks = np.asarray(self.motion_sizes, dtype=np.int64)[g.integers(0, len(self.motion_sizes), B)]
        u4 = g.random((B, 4))
        P["motion_k"] = 1
        for b in np.nonzero(mot)[0]:
            k = int(ks[b])
            xs, xe = int(u4[b, 0] * k), int(u4[b, 1] * k)
            ys = int(u4[b, 2] * k)
            if xs == xe:                                   # two distinct rows
                ye = (ys + 1 + int(u4[b, 3] * (k - 1))) % k
            else:
                ye = int(u4[b, 3] * k)
            ker = bresenham(k, xs, ys, xe, ye).astype(np.float32)
            ker = ker / np.float32(ker.sum())
            P["motion_k"][b] = k
            P["motion_w"][b, :k * k] = ker.reshape(-1)
        flags |= np.where(mot, MOTION, 0)
        P["flags"] = flags
        return P

    def params_for(self, bank: DeviceImageBank, indices, step: int) -> np.ndarray:
        idx = np.asarray(indices, dtype=np.int64)
        P = self.sample(bank.sizes[idx], step)
        P["image"] = idx
        P["key"] = image_keys(idx, step)
        return P

    def __call__(self, bank: DeviceImageBank, indices, boxes, step: int, params: Optional[np.ndarray] = None):
        """-> (x (B,3,Ho,Wo) fp32 in [0,1], frames (B,3,Ho,Wo) uint8, rows [cap,5] fp32, box_offset [B+1] int32), all on
        the bank's device; rows box_offset[n]..box_offset[n+1]-1 are image n's [1,x,y,w,h] boxes.  `boxes`: DeviceBoxes or a
        list of per-image (n,5) arrays for every image of the bank.  `params` overrides the sampled parameters."""
        dev = bank.device
        if not isinstance(boxes, DeviceBoxes):
            boxes = DeviceBoxes(boxes, dev)
        if boxes.n != len(bank):
            raise ValueError(f"boxes cover {boxes.n} images, the bank holds {len(bank)}")
        P = self.params_for(bank, indices, step) if params is None else np.ascontiguousarray(params, dtype=PARAMS_DTYPE)
        B = len(P)
        if B == 0:
            raise ValueError("empty batch")
        Ho, Wo = self.out_hw
        d_params = torch.from_numpy(P.view(np.uint8)).pin_memory().to(dev, non_blocking=True)
        mid = torch.empty(B, 3, Ho, Wo, dtype=torch.uint8, device=dev)
        frames = torch.empty_like(mid)
        x = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=dev)
        cap = B * boxes.max_per_image
        rows = torch.empty(max(cap, 1), 5, dtype=torch.float32, device=dev)
        box_offset = torch.empty(B + 1, dtype=torch.int32, device=dev)
        L, U8, I32 = lib(), torch.uint8, torch.int32
        hp_ = P.ctypes.data
        ht = bank.table.ctypes.data
        check(L.fdet_aug_warp(ptr(bank.data, U8), ptr(bank.d_table, U8), ht, len(bank), ptr(d_params, U8), hp_, B, Ho, Wo,
                              self.seed, ptr(mid, U8), stream()), "fdet_aug_warp")
        check(L.fdet_aug_finish(ptr(mid, U8), ptr(d_params, U8), hp_, B, Ho, Wo, self.seed, ptr(frames, U8), ptr(x), stream()),
              "fdet_aug_finish")
        check(L.fdet_aug_boxes(ptr(boxes.rows), ptr(boxes.offset, I32), ptr(bank.d_table, U8), ht, len(bank),
                               ptr(d_params, U8), hp_, B, Ho, Wo, cap, ptr(rows), ptr(box_offset, I32), stream()),
              "fdet_aug_boxes")
        return x, frames, rows, box_offset


def training_transform(input_shape, seed: int = 0) -> DeviceTransform:
    """WIDERFaceDataModule.training_transform() (datamodule.py:105-124)."""
    return DeviceTransform(input_shape, seed, p_crop=0.2, p_flip=0.5, p_brightness=0.2, p_rotate=0.2, p_noise=0.2,
                           p_glass=0.2, p_motion=0.2)


def default_transform(input_shape, seed: int = 0) -> DeviceTransform:
    """WIDERFaceDataModule.default_transform() (datamodule.py:126-134): Resize alone."""
    return DeviceTransform(input_shape, seed)


def synthetic_bank(n: int, device, seed: int = 0, min_side: int = 300, max_side: int = 1024, max_faces: int = 2):
    """A bank of `n` seeded synthetic images of WIDER-like ragged sizes (smooth random colour fields with a few flat
    rectangles) and their annotations, `synthetic_boxes`-style rows [1,x,y,w,h] (integer w,h in 8..200 clipped to the image,
    0..max_faces per image).  -> (DeviceImageBank, list of (n_i,5) float32 arrays)."""
    g = np.random.default_rng(seed)
    images, boxes = [], []
    for _ in range(n):
        H, W = int(g.integers(min_side, max_side + 1)), int(g.integers(min_side, max_side + 1))
        base = g.integers(0, 256, (H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
        img = np.repeat(np.repeat(base, 16, 0), 16, 1)[:H, :W]
        rows = []
        for _k in range(int(g.integers(0, max_faces + 1))):
            w, h = min(int(g.integers(8, 201)), W), min(int(g.integers(8, 201)), H)
            x, y = int(g.integers(0, W - w + 1)), int(g.integers(0, H - h + 1))
            img[y:y + h, x:x + w] = g.integers(0, 256, 3)
            rows.append([1.0, x, y, w, h])
        images.append(np.ascontiguousarray(img.astype(np.uint8)))
        boxes.append(np.asarray(rows, dtype=np.float32).reshape(-1, 5))
    return DeviceImageBank.from_arrays(images, device), boxes


class DeviceBatches:
    """Re-iterable batches `[x (B,3,H,W) fp32, y targets, gt_bbx]` (the my_collate contract, datamodule.py:162-167) from a
    device image bank, reshuffled every epoch.  `encoder="yolo"`: y = (B,5,S,S) with S = num_of_patches; `"ssd"`:
    y = (B,P,5) with num_of_patches the per-scale patch list.  Producing a batch never synchronises the host."""

    def __init__(self, bank: DeviceImageBank, boxes, batch_size: int, transform: DeviceTransform, num_of_patches,
                 encoder: str = "yolo", shuffle: bool = True, seed: int = 0, drop_last: bool = True):
        if encoder not in ("yolo", "ssd"):
            raise ValueError(f"encoder must be 'yolo' or 'ssd', got {encoder!r}")
        self.bank = bank
        self.boxes = boxes if isinstance(boxes, DeviceBoxes) else DeviceBoxes(boxes, bank.device)
        if self.boxes.n != len(bank):
            raise ValueError(f"boxes cover {self.boxes.n} images, the bank holds {len(bank)}")
        self.batch_size, self.transform, self.encoder = int(batch_size), transform, encoder
        self.num_of_patches = num_of_patches
        self.shuffle, self.seed, self.drop_last = shuffle, int(seed), drop_last
        self.epoch = 0

    def __len__(self) -> int:
        n = len(self.bank)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        n = len(self.bank)
        order = (np.random.Generator(np.random.PCG64([self.seed, epoch])).permutation(n) if self.shuffle
                 else np.arange(n))
        nb = len(self)
        Ho, Wo = self.transform.out_hw
        for i in range(nb):
            idx = order[i * self.batch_size:(i + 1) * self.batch_size]
            x, _, rows, offs = self.transform(self.bank, idx, self.boxes, epoch * nb + i)
            if self.encoder == "yolo":
                y = hp.encode_targets_device(rows, offs, (Wo, Ho), int(self.num_of_patches))
            else:
                y = hp.ssd_encode_targets_device(rows, offs, (Wo, Ho), self.num_of_patches)
            yield [x, y, GtBoxes(rows, offs)]
