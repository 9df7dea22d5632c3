"""Timings of cutting face chips on the device (csrc/fdet_chips.hip).

    python tools/chips_throughput.py [--images 256] [--size 112] [--launches 40] [--out profiles/r12_chips.json]

Input: the workload of tools/bench_render.py: `synthetic_bank` of --images images with sides in 700..1024 (about the pixels of
a 1024x700 photo) and its own annotations as the boxes, 0..16 per image (about 2011 in all).  Device events around single
calls into preallocated outputs, every variant warmed up, the variants alternated launch by launch in one process; median /
min / max over --launches:

  chip_extract          fdet_chip_extract, HWC chips of --size, margin 0.25
  chip_extract_planar   the same, planar chips
  best_update           fdet_chip_best_update on those chips (every image a frame of one sequence, the row index + 1 as the id)
  render_pixelate       context: fdet_render_boxes with pixelation (copy of the bank included) on the same boxes

and beside them the host path: the copy of the bank to the host (`to_arrays`), then PIL `crop().resize()` of every box on 16
threads, wall clock, median of --host-runs.  `extract_chips_ms` is the Python surface end to end (allocation, the read of
`counts`, the entry), host clock around a synchronise.  Prints one JSON line and, with --out, writes it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--margin", type=float, default=0.25)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from fdet_amd import hotpath as hp
    from fdet_amd._native import check, lib, ptr, stream
    from fdet_amd.chips import extract_chips, margin_to_256
    from fdet_amd.datasets import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("chips_throughput needs a GPU")
    bank, boxes = A.synthetic_bank(args.images, "cuda", seed=0, min_side=700, max_side=1024, max_faces=16)
    n, C, m256 = len(bank), args.size, margin_to_256(args.margin)
    K = max(max(len(b) for b in boxes), 1)
    rows = np.zeros((n, K, 5), np.float32)
    counts = np.array([len(b) for b in boxes], np.int32)
    for i, b in enumerate(boxes):
        rows[i, :len(b)] = b
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    h_off = np.zeros(n + 1, np.int32)
    h_off[1:] = np.cumsum(counts)
    d_off = torch.from_numpy(h_off).cuda()
    M = int(h_off[-1])
    U8, I32, I64 = torch.uint8, torch.int32, torch.int64
    chips = torch.empty(M, C, C, 3, dtype=U8, device="cuda")
    info = torch.empty(M * hp.CHIP_INFO_BYTES, dtype=U8, device="cuda")

    def extract(planar):
        check(lib().fdet_chip_extract(ptr(bank.data, U8), ptr(bank.d_table, U8), bank.table.ctypes.data, n, ptr(d_rows), ptr(d_counts, I32),
                                      counts.ctypes.data, ptr(d_off, I32), h_off.ctypes.data, K, C, m256, planar, ptr(chips, U8),
                                      ptr(info, U8), stream()), "fdet_chip_extract")

    # the gallery: one sequence, ids 1..K
    ids = torch.arange(1, K + 1, dtype=I32, device="cuda").repeat(n, 1).contiguous()
    seq = np.array([0, n], np.int32)
    d_seq, base = torch.from_numpy(seq).cuda(), torch.zeros(1, dtype=I32, device="cuda")
    gal = torch.zeros(K * hp.CHIP_BEST_BYTES, dtype=U8, device="cuda")
    gal_chips = torch.zeros(1, K, C * C * 3, dtype=U8, device="cuda")
    scratch, over = torch.zeros(K, dtype=I64, device="cuda"), torch.zeros(1, dtype=I64, device="cuda")

    def best():
        hp.chip_best_update(chips, info, ids, d_seq, seq, base, K, 0, 0, gal, gal_chips, scratch, over)

    # context: pixelation of the same boxes
    sizes = bank.table["h"].astype(np.int64) * bank.table["w"] * 3
    table = np.zeros(n, dtype=A.IMAGE_DTYPE)
    table["offset"][1:] = np.cumsum(sizes)[:-1]
    table["h"], table["w"] = bank.table["h"], bank.table["w"]
    dst = A.DeviceImageBank(torch.empty(int(sizes.sum()), dtype=U8, device="cuda"), table)
    ws = torch.empty(n + 1, dtype=I32, device="cuda")

    def pixelate():
        check(lib().fdet_render_boxes(ptr(bank.data, U8), ptr(bank.d_table, U8), bank.table.ctypes.data, ptr(d_rows), ptr(d_counts, I32),
                                      counts.ctypes.data, n, K, ptr(dst.data, U8), ptr(dst.d_table, U8), dst.table.ctypes.data, 0, 1, 8,
                                      0, 0, 255, ptr(ws, I32), stream()), "fdet_render_boxes")

    variants = {"chip_extract": lambda: extract(0), "chip_extract_planar": lambda: extract(1), "best_update": best,
                "render_pixelate": pixelate}
    extract(0)
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    extract(0)                                               # best_update reads HWC chips (either layout costs the same)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.launches):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))

    def stats(v):
        a = np.sort(np.asarray(v))
        return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4)}

    rec = info.cpu().numpy().view(np.dtype([("i", "<i4", (8,)), ("sharp", "<i8")]))
    S = rec["i"][:, 4][rec["i"][:, 6] == 1]
    res = {"tool": "chips_throughput", "device_name": torch.cuda.get_device_name(0), "images": n, "boxes": M, "size": C,
           "margin256": m256, "launches": args.launches, "bank_MiB": round(float(sizes.sum()) / 2 ** 20, 1),
           "valid_chips": int(len(S)), "window_side": {"min": int(S.min()), "median": float(np.median(S)), "max": int(S.max())},
           "window_pixels_MiB": round(float((S.astype(np.int64) ** 2).sum()) * 3 / 2 ** 20, 1),
           "chips_MiB": round(M * C * C * 3 / 2 ** 20, 1), "device": {k: stats(v) for k, v in ms.items()}}
    wall = []
    for _ in range(args.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cs = extract_chips(bank, d_rows, d_counts, size=C, margin=args.margin)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        del cs
    res["extract_chips_ms"] = stats(wall)

    # the host path: copy of the bank, then PIL crop + resize on 16 threads (the window of rule 2; PIL pads with black
    # where the window leaves the image, so the bytes are not the device's: this is a timing only)
    def host_chips(j, imgs):
        im = Image.fromarray(imgs[j])
        out = []
        for _, x, y, w, h in boxes[j].tolist():
            side = max(w, h)
            s = side * (1 + 2 * args.margin)
            cx, cy = x + w / 2, y + h / 2
            out.append(np.asarray(im.crop((int(cx - s / 2), int(cy - s / 2), int(cx + s / 2), int(cy + s / 2))).resize((C, C), Image.BILINEAR)))
        return out

    copy_ms, host_ms = [], []
    for _ in range(args.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imgs = bank.to_arrays()
        t1 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:
            outs = list(ex.map(lambda j: host_chips(j, imgs), range(n)))
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        host_ms.append((t2 - t0) * 1e3)
        del outs, imgs
    res["host_16_threads"] = {"bank_copy": stats(copy_ms), "copy_crop_resize": stats(host_ms)}
    res["host_over_device"] = round(res["host_16_threads"]["copy_crop_resize"]["median_ms"] / res["device"]["chip_extract"]["median_ms"], 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
