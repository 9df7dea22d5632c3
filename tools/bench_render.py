"""Timings of rendering detections into a second bank (csrc/fdet_render.hip).

    python tools/bench_render.py [--images 256] [--repeats 5] [--out profiles/r08_render.json]

Input: `synthetic_bank` of --images images with sides in 700..1024 (about the pixels of a 1024x700 photo) and its own
annotations as the boxes, 0..16 per image (about 8).  Timed with device events around `--inner` back-to-back calls of
fdet_render_boxes into a preallocated destination, every variant warmed up, the variants alternated repeat by repeat in one
process; median / min / max over --repeats:

  copy              the device-to-device copy of the bank alone (hipMemcpyAsync through torch's copy_)
  outline           copy + outlines
  pixelate          copy + pixelation
  outline_pixelate  copy + pixelation + outlines
  empty             the entry with every count zero: the copy as the entry issues it
  blur              copy + Gaussian blur (fdet_render_boxes_blur; radius = longer side / --blocks), into a
                    preallocated workspace

and beside them the host path on the same boxes: PIL's ImageDraw for the outlines plus a numpy block-mean pixelation, on 16
threads over host copies of the images (the transfers to and from the device, which the host path would also need, are not
counted), and for the blur PIL's crop, GaussianBlur and paste per box.  `render_detections_ms` is the Python surface end to end (allocation of the new bank, the read of `counts`,
the entry), by the host clock around a synchronise.  Prints one JSON line and, with --out, writes it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_render(img, boxes, blocks, pixelate):
    """The host baseline for one image: numpy block means (rule 3 without the priority rule: later boxes overwrite), then
    PIL outlines.  boxes: (k,5) [score,x,y,w,h]."""
    import numpy as np
    from PIL import Image, ImageDraw
    out = img.copy()
    H, W = img.shape[:2]
    if pixelate:
        for _, x, y, w, h in boxes.tolist():
            x0, y0, x1, y1 = int(x), int(y), int(x + w), int(y + h)
            cell = max(1, -(-max(x1 - x0 + 1, y1 - y0 + 1) // blocks))
            for ya in range(max(y0, 0), min(y1, H - 1) + 1, cell):
                for xa in range(max(x0, 0), min(x1, W - 1) + 1, cell):
                    yb, xb = min(ya + cell, y1 + 1, H), min(xa + cell, x1 + 1, W)
                    blk = img[ya:yb, xa:xb].reshape(-1, 3)
                    out[ya:yb, xa:xb] = ((blk.sum(0, dtype=np.int64) + len(blk) // 2) // len(blk)).astype(np.uint8)
    im = Image.fromarray(out)
    d = ImageDraw.Draw(im)
    for _, x, y, w, h in boxes.tolist():
        d.rectangle((x, y, x + w, y + h), outline=(0, 0, 255), width=1 if (w <= 15 or h <= 15) else 3)
    return np.asarray(im)


def host_blur(img, boxes, blocks):
    """The host baseline of the blur for one image: PIL crop, GaussianBlur, paste per box (later boxes over earlier ones)."""
    import numpy as np
    from PIL import Image, ImageFilter
    im = Image.fromarray(img)
    out = im.copy()
    W, H = im.size
    for _, x, y, w, h in boxes.tolist():
        x0, y0, x1, y1 = int(x), int(y), int(x + w), int(y + h)
        box = (max(x0, 0), max(y0, 0), min(x1, W - 1) + 1, min(y1, H - 1) + 1)
        if box[0] >= box[2] or box[1] >= box[3]:
            continue
        out.paste(im.crop(box).filter(ImageFilter.GaussianBlur(max(x1 - x0 + 1, y1 - y0 + 1) / blocks)), box[:2])
    return np.asarray(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls between one pair of events")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from concurrent.futures import ThreadPoolExecutor
    from fdet_amd._native import check, lib, ptr, stream
    from fdet_amd.datasets import augment as A
    from fdet_amd import hotpath
    from fdet_amd.render import blur_table, render_detections
    if not torch.cuda.is_available():
        raise SystemExit("bench_render needs a GPU")
    bank, boxes = A.synthetic_bank(args.images, "cuda", seed=0, min_side=700, max_side=1024, max_faces=16)
    n = len(bank)
    K = max(max(len(b) for b in boxes), 1)
    rows = np.zeros((n, K, 5), np.float32)
    counts = np.array([len(b) for b in boxes], np.int32)
    for i, b in enumerate(boxes):
        rows[i, :len(b)] = b
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    zeros = np.zeros(n, np.int32)
    d_zeros = torch.from_numpy(zeros).cuda()
    sizes = bank.table["h"].astype(np.int64) * bank.table["w"] * 3
    table = np.zeros(n, dtype=A.IMAGE_DTYPE)
    table["offset"][1:] = np.cumsum(sizes)[:-1]
    table["h"], table["w"] = bank.table["h"], bank.table["w"]
    dst = A.DeviceImageBank(torch.empty(int(sizes.sum()), dtype=torch.uint8, device="cuda"), table)
    ws = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    U8, I32 = torch.uint8, torch.int32
    first = int(bank.table["offset"][0])

    def entry(outline, pixelate, d_cnt=d_counts, h_cnt=counts):
        check(lib().fdet_render_boxes(ptr(bank.data, U8), ptr(bank.d_table, U8), bank.table.ctypes.data, ptr(d_rows), ptr(d_cnt, I32),
                                      h_cnt.ctypes.data, n, K, ptr(dst.data, U8), ptr(dst.d_table, U8), dst.table.ctypes.data, outline,
                                      pixelate, args.blocks, 0, 0, 255, ptr(ws, I32), stream()), "fdet_render_boxes")

    d_tab, h_tab = blur_table(args.blocks, None, 2 * int(max(bank.table["h"].max(), bank.table["w"].max())) + 2, "cuda")
    blur_ws = torch.empty(hotpath.render_blur_ws_bytes(bank.table, rows, counts), dtype=U8, device="cuda")
    rejected = torch.zeros(1, dtype=torch.int64, device="cuda")

    def blur():
        hotpath.render_boxes_blur(bank, d_rows, d_counts, counts, dst, d_tab, h_tab, blocks=args.blocks, ws=blur_ws, rejected=rejected)

    variants = {
        "copy": lambda: dst.data.copy_(bank.data[first:first + dst.data.numel()]),
        "outline": lambda: entry(1, 0),
        "pixelate": lambda: entry(0, 1),
        "outline_pixelate": lambda: entry(1, 1),
        "empty": lambda: entry(1, 1, d_zeros, zeros),
        "blur": blur,
    }
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(args.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.inner)

    def stats(v):
        a = np.sort(np.asarray(v))
        return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4)}

    res = {"tool": "bench_render", "device_name": torch.cuda.get_device_name(0), "images": n, "boxes": int(counts.sum()),
           "bank_MiB": round(float(sizes.sum()) / 2 ** 20, 1), "blocks": args.blocks, "repeats": args.repeats, "inner": args.inner,
           "box_pixels_MiB": round(sum(float(((b[:, 3] + 1) * (b[:, 4] + 1)).sum()) for b in boxes) * 3 / 2 ** 20, 1),
           "device": {k: stats(v) for k, v in ms.items()}}
    med = {k: res["device"][k]["median_ms"] for k in variants}
    res["copy_GBps_read_plus_write"] = round(2 * float(sizes.sum()) / (med["copy"] * 1e-3) / 1e9, 1)
    res["ratio_to_copy"] = {k: round(med[k] / med["copy"], 3) for k in ("outline", "pixelate", "outline_pixelate", "empty", "blur")}
    if int(rejected.item()):
        raise SystemExit("bench_render: the blur rejected boxes")
    res["blur_ws_MiB"] = round(blur_ws.numel() / 2 ** 20, 1)
    res["blur_minus_copy_over_pixelate_minus_copy"] = round((med["blur"] - med["copy"]) / max(med["pixelate"] - med["copy"], 1e-6), 1)
    # the Python surface, host clock
    wall = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = render_detections(bank, d_rows, d_counts, anonymize="pixelate", blocks=args.blocks)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        del out
    res["render_detections_ms"] = stats(wall)
    wall = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = render_detections(bank, d_rows, d_counts, outline=False, anonymize="blur", blocks=args.blocks)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        del out
    res["render_detections_blur_ms"] = stats(wall)
    # the host path on the same boxes, 16 threads
    imgs = bank.to_arrays()
    host = {}
    for name, pix in (("outline", False), ("outline_pixelate", True)):
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=16) as ex:
                outs = list(ex.map(lambda j: host_render(imgs[j], boxes[j], args.blocks, pix), range(n)))
            t.append((time.perf_counter() - t0) * 1e3)
        host[name] = stats(t)
        del outs
    t = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:
            outs = list(ex.map(lambda j: host_blur(imgs[j], boxes[j], args.blocks), range(n)))
        t.append((time.perf_counter() - t0) * 1e3)
    host["blur"] = stats(t)
    del outs
    res["host_16_threads"] = host
    res["host_over_device"] = {k: round(host[k]["median_ms"] / med[k], 1) for k in host}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
