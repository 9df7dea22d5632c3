"""What the device JPEG encoder (csrc/fdet_jpeg_enc.hip, fdet_amd/datasets/jpeg.py DeviceJpegEncoder) buys over PIL, measured.

    python tools/jpeg_encode_throughput.py [--images 256] [--repeats 7] [--out profiles/r16_jpeg_encode.json]

Input: the workload of tools/bench_render.py, `synthetic_bank` of --images images with sides in 700..1024 (about the pixels
of a 1024x700 photo); quality 75, 4:2:0.  Timed, every path warmed up once, the paths alternated sample by sample, median and
5th..95th percentile over --repeats:

  to_bytes     the files in memory: PIL on 16 threads after `bank.to_arrays()` (the copy of the pixels included: what
               `save_images` does before it writes) against `DeviceJpegEncoder.encode`
  to_files     `save_images(bank, paths)` as it always was against `save_images(..., encoder="device")`, into a temporary directory
  stages       of the device path on their own: the plan kernels (k_enc_fdct + k_enc_bits + k_enc_scan together), the emit kernel
               with the memset of its scan buffer, the device-to-host copy of the scans (device events); byte stuffing and
               file assembly on the host (host clock); beside a plain device-to-device copy of the bank's bytes, the yardstick
               of the FDCT kernel, which has to read every pixel at least once

Clock: time.perf_counter around work that ends in a stream synchronise (host paths), device events (device stages).  Prints
one JSON line and, with --out, writes it.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    import fdet_amd  # noqa: F401
    from concurrent.futures import ThreadPoolExecutor
    from fdet_amd import hotpath as hp
    from fdet_amd.datasets import augment as A
    from fdet_amd.datasets.jpeg import DeviceJpegEncoder
    from fdet_amd.render import save_images
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_encode_throughput needs a GPU")
    Q, SUB = 75, "4:2:0"

    def stats(v):
        a = np.asarray(v, dtype=np.float64)
        return {"median_ms": round(float(np.median(a)), 3), "p5_ms": round(float(np.percentile(a, 5)), 3),
                "p95_ms": round(float(np.percentile(a, 95)), 3), "samples": len(a)}

    def host_ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def event_ms(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    bank, _boxes = A.synthetic_bank(args.images, "cuda", seed=0, min_side=700, max_side=1024, max_faces=16)
    n = len(bank)
    enc = DeviceJpegEncoder("cuda", quality=Q, subsampling=SUB)
    res = {"tool": "jpeg_encode_throughput", "device": torch.cuda.get_device_name(0), "images": n, "quality": Q, "subsampling": SUB,
           "host_threads": 16, "megapixels": round(bank.nbytes / 3e6, 2), "rgb_MiB": round(bank.nbytes / 2 ** 20, 2),
           "clock": "time.perf_counter around a synchronised call (host paths), device events (device stages)"}

    def pil_bytes():
        arrays = bank.to_arrays()

        def one(a):
            f = io.BytesIO()
            Image.fromarray(a).save(f, "JPEG", quality=Q, subsampling=2)
            return f.getvalue()
        with ThreadPoolExecutor(16) as ex:
            return list(ex.map(one, arrays))

    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: [os.path.join(tmp, k, f"{i:04d}.jpg") for i in range(n)] for k in ("pil", "device")}
        fns = {"to_bytes": {"pil_16_threads": pil_bytes, "device_encoder": lambda: enc.encode(bank)},
               "to_files": {"pil_16_threads": lambda: save_images(bank, paths["pil"]),
                            "device_encoder": lambda: save_images(bank, paths["device"], encoder="device")}}
        got = {k: f() for k, f in fns["to_bytes"].items()}                             # warm-up, and the equality check
        res["byte_equal"] = got["pil_16_threads"] == got["device_encoder"]
        res["file_MiB"] = round(sum(len(b) for b in got["device_encoder"]) / 2 ** 20, 2)
        res["scan_MiB"] = round(enc.scan_bytes / 2 ** 20, 2)
        res["chunks"] = enc.chunks
        del got
        for f in fns["to_files"].values():
            f()
        res["files_equal"] = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths["pil"], paths["device"]))
        for group, pair in fns.items():
            t = {k: [] for k in pair}
            for _ in range(args.repeats):
                for k, f in pair.items():                                              # alternated: both see the same host
                    t[k].append(host_ms(f)[0])
            res[group] = {k: {**stats(v), "images_per_s": round(n / np.median(v) * 1e3, 1)} for k, v in t.items()}
            res[group]["device_over_pil"] = round(float(np.median(t["device_encoder"]) / np.median(t["pil_16_threads"])), 4)

    # the stages of the device path, one chunk holding every image
    idx = np.arange(n)
    descs = enc._descs(bank, idx)
    nb = descs["n_blocks"].astype(np.int64)
    descs["block_base"] = np.cumsum(nb) - nb
    B = int(nb.sum())
    ws = torch.empty(hp.jpeg_enc_ws_bytes(B, n), dtype=torch.uint8, device="cuda")
    d_descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()

    def plan():
        hp.jpeg_enc_plan(bank.data, d_descs, descs, Q, enc.sub, ws)
    plan()
    torch.cuda.synchronize()
    totals = ws[136 * B:136 * B + 4 * n].cpu().numpy().view(np.uint32).copy()
    nbytes = (totals.astype(np.int64) + 7) // 8
    spans = (nbytes + 3) // 4 * 4
    descs["scan_offset"] = np.cumsum(spans) - spans
    d_descs2 = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
    size = int(spans.sum())
    scan = torch.empty(size, dtype=torch.uint8, device="cuda")
    stage = torch.empty(size, dtype=torch.uint8).pin_memory()
    headers = [hp.jpeg_write_header(int(d["width"]), int(d["height"]), Q, enc.sub) for d in descs]

    def emit():
        scan.zero_()
        hp.jpeg_enc_emit(d_descs2, descs, totals, enc.sub, ws, scan)

    def assemble():
        host = stage.numpy()
        return [headers[k] + host[int(o):int(o) + int(m)].tobytes().replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
                for k, (o, m) in enumerate(zip(descs["scan_offset"], nbytes))]
    first = int(bank.table["offset"].min())
    src = bank.data[first:first + bank.nbytes]
    dst = torch.empty_like(src)
    rows = {"plan_kernels": [], "emit_kernel_and_memset": [], "d2h_copy": [], "host_stuff_and_assemble": [], "plain_copy_of_the_bank": []}
    for r in range(args.repeats + 1):                       # the first round is the warm-up
        row = {"plan_kernels": event_ms(plan), "emit_kernel_and_memset": event_ms(emit),
               "d2h_copy": event_ms(lambda: stage.copy_(scan, non_blocking=True)),
               "host_stuff_and_assemble": host_ms(assemble)[0], "plain_copy_of_the_bank": event_ms(lambda: dst.copy_(src))}
        if r:
            for k, v in row.items():
                rows[k].append(v)
    out = {k: stats(v) for k, v in rows.items()}
    out["plan_kernels"].update(blocks=B, rgb_bytes=bank.nbytes, coefficient_bytes=128 * B,
                               rgb_GB_per_s=round(bank.nbytes / out["plan_kernels"]["median_ms"] / 1e6, 1),
                               kernels="k_enc_fdct + k_enc_bits + k_enc_scan, timed together")
    out["d2h_copy"].update(bytes=size, GB_per_s=round(size / out["d2h_copy"]["median_ms"] / 1e6, 1))
    out["plain_copy_of_the_bank"].update(bytes=bank.nbytes, rgb_GB_per_s=round(bank.nbytes / out["plain_copy_of_the_bank"]["median_ms"] / 1e6, 1),
                                         note="torch device-to-device copy: the bank's bytes read once and written once")
    res["stages"] = out
    res["stages_files_equal"] = assemble() == enc.encode(bank)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
