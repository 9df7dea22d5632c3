"""What the device JPEG decoder (csrc/fdet_jpeg.hip, fdet_amd/datasets/jpeg.py) buys over the PIL path, measured.

    python tools/jpeg_throughput.py [--images 256] [--repeats 5] [--out profiles/r10_jpeg.json] [--kernel-stats CSV]
                                    [--huffman host|device|both] [--sub-bits N]

256 seeded images of the synthetic bank's size distribution (about 1024x700) are encoded as 4:2:0 q90 JPEGs with PIL into
a temporary directory.  Timed, every path warmed up once, medians over --repeats, the two end-to-end paths alternated:

  end_to_end   bank_from_files with PIL on 16 threads (the default path) and with decoder="device": host clock around
               the call, which ends in a stream synchronise
  stages       of the device path on their own: reading the files, fdet_jpeg_info + fdet_jpeg_entropy_decode on 16
               threads into pinned memory (host clock), the host-to-device copy of the coefficients and
               fdet_jpeg_reconstruct (device events; its two kernels together), with the bytes the shapes imply (coefficients
               read, sample planes written and read, RGB written) over the time, beside a plain device-to-device copy of as
               many bytes on the same box
  kernels      with --kernel-stats: the per-kernel averages of a `rocprofv3 --kernel-trace --stats` run of this tool
               (taken in a run of its own; tracing slows the host)

  huffman      with --huffman device|both: the decoder with huffman="device" joins the alternated end-to-end
               paths (compare it with `device_decoder`, the huffman="host" path of the same run); its stages -- prepare on the
               host threads, the copy of the scans, the sync passes (count, device events), the emit with its scan and DC sum
               (device events) -- the bytes each mode sends across PCIe, and the end-to-end time at sub_bits 256, 512, 1024
               and 2048 (--sub-bits picks the size the rest of the run uses)

Clock: time.perf_counter for host stages, device events for device stages.  Prints one JSON line and, with --out, writes it.
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def huffman_section(args, np, torch, hp, DeviceJpegDecoder, blobs, infos, descs, n_coef, d_coef, hdec, med, host_ms, event_ms,
                    sub_bits, end_to_end):
    """The huffman="device" path: its stages on their own, the PCIe bytes of both modes, the sub_bits sweep."""
    from concurrent.futures import ThreadPoolExecutor
    chunk = list(enumerate(infos))
    names = [f"image {i}" for i in range(len(blobs))]
    out = {"sub_bits": sub_bits, "huffman_fallbacks": len(hdec.huffman_fallbacks), "sync_passes_end_to_end": hdec.sync_passes,
           "chunks_end_to_end": hdec.chunks}
    dec = DeviceJpegDecoder("cuda", huffman="device", sub_bits=sub_bits)
    rows = {"prepare_16_threads": [], "copy_scans": [], "sync_passes": [], "emit_scan_dcsum": []}
    passes = 0
    with ThreadPoolExecutor(16) as pool:
        for r in range(args.repeats + 1):                   # the first round is the warm-up
            dec.timings, dec.scan_bytes = {}, 0
            ms, staged = host_ms(lambda: dec.huffman_stage(pool, blobs, names, chunk, descs))
            d_scan, d_tab, d_images, images, d_segs, segs, n_subs, host = staged
            state = torch.zeros(3 * n_subs, dtype=torch.int64, device="cuda")
            first = torch.empty(n_subs, dtype=torch.int32, device="cuda")
            changed = torch.zeros(len(blobs), dtype=torch.int32, device="cuda")
            flags = torch.zeros(len(blobs), dtype=torch.int32, device="cuda")
            sync_ms, passes = 0.0, 0
            while True:                                      # pass by pass here: each one timed, the count exact
                changed.zero_()
                sync_ms += event_ms(lambda: hp.jpeg_huffman_sync(d_scan, d_tab, d_images, images, d_segs, segs, sub_bits, state,
                                                                 changed))
                passes += 1
                if not bool(changed.any()) or passes > int(segs["sub_count"].max()) + 1:
                    break
            emit_ms = event_ms(lambda: hp.jpeg_huffman_emit(d_scan, d_tab, d_images, images, d_segs, segs, sub_bits, state, first,
                                                            d_coef[:n_coef], flags))
            assert not bool(flags.any()) and not host
            if r:
                rows["prepare_16_threads"].append(dec.timings["prepare"] * 1e3)
                rows["copy_scans"].append(dec.timings["copy"] * 1e3)
                rows["sync_passes"].append(sync_ms)
                rows["emit_scan_dcsum"].append(emit_ms)
    out["stages"] = {k: med(v) for k, v in rows.items()}
    out["stages"]["sync_passes"]["passes"] = passes
    out["stages"]["sync_passes"]["subsequences"] = int(n_subs)
    out["stages"]["emit_scan_dcsum"]["kernels"] = "k_huff_scan + memset + k_huff_emit + k_huff_dcsum, timed together"
    out["pcie_bytes"] = {"huffman_host": 2 * n_coef + descs.nbytes, "huffman_device": int(dec.scan_bytes) + descs.nbytes,
                         "decoded_rgb": int(sum(int(i["height"]) * int(i["width"]) * 3 for i in infos))}
    # the subsequence size: end to end, the sizes alternated
    sizes = (256, 512, 1024, 2048)
    decs = {sb: DeviceJpegDecoder("cuda", huffman="device", sub_bits=sb) for sb in sizes}
    for d in decs.values():
        d.decode_bytes(blobs)
    t = {sb: [] for sb in sizes}
    for _ in range(args.repeats):
        for sb, d in decs.items():
            t[sb].append(host_ms(lambda: d.decode_bytes(blobs))[0])
    out["sub_bits_sweep"] = {str(sb): {**med(v), "sync_passes": decs[sb].sync_passes} for sb, v in t.items()}
    out["note"] = "decode_bytes (files already read) in the sweep; decode_files in end_to_end"
    a, b = end_to_end["device_decoder_device_huffman"], end_to_end["device_decoder"]
    end_to_end["device_huffman_over_host_huffman"] = round(a["median_ms"] / b["median_ms"], 3)
    end_to_end["spreads_overlap"] = bool(a["p95_ms"] >= b["p5_ms"] and b["p95_ms"] >= a["p5_ms"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--huffman", choices=("host", "device", "both"), default="host",
                    help="device | both: also measure the decoder with huffman='device' (both = beside huffman='host', as device does)")
    ap.add_argument("--sub-bits", type=int, default=None, help="bits per subsequence of the huffman='device' paths")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    import fdet_amd  # noqa: F401
    from concurrent.futures import ThreadPoolExecutor
    from fdet_amd import hotpath as hp
    from fdet_amd.datasets.WIDERFace.annotations import bank_from_files
    from fdet_amd.datasets.jpeg import DeviceJpegDecoder
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_throughput needs a GPU")

    def med(v):
        a = np.sort(np.asarray(v, dtype=np.float64))
        return {"median_ms": round(float(np.median(a)), 3), "min_ms": round(float(a[0]), 3), "max_ms": round(float(a[-1]), 3),
                "p5_ms": round(float(np.percentile(a, 5)), 3), "p95_ms": round(float(np.percentile(a, 95)), 3), "repeats": len(a)}

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

    res = {"tool": "jpeg_throughput", "device": torch.cuda.get_device_name(0), "images": args.images, "host_threads": 16,
           "clock": "time.perf_counter around a synchronised call (host stages), device events (device stages)"}
    with tempfile.TemporaryDirectory() as tmp:
        g = np.random.default_rng(10)
        paths, pixels = [], 0
        for i in range(args.images):
            H, W = int(g.integers(640, 760)), int(g.integers(960, 1088))
            base = g.integers(0, 256, (H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
            img = np.repeat(np.repeat(base, 16, 0), 16, 1)[:H, :W] + g.normal(0, 6, (H, W, 3))
            p = os.path.join(tmp, f"{i:04d}.jpg")
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(p, "JPEG", quality=90, subsampling=2)
            paths.append(p)
            pixels += H * W
        res["file_MiB"] = round(sum(os.path.getsize(p) for p in paths) / 2 ** 20, 2)
        res["megapixels"] = round(pixels / 1e6, 2)

        # end to end, alternated
        fns = {"pil_16_threads": lambda: bank_from_files(paths, "cuda"),
               "device_decoder": lambda: bank_from_files(paths, "cuda", decoder="device")}
        from fdet_amd.datasets.jpeg import DEFAULT_SUB_BITS
        sub_bits = args.sub_bits or DEFAULT_SUB_BITS
        if args.huffman != "host":
            hdec = DeviceJpegDecoder("cuda", huffman="device", sub_bits=sub_bits)  # one decoder: its buffers are reused
            fns["device_decoder_device_huffman"] = lambda: hdec.decode_files(paths)
        banks = {k: f() for k, f in fns.items()}                                   # warm-up, and the equality check
        res["byte_equal"] = all(bool(torch.equal(banks["pil_16_threads"].data, b.data)) for b in banks.values())
        del banks
        t = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, f in fns.items():
                t[k].append(host_ms(f)[0])
        res["end_to_end"] = {k: {**med(v), "images_per_s": round(args.images / np.median(v) * 1e3, 1)} for k, v in t.items()}
        res["end_to_end"]["device_over_pil"] = round(float(np.median(t["device_decoder"]) / np.median(t["pil_16_threads"])), 3)

        # the stages of the device path
        def read_all():
            with ThreadPoolExecutor(16) as ex:
                return list(ex.map(lambda p: open(p, "rb").read(), paths))
        blobs = read_all()
        infos = [hp.jpeg_info(b)[1] for b in blobs]
        dec = DeviceJpegDecoder("cuda")
        table = np.zeros(len(blobs), dtype=[("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])
        off = 0
        for i, info in enumerate(infos):
            table[i] = (off, info["height"], info["width"])
            off += int(info["height"]) * int(info["width"]) * 3
        descs, spans, n_coef, n_ws = dec._describe(list(enumerate(infos)), table)
        stage = torch.empty(n_coef, dtype=torch.int16).pin_memory()
        d_coef = torch.empty(n_coef, dtype=torch.int16, device="cuda")
        ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda")
        data = torch.empty(off, dtype=torch.uint8, device="cuda")
        d_descs = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
        base = stage.data_ptr()

        def entropy():
            with ThreadPoolExecutor(16) as ex:
                rcs = list(ex.map(lambda j: hp.jpeg_entropy_decode(blobs[j[0]], base + 2 * j[1][0], j[1][1])[0], enumerate(spans)))
            assert not any(rcs)

        def probe():
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(lambda b: hp.jpeg_info(b), blobs))
        traffic = 2 * n_coef + 2 * n_ws + off              # coefficients read, planes written then read, RGB written
        src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        stages = {"read_files": [], "jpeg_info": [], "entropy_decode": [], "h2d_copy": [], "reconstruct": [], "plain_copy": []}
        for r in range(args.repeats + 1):                   # the first round is the warm-up
            row = {"read_files": host_ms(read_all)[0], "jpeg_info": host_ms(probe)[0], "entropy_decode": host_ms(entropy)[0],
                   "h2d_copy": event_ms(lambda: d_coef.copy_(stage, non_blocking=True)),
                   "reconstruct": event_ms(lambda: hp.jpeg_reconstruct(d_coef, d_descs, descs, ws, data)),
                   "plain_copy": event_ms(lambda: dst.copy_(src))}
            if r:
                for k, v in row.items():
                    stages[k].append(v)
        out = {k: med(v) for k, v in stages.items()}
        out["entropy_decode"]["megapixels_per_s"] = round(pixels / 1e3 / out["entropy_decode"]["median_ms"], 1)
        out["h2d_copy"].update(bytes=2 * n_coef, GB_per_s=round(2 * n_coef / out["h2d_copy"]["median_ms"] / 1e6, 1))
        out["reconstruct"].update(bytes=traffic, GB_per_s=round(traffic / out["reconstruct"]["median_ms"] / 1e6, 1),
                                  kernels="k_jpeg_idct + k_jpeg_rgb, timed together")
        out["plain_copy"].update(bytes=traffic, GB_per_s=round(traffic / out["plain_copy"]["median_ms"] / 1e6, 1),
                                 note="torch device-to-device copy: traffic / 2 bytes read + traffic / 2 written")
        res["stages"] = out
        if args.huffman != "host":
            res["huffman"] = huffman_section(args, np, torch, hp, DeviceJpegDecoder, blobs, infos, descs, n_coef, d_coef, hdec, med,
                                             host_ms, event_ms, sub_bits, res["end_to_end"])
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "jpeg" in r.get("Name", "")]
        res["kernels"] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2)}
                          for r in rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
