"""Timings of the tiled detection path (csrc/fdet_tiles.hip, fdet_amd/tiling.py), device events, every shape warmed up,
median / min / max over --launches launches, the two kernels of a comparison alternated launch by launch.

    python tools/tile_throughput.py [--launches 40] [--out profiles/r08_tiles.json]

  gather    fdet_tile_gather against fdet_aug_warp (flags = 0, the same windows as crops): 256 windows of 480x480 at scale 1
            and 256 whole images of about 1024x700 -> 480x480, every window in a different image of a bank of more than
            256 MiB; GB/s against the traffic the shapes imply (window bytes read once + frame bytes written)
  merge     fdet_tile_merge at 256 windows of 16 images with about 15 and about 150 detections per window, beside fdet_nms
            on the same number of candidates per image
  detect    TiledDetector.detect on 64 synthetic images of about 1024x700 (PoolResnet F=64, bf16x3 and precision16) beside
            forward_frames + reducer on 256 ready-made frames; the gather and merge launches of one detect timed on their own

Prints one JSON line and, with --out, writes it.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bank", type=int, default=400)
    ap.add_argument("--sections", default="gather,merge,detect")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp, tiling as TL
    from fdet_amd._native import check, lib, ptr, stream
    from fdet_amd.datasets import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("tile_throughput needs a GPU")
    U8 = torch.uint8
    n_l = max(30, args.launches)

    def stats(ms):
        a = np.sort(np.asarray(ms))
        return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4),
                "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(len(a) * 9) // 10]), 4), "launches": len(a)}

    def timed(fns):
        """fns: name -> callable; alternated launch by launch -> name -> list of ms"""
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        out = {k: [] for k in fns}
        for _ in range(n_l):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                out[k].append(e0.elapsed_time(e1))
        return out

    res = {"tool": "tile_throughput", "device": torch.cuda.get_device_name(0)}
    sections = args.sections.split(",")

    if "gather" in sections:
        g = np.random.default_rng(0)
        imgs = []
        for _ in range(args.bank):
            H, W = int(g.integers(640, 760)), int(g.integers(960, 1088))
            base = g.integers(0, 256, (H // 8 + 2, W // 8 + 2, 3), dtype=np.uint8)
            imgs.append(np.ascontiguousarray(np.repeat(np.repeat(base, 8, 0), 8, 1)[:H, :W]))
        bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
        del imgs
        pick = g.permutation(len(bank))[:256]
        sz = bank.sizes
        cases = {
            "identity_480": [(int(i), int(g.integers(0, sz[i, 1] - 480 + 1)), int(g.integers(0, sz[i, 0] - 480 + 1)), 480, 480)
                             for i in pick],
            "whole_1024x700": [(int(i), 0, 0, int(sz[i, 1]), int(sz[i, 0])) for i in pick],
        }
        res["gather"] = {"bank_MiB": round(bank.data.numel() / 2 ** 20, 1), "bank_images": len(bank), "windows": 256}
        for name, wins in cases.items():
            tiles = np.array(wins, dtype=TL.TILE_DTYPE)
            d_tiles = torch.from_numpy(tiles.view(np.uint8).copy()).cuda()
            P = np.zeros(len(tiles), A.PARAMS_DTYPE)
            for k in ("image",):
                P[k] = tiles[k]
            P["crop_x0"], P["crop_y0"], P["crop_w"], P["crop_h"] = tiles["x0"], tiles["y0"], tiles["w"], tiles["h"]
            P["cos_a"], P["alpha"], P["motion_k"] = 1.0, 1.0, 1
            d_P = torch.from_numpy(P.view(np.uint8).copy()).cuda()
            fr_a = torch.empty(256, 3, 480, 480, dtype=U8, device="cuda")
            fr_b = torch.empty_like(fr_a)
            L = lib()

            def warp():
                check(L.fdet_aug_warp(ptr(bank.data, U8), ptr(bank.d_table, U8), bank.table.ctypes.data, len(bank), ptr(d_P, U8),
                                      P.ctypes.data, 256, 480, 480, 0, ptr(fr_a, U8), stream()), "warp")

            def gather():
                hp.tile_gather(bank.data, bank.d_table, bank.table, d_tiles, tiles, (480, 480), fr_b)

            t = timed({"fdet_aug_warp": warp, "fdet_tile_gather": gather})
            same = bool(torch.equal(fr_a, fr_b))
            traffic = int((tiles["w"].astype(np.int64) * tiles["h"] * 3).sum() + 256 * 3 * 480 * 480)
            entry = {"bytes": traffic, "byte_equal": same}
            for k, v in t.items():
                s = stats(v)
                s["GB_per_s"] = round(traffic / s["median_ms"] / 1e6, 1)
                entry[k] = s
            entry["gather_over_warp"] = round(entry["fdet_tile_gather"]["median_ms"] / entry["fdet_aug_warp"]["median_ms"], 3)
            res["gather"][name] = entry
        del bank

    if "merge" in sections:
        res["merge"] = {}
        sizes = [(1560, 1560)] * 16
        plan = TL.plan_tiles(sizes, (480,), 0.25, include_whole=False)
        assert len(plan) == 256
        table = np.zeros(16, A.IMAGE_DTYPE)
        table["h"], table["w"] = 1560, 1560
        d_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        d_tiles = torch.from_numpy(plan.tiles.view(np.uint8).copy()).cuda()
        d_off = torch.from_numpy(plan.tile_offset).cuda()
        K = 225
        for per in (15, 150):
            g = torch.Generator().manual_seed(per)
            rows = torch.rand(256, K, 5, generator=g)
            rows[:, :, 1:3] *= 420
            rows[:, :, 3:] = rows[:, :, 3:] * 60 + 8
            rows = rows.cuda()
            counts = torch.full((256,), per, dtype=torch.int32, device="cuda")
            rej = torch.zeros(1, dtype=torch.int64, device="cuda")
            C = 16 * per
            boxes = torch.rand(16, C, 4, generator=g) * 1500
            boxes[:, :, 2:] = boxes[:, :, :2] + torch.rand(16, C, 2, generator=g) * 60 + 8
            boxes, scores = boxes.cuda(), torch.rand(16, C, generator=g).cuda()
            cnt = torch.full((16,), C, dtype=torch.int32, device="cuda")
            kept = {}

            def merge():
                kept["merge"] = hp.tile_merge(rows, counts, d_tiles, d_off, d_table, (480, 480), 0.0, 0.5, 4864, rej)[1]

            def nms():
                kept["nms"] = hp.nms_batched(boxes, scores, cnt, 0.5)[1]

            t = timed({"fdet_tile_merge": merge, "fdet_nms": nms})
            res["merge"][f"{per}_per_window"] = {"candidates_per_image": C, "rejected": int(rej.item()),
                                                 "survivors_per_image_merge": float(kept["merge"].float().mean()),
                                                 "survivors_per_image_nms": float(kept["nms"].float().mean()),
                                                 **{k: stats(v) for k, v in t.items()}}

    if "detect" in sections:
        from fdet_amd.models.PoolResnet import PoolResnet
        res["detect"] = {}
        bank, _ = A.synthetic_bank(64, "cuda", seed=2, min_side=700, max_side=1024)
        torch.random.manual_seed(0)
        for prec in ("bf16x3", "bf16"):
            model = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10).cuda().eval()
            if prec == "bf16":
                model.engine.set_precision("bf16")
            det = TL.TiledDetector(model, tile_sizes=(480,), overlap=0.25, include_whole=True)
            plan = det.plan(bank.sizes)
            frames = torch.randint(0, 256, (256, 3, 480, 480), dtype=U8, device="cuda")
            idx = list(range(64))
            state = {}

            def detect():
                state["c"] = det.detect(bank, idx)[1]

            def ready_made():
                with torch.no_grad():
                    state["r"] = model.reduce_bounding_boxes.forward_batch(model.forward_frames(frames))

            t = timed({"detect_64_images": detect, "forward_frames_reducer_256": ready_made})
            # the gather and merge launches of one detect on their own
            d_tiles = torch.from_numpy(plan.tiles.view(np.uint8).copy()).cuda()
            T = len(plan)
            rows = torch.zeros(T, 100, 5, device="cuda")
            counts = torch.zeros(T, dtype=torch.int32, device="cuda")
            d_off = torch.from_numpy(plan.tile_offset).cuda()

            def gathers():
                for a in range(0, T, 256):
                    b = min(a + 256, T)
                    hp.tile_gather(bank.data, bank.d_table, bank.table, d_tiles[a * 20:b * 20], plan.tiles[a:b], (480, 480))

            def merge():
                hp.tile_merge(rows, counts, d_tiles, d_off, bank.d_table, (480, 480), 0.0, 0.5, 4864)

            t2 = timed({"gather_launches": gathers, "merge_launch": merge})
            d_ms = float(np.median(t["detect_64_images"]))
            f_ms = float(np.median(t["forward_frames_reducer_256"]))
            gm = float(np.median(t2["gather_launches"]) + np.median(t2["merge_launch"]))
            res["detect"][prec] = {"images": 64, "frames": T, **{k: stats(v) for k, v in {**t, **t2}.items()},
                                   "source_images_per_s": round(64 / d_ms * 1e3, 1), "frames_per_s": round(T / d_ms * 1e3, 1),
                                   "ready_made_frames_per_s": round(256 / f_ms * 1e3, 1),
                                   "gather_plus_merge_share": round(gm / d_ms, 4)}
            del model, det

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
