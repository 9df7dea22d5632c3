"""Timings of the test-time augmentation of tiled detection (csrc/fdet_tiles.hip), by the method of
tools/tile_throughput.py: device events, every shape warmed up, median / min / max over --launches individually timed
launches, the two sides of a comparison alternated launch by launch in one process.

    python tools/tta_throughput.py [--launches 40] [--out profiles/r11_tta.json]

  gather    fdet_tile_gather_flags with half the windows flagged (every second one) against fdet_tile_gather followed by
            flip(-1) of the flagged half, on the windows and the bank of tile_throughput's gather cases.  The flip is taken
            two ways: "fdet_tile_gather_then_flip" flips the strided view fr[1::2] into a temporary and copies it back (two
            launches, each one read and one write of the flagged half); "fdet_tile_gather_then_flip_indexed" is what
            TiledDetector's own fallback runs for arbitrary flags (index_select, flip, index_copy_: three launches).
            "flags_faster" is true only when the flagged gather's slowest launch beat the fastest launch of both, which is
            what tiling.FLAGGED_GATHER_MEASURED_FASTER may be set from
  merge     fdet_tile_merge_vote with vote = 1 and with vote = 0 (no window flagged) beside fdet_tile_merge on the same
            candidates: tile_throughput's two merge cases (random boxes, about 15 and 150 per window) and one with the
            candidates in clusters of about 4.  Per case also the survivors and the suppressed candidates per image and the
            time per image that each vote side adds to fdet_tile_merge
  detect    TiledDetector.detect with flip=True, vote=True beside the default on tile_throughput's 64-image case

Prints one JSON line and, with --out, writes it.
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
    from fdet_amd.datasets import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("tta_throughput needs a GPU")
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

    res = {"tool": "tta_throughput", "device": torch.cuda.get_device_name(0)}
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
        res["gather"] = {"bank_MiB": round(bank.data.numel() / 2 ** 20, 1), "bank_images": len(bank), "windows": 256, "flagged": 128}
        flags = np.zeros(256, np.uint8)
        flags[1::2] = 1
        d_flags = torch.from_numpy(flags).cuda()
        d_sel = torch.from_numpy(np.nonzero(flags)[0]).cuda()
        for name, wins in cases.items():
            tiles = np.array(wins, dtype=TL.TILE_DTYPE)
            d_tiles = torch.from_numpy(tiles.view(np.uint8).copy()).cuda()
            fr_a = torch.empty(256, 3, 480, 480, dtype=U8, device="cuda")
            fr_b = torch.empty_like(fr_a)

            def flagged():
                hp.tile_gather_flags(bank.data, bank.d_table, bank.table, d_tiles, tiles, d_flags, flags, (480, 480), fr_a)

            fr_c = torch.empty_like(fr_a)

            def gather_flip():
                hp.tile_gather(bank.data, bank.d_table, bank.table, d_tiles, tiles, (480, 480), fr_b)
                half = fr_b[1::2]
                half.copy_(half.flip(-1))

            def gather_flip_indexed():
                hp.tile_gather(bank.data, bank.d_table, bank.table, d_tiles, tiles, (480, 480), fr_c)
                fr_c.index_copy_(0, d_sel, fr_c.index_select(0, d_sel).flip(-1))

            t = timed({"fdet_tile_gather_flags": flagged, "fdet_tile_gather_then_flip": gather_flip,
                       "fdet_tile_gather_then_flip_indexed": gather_flip_indexed})
            same = bool(torch.equal(fr_a, fr_b)) and bool(torch.equal(fr_a, fr_c))
            del fr_c
            traffic = int((tiles["w"].astype(np.int64) * tiles["h"] * 3).sum() + 256 * 3 * 480 * 480)
            entry = {"bytes": traffic, "byte_equal": same}
            for k, v in t.items():
                s = stats(v)
                s["GB_per_s"] = round(traffic / s["median_ms"] / 1e6, 1)
                entry[k] = s
            a, b, c = (entry[k] for k in ("fdet_tile_gather_flags", "fdet_tile_gather_then_flip", "fdet_tile_gather_then_flip_indexed"))
            entry["flags_over_gather_flip"] = round(a["median_ms"] / b["median_ms"], 3)
            entry["flags_over_gather_flip_indexed"] = round(a["median_ms"] / c["median_ms"], 3)
            entry["flags_faster"] = bool(a["max_ms"] < min(b["min_ms"], c["min_ms"]))      # beyond the observed min-max spread
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
        for name, per in (("15_per_window", 15), ("150_per_window", 150), ("clusters_of_4", 60)):
            g = torch.Generator().manual_seed(per)
            rows = torch.rand(256, K, 5, generator=g)
            rows[:, :, 1:3] *= 420
            rows[:, :, 3:] = rows[:, :, 3:] * 60 + 8
            if name == "clusters_of_4":                                      # every fourth row four times, jittered by 3 px
                rows = rows[:, ::4].repeat_interleave(4, 1)[:, :K].clone()
                rows[:, :, 1:] = (rows[:, :, 1:] + torch.rand(256, K, 4, generator=g) * 6 - 3).round()
                rows[:, :, 0] = torch.rand(256, K, generator=g)
            rows = rows.cuda()
            counts = torch.full((256,), per, dtype=torch.int32, device="cuda")
            rej = torch.zeros(1, dtype=torch.int64, device="cuda")
            kept = {}

            def merge():
                kept["merge"] = hp.tile_merge(rows, counts, d_tiles, d_off, d_table, (480, 480), 0.0, 0.5, 4864, rej)[1]

            def merge_vote():
                r = hp.tile_merge_vote(rows, counts, d_tiles, None, d_off, d_table, (480, 480), 0.0, 0.5, 4864, True, 1, rej)
                kept["vote"], kept["votes"] = r[2], r[1]

            def merge_vote0():
                kept["vote0"] = hp.tile_merge_vote(rows, counts, d_tiles, None, d_off, d_table, (480, 480), 0.0, 0.5, 4864, False, 1,
                                                   rej)[2]

            t = timed({"fdet_tile_merge": merge, "fdet_tile_merge_vote": merge_vote, "fdet_tile_merge_vote_vote0": merge_vote0})
            n_keep = kept["vote"].float().sum()
            keepers = float(kept["vote"].float().mean())
            members = float(kept["votes"].float().sum()) / 16                # edge_margin 0: every candidate is a member
            entry = {"candidates_per_image": 16 * per, "rejected": int(rej.item()),
                     "survivors_per_image_merge": float(kept["merge"].float().mean()),
                     "survivors_per_image_vote": keepers,
                     "survivors_per_image_vote0": float(kept["vote0"].float().mean()),
                     "suppressed_per_image": round(members - keepers, 2),
                     "members_per_survivor": round(float(kept["votes"].float().sum() / n_keep), 3),
                     **{k: stats(v) for k, v in t.items()}}
            base = entry["fdet_tile_merge"]["median_ms"]
            entry["vote_over_merge"] = round(entry["fdet_tile_merge_vote"]["median_ms"] / base, 3)
            entry["vote0_over_merge"] = round(entry["fdet_tile_merge_vote_vote0"]["median_ms"] / base, 3)
            # one workgroup per image and 16 equal images on 256 CUs: a launch lasts as long as one image
            for k, name2 in (("fdet_tile_merge_vote", "vote"), ("fdet_tile_merge_vote_vote0", "vote0")):
                extra = (entry[k]["median_ms"] - base) * 1e3
                entry[f"{name2}_added_us"] = round(extra, 1)
                entry[f"{name2}_added_us_per_survivor"] = round(extra / keepers, 3)
            res["merge"][name] = entry

    if "detect" in sections:
        from fdet_amd.models.PoolResnet import PoolResnet
        res["detect"] = {"flagged_gather_in_detect": bool(TL.FLAGGED_GATHER_MEASURED_FASTER)}
        bank, _ = A.synthetic_bank(64, "cuda", seed=2, min_side=700, max_side=1024)
        torch.random.manual_seed(0)
        for prec in ("bf16x3", "bf16"):
            model = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10).cuda().eval()
            if prec == "bf16":
                model.engine.set_precision("bf16")
            kw = dict(tile_sizes=(480,), overlap=0.25, include_whole=True)
            plain, tta = TL.TiledDetector(model, **kw), TL.TiledDetector(model, flip=True, vote=True, **kw)
            idx = list(range(64))
            state = {}

            def detect():
                state["c"] = plain.detect(bank, idx)[1]

            def detect_tta():
                state["t"] = tta.detect(bank, idx)[1]

            t = timed({"detect_64_images": detect, "detect_64_images_flip_vote": detect_tta})
            a, b = float(np.median(t["detect_64_images"])), float(np.median(t["detect_64_images_flip_vote"]))
            res["detect"][prec] = {"images": 64, "frames": len(plain.plan(bank.sizes)), "frames_flip": len(tta.plan_tta(bank.sizes)[0]),
                                   **{k: stats(v) for k, v in t.items()},
                                   "source_images_per_s": round(64 / a * 1e3, 1), "source_images_per_s_flip_vote": round(64 / b * 1e3, 1),
                                   "flip_vote_over_default": round(b / a, 3)}
            del model, plain, tta

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
