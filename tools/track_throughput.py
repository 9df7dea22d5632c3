"""Timings of the tracker (csrc/fdet_track.hip, fdet_amd/tracking.py): device events for the device paths, a host clock for the
host path, every shape warmed up, median / min / max over --launches launches, the paths alternated launch by launch.

    python tools/track_throughput.py [--launches 40] [--motion] [--refine] [--out profiles/r11_track.json]

Two configurations, 1 sequence x 256 frames and 16 sequences x 256 frames, about 8 faces per frame (seeded synthetic
sequences: moving boxes, 20 % dropouts, false positives; K = 100 rows per frame as a 10 x 10 head gives).  Three times each:
  fdet_track_update      one launch over all the frames (hotpath.track_update on a fresh copy of one state)
  host_restatement       the device-to-host copy of rows and counts plus tests/track_cpu_ref.track_update, what doing the
                         association on the host would cost at its plainest (a Python loop per frame)
  detector_256_frames    forward_frames + reduce_bounding_boxes.forward_batch on 256 ready-made uint8 frames (PoolResnet F=64,
                         bf16x3), the work that produces 256 frames' rows; context, not part of the tracker
and, for the single sequence, two reduced launches that say where the time of the full one goes:
  no_detections          every count zero: the walk over 256 frames alone (barriers, ballots, the zeroed outputs)
  no_tracks              the same rows with birth_score = inf, so no track ever exists: the walk plus step 1 (rows read,
                         validated and compacted, det_ids written); what the full launch adds to it is matching, updates,
                         births and the emitted rows
With --motion, fdet_track_update_motion (FaceTracker's default motion parameters) is timed too, in both configurations,
alternated launch by launch with fdet_track_update on the same rows, and checked against tests/track_motion_cpu_ref.py;
motion_over_old is the ratio of the two medians, the cost of the motion steps.  The tracks move, so the matching of that
launch is not the old entry's; motion_neutral is the new entry with beta256 = 0, which computes the old entry's bytes (checked)
and so times the added instructions alone, and neutral_over_old is its ratio.  In that alternation every path always follows
the same other path (the new entry follows the detector), so ab_rotated times the three tracker launches once more by
themselves, the order rotated launch by launch so that each follows each equally often; its ratios are the ones to quote.
With --refine, fdet_track_refine (the offline second pass, default parameters of tracking.refine_tracks) runs on what
fdet_track_update returned for the same frames, in both configurations, the order rotated launch by launch with
fdet_track_update; it is checked against tests/track_refine_cpu_ref.py, which is timed once on the host (copies included).
refine_over_update is the ratio of the two medians.  Two reduced launches say where its time goes: refine_no_stitch
(stitch_gap = -1: pass 3 is skipped) and refine_no_rows (no emitted row and no det_id: the two walks over the frames alone,
barriers and dependent loads, with nothing to link, stitch or write but zeros).

Prints one JSON line and, with --out, writes it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-launches", type=int, default=3, help="repetitions of the host restatement (seconds each)")
    ap.add_argument("--motion", action="store_true", help="also time fdet_track_update_motion, alternated with the old entry")
    ap.add_argument("--refine", action="store_true", help="also time fdet_track_refine on the tracker's output")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    import track_cpu_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("track_throughput needs a GPU")
    n_l = max(30, args.launches)
    T, K = 256, 100
    PAR = dict(iou_threshold=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=5, birth_score=0.0)
    MOTION = dict(beta256=128, damp256=256, max_speed=64, grow256=0)
    if args.motion:
        import track_motion_cpu_ref as RM
    REFINE = dict(lookback=5, grow256=0, stitch_gap=10, stitch_iou=0.1, min_length=1)
    if args.refine:
        import track_refine_cpu_ref as RR

    def stats(ms):
        a = np.sort(np.asarray(ms))
        return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4),
                "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(len(a) * 9) // 10]), 4), "launches": len(a)}

    def timed(fns, n, rotate=False):
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        out = {k: [] for k in fns}
        for i in range(n):
            order = list(fns.items())
            if rotate:
                order = order[i % len(order):] + order[:i % len(order)]
            for k, f in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                out[k].append(e0.elapsed_time(e1))
        return out

    from fdet_amd.models.PoolResnet import PoolResnet
    torch.manual_seed(0)
    model = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10).cuda().eval()
    frames = torch.randint(0, 256, (T, 3, 480, 480), dtype=torch.uint8, device="cuda")

    def detector():
        with torch.no_grad():
            model.reduce_bounding_boxes.forward_batch(model.forward_frames(frames))

    res = {"tool": "track_throughput", "device": torch.cuda.get_device_name(0), "frames_per_sequence": T, "K": K,
           "params": PAR, "configs": {}}
    if args.motion:
        res["motion_params"] = MOTION
    if args.refine:
        res["refine_params"] = REFINE
    for n_seq in (1, 16):
        parts = [R.synthetic_sequence(T, K, 100 + s, faces=8, size=(1280, 720), false_positives=0.8) for s in range(n_seq)]
        rows = np.concatenate([p[0] for p in parts])
        counts = np.concatenate([p[1] for p in parts])
        h_off = (np.arange(n_seq + 1) * T).astype(np.int32)
        d_rows, d_counts, d_off = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(h_off).cuda()
        state = torch.zeros(n_seq * hp.TRACK_STATE_BYTES, dtype=torch.uint8, device="cuda")
        rej = torch.zeros(1, dtype=torch.int64, device="cuda")
        keep = {}

        def device(r=d_rows, c=d_counts, par=PAR):
            state.zero_()                                    # every launch starts from the fresh state (a 6 KiB memset)
            keep["out"] = hp.track_update(r, c, d_off, h_off, state, rejected=rej, **par)

        def device_motion():
            state.zero_()
            keep["motion"] = hp.track_update_motion(d_rows, d_counts, d_off, h_off, state, rejected=rej, **PAR, **MOTION)

        def device_neutral():
            state.zero_()
            keep["neutral"] = hp.track_update_motion(d_rows, d_counts, d_off, h_off, state, rejected=rej, **PAR,
                                                     **{**MOTION, "beta256": 0})

        fns = {"fdet_track_update": device, "detector_256_frames": detector}
        if args.motion:
            fns["fdet_track_update_motion"] = device_motion
            fns["motion_neutral"] = device_neutral
        if n_seq == 1:
            zero_counts = torch.zeros_like(d_counts)
            fns["no_detections"] = lambda: device(d_rows, zero_counts)
            fns["no_tracks"] = lambda: device(d_rows, d_counts, {**PAR, "birth_score": float("inf")})
        t = timed(fns, n_l)
        motion_equal = None
        if args.motion:
            ab = timed({"fdet_track_update": device, "fdet_track_update_motion": device_motion, "motion_neutral": device_neutral},
                       3 * ((n_l + 2) // 3), rotate=True)
            device_motion()
            torch.cuda.synchronize()
            got_m = [o.cpu().numpy() for o in keep["motion"][:5]]
            s_m = R.fresh_state(n_seq)
            want_m = RM.track_update_motion(rows, counts, h_off, s_m, **PAR, **MOTION)
            motion_equal = all(np.array_equal(a, b) for a, b in zip(got_m, want_m[:5])) and \
                state.cpu().numpy().tobytes() == s_m.tobytes()
            device_neutral()
            torch.cuda.synchronize()
            got_n, state_n = [o.cpu().numpy() for o in keep["neutral"][:5]], state.cpu().numpy().tobytes()
        device()
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in keep["out"][:5]]
        got_state = state.cpu().numpy().view(R.STATE_DTYPE)

        host_s, want, s_ref = [], None, None
        for _ in range(max(1, args.host_launches)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_rows, h_counts = d_rows.cpu().numpy(), d_counts.cpu().numpy()
            s_ref = R.fresh_state(n_seq)
            want = R.track_update(h_rows, h_counts, h_off, s_ref, **PAR)
            host_s.append((time.perf_counter() - t0) * 1e3)
        equal = all(np.array_equal(a, b) for a, b in zip(got, want[:5])) and got_state.tobytes() == s_ref.tobytes()
        entry = {"sequences": n_seq, "frames": n_seq * T, "detections_per_frame": round(float(counts.mean()), 2),
                 "tracks_emitted_per_frame": round(float(got[3].mean()), 2), "ids": int(got_state["seq"]["next_id"].sum()),
                 "rejected": int(rej.item()), "equal_to_restatement": bool(equal),
                 **{k: stats(v) for k, v in t.items()}, "host_restatement": stats(host_s)}
        d_ms = entry["fdet_track_update"]["median_ms"]
        if args.motion:
            entry["motion_equal_to_restatement"] = bool(motion_equal)
            entry["motion_ids"] = int(s_m["seq"]["next_id"].sum())
            entry["motion_over_old"] = round(entry["fdet_track_update_motion"]["median_ms"] / d_ms, 4)
            entry["neutral_equal_to_old_entry"] = bool(all(np.array_equal(a, b) for a, b in zip(got_n, got)) and
                                                       state_n == got_state.tobytes())
            entry["neutral_over_old"] = round(entry["motion_neutral"]["median_ms"] / d_ms, 4)
            entry["ab_rotated"] = {k: stats(v) for k, v in ab.items()}
            ab_ms = entry["ab_rotated"]["fdet_track_update"]["median_ms"]
            entry["ab_rotated"]["motion_over_old"] = round(entry["ab_rotated"]["fdet_track_update_motion"]["median_ms"] / ab_ms, 4)
            entry["ab_rotated"]["neutral_over_old"] = round(entry["ab_rotated"]["motion_neutral"]["median_ms"] / ab_ms, 4)
        if args.refine:
            o = keep["out"]                                  # what the online pass returned: rows, ids, misses, counts, det_ids
            rej2 = torch.zeros(2, dtype=torch.int64, device="cuda")
            no_counts, no_ids = torch.zeros_like(o[3]), torch.zeros_like(o[4])

            def refine(par=REFINE, c=o[3], di=o[4]):
                keep["refine"] = hp.track_refine(d_rows, di, o[0], o[1], o[2], c, d_off, h_off, rejected=rej2, **par)

            fr = {"fdet_track_update": device, "fdet_track_refine": refine,
                  "refine_no_stitch": lambda: refine({**REFINE, "stitch_gap": -1}),
                  "refine_no_rows": lambda: refine(REFINE, no_counts, no_ids)}
            tr = timed(fr, 4 * ((n_l + 3) // 4), rotate=True)
            rej2.zero_()
            refine()
            torch.cuda.synchronize()
            got_r = [x.cpu().numpy() for x in keep["refine"][:5]] + [keep["refine"][5].cpu().tolist()]
            t0 = time.perf_counter()
            h_in = [x.cpu().numpy() for x in (d_rows, o[4], o[0], o[1], o[2], o[3])]
            want_r = RR.track_refine(*h_in, h_off, **REFINE)
            host_refine_ms = (time.perf_counter() - t0) * 1e3
            entry["refine"] = {k: stats(v) for k, v in tr.items()}
            r = entry["refine"]
            r["equal_to_restatement"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(got_r[:5], want_r[:5])) and
                                             got_r[5] == want_r[5])
            r["host_restatement_ms"] = round(host_refine_ms, 1)
            r["rejected"] = got_r[5]
            r["rows_by_kind"] = [int((got_r[3][got_r[1] > 0] == k).sum()) for k in range(4)]
            r["stitches"], r["chains"] = want_r[6]["stitches"], int(sum(len(np.unique(got_r[1][a:b][got_r[1][a:b] > 0]))
                                                                  for a, b in zip(h_off[:-1], h_off[1:])))
            u_ms, f_ms = r["fdet_track_update"]["median_ms"], r["fdet_track_refine"]["median_ms"]
            r["refine_over_update"] = round(f_ms / u_ms, 3)
            r["host_over_device"] = round(host_refine_ms / f_ms, 1)
            r["us_per_frame_of_a_sequence"] = round(f_ms / T * 1e3, 3)
            r["split_ms"] = {"walks_alone": r["refine_no_rows"]["median_ms"],
                             "stitch": round(f_ms - r["refine_no_stitch"]["median_ms"], 4),
                             "anchors_links_rows": round(r["refine_no_stitch"]["median_ms"] - r["refine_no_rows"]["median_ms"], 4)}
        matched = int((got[4] != 0).sum()) - int(got_state["seq"]["next_id"].sum())
        entry["matches_per_frame"] = round(matched / (n_seq * T), 2)
        if "no_detections" in entry:
            e_ms, c_ms = entry["no_detections"]["median_ms"], entry["no_tracks"]["median_ms"]
            entry["us_per_frame_split"] = {"walk": round(e_ms / T * 1e3, 3), "step_1": round((c_ms - e_ms) / T * 1e3, 3),
                                           "matching_update_births_emit": round((d_ms - c_ms) / T * 1e3, 3)}
        entry["us_per_frame_of_a_sequence"] = round(d_ms / T * 1e3, 3)
        entry["frames_per_s"] = round(n_seq * T / d_ms * 1e3, 1)
        entry["host_over_device"] = round(entry["host_restatement"]["median_ms"] / d_ms, 1)
        entry["device_over_detector_256_frames"] = round(d_ms / entry["detector_256_frames"]["median_ms"], 3)
        res["configs"][f"{n_seq}x{T}"] = entry

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
