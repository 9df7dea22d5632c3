"""Detect and track faces through a directory of video frames and write MOTChallenge text.

    python -m fdet_amd.track_frames --checkpoint CKPT --frames DIR --out FILE [--model poolresnet --filters 128]
        [--tiled --tile 480 --overlap 0.25] [--iou 0.3 --alpha 0.5 --max-misses 5 --min-hits 2 --emit-misses N]
        [--motion constant_velocity [--motion-beta 0.5] [--motion-damping 1.0] [--max-speed 64] [--coast-grow 0.0]]
        [--refine [--lookback 5] [--stitch-gap 10] [--stitch-iou 0.1] [--min-length 1]]
        [--draw DIR [--anonymize pixelate|blur] [--blocks N] [--blur-radius R] [--draw-format png|jpg] [--no-outline]]
        [--best-shots DIR [--chip-size N] [--chip-margin F] [--chip-format png|jpg]]
        [--device-jpeg-encode] [--jpeg-quality Q]

The images directly under DIR (.jpg .jpeg .png .bmp), sorted by name, are the frames of ONE sequence and must all have the
same size.  They are detected in chunks of --max-frames: without --tiled each frame is resized whole to the network's input,
with --tiled `TiledDetector` also runs the --tile windows.  `tracking.FaceTracker` carries its state from chunk to chunk.
FILE receives one line per emitted track and frame, `frame,id,x,y,w,h,score,-1,-1,-1` with frames counted from 1 and the box
in source pixels.  `--draw DIR` writes every frame with the TRACKER's boxes rendered into it (`render.render_detections`), so
with `--anonymize pixelate` a face the detector misses for up to --emit-misses frames stays covered; with `--motion
constant_velocity` the missed track moves on at its estimated velocity, so that also holds for a face that moves, and
`--coast-grow` widens the covered box frame by frame while it is missed (`tracking.FaceTracker`).  The model options are
those of `detect_images`.  `--best-shots DIR` writes one picture per track, `DIR/seq0_track<id>.png`: the sharpest
`--chip-size` x `--chip-size` crop (112) among the frames in which the detector saw the track, cut with `--chip-margin` (0.25)
and kept on the device from chunk to chunk (`chips.BestShots`).  `--refine` is for a finished recording: a
first pass detects and tracks every chunk and logs it (`tracking.TrackLog`), `tracking.refine_tracks` then looks at the whole
sequence once (back-fill for --lookback frames before a track's first detection, growing by --coast-grow; interpolated gaps;
fragments within --stitch-gap frames overlapping by more than --stitch-iou stitched into one id; chains of fewer than
--min-length detections dropped), and a second pass over the chunks writes FILE and --draw from the refined rows, so a face
is also covered before the detector first found it.  --best-shots still goes by the online ids.  Files only: there is no camera or video-container input.
"""
import argparse
import os
from pathlib import Path

from .detect_images import (EXTENSIONS, add_chip_arguments, add_draw_arguments, add_jpeg_encode_arguments, add_model_arguments,
                            add_tile_arguments, check_chip_arguments, check_draw_arguments, check_jpeg_encode_arguments,
                            jpeg_encode_options)


def frame_paths(root):
    """The frames of DIR in name order."""
    return sorted((p for p in Path(root).iterdir() if p.is_file() and p.suffix.lower() in EXTENSIONS), key=lambda p: p.name)


def frame_size(paths):
    """(w, h) shared by every file (read from the headers), or ValueError naming the first that differs."""
    from PIL import Image
    first = None
    for p in paths:
        with Image.open(p) as im:
            size = im.size
        if first is None:
            first = size
        elif size != first:
            raise ValueError(f"{p.name} is {size[0]}x{size[1]}, {paths[0].name} is {first[0]}x{first[1]}")
    return first


def write_mot(f, first_frame, rows, counts, ids) -> int:
    """Append the tracks of consecutive frames (host arrays) to the open text file; first_frame counts from 1."""
    n = 0
    for t in range(len(counts)):
        for k in range(int(counts[t])):
            s, x, y, w, h = rows[t, k].tolist()
            f.write(f"{first_frame + t},{int(ids[t, k])},{x:.0f},{y:.0f},{w:.0f},{h:.0f},{s:.4f},-1,-1,-1\n")
            n += 1
    return n


def main(argv=None):
    """Parse and check the options (the frames' sizes included), then `run` them."""
    ap = argparse.ArgumentParser()
    add_model_arguments(ap)
    ap.add_argument("--frames", required=True, metavar="DIR")
    ap.add_argument("--out", required=True)
    ap.add_argument("--tiled", action="store_true", help="also run the --tile windows of every frame (TiledDetector)")
    add_tile_arguments(ap)
    ap.add_argument("--max-frames", type=int, default=256, help="frames per detection chunk")
    ap.add_argument("--iou", type=float, default=0.3, help="least overlap of a track and a detection")
    ap.add_argument("--alpha", type=float, default=0.5, help="weight of the new detection in a track's box")
    ap.add_argument("--max-misses", type=int, default=5)
    ap.add_argument("--min-hits", type=int, default=2)
    ap.add_argument("--emit-misses", type=int, default=None, help="frames a missed track is still emitted (--max-misses)")
    ap.add_argument("--birth-score", type=float, default=0.0)
    ap.add_argument("--motion", choices=["constant_velocity"], default=None, help="motion model of the tracks (none)")
    ap.add_argument("--motion-beta", type=float, default=0.5, help="gain of the velocity update, 0..1")
    ap.add_argument("--motion-damping", type=float, default=1.0, help="velocity a missed track keeps per frame, 0..1")
    ap.add_argument("--max-speed", type=int, default=64, help="bound on a track's velocity, pixels per frame")
    ap.add_argument("--coast-grow", type=float, default=0.0, help="growth of a missed track's emitted box per frame, 0..1")
    ap.add_argument("--refine", action="store_true", help="second pass over the whole sequence: back-fill, interpolate, stitch ids")
    ap.add_argument("--lookback", type=int, default=5, help="--refine: frames a track is back-filled before its first detection")
    ap.add_argument("--stitch-gap", type=int, default=10, help="--refine: longest gap between two fragments of one id (-1: none)")
    ap.add_argument("--stitch-iou", type=float, default=0.1, help="--refine: least overlap of two fragments of one id")
    ap.add_argument("--min-length", type=int, default=1, help="--refine: detections a chain needs to be kept")
    add_draw_arguments(ap)
    add_chip_arguments(ap, "--best-shots", "also write the sharpest crop of every track under DIR")
    add_jpeg_encode_arguments(ap)
    args = ap.parse_args(argv)
    check_draw_arguments(ap, args)
    check_jpeg_encode_arguments(ap, args)
    check_chip_arguments(ap, args, "--best-shots")
    if args.max_frames < 1:
        ap.error("--max-frames must be >= 1")
    if args.refine and not (0 <= args.lookback <= 1024 and args.stitch_gap <= 65535 and 0.0 <= args.stitch_iou < 1.0 and
                            args.min_length >= 1):
        ap.error("--refine: --lookback must be in 0..1024, --stitch-gap at most 65535, --stitch-iou in [0, 1) and --min-length >= 1")
    if not os.path.isdir(args.frames):
        ap.error(f"--frames: {args.frames} is not a directory")
    args.paths = frame_paths(args.frames)
    if not args.paths:
        ap.error(f"--frames: no image in {args.frames}")
    try:
        args.frame_size = frame_size(args.paths)
    except ValueError as e:
        ap.error(f"--frames: the frames of a sequence must have one size, but {e}")
    return run(args)


def run(args):
    """What `main` does with its parsed options."""
    from .datasets.WIDERFace.annotations import bank_from_files
    from .detect_images import load_model
    from .tiling import TiledDetector
    from .tracking import FaceTracker
    tracker = FaceTracker(1, iou_threshold=args.iou, alpha=args.alpha, max_misses=args.max_misses, min_hits=args.min_hits,
                          emit_misses=args.emit_misses, birth_score=args.birth_score, motion=args.motion, beta=args.motion_beta,
                          damping=args.motion_damping, max_speed=args.max_speed, coast_grow=args.coast_grow)      # checks its options first
    model = load_model(args)
    det = TiledDetector(model, tile_sizes=tuple(args.tile) if args.tiled else (), overlap=args.overlap,
                        include_whole=not (args.tiled and args.no_whole), edge_margin=args.edge_margin,
                        max_out=256)                        # fdet_track_update takes at most 256 valid rows per frame
    best = None
    if getattr(args, "chips_dir", None) is not None:
        from .chips import BestShots
        best = BestShots(1, size=args.chip_size, margin=args.chip_margin)
    paths, lines = args.paths, 0
    out = Path(args.out)
    if out.parent != Path(""):
        out.parent.mkdir(parents=True, exist_ok=True)
    refine = getattr(args, "refine", False)
    log = None
    if refine:
        from .tracking import TrackLog
        log = TrackLog(1)

    def draw(bank, chunk, rows, counts):
        from .render import render_detections, save_images
        drawn = render_detections(bank, rows, counts, outline=not args.no_outline, anonymize=args.anonymize,
                                  blocks=8 if args.blocks is None else args.blocks, blur_radius=args.blur_radius)
        save_images(drawn, [(Path(args.draw) / p.name).with_suffix("." + (args.draw_format or "png")) for p in chunk],
                    **jpeg_encode_options(args))

    with open(out, "w") as f:
        for a in range(0, len(paths), args.max_frames):
            chunk = paths[a:a + args.max_frames]
            bank = bank_from_files(chunk, "cuda")
            rows, counts = det.detect(bank, range(len(bank)))
            res = tracker.update(rows, counts)
            if refine:                                       # the first pass only logs; the text and the pictures come below
                log.append(rows, res)
            elif args.draw is not None:
                draw(bank, chunk, res.rows, res.counts)
            if best is not None:
                best.update(bank, res)
            if not refine:
                lines += write_mot(f, a + 1, res.rows.cpu().numpy(), res.counts.cpu().numpy(), res.ids.cpu().numpy())
        if refine:
            ref = log.refine(lookback=args.lookback, coast_grow=args.coast_grow, stitch_gap=args.stitch_gap,
                             stitch_iou=args.stitch_iou, min_length=args.min_length).tracks      # one sequence: already in file order
            for a in range(0, len(paths), args.max_frames):
                chunk = paths[a:a + args.max_frames]
                rows, counts, ids = (t[a:a + len(chunk)] for t in (ref.rows, ref.counts, ref.ids))
                if args.draw is not None:
                    draw(bank_from_files(chunk, "cuda"), chunk, rows, counts)
                lines += write_mot(f, a + 1, rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy())
            if ref.overflow:
                print(f"--refine: {ref.overflow} rows found no room in their frame's 256")
    if best is not None:
        shots = best.save(args.chips_dir, getattr(args, "chip_format", None) or "png", **jpeg_encode_options(args))
        print(f"{len(shots)} best shots -> {args.chips_dir}" + (f" ({best.overflow} detections of tracks beyond id {best.capacity} left out)"
                                                                if best.overflow else ""))
    snap = tracker.snapshot()
    print(f"{len(paths)} frames, {int(snap['seq']['next_id'][0])} tracks, {lines} lines -> {args.out}")
    return {"frames": len(paths), "tracks": int(snap["seq"]["next_id"][0]), "lines": lines, "dropped": tracker.dropped}


if __name__ == "__main__":
    main()
