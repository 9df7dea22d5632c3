"""Detect faces in image files at their own resolution and write the WIDER Face result text format.

    python -m fdet_amd.detect_images --checkpoint CKPT --images DIR --out FILE [--model poolresnet --filters 128]
        [--tile 480 --overlap 0.25 --no-whole --edge-margin 0 --probability-threshold P --iou-threshold T --precision 16]
        [--flip --vote --min-votes N] [--draw DIR [--anonymize pixelate|blur] [--blocks N] [--blur-radius R] [--draw-format png|jpg] [--no-outline]]
        [--chips DIR [--chip-size N] [--chip-margin F] [--chip-format png|jpg]] [--device-jpeg-encode] [--jpeg-quality Q]
        [--int8 [--calib DIR] [--calib-images N] [--int8-stem {float,integer}]]

The images under DIR (searched recursively: .jpg .jpeg .png .bmp) are decoded with PIL into a device image bank
(`bank_from_files`; `--device-jpeg`: baseline JPEGs are reconstructed on the device instead, with the same bytes), `tiling.TiledDetector` runs the model on overlapping windows of each image (and on the whole image
unless --no-whole) and merges the windows' boxes, and FILE receives, per image: its path relative to DIR, the number of
boxes, then one `x y w h score` line per box in source pixels.  `--pred-dir DIR` additionally writes the per-event directory
the WIDER protocol's tools read (`DIR/<event>/<image>.txt`, `evaluation_wider.write_wider_pred_dir`).
`--flip` runs every window a second time mirrored, `--vote` merges with box voting and `--min-votes N` leaves out boxes that
fewer than N detections agree on.
`--draw DIR` also writes every input image with its boxes rendered into it (`render.render_detections`) to
`DIR/<path relative to --images>` with the suffix replaced by `--draw-format`: blue outlines of the reference's width unless
`--no-outline`, and with `--anonymize pixelate` every box flattened to at most `--blocks` x `--blocks` cells.  The images are
rendered on the device, chunk by chunk, from the bank the detector just read.
`--chips DIR` also writes every detected face as a `--chip-size` x `--chip-size` crop (112) around its box widened by
`--chip-margin` of its longer side (0.25), cut on the device (`chips.extract_chips`), to
`DIR/<path relative to --images without its suffix>_<row>.png` (`--chip-format jpg`: `.jpg`).
Where `--draw-format` or `--chip-format` is jpg, `--jpeg-quality Q` (75) sets the quality and `--device-jpeg-encode` has the
files encoded on the device (`datasets/jpeg.py DeviceJpegEncoder`) instead of by PIL: the same bytes, but only
the compressed scans are copied to the host.
`--int8` (poolresnet) runs the residual trunk post-training-quantised on the integer matrix cores (`quantize.py`, DESIGN.md
5j): the activation scales are calibrated first, with the float model, on the first `--calib-images` images (32) under
`--calib DIR` (default: the input images), each resized whole to the model resolution.  `--int8-stem integer` gives the
int8 model the integer uint8-frame stem; the default, `float`, keeps the float stem and its bytes.
"""
import argparse
import os
from pathlib import Path

import torch

EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp")


def write_wider_results(path, names, rows, counts) -> None:
    """names: n strings; rows (n,K,5) [score,x,y,w,h]; counts (n,) -> the WIDER result text format."""
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    with open(path, "w") as f:
        for i, name in enumerate(names):
            k = int(counts[i])
            f.write(f"{name}\n{k}\n")
            for s, x, y, w, h in rows[i, :k].tolist():
                f.write(f"{x:.0f} {y:.0f} {w:.0f} {h:.0f} {s:.4f}\n")


def add_model_arguments(ap) -> None:
    """The options that choose and load the network (shared with track_frames)."""
    ap.add_argument("--model", choices=("poolresnet", "resnet", "separablecnn", "ssd"), default="poolresnet")
    ap.add_argument("--filters", type=int, default=None, help="default: 128 (poolresnet, separablecnn), 64 (resnet), 16 (ssd)")
    ap.add_argument("--patches", type=int, default=None, help="default: 10 (poolresnet), 15 (resnet); separablecnn fixes 16")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--precision", type=int, choices=(32, 16), default=32)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--probability-threshold", type=float, default=0.5)
    ap.add_argument("--iou-threshold", type=float, default=0.5)


def add_int8_arguments(ap) -> None:
    """--int8 and the calibration options that need it (shared with run_validation_epoch); `check_int8_arguments` checks them."""
    ap.add_argument("--int8", action="store_true", help="poolresnet: run the residual trunk in int8 (post-training quantisation)")
    ap.add_argument("--calib", default=None, metavar="DIR", help="with --int8: calibration images (default: the first input images)")
    ap.add_argument("--calib-images", type=int, default=None, help="with --int8: number of calibration images (32)")
    ap.add_argument("--int8-stem", choices=("float", "integer"), default=None,
                    help="with --int8: the stem of the int8 model, float (default) or the integer uint8-frame kernel")


def check_int8_arguments(ap, args) -> None:
    if not args.int8:
        for flag, given in (("--calib", args.calib is not None), ("--calib-images", args.calib_images is not None),
                            ("--int8-stem", args.int8_stem is not None)):
            if given:
                ap.error(f"{flag} needs --int8")
        args.int8_stem = "float"
        return
    if args.precision == 16:
        ap.error("--int8 and --precision 16 are two arithmetic modes of the same convolutions: choose one")
    if args.model != "poolresnet":
        ap.error("--int8 covers --model poolresnet only")
    if args.calib_images is not None and args.calib_images < 1:
        ap.error("--calib-images must be >= 1")
    args.calib_images = 32 if args.calib_images is None else args.calib_images
    args.int8_stem = "float" if args.int8_stem is None else args.int8_stem


def image_paths(root):
    root = Path(root)
    return sorted(p for p in root.rglob("*") if p.suffix.lower() in EXTENSIONS)


def quantize_loaded_model(model, args, default_bank=None, decoder="pil", huffman="host"):
    """--int8: calibrate `model` on the images under --calib (or on `default_bank`) and return its Int8PoolResnet."""
    from .quantize import Int8PoolResnet, bank_frames, calibrate
    bank = default_bank
    if args.calib is not None:
        from .datasets.WIDERFace.annotations import bank_from_files
        paths = image_paths(args.calib)[:args.calib_images]
        if not paths:
            raise SystemExit(f"no image under {args.calib}")
        bank = bank_from_files(paths, "cuda", decoder=decoder, huffman=huffman)
    qp = calibrate(model, bank_frames(bank, model.input_shape[1:], args.calib_images))
    print(f"int8: calibrated on {qp.images_seen} images ({qp.method})")
    return Int8PoolResnet(model, qp, stem=getattr(args, "int8_stem", None) or "float")


def add_tile_arguments(ap) -> None:
    """The options of `TiledDetector`'s windows (shared with track_frames)."""
    ap.add_argument("--tile", type=int, nargs="*", default=[480], help="tile side(s) in source pixels; none: whole image only")
    ap.add_argument("--overlap", type=float, default=0.25)
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--edge-margin", type=float, default=0.0)


def add_draw_arguments(ap) -> None:
    """--draw and the options that need it (shared with track_frames); `check_draw_arguments` checks them."""
    ap.add_argument("--draw", default=None, metavar="DIR", help="also write every image, rendered, under DIR")
    ap.add_argument("--anonymize", choices=("pixelate", "blur"), default=None, help="with --draw: pixelate or Gaussian-blur every box")
    ap.add_argument("--blocks", type=int, default=None,
                    help="with --draw --anonymize: cells along the longer side of a box; blur: radius = longer side / N (8)")
    ap.add_argument("--blur-radius", type=float, default=None, help="with --anonymize blur: one fixed radius for every box")
    ap.add_argument("--draw-format", choices=("png", "jpg"), default=None, help="with --draw: the files' format (png)")
    ap.add_argument("--no-outline", action="store_true", help="with --draw: no outlines")


def check_draw_arguments(ap, args) -> None:
    if args.draw is None:
        for flag, given in (("--anonymize", args.anonymize is not None), ("--blocks", args.blocks is not None),
                            ("--draw-format", args.draw_format is not None), ("--no-outline", args.no_outline)):
            if given:
                ap.error(f"{flag} needs --draw")
    if args.blocks is not None and args.blocks < 1:
        ap.error("--blocks must be >= 1")
    if args.blur_radius is not None:
        if args.anonymize != "blur":
            ap.error("--blur-radius needs --anonymize blur")
        if not 0 <= args.blur_radius <= 4096:
            ap.error("--blur-radius must be in 0..4096")


def add_chip_arguments(ap, flag, what) -> None:
    """`flag` DIR and the chip options that need it (shared with track_frames); `check_chip_arguments` checks them."""
    ap.add_argument(flag, dest="chips_dir", default=None, metavar="DIR", help=what)
    ap.add_argument("--chip-size", type=int, default=None, help=f"with {flag}: side of a chip in pixels, 8..256 (112)")
    ap.add_argument("--chip-margin", type=float, default=None, help=f"with {flag}: margin as a share of the box's longer side, 0..1 (0.25)")
    ap.add_argument("--chip-format", choices=("png", "jpg"), default=None, help=f"with {flag}: the files' format (png)")


def check_chip_arguments(ap, args, flag) -> None:
    if args.chips_dir is None:
        for name, given in (("--chip-size", args.chip_size is not None), ("--chip-margin", args.chip_margin is not None),
                            ("--chip-format", args.chip_format is not None)):
            if given:
                ap.error(f"{name} needs {flag}")
    if args.chip_size is not None and not 8 <= args.chip_size <= 256:
        ap.error("--chip-size must be in 8..256")
    if args.chip_margin is not None and not 0.0 <= args.chip_margin <= 1.0:
        ap.error("--chip-margin must be in 0..1")
    args.chip_size = 112 if args.chip_size is None else args.chip_size
    args.chip_margin = 0.25 if args.chip_margin is None else args.chip_margin


def add_jpeg_encode_arguments(ap) -> None:
    """How the JPEG files of --draw-format jpg / --chip-format jpg are written (shared with track_frames)."""
    ap.add_argument("--device-jpeg-encode", action="store_true",
                    help="write JPEG files with the device encoder (datasets/jpeg.py) instead of PIL; same bytes")
    ap.add_argument("--jpeg-quality", type=int, default=None, help="quality of the JPEG files written, 1..100 (75)")


def check_jpeg_encode_arguments(ap, args) -> None:
    if args.draw_format != "jpg" and args.chip_format != "jpg":
        for flag, given in (("--device-jpeg-encode", args.device_jpeg_encode), ("--jpeg-quality", args.jpeg_quality is not None)):
            if given:
                ap.error(f"{flag} needs --draw-format jpg or --chip-format jpg")
    if args.jpeg_quality is not None and not 1 <= args.jpeg_quality <= 100:
        ap.error("--jpeg-quality must be in 1..100")


def jpeg_encode_options(args) -> dict:
    """`render.save_images`' encoder options out of the parsed arguments."""
    quality = getattr(args, "jpeg_quality", None)
    return {"encoder": "device" if getattr(args, "device_jpeg_encode", False) else "pil", "quality": 75 if quality is None else quality}


def main(argv=None):
    """Parse and check the options, then `run` them."""
    ap = argparse.ArgumentParser()
    add_model_arguments(ap)
    ap.add_argument("--images", required=True)
    ap.add_argument("--out", required=True)
    add_tile_arguments(ap)
    ap.add_argument("--pred-dir", default=None, help="also write DIR/<event>/<image>.txt, the WIDER protocol's layout")
    ap.add_argument("--batch-images", type=int, default=64, help="source images per detect() call")
    ap.add_argument("--device-jpeg", action="store_true",
                    help="decode baseline JPEGs with the device decoder (datasets/jpeg.py) instead of PIL; same bytes")
    ap.add_argument("--device-jpeg-huffman", action="store_true",
                    help="--device-jpeg: Huffman-decode on the device too, so that only the file bytes cross to it")
    ap.add_argument("--flip", action="store_true", help="every window a second time, mirrored left to right")
    ap.add_argument("--vote", action="store_true", help="box voting: a kept box is the score-weighted mean of its cluster")
    ap.add_argument("--min-votes", type=int, default=1, help="with --vote: leave out boxes with fewer members than this")
    add_draw_arguments(ap)
    add_chip_arguments(ap, "--chips", "also write every detected face as a square crop under DIR")
    add_jpeg_encode_arguments(ap)
    add_int8_arguments(ap)
    args = ap.parse_args(argv)
    check_int8_arguments(ap, args)
    check_draw_arguments(ap, args)
    check_jpeg_encode_arguments(ap, args)
    check_chip_arguments(ap, args, "--chips")
    if args.device_jpeg_huffman and not args.device_jpeg:
        ap.error("--device-jpeg-huffman needs --device-jpeg")
    if args.min_votes < 1:
        ap.error("--min-votes must be >= 1")
    if args.min_votes > 1 and not args.vote:
        ap.error("--min-votes above 1 needs --vote")
    return run(args)


def load_model(args):
    """The network the model options describe, on the GPU, in eval mode, with the checkpoint loaded."""
    from .run_validation_epoch import load_checkpoint
    shape = (3, args.size, args.size)
    kw = dict(probability_threshold=args.probability_threshold, iou_threshold=args.iou_threshold)
    if args.model == "ssd":
        from .models.ModelMetaSSD import ModelMetaSSD as Meta
        from .models.SSD import SSD
        model = SSD(filters=args.filters or 16, input_shape=shape, **kw).cuda()
    else:
        from .models import ModelMeta as Meta
        if args.model == "poolresnet":
            from .models.PoolResnet import PoolResnet
            model = PoolResnet(filters=args.filters or 128, input_shape=shape, num_of_patches=args.patches or 10,
                               num_of_residual_blocks=10, **kw).cuda()
        elif args.model == "separablecnn":
            from .models.SeparableCNN import SeparableCNN
            model = SeparableCNN(filters=args.filters or 128, input_shape=shape, **SeparableCNN.coherent_head(args.size), **kw).cuda()
        else:
            from .models.Resnet import Resnet
            model = Resnet(filters=args.filters or 64, input_shape=shape, num_of_patches=args.patches or 15, **kw).cuda()
    if args.precision == 16:
        model.engine.set_precision("bf16")
    if args.checkpoint:
        log_path = Path("logs/out_detect_images.log")
        log_path.parent.mkdir(parents=True, exist_ok=True)
        load_checkpoint(Meta(model=model, lr=1e-4, log_path=log_path), args.checkpoint)
    return model.eval()


def run(args):
    """What `main` does with its parsed options."""
    from .datasets.WIDERFace.annotations import bank_from_files
    from .tiling import TiledDetector
    root = Path(args.images)
    paths = image_paths(root)
    if not paths:                                   # before the model is built: nothing to detect in needs no GPU to say so
        raise SystemExit(f"no image under {root}")
    model = load_model(args)
    huffman = "device" if getattr(args, "device_jpeg_huffman", False) else "host"
    if getattr(args, "int8", False):
        decoder = "device" if args.device_jpeg else "pil"
        first = None if args.calib is not None else bank_from_files(paths[:args.calib_images], "cuda", decoder=decoder, huffman=huffman)
        model = quantize_loaded_model(model, args, first, decoder, huffman)
    det = TiledDetector(model, tile_sizes=tuple(args.tile), overlap=args.overlap, include_whole=not args.no_whole,
                        edge_margin=args.edge_margin, flip=args.flip, vote=args.vote, min_votes=args.min_votes)
    names, all_rows, all_counts = [], [], []
    for a in range(0, len(paths), args.batch_images):
        chunk = paths[a:a + args.batch_images]
        bank = bank_from_files(chunk, "cuda", decoder="device" if args.device_jpeg else "pil", huffman=huffman)
        rows, counts = det.detect(bank, range(len(bank)))
        if args.draw is not None:
            from .render import render_detections, save_images
            drawn = render_detections(bank, rows, counts, outline=not args.no_outline, anonymize=args.anonymize,
                                      blocks=8 if args.blocks is None else args.blocks, blur_radius=args.blur_radius)
            save_images(drawn, [(Path(args.draw) / os.path.relpath(p, root)).with_suffix("." + (args.draw_format or "png"))
                                for p in chunk], **jpeg_encode_options(args))
        if getattr(args, "chips_dir", None) is not None:
            from .chips import extract_chips
            from .render import save_images
            cs = extract_chips(bank, rows, counts, size=args.chip_size, margin=args.chip_margin)
            stems = [(Path(args.chips_dir) / os.path.relpath(p, root)).with_suffix("") for p in chunk]
            if len(cs):
                ext = getattr(args, "chip_format", None) or "png"
                save_images(cs.as_bank(), [f"{stems[i]}_{j}.{ext}" for i in range(len(chunk)) for j in range(int(cs.offset[i + 1] - cs.offset[i]))],
                            **jpeg_encode_options(args))
        kmax = max(int(counts.max()), 1)
        all_rows.append(rows[:, :kmax].cpu())
        all_counts.append(counts.cpu())
        names += [os.path.relpath(p, root) for p in chunk]
    kmax = max(r.shape[1] for r in all_rows)
    rows = torch.cat([torch.nn.functional.pad(r, (0, 0, 0, kmax - r.shape[1])) for r in all_rows])
    counts = torch.cat(all_counts)
    write_wider_results(args.out, names, rows, counts)
    if args.pred_dir:
        from .evaluation_wider import write_wider_pred_dir
        write_wider_pred_dir(args.pred_dir, names, rows, counts)
    print(f"{len(names)} images, {int(counts.sum())} boxes -> {args.out}")
    return {"names": names, "rows": rows, "counts": counts}


if __name__ == "__main__":
    main()
