"""Counterpart of the reference's run_validation_epoch.py: load a checkpoint, run one validation epoch, print the metrics.

    python -m fdet_amd.run_validation_epoch --model poolresnet --filters 64 --checkpoint last.ckpt --json curve.json

The reference prints the averaged step metrics (`format_metrics(..., training=False)`); this script prints that line and,
below it, what the whole validation set gives through `evaluation.DetectionEvaluator`: average precision at `--iou`, the
best F1 and the score threshold that reaches it.  `--json PATH` writes the precision/recall curve.

Data: `--wider-root DIR --split val` reads DIR/wider_face_split/wider_face_val_bbx_gt.txt and DIR/WIDER_val/images (decoded
once into a device image bank); without it a seeded synthetic bank stands in, so the script runs anywhere.  `--checkpoint`
takes a Lightning-layout file ({"state_dict": {"model.<name>": tensor}}) or a bare state_dict archive (.pth) of the model
class; without it the freshly initialised model is evaluated.  `--precision 16` runs the convolutions in one bf16 pass.
`--tiled` adds a second report: the same evaluator numbers from `tiling.TiledDetector` on the UNRESIZED bank (windows of
`--tile` source pixels with `--overlap`, plus the whole image unless `--no-whole`) against the source-pixel boxes.
With `--flip`, `--vote` or `--min-votes N` the tiled pass runs with test-time augmentation and its AP lines
name the options that ran.
`--wider-gt DIR` (the directory holding wider_face_val.mat and wider_{easy,medium,hard}_val.mat) adds the Easy / Medium /
Hard AP of the WIDER Face protocol (`evaluation_wider.WiderEvaluator`): the resized pass's detections are taken back to
source pixels, and with `--tiled` the tiled rows are evaluated too.  `--json` then gains the keys "wider" / "wider_tiled".
Images are matched to the .mat files by `<event>/<image>`; the synthetic bank's images are called `synthetic/00000`, ...
`--int8` (poolresnet) adds the same evaluator numbers from the int8 post-training-quantised model (`quantize.py`, DESIGN.md
5j) beside the float ones of the same run: the scales are calibrated with the float model on the first `--calib-images`
images (32) under `--calib DIR` (default: the validation bank's first images).  `--json` then gains the key "int8".
`--int8-stem integer` gives that model the integer uint8-frame stem (the default is `float`).
"""
import argparse
import json
from pathlib import Path

import torch


def load_checkpoint(model_setup, path):
    """Lightning layout, a bare ModelMeta state_dict or a bare model state_dict -> loaded into model_setup (strict)."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
    if not isinstance(sd, dict) or not sd:
        raise ValueError(f"{path}: no state_dict found")
    if all(k.startswith("model.") for k in sd):
        model_setup.load_state_dict(sd)
    else:
        model_setup.model.load_state_dict(sd)
    model_setup.model.engine.mark_params_dirty()


def synthetic_names(n: int):
    """The names the synthetic bank's images go by in `--wider-gt` files."""
    return [f"synthetic/{i:05d}" for i in range(n)]


class _WithWider:
    """What `_epoch` takes as its evaluator: feeds the `DetectionEvaluator` exactly as its own `evaluate_batch` does, and
    the same rows, scaled back to source pixels, to a `WiderEvaluator`.  The batches come in bank order."""

    def __init__(self, ev, wider, subsets, gt, bank, out_hw):
        self.ev, self.wider, self.subsets, self.gt, self.next = ev, wider, subsets, gt, 0
        hw = bank.sizes.astype("float32")
        scale = torch.from_numpy(hw[:, ::-1].copy())                       # (W, H)
        scale = scale / torch.tensor([float(out_hw[1]), float(out_hw[0])], dtype=torch.float32)
        self.scale = scale.to(bank.device)

    @torch.no_grad()
    def evaluate_batch(self, model, y_hat, gt):
        rows, counts = self.ev.reducer_for(model).forward_batch(y_hat.detach())
        self.ev.update(rows, counts, gt)
        idx = list(range(self.next, self.next + int(rows.shape[0])))
        self.next = idx[-1] + 1
        self.wider.update(rows, counts, self.subsets.batch(self.gt, idx), scale=self.scale[idx[0]:idx[-1] + 1].contiguous())


def print_wider(r, prefix=""):
    print(f"{prefix}WIDER protocol ({r.n_images} images, {r.n_det} detections, scores normalised by min {r.score_min:.4g} "
          f"range {r.score_range:.4g}): " + ", ".join(f"{k} AP {r.ap[k]:.4f} ({r.n_faces[k]} faces)" for k in r.subset_names))


def tta_label(args) -> str:
    """' [flip, vote, min-votes 2]' for the tiled report lines; empty when none of the three options is set"""
    on = (["flip"] if args.flip else []) + (["vote"] if args.vote else []) + ([f"min-votes {args.min_votes}"] if args.min_votes > 1 else [])
    return f" [{', '.join(on)}]" if on else ""


def main(argv=None):
    """Parse and check the options, then `run` them."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("poolresnet", "resnet", "separablecnn", "ssd"), default="poolresnet")
    ap.add_argument("--filters", type=int, default=None, help="default: 128 (poolresnet, separablecnn), 64 (resnet), 16 (ssd)")
    ap.add_argument("--patches", type=int, default=None, help="default: 10 (poolresnet), 15 (resnet); separablecnn fixes 16")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--precision", type=int, choices=(32, 16), default=32)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--iou", type=float, nargs="+", default=[0.5], help="IoU threshold(s) of a true positive (up to 10)")
    ap.add_argument("--score-floor", type=float, default=0.01)
    ap.add_argument("--wider-root", default=None)
    ap.add_argument("--split", default="val")
    ap.add_argument("--max-faces", type=int, default=None, help="keep images with at most this many faces (reference: 2)")
    ap.add_argument("--max-images", type=int, default=None)
    ap.add_argument("--synthetic-images", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--tiled", action="store_true", help="also evaluate tiled detection on the unresized images")
    ap.add_argument("--tile", type=int, nargs="*", default=[480])
    ap.add_argument("--overlap", type=float, default=0.25)
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--wider-gt", default=None, help="directory of the WIDER protocol's four .mat files: report Easy/Medium/Hard AP")
    ap.add_argument("--device-jpeg", action="store_true",
                    help="--wider-root: decode baseline JPEGs with the device decoder (datasets/jpeg.py) instead of PIL; same bytes")
    ap.add_argument("--device-jpeg-huffman", action="store_true",
                    help="--device-jpeg: Huffman-decode on the device too, so that only the file bytes cross to it")
    ap.add_argument("--flip", action="store_true", help="--tiled: every window a second time, mirrored left to right")
    ap.add_argument("--vote", action="store_true", help="--tiled: box voting instead of plain NMS across windows")
    ap.add_argument("--min-votes", type=int, default=1, help="--tiled --vote: leave out boxes with fewer members than this")
    from .detect_images import add_int8_arguments, check_int8_arguments
    add_int8_arguments(ap)
    args = ap.parse_args(argv)
    check_int8_arguments(ap, args)
    if args.device_jpeg_huffman and not args.device_jpeg:
        ap.error("--device-jpeg-huffman needs --device-jpeg")
    if args.min_votes < 1:
        ap.error("--min-votes must be >= 1")
    if (args.flip or args.vote or args.min_votes > 1) and not args.tiled:
        ap.error("--flip, --vote and --min-votes apply to the tiled pass: add --tiled")
    if args.min_votes > 1 and not args.vote:
        ap.error("--min-votes above 1 needs --vote")
    return run(args)


def run(args):
    """What `main` does with its parsed options."""
    torch.random.manual_seed(0)
    from . import hotpath as hp
    from .datasets.augment import DeviceBatches, default_transform, synthetic_bank
    from .evaluation import DetectionEvaluator
    from .trainer import _epoch
    shape = (3, args.size, args.size)
    if args.model == "ssd":
        from .models.ModelMetaSSD import ModelMetaSSD as Meta
        from .models.SSD import SSD
        model = SSD(filters=args.filters or 16, input_shape=shape).cuda()
        patches, encoder = hp.SSD_PATCH_SIZES, "ssd"
    else:
        from .models import ModelMeta as Meta
        if args.model == "poolresnet":
            from .models.PoolResnet import PoolResnet
            patches = args.patches or 10
            model = PoolResnet(filters=args.filters or 128, input_shape=shape, num_of_patches=patches, num_of_residual_blocks=10).cuda()
        elif args.model == "separablecnn":
            from .models.SeparableCNN import SeparableCNN
            patches = 16                                   # fixed by the model; coherent_head picks the head that reaches it
            model = SeparableCNN(filters=args.filters or 128, input_shape=shape, **SeparableCNN.coherent_head(args.size)).cuda()
        else:
            from .models.Resnet import Resnet
            patches = args.patches or 15
            model = Resnet(filters=args.filters or 64, input_shape=shape, num_of_patches=patches).cuda()
        encoder = "yolo"
    if args.precision == 16:
        model.engine.set_precision("bf16")
    log_path = Path(f"logs/out_{args.model}_single_validate.log")
    log_path.parent.mkdir(parents=True, exist_ok=True)
    model_setup = Meta(model=model, lr=1e-4, log_path=log_path)
    if args.checkpoint:
        load_checkpoint(model_setup, args.checkpoint)
    if args.wider_root:
        from .datasets.WIDERFace.annotations import bank_from_files, read_wider_annotations
        paths, boxes = read_wider_annotations(args.wider_root, args.split, max_faces=args.max_faces, keep_placeholder=False)
        if args.max_images:
            paths, boxes = paths[:args.max_images], boxes[:args.max_images]
        bank = bank_from_files(paths, "cuda", decoder="device" if args.device_jpeg else "pil",
                               huffman="device" if getattr(args, "device_jpeg_huffman", False) else "host")
    else:
        bank, boxes = synthetic_bank(args.synthetic_images, "cuda", seed=2)
    if len(bank) < args.batch_size:
        raise SystemExit(f"{len(bank)} images do not fill one batch of {args.batch_size}")
    val = DeviceBatches(bank, boxes, args.batch_size, default_transform((args.size, args.size)), patches, encoder=encoder,
                        shuffle=False, drop_last=False)
    ev = DetectionEvaluator(iou_thresholds=tuple(args.iou), score_floor=args.score_floor)
    wider = None
    if args.wider_gt:
        from .datasets.augment import DeviceBoxes
        from .evaluation_wider import WiderEvaluator, WiderSubsets
        names = [str(p) for p in paths] if args.wider_root else synthetic_names(len(bank))
        subsets, wider_boxes = WiderSubsets.from_mat(args.wider_gt, names)
        wider_gt = DeviceBoxes(wider_boxes, "cuda")
        wider = _WithWider(ev, WiderEvaluator(subsets.subset_names), subsets, wider_gt, bank, (args.size, args.size))
    outs = _epoch(model_setup, val, False, {}, None, wider or ev)
    metrics = model_setup.format_metrics(outs, training=False)
    r = ev.compute()
    print(f"iou: {metrics['total_iou']:5.3f}, recall {metrics['total_recall']:5.3f}, precision {metrics['total_precision']:5.3f}, "
          f"f1_score {metrics['f1_score']:5.3f}")
    print(f"{r.n_images} images, {r.n_gt} faces, {r.n_det} detections with score >= {args.score_floor}")
    for t, a in zip(r.iou_thresholds, r.ap_per_threshold):
        print(f"AP@{float(t):.2f}: {a:.4f}")
    print(f"best F1 {r.best_f1:.4f} at score threshold {r.best_threshold:.3f}; at the model's threshold "
          f"{model.probability_threshold}: {r.at(model.probability_threshold)}")
    out = {"metrics": metrics, "result": r}
    doc = r.to_json()
    if getattr(args, "int8", False):
        out["int8"] = int8_report(model, val, bank, args, r)
        doc["int8"] = out["int8"].to_json()
    if wider is not None:
        out["wider"] = wider.wider.compute()
        print_wider(out["wider"])
        doc["wider"] = out["wider"].to_json()
    if args.tiled:
        tiled_wider = None
        if wider is not None:
            tiled_wider = (WiderEvaluator(subsets.subset_names), subsets, wider_gt)
        out["tiled"] = tiled_report(model, bank, boxes, args, tiled_wider)
        if tiled_wider is not None:
            out["wider_tiled"] = tiled_wider[0].compute()
            print_wider(out["wider_tiled"], f"tiled{tta_label(args)} ")
            doc["wider_tiled"] = out["wider_tiled"].to_json()
    if args.json:
        Path(args.json).write_text(json.dumps(doc))
    return out


def int8_report(model, val, bank, args, float_result):
    """The evaluator's numbers of the int8 model on the same batches, printed beside the float ones."""
    from .detect_images import quantize_loaded_model
    from .evaluation import DetectionEvaluator
    m8 = quantize_loaded_model(model.eval(), args, bank, "device" if args.device_jpeg else "pil",
                               "device" if getattr(args, "device_jpeg_huffman", False) else "host")
    ev = DetectionEvaluator(iou_thresholds=tuple(args.iou), score_floor=args.score_floor)
    with torch.no_grad():
        for x, _, gt in val:
            ev.evaluate_batch(m8, m8(x), gt)
    r = ev.compute()
    print(f"int8: {r.n_images} images, {r.n_gt} faces, {r.n_det} detections with score >= {args.score_floor}")
    for t, a8, a in zip(r.iou_thresholds, r.ap_per_threshold, float_result.ap_per_threshold):
        print(f"int8 AP@{float(t):.2f}: {a8:.4f} (float {a:.4f})")
    print(f"int8 best F1 {r.best_f1:.4f} at score threshold {r.best_threshold:.3f} (float {float_result.best_f1:.4f})")
    return r


def tiled_report(model, bank, boxes, args, wider=None):
    """The evaluator's numbers from TiledDetector on the unresized bank against the source-pixel boxes.  `wider`: a
    (WiderEvaluator, WiderSubsets, DeviceBoxes) triple that is fed the same rows."""
    from .datasets.augment import DeviceBoxes
    from .evaluation import DetectionEvaluator
    from .tiling import TiledDetector, boxes_for
    model.eval()
    ev = DetectionEvaluator(iou_thresholds=tuple(args.iou), score_floor=args.score_floor)
    det = TiledDetector(model, tile_sizes=tuple(args.tile), overlap=args.overlap, include_whole=not args.no_whole,
                        reducer=ev.reducer_for(model), flip=args.flip, vote=args.vote, min_votes=args.min_votes)
    gt = DeviceBoxes(boxes, "cuda")
    step = max(1, args.batch_size)
    for a in range(0, len(bank), step):
        idx = list(range(a, min(a + step, len(bank))))
        rows, counts = det.detect(bank, idx)
        ev.update(rows, counts, boxes_for(gt, idx), max_gt=max(gt.max_per_image, 1))
        if wider is not None:
            wider[0].update(rows, counts, wider[1].batch(wider[2], idx))
    r = ev.compute()
    print(f"tiled (tile {list(args.tile)}, overlap {args.overlap}, whole image {not args.no_whole}): {r.n_images} images, "
          f"{r.n_gt} faces, {r.n_det} detections with score >= {args.score_floor}")
    for t, a in zip(r.iou_thresholds, r.ap_per_threshold):
        print(f"tiled AP@{float(t):.2f}{tta_label(args)}: {a:.4f}")
    print(f"tiled best F1 {r.best_f1:.4f} at score threshold {r.best_threshold:.3f}")
    return r


if __name__ == "__main__":
    main()
