"""Counterpart of the reference's train_model.py (27-61): build PoolResnet -> ModelMeta -> fit -> to_torchscript.

The WIDER-Face datamodule of the reference downloads and augments the dataset (out of scope); without
`--data` this script trains on synthetic WIDER-Face-shaped batches (uint8 frames + encoded targets), which
is what there is on a box without network.  `--data DIR` expects `DIR/images_u8.pt` (N,3,H,W uint8) and `DIR/boxes.pt`
(list of (n_i,5) [1,x,y,w,h]) prepared offline.

    python -m fdet_amd.train_model --filters 64 --epochs 2 --batch-size 8 --steps-per-epoch 20 --save model.pt

`--precision 16` is the reference's Trainer(precision=16) (train_model.py:50) with bf16 as the 16-bit type: the conv kernels
run one bf16 MFMA pass (engine.set_precision("bf16")); with the defaults (F=128, S=10, batch 8) that is the reference's
own training recipe.  `--precision 32` (default) keeps the fp32-grade bf16x3 arithmetic.

`--augment` trains instead on a device-resident bank of seeded synthetic images of WIDER-like ragged sizes through the
reference's training_transform (datamodule.py:105-124) run on the GPU (datasets/augment.py); validation uses
default_transform (Resize alone).

`--wider-root DIR` trains on the real dataset the same way: the train and val splits under DIR (wider_face_split/ and
WIDER_{train,val}/images, the reference's filter of at most two faces per image) are decoded once into two device image
banks and go through the same training_transform / default_transform.  `--device-jpeg` decodes them with the device
JPEG decoder (datasets/jpeg.py) instead of PIL; the banks are the same bytes.
"""
import argparse
from pathlib import Path

import torch


def synthetic_loader(n_batches, batch_size, size, S, seed):
    """Re-iterable list of (uint8 frames, encoded targets, boxes) host batches."""
    from .datasets.synthetic import synthetic_boxes
    from .datasets.WIDERFace.dataset import encode_batch
    out = []
    g = torch.Generator().manual_seed(seed)
    for b in range(n_batches):
        x = torch.randint(0, 256, (batch_size, 3, size, size), dtype=torch.uint8, generator=g)
        boxes = synthetic_boxes(batch_size, size, seed=seed * 1000 + b)
        y = encode_batch(boxes, (size, size), S).cpu()          # targets as a DataLoader hands them over: host tensors
        out.append((x, y, boxes))
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("poolresnet", "separablecnn"), default="poolresnet")
    ap.add_argument("--filters", type=int, default=128)          # train_model.py:17
    ap.add_argument("--patches", type=int, default=10, help="poolresnet only; separablecnn fixes its grid at 16")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--epochs", type=int, default=70)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--steps-per-epoch", type=int, default=50)
    ap.add_argument("--val-steps", type=int, default=5)
    ap.add_argument("--save", default=None)
    ap.add_argument("--precision", type=int, choices=(32, 16), default=32)   # train_model.py:50 Trainer(precision=...)
    ap.add_argument("--augment", action="store_true", help="on-device training_transform over a synthetic image bank")
    ap.add_argument("--bank-size", type=int, default=None, help="--augment: images in the bank (default: one epoch's worth)")
    ap.add_argument("--wider-root", default=None, help="train on the WIDER Face tree under DIR (train and val splits)")
    ap.add_argument("--device-jpeg", action="store_true", help="--wider-root: decode the JPEGs with the device decoder, not PIL")
    return ap


def wider_batches(root, split, batch_size, transform, patches, decoder, huffman="host", **kw):
    """DeviceBatches over one split of a WIDER Face tree, filtered as the reference filters it (at most two faces)."""
    from .datasets.augment import DeviceBatches
    from .datasets.WIDERFace.annotations import bank_from_files, read_wider_annotations
    paths, boxes = read_wider_annotations(root, split, max_faces=2)
    if len(paths) < batch_size:
        raise SystemExit(f"{root}: the {split} split holds {len(paths)} images with at most two faces, a batch needs {batch_size}")
    bank = bank_from_files(paths, "cuda", decoder=decoder, huffman=huffman)
    return DeviceBatches(bank, boxes, batch_size, transform, patches, **kw)


def main(argv=None):
    ap = build_parser()
    # not a training option: build_parser() stays the set of options that shape the run
    ap.add_argument("--draw-dir", default=None,
                    help="write {train|validation}_epoch_{E}.png (image 0 of the first batch, predicted boxes) there")
    ap.add_argument("--device-jpeg-huffman", action="store_true",
                    help="--device-jpeg: Huffman-decode on the device too, so that only the file bytes cross to it")
    args = ap.parse_args(argv)
    if args.device_jpeg_huffman and not args.device_jpeg:
        ap.error("--device-jpeg-huffman needs --device-jpeg")
    torch.random.manual_seed(0)                                  # train_model.py:13
    from .models import ModelMeta
    from .models.PoolResnet import PoolResnet
    from .trainer import fit
    if args.model == "separablecnn":
        args.patches = 16                                        # fixed by the model (models/SeparableCNN.py:71)
        if args.save is not None:                                # refuse before training, not after the last epoch
            ap.error("--save writes TorchScript, which is not built for --model separablecnn")
    name = f"custom_{args.model}_{args.filters}_{args.patches}x{args.patches}_{args.size}x{args.size}"
    log_path = Path(f"logs/out_{name}.log")
    log_path.parent.mkdir(parents=True, exist_ok=True)
    log_path.unlink(missing_ok=True)
    if args.model == "separablecnn":
        # the head that gives the 16x16 grid num_of_patches=16 decodes: k=6, p=3 at 480x480, k=1, p=0 at 512x512
        from .models.SeparableCNN import SeparableCNN
        model = SeparableCNN(filters=args.filters, input_shape=(3, args.size, args.size), num_of_residual_blocks=10,
                             **SeparableCNN.coherent_head(args.size)).cuda()
    else:
        model = PoolResnet(filters=args.filters, input_shape=(3, args.size, args.size), num_of_patches=args.patches,
                           num_of_residual_blocks=10).cuda()
    if args.precision == 16:
        model.engine.set_precision("bf16")
    model.summary()
    model_setup = ModelMeta(model=model, lr=args.lr, log_path=log_path)
    if args.wider_root:
        from .datasets.augment import default_transform, training_transform
        shape = (args.size, args.size)
        decoder = "device" if args.device_jpeg else "pil"
        huffman = "device" if args.device_jpeg_huffman else "host"
        train = wider_batches(args.wider_root, "train", args.batch_size, training_transform(shape, seed=1), args.patches, decoder,
                              huffman, seed=1)
        val = wider_batches(args.wider_root, "val", args.batch_size, default_transform(shape), args.patches, decoder,
                            huffman, shuffle=False)
    elif args.augment:
        from .datasets.augment import DeviceBatches, default_transform, synthetic_bank, training_transform
        shape = (args.size, args.size)
        n_train = args.bank_size or args.steps_per_epoch * args.batch_size
        bank, boxes = synthetic_bank(n_train, "cuda", seed=1)
        vbank, vboxes = synthetic_bank(args.val_steps * args.batch_size, "cuda", seed=2)
        train = DeviceBatches(bank, boxes, args.batch_size, training_transform(shape, seed=1), args.patches, seed=1)
        val = DeviceBatches(vbank, vboxes, args.batch_size, default_transform(shape), args.patches, shuffle=False)
    else:
        train = synthetic_loader(args.steps_per_epoch, args.batch_size, args.size, args.patches, seed=1)
        val = synthetic_loader(args.val_steps, args.batch_size, args.size, args.patches, seed=2)
    hist = fit(model_setup, train, val, epochs=args.epochs, torchscript_path=args.save, draw_dir=args.draw_dir)
    print(f"\nfinal training loss {float(hist['train'][-1]['loss']):.3f}")
    return hist


if __name__ == "__main__":
    main()
