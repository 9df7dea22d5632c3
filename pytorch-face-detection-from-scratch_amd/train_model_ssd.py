"""Counterpart of the reference's train_model_ssd.py (10-58): build SSD -> ModelMetaSSD -> fit -> to_torchscript.

As in train_model.py, the WIDER-Face datamodule of the reference (downloads and augments the dataset) is out of scope
(SURVEY.md 8): this script trains on synthetic WIDER-Face-shaped batches -- uint8 frames and their multi-scale SSD targets
(hp.ssd_encode_targets), handed over as host tensors, as a DataLoader would.

    python -m fdet_amd.train_model_ssd --epochs 2 --steps-per-epoch 20 --save ssd.pt

The defaults are the reference's recipe: SSD(filters=16) at 480x480, batch 24, lr 1e-4, 70 epochs.  `--precision 16` is
its Trainer(precision=16) (train_model_ssd.py:46-50) with bf16 as the 16-bit type: every matrix-core layer runs one bf16
MFMA pass (engine.set_precision("bf16"), ssdstack.py).  `--precision 32` (default) keeps the fp32-grade bf16x3 arithmetic.

`--augment` trains instead on a device-resident bank of seeded synthetic images of WIDER-like ragged sizes through
default_transform (Resize alone, datasets/augment.py) with the SSD encoder, as the SSD datamodule does.
"""
import argparse
from pathlib import Path

import torch


def synthetic_loader(n_batches, batch_size, size, seed):
    """Re-iterable list of (uint8 frames, encoded SSD targets (B,4774,5), boxes) host batches."""
    from . import hotpath as hp
    from .datasets.synthetic import synthetic_boxes
    out = []
    g = torch.Generator().manual_seed(seed)
    for b in range(n_batches):
        x = torch.randint(0, 256, (batch_size, 3, size, size), dtype=torch.uint8, generator=g)
        boxes = synthetic_boxes(batch_size, size, seed=seed * 1000 + b)
        y = hp.ssd_encode_targets(boxes, (size, size)).cpu()    # targets as a DataLoader hands them over: host tensors
        out.append((x, y, boxes))
    return out


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=16)           # train_model_ssd.py:14
    ap.add_argument("--size", type=int, default=480)             # train_model_ssd.py:13
    ap.add_argument("--lr", type=float, default=1e-4)            # train_model_ssd.py:15
    ap.add_argument("--epochs", type=int, default=70)            # train_model_ssd.py:48
    ap.add_argument("--batch-size", type=int, default=24)        # train_model_ssd.py:55
    ap.add_argument("--steps-per-epoch", type=int, default=50)
    ap.add_argument("--val-steps", type=int, default=5)
    ap.add_argument("--save", default=None)
    ap.add_argument("--precision", type=int, choices=(32, 16), default=32)   # train_model_ssd.py:49 Trainer(precision=...)
    ap.add_argument("--augment", action="store_true", help="on-device default_transform over a synthetic image bank")
    ap.add_argument("--bank-size", type=int, default=None, help="--augment: images in the bank (default: one epoch's worth)")
    ap.add_argument("--draw-dir", default=None,
                    help="write {train|validation}_epoch_{E}.png (image 0 of the first batch, predicted boxes) there")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    torch.random.manual_seed(0)                                  # train_model_ssd.py:11
    from .models.ModelMetaSSD import ModelMetaSSD
    from .models.SSD import SSD
    from .trainer import fit
    name = f"ssd_{args.filters}_{args.size}x{args.size}_sam_adam"
    log_path = Path(f"logs/out_{name}.log")
    log_path.parent.mkdir(parents=True, exist_ok=True)
    log_path.unlink(missing_ok=True)
    model = SSD(filters=args.filters, input_shape=(3, args.size, args.size)).cuda()
    if args.precision == 16:
        model.engine.set_precision("bf16")
    print(f"SSD: {sum(p.numel() for p in model.parameters()):,} parameters, input {tuple(model.input_shape)}")
    model_setup = ModelMetaSSD(model=model, lr=args.lr, log_path=log_path)
    if args.augment:
        from . import hotpath as hp
        from .datasets.augment import DeviceBatches, default_transform, synthetic_bank
        shape = (args.size, args.size)
        bank, boxes = synthetic_bank(args.bank_size or args.steps_per_epoch * args.batch_size, "cuda", seed=1)
        vbank, vboxes = synthetic_bank(args.val_steps * args.batch_size, "cuda", seed=2)
        train = DeviceBatches(bank, boxes, args.batch_size, default_transform(shape), hp.SSD_PATCH_SIZES, encoder="ssd", seed=1)
        val = DeviceBatches(vbank, vboxes, args.batch_size, default_transform(shape), hp.SSD_PATCH_SIZES, encoder="ssd",
                            shuffle=False)
    else:
        train = synthetic_loader(args.steps_per_epoch, args.batch_size, args.size, seed=1)
        val = synthetic_loader(args.val_steps, args.batch_size, args.size, seed=2)
    hist = fit(model_setup, train, val, epochs=args.epochs, torchscript_path=args.save, draw_dir=args.draw_dir)
    print(f"\nfinal training loss {float(hist['train'][-1]['loss']):.3f}")
    return hist


if __name__ == "__main__":
    main()
