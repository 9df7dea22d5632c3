"""Throughput of the on-device augmentation: device image bank -> (x, y) at B=256, timed with device events after a warm-up.

    python tools/augment_throughput.py [--batch 256] [--steps 20] [--warmup 5] [--transform training|default]

Sources are seeded synthetic images of WIDER-like size (~1024x700, ragged), the output 480x480, targets the YOLO S=10
encode.  Prints one JSON line: ms per batch, images/s and the achieved bytes/s against the HBM traffic the shapes imply
(source bytes of the batch read once, the uint8 intermediate written and read back, the uint8 frame and the fp32 image
written).  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bank", type=int, default=512)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--transform", choices=("training", "default"), default="training")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets import augment as A
    if not torch.cuda.is_available():
        raise SystemExit("augment_throughput needs a GPU")
    g = np.random.default_rng(0)
    imgs, boxes = [], []
    for _ in range(args.bank):
        H, W = int(g.integers(640, 760)), int(g.integers(960, 1088))
        base = g.integers(0, 256, (H // 8 + 2, W // 8 + 2, 3), dtype=np.uint8)
        imgs.append(np.ascontiguousarray(np.repeat(np.repeat(base, 8, 0), 8, 1)[:H, :W]))
        boxes.append(np.array([[1, W // 4, H // 4, 64, 80]], np.float32))
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    shape = (args.size, args.size)
    t = A.training_transform(shape, seed=1) if args.transform == "training" else A.default_transform(shape)
    batches = A.DeviceBatches(bank, boxes, args.batch, t, 10, seed=0)
    nb = len(batches)

    def run(n):
        done = 0
        while done < n:
            for x, y, _ in batches:
                done += 1
                if done == n:
                    break
        return x

    run(args.warmup)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(args.steps)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    B, px = args.batch, args.size * args.size
    src = float(bank.nbytes) / len(bank) * B             # mean source bytes of a batch
    traffic = src + B * 3 * px * (1 + 1 + 1 + 4)        # sources, mid write + read, u8 frame, fp32 image
    print(json.dumps({"tool": "augment_throughput", "transform": args.transform, "batch": B, "size": args.size,
                      "bank_images": len(bank), "batches_per_epoch": nb, "ms_per_batch": round(ms, 4),
                      "images_per_s": round(B / ms * 1e3, 1), "bytes_per_batch": int(traffic),
                      "achieved_GB_per_s": round(traffic / ms / 1e6, 1)}))


if __name__ == "__main__":
    main()
