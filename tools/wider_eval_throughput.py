"""Cost of the WIDER protocol evaluation kernel beside the VOC-rule kernel, at B=256.

    python tools/wider_eval_throughput.py [--batch 256] [--launches 30] [--warmup 5] [--epochs 5] [--out profiles/r09_wider_eval.json]

Two measurements, written as one JSON document:
  (a) `fdet_eval_wider` (3 subsets, 1000 thresholds) and `fdet_eval_match` (1 IoU threshold, 1000 bins) on the same random
      batches at the three shapes of tools/eval_throughput.py (YOLO S=10 / S=15, the SSD prior count): launches alternated in
      one process, each timed on its own with device events after a warm-up; median, min and max per kernel;
  (b) the wall time of one validation epoch (PoolResnet F=64, batch 256, device batches) with `DetectionEvaluator` alone and
      with the `WiderEvaluator` fed beside it the way `run_validation_epoch --wider-gt` does, compute() included.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--val-batches", type=int, default=4)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    import wider_cpu_ref as R
    from fdet_amd import evaluation as E, evaluation_wider as W, hotpath as hp
    from fdet_amd import run_validation_epoch as V
    from fdet_amd.datasets import augment as A
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.trainer import _epoch
    if not torch.cuda.is_available():
        raise SystemExit("wider_eval_throughput needs a GPU")
    B = args.batch
    res = {"tool": "wider_eval_throughput", "batch": B, "device": torch.cuda.get_device_name(0)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def stats(ts):
        return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2), "launches": len(ts)}

    # (a) the two kernels, launches alternated
    rng = np.random.default_rng(0)
    kern = {}
    for name, Kmax, max_det in (("yolo_s10", 100, 30), ("yolo_s15", 225, 60), ("ssd_4774", 4774, 300)):
        pred, counts, rows, offs, masks = R.random_batch(rng, B, Kmax, max_det, 5, 3)
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pred, counts, rows, offs, masks.view(np.int32))]
        voc, wid = hp.EvalState((0.5,), 1000), hp.WiderState(3, 0.5, 1000)
        f_voc = lambda: hp.eval_match(d[0], d[1], d[2], d[3], voc)                       # noqa: E731
        f_wid = lambda: hp.eval_wider(d[0], d[1], d[2], d[3], d[4], wid)                 # noqa: E731
        for _ in range(args.warmup):
            f_voc(), f_wid()
        torch.cuda.synchronize()
        t_voc, t_wid = [], []
        for _ in range(args.launches):
            t_voc.append(timed(f_voc))
            t_wid.append(timed(f_wid))
        kern[name] = {"Kmax": Kmax, "mean_detections": float(counts.mean()), "fdet_eval_match_T1": stats(t_voc),
                      "fdet_eval_wider_S3": stats(t_wid)}
    res["a_kernels"] = kern

    # (b) one validation epoch with the VOC evaluator alone and with the WIDER evaluator beside it
    torch.manual_seed(0)
    model = PoolResnet(args.filters, (3, 480, 480), 10).cuda()
    mm = ModelMeta(model=model, lr=1e-4, log_path=os.devnull)
    n = B * args.val_batches
    bank, boxes = A.synthetic_bank(n, "cuda", seed=2, max_side=700)
    val = A.DeviceBatches(bank, boxes, B, A.default_transform((480, 480)), 10, shuffle=False)
    masks = [np.where(np.minimum(b[:, 3], b[:, 4]) >= 60, 7, np.where(np.minimum(b[:, 3], b[:, 4]) >= 25, 6, 4)).astype(np.uint32)
             for b in boxes]
    subsets = W.WiderSubsets.from_masks(masks)
    gt = A.DeviceBoxes(boxes, "cuda")
    ev = E.DetectionEvaluator()

    def epoch(with_wider):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.reset()
        both = V._WithWider(ev, W.WiderEvaluator(), subsets, gt, bank, (480, 480)) if with_wider else None
        outs = _epoch(mm, val, False, {}, None, both or ev)
        float(outs[-1]["loss"])
        ev.compute()
        if both is not None:
            both.wider.compute()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    epoch(False), epoch(True)                              # warm up both paths
    voc_only = [epoch(False) for _ in range(args.epochs)]
    with_wider = [epoch(True) for _ in range(args.epochs)]
    res["b_validation_epoch_ms"] = {
        "val_batches": args.val_batches, "filters": args.filters, "images": n,
        "detection_evaluator": [round(t, 2) for t in voc_only], "with_wider_evaluator": [round(t, 2) for t in with_wider],
        "detection_evaluator_median": round(statistics.median(voc_only), 2), "with_wider_median": round(statistics.median(with_wider), 2),
        "detection_evaluator_spread": round(max(voc_only) - min(voc_only), 2)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
