"""Cost of the on-device detection evaluation at B=256.

    python tools/eval_throughput.py [--batch 256] [--launches 30] [--warmup 5] [--epochs 5] [--out profiles/r07_eval.json]

Three measurements, written as one JSON document:
  (a) `fdet_eval_match` alone at the YOLO S=10 / S=15 shapes and the SSD prior count: median of individually timed launches
      (device events) after a warm-up, on random batches of a few boxes per image;
  (b) the wall time of one validation epoch of `fit`'s validation pass (PoolResnet F=64, batch 256, device batches) without
      an evaluator -- which is what the code did before the evaluator existed -- and with one, five runs each, so the added
      cost can be judged against the run-to-run spread of the former;
  (c) the same evaluation the way it had to be done without the kernel: copy `forward_batch`'s output and the boxes to the
      host and run the numpy restatement (tests/eval_cpu_ref.py) per image.
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
    import eval_cpu_ref as R
    from fdet_amd import evaluation as E
    from fdet_amd.datasets import augment as A
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.trainer import _epoch
    if not torch.cuda.is_available():
        raise SystemExit("eval_throughput needs a GPU")
    B = args.batch
    res = {"tool": "eval_throughput", "batch": B, "device": torch.cuda.get_device_name(0)}

    # (a) the kernel alone
    rng = np.random.default_rng(0)
    kern = {}
    for name, Kmax, max_det, thr in (("yolo_s10", 100, 30, (0.5,)), ("yolo_s15", 225, 60, (0.5,)), ("ssd_4774", 4774, 300, (0.5,)),
                                     ("yolo_s10_T10", 100, 30, tuple(0.5 + 0.05 * i for i in range(10)))):
        pred, counts, rows, offs = R.random_batch(rng, B, Kmax, max_det, 5)
        d = [torch.from_numpy(a).cuda() for a in (pred, counts, rows, offs)]
        ev = E.DetectionEvaluator(iou_thresholds=thr)
        for _ in range(args.warmup):
            ev.update(d[0], d[1], (d[2], d[3]))
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ev.update(d[0], d[1], (d[2], d[3]))
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        kern[name] = {"Kmax": Kmax, "T": len(thr), "mean_detections": float(counts.mean()), "median_us": round(statistics.median(ts), 2),
                      "min_us": round(min(ts), 2), "max_us": round(max(ts), 2), "launches": len(ts)}
    res["a_kernel"] = kern

    # (b) one validation epoch with and without the evaluator
    torch.manual_seed(0)
    model = PoolResnet(args.filters, (3, 480, 480), 10).cuda()
    mm = ModelMeta(model=model, lr=1e-4, log_path=os.devnull)
    bank, boxes = A.synthetic_bank(B * args.val_batches, "cuda", seed=2, max_side=700)
    val = A.DeviceBatches(bank, boxes, B, A.default_transform((480, 480)), 10, shuffle=False)
    ev = E.DetectionEvaluator()

    def epoch(evaluator):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if evaluator is not None:
            evaluator.reset()
        outs = _epoch(mm, val, False, {}, None, evaluator)
        float(outs[-1]["loss"])                            # what format_metrics does: the epoch ends on the host
        r = evaluator.compute() if evaluator is not None else None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    epoch(None), epoch(ev)                                 # warm up both paths
    without = [epoch(None)[0] for _ in range(args.epochs)]
    with_ev = [epoch(ev)[0] for _ in range(args.epochs)]
    res["b_validation_epoch_ms"] = {
        "val_batches": args.val_batches, "filters": args.filters,
        "without_evaluator": [round(t, 2) for t in without], "with_evaluator": [round(t, 2) for t in with_ev],
        "without_median": round(statistics.median(without), 2), "with_median": round(statistics.median(with_ev), 2),
        "without_spread": round(max(without) - min(without), 2)}

    # (c) the same evaluation on the host
    model.eval()
    red = ev.reducer_for(model)
    host = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for x, y, gt in val:
                rows, counts = red.forward_batch(model(x))
                R.evaluate(rows.cpu().numpy(), counts.cpu().numpy(), gt.rows.cpu().numpy(), gt.box_offset.cpu().numpy(),
                           ev.iou_thresholds, ev.n_bins)
        host.append((time.perf_counter() - t0) * 1e3)
    dev = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.reset()
        with torch.no_grad():
            for x, y, gt in val:
                ev.evaluate_batch(model, model(x), gt)
        ev.compute()
        dev.append((time.perf_counter() - t0) * 1e3)
    res["c_forward_plus_evaluation_ms"] = {"host_restatement": [round(t, 2) for t in host], "device_evaluator": [round(t, 2) for t in dev]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
