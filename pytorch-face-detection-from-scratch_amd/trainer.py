"""`fit()`: the counterpart of `Trainer.fit(model=model_setup, datamodule=dm)` + `to_torchscript` of the reference's
train_model.py:27-61 for this engine -- no Lightning needed.  It drives exactly the pieces the reference's Trainer
drives on a ModelMeta: configure_optimizers (SAMSGD(Adam) + MultiStepLR([40], 0.1)), one optimisation step per
batch, `training_epoch_end`, `validation_step` / `validation_epoch_end` under no_grad, `scheduler.step()` once per
epoch, and at the end `to_torchscript(path)`.

Batches are host tensors as a DataLoader yields them: (x, y, gt_bbxs) with x either uint8 frames (B,3,H,W) -- fed
through `U8BatchFeeder` (pinned staging or the loader's own pinned tensors, copy stream, /255 or bilinear resize on the
device, three slots: the copy of batch i+1 runs under step i) -- or float32 in [0,1]; y the encoded targets (B,5,S,S).  The optimisation step is `fused_train_step` (forward +
YoloLoss + backward + all-reduce + Adam as direct kernel launches); its step outputs (loss, total_iou, total_recall,
total_precision) have the meaning of `ModelMeta.training_step`'s (models/ModelMeta.py:115-227).
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional

import torch

from .datasets.feed import U8BatchFeeder
from .hostinfo import limit_host_threads


def _validation_step_with_output(model_meta, batch, step):
    """`validation_step` as it is, plus the forward output it computed (a forward hook on the wrapped model records it
    for the duration of the call): the evaluator sees the same `y_hat` without a second forward."""
    seen = []
    handle = model_meta.model.register_forward_hook(lambda module, args, output: seen.append(output))
    try:
        out = model_meta.validation_step(batch, step)
    finally:
        handle.remove()
    if len(seen) != 1:
        raise RuntimeError(f"validation_step ran the model {len(seen)} times; the evaluator hook expects exactly one forward")
    return out, seen[0]


def _draw_first(model_meta, x0, y_hat, draw_dir, train: bool) -> None:
    """The reference's side effect of step(batch_idx == 0) (models/ModelMeta.py:144-157): image 0 of the batch with the boxes
    the model predicts for it, as `{train|validation}_epoch_{E}.png` under draw_dir."""
    from .datasets.utils import draw_bbx
    model = model_meta.model
    with torch.no_grad():
        pred = model.non_max_suppression(y_hat[:1].detach())[0]
    draw_bbx(img=x0, bbx=pred, input_shape=model.input_shape,
             save_name=f"{'train' if train else 'validation'}_epoch_{model_meta.current_epoch}", save_dir=str(draw_dir))


def _epoch(model_meta, batches, train: bool, feeder_cache: dict, on_step: Optional[Callable], evaluator=None, draw_dir=None):
    model = model_meta.model
    dev = next(model.parameters()).device
    size = tuple(model.input_shape[1:])
    outs: List[dict] = []
    it = iter(batches)
    pending = None                    # (x_dev, y_dev, token) of the batch whose copy is in flight

    def stage(batch):
        x, y = batch[0], batch[1]
        gt = batch[2] if evaluator is not None and not train and len(batch) > 2 else None
        if x.dtype == torch.uint8 and not x.is_cuda:
            key = (tuple(x.shape), tuple(y.shape))
            fd = feeder_cache.get(key)
            if fd is None:
                fd = feeder_cache[key] = U8BatchFeeder(tuple(x.shape), size, dev, target_shape=tuple(y.shape))
            fd.submit(x, y.float())
            return ("feeder", fd, gt)
        return ("direct", (x.to(dev, non_blocking=True).float(), y.to(dev, non_blocking=True).float()), gt)

    nxt = next(it, None)
    if nxt is not None:
        pending = stage(nxt)
    step = 0
    while pending is not None:
        kind, payload, gt = pending
        if kind == "feeder":
            x_d, y_d, tok = payload.get()
        else:
            (x_d, y_d), tok = payload, None
        # the step of THIS batch is enqueued first; only then is the next batch staged.  Staging may block the host on the
        # slot's previous consumer (feed.py: `free.synchronize()`), and with the step already queued the GPU keeps working
        # through that wait; with 3 slots the reused slot belongs to step i-2, which has normally finished.
        if train:
            model.train()
            lsum, y_hat, tot = model_meta.fused_train_step(x_d, y_d, with_metrics=True)
            out = {"loss": lsum.detach().reshape(()), "total_iou": tot[0], "total_recall": tot[1], "total_precision": tot[2]}
            if draw_dir is not None and step == 0:
                _draw_first(model_meta, x_d[0], y_hat, draw_dir, True)
        else:
            model.eval()
            with torch.no_grad():
                if draw_dir is not None and step == 0:
                    out, y_hat = _validation_step_with_output(model_meta, (x_d, y_d, None), step)
                    _draw_first(model_meta, x_d[0], y_hat, draw_dir, False)
                    if evaluator is not None:
                        if gt is None:
                            raise ValueError("fit(evaluator=...): validation batches must carry their true boxes as batch[2]")
                        evaluator.evaluate_batch(model, y_hat, gt)
                elif evaluator is None:
                    out = model_meta.validation_step((x_d, y_d, None), step)
                else:
                    if gt is None:
                        raise ValueError("fit(evaluator=...): validation batches must carry their true boxes as batch[2]")
                    out, y_hat = _validation_step_with_output(model_meta, (x_d, y_d, None), step)
                    evaluator.evaluate_batch(model, y_hat, gt)
        if tok is not None:
            U8BatchFeeder.release(tok)
        nxt = next(it, None)
        following = stage(nxt) if nxt is not None else None          # the next batch's copy overlaps this step
        outs.append(out)
        if on_step is not None:
            on_step(step, train, out)
        step += 1
        pending = following
    return outs


def fit(model_meta, train_batches: Iterable, val_batches: Optional[Iterable] = None, epochs: int = 1,
        torchscript_path: Optional[str] = None, on_step: Optional[Callable] = None, evaluator=None, draw_dir=None) -> dict:
    """Train `model_meta` (a ModelMeta) for `epochs` passes over `train_batches` (re-iterable), validating on
    `val_batches` after every epoch.  Returns {"train": [per-epoch metrics], "val": [...], "scripted": module or None}.

    `evaluator` (an `evaluation.DetectionEvaluator`): the validation pass also feeds it the forward output of every
    validation step and the batch's true boxes (batch[2]: a GtBoxes or a list of (n,5) tensors); it is reset every epoch and
    hist["val"][e] gains "ap", "best_f1", "best_threshold" (one device-to-host copy per epoch).  Step outputs are unchanged.

    `draw_dir` (a directory, created when missing): image 0 of the first training and of the first validation batch of every
    epoch is written there with the boxes predicted for it, as `train_epoch_{E}.png` / `validation_epoch_{E}.png`, the
    reference's `draw_bbx` side effect (models/ModelMeta.py:144-157), rendered on the device.  None (default): nothing."""
    limit_host_threads()                  # 256 OpenMP workers on a 16-core share stall the thread that feeds the GPU
    optimizers, schedulers = model_meta.configure_optimizers()
    sched = schedulers[0]
    feeder_cache: dict = {}
    hist = {"train": [], "val": [], "scripted": None}
    for epoch in range(epochs):
        model_meta.current_epoch = epoch
        if val_batches is not None:
            # Lightning runs the validation loop inside the training epoch and calls validation_epoch_end first, which is
            # why the reference's training line in the log quotes the validation metrics of the same epoch (ModelMeta.py:268-289)
            pass
        tr = _epoch(model_meta, train_batches, True, feeder_cache, on_step, draw_dir=draw_dir)
        if val_batches is not None:
            if evaluator is not None:
                evaluator.reset()
            va = _epoch(model_meta, val_batches, False, feeder_cache, on_step, evaluator, draw_dir)
            hist["val"].append(model_meta.format_metrics(va, training=False))
            if evaluator is not None:
                r = evaluator.compute()
                hist["val"][-1].update(ap=r.ap, best_f1=r.best_f1, best_threshold=r.best_threshold)
        hist["train"].append(model_meta.format_metrics(tr, training=True))
        sched.step()
    model_meta.model.train()
    if torchscript_path is not None:
        hist["scripted"] = model_meta.to_torchscript(torchscript_path)
    return hist
