"""The detection evaluator on the GPU: `fdet_eval_match` against the numpy restatement's sequential loop
(tests/eval_cpu_ref.py).  Every comparison is exact: both sides do the same fp32 operations in the same order and the
results are integers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

T1 = (0.5,)
T10 = tuple((np.arange(10, dtype=np.float32) * np.float32(0.05) + np.float32(0.5)).tolist())      # 0.50:0.05:0.95
SSD_PRIORS = 4774


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import evaluation as E, hotpath as hp
    from fdet_amd.datasets import augment as A
    return E, hp, A


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check(batch, thr, n_bins=1000, max_gt=None):
    E, hp, _ = _mods()
    pred, counts, rows, offs = batch
    ev = E.DetectionEvaluator(iou_thresholds=thr, n_bins=n_bins)
    match = ev.update(*_dev(pred, counts)[:2], tuple(_dev(rows, offs)), max_gt=max_gt, want_match=True)
    r = ev.compute()
    htp, hfp, n_gt, m = R.evaluate(pred, counts, rows, offs, ev.iou_thresholds, n_bins)
    assert np.array_equal(r.tp, htp) and np.array_equal(r.fp, hfp)
    assert (r.n_gt, r.n_images, r.n_det) == (n_gt, len(counts), int(counts.sum()))
    assert np.array_equal(match.cpu().numpy(), m)
    return r


@pytest.mark.parametrize("thr", [T1, T10], ids=["T1", "T10"])
@pytest.mark.parametrize("B,Kmax,max_det,max_gt", [(1, 100, 100, 6), (7, 225, 225, 12), (256, 100, 60, 5), (5, 225, 40, 40)],
                         ids=["yolo10-B1", "yolo15-B7", "yolo10-B256", "yolo15-crowded"])
def test_kernel_equals_sequential_restatement_yolo(B, Kmax, max_det, max_gt, thr):
    rng = np.random.default_rng(B * 1000 + Kmax)
    batch = R.random_batch(rng, B, Kmax, max_det, max_gt, empty_det=(B // 2,) if B > 2 else (), empty_gt=(B // 3,) if B > 2 else ())
    r = _check(batch, thr)
    assert r.tp.sum() > 0 and r.fp.sum() > 0


@pytest.mark.parametrize("thr", [T1, T10], ids=["T1", "T10"])
def test_kernel_equals_sequential_restatement_ssd_shape_and_2048_boxes(thr):
    """The SSD prior count as Kmax: one image with every slot used, one with 2048 boxes, one without detections, one
    without boxes."""
    rng = np.random.default_rng(7)
    pred, counts, rows, offs = R.random_batch(rng, 5, SSD_PRIORS, 700, 30, empty_det=(2,), empty_gt=(3,), big=(1, 2048))
    full = R.random_batch(rng, 1, SSD_PRIORS, SSD_PRIORS, 30)
    while full[1][0] < 4000:                                 # (an image that uses most of the slots)
        full = R.random_batch(rng, 1, SSD_PRIORS, SSD_PRIORS, 30)
    pred[4], counts[4] = full[0][0], full[1][0]              # its detections against image 4's boxes
    assert (offs[2] - offs[1]) == 2048 and counts[2] == 0 and offs[4] == offs[3]
    _check((pred, counts, rows, offs), thr, max_gt=2048)


def test_odd_bins_and_scores_outside_the_unit_interval():
    rng = np.random.default_rng(3)
    pred, counts, rows, offs = R.random_batch(rng, 9, 100, 100, 6)
    pred[0, :4, 0] = [1.0, 1.5, -0.25, np.nan]
    pred[1, :2, 0] = [np.inf, -np.inf]
    counts[0], counts[1] = max(counts[0], 4), max(counts[1], 2)
    _check((pred, counts, rows, offs), T1, n_bins=37)
    _check((pred, counts, rows, offs), T10, n_bins=4096)


def test_two_updates_equal_one_on_the_concatenated_batch_and_reset():
    E, hp, _ = _mods()
    rng = np.random.default_rng(21)
    a = R.random_batch(rng, 6, 225, 80, 9)
    b = R.random_batch(rng, 11, 225, 80, 9)
    ev = E.DetectionEvaluator(iou_thresholds=T10)
    for pred, counts, rows, offs in (a, b):
        ev.update(*_dev(pred, counts), tuple(_dev(rows, offs)))
    two = ev.compute()
    na = int(a[3][-1])
    rows = np.concatenate([a[2][:na], b[2]], 0)
    offs = np.concatenate([a[3], b[3][1:] + na]).astype(np.int32)
    ev2 = E.DetectionEvaluator(iou_thresholds=T10)
    ev2.update(*_dev(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), tuple(_dev(rows, offs)))
    one = ev2.compute()
    assert np.array_equal(one.tp, two.tp) and np.array_equal(one.fp, two.fp)
    assert (one.n_gt, one.n_images, one.n_det) == (two.n_gt, two.n_images, two.n_det) and one.n_images == 17
    assert one.ap_per_threshold.tolist() == two.ap_per_threshold.tolist()
    ev.reset()
    z = ev.compute()
    assert z.tp.sum() == 0 and z.fp.sum() == 0 and (z.n_gt, z.n_images, z.n_det) == (0, 0, 0)
    # the reference's list-of-tensors form packs to the same thing
    ev.update(*_dev(a[0], a[1]), [torch.from_numpy(a[2][a[3][i]:a[3][i + 1]]) for i in range(6)])
    ev3 = E.DetectionEvaluator(iou_thresholds=T10)
    ev3.update(*_dev(a[0], a[1]), tuple(_dev(a[2], a[3])))
    assert np.array_equal(ev.compute().tp, ev3.compute().tp) and np.array_equal(ev.compute().fp, ev3.compute().fp)
    # merge on the device
    ev3.merge(ev)
    assert np.array_equal(ev3.compute().tp, 2 * ev.compute().tp) and ev3.compute().n_gt == 2 * ev.compute().n_gt


def test_unsupported_sizes_are_errors_not_truncation():
    E, hp, _ = _mods()
    from fdet_amd import FdetError
    rng = np.random.default_rng(2)
    pred, counts, rows, offs = R.random_batch(rng, 4, 100, 50, 8, big=(1, 40))
    d = _dev(pred, counts, rows, offs)
    with pytest.raises(ValueError):
        hp.eval_match(torch.zeros(1, 4865, 5, device="cuda"), d[1][:1], d[2], d[3][:2], hp.EvalState())
    with pytest.raises(ValueError):
        hp.eval_match(d[0], d[1], d[2], d[3], hp.EvalState(), max_gt=4097)
    L = hp.lib()
    st = hp.EvalState()
    rc = L.fdet_eval_match(d[0].data_ptr(), d[1].data_ptr(), 4, 100, d[2].data_ptr(), d[3].data_ptr(), d[2].shape[0], 8,
                           st._thr_c, 11, 1000, st.hist[0].data_ptr(), st.hist[1].data_ptr(), st.counters.data_ptr(), None, None)
    assert rc == -1 and b"thresholds" in L.fdet_last_error()
    # an image with more boxes than the launch was sized for is rejected as a whole and reported
    ev = E.DetectionEvaluator()
    m = ev.update(d[0], d[1], (d[2], d[3]), max_gt=16, want_match=True)
    assert ev.state.counters.cpu().tolist()[3] == 1 and bool((m[1] == -1).all())
    with pytest.raises(FdetError, match="1 image"):
        ev.compute()
    keep = [0, 2, 3]                                          # the others were evaluated in full
    ev.state.counters[3] = 0
    r = ev.compute()
    want_tp, want_fp = np.zeros((1, 1000), np.int64), np.zeros((1, 1000), np.int64)
    for n in keep:
        tp, _ = R.match_image(pred[n, :counts[n]], rows[offs[n]:offs[n + 1]], np.asarray(T1, np.float32))
        bins = R.score_bin(pred[n, :counts[n], 0], 1000)
        np.add.at(want_tp[0], bins[tp[0]], 1)
        np.add.at(want_fp[0], bins[~tp[0]], 1)
    assert np.array_equal(r.tp, want_tp) and np.array_equal(r.fp, want_fp) and r.n_images == 3


def test_update_and_evaluate_batch_do_not_synchronise_the_host(monkeypatch):
    E, hp, A = _mods()
    from fdet_amd.models.PoolResnet import PoolResnet
    bank, boxes = A.synthetic_bank(16, "cuda", seed=3, max_side=600)
    batches = list(A.DeviceBatches(bank, boxes, 8, A.default_transform((480, 480)), 10, shuffle=False))
    model = PoolResnet(16, (3, 480, 480), 10).cuda().eval()
    with torch.no_grad():
        y_hats = [model(b[0]) for b in batches]
    ev = E.DetectionEvaluator(iou_thresholds=T10)
    red = ev.reducer_for(model)
    rows, counts = red.forward_batch(y_hats[0])
    ev.update(rows, counts, batches[0][2])                    # warm up (first launch, allocator)
    ev.evaluate_batch(model, y_hats[1], batches[1][2])
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(rows, counts, batches[0][2])
        ev.evaluate_batch(model, y_hats[1], batches[1][2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    calls = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: calls.append("item"))
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self, *a, **k: calls.append("tolist"))
    ev.update(rows, counts, batches[0][2])
    ev.evaluate_batch(model, y_hats[1], batches[1][2])
    monkeypatch.undo()
    assert calls == [] and not batches[0][2].materialized and not batches[1][2].materialized
    assert ev.compute().n_images == 32
    assert model.reduce_bounding_boxes.probability_threshold == 0.5 and red.probability_threshold == 0.01


def _same_bits(a, b):
    a, b = torch.as_tensor(a).detach().float().reshape(-1).cpu(), torch.as_tensor(b).detach().float().reshape(-1).cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))       # NaN-safe bit comparison


def _restated_at(E, model, ev, y_hats, gts, threshold):
    """precision / recall at `threshold` recomputed by the restatement from the same head outputs: the detections of the
    evaluator's reducer with score >= threshold, matched by the sequential loop."""
    red = ev.reducer_for(model)
    tp = fp = n_gt = 0
    for y_hat, gt in zip(y_hats, gts):
        rows, counts = red.forward_batch(y_hat)
        rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
        g_rows, g_offs = gt.rows.cpu().numpy(), gt.box_offset.cpu().numpy()
        for n in range(len(counts)):
            det = rows[n, :counts[n]]
            det = det[det[:, 0] >= np.float32(threshold)]
            g = g_rows[g_offs[n]:g_offs[n + 1]]
            hit, _ = R.match_image(det, g, ev.iou_thresholds[:1])
            tp += int(hit[0].sum())
            fp += int((~hit[0]).sum())
            n_gt += len(g)
    return tp, fp, n_gt


def _fit_twice(make, tmp_path, encoder, patches):
    E, hp, A = _mods()
    from fdet_amd.trainer import fit
    bank, boxes = A.synthetic_bank(48, "cuda", seed=5, max_side=700)
    runs = []
    for with_ev in (False, True):
        torch.manual_seed(0)
        mm = make(tmp_path / f"out{int(with_ev)}.log")
        tr = A.DeviceBatches(bank, boxes, 8, A.training_transform((3, 480, 480), seed=1), patches, encoder=encoder, seed=1)
        va = A.DeviceBatches(bank.subset(range(16)), boxes[:16], 8, A.default_transform((480, 480)), patches, encoder=encoder,
                             shuffle=False)
        steps, y_hats, gts = [], [], []
        ev = E.DetectionEvaluator() if with_ev else None
        if with_ev:                                         # keep what the last epoch's validation pass saw
            inner = ev.evaluate_batch

            def spy(model, y_hat, gt, **kw):
                y_hats.append(y_hat.clone())
                gts.append(gt)
                return inner(model, y_hat, gt, **kw)

            ev.evaluate_batch = spy
        hist = fit(mm, tr, va, epochs=2, on_step=lambda i, t, o: steps.append({k: v.detach().clone() for k, v in o.items()}),
                   **({"evaluator": ev} if with_ev else {}))
        runs.append((mm, hist, steps, ev, y_hats, gts))
    (mm0, h0, s0, _, _, _), (mm1, h1, s1, ev, y_hats, gts) = runs
    assert len(s0) == len(s1) == 2 * (6 + 2)
    for a, b in zip(s0, s1):
        assert a.keys() == b.keys()
        for k in a:
            assert _same_bits(a[k], b[k]), k
    for (n0, p0), (n1, p1) in zip(mm0.model.named_parameters(), mm1.model.named_parameters()):
        assert n0 == n1 and torch.equal(p0, p1), n0
    for e in range(2):
        assert "ap" not in h0["val"][e]
        for k in ("loss", "total_iou", "total_recall", "total_precision"):
            assert _same_bits(h0["val"][e][k], h1["val"][e][k])
        ap = h1["val"][e]["ap"]
        assert np.isfinite(ap) and 0.0 <= ap <= 1.0 and 0.0 <= h1["val"][e]["best_threshold"] < 1.0
    # the evaluator still holds the last epoch: its operating point at the model's threshold against the restatement
    model = mm1.model
    r = ev.compute()
    assert r.n_images == 16 and len(y_hats) == 4
    at = r.at(model.probability_threshold)
    tp, fp, n_gt = _restated_at(E, model, ev, y_hats[2:], gts[2:], model.probability_threshold)
    assert (at["tp"], at["fp"], r.n_gt) == (tp, fp, n_gt)
    assert r.ap == h1["val"][1]["ap"]


def test_fit_with_evaluator_poolresnet(tmp_path):
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    _fit_twice(lambda log: ModelMeta(model=PoolResnet(64, (3, 480, 480), 10).cuda(), lr=1e-3, log_path=log), tmp_path, "yolo", 10)


def test_fit_with_evaluator_ssd(tmp_path):
    _, hp, _ = _mods()
    from fdet_amd.models.ModelMetaSSD import ModelMetaSSD
    from fdet_amd.models.SSD import SSD
    _fit_twice(lambda log: ModelMetaSSD(model=SSD(filters=16, input_shape=(3, 480, 480)).cuda(), lr=1e-3, log_path=log),
               tmp_path, "ssd", hp.SSD_PATCH_SIZES)


@pytest.mark.parametrize("precision", ["32", "16"])
def test_run_validation_epoch_on_the_synthetic_bank(tmp_path, monkeypatch, precision, capsys):
    import json
    from fdet_amd import run_validation_epoch
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    src = ModelMeta(model=PoolResnet(64, (3, 480, 480), 10), lr=1e-4)
    torch.save({"state_dict": src.state_dict(), "epoch": 0, "global_step": 1}, tmp_path / "last.ckpt")
    out = run_validation_epoch.main(["--model", "poolresnet", "--filters", "64", "--batch-size", "8", "--synthetic-images", "20",
                                     "--precision", precision, "--checkpoint", str(tmp_path / "last.ckpt"), "--iou", "0.5", "0.75",
                                     "--json", str(tmp_path / "curve.json")])
    r = out["result"]
    assert r.n_images == 20 and r.n_gt > 0 and np.isfinite(r.ap) and 0.0 <= r.ap <= 1.0
    curve = json.loads((tmp_path / "curve.json").read_text())
    assert curve["n_bins"] == 1000 and len(curve["precision"]) == 2 and curve["n_images"] == 20
    text = capsys.readouterr().out
    assert "validation, loss:" in text and "AP@0.50" in text and "AP@0.75" in text and "best F1" in text


def test_run_validation_epoch_ssd(tmp_path, monkeypatch):
    from fdet_amd import run_validation_epoch
    monkeypatch.chdir(tmp_path)
    out = run_validation_epoch.main(["--model", "ssd", "--batch-size", "8", "--synthetic-images", "16", "--precision", "16"])
    assert out["result"].n_images == 16 and np.isfinite(out["result"].ap)


def test_encoded_targets_as_predictions_score_ap_one():
    """The evaluator against the package's own encode / decode: a head that emits the encoded targets themselves is a
    perfect detector when the faces fall in distinct cells."""
    E, hp, _ = _mods()
    from fdet_amd.models.PoolResnet import PoolResnet
    model = PoolResnet(16, (3, 480, 480), 10)                 # geometry only: its reducer's shape and thresholds
    rng = np.random.default_rng(9)
    B, rows, offs = 64, [], [0]
    for n in range(B):
        k = int(rng.integers(0, 3))
        if k >= 1:
            rows.append([1, rng.integers(0, 100), rng.integers(0, 100), rng.integers(20, 100), rng.integers(20, 100)])
        if k == 2:
            rows.append([1, rng.integers(260, 370), rng.integers(260, 370), rng.integers(20, 100), rng.integers(20, 100)])
        offs.append(len(rows))
    d_rows, d_offs = _dev(np.asarray(rows, np.float32), np.asarray(offs, np.int32))
    y = hp.encode_targets_device(d_rows, d_offs, (480, 480), 10)
    ev = E.DetectionEvaluator(iou_thresholds=(0.5,))
    ev.evaluate_batch(model, y, (d_rows, d_offs))
    r = ev.compute()
    assert r.n_gt == len(rows) and r.n_det == len(rows) and int(r.tp.sum()) == len(rows) and int(r.fp.sum()) == 0
    assert r.ap == 1.0 and r.best_f1 == 1.0
