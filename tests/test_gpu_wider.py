"""The WIDER Face protocol evaluator on the GPU: `fdet_eval_wider` against the sequential numpy float64 restatement
(tests/wider_cpu_ref.py).  Histograms and counters are integers and every comparison of them is exact: both sides do the
same fp32 scaling and the same fp64 operations in the same order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wider_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SSD_PRIORS = 4774


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import evaluation_wider as W, hotpath as hp
    return W, hp


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _gt(W, rows, offs, masks, max_gt=None):
    r, o, m = _dev(rows, offs, masks.view(np.int32))
    return W.WiderGt(r, o, m, max_gt)


def _names(n):
    return tuple(f"s{i}" for i in range(n))


def _run(batch, n_subsets, n_bins=1000, normalize=False, scale=None, iou=0.5, max_gt=None):
    W, hp = _mods()
    pred, counts, rows, offs, masks = batch
    ev = W.WiderEvaluator(_names(n_subsets), iou, n_bins, normalize)
    ev.update(*_dev(pred, counts), _gt(W, rows, offs, masks, max_gt), scale=None if scale is None else _dev(scale)[0])
    return ev, ev.compute()


def _check(batch, n_subsets, n_bins=1000, normalize=False, scale=None, iou=0.5, max_gt=None):
    pred, counts, rows, offs, masks = batch
    ev, r = _run(batch, n_subsets, n_bins, normalize, scale, iou, max_gt)
    norm = R.score_range(pred, counts) if normalize else (0.0, 1.0)
    p, h, nf = R.evaluate(pred, counts, rows, offs, masks, n_subsets, iou, n_bins, norm, scale)
    print(f"proposals {r.proposals.sum(1).tolist()} / {p.sum(1).tolist()}  hits {r.hits.sum(1).tolist()} / {h.sum(1).tolist()}  "
          f"mismatching bins {int((r.proposals != p).sum())} + {int((r.hits != h).sum())}")
    assert np.array_equal(r.proposals, p) and np.array_equal(r.hits, h)
    assert [r.n_faces[k] for k in r.subset_names] == nf.tolist()
    assert (r.n_images, r.n_det) == (len(counts), int(counts.sum()))
    assert (r.score_min, r.score_range) == (float(norm[0]), float(norm[1]))
    for s, k in enumerate(r.subset_names):
        ap = R.curve(p[s], h[s], nf[s])[2]
        assert (np.isnan(ap) and np.isnan(r.ap[k])) or abs(ap - r.ap[k]) <= 1e-12
    return r


@pytest.mark.parametrize("B,Kmax,max_det,max_gt,n_subsets", [(9, 100, 100, 6, 3), (7, 225, 225, 12, 1), (64, 100, 60, 5, 8),
                                                             (5, 225, 60, 40, 3), (4, SSD_PRIORS, 700, 30, 8), (6, SSD_PRIORS, 500, 20, 3)],
                         ids=["yolo10-S3", "yolo15-S1", "yolo10-B64-S8", "yolo15-crowded-S3", "ssd-S8", "ssd-S3"])
def test_kernel_equals_sequential_restatement(B, Kmax, max_det, max_gt, n_subsets):
    """Per case: an image without detections, one without boxes, one whose boxes are all ignored, a NaN score, scores
    quantised to two decimals, jittered and duplicated copies of the boxes."""
    rng = np.random.default_rng(B * 1000 + Kmax + n_subsets)
    batch = R.random_batch(rng, B, Kmax, max_det, max_gt, n_subsets, empty_det=(0,), empty_gt=(1,), all_ignored=(2,))
    pred, counts, rows, offs, masks = batch
    pred[B - 1, 1, 0] = np.nan
    assert counts[0] == 0 and offs[2] == offs[1] and counts[B - 1] >= 2
    assert not (masks[offs[2]:offs[3]] & np.uint32((1 << n_subsets) - 1)).any() and offs[3] > offs[2]
    ex = R.exercised(*batch, n_subsets)
    assert ex["ignored_hits"] > 0 and ex["duplicates"] > 0 and ex["ties"] > 0, ex
    M = np.concatenate([R.overlap_matrix(pred[i, :counts[i], 1:], rows[offs[i]:offs[i + 1], 1:]).max(1, initial=0.0) for i in range(B)])
    assert ((M > 0) & (M < 0.5)).any() and (M >= 0.5).any()              # overlaps on both sides of the threshold
    r = _check(batch, n_subsets)
    assert r.hits.sum() > 0 and (r.proposals.sum(1) < counts.sum()).all()


def test_ssd_shape_with_most_slots_used_and_2048_boxes():
    rng = np.random.default_rng(17)
    batch = R.random_batch(rng, 3, SSD_PRIORS, 4600, 30, 3, big=(1, 2048))
    pred, counts, rows, offs, masks = batch
    counts[2] = SSD_PRIORS                                               # every slot (the tail holds uniform garbage rows)
    assert offs[2] - offs[1] == 2048
    ex = R.exercised(*batch, 3)
    assert ex["ignored_hits"] > 0 and ex["duplicates"] > 0 and ex["ties"] > 0, ex
    _check(batch, 3, max_gt=2048)


def test_overlap_of_exactly_one_half_is_a_hit():
    """Detection 0,0,9,9 on box 0,0,9,19: inclusive areas 100 and 200, intersection 100."""
    assert R.overlap_matrix([[0, 0, 9, 9]], [[0, 0, 9, 19]])[0, 0] == 0.5
    pred = np.zeros((2, 4, 5), np.float32)
    pred[0, 0] = [0.9, 0, 0, 9, 9]
    pred[1, 0] = [0.9, 0, 0, 9, 8]                                       # 90 / 200: below
    counts = np.array([1, 1], np.int32)
    rows = np.array([[1, 0, 0, 9, 19], [1, 0, 0, 9, 19]], np.float32)
    offs = np.array([0, 1, 2], np.int32)
    r = _check((pred, counts, rows, offs, np.array([1, 1], np.uint32)), 1)
    assert r.hits.sum() == 1 and r.proposals.sum() == 2 and r.hits[0, 100] == 1      # 0.9f = 0.899999976 < 1 - 100/1000
    # an ignored box at exactly one half swallows the detection
    r = _check((pred, counts, rows, offs, np.array([0, 0], np.uint32)), 1)
    assert r.hits.sum() == 0 and r.proposals.sum() == 1


@pytest.mark.parametrize("n_bins", [37, 4096])
def test_odd_bins_and_scores_outside_the_unit_interval(n_bins):
    rng = np.random.default_rng(3)
    batch = R.random_batch(rng, 9, 100, 100, 6, 3)
    pred, counts = batch[0], batch[1]
    pred[0, :6, 0] = [1.0, 1.5, -0.25, np.nan, 0.0, -0.0]
    pred[1, :2, 0] = [np.inf, -np.inf]
    r = _check(batch, 3, n_bins=n_bins)
    assert r.proposals.sum(1).max() < counts.sum()                       # the negative, NaN and -inf scores are counted nowhere


def test_non_unit_pred_scale():
    rng = np.random.default_rng(5)
    scale = np.c_[rng.uniform(0.6, 2.2, 12), rng.uniform(0.6, 2.2, 12)].astype(np.float32)
    batch = R.random_batch(rng, 12, 225, 120, 8, 3, scale=scale)
    ex = R.exercised(*batch, 3, scale=scale)
    assert ex["ignored_hits"] > 0 and ex["duplicates"] > 0 and ex["ties"] > 0, ex
    r = _check(batch, 3, scale=scale)
    assert r.hits.sum() > 0
    unscaled = _run(batch, 3)[1]
    assert not np.array_equal(unscaled.hits, r.hits)                     # the scale matters to the result


def test_normalisation():
    W, hp = _mods()
    rng = np.random.default_rng(8)
    batch = R.random_batch(rng, 10, 100, 80, 6, 3)
    pred, counts = batch[0], batch[1]
    pred[:, :, 0] = np.float32(0.2) + np.float32(0.5) * pred[:, :, 0]   # scores in [0.2, 0.7]
    r = _check(batch, 3, normalize=True)
    assert 0.19 < r.score_min < 0.3 and 0.4 < r.score_range <= 0.5
    raw = _run(batch, 3, normalize=False)[1]
    assert not np.array_equal(raw.proposals, r.proposals)
    # pre-normalised scores (min exactly 0, max exactly 1): normalising changes nothing
    batch2 = R.random_batch(rng, 10, 100, 80, 6, 3)
    batch2[0][3, 0, 0], batch2[0][3, 1, 0] = 0.0, 1.0
    a, b = _run(batch2, 3, normalize=True)[1], _run(batch2, 3, normalize=False)[1]
    assert (a.score_min, a.score_range) == (0.0, 1.0)
    assert np.array_equal(a.proposals, b.proposals) and np.array_equal(a.hits, b.hits) and a.ap == b.ap
    # every score equal: the protocol would divide by zero
    batch2[0][:, :, 0] = 0.5
    ev = W.WiderEvaluator(_names(3))
    ev.update(*_dev(batch2[0], batch2[1]), _gt(W, *batch2[2:]))
    with pytest.raises(hp.N.FdetError, match="divides by zero"):
        ev.compute()


@pytest.mark.parametrize("normalize", [False, True])
def test_two_updates_equal_one_on_the_concatenation_merge_and_reset(normalize):
    W, hp = _mods()
    rng = np.random.default_rng(21)
    a = R.random_batch(rng, 6, 225, 80, 9, 3)
    b = R.random_batch(rng, 11, 225, 80, 9, 3)
    b[0][:, :, 0] *= np.float32(0.5)                                     # the two halves have different score ranges
    ev = W.WiderEvaluator(_names(3), normalize=normalize)
    for pred, counts, rows, offs, masks in (a, b):
        ev.update(*_dev(pred, counts), _gt(W, rows, offs, masks))
    two = ev.compute()
    again = ev.compute()                                                 # compute() does not accumulate twice
    assert np.array_equal(two.proposals, again.proposals) and np.array_equal(two.hits, again.hits)
    na = int(a[3][-1])
    cat = (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2][:na], b[2]], 0),
           np.concatenate([a[3], b[3][1:] + na]).astype(np.int32), np.concatenate([a[4][:na], b[4]]))
    one = _check(cat, 3, normalize=normalize)
    assert np.array_equal(one.proposals, two.proposals) and np.array_equal(one.hits, two.hits)
    assert (one.n_faces, one.n_images, one.n_det, one.ap) == (two.n_faces, two.n_images, two.n_det, two.ap) and one.n_images == 17
    # merge of two evaluators
    e1, e2 = W.WiderEvaluator(_names(3), normalize=normalize), W.WiderEvaluator(_names(3), normalize=normalize)
    e1.update(*_dev(a[0], a[1]), _gt(W, *a[2:]))
    e2.update(*_dev(b[0], b[1]), _gt(W, *b[2:]))
    m = e1.merge(e2).compute()
    assert np.array_equal(m.proposals, one.proposals) and np.array_equal(m.hits, one.hits) and m.n_faces == one.n_faces
    with pytest.raises(ValueError):
        e1.merge(W.WiderEvaluator(_names(2), normalize=normalize))
    ev.reset()
    z = ev.compute()
    assert z.proposals.sum() == 0 and z.hits.sum() == 0 and (z.n_images, z.n_det) == (0, 0) and all(np.isnan(v) for v in z.ap.values())


@pytest.mark.parametrize("normalize", [False, True])
def test_an_image_over_max_gt_is_rejected_and_compute_raises(normalize):
    W, hp = _mods()
    rng = np.random.default_rng(2)
    batch = R.random_batch(rng, 4, 100, 50, 8, 3, big=(1, 40))
    pred, counts, rows, offs, masks = batch
    ev = W.WiderEvaluator(_names(3), normalize=normalize)
    ev.update(*_dev(pred, counts), _gt(W, rows, offs, masks), max_gt=16)
    with pytest.raises(hp.N.FdetError, match="1 image"):
        ev.compute()
    d = _dev(pred, counts, rows, offs, masks.view(np.int32))
    with pytest.raises(ValueError):
        hp.eval_wider(torch.zeros(1, 4865, 5, device="cuda"), d[1][:1], d[2], d[3][:2], d[4], hp.WiderState())
    with pytest.raises(ValueError):
        hp.eval_wider(*d, hp.WiderState(), max_gt=4097)
    with pytest.raises(ValueError):
        hp.eval_wider(d[0], d[1], d[2], d[3], d[4][:-1], hp.WiderState())
    # the others were evaluated in full
    st = hp.WiderState(3)
    hp.eval_wider(*d, st, max_gt=16)
    c = st.counters.cpu().tolist()
    keep = [0, 2, 3]
    p = np.zeros((3, 1000), np.int64)
    h = np.zeros((3, 1000), np.int64)
    nf = np.zeros(3, np.int64)
    for n in keep:
        q = R.evaluate(pred[n:n + 1], counts[n:n + 1], rows, offs[n:n + 2], masks, 3)
        p, h, nf = p + q[0], h + q[1], nf + q[2]
    assert c[3:] == [3, int(counts[keep].sum()), 1] and c[:3] == nf.tolist()
    got = (st.hist.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
    assert np.array_equal(got[0], p) and np.array_equal(got[1], h)


def test_update_does_not_synchronise_the_host():
    W, hp = _mods()
    rng = np.random.default_rng(4)
    batch = R.random_batch(rng, 8, 100, 60, 5, 3)
    d = _dev(batch[0], batch[1])
    gt = _gt(W, *batch[2:])
    for normalize in (False, True):
        ev = W.WiderEvaluator(_names(3), normalize=normalize)
        ev.update(d[0], d[1], gt)                                        # warm up
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ev.update(d[0], d[1], gt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert ev.compute().n_images == 16


def _synthetic_protocol(tmp_path, n, seed=2):
    """The .mat files of a synthetic bank: its own boxes plus one extra box per image that no subset keeps; easy keeps
    boxes with both sides >= 60, medium >= 25, hard every box of the bank."""
    import fdet_amd  # noqa: F401
    from fdet_amd import run_validation_epoch as V
    from fdet_amd.datasets import augment as A
    bank, boxes = A.synthetic_bank(n, "cuda", seed=seed)
    names = V.synthetic_names(n)
    full, keeps = [], {"easy": [], "medium": [], "hard": []}
    for i, b in enumerate(boxes):
        h, w = bank.sizes[i]
        extra = np.array([[w // 3, h // 3, 40, 50]], np.float64)
        f = np.concatenate([extra, b[:, 1:].astype(np.float64)], 0)     # the ignored box comes first: 1-based indices shift
        full.append(f)
        side = np.minimum(f[:, 2], f[:, 3])
        own = np.arange(len(f)) >= 1
        keeps["easy"].append(np.nonzero(own & (side >= 60))[0])
        keeps["medium"].append(np.nonzero(own & (side >= 25))[0])
        keeps["hard"].append(np.nonzero(own)[0])
    R.write_mats(str(tmp_path / "gt"), names, full, keeps)
    return names, full, keeps


@pytest.mark.parametrize("tiled", [False, True], ids=["resized", "tiled"])
def test_run_validation_epoch_reports_the_restatements_three_aps(tmp_path, monkeypatch, capsys, tiled):
    import json
    W, hp = _mods()
    from fdet_amd import run_validation_epoch as V
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    monkeypatch.chdir(tmp_path)
    n = 20
    names, full, keeps = _synthetic_protocol(tmp_path, n)
    torch.manual_seed(3)
    src = ModelMeta(model=PoolResnet(64, (3, 480, 480), 10), lr=1e-4)
    torch.save({"state_dict": src.state_dict(), "epoch": 0, "global_step": 1}, tmp_path / "last.ckpt")
    argv = ["--model", "poolresnet", "--filters", "64", "--batch-size", "8", "--synthetic-images", str(n), "--checkpoint",
            str(tmp_path / "last.ckpt"), "--iou", "0.5", "0.75"] + (["--tiled", "--tile", "480"] if tiled else [])
    plain = V.main(argv + ["--json", str(tmp_path / "plain.json")])
    plain_text = capsys.readouterr().out
    seen = []
    inner = W.WiderEvaluator.update

    def spy(self, pred_rows, pred_counts, gt, scale=None, max_gt=None):
        seen.append((self, pred_rows.cpu().numpy().copy(), pred_counts.cpu().numpy().copy(), gt.rows.cpu().numpy(), gt.box_offset.cpu().numpy(),
                     gt.subsets.cpu().numpy().view(np.uint32), None if scale is None else scale.cpu().numpy()))
        return inner(self, pred_rows, pred_counts, gt, scale, max_gt)

    monkeypatch.setattr(W.WiderEvaluator, "update", spy)
    out = V.main(argv + ["--json", str(tmp_path / "wider.json"), "--wider-gt", str(tmp_path / "gt")])
    text = capsys.readouterr().out
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    # the DetectionEvaluator's results are bit-identical with and without --wider-gt
    for key in ("result",) + (("tiled",) if tiled else ()):
        a, b = plain[key], out[key]
        assert np.array_equal(a.tp, b.tp) and np.array_equal(a.fp, b.fp) and (a.n_gt, a.n_images, a.n_det) == (b.n_gt, b.n_images, b.n_det)
        assert a.ap_per_threshold.tobytes() == b.ap_per_threshold.tobytes() and a.precision.tobytes() == b.precision.tobytes()
    assert plain["metrics"].keys() == out["metrics"].keys()
    for k in plain["metrics"]:
        assert float(plain["metrics"][k]) == float(out["metrics"][k]) or (plain["metrics"][k] != plain["metrics"][k])
    assert "wider" not in plain and "WIDER" not in plain_text
    assert [ln for ln in text.splitlines() if "WIDER" not in ln] == plain_text.splitlines()
    pj, wj = json.loads((tmp_path / "plain.json").read_text()), json.loads((tmp_path / "wider.json").read_text())
    assert set(wj) - set(pj) == ({"wider", "wider_tiled"} if tiled else {"wider"}) and all(wj[k] == pj[k] for k in pj)
    # the three APs against the restatement fed with the same rows
    for key in ("wider",) + (("wider_tiled",) if tiled else ()):
        r = out[key]
        mine = [s for s in seen if s[0] is seen[0 if key == "wider" else -1][0]]
        assert sum(len(s[2]) for s in mine) == n and r.n_images == n
        assert (mine[0][6] is None) == (key == "wider_tiled")            # the resized pass is scaled back to source pixels
        lo, hi = 1.0, 0.0
        for s in mine:
            q = R.score_min_max(s[1], s[2])
            lo, hi = min(lo, q[0]), max(hi, q[1])
        assert (r.score_min, r.score_range) == (lo, hi - lo)
        p = np.zeros((3, 1000), np.int64)
        h = np.zeros((3, 1000), np.int64)
        nf = np.zeros(3, np.int64)
        for s in mine:
            q = R.evaluate(s[1], s[2], s[3], s[4], s[5], 3, 0.5, 1000, (lo, hi - lo), s[6])
            p, h, nf = p + q[0], h + q[1], nf + q[2]
        assert np.array_equal(r.proposals, p) and np.array_equal(r.hits, h) and r.proposals.sum() > 0
        assert [r.n_faces[k] for k in ("easy", "medium", "hard")] == nf.tolist() == [sum(len(k) for k in keeps[s]) for s in ("easy", "medium", "hard")]
        assert nf[0] < nf[1] <= nf[2] and nf[0] > 0
        for s, k in enumerate(("easy", "medium", "hard")):
            ap = R.curve(p[s], h[s], nf[s])[2]
            print(key, k, "AP", r.ap[k], "restatement", ap)
            assert abs(r.ap[k] - ap) <= 1e-12
            assert wj[key]["ap"][k] == r.ap[k] and f"{k} AP {r.ap[k]:.4f}" in text
        # the ground truth the evaluator saw is the .mat's full list, ignored box included
        assert sum(int(s[4][-1]) for s in mine) == sum(len(f) for f in full)


def test_detect_images_writes_the_prediction_directory(tmp_path, monkeypatch):
    from PIL import Image
    W, hp = _mods()
    from fdet_amd import detect_images
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    for event, name, hw in (("0--Parade", "0_Parade_a.jpg", (300, 400)), ("0--Parade", "0_Parade_b.png", (500, 350)), ("1--Riot", "1_Riot_c.png", (480, 480))):
        os.makedirs(tmp_path / "images" / event, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(tmp_path / "images" / event / name)
    out = detect_images.main(["--filters", "16", "--images", str(tmp_path / "images"), "--out", str(tmp_path / "res.txt"),
                              "--pred-dir", str(tmp_path / "pred"), "--probability-threshold", "0.3"])
    names, rows, counts = W.read_wider_pred_dir(tmp_path / "pred")
    assert names == ["0--Parade/0_Parade_a", "0--Parade/0_Parade_b", "1--Riot/1_Riot_c"] == [W.image_key(n) for n in out["names"]]
    assert np.array_equal(counts, out["counts"].numpy())
    for i in range(3):
        want = out["rows"][i, :counts[i]].numpy()
        assert np.array_equal(rows[i, :counts[i]], want[R.visiting_order(want[:, 0])])
    assert (tmp_path / "res.txt").read_text().splitlines()[0] == "0--Parade/0_Parade_a.jpg"
