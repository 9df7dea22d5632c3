"""Host-side checks of the detection evaluator: the matching rule and AP on hand-made cases with known answers (through the
numpy restatement tests/eval_cpu_ref.py, which the GPU tests compare the kernel with), `EvalResult` on hand-written
histograms, binned AP against a brute-force AP over the exactly sorted detection list, merge / gloo all_reduce of the
integer state, the WIDER annotation parser, `bank_from_files`' decode, and the argument checks of `hotpath.eval_match`."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_cpu_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ev():
    import fdet_amd  # noqa: F401
    from fdet_amd import evaluation
    return evaluation


def _result(E, pred, counts, rows, offs, thr=(0.5,), n_bins=1000):
    """EvalResult of a batch, the histograms coming from the restatement (what the kernel computes on the GPU)."""
    htp, hfp, n_gt, match = R.evaluate(pred, counts, rows, offs, np.asarray(thr, np.float32), n_bins)
    n_det = int(np.sum(counts))
    return E.EvalResult(htp, hfp, n_gt, len(counts), n_det, np.asarray(thr, np.float32)), match


def _batch(images):
    """[(detections (K,5), boxes (G,4))] -> kernel layout."""
    Kmax = max(1, max(len(d) for d, _ in images))
    pred = np.zeros((len(images), Kmax, 5), np.float32)
    counts = np.zeros(len(images), np.int32)
    rows, offs = [], [0]
    for n, (d, g) in enumerate(images):
        d = np.asarray(d, np.float32).reshape(-1, 5)
        pred[n, :len(d)] = d
        counts[n] = len(d)
        g = np.asarray(g, np.float32).reshape(-1, 4)
        rows.append(np.c_[np.ones(len(g), np.float32), g])
        offs.append(offs[-1] + len(g))
    rows = np.concatenate(rows + [np.zeros((1, 5), np.float32)], 0)
    return pred, counts, rows, np.asarray(offs, np.int32)


A, B_, C = [10, 10, 40, 40], [200, 200, 50, 50], [300, 50, 30, 60]


def test_perfect_detector_has_ap_one():
    E = _ev()
    r, m = _result(E, *_batch([([[0.9] + A, [0.8] + B_], [A, B_]), ([[0.7] + C], [C])]))
    assert r.ap == 1.0 and r.n_gt == 3 and r.n_images == 2
    assert r.best_f1 == 1.0 and r.best_threshold == 0.7
    assert m[0].tolist() == [0, 1] and m[1].tolist() == [2, -1]


def test_no_detections_has_ap_zero():
    E = _ev()
    r, _ = _result(E, *_batch([([], [A, B_])]))
    assert r.ap == 0.0 and r.n_det == 0 and np.isnan(r.best_f1)


def test_duplicate_detection_is_one_tp_and_one_fp():
    E = _ev()
    r, m = _result(E, *_batch([([[0.6] + A, [0.9] + A], [A])]))
    assert int(r.tp.sum()) == 1 and int(r.fp.sum()) == 1
    assert m[0].tolist() == [-1, 0]                         # the higher score claims the face, whatever the row order
    assert r.at(0.9) == {"bin": 900, "tp": 1, "fp": 0, "precision": 1.0, "recall": 1.0, "f1": 1.0}
    assert r.at(0.6)["precision"] == 0.5 and r.ap == 1.0


def test_tied_scores_go_by_row_index():
    E = _ev()
    _, m = _result(E, *_batch([([[0.5] + A, [0.5] + A], [A])]))
    assert m[0].tolist() == [0, -1]


def test_best_box_already_claimed_is_fp_although_a_second_box_overlaps():
    """VOC / WIDER rule: the candidate is the box of highest IoU among ALL boxes.  Detection 1 overlaps box 0 best (already
    claimed by detection 0) and box 1 with IoU >= 0.5 as well: it is a false positive, not a match of box 1."""
    E = _ev()
    g0, g1 = [0, 0, 100, 100], [30, 0, 100, 100]
    d0, d1 = [0.9, 0, 0, 100, 100], [0.8, 10, 0, 100, 100]
    iou = R.iou_matrix([d1[1:]], [g0, g1])[0]
    assert iou[0] > iou[1] >= 0.5
    r, m = _result(E, *_batch([([d0, d1], [g0, g1])]))
    assert m[0].tolist() == [0, -1] and int(r.tp.sum()) == 1 and int(r.fp.sum()) == 1
    assert r.recall[0, 0] == 0.5


def test_zero_face_image_counts_only_false_positives():
    E = _ev()
    r, _ = _result(E, *_batch([([[0.9] + A], []), ([[0.8] + B_], [B_])]))
    assert int(r.fp.sum()) == 1 and int(r.tp.sum()) == 1 and r.n_gt == 1
    assert r.ap == 0.5                                        # recall 1 is reached at precision 1/2


def test_no_ground_truth_gives_nan_not_an_exception():
    E = _ev()
    r, _ = _result(E, *_batch([([[0.9] + A], [])]))
    assert np.isnan(r.ap) and np.isnan(r.mean_ap) and r.n_gt == 0
    assert np.isnan(r.at(0.5)["recall"])
    r.to_json()


def test_degenerate_boxes_never_match():
    E = _ev()
    _, m = _result(E, *_batch([([[0.9, 5, 5, 0, 0]], [[5, 5, 0, 0]])]))      # 0/0 IoU
    assert m[0].tolist() == [-1]


def test_compute_on_hand_written_histograms():
    E = _ev()
    tp = np.zeros((1, 4), np.int64)
    fp = np.zeros((1, 4), np.int64)
    tp[0] = [1, 0, 1, 2]                                      # bins [0,.25) [.25,.5) [.5,.75) [.75,1]
    fp[0] = [3, 1, 1, 0]
    r = E.EvalResult(tp, fp, 5, 3, 9, np.asarray([0.5], np.float32))
    assert r.cum_tp[0].tolist() == [4, 3, 3, 2] and r.cum_fp[0].tolist() == [5, 2, 1, 0]
    assert np.allclose(r.precision[0], [4 / 9, 3 / 5, 3 / 4, 1.0], rtol=0, atol=0)
    assert np.allclose(r.recall[0], [0.8, 0.6, 0.6, 0.4], rtol=0, atol=0)
    # recall steps 0 -> .4 at precision 1, .4 -> .6 at 3/4 (the envelope over 3/5), .6 -> .8 at 4/9
    assert abs(r.ap - (0.4 * 1.0 + 0.2 * 0.75 + 0.2 * 4 / 9)) < 1e-15
    f1 = [2 * p * q / (p + q) for p, q in zip(r.precision[0], r.recall[0])]
    assert r.best_bin == int(np.argmax(f1)) and abs(r.best_f1 - max(f1)) < 1e-15 and r.best_threshold == r.best_bin / 4
    assert r.at(0.5) == {"bin": 2, "tp": 3, "fp": 1, "precision": 0.75, "recall": 0.6, "f1": r.f1[0, 2]}
    assert r.at(0.6)["bin"] == 2                              # between edges: the edge at or below
    assert E.voc_ap(r.recall[0][::-1], r.precision[0][::-1]) == R.voc_ap(r.recall[0][::-1], r.precision[0][::-1])


def test_binned_ap_equals_brute_force_ap_for_scores_on_bin_edges():
    """With every score a distinct multiple of 1/n_bins (one detection per bin) the binned curve has exactly the points of
    the sorted detection list, so AP agrees to rounding (1e-12)."""
    E = _ev()
    n_bins = 1000
    edges = [k for k in range(n_bins) if R.score_bin([np.float32(k) / np.float32(n_bins)], n_bins)[0] == k]
    assert len(edges) > 900
    rng = np.random.default_rng(5)
    for trial in range(5):
        pred, counts, rows, offs = R.random_batch(rng, 12, 40, 40, 6)
        ks = rng.permutation(edges)[:int(counts.sum())]
        i = 0
        for n in range(len(counts)):
            pred[n, :counts[n], 0] = (ks[i:i + counts[n]].astype(np.float32) / np.float32(n_bins))
            i += counts[n]
        thr = np.asarray([0.5, 0.75], np.float32)
        r, _ = _result(E, pred, counts, rows, offs, thr=thr, n_bins=n_bins)
        for t in range(2):
            scores, flags = [], []
            for n in range(len(counts)):
                tp, _ = R.match_image(pred[n, :counts[n]], rows[offs[n]:offs[n + 1]], thr[t:t + 1])
                scores += pred[n, :counts[n], 0].tolist()
                flags += tp[0].tolist()
            exact = R.ap_exact(np.asarray(scores, np.float32), np.asarray(flags, bool), r.n_gt)
            assert abs(r.ap_per_threshold[t] - exact) <= 1e-12, (trial, t, r.ap_per_threshold[t], exact)
            assert abs(R.ap_from_hist(r.tp[t], r.fp[t], r.n_gt) - r.ap_per_threshold[t]) <= 1e-15


def test_parallel_formulation_equals_the_sequential_loop():
    """What the kernel does (independent arg-max, per-box winner of lowest rank) against the sequential loop."""
    rng = np.random.default_rng(11)
    thr = np.arange(10, dtype=np.float32) * np.float32(0.05) + np.float32(0.5)
    for _ in range(200):
        pred, counts, rows, offs = R.random_batch(rng, 1, 40, 40, 12)
        K, gt = int(counts[0]), rows[offs[0]:offs[1]]
        tp_seq, _ = R.match_image(pred[0, :K], gt, thr)
        if K == 0 or len(gt) == 0:
            assert not tp_seq.any()
            continue
        M = R.iou_matrix(pred[0, :K, 1:], gt[:, 1:])
        order = R.visiting_order(pred[0, :K, 0])
        rank = np.empty(K, np.int64)
        rank[order] = np.arange(K)
        am = M.argmax(1)
        for t, th in enumerate(thr):
            ok = M[np.arange(K), am] >= th
            first = np.full(len(gt), K + 1)
            np.minimum.at(first, am[ok], rank[ok])
            assert np.array_equal(ok & (first[am] == rank), tp_seq[t])


def _filled(E, seed, device="cpu"):
    ev = E.DetectionEvaluator(iou_thresholds=(0.5, 0.75), n_bins=50, device=device)
    g = torch.Generator().manual_seed(seed)
    ev.state.hist.copy_(torch.randint(0, 1000, tuple(ev.state.hist.shape), generator=g, dtype=torch.int32))
    ev.state.counters.copy_(torch.tensor([100 + seed, 10, 300, 0]))
    return ev


def test_merge_adds_the_integer_state():
    E = _ev()
    a, b = _filled(E, 1), _filled(E, 2)
    want_h, want_c = a.state.hist + b.state.hist, a.state.counters + b.state.counters
    a.state.hist[0, 0, 0] = -5                               # uint32 4294967291: the sum wraps like uint32 addition
    a.merge(b)
    want_h[0, 0, 0] = -5 + int(b.state.hist[0, 0, 0])
    assert torch.equal(a.state.hist, want_h) and torch.equal(a.state.counters, want_c)
    r = a.compute()
    assert r.n_gt == 203 and r.tp[0, 0] == (want_h[0, 0, 0].item() & 0xFFFFFFFF)
    with pytest.raises(ValueError):
        a.merge(E.DetectionEvaluator(iou_thresholds=(0.5,), n_bins=50, device="cpu"))
    a.reset()
    assert int(a.state.hist.abs().sum()) == 0 and int(a.state.counters.sum()) == 0


def test_rejected_images_make_compute_raise():
    E = _ev()
    from fdet_amd import FdetError
    ev = _filled(E, 3)
    ev.state.counters[3] = 2
    with pytest.raises(FdetError, match="2 image"):
        ev.compute()


def test_all_reduce_over_gloo(tmp_path):
    import torch.distributed as dist
    E = _ev()
    if not dist.is_available():
        pytest.skip("torch.distributed is not built in")
    a = _filled(E, 4)
    want_h, want_c = a.state.hist.clone(), a.state.counters.clone()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        a.all_reduce()
        assert torch.equal(a.state.hist, want_h) and torch.equal(a.state.counters, want_c)      # world of one: identity
    finally:
        dist.destroy_process_group()


def _rank(rank, world, path, out):
    import torch.distributed as dist
    import fdet_amd  # noqa: F401
    from fdet_amd import evaluation as E
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=world)
    ev = _filled(E, 10 + rank)
    ev.all_reduce()
    out.put((rank, ev.state.hist.numpy().copy(), ev.state.counters.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_two_ranks_gloo(tmp_path):
    import torch.multiprocessing as mp
    E = _ev()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_rank, args=(r, 2, str(tmp_path / "pg2"), q)) for r in range(2)]
    for p in ps:
        p.start()
    got = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    want_h = (_filled(E, 10).state.hist + _filled(E, 11).state.hist).numpy()
    want_c = (_filled(E, 10).state.counters + _filled(E, 11).state.counters).numpy()
    for _, h, c in got:
        assert np.array_equal(h, want_h) and np.array_equal(c, want_c)


def test_wider_annotation_parser(tmp_path):
    import shutil
    from fdet_amd.datasets.WIDERFace.annotations import read_wider_annotations
    root = tmp_path / "wider"
    (root / "wider_face_split").mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "wider_face_mini_bbx_gt.txt"), root / "wider_face_split" / "wider_face_val_bbx_gt.txt")
    paths, boxes = read_wider_annotations(root, "val")
    assert [p.relative_to(root).as_posix() for p in paths] == [
        "WIDER_val/images/0--Parade/0_Parade_mini_0001.jpg", "WIDER_val/images/1--Handshaking/1_Handshaking_mini_0002.jpg",
        "WIDER_val/images/2--Demonstration/2_Demonstration_mini_0003.jpg", "WIDER_val/images/3--Riot/3_Riot_mini_0004.jpg"]
    assert [b.shape for b in boxes] == [(1, 5), (1, 5), (3, 5), (2, 5)] and all(b.dtype == np.float32 for b in boxes)
    assert boxes[0].tolist() == [[1, 40, 30, 50, 60]]
    assert boxes[1].tolist() == [[1, 0, 0, 0, 0]]            # the placeholder row, kept as the reference keeps it
    assert boxes[2][1].tolist() == [1, 100, 90, 33, 41]
    paths2, boxes2 = read_wider_annotations(root, "val", max_faces=2)        # the reference's `< 3` filter
    assert [p.name for p in paths2] == ["0_Parade_mini_0001.jpg", "1_Handshaking_mini_0002.jpg", "3_Riot_mini_0004.jpg"]
    _, boxes3 = read_wider_annotations(root, "val", keep_placeholder=False)
    assert boxes3[1].shape == (0, 5) and boxes3[3].shape == (2, 5)
    with pytest.raises(FileNotFoundError):
        read_wider_annotations(root, "train")


def test_bank_from_files_decodes_with_pil(tmp_path, monkeypatch):
    from PIL import Image
    from fdet_amd.datasets import augment as A
    from fdet_amd.datasets.WIDERFace import annotations as W
    rng = np.random.default_rng(0)
    imgs, paths = [], []
    for i, (h, w) in enumerate([(12, 20), (7, 9), (30, 16)]):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = tmp_path / f"im{i}.png"                           # PNG is lossless: decoded pixels equal what was written
        Image.fromarray(a).save(p)
        imgs.append(a)
        paths.append(p)
    grey = tmp_path / "grey.png"
    Image.fromarray(imgs[0][:, :, 0]).save(grey)              # a greyscale file comes back as RGB
    got = {}

    def fake_from_arrays(images, device, **kw):
        got["images"], got["device"] = images, device
        return "bank"

    monkeypatch.setattr(A.DeviceImageBank, "from_arrays", staticmethod(fake_from_arrays))
    assert W.bank_from_files(paths + [grey], "cuda", workers=64) == "bank"
    assert got["device"] == "cuda" and len(got["images"]) == 4
    for a, b in zip(got["images"][:3], imgs):
        assert a.dtype == np.uint8 and np.array_equal(a, b)
    assert got["images"][3].shape == (12, 20, 3) and np.array_equal(got["images"][3][:, :, 1], imgs[0][:, :, 0])


def test_eval_match_argument_checks_need_no_gpu():
    import fdet_amd  # noqa: F401
    from fdet_amd import FdetError, hotpath as hp
    st = hp.EvalState((0.5,), 1000, "cpu")
    pred, cnt = torch.zeros(2, 100, 5), torch.zeros(2, dtype=torch.int32)
    rows, offs = torch.zeros(4, 5), torch.zeros(3, dtype=torch.int32)
    for bad in (dict(pred=torch.zeros(2, 100, 4)), dict(pred=torch.zeros(2, 100, 5, dtype=torch.float64)),
                dict(pred=torch.zeros(2, 5000, 5)), dict(cnt=torch.zeros(3, dtype=torch.int32)),
                dict(cnt=torch.zeros(2, dtype=torch.int64)), dict(rows=torch.zeros(4, 4)), dict(rows=torch.zeros(0, 5)),
                dict(offs=torch.zeros(2, dtype=torch.int32)), dict(offs=torch.zeros(3, dtype=torch.int64)),
                dict(max_gt=5000), dict(max_gt=0), dict(st=None)):
        kw = dict(pred=pred, cnt=cnt, rows=rows, offs=offs, st=st, max_gt=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            hp.eval_match(kw["pred"], kw["cnt"], kw["rows"], kw["offs"], kw["st"], kw["max_gt"])
    with pytest.raises(ValueError):
        hp.EvalState([0.5] * 11, 1000, "cpu")
    with pytest.raises(ValueError):
        hp.EvalState((0.5,), 5000, "cpu")
    with pytest.raises(FdetError):                            # well-formed but on the host: no CPU fallback
        hp.eval_match(pred, cnt, rows, offs, st)


def test_entry_point_rejects_unsupported_sizes_without_a_gpu():
    """Sizes the host knows are refused with a status and a message before anything is enqueued."""
    import ctypes
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    L = _native.lib()
    thr = (ctypes.c_float * 1)(0.5)
    one = ctypes.c_void_p(16)                                # never dereferenced: the checks come first
    ok = dict(B=1, Kmax=100, cap=4, max_gt=4, T=1, n_bins=1000)
    for bad, word in ((dict(Kmax=4865), b"Kmax"), (dict(max_gt=4097), b"max_gt"), (dict(T=11), b"thresholds"),
                      (dict(T=0), b"thresholds"), (dict(n_bins=4097), b"n_bins"), (dict(B=0), b"B=")):
        a = dict(ok)
        a.update(bad)
        rc = L.fdet_eval_match(one, one, a["B"], a["Kmax"], one, one, a["cap"], a["max_gt"], thr, a["T"], a["n_bins"], one,
                               one, one, None, None)
        assert rc == -1 and word in L.fdet_last_error(), (bad, L.fdet_last_error())
    assert L.fdet_eval_match(None, one, 1, 100, one, one, 4, 4, thr, 1, 1000, one, one, one, None, None) == -1
    assert "fdet_eval_match" in _native.header_symbols()


def test_fit_takes_an_evaluator_and_the_script_parses():
    from fdet_amd import run_validation_epoch, trainer
    assert inspect.signature(trainer.fit).parameters["evaluator"].default is None
    with pytest.raises(SystemExit):
        run_validation_epoch.main(["--model", "nonesuch"])
