"""Host-side checks of the WIDER Face protocol evaluation: the sequential restatement (tests/wider_cpu_ref.py) against a
second, histogram-form numpy implementation, a worked example, the .mat reader, the prediction directory, the host
arithmetic of `WiderResult`, and the C-ABI surface of csrc/fdet_eval_wider.hip.  No GPU."""
import os
import re

import numpy as np
import pytest

import wider_cpu_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wider_face_mini_bbx_gt.txt")


def _W():
    import fdet_amd  # noqa: F401
    from fdet_amd import evaluation_wider
    return evaluation_wider


# ---- a second implementation: no walk, two histograms per image (the form the kernel has) -------------------------------
def _bin_of(n, n_bins):
    for t in range(n_bins):
        if n >= 1.0 - np.float64(t + 1) / np.float64(n_bins):
            return t
    return -1                                                           # n < 0 or NaN


def histogram_form(pred, counts, gt_rows, gt_offset, masks, n_subsets, iou_threshold, n_bins, norm=(0.0, 1.0), scale=None):
    prop = np.zeros((n_subsets, n_bins), np.int64)
    hits = np.zeros((n_subsets, n_bins), np.int64)
    for i in range(len(counts)):
        K, g0, g1 = int(counts[i]), int(gt_offset[i]), int(gt_offset[i + 1])
        det = np.asarray(pred[i, :K], np.float32)
        rank = np.empty(K, np.int64)
        rank[R.visiting_order(det[:, 0])] = np.arange(K)
        M = R.overlap_matrix(det[:, 1:], gt_rows[g0:g1, 1:], (1.0, 1.0) if scale is None else scale[i])
        M = np.where(np.isnan(M), -np.inf, M)
        n = R.normalise(det[:, 0], norm)
        bins = [_bin_of(v, n_bins) for v in n]
        cand = [int(np.argmax(M[d])) if g1 > g0 and M[d].max() > -np.inf else -1 for d in range(K)]
        reach = [cand[d] >= 0 and M[d, cand[d]] >= iou_threshold for d in range(K)]
        winner = {}
        for d in range(K):
            if reach[d] and (cand[d] not in winner or rank[d] < rank[winner[cand[d]]]):
                winner[cand[d]] = d
        for s in range(n_subsets):
            for d in range(K):
                keep = reach[d] and bool((int(masks[g0 + cand[d]]) >> s) & 1)
                if bins[d] < 0 or (reach[d] and not keep):
                    continue
                prop[s, bins[d]] += 1
                if keep and winner[cand[d]] == d:
                    hits[s, bins[d]] += 1
    return prop, hits


@pytest.mark.parametrize("seed,n_subsets,n_bins,norm", [(0, 3, 1000, (0.0, 1.0)), (1, 1, 37, (0.0, 1.0)), (2, 8, 100, (0.07, 0.9)),
                                                        (3, 3, 1000, (0.25, 0.5))])
def test_sequential_walk_equals_the_histogram_form(seed, n_subsets, n_bins, norm):
    rng = np.random.default_rng(seed)
    scale = np.c_[rng.uniform(0.5, 2.0, 15), rng.uniform(0.5, 2.0, 15)].astype(np.float32) if seed == 2 else None
    pred, counts, rows, offs, masks = R.random_batch(rng, 15, 60, 60, 7, n_subsets, empty_det=(3,), empty_gt=(4,), all_ignored=(5,),
                                                     scale=scale)
    pred[0, :3, 0] = [np.nan, 1.0, 0.0]
    counts[0] = max(counts[0], 3)
    ex = R.exercised(pred, counts, rows, offs, masks, n_subsets, 0.5, scale)
    assert ex["ignored_hits"] > 0 and ex["duplicates"] > 0 and ex["ties"] > 0, ex
    p0, h0, nf = R.evaluate(pred, counts, rows, offs, masks, n_subsets, 0.5, n_bins, norm, scale)
    p1, h1 = histogram_form(pred, counts, rows, offs, masks, n_subsets, 0.5, n_bins, norm, scale)
    assert np.array_equal(p0, p1) and np.array_equal(h0, h1)
    assert h0.sum() > 0 and (p0.sum(1) < counts.sum()).all()             # something was recalled, something vanished
    want = [sum(int((int(m) >> s) & 1) for m in masks[:offs[-1]]) for s in range(n_subsets)]
    assert nf.tolist() == want


def test_worked_example():
    """Three boxes, five detections, n_bins = 10 (thresholds 0.9, 0.8, ..., 0.0), raw scores.

        boxes (x,y,w,h):  A (0,0,9,9)   B (100,0,9,9)   C (200,0,9,9);   subset 0 keeps A, C;  subset 1 keeps B, C
        detections, given out of order (row: score, box):
            row 0: 0.30 at (300,0,9,9)   overlaps nothing: candidate A (first of the zeros), overlap 0 -> a false proposal
            row 1: 0.80 on C             inclusive areas 100/100, intersection 100: overlap 1
            row 2: 0.95 on A
            row 3: 0.80 on A             ties go by ascending row: row 1 (C) is visited before row 3 (A)
            row 4: 0.85 on B
        visiting order: row 2 (0.95), row 4 (0.85), row 1 (0.80), row 3 (0.80), row 0 (0.30)
        bins (smallest t with score >= 1-(t+1)/10): 0.95 -> 0;  0.85 -> 1;  0.80 (fp32 0.800000012) -> 1 (threshold 0.8);
            0.30 (fp32 0.300000012) -> 6 (threshold 1-0.7 = 0.30000000000000004)
        subset 0: row 2 recalls A; row 4 lands on ignored B and vanishes; row 1 recalls C; row 3 is a duplicate on A: a
            proposal without recall; row 0 a proposal.
            proposals: bin0 1, bin1 2, bin6 1;  hits: bin0 1, bin1 1;  faces 2
            cumulative (proposals, hits): t=0 (1,1); t=1..5 (3,2); t=6..9 (4,2)
            precision 1, 2/3 x5, 1/2 x4; recall 1/2, 1 ...;  AP = 1/2 * 1 + 1/2 * 2/3 = 5/6
        subset 1: row 2 and row 3 land on ignored A and vanish; row 4 recalls B; row 1 recalls C; row 0 a proposal.
            proposals: bin1 2, bin6 1;  hits: bin1 2;  faces 2
            t=0: no proposal: precision 0 (by rule), recall 0; t=1..5 (2,2): precision 1, recall 1;  AP = 1
        The two 0.80 detections tie across threshold t=1: the walk reads its counts at the LAST of them."""
    gt = np.array([[1, 0, 0, 9, 9], [1, 100, 0, 9, 9], [1, 200, 0, 9, 9]], np.float32)
    masks = np.array([0b01, 0b10, 0b11], np.uint32)
    det = np.array([[0.30, 300, 0, 9, 9], [0.80, 200, 0, 9, 9], [0.95, 0, 0, 9, 9], [0.80, 0, 0, 9, 9], [0.85, 100, 0, 9, 9]], np.float32)
    assert R.visiting_order(det[:, 0]).tolist() == [2, 4, 1, 3, 0]
    M = R.overlap_matrix(det[:, 1:], gt[:, 1:])
    assert M[1, 2] == 1.0 and M[2, 0] == 1.0 and (M[0] == 0).all()
    pred, counts, offs = det[None], np.array([5], np.int32), np.array([0, 3], np.int32)
    for impl in ("walk", "hist"):
        if impl == "walk":
            p, h, nf = R.evaluate(pred, counts, gt, offs, masks, 2, 0.5, 10)
        else:
            p, h = histogram_form(pred, counts, gt, offs, masks, 2, 0.5, 10)
        assert p.tolist() == [[1, 2, 0, 0, 0, 0, 1, 0, 0, 0], [0, 2, 0, 0, 0, 0, 1, 0, 0, 0]], impl
        assert h.tolist() == [[1, 1, 0, 0, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0, 0, 0]], impl
    assert nf.tolist() == [2, 2]
    assert R.exercised(pred, counts, gt, offs, masks, 2) == {"ignored_hits": 3, "duplicates": 1, "ties": 1}
    pr0, rc0, ap0 = R.curve(p[0], h[0], 2)
    assert pr0.tolist() == [1.0] + [2 / 3] * 5 + [0.5] * 4 and rc0.tolist() == [0.5] + [1.0] * 9
    assert abs(ap0 - 5 / 6) < 1e-15
    pr1, rc1, ap1 = R.curve(p[1], h[1], 2)
    assert pr1[0] == 0.0 and rc1[0] == 0.0 and ap1 == 1.0
    # the package's host arithmetic gives the same curve
    W = _W()
    r = W.WiderResult(p, h, nf, 1, 5, ("a", "b"), (0.0, 1.0))
    assert r.ap["a"] == ap0 and r.ap["b"] == 1.0 and r.precision["a"].tolist() == pr0.tolist() and r.recall["b"].tolist() == rc1.tolist()
    assert r.n_faces == {"a": 2, "b": 2} and r.to_json()["ap"] == {"a": ap0, "b": 1.0}
    empty = W.WiderResult(np.zeros((1, 10)), np.zeros((1, 10)), [0], 0, 0, ("a",), (0.0, 1.0))
    assert np.isnan(empty.ap["a"]) and empty.to_json()["ap"]["a"] is None


def test_overlap_of_exactly_one_half_counts():
    ov = R.overlap_matrix([[0, 0, 9, 9]], [[0, 0, 9, 19]])
    assert ov[0, 0] == 0.5                                               # inclusive areas 100 and 200, intersection 100
    gt = np.array([[1, 0, 0, 9, 19]], np.float32)
    det = np.array([[[0.9, 0, 0, 9, 9]]], np.float32)
    p, h, nf = R.evaluate(det, [1], gt, [0, 1], np.array([1], np.uint32), 1, 0.5, 10)
    assert h.sum() == 1 and p.sum() == 1


def _golden():
    names, boxes = [], []
    with open(GOLDEN) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    i = 0
    while i < len(lines):
        names.append(lines[i])
        n = int(lines[i + 1])
        rows = [[float(v) for v in ln.split()[:4]] for ln in lines[i + 2:i + 2 + max(n, 1)]]
        boxes.append(np.asarray(rows[:n], np.float64).reshape(-1, 4))
        i += 2 + max(n, 1)
    return names, boxes


def test_from_mat_reads_the_nested_cell_layout(tmp_path):
    pytest.importorskip("scipy.io", reason="scipy is needed to write and read the .mat files")
    W = _W()
    names, boxes = _golden()
    assert len(names) == 4 and [len(b) for b in boxes] == [1, 0, 3, 2]
    keeps = {"easy": [[0], [], [1], [0, 1]], "medium": [[0], [], [0, 1], [0, 1]], "hard": [[0], [], [0, 1, 2], [0, 1]]}
    R.write_mats(str(tmp_path), names, boxes, keeps)
    order = [2, 0, 3, 1]                                                 # bank order differs from file order; full paths
    subsets, got = W.WiderSubsets.from_mat(tmp_path, [f"/data/WIDER_val/images/{names[i]}" for i in order])
    assert subsets.subset_names == ("easy", "medium", "hard") and len(subsets) == 4
    for k, i in enumerate(order):
        assert got[k].dtype == np.float32 and got[k].shape == (len(boxes[i]), 5)
        assert np.array_equal(got[k][:, 1:], boxes[i].astype(np.float32)) and (got[k][:, 0] == 1).all()
        want = np.zeros(len(boxes[i]), np.uint32)
        for s, name in enumerate(("easy", "medium", "hard")):
            want[keeps[name][i]] |= np.uint32(1 << s)
        assert np.array_equal(subsets.masks[k], want)
    assert subsets.masks[0].tolist() == [0b110, 0b111, 0b100]            # the Demonstration image: 1-based gt_list decoded
    one, _ = W.WiderSubsets.from_mat(tmp_path, names[:1], subset_names=("hard",))
    assert one.subset_names == ("hard",) and one.masks[0].tolist() == [1]
    with pytest.raises(KeyError):
        W.WiderSubsets.from_mat(tmp_path, ["9--Nowhere/none.jpg"])
    allk = W.WiderSubsets.all_kept([np.zeros((2, 5)), np.zeros((0, 5))])
    assert allk.subset_names == ("all",) and [m.tolist() for m in allk.masks] == [[1, 1], []]
    assert W.WiderSubsets.from_masks([[5, 0]]).masks[0].dtype == np.uint32


def test_prediction_directory_round_trip(tmp_path):
    W = _W()
    rng = np.random.default_rng(11)
    pred, counts, rows, offs, masks = R.random_batch(rng, 6, 40, 40, 5, 3, empty_det=(2,))
    pred[:, :, 1:] += rng.uniform(0, 1, pred[:, :, 1:].shape).astype(np.float32)        # values that need all 9 digits
    pred[0, 0, 0] = np.float32(1) / np.float32(3)
    names = [f"{i % 2}--Event{i % 2}/{i % 2}_Event_img_{i:03d}.jpg" for i in range(6)]
    W.write_wider_pred_dir(tmp_path / "pred", names, pred, counts)
    txt = (tmp_path / "pred" / "0--Event0" / "0_Event_img_000.txt").read_text().splitlines()
    assert txt[0] == "0_Event_img_000" and int(txt[1]) == counts[0] and len(txt) == 2 + counts[0]
    sc = [float(ln.split()[4]) for ln in txt[2:]]
    assert sc == sorted(sc, reverse=True) and len(txt[2].split()) == 5
    got_names, got_rows, got_counts = W.read_wider_pred_dir(tmp_path / "pred")
    keys = [W.image_key(n) for n in names]
    assert sorted(keys) == got_names
    back = [got_names.index(k) for k in keys]                           # the directory comes back sorted by name
    assert np.array_equal(got_counts[back], counts)
    for i, b in enumerate(back):                                        # same float32 values, in descending score
        want = pred[i, :counts[i]][R.visiting_order(pred[i, :counts[i], 0])]
        assert np.array_equal(got_rows[b, :counts[i]], want)
    K = got_rows.shape[1]
    a = R.evaluate(pred, counts, rows, offs, masks, 3, 0.5, 1000)
    b = R.evaluate(got_rows[back], got_counts[back], rows, offs, masks, 3, 0.5, 1000)
    assert K <= 40 and all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].sum() > 0


def test_cabi_rejects_bad_sizes_without_a_gpu():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native, hotpath as hp
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    L = _native.lib()
    assert "fdet_eval_wider" in _native.header_symbols() and "fdet_eval_wider" in _native.SIGNATURES
    txt = open(_native.HEADER_PATH).read()
    assert re.search(r"#define FDET_EVAL_WIDER_MAX_SUBSETS 8\b", txt) and hp.EVAL_WIDER_MAX_SUBSETS == 8

    def call(B=1, Kmax=100, n_subsets=3, max_gt=16, n_bins=1000, p=None):
        return L.fdet_eval_wider(p, p, B, Kmax, None, p, p, 8, p, n_subsets, max_gt, 0.5, None, n_bins, p, p, p, None)

    for kw, word in (({"n_subsets": 0}, b"n_subsets"), ({"n_subsets": 9}, b"n_subsets"), ({"n_bins": hp.EVAL_MAX_BINS + 1}, b"n_bins"),
                     ({"n_bins": 0}, b"n_bins"), ({"Kmax": hp.EVAL_MAX_DET + 1}, b"Kmax"), ({"max_gt": hp.EVAL_MAX_GT + 1}, b"max_gt"),
                     ({"B": 0}, b"B=0"), ({}, b"null")):
        assert call(**kw) == -1, kw
        assert word in L.fdet_last_error(), (kw, L.fdet_last_error())
    with pytest.raises(ValueError):
        hp.WiderState(n_subsets=9)
    with pytest.raises(ValueError):
        hp.WiderState(n_bins=hp.EVAL_MAX_BINS + 1)


def test_generated_assembly_has_no_scalar_memory_store_or_scalar_atomic(tmp_path):
    """csrc/fdet_eval_wider.hip cross-compiled to gfx950 assembly: the atomics are the LDS min and add and the 32- and 64-bit
    vector adds on the histograms and counters.  (That no multiply-add is contracted is what the exact comparisons of
    tests/test_gpu_wider.py show; the build passes -ffp-contract=off and the file carries the pragma.)"""
    import shutil
    import subprocess
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(os.path.dirname(_native.LIB_PATH), "..", "csrc")
    out = tmp_path / "fdet_eval_wider.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.dirname(_native.HEADER_PATH),
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(csrc, "fdet_eval_wider.hip")], check=True, capture_output=True)
    text = out.read_text()
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\b", text, flags=re.M)
    scalar_mem = [o for o in ops if re.match(r"s_(store|buffer_store|scratch_store|atomic|buffer_atomic|dcache_wb|dcache_discard)", o)]
    assert not scalar_mem, sorted(set(scalar_mem))
    atomics = sorted({o for o in ops if "atomic" in o})
    assert atomics == ["global_atomic_add", "global_atomic_add_x2"], atomics
    lds_rmw = sorted({o for o in ops if re.match(r"ds_(min|max|add|sub|inc|dec|and|or|xor|cmpst|wrxchg)", o)})
    assert lds_rmw == ["ds_add_u32", "ds_min_u32"], lds_rmw
    assert "k_eval_wider" in text
    assert "clang fp contract(off)" in open(os.path.join(csrc, "fdet_eval_wider.hip")).read()
