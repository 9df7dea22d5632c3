"""fdet_track_refine without a GPU: the restatement (tests/track_refine_cpu_ref.py) on the hand-made cases of
tests/track_refine_cases.py, whose expected rows are written out here; its properties on the random sequences; and the host
validation of the C entry, which launches nothing."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cpu_ref as R  # noqa: E402
import track_refine_cases as C  # noqa: E402
import track_refine_cpu_ref as RR  # noqa: E402


COVER = dict(lookback=5, grow256=0, stitch_gap=10, stitch_iou=0.3, min_length=1)


def refine(inp, **par):
    return RR.track_refine(*(inp[k] for k in C.ARGS), **{**C.OFF, **par})


def rows_of(out, t):
    """[(id, kind, misses, [x, y, w, h]), ...] of frame t."""
    n = int(out[4][t])
    return [(int(out[1][t, k]), int(out[3][t, k]), int(out[2][t, k]), out[0][t, k, 1:].tolist()) for k in range(n)]


# ------------------------------------------------------------------------------------------ hand-made
def test_linear_motion_is_interpolated_exactly():
    inp, true = C.linear_motion()
    assert inp["trk_counts"].tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    out = refine(inp)
    for t in range(10):
        kind, misses = (2, t - 3) if t in (4, 5, 6) else (0, 0)
        assert rows_of(out, t) == [(1, kind, misses, true[t].tolist())], t
    assert out[6]["kind2"] == 3 and out[5] == [0, 0]


def test_half_steps_round_up_on_both_signs():
    out = refine(C.half_steps())
    assert rows_of(out, 1) == [(1, 2, 1, [12.0, 49.0, 20.0, 20.0])]        # 10 + 1.5 -> 12, 50 - 1.5 -> 49
    assert RR.interpolate((10, 50, 30, 70), (13, 47, 33, 67), 0, 2, 1) == (12, 49, 32, 69)


@pytest.mark.parametrize("grow256", [0, 13, 256])
def test_back_fill_is_cut_by_lookback_and_grows(grow256):
    out = refine(C.late_face(), lookback=3, grow256=grow256)
    assert out[4].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    for t in (3, 4, 5):
        m = 6 - t
        gx, gy = (grow256 * m * 16 + 256) >> 9, (grow256 * m * 24 + 256) >> 9
        assert rows_of(out, t) == [(1, 3, m, [100.0 - gx, 80.0 - gy, 16.0 + 2 * gx, 24.0 + 2 * gy])], t
        assert out[0][t, 0, 0] == np.float32(0.8)
    assert rows_of(out, 6) == [(1, 0, 0, [100.0, 80.0, 16.0, 24.0])]
    if grow256 == 256:
        assert rows_of(out, 3)[0][3] == [76.0, 44.0, 64.0, 96.0]


def test_back_fill_stops_at_the_start_of_its_sequence():
    out = refine(C.late_face(), lookback=1024)
    assert out[4].tolist() == [1] * 10 and [rows_of(out, t)[0][1:3] for t in range(6)] == [(3, 6 - t) for t in range(6)]
    assert out[6]["backfill_clipped"] == 1 and out[6]["backfill_unclipped"] == 0
    out = refine(C.two_sequences(), lookback=5)                # the face of sequence 1 is born in frame 5, its second frame
    assert out[4].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert [r[0][:2] for r in (rows_of(out, t) for t in range(9))] == [(1, 0)] * 4 + [(1, 3)] + [(1, 0)] * 4
    assert rows_of(out, 3)[0][3] == [30.0, 30.0, 20.0, 20.0] and rows_of(out, 4)[0][3] == [100.0, 80.0, 16.0, 24.0]


def test_unconfirmed_detections_come_back_from_det_rows():
    inp = C.unconfirmed()
    assert inp["trk_counts"].tolist() == [0, 0, 1, 1, 1, 1] and inp["det_ids"][:, 0].tolist() == [1] * 6
    out = refine(inp)
    assert out[4].tolist() == [1] * 6 and out[3][:, 0].tolist() == [0] * 6 and out[1][:, 0].tolist() == [1] * 6
    for t in (0, 1):
        assert out[0][t, 0].tobytes() == inp["det_rows"][t, 0].tobytes()
    for t in range(2, 6):
        assert out[0][t, 0].tobytes() == inp["trk_rows"][t, 0].tobytes()


def test_stitching_gives_one_id_and_an_interpolated_gap():
    inp = C.reappears()
    assert sorted(set(inp["trk_ids"][inp["trk_ids"] > 0].tolist())) == [1, 2] and inp["trk_counts"].tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    out = refine(inp, stitch_gap=4)
    assert out[6]["stitches"] == 1 and out[4].tolist() == [1] * 10 and set(out[1][:, 0].tolist()) == {1}
    assert out[3][:, 0].tolist() == [0, 0, 0, 2, 2, 2, 2, 0, 0, 0] and out[2][:, 0].tolist() == [0, 0, 0, 1, 2, 3, 4, 0, 0, 0]
    assert [rows_of(out, t)[0][3][0] for t in (3, 4, 5, 6)] == [50.0, 51.0, 51.0, 52.0]       # 50.4, 50.8, 51.2, 51.6
    for par in (dict(stitch_gap=3), dict(stitch_gap=-1)):                                   # the gap is stitch_gap + 1; never
        out = refine(inp, **par)
        assert out[6]["stitches"] == 0 and out[1][7:, 0].tolist() == [2, 2, 2] and out[3][3, 0] == 1 and out[4][4:7].tolist() == [0, 0, 0]
    tie = C.reappears(second=(60, 40, 30, 20))                 # inter 400, uni 800
    assert refine(tie, stitch_gap=10, stitch_iou=0.5)[6]["stitches"] == 0                   # strict >
    assert refine(tie, stitch_gap=10, stitch_iou=0.4999)[6]["stitches"] == 1


def test_stitching_needs_an_earlier_last_anchor_and_prefers_the_lower_id():
    out = refine(C.later_anchor(), stitch_gap=10, stitch_iou=0.1)
    assert out[6]["stitches"] == 0 and out[1][7, :2].tolist() == [1, 2]
    inp = C.equal_candidates()
    assert inp["det_ids"][5, 0] == 3
    out = refine(inp, stitch_gap=10, stitch_iou=0.1)
    assert out[6]["stitches"] == 1 and out[1][5:, 0].tolist() == [1, 1, 1] and out[4][5:].tolist() == [1, 1, 1]
    assert rows_of(out, 3) == [(1, 2, 2, [10.0, 40.0, 30.0, 20.0])]      # chain 1 from x = 0 to x = 20; track 2 has died
    out = refine(C.three_fragments(), stitch_gap=3)
    assert out[6]["stitches"] == 2 and out[4].tolist() == [1] * 12 and set(out[1][:, 0].tolist()) == {1}
    assert refine(C.three_fragments())[6]["stitches"] == 0


def test_min_length_drops_the_false_positive_and_keeps_the_stitched_fragments():
    inp = C.three_fragments(false_positive=True, fragments=2)
    assert inp["trk_ids"][2, :2].tolist() == [1, 2] and inp["trk_ids"][3, 0] == 2 and inp["trk_misses"][3, 0] == 1
    out = refine(inp, stitch_gap=3, min_length=3)
    assert out[6]["dropped_chains"] == 1 and out[6]["stitches"] == 1
    assert out[4].tolist() == [1] * 7 + [1] + [0] * 4 and set(out[1][:8, 0].tolist()) == {1} and not (out[1] == 2).any()
    out = refine(inp, min_length=3)                           # unstitched, every chain is too short
    assert out[6]["dropped_chains"] == 3 and not out[4].any()


def test_room_and_order():
    inp = C.room()
    out = refine(inp, lookback=2)
    assert out[5] == [0, 128] and out[4].tolist() == [256, 256, 128]
    assert out[1][0].tolist() == list(range(1, 257)) and out[3][0].tolist() == [0] * 128 + [3] * 128
    assert out[1][1].tolist() == list(range(129, 385)) and out[3][1].tolist() == [0] * 128 + [3] * 128
    out = refine(inp, lookback=1)
    assert out[5] == [0, 0] and out[4].tolist() == [256, 256, 128]


def test_empty_inputs_and_rejection():
    inp = C.empties()
    out = refine(inp, lookback=1)
    assert out[5] == [0, 0] and out[4].tolist() == [1, 1, 1, 1] + [1] * 8 and rows_of(out, 0)[0][1] == 3
    bad = {**inp, "trk_counts": inp["trk_counts"].copy()}
    bad["trk_counts"][9] = 129
    out = refine(bad, lookback=1)
    assert out[5] == [1, 0] and out[4].tolist() == [1] * 8 + [0] * 4 and not out[0][8:].any() and not out[1][8:].any()
    for key, value in (("trk_counts", -1), ("trk_ids", 0), ("trk_ids", 5000), ("trk_rows", np.nan)):
        bad = {**inp, key: inp[key].copy()}
        bad[key][(9,) if key == "trk_counts" else (9, 0) if key == "trk_ids" else (9, 0, 1)] = value
        assert refine(bad)[5][0] == 1, (key, value)
    none = {k: inp[k][:0] for k in C.ARGS[:-1]}
    out = refine({**none, "seq_offset": np.array([0, 0], np.int32)})
    assert out[0].shape == (0, 256, 5) and out[5] == [0, 0]
    out = refine(C.carried_over(), lookback=3, min_length=5)   # no anchor: nothing concerns it
    assert [rows_of(out, t) for t in range(3)] == [[(1, 1, t + 1, [50.0, 40.0, 30.0, 20.0])] for t in range(3)]


# ------------------------------------------------------------------------------------------ random sequences
def test_the_random_set_exercises_every_step():
    total = dict.fromkeys(RR.STAT_KEYS, 0)
    for tracker in C.TRACKERS:
        for par in C.PARAMS:
            out = refine(C.random_inputs(tracker), **par)
            assert out[5][0] == 0
            for t in range(out[0].shape[0]):
                ids = out[1][t, :out[4][t]]
                assert len(set(ids.tolist())) == len(ids) and (ids > 0).all(), "a chain twice in one frame"
            for k in RR.STAT_KEYS:
                total[k] += out[6][k]
    assert all(total[k] > 0 for k in RR.STAT_KEYS), total


@pytest.mark.parametrize("tracker", list(C.TRACKERS))
def test_detected_and_coasted_rows_are_rows_of_the_input(tracker):
    inp = C.random_inputs(tracker)
    out = refine(inp, **C.PARAMS[0])
    seen = {0: 0, 1: 0}
    for t in range(out[0].shape[0]):
        c = int(inp["trk_counts"][t])
        coasted = {(inp["trk_rows"][t, p].tobytes(), int(inp["trk_misses"][t, p])) for p in range(c) if inp["trk_misses"][t, p] != 0}
        detected = {inp["trk_rows"][t, p].tobytes() for p in range(c) if inp["trk_misses"][t, p] == 0} | \
            {inp["det_rows"][t, j].tobytes() for j in range(inp["det_rows"].shape[1]) if inp["det_ids"][t, j] > 0}
        for k in range(int(out[4][t])):
            kind = int(out[3][t, k])
            if kind == 0:
                assert out[0][t, k].tobytes() in detected and out[2][t, k] == 0
            elif kind == 1:
                assert (out[0][t, k].tobytes(), int(out[2][t, k])) in coasted
            seen[kind] = seen.get(kind, 0) + 1
    assert seen[0] > 100 and seen[1] > 0


def test_a_neutral_pass_reorders_the_input_by_id():
    rows, counts = R.synthetic_sequence(40, 16, 32, faces=8, negative=True)
    inp = C.online(rows, counts, [0, 40], alpha256=128, max_misses=0, min_hits=1)          # a track dies with its first miss
    out = refine(inp)
    assert out[5] == [0, 0] and np.array_equal(out[4], inp["trk_counts"]) and not out[3].any() and not out[2].any()
    for t in range(40):
        c = int(inp["trk_counts"][t])
        order = np.argsort(inp["trk_ids"][t, :c], kind="stable")
        assert np.array_equal(out[1][t, :c], inp["trk_ids"][t, :c][order])
        assert out[0][t, :c].tobytes() == inp["trk_rows"][t, :c][order].tobytes()
        assert not out[0][t, c:].any() and not out[1][t, c:].any()


def _inside(row, true_t):
    """Which of the frame's true boxes have their centre inside the row's box."""
    x, y, w, h = (float(v) for v in row[1:])
    cx, cy = true_t[:, 0] + true_t[:, 2] / 2, true_t[:, 1] + true_t[:, 3] / 2
    return (cx >= x) & (cx <= x + w) & (cy >= y) & (cy <= y + h)


def _faces_of_tracks(inp, true):
    """Online id -> the face whose centre most of the detections given that id hold (none: no face)."""
    votes = {}
    for t, j in zip(*np.nonzero(inp["det_ids"] > 0)):
        votes.setdefault(int(inp["det_ids"][t, j]), np.zeros(true.shape[1], np.int64))[:] += _inside(inp["det_rows"][t, j], true[t])
    return {i: int(np.argmax(v)) for i, v in votes.items() if v.max() > 0}


def _members(inp, out):
    """Chain id -> the online ids whose detections it holds: a row of kind 0 is a row of the input, byte for byte."""
    members = {}
    for t in range(out[0].shape[0]):
        c = int(inp["trk_counts"][t])
        src = {inp["trk_rows"][t, p].tobytes(): int(inp["trk_ids"][t, p]) for p in range(c) if inp["trk_misses"][t, p] == 0}
        emitted = set(inp["trk_ids"][t, :c].tolist())
        for j in np.nonzero(inp["det_ids"][t] > 0)[0]:
            if int(inp["det_ids"][t, j]) not in emitted:
                src[inp["det_rows"][t, j].tobytes()] = int(inp["det_ids"][t, j])
        for k in range(int(out[4][t])):
            if out[3][t, k] == 0:
                members.setdefault(int(out[1][t, k]), set()).add(src[out[0][t, k].tobytes()])
    return members


def _covered(rows, ids, counts, faces_of, true):
    """{(face, t)}: the truth's centre lies inside a box emitted under an id that belongs to the face."""
    got = set()
    for t in range(rows.shape[0]):
        for k in range(int(counts[t])):
            hit = _inside(rows[t, k], true[t])
            got.update((f, t) for f in faces_of.get(int(ids[t, k]), ()) if hit[f])
    return got


@pytest.mark.parametrize("tracker", list(C.TRACKERS))
def test_refined_rows_cover_more_of_the_truth(tracker):
    """A chain is the right one for a face when one of the online tracks stitched into it is, and an online track belongs to
    the face that most of its detections hold.  Stitching asks for the overlap the online tracker asks for (0.3): two faces
    that cross are then no more one chain than they are one track."""
    inp = C.sub_sequence(C.random_inputs(tracker), 3)
    T, seed, neg = C.SEEDS[3]
    true = C.truth(T, seed, negative=neg)
    out = refine(inp, **COVER)
    face_of = _faces_of_tracks(inp, true)
    before = _covered(inp["trk_rows"], inp["trk_ids"], inp["trk_counts"], {i: (f,) for i, f in face_of.items()}, true)
    chains = {c: {face_of[j] for j in m if j in face_of} for c, m in _members(inp, out).items()}
    after = _covered(out[0], out[1], out[4], chains, true)
    assert before <= after, sorted(before - after)[:10]
    assert len(after) > len(before) > 0.5 * T * true.shape[1], (len(before), len(after))


# ------------------------------------------------------------------------------------------ the C entry and the script
def _call(L, inp, T=None, n_seq=None, ws_bytes=None, null=(), **par):
    """fdet_track_refine on host arrays used as if they were device memory: only good for calls that launch nothing."""
    par = {**dict(lookback=5, grow256=0, stitch_gap=10, stitch_iou=0.1, min_length=1), **par}
    T = inp["trk_rows"].shape[0] if T is None else T
    K = inp["det_rows"].shape[1]
    off = np.ascontiguousarray(inp["seq_offset"], np.int32)
    n_seq = off.size - 1 if n_seq is None else n_seq
    need = L.fdet_track_refine_ws_bytes(n_seq, T)
    outs = {k: np.zeros((max(T, 1), 256, 5), np.float32) for k in ("out_rows", "out_ids", "out_misses", "out_kind", "out_counts")}
    bufs = {**{k: np.ascontiguousarray(inp[k]) for k in C.ARGS[:-1]}, **outs, "ws": np.zeros(max(need, 4), np.uint8),
            "seq_offset": off, "h_seq_offset": off, "rejected": np.zeros(2, np.uint64)}
    p = {k: (None if k in null else v.ctypes.data) for k, v in bufs.items()}
    return L.fdet_track_refine(p["det_rows"], p["det_ids"], K, p["trk_rows"], p["trk_ids"], p["trk_misses"], p["trk_counts"],
                               p["seq_offset"], p["h_seq_offset"], n_seq, T, par["lookback"], par["grow256"], par["stitch_gap"],
                               par["stitch_iou"], par["min_length"], p["out_rows"], p["out_ids"], p["out_misses"], p["out_kind"],
                               p["out_counts"], p["ws"], need if ws_bytes is None else ws_bytes, p["rejected"], None)


def test_host_validation_launches_nothing():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    L = _native.lib()
    inp = C.two_sequences()
    assert L.fdet_track_refine_ws_bytes(2, 9) == 9 * (128 * 32 + 4) and L.fdet_track_refine_ws_bytes(1, 0) == 0
    assert L.fdet_track_refine_ws_bytes(0, 9) == 0
    bad = [dict(lookback=-1), dict(lookback=1025), dict(grow256=-1), dict(grow256=257), dict(stitch_gap=65536), dict(stitch_iou=-0.1),
           dict(stitch_iou=1.0), dict(stitch_iou=float("nan")), dict(min_length=0), dict(ws_bytes=9 * (128 * 32 + 4) - 1),
           dict(n_seq=0), dict(T=-1), dict(T=8)]
    bad += [dict(null=(k,)) for k in C.ARGS + ("h_seq_offset", "out_rows", "out_ids", "out_misses", "out_kind", "out_counts", "ws",
                                               "rejected")]
    for kw in bad:
        assert _call(L, inp, **kw) == -1, kw
        assert b"fdet_track_refine" in L.fdet_last_error(), kw
    for off in ([1, 4, 9], [0, 5, 4], [0, 4, 8], [0, 10, 9]):
        assert _call(L, {**inp, "seq_offset": np.array(off, np.int32)}) == -1, off
    none = {**{k: inp[k][:0] for k in C.ARGS[:-1]}, "seq_offset": np.array([0, 0, 0], np.int32)}
    assert _call(L, none, null=C.ARGS[:-1] + ("out_rows", "out_ids", "out_misses", "out_kind", "out_counts", "ws")) == 0      # T = 0


def test_python_layers_check_their_arguments():
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tracking
    assert (hotpath.TRACK_REFINE_ROWS, hotpath.TRACK_REFINE_MAX_IDS) == (RR.ROWS, RR.MAX_IDS)
    assert tracking.RefinedTracks._fields == ("rows", "counts", "ids", "misses", "kind") and tracking.RefinedTracks.overflow == 0
    assert "guesses" in tracking.refine_tracks.__doc__
    with pytest.raises(ValueError):
        tracking.TrackLog(0)
    with pytest.raises(ValueError, match="nothing"):
        tracking.TrackLog().refine()
    log = tracking.TrackLog(2)
    res = tracking.TrackResult(torch.zeros(3, 128, 5), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 128, dtype=torch.int32),
                               torch.zeros(3, 128, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="seq_offset"):
        log.append(torch.zeros(3, 4, 5), res)
    with pytest.raises(ValueError, match="seq_offset"):
        log.append(torch.zeros(3, 4, 5), res, [0, 2, 1])
    with pytest.raises(ValueError, match="belong"):
        log.append(torch.zeros(2, 4, 5), res, [0, 1, 2])
    log.append(torch.zeros(3, 4, 5), res, [0, 1, 3])
    assert len(log) == 3


def test_track_frames_refine_options(tmp_path):
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import track_frames
    Image.new("RGB", (8, 6)).save(tmp_path / "f000.png")
    seen = {}
    real, track_frames.run = track_frames.run, lambda args: seen.update(vars(args))
    try:
        base = ["--frames", str(tmp_path), "--out", str(tmp_path / "o.txt")]
        track_frames.main(base)
        assert seen["refine"] is False
        track_frames.main(base + ["--refine", "--lookback", "7", "--stitch-gap", "-1", "--stitch-iou", "0.25", "--min-length", "3",
                                  "--coast-grow", "0.125"])
        assert (seen["refine"], seen["lookback"], seen["stitch_gap"], seen["stitch_iou"], seen["min_length"], seen["coast_grow"]) == \
            (True, 7, -1, 0.25, 3, 0.125)
        for wrong in (["--lookback", "1025"], ["--stitch-iou", "1.0"], ["--min-length", "0"], ["--stitch-gap", "70000"]):
            with pytest.raises(SystemExit):
                track_frames.main(base + ["--refine"] + wrong)
    finally:
        track_frames.run = real
