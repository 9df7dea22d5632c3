"""fdet_track_refine / tracking.refine_tracks / tracking.TrackLog on the GPU against the restatement on Python
ints (tests/track_refine_cpu_ref.py), on the cases of tests/track_refine_cases.py.  No tolerance anywhere: every comparison is
equality of all five outputs and of both counters."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cpu_ref as RC  # noqa: E402
import track_cpu_ref as R  # noqa: E402
import track_refine_cases as C  # noqa: E402
import track_refine_cpu_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tracking
    return hotpath, tracking


def _device(inp, **par):
    hp, _ = _mods()
    par = {**C.OFF, **par}
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in C.ARGS}
    out = hp.track_refine(*(t[k] for k in C.ARGS), np.ascontiguousarray(inp["seq_offset"], np.int32), par["lookback"],
                          par["grow256"], par["stitch_gap"], par["stitch_iou"], par["min_length"])
    return tuple(o.cpu().numpy() for o in out[:5]) + (out[5].cpu().tolist(),)


def _same(got, want, what=""):
    for name, a, b in zip(RR.NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}{name}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
        assert a.tobytes() == b.tobytes(), f"{what}{name} differs at {np.argwhere(a != b)[:5].tolist()}"
    assert got[5] == want[5], f"{what}rejected {got[5]} vs {want[5]}"


def _both(inp, **par):
    got = _device(inp, **par)
    want = RR.track_refine(*(inp[k] for k in C.ARGS), **{**C.OFF, **par})
    _same(got, want)
    return got, want[6]


def _tensors(res):
    return tuple(t.cpu().numpy() for t in (res.rows, res.ids, res.misses, res.kind, res.counts))


# ------------------------------------------------------------------------------------------ hand-made
HAND = {
    "linear": (lambda: C.linear_motion()[0], [dict()]),
    "half_steps": (C.half_steps, [dict()]),
    "late_face": (C.late_face, [dict(lookback=3, grow256=g) for g in (0, 13, 256)] + [dict(lookback=1024), dict(lookback=6, grow256=256)]),
    "two_sequences": (C.two_sequences, [dict(lookback=5), dict(lookback=1, grow256=64)]),
    "unconfirmed": (C.unconfirmed, [dict(), dict(lookback=2, min_length=6), dict(min_length=7)]),
    "reappears": (C.reappears, [dict(stitch_gap=4), dict(stitch_gap=3), dict(stitch_gap=-1, lookback=2), dict(stitch_gap=65535, stitch_iou=0.0)]),
    "threshold": (lambda: C.reappears(second=(60, 40, 30, 20)), [dict(stitch_gap=10, stitch_iou=0.5), dict(stitch_gap=10, stitch_iou=0.4999)]),
    "later_anchor": (C.later_anchor, [dict(stitch_gap=10)]),
    "equal_candidates": (C.equal_candidates, [dict(stitch_gap=10), dict(stitch_gap=10, lookback=3, grow256=40)]),
    "three_fragments": (C.three_fragments, [dict(stitch_gap=3), dict(stitch_gap=2), dict(), dict(stitch_gap=3, min_length=7)]),
    "false_positive": (lambda: C.three_fragments(True, 2), [dict(stitch_gap=3, min_length=3), dict(min_length=3), dict(min_length=2)]),
    "room": (C.room, [dict(lookback=2), dict(lookback=1), dict(lookback=2, min_length=2)]),
    "carried_over": (C.carried_over, [dict(lookback=3, min_length=5, stitch_gap=10)]),
    "empties": (C.empties, [dict(lookback=1), dict(lookback=4, stitch_gap=5)]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_cases(name):
    make, params = HAND[name]
    inp = make()
    for par in params:
        got, stats = _both(inp, **par)
    if name == "linear":
        true = C.linear_motion()[1]
        assert np.array_equal(got[0][:, 0, 1:], true.astype(np.float32)) and got[3][:, 0].tolist() == [0] * 4 + [2] * 3 + [0] * 3
    if name == "room":                                      # the last parameters drop every chain: one anchor each
        assert not got[4].any() and stats["dropped_chains"] == 384
        got, _ = _both(inp, lookback=2)
        assert got[5] == [0, 128] and got[1][0].tolist() == list(range(1, 257)) and got[3][0].tolist() == [0] * 128 + [3] * 128


def test_rejection_beside_good_sequences_and_no_frames():
    inp = C.empties()
    for key, where, value in (("trk_counts", (9,), 129), ("trk_counts", (5,), -1), ("trk_ids", (9, 0), 0), ("trk_ids", (9, 0), 4097),
                              ("trk_rows", (9, 0, 3), np.inf), ("det_ids", (2, 3), 4500)):
        bad = {**inp, key: inp[key].copy()}
        bad[key][where] = value
        got, _ = _both(bad, lookback=1)
        s = 3 if where[0] >= 8 else 2 if where[0] >= 4 else 1
        a, b = int(inp["seq_offset"][s]), int(inp["seq_offset"][s + 1])
        assert got[5] == [1, 0] and not got[4][a:b].any() and got[4].sum() == 12 - (b - a), (key, value)
    ok = {**inp, "trk_ids": np.where(inp["trk_ids"] > 0, inp["trk_ids"] + 2_000_000_000, 0).astype(np.int32),
          "det_ids": np.where(inp["det_ids"] > 0, inp["det_ids"] + 2_000_000_000, 0).astype(np.int32)}
    got, _ = _both(ok, lookback=1)                             # only the span of the ids is bounded
    assert got[5] == [0, 0] and got[1].max() == 2_000_000_001
    span = {**inp, "det_ids": inp["det_ids"].copy()}
    span["det_ids"][2, 3] = 4096                               # an unconfirmed detection with the last id the tables hold
    span["det_rows"] = inp["det_rows"].copy()
    span["det_rows"][2, 3] = (0.5, 200, 200, 10, 10)
    got, _ = _both(span, lookback=1)                           # 1..4096 is the widest span
    assert got[5] == [0, 0] and 4096 in got[1][2].tolist()
    none = {**{k: inp[k][:0] for k in C.ARGS[:-1]}, "seq_offset": np.array([0, 0, 0], np.int32)}
    got, _ = _both(none)
    assert got[0].shape == (0, 256, 5) and got[5] == [0, 0]


def test_more_anchors_than_slots_in_a_frame_is_rejected():
    inp = C.room()
    bad = {**inp, "det_ids": inp["det_ids"].copy()}
    bad["det_ids"][0, 5] = 300                                 # an id that frame 0 does not emit: a 129th anchor
    got, _ = _both(bad)
    assert got[5] == [1, 0]


# ------------------------------------------------------------------------------------------ random sequences
@pytest.mark.parametrize("tracker", list(C.TRACKERS))
def test_random_sequences(tracker):
    inp = C.random_inputs(tracker)
    total = dict.fromkeys(RR.STAT_KEYS, 0)
    for par in C.PARAMS:
        got, stats = _both(inp, **par)
        assert got[5][0] == 0 and got[4].sum() > 500
        for k in RR.STAT_KEYS:
            total[k] += stats[k]
    assert total["kind2"] > 0 and total["kind3"] > 0 and total["kind1"] > 0 and total["stitches"] > 0 and total["dropped_chains"] > 0


# ------------------------------------------------------------------------------------------ the Python layers
@functools.lru_cache(maxsize=None)
def _video():
    return R.synthetic_sequence(40, 16, 33, faces=8, negative=True, dropout=0.3)


def test_track_log_does_not_depend_on_the_chunks():
    _, tracking = _mods()
    rows, counts = _video()
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    kw = dict(max_misses=2, min_hits=2, motion="constant_velocity", coast_grow=0.125)
    par = dict(lookback=4, coast_grow=0.125, stitch_gap=8, stitch_iou=0.2, min_length=2)
    outs = []
    for chunk in (40, 7, 1):
        tr, log = tracking.FaceTracker(**kw), tracking.TrackLog()
        for a in range(0, 40, chunk):
            log.append(d_rows[a:a + chunk], tr.update(d_rows[a:a + chunk], d_counts[a:a + chunk]))
        assert len(log) == 40
        ref = log.refine(**par)
        assert ref.seq_offset.tolist() == [0, 40] and ref.position.tolist() == list(range(40)) and ref.tracks.overflow == 0
        outs.append(_tensors(ref.tracks))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a.tobytes() == b.tobytes()
    inp = C.online(rows, counts, [0, 40], motion=dict(beta256=128, damp256=256, max_speed=64, grow256=32), alpha256=128, max_misses=2,
                   min_hits=2)
    want = RR.track_refine(*(inp[k] for k in C.ARGS), lookback=4, grow256=32, stitch_gap=8, stitch_iou=0.2, min_length=2)
    _same(outs[0] + ([0, 0],), want)
    assert want[6]["kind2"] > 0 and want[6]["kind3"] > 0


def test_track_log_gathers_two_sequences():
    """Two cameras tracked in calls that hold frames of both: refine sees each camera's frames together, in time order."""
    _, tracking = _mods()
    rows, counts = _video()
    other = R.synthetic_sequence(24, 16, 34, faces=5)
    cams = [(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()), (torch.from_numpy(other[0]).cuda(), torch.from_numpy(other[1]).cuda())]
    tr, log = tracking.FaceTracker(2, min_hits=1, max_misses=2), tracking.TrackLog(2)
    cuts = [((0, 10), (0, 0)), ((10, 25), (0, 20)), ((25, 40), (20, 24))]
    for (a0, a1), (b0, b1) in cuts:
        r = torch.cat([cams[0][0][a0:a1], cams[1][0][b0:b1]])
        c = torch.cat([cams[0][1][a0:a1], cams[1][1][b0:b1]])
        off = [0, a1 - a0, a1 - a0 + b1 - b0]
        log.append(r, tr.update(r, c, off), off)
    ref = log.refine(lookback=3, stitch_gap=5)
    assert ref.seq_offset.tolist() == [0, 40, 64]
    assert ref.position.tolist() == list(range(0, 10)) + list(range(10, 25)) + list(range(45, 60)) + list(range(25, 45)) + list(range(60, 64))
    whole = tracking.FaceTracker(2, min_hits=1, max_misses=2)
    r, c = torch.cat([cams[0][0], cams[1][0]]), torch.cat([cams[0][1], cams[1][1]])
    direct = tracking.refine_tracks(r, whole.update(r, c, [0, 40, 64]), [0, 40, 64], lookback=3, stitch_gap=5)
    for a, b in zip(_tensors(ref.tracks), _tensors(direct)):
        assert a.tobytes() == b.tobytes()
    inp = C.online(r.cpu().numpy(), c.cpu().numpy(), [0, 40, 64], alpha256=128, max_misses=2, min_hits=1)
    _same(_tensors(direct) + ([0, 0],), RR.track_refine(*(inp[k] for k in C.ARGS), lookback=3, stitch_gap=5))


def test_refine_tracks_reports_rejection_and_overflow():
    _, tracking = _mods()
    from fdet_amd import FdetError
    inp = C.room()
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in C.ARGS}
    res = tracking.TrackResult(t["trk_rows"], t["trk_counts"], t["trk_ids"], t["trk_misses"], t["det_ids"])
    ref = tracking.refine_tracks(t["det_rows"], res, lookback=2, stitch_gap=-1)
    assert ref.overflow == 128 and ref.counts.tolist() == [256, 256, 128] and ref.rows.shape == (3, 256, 5)
    broken = res._replace(counts=torch.tensor([128, 129, 128], dtype=torch.int32, device="cuda"))
    with pytest.raises(FdetError, match="fdet_track_refine"):
        tracking.refine_tracks(t["det_rows"], broken)
    with pytest.raises(FdetError, match="lookback"):
        tracking.refine_tracks(t["det_rows"], res, lookback=2000)


def test_refined_rows_render_like_any_rows():
    """K = 256 rows per frame into the renderer: the pixelated frames are those of tests/render_cpu_ref.py."""
    _, tracking = _mods()
    from fdet_amd.datasets import augment as A
    from fdet_amd.render import render_detections
    inp, true = C.linear_motion()
    g = np.random.default_rng(5)
    images = [g.integers(0, 256, (64, 96, 3)).astype(np.uint8) for _ in range(10)]
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).cuda() for k in C.ARGS}
    res = tracking.TrackResult(t["trk_rows"], t["trk_counts"], t["trk_ids"], t["trk_misses"], t["det_ids"])
    ref = tracking.refine_tracks(t["det_rows"], res, lookback=0, stitch_gap=-1)
    assert ref.rows.shape == (10, 256, 5) and ref.counts.tolist() == [1] * 10
    bank = A.DeviceImageBank.from_arrays(images, "cuda")
    drawn = render_detections(bank, ref.rows, ref.counts, anonymize="pixelate").to_arrays()
    expect = RC.render(images, ref.rows.cpu().numpy(), ref.counts.cpu().numpy(), True, True, 8)
    true_rows = np.zeros((10, 1, 5), np.float32)
    true_rows[:, 0, 0], true_rows[:, 0, 1:] = 0.8, true
    by_truth = RC.render(images, true_rows, np.ones(10, np.int32), True, True, 8)
    for i in range(10):
        assert np.array_equal(drawn[i], expect[i]) and np.array_equal(drawn[i], by_truth[i]), i
    online = render_detections(bank, res.rows, res.counts, anonymize="pixelate").to_arrays()
    assert all(np.array_equal(online[i], images[i]) for i in (4, 5, 6))            # what the pass buys: the frames of the gap


def test_track_frames_refine_script(tmp_path, monkeypatch):
    """The frames of test_gpu_track.test_track_frames_script: with --refine the MOT text holds TrackLog.refine's rows, without
    it the online tracker's."""
    from PIL import Image
    _, tracking = _mods()
    from fdet_amd import track_frames
    monkeypatch.chdir(tmp_path)
    g = np.random.default_rng(3)
    base = g.integers(0, 256, (12, 16, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(5):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(frames / f"f{i:03d}.png")
    common = ["--frames", str(frames), "--model", "poolresnet", "--filters", "64", "--probability-threshold", "0.02",
              "--min-hits", "1", "--max-misses", "2", "--max-frames", "2"]
    seen = {"online": [], "refined": []}
    real_update, real_refine = tracking.FaceTracker.update, tracking.TrackLog.refine

    def update(self, *a, **k):
        seen["online"].append(real_update(self, *a, **k))
        return seen["online"][-1]

    def refine(self, **k):
        seen["refined"].append(real_refine(self, **k))
        return seen["refined"][-1]

    monkeypatch.setattr(tracking.FaceTracker, "update", update)
    monkeypatch.setattr(tracking.TrackLog, "refine", refine)

    def text(rows, counts, ids):
        import io
        f = io.StringIO()
        track_frames.write_mot(f, 1, rows.cpu().numpy(), counts.cpu().numpy(), ids.cpu().numpy())
        return f.getvalue()

    torch.manual_seed(11)
    plain = track_frames.main(common + ["--out", str(tmp_path / "plain.txt")])
    assert not seen["refined"] and len(seen["online"]) == 3
    cat = [torch.cat([getattr(r, f) for r in seen["online"]]) for f in ("rows", "counts", "ids")]
    assert (tmp_path / "plain.txt").read_text() == text(*cat) and plain["lines"] > 0
    torch.manual_seed(11)
    out = track_frames.main(common + ["--out", str(tmp_path / "refined.txt"), "--refine", "--lookback", "3", "--draw", str(tmp_path / "drawn"),
                                      "--anonymize", "pixelate"])
    ref = seen["refined"][0].tracks
    got = (tmp_path / "refined.txt").read_text()
    assert got == text(ref.rows, ref.counts, ref.ids) and out["lines"] == int(ref.counts.sum()) >= plain["lines"]
    assert [ln.split(",")[1] for ln in got.splitlines()] == [str(int(i)) for t in range(5) for i in ref.ids[t, :int(ref.counts[t])]]
    assert (ref.kind == 0).sum() > 0 and sorted(p.name for p in (tmp_path / "drawn").iterdir()) == [f"f{i:03d}.png" for i in range(5)]
