"""fdet_track_update / FaceTracker on the GPU against the numpy restatement (tests/track_cpu_ref.py).
No tolerance anywhere: every comparison is equality of all five outputs and of the state."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cpu_ref as RR  # noqa: E402
import track_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
NAMES = ("out_rows", "out_ids", "out_misses", "out_counts", "det_ids")


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tracking
    return hotpath, tracking


def _device(rows, counts, seq_offset, state, iou_threshold=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=None,
            birth_score=0.0):
    """fdet_track_update on host arrays with the restatement's signature: `state` ((n_seq,) records) is modified in place."""
    hp, _ = _mods()
    h_off = np.ascontiguousarray(np.asarray(seq_offset, np.int32))
    d_state = torch.from_numpy(state.view(np.uint8).copy()).cuda()
    out = hp.track_update(torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda(), torch.from_numpy(h_off).cuda(), h_off,
                          d_state, iou_threshold, alpha256, max_misses, min_hits, max_misses if emit_misses is None else emit_misses,
                          birth_score)
    state[...] = d_state.cpu().numpy().view(R.STATE_DTYPE)
    return tuple(o.cpu().numpy() for o in out[:5]) + (int(out[5].item()),)


def _same(got, want, what=""):
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}{name}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
        assert np.array_equal(a, b), f"{what}{name} differs at {np.argwhere(a != b)[:5].tolist()}"
    assert got[5] == want[5], f"{what}rejected {got[5]} vs {want[5]}"


def _both(rows, counts, seq_offset, n_seq, state=None, **kw):
    """The same call on the device and in the restatement from the same state -> (device outputs, device state)."""
    s_dev = R.fresh_state(n_seq) if state is None else state.copy()
    s_ref = s_dev.copy()
    got = _device(rows, counts, seq_offset, s_dev, **kw)
    want = R.track_update(rows, counts, seq_offset, s_ref, **kw)
    _same(got, want)
    assert s_dev.tobytes() == s_ref.tobytes(), "state differs"
    return got, s_dev


# ------------------------------------------------------------------------------------------ random sequences
@functools.lru_cache(maxsize=None)
def _three_sequences():
    parts = [R.synthetic_sequence(1, 16, 10), R.synthetic_sequence(7, 16, 11, negative=True),
             R.synthetic_sequence(40, 16, 12, faces=5, negative=True)]
    rows, counts = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return rows, counts, np.array([0, 1, 8, 48], np.int32)


@pytest.mark.parametrize("alpha256", [64, 256])
def test_random_sequences(alpha256):
    _, tracking = _mods()
    rows, counts, off = _three_sequences()
    valid = rows[np.arange(16)[None] < counts[:, None]]
    assert (valid[:, 1] < 0).any() and (valid[:, 2] < 0).any()
    got, state = _both(rows, counts, off, 3, alpha256=alpha256)
    assert got[3].sum() > 40 and got[2].max() >= 1 and int(state["seq"]["next_id"].min()) >= 1
    assert (state["tracks"]["x1q"] < 0).any()                                 # the floor shift saw negative corners
    # the same through FaceTracker, whose snapshot() is the state
    tr = tracking.FaceTracker(n_seq=3, alpha=alpha256 / 256)
    res = tr.update(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), off)
    _same(tuple(t.cpu().numpy() for t in (res.rows, res.ids, res.misses, res.counts, res.det_ids)) + (0,), got)
    snap = tr.snapshot()
    assert snap.dtype == tracking.STATE_DTYPE and snap.tobytes() == state.tobytes()
    assert tr.dropped == 0
    tr.reset()
    assert not tr.snapshot().view(np.uint8).any()


def test_chunk_invariance_on_the_device():
    _, tracking = _mods()
    rows, counts = R.synthetic_sequence(40, 16, 13, negative=True)
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    one = tracking.FaceTracker()
    whole = one.update(d_rows, d_counts)
    parts = tracking.FaceTracker()
    res, a = [], 0
    for n in (1, 13, 26):
        res.append(parts.update(d_rows[a:a + n], d_counts[a:a + n]))
        a += n
    for f in tracking.TrackResult._fields:
        assert torch.equal(torch.cat([getattr(r, f) for r in res]), getattr(whole, f)), f
    assert torch.equal(parts.state, one.state)
    s_ref = R.fresh_state(1)
    want = R.track_update(rows, counts, [0, 40], s_ref)
    _same(tuple(t.cpu().numpy() for t in (whole.rows, whole.ids, whole.misses, whole.counts, whole.det_ids)) + (0,), want)
    assert one.snapshot().tobytes() == s_ref.tobytes()


# ------------------------------------------------------------------------------------------ ties
def test_ties_go_to_the_lower_slot_then_the_lower_row():
    kw = dict(iou_threshold=0.05, alpha256=256, min_hits=1)
    # two identical tracks, two identical detections: slot 0 takes row 0, slot 1 row 1 (the scores tell them apart)
    rows = np.zeros((2, 4, 5), np.float32)
    rows[0, :2] = [(0.5, 10, 10, 20, 20), (0.5, 10, 10, 20, 20)]
    rows[1, :2] = [(0.9, 10, 10, 20, 20), (0.8, 10, 10, 20, 20)]
    got, state = _both(rows, np.array([2, 2], np.int32), [0, 2], 1, **kw)
    assert got[4][1].tolist() == [1, 2, 0, 0]
    assert state[0]["tracks"]["score"][:2].tolist() == [np.float32(0.9), np.float32(0.8)]
    # one detection equally good for two tracks: the lower slot takes it, the other misses
    rows = np.zeros((2, 4, 5), np.float32)
    rows[0, :2] = [(0.5, 30, 0, 20, 20), (0.5, 0, 0, 20, 20)]                  # slot 0 is the RIGHT box
    rows[1, 0] = (0.7, 15, 0, 20, 20)
    got, state = _both(rows, np.array([2, 1], np.int32), [0, 2], 1, **kw)
    assert got[4][1].tolist() == [1, 0, 0, 0]
    assert state[0]["tracks"]["misses"][:2].tolist() == [0, 1] and state[0]["tracks"]["x1q"][0] == 15 * 16
    # two detections equally good for one track: the lower row takes it, the other is born
    rows = np.zeros((2, 4, 5), np.float32)
    rows[0, 0] = (0.5, 15, 0, 20, 20)
    rows[1, :2] = [(0.6, 30, 0, 20, 20), (0.7, 0, 0, 20, 20)]
    got, state = _both(rows, np.array([1, 2], np.int32), [0, 2], 1, **kw)
    assert got[4][1].tolist() == [1, 2, 0, 0] and state[0]["tracks"]["x1q"][:2].tolist() == [30 * 16, 0]


# ------------------------------------------------------------------------------------------ wave boundaries
def _grid_boxes(n, g, jitter):
    """n boxes of 50x50 on a 16 x 16 grid of 40-pixel cells (neighbours overlap), cell order, jittered by up to `jitter`."""
    i = np.arange(n)
    b = np.stack([np.full(n, 0.6), 40.0 * (i % 16) - 100, 40.0 * (i // 16) - 100, np.full(n, 50.0), np.full(n, 50.0)], 1)
    b[:, 1:] += g.integers(-jitter, jitter + 1, (n, 4))
    b[:, 0] += g.uniform(0, 0.3, n)
    return b.astype(np.float32)


@pytest.mark.parametrize("n_tracks", [63, 64, 65, 128])
def test_wave_boundaries(n_tracks):
    dets = (63, 64, 65, 255, 256)
    g = np.random.default_rng(n_tracks)
    K = 256
    rows = np.zeros((2 * len(dets), K, 5), np.float32)
    counts = np.zeros(2 * len(dets), np.int32)
    for s, n_d in enumerate(dets):
        rows[2 * s, :n_tracks], counts[2 * s] = _grid_boxes(n_tracks, g, 0), n_tracks
        rows[2 * s + 1, :n_d], counts[2 * s + 1] = _grid_boxes(n_d, g, 4)[g.permutation(n_d)], n_d
    got, state = _both(rows, counts, 2 * np.arange(len(dets) + 1), len(dets), iou_threshold=0.05, alpha256=192, min_hits=1)
    for s, n_d in enumerate(dets):
        assert int(got[3][2 * s]) == n_tracks                                  # every first-frame box is a track
        assert int((got[4][2 * s + 1] != 0).sum()) == min(n_d, 128 + min(n_d, n_tracks) - n_tracks)
        assert int(state[s]["seq"]["dropped"]) == max(0, n_d - n_tracks - (128 - n_tracks))


# ------------------------------------------------------------------------------------------ limits
def test_slot_exhaustion_drops_the_highest_rows():
    _, tracking = _mods()
    i = np.arange(130)
    rows = np.zeros((1, 160, 5), np.float32)
    rows[0, :130] = np.stack([np.full(130, 0.5), 30.0 * (i % 16), 30.0 * (i // 16), np.full(130, 20.0), np.full(130, 20.0)], 1)
    counts = np.array([130], np.int32)
    got, state = _both(rows, counts, [0, 1], 1, min_hits=1)
    assert int(state[0]["seq"]["dropped"]) == 2 and int(state[0]["seq"]["next_id"]) == 128
    assert got[4][0, :128].tolist() == list(range(1, 129)) and got[4][0, 128:].tolist() == [0] * 32
    assert int(got[3][0]) == 128
    tr = tracking.FaceTracker(min_hits=1)
    tr.update(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda())
    assert tr.dropped == 2


def test_invalid_rows_are_ignored():
    bad = [(NAN, 10, 10, 20, 20), (INF, 10, 10, 20, 20), (0.5, NAN, 10, 20, 20), (0.5, 10, -INF, 20, 20), (0.5, 10, 10, INF, 20),
           (0.5, 10, 10, 20, NAN), (0.5, 10, 10, 0.4, 20), (0.5, 10, 10, 20, 0.0), (0.5, 10, 10, -5, 20),
           (0.5, 16380, 10, 5, 20),                                            # X2 = 16385
           (0.5, 10, -16385, 20, 20), (0.5, 3e38, 10, 3e38, 20), (0.5, 1e9, 10, 20, 20),
           (0.5, 1.5, 10, 1.0, 20),                                            # rint(1.5) = rint(2.5) = 2: width 0
           (0.5, 10, 0.5, 20, 1.0)]                                            # rint(0.5) = 0, rint(1.5) = 2: VALID, height 2
    good = [(0.5, 16364, -16384, 20, 20), (0.5, 100, 100, 20, 20)]             # corners at the limit are valid
    frame = np.asarray(bad[:7] + good[:1] + bad[7:] + good[1:], np.float32)
    valid_at = [7, len(frame) - 2, len(frame) - 1]
    rows = np.zeros((3, 24, 5), np.float32)
    rows[:, :len(frame)] = frame
    rows[:, len(frame):] = NAN                                                 # past the count: never read
    counts = np.full(3, len(frame), np.int32)
    got, state = _both(rows, counts, [0, 3], 1, min_hits=1, alpha256=256)
    want_ids = np.zeros(24, np.int32)
    want_ids[valid_at] = (1, 2, 3)
    for t in range(3):
        assert got[4][t].tolist() == want_ids.tolist()
    assert int(got[3][2]) == 3 and int(state[0]["seq"]["next_id"]) == 3
    assert state[0]["tracks"]["y1q"][:3].tolist() == [-16384 * 16, 0, 100 * 16]


def test_largest_boxes():
    """Sides of 2^15, areas of 2^30, a union of 2^31 and cross products near 2^61: the widest values the limits admit."""
    L = 16384.0
    rows = np.zeros((3, 6, 5), np.float32)
    rows[0, :3] = [(0.5, -L, -L, 2 * L, 2 * L), (0.6, -L, -L, 2 * L, L), (0.7, 0, 0, L, L)]
    rows[1, :5] = [(0.5, -L, -L + 1, 2 * L, 2 * L - 1), (0.6, -L, -L, 2 * L, L - 1), (0.7, 1, 0, L - 1, L),
                   (0.8, -L, -L, 2 * L, 2 * L), (0.9, -L, 0, L, L)]
    rows[2, :4] = [(0.5, -L, -L, 2 * L, 2 * L), (0.5, -L, -L, 2 * L - 1, 2 * L), (0.5, -L, -L, 2 * L, 2 * L - 1), (0.5, -L, -L, 1, 1)]
    counts = np.array([3, 5, 4], np.int32)
    for thr, alpha256 in ((0.0, 256), (0.3, 128), (0.999, 1)):
        got, state = _both(rows, counts, [0, 3], 1, iou_threshold=thr, alpha256=alpha256, min_hits=1)
        assert int(got[3][0]) == 3 and got[4][1, 3] == 1                       # the identical full box is track 1 again
    # a pair whose boxes only touch has no overlap; boxes at opposite corners give the widest union
    rows = np.zeros((2, 2, 5), np.float32)
    rows[0, 0] = (0.5, -L, -L, L, L)
    rows[1, :2] = [(0.5, 0, 0, L, L), (0.5, -1, -1, L + 1, L + 1)]
    got, _ = _both(rows, np.array([1, 2], np.int32), [0, 2], 1, iou_threshold=0.0, min_hits=1)
    assert got[4][1].tolist() == [2, 1]


@pytest.mark.parametrize("case", ["count_above_K", "count_negative", "257_valid_rows"])
def test_rejection_leaves_the_sequence_as_it_was(case):
    hp, tracking = _mods()
    from fdet_amd import FdetError
    K = 300 if case == "257_valid_rows" else 16
    parts = [R.synthetic_sequence(n, 16, 20 + i) for i, n in enumerate((5, 6, 7))]
    rows = np.zeros((18, K, 5), np.float32)
    rows[:, :16] = np.concatenate([p[0] for p in parts])
    counts = np.concatenate([p[1] for p in parts])
    off = np.array([0, 5, 11, 18], np.int32)
    _, before = _both(rows, counts, off, 3, min_hits=1)                        # a state with live tracks in every sequence
    assert (before["tracks"]["id"] != 0).any(axis=1).all()
    if case == "257_valid_rows":
        i = np.arange(257)
        rows[8, :257] = np.stack([np.full(257, 0.5), 30.0 * (i % 20), 30.0 * (i // 20), np.full(257, 20.0), np.full(257, 20.0)], 1)
        counts[8] = 257
    else:
        counts[8] = K + 1 if case == "count_above_K" else -1                   # frame 8 is the fourth frame of sequence 1
    got, after = _both(rows, counts, off, 3, state=before, min_hits=1)
    assert got[5] == 1
    assert after[1].tobytes() == before[1].tobytes()
    assert after[0].tobytes() != before[0].tobytes() and after[2].tobytes() != before[2].tobytes()
    for o in got[:5]:
        assert not o[5:11].any()
    assert got[3][:5].sum() > 0 and got[3][11:].sum() > 0
    # FaceTracker raises, and goes on from the states the call left
    tr = tracking.FaceTracker(n_seq=3, min_hits=1)
    tr.state.copy_(torch.from_numpy(before.view(np.uint8).copy()))
    with pytest.raises(FdetError, match="1 sequence"):
        tr.update(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), off)
    assert tr.snapshot().tobytes() == after.tobytes()


# ------------------------------------------------------------------------------------------ end to end
def test_bridging_closes_the_gap_of_a_pixelated_sequence():
    _, tracking = _mods()
    from fdet_amd.datasets import augment as A
    from fdet_amd.render import render_detections
    g = np.random.default_rng(5)
    images = [g.integers(0, 256, (48, 64, 3)).astype(np.uint8) for _ in range(6)]
    bank = A.DeviceImageBank.from_arrays(images, "cuda")
    rows = np.zeros((6, 4, 5), np.float32)
    rows[:, 0] = (0.9, 20.3, 10.6, 24.0, 20.0)
    counts = np.array([1, 1, 0, 0, 1, 1], np.int32)
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    tr = tracking.FaceTracker(max_misses=3, min_hits=1)
    res = tr.update(d_rows, d_counts)
    want = R.track_update(rows, counts, [0, 6], R.fresh_state(1), max_misses=3, min_hits=1)
    _same(tuple(t.cpu().numpy() for t in (res.rows, res.ids, res.misses, res.counts, res.det_ids)) + (0,), want)
    assert res.counts.tolist() == [1] * 6 and res.ids[:, 0].tolist() == [1] * 6
    assert res.misses[:, 0].tolist() == [0, 0, 1, 2, 0, 0]
    bridged = render_detections(bank, res.rows, res.counts, anonymize="pixelate").to_arrays()
    expect = RR.render(images, want[0], want[3], True, True, 8)
    for a, b in zip(bridged, expect):
        assert np.array_equal(a, b)
    for t in (2, 3):
        assert not np.array_equal(bridged[t], images[t])                       # covered in the gap
    raw = render_detections(bank, d_rows, d_counts, anonymize="pixelate").to_arrays()
    for t in (2, 3):
        assert np.array_equal(raw[t], images[t])                               # the per-frame anonymiser shows the face
    assert not np.array_equal(raw[0], images[0])


def test_through_the_model():
    _, tracking = _mods()
    from fdet_amd.models.PoolResnet import PoolResnet
    torch.manual_seed(7)
    model = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.5,
                       iou_threshold=0.3).cuda().eval()
    g = torch.Generator().manual_seed(8)
    base = torch.randint(0, 256, (1, 3, 480, 480), dtype=torch.uint8, generator=g)
    noise = torch.randint(0, 8, (8, 3, 480, 480), dtype=torch.uint8, generator=g)
    frames = (base // 2 + noise).cuda()                                        # eight frames that differ a little
    from fdet_amd.datasets.utils import ReduceBoundingBoxes
    with torch.no_grad():
        maps = model.forward_frames(frames)
        for pt in (0.5, 0.3, 0.1, 0.02, 0.001):                                # untrained weights: the first threshold with output
            reducer = ReduceBoundingBoxes(pt, 0.3, model.reduce_bounding_boxes.input_shape, 10)
            rows, counts = reducer.forward_batch(maps)
            if int(counts.min()) > 0:
                break
    assert rows.shape == (8, 100, 5) and int(counts.sum()) > 0
    tr = tracking.FaceTracker(min_hits=1)
    res = tr.update(rows, counts)
    s_ref = R.fresh_state(1)
    want = R.track_update(rows.cpu().numpy(), counts.cpu().numpy(), [0, 8], s_ref, min_hits=1)
    _same(tuple(t.cpu().numpy() for t in (res.rows, res.ids, res.misses, res.counts, res.det_ids)) + (0,), want)
    assert tr.snapshot().tobytes() == s_ref.tobytes()
    assert int(res.counts.sum()) > 0


def test_track_frames_script(tmp_path, monkeypatch):
    """The frame script end to end on an untrained network: chunked detection with the state carried over gives the text of
    one chunk, every line is a MOTChallenge line, and --draw writes one image per frame."""
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import track_frames
    monkeypatch.chdir(tmp_path)
    g = np.random.default_rng(3)
    base = g.integers(0, 256, (12, 16, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)          # 96 x 128, blocky
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(5):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(frames / f"f{i:03d}.png")
    common = ["--frames", str(frames), "--model", "poolresnet", "--filters", "64", "--probability-threshold", "0.02",
              "--min-hits", "1", "--max-misses", "2"]
    torch.manual_seed(11)
    one = track_frames.main(common + ["--out", str(tmp_path / "one.txt")])
    torch.manual_seed(11)
    parts = track_frames.main(common + ["--out", str(tmp_path / "parts.txt"), "--max-frames", "2", "--draw", str(tmp_path / "drawn"),
                                        "--anonymize", "pixelate"])
    text = (tmp_path / "one.txt").read_text()
    assert text == (tmp_path / "parts.txt").read_text() and one == parts
    lines = text.splitlines()
    assert one["frames"] == 5 and one["lines"] == len(lines) > 0 and one["tracks"] > 0
    seen = set()
    for ln in lines:
        f = ln.split(",")
        assert len(f) == 10 and f[7:] == ["-1", "-1", "-1"] and 1 <= int(f[0]) <= 5 and int(f[1]) >= 1
        assert (int(f[0]), int(f[1])) not in seen and int(f[4]) >= 1 and int(f[5]) >= 1
        seen.add((int(f[0]), int(f[1])))
    drawn = sorted(p.name for p in (tmp_path / "drawn").iterdir())
    assert drawn == [f"f{i:03d}.png" for i in range(5)]
    assert Image.open(tmp_path / "drawn" / "f000.png").size == (128, 96)
