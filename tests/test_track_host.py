"""Host-side checks of the tracker: the numpy restatement's own invariants, the C-ABI's argument validation
and the frame script's refusal of mixed frame sizes.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cpu_ref as R  # noqa: E402

T, K = 40, 16
PARAMS = dict(iou_threshold=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=None, birth_score=0.0)


def _run(rows, counts, chunks, **kw):
    """The sequence fed in `chunks` consecutive calls -> (state, concatenated outputs, per-frame snapshots of the last call)."""
    p = {**PARAMS, **kw}
    state = R.fresh_state(1)
    outs, a = [], 0
    for n in chunks:
        outs.append(R.track_update(rows[a:a + n], counts[a:a + n], [0, n], state, **p))
        a += n
    assert a == len(counts) and all(o[5] == 0 for o in outs)
    return state, [np.concatenate([o[i] for o in outs]) for i in range(5)]


@pytest.mark.parametrize("seed,negative", [(0, False), (1, True), (2, False)])
def test_ids_unique_and_never_reused(seed, negative):
    rows, counts = R.synthetic_sequence(T, K, seed, negative=negative)
    state = R.fresh_state(1)
    seen_alive, dead = {}, set()
    for t in range(T):
        out_rows, out_ids, out_misses, out_counts, det_ids, rej = R.track_update(rows[t:t + 1], counts[t:t + 1], [0, 1], state,
                                                                                 **PARAMS)
        assert rej == 0
        tr = state[0]["tracks"]
        ids = tr["id"][tr["id"] != 0]
        assert len(set(ids.tolist())) == len(ids)                              # unique among the live tracks
        assert not (set(ids.tolist()) & dead)                                  # a dead id never comes back
        dead |= set(seen_alive) - set(ids.tolist())
        for i in ids.tolist():
            seen_alive[i] = t
        live = tr[tr["id"] != 0]
        assert (live["x2q"] - live["x1q"] >= 16).all() and (live["y2q"] - live["y1q"] >= 16).all()
        n = int(out_counts[0])
        assert len(set(out_ids[0, :n].tolist())) == n and (out_ids[0, :n] > 0).all() and (out_ids[0, n:] == 0).all()
        assert (out_rows[0, :n, 3] >= 1).all() and (out_rows[0, :n, 4] >= 1).all()
        got = det_ids[0][det_ids[0] != 0]
        assert len(set(got.tolist())) == len(got)                              # one detection per track and frame
    assert int(state[0]["seq"]["next_id"]) == len(seen_alive) + len(dead - set(seen_alive)) and state[0]["seq"]["frame"] == T
    assert len(dead) > 0 and max(seen_alive) == int(state[0]["seq"]["next_id"])


def test_the_generator_covers_the_cases():
    rows, counts = R.synthetic_sequence(T, K, 1, negative=True)
    valid = rows[np.arange(K)[None] < counts[:, None]]
    assert (valid[:, 1] < 0).any() and (valid[:, 2] < 0).any()                 # the floor shift is exercised
    assert counts.min() < 4 and counts.max() > 4                               # dropouts and false positives
    assert (np.abs(valid[:, 1:] - np.rint(valid[:, 1:])) > 0.01).any()


@pytest.mark.parametrize("alpha256", [64, 256])
def test_chunks_give_the_state_and_outputs_of_one_pass(alpha256):
    rows, counts = R.synthetic_sequence(T, K, 3, negative=True)
    s_one, o_one = _run(rows, counts, [T], alpha256=alpha256)
    assert o_one[3].sum() > T and o_one[2].max() >= 1                          # tracks are emitted, and some bridged
    for chunks in ([1] * T, [13, 13, 13, 1], [26, 14], [1, 13, 26]):
        s, o = _run(rows, counts, chunks, alpha256=alpha256)
        assert s.tobytes() == s_one.tobytes()
        for a, b in zip(o, o_one):
            assert np.array_equal(a, b)


def test_bridging_and_emission_rules():
    face = np.array([0.9, 10.4, 12.6, 20.0, 24.0], np.float32)
    rows = np.zeros((6, 2, 5), np.float32)
    rows[:, 0] = face
    counts = np.array([1, 1, 0, 0, 1, 1], np.int32)
    state = R.fresh_state(1)
    out_rows, out_ids, out_misses, out_counts, det_ids, _ = R.track_update(rows, counts, [0, 6], state, 0.3, 256, 3, 1, 3, 0.0)
    assert out_counts.tolist() == [1] * 6 and out_ids[:, 0].tolist() == [1] * 6
    assert out_misses[:, 0].tolist() == [0, 0, 1, 2, 0, 0]
    assert out_rows[3, 0].tolist() == [np.float32(0.9), 10.0, 13.0, 20.0, 24.0]      # rint(30.4) - rint(10.4), rint(36.6) - 13
    assert det_ids[:, 0].tolist() == [1, 1, 0, 0, 1, 1]
    # emit_misses = 0 never bridges; min_hits = 2 holds the first frame back; max_misses = 1 kills the track in the gap
    state = R.fresh_state(1)
    o = R.track_update(rows, counts, [0, 6], state, 0.3, 256, 1, 2, 0, 0.0)
    assert o[3].tolist() == [0, 1, 0, 0, 0, 1] and o[1][:, 0].tolist() == [0, 1, 0, 0, 0, 2]


def _lib():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


def test_state_bytes():
    L = _lib()
    assert L.fdet_track_state_bytes(3) == 3 * 6160
    assert L.fdet_track_state_bytes(1) == 6160 and L.fdet_track_state_bytes(0) == 0 and L.fdet_track_state_bytes(-2) == 0


def test_dtype_sizes():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tracking
    assert tracking.SEQ_DTYPE.itemsize == 16 and tracking.TRACK_DTYPE.itemsize == 48
    assert tracking.STATE_DTYPE.itemsize == 6160 == hotpath.TRACK_STATE_BYTES
    assert tracking.TRACK_DTYPE == R.TRACK_DTYPE and tracking.SEQ_DTYPE == R.SEQ_DTYPE
    assert (hotpath.TRACK_SLOTS, hotpath.TRACK_MAX_DETS, hotpath.TRACK_MAX_COORD) == (R.SLOTS, R.MAX_DETS, R.MAX_COORD)
    assert tracking.alpha_to_256(0.5) == 128 and tracking.alpha_to_256(1.0) == 256 and tracking.alpha_to_256(0.002) == 1
    for bad in (0.0, 0.001, 1.01, -0.5):
        with pytest.raises(ValueError):
            tracking.alpha_to_256(bad)


# every pointer of the call is a dummy non-null address: validation must return before anything dereferences a device one
GOOD = dict(n_seq=2, T=4, K=3, iou=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=5, offs=(0, 1, 4))
BAD = [
    ("offset does not start at 0", dict(offs=(1, 2, 4))),
    ("offset does not end at T", dict(offs=(0, 2, 3))),
    ("offset not monotone", dict(offs=(0, 5, 4))),
    ("n_seq < 1", dict(n_seq=0)),
    ("T < 0", dict(T=-1)),
    ("K < 0", dict(K=-1)),
    ("alpha256 = 0", dict(alpha256=0)),
    ("alpha256 = 257", dict(alpha256=257)),
    ("max_misses < 0", dict(max_misses=-1, emit_misses=0)),
    ("min_hits < 1", dict(min_hits=0)),
    ("emit_misses < 0", dict(emit_misses=-1)),
    ("emit_misses > max_misses", dict(emit_misses=6)),
    ("iou_threshold = 1", dict(iou=1.0)),
    ("iou_threshold < 0", dict(iou=-0.1)),
    ("iou_threshold NaN", dict(iou=float("nan"))),
] + [(f"null pointer {i}", dict(null=i)) for i in (0, 1, 2, 3, 13, 14, 15, 16, 17, 18, 19)]


@pytest.mark.parametrize("why,change", BAD, ids=[b[0] for b in BAD])
def test_host_validation_needs_no_gpu(why, change):
    L = _lib()
    a = {**GOOD, **change}
    h_off = np.asarray(a["offs"], np.int32)
    dummy = ctypes.c_void_p(4096)
    args = [dummy, dummy, dummy, h_off.ctypes.data, a["n_seq"], a["T"], a["K"], a["iou"], a["alpha256"], a["max_misses"],
            a["min_hits"], a["emit_misses"], 0.0, dummy, dummy, dummy, dummy, dummy, dummy, dummy, None]
    if "null" in a:
        args[a["null"]] = None
    assert L.fdet_track_update(*args) == -1, why                               # FDET_EINVAL
    assert b"fdet_track_update" in L.fdet_last_error()


def test_script_refuses_mixed_frame_sizes(tmp_path, capsys):
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import track_frames
    for i, size in enumerate([(8, 6), (8, 6), (6, 8)]):
        Image.new("RGB", size, (i, 2 * i, 3 * i)).save(tmp_path / f"f{i:03d}.png")
    assert [p.name for p in track_frames.frame_paths(tmp_path)] == ["f000.png", "f001.png", "f002.png"]
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--frames", str(tmp_path), "--out", str(tmp_path / "out.txt")])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "one size" in err and "f002.png" in err and "6x8" in err
    assert not (tmp_path / "out.txt").exists()
    (tmp_path / "f002.png").unlink()
    assert track_frames.frame_size(track_frames.frame_paths(tmp_path)) == (8, 6)


def test_mot_lines(tmp_path):
    import fdet_amd  # noqa: F401
    from fdet_amd import track_frames
    rows = np.zeros((2, 128, 5), np.float32)
    rows[0, 0] = (0.875, 3, -4, 10, 12)
    rows[1, :2] = [(0.5, 4, -3, 10, 12), (0.25, 100, 50, 20, 20)]
    ids = np.zeros((2, 128), np.int32)
    ids[0, 0], ids[1, :2] = 7, (7, 9)
    with open(tmp_path / "mot.txt", "w") as f:
        assert track_frames.write_mot(f, 5, rows, np.array([1, 2], np.int32), ids) == 3
    assert (tmp_path / "mot.txt").read_text().splitlines() == [
        "5,7,3,-4,10,12,0.8750,-1,-1,-1", "6,7,4,-3,10,12,0.5000,-1,-1,-1", "6,9,100,50,20,20,0.2500,-1,-1,-1"]
