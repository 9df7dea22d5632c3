"""Host-side checks of the tracker's motion model: the restatement tests/track_motion_cpu_ref.py against
tests/track_cpu_ref.py with neutral parameters, its exact prediction of constant motion, its bounds with hand-computed
values, and the argument validation of fdet_track_update_motion and FaceTracker.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cpu_ref as R  # noqa: E402
import track_motion_cpu_ref as RM  # noqa: E402

M = R.MAX_COORD


# ------------------------------------------------------------------------------------------ neutral parameters
@pytest.mark.parametrize("seed,negative,alpha256,max_speed", [(0, False, 128, 64), (1, True, 64, 0), (2, True, 256, 1024)])
def test_neutral_parameters_give_the_old_rule(seed, negative, alpha256, max_speed):
    rows, counts = R.synthetic_sequence(40, 16, seed, negative=negative)
    for damp256 in (256, 77):
        s_old, s_new = R.fresh_state(1), R.fresh_state(1)
        a, b = 0, 0
        for n in (13, 27):                                                    # two calls: the carried state too
            old = R.track_update(rows[a:a + n], counts[a:a + n], [0, n], s_old, alpha256=alpha256)
            new = RM.track_update_motion(rows[a:a + n], counts[a:a + n], [0, n], s_new, alpha256=alpha256, beta256=0,
                                         damp256=damp256, max_speed=max_speed, grow256=0)
            a += n
            for x, y in zip(old[:5], new[:5]):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            assert old[5] == new[5] == 0 and s_old.tobytes() == s_new.tobytes()
            b += int(old[3].sum())
        assert b > 40 and not s_new["tracks"]["reserved"].any()


def test_rejection_leaves_the_velocities():
    rows, counts, _ = RM.moving_face()
    state = R.fresh_state(1)
    RM.track_update_motion(rows[:4], counts[:4], [0, 4], state, **RM.MOVING_PARAMS, **RM.MOVING_MOTION)
    assert state[0]["tracks"]["reserved"][0].tolist() == [6 * 256, 2 * 256, 0]
    before = state.copy()
    bad = counts[4:8].copy()
    bad[2] = 5                                                                # K = 4
    out = RM.track_update_motion(rows[4:8], bad, [0, 4], state, **RM.MOVING_PARAMS, **RM.MOVING_MOTION)
    assert out[5] == 1 and state.tobytes() == before.tobytes() and not any(o.any() for o in out[:5])


# ------------------------------------------------------------------------------------------ exact prediction
def test_constant_motion_is_predicted_exactly_and_keeps_its_id():
    rows, counts, true = RM.moving_face()
    state = R.fresh_state(1)
    out_rows, out_ids, out_misses, out_counts, det_ids, rej = RM.track_update_motion(rows, counts, [0, RM.MOVING_T], state,
                                                                                     **RM.MOVING_PARAMS, **RM.MOVING_MOTION)
    assert rej == 0 and out_counts.tolist() == [1] * 12 and out_ids[:, 0].tolist() == [1] * 12
    assert out_misses[:, 0].tolist() == [0] * 5 + [1, 2, 3] + [0] * 4
    for t in range(2, 12):                                                    # the gap included
        assert out_rows[t, 0, 1:].tolist() == true[t].tolist(), t
    assert det_ids[:, 0].tolist() == [1] * 5 + [0] * 3 + [1] * 4
    tr = state[0]["tracks"][0]
    assert int(state[0]["seq"]["next_id"]) == 1 and tr["reserved"].tolist() == [6 * 256, 2 * 256, 0]
    # the prediction is made before the match: in frame 1 the track is where frame 0 left it, and the match moves it
    assert out_rows[1, 0, 1:].tolist() == true[1].tolist() and out_rows[0, 0, 1:].tolist() == true[0].tolist()

    # the old rule on the same input: the stale box through the gap, then a second id
    s_old = R.fresh_state(1)
    o_rows, o_ids, o_misses, o_counts, o_det, _ = R.track_update(rows, counts, [0, RM.MOVING_T], s_old, **RM.MOVING_PARAMS)
    for t in RM.MOVING_MISSED:
        assert o_counts[t] == 1 and o_rows[t, 0, 1:].tolist() == true[4].tolist()
    assert o_det[8, 0] == 2 and int(s_old[0]["seq"]["next_id"]) == 2
    assert sorted(o_ids[8, :2].tolist()) == [1, 2]                            # one person, two galleries


def test_negative_whole_pixel_velocities_are_exact_too():
    rows, counts, true = RM.moving_face()
    rows[:, 0, 1] = 200 - rows[:, 0, 1]                                       # -6 px/frame in x, mirrored about 100
    rows[counts == 0] = 0
    true = true.copy()
    true[:, 0] = 200 - true[:, 0]
    state = R.fresh_state(1)
    out = RM.track_update_motion(rows, counts, [0, 12], state, **RM.MOVING_PARAMS, **RM.MOVING_MOTION)
    for t in range(2, 12):
        assert out[0][t, 0, 1:].tolist() == true[t].tolist(), t
    assert state[0]["tracks"][0]["reserved"].tolist() == [-6 * 256, 2 * 256, 0] and out[1][:, 0].tolist() == [1] * 12


# ------------------------------------------------------------------------------------------ bounds
def _one_face(boxes, K=2):
    """rows, counts of one face per frame; None = missed."""
    rows = np.zeros((len(boxes), K, 5), np.float32)
    counts = np.zeros(len(boxes), np.int32)
    for t, b in enumerate(boxes):
        if b is not None:
            rows[t, 0], counts[t] = (0.8, *b), 1
    return rows, counts


BOUND_PARAMS = dict(iou_threshold=0.05, alpha256=256, max_misses=5, min_hits=1, emit_misses=5, birth_score=0.0)


@pytest.mark.parametrize("sign", [1, -1])
def test_a_track_stops_at_the_coordinate_bound(sign):
    # 20 wide, 12 px/frame in x towards +-M, 3 px/frame in y; frames 0..2 detected, 3..4 missed
    xs = [16330, 16342, 16354]
    boxes = [((x if sign > 0 else -x - 20), 100 + 3 * t, 20, 20) for t, x in enumerate(xs)] + [None, None]
    rows, counts = _one_face(boxes)
    state = R.fresh_state(1)
    out = RM.track_update_motion(rows[:3], counts[:3], [0, 3], state, **BOUND_PARAMS, beta256=256, damp256=256, max_speed=64)
    tr = state[0]["tracks"][0]
    assert tr["reserved"].tolist() == [sign * 12 * 256, 3 * 256, 0]
    x1 = 16354 if sign > 0 else -16374
    assert (tr["x1q"], tr["x2q"]) == (16 * x1, 16 * (x1 + 20))
    out = RM.track_update_motion(rows[3:], counts[3:], [0, 2], state, **BOUND_PARAMS, beta256=256, damp256=256, max_speed=64)
    tr = state[0]["tracks"][0]
    # x: 16366 + 20 would pass M = 16384: the corners stay and the velocity is zeroed; y goes on
    assert tr["reserved"].tolist() == [0, 3 * 256, 0] and (tr["x1q"], tr["x2q"]) == (16 * x1, 16 * (x1 + 20))
    assert (tr["y1q"], tr["y2q"]) == (16 * 112, 16 * 132) and tr["misses"] == 2
    assert out[0][:, 0, 1:].tolist() == [[x1, 109, 20, 20], [x1, 112, 20, 20]]
    # exactly at the bound is allowed: 16364 + 20 = M
    boxes = [((x if sign > 0 else -x - 20), 100, 20, 20) for x in (16356, 16360)] + [None, None]
    rows, counts = _one_face(boxes)
    state = R.fresh_state(1)
    out = RM.track_update_motion(rows, counts, [0, 4], state, **BOUND_PARAMS, beta256=256, damp256=256, max_speed=64)
    want = [16364, 16364] if sign > 0 else [-M, -M]
    assert out[0][2:, 0, 1].tolist() == want and state[0]["tracks"][0]["reserved"].tolist() == [0, 0, 0]


def test_the_velocity_clamps_at_max_speed():
    boxes = [(100 + 10 * t, 300 - 10 * t, 40, 40) for t in range(4)]
    rows, counts = _one_face(boxes)
    state = R.fresh_state(1)
    RM.track_update_motion(rows, counts, [0, 4], state, **BOUND_PARAMS, beta256=256, damp256=256, max_speed=4)
    assert state[0]["tracks"][0]["reserved"].tolist() == [4 * 256, -4 * 256, 0] and int(state[0]["seq"]["next_id"]) == 1
    state = R.fresh_state(1)
    RM.track_update_motion(rows, counts, [0, 4], state, **BOUND_PARAMS, beta256=256, damp256=256, max_speed=0)
    assert state[0]["tracks"][0]["reserved"].tolist() == [0, 0, 0]
    state = R.fresh_state(1)                                                   # half gain, no clamp: 5 px/frame after one match
    RM.track_update_motion(rows[:2], counts[:2], [0, 2], state, **BOUND_PARAMS, beta256=128, damp256=256, max_speed=1024)
    assert state[0]["tracks"][0]["reserved"].tolist() == [5 * 256, -5 * 256, 0]


def test_damping_floors_negative_velocities():
    boxes = [(200 - 6 * t, 200 - 2 * t, 16, 16) for t in range(3)] + [None] * 3
    rows, counts = _one_face(boxes)
    state = R.fresh_state(1)
    kw = dict(**BOUND_PARAMS, beta256=256, damp256=100, max_speed=64)
    RM.track_update_motion(rows[:3], counts[:3], [0, 3], state, **kw)
    assert state[0]["tracks"][0]["reserved"].tolist() == [-1536, -512, 0]
    # (-1536 * 100 + 128) >> 8 = floor(-599.5) = -600, not -599; (-512 * 100 + 128) >> 8 = floor(-199.5) = -200
    want = [[-600, -200], [-234, -78], [-91, -30]]
    for t in range(3):
        RM.track_update_motion(rows[3 + t:4 + t], counts[3 + t:4 + t], [0, 1], state, **kw)
        assert state[0]["tracks"][0]["reserved"][:2].tolist() == want[t], t
    # the positions took the damped velocities of the frame before: s = (v256 + 8) >> 4
    x = 16 * 188 + ((-1536 + 8) >> 4) + ((-600 + 8) >> 4) + ((-234 + 8) >> 4)
    assert int(state[0]["tracks"][0]["x1q"]) == x and int(state[0]["tracks"][0]["x2q"]) == x + 256


def test_growth_of_a_coasting_track():
    boxes = [(50, 60, 16, 24)] + [None] * 5 + [(50, 60, 16, 24)]
    rows, counts = _one_face(boxes)
    state = R.fresh_state(1)
    out = RM.track_update_motion(rows, counts, [0, 7], state, **BOUND_PARAMS, beta256=128, damp256=256, max_speed=64, grow256=64)
    # gx = (64 * m * 16 + 256) >> 9, gy = (64 * m * 24 + 256) >> 9 for m = 1..5 = max_misses
    gx, gy = [0, 2, 4, 6, 8, 10, 0], [0, 3, 6, 9, 12, 15, 0]
    assert out[2][:, 0].tolist() == [0, 1, 2, 3, 4, 5, 0]
    for t in range(7):
        assert out[0][t, 0, 1:].tolist() == [50 - gx[t], 60 - gy[t], 16 + 2 * gx[t], 24 + 2 * gy[t]], t
    tr = state[0]["tracks"][0]                                                # matched again in frame 6: the state never grew
    assert (tr["x1q"], tr["y1q"], tr["x2q"], tr["y2q"]) == (800, 960, 1056, 1344) and out[4][6, 0] == 1
    # the cap: the largest box, grow256 = 256: g = 16384 * m, held at M; 2^16 wide, below 2^17
    rows, counts = _one_face([(-M, -M, 2 * M, 2 * M), None, None])
    out = RM.track_update_motion(rows, counts, [0, 3], R.fresh_state(1), **BOUND_PARAMS, beta256=128, damp256=256, max_speed=64,
                                 grow256=256)
    assert out[0][1:, 0, 1:].tolist() == [[-2 * M, -2 * M, 4 * M, 4 * M]] * 2
    out = RM.track_update_motion(rows, counts, [0, 3], R.fresh_state(1), **BOUND_PARAMS, beta256=128, damp256=256, max_speed=64,
                                 grow256=1)
    assert out[0][1:, 0, 1:].tolist() == [[-M - 64, -M - 64, 2 * M + 128, 2 * M + 128], [-M - 128, -M - 128, 2 * M + 256, 2 * M + 256]]


# ------------------------------------------------------------------------------------------ the C ABI and FaceTracker
def _lib():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


GOOD = dict(n_seq=2, T=4, K=3, iou=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=5, beta256=128, damp256=256,
            max_speed=64, grow256=0, offs=(0, 1, 4))
BAD = [(f"{k} = {v}", {k: v}) for k, v in (("beta256", -1), ("beta256", 257), ("damp256", -1), ("damp256", 257), ("grow256", -1),
                                           ("grow256", 257), ("max_speed", -1), ("max_speed", 1025))] + [
    ("alpha256 = 0", dict(alpha256=0)), ("emit_misses > max_misses", dict(emit_misses=6)), ("iou_threshold = 1", dict(iou=1.0)),
    ("offset does not end at T", dict(offs=(0, 2, 3))), ("n_seq < 1", dict(n_seq=0)), ("null state", dict(null=17)),
    ("null rejected", dict(null=23))]


@pytest.mark.parametrize("why,change", BAD, ids=[b[0] for b in BAD])
def test_host_validation_needs_no_gpu(why, change):
    """Every pointer is a dummy non-null address: validation must return before anything dereferences a device one."""
    L = _lib()
    a = {**GOOD, **change}
    h_off = np.asarray(a["offs"], np.int32)
    dummy = ctypes.c_void_p(4096)
    args = [dummy, dummy, dummy, h_off.ctypes.data, a["n_seq"], a["T"], a["K"], a["iou"], a["alpha256"], a["max_misses"],
            a["min_hits"], a["emit_misses"], 0.0, a["beta256"], a["damp256"], a["max_speed"], a["grow256"], dummy, dummy, dummy,
            dummy, dummy, dummy, dummy, None]
    if "null" in a:
        args[a["null"]] = None
    assert L.fdet_track_update_motion(*args) == -1, why                        # FDET_EINVAL
    assert b"fdet_track_update_motion" in L.fdet_last_error()


def test_face_tracker_arguments():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tracking
    assert callable(hotpath.track_update_motion)
    tr = tracking.FaceTracker(device="cpu")
    assert tr.motion is None
    tr = tracking.FaceTracker(device="cpu", motion="constant_velocity", beta=0.3, damping=0.9, max_speed=32, coast_grow=0.1)
    assert (tr.beta256, tr.damp256, tr.max_speed, tr.grow256) == (77, 230, 32, 26)          # rint
    tr = tracking.FaceTracker(device="cpu", motion="constant_velocity")
    assert (tr.beta256, tr.damp256, tr.max_speed, tr.grow256) == (128, 256, 64, 0)
    snap = tr.snapshot()
    assert snap.dtype == tracking.MOTION_STATE_DTYPE and snap.dtype.itemsize == R.STATE_DTYPE.itemsize
    for name in R.TRACK_DTYPE.names[:9]:
        assert tracking.MOTION_TRACK_DTYPE.fields[name][1] == R.TRACK_DTYPE.fields[name][1]
    assert tracking.MOTION_TRACK_DTYPE.fields["vx256"][1] == 36 and tracking.MOTION_TRACK_DTYPE.fields["vy256"][1] == 40
    for bad in (dict(motion="kalman"), dict(beta=1.01), dict(beta=-0.1), dict(damping=1.5), dict(coast_grow=-0.01),
                dict(coast_grow=2.0), dict(max_speed=1025), dict(max_speed=-1), dict(max_speed=1.5)):
        with pytest.raises(ValueError):
            tracking.FaceTracker(device="cpu", **{"motion": "constant_velocity", **bad})


def test_track_frames_options(tmp_path, capsys):
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import track_frames
    Image.new("RGB", (8, 6)).save(tmp_path / "f000.png")
    with pytest.raises(SystemExit) as e:
        track_frames.main(["--frames", str(tmp_path), "--out", str(tmp_path / "o.txt"), "--motion", "kalman"])
    assert e.value.code == 2 and "--motion" in capsys.readouterr().err
    seen = {}

    def run(args):
        seen.update(vars(args))
    real, track_frames.run = track_frames.run, run
    try:
        track_frames.main(["--frames", str(tmp_path), "--out", str(tmp_path / "o.txt"), "--motion", "constant_velocity",
                           "--motion-beta", "0.25", "--motion-damping", "0.9", "--max-speed", "12", "--coast-grow", "0.2"])
    finally:
        track_frames.run = real
    assert (seen["motion"], seen["motion_beta"], seen["motion_damping"], seen["max_speed"], seen["coast_grow"]) == \
        ("constant_velocity", 0.25, 0.9, 12, 0.2)
