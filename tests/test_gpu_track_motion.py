"""fdet_track_update_motion / FaceTracker(motion="constant_velocity") on the GPU against the restatement on
Python ints (tests/track_motion_cpu_ref.py).  No tolerance anywhere: every comparison is equality of all five outputs and of
the state bytes."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cpu_ref as RR  # noqa: E402
import track_cpu_ref as R  # noqa: E402
import track_motion_cpu_ref as RM  # noqa: E402

pytestmark = pytest.mark.gpu

M = R.MAX_COORD
NAMES = ("out_rows", "out_ids", "out_misses", "out_counts", "det_ids")


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tracking
    return hotpath, tracking


def _device(rows, counts, seq_offset, state, iou_threshold=0.3, alpha256=128, max_misses=5, min_hits=2, emit_misses=None,
            birth_score=0.0, beta256=128, damp256=256, max_speed=64, grow256=0, motion=True):
    """fdet_track_update_motion (motion=False: fdet_track_update) on host arrays with the restatement's signature: `state`
    ((n_seq,) records) is modified in place."""
    hp, _ = _mods()
    h_off = np.ascontiguousarray(np.asarray(seq_offset, np.int32))
    d_state = torch.from_numpy(state.view(np.uint8).copy()).cuda()
    args = (torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda(), torch.from_numpy(h_off).cuda(), h_off, d_state,
            iou_threshold, alpha256, max_misses, min_hits, max_misses if emit_misses is None else emit_misses, birth_score)
    out = hp.track_update_motion(*args, beta256, damp256, max_speed, grow256) if motion else hp.track_update(*args)
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
    want = RM.track_update_motion(rows, counts, seq_offset, s_ref, **kw)
    _same(got, want)
    assert s_dev.tobytes() == s_ref.tobytes(), "state differs"
    return got, s_dev


def _result(res):
    return tuple(t.cpu().numpy() for t in (res.rows, res.ids, res.misses, res.counts, res.det_ids)) + (0,)


# ------------------------------------------------------------------------------------------ random sequences
@functools.lru_cache(maxsize=None)
def _three_sequences():
    """T = 48 frames of K = 16 rows in sequences of 1, 7 and 40 frames: 8 moving faces, dropouts, false positives."""
    parts = [R.synthetic_sequence(1, 16, 30, faces=8), R.synthetic_sequence(7, 16, 31, faces=8, negative=True),
             R.synthetic_sequence(40, 16, 32, faces=8, negative=True)]
    rows, counts = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return rows, counts, np.array([0, 1, 8, 48], np.int32)


@pytest.mark.parametrize("alpha256,beta256,damp256,grow256", [(128, 128, 256, 0), (256, 256, 230, 64), (64, 40, 200, 256),
                                                              (192, 256, 0, 13)])
def test_random_sequences(alpha256, beta256, damp256, grow256):
    _, tracking = _mods()
    rows, counts, off = _three_sequences()
    got, state = _both(rows, counts, off, 3, alpha256=alpha256, beta256=beta256, damp256=damp256, grow256=grow256, max_speed=8)
    v = state["tracks"]["reserved"]
    assert got[3].sum() > 100 and got[2].max() >= 1 and (v[..., 0] > 0).any() and (v[..., 1] < 0).any() and not v[..., 2].any()
    assert np.abs(v).max() <= 8 * 256
    # the same through FaceTracker, whose snapshot() carries the velocities
    tr = tracking.FaceTracker(n_seq=3, alpha=alpha256 / 256, motion="constant_velocity", beta=beta256 / 256, damping=damp256 / 256,
                              max_speed=8, coast_grow=grow256 / 256)
    res = tr.update(torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(counts.copy()).cuda(), off)
    _same(_result(res), got)
    snap = tr.snapshot()
    assert snap.dtype == tracking.MOTION_STATE_DTYPE and snap.tobytes() == state.tobytes()
    assert np.array_equal(snap["tracks"]["vx256"], v[..., 0]) and np.array_equal(snap["tracks"]["vy256"], v[..., 1])


def test_chunk_invariance_on_the_device():
    _, tracking = _mods()
    rows, counts = R.synthetic_sequence(40, 16, 33, faces=8, negative=True)
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    kw = dict(motion="constant_velocity", beta=0.75, damping=0.9, max_speed=16, coast_grow=0.125)
    one = tracking.FaceTracker(**kw)
    whole = one.update(d_rows, d_counts)
    for chunk in (1, 5):
        parts = tracking.FaceTracker(**kw)
        res = [parts.update(d_rows[a:a + chunk], d_counts[a:a + chunk]) for a in range(0, 40, chunk)]
        for f in tracking.TrackResult._fields:
            assert torch.equal(torch.cat([getattr(r, f) for r in res]), getattr(whole, f)), (chunk, f)
        assert torch.equal(parts.state, one.state), chunk
    s_ref = R.fresh_state(1)
    want = RM.track_update_motion(rows, counts, [0, 40], s_ref, beta256=192, damp256=230, max_speed=16, grow256=32)
    _same(_result(whole), want)
    assert one.snapshot().tobytes() == s_ref.tobytes() and s_ref["tracks"]["reserved"].any()


def test_neutral_parameters_are_the_old_entry_byte_for_byte():
    rows, counts, off = _three_sequences()
    for alpha256, damp256, max_speed in ((128, 256, 64), (256, 100, 0)):
        s_old, s_new = R.fresh_state(3), R.fresh_state(3)
        old = _device(rows, counts, off, s_old, alpha256=alpha256, motion=False)
        new = _device(rows, counts, off, s_new, alpha256=alpha256, beta256=0, damp256=damp256, max_speed=max_speed, grow256=0)
        _same(new, old)
        assert s_new.tobytes() == s_old.tobytes() and old[3].sum() > 100


# ------------------------------------------------------------------------------------------ edges
def test_128_tracks_256_detections_with_velocities():
    """Frame 0 fills the 128 slots, frame 1 moves every box (each by its own few pixels: every velocity is non-zero), frame 2
    has 256 detections: both waves of slots and all four of detections, neighbours overlapping."""
    g = np.random.default_rng(7)
    i = np.arange(256)
    grid = np.stack([np.full(256, 0.6), 40.0 * (i % 16) - 100, 40.0 * (i // 16) - 100, np.full(256, 50.0), np.full(256, 50.0)], 1)
    step = g.integers(1, 7, (128, 2)) * g.choice([-1, 1], (128, 2))
    rows = np.zeros((3, 256, 5), np.float32)
    rows[0, :128] = grid[:128]
    rows[1, :128] = grid[:128]
    rows[1, :128, 1:3] += step
    f2 = grid.copy()
    f2[:128, 1:3] += 2 * step
    f2[:, 1:] += g.integers(-4, 5, (256, 4))
    f2[:, 0] += g.uniform(0, 0.3, 256)
    rows[1, :128] = rows[1, g.permutation(128)]
    rows[2] = f2[g.permutation(256)]
    counts = np.array([128, 128, 256], np.int32)
    kw = dict(iou_threshold=0.05, alpha256=192, min_hits=1, beta256=200, damp256=240, max_speed=64, grow256=32)
    _, mid = _both(rows[:2], counts[:2], [0, 2], 1, **kw)
    v = mid[0]["tracks"]["reserved"]
    assert (mid[0]["tracks"]["id"] != 0).all() and (v[:, :2] != 0).all()
    got, state = _both(rows[2:], counts[2:], [0, 1], 1, state=mid, **kw)
    assert int(got[3][0]) == 128 and int(state[0]["seq"]["dropped"]) > 0 and int((got[4][0] != 0).sum()) >= 128
    _both(rows, counts, [0, 3], 1, **kw)                                       # and in one launch


def _one_face(boxes, K=2):
    rows = np.zeros((len(boxes), K, 5), np.float32)
    counts = np.zeros(len(boxes), np.int32)
    for t, b in enumerate(boxes):
        if b is not None:
            rows[t, 0], counts[t] = (0.8, *b), 1
    return rows, counts


BOUND = dict(iou_threshold=0.05, alpha256=256, max_misses=5, min_hits=1, emit_misses=5, beta256=256, damp256=256, max_speed=64)


def test_bounds_and_clamps():
    """The cases of tests/test_track_motion_host.py, as four sequences of one launch each."""
    seqs, want_v = [], []
    for sign in (1, -1):                                                       # stops at +-M with the x velocity zeroed
        xs = [16330, 16342, 16354]
        seqs.append([((x if sign > 0 else -x - 20), 100 + 3 * t, 20, 20) for t, x in enumerate(xs)] + [None, None])
        want_v.append([0, 3 * 256])
    seqs.append([(100 + 10 * t, 300 - 10 * t, 40, 40) for t in range(5)])      # 10 px/frame against max_speed = 4
    seqs.append([(200 - 6 * t, 200 - 2 * t, 16, 16) for t in range(3)] + [None, None])
    parts = [_one_face(b) for b in seqs]
    rows, counts = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    off = np.arange(5) * 5
    got, state = _both(rows, counts, off, 4, **BOUND)
    for s in range(2):
        tr = state[s]["tracks"][0]
        x1 = 16354 if s == 0 else -16374
        assert tr["reserved"][:2].tolist() == want_v[s] and (tr["x1q"], tr["x2q"]) == (16 * x1, 16 * (x1 + 20))
        assert got[0][5 * s + 3:5 * s + 5, 0, 1:].tolist() == [[x1, 109, 20, 20], [x1, 112, 20, 20]]
    got, state = _both(rows, counts, off, 4, **{**BOUND, "max_speed": 4})
    assert state[2]["tracks"][0]["reserved"][:2].tolist() == [1024, -1024]
    got, state = _both(rows, counts, off, 4, **{**BOUND, "damp256": 100})
    assert state[3]["tracks"][0]["reserved"][:2].tolist() == [-234, -78]       # -1536 -> -600 -> -234: the shift floors


def test_growth_up_to_max_misses_and_its_cap():
    a = _one_face([(50, 60, 16, 24)] + [None] * 5 + [(50, 60, 16, 24)])
    b = _one_face([(-M, -M, 2 * M, 2 * M)] + [None] * 6)                       # dies in its last frame
    rows, counts = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    got, _ = _both(rows, counts, [0, 7, 14], 2, **{**BOUND, "grow256": 64})
    assert got[0][1:6, 0, 1:].tolist() == [[50 - 2 * m, 60 - 3 * m, 16 + 4 * m, 24 + 6 * m] for m in range(1, 6)]
    assert got[0][6, 0, 1:].tolist() == [50, 60, 16, 24]
    got, _ = _both(rows, counts, [0, 7, 14], 2, **{**BOUND, "grow256": 256})
    assert got[0][8:13, 0, 1:].tolist() == [[-2 * M, -2 * M, 4 * M, 4 * M]] * 5 and got[3][13] == 0
    # misses far beyond any box: the product is taken in 64 bits
    got, _ = _both(rows[7:9].repeat([1, 300], 0), counts[7:9].repeat([1, 300]), [0, 301], 1,
                   **{**BOUND, "grow256": 255, "max_misses": 1 << 30, "emit_misses": 1 << 30})
    assert got[0][300, 0, 1:].tolist() == [-2 * M, -2 * M, 4 * M, 4 * M] and got[2][300, 0] == 300


@pytest.mark.parametrize("case", ["count_above_K", "count_negative"])
def test_rejection_leaves_the_velocities_as_they_were(case):
    _, tracking = _mods()
    from fdet_amd import FdetError
    parts = [R.synthetic_sequence(n, 16, 40 + i, faces=8) for i, n in enumerate((5, 6, 7))]
    rows, counts = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    off = np.array([0, 5, 11, 18], np.int32)
    kw = dict(min_hits=1, beta256=256, damp256=200, grow256=16)
    _, before = _both(rows, counts, off, 3, **kw)
    assert before["tracks"]["reserved"][:, :, :2].any(axis=(1, 2)).all()       # velocities live in every sequence
    counts = counts.copy()
    counts[8] = 17 if case == "count_above_K" else -1                          # the fourth frame of sequence 1
    got, after = _both(rows, counts, off, 3, state=before, **kw)
    assert got[5] == 1 and after[1].tobytes() == before[1].tobytes()
    assert after[0].tobytes() != before[0].tobytes() and after[2].tobytes() != before[2].tobytes()
    for o in got[:5]:
        assert not o[5:11].any()
    tr = tracking.FaceTracker(n_seq=3, min_hits=1, motion="constant_velocity", beta=1.0, damping=200 / 256, coast_grow=16 / 256)
    tr.state.copy_(torch.from_numpy(before.view(np.uint8).copy()))
    with pytest.raises(FdetError, match="fdet_track_update_motion"):
        tr.update(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), off)
    assert tr.snapshot().tobytes() == after.tobytes()


def test_empty_sequence():
    rows, counts, _ = _three_sequences()
    _, before = _both(rows[8:20], counts[8:20], [0, 12], 1, min_hits=1)
    got, after = _both(np.zeros((0, 16, 5), np.float32), np.zeros(0, np.int32), [0, 0], 1, state=before, min_hits=1)
    assert after.tobytes() == before.tobytes() and got[0].shape == (0, 128, 5) and got[5] == 0
    # a sequence without frames beside one with frames
    got, after = _both(rows[20:24], counts[20:24], [0, 0, 4], 2, state=np.concatenate([before, before]), min_hits=1)
    assert after[0].tobytes() == before.tobytes() and after[1].tobytes() != before.tobytes()


@pytest.mark.parametrize("bad", [dict(beta256=-1), dict(beta256=257), dict(damp256=-1), dict(damp256=257), dict(grow256=-1),
                                 dict(grow256=257), dict(max_speed=-1), dict(max_speed=1025)], ids=lambda b: str(b))
def test_argument_validation_launches_nothing(bad):
    hp, _ = _mods()
    from fdet_amd import FdetError
    rows, counts, off = _three_sequences()
    _, before = _both(rows, counts, off, 3, min_hits=1)
    d_state = torch.from_numpy(before.view(np.uint8).copy()).cuda()
    rej = torch.zeros(1, dtype=torch.int64, device=d_state.device)
    par = {**dict(beta256=128, damp256=256, max_speed=64, grow256=0), **bad}
    with pytest.raises(FdetError, match="fdet_track_update_motion"):
        hp.track_update_motion(torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(counts.copy()).cuda(),
                               torch.from_numpy(off).cuda(), off, d_state, 0.3, 128, 5, 1, 5, 0.0, rejected=rej, **par)
    assert d_state.cpu().numpy().tobytes() == before.tobytes() and int(rej.item()) == 0


# ------------------------------------------------------------------------------------------ end to end
def test_a_moving_face_stays_covered_through_the_gap():
    """The 12-frame sequence of the host test on 64 x 96 images: with the motion model the pixelated frames are those of the
    true boxes, the gap included; without it frames 5..7 cover the place the face has left."""
    _, tracking = _mods()
    from fdet_amd.datasets import augment as A
    from fdet_amd.render import render_detections
    g = np.random.default_rng(9)
    images = [g.integers(0, 256, (64, 96, 3)).astype(np.uint8) for _ in range(RM.MOVING_T)]
    rows, counts, true = RM.moving_face()
    true_rows = np.zeros((RM.MOVING_T, 1, 5), np.float32)
    true_rows[:, 0, 0], true_rows[:, 0, 1:] = 0.9, true
    expect = RR.render(images, true_rows, np.ones(RM.MOVING_T, np.int32), True, True, 8)
    d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    kw = dict(alpha=1.0, max_misses=5, min_hits=1)
    tr = tracking.FaceTracker(motion="constant_velocity", beta=1.0, **kw)
    res = tr.update(d_rows, d_counts)
    want = RM.track_update_motion(rows, counts, [0, RM.MOVING_T], R.fresh_state(1), **RM.MOVING_PARAMS, **RM.MOVING_MOTION)
    _same(_result(res), want)
    assert res.ids[:, 0].tolist() == [1] * 12 and res.counts.tolist() == [1] * 12
    assert res.misses[:, 0].tolist() == [0] * 5 + [1, 2, 3] + [0] * 4
    assert np.array_equal(res.rows[:, 0, 1:].cpu().numpy(), true.astype(np.float32))
    bank = A.DeviceImageBank.from_arrays(images, "cuda")
    covered = render_detections(bank, res.rows, res.counts, anonymize="pixelate").to_arrays()
    for t in range(RM.MOVING_T):
        assert np.array_equal(covered[t], expect[t]), t
        assert not np.array_equal(covered[t], images[t])
    old = tracking.FaceTracker(**kw)                                           # motion=None
    res_old = old.update(d_rows, d_counts)
    stale = render_detections(bank, res_old.rows, res_old.counts, anonymize="pixelate").to_arrays()
    for t in range(8):                                                         # what the feature buys: frames 5..7
        assert np.array_equal(stale[t], expect[t]) == (t not in RM.MOVING_MISSED), t
    assert int(old.snapshot()["seq"]["next_id"][0]) == 2 and int(tr.snapshot()["seq"]["next_id"][0]) == 1
