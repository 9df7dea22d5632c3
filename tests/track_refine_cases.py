"""The inputs the host and the GPU tests of fdet_track_refine share: hand-made sequences run through the numpy restatements
of the online trackers (tests/track_cpu_ref.py, tests/track_motion_cpu_ref.py), and the random sequences with their truth.
Every case is (inputs for track_refine as a dict of arrays, the refine parameters)."""
import functools

import numpy as np

import track_cpu_ref as R
import track_motion_cpu_ref as RM

ARGS = ("det_rows", "det_ids", "trk_rows", "trk_ids", "trk_misses", "trk_counts", "seq_offset")
TRACKER = dict(iou_threshold=0.3, alpha256=256, max_misses=5, min_hits=1, emit_misses=None, birth_score=0.0)
OFF = dict(lookback=0, grow256=0, stitch_gap=-1, stitch_iou=0.1, min_length=1)           # a refine pass that adds nothing


def online(rows, counts, seq_offset, state=None, motion=None, **kw):
    """The online tracker's restatement on (rows, counts) -> the inputs of track_refine."""
    seq_offset = np.asarray(seq_offset, np.int32)
    state = R.fresh_state(len(seq_offset) - 1) if state is None else state
    par = {**TRACKER, **kw}
    out = R.track_update(rows, counts, seq_offset, state, **par) if motion is None else \
        RM.track_update_motion(rows, counts, seq_offset, state, **par, **motion)
    assert out[5] == 0
    return dict(det_rows=np.asarray(rows, np.float32), det_ids=out[4], trk_rows=out[0], trk_ids=out[1], trk_misses=out[2],
                trk_counts=out[3], seq_offset=seq_offset)


def frames(T, faces, K=4, score=0.8):
    """faces: one {frame: (x, y, w, h)} per face -> (rows (T,K,5), counts (T,)); face k is row k's successor in each frame."""
    rows = np.zeros((T, K, 5), np.float32)
    counts = np.zeros(T, np.int32)
    for face in faces:
        for t, box in face.items():
            rows[t, counts[t]] = (score, *box)
            counts[t] += 1
    return rows, counts


def still(box, ts):
    return {t: box for t in ts}


# ------------------------------------------------------------------------------------------ hand-made
def linear_motion():
    """+3 px per frame, 2 px wider per frame, missed in frames 4..6, never coasted."""
    true = [(10 + 3 * t, 20, 20 + 2 * t, 30) for t in range(10)]
    rows, counts = frames(10, [{t: true[t] for t in range(10) if t not in (4, 5, 6)}])
    return online(rows, counts, [0, 10], iou_threshold=0.05, emit_misses=0), np.asarray(true)


def half_steps():
    """A gap of 2 with corner differences of +3 (x) and -3 (y)."""
    rows, counts = frames(3, [{0: (10, 50, 20, 20), 2: (13, 47, 20, 20)}])
    return online(rows, counts, [0, 3], emit_misses=0)


def late_face(first=6, T=10, box=(100, 80, 16, 24)):
    rows, counts = frames(T, [still(box, range(first, T))])
    return online(rows, counts, [0, T])


def two_sequences():
    """Sequence 0: 4 frames with a face throughout; sequence 1: 5 frames, its face is first seen in its frame 1."""
    rows, counts = frames(9, [still((30, 30, 20, 20), range(0, 4)), still((100, 80, 16, 24), range(5, 9))])
    return online(rows, counts, [0, 4, 9])


def unconfirmed():
    """min_hits = 3: the first two detections of the track are not emitted."""
    rows, counts = frames(6, [{t: (40.25 + t, 30.5, 20, 20.75) for t in range(6)}])
    return online(rows, counts, [0, 6], min_hits=3)


def reappears(gap=4, second=(52, 40, 30, 20)):
    """max_misses = 1: a face at frames 0..2 is lost and comes back `gap` frames later under a new id."""
    rows, counts = frames(6 + gap, [still((50, 40, 30, 20), range(3)), still(second, range(3 + gap, 6 + gap))])
    return online(rows, counts, [0, 6 + gap], max_misses=1)


def later_anchor():
    """Track 2 appears beside the living track 1, overlapping it by less than the tracker asks for: 1 has later anchors."""
    rows, counts = frames(8, [still((50, 40, 30, 20), range(8)), still((70, 40, 30, 20), range(4, 8))])
    return online(rows, counts, [0, 8], max_misses=1)


def equal_candidates():
    """Two lost tracks overlap the newcomer alike."""
    rows, counts = frames(8, [still((0, 40, 30, 20), range(2)), still((40, 40, 30, 20), range(2)), still((20, 40, 30, 20), range(5, 8))])
    return online(rows, counts, [0, 8], max_misses=1)


def three_fragments(false_positive=False, fragments=3):
    """Frames 0..1, 5..6, 10..11 of one face under max_misses = 1: three ids; optionally a one-frame false positive at 2."""
    faces = [still((50, 40, 30, 20), (0, 1)), still((52, 41, 30, 20), (5, 6)), still((54, 42, 30, 20), (10, 11))][:fragments]
    if false_positive:
        faces.append(still((200, 10, 12, 12), (2,)))
    rows, counts = frames(12, faces)
    return online(rows, counts, [0, 12], max_misses=1)


def room():
    """Three generations of 128 disjoint faces in three frames, max_misses = 0."""
    i = np.arange(128)
    rows = np.zeros((3, 128, 5), np.float32)
    for g in range(3):
        rows[g] = np.stack([np.full(128, 0.5 + 0.1 * g), 40.0 * (i % 16) + 12 * g, 40.0 * (i // 16), np.full(128, 10.0),
                            np.full(128, 10.0)], 1)
    return online(rows, np.full(3, 128, np.int32), [0, 3], max_misses=0)


def carried_over():
    """A track from an earlier call that is never detected in this one: coasted rows without an anchor."""
    rows, counts = frames(5, [still((50, 40, 30, 20), (0, 1))])
    state = R.fresh_state(1)
    online(rows[:2], counts[:2], [0, 2], state=state)
    return online(rows[2:], counts[2:], [0, 3], state=state)


def empties():
    """Sequence 0 owns no frame, 1 has frames without rows around a face, 2 is good, 3 will be broken by the caller."""
    rows, counts = frames(12, [still((50, 40, 30, 20), (1, 2)), still((20, 20, 16, 16), range(4, 8)), still((90, 20, 16, 16), range(8, 12))])
    return online(rows, counts, [0, 0, 4, 8, 12])


# ------------------------------------------------------------------------------------------ random
SIZE = (640, 480)
SEEDS = ((1, 30, False), (7, 31, True), (40, 32, True), (200, 35, False))       # frames, seed, negative
LONG_DROPOUT = 0.4
PARAMS = (dict(lookback=5, grow256=0, stitch_gap=10, stitch_iou=0.1, min_length=1),
          dict(lookback=0, grow256=64, stitch_gap=-1, stitch_iou=0.3, min_length=3),
          dict(lookback=1024, grow256=256, stitch_gap=65535, stitch_iou=0.0, min_length=2),
          dict(lookback=2, grow256=13, stitch_gap=3, stitch_iou=0.5, min_length=5))
TRACKERS = {"plain": (None, dict(alpha256=128, max_misses=3, min_hits=2, emit_misses=2)),
            "motion": (dict(beta256=128, damp256=256, max_speed=64, grow256=32), dict(alpha256=192, max_misses=4, min_hits=2))}


def truth(T, seed, faces=8, negative=False):
    """The boxes R.synthetic_sequence moves about, (T, faces, 4) [x, y, w, h] before the detector's noise: its first three
    draws and its straight-line motion."""
    g = np.random.default_rng(seed)
    W, H = SIZE
    pos = np.stack([g.uniform(0.1 * W, 0.8 * W, faces), g.uniform(0.1 * H, 0.8 * H, faces)], 1)
    vel = g.uniform(-4, 4, (faces, 2))
    wh = g.uniform(24, 90, (faces, 2))
    pos[0], pos[1] = (0.2 * W, 0.5 * H), (0.2 * W + 6.0 * min(T, 30), 0.5 * H + 3)
    vel[0], vel[1] = (6.0, 0.0), (-6.0, 0.0)
    wh[0] = wh[1] = (60, 60)
    shift = np.array([0.3 * W, 0.3 * H]) if negative else np.zeros(2)
    t = np.arange(T)[:, None, None]
    return np.concatenate([pos[None] - shift + vel[None] * t, np.broadcast_to(wh, (T, faces, 2))], 2)


@functools.lru_cache(maxsize=None)
def random_detections():
    """248 frames of K = 16 rows in sequences of 1, 7, 40 and 200 frames."""
    parts = [R.synthetic_sequence(T, 16, seed, faces=8, negative=neg, dropout=LONG_DROPOUT if T == 200 else 0.2)
             for T, seed, neg in SEEDS]
    off = np.concatenate([[0], np.cumsum([T for T, _, _ in SEEDS])]).astype(np.int32)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), off


@functools.lru_cache(maxsize=None)
def random_inputs(tracker):
    rows, counts, off = random_detections()
    motion, par = TRACKERS[tracker]
    return online(rows, counts, off, motion=motion, **par)


def sub_sequence(inp, s):
    """Sequence s of the inputs as inputs of its own."""
    a, b = int(inp["seq_offset"][s]), int(inp["seq_offset"][s + 1])
    return {**{k: inp[k][a:b] for k in ARGS[:-1]}, "seq_offset": np.array([0, b - a], np.int32)}
