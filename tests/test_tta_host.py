"""Host-side checks of the test-time augmentation of tiled detection: `tiling.plan_tta`, the numpy restatement
of tests/tta_cpu_ref.py against tests/tiles_cpu_ref.py and against hand-worked votes, the C-ABI surface of the two new
entries of csrc/fdet_tiles.hip, and the new options of TiledDetector and the two scripts.  No GPU."""
import os

import numpy as np
import pytest

import tiles_cpu_ref as R
import tta_cpu_ref as V

f32 = np.float32
SIZES = [(1, 1), (480, 480), (700, 1024), (3000, 4000)]                     # (h, w)


def _T():
    import fdet_amd  # noqa: F401
    from fdet_amd import tiling
    return tiling


# ---------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("tile_sizes", [(), (480,), (240, 960)])
def test_plan_tta_without_flip_is_plan_tiles_with_zero_flags(tile_sizes):
    T = _T()
    p = T.plan_tiles(SIZES, tile_sizes, 0.25, True)
    q, flags = T.plan_tta(SIZES, tile_sizes, 0.25, True, False)
    assert q.tiles.dtype == T.TILE_DTYPE and q.tiles.tobytes() == p.tiles.tobytes()
    assert q.tile_offset.dtype == np.int32 and np.array_equal(q.tile_offset, p.tile_offset)
    assert flags.dtype == np.uint8 and flags.shape == (len(p),) and not flags.any()


@pytest.mark.parametrize("tile_sizes", [(), (480,), (240, 960)])
def test_plan_tta_with_flip_repeats_every_images_windows_flagged(tile_sizes):
    T = _T()
    p = T.plan_tiles(SIZES, tile_sizes, 0.25, True)
    q, flags = T.plan_tta(SIZES, tile_sizes, 0.25, True, True)
    assert q.tiles.dtype == T.TILE_DTYPE and q.tile_offset.dtype == np.int32 and flags.dtype == np.uint8
    assert q.tiles.flags.c_contiguous and flags.flags.c_contiguous
    assert len(q) == 2 * len(p) == len(flags) and q.tile_offset.tolist() == (2 * p.tile_offset).tolist()
    for i in range(len(SIZES)):
        a, b = int(p.tile_offset[i]), int(p.tile_offset[i + 1])
        m = b - a
        mine, fl = q.tiles[2 * a:2 * b], flags[2 * a:2 * b]
        assert (mine["image"] == i).all()
        assert mine[:m].tobytes() == p.tiles[a:b].tobytes() and mine[m:].tobytes() == p.tiles[a:b].tobytes()
        assert fl[:m].tolist() == [0] * m and fl[m:].tolist() == [1] * m
    recs, offs, rf = V.plan_tta(SIZES, tile_sizes, 0.25, True, True)          # the restatement agrees
    assert [tuple(int(v) for v in t) for t in q.tiles] == recs and q.tile_offset.tolist() == offs and flags.tolist() == rf


# ------------------------------------------------------------------------------------------- reference against itself
def _random_case(seed, n_images=3, K=24):
    g = np.random.default_rng(seed)
    sizes = [(int(g.integers(300, 1200)), int(g.integers(300, 1200))) for _ in range(n_images)]
    recs, offs = R.plan(sizes, (480,), 0.25, True)
    Tn = len(recs)
    rows = np.full((Tn, K, 5), -7.0, f32)
    counts = g.integers(0, K + 1, Tn).astype(np.int32)
    counts[g.integers(0, Tn, max(1, Tn // 4))] = 0
    for t in range(Tn):
        c = int(counts[t])
        sc = np.round(g.uniform(0.01, 1.0, c) * 8) / 8                        # many equal scores
        xy = g.uniform(-5, 470, (c, 2))
        wh = g.uniform(0, 120, (c, 2))
        wh[g.uniform(size=c) < 0.15] = 0
        rows[t, :c] = np.concatenate([sc[:, None], xy, wh], 1).astype(f32)
    t = int(np.argmax(counts))
    rows[t, 0, 0] = np.nan                                                    # a NaN score is visited last
    return sizes, recs, offs, rows, counts


@pytest.mark.parametrize("seed,margin,thr", [(0, 0.0, 0.5), (1, 0.0, 0.01), (2, 12.0, 0.5), (3, 40.0, 0.3)])
def test_reference_with_everything_off_is_the_plain_merge(seed, margin, thr):
    sizes, recs, offs, rows, counts = _random_case(seed)
    a = R.merge(rows, counts, recs, offs, sizes, 480, 480, margin, thr, 4864)
    for flags in (None, np.zeros(len(recs), np.uint8)):
        b = V.merge_vote(rows, counts, recs, flags, offs, sizes, 480, 480, margin, thr, 4864, vote=0, min_votes=1)
        assert a[2] == b[3] == 0 and np.array_equal(a[1], b[2]) and a[1].sum() > 0
        assert np.array_equal(a[0], b[0], equal_nan=True)
        assert all((b[1][i, :b[2][i]] >= 1).all() and not b[1][i, b[2][i]:].any() for i in range(len(sizes)))
    # the votes of an image add up to its candidates: every candidate is owned exactly once
    v = V.merge_vote(rows, counts, recs, None, offs, sizes, 480, 480, 0.0, thr, 4864, vote=1, min_votes=1)
    for i in range(len(sizes)):
        assert int(v[1][i].sum()) == int(counts[offs[i]:offs[i + 1]].sum())
    # voting moves boxes, never scores, counts or the visiting order
    assert np.array_equal(v[2], V.merge_vote(rows, counts, recs, None, offs, sizes, 480, 480, 0.0, thr, 4864, vote=0)[2])
    w = V.merge_vote(rows, counts, recs, None, offs, sizes, 480, 480, 0.0, thr, 4864, vote=0)
    assert np.array_equal(v[0][:, :, 0], w[0][:, :, 0], equal_nan=True) and np.array_equal(v[1], w[1])


def test_reference_unmirrors_flagged_tiles():
    """A box seen in a mirrored frame at x lands where the same face seen unmirrored at Wo - x - w lands."""
    tiles = [(0, 480, 0, 480, 480), (0, 480, 0, 480, 480)]
    rows = np.zeros((2, 2, 5), f32)
    rows[0, 0] = [0.9, 100, 50, 40, 60]
    rows[1, 0] = [0.8, 480 - 100 - 40, 50, 40, 60]                           # the same box in the mirrored frame
    rows[1, 1] = [0.7, 10, 300, 30, 30]
    out, votes, cnt, rej = V.merge_vote(rows, [1, 2], tiles, [0, 1], [0, 2], [(960, 960)], 480, 480, 0.0, 0.5, 8, vote=1)
    assert rej == 0 and cnt[0] == 2 and votes[0, :2].tolist() == [2, 1]
    assert out[0, 0].tolist() == [f32(0.9), 580.0, 50.0, 40.0, 60.0]
    assert out[0, 1].tolist() == [f32(0.7), 480.0 + (480 - 10 - 30), 300.0, 30.0, 30.0]
    assert np.array_equal(V.unmirror_rows(rows, [0, 1], 480)[1, 0], np.array([0.8, 100, 50, 40, 60], f32))


# ----------------------------------------------------------------------------------------------- hand-checked votes
WHOLE = [(0, 0, 0, 480, 480)]                                                # a 480x480 image as one window: frame = source


def _one(rows, thr=0.5, vote=1, min_votes=1, Kout=16):
    rows = np.asarray(rows, f32)[None]
    return V.merge_vote(rows, [rows.shape[1]], WHOLE, [0], [0, 1], [(480, 480)], 480, 480, 0.0, thr, Kout, vote, min_votes)


def test_vote_of_three_boxes_by_hand():
    # overlaps with the first box: 360 / 440 = 0.82 and 288 / 512 = 0.56, both above 0.5
    out, votes, cnt, rej = _one([[0.9, 10, 10, 20, 20], [0.6, 12, 10, 20, 20], [0.3, 14, 12, 20, 20]])
    # q = llrint(float32(score) * 2^20): float32 0.9 = 0.899999976..., 0.6 = 0.600000023..., 0.3 = 0.300000011...
    q = [943718, 629146, 314573]
    assert q == [int(np.rint(np.float64(f32(s)) * 2 ** 20)) for s in (0.9, 0.6, 0.3)]
    Q = sum(q)
    assert Q == 1887437
    sx1 = q[0] * 10 + q[1] * 12 + q[2] * 14
    sy1 = q[0] * 10 + q[1] * 10 + q[2] * 12
    sx2 = q[0] * 30 + q[1] * 32 + q[2] * 34
    sy2 = q[0] * 30 + q[1] * 30 + q[2] * 32
    assert (sx1, sy1, sx2, sy2) == (21390954, 19503516, 59139694, 57252256)
    # 11.33, 10.33, 31.33, 30.33 -> 11, 10, 31, 30
    assert [round(s / Q) for s in (sx1, sy1, sx2, sy2)] == [11, 10, 31, 30]
    assert rej == 0 and cnt[0] == 1 and votes[0].tolist() == [3] + [0] * 15
    assert out[0, 0].tolist() == [f32(0.9), 11.0, 10.0, 20.0, 20.0] and not out[0, 1:].any()
    # without the vote the keeper's own box comes out, with the same member count
    out0, votes0, cnt0, _ = _one([[0.9, 10, 10, 20, 20], [0.6, 12, 10, 20, 20], [0.3, 14, 12, 20, 20]], vote=0)
    assert out0[0, 0].tolist() == [f32(0.9), 10.0, 10.0, 20.0, 20.0] and votes0[0, 0] == 3 and cnt0[0] == 1


def test_a_member_is_owned_by_the_first_keeper_only():
    # A over B (0.6), B over C (0.6), A not over C (0.33): A owns B, C is a keeper of its own; D overlaps A and C and is
    # suppressed by A first, so C never counts it
    A, B, C = [0.9, 0, 0, 40, 40], [0.8, 10, 0, 40, 40], [0.7, 20, 0, 40, 40]
    D = [0.6, 8, 0, 40, 40]                                                  # with A: 32/48 = 0.67; with C: 28/52 = 0.54
    out, votes, cnt, rej = _one([A, B, C, D], thr=0.5)
    assert rej == 0 and cnt[0] == 2 and votes[0, :2].tolist() == [3, 1]
    q = [int(np.rint(np.float64(f32(s)) * 2 ** 20)) for s in (0.9, 0.8, 0.6)]
    x1 = round((q[0] * 0 + q[1] * 10 + q[2] * 8) / sum(q))
    assert out[0, 0].tolist() == [f32(0.9), float(x1), 0.0, 40.0, 40.0] and x1 == 6
    assert out[0, 1].tolist() == [f32(0.7), 20.0, 0.0, 40.0, 40.0]           # C alone: its own box


def test_zero_total_weight_falls_back_to_the_keepers_own_box():
    # the scores 0, NaN and -1 weigh nothing; 0 is visited first (NaN is ordered as -inf, after -1) and owns the other two
    out, votes, cnt, rej = _one([[0.0, 10, 10, 20, 20], [np.nan, 12, 10, 20, 20], [-1.0, 11, 11, 20, 20]])
    assert rej == 0 and cnt[0] == 1 and votes[0, 0] == 3
    assert out[0, 0].tolist() == [0.0, 10.0, 10.0, 20.0, 20.0]
    # a score above 1 weighs as 1: two equal weights give the midpoint, half to even
    out, votes, cnt, rej = _one([[7.0, 10, 10, 20, 20], [1.0, 13, 11, 20, 20]])
    assert votes[0, 0] == 2 and out[0, 0].tolist() == [7.0, 12.0, 10.0, 20.0, 20.0]      # 11.5 -> 12, 10.5 -> 10; 31.5 -> 32, 30.5 -> 30
    # a member beyond 2^24 weighs nothing
    assert V.weight(f32(0.5), f32(0), f32(0), f32(2.0 ** 24), f32(1)) == 524288
    assert V.weight(f32(0.5), f32(0), f32(0), f32(2.0 ** 24 + 2), f32(1)) == 0
    assert V.weight(f32(0.5), f32(0), f32(np.inf), f32(1), f32(1)) == 0 and V.weight(f32(-np.inf), 0, 0, 1, 1) == 0


def test_min_votes_drops_singletons_that_still_suppress():
    # S (a singleton keeper, the best score) suppresses nothing; A owns B.  With min_votes = 2 only A comes out.
    S, A, B = [0.95, 300, 300, 30, 30], [0.9, 10, 10, 20, 20], [0.6, 12, 10, 20, 20]
    out, votes, cnt, rej = _one([S, A, B], min_votes=2)
    assert rej == 0 and cnt[0] == 1 and votes[0, :2].tolist() == [2, 0] and out[0, 0, 0] == f32(0.9)
    # a keeper that is dropped for having too few members has still suppressed: K1 owns M; K2 (a singleton) is dropped at
    # min_votes = 2, and with min_votes = 3 nothing is left although M was only ever suppressed, never output
    K1, M, K2 = [0.9, 0, 0, 40, 40], [0.8, 10, 0, 40, 40], [0.7, 200, 0, 40, 40]
    a = _one([K1, M, K2], min_votes=1)
    b = _one([K1, M, K2], min_votes=2)
    c = _one([K1, M, K2], min_votes=3)
    assert a[2][0] == 2 and a[1][0, :2].tolist() == [2, 1]
    assert b[2][0] == 1 and b[1][0, :2].tolist() == [2, 0] and np.array_equal(b[0][0, 0], a[0][0, 0])
    assert c[2][0] == 0 and not c[0].any() and not c[1].any()
    # dropped keepers do not count towards Kout
    assert _one([K1, M, K2], min_votes=2, Kout=1)[3] == 0 and _one([K1, M, K2], min_votes=1, Kout=1)[3] == 1


# -------------------------------------------------------------------------------------------- built library and scripts
def test_library_exports_the_two_entries_and_refuses_bad_arguments_on_the_host():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    L = _native.lib()
    for name in ("fdet_tile_gather_flags", "fdet_tile_merge_vote"):
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(L, name), f"{name} declared in include/fdet.h but not exported"
    assert L.fdet_tile_gather_flags(None, None, None, 1, None, None, None, None, 1, 480, 480, None, None) == -1
    assert b"tile_gather_flags" in L.fdet_last_error()
    assert L.fdet_tile_merge_vote(None, None, None, None, None, 1, 1, 1, 480, 480, None, 0.0, 0.5, 1, 1, 1, None, None, None, None,
                                  None) == -1
    assert b"tile_merge_vote" in L.fdet_last_error()


class _Model:
    training = False
    input_shape = (3, 480, 480)


def test_tiled_detector_options():
    T = _T()
    with pytest.raises(ValueError, match="min_votes"):
        T.TiledDetector(_Model(), min_votes=2)
    with pytest.raises(ValueError, match="min_votes"):
        T.TiledDetector(_Model(), vote=True, min_votes=0)
    d = T.TiledDetector(_Model())
    assert (d.flip, d.vote, d.min_votes, d.last_votes) == (False, False, 1, None)
    d = T.TiledDetector(_Model(), flip=True, vote=True, min_votes=2)
    assert (d.flip, d.vote, d.min_votes) == (True, True, 2)
    plan, flags = d.plan_tta([(700, 1024)])
    assert len(plan) == 2 * len(d.plan([(700, 1024)])) and int(flags.sum()) == len(plan) // 2
    assert isinstance(T.FLAGGED_GATHER_MEASURED_FASTER, bool)


def test_script_parsers_accept_the_new_options(monkeypatch):
    """`main` parses and checks, then hands the options to `run`, which is replaced here so that nothing runs."""
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images, run_validation_epoch
    for mod in (detect_images, run_validation_epoch):
        monkeypatch.setattr(mod, "run", lambda args: args)
    a = detect_images.main(["--images", "d", "--out", "f", "--flip", "--vote", "--min-votes", "2"])
    assert (a.flip, a.vote, a.min_votes) == (True, True, 2)
    a = detect_images.main(["--images", "d", "--out", "f"])
    assert (a.flip, a.vote, a.min_votes) == (False, False, 1)
    b = run_validation_epoch.main(["--tiled", "--flip", "--vote", "--min-votes", "3"])
    assert (b.tiled, b.flip, b.vote, b.min_votes) == (True, True, True, 3)
    assert run_validation_epoch.tta_label(b) == " [flip, vote, min-votes 3]"
    assert run_validation_epoch.tta_label(run_validation_epoch.main(["--tiled"])) == ""
    assert run_validation_epoch.main(["--tiled", "--flip"]).flip is True


@pytest.mark.parametrize("script,argv", [
    ("detect_images", ["--images", "d", "--out", "f", "--min-votes", "2"]),             # min-votes above 1 without --vote
    ("detect_images", ["--images", "d", "--out", "f", "--vote", "--min-votes", "0"]),
    ("run_validation_epoch", ["--tiled", "--min-votes", "2"]),
    ("run_validation_epoch", ["--tiled", "--vote", "--min-votes", "0"]),
    ("run_validation_epoch", ["--flip"]),                                                # the three apply to --tiled only
    ("run_validation_epoch", ["--vote"]),
    ("run_validation_epoch", ["--vote", "--min-votes", "2"]),
])
def test_scripts_refuse_option_combinations_before_anything_runs(script, argv, capsys, monkeypatch):
    import importlib
    import fdet_amd  # noqa: F401
    mod = importlib.import_module(f"fdet_amd.{script}")
    ran = []
    monkeypatch.setattr(mod, "run", ran.append)
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert e.value.code == 2 and not ran
    err = capsys.readouterr().err
    assert "--min-votes" in err or "--tiled" in err
