"""Host-side checks of the face-chip feature that need no GPU: properties of the numpy restatement
(tests/chips_cpu_ref.py) that tie its rule to things known independently, the argument validation of fdet_chip_extract /
fdet_chip_best_update through the loaded library (bad arguments are refused before anything is enqueued), and the Python
layer's own argument errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chips_cpu_ref as R  # noqa: E402

EINVAL = -1
IMAGE_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])          # fdet_aug_image


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------ the restatement
def test_equal_window_and_chip_is_a_byte_copy():
    img = _noise(40, 50, 0)
    for C, wx0, wy0 in ((8, 3, 5), (16, 0, 0), (21, 29, 19)):
        assert np.array_equal(R.cut(img, wx0, wy0, C, C), img[wy0:wy0 + C, wx0:wx0 + C])
    # across the edge: replication
    got = R.cut(img, -2, 36, 8, 8)
    yy, xx = np.clip(36 + np.arange(8), 0, 39), np.clip(-2 + np.arange(8), 0, 49)
    assert np.array_equal(got, img[yy][:, xx])


@pytest.mark.parametrize("S,C", [(5, 8), (3, 8), (7, 16)])
def test_upscale_stays_within_one_level_of_pil_bilinear(S, C):
    from PIL import Image
    img = _noise(24, 24, S * 100 + C)
    wx0, wy0 = 4, 9
    want = np.asarray(Image.fromarray(img[wy0:wy0 + S, wx0:wx0 + S]).resize((C, C), Image.BILINEAR)).astype(np.int64)
    got = R.cut(img, wx0, wy0, S, C).astype(np.int64)
    worst = int(np.abs(got - want).max())
    print(f"S={S} C={C}: largest difference from PIL BILINEAR {worst}")
    assert worst <= 1


@pytest.mark.parametrize("C", [8, 13])
def test_halving_is_the_two_by_two_integer_mean(C):
    img = _noise(2 * C + 6, 2 * C + 4, C).astype(np.int64)
    wx0, wy0, S = 3, 2, 2 * C
    w = img[wy0:wy0 + S, wx0:wx0 + S]
    want = (w[0::2, 0::2] + w[0::2, 1::2] + w[1::2, 0::2] + w[1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.cut(img.astype(np.uint8), wx0, wy0, S, C), want.astype(np.uint8))


def test_tap_weights_sum_to_d():
    for C in (8, 9, 16, 112, 256):
        for S in sorted({1, 2, 3, 5, 7, C - 1, C, C + 1, 2 * C - 1, 2 * C, 3 * C + 1, 20, 23, 33, 1000, 8192}):
            Wm, D = R.axis_weights(S, C)
            assert D == (S if S >= C else 2 * C)
            assert (Wm >= 0).all() and (Wm.sum(1) == D).all(), (S, C)
            assert D * D * 255 < 2 ** 35
            for u in {0, 1, C // 2, C - 1}:                  # the vectorised matrix is the tap list
                row = np.zeros(S, np.int64)
                for i, w in R.axis_taps(u, S, C)[0]:
                    assert 0 <= i < S and w >= 0
                    row[i] += w
                assert np.array_equal(row, Wm[u]), (S, C, u)


def test_folded_gather_equals_the_explicit_window():
    """image_weights folds rule 4's clamp into the matrix; the explicit S x S window gives the same chip."""
    img = _noise(40, 50, 7)
    for (wx0, wy0, S, C) in ((-7, -3, 23, 8), (30, 25, 33, 16), (10, 10, 5, 16), (-40, -40, 120, 9)):
        yy, xx = np.clip(wy0 + np.arange(S), 0, 39), np.clip(wx0 + np.arange(S), 0, 49)
        win = img[yy][:, xx].astype(np.int64)
        Wm, D = R.axis_weights(S, C)
        want = np.stack([(Wm @ win[:, :, c] @ Wm.T + D * D // 2) // (D * D) for c in range(3)], -1)
        assert np.array_equal(R.cut(img, wx0, wy0, S, C), want.astype(np.uint8))


def test_window_rule():
    assert R.window([1, 10, 20, 8, 8], 50, 40, 0) == (10, 20, 8)
    assert R.window([1, 10, 20, 8, 4], 50, 40, 0) == (10, 18, 8)             # square on the longer side, centred
    assert R.window([1, 10, 20, 7, 8], 50, 40, 0) == (9, 20, 8)              # odd X1 + X2 - S: floor
    assert R.window([1, 10, 20, 8, 8], 50, 40, 64) == (8, 18, 12)            # m = (8 * 64 + 128) >> 8 = 2
    assert R.window([1, 10, 20, 8, 8], 50, 40, 256) == (2, 12, 24)
    assert R.window([1, 0.5, 1.5, 2, 2], 50, 40, 0) == (0, 2, 2)             # half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    nan, inf = float("nan"), float("inf")
    for bad in ([nan, 1, 1, 4, 4], [1, inf, 1, 4, 4], [1, 1, 1, 0.4, 4], [1, 16390, 1, 4, 4], [1, 50, 1, 4, 4], [1, -4, 1, 4, 4],
                [1, 1, 40, 4, 4], [1, 1, -9, 4, 4], [1, 0, 0, 8193, 10], [1, 0, 0, 3000, 3000]):
        assert R.window(bad, 50, 40, 256 if bad[3] == 3000 else 0) is None, bad
    assert R.window([1, 0, 0, 8192, 10], 50, 40, 0) == (0, -4091, 8192)


def test_sharpness_of_a_checkerboard_is_the_stated_maximum():
    C = 256
    board = (((np.arange(C)[:, None] + np.arange(C)[None, :]) & 1) * 255).astype(np.uint8)
    chip = np.repeat(board[:, :, None], 3, 2)
    assert R.sharpness(chip) == 254 ** 2 * 1020 ** 2 == 67122446400 and R.sharpness(chip) > 2 ** 32
    assert R.sharpness(np.full((8, 8, 3), 77, np.uint8)) == 0


def test_best_update_restatement_is_chunk_independent():
    g = np.random.default_rng(3)
    T, K, C, G = 12, 3, 8, 4
    M = T * K
    chips = g.integers(0, 256, (M, C, C, 3), dtype=np.uint8)
    info = np.zeros(M, R.INFO_DTYPE)
    info["image"], info["row"] = np.repeat(np.arange(T), K), np.tile(np.arange(K), T)
    info["S"], info["inside256"], info["flags"] = 20, 256, 1
    info["sharp"] = g.integers(0, 4, M)                       # many ties
    ids = g.integers(0, G + 2, (T, K)).astype(np.int32)
    whole = R.fresh_gallery(1, G, C)
    over = R.best_update(chips, info, ids, [0, T], [0], *whole)
    parts = R.fresh_gallery(1, G, C)
    over2, base = 0, 0
    for a, b in ((0, 1), (1, 6), (6, 12)):
        sub = info[a * K:b * K].copy()
        sub["image"] -= a
        over2 += R.best_update(chips[a * K:b * K], sub, ids[a:b], [0, b - a], [base], *parts)
        base += b - a
    assert over == over2 == int((ids > G).sum())
    assert whole[0].tobytes() == parts[0].tobytes() and np.array_equal(whole[1], parts[1])
    assert int(whole[0]["seen"].sum()) == int(((ids >= 1) & (ids <= G)).sum())


# ------------------------------------------------------------------------------------------ the library's validation
def _lib():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


FAKE = 0x1000                                                # stands for a device pointer: nothing is launched, nothing reads it


def _extract_args(**kw):
    """A valid call on two images with counts (2, 1), K = 2; `kw` replaces arguments by name."""
    table = np.zeros(2, IMAGE_DTYPE)
    table["offset"], table["h"], table["w"] = (0, 6000), 40, 50
    counts = np.array([2, 1], np.int32)
    off = np.array([0, 2, 3], np.int32)
    a = dict(bank=FAKE, table=FAKE, h_table=table, n_images=2, rows=FAKE, counts=FAKE, h_counts=counts, chip_offset=FAKE,
             h_chip_offset=off, K=2, C=16, margin256=64, planar=0, chips=FAKE, info=FAKE, stream=None)
    a.update(kw)
    return a


def _call_extract(L, a):
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]            # alive during the call
    p = {k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    rc = L.fdet_chip_extract(p["bank"], p["table"], p["h_table"], p["n_images"], p["rows"], p["counts"], p["h_counts"],
                             p["chip_offset"], p["h_chip_offset"], p["K"], p["C"], p["margin256"], p["planar"], p["chips"],
                             p["info"], p["stream"])
    del keep
    return rc


def _bad_table(h, w):
    t = _extract_args()["h_table"]
    t["h"][1], t["w"][1] = h, w
    return t


EXTRACT_BAD = {
    "C below 8": dict(C=7), "C above 256": dict(C=257), "margin256 below 0": dict(margin256=-1), "margin256 above 256": dict(margin256=257),
    "planar 2": dict(planar=2), "planar -1": dict(planar=-1), "K negative": dict(K=-1), "no image": dict(n_images=0),
    "count below 0": dict(h_counts=np.array([2, -1], np.int32), h_chip_offset=np.array([0, 2, 1], np.int32)),
    "count above K": dict(h_counts=np.array([3, 0], np.int32), h_chip_offset=np.array([0, 3, 3], np.int32)),
    "offset not the prefix sum": dict(h_chip_offset=np.array([0, 1, 3], np.int32)),
    "offset not from 0": dict(h_chip_offset=np.array([1, 3, 4], np.int32)),
    "offset total off": dict(h_chip_offset=np.array([0, 2, 4], np.int32)),
    "too many chips": dict(K=1 << 20, h_counts=np.array([1 << 20, 1], np.int32), h_chip_offset=np.array([0, 1 << 20, (1 << 20) + 1], np.int32)),
    "table height 0": dict(h_table=_bad_table(0, 50)), "table width negative": dict(h_table=_bad_table(40, -1)),
    "null bank": dict(bank=None), "null table": dict(table=None), "null h_table": dict(h_table=None), "null rows": dict(rows=None),
    "null counts": dict(counts=None), "null h_counts": dict(h_counts=None), "null chip_offset": dict(chip_offset=None),
    "null h_chip_offset": dict(h_chip_offset=None), "null chips": dict(chips=None), "null info": dict(info=None),
}


@pytest.mark.parametrize("case", sorted(EXTRACT_BAD))
def test_chip_extract_refuses_bad_arguments_without_a_gpu(case):
    L = _lib()
    assert _call_extract(L, _extract_args(**EXTRACT_BAD[case])) == EINVAL, case
    assert b"fdet_chip_extract" in L.fdet_last_error()


def test_chip_extract_without_chips_is_success_with_no_launch():
    L = _lib()
    zero = dict(h_counts=np.zeros(2, np.int32), h_chip_offset=np.zeros(3, np.int32), chips=None, info=None)
    assert _call_extract(L, _extract_args(**zero)) == 0
    assert _call_extract(L, _extract_args(K=0, rows=None, **zero)) == 0                 # K = 0 needs no rows
    assert _call_extract(L, _extract_args(h_counts=np.array([1 << 20, 0], np.int32), K=1 << 20, C=7,
                                          h_chip_offset=np.array([0, 1 << 20, 1 << 20], np.int32))) == EINVAL


def _best_args(**kw):
    a = dict(chips=FAKE, info=FAKE, M=3, C=16, ids=FAKE, K=2, seq_offset=FAKE, h_seq_offset=np.array([0, 1, 2], np.int32), n_seq=2,
             frame_base=FAKE, G=4, min_side=0, min_inside256=0, gallery=FAKE, gallery_chips=FAKE, scratch=FAKE, overflow=FAKE,
             stream=None)
    a.update(kw)
    return a


def _call_best(L, a):
    h = a["h_seq_offset"]
    return L.fdet_chip_best_update(a["chips"], a["info"], a["M"], a["C"], a["ids"], a["K"], a["seq_offset"],
                                   h.ctypes.data if isinstance(h, np.ndarray) else h, a["n_seq"], a["frame_base"], a["G"],
                                   a["min_side"], a["min_inside256"], a["gallery"], a["gallery_chips"], a["scratch"], a["overflow"],
                                   a["stream"])


BEST_BAD = {
    "G 0": dict(G=0), "M negative": dict(M=-1), "M above the limit": dict(M=(1 << 20) + 1), "C below 8": dict(C=7), "C above 256": dict(C=257),
    "offset not from 0": dict(h_seq_offset=np.array([1, 1, 2], np.int32)), "offset falls": dict(h_seq_offset=np.array([0, 2, 1], np.int32)),
    "no sequence": dict(n_seq=0), "min_side negative": dict(min_side=-1), "min_inside256 below 0": dict(min_inside256=-1),
    "min_inside256 above 256": dict(min_inside256=257), "K negative": dict(K=-1),
    "null chips": dict(chips=None), "null info": dict(info=None), "null ids": dict(ids=None), "null seq_offset": dict(seq_offset=None),
    "null h_seq_offset": dict(h_seq_offset=None), "null frame_base": dict(frame_base=None), "null gallery": dict(gallery=None),
    "null gallery_chips": dict(gallery_chips=None), "null scratch": dict(scratch=None), "null overflow": dict(overflow=None),
}


@pytest.mark.parametrize("case", sorted(BEST_BAD))
def test_chip_best_update_refuses_bad_arguments_without_a_gpu(case):
    L = _lib()
    assert _call_best(L, _best_args(**BEST_BAD[case])) == EINVAL, case
    assert b"fdet_chip_best_update" in L.fdet_last_error()


def test_chip_best_update_without_chips_is_success_with_no_launch():
    L = _lib()
    assert _call_best(L, _best_args(M=0, chips=None, info=None, ids=None)) == 0
    assert _call_best(L, _best_args(M=0, G=0)) == EINVAL


def test_gallery_bytes():
    L = _lib()
    assert L.fdet_chip_gallery_bytes(1, 1) == 40 and L.fdet_chip_gallery_bytes(3, 1024) == 3 * 1024 * 40
    assert L.fdet_chip_gallery_bytes(0, 4) == 0 and L.fdet_chip_gallery_bytes(2, 0) == 0 and L.fdet_chip_gallery_bytes(-1, -1) == 0
    assert ctypes.sizeof(ctypes.c_int32) * 8 + 8 == R.INFO_DTYPE.itemsize == R.BEST_DTYPE.itemsize == 40


# ------------------------------------------------------------------------------------------ the Python layer
def test_python_argument_errors():
    import fdet_amd  # noqa: F401
    from fdet_amd import chips
    assert chips.INFO_DTYPE == R.INFO_DTYPE and chips.BEST_DTYPE == R.BEST_DTYPE
    assert chips.margin_to_256(0.25) == 64 and chips.margin_to_256(0) == 0 and chips.margin_to_256(1.0) == 256
    for kw in (dict(size=7), dict(size=257), dict(margin=-0.01), dict(margin=1.01)):
        with pytest.raises(ValueError):
            chips.extract_chips(None, None, None, **kw)
        with pytest.raises(ValueError):
            chips.BestShots(**kw)
    for kw in (dict(n_seq=0), dict(capacity=0), dict(min_side=-1), dict(min_inside=-0.1), dict(min_inside=1.1)):
        with pytest.raises(ValueError):
            chips.BestShots(**kw)
