"""fdet_chip_extract / fdet_chip_best_update and chips.py on the GPU against the numpy restatement
(tests/chips_cpu_ref.py).  No tolerance anywhere: every comparison is equality of the chips, of every info field and of the
gallery's bytes."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chips_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import chips, hotpath, tracking
    from fdet_amd.datasets.augment import DeviceImageBank
    return hotpath, chips, tracking, DeviceImageBank


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _images():
    """40x50 (H x W), 1x1 and 64x64, seeded noise."""
    return (_noise(40, 50, 1), _noise(1, 1, 2), _noise(64, 64, 3))


@functools.lru_cache(maxsize=None)
def _bank():
    _, _, _, Bank = _mods()
    return Bank.from_arrays(list(_images()), "cuda")


def _pack(per_image):
    """lists of [score,x,y,w,h] per image -> rows (n,K,5), counts (n,)"""
    K = max(1, max(len(r) for r in per_image))
    rows = np.zeros((len(per_image), K, 5), np.float32)
    for i, r in enumerate(per_image):
        if r:
            rows[i, :len(r)] = np.asarray(r, np.float32)
    return rows, np.array([len(r) for r in per_image], np.int32)


def _device(bank, rows, counts, C, margin256, planar):
    hp = _mods()[0]
    d_counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    chips, info, off = hp.chip_extract(bank.data, bank.d_table, bank.table, torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda(),
                                       d_counts, np.ascontiguousarray(counts, np.int32), C, margin256, planar)
    return chips.cpu().numpy(), info.cpu().numpy().view(R.INFO_DTYPE), off


def _same_extract(got, want, what=""):
    (gc, gi, go), (wc, wi, wo) = got, want
    assert np.array_equal(go, wo), f"{what}offset {go} vs {wo}"
    assert gi.shape == wi.shape and gc.shape == wc.shape and gc.dtype == wc.dtype
    for name in R.INFO_DTYPE.names:
        assert np.array_equal(gi[name], wi[name]), f"{what}info.{name} differs at {np.argwhere(gi[name] != wi[name])[:5].ravel().tolist()}: " \
                                                   f"{gi[name][gi[name] != wi[name]][:5]} vs {wi[name][gi[name] != wi[name]][:5]}"
    if not np.array_equal(gc, wc):
        raise AssertionError(f"{what}chips {np.argwhere((gc != wc).reshape(len(gc), -1).any(1)).ravel()[:8].tolist()} differ")


def _both(images, bank, per_image, C, margin256, planar=0):
    rows, counts = _pack(per_image)
    got = _device(bank, rows, counts, C, margin256, planar)
    want = R.extract(list(images), rows, counts, C, margin256, planar)
    _same_extract(got, want, f"C={C} margin256={margin256} planar={planar}: ")
    return got


# rows of the 40x50 image: every window side of the issue at margin 0, the four edges, both parities of X1 + X2 - S, and the
# invalid rows between valid neighbours
ROWS_0 = [
    [0.9, 10, 12, 1, 1], [0.9, 20, 7, 3, 3], [0.9, 31, 22, 5, 5], [0.9, 4, 4, 8, 8], [0.9, 15, 10, 20, 20], [0.9, 11, 9, 23, 23],
    [NAN, 5, 5, 8, 8],                                       # NaN score
    [0.9, 3, 2, 33, 33],
    [0.9, INF, 5, 8, 8],
    [0.9, -5, 10, 12, 12], [0.9, 12, -6, 13, 13], [0.9, 45, 14, 10, 10], [0.9, 20, 35, 10, 10],       # left, top, right, bottom
    [0.9, 5, 5, 0.4, 8],                                     # w < 1
    [0.9, 10, 20, 7, 8], [0.9, 10, 20, 8, 8], [0.9, 9.5, 20.5, 8, 5],                                   # odd / even X1 + X2 - S
    [0.9, 16390, 5, 8, 8],                                   # a corner past 16384
    [0.9, 60, 5, 8, 8], [0.9, 5, -30, 8, 8],                 # outside the image
    [0.9, 0, 0, 8193, 10],                                   # S > 8192
    [0.9, -4000, -4100, 8192, 8192],                         # S = 8192 at margin 0: the whole image and far beyond
    [0.9, 1, 1, 47.5, 37.5], [-INF, 5, 5, 8, 8], [0.9, 5, NAN, 8, 8], [0.9, 5, 5, 8, INF],
]
ROWS_1 = [[0.5, 0, 0, 1, 1], [0.5, -3, -2, 8, 6]]            # the whole 1x1 image; a window far larger than it
ROWS_2 = [[0.7, 2, 3, 60, 60], [0.7, -10, 20, 100, 90], [0.7, 30, -80, 150, 200], [0.7, 16, 16, 17, 17], [0.7, 40, 7, 16, 16]]


@pytest.mark.parametrize("margin256", [0, 64, 256])
@pytest.mark.parametrize("C", [8, 16])
def test_extract_small_chips(C, margin256):
    images, bank = _images(), _bank()
    per_image = [ROWS_0, ROWS_1, ROWS_2]
    chips, info, off = _both(images, bank, per_image, C, margin256)
    valid = info["flags"][:len(ROWS_0)] == 1
    n_bad = 10 if margin256 == 0 else 11                    # with any margin the S = 8192 row passes the limit
    assert int((~valid).sum()) == n_bad and not chips[:len(ROWS_0)][~valid].any()
    for name in ("wx0", "wy0", "S", "inside256", "flags", "reserved", "sharp"):
        assert not info[name][:len(ROWS_0)][~valid].any()
    S = set(info["S"][info["flags"] == 1].tolist())
    if margin256 == 0:
        assert {1, 3, 5, 8, 16, 20, 23, 33, 8192} <= S
        assert any(s > 64 * C for s in S) and any(8 * C < s < 64 * C for s in S) and any(C < s <= 8 * C for s in S) \
            and any(s < C for s in S)                        # a wave per pixel along rows and row-major, a thread per pixel, bilinear
    n0 = len(ROWS_0)
    assert len(info) == sum(map(len, per_image)) and off.tolist() == [0, n0, n0 + len(ROWS_1), n0 + len(ROWS_1) + len(ROWS_2)]
    inside = info["inside256"][info["flags"] == 1]
    assert (inside <= 256).all() and (inside == 256).any() and (inside < 256).any() and (inside == 0).sum() <= 1
    # planar: the same pixels
    pchips, pinfo, _ = _both(images, bank, per_image, C, margin256, planar=1)
    assert np.array_equal(pchips.transpose(0, 2, 3, 1), chips) and pinfo.tobytes() == info.tobytes()


def test_extract_counts_of_zero_no_rows_and_one_image():
    hp, chips_mod, _, Bank = _mods()
    images, bank = _images(), _bank()
    got = _both(images, bank, [ROWS_0[:4], [], ROWS_2[:2]], 8, 64)                                         # a count of 0 between two others
    assert got[2].tolist() == [0, 4, 4, 6]
    got = _both(images, bank, [[], [], []], 8, 64)
    assert got[0].shape == (0, 8, 8, 3) and got[2].tolist() == [0, 0, 0, 0]
    # K = 0
    rows0 = torch.zeros(3, 0, 5, device="cuda")
    cs = chips_mod.extract_chips(bank, rows0, torch.zeros(3, dtype=torch.int32, device="cuda"), size=16)
    assert len(cs) == 0 and tuple(cs.chips.shape) == (0, 16, 16, 3) and cs.offset.tolist() == [0, 0, 0, 0] and len(cs.records()) == 0
    # n_images = 1, through extract_chips with indices (image 2 of the bank) and a fractional margin
    rows, counts = _pack([ROWS_2])
    cs = chips_mod.extract_chips(bank, torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), indices=[2], size=16, margin=0.25)
    want = R.extract([images[2]], rows, counts, 16, 64)
    _same_extract((cs.chips.cpu().numpy(), cs.records(), cs.offset), want)
    # the chips as a bank
    arrays = cs.as_bank().to_arrays()
    assert len(arrays) == len(ROWS_2) and all(np.array_equal(a, c) for a, c in zip(arrays, want[0]))
    with pytest.raises(ValueError):
        chips_mod.extract_chips(bank, torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(), indices=[2], size=16, planar=True).as_bank()
    # a count beyond K is refused by the library before anything is written
    from fdet_amd import FdetError
    with pytest.raises(FdetError):
        chips_mod.extract_chips(bank, torch.from_numpy(rows).cuda(), torch.tensor([99], dtype=torch.int32, device="cuda"), indices=[2], size=16)


def test_extract_112():
    images, bank = _images(), _bank()
    chips, info, _ = _both(images, bank, [[], [], [[0.7, 9, 11, 45, 40]]], 112, 0)                         # S = 45 < C: bilinear
    assert info["S"][0] == 45 and info["sharp"][0] > 0
    _both(images, bank, [[[0.7, 3, -4, 30, 30]], [], [[0.7, 1, 2, 60, 61], [0.7, 0, 0, 64, 64]]], 112, 256)  # S = 90 (bilinear), 183, 192 (area)


def test_extract_256_checkerboard_sharpness_does_not_wrap():
    _, _, _, Bank = _mods()
    C = 256
    board = (((np.arange(C)[:, None] + np.arange(C)[None, :]) & 1) * 255).astype(np.uint8)
    img = np.ascontiguousarray(np.repeat(board[:, :, None], 3, 2))
    bank = Bank.from_arrays([img], "cuda")
    chips, info, _ = _both([img], bank, [[[1.0, 0, 0, 256, 256], [1.0, -20, 100, 300, 280]]], C, 0)
    assert np.array_equal(chips[0], img) and info["S"][0] == 256 and info["inside256"][0] == 256
    assert int(info["sharp"][0]) == 254 ** 2 * 1020 ** 2 == 67122446400 > 2 ** 32
    assert info["S"][1] == 300 and 0 < info["inside256"][1] < 256


# ------------------------------------------------------------------------------------------ the gallery
def _info(image, row, sharp, S=20, inside256=256, flags=1):
    n = len(image)
    f = np.zeros(n, R.INFO_DTYPE)
    f["image"], f["row"], f["sharp"], f["S"], f["inside256"], f["flags"] = image, row, sharp, S, inside256, flags
    f["wx0"], f["wy0"] = np.arange(n) * 3 - 5, 7 - np.arange(n)
    return f


class _Gallery:
    """The same gallery on the device and in the restatement."""

    def __init__(self, n_seq, G, C):
        self.n_seq, self.G, self.C = n_seq, G, C
        self.ref, self.ref_chips = R.fresh_gallery(n_seq, G, C)
        self.ref_over = 0
        self.state = torch.zeros(n_seq * G * 40, dtype=torch.uint8, device="cuda")
        self.chips = torch.zeros(n_seq, G, C * C * 3, dtype=torch.uint8, device="cuda")
        self.scratch = torch.full((n_seq * G,), -1, dtype=torch.int64, device="cuda")      # stale: the call clears it
        self.over = torch.zeros(1, dtype=torch.int64, device="cuda")

    def update(self, chips, info, ids, seq_offset, frame_base, min_side=0, min_inside256=0):
        hp = _mods()[0]
        h_off = np.ascontiguousarray(seq_offset, np.int32)
        hp.chip_best_update(torch.from_numpy(chips).cuda(), torch.from_numpy(info.view(np.uint8).copy()).cuda(),
                            torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda(), torch.from_numpy(h_off).cuda(), h_off,
                            torch.from_numpy(np.ascontiguousarray(frame_base, np.int32)).cuda(), self.G, min_side, min_inside256,
                            self.state, self.chips, self.scratch, self.over)
        self.ref_over += R.best_update(chips, info, ids, seq_offset, frame_base, self.ref, self.ref_chips, min_side, min_inside256)
        return self.check()

    def check(self):
        got = self.state.cpu().numpy().view(R.BEST_DTYPE).reshape(self.n_seq, self.G)
        for name in R.BEST_DTYPE.names:
            assert np.array_equal(got[name], self.ref[name]), f"gallery.{name}: {got[name].tolist()} vs {self.ref[name].tolist()}"
        assert got.tobytes() == self.ref.tobytes()
        assert np.array_equal(self.chips.cpu().numpy(), self.ref_chips), "gallery chips differ"
        assert int(self.over.item()) == self.ref_over
        return got


def test_gallery_rules():
    C, G, K = 8, 3, 4
    g = _Gallery(2, G, C)
    chips = np.random.default_rng(5).integers(0, 256, (16, C, C, 3), dtype=np.uint8)
    # four frames of four rows; frames 0-1 are sequence 0, frames 2-3 sequence 1
    image, row = np.repeat(np.arange(4), K), np.tile(np.arange(K), 4)
    ids = np.array([[1, 2, 0, 5],        # id 0 is ignored, id 5 > G overflows
                    [1, 2, 3, 1],
                    [1, 2, 2, -1],       # the same ids in the other sequence
                    [2, 1, 4, 3]], np.int32)
    sharp = np.array([50, 70, 9999, 9999,
                      50, 60, 10, 40,    # id 1: 50 (chip 0) ties with 50 (chip 4): the lower index; chip 7 also id 1
                      30, 80, 80, 9999,  # id 2 of sequence 1: chips 9 and 10 tie
                      90, 30, 9999, 5], np.int64)
    info = _info(image, row, sharp)
    info["S"][6], info["inside256"][15] = 9, 100             # gated below
    got = g.update(chips, info, ids, [0, 2, 4], [100, 200], min_side=10, min_inside256=128)
    assert got["id"].tolist() == [[1, 2, 0], [1, 2, 0]]       # id 3: chip 6 fails min_side, chip 15 min_inside256
    assert got["sharp"].tolist() == [[50, 70, 0], [30, 90, 0]] and got["seen"].tolist() == [[3, 2, 0], [2, 3, 0]]
    assert got["frame"].tolist() == [[100, 100, 0], [200, 201, 0]]
    assert int(g.over.item()) == 2                          # ids 5 and 4
    dev_chips = g.chips.cpu().numpy()
    assert np.array_equal(dev_chips[0, 0], chips[0].reshape(-1)) and np.array_equal(dev_chips[1, 1], chips[12].reshape(-1))
    assert not dev_chips[:, 2].any()
    # a later call with equal sharpness replaces nothing; seen still counts
    chips2 = np.random.default_rng(6).integers(0, 256, (2, C, C, 3), dtype=np.uint8)
    got = g.update(chips2, _info([0, 0], [0, 1], [50, 70]), np.array([[1, 2, 0, 0]], np.int32), [0, 1, 1], [102, 202])
    assert got["frame"].tolist()[0] == [100, 100, 0] and got["seen"].tolist() == [[4, 3, 0], [2, 3, 0]]
    assert np.array_equal(g.chips.cpu().numpy()[0, 0], chips[0].reshape(-1))
    # a sharper one replaces and copies its bytes; the gates are off now, so id 3 gets its first entry
    got = g.update(chips2, _info([0, 0], [2, 0], [51, 1], S=[5, 5], inside256=[3, 3]), np.array([[3, 0, 1, 0]], np.int32), [0, 0, 1],
                   [103, 203])
    assert got["sharp"].tolist() == [[50, 70, 0], [51, 90, 1]] and got["frame"].tolist()[1] == [203, 201, 203]
    assert np.array_equal(g.chips.cpu().numpy()[1, 0], chips2[0].reshape(-1)) and got["seen"].tolist()[1] == [3, 3, 1]
    # invalid chips and M = 0 change nothing
    before = g.state.clone()
    g.update(chips2, _info([0, 0], [0, 1], [10 ** 6, 10 ** 6], flags=0), np.array([[1, 2]], np.int32), [0, 1, 1], [0, 0])
    g.update(chips2[:0], _info([], [], []), np.zeros((1, 2), np.int32), [0, 1, 1], [0, 0])
    assert torch.equal(before, g.state)


Res = namedtuple("Res", "rows counts ids misses")            # what BestShots.update reads of a TrackResult


@functools.lru_cache(maxsize=None)
def _sequence():
    """24 frames of 48x64 noise of varying contrast, three rows per frame with ids in 0..5 (capacity 4: id 5 overflows), some
    bridged (misses > 0).  Frames t and t + 12 and their boxes are equal, so sharpness ties between chunks."""
    g = np.random.default_rng(11)
    T, K = 24, 3
    frames = []
    for t in range(T):
        f = _noise(48, 64, 100 + t % 12).astype(np.int64)
        frames.append(np.ascontiguousarray((128 + (f - 128) * (1 + t % 4) // 4).astype(np.uint8)))
    rows = np.zeros((T, K, 5), np.float32)
    rows[..., 0] = 0.9
    rows[..., 1:3] = np.array([[4, 5], [30, 9], [20, 25]], np.float32)[None] + np.tile(g.integers(-1, 2, (12, 1, 2)), (2, 1, 1))
    rows[..., 3:] = np.array([[16, 18], [21, 20], [30, 24]], np.float32)[None]
    counts = g.integers(1, K + 1, T).astype(np.int32)
    ids = g.integers(0, 6, (T, K)).astype(np.int32)
    misses = (g.random((T, K)) < 0.25).astype(np.int32)
    return tuple(frames), rows, counts, ids, misses


def test_gallery_is_independent_of_the_chunking():
    _, chips_mod, _, Bank = _mods()
    frames, rows, counts, ids, misses = _sequence()
    T, C, G = len(frames), 16, 4
    bank = Bank.from_arrays(list(frames), "cuda")
    # the restatement, whole
    ref, ref_chips = R.fresh_gallery(1, G, C)
    rc, ri, _ = R.extract(list(frames), rows, counts, C, 64)
    over = R.best_update(rc, ri, np.where(misses == 0, ids, 0), [0, T], [0], ref, ref_chips)
    assert over > 0 and (ref["id"] != 0).all() and len(set(ref["frame"][0].tolist())) > 1
    d = [torch.from_numpy(a).cuda() for a in (rows, counts, ids, misses)]
    for chunk in (24, 1, 5):
        best = chips_mod.BestShots(capacity=G, size=C, margin=0.25)
        for a in range(0, T, chunk):
            b = min(a + chunk, T)
            best.update(bank, Res(*(x[a:b] for x in d)), indices=range(a, b))
        assert best.snapshot().tobytes() == ref.tobytes(), f"chunks of {chunk}: gallery records differ"
        assert np.array_equal(best.chips.cpu().numpy(), ref_chips), f"chunks of {chunk}: gallery chips differ"
        assert best.overflow == over
        rec, pics = best.gallery()
        assert rec["id"].tolist() == [1, 2, 3, 4] and np.array_equal(pics.reshape(G, -1), ref_chips[0])
    best.reset()
    assert not best.snapshot()["id"].any() and best.overflow == 0 and not best.frame_base.any()


def test_tracker_to_best_shots_a_bridged_frame_never_wins(tmp_path):
    _, chips_mod, tracking, Bank = _mods()
    T, C = 6, 16
    frames = []
    for t in range(T):
        f = _noise(60, 80, 40 + t).astype(np.int64)
        amp = 16 if t == 3 else (t + 1)                      # frame 3 holds by far the sharpest pixels
        frames.append(np.ascontiguousarray((128 + (f - 128) * amp // 16).astype(np.uint8)))
    rows = np.zeros((T, 2, 5), np.float32)
    rows[:, 0] = [0.9, 20, 15, 24, 26]
    counts = np.ones(T, np.int32)
    counts[3] = 0                                            # the detector misses the face in frame 3
    bank = Bank.from_arrays(frames, "cuda")
    tr = tracking.FaceTracker(min_hits=1, max_misses=3, alpha=1.0)
    res = tr.update(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda())
    assert res.counts.cpu().tolist() == [1] * T and res.misses[:, 0].cpu().tolist() == [0, 0, 0, 1, 0, 0]      # bridged
    best = chips_mod.BestShots(size=C, capacity=8)
    cs = best.update(bank, res)
    rec = cs.records()
    assert int(np.argmax(rec["sharp"])) == 3 and (rec["flags"] == 1).all()
    grec, pics = best.gallery()
    seen_frames = [t for t in range(T) if t != 3]
    want = seen_frames[int(np.argmax(rec["sharp"][seen_frames]))]
    assert grec["id"].tolist() == [1] and int(grec["frame"][0]) == want != 3 and int(grec["seen"][0]) == T - 1
    assert int(grec["sharp"][0]) == int(rec["sharp"][want]) and np.array_equal(pics[0], cs.chips[want].cpu().numpy())
    # against the restatement, from the tracker's own rows
    ref, ref_chips = R.fresh_gallery(1, 8, C)
    rc, ri, _ = R.extract(frames, res.rows.cpu().numpy(), res.counts.cpu().numpy(), C, 64)
    R.best_update(rc, ri, np.where(res.misses.cpu().numpy() == 0, res.ids.cpu().numpy(), 0), [0, T], [0], ref, ref_chips)
    assert best.snapshot().tobytes() == ref.tobytes() and np.array_equal(best.chips.cpu().numpy(), ref_chips)
    from PIL import Image
    paths = best.save(tmp_path)
    assert [os.path.basename(p) for p in paths] == ["seq0_track1.png"] and np.array_equal(np.asarray(Image.open(paths[0])), pics[0])


def test_two_sequences_through_best_shots():
    _, chips_mod, _, Bank = _mods()
    frames, rows, counts, ids, misses = _sequence()
    T, C, G = 10, 8, 8
    bank = Bank.from_arrays(list(frames[:T]), "cuda")
    off = [0, 4, 10]
    best = chips_mod.BestShots(n_seq=2, capacity=G, size=C, margin=0.0, min_side=20, min_inside=0.5)
    d = [torch.from_numpy(a[:T]).cuda() for a in (rows, counts, ids, misses)]
    with pytest.raises(ValueError):
        best.update(bank, Res(*d))                           # two sequences need seq_offset
    best.update(bank, Res(*d), seq_offset=off)
    best.update(bank, Res(*d), seq_offset=off)               # the same frames again: equal sharpness, nothing replaced
    ref, ref_chips = R.fresh_gallery(2, G, C)
    rc, ri, _ = R.extract(list(frames[:T]), rows[:T], counts[:T], C, 0)
    for base in ([0, 0], [4, 6]):
        R.best_update(rc, ri, np.where(misses[:T] == 0, ids[:T], 0), off, base, ref, ref_chips, 20, 128)
    assert best.snapshot().tobytes() == ref.tobytes() and np.array_equal(best.chips.cpu().numpy(), ref_chips)
    assert (ref["id"][0] != 0).any() and (ref["id"][1] != 0).any() and ref["frame"].max() < 6 and best.frame_base.tolist() == [8, 12]


# ------------------------------------------------------------------------------------------ scripts
def test_scripts_write_chips_only_when_asked(tmp_path, monkeypatch):
    """track_frames --best-shots and detect_images --chips on an untrained network: the text outputs are those of a run
    without the flags, the gallery does not depend on the chunking, and the files are the chips of the boxes written."""
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images, track_frames
    monkeypatch.chdir(tmp_path)
    g = np.random.default_rng(3)
    base = g.integers(0, 256, (12, 16, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)          # 96 x 128, blocky
    frames = tmp_path / "frames"
    frames.mkdir()
    arrays = [np.roll(base, 2 * i, axis=1) for i in range(4)]
    for i, a in enumerate(arrays):
        Image.fromarray(a).save(frames / f"f{i:03d}.png")
    common = ["--frames", str(frames), "--model", "poolresnet", "--filters", "64", "--probability-threshold", "0.02",
              "--min-hits", "1", "--max-misses", "2"]
    torch.manual_seed(11)
    plain = track_frames.main(common + ["--out", str(tmp_path / "plain.txt")])
    torch.manual_seed(11)
    shots = track_frames.main(common + ["--out", str(tmp_path / "shots.txt"), "--best-shots", str(tmp_path / "a"), "--chip-size", "24",
                                        "--max-frames", "3"])
    text = (tmp_path / "plain.txt").read_text()
    assert plain == shots and text == (tmp_path / "shots.txt").read_text() and plain["tracks"] > 0
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names and set(names) <= {f"seq0_track{k}.png" for k in range(1, plain["tracks"] + 1)}
    # the picture of track k is the chip of one of the lines of track k
    boxes = {}
    for ln in text.splitlines():
        f = ln.split(",")
        boxes.setdefault(int(f[1]), []).append((int(f[0]) - 1, [float(f[6])] + [float(v) for v in f[2:6]]))
    for n in names:
        k = int(n[len("seq0_track"):-4])
        cuts = [R.cut(arrays[t], *R.window(row, 128, 96, 64), 24) for t, row in boxes[k] if R.window(row, 128, 96, 64) is not None]
        a = np.asarray(Image.open(tmp_path / "a" / n))
        assert a.shape == (24, 24, 3) and any(np.array_equal(a, c) for c in cuts), n
    # detect_images: the same result file, and one chip file per box
    imgs = tmp_path / "imgs" / "sub"
    imgs.mkdir(parents=True)
    Image.fromarray(arrays[0]).save(imgs / "x.png")
    Image.fromarray(arrays[1][:50]).save(tmp_path / "imgs" / "y.png")
    dcommon = ["--model", "poolresnet", "--filters", "64", "--images", str(tmp_path / "imgs"), "--tile", "--probability-threshold", "0.02"]
    torch.manual_seed(11)
    d0 = detect_images.main(dcommon + ["--out", str(tmp_path / "d0.txt")])
    torch.manual_seed(11)
    d1 = detect_images.main(dcommon + ["--out", str(tmp_path / "d1.txt"), "--chips", str(tmp_path / "faces"), "--chip-margin", "0"])
    assert (tmp_path / "d0.txt").read_text() == (tmp_path / "d1.txt").read_text() and torch.equal(d0["rows"], d1["rows"])
    assert int(d1["counts"].sum()) > 0
    want = {os.path.join("faces", os.path.splitext(n)[0] + f"_{j}.png") for n, c in zip(d1["names"], d1["counts"].tolist()) for j in range(c)}
    got = {os.path.relpath(p, tmp_path) for p in (tmp_path / "faces").rglob("*.png")}
    assert got == want
    src = {"sub/x.png": arrays[0], "y.png": arrays[1][:50]}
    for i, n in enumerate(d1["names"]):
        for j in range(int(d1["counts"][i])):
            a = np.asarray(Image.open(tmp_path / "faces" / (os.path.splitext(n)[0] + f"_{j}.png")))
            win = R.window(d1["rows"][i, j].numpy(), src[n].shape[1], src[n].shape[0], 0)
            assert a.shape == (112, 112, 3) and (not a.any() if win is None else np.array_equal(a, R.cut(src[n], *win, 112)))
