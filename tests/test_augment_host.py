"""Host-side checks of the on-device augmentation (fdet_amd/datasets/augment.py, tests/aug_cpu_ref.py): the parameter sampler's
rates and ranges, seed/step replay, the pixel hash, the motion-blur line kernels, the box transform on hand-worked cases and
the C-ABI's argument checks.  No GPU needed."""
import ctypes
import math

import numpy as np
import pytest

import aug_cpu_ref as R


def _aug():
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets import augment
    return augment


def _wider_sizes(n, seed=0):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(300, 1400, n), g.integers(400, 1024, n)], 1)


def _rate_ok(hits, n, p):
    sd = math.sqrt(n * p * (1 - p))
    return abs(hits - n * p) <= 4 * sd


def test_sampler_rates_and_ranges():
    A = _aug()
    t = A.training_transform((3, 480, 480), seed=5)
    n = 20000
    sizes = _wider_sizes(n)
    P = t.sample(sizes, step=3)
    f = P["flags"]
    for bit in (A.CROP, A.BRIGHTNESS, A.ROTATE, A.NOISE, A.GLASS, A.MOTION):
        assert _rate_ok(int(((f & bit) != 0).sum()), n, 0.2), bit
    assert _rate_ok(int(((f & A.FLIP) != 0).sum()), n, 0.5)
    assert np.all(np.abs(P["angle"]) <= 20.0) and np.all(P["angle"][(f & A.ROTATE) == 0] == 0)
    assert np.abs(P["angle"][(f & A.ROTATE) != 0]).max() > 15.0
    s2 = P["sigma"].astype(np.float64) ** 2
    assert np.all(s2 >= 0) and np.all(s2 <= 400.0 * (1 + 1e-6))
    on = (f & A.BRIGHTNESS) != 0
    assert np.all(np.abs(P["alpha"][on] - 1) <= 0.2 + 1e-6) and np.all(np.abs(P["beta"][on]) <= 51 + 1e-4)
    assert set(np.unique(P["motion_k"][(f & A.MOTION) != 0])) == {3, 5, 7}
    assert np.all(P["motion_k"][(f & A.MOTION) == 0] == 1)
    for p in P[(f & A.MOTION) != 0][:200]:
        k = int(p["motion_k"])
        w = p["motion_w"][:k * k]
        assert abs(float(w.sum()) - 1) < 1e-5 and np.all(p["motion_w"][k * k:] == 0)
    H, W = sizes[:, 0], sizes[:, 1]
    x0, y0, cw, ch = P["crop_x0"], P["crop_y0"], P["crop_w"], P["crop_h"]
    assert np.all(x0 >= 0) and np.all(y0 >= 0) and np.all(cw >= 1) and np.all(ch >= 1)
    assert np.all(x0 + cw <= W) and np.all(y0 + ch <= H)
    nocrop = (f & A.CROP) == 0
    assert np.all(cw[nocrop] == W[nocrop]) and np.all(ch[nocrop] == H[nocrop]) and np.all(x0[nocrop] == 0)
    drawn = ((f & A.CROP) != 0) & ((f & A.CROP_FALLBACK) == 0)
    # w and h are rounded: the ratio bound holds up to half a pixel on each side
    assert np.all((cw[drawn] + 0.5) / (ch[drawn] - 0.5) >= 0.75) and np.all((cw[drawn] - 0.5) / (ch[drawn] + 0.5) <= 4 / 3)
    area = (cw * ch / (H * W.astype(np.float64)))[drawn]
    assert area.min() < 0.15 and area.max() > 0.9


def test_crop_fallback_on_extreme_aspect_ratios():
    A = _aug()
    t = A.DeviceTransform((480, 480), seed=1, p_crop=1.0)
    P = t.sample(np.array([[10, 1000]] * 50 + [[1000, 10]] * 50), step=0)
    assert np.all(P["flags"] & A.CROP_FALLBACK)
    wide, tall = P[:50], P[50:]
    assert np.all(wide["crop_h"] == 10) and np.all(wide["crop_w"] == 13) and np.all(wide["crop_x0"] == (1000 - 13) // 2)
    assert np.all(tall["crop_w"] == 10) and np.all(tall["crop_h"] == 13) and np.all(tall["crop_y0"] == (1000 - 13) // 2)


def test_seed_and_step_replay():
    A = _aug()
    sizes = _wider_sizes(300, seed=4)
    a = A.training_transform((480, 480), seed=9).sample(sizes, 17)
    b = A.training_transform((480, 480), seed=9).sample(sizes, 17)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != A.training_transform((480, 480), seed=9).sample(sizes, 18).tobytes()
    assert a.tobytes() != A.training_transform((480, 480), seed=10).sample(sizes, 17).tobytes()
    d = A.default_transform((3, 480, 480)).sample(sizes, 0)
    assert np.all(d["flags"] == 0) and np.all(d["crop_w"] == sizes[:, 1]) and np.all(d["crop_h"] == sizes[:, 0])


def _fmix_py(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def test_hash_matches_hand_computed_vectors():
    # murmur3's published finaliser values
    assert int(R.fmix32(0)) == 0 and int(R.fmix32(1)) == 0x514E28B7
    assert [int(v) for v in R.fmix32(np.array([1, 2, 0xFFFFFFFF]))] == [_fmix_py(1), _fmix_py(2), _fmix_py(0xFFFFFFFF)]
    for seed, key, tag, y, x in [(0, 0, 0, 0, 0), (1, 2, 3, 4, 5), (0xFFFFFFFF, 0x12345678, 6, 479, 0), (7, 99, 1, 0, 479)]:
        h = _fmix_py(seed ^ 0x9E3779B9)
        for w in (key, tag, y, x):
            h = _fmix_py(h ^ w)
        assert int(R.aug_hash(seed, key, tag, y, x)) == h
    v = R.aug_hash(3, 4, 5, np.arange(4)[:, None], np.arange(6)[None, :])
    assert v.shape == (4, 6) and int(v[2, 5]) == int(R.aug_hash(3, 4, 5, 2, 5))
    n = R.normal(1, 2, 0, np.arange(200)[:, None], np.arange(200)[None, :])
    assert abs(n.mean()) < 0.02 and abs(n.std() - 1) < 0.02


def test_bresenham_kernels_match_hand_drawn_lines():
    A = _aug()
    assert A.bresenham(3, 0, 0, 2, 2).tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert A.bresenham(3, 2, 0, 2, 2).tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1]]
    want5 = np.zeros((5, 5), int)
    for x, y in [(0, 1), (1, 2), (2, 2), (3, 3), (4, 3)]:
        want5[y, x] = 1
    assert A.bresenham(5, 0, 1, 4, 3).tolist() == want5.tolist()
    want7 = np.zeros((7, 7), int)
    for x, y in [(1, 0), (1, 1), (1, 2), (2, 3), (2, 4), (2, 5), (2, 6)]:
        want7[y, x] = 1
    assert A.bresenham(7, 1, 0, 2, 6).tolist() == want7.tolist()
    assert A.bresenham(7, 0, 2, 6, 2).tolist() == [[1 if y == 2 else 0 for _ in range(7)] for y in range(7)]
    assert A.bresenham(7, 6, 5, 0, 5).sum() == 7                      # either direction


def _params(A, H, W, flags=0, crop=None, angle=0.0):
    P = np.zeros(1, A.PARAMS_DTYPE)[0]
    P["flags"] = flags
    P["crop_x0"], P["crop_y0"], P["crop_w"], P["crop_h"] = crop if crop else (0, 0, W, H)
    P["cos_a"], P["sin_a"] = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    P["motion_k"] = 1
    return P


def test_box_transform_hand_worked_cases():
    A = _aug()
    # flip: x -> Wo - x - w
    got = R.boxes([[1, 10, 20, 30, 40]], _params(A, 100, 200, A.FLIP), 100, 200, 100, 200)
    assert got.tolist() == [[1, 160, 20, 30, 40]]
    # crop clipping: window (20,20,50,50), box partly left of it
    got = R.boxes([[1, 10, 30, 20, 10]], _params(A, 100, 100, crop=(20, 20, 50, 50)), 100, 100, 50, 50)
    assert got.tolist() == [[1, 0, 10, 10, 10]]
    # a box wholly outside the crop goes; one that overhangs the source keeps its inside part
    assert R.boxes([[1, 80, 80, 10, 10]], _params(A, 100, 100, crop=(20, 20, 50, 50)), 100, 100, 50, 50).shape == (0, 5)
    assert R.boxes([[1, 98, 10, 10, 10]], _params(A, 100, 100), 100, 100, 100, 100).tolist() == [[1, 98, 10, 2, 10]]
    # min_area=10: 3x3 dropped, 2x5 kept; zero width dropped
    got = R.boxes([[1, 5, 5, 3, 3], [1, 5, 5, 2, 5], [1, 5, 5, 0, 50]], _params(A, 100, 100), 100, 100, 100, 100)
    assert got.tolist() == [[1, 5, 5, 2, 5]]
    # half-to-even: 100 -> 50 halves 5 -> 2.5 -> 2, 9 -> 4.5 -> 4, 7 -> 3.5 -> 4
    got = R.boxes([[1, 5, 5, 9, 9], [1, 7, 7, 9, 9]], _params(A, 100, 100), 100, 100, 50, 50)
    assert got.tolist() == [[1, 2, 2, 4, 4], [1, 4, 4, 4, 4]]
    # rotated envelope of a centred 20x20 square by 45 degrees: half-diagonal 14.142 around the centre
    got = R.boxes([[0.5, 40, 40, 20, 20]], _params(A, 100, 100, A.ROTATE, angle=45.0), 100, 100, 100, 100)
    assert got.tolist() == [[1, 36, 36, 28, 28]]
    # the same square by 90 degrees is itself
    got = R.boxes([[1, 40, 40, 20, 20]], _params(A, 100, 100, A.ROTATE, angle=90.0), 100, 100, 100, 100)
    assert got.tolist() == [[1, 40, 40, 20, 20]]


def test_glass_restatement_is_a_permutation_of_neighbours():
    """The literal albumentations swap only ever moves a pixel by at most one row and one column."""
    g = np.random.default_rng(0)
    x0 = g.integers(0, 256, (3, 9, 11), dtype=np.uint8)
    x1 = R.glass(x0, 3, 4)
    assert x1.shape == x0.shape and not np.array_equal(x1, x0)
    for y in range(9):
        for x in range(11):
            nb = x0[:, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(3, -1)
            assert any(np.array_equal(x1[:, y, x], nb[:, j]) for j in range(nb.shape[1]))


def test_cabi_rejects_bad_arguments_on_the_host():
    A = _aug()
    from fdet_amd import _native
    L = _native.lib()
    table = np.zeros(1, A.IMAGE_DTYPE)
    table[0] = (0, 100, 200)
    P = np.zeros(1, A.PARAMS_DTYPE)
    P["crop_w"], P["crop_h"], P["motion_k"] = 200, 100, 1
    fake = ctypes.c_void_p(0x1000)        # never dereferenced: every call below fails validation first
    assert L.fdet_aug_warp(None, fake, table.ctypes.data, 1, fake, P.ctypes.data, 1, 480, 480, 0, fake, None) == -1
    assert b"null" in L.fdet_last_error()
    assert L.fdet_aug_warp(fake, fake, table.ctypes.data, 1, fake, P.ctypes.data, 0, 480, 480, 0, fake, None) == -1
    assert L.fdet_aug_warp(fake, fake, table.ctypes.data, 1, fake, P.ctypes.data, 1, 480, -3, 0, fake, None) == -1
    bad = P.copy()
    bad["crop_x0"] = 1                    # 1 + 200 > 200
    assert L.fdet_aug_warp(fake, fake, table.ctypes.data, 1, fake, bad.ctypes.data, 1, 480, 480, 0, fake, None) == -1
    assert b"crop" in L.fdet_last_error()
    bad = P.copy()
    bad["image"] = 1                      # outside the table
    assert L.fdet_aug_boxes(fake, fake, fake, table.ctypes.data, 1, fake, bad.ctypes.data, 1, 480, 480, 4, fake, fake, None) == -1
    bad = P.copy()
    bad["crop_h"] = 0
    assert L.fdet_aug_boxes(fake, fake, fake, table.ctypes.data, 1, fake, bad.ctypes.data, 1, 480, 480, 4, fake, fake, None) == -1
    for k in (0, 2, 4, 9):
        bad = P.copy()
        bad["motion_k"] = k
        assert L.fdet_aug_finish(fake, fake, bad.ctypes.data, 1, 480, 480, 0, fake, fake, None) == -1
        assert b"motion_k" in L.fdet_last_error()
