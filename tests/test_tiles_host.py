"""Host-side checks of tiled detection: the tile plan (fdet_amd/tiling.py), the numpy merge of tests/tiles_cpu_ref.py
against a brute-force version, and the C-ABI surface of csrc/fdet_tiles.hip.  No GPU."""
import os
import re

import numpy as np
import pytest

import tiles_cpu_ref as R

SIZES = [(100, 300), (480, 480), (481, 480), (480, 481), (481, 481), (700, 1024), (3000, 4000), (1, 1), (479, 2000)]  # (h, w)


def _T():
    import fdet_amd  # noqa: F401
    from fdet_amd import tiling
    return tiling


@pytest.mark.parametrize("tile_sizes,overlap,whole", [((480,), 0.25, True), ((480,), 0.0, False), ((320, 640), 0.5, True),
                                                      ((7,), 0.9, False), ((), 0.25, True)])
def test_plan_covers_every_pixel_and_matches_the_closed_form(tile_sizes, overlap, whole):
    T = _T()
    sizes = SIZES if tile_sizes != (7,) else [(1, 1), (7, 7), (8, 7), (30, 61)]
    p = T.plan_tiles(sizes, tile_sizes, overlap, whole)
    q = T.plan_tiles(np.asarray(sizes), tile_sizes, overlap, whole)
    assert p.tiles.dtype == T.TILE_DTYPE and p.tile_offset.dtype == np.int32
    assert p.tiles.tobytes() == q.tiles.tobytes() and np.array_equal(p.tile_offset, q.tile_offset)      # deterministic
    recs, offs = R.plan(sizes, tile_sizes, overlap, whole)
    assert [tuple(int(v) for v in t) for t in p.tiles] == recs and p.tile_offset.tolist() == offs
    for i, (h, w) in enumerate(sizes):
        mine = p.tiles[p.tile_offset[i]:p.tile_offset[i + 1]]
        assert (mine["image"] == i).all()
        assert (mine["x0"] >= 0).all() and (mine["y0"] >= 0).all() and (mine["w"] > 0).all() and (mine["h"] > 0).all()
        assert (mine["x0"] + mine["w"] <= w).all() and (mine["y0"] + mine["h"] <= h).all()
        whole_n = sum(1 for t in mine if (t["x0"], t["y0"], t["w"], t["h"]) == (0, 0, w, h))
        tiles_only = [t for t in mine if (t["x0"], t["y0"], t["w"], t["h"]) != (0, 0, w, h)]
        fits = any(min(t, w) == w and min(t, h) == h for t in tile_sizes)
        assert whole_n == (1 if whole or fits else 0)
        if whole:
            assert tuple(mine[0])[1:] == (0, 0, w, h)                       # the whole-image window comes first
        # closed form: per tile side n_origins(h) * n_origins(w) windows, minus the ones equal to the whole image
        want = 0
        for t in tile_sizes:
            s = R.stride_of(t, overlap)
            want += R.n_origins(h, t, s) * R.n_origins(w, t, s) - (1 if (min(t, w) == w and min(t, h) == h) else 0)
        assert len(tiles_only) == want
        # coverage by the tile windows alone (the whole-image window would make it trivial)
        if tile_sizes:
            cover = np.zeros((h, w), bool) if h * w <= 1 << 21 else None
            if cover is not None:
                for t in mine if not whole else list(tiles_only) + ([mine[0]] if fits else []):
                    cover[t["y0"]:t["y0"] + t["h"], t["x0"]:t["x0"] + t["w"]] = True
                assert cover.all()
            else:                                                            # separable: every row and column is covered
                for t in tile_sizes:
                    s = R.stride_of(t, overlap)
                    for L in (h, w):
                        o = R.origins(L, t, s)
                        c = np.zeros(L, bool)
                        for a in o:
                            c[a:a + min(t, L)] = True
                        assert c.all()


@pytest.mark.parametrize("t,overlap", [(480, 0.25), (480, 0.0), (320, 0.5), (7, 0.9), (100, 0.33)])
def test_adjacent_windows_overlap_by_at_least_the_requested_amount(t, overlap):
    T = _T()
    ov = int(np.floor(overlap * t + 0.5))
    s = T.tile_stride(t, overlap)
    assert s == max(1, t - ov) == R.stride_of(t, overlap)
    for L in (1, t - 1, t, t + 1, t + s, t + s + 1, 700, 1024, 3000, 4000):
        o = T.axis_origins(L, t, s)
        assert o == R.origins(L, t, s) and len(o) == R.n_origins(L, t, s)
        assert o[0] == 0 and o[-1] + min(t, L) == L and all(b > a for a, b in zip(o, o[1:]))
        for a, b in zip(o, o[1:]):
            assert a + t - b >= ov                                          # shared pixels of neighbours


def test_tile_counts_of_the_named_sizes():
    T = _T()
    s = T.tile_stride(480, 0.25)
    assert s == 360
    n = lambda L: len(T.axis_origins(L, 480, s))
    assert [n(L) for L in (100, 480, 481, 700, 1024, 3000, 4000)] == [1, 1, 2, 2, 3, 8, 11]
    p = T.plan_tiles([(700, 1024), (3000, 4000), (480, 480)], (480,), 0.25, True)
    assert np.diff(p.tile_offset).tolist() == [1 + 2 * 3, 1 + 8 * 11, 1]
    with pytest.raises(ValueError):
        T.plan_tiles([(10, 10)], (), 0.25, False)
    with pytest.raises(ValueError):
        T.plan_tiles([(10, 10)], (480,), 1.0, True)


def _random_case(seed, n_images=3, K=24, margin=0.0, ties=True):
    g = np.random.default_rng(seed)
    sizes = [(int(g.integers(300, 1200)), int(g.integers(300, 1200))) for _ in range(n_images)]
    recs, offs = R.plan(sizes, (480,), 0.25, True)
    Tn = len(recs)
    rows = np.zeros((Tn, K, 5), np.float32)
    counts = g.integers(0, K + 1, Tn).astype(np.int32)
    counts[g.integers(0, Tn, max(1, Tn // 4))] = 0                          # empty tiles
    for t in range(Tn):
        c = int(counts[t])
        sc = g.uniform(0.01, 1.0, c).astype(np.float32)
        if ties:
            sc = np.round(sc * 8) / 8                                       # many equal scores
        xy = g.uniform(-5, 470, (c, 2))
        wh = g.uniform(0, 120, (c, 2))
        wh[g.uniform(size=c) < 0.15] = 0                                    # zero-area boxes
        rows[t, :c] = np.concatenate([sc[:, None], xy, wh], 1).astype(np.float32)
        rows[t, c:] = -7.0                                                  # garbage past the count is never read
    return sizes, recs, offs, rows, counts


@pytest.mark.parametrize("seed,margin,thr", [(0, 0.0, 0.5), (1, 0.0, 0.01), (2, 12.0, 0.5), (3, 40.0, 0.3)])
def test_numpy_merge_equals_the_bruteforce(seed, margin, thr):
    sizes, recs, offs, rows, counts = _random_case(seed, margin=margin)
    a = R.merge(rows, counts, recs, offs, sizes, 480, 480, margin, thr, 4864)
    b = R.merge(rows, counts, recs, offs, sizes, 480, 480, margin, thr, 4864, one=R.merge_image_bruteforce)
    assert a[2] == b[2] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    assert a[1].sum() > 0
    for i in range(len(sizes)):                                             # survivors come in descending score
        s = a[0][i, :a[1][i], 0]
        assert (np.diff(s) <= 0).all()


def test_edge_rule_on_every_side():
    """A 960x960 image, tile 480, overlap 0: window (480, 0) has interior left and bottom sides and image top and right
    sides.  A box hugging an interior side is dropped, the same box hugging an image side is kept."""
    Ho = Wo = 480
    hw = (960, 960)
    box = lambda x, y, w=50, h=50: np.array([0.9, x, y, w, h], np.float32)
    cases = {  # window -> (dropped boxes, kept boxes)
        (480, 0, 480, 480): ([box(2, 200), box(200, 429)], [box(200, 0), box(430, 200), box(10, 200), box(200, 420)]),
        (0, 480, 480, 480): ([box(200, 3), box(428, 200)], [box(0, 200), box(200, 430)]),
        (0, 0, 960, 960): ([], [box(0, 0), box(430, 430), box(0, 430), box(430, 0)]),
        (240, 240, 480, 480): ([box(9.5, 100), box(100, 9.5), box(421, 100), box(100, 421)], [box(10, 10, 460, 460)]),
    }
    for win, (dropped, kept) in cases.items():
        for d in dropped:
            assert R.cut_by_window(d, win, hw, Ho, Wo, 10.0), (win, d)
            assert not R.cut_by_window(d, win, hw, Ho, Wo, 0.0)
        for d in kept:
            assert not R.cut_by_window(d, win, hw, Ho, Wo, 10.0), (win, d)
    # through the merge: only the kept boxes come out, in source pixels
    win = (480, 0, 480, 480)
    d, k = cases[win]
    rows = np.stack(d + k)[None]
    out, cnt, rej = R.merge(rows, [len(d) + len(k)], [(0,) + win], [0, 1], [hw], Ho, Wo, 10.0, 0.99, 16)
    assert rej == 0 and cnt[0] == len(k)
    assert sorted(map(tuple, out[0, :cnt[0], 1:3].tolist())) == sorted((float(b[1] + 480), float(b[2])) for b in k)


def test_merge_limits_reject_whole_images():
    rows = np.zeros((2, 3, 5), np.float32)
    rows[:, :, 0] = 0.5
    rows[0, :, 1] = [0, 100, 200]
    rows[1, :, 1] = [0, 100, 200]
    rows[:, :, 3:] = 10
    tiles = [(0, 0, 0, 480, 480), (1, 0, 0, 480, 480)]
    out, cnt, rej = R.merge(rows, [3, 3], tiles, [0, 1, 2], [(480, 480)] * 2, 480, 480, 0.0, 0.5, 2)
    assert rej == 2 and cnt.tolist() == [0, 0] and not out.any()            # three survivors, room for two
    out, cnt, rej = R.merge(rows, [3, 4], tiles, [0, 1, 2], [(480, 480)] * 2, 480, 480, 0.0, 0.5, 3)
    assert rej == 1 and cnt.tolist() == [3, 0]                              # counts[t] > K


def test_header_declares_and_library_exports_the_entry_points():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    txt = open(_native.HEADER_PATH).read()
    assert re.search(r"typedef struct fdet_tile \{\s*int32_t image, x0, y0, w, h;", txt)
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    L = _native.lib()
    for name in ("fdet_tile_gather", "fdet_tile_merge"):
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(L, name), f"{name} declared in include/fdet.h but not exported"
    # host-side validation needs no GPU: null pointers and bad sizes are refused before any launch
    assert L.fdet_tile_gather(None, None, None, 1, None, None, 1, 480, 480, None, None) == -1
    assert b"tile_gather" in L.fdet_last_error()
    assert L.fdet_tile_merge(None, None, None, None, 1, 1, 1, 480, 480, None, 0.0, 0.5, 1, None, None, None, None) == -1
    assert b"tile_merge" in L.fdet_last_error()


def test_generated_assembly_has_no_scalar_memory_store_or_scalar_atomic(tmp_path):
    """csrc/fdet_tiles.hip cross-compiled to gfx950 assembly: the only atomic is the 64-bit vector add on the rejected counter."""
    import shutil
    import subprocess
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(os.path.dirname(_native.LIB_PATH), "..", "csrc")
    out = tmp_path / "fdet_tiles.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.dirname(_native.HEADER_PATH),
                    "-S", "--cuda-device-only", "-o", str(out), os.path.join(csrc, "fdet_tiles.hip")], check=True, capture_output=True)
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\b", out.read_text(), flags=re.M)
    scalar_mem = [o for o in ops if re.match(r"s_(store|buffer_store|scratch_store|atomic|buffer_atomic|dcache_wb|dcache_discard)", o)]
    assert not scalar_mem, sorted(set(scalar_mem))
    atomics = sorted({o for o in ops if "atomic" in o})
    assert atomics == ["global_atomic_add_x2"], atomics
    assert "k_tile_gather" in out.read_text() and "k_tile_merge" in out.read_text()
