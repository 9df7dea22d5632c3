"""The host side of Gaussian-blur anonymisation against Pillow: the radius arithmetic of `render.blur_table`,
the restated pass (tests/render_blur_cpu_ref.py) and the whole rule.  No tolerance anywhere: every comparison is equality of
bytes.  Needs no GPU."""
import functools
import os
import sys

import numpy as np
import pytest

pytest.importorskip("PIL")
from PIL import Image, ImageFilter  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_blur_cpu_ref as B  # noqa: E402
import render_cpu_ref as R  # noqa: E402

FIXED_RADII = [0.3, 0.5, 1, 1.5, 2, 3.3, 5, 8, 12.5, 20, 40]


def _render():
    import fdet_amd  # noqa: F401
    from fdet_amd import render
    return render


def _pil(region, radius):
    return np.asarray(Image.fromarray(region).filter(ImageFilter.GaussianBlur(float(np.float32(radius)))))


def _content(g, h, w, kind):
    if kind == 0:
        return g.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 1:
        return np.broadcast_to(g.integers(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 7 + yy * 3) % 256, (xx * xx + yy) % 256, (255 - xx - 2 * yy) % 256], -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _cases():
    g = np.random.default_rng(2023)
    cases = []
    for k in range(1000):
        h, w = (int(v) for v in g.integers(1, 70, 2))
        radius = float(np.float32(np.exp(g.uniform(np.log(0.1), np.log(50.0)))))
        cases.append((_content(g, h, w, k % 3), radius))
    for radius in FIXED_RADII:
        for h, w in ((1, 1), (1, 23), (23, 1), (2, 2), (3, 5), (17, 31), (64, 69)):      # 1xn, nx1, 1x1; 20 and 40 exceed most
            cases.append((_content(g, h, w, 0), radius))
    return tuple(cases)


def test_box_radius_box_params_and_one_pass_equal_pil_gaussian_blur():
    cases = _cases()
    assert len(cases) >= 1000 and any(r > max(a.shape[:2]) for a, r in cases)
    for a, radius in cases:
        r, ww, fw = B.box_params(B.box_radius(radius))
        assert B.validate([[r, ww, fw]])
        got = B.gaussian(a, r, ww, fw)
        want = _pil(a, radius)
        assert np.array_equal(got, want), (a.shape, radius, (r, ww, fw), int((got != want).sum()))


def test_blur_table_equals_the_scalar_restatement():
    render = _render()
    for blocks in (1, 3, 8, 64):
        assert np.array_equal(render.blur_table(blocks, None, 300), B.table(blocks, None, 300)), blocks
    for radius in FIXED_RADII + [0.0, 0.1, 50.0]:
        assert np.array_equal(render.blur_table(8, radius, 5), B.table(8, radius, 5)), radius
    tab = render.blur_table(8, None, 300)
    assert tab.dtype == np.int32 and tab.shape == (300, 3) and render.blur_table(8, None, 300) is tab      # cached
    assert tab[0].tolist() == [0, 1 << 24, 0]                                      # radius 0: the identity
    with pytest.raises(ValueError):
        render.blur_table(0)
    with pytest.raises(ValueError):
        render.blur_table(8, -1.0, 4)


def test_every_table_entry_satisfies_the_bound_and_a_violation_is_refused():
    render = _render()
    for blocks in range(1, 65):
        tab = render.blur_table(blocks, None, 8193)
        assert B.validate(tab), blocks
        render.check_blur_table(tab)
    for bad in ([[0, (1 << 24) + 1, 0]], [[1, 1 << 23, 0]], [[-1, 5, 5]], [[2, -1, 0]], [[2, 1, -1]], [[0, 1 << 24, 1]],
                [[1 << 30, 1 << 10, 0]]):
        assert not B.validate(bad)
        with pytest.raises(ValueError):
            render.check_blur_table(np.asarray(bad, np.int32))
    render.check_blur_table(np.asarray([[0, 1 << 24, 0], [1 << 30, 0, 1 << 23]], np.int32))     # on the bound


def _boxes(g, H, W, integer):
    n = int(g.integers(1, 4))
    b = np.zeros((n + 1, 5), np.float32)
    for k in range(n):
        x, y = g.uniform(-10, W + 4), g.uniform(-10, H + 4)
        w, h = g.uniform(1, W + 12), g.uniform(1, H + 12)
        b[k, 1:] = np.round([x, y, w, h]) if integer else [x, y, w, h]
    b[:, 0] = 0.9
    b[n, 1:] = [3, 3, 0.5, 9]                                      # skipped by step 2
    order = g.permutation(n + 1)
    return b[order]


def test_the_whole_rule_equals_pil_crop_filter_paste():
    g = np.random.default_rng(77)
    blurred = overlapped = 0
    for case in range(120):
        H, W = (int(v) for v in g.integers(1, 60, 2))
        src = _content(g, H, W, case % 3 if case % 3 != 1 else 0)
        rows = _boxes(g, H, W, integer=case % 2 == 0)
        blocks = int(g.integers(1, 12))
        fixed = None if case % 4 else float(np.float32(g.uniform(0.2, 9)))
        tab = B.table(blocks, fixed, 2 * max(H, W) + 2 if case % 5 else 7)          # a short table: the clamp beyond n
        got = B.render_one(src, rows, len(rows), tab)
        im = Image.fromarray(src)
        want = im.copy()
        rects = [R.box_rect(r) for r in rows]
        assert sum(r is None for r in rects) == 1
        cover = np.zeros((H, W), int)
        for rect in reversed([r for r in rects if r is not None]):                 # descending row index, each from the original
            x0, y0, x1, y1 = rect[:4]
            cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
            if cx0 > cx1 or cy0 > cy1:
                continue
            S = min(max(x1 - x0 + 1, y1 - y0 + 1), len(tab) - 1)
            radius = float(np.float32(S) / np.float32(blocks)) if fixed is None else fixed
            want.paste(im.crop((cx0, cy0, cx1 + 1, cy1 + 1)).filter(ImageFilter.GaussianBlur(radius)), (cx0, cy0))
            cover[cy0:cy1 + 1, cx0:cx1 + 1] += 1
            blurred += 1
        overlapped += int((cover > 1).any())
        assert np.array_equal(got, np.asarray(want)), (case, H, W, rows.tolist(), blocks, fixed)
    assert blurred >= 150 and overlapped >= 20                     # the cases did blur, and did decide ownership


def test_a_constant_region_stays_constant():
    for radius in FIXED_RADII:
        r, ww, fw = B.box_params(B.box_radius(radius))
        for value in (0, 1, 127, 254, 255):
            a = np.full((9, 14, 3), value, np.uint8)
            assert np.array_equal(B.gaussian(a, r, ww, fw), a), (radius, value)


def test_an_impulse_spreads_to_exactly_the_closed_forms_taps():
    """One pass reaches r + 1 pixels to either side, three passes 3 (r + 1): 2 * 3 * (r + 1) + 1 taps per axis."""
    for radius in (0.5, 1, 2, 3.3, 5, 8):
        r, ww, fw = B.box_params(B.box_radius(radius))
        assert fw > 0
        reach = 3 * (r + 1)
        side = 2 * reach + 9
        a = np.zeros((side, side, 3), np.uint8)
        a[side // 2, side // 2] = 255
        # the support of the weights, in exact integers: the impulse response without the uint8 roundings in between
        k1 = np.array([fw] + [ww] * (2 * r + 1) + [fw], dtype=np.int64)
        k3 = np.convolve(np.convolve(k1 > 0, k1 > 0), k1 > 0)         # the support of three passes
        assert len(k3) == 2 * reach + 1 and (k3 > 0).all()
        got = B.gaussian(a, r, ww, fw)[..., 0]
        ys, xs = np.nonzero(got)
        if len(ys):                                                 # the roundings can only shrink the support, never widen it
            assert xs.min() >= side // 2 - reach and xs.max() <= side // 2 + reach
            assert ys.min() >= side // 2 - reach and ys.max() <= side // 2 + reach
        # along one axis, before any rounding to zero: a single pass has exactly 2 (r + 1) + 1 non-zero taps
        line = np.zeros((1, side), np.uint8)
        line[0, side // 2] = 255
        one = B.one_pass(line, r, ww, fw)[0]
        want = (np.pad(k1 * 255, (side // 2 - r - 1, side // 2 - r - 1)) + (1 << 23)) >> 24
        assert np.array_equal(one, want.astype(np.uint8))
        assert np.array_equal(got, np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius)))[..., 0])


def test_arguments():
    from fdet_amd import detect_images
    with pytest.raises(SystemExit):
        detect_images.main(["--images", "x", "--out", "y", "--draw", "d", "--blur-radius", "2"])
    with pytest.raises(SystemExit):
        detect_images.main(["--images", "x", "--out", "y", "--draw", "d", "--anonymize", "pixelate", "--blur-radius", "2"])
    with pytest.raises(SystemExit):
        detect_images.main(["--images", "x", "--out", "y", "--anonymize", "blur"])
