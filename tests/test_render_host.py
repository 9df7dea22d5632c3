"""Rendering detections, the parts that need no GPU: the numpy restatement of the rules
(tests/render_cpu_ref.py) against PIL's own ImageDraw, the properties of the pixelation, and the library / script surface.
Every comparison is equality of bytes."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cpu_ref as R  # noqa: E402

BLUE = (0, 0, 255)


def _pil_outline(img, rows):
    """PIL drawn directly, as the reference's draw_bbx does (datasets/utils.py:194-203)."""
    im = Image.fromarray(img.copy())
    d = ImageDraw.Draw(im)
    for r in rows:
        x, y, w, h = (float(v) for v in r[1:5])
        d.rectangle((x, y, x + w, y + h), outline=BLUE, width=1 if (w <= 15 or h <= 15) else 3)
    return np.asarray(im)


def _random_case(g, floats):
    H, W = int(g.integers(1, 41)), int(g.integers(1, 41))
    img = g.integers(0, 256, (H, W, 3)).astype(np.uint8)
    rows = []
    for _ in range(int(g.integers(1, 4))):
        if floats:
            x, y, w, h = g.uniform(-10, W + 5), g.uniform(-10, H + 5), g.uniform(1, 30), g.uniform(1, 30)
        else:
            x, y, w, h = g.integers(-10, W + 6), g.integers(-10, H + 6), g.integers(1, 31), g.integers(1, 31)
        rows.append([g.uniform(0, 1), x, y, w, h])
    return img, np.asarray(rows, np.float32)


# ------------------------------------------------------------------------------------------------ outline against PIL
@pytest.mark.parametrize("floats", [False, True])
def test_outline_equals_pil_on_random_boxes(floats):
    """1500 seeded cases each of integer and of float boxes: images 1x1..40x40, 1-3 boxes, origins from -10 to beyond the
    image, w and h in [1, 30].  Boxes the renderer skips (rule 2) are left out of what PIL draws; with w, h >= 1 those are
    the boxes truncation folds onto a single pixel row or column (a start in (-1, 0), an end in [0, 1)), which PIL paints by
    another rule; the second test below confirms they are skipped."""
    g = np.random.default_rng(20 + int(floats))
    drawn = 0
    for _ in range(1500):
        img, rows = _random_case(g, floats)
        kept = np.asarray([r for r in rows if R.box_rect(r) is not None], np.float32).reshape(-1, 5)
        drawn += len(kept)
        got = R.render_one(img, rows, len(rows), outline=True, pixelate_=False, color=BLUE)
        assert np.array_equal(got, _pil_outline(img, kept)), (img.shape, rows)
    assert drawn >= 2500


def test_boxes_below_one_pixel_and_degenerate_rectangles_are_skipped():
    g = np.random.default_rng(5)
    img = g.integers(0, 256, (20, 24, 3)).astype(np.uint8)
    skipped = [[1, 3, 3, 0.99, 10], [1, 3, 3, 10, 0.5], [1, 3, 3, 0, 0], [1, 3, 3, -4, 5], [1, np.nan, 3, 4, 5], [1, 3, np.inf, 4, 5],
               [1, 3, 3, np.inf, 5], [1, 3, 3, 4, np.nan], [1, 2e7, 3, 4, 5], [1, 3, -2e7, 4, 5], [1, 3, 3, 3e7, 5],
               [1, -0.5, 3, 1.2, 6], [1, 4, -0.9, 6, 1.5]]                           # the last two: x1 == x0, y1 == y0
    for row in skipped:
        assert R.box_rect(np.asarray(row, np.float32)) is None, row
    rows = np.asarray(skipped, np.float32)
    for pix in (False, True):
        assert np.array_equal(R.render_one(img, rows, len(rows), outline=True, pixelate_=pix, blocks=3), img)
    # one box drawn between them, and a count that stops before it
    rows2 = np.concatenate([rows[:4], np.asarray([[1, 2, 2, 8, 8]], np.float32), rows[4:]])
    assert not np.array_equal(R.render_one(img, rows2, len(rows2)), img)
    assert np.array_equal(R.render_one(img, rows2, 4), img)
    assert np.array_equal(R.render_one(img, rows2, len(rows2)), _pil_outline(img, rows2[4:5]))


def test_thickness_switches_above_fifteen():
    img = np.zeros((40, 33, 3), np.uint8)
    for w, t in ((15, 1), (15.5, 3), (16, 3)):
        out = R.render_one(img, np.asarray([[1, 4, 5, w, 20]], np.float32), 1)
        assert np.array_equal(out, _pil_outline(img, np.asarray([[1, 4, 5, w, 20]], np.float32)))
        assert int((out[15, :, 2] > 0).sum()) == 2 * t


# ------------------------------------------------------------------------------------------------ pixelate properties
def _boxes(g, H, W, k):
    return np.asarray([[1, g.uniform(-8, W), g.uniform(-8, H), g.uniform(1, 30), g.uniform(1, 30)] for _ in range(k)], np.float32)


def test_pixelate_leaves_a_constant_image_and_the_outside_unchanged():
    g = np.random.default_rng(1)
    for _ in range(40):
        H, W = int(g.integers(1, 41)), int(g.integers(1, 41))
        rows = _boxes(g, H, W, 3)
        blocks = int(g.integers(1, 10))
        flat = np.full((H, W, 3), g.integers(0, 256, 3), np.uint8)
        assert np.array_equal(R.render_one(flat, rows, 3, outline=False, pixelate_=True, blocks=blocks), flat)
        img = g.integers(0, 256, (H, W, 3)).astype(np.uint8)
        out = R.render_one(img, rows, 3, outline=False, pixelate_=True, blocks=blocks)
        yy, xx = np.mgrid[0:H, 0:W]
        inside = np.zeros((H, W), bool)
        for r in rows:
            q = R.box_rect(r)
            if q is not None:
                inside |= (xx >= q[0]) & (xx <= q[2]) & (yy >= q[1]) & (yy <= q[3])
        assert np.array_equal(out[~inside], img[~inside])


def test_reversing_the_boxes_changes_only_pixels_covered_twice():
    g = np.random.default_rng(2)
    changed = 0
    for _ in range(60):
        H, W = int(g.integers(8, 41)), int(g.integers(8, 41))
        img = g.integers(0, 256, (H, W, 3)).astype(np.uint8)
        rows = _boxes(g, H, W, 3)
        a = R.render_one(img, rows, 3, outline=False, pixelate_=True, blocks=3)
        b = R.render_one(img, rows[::-1].copy(), 3, outline=False, pixelate_=True, blocks=3)
        yy, xx = np.mgrid[0:H, 0:W]
        cover = np.zeros((H, W), int)
        for r in rows:
            q = R.box_rect(r)
            if q is not None:
                cover += (xx >= q[0]) & (xx <= q[2]) & (yy >= q[1]) & (yy <= q[3])
        diff = (a != b).any(2)
        assert not (diff & (cover < 2)).any()
        changed += int(diff.sum())
    assert changed > 0                                     # the priority rule is exercised


def test_pixelate_hand_computed_4x4():
    """Box (x, y, w, h) = (0, 0, 3, 3) -> pixels 0..3 x 0..3, blocks = 2 -> cell = 2: four 2x2 cells.  Channel 0 holds
    0..15 row-major: the cells sum to 10, 18, 42, 50 -> (s + 2) // 4 = 3, 5, 11, 13.  Channel 1 is 255 everywhere (stays),
    channel 2 holds 1 at (0, 0) and (0, 1) only: (2 + 2) // 4 = 1 in the first cell (round half up), 0 elsewhere."""
    img = np.zeros((4, 4, 3), np.uint8)
    img[:, :, 0] = np.arange(16).reshape(4, 4)
    img[:, :, 1] = 255
    img[0, 0, 2] = img[0, 1, 2] = 1
    out = R.render_one(img, np.asarray([[1, 0, 0, 3, 3]], np.float32), 1, outline=False, pixelate_=True, blocks=2)
    want = np.zeros((4, 4, 3), np.uint8)
    want[:, :, 0] = np.kron(np.array([[3, 5], [11, 13]]), np.ones((2, 2), int))
    want[:, :, 1] = 255
    want[:2, :2, 2] = 1
    assert np.array_equal(out, want)
    # a second box over the right half takes nothing from the first; its own mean comes from the SOURCE pixels
    rows = np.asarray([[1, 0, 0, 3, 3], [1, 2, 0, 1.5, 3.5]], np.float32)      # second: pixels 2..3 x 0..3, cell 2
    assert np.array_equal(R.render_one(img, rows, 2, outline=False, pixelate_=True, blocks=2), want)
    rev = R.render_one(img, rows[::-1].copy(), 2, outline=False, pixelate_=True, blocks=2)
    assert np.array_equal(rev, want)                       # the two boxes' cells coincide there, so even the order agrees
    one = R.render_one(img, rows[1:], 1, outline=False, pixelate_=True, blocks=1)       # cell 4: one cell of 2 x 4 pixels
    assert one[0, 2, 0] == (2 + 3 + 6 + 7 + 10 + 11 + 14 + 15 + 4) // 8 and np.array_equal(one[:, :2], img[:, :2])


# ------------------------------------------------------------------------------------------ script and library surface
def test_detect_images_draw_options_need_draw(capsys):
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images
    base = ["--images", "nowhere", "--out", "nothing.txt"]
    for extra, flag in ((["--anonymize", "pixelate"], "--anonymize"), (["--blocks", "4"], "--blocks"),
                        (["--draw-format", "jpg"], "--draw-format"), (["--no-outline"], "--no-outline")):
        with pytest.raises(SystemExit) as e:
            detect_images.main(base + extra)
        assert e.value.code == 2
        assert f"{flag} needs --draw" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        detect_images.main(base + ["--draw", "d", "--anonymize", "blur"])
    with pytest.raises(SystemExit):
        detect_images.main(base + ["--draw", "d", "--blocks", "0"])


def _lib():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native, _native.lib()


def test_render_entry_is_exported_and_declared():
    N, L = _lib()
    assert hasattr(L, "fdet_render_boxes")
    assert "fdet_render_boxes" in N.SIGNATURES and "fdet_render_boxes" in N.header_symbols()
    from fdet_amd.render import render_detections, save_images  # noqa: F401
    from fdet_amd.datasets.augment import DeviceImageBank
    from fdet_amd.datasets.utils import draw_bbx  # noqa: F401
    assert hasattr(DeviceImageBank, "to_arrays")


def test_render_entry_validates_on_the_host_before_touching_anything():
    """Every refusal below is decided from the host copies alone, so it needs no GPU: the 'device' pointers are host
    buffers that must come back untouched."""
    N, L = _lib()
    from fdet_amd.datasets.augment import IMAGE_DTYPE
    src = np.full(4096, 7, np.uint8)
    dst = np.full(4096, 9, np.uint8)
    t_src = np.array([(5, 10, 11), (5 + 330, 3, 4)], dtype=IMAGE_DTYPE)
    t_dst = np.array([(0, 10, 11), (330, 3, 4)], dtype=IMAGE_DTYPE)
    rows = np.zeros((2, 3, 5), np.float32)
    counts = np.array([1, 3], np.int32)
    ws = np.zeros(3, np.int32)

    def call(src_p=None, t_d=t_dst, cnt=counts, K=3, outline=1, pixelate=1, blocks=8, col=(0, 0, 255), dst_p=None):
        return L.fdet_render_boxes(src.ctypes.data if src_p is None else src_p, t_src.ctypes.data, t_src.ctypes.data, rows.ctypes.data,
                                   cnt.ctypes.data, cnt.ctypes.data, 2, K, dst.ctypes.data if dst_p is None else dst_p, t_d.ctypes.data,
                                   t_d.ctypes.data, outline, pixelate, blocks, col[0], col[1], col[2], ws.ctypes.data, None)

    bad_hw = t_dst.copy()
    bad_hw["w"][1] = 5
    cases = {
        "overlap": dict(dst_p=src.ctypes.data + 100),
        "does not match": dict(t_d=bad_hw),
        "blocks": dict(blocks=0),
        "K=-1": dict(K=-1),
        "counts[1]=3": dict(K=2),
        "counts[0]=-1": dict(cnt=np.array([-1, 0], np.int32)),
        "must be 0 or 1": dict(outline=2),
        "colour": dict(col=(0, 0, 256)),
    }
    for word, kw in cases.items():
        assert call(**kw) == -1, word
        assert word.encode() in L.fdet_last_error(), (word, L.fdet_last_error())
    assert (src == 7).all() and (dst == 9).all()
    # source and destination in one buffer, back to back, do not overlap: refused only when the ranges meet
    assert call(dst_p=src.ctypes.data + 5 + 330 + 36 - 1) == -1 and b"overlap" in L.fdet_last_error()


def test_draw_bbx_on_cpu_tensors_is_pil_drawn_directly(tmp_path, monkeypatch):
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets.utils import draw_bbx
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(3, 37, 53, generator=g)
    boxes5 = torch.tensor([[0.9, 4.0, 5.0, 20.0, 18.0], [0.8, 30.5, 2.25, 12.0, 40.0], [0.7, -3.0, 20.0, 16.0, 16.0]])
    u8 = img.mul(255).byte().permute(1, 2, 0).numpy()
    want = _pil_outline(u8, boxes5.numpy())
    draw_bbx(img, boxes5, save_name="five")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "imgs" / "five.png")), want)
    draw_bbx(img, [b[1:] for b in boxes5], input_shape=(3, 37, 53), save_name="four", save_dir=str(tmp_path / "elsewhere"))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "elsewhere" / "four.png")), want)
    draw_bbx(img.mul(255).byte(), torch.empty(0).reshape(0, 5), save_name="none")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "imgs" / "none.png")), u8)
    with pytest.raises(ValueError):
        draw_bbx(img, boxes5, show=True)


def test_training_entry_points_take_a_draw_directory():
    import inspect
    import fdet_amd  # noqa: F401
    from fdet_amd import train_model, train_model_ssd, trainer
    assert inspect.signature(trainer.fit).parameters["draw_dir"].default is None
    assert train_model_ssd.parser().parse_args([]).draw_dir is None
    assert train_model_ssd.parser().parse_args(["--draw-dir", "d"]).draw_dir == "d"
    assert '"--draw-dir"' in inspect.getsource(train_model.main) and "draw_dir=args.draw_dir" in inspect.getsource(train_model.main)
