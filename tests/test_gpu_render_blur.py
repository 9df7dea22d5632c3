"""fdet_render_boxes_blur / render_detections(anonymize="blur") on the GPU against the numpy restatement
(tests/render_blur_cpu_ref.py, which tests/test_render_blur_host.py holds against Pillow).  No tolerance anywhere: every
comparison is equality of bytes."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_blur_cpu_ref as B  # noqa: E402
import render_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 8192              # BL_CAP = FDET_BLUR_MAX_LINE (csrc/fdet_render.hip): the LDS bytes a chunk of lines fills, the longest line
SPLIT = 16              # BL_SPLIT: workgroups per box; a box of more chunks makes a workgroup walk several
THREADS = 256           # BL_THREADS
NAN = float("nan")
K = 16


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, render
    from fdet_amd.datasets import augment as A
    return A, render, hotpath


def _dev(rows, counts):
    return torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()


def _pack(boxes_per_image, k=K):
    """lists of [x,y,w,h] -> rows (n,k,5) with NaN / huge rows past the counts, counts (n,)."""
    n = len(boxes_per_image)
    rows = np.full((n, k, 5), NAN, np.float32)
    rows[:, 1::2] = 3.0e38                                                 # what lies past the counts must never be read
    counts = np.zeros(n, np.int32)
    for i, b in enumerate(boxes_per_image):
        assert len(b) <= k
        if len(b):
            rows[i, :len(b), 0] = 1.0 - 0.01 * np.arange(len(b))
            rows[i, :len(b), 1:] = np.asarray(b, np.float32)
        counts[i] = len(b)
    return rows, counts


def _empty_like(A, src):
    n = len(src)
    table = np.zeros(n, dtype=A.IMAGE_DTYPE)
    sizes = src.table["h"].astype(np.int64) * src.table["w"] * 3
    table["offset"][1:] = np.cumsum(sizes)[:-1]
    table["h"], table["w"] = src.table["h"], src.table["w"]
    return A.DeviceImageBank(torch.full((int(sizes.sum()),), 0xA5, dtype=torch.uint8, device="cuda"), table)


def _raw(images, rows, counts, tab, outline=False, lead=0):
    """The C entry through hotpath.render_boxes_blur with a table of the test's own."""
    A, _, hp = _mods()
    bank = A.DeviceImageBank.from_arrays(list(images), "cuda", lead_bytes=lead)
    out = _empty_like(A, bank)
    d_rows, d_counts = _dev(rows, counts)
    tab = np.ascontiguousarray(tab, np.int32)
    rej = hp.render_boxes_blur(bank, d_rows, d_counts, np.ascontiguousarray(counts, np.int32), out, torch.from_numpy(tab).cuda(), tab,
                               outline=outline)
    assert int(rej.item()) == 0
    return out.to_arrays()


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (i, g.shape, int((g != w).any(2).sum()))


# ------------------------------------------------------------------------------------------------------------ geometry
SIZES = [(1, 1), (1, 7), (7, 1), (37, 53), (5, 7)]                         # (H, W); the last image carries counts = 0


@functools.lru_cache(maxsize=None)
def _images():
    g = np.random.default_rng(23)
    return tuple(g.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES)


def _box_set(H, W):
    return [[4, 3, 1, 1], [9, 11, 2, 1.5], [20, 5, 1.5, 0.99],            # S = 2, S = 3, w or h < 1: skipped
            [-0.5, 2, 1.25, 6], [NAN, 3, 4, 5], [3, 3, 4, float("inf")],   # x1 == x0 (the only way to S = 1): skipped; NaN; inf
            [8, 8, 25, 25], [15, 12, 30, 20], [12, 18, 18, 30],            # three mutually overlapping boxes
            [-6, H // 3, 12, 9], [W - 4, -3, 12.5, 10.25],                 # across borders, float corners
            [0, 0, W - 1, H - 1] if W > 1 and H > 1 else [0, 0, W, H],     # exactly the whole image (where it has two pixels a side)
            ] + [[-3, -2, W + 7, H + 5]]                                   # larger than the image on every side, lowest priority


@functools.lru_cache(maxsize=None)
def _rows_counts():
    return _pack([_box_set(h, w) for h, w in SIZES[:-1]] + [[]], k=K + 3)


@functools.lru_cache(maxsize=None)
def _bank():
    A, _, _ = _mods()
    return A.DeviceImageBank.from_arrays(list(_images()), "cuda", lead_bytes=5)


@functools.lru_cache(maxsize=None)
def _want(outline, blocks, radius):
    rows, counts = _rows_counts()
    n_tab = 2 * max(max(s) for s in SIZES) + 2
    return tuple(B.render(_images(), rows, counts, B.table(blocks, radius, n_tab), outline))


@pytest.mark.parametrize("outline", [False, True])
@pytest.mark.parametrize("blocks,radius", [(8, None), (1, None), (3, None), (8, 2.0), (8, 60.0)])
def test_blur_equals_the_restatement(blocks, radius, outline):
    """1x1, 1x7, 7x1 and 37x53 images at odd byte offsets; blocks = 1 and radius 60 put r above the region's sides."""
    _, render, _ = _mods()
    bank = _bank()
    assert int(bank.table["offset"][0]) == 5
    before = bank.data.clone()
    rows, counts = _dev(*_rows_counts())
    out = render.render_detections(bank, rows, counts, outline=outline, anonymize="blur", blocks=blocks, blur_radius=radius)
    got = out.to_arrays()
    _same(got, _want(outline, blocks, radius))
    assert torch.equal(bank.data, before)                                  # the source is never written
    assert any(not np.array_equal(g, s) for g, s in zip(got, _images()))
    assert np.array_equal(got[-1], _images()[-1])                          # counts = 0
    again = render.render_detections(bank, rows, counts, outline=outline, anonymize="blur", blocks=blocks, blur_radius=radius)
    assert torch.equal(again.data, out.data)                               # two calls, equal bytes


def test_tables_of_the_tests_own():
    """r = 0 with and without side taps, r far above the region with ww = 0 (the bound's corner), and a table shorter than S."""
    imgs = [_images()[3]]
    rows, counts = _pack([[[2, 3, 30, 20], [20, 10, 40, 40], [-4, -4, 70, 70]]])
    for tab in ([[0, 1 << 24, 0]],                                         # the identity
                [B.box_params(np.float32(0.4))],                           # r = 0, side taps only
                [[1 << 30, 0, 1 << 23]],                                   # every pixel the mean of its line's two ends
                [[100, (1 << 24) // 201, ((1 << 24) - 201 * ((1 << 24) // 201)) // 2]],      # r >= both sides of the image
                B.table(2, None, 9)):                                      # S = 21, 41, 71 all clamp to entry 8
        assert B.validate(tab)
        _same(_raw(imgs, rows, counts, tab, lead=3), B.render(imgs, rows, counts, np.asarray(tab)))
    assert np.array_equal(_raw(imgs, rows, counts, [[0, 1 << 24, 0]])[0], imgs[0])


def test_an_impulse_and_a_constant_region():
    imp = np.zeros((41, 45, 3), np.uint8)
    imp[20, 22] = (255, 200, 90)
    const = np.random.default_rng(5).integers(0, 256, (30, 33, 3)).astype(np.uint8)
    const[4:25, 6:29] = (17, 255, 1)
    rows, counts = _pack([[[0, 0, 44, 40]], [[6, 4, 22, 20]]])
    tab = B.table(8, 2.0, 4)
    got = _raw([imp, const], rows, counts, tab)
    _same(got, B.render([imp, const], rows, counts, tab))
    r = int(tab[0][0])
    ys, xs = np.nonzero(got[0].any(2))
    assert len(ys) > 1 and abs(ys - 20).max() <= 3 * (r + 1) and abs(xs - 22).max() <= 3 * (r + 1)
    assert np.array_equal(got[1], const)                                   # a constant region stays constant


# ---------------------------------------------------------------------------------------------------------- long lines
def _smooth(h, w, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (h, w, 3)).astype(np.uint8)


# a line fills 1/3, 1/2 or all of a chunk: 3+, 2 or 1 lines per chunk; the last is the longest line the entry takes
@pytest.mark.parametrize("hw,box,radius", [
    ((7, 720), [10, 1, 699, 4], 6.0),                                      # a 5 x 700 box
    ((720, 7), [1, 10, 4, 699], 6.0),                                      # a 700 x 5 box
    ((300, 310), [3, 4, 299.5, 289], None),                                # 3 * 290 lines of 300: more chunks than SPLIT, each of several lines
    ((3, CAP // 3 + 5), [-2, -2, CAP, 9], 3.3),                            # rows of 2 lines per chunk; columns of 3
    ((CAP // 3 + 5, 2), [-2, -2, 9, CAP], 3.3),
    ((2, CAP // 2 + 3), [0, 0, CAP, 2], 9.0),                              # rows of 1 line per chunk
    ((CAP // 2 + 3, 2), [0, 0, 2, CAP], 9.0),
    ((1, CAP), [-1, -1, CAP + 2, 3], 1.5),                                 # the longest line: every thread scans 32 bytes
    ((CAP, 1), [-1, -1, 3, CAP + 2], 1.5),
])
def test_lines_longer_than_a_chunk_share_and_boxes_of_many_chunks(hw, box, radius):
    img = _smooth(hw[0], hw[1], hw[0] * 7 + hw[1])
    rows, counts = _pack([[box]])
    if hw == (300, 310):
        rect = R.box_rect(rows[0, 0])
        lines, n = 3 * (min(rect[3], hw[0] - 1) - max(rect[1], 0) + 1), min(rect[2], hw[1] - 1) - max(rect[0], 0) + 1
        assert -(-lines // (CAP // n)) > SPLIT and CAP // n >= 3 and lines * n > THREADS * 32
    tab = B.table(8, radius, 2 * max(hw) + 2 if radius is None else 4)      # a fixed radius: every entry is the same
    _same(_raw([img], rows, counts, tab, outline=hw[0] == 300), B.render([img], rows, counts, tab, outline=hw[0] == 300))


# --------------------------------------------------------------------------------------------------------------- calls
def test_counts_all_zero_k_zero_indices_and_a_fixed_radius():
    _, render, _ = _mods()
    bank = _bank()
    rows, counts = _rows_counts()
    d_rows, _ = _dev(rows, counts)
    zero = torch.zeros(len(SIZES), dtype=torch.int32, device="cuda")
    _same(render.render_detections(bank, d_rows, zero, outline=True, anonymize="blur").to_arrays(), _images())
    none = torch.zeros(len(SIZES), 0, 5, dtype=torch.float32, device="cuda")
    _same(render.render_detections(bank, none, zero, anonymize="blur").to_arrays(), _images())
    idx = [3, 1, 3, 0]                                                     # a permuted subset, one image twice
    out = render.render_detections(bank, *_dev(rows[idx], counts[idx]), indices=idx, outline=True, anonymize="blur", blocks=3,
                                   color=(250, 3, 77))
    want = B.render([_images()[i] for i in idx], rows[idx], counts[idx], B.table(3, None, 2 * 53 + 2), True, (250, 3, 77))
    assert out.sizes.tolist() == [list(SIZES[i]) for i in idx]
    _same(out.to_arrays(), want)
    with pytest.raises(ValueError):
        render.render_detections(bank, d_rows, zero, anonymize="pixelate", blur_radius=2.0)
    with pytest.raises(ValueError):
        render.render_detections(bank, d_rows, zero, anonymize="gauss")


# ------------------------------------------------------------------------------------------------------------ contract
def _call(lib, ptr, stream, bank, d_rows, d_cnt, h_counts, k, dst, table, outline=1, pixelate=0, blur=1, blocks=8, tab=None, h_tab=None,
          n_tab=None, ws=None, ws_bytes=None, rej=None):
    U8, I32 = torch.uint8, torch.int32
    d_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    h_counts = np.ascontiguousarray(h_counts)
    return lib().fdet_render_boxes_blur(ptr(bank.data, U8), ptr(bank.d_table, U8), bank.table.ctypes.data, ptr(d_rows), ptr(d_cnt, I32),
                                        h_counts.ctypes.data, len(bank), k, ptr(dst, U8), ptr(d_table, U8), table.ctypes.data, outline,
                                        pixelate, blur, blocks, None if tab is None else ptr(tab, I32),
                                        None if h_tab is None else h_tab.ctypes.data, 0 if h_tab is None else (len(h_tab) if n_tab is None else n_tab),
                                        0, 0, 255, ptr(ws, U8), int(ws.numel()) if ws_bytes is None else ws_bytes,
                                        None if rej is None else ptr(rej, torch.int64), stream())


def test_blur_off_equals_fdet_render_boxes_and_bad_calls_write_nothing():
    A, render, hp = _mods()
    from fdet_amd._native import lib, ptr, stream
    bank = _bank()
    n = len(bank)
    rows, counts = _rows_counts()
    kk = rows.shape[1]
    d_rows, d_counts = _dev(rows, counts)
    total = bank.nbytes
    proto = _empty_like(A, bank)
    t_dst = proto.table
    dst = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    h_tab = np.ascontiguousarray(render.blur_table(8, None, 120))
    tab = torch.from_numpy(h_tab.copy()).cuda()
    need = hp.render_blur_ws_bytes(bank.table, rows, counts)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rej = torch.zeros(1, dtype=torch.int64, device="cuda")
    before = bank.data.clone()

    def call(**kw):
        a = dict(bank=bank, d_rows=d_rows, d_cnt=d_counts, h_counts=counts, k=kk, dst=dst, table=t_dst, tab=tab, h_tab=h_tab, ws=ws, rej=rej)
        a.update(kw)
        return _call(lib, ptr, stream, **a)

    wrong = t_dst.copy()
    wrong["h"][2] += 1
    over = counts.copy()
    over[3] = kk + 1
    bad_tab = h_tab.copy()
    bad_tab[7] = [3, 1 << 22, 0]                                           # 7 * 2^22 > 2^24
    neg_tab = h_tab.copy()
    neg_tab[0, 2] = -1
    assert call(dst=bank.data[3:]) == -1                                   # the destination inside the source
    assert call(table=wrong) == -1
    assert call(blocks=0) == -1
    assert call(h_counts=over, d_cnt=torch.from_numpy(over).cuda()) == -1
    assert call(k=-1) == -1
    assert call(pixelate=1) == -1                                          # blur with pixelate
    assert call(blur=2) == -1
    assert call(h_tab=bad_tab) == -1 and call(h_tab=neg_tab) == -1
    assert call(n_tab=0) == -1
    assert call(tab=None) == -1 and call(rej=None) == -1
    assert call(ws_bytes=4 * (n + 1) + 8 * int(counts.sum()) - 1) == -1    # not even the offsets fit
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and torch.equal(bank.data, before) and int(rej.item()) == 0
    with pytest.raises(ValueError):
        hp.render_blur_ws_bytes(bank.table, rows, over)
    # an image beyond the longest line is refused whole
    long_bank = A.DeviceImageBank.from_arrays([np.zeros((1, CAP + 1, 3), np.uint8)], "cuda")
    long_dst = _empty_like(A, long_bank)
    r1, c1 = _pack([[[0, 0, 5, 5]]])
    assert _call(lib, ptr, stream, long_bank, *_dev(r1, c1), c1, r1.shape[1], long_dst.data, long_dst.table, tab=tab, h_tab=h_tab, ws=ws,
                 rej=rej) == -1
    torch.cuda.synchronize()
    assert bool((long_dst.data == 0xA5).all())
    # blur = 0: fdet_render_boxes's bytes, table and counter not needed
    for outline, pixelate in ((1, 0), (0, 1), (1, 1), (0, 0)):
        dst.fill_(0xA5)
        assert call(blur=0, outline=outline, pixelate=pixelate, tab=None, h_tab=None, rej=None, ws_bytes=4 * (n + 1)) == 0
        torch.cuda.synchronize()
        got = A.DeviceImageBank(dst, t_dst).to_arrays()
        _same(got, R.render(_images(), rows, counts, bool(outline), bool(pixelate), 8))
        ref = render.render_detections(bank, d_rows, d_counts, outline=bool(outline), anonymize="pixelate" if pixelate else None)
        assert torch.equal(ref.data, dst[:total]) and bool((dst[total:] == 0xA5).all())
    # and the same call with nothing wrong blurs
    dst.fill_(0xA5)
    assert call() == 0
    torch.cuda.synchronize()
    _same(A.DeviceImageBank(dst, t_dst).to_arrays(), B.render(_images(), rows, counts, h_tab, True))
    assert bool((dst[total:] == 0xA5).all()) and int(rej.item()) == 0 and torch.equal(bank.data, before)


def test_a_workspace_one_box_too_small_rejects_that_box_and_raises():
    """Valid arguments, but the workspace ends one byte before the last box's share: the device's own size check leaves that box
    as the copy and counts it; nothing is written past the workspace; render_detections raises."""
    A, render, hp = _mods()
    from fdet_amd import FdetError
    img = _images()[3]
    boxes = [[2, 3, 20, 15], [30, 5, 15, 25], [10, 20, 30, 12]]
    rows, counts = _pack([boxes])
    bank = A.DeviceImageBank.from_arrays([img], "cuda")
    need = hp.render_blur_ws_bytes(bank.table, rows, counts)
    last = R.box_rect(rows[0, 2])
    assert need == 8 + 8 * 3 + 3 * sum((r[2] - r[0] + 1) * (r[3] - r[1] + 1) for r in (R.box_rect(b) for b in rows[0, :3]))
    d_rows, d_counts = _dev(rows, counts)
    h_tab = np.ascontiguousarray(render.blur_table(8, None, 120))
    tab = torch.from_numpy(h_tab.copy()).cuda()
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    out = _empty_like(A, bank)
    rej = hp.render_boxes_blur(bank, d_rows, d_counts, counts, out, tab, h_tab, ws=big[:need - 1])
    assert int(rej.item()) == 1
    assert bool((big[need - 1:] == 0xA5).all())
    rows2, counts2 = _pack([boxes[:2]])
    want = B.render([img], rows2, counts2, h_tab)[0]                       # the first two boxes blurred, the third left as the copy
    assert np.array_equal(out.to_arrays()[0], want) and last is not None
    with pytest.raises(FdetError):
        render.render_detections(bank, d_rows, d_counts, anonymize="blur", ws=big[:need - 1])
    ok = render.render_detections(bank, d_rows, d_counts, outline=False, anonymize="blur", ws=big[:need])
    assert np.array_equal(ok.to_arrays()[0], B.render([img], rows, counts, h_tab)[0])
    assert bool((big[need:] == 0xA5).all())


# ---------------------------------------------------------------------------------------------------------- end to end
def test_detect_images_and_track_frames_anonymize_blur(golden, tmp_path, monkeypatch):
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images, track_frames
    from fdet_amd.models.PoolResnet import PoolResnet
    monkeypatch.chdir(tmp_path)
    g = golden("g6_trained_small")
    model = PoolResnet(filters=32, input_shape=(3, 480, 480), num_of_patches=10)
    model.load_state_dict({k[len("param/"):]: v.clone() for k, v in g.items() if k.startswith("param/")})
    torch.save(model.state_dict(), tmp_path / "small.pth")
    frames = g["images"].numpy().transpose(0, 2, 3, 1)                     # (3,480,480,3)
    sources = {"a.png": frames[0], "b.png": frames[1]}
    for name, arr in sources.items():
        (tmp_path / "in").mkdir(exist_ok=True)
        Image.fromarray(arr).save(tmp_path / "in" / name)
    model_args = ["--model", "poolresnet", "--filters", "32", "--checkpoint", str(tmp_path / "small.pth"), "--probability-threshold", "0.3",
                  "--iou-threshold", "0.3"]
    base = model_args + ["--images", str(tmp_path / "in"), "--out", str(tmp_path / "res.txt"), "--tile", "--draw-format", "png"]
    for extra, blocks, radius, outline in ((["--anonymize", "blur", "--no-outline"], 8, None, False),
                                           (["--anonymize", "blur", "--blur-radius", "3.5", "--blocks", "4"], 4, 3.5, True)):
        out = detect_images.main(base + ["--draw", str(tmp_path / "drawn")] + extra)
        rows, counts = out["rows"].numpy(), out["counts"].numpy()
        assert int(counts.sum()) >= 2
        tab = B.table(blocks, radius, 2 * 480 + 2 if radius is None else 4)
        for i, name in enumerate(out["names"]):
            got = np.asarray(Image.open(tmp_path / "drawn" / name).convert("RGB"))
            assert np.array_equal(got, B.render_one(sources[name], rows[i], counts[i], tab, outline)), (name, extra)
            assert not np.array_equal(got, sources[name])
    track_frames.main(model_args + ["--frames", str(tmp_path / "in"), "--out", str(tmp_path / "tracks.txt"), "--min-hits", "1",
                                    "--draw", str(tmp_path / "seq"), "--anonymize", "blur", "--no-outline"])
    assert sorted(os.listdir(tmp_path / "seq")) == ["a.png", "b.png"]
    assert any(not np.array_equal(np.asarray(Image.open(tmp_path / "seq" / n).convert("RGB")), sources[n]) for n in sources)
    with pytest.raises(SystemExit):
        track_frames.main(model_args + ["--frames", str(tmp_path / "in"), "--out", str(tmp_path / "t.txt"), "--draw", "d", "--blur-radius", "2"])
