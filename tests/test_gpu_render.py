"""fdet_render_boxes / render_detections on the GPU against the numpy restatement (tests/render_cpu_ref.py)
and PIL.  No tolerance anywhere: every comparison is equality of bytes."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (33, 40), (67, 131), (96, 64), (5, 7)]          # (H, W); the last image carries counts = 0
K = 40                                                                    # larger than every count
NAN, INF, HUGE = float("nan"), float("inf"), 3.0e38


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import render
    from fdet_amd.datasets import augment as A
    return A, render


@functools.lru_cache(maxsize=None)
def _images():
    g = np.random.default_rng(11)
    return tuple(g.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES)


def _box_set(H, W):
    """[x, y, w, h] rows for one image: inside, across each border, outside, covering, the thickness switch, skipped rows,
    and mutually overlapping boxes."""
    b = [[10, 10, 20, 20],                                                 # fully inside (where the image is large enough)
         [-5, H // 3, 12, 9], [W - 6, 2, 12, 10], [W // 3, -4, 9, 11], [2, H - 5, 10, 12],      # across the four borders
         [W + 3, H + 3, 10, 10], [-30, -30, 10, 10],                       # fully outside
         [2, 3, 15, 20], [2, 3, 15.5, 20], [2, 3, 16, 20],                  # thickness 1 | 3 | 3
         [0.5, 0, 0.99, 9], [3, 3, 9, 0.5],                                 # below one pixel: skipped
         [NAN, 3, 4, 5], [3, 3, INF, 5], [3, -INF, 4, 5], [3, 3, 4, NAN], [2e7, 1, 5, 5], [1, 1, 3e7, 5],
         [-0.5, 2, 1.25, 6],                                                # x1 == x0: skipped
         [8, 8, 25, 25], [15, 12, 30, 20], [12, 18, 18, 30],                # three mutually overlapping boxes
         [20.25, 30.75, 17.5, 33.1], [40.6, 5.2, 60.3, 50.9],               # float corners, one reaching a wide cell
         [-2, -2, W + 4, H + 4]]                                            # covering the whole image, lowest priority
    return np.asarray(b, np.float32)


@functools.lru_cache(maxsize=None)
def _rows_counts():
    rows = np.full((len(SIZES), K, 5), NAN, np.float32)
    rows[:, 1::2] = HUGE                                                   # what lies past the counts must never be read
    counts = np.zeros(len(SIZES), np.int32)
    for i, (h, w) in enumerate(SIZES[:-1]):
        b = _box_set(h, w)
        rows[i, :len(b), 0] = 1.0 - 0.01 * np.arange(len(b))
        rows[i, :len(b), 1:] = b
        counts[i] = len(b)
    assert counts.max() < K and counts[-1] == 0
    return rows, counts


@functools.lru_cache(maxsize=None)
def _bank():
    A, _ = _mods()
    return A.DeviceImageBank.from_arrays(list(_images()), "cuda", lead_bytes=5)


@functools.lru_cache(maxsize=None)
def _want(outline, pixelate, blocks):
    rows, counts = _rows_counts()
    return R.render(_images(), rows, counts, outline, pixelate, blocks)


def _dev(rows, counts):
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda(), torch.from_numpy(np.ascontiguousarray(counts)).cuda()


# ------------------------------------------------------------------------------------------ equality with the restatement
@pytest.mark.parametrize("blocks", [1, 3, 8])
@pytest.mark.parametrize("outline,pixelate", [(False, False), (True, False), (False, True), (True, True)])
def test_render_equals_the_restatement(outline, pixelate, blocks):
    _, render = _mods()
    bank = _bank()
    assert int(bank.table["offset"][0]) == 5
    before = bank.data.clone()
    rows, counts = _dev(*_rows_counts())
    out = render.render_detections(bank, rows, counts, outline=outline, anonymize="pixelate" if pixelate else None, blocks=blocks)
    got = out.to_arrays()
    want = _want(outline, pixelate, blocks)
    assert out.data.data_ptr() != bank.data.data_ptr() and len(got) == len(SIZES)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (i, SIZES[i], int((g != w).any(2).sum()))
    assert torch.equal(bank.data, before)                                  # the source is never written
    if not outline and not pixelate:
        assert all(np.array_equal(g, s) for g, s in zip(got, _images()))
    else:
        assert any(not np.array_equal(g, s) for g, s in zip(got, _images()))
    assert np.array_equal(got[-1], _images()[-1])                          # counts = 0


def test_indices_a_permuted_subset_a_colour_and_save_images(tmp_path):
    from PIL import Image
    _, render = _mods()
    bank = _bank()
    rows, counts = _rows_counts()
    idx = [4, 1, 3]
    d_rows, d_counts = _dev(rows[idx], counts[idx])
    out = render.render_detections(bank, d_rows, d_counts, indices=idx, anonymize="pixelate", blocks=3, color=(250, 3, 77))
    want = R.render([_images()[i] for i in idx], rows[idx], counts[idx], True, True, 3, (250, 3, 77))
    assert len(out) == 3 and out.sizes.tolist() == [list(SIZES[i]) for i in idx]
    for g, w in zip(out.to_arrays(), want):
        assert np.array_equal(g, w)
    assert all(np.array_equal(a, b) for a, b in zip(out.to_arrays([2, 0]), [want[2], want[0]]))
    paths = [tmp_path / "x" / "a.jpg", tmp_path / "y" / "z" / "b.png", tmp_path / "c.png"]
    render.save_images(out, paths, threads=2)
    assert Image.open(paths[0]).format == "JPEG" and Image.open(paths[0]).size == (SIZES[4][1], SIZES[4][0])
    assert np.array_equal(np.asarray(Image.open(paths[1])), want[1]) and np.array_equal(np.asarray(Image.open(paths[2])), want[2])
    with pytest.raises(ValueError):
        render.save_images(out, paths[:2])


def test_more_overlapping_earlier_boxes_than_the_lds_list_holds():
    """600 boxes that all overlap on one 33x40 image: past 512 listed boxes the ownership test re-reads the rows."""
    A, render = _mods()
    g = np.random.default_rng(3)
    img = g.integers(0, 256, (33, 40, 3)).astype(np.uint8)
    n = 600
    rows = np.zeros((1, n, 5), np.float32)
    rows[0, :, 1] = g.uniform(12, 22, n)
    rows[0, :, 2] = g.uniform(10, 18, n)
    rows[0, :, 3] = g.uniform(2, 9, n)
    rows[0, :, 4] = g.uniform(2, 9, n)
    rows[0, -1, 1:] = [-3, -3, 50, 50]                                     # the last box sees every other one
    counts = np.array([n], np.int32)
    bank = A.DeviceImageBank.from_arrays([img], "cuda")
    out = render.render_detections(bank, *_dev(rows, counts), outline=False, anonymize="pixelate", blocks=3)
    want = R.render([img], rows, counts, False, True, 3)[0]
    assert np.array_equal(out.to_arrays()[0], want)


def test_to_arrays_inverts_from_arrays():
    A, _ = _mods()
    imgs = list(_images())
    for lead in (0, 5):
        bank = A.DeviceImageBank.from_arrays(imgs, "cuda", lead_bytes=lead)
        back = bank.to_arrays()
        assert len(back) == len(imgs) and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(back, imgs))
        back = bank.to_arrays([3, 0, 4], chunk_bytes=100)                  # several staging chunks
        assert all(np.array_equal(a, imgs[i]) for a, i in zip(back, [3, 0, 4]))
    assert bank.to_arrays([]) == []
    with pytest.raises(IndexError):
        bank.to_arrays([len(imgs)])


# ------------------------------------------------------------------------------------------------------ against PIL
def test_outline_mode_equals_pil_on_integer_boxes():
    from PIL import Image, ImageDraw
    _, render = _mods()
    bank = _bank()
    rows, counts = _rows_counts()
    keep = np.zeros_like(rows)
    kc = np.zeros_like(counts)
    for i in range(len(SIZES)):
        ok = [r for r in rows[i, :counts[i]] if np.isfinite(r).all() and (r[1:] == np.floor(r[1:])).all() and r[3] >= 1 and r[4] >= 1
              and np.abs(r).max() < 1e6]
        if ok:
            keep[i, :len(ok)] = np.asarray(ok)
        kc[i] = len(ok)
    assert kc[:-1].min() >= 12
    got = render.render_detections(bank, *_dev(keep, kc)).to_arrays()
    for i, src in enumerate(_images()):
        im = Image.fromarray(src.copy())
        d = ImageDraw.Draw(im)
        for _, x, y, w, h in keep[i, :kc[i]].tolist():
            d.rectangle((x, y, x + w, y + h), outline=(0, 0, 255), width=1 if (w <= 15 or h <= 15) else 3)
        assert np.array_equal(got[i], np.asarray(im)), SIZES[i]


# ------------------------------------------------------------------------------------------------------- validation
def test_bad_calls_are_refused_and_write_nothing():
    A, _ = _mods()
    from fdet_amd._native import lib, ptr, stream
    bank = _bank()
    n = len(bank)
    rows, counts = _rows_counts()
    d_rows, d_counts = _dev(rows, counts)
    total = bank.nbytes
    dst = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    t_dst = np.zeros(n, dtype=A.IMAGE_DTYPE)
    sizes = bank.table["h"].astype(np.int64) * bank.table["w"] * 3
    t_dst["offset"][1:] = np.cumsum(sizes)[:-1]
    t_dst["h"], t_dst["w"] = bank.table["h"], bank.table["w"]
    ws = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    U8, I32 = torch.uint8, torch.int32

    def call(dst_t=dst, table=t_dst, h_counts=counts, d_cnt=d_counts, k=K, blocks=8):
        d_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
        h_counts = np.ascontiguousarray(h_counts)
        return lib().fdet_render_boxes(ptr(bank.data, U8), ptr(bank.d_table, U8), bank.table.ctypes.data, ptr(d_rows), ptr(d_cnt, I32),
                                       h_counts.ctypes.data, n, k, ptr(dst_t, U8), ptr(d_table, U8), table.ctypes.data, 1, 1, blocks,
                                       0, 0, 255, ptr(ws, I32), stream())

    before = bank.data.clone()
    wrong = t_dst.copy()
    wrong["h"][2] += 1
    over = counts.copy()
    over[3] = K + 1
    assert call(dst_t=bank.data[3:]) == -1                                 # the destination inside the source
    assert call(table=wrong) == -1
    assert call(blocks=0) == -1
    assert call(h_counts=over, d_cnt=torch.from_numpy(over).cuda()) == -1
    assert call(k=-1) == -1
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and torch.equal(bank.data, before)
    assert call() == 0                                                     # and the same call with nothing wrong renders
    torch.cuda.synchronize()
    out = A.DeviceImageBank(dst, t_dst)
    assert all(np.array_equal(g, w) for g, w in zip(out.to_arrays(), _want(True, True, 8)))
    assert bool((dst[total:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------------- end to end
def _trained(golden):
    from fdet_amd.models.PoolResnet import PoolResnet
    g = golden("g6_trained_small")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    model = PoolResnet(filters=32, input_shape=(3, 480, 480), num_of_patches=10)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    return model.cuda().eval()


def test_detect_images_draw_writes_rendered_images_at_mirrored_paths(golden, tmp_path, monkeypatch):
    from PIL import Image
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images
    monkeypatch.chdir(tmp_path)
    torch.save(_trained(golden).state_dict(), tmp_path / "small.pth")
    frames = golden("g6_trained_small")["images"].numpy().transpose(0, 2, 3, 1)         # (3,480,480,3)
    mosaic = np.concatenate([np.concatenate([frames[0], frames[1]], 1), np.concatenate([frames[2], frames[0]], 1)], 0)
    sources = {"a.png": frames[0], "sub/b.png": frames[1], "sub/deep/c.png": frames[2], "mosaic.png": mosaic,
               "sub/crop.png": np.ascontiguousarray(frames[1][40:341, 60:393])}
    for name, arr in sources.items():
        (tmp_path / "in" / name).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(arr).save(tmp_path / "in" / name)
    base = ["--model", "poolresnet", "--filters", "32", "--checkpoint", str(tmp_path / "small.pth"), "--images", str(tmp_path / "in"),
            "--out", str(tmp_path / "res.txt"), "--probability-threshold", "0.3", "--iou-threshold", "0.3", "--batch-images", "2"]
    plain = detect_images.main(base)
    text = (tmp_path / "res.txt").read_text()
    out = detect_images.main(base + ["--draw", str(tmp_path / "drawn")])
    assert (tmp_path / "res.txt").read_text() == text and torch.equal(out["rows"], plain["rows"])       # the text is unchanged
    assert sorted(out["names"]) == sorted(sources) and int(out["counts"].sum()) >= 3
    rows, counts = out["rows"].numpy(), out["counts"].numpy()
    outlined = {}
    for i, name in enumerate(out["names"]):
        got = np.asarray(Image.open(tmp_path / "drawn" / name).convert("RGB"))
        assert np.array_equal(got, R.render_one(sources[name], rows[i], counts[i])), name
        outlined[name] = got
    both = detect_images.main(base + ["--draw", str(tmp_path / "both"), "--anonymize", "pixelate", "--draw-format", "png"])
    differs = 0
    for i, name in enumerate(both["names"]):
        got = np.asarray(Image.open(tmp_path / "both" / name).convert("RGB"))
        assert np.array_equal(got, R.render_one(sources[name], rows[i], counts[i], True, True, 8)), name
        differs += int((got != outlined[name]).any(2).sum())
    assert differs >= 1


def test_fit_draw_dir_writes_the_first_image_of_each_epoch(tmp_path):
    from PIL import Image
    import oracle as O
    import fdet_amd  # noqa: F401
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.trainer import fit
    F_, size, S, B = 64, 480, 10, 2
    g = torch.Generator().manual_seed(5)
    batches = []
    for b in range(2):
        x = torch.randint(0, 256, (B, 3, size, size), dtype=torch.uint8, generator=g)
        boxes = O.synthetic_boxes(B, size, seed=50 + b)
        batches.append((x, torch.stack([O.encode_targets(bb, (size, size), S) for bb in boxes]), boxes))
    mm = ModelMeta(model=PoolResnet(F_, (3, size, size), S).cuda(), lr=1e-4, log_path=tmp_path / "out.log")
    fit(mm, batches, batches[:1], epochs=1, draw_dir=tmp_path / "drawn")
    for name in ("train_epoch_0.png", "validation_epoch_0.png"):
        im = Image.open(tmp_path / "drawn" / name)
        assert im.size == (size, size) and im.mode == "RGB"
    assert sorted(os.listdir(tmp_path / "drawn")) == ["train_epoch_0.png", "validation_epoch_0.png"]
