"""Tiled full-resolution detection on the GPU (csrc/fdet_tiles.hip, fdet_amd/tiling.py): fdet_tile_gather against the
source bytes, against fdet_aug_warp (flags = 0, the window as its crop) and against the numpy restatement; fdet_tile_merge
against tests/tiles_cpu_ref.py; TiledDetector end to end with the stored trained weights."""
import numpy as np
import pytest
import torch

import tiles_cpu_ref as R

pytestmark = pytest.mark.gpu

HO = WO = 480


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tiling
    from fdet_amd.datasets import augment
    return augment, hotpath, tiling


def _images(sizes, seed=0, smooth=True):
    """(H,W,3) uint8 images: a smooth field plus texture, or pure noise (as tests/test_gpu_augment.py builds them)."""
    g = np.random.default_rng(seed)
    out = []
    for H, W in sizes:
        if smooth:
            yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
            base = np.stack([200 * xx + 30 * yy, 120 + 100 * np.sin(6 * xx + 3 * yy), 255 * yy * (1 - xx)], -1)
            img = np.clip(base + g.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        else:
            img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out.append(img)
    return out


def _lsb(got, want, exact_frac):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, d.max()
    assert (d == 0).mean() >= exact_frac, (d == 0).mean()


def _tiles(T, wins):
    t = np.zeros(len(wins), T.TILE_DTYPE)
    for i, w in enumerate(wins):
        t[i] = tuple(w)
    return t


def _gather(bank, tiles, Ho=HO, Wo=WO, out=None):
    _, hp, _ = _mods()
    d = torch.from_numpy(tiles.view(np.uint8).copy()).cuda()
    fr = hp.tile_gather(bank.data, bank.d_table, bank.table, d, tiles, (Ho, Wo), out)
    torch.cuda.synchronize()
    return fr.cpu().numpy()


def _warp(bank, tiles, Ho=HO, Wo=WO):
    """fdet_aug_warp with flags = 0 and every window as its crop"""
    A, _, _ = _mods()
    from fdet_amd._native import check, lib, ptr, stream
    P = np.zeros(len(tiles), A.PARAMS_DTYPE)
    P["image"], P["crop_x0"], P["crop_y0"], P["crop_w"], P["crop_h"] = tiles["image"], tiles["x0"], tiles["y0"], tiles["w"], tiles["h"]
    P["cos_a"], P["alpha"], P["motion_k"] = 1.0, 1.0, 1
    d = torch.from_numpy(P.view(np.uint8).copy()).cuda()
    mid = torch.empty(len(P), 3, Ho, Wo, dtype=torch.uint8, device="cuda")
    u8 = torch.uint8
    check(lib().fdet_aug_warp(ptr(bank.data, u8), ptr(bank.d_table, u8), bank.table.ctypes.data, len(bank), ptr(d, u8),
                              P.ctypes.data, len(P), Ho, Wo, 7, ptr(mid, u8), stream()), "warp")
    torch.cuda.synchronize()
    return mid.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("lead", [0, 5])
def test_gather_identity_windows_are_byte_exact_copies(lead):
    A, _, T = _mods()
    sizes = [(600, 701), (480, 480), (483, 1001), (997, 481)]                # (h, w): widths 701, 1001, 481 are not % 4
    imgs = _images(sizes, seed=1, smooth=False)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda", lead_bytes=lead)
    wins = [(0, 0, 0), (0, 221, 120), (0, 1, 119), (0, 220, 0), (0, 97, 33),  # the four corners of image 0, an odd origin
            (1, 0, 0), (2, 0, 0), (2, 521, 3), (2, 13, 1), (3, 1, 517), (3, 0, 0), (3, 1, 1)]
    tiles = _tiles(T, [(i, x, y, WO, HO) for i, x, y in wins])
    got = _gather(bank, tiles)
    for k, (i, x, y) in enumerate(wins):
        want = imgs[i][y:y + HO, x:x + WO].transpose(2, 0, 1)
        assert np.array_equal(got[k], want), (k, i, x, y)
    assert np.array_equal(got, _warp(bank, tiles))


@pytest.mark.parametrize("wh", [(1024, 683), (300, 451), (479, 1), (2000, 300), (1, 1)])
def test_gather_whole_images_equal_the_warp_and_the_restatement(wh):
    A, _, T = _mods()
    W, H = wh
    imgs = _images([(H, W)], seed=W)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    tiles = _tiles(T, [(0, 0, 0, W, H)])
    got = _gather(bank, tiles)
    assert np.array_equal(got, _warp(bank, tiles))                          # (a) the parent commit's kernel, byte for byte
    _lsb(got[0], R.gather(imgs[0], (0, 0, W, H), HO, WO), 0.999)            # (b) the numpy restatement


def test_gather_interior_windows_up_and_down():
    A, _, T = _mods()
    sizes = [(1100, 1300), (700, 1024), (3000, 4000)]
    imgs = _images(sizes, seed=9)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda", lead_bytes=3)
    wins = [(0, 101, 53, 320, 320),       # up 1.5x
            (0, 201, 7, 1022, 1023),      # down 2.13x
            (0, 980, 780, 320, 320),      # flush with the far corner
            (1, 333, 111, 480, 360), (1, 0, 0, 1024, 700),
            (2, 0, 0, 4000, 3000),        # down 8.3x: beyond the LDS stage, the direct path
            (2, 1777, 1201, 1441, 1500)]  # 3x: around the switch between the two paths
    tiles = _tiles(T, wins)
    got = _gather(bank, tiles)
    assert np.array_equal(got, _warp(bank, tiles))
    for k, w in enumerate(wins):
        _lsb(got[k], R.gather(imgs[w[0]], w[1:], HO, WO), 0.999)


@pytest.mark.parametrize("hw", [(37, 50), (8, 129), (260, 436)])
def test_gather_other_frame_sizes(hw):
    A, _, T = _mods()
    Ho, Wo = hw
    imgs = _images([(300, 451), (64, 200)], seed=4)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda", lead_bytes=1)
    wins = [(0, 0, 0, 451, 300), (0, 11, 17, Wo, Ho), (1, 3, 5, 150, 40), (1, 0, 0, 200, 64), (0, 450, 299, 1, 1)]
    tiles = _tiles(T, wins)
    got = _gather(bank, tiles, Ho, Wo)
    assert np.array_equal(got, _warp(bank, tiles, Ho, Wo))
    assert np.array_equal(got[1], imgs[0][17:17 + Ho, 11:11 + Wo].transpose(2, 0, 1))
    for k, w in enumerate(wins):
        _lsb(got[k], R.gather(imgs[w[0]], w[1:], Ho, Wo), 0.999)


def test_gather_rejects_bad_windows_and_writes_nothing():
    A, _, T = _mods()
    from fdet_amd import FdetError
    imgs = _images([(500, 600)], seed=2)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    good = (0, 10, 10, 480, 480)
    for bad in [(0, 121, 10, 480, 480), (0, 10, 21, 480, 480), (0, -1, 0, 100, 100), (0, 0, -1, 100, 100), (0, 0, 0, 0, 100),
                (0, 0, 0, 100, -3), (1, 0, 0, 100, 100), (-1, 0, 0, 100, 100), (0, 0, 0, 601, 500)]:
        out = torch.full((2, 3, HO, WO), 171, dtype=torch.uint8, device="cuda")
        with pytest.raises(FdetError, match="tile_gather"):
            _gather(bank, _tiles(T, [good, bad]), out=out)
        torch.cuda.synchronize()
        assert bool((out == 171).all()), bad


# ------------------------------------------------------------------------------------------------------------- merge
def _merge_gpu(rows, counts, tiles, offs, sizes, margin, thr, Kout):
    A, hp, T = _mods()
    table = np.zeros(len(sizes), A.IMAGE_DTYPE)
    table["h"], table["w"] = [s[0] for s in sizes], [s[1] for s in sizes]
    d_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    d_tiles = torch.from_numpy(tiles.view(np.uint8).copy()).cuda()
    out, cnt, rej = hp.tile_merge(torch.from_numpy(rows).cuda(), torch.from_numpy(np.asarray(counts, np.int32)).cuda(), d_tiles,
                                  torch.from_numpy(np.asarray(offs, np.int32)).cuda(), d_table, (HO, WO), margin, thr, Kout)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy(), int(rej.item())


def _case(seed, sizes, K, full=()):
    """Random rows with tied scores, zero-area boxes and empty tiles; images in `full` get K rows in every tile."""
    _, _, T = _mods()
    g = np.random.default_rng(seed)
    plan = T.plan_tiles(sizes, (480,), 0.25, True)
    Tn = len(plan)
    rows = np.full((Tn, K, 5), -7.0, np.float32)                            # garbage past the counts is never read
    counts = g.integers(0, min(K, 30) + 1, Tn).astype(np.int32)
    counts[g.integers(0, Tn, max(1, Tn // 4))] = 0
    for t in range(Tn):
        if plan.tiles[t]["image"] in full:
            counts[t] = K
        c = int(counts[t])
        sc = np.round(g.uniform(0.01, 1.0, c) * 16) / 16
        xy = g.uniform(-5, 470, (c, 2))
        wh = g.uniform(0, 90, (c, 2))
        wh[g.uniform(size=c) < 0.15] = 0
        rows[t, :c] = np.concatenate([sc[:, None], xy, wh], 1).astype(np.float32)
    return plan, rows, counts


@pytest.mark.parametrize("seed,margin,thr", [(0, 0.0, 0.5), (1, 0.0, 0.01), (2, 12.0, 0.5), (3, 33.5, 0.3)])
def test_merge_equals_the_numpy_restatement(seed, margin, thr):
    sizes = [(700, 1024), (480, 480), (1300, 900), (333, 2000), (600, 600)]
    plan, rows, counts = _case(seed, sizes, K=100)
    a, b = int(plan.tile_offset[4]), int(plan.tile_offset[5])
    counts[a:b] = 0                                                         # an image whose tiles detect nothing
    if seed == 1:
        rows[0, 0, 0] = np.nan                                              # a NaN score is visited last
    want = R.merge(rows, counts, plan.tiles, plan.tile_offset, sizes, HO, WO, margin, thr, 4864)
    got = _merge_gpu(rows, counts, plan.tiles, plan.tile_offset, sizes, margin, thr, 4864)
    assert got[2] == want[2] == 0
    assert np.array_equal(got[1], want[1]) and want[1][4] == 0 and want[1][[0, 2, 3]].min() > 0
    assert np.array_equal(got[0], want[0], equal_nan=True)


def test_merge_rejects_an_image_over_4864_candidates_and_leaves_the_others():
    sizes = [(700, 1024), (3000, 4000), (600, 600)]                         # image 1: 89 windows
    plan, rows, counts = _case(5, sizes, K=100, full=(1,))
    a, b = int(plan.tile_offset[1]), int(plan.tile_offset[2])
    assert int(counts[a:b].sum()) == 8900 > 4864
    want = R.merge(rows, counts, plan.tiles, plan.tile_offset, sizes, HO, WO, 0.0, 0.5, 4864)
    got = _merge_gpu(rows, counts, plan.tiles, plan.tile_offset, sizes, 0.0, 0.5, 4864)
    assert want[2] == 1 and got[2] == 1
    assert got[1][1] == 0 and got[1][0] > 0 and got[1][2] > 0
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    # exactly at the limit is fine: 48 full windows + 64 rows = 4864 candidates
    counts[a:b] = 0
    counts[a:a + 48] = 100
    counts[a + 48] = 64
    want = R.merge(rows, counts, plan.tiles, plan.tile_offset, sizes, HO, WO, 0.0, 0.5, 4864)
    got = _merge_gpu(rows, counts, plan.tiles, plan.tile_offset, sizes, 0.0, 0.5, 4864)
    assert want[2] == 0 and got[2] == 0 and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    # too few output rows and a count above K reject too
    small = _merge_gpu(rows, counts, plan.tiles, plan.tile_offset, sizes, 0.0, 0.5, int(want[1][0]) - 1)
    assert small[2] >= 1 and small[1][0] == 0
    counts[0] = 101
    over = _merge_gpu(rows, counts, plan.tiles, plan.tile_offset, sizes, 0.0, 0.5, 4864)
    assert over[2] == 1 and over[1][0] == 0 and np.array_equal(over[1][1:], want[1][1:])


# ------------------------------------------------------------------------------------------------------- end to end
def _trained(golden, name, filters):
    from fdet_amd.models.PoolResnet import PoolResnet
    g = golden(name)
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    model = PoolResnet(filters=filters, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.7, iou_threshold=0.01)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    return model.cuda().eval()


QUADS = [0, 1, 2, 0]                                                        # stored frames 0 and 1 carry faces, 2 none
ORIGINS = [(0, 0), (480, 0), (0, 480), (480, 480)]                          # (x0, y0) in plan order (row-major)


def _mosaic(golden):
    A, _, _ = _mods()
    images = golden("g6_trained_small")["images"].numpy()                  # (3,3,480,480) uint8
    src = np.zeros((960, 960, 3), np.uint8)
    for q, (x0, y0) in zip(QUADS, ORIGINS):
        src[y0:y0 + 480, x0:x0 + 480] = images[q].transpose(1, 2, 0)
    return A.DeviceImageBank.from_arrays([src], "cuda"), images


def _per_frame(model, reducer, images):
    """the existing path, one frame at a time"""
    out = []
    with torch.no_grad():
        for q in QUADS:
            r, c = reducer.forward_batch(model.forward_frames(torch.from_numpy(images[q])[None].cuda()))
            out.append((r[0].cpu().numpy(), int(c[0])))
    return out


def _expected_mosaic(per, thr, Kout=4864):
    K = per[0][0].shape[0]
    rows = np.stack([p[0] for p in per])
    counts = [p[1] for p in per]
    tiles = [(0, x0, y0, 480, 480) for x0, y0 in ORIGINS]
    return R.merge(rows, counts, tiles, [0, 4], [(960, 960)], HO, WO, 0.0, thr, Kout)


@pytest.mark.parametrize("name,filters", [("g6_trained_small", 32), ("g16_trained_medium", 64)])
def test_mosaic_of_stored_frames_equals_the_merged_per_frame_results(golden, name, filters):
    _, _, T = _mods()
    model = _trained(golden, name, filters)
    if filters == 64:
        assert model.engine.ps
    bank, images = _mosaic(golden)
    per = _per_frame(model, model.reduce_bounding_boxes, images)
    assert sum(1 for _, c in per if c >= 1) >= 2                            # cannot pass on empty output
    want = _expected_mosaic(per, 0.01)
    det = T.TiledDetector(model, tile_sizes=(480,), overlap=0.0, include_whole=False)
    assert [tuple(t)[1:3] for t in det.plan([(960, 960)]).tiles] == ORIGINS
    rows, counts = det.detect(bank, [0])
    assert tuple(rows.shape) == (1, 4864, 5) and counts.dtype == torch.int32
    assert int(counts[0]) == int(want[1][0]) >= 2
    assert np.array_equal(rows.cpu().numpy(), want[0])
    split = det.detect_split(bank, [0])
    assert len(split) == 1 and np.array_equal(split[0].cpu().numpy(), want[0][0, :want[1][0]])


def test_whole_image_window_alone_is_todays_result(golden):
    A, _, T = _mods()
    model = _trained(golden, "g6_trained_small", 32)
    images = golden("g6_trained_small")["images"]
    bank = A.DeviceImageBank.from_arrays([im.numpy().transpose(1, 2, 0) for im in images], "cuda")
    with torch.no_grad():
        r, c = model.reduce_bounding_boxes.forward_batch(model.forward_frames(images.cuda()))
    rows, counts = T.TiledDetector(model, tile_sizes=(), include_whole=True, max_out=100).detect(bank, [0, 1, 2])
    assert int(c.sum()) >= 2 and torch.equal(counts, c) and torch.equal(rows, r)
    with torch.no_grad():
        r2, c2 = model.reduce_bounding_boxes.forward_batch(model.forward_frames(images[[1, 0]].cuda()))
    rows2, counts2 = T.TiledDetector(model, tile_sizes=(), include_whole=True, max_out=100).detect(bank, [1, 0])
    assert int(c2.sum()) >= 2 and torch.equal(rows2, r2) and torch.equal(counts2, c2)


def test_chunking_does_not_change_the_result(golden):
    _, _, T = _mods()
    model = _trained(golden, "g6_trained_small", 32)
    bank, _ = _mosaic(golden)
    kw = dict(tile_sizes=(480,), overlap=0.25, include_whole=True, edge_margin=4.0)
    assert len(T.TiledDetector(model, **kw).plan(bank.sizes)) == 10
    a = T.TiledDetector(model, max_frames=3, **kw).detect(bank, [0])
    b = T.TiledDetector(model, max_frames=256, **kw).detect(bank, [0])
    assert int(b[1][0]) >= 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_evaluator_pairing_and_low_score_reducer(golden):
    _, _, T = _mods()
    from fdet_amd.evaluation import DetectionEvaluator
    model = _trained(golden, "g16_trained_medium", 64)
    bank, images = _mosaic(golden)
    det = T.TiledDetector(model, tile_sizes=(480,), overlap=0.0, include_whole=False)
    rows, counts = det.detect(bank, [0])
    k = int(counts[0])
    assert k >= 2
    ev = DetectionEvaluator()
    gt = rows[0, :k].clone()
    gt[:, 0] = 1.0
    ev.update(rows, counts, [gt])
    r = ev.compute()
    assert r.ap == 1.0 and (r.n_gt, r.n_images, r.n_det) == (k, 1, k) and int(r.fp.sum()) == 0
    assert int(ev.state.counters[3]) == 0
    # the evaluator's reducer keeps everything the model's own reducer kept at its higher threshold
    low = ev.reducer_for(model)
    assert low.probability_threshold < model.reduce_bounding_boxes.probability_threshold
    hi_rows = _per_frame(model, model.reduce_bounding_boxes, images)
    lo_rows = _per_frame(model, low, images)
    for (hr, hc), (lr, lc) in zip(hi_rows, lo_rows):
        have = {tuple(v) for v in lr[:lc].tolist()}
        assert lc >= hc and all(tuple(v) in have for v in hr[:hc].tolist())
    rows_lo, counts_lo = T.TiledDetector(model, tile_sizes=(480,), overlap=0.0, include_whole=False, reducer=low).detect(bank, [0])
    assert int(counts_lo[0]) >= k
    assert model.reduce_bounding_boxes.probability_threshold == 0.7         # never modified


class _FullReducer:
    """stands in for a reducer at a threshold so low that every cell of every window fires"""
    iou_threshold = 0.5

    def forward_batch(self, y):
        B = y.shape[0]
        g = torch.Generator().manual_seed(B)
        rows = torch.rand(B, 100, 5, generator=g) * 300 + 1
        rows[:, :, 0] = 0.5
        return rows.cuda(), torch.full((B,), 100, dtype=torch.int32, device="cuda")


def test_detect_raises_when_an_image_is_over_the_limit():
    A, _, T = _mods()
    from fdet_amd import FdetError
    from fdet_amd.models.PoolResnet import PoolResnet
    model = PoolResnet(filters=32, input_shape=(3, 480, 480), num_of_patches=10).cuda().eval()
    imgs = _images([(500, 500), (3000, 4000)], seed=3, smooth=False)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    det = T.TiledDetector(model, reducer=_FullReducer(), max_frames=32)
    rows, counts = det.detect(bank, [0])                                    # 1 + 4 windows: 500 candidates
    assert int(counts[0]) > 0
    with pytest.raises(FdetError, match="exceed a limit"):
        det.detect(bank, [0, 1])                                            # 90 windows of image 1: 9000 candidates
    with pytest.raises(ValueError):
        T.TiledDetector(model.train()).detect(bank, [0])


def test_ssd_mosaic_equals_the_merged_per_frame_results(golden):
    _, hp, T = _mods()
    import oracle.ssd_model_oracle as SM
    from fdet_amd.models.SSD import SSD
    from fdet_amd.datasets.utils import ReduceSSDBoundingBoxes
    model = SSD(filters=16, input_shape=(3, 480, 480), probability_threshold=0.5, iou_threshold=0.3)
    model.load_state_dict({k: v.clone() for k, v in SM.init_params(16, 11).items()})
    model = model.cuda().eval()
    bank, images = _mosaic(golden)
    own = model.reduce_bounding_boxes
    chosen = None
    for pt in (0.9, 0.7, 0.5, 0.3, 0.1, 0.01):                              # untrained weights: take the first threshold
        red = ReduceSSDBoundingBoxes(probability_threshold=pt, iou_threshold=0.3, input_shape=own.input_shape,    # with output
                                     patch_sizes=own.patch_sizes, priors=own.priors, with_priors=own.with_priors)
        per = []
        with torch.no_grad():
            for q in QUADS:
                x = hp.resize_bilinear_norm(torch.from_numpy(images[q])[None].cuda(), (480, 480))
                r, c = red.forward_batch(model(x))
                per.append((r[0].cpu().numpy(), int(c[0])))
        if sum(1 for _, c in per if c >= 1) >= 2:
            chosen = (red, per)
            break
    assert chosen is not None
    red, per = chosen
    assert sum(c for _, c in per) <= 4864
    want = _expected_mosaic(per, 0.3)
    rows, counts = T.TiledDetector(model, tile_sizes=(480,), overlap=0.0, include_whole=False, reducer=red).detect(bank, [0])
    assert per[0][0].shape[0] == hp.ssd_num_priors()
    assert int(counts[0]) == int(want[1][0]) >= 1
    assert np.array_equal(rows.cpu().numpy(), want[0])


# ------------------------------------------------------------------------------------------------------------ scripts
def test_detect_images_writes_the_wider_result_format(golden, tmp_path, monkeypatch):
    from PIL import Image
    from fdet_amd import detect_images
    monkeypatch.chdir(tmp_path)
    model = _trained(golden, "g6_trained_small", 32)
    torch.save(model.state_dict(), tmp_path / "small.pth")
    images = golden("g6_trained_small")["images"].numpy()
    (tmp_path / "imgs" / "sub").mkdir(parents=True)
    mosaic = np.zeros((960, 960, 3), np.uint8)
    for q, (x0, y0) in zip(QUADS, ORIGINS):
        mosaic[y0:y0 + 480, x0:x0 + 480] = images[q].transpose(1, 2, 0)
    Image.fromarray(mosaic).save(tmp_path / "imgs" / "sub" / "mosaic.png")
    Image.fromarray(images[2].transpose(1, 2, 0)).save(tmp_path / "imgs" / "empty.png")
    out = detect_images.main(["--model", "poolresnet", "--filters", "32", "--checkpoint", str(tmp_path / "small.pth"), "--images",
                              str(tmp_path / "imgs"), "--out", str(tmp_path / "res.txt"), "--tile", "480", "--overlap", "0",
                              "--no-whole", "--probability-threshold", "0.7", "--iou-threshold", "0.01"])
    per = _per_frame(model, model.reduce_bounding_boxes, images)
    want = _expected_mosaic(per, 0.01)
    assert out["names"] == ["empty.png", "sub/mosaic.png"] and out["counts"].tolist() == [0, int(want[1][0])]
    lines = (tmp_path / "res.txt").read_text().split("\n")
    k = int(want[1][0])
    assert lines[0] == "empty.png" and lines[1] == "0" and lines[2] == "sub/mosaic.png" and lines[3] == str(k) and k >= 2
    for line, row in zip(lines[4:4 + k], want[0][0, :k]):
        x, y, w, h, s = line.split()
        assert [float(x), float(y), float(w), float(h)] == row[1:].tolist() and abs(float(s) - row[0]) < 1e-4
    assert lines[4 + k:] == [""]


def test_run_validation_epoch_tiled_report(tmp_path, monkeypatch, capsys):
    from fdet_amd import run_validation_epoch
    monkeypatch.chdir(tmp_path)
    base = ["--model", "poolresnet", "--filters", "64", "--batch-size", "8", "--synthetic-images", "16"]
    torch.manual_seed(3)
    plain = run_validation_epoch.main(base)
    text_plain = capsys.readouterr().out
    assert "tiled" not in plain and "tiled" not in text_plain
    torch.manual_seed(3)
    out = run_validation_epoch.main(base + ["--tiled", "--tile", "480", "--overlap", "0.25"])
    text = capsys.readouterr().out
    assert text.startswith(text_plain) and "tiled AP@0.50" in text           # the existing lines are unchanged
    r = out["tiled"]
    assert (r.n_images, r.n_gt) == (16, out["result"].n_gt) and np.isfinite(r.ap) and 0.0 <= r.ap <= 1.0
