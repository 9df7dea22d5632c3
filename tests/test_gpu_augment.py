"""On-device augmentation (csrc/fdet_augment.hip, fdet_amd/datasets/augment.py) against the numpy restatement
tests/aug_cpu_ref.py on the same sampled parameters, plus the bank / batch / fit plumbing around it."""
import numpy as np
import pytest
import torch

import aug_cpu_ref as R

pytestmark = pytest.mark.gpu

HO = WO = 480


def _A():
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets import augment
    return augment


def _hp():
    from fdet_amd import hotpath
    return hotpath


def _images(sizes, seed=0, smooth=True):
    """(H,W,3) uint8 images: a smooth field (bilinear-friendly) plus texture, or pure noise."""
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


def _base_params(A, sizes, flags=0):
    P = np.zeros(len(sizes), A.PARAMS_DTYPE)
    for i, (H, W) in enumerate(sizes):
        P[i]["image"] = i
        P[i]["crop_w"], P[i]["crop_h"] = W, H
        P[i]["key"] = 1000 + i
    P["flags"] = flags
    P["cos_a"], P["alpha"], P["motion_k"] = 1.0, 1.0, 1
    return P


def _run(A, bank, P, seed=7, Ho=HO, Wo=WO):
    """The two pixel kernels through the C-ABI: -> (mid, frames, x) on the device."""
    from fdet_amd._native import check, lib, ptr, stream
    B = len(P)
    P = np.ascontiguousarray(P)
    d = torch.from_numpy(P.view(np.uint8).copy()).cuda()
    mid = torch.empty(B, 3, Ho, Wo, dtype=torch.uint8, device="cuda")
    fr, x = torch.empty_like(mid), torch.empty(B, 3, Ho, Wo, device="cuda")
    u8 = torch.uint8
    check(lib().fdet_aug_warp(ptr(bank.data, u8), ptr(bank.d_table, u8), bank.table.ctypes.data, len(bank), ptr(d, u8),
                              P.ctypes.data, B, Ho, Wo, seed, ptr(mid, u8), stream()), "warp")
    check(lib().fdet_aug_finish(ptr(mid, u8), ptr(d, u8), P.ctypes.data, B, Ho, Wo, seed, ptr(fr, u8), ptr(x), stream()), "finish")
    torch.cuda.synchronize()
    return mid.cpu().numpy(), fr.cpu().numpy(), x


def _lsb(got, want, exact_frac):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1, d.max()
    assert (d == 0).mean() >= exact_frac, (d == 0).mean()


def _f32_matches(frames_dev, x):
    ref = _hp().u8_to_f32_norm(frames_dev)
    assert torch.equal(ref.view(torch.int32), x.view(torch.int32))


def test_identity_is_the_hwc_to_chw_permute():
    A = _A()
    imgs = _images([(480, 480)], smooth=False)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    mid, fr, x = _run(A, bank, _base_params(A, [(480, 480)]))
    want = imgs[0].transpose(2, 0, 1)
    assert np.array_equal(mid[0], want) and np.array_equal(fr[0], want)
    _f32_matches(torch.from_numpy(fr).cuda(), x)


@pytest.mark.parametrize("wh", [(1024, 683), (300, 451), (479, 1), (2000, 300), (1, 1)])
def test_resize_only(wh):
    A, hp = _A(), _hp()
    W, H = wh
    imgs = _images([(H, W)], seed=W)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    P = _base_params(A, [(H, W)])
    mid, fr, x = _run(A, bank, P)
    want = R.to_u8(R.warp_values(imgs[0], P[0], HO, WO, 7))
    _lsb(fr[0], want, 0.999)
    assert np.array_equal(mid, fr)
    src = torch.from_numpy(imgs[0].transpose(2, 0, 1).copy())[None].cuda()
    aten = (hp.resize_bilinear_norm(src, (HO, WO)) * 255).cpu().numpy()[0]
    assert np.abs(aten - fr[0].astype(np.float64)).max() <= 1 + 1e-3
    _f32_matches(torch.from_numpy(fr).cuda(), x)


def test_flip_mirrors_bit_exactly():
    A = _A()
    sizes = [(683, 1024), (451, 300)]
    bank = A.DeviceImageBank.from_arrays(_images(sizes, seed=3), "cuda")
    P = _base_params(A, sizes)
    P[1]["crop_x0"], P[1]["crop_y0"], P[1]["crop_w"], P[1]["crop_h"] = 17, 40, 201, 300
    _, a, _ = _run(A, bank, P)
    P["flags"] = A.FLIP
    _, b, _ = _run(A, bank, P)
    assert np.array_equal(b, a[..., ::-1])


def _photometric_params(A, sizes, flags):
    P = _base_params(A, sizes, flags)
    g = np.random.default_rng(11)
    ang = g.uniform(-20, 20, len(sizes))
    P["angle"], P["cos_a"], P["sin_a"] = ang, np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
    P["alpha"], P["beta"] = 1 + g.uniform(-0.2, 0.2, len(sizes)), 255 * g.uniform(-0.2, 0.2, len(sizes))
    P["sigma"] = np.sqrt(g.uniform(0, 400, len(sizes)))
    for i, (H, W) in enumerate(sizes):
        if i % 2:
            P[i]["crop_x0"], P[i]["crop_y0"], P[i]["crop_w"], P[i]["crop_h"] = W // 5, H // 7, W // 2, H // 2
    return P


@pytest.mark.parametrize("name", ["rotate", "brightness", "noise", "all"])
def test_photometric_and_rotation_within_one_lsb(name):
    A = _A()
    flags = {"rotate": A.ROTATE, "brightness": A.BRIGHTNESS, "noise": A.NOISE,
             "all": A.ROTATE | A.BRIGHTNESS | A.NOISE | A.FLIP | A.GLASS | A.MOTION}[name]
    sizes = [(683, 1024), (451, 300), (700, 990)]
    imgs = _images(sizes, seed=5)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    P = _photometric_params(A, sizes, flags)
    if flags & A.MOTION:
        for i, k in enumerate((3, 5, 7)):
            ker = A.bresenham(k, 0, i, k - 1, k - 1 - i).astype(np.float32)
            P[i]["motion_k"], P[i]["motion_w"][:k * k] = k, (ker / ker.sum()).reshape(-1)
    mid, fr, x = _run(A, bank, P)
    for i in range(len(sizes)):
        _lsb(mid[i], R.to_u8(R.warp_values(imgs[i], P[i], HO, WO, 7)), 0.99)
        want = R.finish(mid[i], P[i], 7)
        if flags & A.MOTION:
            _lsb(fr[i], want, 0.99)
        else:
            assert np.array_equal(fr[i], want)
    _f32_matches(torch.from_numpy(fr).cuda(), x)


def test_glass_alone_bit_exact_and_motion_alone_within_one_lsb():
    A = _A()
    sizes = [(480, 480), (480, 480), (480, 480)]
    imgs = _images(sizes, seed=9, smooth=False)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    P = _base_params(A, sizes, A.GLASS)
    mid, fr, _ = _run(A, bank, P)
    for i in range(3):
        assert np.array_equal(mid[i], imgs[i].transpose(2, 0, 1))
        assert np.array_equal(fr[i], R.glass(mid[i], 7, int(P[i]["key"])))
        assert not np.array_equal(fr[i], mid[i])
    P["flags"] = A.MOTION
    for i, (k, line) in enumerate([(3, (0, 0, 2, 2)), (5, (0, 1, 4, 3)), (7, (3, 0, 3, 6))]):
        ker = A.bresenham(k, *line).astype(np.float32)
        P[i]["motion_k"], P[i]["motion_w"][:k * k] = k, (ker / ker.sum()).reshape(-1)
    mid, fr, _ = _run(A, bank, P)
    for i in range(3):
        _lsb(fr[i], R.finish(mid[i], P[i], 7), 0.99)


def test_image_and_boxes_stay_consistent():
    """Flat background, one filled rectangle per image; after crop + rotation every surviving box encloses its rectangle's
    pixels to within 1 px."""
    A = _A()
    g = np.random.default_rng(2)
    sizes, imgs, boxes = [], [], []
    for i in range(8):
        H, W = int(g.integers(600, 900)), int(g.integers(600, 900))
        img = np.full((H, W, 3), 40, np.uint8)
        w, h = int(g.integers(60, 120)), int(g.integers(60, 120))
        x, y = int(g.integers(W // 4, W // 2)), int(g.integers(H // 4, H // 2))
        img[y:y + h, x:x + w] = (220, 180, 90)
        sizes.append((H, W))
        imgs.append(img)
        boxes.append(np.array([[1, x, y, w, h]], np.float32))
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    P = _base_params(A, sizes, A.ROTATE | A.CROP)
    ang = g.uniform(-20, 20, 8)
    P["angle"], P["cos_a"], P["sin_a"] = ang, np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
    for i, (H, W) in enumerate(sizes):
        P[i]["crop_x0"], P[i]["crop_y0"] = W // 8, H // 8
        P[i]["crop_w"], P[i]["crop_h"] = W - W // 4, H - H // 4
    t = A.default_transform((HO, WO))
    x, fr, rows, offs = t(bank, np.arange(8), boxes, 0, params=P)
    fr, rows, offs = fr.cpu().numpy(), rows.cpu().numpy(), offs.cpu().numpy()
    assert offs[-1] == 8
    for i in range(8):
        _, bx, by, bw, bh = rows[offs[i]]
        ys, xs = np.nonzero(np.abs(fr[i].astype(np.int32) - 40).max(0) > 2)
        assert xs.min() >= bx - 1 and xs.max() + 1 <= bx + bw + 1 and ys.min() >= by - 1 and ys.max() + 1 <= by + bh + 1, i
        # and the box is not loose beyond the rotated envelope: its area at most twice the pixels' bounding box
        assert bw * bh <= 2 * (xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)


def _box_batch(A, n=12, seed=4):
    g = np.random.default_rng(seed)
    sizes = [(int(g.integers(300, 800)), int(g.integers(300, 1000))) for _ in range(n)]
    boxes = []
    for i, (H, W) in enumerate(sizes):
        k = 0 if i % 4 == 0 else int(g.integers(1, 4))
        r = [[1, g.integers(-20, W - 10), g.integers(-20, H - 10), g.integers(2, 200), g.integers(2, 200)] for _ in range(k)]
        boxes.append(np.asarray(r, np.float32).reshape(-1, 5))
    return sizes, boxes


def test_boxes_and_targets_match_the_restatement():
    A, hp = _A(), _hp()
    sizes, boxes = _box_batch(A)
    bank = A.DeviceImageBank.from_arrays(_images(sizes, seed=1), "cuda")
    t = A.training_transform((HO, WO), seed=3)
    for step in range(4):
        idx = np.arange(len(sizes))[::-1].copy()
        P = t.params_for(bank, idx, step)
        P["flags"] |= np.where(np.arange(len(P)) % 2 == 0, A.ROTATE, 0)
        P["cos_a"] = np.where(P["flags"] & A.ROTATE, np.cos(0.3), P["cos_a"])
        P["sin_a"] = np.where(P["flags"] & A.ROTATE, np.sin(0.3), P["sin_a"])
        x, fr, rows, offs = t(bank, idx, boxes, step, params=P)
        want_rows, want_offs = [], [0]
        for p in P:
            r = R.boxes(boxes[p["image"]], p, *sizes[p["image"]], HO, WO)
            want_rows.append(r)
            want_offs.append(want_offs[-1] + len(r))
        want_rows = np.concatenate(want_rows)
        got_offs = offs.cpu().numpy()
        assert got_offs.tolist() == want_offs
        assert np.array_equal(rows.cpu().numpy()[:want_offs[-1]], want_rows)
        per = [torch.from_numpy(want_rows[want_offs[i]:want_offs[i + 1]]) for i in range(len(P))]
        for S in (10, 15):
            assert torch.equal(hp.encode_targets_device(rows, offs, (WO, HO), S), hp.encode_targets(per, (WO, HO), S))
        assert torch.equal(hp.ssd_encode_targets_device(rows, offs, (WO, HO)), hp.ssd_encode_targets(per, (WO, HO)))


def test_batches_with_no_surviving_boxes():
    A, hp = _A(), _hp()
    sizes = [(400, 600)] * 5
    boxes = [np.zeros((0, 5), np.float32)] + [np.array([[1, 10, 10, 2, 2], [1, 700, 10, 20, 20]], np.float32)] * 4
    bank = A.DeviceImageBank.from_arrays(_images(sizes), "cuda")
    t = A.default_transform((HO, WO))
    _, _, rows, offs = t(bank, np.arange(5), boxes, 0)
    assert offs.cpu().tolist() == [0] * 6
    assert torch.count_nonzero(hp.encode_targets_device(rows, offs, (WO, HO), 10)) == 0
    assert torch.equal(hp.ssd_encode_targets_device(rows, offs, (WO, HO)), hp.ssd_encode_targets([torch.zeros(0, 5)] * 5, (WO, HO)))
    empty = [np.zeros((0, 5), np.float32)] * 5
    _, _, rows, offs = t(bank, np.arange(5), empty, 0)
    assert offs.cpu().tolist() == [0] * 6


@pytest.mark.parametrize("B", [1, 7, 64, 256])
def test_batch_shapes(B):
    A = _A()
    g = np.random.default_rng(B)
    n = max(B, 8)
    sizes = [(int(g.integers(300, 720)), int(g.integers(300, 1024))) for _ in range(n)]
    imgs = _images(sizes, seed=B, smooth=False)
    boxes = [np.array([[1, 5, 5, 50, 60]], np.float32)] * n
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    t = A.training_transform((HO, WO), seed=B)
    idx = g.permutation(n)[:B]
    x, fr, rows, offs = t(bank, idx, boxes, 5)
    assert x.shape == (B, 3, HO, WO) and fr.shape == (B, 3, HO, WO) and offs.shape == (B + 1,)
    _f32_matches(fr, x)
    P = t.params_for(bank, idx, 5)
    frn = fr.cpu().numpy()
    for i in sorted({0, B // 2, B - 1}):
        v = R.warp_values(imgs[idx[i]], P[i], HO, WO, t.seed)
        want = R.finish(R.to_u8(v), P[i], t.seed)
        d = np.abs(frn[i].astype(np.int32) - want.astype(np.int32))
        # the restatement's own intermediate: a 1-LSB difference there passes through glass unchanged and through motion
        # blur's weighted mean as at most one more LSB after rounding
        assert (d <= 1).mean() >= 0.99 and d.max() <= 2, (i, d.max())
    if B == 64:
        _, a, _, _ = t(bank, idx[:32], boxes, 5, params=P[:32])
        _, b, _, _ = t(bank, idx[32:], boxes, 5, params=P[32:])
        assert torch.equal(torch.cat([a, b]), fr)


def test_bank_beyond_4gib_gives_the_same_output():
    A = _A()
    sizes = [(683, 1024), (451, 300), (700, 990)]
    imgs = _images(sizes, seed=8, smooth=False)
    boxes = [np.array([[1, 20, 30, 100, 80]], np.float32)] * 3
    small = A.DeviceImageBank.from_arrays(imgs, "cuda")
    lead = (1 << 32) + 12345
    big = A.DeviceImageBank.from_arrays(imgs, "cuda", lead_bytes=lead)
    assert int(big.table["offset"][0]) == lead and big.data.numel() > (1 << 32)
    t = A.training_transform((HO, WO), seed=1)
    P = t.params_for(small, np.arange(3), 0)
    P["flags"] |= A.ROTATE | A.NOISE | A.GLASS
    outs = [t(bk, np.arange(3), boxes, 0, params=P) for bk in (small, big)]
    (xa, fa, ra, oa), (xb, fb, rb, ob) = outs
    assert torch.equal(xa, xb) and torch.equal(fa, fb) and torch.equal(oa, ob)
    n = int(oa[-1])
    assert n > 0 and torch.equal(ra[:n], rb[:n])
    del big, outs
    torch.cuda.empty_cache()


def test_subset_and_bank_sizes():
    A = _A()
    sizes = [(10, 20), (30, 40), (5, 6)]
    imgs = _images(sizes, smooth=False)
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda", chunk_bytes=1000)     # several staging chunks, one oversize image
    assert bank.sizes.tolist() == [[10, 20], [30, 40], [5, 6]] and bank.nbytes == sum(i.size for i in imgs)
    data = bank.data.cpu().numpy()
    for i, im in enumerate(imgs):
        o = int(bank.table["offset"][i])
        assert np.array_equal(data[o:o + im.size], im.reshape(-1))
    sub = bank.subset([2, 0])
    assert sub.sizes.tolist() == [[5, 6], [10, 20]] and sub.data.data_ptr() == bank.data.data_ptr()


def test_producing_batches_does_not_synchronise_the_host(monkeypatch):
    A, hp = _A(), _hp()
    bank, boxes = A.synthetic_bank(24, "cuda", seed=3, max_side=600)
    batches = A.DeviceBatches(bank, boxes, 8, A.training_transform((HO, WO), seed=2), 10)
    list(batches)                                              # warm up (first launches, allocator)
    torch.cuda.synchronize()
    got = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            got.append(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(got) == 3 and all(not b[2].materialized for b in got)
    # sync debug mode may not be honoured on every runtime: also check no .item()/.cpu() is reached
    calls = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self, *a, **k: calls.append("item"))
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self, *a, **k: calls.append("tolist"))
    for b in batches:
        assert b[0].shape == (8, 3, HO, WO) and b[1].shape == (8, 5, 10, 10)
    monkeypatch.undo()
    assert calls == []
    torch.cuda.synchronize()
    x, y, gt = got[0]
    assert len(gt) == 8 and all(gt[i].shape[1] == 5 for i in range(8)) and gt.materialized
    per = [gt[i].cpu() for i in range(8)]
    assert torch.equal(y, hp.encode_targets(per, (WO, HO), 10))


def _moved(model, before):
    return all(not torch.equal(p.detach().cpu(), before[n]) for n, p in model.named_parameters())


def test_fit_over_device_batches_poolresnet(tmp_path):
    A = _A()
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.trainer import fit
    torch.manual_seed(0)
    bank, boxes = A.synthetic_bank(100, "cuda", seed=5, max_side=800)
    model = PoolResnet(16, (3, HO, WO), 10).cuda()
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    mm = ModelMeta(model=model, lr=1e-3, log_path=tmp_path / "out.log")
    tr = A.DeviceBatches(bank, boxes, 16, A.training_transform((3, HO, WO), seed=1), 10)
    va = A.DeviceBatches(bank.subset(range(32)), boxes[:32], 16, A.default_transform((HO, WO)), 10, shuffle=False)
    losses = []
    hist = fit(mm, tr, va, epochs=2, on_step=lambda i, t, o: losses.append(float(o["loss"])) if t else None)
    assert len(losses) == 12 and np.all(np.isfinite(losses)) and len(hist["train"]) == 2
    assert _moved(model, before)


def test_fit_over_device_batches_ssd(tmp_path):
    A, hp = _A(), _hp()
    from fdet_amd.models.ModelMetaSSD import ModelMetaSSD
    from fdet_amd.models.SSD import SSD
    from fdet_amd.trainer import fit
    torch.manual_seed(0)
    bank, boxes = A.synthetic_bank(100, "cuda", seed=6, max_side=800)
    model = SSD(filters=16, input_shape=(3, HO, WO)).cuda()
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    mm = ModelMetaSSD(model=model, lr=1e-3, log_path=tmp_path / "out.log")
    tr = A.DeviceBatches(bank, boxes, 16, A.default_transform((HO, WO)), hp.SSD_PATCH_SIZES, encoder="ssd", seed=1)
    losses = []
    fit(mm, tr, None, epochs=2, on_step=lambda i, t, o: losses.append(float(o["loss"])))
    assert len(losses) == 12 and np.all(np.isfinite(losses))
    assert _moved(model, before)


def test_train_model_augment_runs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from fdet_amd import train_model
    hist = train_model.main(["--filters", "16", "--epochs", "2", "--batch-size", "4", "--steps-per-epoch", "3",
                             "--val-steps", "1", "--augment"])
    assert len(hist["train"]) == 2 and np.isfinite(float(hist["train"][-1]["loss"]))
