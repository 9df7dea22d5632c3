"""GPU checks of the int8 inference path (csrc/fdet_q8.hip, quantize.py) against the numpy restatement tests/q8_cpu_ref.py.
The arithmetic is integer with one-rounding float steps, so every comparison is equality."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def _to_q8(a, out=None):
    """numpy int8 (N,C,H,W) -> Q8Tensor, the layout built with torch (not with the kernel under test)."""
    hp = _hp()
    N, C, H, W = a.shape
    t = out if out is not None else hp.Q8Tensor(N, C, H, W, "cuda")
    assert t.shape == (N, C, H, W)
    v = t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)
    v[:, 1:-1, 1:-1, :] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return t


def _halo_is_zero(t):
    N, C, H, W = t.shape
    v = t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)
    return not bool(v[:, 0].any() or v[:, -1].any() or v[:, :, 0].any() or v[:, :, -1].any())


def _run_conv(d, x=None, y=None, skip=None):
    hp = _hp()
    N, C, H, W = d["shape"]
    x = _to_q8(d["x"], x)
    skip = _to_q8(d["skip"], skip) if d["skip"] is not None else None
    if y is None:
        y = hp.Q8Tensor(N, C, H // 2, W // 2, "cuda") if d["pool"] else hp.Q8Tensor(N, C, H, W, "cuda")
    wpk = hp.q8_pack_weights(torch.from_numpy(d["w"]).cuda())
    hp.q8_conv3x3(x, wpk, torch.from_numpy(d["b"]).cuda(), torch.from_numpy(d["mul"]).cuda(), y, skip=skip,
                  skip_mul=float(d["skip_mul"]) if skip is not None else 0.0, pool=d["pool"], slope=d.get("slope", 0.2))
    torch.cuda.synchronize()
    assert _halo_is_zero(y)
    return y.nchw().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(idx):
    d = R.make_case(idx)
    return d, R.conv3x3(d["x"], d["w"], d["b"], d["mul"], d["skip"], d["skip_mul"], d["pool"])


# ------------------------------------------------------------------------------------------------------- lane map
def _one_hot_input():
    """5x5, 64 channels: at every position the 64 channels differ, in every channel the 25 positions differ (7 and 29 are
    units modulo 255), values over the whole range -127..127."""
    c = np.arange(64)[:, None, None]
    p = (np.arange(5)[:, None] * 5 + np.arange(5)[None, :])[None]
    return ((7 * c + 29 * p) % 255 - 127).astype(np.int8)[None]


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_weights_shift_and_permute(tap):
    """w[co][ci][ky][kx] = (ci == (5 co + 3) % 64 and (ky, kx) == tap), mul 1, bias 0, slope 1 (so that negative values keep
    their identity too): the output is the input shifted by the tap and permuted over the channels, value for value over
    the whole range -127..127.  The pattern is asymmetric in co / ci, in the position inside a 16-channel run and in the tap,
    so a transposed operand, a wrong k order or a wrong tap order shows."""
    ky, kx = divmod(tap, 3)
    x = _one_hot_input()
    w = np.zeros((64, 64, 3, 3), np.int8)
    perm = (5 * np.arange(64) + 3) % 64
    w[np.arange(64), perm, ky, kx] = 1
    d = dict(shape=(1, 64, 5, 5), pool=False, x=x, w=w, b=np.zeros(64, np.int32), mul=np.ones(64, F32), skip=None, skip_mul=None,
             slope=1.0)
    got = _run_conv(d)
    xp = np.zeros((1, 64, 7, 7), np.int8)
    xp[:, :, 1:-1, 1:-1] = x
    want = xp[:, perm, ky:ky + 5, kx:kx + 5]
    assert np.array_equal(got, want)
    assert np.array_equal(want, R.conv3x3(x, w, d["b"], d["mul"], slope=F32(1.0)))      # (the restatement says the same)


# ------------------------------------------------------------------------------------------------------- random cases
@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=[f"{c[0]}-{c[3]}" for c in R.CASES])
def test_conv_equals_the_restatement(idx):
    d, want = _case(idx)
    got = _run_conv(d)
    assert got.shape == want.shape and got.dtype == np.int8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ"


# ------------------------------------------------------------------------------------------------------- converters
@pytest.mark.parametrize("shape", sorted({c[0] for c in R.CASES}))
def test_quantize_and_dequantize(shape):
    hp = _hp()
    rng = np.random.default_rng(sum(shape))
    s = F32(0.0625)                                                        # a power of two: k + 0.5 steps are exact ties
    x = (rng.standard_normal(shape) * 3.0).astype(F32)                     # about 1 % beyond +-127 s = 7.94
    flat = x.reshape(-1)
    k = rng.integers(-130, 130, flat.size // 3)
    flat[::3][:k.size] = ((k + 0.5) * s).astype(F32)                        # exact ties, some beyond the range
    flat[0] = np.nan
    flat[-1] = np.inf
    flat[flat.size // 2] = -1e30
    want = R.quantize(x, s)
    assert want.min() == -127 and want.max() == 127 and want.reshape(-1)[0] == 0
    q = hp.q8_quantize(torch.from_numpy(x).cuda(), float(s))
    assert _halo_is_zero(q)
    assert np.array_equal(q.nchw().cpu().numpy(), want)
    assert np.array_equal(_to_q8(want).storage.cpu().numpy(), q.storage.cpu().numpy())       # the layout, halo included
    # a scale that is no power of two: x * (1.0f / s), not x / s
    s3 = F32(0.0437)
    assert np.array_equal(hp.q8_quantize(torch.from_numpy(x).cuda(), float(s3)).nchw().cpu().numpy(), R.quantize(x, s3))
    back = hp.q8_dequantize(q, float(s3)).cpu().numpy()
    assert back.dtype == np.float32 and np.array_equal(back, R.dequantize(want, s3))
    # a scale whose reciprocal overflows: 0 * inf is a NaN product -> 0, everything else saturates
    tiny = F32(1e-40)
    xs = x.copy()
    xs.reshape(-1)[1:4] = (0.0, -0.0, 1e-30)
    assert np.array_equal(hp.q8_quantize(torch.from_numpy(xs).cuda(), float(tiny)).nchw().cpu().numpy(), R.quantize(xs, tiny))
    # scale 1 carries exact integers in and out
    ints = rng.integers(-127, 128, shape).astype(np.int8)
    q1 = hp.q8_quantize(torch.from_numpy(ints.astype(F32)).cuda(), 1.0)
    assert np.array_equal(q1.nchw().cpu().numpy(), ints)
    assert np.array_equal(hp.q8_dequantize(q1, 1.0).cpu().numpy(), ints.astype(F32))


# ------------------------------------------------------------------------------------------------------- recycled buffers
def test_recycled_buffers_keep_a_zero_halo():
    """A large map, then a smaller one in the same allocations (Q8Tensor.reshape_ zero-fills when the shape changes), then
    the same shape again over a dirty interior (nothing is cleared: producers write real pixels only)."""
    hp = _hp()
    big, want_big = _case(6)                                               # (1,64,30,30) pooled with skip
    x, sk = hp.Q8Tensor(1, 64, 30, 30, "cuda"), hp.Q8Tensor(1, 64, 30, 30, "cuda")
    y = hp.Q8Tensor(1, 64, 30, 30, "cuda")                                 # larger than the pooled output needs
    y.reshape_(1, 64, 15, 15)
    assert np.array_equal(_run_conv(big, x, y, sk), want_big)
    small, want_small = _case(4)                                           # (1,64,17,5) plain
    for t in (x, y):
        t.reshape_(1, 64, 17, 5)
        assert not bool(t.storage.any())
    assert np.array_equal(_run_conv(small, x, y), want_small)
    d2 = dict(small)
    d2["x"] = np.ascontiguousarray(small["x"][:, ::-1])                    # other data, the same buffers, nothing cleared
    ptr = y.storage.data_ptr()
    assert np.array_equal(_run_conv(d2, x, y), R.conv3x3(d2["x"], d2["w"], d2["b"], d2["mul"]))
    assert y.storage.data_ptr() == ptr and _halo_is_zero(x) and _halo_is_zero(y)
    with pytest.raises(ValueError):
        y.reshape_(1, 64, 60, 60)                                          # does not fit the allocation


# ------------------------------------------------------------------------------------------------------- the trunk on g16
@pytest.fixture(scope="module")
def trained(golden):
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.quantize import Int8PoolResnet, calibrate
    g = golden("g16_trained_medium")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    model = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.7, iou_threshold=0.01)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().eval()
    images = golden("g6_trained_small")["images"]
    qp = calibrate(model, [images[:2].cuda(), images[2:].cuda()])
    return model, Int8PoolResnet(model, qp), qp, P, images, g


def test_calibration_reads_the_float_engine(trained):
    """abs-max scales from the engine's saved intermediates against torch fp32 on the CPU: the engine is fp32-grade
    (bf16x3, ~1e-5 relative), the scales agree to 1e-4 relative."""
    model, m8, qp, P, images, _ = trained
    assert qp.images_seen == 3 and qp.method == "absmax" and qp.num_blocks == 10
    x = images.float() / 255.0
    with torch.no_grad():
        h = F.conv2d(x, P["conv1.weight"], P["conv1.bias"], stride=8, padding=2)
        hs, as_ = [], []
        for k in range(10):
            n = f"residual_blocks.{k}"
            hs.append(h)
            a = F.leaky_relu(F.conv2d(h, P[n + ".conv1.weight"], P[n + ".conv1.bias"], padding=1), 0.2)
            as_.append(a)
            e = F.leaky_relu(F.conv2d(a, P[n + ".conv2.weight"], P[n + ".conv2.bias"], padding=1), 0.2) + h
            h = F.max_pool2d(e, 2) if e.shape[2] > 20 else e
        hs.append(h)
    want_h = np.array([float(t.abs().max()) / 127.0 for t in hs])
    want_a = np.array([float(t.abs().max()) / 127.0 for t in as_])
    assert np.allclose(qp.s_h, want_h, rtol=1e-4, atol=0) and np.allclose(qp.s_a, want_a, rtol=1e-4, atol=0)
    # the float model is untouched by the calibration pass
    with torch.no_grad():
        y = model(x[:2].cuda())
    assert torch.allclose(y.cpu(), trained[5]["y"][:2], atol=1e-4)


def test_trunk_equals_the_restatement_on_the_trained_archive(trained):
    _, m8, qp, P, images, g = trained
    tr = m8.trace(images.cuda())
    stem = tr["stem"].cpu()
    assert tuple(stem.shape) == (3, 64, 60, 60) and len(tr["blocks"]) == 10
    outs, hd = R.trunk(stem.numpy(), {k: v.numpy() for k, v in P.items()}, qp.s_h, qp.s_a, S=10)
    for k, (got, want) in enumerate(zip(tr["blocks"], outs)):
        assert got.dtype == torch.int8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), f"block {k}"
    with torch.no_grad():
        y_ref = torch.sigmoid(F.conv2d(torch.from_numpy(hd), P["out.weight"], P["out.bias"]))
    assert float((tr["y"].cpu() - y_ref).abs().max()) <= 1e-4
    # and the model surface returns that y: frames, float images, predict=1
    y = m8.forward_frames(images.cuda())
    assert torch.equal(y, tr["y"])
    assert torch.equal(m8(_hp().u8_to_f32_norm(images.cuda())), y)          # (the exact x / 255 the frames path applies)
    assert torch.equal(y[:, 0].cpu() > 0.7, g["y"][:, 0] > 0.7)
    det = m8(images[:2].cuda(), predict=torch.tensor(1))
    rows, counts = m8.reduce_bounding_boxes.forward_batch(y[:2])
    assert int(counts[0]) >= 1 and torch.equal(det, rows[0, :int(counts[0])])
    per_image = m8.non_max_suppression(y)
    assert len(per_image) == 3 and torch.equal(per_image[0], det)


# ------------------------------------------------------------------------------------------------------- plumbing
def test_graphed_predict_replay_equals_eager(trained):
    _, m8, _, _, images, _ = trained
    frames = images.cuda()
    eager = m8.non_max_suppression(m8.forward_frames(frames))
    gp = m8.graphed_predict(frames[[2, 2, 2]])
    out = gp(frames)
    assert len(out) == len(eager) == 3 and sum(int(o.shape[0]) for o in eager) >= 2
    for a, b in zip(out, eager):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b.cpu())
    first = gp.first(frames[[1, 0, 2]])
    assert torch.equal(first.cpu(), eager[1].cpu())


def test_tiled_detector_runs_on_the_int8_model(trained):
    """A 960x960 mosaic of the stored frames and one 480x480 frame, tiles of 480 plus the whole image: the mosaic's windows are
    four crops and one window resized from 960 to 480.  The detector's rows equal the restated merge (tests/tiles_cpu_ref.py)
    of the rows that `forward_frames` gives on the gathered windows."""
    import tiles_cpu_ref as TR
    from fdet_amd.datasets import augment as A
    from fdet_amd.tiling import TiledDetector
    _, m8, _, _, images, _ = trained
    hp = _hp()
    hwc = images.numpy().transpose(0, 2, 3, 1)
    mosaic = np.zeros((960, 960, 3), np.uint8)
    for q, (x0, y0) in zip((0, 1, 2, 0), ((0, 0), (480, 0), (0, 480), (480, 480))):
        mosaic[y0:y0 + 480, x0:x0 + 480] = hwc[q]
    bank = A.DeviceImageBank.from_arrays([mosaic, hwc[1]], "cuda")
    det = TiledDetector(m8, tile_sizes=(480,), overlap=0.0, include_whole=True, edge_margin=0.0, max_out=200)
    plan = det.plan(bank.sizes)
    wins = [tuple(int(v) for v in t) for t in plan.tiles]
    assert wins[:5] == [(0, 0, 0, 960, 960), (0, 0, 0, 480, 480), (0, 480, 0, 480, 480), (0, 0, 480, 480, 480), (0, 480, 480, 480, 480)]
    assert int(plan.tile_offset[1]) == 5 and len(wins) == int(plan.tile_offset[2]) > 5
    d_tiles = torch.from_numpy(plan.tiles.view(np.uint8).copy()).cuda()
    frames = hp.tile_gather(bank.data, bank.d_table, bank.table, d_tiles, plan.tiles, (480, 480))
    assert torch.equal(frames[1].cpu(), images[0]) and not torch.equal(frames[0].cpu(), images[0])
    r, c = m8.reduce_bounding_boxes.forward_batch(m8.forward_frames(frames))
    assert int(c[1:5].sum()) >= 3                                          # the crops of frames 0, 1 and 0 again carry faces
    want, want_counts, rejected = TR.merge(r.cpu().numpy(), c.cpu().numpy(), wins, list(plan.tile_offset), bank.sizes, 480, 480,
                                           0.0, 0.01, 200)
    rows, counts = det.detect(bank, [0, 1])
    assert rejected == 0 and int(want_counts[0]) >= 2 and int(want_counts[1]) >= 1
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(rows.cpu().numpy(), want)


def test_script_calibration_equals_calibrate_on_the_same_frames(trained, capsys):
    """`bank_frames` hands `calibrate` uint8 FRAMES (0..255), which is what it preprocesses: on a bank of model-resolution
    images the scales of the scripts' path (`detect_images.quantize_loaded_model`) are those of `calibrate` on the images
    themselves -- not those of images divided by 255 twice."""
    from types import SimpleNamespace
    from fdet_amd import detect_images as D
    from fdet_amd.datasets import augment as A
    from fdet_amd.quantize import bank_frames, calibrate
    model, _, _, _, images, _ = trained
    bank = A.DeviceImageBank.from_arrays([im.numpy().transpose(1, 2, 0) for im in images], "cuda")
    batches = list(bank_frames(bank, (480, 480), batch_size=2))
    assert [tuple(b.shape) for b in batches] == [(2, 3, 480, 480), (1, 3, 480, 480)] and batches[0].dtype == torch.uint8
    assert torch.equal(torch.cat(batches).cpu(), images)                   # the resize to the images' own size is the identity
    want = calibrate(model, [images.cuda()])
    m8 = D.quantize_loaded_model(model, SimpleNamespace(calib=None, calib_images=3), bank)
    assert "calibrated on 3 images" in capsys.readouterr().out
    assert m8.qparams == want
    assert len(list(bank_frames(bank, (480, 480), max_images=2))) == 1
    dark = calibrate(model, [images.cuda().float() / 255.0])                # what the path must NOT do: a twice-divided input
    assert not np.allclose(dark.s_h, want.s_h, rtol=0.05)


def test_run_validation_epoch_reports_int8_beside_float(capsys, tmp_path, monkeypatch):
    from fdet_amd import run_validation_epoch as V
    monkeypatch.chdir(tmp_path)                                             # the script writes logs/ where it runs
    out = V.main(["--filters", "64", "--synthetic-images", "8", "--batch-size", "4", "--int8", "--calib-images", "4",
                  "--json", str(tmp_path / "curve.json")])
    text = capsys.readouterr().out
    assert "int8: calibrated on 4 images (absmax)" in text and "int8 AP@0.50:" in text and "(float " in text
    r8, r = out["int8"], out["result"]
    assert (r8.n_images, r8.n_gt) == (r.n_images, r.n_gt) == (8, r.n_gt)
    import json
    assert "int8" in json.loads((tmp_path / "curve.json").read_text())
