"""GPU checks of Int8Resnet (csrc/fdet_stem_q8.hip, quantize.py) against the numpy restatements tests/q8_resnet_cpu_ref.py and
tests/q8_cpu_ref.py.  The arithmetic is integer with one-rounding float steps, so every int8 comparison is equality."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_resnet_cpu_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FILL = 0x55


def _hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def _view(t):
    N, C, H, W = t.shape
    return t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)


def _to_q8(a):
    """numpy int8 (N,C,H,W) -> Q8Tensor, the layout built with torch."""
    t = _hp().Q8Tensor(*a.shape, "cuda")
    _view(t)[:, 1:-1, 1:-1, :] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return t


def _run_stem(x, w_q, b_q, mul):
    """The kernel on numpy inputs into a buffer filled with 0x55: returns the interior; the halo must still be 0x55 and nothing
    may be written past the tensor."""
    hp = _hp()
    N, _, H, W = x.shape
    F_ = w_q.shape[0]
    nbytes = hp.q8_act_bytes(N, F_, H // 2, W // 2)
    store = torch.zeros(nbytes + 256, dtype=torch.int8, device="cuda")
    out = hp.Q8Tensor(N, F_, H // 2, W // 2, "cuda", storage=store)
    store.fill_(FILL)
    hp.stem3_fwd_q8_u8(torch.from_numpy(x).cuda(), hp.q8_pack_stem_weights(torch.from_numpy(w_q).cuda()),
                       torch.from_numpy(b_q).cuda(), torch.from_numpy(mul).cuda(), out)
    torch.cuda.synchronize()
    v = _view(out).clone()
    assert bool((store[nbytes:] == FILL).all())
    got = out.nchw().cpu().numpy()
    v[:, 1:-1, 1:-1, :] = FILL
    assert bool((v == FILL).all()), "the stem wrote into the halo"
    return got


def _stem_case(seed, N, F_, H, W):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (N, 3, H, W)).astype(np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    w = rng.integers(-127, 128, (F_, 3, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, F_).astype(np.int32)
    mul = np.exp2(rng.uniform(-11.5, -8.5, F_)).astype(F32)
    return x, w, b, mul


# ------------------------------------------------------------------------------------------------------- stem: lane map
@pytest.mark.parametrize("tap", range(27))
def test_stem_one_hot_taps(tap):
    """Weight 127 at one tap per output channel: tap (c0, ky, kx) with the input channel rotated by the output channel,
    ci = (c0 + co) % 3 (ci = co % 3 for c0 = 0), a multiplier that differs from channel to channel, random frames of 12 x 36.
    A wrong tap, lane, input channel or output channel order shows."""
    c0, r = divmod(tap, 9)
    ky, kx = divmod(r, 3)
    x = np.random.default_rng(100 + tap).integers(0, 256, (1, 3, 12, 36)).astype(np.uint8)
    w = np.zeros((64, 3, 3, 3), np.int8)
    co = np.arange(64)
    w[co, (c0 + co) % 3, ky, kx] = 127
    b = (co * 7 - 200).astype(np.int32)
    mul = ((1.0 + co % 5) / 1024.0).astype(F32)
    want = RR.stem3_q(x, w, b, mul)
    assert len(np.unique(want)) > 60
    got = _run_stem(x, w, b, mul)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ"


# ------------------------------------------------------------------------------------------------------- stem: shapes
STEM_SHAPES = [(1, 64, 2, 2), (1, 64, 6, 34), (3, 64, 10, 66), (2, 128, 8, 40), (1, 64, 4, 520)]


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in STEM_SHAPES])
def test_stem_equals_the_restatement(shape):
    x, w, b, mul = _stem_case(sum(shape), *shape)
    want = RR.stem3_q(x, w, b, mul)
    sat = float(np.mean(np.abs(want.astype(np.int32)) == 127))
    assert 0.005 <= sat <= 0.5, sat
    got = _run_stem(x, w, b, mul)
    assert got.shape == want.shape and got.dtype == np.int8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ"


def test_stem_extremes_and_ties():
    # all-255 frames, all +-127 weights, a multiplier that saturates: both clamps, and -128 never
    x = np.full((1, 3, 8, 40), 255, np.uint8)
    w = np.full((64, 3, 3, 3), 127, np.int8)
    w[1::2] = -127
    b = np.zeros(64, np.int32)
    mul = np.ones(64, F32)
    got = _run_stem(x, w, b, mul)
    assert np.array_equal(got, RR.stem3_q(x, w, b, mul))
    assert (got[:, 0::2] == 127).all() and (got[:, 1::2] == -127).all()
    # all-zero frames: the bias alone (the folded constant cancels exactly)
    x0 = np.zeros((2, 3, 6, 34), np.uint8)
    _, w, b, mul = _stem_case(77, 2, 64, 6, 34)
    got = _run_stem(x0, w, b, mul)
    assert np.array_equal(got, RR.stem3_q(x0, w, b, mul))
    assert np.array_equal(got[0, :, 1, 1], R.rint_clamp(b.astype(F32) * mul))
    # exact ties: mul = 0.5, small odd accumulators (sparse unit weights on frames of 0 / 1)
    rng = np.random.default_rng(78)
    xt = rng.integers(0, 2, (1, 3, 8, 40)).astype(np.uint8)
    wt = (rng.integers(-1, 2, (64, 3, 3, 3)) * (rng.random((64, 3, 3, 3)) < 0.5)).astype(np.int8)
    bt = rng.integers(-9, 10, 64).astype(np.int32)
    half = np.full(64, 0.5, F32)
    t = RR.stem3_acc(xt, wt, bt).astype(F32) * F32(0.5)
    assert float(np.mean(np.abs(t - np.floor(t)) == 0.5)) > 0.2
    assert np.array_equal(_run_stem(xt, wt, bt, half), RR.stem3_q(xt, wt, bt, half))


# ------------------------------------------------------------------------------------------------------- conv: wide maps
@pytest.mark.parametrize("shape,skip,pool", [((1, 64, 6, 83), False, False), ((1, 64, 4, 130), True, True)], ids=["6x83-plain", "4x130-skip-pool"])
def test_conv_on_resnet_map_widths(shape, skip, pool):
    """fdet_q8_conv3x3 beyond the 60 columns of the PoolResnet cases: several column tiles, a partial last tile."""
    hp = _hp()
    rng = np.random.default_rng(sum(shape))
    N, C, H, W = shape
    x = rng.integers(-127, 128, shape).astype(np.int8)
    w = rng.integers(-127, 128, (C, C, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, C).astype(np.int32)
    mul = np.exp2(rng.uniform(-13.0, -9.5, C) if pool else rng.uniform(-12.0, -8.0, C)).astype(F32)
    sk = rng.integers(-127, 128, shape).astype(np.int8) if skip else None
    want = R.conv3x3(x, w, b, mul, sk, F32(0.75) if skip else None, pool)
    y = hp.Q8Tensor(N, C, H // 2, W // 2, "cuda") if pool else hp.Q8Tensor(N, C, H, W, "cuda")
    hp.q8_conv3x3(_to_q8(x), hp.q8_pack_weights(torch.from_numpy(w).cuda()), torch.from_numpy(b).cuda(), torch.from_numpy(mul).cuda(),
                  y, skip=_to_q8(sk) if skip else None, skip_mul=0.75 if skip else 0.0, pool=pool)
    torch.cuda.synchronize()
    v = _view(y)
    assert not bool(v[:, 0].any() or v[:, -1].any() or v[:, :, 0].any() or v[:, :, -1].any())
    assert np.array_equal(y.nchw().cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------- small models
def _small_model(size, S, nb, seed):
    from fdet_amd.models.Resnet import Resnet
    torch.manual_seed(seed)
    model = Resnet(64, (3, size, size), S, num_of_residual_blocks=nb).cuda().eval()
    frames = torch.randint(0, 256, (2, 3, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed + 1))
    return model, frames


def _check_against_restatement(m8, model, frames, S):
    P = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    q0, outs, y = RR.model_q(frames.numpy(), P, m8.qparams.s_h, m8.qparams.s_a, S)
    tr = m8.trace(frames.cuda())
    assert tr["stem"].dtype == torch.int8 and np.array_equal(tr["stem"].cpu().numpy(), q0), "stem"
    assert len(tr["blocks"]) == len(outs)
    for k, (got, want) in enumerate(zip(tr["blocks"], outs)):
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want), f"block {k}"
    assert float((tr["y"].cpu() - y).abs().max()) <= 1e-4
    return tr


def _scales_follow_torch(model, frames, qp, S):
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    hs, as_, _ = RR.float_intermediates(P, frames.float() / 255.0, S)
    s_h, s_a = RR.absmax_scales(hs, as_)
    assert np.allclose(qp.s_h, s_h, rtol=1e-4, atol=0) and np.allclose(qp.s_a, s_a, rtol=1e-4, atol=0)


def test_small_model_with_a_chained_tail(monkeypatch):
    """64 x 64 frames, S = 4, five blocks: 32 -> 16 -> 8 -> 4 pooled, then two blocks at 4 x 4 as one fdet_q8_chain launch."""
    from fdet_amd.quantize import Int8Resnet
    model, frames = _small_model(64, 4, 5, 31)
    monkeypatch.delenv("FDET_Q8_CHAIN", raising=False)
    m8 = model.quantize([frames.cuda()])
    assert type(m8) is Int8Resnet and [h for h, _ in m8.lv] == [32, 16, 8, 4, 4] and m8.chain_on()
    _scales_follow_torch(model, frames, m8.qparams, 4)
    tr = _check_against_restatement(m8, model, frames, 4)
    assert m8.counters["chain"] == 1 and m8.counters["layers"] == 0 and m8.counters["stem_q8"] == 1
    monkeypatch.setenv("FDET_Q8_CHAIN", "0")
    m0 = Int8Resnet(model, m8.qparams)
    t0 = m0.trace(frames.cuda())
    assert m0.counters["chain"] == 0 and m0.counters["layers"] == 1
    assert torch.equal(t0["stem"], tr["stem"]) and torch.equal(t0["y"], tr["y"])
    assert all(torch.equal(a, b) for a, b in zip(t0["blocks"], tr["blocks"]))


def test_small_model_with_a_20x20_tail():
    """80 x 80 frames, S = 20, three blocks: 40 pooled, then two blocks at 20 x 20, wider than the chain takes: per-conv
    launches."""
    model, frames = _small_model(80, 20, 3, 41)
    m8 = model.quantize([frames.cuda()])
    assert [h for h, _ in m8.lv] == [40, 20, 20] and not m8.chain_on()
    _scales_follow_torch(model, frames, m8.qparams, 20)
    _check_against_restatement(m8, model, frames, 20)
    assert m8.counters["layers"] == 1 and m8.counters["chain"] == 0


# ------------------------------------------------------------------------------------------------------- the trained archive
@pytest.fixture(scope="module")
def trained(golden):
    from fdet_amd.models.Resnet import Resnet
    from fdet_amd.quantize import Int8Resnet, calibrate
    g = RR.load_g22()
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    model = Resnet(filters=64, input_shape=(3, 480, 480), num_of_patches=15, probability_threshold=0.7, iou_threshold=0.01)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().eval()
    images = golden("g6_trained_small")["images"]
    qp = calibrate(model, [images[:2].cuda(), images[2:].cuda()])
    return model, Int8Resnet(model, qp), qp, P, images, g


def test_calibration_reads_the_float_engine_on_strip_maps(trained):
    """abs-max scales from the engine's saved intermediates (column strips at 240 and 120 columns) against torch fp32 on the
    CPU, 1e-4 relative as for PoolResnet; the float model's output is what it was."""
    model, _, qp, P, images, g = trained
    assert qp.images_seen == 3 and qp.method == "absmax" and qp.num_blocks == 10
    _scales_follow_torch(model, images, qp, 15)
    with torch.no_grad():
        y = model(images[:2].cuda().float() / 255.0)
    assert torch.allclose(y.cpu(), g["y"][:2], atol=1e-4)


def test_network_equals_the_restatement_on_the_trained_archive(trained):
    model, m8, qp, P, images, g = trained
    tr = _check_against_restatement(m8, model, images, 15)
    assert tuple(tr["stem"].shape) == (3, 64, 240, 240) and [int(b.shape[2]) for b in tr["blocks"]] == [120, 60, 30, 15] + [15] * 6
    assert m8.chain_on() and m8.counters["chain"] == 1
    # one arithmetic for every input: frames, float images, predict=1
    y = m8.forward_frames(images.cuda())
    assert torch.equal(y, tr["y"])
    assert torch.equal(m8(_hp().u8_to_f32_norm(images.cuda())), y)
    assert torch.equal(m8(images.cuda().float() / 255.0), y)
    det = m8(images[:2].cuda(), predict=torch.tensor(1))
    rows, counts = m8.reduce_bounding_boxes.forward_batch(y[:2])
    assert int(counts[0]) >= 1 and torch.equal(det, rows[0, :int(counts[0])])
    per_image = m8.non_max_suppression(y)
    assert len(per_image) == 3 and torch.equal(per_image[0], det)
    d = (y.cpu() - g["y"]).abs()
    print(f"g22 on the GPU: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}")


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


def test_tiled_detector_runs_on_the_int8_model(trained):
    from fdet_amd.datasets import augment as A
    from fdet_amd.tiling import TiledDetector
    _, m8, _, _, images, _ = trained
    hwc = images.numpy().transpose(0, 2, 3, 1)
    wide = np.concatenate([hwc[0], hwc[1]], axis=1)                          # 480 x 960: two tiles
    bank = A.DeviceImageBank.from_arrays([wide, hwc[2]], "cuda")
    det = TiledDetector(m8, tile_sizes=(480,), overlap=0.0, include_whole=False, edge_margin=0.0, max_out=100)
    rows, counts = det.detect(bank, [0, 1])
    assert tuple(rows.shape[::2]) == (2, 5) and counts.cpu().tolist()[0] >= 2 and counts.cpu().tolist()[1] >= 1
    assert bool(torch.isfinite(rows).all())


def test_frames_of_another_size_take_the_resize_route(trained):
    _, m8, _, _, images, _ = trained
    before = m8.counters["stem_q8"]
    frames = torch.randint(0, 256, (2, 3, 300, 400), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda()
    y = m8.forward_frames(frames)
    assert tuple(y.shape) == (2, 5, 15, 15) and bool(torch.isfinite(y).all()) and m8.counters["stem_q8"] == before + 1
    small = F.interpolate(images[:1].float(), size=(240, 240), mode="bilinear", align_corners=False)      # float frames 0..255
    y2 = m8.forward_frames(small.cuda())
    assert tuple(y2.shape) == (1, 5, 15, 15) and bool(torch.isfinite(y2).all())
    # the codes of a float image: NaN -> 0, values beyond [0, 1] clamp, uint8 / 255 recovers the bytes
    ramp = torch.arange(256, dtype=torch.uint8).cuda()
    assert torch.equal(m8._codes(_hp().u8_to_f32_norm(ramp)), ramp) and torch.equal(m8._codes(ramp.float() / 255.0), ramp)
    odd = torch.tensor([float("nan"), -1.0, 2.0, float("inf"), float("-inf"), 0.4 / 255.0, 1.6 / 255.0]).cuda()
    assert m8._codes(odd).tolist() == [0, 0, 255, 255, 0, 0, 2]
