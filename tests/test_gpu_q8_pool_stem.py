"""GPU checks of Int8PoolResnet's integer stem (csrc/fdet_stem_q8.hip: k_stem10_q8; quantize.py, stem="integer") against the
numpy restatements tests/q8_pool_stem_cpu_ref.py and tests/q8_cpu_ref.py.  The arithmetic is integer with one-rounding float
steps, so every int8 comparison is equality.  Every kernel call writes into a buffer pre-filled with 0x55: the halo and the 256
bytes past the tensor must still be 0x55 afterwards."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_pool_stem_cpu_ref as RP  # noqa: E402

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


def _run_stem(x, w_q, b_q, mul, offset=0):
    """The kernel on numpy inputs into a buffer filled with 0x55: returns the interior; the halo must still be 0x55 and nothing
    may be written past the tensor.  offset: the frames start that many bytes into their allocation."""
    hp = _hp()
    N, _, H, W = x.shape
    F_ = w_q.shape[0]
    Ho, Wo = RP.out_hw(H, W)
    nbytes = hp.q8_act_bytes(N, F_, Ho, Wo)
    store = torch.zeros(nbytes + 256, dtype=torch.int8, device="cuda")
    out = hp.Q8Tensor(N, F_, Ho, Wo, "cuda", storage=store)
    store.fill_(FILL)
    frames = torch.zeros(x.size + offset, dtype=torch.uint8, device="cuda")[offset:].view(x.shape)
    frames.copy_(torch.from_numpy(x))
    assert frames.data_ptr() % 16 == offset % 16
    hp.stem10_fwd_q8_u8(frames, hp.q8_pack_stem10_weights(torch.from_numpy(w_q).cuda()),
                        torch.from_numpy(b_q).cuda(), torch.from_numpy(mul).cuda(), out)
    torch.cuda.synchronize()
    v = _view(out).clone()
    assert bool((store[nbytes:] == FILL).all()), "the stem wrote past the tensor"
    got = out.nchw().cpu().numpy()
    v[:, 1:-1, 1:-1, :] = FILL
    assert bool((v == FILL).all()), "the stem wrote into the halo"
    return got


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.int8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ"


# ------------------------------------------------------------------------------------------------------- stem: lane map
@pytest.mark.parametrize("rnd", range(5))
def test_stem_one_hot_taps(rnd):
    """Weight 127 at one tap per output channel: in round r channel co carries tap (64 r + co) % 300 of the flattened
    (ci, ky, kx), so the five rounds cover all 300 taps; bias and multiplier differ from channel to channel; a random frame of
    14 x 134 (two output rows, 17 columns).  A wrong tap, K row, lane group, input channel or output channel order shows."""
    x = np.random.default_rng(100 + rnd).integers(0, 256, (1, 3, 14, 134)).astype(np.uint8)
    co = np.arange(64)
    w = np.zeros((64, 300), np.int8)
    w[co, (64 * rnd + co) % 300] = 127
    w = w.reshape(64, 3, 10, 10)
    b = (co * 7 - 200).astype(np.int32)
    mul = ((1.0 + co % 5) / 1024.0).astype(F32)
    want = RP.stem10_q(x, w, b, mul)
    assert len(np.unique(want)) > 100
    _same(_run_stem(x, w, b, mul), want)


def test_the_one_hot_rounds_cover_every_tap():
    assert sorted({(64 * r + co) % 300 for r in range(5) for co in range(64)}) == list(range(300))


# ------------------------------------------------------------------------------------------------------- stem: shapes
@pytest.mark.parametrize("shape", RP.SHAPES, ids=["x".join(map(str, s)) for s in RP.SHAPES])
def test_stem_equals_the_restatement(shape):
    x, w, b, mul = RP.make_case(shape)
    want = RP.stem10_q(x, w, b, mul)
    sat = float(np.mean(np.abs(want.astype(np.int32)) == 127))
    assert 0.005 <= sat <= 0.5, sat
    _same(_run_stem(x, w, b, mul), want)


# The kernel reads a row in one of three ways: 16-byte loads (W % 16 == 0 and a 16-byte aligned frame pointer), dwords
# (W % 4 == 0, 4-byte aligned), bytes (everything else; the six shapes above).  (N, F, H, W, byte offset of the frames):
ALIGNED = [(1, 64, 6, 16, 0), (2, 64, 22, 144, 0), (1, 64, 38, 528, 0), (1, 128, 14, 136, 0), (1, 64, 14, 144, 4), (1, 64, 14, 144, 3)]


@pytest.mark.parametrize("case", ALIGNED, ids=["x".join(map(str, c[:4])) + f"+{c[4]}" for c in ALIGNED])
def test_stem_row_read_paths(case):
    """16-byte path: one window; two images of 3 x 18 outputs; two column segments with two row groups.  Dword path by the
    width and by the pointer; byte path by the pointer."""
    x, w, b, mul = RP.make_case(case[:4])
    want = RP.stem10_q(x, w, b, mul)
    sat = float(np.mean(np.abs(want.astype(np.int32)) == 127))
    assert 0.005 <= sat <= 0.5, sat
    _same(_run_stem(x, w, b, mul, offset=case[4]), want)


def test_stem_extremes():
    # all-255 frames, all +-127 weights, a multiplier that saturates: both clamps, and -128 never
    x = np.full((1, 3, 14, 134), 255, np.uint8)
    w = np.full((64, 3, 10, 10), 127, np.int8)
    w[1::2] = -127
    b = np.zeros(64, np.int32)
    mul = np.ones(64, F32)
    got = _run_stem(x, w, b, mul)
    _same(got, RP.stem10_q(x, w, b, mul))
    assert (got[:, 0::2] == 127).all() and (got[:, 1::2] == -127).all()
    # all-zero frames: the bias alone (the folded constant cancels exactly)
    x0 = np.zeros((2, 3, 14, 134), np.uint8)
    _, w, b, mul = RP.make_case((2, 64, 14, 134))
    got = _run_stem(x0, w, b, mul)
    _same(got, RP.stem10_q(x0, w, b, mul))
    assert np.array_equal(got[0, :, 1, 1], R.rint_clamp(b.astype(F32) * mul))


def test_stem_rounds_ties_to_even():
    """mul = 0.5 and small accumulators (sparse unit weights on frames of 0 / 1): every odd accumulator is an exact tie."""
    rng = np.random.default_rng(78)
    xt = rng.integers(0, 2, (1, 3, 14, 134)).astype(np.uint8)
    wt = (rng.integers(-1, 2, (64, 3, 10, 10)) * (rng.random((64, 3, 10, 10)) < 0.5)).astype(np.int8)
    bt = rng.integers(-9, 10, 64).astype(np.int32)
    half = np.full(64, 0.5, F32)
    t = RP.stem10_acc(xt, wt, bt).astype(F32) * F32(0.5)
    assert float(np.mean(np.abs(t - np.floor(t)) == 0.5)) > 0.2
    _same(_run_stem(xt, wt, bt, half), RP.stem10_q(xt, wt, bt, half))


# ------------------------------------------------------------------------------------------------------- small models
SIZE, S_SMALL = 160, 5                                       # 160 x 160 frames: a 20 x 20 stem output, pooled once to 10 x 10, S = 5


def _float_scales(P, x, S):
    """abs-max scales from a torch fp32 forward on the CPU (s_h[0] from the float stem's output, as calibrate does)."""
    nb = sum(1 for k in P if k.startswith("residual_blocks.") and k.endswith(".conv1.weight"))
    with torch.no_grad():
        h = F.conv2d(x, P["conv1.weight"], P["conv1.bias"], stride=8, padding=2)
        hs, as_ = [], []
        for k in range(nb):
            n = f"residual_blocks.{k}"
            hs.append(h)
            a = F.leaky_relu(F.conv2d(h, P[n + ".conv1.weight"], P[n + ".conv1.bias"], padding=1), 0.2)
            as_.append(a)
            e = F.leaky_relu(F.conv2d(a, P[n + ".conv2.weight"], P[n + ".conv2.bias"], padding=1), 0.2) + h
            h = F.max_pool2d(e, 2) if e.shape[2] > 2 * S else e
        hs.append(h)

    def scale(t):
        v = float(t.abs().max())
        return F32(1.0) if v == 0.0 else F32(v) / F32(127.0)
    return [scale(t) for t in hs], [scale(t) for t in as_]


@pytest.fixture(scope="module")
def small():
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.quantize import QuantParams
    torch.manual_seed(51)
    model = PoolResnet(64, (3, SIZE, SIZE), S_SMALL, num_of_residual_blocks=3).eval()
    frames = torch.randint(0, 256, (2, 3, SIZE, SIZE), dtype=torch.uint8, generator=torch.Generator().manual_seed(52))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    qp = QuantParams(*_float_scales(P, frames.float() / 255.0, S_SMALL))
    return model.cuda(), frames, {k: v.numpy() for k, v in P.items()}, qp


def _check_against_restatement(m8, P, frames, S):
    q0, outs, y = RP.model_q(frames.numpy(), P, m8.qparams.s_h, m8.qparams.s_a, S)
    tr = m8.trace(frames.cuda())
    assert tr["stem"].dtype == torch.int8 and np.array_equal(tr["stem"].cpu().numpy(), q0), "stem"
    assert len(tr["blocks"]) == len(outs)
    for k, (got, want) in enumerate(zip(tr["blocks"], outs)):
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want), f"block {k}"
    assert float((tr["y"].cpu() - y).abs().max()) <= 1e-4
    return tr


def test_small_model_equals_the_restatement_and_has_one_input_rule(small):
    from fdet_amd.quantize import Int8PoolResnet
    model, frames, P, qp = small
    m8 = Int8PoolResnet(model, qp, stem="integer")
    assert m8.stem == "integer" and m8.h0 == 20 and [h for h, _ in m8.lv] == [20, 10, 10]
    assert m8.counters == {"chain": 0, "layers": 0, "stem_q8": 0, "stem_f32": 0}
    tr = _check_against_restatement(m8, P, frames, S_SMALL)
    assert m8.counters["stem_q8"] == 1
    # uint8 frames, float frames 0..255, float images in [0,1] built from those bytes: one kernel, one set of bytes
    dev = frames.cuda()
    y = m8.forward_frames(dev)
    assert torch.equal(y, tr["y"]) and m8.counters["stem_q8"] == 2
    assert torch.equal(m8.forward_frames(dev.float()), y) and m8.counters["stem_q8"] == 3
    assert torch.equal(m8(dev.float() / 255.0), y) and m8.counters["stem_q8"] == 4
    assert torch.equal(m8(_hp().u8_to_f32_norm(dev)), y) and m8.counters["stem_q8"] == 5
    # frames of another size take the resize route to the same kernel
    other = torch.randint(0, 256, (2, 3, 120, 200), dtype=torch.uint8, generator=torch.Generator().manual_seed(53)).cuda()
    y2 = m8.forward_frames(other)
    assert tuple(y2.shape) == (2, 5, S_SMALL, S_SMALL) and bool(torch.isfinite(y2).all()) and m8.counters["stem_q8"] == 6
    assert m8.counters["stem_f32"] == 0


def test_float_stem_stays_the_default_and_keeps_its_bytes(small):
    from fdet_amd.quantize import Int8PoolResnet
    model, frames, _, qp = small
    dev = frames.cuda()
    base = Int8PoolResnet(model, qp)
    named = Int8PoolResnet(model, qp, stem="float")
    assert base.stem == named.stem == "float"
    ya, yb = base.forward_frames(dev), named.forward_frames(dev)
    assert torch.equal(ya, yb) and base.counters == named.counters
    ta, tb = base.trace(dev), named.trace(dev)
    assert ta["stem"].dtype == torch.float32 and torch.equal(ta["stem"], tb["stem"]) and torch.equal(ta["y"], tb["y"])
    assert all(torch.equal(a, b) for a, b in zip(ta["blocks"], tb["blocks"]))


def test_wide_model_runs_with_the_integer_stem():
    """F = 128: the integer stem takes it (two channel blocks); the trunk keeps its per-conv launches."""
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.quantize import Int8PoolResnet, QuantParams
    torch.manual_seed(5)
    model = PoolResnet(128, (3, SIZE, SIZE), S_SMALL, num_of_residual_blocks=2).eval()
    frames = torch.randint(0, 256, (2, 3, SIZE, SIZE), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    qp = QuantParams(*_float_scales(P, frames.float() / 255.0, S_SMALL))
    m8 = Int8PoolResnet(model.cuda(), qp, stem="integer")
    assert not m8.chain_on()
    _check_against_restatement(m8, {k: v.numpy() for k, v in P.items()}, frames, S_SMALL)
    assert m8.counters == {"chain": 0, "layers": 1, "stem_q8": 1, "stem_f32": 0}


# ------------------------------------------------------------------------------------------------------- the trained archive
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
    m8 = model.quantize([images[:2].cuda(), images[2:].cuda()], stem="integer")       # calibrate + Int8PoolResnet(stem="integer")
    assert type(m8) is Int8PoolResnet and m8.stem == "integer" and m8.qparams == calibrate(model, [images[:2].cuda(), images[2:].cuda()])
    return m8, {k: v.numpy() for k, v in P.items()}, images, g


def test_network_equals_the_restatement_on_the_trained_archive(trained):
    m8, P, images, g = trained
    tr = _check_against_restatement(m8, P, images, 10)
    assert tuple(tr["stem"].shape) == (3, 64, 60, 60) and [int(b.shape[2]) for b in tr["blocks"]] == [30, 15] + [15] * 8
    y = m8.forward_frames(images.cuda())
    assert torch.equal(y, tr["y"]) and torch.equal(m8(images.cuda().float() / 255.0), y)
    assert torch.equal((y[:, 0] > 0.7).cpu(), g["y"][:, 0] > 0.7)
    d = (y.cpu() - g["y"]).abs()
    print(f"g16, integer stem, on the GPU: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}")
    assert m8.counters["stem_f32"] == 0


def test_graphed_predict_replay_equals_eager(trained):
    m8, _, images, _ = trained
    frames = images.cuda()
    eager = m8.non_max_suppression(m8.forward_frames(frames))
    gp = m8.graphed_predict(frames[[2, 2, 2]])
    out = gp(frames)
    assert len(out) == len(eager) == 3 and sum(int(o.shape[0]) for o in eager) >= 2
    for a, b in zip(out, eager):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b.cpu())


def test_tiled_detector_windows_reach_the_integer_stem(trained):
    from fdet_amd.datasets import augment as A
    from fdet_amd.tiling import TiledDetector
    m8, _, images, _ = trained
    hwc = images.numpy().transpose(0, 2, 3, 1)
    wide = np.concatenate([hwc[0], hwc[1]], axis=1)                          # 480 x 960: two tiles
    bank = A.DeviceImageBank.from_arrays([wide, hwc[2]], "cuda")
    det = TiledDetector(m8, tile_sizes=(480,), overlap=0.0, include_whole=False, edge_margin=0.0, max_out=100)
    before = m8.counters["stem_q8"]
    rows, counts = det.detect(bank, [0, 1])
    # (frames 0 and 1 carry the archive's faces; frame 2 has no cell above 0.7 in the reference either)
    assert tuple(rows.shape[::2]) == (2, 5) and counts.cpu().tolist()[0] >= 2
    assert bool(torch.isfinite(rows).all())
    assert m8.counters["stem_q8"] > before and m8.counters["stem_f32"] == 0
