"""GPU checks of the int8 SSD (csrc/fdet_q8.hip and csrc/fdet_stem_q8.hip, quantize.Int8SSD) against the numpy restatement
tests/q8_ssd_cpu_ref.py.  The arithmetic is integer with one-rounding float steps, so every comparison of int8 tensors and of
the heads' fp32 z is equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_resnet_cpu_ref as RR  # noqa: E402
import q8_ssd_cpu_ref as SC  # noqa: E402
from test_q8_ssd_host import SSD_DS_MAX, SSD_DS_MEAN, SSD_DZ_MAX, SSD_DZ_MEAN  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
FILL = 0x55
TAIL = 256


def _hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def _view(t):
    N, C, H, W = t.shape
    return t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)


def _to_q8(a):
    """numpy int8 (N,C,H,W) -> Q8XTensor, the layout built with torch."""
    t = _hp().Q8XTensor(*a.shape, "cuda")
    _view(t)[:, 1:-1, 1:-1, :] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return t


def _sentinel(N, C, H, W):
    """An output tensor whose every byte, halo and TAIL bytes past the end included, is FILL."""
    t = _hp().Q8XTensor(N, C, H, W, "cuda")
    t.storage = torch.full((t.storage.numel() + TAIL,), FILL, dtype=torch.int8, device="cuda")
    return t


def _interior(t):
    """The real pixels as numpy; asserts that the halo and the bytes past the tensor are still FILL."""
    torch.cuda.synchronize()
    N, C, H, W = t.shape
    nbytes = N * (H + 2) * (W + 2) * C
    assert bool((t.storage[nbytes:] == FILL).all()), "bytes past the tensor were written"
    got = t.nchw().cpu().numpy()
    v = _view(t).clone()
    v[:, 1:-1, 1:-1, :] = FILL
    assert bool((v == FILL).all()), "the halo was written"
    return got


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(seed, N, ci, co, H, W, skip, pool=False):
    """Full-range inputs; multipliers scaled so that a few percent of the outputs saturate at any Cin."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-127, 128, (N, ci, H, W)).astype(np.int8)
    w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8)
    x.reshape(-1)[:2] = (127, -127)
    w.reshape(-1)[:2] = (-127, 127)
    b = rng.integers(-40000, 40001, co).astype(np.int32)
    lo, hi = (-13.0, -9.5) if pool else (-12.0, -8.0)
    mul = np.exp2(rng.uniform(lo, hi, co) - 0.5 * np.log2(ci / 64.0)).astype(F32)
    sk = rng.integers(-127, 128, (N, co, H, W)).astype(np.int8) if skip else None
    return x, w, b, mul, sk, (F32(0.75) if skip else None)


def _run_conv(x, w, b, mul, sk=None, sm=None, pool=False):
    hp = _hp()
    N, _, H, W = x.shape
    co = w.shape[0]
    y = _sentinel(N, co, H // 2, W // 2) if pool else _sentinel(N, co, H, W)
    hp.q8x_conv3x3(_to_q8(x), hp.q8x_pack_weights(_dev(w)), _dev(b), _dev(mul), y, skip=_to_q8(sk) if sk is not None else None,
                   skip_mul=float(sm) if sm is not None else 0.0, pool=pool)
    return _interior(y)


WIDTHS = [(16, 32), (32, 32), (32, 64), (64, 128), (128, 256), (256, 256)]
MAPS = [(1, 1), (3, 5), (7, 18)]                          # 7 x 18 crosses the 16-column tile and the 4-row group


# ------------------------------------------------------------------------------------------------------- conv
@pytest.mark.parametrize("ci,co", WIDTHS, ids=[f"{a}-{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
def test_conv_equals_the_restatement(ci, co, skip):
    for H, W in MAPS:
        x, w, b, mul, sk, sm = _case(ci + co + 10 * H + W + skip, 2, ci, co, H, W, skip)
        want = SC.conv3x3(x, w, b, mul, sk, sm)
        if H * W > 1:
            sat = float(np.mean(np.abs(want.astype(np.int32)) == 127))
            assert 0.002 <= sat <= 0.6, sat
        got = _run_conv(x, w, b, mul, sk, sm)
        assert got.shape == want.shape and np.array_equal(got, want), f"{H}x{W}: {int((got != want).sum())} of {want.size} differ"


POOLED = [((15, 15), (7, 7)), ((6, 34), (3, 17)), ((5, 3), (2, 1))]


@pytest.mark.parametrize("ci,co", [(16, 32), (32, 32), (64, 128), (256, 256)], ids=["16-32", "32-32", "64-128", "256-256"])
def test_floor_pooled_conv_equals_the_restatement(ci, co):
    """Odd maps: the last row / column takes part in no window; the output's halo and the bytes past it stay untouched."""
    for (H, W), (Ho, Wo) in POOLED:
        x, w, b, mul, sk, sm = _case(7 * ci + co + H, 2, ci, co, H, W, True, pool=True)
        want = SC.conv3x3(x, w, b, mul, sk, sm, pool=True)
        assert want.shape == (2, co, Ho, Wo)
        got = _run_conv(x, w, b, mul, sk, sm, pool=True)
        assert np.array_equal(got, want), f"{H}x{W}: {int((got != want).sum())} of {want.size} differ"
        # the skip values of an odd last row and column reach no window
        sk2 = sk.copy()
        if H & 1:
            sk2[:, :, -1, :] = 127
        if W & 1:
            sk2[:, :, :, -1] = 127
        assert np.array_equal(_run_conv(x, w, b, mul, sk2, sm, pool=True), want)


@pytest.mark.parametrize("ci", [16, 32])
@pytest.mark.parametrize("tap", range(9))
def test_conv_one_hot_taps_and_channels(ci, tap):
    """One weight per output channel, at tap (ky, kx) and at the first (even co) or last (odd co) input channel, its value
    different from channel to channel: a wrong K flattening, a wrong tap offset or a read of a zero slot's bytes shows."""
    ky, kx = divmod(tap, 3)
    co = 32
    x = np.random.default_rng(300 + tap + ci).integers(-127, 128, (1, ci, 5, 18)).astype(np.int8)
    w = np.zeros((co, ci, 3, 3), np.int8)
    for o in range(co):
        w[o, 0 if o % 2 == 0 else ci - 1, ky, kx] = 127 - 3 * o
    b = (np.arange(co) * 7 - 100).astype(np.int32)
    mul = ((1.0 + np.arange(co) % 5) / 256.0).astype(F32)
    want = SC.conv3x3(x, w, b, mul)
    assert len(np.unique(want)) > 60
    assert np.array_equal(want, SC.conv3x3_loops(x, w, b, mul))
    got = _run_conv(x, w, b, mul)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ"


def test_conv_extremes_and_ties():
    # all +-127 at Cin = 256: the largest accumulator the contract allows, 9 * 256 * 127 * 127 < 2^26
    x = np.full((1, 256, 6, 18), 127, np.int8)
    w = np.full((64, 256, 3, 3), 127, np.int8)
    w[1::2] = -127
    b = np.zeros(64, np.int32)
    mul = np.full(64, 2.0 ** -19, F32)
    got = _run_conv(x, w, b, mul)
    assert np.array_equal(got, SC.conv3x3(x, w, b, mul))
    full = 9 * 256 * 127 * 127
    assert full < 2 ** 26 and got[0, 0, 2, 5] == int(np.rint(F32(full) * F32(2.0 ** -19))) == 71
    assert got[0, 1, 2, 5] == int(np.rint(F32(-full) * F32(2.0 ** -19) * F32(0.2)))
    # a multiplier of 1: both clamps, and -128 never
    one = np.ones(64, F32)
    got = _run_conv(x, w, b, one, sk=np.full((1, 64, 6, 18), -127, np.int8), sm=F32(1.0))
    assert (got[:, 0::2] == 127).all() and (got[:, 1::2] == -127).all()
    # exact ties at Cin = 16 and 32: mul = 0.5, sparse unit weights, so every odd accumulator sits on .5
    for ci in (16, 32):
        rng = np.random.default_rng(40 + ci)
        xt = rng.integers(-3, 4, (1, ci, 7, 18)).astype(np.int8)
        wt = (rng.integers(-1, 2, (32, ci, 3, 3)) * (rng.random((32, ci, 3, 3)) < 0.05)).astype(np.int8)
        bt = rng.integers(-9, 10, 32).astype(np.int32)
        half = np.full(32, 0.5, F32)
        t = R.epilogue_float(RR.conv_acc(xt, wt, bt), half, slope=F32(1.0))
        assert float(np.mean(np.abs(t - np.floor(t)) == 0.5)) > 0.2
        assert np.array_equal(_run_conv(xt, wt, bt, half), SC.conv3x3(xt, wt, bt, half))


@pytest.mark.parametrize("C", [64, 256])
def test_conv_equals_the_existing_kernel_where_both_run(C):
    """C -> C on an even map, pooled with a skip and plain: fdet_q8x_conv3x3 and fdet_q8_conv3x3 write the same bytes, from
    the same packed weights."""
    hp = _hp()
    x, w, b, mul, sk, sm = _case(C, 2, C, C, 6, 20, True, pool=True)
    wpk = hp.q8_pack_weights(_dev(w))
    assert torch.equal(wpk, hp.q8x_pack_weights(_dev(w)))
    for pool in (True, False):
        shape = (2, C, 3, 10) if pool else (2, C, 6, 20)
        ya, yb = hp.Q8Tensor(*shape, "cuda"), hp.Q8XTensor(*shape, "cuda")
        xq, sq = hp.Q8Tensor(2, C, 6, 20, "cuda"), hp.Q8Tensor(2, C, 6, 20, "cuda")
        _view(xq)[:, 1:-1, 1:-1, :] = _dev(x.transpose(0, 2, 3, 1))
        _view(sq)[:, 1:-1, 1:-1, :] = _dev(sk.transpose(0, 2, 3, 1))
        hp.q8_conv3x3(xq, wpk, _dev(b), _dev(mul), ya, skip=sq, skip_mul=float(sm), pool=pool)
        hp.q8x_conv3x3(xq, wpk, _dev(b), _dev(mul), yb, skip=sq, skip_mul=float(sm), pool=pool)
        torch.cuda.synchronize()
        assert torch.equal(ya.storage, yb.storage)
        assert np.array_equal(yb.nchw().cpu().numpy(), SC.conv3x3(x, w, b, mul, sk, sm, pool))


@pytest.mark.parametrize("H,W,skip,pool", [(5, 18, False, False), (5, 18, True, False), (6, 18, True, True)],
                         ids=["5x18-plain", "5x18-skip", "6x18-pooled-skip"])
def test_three_chunk_conv_through_both_entries(H, W, skip, pool):
    """C = 192 is three 64-channel chunks, the only width at which the chunk walk runs an odd count above one.  18 columns
    cross the 16-column tile, 5 and 6 rows the 4-row group.  Both entries, from the same packed weights, write the same bytes,
    and these are the restatement's."""
    hp = _hp()
    C, N = 192, 2
    x, w, b, mul, sk, sm = _case(192, N, C, C, H, W, skip, pool)
    want = SC.conv3x3(x, w, b, mul, sk, sm, pool)
    sat = float(np.mean(np.abs(want.astype(np.int32)) == 127))
    assert 0.002 <= sat <= 0.6, sat
    wpk = hp.q8_pack_weights(_dev(w))
    assert torch.equal(wpk, hp.q8x_pack_weights(_dev(w)))
    shape = (N, C, H // 2, W // 2) if pool else (N, C, H, W)
    ya, yb = hp.Q8Tensor(*shape, "cuda"), hp.Q8XTensor(*shape, "cuda")
    xq = hp.Q8Tensor(N, C, H, W, "cuda")
    _view(xq)[:, 1:-1, 1:-1, :] = _dev(x.transpose(0, 2, 3, 1))
    sq = None
    if skip:
        sq = hp.Q8Tensor(N, C, H, W, "cuda")
        _view(sq)[:, 1:-1, 1:-1, :] = _dev(sk.transpose(0, 2, 3, 1))
    hp.q8_conv3x3(xq, wpk, _dev(b), _dev(mul), ya, skip=sq, skip_mul=float(sm) if skip else 0.0, pool=pool)
    hp.q8x_conv3x3(xq, wpk, _dev(b), _dev(mul), yb, skip=sq, skip_mul=float(sm) if skip else 0.0, pool=pool)
    torch.cuda.synchronize()
    assert torch.equal(ya.storage, yb.storage)
    for y in (ya, yb):
        got = y.nchw().cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ"


# ------------------------------------------------------------------------------------------------------- skip conv, head
@pytest.mark.parametrize("ci,co", [(16, 32), (32, 64), (64, 128), (128, 256), (48, 16)], ids=lambda v: str(v))
def test_pointwise_equals_the_restatement(ci, co):
    hp = _hp()
    for H, W in MAPS:
        rng = np.random.default_rng(ci + co + H)
        x = rng.integers(-127, 128, (2, ci, H, W)).astype(np.int8)
        w = rng.integers(-127, 128, (co, ci, 1, 1)).astype(np.int8)
        b = rng.integers(-20000, 20001, co).astype(np.int32)
        mul = np.exp2(rng.uniform(-12.0, -8.0, co) - 0.5 * np.log2(ci / 64.0)).astype(F32)
        want = SC.pointwise(x, w, b, mul)
        y = _sentinel(2, co, H, W)
        hp.q8x_pointwise(_to_q8(x), hp.q8x_pack_weights(_dev(w)), _dev(b), _dev(mul), y)
        got = _interior(y)
        assert np.array_equal(got, want), f"{H}x{W}: {int((got != want).sum())} of {want.size} differ"
        assert (want < 0).any() and (want > 0).any()                        # identity activation: negatives pass unscaled


@pytest.mark.parametrize("C,H,W", [(16, 3, 5), (128, 7, 18), (256, 15, 15), (256, 7, 7)])
def test_head_equals_the_restatement(C, H, W):
    hp = _hp()
    rng = np.random.default_rng(C + H)
    x = rng.integers(-127, 128, (3, C, H, W)).astype(np.int8)
    w = rng.integers(-127, 128, (5, C)).astype(np.int8)
    b = rng.integers(-20000, 20001, 5).astype(np.int32)
    m = np.exp2(rng.uniform(-16.0, -12.0, 5)).astype(F32)
    z = torch.full((3 * 5 * H * W + 64,), 7.0, dtype=torch.float32, device="cuda")
    hp.q8x_head_f32(_to_q8(x), _dev(w), _dev(b), _dev(m), z[:3 * 5 * H * W].view(3, 5, H, W))
    torch.cuda.synchronize()
    assert bool((z[3 * 5 * H * W:] == 7.0).all())
    assert np.array_equal(z[:3 * 5 * H * W].view(3, 5, H, W).cpu().numpy(), SC.head(x, w, b, m))


# ------------------------------------------------------------------------------------------------------- stem
def _stem_case(seed, N, F_, H, W):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (N, 3, H, W)).astype(np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    w = rng.integers(-127, 128, (F_, 3, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, F_).astype(np.int32)
    mul = np.exp2(rng.uniform(-11.5, -8.5, F_)).astype(F32)
    return x, w, b, mul


def _run_stem(x, w, b, mul):
    hp = _hp()
    N, _, H, W = x.shape
    out = _sentinel(N, w.shape[0], H // 2, W // 2)
    hp.stem3_fwd_q8x_u8(_dev(x), hp.q8x_pack_stem_weights(_dev(w)), _dev(b), _dev(mul), out)
    return _interior(out), out


@pytest.mark.parametrize("F_", [16, 32, 48])
def test_stem_equals_the_restatement(F_):
    for H, W in ((2, 2), (4, 6), (34, 70)):
        x, w, b, mul = _stem_case(F_ + H, 2, F_, H, W)
        want = RR.stem3_q(x, w, b, mul)
        got, _ = _run_stem(x, w, b, mul)
        assert got.shape == want.shape and np.array_equal(got, want), f"{H}x{W}: {int((got != want).sum())} of {want.size} differ"
    # one-hot taps: weight at tap k of channel co, k = co % 27
    x = np.random.default_rng(F_).integers(0, 256, (1, 3, 12, 36)).astype(np.uint8)
    w = np.zeros((F_, 27), np.int8)
    w[np.arange(F_), np.arange(F_) % 27] = 127 - np.arange(F_)
    w = w.reshape(F_, 3, 3, 3)
    b = (np.arange(F_) * 7 - 200).astype(np.int32)
    mul = ((1.0 + np.arange(F_) % 5) / 1024.0).astype(F32)
    got, _ = _run_stem(x, w, b, mul)
    assert np.array_equal(got, RR.stem3_q(x, w, b, mul))


def test_stem_of_64_filters_is_the_existing_entry():
    hp = _hp()
    x, w, b, mul = _stem_case(64, 2, 64, 10, 66)
    got, out = _run_stem(x, w, b, mul)
    old = hp.Q8Tensor(2, 64, 5, 33, "cuda")
    hp.stem3_fwd_q8_u8(_dev(x), hp.q8_pack_stem_weights(_dev(w)), _dev(b), _dev(mul), old)
    torch.cuda.synchronize()
    assert torch.equal(old.nchw(), out.nchw()) and np.array_equal(got, RR.stem3_q(x, w, b, mul))


# ------------------------------------------------------------------------------------------------------- the whole model
@pytest.fixture(scope="module")
def ssd8():
    """The seeded SSD(16) on the GPU, quantised on its two frames, and the restatement of frame 0 with the same scales
    (computed once, shared, never changed)."""
    from fdet_amd.quantize import Int8SSD
    model, frames = SC.seeded_ssd()
    model = model.cuda().eval()
    m8 = model.quantize([frames.cuda()])
    assert type(m8) is Int8SSD and m8.qparams.images_seen == 2 and m8.qparams.method == "absmax"
    P = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    qp = m8.qparams
    ref = SC.model_q(frames[:1].numpy(), P, qp.s_h, qp.s_a, qp.s_k)
    return model, m8, frames, P, ref


def test_calibration_follows_torch_on_the_cpu(ssd8):
    _, m8, frames, P, _ = ssd8
    hs, as_, ks, _ = SC.float_model(P, frames.float() / 255.0)
    qp = m8.qparams
    assert qp.num_blocks == 13 and qp.s_k.size == 4
    assert np.allclose(qp.s_h, SC.absmax_scales(hs), rtol=1e-4, atol=0)
    assert np.allclose(qp.s_a, SC.absmax_scales(as_), rtol=1e-4, atol=0)
    assert np.allclose(qp.s_k, SC.absmax_scales(ks), rtol=1e-4, atol=0)


def test_network_equals_the_restatement(ssd8):
    """N = 1: stem, every block and the heads' z equal the restatement exactly; after the float head-pack, y equals what
    fdet_ssd_head_pack_fwd makes of the restatement's z (the float kernel's own bytes)."""
    hp = _hp()
    _, m8, frames, _, (q0, outs, zs) = ssd8
    before = dict(m8.counters)
    tr = m8.trace(frames[:1].cuda())
    assert tr["stem"].dtype == torch.int8 and np.array_equal(tr["stem"].cpu().numpy(), q0), "stem"
    assert len(tr["blocks"]) == 13
    for k, (got, want) in enumerate(zip(tr["blocks"], outs)):
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want), f"block {k}"
    assert len(tr["z"]) == 4
    for k, (got, want) in enumerate(zip(tr["z"], zs)):
        assert np.array_equal(got.cpu().numpy(), want), f"head {k}"
    y = torch.zeros(1, 4774, 5, device="cuda")
    for k, z in enumerate(zs):
        hp.ssd_head_pack_fwd(torch.from_numpy(z).cuda(), SC.PATCH_SIZES[k], m8.starts[k], y)
    assert tuple(tr["y"].shape) == (1, 4774, 5) and torch.equal(tr["y"], y)
    assert {k: m8.counters[k] - before[k] for k in before} == {"stem_q8": 1, "convs": 26, "pointwise": 4, "heads": 4}
    # one arithmetic for every input: frames, float images in [0,1], predict=1
    y1 = m8.forward_frames(frames[:1].cuda()).clone()
    assert torch.equal(y1, y)
    assert torch.equal(m8(hp.u8_to_f32_norm(frames[:1].cuda())), y) and torch.equal(m8(frames[:1].cuda().float() / 255.0), y)
    det = m8(frames[:1].cuda(), predict=torch.tensor(1))
    want = m8.non_max_suppression(y)
    assert len(det) == len(want) == 1 and torch.equal(det[0], want[0])
    with pytest.raises(Exception):
        m8.train()
    assert m8.eval() is m8


def test_batch_of_three_equals_three_single_runs(ssd8):
    _, m8, frames, _, _ = ssd8
    x = torch.cat([frames, frames[:1].flip(-1)]).cuda()
    singles = [m8.forward_frames(x[i:i + 1]).clone() for i in range(3)]
    y3 = m8.forward_frames(x)
    assert tuple(y3.shape) == (3, 4774, 5)
    for i in range(3):
        assert torch.equal(y3[i:i + 1], singles[i]), f"image {i}"
    # a second call with the same N hands out the same buffers
    p = y3.data_ptr()
    mem = torch.cuda.memory_allocated()
    assert m8.forward_frames(x).data_ptr() == p and torch.cuda.memory_allocated() == mem


def test_graph_replay_equals_eager(ssd8):
    _, m8, frames, _, _ = ssd8
    x = frames.cuda()
    eager = m8.forward_frames(x).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m8.forward_frames(x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = m8.forward_frames(x)
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


def test_other_inputs_take_the_resize_route(ssd8):
    _, m8, frames, _, _ = ssd8
    before = m8.counters["stem_q8"]
    odd = torch.randint(0, 256, (2, 3, 300, 400), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda()
    y = m8.forward_frames(odd)
    assert tuple(y.shape) == (2, 4774, 5) and bool(torch.isfinite(y).all()) and m8.counters["stem_q8"] == before + 1
    # float frames 0..255 at the model resolution are the same image as their bytes
    assert torch.equal(m8.forward_frames(frames.cuda().float()).clone(), m8.forward_frames(frames.cuda()))
    assert torch.equal(m8.forward_frames(frames[0].cuda()).clone(), m8.forward_frames(frames[:1].cuda()))


def test_tiled_detector_and_evaluator_take_the_int8_model(ssd8):
    from fdet_amd.datasets import augment as A
    from fdet_amd.datasets.utils import ReduceSSDBoundingBoxes
    from fdet_amd.evaluation import DetectionEvaluator
    from fdet_amd.tiling import TiledDetector
    _, m8, frames, _, _ = ssd8
    hwc = frames.numpy().transpose(0, 2, 3, 1)
    wide = np.concatenate([hwc[0], hwc[1]], axis=1)                          # 480 x 960: two tiles
    bank = A.DeviceImageBank.from_arrays([wide, hwc[1]], "cuda")
    assert isinstance(DetectionEvaluator().reducer_for(m8), ReduceSSDBoundingBoxes)
    # an untrained model scores every prior near 0.5: a threshold between the 10th and 11th best score of the two frames (the
    # windows are exactly these frames) keeps a handful of candidates per window
    top = m8.forward_frames(frames.cuda())[..., 0].reshape(-1).sort(descending=True).values
    red = ReduceSSDBoundingBoxes(probability_threshold=float(top[9] + top[10]) / 2, iou_threshold=0.5, input_shape=m8.input_shape,
                                 patch_sizes=m8.patch_sizes)
    det = TiledDetector(m8, tile_sizes=(480,), overlap=0.0, include_whole=False, edge_margin=0.0, max_out=100, reducer=red)
    rows, counts = det.detect(bank, [0, 1])
    assert tuple(rows.shape[::2]) == (2, 5) and tuple(counts.shape) == (2,)
    assert 1 <= int(counts.sum()) <= 200 and bool(torch.isfinite(rows).all())


def test_quantisation_error_against_the_float_engine(ssd8):
    """max / mean |dz| over the (1,4774,5) rows before sigmoid and priors and max / mean |dscore| of frame 0, int8 against the
    float bf16x3 engine.  The bound is 1.25 x what the RESTATEMENT gives on the CPU against torch fp32 for the same seed
    (tests/test_q8_ssd_host.py measures and pins those constants): max |dz| 0.009743, mean |dz| 0.001645, max |dscore|
    0.002353, mean |dscore| 0.000419 on max |z| 0.168."""
    model, m8, frames, _, _ = ssd8
    x = frames[:1].cuda()
    zs_q = [z.cpu().numpy() for z in m8.trace(x)["z"]]
    names, params = model.named_stack_params()
    Pd = {n: p.detach() for n, p in zip(names, params)}
    with torch.no_grad():
        y_f, saved = model.engine.forward(x.float() / 255.0, Pd, None, save=True)
        zs_f = []
        for k in range(4):
            hn = f"extracting_layers.{k}.0"
            zs_f.append(torch.nn.functional.conv2d(saved["heads"][k], Pd[hn + ".weight"][:, :, None, None], Pd[hn + ".bias"]).cpu().numpy())
    e = SC.quant_error(zs_q, zs_f)
    ds = (m8.forward_frames(x)[..., 0] - y_f[..., 0]).abs()
    print(f"int8 SSD against the float engine: max |dz| {e[0]:.6f}, mean |dz| {e[1]:.6f}, max |dscore| {e[2]:.6f}, "
          f"mean |dscore| {e[3]:.6f}; on y: max |dscore| {float(ds.max()):.6f}, mean {float(ds.mean()):.6f}")
    assert e[0] <= 1.25 * SSD_DZ_MAX and e[1] <= 1.25 * SSD_DZ_MEAN
    assert e[2] <= 1.25 * SSD_DS_MAX and e[3] <= 1.25 * SSD_DS_MEAN
    assert float(ds.max()) <= 1.25 * SSD_DS_MAX and float(ds.mean()) <= 1.25 * SSD_DS_MEAN
