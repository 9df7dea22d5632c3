"""GPU checks of the int8 chain (fdet_q8_chain) and the quantising stem (fdet_stem_fwd_q8_u8) against the numpy restatement
(tests/q8_chain_cases.py over tests/q8_cpu_ref.py) and against the launches they replace.  Every comparison is equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_chain_cases as CC  # noqa: E402
import q8_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
OUT_SCALE = 0.0437                                         # no power of two


def _hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def _to_q8(a):
    """numpy int8 (N,C,H,W) -> Q8Tensor, the layout built with torch (not with a kernel under test)."""
    hp = _hp()
    N, C, H, W = a.shape
    t = hp.Q8Tensor(N, C, H, W, "cuda")
    v = t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)
    v[:, 1:-1, 1:-1, :] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return t


def _halo(t):
    N, C, H, W = t.shape
    v = t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)
    return torch.cat([v[:, 0].reshape(-1), v[:, -1].reshape(-1), v[:, :, 0].reshape(-1), v[:, :, -1].reshape(-1)])


def _dev(conv):
    hp = _hp()
    w, b, mul = conv
    return hp.q8_pack_weights(torch.from_numpy(w).cuda()), torch.from_numpy(b).cuda(), torch.from_numpy(mul).cuda()


def _weights(d):
    hp = _hp()
    c1 = [_dev(b[0]) for b in d["blocks"]]
    c2 = [_dev(b[1]) for b in d["blocks"]]
    return hp.Q8ChainWeights(c1, c2, [float(v) for v in d["skip_mul"]])


def _run_chain(d, want_out=None, f32=True):
    """-> (list of Q8Tensor or None per block, fp32 output or None)"""
    hp = _hp()
    N, C, H, W = d["shape"]
    nb = len(d["blocks"])
    x = _to_q8(d["x"])
    x_before = x.storage.clone()
    want_out = range(nb) if want_out is None else want_out
    outs = [hp.Q8Tensor(N, C, H, W, "cuda") if k in want_out else None for k in range(nb)]
    of = torch.full((N, C, H, W), float("nan"), device="cuda") if f32 else None
    hp.q8_chain(x, _weights(d), outs=outs if any(o is not None for o in outs) else None, out_f32=of, out_scale=OUT_SCALE,
                slope=float(d["slope"]))
    torch.cuda.synchronize()
    assert torch.equal(x.storage, x_before)                                # the input is read only
    for o in outs:
        assert o is None or not bool(_halo(o).any())
    return outs, of


def _run_layers(d):
    """The same blocks through fdet_q8_conv3x3, launch by launch -> list of Q8Tensor per block"""
    hp = _hp()
    N, C, H, W = d["shape"]
    h, outs = _to_q8(d["x"]), []
    for (c1, c2), sm in zip(d["blocks"], d["skip_mul"]):
        a, o = hp.Q8Tensor(N, C, H, W, "cuda"), hp.Q8Tensor(N, C, H, W, "cuda")
        hp.q8_conv3x3(h, *_dev(c1), a, slope=float(d["slope"]))
        hp.q8_conv3x3(a, *_dev(c2), o, skip=h, skip_mul=float(sm), slope=float(d["slope"]))
        outs.append(o)
        h = o
    return outs


def _check(d, ref):
    hp = _hp()
    outs, of = _run_chain(d)
    layers = _run_layers(d)
    for k, (o, l, (_, want)) in enumerate(zip(outs, layers, ref)):
        got = o.nchw().cpu().numpy()
        assert np.array_equal(got, want), f"block {k}: {int((got != want).sum())} of {want.size} differ from the restatement"
        assert torch.equal(o.storage, l.storage), f"block {k}: differs from fdet_q8_conv3x3"
    assert torch.equal(of, hp.q8_dequantize(outs[-1], OUT_SCALE))
    assert np.array_equal(of.cpu().numpy(), R.dequantize(ref[-1][1], F32(OUT_SCALE)))
    return outs, of


# ------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("i", range(len(CC.CHAIN_CASES)), ids=CC.CHAIN_IDS)
def test_chain_equals_the_restatement_and_the_launches_it_replaces(i):
    _check(CC.make_chain_case(i), CC.chain_ref(i))


def test_chain_outputs_are_optional():
    """(3,15,15,8) with only blocks 2 and 7 written, and with the fp32 output alone: the same bytes."""
    d, ref = CC.make_chain_case(1), CC.chain_ref(1)
    outs, of = _run_chain(d, want_out=(2, 7))
    assert [o is not None for o in outs] == [False, False, True, False, False, False, False, True]
    assert np.array_equal(outs[2].nchw().cpu().numpy(), ref[2][1]) and np.array_equal(outs[7].nchw().cpu().numpy(), ref[7][1])
    want_f = R.dequantize(ref[7][1], F32(OUT_SCALE))
    assert np.array_equal(of.cpu().numpy(), want_f)
    outs2, of2 = _run_chain(d, want_out=())
    assert all(o is None for o in outs2) and np.array_equal(of2.cpu().numpy(), want_f)
    outs3, of3 = _run_chain(d, want_out=(7,), f32=False)
    assert of3 is None and np.array_equal(outs3[7].nchw().cpu().numpy(), ref[7][1])
    with pytest.raises(ValueError):
        _run_chain(d, want_out=(2,), f32=False)


# ------------------------------------------------------------------------------------------------------- lane map
@pytest.mark.parametrize("tap", range(9))
def test_one_hot_chain_tells_rows_columns_taps_and_channels_apart(tap):
    """Two blocks at 15x15, unit multipliers, no bias, slope 1, skip_mul 0: the first conv of a block is the single tap with
    the channel permutation ci = (5 co + 3) % 64, the second the centre-tap identity -- a block shifts its input by the tap
    and permutes its channels, value for value, and the chain does it twice.  At every position the 64 channels differ and
    in every channel the 225 positions differ (7 and 29 are units modulo 255)."""
    ky, kx = divmod(tap, 3)
    c = np.arange(64)[:, None, None]
    p = (np.arange(15)[:, None] * 15 + np.arange(15)[None, :])[None]
    x = ((7 * c + 29 * p) % 255 - 127).astype(np.int8)[None]
    perm = (5 * np.arange(64) + 3) % 64
    w1 = np.zeros((64, 64, 3, 3), np.int8)
    w1[np.arange(64), perm, ky, kx] = 1
    w2 = np.zeros((64, 64, 3, 3), np.int8)
    w2[np.arange(64), np.arange(64), 1, 1] = 1
    z, one = np.zeros(64, np.int32), np.ones(64, F32)
    d = dict(shape=(1, 64, 15, 15), x=x, blocks=[((w1, z, one), (w2, z, one))] * 2, skip_mul=[F32(0.0)] * 2, slope=F32(1.0))
    ref = CC.restate(d)

    def shift(t):
        tp = np.zeros((1, 64, 17, 17), np.int8)
        tp[:, :, 1:-1, 1:-1] = t
        return tp[:, perm, ky:ky + 15, kx:kx + 15]
    assert np.array_equal(ref[0][1], shift(x)) and np.array_equal(ref[1][1], shift(shift(x)))      # (the restatement says the same)
    _check(d, ref)


# ------------------------------------------------------------------------------------------------------- ties
def test_chain_rounds_ties_to_even():
    d = CC.make_ties_case()
    _check(d, CC.restate(d))


# ------------------------------------------------------------------------------------------------------- the stem
# (N, H, W): two output rows; an odd total row count (15: the dummy row of the pair walk); W % 8 != 0 (twice); the model's
# shape; the edge shapes of tests/test_gpu_stem_paths.py that the uint8 PS stem accepts; more rows (300) than the launch has
# workgroups.  The stem kernels take Wo % 4 == 0 only (fdet_stem_fwd_bf16x3, the reference of this test, included), so the
# small shapes are 36 and 68 wide: (1,16,16), (3,40,40) and (2,36,52) have Wo = 2, 5 and 6 and every form refuses them, see
# test_quantising_stem_refuses_what_the_uint8_stem_refuses.
STEM_SHAPES = [(1, 16, 36), (3, 40, 36), (2, 36, 68), (2, 36, 36), (2, 480, 480), (2, 478, 484), (2, 62, 416), (2, 10, 36),
               (2, 102, 224), (5, 478, 36)]
STEM_REFUSED = [(1, 16, 16), (3, 40, 40), (2, 36, 52), (2, 478, 478), (2, 70, 512)]


def test_quantising_stem_refuses_what_the_uint8_stem_refuses():
    hp = _hp()
    for N, H, W in STEM_REFUSED:
        assert not hp.stem_fwd_ps_ok(N, 3, 64, H, W, 10, 8, 2, u8=True) and not hp.stem_fwd_q8_ok(N, 3, 64, H, W, 10, 8, 2), (N, H, W)
        Ho, Wo = (H + 4 - 10) // 8 + 1, (W + 4 - 10) // 8 + 1
        frames = torch.zeros(N, 3, H, W, dtype=torch.uint8, device="cuda")
        with pytest.raises(hp.N.FdetError):
            hp.stem_fwd_q8_u8(frames, torch.zeros(64, 3, 10, 10, device="cuda"), torch.zeros(64, device="cuda"), 1.0,
                              hp.Q8Tensor(N, 64, Ho, Wo, "cuda"))
    for N, H, W in STEM_SHAPES:
        assert hp.stem_fwd_ps_ok(N, 3, 64, H, W, 10, 8, 2, u8=True) and hp.stem_fwd_q8_ok(N, 3, 64, H, W, 10, 8, 2), (N, H, W)


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=["x".join(str(v) for v in s) for s in STEM_SHAPES])
def test_quantising_stem_equals_stem_then_quantise(shape):
    hp = _hp()
    N, H, W = shape
    gen = torch.Generator().manual_seed(100 * H + W + N)
    frames = torch.randint(0, 256, (N, 3, H, W), dtype=torch.uint8, generator=gen).cuda()
    w = (torch.randn(64, 3, 10, 10, generator=gen) * 0.08).cuda()
    b = (torch.randn(64, generator=gen) * 0.5).cuda()
    assert hp.stem_fwd_q8_ok(N, 3, 64, H, W, 10, 8, 2)
    Ho, Wo = (H + 4 - 10) // 8 + 1, (W + 4 - 10) // 8 + 1
    x = hp.u8_to_f32_norm(frames)
    y = torch.empty(N, 64, Ho, Wo, device="cuda")
    nws = hp.stem_ws_bytes(N, 3, 64, H, W, 10, 8, 2)
    ws = torch.empty(max((nws + 3) // 4, 4), device="cuda")
    hp.stem_fwd(x, w, b, y, ws, 10, 8, 2, x3=True)
    full = float(y.abs().max()) / 127.0
    for scale in (full, full / 4.0):                       # a quarter of the range: a real share clamps
        want = hp.q8_quantize(y, scale)
        got = hp.stem_fwd_q8_u8(frames, w, b, scale, hp.Q8Tensor(N, 64, Ho, Wo, "cuda"))
        torch.cuda.synchronize()
        assert torch.equal(got.storage, want.storage), f"{int((got.storage != want.storage).sum())} bytes differ at scale {scale}"
        assert not bool(_halo(got).any())
        if scale != full:
            assert float((want.nchw().abs() == 127).float().mean()) > 0.01
        # producers write real pixels only: a buffer with a nonzero halo keeps it
        dirty = hp.Q8Tensor(N, 64, Ho, Wo, "cuda")
        dirty.storage.fill_(5)
        hp.stem_fwd_q8_u8(frames, w, b, scale, dirty)
        assert torch.equal(dirty.nchw(), want.nchw()) and bool((_halo(dirty) == 5).all())
        tail = dirty.storage[N * (Ho + 2) * (Wo + 2) * 64:]
        assert bool((tail == 5).all())


# ------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def trained(golden):
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.quantize import calibrate
    g = golden("g16_trained_medium")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    model = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.7, iou_threshold=0.01)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().eval()
    images = golden("g6_trained_small")["images"]
    qp = calibrate(model, [images[:2].cuda(), images[2:].cuda()])
    return model, qp, images


def _model(trained, chain, stem, monkeypatch):
    from fdet_amd.quantize import Int8PoolResnet
    monkeypatch.setenv("FDET_Q8_CHAIN", chain)
    monkeypatch.setenv("FDET_Q8_STEM", stem)
    return Int8PoolResnet(trained[0], trained[1])


def test_model_paths_agree_bit_for_bit(trained, monkeypatch):
    frames = trained[2].cuda()
    ys, ys_float, traces = {}, {}, {}
    for chain, stem in (("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")):
        m8 = _model(trained, chain, stem, monkeypatch)
        assert m8.counters == {"chain": 0, "layers": 0, "stem_q8": 0, "stem_f32": 0}
        ys[chain, stem] = m8.forward_frames(frames)
        assert m8.counters == {"chain": int(chain), "layers": 1 - int(chain), "stem_q8": int(stem), "stem_f32": 1 - int(stem)}
        ys_float[chain, stem] = m8.forward_frames(frames.float())          # float frames keep the float stem
        assert m8.counters["stem_f32"] == 2 - int(stem) and m8.counters["stem_q8"] == int(stem)
        traces[chain, stem] = m8.trace(frames)
        assert m8.counters["chain"] == 2 * int(chain) + int(chain) and m8.counters["stem_q8"] == int(stem)      # trace(): the float stem
    base = ys["0", "0"]
    assert tuple(base.shape) == (3, 5, 10, 10) and bool((base[:, 0] > 0.7).any())
    for k, y in ys.items():
        assert torch.equal(y, base) and torch.equal(ys_float[k], ys_float["0", "0"]), k
    tb = traces["0", "0"]
    assert len(tb["blocks"]) == 10 and tuple(tb["stem"].shape) == (3, 64, 60, 60) and tb["stem"].dtype == torch.float32
    for k, t in traces.items():
        assert torch.equal(t["y"], base) and torch.equal(t["stem"], tb["stem"]) and len(t["blocks"]) == 10, k
        for j, (a, b) in enumerate(zip(t["blocks"], tb["blocks"])):
            assert a.dtype == torch.int8 and torch.equal(a, b), (k, j)


def test_wide_model_falls_back_to_layers_and_the_float_stem(monkeypatch):
    """F = 128: neither new kernel takes it (a layer's weights are 147 KB; the stem is built for 64 channels)."""
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.quantize import Int8PoolResnet, QuantParams
    torch.manual_seed(5)
    model = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10).cuda().eval()
    nb = len(model.residual_blocks)
    qp = QuantParams(np.full(nb + 1, 0.05), np.full(nb, 0.05))
    monkeypatch.setenv("FDET_Q8_CHAIN", "1")
    monkeypatch.setenv("FDET_Q8_STEM", "1")
    m8 = Int8PoolResnet(model, qp)
    assert not m8.chain_on() and not m8.stem_q8_on(2)
    frames = torch.randint(0, 256, (2, 3, 480, 480), dtype=torch.uint8, generator=torch.Generator().manual_seed(6)).cuda()
    y = m8.forward_frames(frames)
    assert tuple(y.shape) == (2, 5, 10, 10) and bool(torch.isfinite(y).all())
    assert m8.counters == {"chain": 0, "layers": 1, "stem_q8": 0, "stem_f32": 1}


def test_graphed_predict_replay_with_both_paths_equals_eager(trained, monkeypatch):
    """Two frames, one capture, two replays: the chain's pointer arrays travel by value, so nothing in it needs a copy."""
    m8 = _model(trained, "1", "1", monkeypatch)
    frames = trained[2].cuda()
    eager_a = m8.non_max_suppression(m8.forward_frames(frames[:2]))
    eager_b = m8.non_max_suppression(m8.forward_frames(frames[[2, 0]]))
    gp = m8.graphed_predict(frames[[1, 1]])
    before = dict(m8.counters)
    for fr, eager in ((frames[:2], eager_a), (frames[[2, 0]], eager_b)):
        out = gp(fr)
        assert len(out) == len(eager) == 2 and sum(int(o.shape[0]) for o in eager) >= 1
        for a, b in zip(out, eager):
            assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b.cpu())
    assert m8.counters == before and before["chain"] >= 3 and before["stem_q8"] >= 3 and before["layers"] == before["stem_f32"] == 0
