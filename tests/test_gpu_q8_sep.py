"""GPU checks of the int8 separable block (csrc/fdet_q8_sep.hip: fdet_q8_sepblock, fdet_q8_sepchain) and of Int8SeparableCNN
against the numpy restatement tests/q8_sep_cpu_ref.py.  The arithmetic is integer with one-rounding float steps, so every int8
comparison is equality; the two tolerances are the float head's (1e-4, as tests/test_gpu_q8_pool_stem.py) and the accuracy
bound against the float engine (q8_sep_cpu_ref.ACCURACY_RECORDED times 1.25)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_sep_cpu_ref as RS  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
OUT_SCALE = 0.0437                                         # no power of two


def _hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def _view(t):
    N, C, H, W = t.shape
    return t.storage[:N * (H + 2) * (W + 2) * C].view(N, H + 2, W + 2, C)


def _to_q8(a):
    """numpy int8 (N,C,H,W) -> Q8Tensor, the layout built with torch (not with a kernel under test)."""
    t = _hp().Q8Tensor(*a.shape, "cuda")
    _view(t)[:, 1:-1, 1:-1, :] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return t


def _halo(t):
    v = _view(t)
    return torch.cat([v[:, 0].reshape(-1), v[:, -1].reshape(-1), v[:, :, 0].reshape(-1), v[:, :, -1].reshape(-1)])


def _dev(p):
    """restatement parameters -> the kernel's device tensors (w1, mul1, wd, mul2, w2, mul3)"""
    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return (t(p["w1"]).reshape(-1), t(p["mul1"]), t(RS.pack_dw(p["wd"])).reshape(-1), t(p["mul2"]), t(p["w2"]).reshape(-1), t(p["mul3"]))


def _run_block(d, tile=None):
    """One fdet_q8_sepblock call -> numpy (N,C,H',W').  The input must come back unchanged and y's halo must still be zero."""
    hp = _hp()
    N, C, H, W = d["shape"]
    x = _to_q8(d["x"])
    before = x.storage.clone()
    y = hp.Q8Tensor(N, C, H // 2, W // 2, "cuda") if d["pool"] else hp.Q8Tensor(N, C, H, W, "cuda")
    hp.q8_sepblock(x, *_dev(d["p"]), float(d["p"]["skip_mul"]), y, pool=d["pool"], tile=d["tile"] if tile is None else tile,
                   slope=float(d["slope"]))
    torch.cuda.synchronize()
    assert torch.equal(x.storage, before), "the block wrote into its input"
    assert not bool(_halo(y).any()), "the block wrote into the halo of y"
    return y.nchw().cpu().numpy()


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.int8
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} differ from the restatement"


# ------------------------------------------------------------------------------------------------------- the block
@pytest.mark.parametrize("idx", range(len(RS.CASES)), ids=RS.CASE_IDS)
def test_block_equals_the_restatement(idx):
    d = RS.make_case(idx)
    _same(_run_block(d), RS.sepblock(d["x"], d["p"], d["pool"], d["slope"]), RS.CASE_IDS[idx])


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_depthwise_taps_and_the_halo(tap):
    """(1,64,3,3): w1 = w2 = identity * 127, the depthwise filter one-hot on one tap: the block shifts its input by that tap,
    zeros coming in from the halo.  A transposed or mirrored tap order, or padding that is not zero, shows."""
    d = RS.make_onehot_case(tap)
    want = RS.shifted(d["x"], tap)
    assert np.array_equal(RS.sepblock(d["x"], d["p"], False, d["slope"]), want)
    _same(_run_block(d), want, f"tap {tap}")


def test_forced_tilings_and_the_planner_agree():
    """(1,64,12,10): the planner's single tile, 4x4 (seams both ways, ragged last segment), 5x3, 1x1 and 12x1: the same bytes."""
    d = RS.make_case(8)
    want = RS.sepblock(d["x"], d["p"], d["pool"], d["slope"])
    assert _hp().q8_sepblock_plan(64, 12, 10)[:2] == (12, 10)
    for tile in ((0, 0), (4, 4), (5, 3), (1, 1), (12, 1), (16, 16)):
        _same(_run_block(d, tile), want, f"tile {tile}")
    with pytest.raises(_hp().N.FdetError, match="LDS"):
        _run_block(d, (64, 64))
    with pytest.raises(_hp().N.FdetError, match="both"):
        _run_block(d, (4, 0))
    dp = RS.make_case(6)
    with pytest.raises(_hp().N.FdetError, match="even when pooled"):
        _run_block(dp, (3, 2))


def test_block_writes_real_pixels_only():
    """A y buffer with a nonzero halo and tail keeps them (un-pooled with forced seams, and pooled)."""
    hp = _hp()
    for idx in (8, 6):
        d = RS.make_case(idx)
        N, C, H, W = d["shape"]
        Ho, Wo = (H // 2, W // 2) if d["pool"] else (H, W)
        nbytes = hp.q8_act_bytes(N, C, Ho, Wo)
        store = torch.zeros(nbytes + 256, dtype=torch.int8, device="cuda")
        y = hp.Q8Tensor(N, C, Ho, Wo, "cuda", storage=store)
        store.fill_(0x55)
        hp.q8_sepblock(_to_q8(d["x"]), *_dev(d["p"]), float(d["p"]["skip_mul"]), y, pool=d["pool"], tile=d["tile"], slope=float(d["slope"]))
        torch.cuda.synchronize()
        _same(y.nchw().cpu().numpy(), RS.sepblock(d["x"], d["p"], d["pool"], d["slope"]), RS.CASE_IDS[idx])
        assert bool((_halo(y) == 0x55).all()) and bool((store[nbytes:] == 0x55).all())


# ------------------------------------------------------------------------------------------------------- the chain
def _chain_weights(d):
    hp = _hp()
    return hp.Q8SepChainWeights([_dev(p) for p in d["blocks"]], [float(p["skip_mul"]) for p in d["blocks"]])


def _run_chain(d, want_out=None, f32=True, weights=None):
    hp = _hp()
    N, C, H, W = d["shape"]
    nb = len(d["blocks"])
    x = _to_q8(d["x"])
    before = x.storage.clone()
    want_out = range(nb) if want_out is None else want_out
    outs = [hp.Q8Tensor(N, C, H, W, "cuda") if k in want_out else None for k in range(nb)]
    of = torch.full((N, C, H, W), float("nan"), device="cuda") if f32 else None
    hp.q8_sepchain(x, weights or _chain_weights(d), outs=outs if any(o is not None for o in outs) else None, out_f32=of,
                   out_scale=OUT_SCALE, slope=float(d["slope"]))
    torch.cuda.synchronize()
    assert torch.equal(x.storage, before)
    for o in outs:
        assert o is None or not bool(_halo(o).any())
    return outs, of


def _run_blocks(d):
    """The same blocks through fdet_q8_sepblock, launch by launch -> list of Q8Tensor per block"""
    hp = _hp()
    N, C, H, W = d["shape"]
    h, outs = _to_q8(d["x"]), []
    for p in d["blocks"]:
        o = hp.Q8Tensor(N, C, H, W, "cuda")
        hp.q8_sepblock(h, *_dev(p), float(p["skip_mul"]), o, slope=float(d["slope"]))
        outs.append(o)
        h = o
    return outs


@pytest.mark.parametrize("i", range(len(RS.CHAIN_CASES)), ids=RS.CHAIN_IDS)
def test_chain_equals_the_restatement_and_the_launches_it_replaces(i):
    hp = _hp()
    d = RS.make_chain_case(i)
    ref = RS.sepchain(d["x"], d["blocks"], d["slope"])
    outs, of = _run_chain(d)
    for k, (o, l, want) in enumerate(zip(outs, _run_blocks(d), ref)):
        _same(o.nchw().cpu().numpy(), want, f"block {k}")
        assert torch.equal(o.storage, l.storage), f"block {k}: differs from fdet_q8_sepblock"
    assert torch.equal(of, hp.q8_dequantize(outs[-1], OUT_SCALE))
    assert np.array_equal(of.cpu().numpy(), R.dequantize(ref[-1], F32(OUT_SCALE)))


def test_chain_outputs_are_optional():
    d = RS.make_chain_case(2)                                              # 8 blocks at 15x15
    ref = RS.sepchain(d["x"], d["blocks"], d["slope"])
    want_f = R.dequantize(ref[7], F32(OUT_SCALE))
    outs, of = _run_chain(d, want_out=(2, 7))
    assert [o is not None for o in outs] == [False, False, True, False, False, False, False, True]
    _same(outs[2].nchw().cpu().numpy(), ref[2])
    _same(outs[7].nchw().cpu().numpy(), ref[7])
    assert np.array_equal(of.cpu().numpy(), want_f)
    outs2, of2 = _run_chain(d, want_out=())
    assert all(o is None for o in outs2) and np.array_equal(of2.cpu().numpy(), want_f)
    outs3, of3 = _run_chain(d, want_out=(7,), f32=False)
    assert of3 is None and np.array_equal(outs3[7].nchw().cpu().numpy(), ref[7])
    with pytest.raises(ValueError):
        _run_chain(d, want_out=(2,), f32=False)


def test_chain_of_more_blocks_than_stay_in_lds():
    """12 and 16 blocks: the parameters are staged in windows of ten; the same bytes as the launches."""
    rng = np.random.default_rng(1990)
    x = rng.integers(-127, 128, (2, 64, 15, 15)).astype(np.int8)
    blocks = [RS.random_params(rng, 64) for _ in range(16)]
    ref = RS.sepchain(x, blocks)
    for nb in (12, 16):
        d = dict(shape=x.shape, x=x, blocks=blocks[:nb], slope=RS.SLOPE)
        outs, of = _run_chain(d, want_out=(9, 10, nb - 1))
        for k in (9, 10, nb - 1):
            _same(outs[k].nchw().cpu().numpy(), ref[k], f"{nb} blocks, block {k}")
        assert np.array_equal(of.cpu().numpy(), R.dequantize(ref[nb - 1], F32(OUT_SCALE)))


def test_chain_replays_from_a_captured_graph():
    """The pointer arrays travel by value: one capture, two replays on new input bytes, equal bytes."""
    hp = _hp()
    d = RS.make_chain_case(2)
    N, C, H, W = d["shape"]
    w = _chain_weights(d)
    x = _to_q8(d["x"])
    outs = [hp.Q8Tensor(N, C, H, W, "cuda") for _ in d["blocks"]]
    of = torch.zeros(N, C, H, W, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hp.q8_sepchain(x, w, outs=outs, out_f32=of, out_scale=OUT_SCALE)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hp.q8_sepchain(x, w, outs=outs, out_f32=of, out_scale=OUT_SCALE)
    for flip in (False, True):
        xin = d["x"][:, :, ::-1].copy() if flip else d["x"]
        x.storage.copy_(_to_q8(xin).storage)
        for o in outs:
            _view(o)[:, 1:-1, 1:-1, :] = 0
        of.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref = RS.sepchain(xin, d["blocks"])
        for k, (o, want) in enumerate(zip(outs, ref)):
            _same(o.nchw().cpu().numpy(), want, f"replay (flip={flip}), block {k}")
        assert np.array_equal(of.cpu().numpy(), R.dequantize(ref[-1], F32(OUT_SCALE)))


# ------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module", params=range(len(RS.ACCURACY_MODELS)), ids=[f"{m[1]}" for m in RS.ACCURACY_MODELS])
def net(request):
    """A seeded random SeparableCNN(filters=64) (480x480 with output_padding=3, or 512x512 with output_kernel_size=1), absmax
    scales from the float oracle on the CPU, and the restatement of the int8 network on its three frames, computed once."""
    from fdet_amd.quantize import QuantParams
    model, P, frames, head_pad = RS.accuracy_model(request.param)
    hs, as_, bs, y = RS.float_forward(P, frames, head_pad)
    s_h, s_a, s_b = RS.absmax_scales(hs, as_, bs)
    qp = QuantParams(s_h, s_a, s_b=s_b)
    return dict(i=request.param, model=model.cuda().eval(), P=P, frames=torch.from_numpy(frames), qp=qp, y_float=y,
                ref=RS.model_q(frames, P, s_h, s_a, s_b, head_pad))


def _m8(net, chain, monkeypatch):
    from fdet_amd.quantize import Int8SeparableCNN
    if chain is None:
        monkeypatch.delenv("FDET_Q8_SEPCHAIN", raising=False)
    else:
        monkeypatch.setenv("FDET_Q8_SEPCHAIN", chain)
    return Int8SeparableCNN(net["model"], net["qp"])


def test_model_equals_the_restatement_with_and_without_the_chain(net, monkeypatch):
    q0, outs, hd, y = net["ref"]
    frames = net["frames"][:2].cuda()                                      # N = 2
    ys = {}
    for chain in ("0", "1"):
        m8 = _m8(net, chain, monkeypatch)
        assert m8.counters == {"sepchain": 0, "sepblocks": 0, "stem_q8": 0} and m8.chain_on() == (chain == "1")
        tr = m8.trace(frames)
        assert m8.counters == {"sepchain": int(chain), "sepblocks": 2 if chain == "1" else 10, "stem_q8": 1}
        assert tr["stem"].dtype == torch.int8 and np.array_equal(tr["stem"].cpu().numpy(), q0[:2]), "stem"
        assert len(tr["blocks"]) == 10
        for k, (got, want) in enumerate(zip(tr["blocks"], outs)):
            assert got.dtype == torch.int8
            _same(got.cpu().numpy(), want[:2], f"chain={chain}, block {k}")
        assert tuple(tr["y"].shape) == (2, 5, 16, 16)
        assert float((tr["y"].cpu() - y[:2]).abs().max()) <= 1e-4            # the float head on the dequantised last block
        ys[chain] = m8.forward_frames(frames)
        assert torch.equal(ys[chain], tr["y"])
        # one input rule: float frames 0..255 and float images in [0,1] built from those bytes reach the same kernel
        assert torch.equal(m8.forward_frames(frames.float()), ys[chain]) and torch.equal(m8(frames.float() / 255.0), ys[chain])
        assert m8.counters["stem_q8"] == 4
    assert torch.equal(ys["0"], ys["1"])
    from fdet_amd import quantize as Q
    assert _m8(net, None, monkeypatch).chain_on() == Q.SEPCHAIN_MEASURED_FASTER


def test_model_accuracy_against_the_float_engine(net, monkeypatch):
    """The bound of tests/test_q8_sep_host.py (recorded on the CPU, times 1.25), here int8 kernels against the float engine."""
    frames = net["frames"].cuda()
    m8 = _m8(net, None, monkeypatch)
    with torch.no_grad():
        y_float = net["model"].forward_frames(frames)
    assert float((y_float.cpu() - net["y_float"]).abs().max()) <= 1e-4        # (the engine is the oracle's arithmetic)
    d = (m8.forward_frames(frames) - y_float).abs()
    print(f"model {RS.ACCURACY_MODELS[net['i']]} on the GPU: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}")
    rec_max, rec_mean = RS.ACCURACY_RECORDED[net["i"]]
    assert float(d.max()) <= 1.25 * rec_max
    assert float(d.mean()) <= 1.25 * rec_mean


def test_calibrate_and_quantize_give_the_oracles_scales(net):
    from fdet_amd.quantize import Int8SeparableCNN, calibrate
    frames = net["frames"].cuda()
    qp = calibrate(net["model"], [frames[:2], frames[2:]])
    assert qp.s_b is not None and qp.num_blocks == 10 and qp.images_seen == 3 and qp.method == "absmax"
    for got, want in ((qp.s_h, net["qp"].s_h), (qp.s_a, net["qp"].s_a), (qp.s_b, net["qp"].s_b)):
        assert np.allclose(got, want, rtol=1e-4, atol=0)
    m8 = net["model"].quantize([frames])
    assert type(m8) is Int8SeparableCNN and m8.qparams == qp
    assert tuple(m8.forward_frames(frames[:1]).shape) == (1, 5, 16, 16)


def test_wide_model_runs_launch_by_launch(monkeypatch):
    """filters=128 at 160x160 (20x20 pooled to 10x10, three blocks): the chain is built for 64 channels."""
    from fdet_amd.models.SeparableCNN import SeparableCNN
    from fdet_amd.quantize import Int8SeparableCNN, QuantParams
    torch.manual_seed(195)
    model = SeparableCNN(filters=128, input_shape=(3, 160, 160), num_of_residual_blocks=3).eval()
    frames = torch.randint(0, 256, (2, 3, 160, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(196))
    P = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    hs, as_, bs, _ = RS.float_forward(P, frames.numpy(), 0)
    s_h, s_a, s_b = RS.absmax_scales(hs, as_, bs)
    monkeypatch.setenv("FDET_Q8_SEPCHAIN", "1")
    m8 = Int8SeparableCNN(model.cuda(), QuantParams(s_h, s_a, s_b=s_b))
    assert not m8.chain_on() and [h for h, _ in m8.lv] == [20, 10, 10]
    q0, outs, _, y = RS.model_q(frames.numpy(), P, s_h, s_a, s_b, 0)
    tr = m8.trace(frames.cuda())
    assert np.array_equal(tr["stem"].cpu().numpy(), q0)
    for k, (got, want) in enumerate(zip(tr["blocks"], outs)):
        _same(got.cpu().numpy(), want, f"block {k}")
    assert tuple(tr["y"].shape) == (2, 5, 5, 5) and float((tr["y"].cpu() - y).abs().max()) <= 1e-4
    assert m8.counters == {"sepchain": 0, "sepblocks": 3, "stem_q8": 1}


def test_model_refusals(net):
    from fdet_amd import FdetError
    from fdet_amd.quantize import Int8SeparableCNN, QuantParams, calibrate
    m8 = Int8SeparableCNN(net["model"], net["qp"])
    assert m8.eval() is m8 and m8.train(False) is m8 and not m8.training
    with pytest.raises(FdetError, match="inference only"):
        m8.train(True)
    with pytest.raises(ValueError, match="residual blocks"):
        Int8SeparableCNN(net["model"], QuantParams([1.0] * 4, [1.0] * 3, s_b=[1.0] * 3))
    with pytest.raises(ValueError, match="s_b"):
        Int8SeparableCNN(net["model"], QuantParams(net["qp"].s_h, net["qp"].s_a))
    with pytest.raises(FdetError, match="GPU only"):
        m8.forward_frames(net["frames"][:1])                               # CPU frames: no CPU fallback
    eng = net["model"].engine
    eng.p16 = True
    try:
        with pytest.raises(FdetError, match="precision16"):
            calibrate(net["model"], [net["frames"][:1].cuda()])
    finally:
        eng.p16 = False


def test_graphed_predict_replay_equals_eager(net, monkeypatch):
    m8 = _m8(net, "1", monkeypatch)
    frames = net["frames"].cuda()
    eager = m8.non_max_suppression(m8.forward_frames(frames[:2]))
    gp = m8.graphed_predict(frames[[2, 2]])
    out = gp(frames[:2])
    assert len(out) == len(eager) == 2
    for a, b in zip(out, eager):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b.cpu())


def test_tiled_detector_and_evaluator_take_the_int8_model(net, monkeypatch):
    """Whole-image windows of a two-image bank at the model's size: the rows of forward_frames plus the reducer by hand."""
    from fdet_amd.datasets import augment as A
    from fdet_amd.evaluation import DetectionEvaluator
    from fdet_amd.tiling import TiledDetector
    m8 = _m8(net, None, monkeypatch)
    frames = net["frames"][:2]
    bank = A.DeviceImageBank.from_arrays([im.numpy().transpose(1, 2, 0) for im in frames], "cuda")
    from fdet_amd.datasets.utils import ReduceBoundingBoxes
    with torch.no_grad():
        y = m8.forward_frames(frames.cuda())
        # (a random model's confidences lie round 0.5: a threshold just under the largest keeps a handful of cells)
        red = ReduceBoundingBoxes(probability_threshold=float(y[:, 0].max()) - 0.02, iou_threshold=0.5, input_shape=m8.input_shape,
                                  num_of_patches=m8.num_of_patches)
        r, c = red.forward_batch(y)
    before = m8.counters["stem_q8"]
    rows, counts = TiledDetector(m8, tile_sizes=(), include_whole=True, reducer=red, max_out=int(r.shape[1])).detect(bank, [0, 1])
    assert m8.counters["stem_q8"] == before + 1
    assert int(c.sum()) >= 1 and torch.equal(counts, c) and torch.equal(rows, r)
    red = DetectionEvaluator().reducer_for(m8)                             # the evaluator's low-score reducer is built from the model
    r2, c2 = red.forward_batch(m8.forward_frames(frames.cuda()))
    assert int(c2.sum()) >= int(c.sum())
