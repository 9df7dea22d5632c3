"""CPU checks of the int8 separable block: the numpy restatement (tests/q8_sep_cpu_ref.py) against literal loops, the data
conditions of the GPU cases, weight preparation, QuantParams with and without s_b, the accuracy of the int8 network on seeded
random SeparableCNN models against the float oracle (tests/sepcnn_cpu_ref.py), and the host side of the new C-ABI entries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_sep_cpu_ref as RS  # noqa: E402

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = [i for i, c in enumerate(RS.CASES) if c[0][0] * c[0][2] * c[0][3] <= 100]


# ------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("idx", SMALL, ids=[RS.CASE_IDS[i] for i in SMALL])
def test_restatement_equals_the_literal_loops(idx):
    d = RS.make_case(idx)
    got = RS.sepblock(d["x"], d["p"], d["pool"], d["slope"])
    N, C, H, W = d["shape"]
    assert got.dtype == np.int8 and got.shape == ((N, C, H // 2, W // 2) if d["pool"] else (N, C, H, W))
    assert np.array_equal(got, RS.sepblock_loops(d["x"], d["p"], d["pool"], d["slope"]))
    assert got.min() >= -127


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_block_shifts_its_input_by_the_tap(tap):
    d = RS.make_onehot_case(tap)
    want = RS.shifted(d["x"], tap)
    assert np.array_equal(RS.sepblock(d["x"], d["p"], False, d["slope"]), want)
    assert np.array_equal(RS.sepblock_loops(d["x"], d["p"], False, d["slope"]), want)
    assert tap == 4 or not np.array_equal(want, d["x"])


@pytest.mark.parametrize("idx", range(len(RS.CASES)), ids=RS.CASE_IDS)
def test_cases_are_neither_saturated_nor_trivial(idx):
    """Inputs over the full range with both ends present; under 10 % of each of a_q, b_q and y at +-127 and at least one code
    of the case there; "ties": a real share of exact .5 values at each of the three roundings."""
    d = RS.make_case(idx)
    a, b, ts, y = RS.sepblock_parts(d["x"], d["p"], d["pool"], d["slope"])
    assert d["x"].min() == -127 and d["x"].max() == 127
    assert float(d["p"]["skip_mul"]) == 0.75
    sat = [RS.saturation(t) for t in (a, b, y)]
    assert max(sat) < 0.10, sat
    assert sum(int((np.abs(t.astype(np.int32)) == 127).sum()) for t in (a, b, y)) > 0
    assert len(np.unique(y)) > min(40, y.size // 4)
    if d["tag"] == "ties":
        for t in ts:
            assert float(np.mean(np.abs(t - np.floor(t)) == 0.5)) > 0.1
    else:
        for k in ("w1", "wd", "w2"):
            assert d["p"][k].min() == -127 and d["p"][k].max() == 127


def test_depthwise_accumulator_needs_more_than_16_bits():
    a = np.full((1, 64, 3, 3), 127, np.int8)
    wd = np.full((64, 3, 3), 127, np.int8)
    acc = RS.depthwise_acc(a, wd)
    assert int(acc[0, 0, 1, 1]) == 9 * 127 * 127 == 145161 and int(acc[0, 0, 0, 0]) == 4 * 127 * 127


# ------------------------------------------------------------------------------------------------------- preparation
def test_weight_preparation():
    from fdet_amd.quantize import prepare_sepblock
    rng = np.random.default_rng(7)
    C = 64
    w1 = rng.normal(0, 0.1, (C, C, 1, 1)).astype(F32)
    wd = rng.normal(0, 0.3, (C, 1, 3, 3)).astype(F32)
    w2 = rng.normal(0, 0.1, (C, C, 1, 1)).astype(F32)
    w1[3] = 0                                                              # a channel of zeros gets scale 1
    wd[5] = 0
    s_in, s_a, s_b, s_out = F32(0.031), F32(0.017), F32(0.023), F32(0.029)
    p = RS.prepare_block(w1, wd, w2, s_in, s_a, s_b, s_out)
    w1_q, mul1, wd_q, mul2, w2_q, mul3, sm = prepare_sepblock(w1, wd, w2, s_in, s_a, s_b, s_out)
    assert np.array_equal(w1_q.reshape(C, C), p["w1"]) and np.array_equal(wd_q.reshape(C, 3, 3), p["wd"])
    assert np.array_equal(w2_q.reshape(C, C), p["w2"])
    for got, want in ((mul1, p["mul1"]), (mul2, p["mul2"]), (mul3, p["mul3"])):
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert F32(sm) == p["skip_mul"] == F32(s_in / s_out)
    assert np.abs(p["w1"]).max(axis=1)[[0, 1, 2]].tolist() == [127] * 3 and not p["w1"][3].any()
    assert p["mul1"][3] == (F32(1.0) * s_in) / s_a and p["mul2"][5] == (F32(1.0) * s_a) / s_b
    s_w = R.weight_scales(wd)
    assert np.array_equal(p["mul2"], (s_w * s_a) / s_b)
    # the kernel's depthwise layout is a plain permutation
    pk = RS.pack_dw(p["wd"])
    assert pk.shape == (9, C) and all(pk[3 * ky + kx, c] == p["wd"][c, ky, kx] for c in (0, 17, 63) for ky in range(3) for kx in range(3))


# ------------------------------------------------------------------------------------------------------- QuantParams
def test_quant_params_with_and_without_s_b(tmp_path):
    from fdet_amd.quantize import ActivationObserver, QuantParams
    s_h, s_a, s_b = np.linspace(0.01, 0.05, 4), np.linspace(0.02, 0.03, 3), np.linspace(0.04, 0.06, 3)
    plain = QuantParams(s_h, s_a, "percentile", 99.9, 5)
    sep = QuantParams(s_h, s_a, "percentile", 99.9, 5, s_b=s_b)
    assert plain.s_b is None and sep.s_b.dtype == np.float32 and sep.num_blocks == 3
    assert plain == QuantParams(s_h, s_a, "percentile", 99.9, 5) and sep == QuantParams(s_h, s_a, "percentile", 99.9, 5, s_b)
    assert plain != sep and sep != plain and sep != QuantParams(s_h, s_a, "percentile", 99.9, 5, s_b * 2)
    a, b = str(tmp_path / "plain.npz"), str(tmp_path / "sep.npz")
    plain.save(a)
    sep.save(b)
    with np.load(a) as z:                                                  # a file without s_b is what it was
        assert sorted(z.files) == ["images_seen", "method", "percentile", "s_a", "s_h"]
        assert z["s_h"].tobytes() == plain.s_h.tobytes() and z["s_a"].tobytes() == plain.s_a.tobytes()
    back = QuantParams.load(a)
    assert back == plain and back.s_b is None and back.s_h.tobytes() == plain.s_h.tobytes() and back.s_a.tobytes() == plain.s_a.tobytes()
    back = QuantParams.load(b)
    assert back == sep and back.s_b.tobytes() == sep.s_b.tobytes() and back.percentile == 99.9 and back.images_seen == 5
    for bad in ([0.04, 0.05], [0.04, 0.05, 0.0], [0.04, 0.05, float("nan")], [0.04, -0.05, 0.06]):
        with pytest.raises(ValueError):
            QuantParams(s_h, s_a, s_b=bad)
    obs = ActivationObserver(2, with_b=True)
    t = torch.tensor
    obs.observe([t([[1.0]]), t([[2.0]]), t([[0.0]])], [t([[3.0]]), t([[4.0]])], [t([[5.0]]), t([[0.0]])])
    qp = obs.params()
    assert np.array_equal(qp.s_b, np.array([5.0, 127.0], F32) / F32(127.0)) and qp.s_h[2] == 1.0
    with pytest.raises(ValueError):
        obs.observe([t([[1.0]])] * 3, [t([[1.0]])] * 2)                    # an observer made with_b wants b
    with pytest.raises(ValueError):
        ActivationObserver(2).observe([t([[1.0]])] * 3, [t([[1.0]])] * 2, [t([[1.0]])] * 2)
    assert ActivationObserver(2).b is None


def test_quant_params_file_of_the_parent_format_loads_unchanged():
    """tests/golden/q8_quantparams_v1.npz was written by QuantParams.save before s_b existed."""
    from fdet_amd.quantize import QuantParams
    qp = QuantParams.load(os.path.join(GOLDEN, "q8_quantparams_v1.npz"))
    assert qp.s_b is None and qp.num_blocks == 10 and qp.method == "percentile" and qp.percentile == 99.99 and qp.images_seen == 37
    assert np.array_equal(qp.s_h, np.linspace(0.01, 0.05, 11).astype(F32)) and np.array_equal(qp.s_a, np.linspace(0.02, 0.03, 10).astype(F32))
    assert qp == QuantParams(np.linspace(0.01, 0.05, 11), np.linspace(0.02, 0.03, 10), "percentile", 99.99, 37)


# ------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("i", range(len(RS.ACCURACY_MODELS)), ids=[f"seed{m[0]}-{m[1]}" for m in RS.ACCURACY_MODELS])
def test_int8_network_on_seeded_random_models(i):
    """Seeded random SeparableCNN(filters=64), three seeded uint8 frames, absmax scales from the float oracle's activations:
    |y_int8 - y_float| over the maps stays within the recorded values (q8_sep_cpu_ref.ACCURACY_RECORDED) times
    1.25, the margin of the stem test in test_q8_pool_stem_host.py.  Accuracy on trained weights is unpinned: no trained
    SeparableCNN archive exists."""
    _, P, frames, head_pad = RS.accuracy_model(i)
    hs, as_, bs, y = RS.float_forward(P, frames, head_pad)
    s_h, s_a, s_b = RS.absmax_scales(hs, as_, bs)
    q0, outs, _, y8 = RS.model_q(frames, P, s_h, s_a, s_b, head_pad)
    assert tuple(y8.shape) == tuple(y.shape) == (3, 5, 16, 16)
    assert [o.shape[2] for o in outs] == ([30, 15] if frames.shape[2] == 480 else [32, 16]) + [outs[-1].shape[2]] * 8
    d = (y8 - y).abs()
    sat = sum(int((np.abs(o.astype(np.int32)) == 127).sum()) for o in outs) / sum(o.size for o in outs)
    print(f"model {RS.ACCURACY_MODELS[i]}: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}, block outputs at +-127 {sat:.2e}, "
          f"y in {float(y.min()):.4f} .. {float(y.max()):.4f}")
    rec_max, rec_mean = RS.ACCURACY_RECORDED[i]
    assert float(d.max()) <= 1.25 * rec_max
    assert float(d.mean()) <= 1.25 * rec_mean


# ------------------------------------------------------------------------------------------------------- refusals
def test_int8_separable_model_refuses_what_it_cannot_run():
    from fdet_amd import FdetError
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.models.SeparableCNN import SeparableCNN
    from fdet_amd.quantize import Int8PoolResnet, Int8SeparableCNN, QuantParams, calibrate, quantize_model
    m = SeparableCNN(filters=64, input_shape=(3, 480, 480), num_of_residual_blocks=3, output_padding=3)
    qp = QuantParams([1.0] * 4, [1.0] * 3, s_b=[1.0] * 3)
    with pytest.raises(TypeError, match="SeparableCNN only"):
        Int8SeparableCNN(PoolResnet(64, (3, 480, 480), 10, num_of_residual_blocks=3), qp)
    with pytest.raises(TypeError, match="PoolResnet only"):
        Int8PoolResnet(m, qp)
    with pytest.raises(TypeError, match="QuantParams"):
        Int8SeparableCNN(m, None)
    with pytest.raises(ValueError, match="s_b"):
        Int8SeparableCNN(m, QuantParams([1.0] * 4, [1.0] * 3))
    with pytest.raises(ValueError, match="residual blocks"):
        Int8SeparableCNN(m, QuantParams([1.0] * 3, [1.0] * 2, s_b=[1.0] * 2))
    with pytest.raises(FdetError, match="GPU only"):
        Int8SeparableCNN(m, qp)                                            # a CPU model: no CPU fallback
    with pytest.raises(ValueError, match="no image"):
        calibrate(m, [])                                                   # a SeparableCNN is accepted; nothing was seen
    with pytest.raises(TypeError, match="PoolResnet only"):
        calibrate(torch.nn.Linear(2, 2), [])
    with pytest.raises(ValueError, match="stem="):
        quantize_model(m, [], stem="integer")
    m.engine.p16 = True                                                    # (the separable engine never is; calibrate asks all the same)
    with pytest.raises(FdetError, match="precision16"):
        calibrate(m, [])
    assert callable(getattr(m, "quantize"))


# ------------------------------------------------------------------------------------------------------- C-ABI, host side
def test_planner_and_argument_rejection_need_no_gpu():
    from fdet_amd import _native
    from fdet_amd import hotpath as hp
    L = _native.lib()
    for C, H, W, ok in ((64, 1, 1, 1), (128, 4096, 4096, 1), (64, 4097, 4, 0), (64, 0, 4, 0), (32, 8, 8, 0), (192, 8, 8, 0), (256, 8, 8, 0)):
        assert L.fdet_q8_sepblock_supported(C, H, W) == ok, (C, H, W)
    for C, H, W, ok in ((64, 16, 16, 1), (64, 1, 1, 1), (64, 17, 16, 0), (128, 15, 15, 0), (64, 0, 1, 0)):
        assert L.fdet_q8_sepchain_supported(C, H, W) == ok, (C, H, W)
    # the planner: a whole small map is one tile; the model's levels fit the budget of two workgroups per CU; pooled tiles are even
    assert hp.q8_sepblock_plan(64, 15, 15)[:2] == (15, 15) and hp.q8_sepblock_plan(64, 16, 16)[:2] == (16, 16)
    assert hp.q8_sepblock_plan(64, 15, 15, pool=True) is None and hp.q8_sepblock_plan(96, 8, 8) is None
    for C, H, pool in ((64, 60, True), (64, 30, True), (128, 60, True), (64, 64, True), (64, 4096, False), (128, 4096, True), (64, 17, False)):
        r, c, lds = hp.q8_sepblock_plan(C, H, H, pool)
        assert 1 <= r <= H + 1 and 1 <= c <= H + 1 and (not pool or (r % 2 == 0 and c % 2 == 0)), (C, H, pool, r, c)
        assert lds == 2 * C * C + 21 * C + C * (2 * (r + 2) * (c + 2) + r * c) and lds <= 80 * 1024, (C, H, pool, r, c, lds)
    z = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused first
    args = (z, z, z, z, z, z, z, 0.75)
    rc = L.fdet_q8_sepblock(*args, ctypes.c_void_p(512), 1, 96, 8, 8, 0, 0, 0, 0.2, None)
    assert rc != 0 and b"unsupported shape" in L.fdet_last_error()
    rc = L.fdet_q8_sepblock(*args, ctypes.c_void_p(512), 1, 64, 7, 8, 1, 0, 0, 0.2, None)
    assert rc != 0 and b"even H and W" in L.fdet_last_error()
    rc = L.fdet_q8_sepblock(*args, ctypes.c_void_p(512), 1, 64, 8, 8, 0, 4, 0, 0.2, None)
    assert rc != 0 and b"both" in L.fdet_last_error()
    rc = L.fdet_q8_sepblock(*args, ctypes.c_void_p(512), 1, 64, 8, 8, 1, 3, 4, 0.2, None)
    assert rc != 0 and b"even when pooled" in L.fdet_last_error()
    rc = L.fdet_q8_sepblock(*args, ctypes.c_void_p(512), 1, 64, 64, 64, 0, 64, 64, 0.2, None)
    assert rc != 0 and b"LDS" in L.fdet_last_error()
    rc = L.fdet_q8_sepblock(*args, ctypes.c_void_p(520), 1, 64, 8, 8, 0, 0, 0, 0.2, None)
    assert rc != 0 and b"16-byte aligned" in L.fdet_last_error()
    rc = L.fdet_q8_sepblock(*args, z, 1, 64, 8, 8, 0, 0, 0, 0.2, None)
    assert rc != 0 and b"alias" in L.fdet_last_error()
    arr = (ctypes.c_void_p * 17)(*([256] * 17))
    sm = (ctypes.c_float * 17)(*([0.75] * 17))
    for nb, C, H, msg in ((0, 64, 15, b"nblocks"), (17, 64, 15, b"nblocks"), (2, 128, 15, b"unsupported shape"), (2, 64, 17, b"unsupported shape")):
        rc = L.fdet_q8_sepchain(z, arr, arr, arr, arr, arr, arr, sm, None, ctypes.c_void_p(512), 1.0, nb, 1, C, H, H, 0.2, None)
        assert rc != 0 and msg in L.fdet_last_error(), (nb, C, H)
    rc = L.fdet_q8_sepchain(z, arr, arr, arr, arr, arr, arr, sm, None, None, 1.0, 2, 1, 64, 15, 15, 0.2, None)
    assert rc != 0 and b"needs an output" in L.fdet_last_error()


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from fdet_amd import hotpath as hp
    w = torch.zeros(64, 64, 1, 1, dtype=torch.int8)
    assert hp.q8_pack_sep_pw(w).shape == (4096,)
    wd = torch.arange(64 * 9, dtype=torch.int32).remainder(127).to(torch.int8).reshape(64, 1, 3, 3)
    assert torch.equal(hp.q8_pack_sep_dw(wd).reshape(9, 64), wd.reshape(64, 9).t())
    for bad in (torch.zeros(64, 32, 1, 1, dtype=torch.int8), torch.zeros(64, 64, 1, 1)):
        with pytest.raises(ValueError):
            hp.q8_pack_sep_pw(bad)
    with pytest.raises(ValueError):
        hp.q8_pack_sep_dw(torch.zeros(64, 1, 3, 3))
    with pytest.raises(ValueError):
        hp.q8_sepblock(torch.zeros(1), w, None, wd, None, w, None, 0.75, None)
    with pytest.raises(ValueError):
        hp.Q8SepChainWeights([], [])
    with pytest.raises(ValueError):
        hp.q8_sepchain(torch.zeros(1), None)
