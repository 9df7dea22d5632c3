"""CPU checks of the int8 inference path: the numpy restatement (tests/q8_cpu_ref.py) against a literal loop version of the
contract, the data conditions of the random cases the GPU file reuses, the accuracy of the int8 trunk on the trained medium
archive (g16), QuantParams, and the host side of the C-ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("with_skip,pool", [(False, False), (True, False), (True, True)])
def test_restatement_equals_the_literal_loops(with_skip, pool):
    rng = np.random.default_rng(7)
    N, C, H, W = 1, 64, 4, 6
    x = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8)
    w = rng.integers(-127, 128, (C, C, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, C).astype(np.int32)
    mul = np.exp2(rng.uniform(-12, -8, C)).astype(F32)
    skip = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8) if with_skip else None
    sm = F32(0.75) if with_skip else None
    got = R.conv3x3(x, w, b, mul, skip, sm, pool)
    want = R.conv3x3_loops(x, w, b, mul, skip, sm, pool)
    assert got.dtype == np.int8 and got.shape == want.shape
    assert np.array_equal(got, want)


def test_rounding_ties_go_to_even_and_the_clamp_never_yields_minus_128():
    t = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.5, -126.5, -127.5, -128.0, -1e9, 1e9, 127.49, -127.51], F32)
    assert R.rint_clamp(t).tolist() == [0, 2, 2, 0, -2, -2, 126, 127, -126, -127, -127, -127, 127, 127, -127]
    # the quantiser: ties, values beyond +-127 s, a NaN, infinities
    s = F32(0.25)
    x = np.array([0.125, 0.375, 0.625, -0.125, -0.375, 31.75, 31.875, 100.0, -100.0, np.nan, np.inf, -np.inf], F32)
    assert R.quantize(x, s).tolist() == [0, 2, 2, 0, -2, 127, 127, 127, -127, 0, 127, -127]
    every = R.quantize(np.linspace(-200, 200, 100001).astype(F32), F32(1.0))
    assert every.min() == -127 and every.max() == 127
    # a conv whose accumulator is exactly odd with mul 0.5: ties in the epilogue
    acc = np.arange(-9, 10, dtype=np.int64).reshape(1, 1, 1, 19).repeat(2, axis=1)
    q = R.rint_clamp(R.epilogue_float(acc, np.full(2, 0.5, F32), slope=F32(1.0)))
    assert q[0, 0, 0].tolist() == [-4, -4, -4, -3, -2, -2, -2, -1, 0, 0, 0, 1, 2, 2, 2, 3, 4, 4, 4]


def test_pool_after_requantise_equals_requantise_after_pool():
    rng = np.random.default_rng(3)
    t = (rng.standard_normal((2, 8, 6, 10)) * 90).astype(F32)
    t.reshape(-1)[::7] = np.rint(t.reshape(-1)[::7]) + F32(0.5)            # plenty of ties
    a = R.maxpool2(R.rint_clamp(t))
    N, C, H, W = t.shape
    b = R.rint_clamp(t.reshape(N, C, H // 2, 2, W // 2, 2).max(axis=(3, 5)))
    assert np.array_equal(a, b)


def test_weight_and_bias_preparation():
    w = np.zeros((4, 64, 3, 3), F32)
    w[0, 0, 0, 0], w[0, 1, 1, 1] = 2.54, -1.27
    w[1] = -0.5
    w[3, 5, 2, 2] = 1e-3
    s_w = R.weight_scales(w)
    assert s_w[2] == 1.0 and s_w[0] == F32(2.54) / F32(127) and s_w[1] == F32(0.5) / F32(127)
    w_q = R.quantize_weights(w, s_w)
    assert w_q[0, 0, 0, 0] == 127 and w_q[0, 1, 1, 1] in (-63, -64) and (w_q[1] == -127).all() and not w_q[2].any()
    assert w_q.min() >= -127
    b_q = R.quantize_bias(np.array([1.0, -1.0, 3.0, 0.0], F32), s_w, F32(0.5))
    assert b_q.dtype == np.int32
    assert b_q[0] == int(np.rint(1.0 / (float(s_w[0]) * 0.5))) and b_q[2] == 6 and b_q[3] == 0
    # the package prepares the same integers and multipliers
    from fdet_amd import quantize as Q
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((64, 64, 3, 3)) * 0.05).astype(F32)
    w[7] = 0
    b = rng.standard_normal(64).astype(F32)
    for got, want in zip(Q.prepare_conv(w, b, F32(0.031), F32(0.017)), R.prepare_conv(w, b, F32(0.031), F32(0.017))):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    pk = R.pack_weights(R.quantize_weights(w, R.weight_scales(w)))
    got = Q.hp.q8_pack_weights(torch.from_numpy(R.quantize_weights(w, R.weight_scales(w)))).numpy()
    assert np.array_equal(got, pk.reshape(-1))


# ------------------------------------------------------------------------------------------------------- the random cases
@pytest.mark.parametrize("idx", range(len(R.CASES)))
def test_random_cases_are_neither_saturated_nor_trivial(idx):
    """Under the restatement alone: 1 % .. 30 % of the outputs at +-127, at least 10 % of the pre-activations negative."""
    d = R.make_case(idx)
    acc = R.conv_acc(d["x"], d["w"], d["b"])
    pre = acc.astype(F32) * d["mul"][None, :, None, None]
    out = R.conv3x3(d["x"], d["w"], d["b"], d["mul"], d["skip"], d["skip_mul"], d["pool"])
    sat = float(np.mean(np.abs(out.astype(np.int32)) == 127))
    neg = float(np.mean(pre < 0))
    print(f"case {idx} {R.CASES[idx]}: saturated {sat:.4f}, negative pre-activations {neg:.4f}")
    assert 0.01 <= sat <= 0.30
    assert neg >= 0.10
    assert out.min() >= -127
    if d["tag"] == "ties":
        t = R.epilogue_float(acc, d["mul"])
        assert np.all(d["mul"] == 0.5) and float(np.mean(np.abs(t - np.floor(t)) == 0.5)) > 0.2
    else:
        assert d["x"].min() == -127 and d["x"].max() == 127 and d["w"].min() == -127 and d["w"].max() == 127


# ------------------------------------------------------------------------------------------------------- accuracy on g16
# measured with this file (abs-max calibration on the three stored frames): see the test's docstring
G16_MAX, G16_MEAN = 0.059795, 0.002679


def _float_intermediates(P, x):
    """torch fp32 ops on the CPU, as the oracle: stem output, block inputs h_0..h_nb, first-conv outputs a_k."""
    h = F.conv2d(x, P["conv1.weight"], P["conv1.bias"], stride=8, padding=2)
    hs, as_ = [], []
    for k in range(10):
        n = f"residual_blocks.{k}"
        hs.append(h)
        a = F.leaky_relu(F.conv2d(h, P[n + ".conv1.weight"], P[n + ".conv1.bias"], padding=1), 0.2)
        as_.append(a)
        c = F.leaky_relu(F.conv2d(a, P[n + ".conv2.weight"], P[n + ".conv2.bias"], padding=1), 0.2)
        e = c + h
        h = F.max_pool2d(e, 2) if e.shape[2] > 20 else e
    hs.append(h)
    return hs, as_


def test_int8_trunk_on_the_trained_medium_archive(golden):
    """g16 weights, the three g6 frames, abs-max calibration on those frames; float stem -> restatement trunk -> float head
    against the reference y stored in g16.  Measured: max |dy| 0.059795, mean |dy| 0.002679 (the bound is the measured value
    times 1.25); the cells with confidence > 0.7 are the reference's."""
    from fdet_amd import quantize as Q
    g = golden("g16_trained_medium")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    x = golden("g6_trained_small")["images"].float() / 255.0
    with torch.no_grad():
        hs, as_ = _float_intermediates(P, x)
        obs = Q.ActivationObserver(10, "absmax")
        obs.observe(hs, as_)
        qp = obs.params()
        assert qp.images_seen == 3 and qp.method == "absmax"
        assert qp.s_h[0] == F32(float(hs[0].abs().max())) / F32(127.0)
        Pn = {k: v.numpy() for k, v in P.items()}
        outs, hd = R.trunk(hs[0].numpy(), Pn, qp.s_h, qp.s_a, S=10)
        y = torch.sigmoid(F.conv2d(torch.from_numpy(hd), P["out.weight"], P["out.bias"]))
    assert [o.shape[2] for o in outs] == [30, 15] + [15] * 8
    d = (y - g["y"]).abs()
    sat = float(np.mean([np.mean(np.abs(o.astype(np.int32)) == 127) for o in outs]))       # mean of the ten blocks' shares
    n_sat, n_out = sum(int((np.abs(o.astype(np.int32)) == 127).sum()) for o in outs), sum(o.size for o in outs)
    print(f"g16 int8 trunk: {n_sat} of {n_out} block outputs at +-127 ({n_sat / n_out:.2e} of all outputs)")
    print(f"g16 int8 trunk: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}, saturated share {sat:.2e}")
    assert float(d.max()) <= 1.25 * G16_MAX
    assert float(d.mean()) <= 1.25 * G16_MEAN
    assert torch.equal(y[:, 0] > 0.7, g["y"][:, 0] > 0.7) and int((y[:, 0] > 0.7).sum()) >= 2


# ------------------------------------------------------------------------------------------------------- QuantParams
def test_quant_params_round_trip(tmp_path):
    from fdet_amd.quantize import ActivationObserver, QuantParams
    qp = QuantParams(np.linspace(0.01, 0.05, 11), np.linspace(0.02, 0.03, 10), "percentile", 99.99, 37)
    path = str(tmp_path / "qp.npz")
    qp.save(path)
    back = QuantParams.load(path)
    assert back == qp and back.s_h.dtype == np.float32 and back.percentile == 99.99 and back.images_seen == 37
    qp2 = QuantParams([0.5, 0.25], [1.0])
    qp2.save(path)
    assert QuantParams.load(path) == qp2 and QuantParams.load(path).percentile is None and qp2.method == "explicit"
    for bad in (([0.5], [1.0]), ([0.5, 0.0], [1.0]), ([0.5, np.nan], [1.0]), ([0.5, 1.0], [-1.0]), ([0.5, 1.0], [])):
        with pytest.raises(ValueError):
            QuantParams(*bad)
    # percentile: the k-th smallest magnitude with k = ceil(p / 100 * n), the largest over the batches
    obs = ActivationObserver(1, "percentile", 90.0)
    t = torch.arange(1, 101, dtype=torch.float32).reshape(1, 1, 10, 10)
    obs.observe([t, -t * 2], [t * 0])
    obs.observe([t / 2, t], [t * 0])
    p = obs.params()
    assert p.s_h.tolist() == [F32(90.0) / F32(127.0), F32(180.0) / F32(127.0)] and p.s_a.tolist() == [1.0] and p.images_seen == 2
    with pytest.raises(ValueError):
        ActivationObserver(1, "percentile")
    with pytest.raises(ValueError):
        ActivationObserver(1, "absmax").params()


def test_int8_model_refuses_other_models():
    from fdet_amd import FdetError
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.models.Resnet import Resnet
    from fdet_amd.quantize import Int8PoolResnet, QuantParams, calibrate
    qp = QuantParams([1.0] * 3, [1.0] * 2)
    with pytest.raises(TypeError, match="PoolResnet only"):
        Int8PoolResnet(Resnet(8, (3, 64, 64), 4, num_of_residual_blocks=2), qp)
    with pytest.raises(TypeError, match="PoolResnet only"):
        calibrate(torch.nn.Conv2d(3, 3, 1), [])
    m = PoolResnet(64, (3, 480, 480), 10, num_of_residual_blocks=2)
    with pytest.raises(ValueError, match="residual blocks"):
        Int8PoolResnet(m, QuantParams([1.0] * 4, [1.0] * 3))
    with pytest.raises(FdetError, match="GPU only"):
        Int8PoolResnet(m, qp)                                                # a CPU model: no CPU fallback


# ------------------------------------------------------------------------------------------------------- C-ABI, host side
def test_size_helpers_and_argument_rejection_need_no_gpu():
    from fdet_amd import _native
    L = _native.lib()
    assert [L.fdet_q8_supported(c, 15, 15) for c in (64, 128, 192, 256, 320, 32, 96, 0)] == [1, 1, 1, 1, 0, 0, 0, 0]
    assert L.fdet_q8_supported(64, 1, 1) == 1 and L.fdet_q8_supported(64, 0, 5) == 0 and L.fdet_q8_supported(64, 5, -1) == 0
    assert L.fdet_q8_supported(64, 61, 17) == 1
    assert L.fdet_q8_act_bytes(256, 64, 60, 60) == 256 * 62 * 62 * 64
    assert L.fdet_q8_act_bytes(1, 128, 1, 3) == 3 * 5 * 128
    assert L.fdet_q8_act_bytes(1, 192, 5, 18) == L.fdet_q8x_act_bytes(1, 192, 5, 18) == 7 * 20 * 192    # one layout function
    assert L.fdet_q8_act_bytes(2, 60, 15, 15) == 0 and L.fdet_q8_act_bytes(0, 64, 15, 15) == 0
    assert L.fdet_q8_act_bytes(4096, 256, 60, 60) == 0                       # 2^31 bytes and more
    buf = ctypes.create_string_buffer(64)                                    # a host address: only ever compared with NULL
    p = ctypes.addressof(buf)
    p16 = (p + 15) & ~15
    rc = L.fdet_q8_conv3x3(None, None, None, None, None, 0.0, None, 1, 64, 4, 4, 0, 0.2, None)
    assert rc == -1 and b"q8_conv3x3" in L.fdet_last_error()
    assert L.fdet_q8_conv3x3(p16, p16, p16, p16, None, 0.0, p16 + 16, 1, 48, 4, 4, 0, 0.2, None) == -1      # channels
    assert L.fdet_q8_conv3x3(p16, p16, p16, p16, None, 0.0, p16 + 16, 1, 64, 5, 4, 1, 0.2, None) == -1      # odd pooled map
    assert b"even" in L.fdet_last_error()
    assert L.fdet_q8_conv3x3(p16, p16, p16, p16, None, 0.0, p16 + 16, 1, 64, 4, 4, 2, 0.2, None) == -1      # pool flag
    assert L.fdet_q8_conv3x3(p16 + 4, p16, p16, p16, None, 0.0, p16 + 16, 1, 64, 4, 4, 0, 0.2, None) == -1  # alignment
    assert b"aligned" in L.fdet_last_error()
    assert L.fdet_q8_conv3x3(p16, p16, p16, p16, None, 0.0, p16, 1, 64, 4, 4, 0, 0.2, None) == -1           # y aliases x
    assert L.fdet_q8_quantize(None, 1.0, p16, 1, 64, 4, 4, None) == -1 and b"q8_quantize" in L.fdet_last_error()
    assert L.fdet_q8_quantize(p16, 0.0, p16, 1, 64, 4, 4, None) == -1 and b"scale" in L.fdet_last_error()
    assert L.fdet_q8_quantize(p16, float("nan"), p16, 1, 64, 4, 4, None) == -1
    assert L.fdet_q8_dequantize(p16, 1.0, None, 1, 64, 4, 4, None) == -1 and b"q8_dequantize" in L.fdet_last_error()
    assert L.fdet_q8_dequantize(p16, 1.0, p16, 1, 65, 4, 4, None) == -1
    assert L.fdet_q8_dequantize(p16, float("inf"), p16, 1, 64, 4, 4, None) == -1


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from fdet_amd import FdetError
    from fdet_amd import hotpath as hp
    with pytest.raises(FdetError):
        hp.Q8Tensor(1, 48, 4, 4, "cpu")
    with pytest.raises(ValueError):
        hp.q8_pack_weights(torch.zeros(64, 48, 3, 3, dtype=torch.int8))
    with pytest.raises(ValueError):
        hp.Q8Tensor(1, 64, 4, 4, "cpu", storage=torch.zeros(16, dtype=torch.int8))


def test_scripts_check_the_int8_options(capsys):
    from fdet_amd import detect_images as D
    from fdet_amd import run_validation_epoch as V
    io = ["--images", "in", "--out", "out.txt"]
    for mod, argv, msg in ((D, io + ["--int8", "--precision", "16"], "--int8 and --precision 16"),
                           (V, ["--int8", "--precision", "16"], "--int8 and --precision 16"),
                           (D, io + ["--calib", "dir"], "--calib needs --int8"),
                           (V, ["--calib-images", "4"], "--calib-images needs --int8"),
                           (D, io + ["--int8", "--model", "resnet"], "poolresnet only"),
                           (V, ["--int8", "--calib-images", "0"], "--calib-images must be >= 1")):
        with pytest.raises(SystemExit):
            mod.main(argv)
        assert msg in capsys.readouterr().err
