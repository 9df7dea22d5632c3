"""CPU checks of Int8Resnet's arithmetic: the numpy restatement (tests/q8_resnet_cpu_ref.py) against q8_cpu_ref and literal
loops, the shift identity the integer stem kernel relies on, the accuracy of the whole int8 network on the trained medium
archive (g22), and the host side of the new C-ABI entry."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_resnet_cpu_ref as RR  # noqa: E402

F32 = np.float32


def _stem_case(seed, N, F_, H, W):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (N, 3, H, W)).astype(np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    w = rng.integers(-127, 128, (F_, 3, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, F_).astype(np.int32)
    mul = np.exp2(rng.uniform(-11.5, -8.5, F_)).astype(F32)
    return x, w, b, mul


# ------------------------------------------------------------------------------------------------------- restatement
def test_stem_restatement_equals_the_literal_loops():
    x, w, b, mul = _stem_case(11, 2, 8, 6, 10)
    got = RR.stem3_q(x, w, b, mul)
    assert got.dtype == np.int8 and got.shape == (2, 8, 3, 5)
    assert np.array_equal(got, RR.stem3_loops(x, w, b, mul))
    assert 0.005 <= float(np.mean(np.abs(got.astype(np.int32)) == 127)) <= 0.5 and got.min() >= -127
    one = RR.stem3_q(x[:, :, :2, :2], w, b, mul)                            # one output pixel: five of nine taps outside
    assert one.shape == (2, 8, 1, 1) and np.array_equal(one, RR.stem3_loops(x[:, :, :2, :2], w, b, mul))


def test_torch_conv_accumulator_equals_q8_cpu_ref():
    rng = np.random.default_rng(12)
    x = rng.integers(-127, 128, (2, 64, 5, 7)).astype(np.int8)
    w = rng.integers(-127, 128, (64, 64, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, 64).astype(np.int32)
    assert np.array_equal(RR.conv_acc(x, w, b), R.conv_acc(x, w, b))
    mul = np.exp2(rng.uniform(-12, -8, 64)).astype(F32)
    sk = rng.integers(-127, 128, x.shape).astype(np.int8)
    assert np.array_equal(RR.conv3x3(x[:, :, :4, :6], w, b, mul, sk[:, :, :4, :6], F32(0.75), True),
                          R.conv3x3(x[:, :, :4, :6], w, b, mul, sk[:, :, :4, :6], F32(0.75), True))


def test_trunk_pools_while_the_map_is_larger_than_S():
    rng = np.random.default_rng(13)
    P = {}
    for k in range(3):
        for c in ("conv1", "conv2"):
            P[f"residual_blocks.{k}.{c}.weight"] = (rng.standard_normal((64, 64, 3, 3)) * 0.04).astype(F32)
            P[f"residual_blocks.{k}.{c}.bias"] = (rng.standard_normal(64) * 0.1).astype(F32)
    q0 = rng.integers(-127, 128, (1, 64, 8, 8)).astype(np.int8)
    s_h, s_a = np.full(4, 0.03, F32), np.full(3, 0.03, F32)
    outs, hd = RR.trunk_q(q0, P, s_h, s_a, S=4)
    assert [o.shape[2] for o in outs] == [4, 4, 4] and hd.shape == (1, 64, 4, 4)
    T = R.prepare_trunk(P, s_h, s_a)
    h1 = R.block(q0, *T[0], pool=True)[1]
    h2 = R.block(h1, *T[1], pool=False)[1]
    assert np.array_equal(outs[0], h1) and np.array_equal(outs[1], h2)
    assert np.array_equal(hd, R.dequantize(outs[2], s_h[-1]))


def test_shift_identity_of_the_signed_staging():
    """sum x * w with zero padding == sum (x - 128) * w over all 27 taps with -128 padding + 128 * sum(w), in integers."""
    for seed, shape in ((21, (2, 64, 6, 10)), (22, (1, 64, 2, 2)), (23, (1, 64, 4, 34))):
        x, w, b, _ = _stem_case(seed, *shape)
        assert np.array_equal(RR.stem3_shifted_acc(x, w, b), RR.stem3_acc(x, w, b))
    x = np.full((1, 3, 4, 4), 255, np.uint8)
    for sign in (127, -127):
        w = np.full((64, 3, 3, 3), sign, np.int8)
        b = np.zeros(64, np.int32)
        acc = RR.stem3_acc(x, w, b)
        assert np.array_equal(RR.stem3_shifted_acc(x, w, b), acc) and abs(int(acc[0, 0, 1, 1])) == 27 * 255 * 127
    pk = RR.pack_stem_weights(_stem_case(5, 1, 64, 2, 2)[1])
    assert pk.shape == (64, 32) and not pk[:, 27:].any()
    from fdet_amd import hotpath as hp
    w = _stem_case(5, 1, 64, 2, 2)[1]
    assert np.array_equal(hp.q8_pack_stem_weights(torch.from_numpy(w)).numpy(), pk.reshape(-1))
    with pytest.raises(ValueError):
        hp.q8_pack_stem_weights(torch.zeros(48, 3, 3, 3, dtype=torch.int8))
    with pytest.raises(ValueError):
        hp.q8_pack_stem_weights(torch.zeros(64, 3, 3, 3))


# ------------------------------------------------------------------------------------------------------- accuracy on g22
# measured with this file (abs-max calibration on the three stored frames): see the test's docstring
G22_MAX, G22_MEAN = 0.064129, 0.002336


@pytest.fixture(scope="module")
def g22_int8():
    g = RR.load_g22()
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    images = torch.from_numpy(np.load(os.path.join(RR.GOLDEN, "g6_trained_small.npz"))["images"])
    hs, as_, y_f = RR.float_intermediates(P, images.float() / 255.0, 15)
    s_h, s_a = RR.absmax_scales(hs, as_)
    q0, outs, y = RR.model_q(images.numpy(), {k: v.numpy() for k, v in P.items()}, s_h, s_a, 15)
    return g, P, images, (hs, as_), (s_h, s_a), q0, outs, y, y_f


def test_int8_resnet_on_the_trained_medium_archive(g22_int8):
    """g22 weights, the three g6 frames, abs-max scales from a torch fp32 forward of those frames; integer stem -> restatement
    trunk -> float head against the reference's y stored in g22.  Measured: max |dy| 0.064129, mean |dy| 0.002336 (the bound
    is the measured value times 1.25, the rule of test_int8_trunk_on_the_trained_medium_archive).  The cells above 0.7 are
    not asserted: the reference's nearest confidences, 0.714 and 0.686, lie inside max |dy|."""
    from fdet_amd import quantize as Q
    g, P, images, (hs, as_), (s_h, s_a), q0, outs, y, y_f = g22_int8
    assert float((y_f - g["y"]).abs().max()) <= 1e-5                        # the torch forward is the reference's
    obs = Q.ActivationObserver(10, "absmax")
    obs.observe(hs, as_)
    qp = obs.params()
    assert np.array_equal(qp.s_h, s_h) and np.array_equal(qp.s_a, s_a)      # the package's observer gives these scales
    assert tuple(q0.shape) == (3, 64, 240, 240) and [o.shape[2] for o in outs] == [120, 60, 30, 15] + [15] * 6
    w_q, b_q, mul = Q.prepare_conv(P["conv1.weight"].numpy(), P["conv1.bias"].numpy(), Q.STEM_IN_SCALE, s_h[0])
    acc = RR.stem3_acc(images.numpy(), w_q, b_q)
    qf = R.quantize(hs[0].numpy(), s_h[0])                                  # the float stem, quantised
    diff = np.abs(q0.astype(np.int32) - qf.astype(np.int32))
    n_sat, n_out = sum(int((np.abs(o.astype(np.int32)) == 127).sum()) for o in outs), sum(o.size for o in outs)
    d = (y - g["y"]).abs()
    print(f"g22 int8: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}, largest stem |acc| {int(np.abs(acc).max())}, "
          f"stem codes off by one {float(np.mean(diff == 1)):.4f} (max {int(diff.max())}), outputs at +-127 {n_sat / n_out:.2e}")
    assert int(np.abs(acc).max()) < 2 ** 24                                # int -> float is exact at this size
    assert int(diff.max()) <= 1
    assert float(d.max()) <= 1.25 * G22_MAX
    assert float(d.mean()) <= 1.25 * G22_MEAN


# ------------------------------------------------------------------------------------------------------- refusals
def test_calibrate_and_int8_resnet_refuse_other_models():
    from fdet_amd import FdetError
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.models.Resnet import Resnet
    from fdet_amd.quantize import Int8PoolResnet, Int8Resnet, QuantParams, calibrate, quantize_model
    qp = QuantParams([1.0] * 3, [1.0] * 2)
    with pytest.raises(TypeError, match="Resnet only"):
        Int8Resnet(PoolResnet(64, (3, 480, 480), 10, num_of_residual_blocks=2), qp)
    with pytest.raises(TypeError, match="Resnet only"):
        Int8Resnet(torch.nn.Conv2d(3, 3, 1), qp)
    with pytest.raises(TypeError, match="Resnet and PoolResnet only"):
        calibrate(torch.nn.Conv2d(3, 3, 1), [])
    with pytest.raises(TypeError, match="PoolResnet only"):
        calibrate(torch.nn.Linear(2, 2), [])
    with pytest.raises(TypeError, match="PoolResnet only"):
        Int8PoolResnet(Resnet(64, (3, 64, 64), 4, num_of_residual_blocks=2), qp)
    m = Resnet(64, (3, 64, 64), 8, num_of_residual_blocks=2)
    with pytest.raises(ValueError, match="residual blocks"):
        Int8Resnet(m, QuantParams([1.0] * 4, [1.0] * 3))
    with pytest.raises(FdetError, match="GPU only"):
        Int8Resnet(m, qp)                                                  # a CPU model: no CPU fallback
    with pytest.raises(ValueError, match="no image"):
        calibrate(m, [])                                                   # a Resnet is accepted; nothing was seen
    assert callable(getattr(m, "quantize")) and quantize_model is not None


# ------------------------------------------------------------------------------------------------------- C-ABI, host side
def test_stem3_size_helper_and_argument_rejection_need_no_gpu():
    from fdet_amd import _native
    L = _native.lib()
    ok = L.fdet_stem3_fwd_q8_ok
    assert [ok(1, 3, f, 480, 480) for f in (64, 128, 192, 256, 320, 48, 32, 0)] == [1, 1, 1, 1, 0, 0, 0, 0]
    assert ok(1, 3, 64, 2, 2) == 1 and ok(1, 3, 64, 4096, 4096) == 1 and ok(1, 3, 64, 4098, 64) == 0
    assert ok(1, 3, 64, 481, 480) == 0 and ok(1, 3, 64, 480, 6 + 1) == 0 and ok(1, 3, 64, 0, 4) == 0
    assert ok(1, 1, 64, 480, 480) == 0 and ok(1, 4, 64, 480, 480) == 0 and ok(0, 3, 64, 480, 480) == 0
    assert ok(256, 3, 64, 480, 480) == 1 and ok(1024, 3, 64, 480, 480) == 0              # 2^31 bytes of output and more
    buf = ctypes.create_string_buffer(96)                                  # a host address: only ever compared with NULL
    p16 = (ctypes.addressof(buf) + 15) & ~15
    call = L.fdet_stem3_fwd_q8_u8
    assert call(None, None, None, None, None, 1, 3, 64, 4, 4, None) == -1 and b"stem3_fwd_q8" in L.fdet_last_error()
    for hole in range(5):
        args = [p16] * 5
        args[hole] = None
        assert call(*args, 1, 3, 64, 4, 4, None) == -1 and b"null" in L.fdet_last_error()
    assert call(p16, p16, p16, p16, p16, 1, 3, 64, 5, 4, None) == -1 and b"even" in L.fdet_last_error()       # odd H
    assert call(p16, p16, p16, p16, p16, 1, 3, 48, 4, 4, None) == -1 and b"unsupported" in L.fdet_last_error()  # F = 48
    assert call(p16, p16, p16, p16, p16, 1, 4, 64, 4, 4, None) == -1
    assert call(p16, p16, p16, p16, p16, 0, 3, 64, 4, 4, None) == -1
    assert call(p16, p16, p16, p16, p16 + 4, 1, 3, 64, 4, 4, None) == -1 and b"aligned" in L.fdet_last_error()  # q
    assert call(p16, p16 + 8, p16, p16, p16, 1, 3, 64, 4, 4, None) == -1 and b"aligned" in L.fdet_last_error()  # w_q


def test_stem3_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from fdet_amd import FdetError
    from fdet_amd import hotpath as hp
    with pytest.raises(ValueError):
        hp.stem3_fwd_q8_u8(torch.zeros(1, 3, 4, 4), torch.zeros(2048, dtype=torch.int8), torch.zeros(64, dtype=torch.int32),
                           torch.zeros(64), None)                           # float frames
    with pytest.raises(ValueError):
        hp.stem3_fwd_q8_u8(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(27 * 64, dtype=torch.int8),
                           torch.zeros(64, dtype=torch.int32), torch.zeros(64), None)     # unpacked weights
    assert hp.stem3_fwd_q8_ok(2, 3, 64, 480, 480) and not hp.stem3_fwd_q8_ok(2, 3, 64, 480, 483)
    with pytest.raises(FdetError):                                          # CPU tensors never reach the library
        hp.stem3_fwd_q8_u8(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(2048, dtype=torch.int8),
                           torch.zeros(64, dtype=torch.int32), torch.zeros(64), hp.Q8Tensor(1, 64, 2, 2, "cpu"))
