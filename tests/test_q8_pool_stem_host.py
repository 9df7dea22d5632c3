"""CPU checks of Int8PoolResnet's integer stem: the numpy restatement (tests/q8_pool_stem_cpu_ref.py) against literal loops,
the shift identity the kernel relies on, the packed weight layout, the accuracy of the int8 network with the integer stem in
front on the trained medium archive (g16), and the host side of the new C-ABI entry, wrappers and script flag."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_pool_stem_cpu_ref as RP  # noqa: E402

F32 = np.float32


# ------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("shape", [(1, 64, 6, 6), (1, 64, 14, 22)], ids=["6x6", "14x22"])
def test_stem_restatement_equals_the_literal_loops(shape):
    x, w, b, mul = RP.make_case(shape)
    w, b, mul = w[:8], b[:8], mul[:8]                                      # 8 output channels keep the loops within seconds
    got = RP.stem10_q(x, w, b, mul)
    assert got.dtype == np.int8 and got.shape == (1, 8) + RP.out_hw(*shape[2:])
    assert np.array_equal(got, RP.stem10_loops(x, w, b, mul))
    assert got.min() >= -127


@pytest.mark.parametrize("shape", RP.SHAPES, ids=["x".join(map(str, s)) for s in RP.SHAPES])
def test_shift_identity_of_the_signed_staging(shape):
    """sum x * w with zero padding == sum (x - 128) * w over all 300 taps with -128 outside + 128 * sum(w), in integers."""
    x, w, b, _ = RP.make_case(shape)
    acc = RP.stem10_acc(x, w, b)
    assert acc.shape == (shape[0], shape[1]) + RP.out_hw(*shape[2:])
    assert np.array_equal(RP.stem10_shifted_acc(x, w, b), acc)


def test_packed_weights_are_a_zero_padded_permutation():
    from fdet_amd import hotpath as hp
    w = RP.make_case((1, 128, 6, 6))[1]
    pk = RP.pack_stem10_weights(w)
    assert pk.shape == (128, 32, 16) and not pk[:, 30:].any() and not pk[:, :, 10:].any()
    assert np.array_equal(pk[:, :30, :10].reshape(128, 3, 10, 10), w)       # the real weights, each once, in (ci, ky, kx) order
    assert np.array_equal(hp.q8_pack_stem10_weights(torch.from_numpy(w)).numpy(), pk.reshape(-1))
    with pytest.raises(ValueError):
        hp.q8_pack_stem10_weights(torch.zeros(48, 3, 10, 10, dtype=torch.int8))
    with pytest.raises(ValueError):
        hp.q8_pack_stem10_weights(torch.zeros(64, 3, 3, 3, dtype=torch.int8))
    with pytest.raises(ValueError):
        hp.q8_pack_stem10_weights(torch.zeros(64, 3, 10, 10))


# ------------------------------------------------------------------------------------------------------- accuracy on g16
# The bounds are those of tests/test_q8_host.py::test_int8_trunk_on_the_trained_medium_archive (float stem -> int8 trunk): what
# that test measures, times 1.25.
G16_MAX, G16_MEAN = 0.059795, 0.002679


def _float_intermediates(P, x):
    """torch fp32 ops on the CPU: block inputs h_0..h_nb (h_0 is the stem output) and first-conv outputs a_k."""
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
    return hs, as_


def test_integer_stem_in_front_of_the_int8_trunk_on_the_trained_medium_archive(golden):
    """g16 weights, the three g6 frames, abs-max calibration on those frames (the float stem's output gives s_h[0]); integer
    stem -> restatement trunk -> float head against the reference y stored in g16.  Measured: max |dy| 0.036357, mean |dy|
    0.002638 (bounds: the float-stem test's 0.059795 and 0.002679, times 1.25); 8.6 % of the stem's codes differ from the
    quantised float stem's, none by more than one; largest |acc| 627,687; the cells above 0.7 are the reference's four."""
    from fdet_amd import quantize as Q
    g = golden("g16_trained_medium")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    images = golden("g6_trained_small")["images"]
    with torch.no_grad():
        hs, as_ = _float_intermediates(P, images.float() / 255.0)
    obs = Q.ActivationObserver(10, "absmax")
    obs.observe(hs, as_)
    qp = obs.params()
    Pn = {k: v.numpy() for k, v in P.items()}
    q0, outs, y = RP.model_q(images.numpy(), Pn, qp.s_h, qp.s_a, S=10)
    assert tuple(q0.shape) == (3, 64, 60, 60) and [o.shape[2] for o in outs] == [30, 15] + [15] * 8
    w_q, b_q, mul = Q.prepare_conv(Pn["conv1.weight"], Pn["conv1.bias"], Q.STEM_IN_SCALE, qp.s_h[0])
    for a, b in zip((w_q, b_q, mul), R.prepare_conv(Pn["conv1.weight"], Pn["conv1.bias"], RP.S_IN, qp.s_h[0])):
        assert a.dtype == b.dtype and np.array_equal(a, b)                  # the package prepares what the restatement does
    acc = RP.stem10_acc(images.numpy(), w_q, b_q)
    worst = int((255 * np.abs(w_q.astype(np.int64)).reshape(64, -1).sum(axis=1) + np.abs(b_q.astype(np.int64))).max())
    qf = R.quantize(hs[0].numpy(), qp.s_h[0])                               # the float stem, quantised
    diff = np.abs(q0.astype(np.int32) - qf.astype(np.int32))
    d = (y - g["y"]).abs()
    cells, want = y[:, 0] > 0.7, g["y"][:, 0] > 0.7
    print(f"g16 integer stem: max |dy| {float(d.max()):.6f}, mean |dy| {float(d.mean()):.6f}, cells above 0.7 {int(cells.sum())}, "
          f"stem codes that differ {float(np.mean(diff != 0)):.4f} (max {int(diff.max())}), largest |acc| {int(np.abs(acc).max())}, "
          f"worst case {worst}")
    assert int(np.abs(acc).max()) < 2 ** 24 and worst < 2 ** 24             # int -> float is exact at this size
    assert int(diff.max()) <= 1
    assert float(d.max()) <= 1.25 * G16_MAX
    assert float(d.mean()) <= 1.25 * G16_MEAN
    assert torch.equal(cells, want) and int(cells.sum()) >= 2


# ------------------------------------------------------------------------------------------------------- refusals
def test_stem_keyword_is_checked():
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.models.Resnet import Resnet
    from fdet_amd.quantize import Int8PoolResnet, QuantParams, quantize_model
    qp = QuantParams([1.0] * 3, [1.0] * 2)
    model = PoolResnet(64, (3, 480, 480), 10, num_of_residual_blocks=2)
    with pytest.raises(ValueError, match="stem must be one of"):
        Int8PoolResnet(model, qp, stem="bogus")
    with pytest.raises(ValueError, match="stem must be one of"):
        quantize_model(model, [], stem="bogus")
    with pytest.raises(ValueError, match="stem must be one of"):
        model.quantize([], stem="bogus")
    with pytest.raises(ValueError, match="integer stem only"):
        quantize_model(Resnet(64, (3, 64, 64), 8, num_of_residual_blocks=2), [], stem="integer")
    from fdet_amd import FdetError
    for stem in Int8PoolResnet.STEMS:
        with pytest.raises(FdetError, match="GPU only"):
            Int8PoolResnet(model, qp, stem=stem)                            # a CPU model: no CPU fallback, either stem


def test_scripts_check_the_int8_stem_option(capsys):
    from fdet_amd import detect_images as D
    from fdet_amd import run_validation_epoch as V
    io = ["--images", "in", "--out", "out.txt"]
    for mod, argv, msg in ((D, io + ["--int8-stem", "integer"], "--int8-stem needs --int8"),
                           (V, ["--int8-stem", "integer"], "--int8-stem needs --int8"),
                           (V, ["--int8-stem", "float"], "--int8-stem needs --int8"),
                           (D, io + ["--int8", "--int8-stem", "bogus"], "invalid choice"),
                           (D, io + ["--int8", "--int8-stem", "integer", "--model", "resnet"], "poolresnet only")):
        with pytest.raises(SystemExit):
            mod.main(argv)
        assert msg in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------- C-ABI, host side
def test_stem10_size_helper_and_argument_rejection_need_no_gpu():
    from fdet_amd import _native
    L = _native.lib()
    ok = L.fdet_stem10_fwd_q8_ok
    assert [ok(1, 3, f, 480, 480) for f in (64, 128, 192, 256, 320, 96, 48, 0)] == [1, 1, 1, 1, 0, 0, 0, 0]
    assert ok(1, 3, 64, 6, 6) == 1 and ok(1, 3, 64, 4096, 4096) == 1 and ok(1, 3, 64, 17, 45) == 1 and ok(1, 3, 64, 481, 483) == 1
    assert ok(1, 3, 64, 5, 480) == 0 and ok(1, 3, 64, 480, 5) == 0 and ok(1, 3, 64, 480, 4097) == 0 and ok(1, 3, 64, 4097, 480) == 0
    assert ok(1, 1, 64, 480, 480) == 0 and ok(1, 4, 64, 480, 480) == 0 and ok(0, 3, 64, 480, 480) == 0
    # 62 x 62 x 64 bytes per image: 8729 images stay under 2^31 bytes of output, 8730 do not
    assert ok(8729, 3, 64, 480, 480) == 1 and ok(8730, 3, 64, 480, 480) == 0
    buf = ctypes.create_string_buffer(96)                                  # a host address: only ever compared with NULL
    p16 = (ctypes.addressof(buf) + 15) & ~15
    call = L.fdet_stem10_fwd_q8_u8
    assert call(None, None, None, None, None, 1, 3, 64, 6, 6, None) == -1 and b"stem10_fwd_q8" in L.fdet_last_error()
    for hole in range(5):
        args = [p16] * 5
        args[hole] = None
        assert call(*args, 1, 3, 64, 6, 6, None) == -1 and b"null" in L.fdet_last_error()
    assert call(p16, p16, p16, p16, p16, 1, 3, 64, 5, 6, None) == -1 and b"unsupported" in L.fdet_last_error()   # H = 5
    assert call(p16, p16, p16, p16, p16, 1, 3, 96, 6, 6, None) == -1 and b"unsupported" in L.fdet_last_error()   # F = 96
    assert call(p16, p16, p16, p16, p16, 1, 1, 64, 6, 6, None) == -1
    assert call(p16, p16, p16, p16, p16, 1, 3, 64, 6, 4097, None) == -1
    assert call(p16, p16, p16, p16, p16, 8730, 3, 64, 480, 480, None) == -1
    assert call(p16, p16, p16, p16, p16 + 4, 1, 3, 64, 6, 6, None) == -1 and b"aligned" in L.fdet_last_error()   # q
    assert call(p16, p16 + 8, p16, p16, p16, 1, 3, 64, 6, 6, None) == -1 and b"aligned" in L.fdet_last_error()   # w_q


def test_stem10_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from fdet_amd import FdetError
    from fdet_amd import hotpath as hp
    wpk, bias, mul = torch.zeros(512 * 64, dtype=torch.int8), torch.zeros(64, dtype=torch.int32), torch.zeros(64)
    with pytest.raises(ValueError):
        hp.stem10_fwd_q8_u8(torch.zeros(1, 3, 6, 6), wpk, bias, mul, None)   # float frames
    with pytest.raises(ValueError):
        hp.stem10_fwd_q8_u8(torch.zeros(1, 3, 6, 6, dtype=torch.uint8), torch.zeros(300 * 64, dtype=torch.int8), bias, mul, None)
    with pytest.raises(ValueError):
        hp.stem10_fwd_q8_u8(torch.zeros(1, 3, 5, 6, dtype=torch.uint8), wpk, bias, mul, None)                 # H = 5
    with pytest.raises(ValueError):                                         # an output of the wrong shape
        hp.stem10_fwd_q8_u8(torch.zeros(1, 3, 14, 14, dtype=torch.uint8), wpk, bias, mul, hp.Q8Tensor(1, 64, 1, 1, "cpu"))
    assert hp.stem10_fwd_q8_ok(2, 3, 64, 480, 483) and not hp.stem10_fwd_q8_ok(2, 3, 64, 480, 4097)
    with pytest.raises(FdetError):                                          # CPU tensors never reach the library
        hp.stem10_fwd_q8_u8(torch.zeros(1, 3, 6, 6, dtype=torch.uint8), wpk, bias, mul, hp.Q8Tensor(1, 64, 1, 1, "cpu"))
