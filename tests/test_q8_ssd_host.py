"""Host checks of the int8 SSD (no GPU): the numpy restatement tests/q8_ssd_cpu_ref.py against literal loops, the
weight packing, SSDQuantParams, the host-side argument checks of every fdet_q8x entry, the refusals of Int8SSD and
calibrate_ssd, and the quantisation error of the restatement on the seeded model (the bound of tests/test_gpu_q8_ssd.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cpu_ref as R  # noqa: E402
import q8_resnet_cpu_ref as RR  # noqa: E402
import q8_ssd_cpu_ref as SC  # noqa: E402

F32 = np.float32


def _case(seed, N, ci, co, H, W, skip):
    rng = np.random.default_rng(seed)
    x = rng.integers(-127, 128, (N, ci, H, W)).astype(np.int8)
    w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, co).astype(np.int32)
    mul = np.exp2(rng.uniform(-12.0, -8.0, co) - 0.5 * np.log2(ci / 64.0)).astype(F32)
    sk = rng.integers(-127, 128, (N, co, H, W)).astype(np.int8) if skip else None
    return x, w, b, mul, sk, (F32(0.75) if skip else None)


# ------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("ci,co,H,W,skip,pool", [(16, 32, 3, 5, False, False), (32, 16, 2, 3, True, False), (16, 16, 5, 3, True, True),
                                                 (48, 32, 3, 3, False, True), (16, 32, 1, 1, True, False)])
def test_conv_restatement_equals_literal_loops(ci, co, H, W, skip, pool):
    x, w, b, mul, sk, sm = _case(ci + co + H, 1, ci, co, H, W, skip)
    want = SC.conv3x3_loops(x, w, b, mul, sk, sm, pool)
    got = SC.conv3x3(x, w, b, mul, sk, sm, pool)
    assert got.shape == (1, co, H // 2, W // 2) if pool else got.shape == (1, co, H, W)
    assert np.array_equal(got, want)
    # the other matmul restatement of the accumulator (q8_cpu_ref.conv_acc) agrees for Cin != Cout
    assert np.array_equal(R.conv_acc(x, w, b), RR.conv_acc(x, w, b))


def test_floor_pool_drops_the_odd_last_row_and_column():
    q = np.arange(2 * 5 * 7, dtype=np.int8).reshape(1, 2, 5, 7)
    p = SC.maxpool2_floor(q)
    assert p.shape == (1, 2, 2, 3)
    assert p[0, 0, 1, 2] == max(q[0, 0, 2, 4], q[0, 0, 2, 5], q[0, 0, 3, 4], q[0, 0, 3, 5])
    big = np.full((1, 1, 15, 15), -5, np.int8)
    big[0, 0, 14, :] = 100
    big[0, 0, :, 14] = 100
    assert SC.maxpool2_floor(big).shape == (1, 1, 7, 7) and (SC.maxpool2_floor(big) == -5).all()
    even = np.random.default_rng(1).integers(-127, 128, (2, 3, 6, 4)).astype(np.int8)
    assert np.array_equal(SC.maxpool2_floor(even), R.maxpool2(even))


def test_pointwise_head_and_stem_restatements_equal_literal_loops():
    rng = np.random.default_rng(5)
    x = rng.integers(-127, 128, (2, 16, 2, 3)).astype(np.int8)
    w = rng.integers(-127, 128, (32, 16, 1, 1)).astype(np.int8)
    b = rng.integers(-4000, 4001, 32).astype(np.int32)
    mul = np.exp2(rng.uniform(-10.0, -7.0, 32)).astype(F32)
    assert np.array_equal(SC.pointwise(x, w, b, mul), SC.pointwise_loops(x, w, b, mul))
    hw = rng.integers(-127, 128, (5, 16)).astype(np.int8)
    hb = rng.integers(-4000, 4001, 5).astype(np.int32)
    m = np.exp2(rng.uniform(-14.0, -10.0, 5)).astype(F32)
    z = SC.head(x, hw, hb, m)
    assert z.dtype == F32 and np.array_equal(z, SC.head_loops(x, hw, hb, m))
    f = rng.integers(0, 256, (1, 3, 4, 6)).astype(np.uint8)
    sw = rng.integers(-127, 128, (16, 3, 3, 3)).astype(np.int8)
    sb = rng.integers(-40000, 40001, 16).astype(np.int32)
    smul = np.exp2(rng.uniform(-11.5, -8.5, 16)).astype(F32)
    assert np.array_equal(RR.stem3_q(f, sw, sb, smul), RR.stem3_loops(f, sw, sb, smul))


def test_prepare_head_follows_the_contract():
    rng = np.random.default_rng(6)
    w = rng.normal(0, 0.1, (5, 32)).astype(F32)
    w[3] = 0
    b = rng.normal(0, 0.1, 5).astype(F32)
    s_in = F32(0.0123)
    w_q, b_q, m = SC.prepare_head(w, b, s_in)
    s_w = np.abs(w).max(axis=1) / F32(127.0)
    s_w[3] = 1.0
    assert w_q.dtype == np.int8 and (w_q[3] == 0).all() and np.abs(w_q[:3]).max() == 127
    assert np.array_equal(m, s_w.astype(F32) * s_in)
    assert np.array_equal(b_q, np.rint(b.astype(np.float64) / (s_w.astype(np.float64) * np.float64(s_in))).astype(np.int32))
    import fdet_amd  # noqa: F401
    from fdet_amd.quantize import prepare_head
    for a, c in zip(prepare_head(w, b, s_in), (w_q, b_q, m)):
        assert a.dtype == c.dtype and np.array_equal(a, c)


# ------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("co,ci,side", [(32, 16, 3), (32, 32, 3), (64, 32, 3), (16, 48, 3), (128, 64, 3), (32, 16, 1), (128, 64, 1),
                                        (256, 128, 1)])
def test_weight_packing_is_the_stated_permutation(co, ci, side):
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    w = np.random.default_rng(co + ci).integers(-127, 128, (co, ci, side, side)).astype(np.int8)
    w[w == 0] = 1                                           # (every real byte non-zero: a pad byte cannot hide)
    got = hp.q8x_pack_weights(torch.from_numpy(w)).numpy()
    K = ci * side * side
    assert got.size == (K + 63) // 64 * 64 * co
    assert np.array_equal(got.reshape(-1, co, 64), SC.pack_weights(w))
    back, pad = SC.unpack_weights(got, co, ci, side * side)
    assert np.array_equal(back, w) and not pad.any() and pad.size == ((K + 63) // 64 * 64 - K) * co
    if ci % 64 == 0 and side == 3 and co == ci:             # the order of fdet_q8_conv3x3 where both exist
        assert np.array_equal(got, hp.q8_pack_weights(torch.from_numpy(w)).numpy())
    if ci % 64 == 0 and side == 3:
        assert np.array_equal(got.reshape(9, ci // 64, co, 64), R.pack_weights(w))


def test_pack_weights_refuses_other_shapes():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    for shape, dt in (((32, 16, 2, 2), torch.int8), ((32, 24, 3, 3), torch.int8), ((24, 16, 3, 3), torch.int8), ((32, 16, 3, 3), torch.int32)):
        with pytest.raises(ValueError):
            hp.q8x_pack_weights(torch.zeros(shape, dtype=dt))
    with pytest.raises(ValueError):
        hp.q8x_pack_stem_weights(torch.zeros(24, 3, 3, 3, dtype=torch.int8))
    p = hp.q8x_pack_stem_weights(torch.ones(16, 3, 3, 3, dtype=torch.int8)).reshape(16, 32)
    assert bool((p[:, :27] == 1).all()) and not bool(p[:, 27:].any())


# ------------------------------------------------------------------------------------------------------- scales
def _qp(**kw):
    import fdet_amd  # noqa: F401
    from fdet_amd.quantize import SSDQuantParams
    a = dict(s_h=np.linspace(0.01, 0.02, 14), s_a=np.linspace(0.02, 0.03, 13), s_k=np.linspace(0.03, 0.04, 4))
    a.update(kw)
    return SSDQuantParams(**a)


def test_ssd_quant_params_validate_and_round_trip(tmp_path):
    from fdet_amd.quantize import QuantParams, SSDQuantParams
    q = _qp(method="percentile", percentile=99.9, images_seen=7)
    assert q.num_blocks == 13 and q.s_h.dtype == F32 and q.s_k.size == 4 and "SSDQuantParams" in repr(q)
    path = str(tmp_path / "ssd_q.npz")
    q.save(path)
    assert SSDQuantParams.load(path) == q
    with np.load(path) as z:
        assert str(z["kind"]) == "ssd" and int(z["version"]) == 1
    assert _qp() != q and _qp() == _qp()
    for bad in (dict(s_h=np.ones(13)), dict(s_a=np.ones(12)), dict(s_k=np.ones(14)), dict(s_k=[0.1, 0.0, 0.1, 0.1]),
                dict(s_a=[-1.0] * 13), dict(s_h=[float("nan")] * 14), dict(s_k=[float("inf")] * 4), dict(method="guess")):
        with pytest.raises(ValueError):
            _qp(**bad)
    # the two kinds of file do not read each other; another version is refused
    old = str(tmp_path / "old.npz")
    QuantParams(np.ones(3), np.ones(2)).save(old)
    with pytest.raises(ValueError):
        SSDQuantParams.load(old)
    with pytest.raises(KeyError):
        QuantParams.load(path)                              # (no s_h / s_a layout of a trunk: QuantParams needs its own file)
    with np.load(path) as z:
        d = {k: z[k] for k in z.files}
    d["version"] = np.array(2, dtype=np.int64)
    np.savez(str(tmp_path / "v2.npz"), **d)
    with pytest.raises(ValueError):
        SSDQuantParams.load(str(tmp_path / "v2.npz"))


# ------------------------------------------------------------------------------------------------------- C entries
def test_ok_helpers_and_old_helpers_keep_their_answers():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    L = _native.lib()
    for C in (16, 32, 48, 64, 128, 256):
        assert L.fdet_q8x_supported(C, 1, 1) == 1 and L.fdet_q8x_supported(C, 4096, 4096) == 1
    for C, H, W in ((0, 4, 4), (8, 4, 4), (24, 4, 4), (272, 4, 4), (16, 0, 4), (16, 4, 4097)):
        assert L.fdet_q8x_supported(C, H, W) == 0
    assert L.fdet_q8x_act_bytes(3, 16, 240, 240) == 3 * 242 * 242 * 16
    assert L.fdet_q8x_act_bytes(1, 32, 60, 60) == 62 * 62 * 32
    assert L.fdet_q8x_act_bytes(0, 16, 4, 4) == 0 and L.fdet_q8x_act_bytes(1, 20, 4, 4) == 0
    assert L.fdet_q8x_act_bytes(2048, 256, 62, 62) == 0                     # 2^31 bytes: no layout
    assert L.fdet_q8x_act_bytes(2047, 256, 62, 62) == 2047 * 64 * 64 * 256
    # what the existing entries refuse stays refused
    assert L.fdet_q8_supported(32, 60, 60) == 0 and L.fdet_q8_act_bytes(1, 32, 60, 60) == 0
    assert L.fdet_stem3_fwd_q8_ok(1, 3, 16, 480, 480) == 0 and L.fdet_stem3_fwd_q8_ok(1, 3, 32, 480, 480) == 0
    assert L.fdet_q8x_conv3x3_ok(1, 16, 32, 240, 240, 1) == 1 and L.fdet_q8x_conv3x3_ok(1, 256, 256, 15, 15, 1) == 1
    assert L.fdet_q8x_conv3x3_ok(1, 16, 32, 1, 1, 0) == 1
    for a in ((1, 16, 32, 1, 4, 1), (1, 16, 32, 4, 1, 1), (1, 16, 40, 4, 4, 0), (1, 8, 32, 4, 4, 0), (0, 16, 32, 4, 4, 0),
              (1, 16, 32, 4, 4, 2), (1, 16, 512, 4, 4, 0)):
        assert L.fdet_q8x_conv3x3_ok(*a) == 0, a
    assert L.fdet_q8x_pointwise_ok(2, 16, 32, 240, 240) == 1 and L.fdet_q8x_pointwise_ok(2, 16, 36, 240, 240) == 0
    assert L.fdet_q8x_head_ok(4, 128, 60, 60) == 1 and L.fdet_q8x_head_ok(4, 100, 60, 60) == 0 and L.fdet_q8x_head_ok(0, 128, 60, 60) == 0
    assert L.fdet_stem3_fwd_q8x_ok(1, 3, 16, 480, 480) == 1 and L.fdet_stem3_fwd_q8x_ok(1, 3, 64, 480, 480) == 1
    for a in ((1, 1, 16, 480, 480), (1, 3, 8, 480, 480), (1, 3, 16, 481, 480), (1, 3, 16, 480, 0), (0, 3, 16, 480, 480),
              (1, 3, 272, 480, 480), (1 << 20, 3, 256, 480, 480)):
        assert L.fdet_stem3_fwd_q8x_ok(*a) == 0, a


def test_entries_reject_bad_arguments_on_the_host():
    """Nothing is launched: every call below fails a host check (addresses are made up and never read)."""
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    L = _native.lib()
    A, B, C, D, E, Y = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000

    def fails(rc, word):
        assert rc == -1
        assert word in L.fdet_last_error(), L.fdet_last_error()
    fails(L.fdet_q8x_conv3x3(None, B, C, D, None, 0.0, Y, 1, 16, 32, 4, 4, 0, 0.2, None), b"null")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, None, 0.0, None, 1, 16, 32, 4, 4, 0, 0.2, None), b"null")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, None, 0.0, Y, 1, 16, 24, 4, 4, 0, 0.2, None), b"unsupported shape")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, None, 0.0, Y, 1, 16, 32, 4, 4, 3, 0.2, None), b"pool")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, None, 0.0, Y, 1, 16, 32, 1, 4, 1, 0.2, None), b"unsupported shape")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, None, 0.0, Y, 4096, 256, 256, 60, 60, 0, 0.2, None), b"unsupported shape")
    fails(L.fdet_q8x_conv3x3(A + 4, B, C, D, None, 0.0, Y, 1, 16, 32, 4, 4, 0, 0.2, None), b"aligned")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, E + 8, 0.5, Y, 1, 16, 32, 4, 4, 0, 0.2, None), b"aligned")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, None, 0.0, A, 1, 16, 32, 4, 4, 0, 0.2, None), b"alias")
    fails(L.fdet_q8x_conv3x3(A, B, C, D, Y, 0.5, Y, 1, 16, 32, 4, 4, 0, 0.2, None), b"alias")
    fails(L.fdet_q8x_pointwise(A, None, C, D, Y, 1, 16, 32, 4, 4, None), b"null")
    fails(L.fdet_q8x_pointwise(A, B, C, D, Y, 1, 16, 32, 0, 4, None), b"unsupported shape")
    fails(L.fdet_q8x_pointwise(A, B, C, D, Y, 1, 20, 32, 4, 4, None), b"unsupported shape")
    fails(L.fdet_q8x_pointwise(A, B, C + 2, D, Y, 1, 16, 32, 4, 4, None), b"aligned")
    fails(L.fdet_q8x_pointwise(A, B, C, D, A, 1, 16, 32, 4, 4, None), b"alias")
    fails(L.fdet_q8x_head_f32(A, B, C, None, Y, 1, 16, 4, 4, None), b"null")
    fails(L.fdet_q8x_head_f32(A, B, C, D, Y, 1, 300, 4, 4, None), b"unsupported shape")
    fails(L.fdet_q8x_head_f32(A, B, C, D, Y + 4, 1, 16, 4, 4, None), b"aligned")
    fails(L.fdet_stem3_fwd_q8x_u8(None, B, C, D, Y, 1, 3, 16, 4, 4, None), b"null")
    fails(L.fdet_stem3_fwd_q8x_u8(A, B, C, D, Y, 1, 3, 16, 5, 4, None), b"unsupported shape")
    fails(L.fdet_stem3_fwd_q8x_u8(A, B, C, D, Y, 1, 3, 24, 4, 4, None), b"unsupported shape")
    fails(L.fdet_stem3_fwd_q8x_u8(A, B, C, D, Y, 1, 4, 16, 4, 4, None), b"unsupported shape")
    fails(L.fdet_stem3_fwd_q8x_u8(A, B + 1, C, D, Y, 1, 3, 16, 4, 4, None), b"aligned")
    fails(L.fdet_stem3_fwd_q8x_u8(A, B, C, D, Y + 8, 1, 3, 64, 4, 4, None), b"aligned")


# ------------------------------------------------------------------------------------------------------- refusals
def test_int8_ssd_and_calibrate_ssd_refuse_what_they_do_not_cover():
    import fdet_amd  # noqa: F401
    from fdet_amd import FdetError
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.models.SSD import SSD
    from fdet_amd.quantize import Int8SSD, QuantParams, calibrate, calibrate_ssd
    qp = _qp()
    other = PoolResnet(64, (3, 480, 480), 15)
    with pytest.raises(TypeError, match="SSD only"):
        Int8SSD(other, qp)
    with pytest.raises(TypeError, match="SSD only"):
        calibrate_ssd(other, [])
    ssd = SSD(16, (3, 480, 480))
    assert hasattr(ssd, "quantize")
    with pytest.raises(TypeError, match="SSDQuantParams"):
        Int8SSD(ssd, QuantParams(np.ones(14), np.ones(13)))
    with pytest.raises(ValueError, match="13 blocks"):
        Int8SSD(ssd, _qp(s_k=np.ones(3)))
    with pytest.raises(FdetError, match="GPU only"):
        Int8SSD(ssd, qp)                                    # a CPU model
    with pytest.raises(ValueError, match="256 channels"):
        Int8SSD(SSD(32, (3, 480, 480)), qp)
    with pytest.raises(ValueError, match="256 channels"):
        SSD(32, (3, 480, 480)).quantize([])
    ssd.engine.set_precision("bf16")
    with pytest.raises(FdetError, match="precision16"):
        calibrate_ssd(ssd, [torch.zeros(1, 3, 480, 480, dtype=torch.uint8)])
    ssd.engine.set_precision("bf16x3")
    # `calibrate` and the text of its refusal are what they were
    with pytest.raises(TypeError, match="Resnet and PoolResnet only"):
        calibrate(ssd, [])


# ------------------------------------------------------------------------------------------------------- quantisation error
# measured with this file (seeded SSD(16), abs-max calibration on its two frames, frame 0): see the test's docstring
SSD_DZ_MAX, SSD_DZ_MEAN, SSD_DS_MAX, SSD_DS_MEAN = 0.009743, 0.001645, 0.002353, 0.000419


def test_restatement_quantisation_error_of_the_seeded_model():
    """The whole SSD(16) restated on the CPU for frame 0 of the seeded pair against torch fp32: max / mean |dz| over the
    (1,4774,5) rows before sigmoid and priors, and max / mean |dscore|.  The constants above are what this test prints; it
    and tests/test_gpu_q8_ssd.py assert 1.25 x them."""
    model, frames = SC.seeded_ssd()
    P = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    hs, as_, ks, zs_f = SC.float_model(P, frames.float() / 255.0)
    s_h, s_a, s_k = SC.absmax_scales(hs), SC.absmax_scales(as_), SC.absmax_scales(ks)
    assert len(s_h) == 14 and len(s_a) == 13 and len(s_k) == 4
    q0, outs, zs = SC.model_q(frames[:1].numpy(), P, s_h, s_a, s_k)
    assert q0.shape == (1, 16, 240, 240) and [o.shape[1:] for o in outs][-4:] == [(128, 60, 60), (256, 30, 30), (256, 15, 15), (256, 7, 7)]
    assert SC.rows(zs).shape == (1, 4774, 5)
    used = [int(np.abs(o.astype(np.int32)).max()) for o in outs]
    assert min(used) >= 64, used                            # every level uses its codes
    e = SC.quant_error(zs, [z[:1].numpy() for z in zs_f])
    zmax = max(float(z.abs().max()) for z in zs_f)
    print(f"seeded SSD(16): max |z| {zmax:.4f}; max |dz| {e[0]:.6f}, mean |dz| {e[1]:.6f}, max |dscore| {e[2]:.6f}, mean |dscore| {e[3]:.6f}")
    assert e[0] <= 1.25 * SSD_DZ_MAX and e[1] <= 1.25 * SSD_DZ_MEAN and e[2] <= 1.25 * SSD_DS_MAX and e[3] <= 1.25 * SSD_DS_MEAN
