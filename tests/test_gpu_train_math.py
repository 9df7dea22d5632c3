"""The kernels that close a training step around the conv stack, held to the references of tests/train_math_cpu_ref.py at
their edges: the dropout generator (byte-equal), the SSD loss with hard-negative mining (mask exact; ties, every kk
path, saturated confidences), the SSD head pack, the residual-block tail (odd maps, NaN, ties, grid-stride), Adam
(grid-stride, tails, non-zero state), the yolo loss and the step metrics.

Value comparisons against float64 use the project's existing bound for the kernel; where it has none (head pack,
per-image metrics) the bound is 4 x the distance of a plain fp32 torch evaluation from the float64 reference on the same
inputs, floor 1e-6 of the tensor's scale (train_math_cpu_ref.rule_tol), computed on the CPU at run time.  Everything
index-like is exact.  tests/test_train_math_host.py proves references and inputs on the CPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_math_cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
I32 = torch.int32


@pytest.fixture(scope="module")
def hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def same_bits(got: torch.Tensor, want) -> bool:
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    got = got.detach().cpu().contiguous()
    return got.shape == want.shape and torch.equal(got.view(I32), want.contiguous().view(I32))


def same_with_nan(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Equal values, NaN in the same places (torch.equal calls NaN unequal to itself)."""
    got = got.detach().cpu()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 3.0), torch.nan_to_num(want, 3.0))


# ------------------------------------------------------------------------------------------
# dropout generator
# ------------------------------------------------------------------------------------------
SEEDS = ((1234, 0), ((1 << 64) - 1, (1 << 64) - 3), (7, 3 << 40))


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_dropout_scales_bytes(hp, n, p):
    for seed, off in SEEDS:
        out = torch.full((n + 64,), 7.0, device="cuda")
        hp.dropout_scales(out[:n], p, seed, off)
        want = R.dropout_scales(n, p, seed, off)
        assert same_bits(out[:n], want), (seed, off)
        assert bool((out[n:] == 7.0).all())                                    # nothing past n
        if p == 0.0:
            assert bool((out[:n] == 1.0).all())


LAYER_CASES = (([16, 64, 5], [0.25, 0.25, 0.5], 7), ([64] * 11, [0.25] * 10 + [0.5], 3), ([8] * 32, [0.25] * 32, 2))


@pytest.mark.parametrize("case", range(len(LAYER_CASES)))
def test_dropout_layers_bytes_layout_and_cross_kernel(hp, case):
    ch, p, n = LAYER_CASES[case]
    seed, base, first = 4242 + case, (1 << 64) - 1000, 5                        # the counter wraps inside the draw
    views = hp.dropout_scales_layers(n, ch, p, seed, base, first, "cuda")
    want = R.dropout_layers(n, ch, p, seed, base, first)
    ls, pre = sum(ch), 0
    assert len(views) == len(ch)
    for k, C in enumerate(ch):
        assert tuple(views[k].shape) == (n, C)
        assert views[k].data_ptr() == views[0].data_ptr() + 4 * n * pre       # layer k at float offset n * pre_k
        assert same_bits(views[k], want[k]), k
        for i in range(n):                                                     # the single kernel at the documented counter
            one = torch.empty(C, device="cuda")
            hp.dropout_scales(one, p[k], seed, base + (first + i) * ls + pre)
            assert same_bits(one, views[k][i].cpu()), (k, i)
        pre += C
    if case == 0:
        assert ls == 85 and n * ls == 595


def test_dropout_layers_split_is_the_whole_batch(hp):
    ch, p = [16, 64, 5], [0.25, 0.25, 0.5]
    whole = hp.dropout_scales_layers(5, ch, p, 99, 12345, 0, "cuda")
    part = hp.dropout_scales_layers(3, ch, p, 99, 12345, 2, "cuda")
    for a, b in zip(whole, part):
        assert same_bits(a[2:5], b.cpu())
    assert any(not same_bits(a[0:3], b.cpu()) for a, b in zip(whole, part))    # and it is not the first three rows


def test_dropout_refusals_and_empty_batch(hp):
    from fdet_amd import _native
    L = _native.lib()
    buf = torch.full((1024,), 7.0, device="cuda")
    st = _native.stream()

    def layers(n, ch, p):
        k = len(ch)
        return L.fdet_dropout_scales_layers(buf.data_ptr(), n, k, (ctypes.c_int * k)(*ch), (ctypes.c_float * k)(*p), 1, 0, 0, st)
    assert layers(1, [8] * 33, [0.25] * 33) == -1 and b"at most 32 layers" in L.fdet_last_error()
    assert layers(1, [8, 8], [0.25, 1.0]) == -1 and b"layer 1" in L.fdet_last_error() and b"p=1.0" in L.fdet_last_error()
    assert layers(1, [8, 0, 8], [0.25] * 3) == -1 and b"layer 1" in L.fdet_last_error() and b"channels=0" in L.fdet_last_error()
    assert L.fdet_dropout_scales(buf.data_ptr(), 4, 1.0, 1, 0, st) == -1 and b"dropout_scales" in L.fdet_last_error()
    assert layers(0, [16, 64, 5], [0.25, 0.25, 0.5]) == 0                      # n = 0: fine, and nothing is written
    assert L.fdet_dropout_scales(buf.data_ptr(), 0, 0.25, 1, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


# ------------------------------------------------------------------------------------------
# SSD loss and hard-negative mining
# ------------------------------------------------------------------------------------------
def _ssd_check(hp, pred, target, ratio):
    ref = R.ssd_loss64(pred, target, ratio)
    loss, grad, mask = hp.ssd_loss_fwd_bwd(pred.cuda(), target.cuda(), ratio, want_grad=True, want_mask=True)
    loss, grad, mask = loss.cpu(), grad.cpu(), mask.cpu()
    assert torch.equal(mask.bool(), ref["mask"])
    print(f"ssd loss {float(loss):.9g} ref {float(ref['loss']):.9g} max|dgrad| {float((grad.double() - ref['grad']).abs().max()):.3g}")
    assert abs(float(loss) - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"]))
    assert torch.allclose(grad.double(), ref["grad"], rtol=1e-5, atol=1e-9)
    assert bool((grad[:, :, 0][~ref["mask"]] == 0).all())                       # unselected: exactly no gradient
    return ref, loss, grad, mask


def test_ssd_mining_ties_at_the_threshold(hp):
    """Confidences on 63 levels: every image's threshold loss is shared by selected and unselected negatives (26..40
    against 27..57, the selected ones from 6..12 different 256-prior sweeps); the lowest indices must be taken."""
    pred, target = R.ssd_tie_case()
    enc = hp.ssd_encode_targets(R.ssd_tie_boxes(), (R.SIZE, R.SIZE)).cpu()
    assert torch.equal(enc, target)
    ref, _, grad, mask = _ssd_check(hp, pred, target, 10)
    assert int(mask[2].sum()) == 0 and not bool(grad[2].any())                   # the image without boxes selects nothing


def test_ssd_loss_parts_on_the_tie_batch(hp):
    pred, target = R.ssd_tie_case()
    pred, target = pred.cuda(), target.cuda()
    loss_ref, grad_ref, _ = hp.ssd_loss_fwd_bwd(pred, target, 10, want_grad=True)
    sa, ga = hp.ssd_loss_parts(pred[:2].contiguous(), target[:2].contiguous(), 10)
    sb, gb = hp.ssd_loss_parts(pred[2:].contiguous(), target[2:].contiguous(), 10)
    tot = sa + sb
    la, lb = hp.ssd_loss_finish(tot, ga), hp.ssd_loss_finish(tot, gb)
    assert float(la) == float(lb) and abs(float(la) - float(loss_ref)) <= 1e-6 * abs(float(loss_ref))
    assert torch.allclose(torch.cat([ga, gb]), grad_ref, rtol=1e-6, atol=1e-9)
    assert torch.allclose(torch.cat([ga, gb]).cpu().double(), R.ssd_loss64(pred.cpu(), target.cpu(), 10)["grad"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("P", R.SSD_SMALL_P)
def test_ssd_loss_small_and_ragged_P(hp, P):
    """P below, at and off a multiple of 256; kk < P_neg, kk == P_neg (P % 4 == 0) and kk > P_neg in the three images."""
    pred, target = R.ssd_small_case(P)
    _ssd_check(hp, pred, target, 3)


def test_ssd_loss_ratio_zero(hp):
    pred, target = R.ssd_small_case(300)
    ref, _, grad, mask = _ssd_check(hp, pred, target, 0)
    assert torch.equal(mask.bool(), target[:, :, 0] > 0)                         # the BCE is over positives only


def test_ssd_loss_saturated_confidences(hp):
    """Confidences of exactly 0 and 1 (losses +inf and -0), the clamp's bounds and their neighbours outside: the +inf
    negatives are mined first, the gradient is exactly 0 outside the clamp and finite at its bounds."""
    pred, target = R.ssd_saturated_case()
    ref, loss, grad, mask = _ssd_check(hp, pred, target, 10)
    conf, neg = pred[:, :, 0], target[:, :, 0] == 0
    assert torch.equal(mask[1].bool() & neg[1], neg[1] & (conf[1] == 0))
    sel = mask.bool()
    outside = sel & ((conf < R.LO32) | (conf > R.HI32))
    at = sel & ((conf == R.LO32) | (conf == R.HI32))
    assert int(outside.sum()) >= 10 and bool((grad[:, :, 0][outside] == 0).all())
    assert int(at.sum()) >= 4 and bool(torch.isfinite(grad[:, :, 0][at]).all()) and bool((grad[:, :, 0][at] != 0).all())
    assert math.isfinite(float(loss))


def test_ssd_loss_labels_and_smooth_l1_knees(hp):
    """Labels 0.3 and 0.5 are positive for mining and 0 for the BCE; |d| of exactly 1 and of the float below it."""
    pred, target = R.ssd_label_case()
    _ssd_check(hp, pred, target, 3)


def test_ssd_loss_all_negative_batch(hp):
    """No positive prior in the whole batch.  The reference divides 0 by 0: the loss is NaN; autograd leaves every gradient
    at 0, because nothing was selected and the 1/0 never meets an element.  The kernel used to scale its (all zero)
    gradient by 1/0 and return NaN everywhere, which an optimiser step would have written into every weight; found by
    this test, fixed in k_ssd_loss_total / k_ssd_loss_finish (scale 0 when there is no positive)."""
    pred, target = R.ssd_all_negative_case()
    ref = R.ssd_loss64(pred, target, 10)
    loss, grad, mask = hp.ssd_loss_fwd_bwd(pred.cuda(), target.cuda(), 10, want_grad=True, want_mask=True)
    assert math.isnan(float(loss)) and math.isnan(float(ref["loss"]))
    assert int(mask.sum()) == 0
    assert same_with_nan(grad.double(), ref["grad"])
    sums, g = hp.ssd_loss_parts(pred.cuda(), target.cuda(), 10)
    assert math.isnan(float(hp.ssd_loss_finish(sums, g))) and same_with_nan(g.double(), ref["grad"])


# ------------------------------------------------------------------------------------------
# SSD head pack
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,CP,ps", [(2, 5, 7), (3, 8, 15), (1, 5, 60)])
def test_ssd_head_pack_vs_float64(hp, N, CP, ps):
    """Measured on the MI355X, max abs distance from float64 (fp32 torch on the CPU / the kernel / the bound):
      ps  7: y 5.5e-8 / 1.5e-7 / 2.9e-6;  dz 3.7e-8 / 4.1e-8 / 3.1e-6
      ps 15: y 6.8e-8 / 1.3e-7 / 3.4e-6;  dz 8.7e-8 / 9.5e-8 / 3.8e-6
      ps 60: y 8.3e-8 / 1.2e-7 / 3.9e-6;  dz 1.6e-7 / 1.6e-7 / 3.7e-6
    Every bound is the floor (1e-6 of the tensor's scale, about 3..4); the kernel multiplies by float(1/ps) where the
    reference divides, which costs it one more rounding in y."""
    z, dy = R.head_pack_case(N, CP, ps, 60 + ps)
    start, P = R.SSD_START[ps], R.SSD_P
    y64, dz64 = R.head_pack64(z, ps, start, P, dy)
    y32, dz32 = R.head_pack_eval(z, ps, start, P, dy, torch.float32)
    y = torch.full((N, P, 5), math.nan, device="cuda")
    hp.ssd_head_pack_fwd(z.cuda(), ps, start, y)
    dz = torch.full((N, CP, ps, ps), math.nan, device="cuda")
    hp.ssd_head_pack_bwd(dy.cuda(), y, ps, start, dz)
    y, dz = y.cpu(), dz.cpu()
    assert torch.equal(torch.isnan(y), torch.isnan(y64))                          # rows of the other heads untouched
    tol_y, tol_dz = R.rule_tol(y32, y64), R.rule_tol(dz32, dz64)
    print(f"head pack ps={ps}: y fp32 {R.dist(y32, y64):.3g} kernel {R.dist(y, y64):.3g} bound {tol_y:.3g}; "
          f"dz fp32 {R.dist(dz32, dz64):.3g} kernel {R.dist(dz, dz64):.3g} bound {tol_dz:.3g}")
    assert R.dist(y, y64) <= tol_y
    assert not bool(torch.isnan(dz).any()) and R.dist(dz, dz64) <= tol_dz
    assert not bool(dz[:, 5:].any())                                              # channels 5..CP-1: exact zeros
    assert y[0, start, 0] == 1.0 and y[0, start + 1, 0] == 0.0 and y[0, start + 2, 0] == 0.5
    assert dz[0, 0, 0, 0] == 0.0 and dz[0, 0, 0, 1] == 0.0 and dz[-1, 0, -1, -1] == 0.0 and dz[-1, 0, -1, -2] == 0.0
    assert float(dz[0, 0, 0, 2]) == float(dy[0, start + 2, 0]) * 0.25


def test_ssd_head_pack_grid_stride(hp):
    """292 x 60 x 60 = 1 051 200 cells: more than 4096 blocks of 256, so the kernel's loop runs a second round."""
    N, CP, ps = 292, 5, 60
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(N, CP, ps, ps, generator=gen)
    y = torch.empty(N, ps * ps, 5, device="cuda")
    hp.ssd_head_pack_fwd(z.cuda(), ps, 0, y)
    total = N * ps * ps
    assert total > 4096 * 256
    idx = torch.cat([torch.arange(0, total, 997), torch.arange(total - 512, total)]).unique()
    n, c = idx // (ps * ps), idx % (ps * ps)
    zs = z.reshape(N, CP, ps * ps)[n, :, c]                                       # (K, 5)

    def rows(dtype):
        q, i, j = zs.to(dtype), (c // ps).to(dtype), (c % ps).to(dtype)
        return torch.stack([torch.sigmoid(q[:, 0]), q[:, 1] / ps + i / ps, q[:, 2] / ps + j / ps, q[:, 3], q[:, 4]], -1)
    ref = rows(torch.float64)
    got = y.cpu().reshape(total, 5)[idx]
    assert R.dist(got, ref) <= R.rule_tol(rows(torch.float32), ref)


# ------------------------------------------------------------------------------------------
# residual-block tail
# ------------------------------------------------------------------------------------------
def _tail_run(hp, c, x, scale, pool, slope, dout):
    N, C, H, W = c.shape
    sd = None if scale is None else scale.cuda()
    out = torch.full((N, C, H // pool, W // pool), math.nan, device="cuda")
    hp.block_tail_fwd(c.cuda(), x.cuda(), sd, out, pool)
    if dout is None:
        return out.cpu(), None, None
    dz2 = torch.full((N, C, H, W), math.nan, device="cuda")
    de = torch.full((N, C, H, W), math.nan, device="cuda") if pool == 2 else None
    hp.block_tail_bwd(dout.cuda(), c.cuda(), x.cuda(), sd, dz2, de, pool, slope)
    return out.cpu(), dz2.cpu(), None if de is None else de.cpu()


def _tail_check(hp, c, x, scale, pool, slope, dout):
    """Forward and de bit-equal to fp32 torch on the CPU, dz2 within the project's bound of the float64 reference."""
    out, dz2, de = _tail_run(hp, c, x, scale, pool, slope, dout)
    out32, gz32, gx32 = R.tail_eval(c, x, scale, pool, slope, dout, torch.float32)
    assert same_with_nan(out, out32.detach())
    if dout is not None:
        _, gz64, _ = R.tail64(c, x, scale, pool, slope, dout)
        assert not bool(torch.isnan(dz2).any())
        assert torch.allclose(dz2.double(), gz64, rtol=1e-6, atol=1e-6)
        if pool == 2:
            assert torch.equal(de, gx32)
    return out, dz2, de


@pytest.mark.parametrize("kind", ["drop", "none"])
@pytest.mark.parametrize("shape", [(2, 16, 15, 15), (1, 8, 7, 9), (1, 4, 3, 2), (1, 4, 2, 2)])
def test_block_tail_pool_on_odd_maps(hp, shape, kind):
    """floor(H/2) x floor(W/2) windows; the odd last row / column belongs to none: gradients there are exactly 0 although
    the buffers arrive full of NaN.  With and without a scale; channel (0, 1) is dropped (scale 0)."""
    c, x, scale, gen = R.tail_case(shape, 15, kind)
    N, C, H, W = shape
    c[0, 0, :2, :2], x[0, 0, :2, :2] = 0.0, 1.0                                  # ties in the four corners' windows: first wins
    c[0, 0, :2, 2 * (W // 2) - 2:2 * (W // 2)], x[0, 0, :2, 2 * (W // 2) - 2:2 * (W // 2)] = 0.0, 1.0
    c[0, 0, 2 * (H // 2) - 2:2 * (H // 2), :2], x[0, 0, 2 * (H // 2) - 2:2 * (H // 2), :2] = 0.0, 1.0
    c[0, 0, 2 * (H // 2) - 2:2 * (H // 2), 2 * (W // 2) - 2:2 * (W // 2)] = 0.0
    x[0, 0, 2 * (H // 2) - 2:2 * (H // 2), 2 * (W // 2) - 2:2 * (W // 2)] = 1.0
    dout = torch.randn(N, C, H // 2, W // 2, generator=gen)
    out, dz2, de = _tail_check(hp, c, x, scale, 2, 0.2, dout)
    assert out.shape == (N, C, H // 2, W // 2)
    if H % 2:
        assert not bool(dz2[:, :, H - 1].any()) and not bool(de[:, :, H - 1].any())
    if W % 2:
        assert not bool(dz2[:, :, :, W - 1].any()) and not bool(de[:, :, :, W - 1].any())
    assert float(de[0, 0, 0, 0]) == float(dout[0, 0, 0, 0]) and not bool(de[0, 0, :2, :2].flatten()[1:].any())
    if kind == "drop":
        assert torch.equal(out[0, 1], F.max_pool2d(x[0:1, 1:2], 2)[0, 0]) and not bool(dz2[0, 1].any())


@pytest.mark.parametrize("kind", ["drop", "none"])
@pytest.mark.parametrize("pool", [1, 2])
def test_block_tail_slope_one_and_no_scale(hp, pool, kind):
    """slope = 1.0 (what sepstack passes): dz2 = unpool(dout) * scale, bit for bit; also the default slope on this map."""
    c, x, scale, gen = R.tail_case((2, 8, 7, 9), 21 + pool, kind)
    dout = torch.randn(2, 8, 7 // pool, 9 // pool, generator=gen)
    _tail_check(hp, c, x, scale, pool, 0.2, dout)
    out, dz2, de = _tail_check(hp, c, x, scale, pool, 1.0, dout)
    up = de if pool == 2 else dout
    assert torch.equal(dz2, up if scale is None else up * scale[:, :, None, None])
    if kind == "drop" and pool == 1:
        assert torch.equal(out[0, 1], x[0, 1]) and not bool(dz2[0, 1].any())


def test_block_tail_nan_in_a_window(hp):
    """One NaN inside a window and a window of four NaNs: the output is NaN and the gradient goes where ATen's CPU
    max_pool2d sends it (F.max_pool2d(..., return_indices=True)): a NaN replaces whatever came before it, another NaN
    included, and no later finite value replaces a NaN.  So the last NaN of a window takes the gradient (index 21 = (3,3)
    for the window of four), not the larger 50.0 behind the single NaN."""
    c, x, scale, gen = R.tail_case((1, 4, 6, 6), 31, "drop")
    x[0, 0, 0, 1] = math.nan; x[0, 0, 1, 1] = 50.0                               # a NaN, then a larger value after it
    x[0, 0, 2:4, 2:4] = math.nan                                                 # four NaNs
    x[0, 2, 5, 4] = math.nan                                                     # the NaN last in its window
    x[0, 3, 0, 0] = math.nan                                                     # the NaN first in its window
    dout = torch.randn(1, 4, 3, 3, generator=gen)
    out, dz2, de = _tail_check(hp, c, x, scale, 2, 0.2, dout)
    e = c * scale[:, :, None, None] + x
    pooled, idx = F.max_pool2d(e, 2, return_indices=True)
    want = torch.zeros(1, 4, 36).scatter_(2, idx.reshape(1, 4, 9), dout.reshape(1, 4, 9)).reshape(1, 4, 6, 6)
    assert torch.equal(de, want)
    assert math.isnan(float(out[0, 0, 0, 0])) and math.isnan(float(out[0, 0, 1, 1])) and math.isnan(float(out[0, 2, 2, 2]))
    assert int(torch.isnan(out).sum()) == 4 and int(idx[0, 0, 0, 0]) == 1


def test_block_tail_grid_stride(hp):
    """More outputs than 8192 blocks of 256: pool 1 forward and backward on (3, 64, 120, 120), pool 2 forward on
    (3, 64, 240, 240)."""
    shape = (3, 64, 120, 120)
    assert 3 * 64 * 120 * 120 > 8192 * 256
    c, x, scale, gen = R.tail_case(shape, 41, "drop")
    dout = torch.randn(shape, generator=gen)
    out, dz2, _ = _tail_run(hp, c, x, scale, 1, 0.2, dout)
    sc = scale[:, :, None, None]
    assert torch.equal(out, c * sc + x)
    want = dout * sc * torch.where(c > 0, torch.ones(()), torch.full((), 0.2))
    assert torch.allclose(dz2, want, rtol=1e-6, atol=1e-6)
    c, x, scale, gen = R.tail_case((3, 64, 240, 240), 42, "drop")
    out, _, _ = _tail_run(hp, c, x, scale, 2, 0.2, None)
    assert torch.equal(out, F.max_pool2d(c * scale[:, :, None, None] + x, 2))


# ------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ADAM_LENGTHS)
def test_adam_vs_float64(hp, n):
    """Lengths around the 4-wide vector body and its scalar tail, and two past 2048 * 256 * 4 (the grid-stride loop, with and
    without a tail); non-zero state; steps 1, 2, 1000, 100000; grad_scale 1, 1/2, 1/8; two consecutive calls."""
    for ci, step, gs in R.adam_combos(n):
        p, m, v, grads, dead = R.adam_case(n, 100 * ci + n % 97)
        pd, md, vd = p.cuda(), m.cuda(), v.cuda()
        p64, m64, v64 = p.double(), m.double(), v.double()
        for k, g in enumerate(grads):
            hp.adam_step(pd, g.cuda(), md, vd, step + k, lr=1e-3, grad_scale=gs)
            p64, m64, v64 = R.adam64(p64, g, m64, v64, step + k, lr=1e-3, grad_scale=gs)
            pc, mc, vc = pd.cpu(), md.cpu(), vd.cpu()
            assert torch.allclose(pc.double(), p64, rtol=1e-6, atol=1e-7), (ci, k)
            assert torch.allclose(mc.double(), m64, rtol=1e-5, atol=1e-6 * float(m64.abs().max())), (ci, k)
            assert torch.allclose(vc.double(), v64, rtol=1e-5, atol=1e-6 * float(v64.abs().max())), (ci, k)
            # g == m == v == 0: the parameter keeps its bits, the moments stay 0
            assert same_bits(pc[dead], p[dead]) and not bool(mc[dead].any()) and not bool(vc[dead].any())


def test_adam_refuses_an_unaligned_buffer(hp):
    from fdet_amd import FdetError
    t = [torch.zeros(9, device="cuda") for _ in range(4)]
    with pytest.raises(FdetError, match="16-byte aligned"):
        hp.adam_step(t[0][1:], t[1][1:], t[2][1:], t[3][1:], 1)
    assert not any(bool(a.any()) for a in t)


# ------------------------------------------------------------------------------------------
# yolo loss
# ------------------------------------------------------------------------------------------
def _yolo_check(hp, pred, gt):
    l64, g64 = R.yolo64(pred, gt)
    lpi, lsum, grad = hp.yolo_loss_fwd_bwd(pred.cuda(), gt.cuda())
    lpi, lsum, grad = lpi.cpu(), lsum.cpu(), grad.cpu()
    assert torch.equal(torch.isnan(lpi), torch.isnan(l64))
    fin = torch.isfinite(l64)
    assert bool(((lpi.double() - l64)[fin].abs() <= 1e-4 * l64[fin].abs()).all())
    if bool(fin.all()):
        assert abs(float(lsum) - float(l64.sum())) <= 1e-4 * abs(float(l64.sum()))
    assert torch.equal(torch.isnan(grad), torch.isnan(g64))
    assert torch.equal(torch.isinf(grad), torch.isinf(g64)) and torch.equal(grad[torch.isinf(g64)].double(), g64[torch.isinf(g64)])
    ok = torch.isfinite(g64)
    assert torch.allclose(grad[ok].double(), g64[ok], rtol=1e-4, atol=1e-6)
    return lpi, lsum, grad


@pytest.mark.parametrize("S_", [1, 7, 8, 9, 64])
def test_yolo_loss_grid_sizes(hp, S_):
    """1 cell, under a wave, exactly a wave, just over a wave, 4096 cells."""
    pred, gt = R.yolo_case(3, S_, 50 + S_)
    _yolo_check(hp, pred, gt)


def test_yolo_loss_sum_over_300_images(hp):
    pred, gt = R.yolo_case(300, 10, 7)
    lpi, lsum, _ = _yolo_check(hp, pred, gt)
    assert abs(float(lsum) - float(lpi.double().sum())) <= 1e-6 * float(lpi.double().sum())


def test_yolo_loss_grad_scale_and_no_grad(hp):
    pred, gt = R.yolo_case(3, 9, 8)
    lpi, lsum, grad = hp.yolo_loss_fwd_bwd(pred.cuda(), gt.cuda())
    lpi2, lsum2, grad2 = hp.yolo_loss_fwd_bwd(pred.cuda(), gt.cuda(), grad_scale=1.0 / 256)
    assert same_bits(grad2, grad.cpu() * 2.0 ** -8) and bool(grad.any())
    assert same_bits(lpi2, lpi.cpu()) and same_bits(lsum2, lsum.cpu())
    lpi3, lsum3, none = hp.yolo_loss_fwd_bwd(pred.cuda(), gt.cuda(), want_grad=False)
    assert none is None and same_bits(lpi3, lpi.cpu()) and same_bits(lsum3, lsum.cpu())


def test_yolo_loss_nansum_zero_keeps_the_nan(hp):
    """nansum(pred) == 0: nan_to_num does not run and the NaN reaches the loss; with a non-zero nansum the NaN becomes 0.1,
    the loss is finite and the gradient at the NaN's place is exactly 0."""
    pred, gt = R.yolo_nan_case()
    lpi, _, grad = _yolo_check(hp, pred, gt)
    assert math.isnan(float(lpi[0])) and math.isfinite(float(lpi[1]))
    assert float(grad[1, 0, 3, 5]) == 0.0 and not bool(torch.isnan(grad[1]).any())


def test_yolo_loss_zero_width_singularity(hp):
    pred, gt = R.yolo_zero_wh_case()
    _, _, grad = _yolo_check(hp, pred, gt)
    assert bool(torch.isnan(grad).any()) and bool(torch.isinf(grad).any())


# ------------------------------------------------------------------------------------------
# step metrics
# ------------------------------------------------------------------------------------------
def test_step_metrics_per_image(hp):
    """(G, P) = (0,0), (0,3), (3,0), (1,1) identical, (12,12) (144 pairs: the lane loop runs three times), (5,7); zero-area
    boxes on both sides (0/0 -> 0).  Recall and precision exact; the iou sum within 4 x the fp32 evaluation's own distance
    from float64 (floor 1e-6 of the column's scale), never above the project's 1e-4.  Measured on the MI355X: fp32 torch
    1.8e-7, the kernel 1.8e-7, bound 1.1e-5 (the floor: the largest sum is 10.98)."""
    gt, gc, pr, pc = R.metrics_case()
    ref = R.metrics_per_image(gt, gc, pr, pc)
    ref32 = R.metrics_per_image(gt, gc, pr, pc, dtype=torch.float32)
    per, tot = hp.step_metrics(gt.cuda(), gc.cuda(), pr.cuda(), pc.cuda())
    per, tot = per.cpu(), tot.cpu()
    assert torch.equal(per[:, 1:], ref[:, 1:].float())
    tol = min(R.rule_tol(ref32[:, 0], ref[:, 0]), 1e-4 * max(1.0, float(ref[:, 0].abs().max())))
    print(f"metrics iou sum: fp32 {R.dist(ref32[:, 0], ref[:, 0]):.3g} kernel {R.dist(per[:, 0], ref[:, 0]):.3g} bound {tol:.3g}")
    assert R.dist(per[:, 0], ref[:, 0]) <= tol
    assert not bool(per[:3].any())
    assert torch.equal(tot, (per.double().sum(0) / per.shape[0]).float())
