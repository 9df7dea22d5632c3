"""CPU checks of tests/train_math_cpu_ref.py: the references agree with the fp32 oracle, the golden fixtures and plain
torch, and the input builders produce the cases they were built for (ties at the mining threshold, saturated
confidences, inputs on which fp32 itself meets the GPU test's bounds) before any kernel sees them."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as O
from oracle import ssd_oracle as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_math_cpu_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------
# dropout restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_restatement_drops_p_of_the_draws(p):
    n = 1 << 20
    s = R.dropout_scales(n, p, 1234, 0)
    ks = R.keep_scale(p)
    assert s.dtype == np.float32 and set(np.unique(s).tolist()) == {0.0, float(ks)}
    assert float(ks) == float(np.float32(1) / np.float32(1 - p))
    dropped = float((s == 0).mean())
    assert abs(dropped - p) <= 5 * math.sqrt(p * (1 - p) / n), dropped      # 0.0021 / 0.0024: the binomial's 5 sigma
    u = R.u01(1234, np.arange(n, dtype=np.uint64))
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal(s == 0, u < np.float32(p))


def test_dropout_restatement_counters_concatenate_and_wrap():
    a, n = 3 << 40, 1000
    whole = R.dropout_scales(2 * n, 0.25, 7, a)
    assert np.array_equal(np.concatenate([R.dropout_scales(n, 0.25, 7, a), R.dropout_scales(n, 0.25, 7, a + n)]), whole)
    assert np.all(R.dropout_scales(257, 0.0, 7, a) == 1.0)
    # mod 2^64: seed 2^64 - 1, counters 2^64 - 3 .. 2^64 + 4, against python integers
    seed, off = (1 << 64) - 1, (1 << 64) - 3
    want = []
    for i in range(8):
        z = (seed + 0x9E3779B97F4A7C15 * ((off + i + 1) & R.M64)) & R.M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
        z = z ^ (z >> 31)
        want.append((z >> 40) / 16777216.0)
    u = R.u01(seed, np.array([(off + i) & R.M64 for i in range(8)], dtype=np.uint64))
    assert u.tolist() == want
    got = R.dropout_scales(8, 0.5, seed, off)
    assert got.tolist() == [0.0 if w < 0.5 else 2.0 for w in want] and 0 < int((got == 0).sum()) < 8
    assert np.array_equal(got[3:], R.dropout_scales(5, 0.5, seed, 0))      # the counter wrapped to 0 at i = 3


def test_dropout_layers_restatement_layout():
    ch, p, n = [16, 64, 5], [0.25, 0.25, 0.5], 7
    base, first = 1 << 33, 11
    L = R.dropout_layers(n, ch, p, 99, base, first)
    assert [a.shape for a in L] == [(n, c) for c in ch]
    ls, pre = sum(ch), 0
    for k, C in enumerate(ch):
        for i in (0, 3, 6):
            assert np.array_equal(L[k][i], R.dropout_scales(C, p[k], 99, base + (first + i) * ls + pre))
        pre += C
    # the data-parallel promise: rows 2..4 of a 5-image call are the 3-image call that starts at image 2
    A, B = R.dropout_layers(5, ch, p, 99, base, 0), R.dropout_layers(3, ch, p, 99, base, 2)
    assert all(np.array_equal(a[2:5], b) for a, b in zip(A, B))


# ------------------------------------------------------------------------------------------
# mining inputs
# ------------------------------------------------------------------------------------------
def test_tie_batch_has_ties_across_the_threshold():
    boxes = R.ssd_tie_boxes()
    assert [int(b.shape[0] > 0) for b in boxes] == [1, 1, 0, 1]
    pred, target = R.ssd_tie_case()
    st = R.mining_stats(pred, target, 10)
    assert st[2]["npos"] == 0 and st[2]["selected"] == 0 and st[2]["kk"] == 0
    tied = [s for s in st if 0 < s["kk"] < s["P_neg"] and s["tie_sel"] > 0 and s["tie_unsel"] > 0]
    assert len(tied) >= 1, st
    assert all(s["ordered"] for s in st), st
    assert any(s["tie_sweeps"] >= 2 for s in tied), st                      # the tied run crosses a multiple of 256
    assert all(s["selected"] == s["kk"] for s in st), st
    # the four images' encode is what a positive label means everywhere below
    assert int((target[:, :, 0] > 0).sum()) == sum(s["npos"] for s in st) > 0


@pytest.mark.parametrize("P", R.SSD_SMALL_P)
def test_small_batches_reach_every_kk_path(P):
    pred, target = R.ssd_small_case(P)
    st = R.mining_stats(pred, target, 3)
    if P == 1:
        assert [(s["npos"], s["P_neg"]) for s in st] == [(1, 0), (0, 1), (0, 1)]
        assert [s["selected"] for s in st] == [0, 0, 0]
        return
    a, b, c = st
    assert 0 < a["npos"] * 3 < a["P_neg"] and a["selected"] == a["npos"] * 3
    if P % 4 == 0:
        assert b["npos"] * 3 == b["P_neg"]                                  # kk == P_neg exactly
    else:
        assert b["P_neg"] < b["npos"] * 3 <= b["P_neg"] + 3
    assert c["npos"] * 3 > c["P_neg"] + 3
    assert b["selected"] == b["P_neg"] and c["selected"] == c["P_neg"] and b["P_neg"] > 0 and c["P_neg"] > 0
    assert all(s["ordered"] for s in st)
    # ratio 0: nothing is mined
    assert not bool((R.ssd_mask32(pred, target, 0) & ~(target[:, :, 0] > 0)).any())


def test_saturated_batch_is_what_it_says():
    pred, target = R.ssd_saturated_case()
    st = R.mining_stats(pred, target, 10)
    assert [(s["npos"], s["kk"], s["P_neg"]) for s in st] == [(10, 100, 290), (2, 20, 298), (40, 260, 260)]
    mask = R.ssd_mask32(pred, target, 10)
    neg = target[:, :, 0] == 0
    conf = pred[:, :, 0]
    zero_neg = neg[1] & (conf[1] == 0)
    assert int(zero_neg.sum()) == 20 and torch.equal(mask[1] & neg[1], zero_neg)     # +inf losses are mined first
    for n in (0, 2):
        for v in (0.0, 1.0, R.LO32, R.HI32, 1e-8):
            assert bool((neg[n] & (conf[n] == np.float32(v))).any()), (n, v)
        assert bool((neg[n] & (conf[n] < R.LO32) & (conf[n] > 1e-8)).any()) and bool((neg[n] & (conf[n] > R.HI32) & (conf[n] < 1)).any())
        pos = ~neg[n]
        assert bool((pos & (conf[n] == 0)).any()) and bool((pos & (conf[n] == 1)).any())
    assert bool(mask[2].all())
    ref = R.ssd_loss64(pred, target, 10)
    g0 = ref["grad"][:, :, 0]
    outside = mask & ((conf < R.LO32) | (conf > R.HI32))
    assert int(outside.sum()) >= 10 and bool((g0[outside] == 0).all())
    at = mask & ((conf == R.LO32) | (conf == R.HI32))
    assert int(at.sum()) >= 4 and bool(torch.isfinite(g0[at]).all()) and bool((g0[at] != 0).all())
    assert math.isfinite(float(ref["loss"]))


def test_label_batch_is_what_it_says():
    pred, target = R.ssd_label_case()
    lab = target[:, :, 0]
    assert int((lab == np.float32(0.3)).sum()) == 8 and int((lab == 0.5).sum()) == 8 and int((lab == np.float32(0.94)).sum()) == 8
    assert float(torch.round(torch.tensor(0.5))) == 0.0
    pos = lab > 0
    d = (pred[:, :, 1:] - target[:, :, 1:])[pos]
    for v in R.SL1_D:
        assert bool((d == np.float32(v)).any()), v
    st = R.mining_stats(pred, target, 3)
    assert all(s["npos"] == 12 and s["selected"] == 36 for s in st)


# ------------------------------------------------------------------------------------------
# references against the fp32 oracle, the goldens and plain torch
# ------------------------------------------------------------------------------------------
def _close_ssd(ref, loss, gc, gl):
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-5 * abs(float(loss))
    assert torch.allclose(ref["grad"][:, :, 0].float(), gc, rtol=1e-5, atol=1e-9)
    assert torch.allclose(ref["grad"][:, :, 1:].float(), gl, rtol=1e-5, atol=1e-9)


def test_ssd_loss64_equals_the_fp32_oracle_on_a_random_batch():
    gen = torch.Generator().manual_seed(3)
    boxes = O.synthetic_boxes(3, R.SIZE, seed=8, max_faces=6)
    target = torch.stack([S.ssd_encode(b if b.numel() else torch.tensor([]), (R.SIZE, R.SIZE)) for b in boxes])
    pred = torch.rand(3, R.SSD_P, 5, generator=gen) * 0.98 + 0.01
    loss, gc, gl = S.ssd_loss_and_grads(pred[:, :, 0], pred[:, :, 1:], target[:, :, 0], target[:, :, 1:], 10)
    _close_ssd(R.ssd_loss64(pred, target, 10), loss, gc, gl)
    for case, ratio in ((R.ssd_tie_case(), 10), (R.ssd_label_case(), 3), (R.ssd_small_case(257), 3)):
        pred, target = case
        loss, gc, gl = S.ssd_loss_and_grads(pred[:, :, 0], pred[:, :, 1:], target[:, :, 0], target[:, :, 1:], ratio)
        _close_ssd(R.ssd_loss64(pred, target, ratio), loss, gc, gl)


def test_ssd_loss64_equals_the_golden(golden):
    g = golden("g9_ssd")
    ref = R.ssd_loss64(g["loss_pred"], g["loss_y"], 10)
    assert torch.equal(ref["mask"], g["mask"].bool())
    _close_ssd(ref, g["loss"], g["loss_gc"], g["loss_gl"])


def test_ssd_loss64_all_negative_batch_follows_autograd():
    """No positive prior in the batch: 0 / 0 is NaN, and autograd sends nothing to the predictions (nothing was selected)."""
    pred, target = R.ssd_all_negative_case()
    ref = R.ssd_loss64(pred, target, 10)
    assert math.isnan(float(ref["loss"])) and not bool(ref["mask"].any())
    loss, gc, gl = S.ssd_loss_and_grads(pred[:, :, 0], pred[:, :, 1:], target[:, :, 0], target[:, :, 1:], 10)
    assert math.isnan(float(loss))
    assert torch.equal(torch.isnan(gc), torch.isnan(ref["grad"][:, :, 0])) and torch.equal(torch.isnan(gl), torch.isnan(ref["grad"][:, :, 1:]))
    assert torch.equal(torch.nan_to_num(gc, 7.0).double(), torch.nan_to_num(ref["grad"][:, :, 0], 7.0))
    assert torch.equal(torch.nan_to_num(gl, 7.0).double(), torch.nan_to_num(ref["grad"][:, :, 1:], 7.0))


@pytest.mark.parametrize("n", R.ADAM_LENGTHS)
def test_adam_fp32_oracle_is_within_half_the_gpu_bounds(n):
    """On every input of the GPU test the fp32 oracle stays within half of each bound of adam64: the bound is one fp32
    arithmetic can meet there."""
    worst = [0.0, 0.0, 0.0]
    for ci, step, gs in R.adam_combos(n):
        p, m, v, grads, dead = R.adam_case(n, 100 * ci + n % 97)
        p32, m32, v32 = p, m, v
        p64, m64, v64 = p.double(), m.double(), v.double()
        for k, g in enumerate(grads):
            p32, m32, v32 = R.adam32(p32, g, m32, v32, step + k, lr=1e-3, grad_scale=gs)
            p64, m64, v64 = R.adam64(p64, g, m64, v64, step + k, lr=1e-3, grad_scale=gs)
            for w, (a, b, rtol, atol) in enumerate(((p32, p64, 1e-6, 1e-7), (m32, m64, 1e-5, 1e-6 * float(m64.abs().max())),
                                                    (v32, v64, 1e-5, 1e-6 * float(v64.abs().max())))):
                frac = ((a.double() - b).abs() / (atol + rtol * b.abs())).max()
                worst[w] = max(worst[w], float(frac))
            assert torch.equal(p32[dead], p[dead]) and not bool(m32[dead].any()) and not bool(v32[dead].any())
    assert max(worst) <= 0.5, worst


@pytest.mark.parametrize("pool,slope,kind", [(2, 0.2, "drop"), (1, 0.2, "drop"), (2, 1.0, "none"), (1, 1.0, "drop")])
def test_tail64_equals_plain_fp32_torch(pool, slope, kind):
    c, x, scale, gen = R.tail_case((2, 8, 7, 9), 5, kind)
    dout = torch.randn(2, 8, 7 // pool, 9 // pool, generator=gen)
    out64, gz64, gx64 = R.tail64(c, x, scale, pool, slope, dout)
    cr, xr = c.clone().requires_grad_(True), x.clone().requires_grad_(True)
    sc = 1.0 if scale is None else scale[:, :, None, None]
    e = cr * sc + xr
    out = F.max_pool2d(e, 2) if pool == 2 else e
    gc, gx = torch.autograd.grad(out, [cr, xr], dout)
    gz = gc * torch.where(c > 0, torch.ones(()), torch.full((), slope))        # dz2 = dc * lrelu'(c)
    assert torch.allclose(out64.float(), out.detach(), rtol=1e-6, atol=1e-6)
    assert torch.allclose(gz64.float(), gz, rtol=1e-6, atol=1e-6)
    assert torch.equal(gx64.float(), gx)
    if pool == 2:                                                              # floor: the odd last row / column is in no window
        assert out64.shape[2:] == (3, 4) and not bool(gx64[:, :, 6].any()) and not bool(gx64[:, :, :, 8].any())


@pytest.mark.parametrize("N,CP,ps", [(2, 5, 7), (3, 8, 15)])
def test_head_pack64_equals_plain_fp32_torch(N, CP, ps):
    z, dy = R.head_pack_case(N, CP, ps, 6)
    start = R.SSD_START[ps]
    y64, dz64 = R.head_pack64(z, ps, start, R.SSD_P, dy)
    zr = z.clone().requires_grad_(True)
    y = torch.full((N, R.SSD_P, 5), math.nan)
    rows = []
    for i in range(ps):
        for j in range(ps):
            rows.append(torch.stack([torch.sigmoid(zr[:, 0, i, j]), zr[:, 1, i, j] / ps + i / ps, zr[:, 2, i, j] / ps + j / ps,
                                     zr[:, 3, i, j], zr[:, 4, i, j]], -1))
    rows = torch.stack(rows, 1)
    y[:, start:start + ps * ps] = rows.detach()
    (dz,) = torch.autograd.grad(rows, zr, dy[:, start:start + ps * ps])
    assert torch.equal(torch.isnan(y64), torch.isnan(y)) and int(torch.isnan(y).sum()) == N * (R.SSD_P - ps * ps) * 5
    assert torch.allclose(torch.nan_to_num(y64).float(), torch.nan_to_num(y), rtol=1e-6, atol=1e-7)
    assert torch.allclose(dz64.float(), dz, rtol=1e-5, atol=1e-7)
    assert not bool(dz64[:, 5:].any())
    assert float(y[0, start, 0]) == 1.0 and float(y[0, start + 1, 0]) == 0.0 and float(y[0, start + 2, 0]) == 0.5
    assert float(dz[0, 0, 0, 0]) == 0.0 and float(dz[0, 0, 0, 1]) == 0.0      # fp32 sigmoid saturates: gradient exactly 0


def test_metrics_per_image_sums_to_the_oracle():
    B, S_, size = 32, 10, 480
    g = torch.Generator().manual_seed(4)
    y = torch.stack([O.encode_targets(b, (size, size), S_) for b in O.synthetic_boxes(B, size, seed=3)])
    y_hat = (y + 0.08 * torch.rand(B, 5, S_, S_, generator=g)).clamp(0, 1)
    y_hat[:, 0] = torch.where(torch.rand(B, S_, S_, generator=g) > 0.97, torch.ones(()), y_hat[:, 0])
    red = O.ReduceBoundingBoxes(0.5, 0.5, (3, size, size), S_)
    ref = O.step_metrics(y_hat, y, red)
    K = S_ * S_
    gt, pr = torch.zeros(B, K, 5), torch.zeros(B, K, 5)
    gc, pc = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for n in range(B):
        a, b = red(y[n]), red(y_hat[n])
        gt[n, :a.shape[0]], pr[n, :b.shape[0]] = a, b
        gc[n], pc[n] = a.shape[0], b.shape[0]
    per = R.metrics_per_image(gt, gc, pr, pc, dtype=torch.float32)
    tot = per.sum(0) / B
    assert float(tot[0]) > 0 and int((pc > 0).sum()) > 1
    for k in range(3):
        assert abs(float(tot[k]) - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (k, float(tot[k]), ref[k])


def test_metrics_case_is_what_it_says():
    gt, gc, pr, pc = R.metrics_case()
    assert list(zip(gc.tolist(), pc.tolist())) == list(R.METRIC_COUNTS) and gt.shape == (6, 12, 5)
    assert torch.equal(gt, gt.round()) and torch.equal(pr, pr.round())
    per = R.metrics_per_image(gt, gc, pr, pc)
    assert per[:3].abs().sum() == 0                                           # (0,0), (0,3), (3,0): nothing counted
    assert per[3].tolist() == [1.0, 1.0, 1.0]
    assert 0 < float(per[4, 1]) < 1 and 0 < float(per[5, 2]) < 1               # hits and misses in the lane loop
    # the zero-area pair is 0 / 0 before nan_to_num
    b = gt[4, 1:2, 1:].clone(); b[:, 2:] += b[:, :2]
    q = pr[4, 2:3, 1:].clone(); q[:, 2:] += q[:, :2]
    assert bool(torch.isnan(O.box_iou(b, q)).all())


def test_yolo_cases_are_what_they_say():
    pred, gt = R.yolo_nan_case()
    assert float(torch.nansum(pred[0])) == 0.0 and float(torch.nansum(pred[1])) != 0.0
    l64, g64 = R.yolo64(pred, gt)
    l32 = torch.stack([O.yolo_loss(pred[n], gt[n]) for n in range(2)])
    assert math.isnan(float(l32[0])) and math.isnan(float(l64[0])) and math.isfinite(float(l64[1]))
    assert float(g64[1, 0, 3, 5]) == 0.0
    pred, gt = R.yolo_zero_wh_case()
    _, g = R.yolo64(pred, gt)
    assert bool(torch.isinf(g[0]).any()) and bool(torch.isnan(g[0]).any()) and bool(torch.isnan(g[1]).any())
    for S_ in (1, 7, 8, 9, 64):
        pred, gt = R.yolo_case(3, S_, 50 + S_)
        assert float(gt[0, 0].sum()) == 1.0 and bool(torch.isfinite(R.yolo64(pred, gt)[1]).all())
