"""numpy restatement of Int8Resnet's arithmetic (include/fdet.h, "Int8 inference": fdet_stem3_fwd_q8_u8), on top
of tests/q8_cpu_ref.py.

Written from the contract, not from the kernels.  The input of the stem is the uint8 frame itself (codes 0..255, scale
1 / 255); its weights are prepared exactly as a trunk conv's.  Integers stay exact: the integer GEMMs run as float64
`torch.conv2d` of integer values (|acc| < 2^53), every float step is one float32 operation, rounding is numpy's rint."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import q8_cpu_ref as R

F32 = np.float32
S_IN = F32(1.0) / F32(255.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G22_PARTS = ("g22_trained_resnet_medium", "g22_trained_resnet_medium_b", "g22_trained_resnet_medium_c",
             "g22_trained_resnet_medium_d")


def load_g22():
    """The trained Resnet-medium fixture (tools/make_goldens_resnet.py) as {name: tensor}: the archive's tensors are spread
    over four files (a committed file stays under 1 MiB), `y` / `dets` / `ndets` are in the first."""
    out = {}
    for name in G22_PARTS:
        with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
            for k in z.files:
                out[k] = torch.from_numpy(z[k]) if z[k].dtype.kind in "fiub" else z[k]
    return out


# ------------------------------------------------------------------------------------------------------- integer convs
def _acc(x_int, w_q, b_q, stride, pad=1):
    """b_q[co] + sum x * w as an exact float64 conv -> int64 (N,Co,Ho,Wo)."""
    x = torch.from_numpy(np.ascontiguousarray(x_int).astype(np.float64))
    w = torch.from_numpy(np.ascontiguousarray(w_q).astype(np.float64))
    acc = F.conv2d(x, w, torch.from_numpy(np.asarray(b_q).astype(np.float64)), stride=stride, padding=pad).numpy()
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return np.rint(acc).astype(np.int64)


def conv_acc(x_q, w_q, b_q):
    """q8_cpu_ref.conv_acc by torch.conv2d (the same integers, faster on large maps)."""
    return _acc(x_q, w_q, b_q, 1)


def stem3_acc(frames_u8, w_q, b_q):
    """acc = b_q[co] + sum over (ci,ky,kx) of x_u8[ci][2oy+ky-1][2ox+kx-1] * w_q[co][ci][ky][kx]; outside the image: 0."""
    assert frames_u8.dtype == np.uint8 and w_q.shape[1:] == (3, 3, 3)
    return _acc(frames_u8, w_q, b_q, 2)


def stem3_q(frames_u8, w_q, b_q, mul):
    """fdet_stem3_fwd_q8_u8 on plain NCHW: t = float(acc) * mul[co]; q = clamp(rint(t), -127, 127).  No LeakyReLU."""
    acc = stem3_acc(frames_u8, w_q, b_q)
    return R.rint_clamp(acc.astype(F32) * np.asarray(mul, F32)[None, :, None, None])


def stem3(frames_u8, w, b, s_out):
    """uint8 frames (N,3,H,W), float conv1 weights / bias, the stem's output scale -> int8 (N,F,H/2,W/2)."""
    return stem3_q(frames_u8, *R.prepare_conv(np.asarray(w), np.asarray(b), S_IN, s_out))


def stem3_loops(frames_u8, w_q, b_q, mul):
    """The contract element by element (python ints, one float32 op at a time); for small shapes."""
    N, C, H, W = frames_u8.shape
    Co = w_q.shape[0]
    q = np.zeros((N, Co, H // 2, W // 2), np.int8)
    for n in range(N):
        for co in range(Co):
            for oy in range(H // 2):
                for ox in range(W // 2):
                    acc = int(b_q[co])
                    for ci in range(C):
                        for ky in range(3):
                            for kx in range(3):
                                y, x = 2 * oy + ky - 1, 2 * ox + kx - 1
                                if 0 <= y < H and 0 <= x < W:
                                    acc += int(frames_u8[n, ci, y, x]) * int(w_q[co, ci, ky, kx])
                    t = F32(acc) * F32(mul[co])
                    q[n, co, oy, ox] = int(min(max(np.rint(t), -127), 127))
    return q


def stem3_shifted_acc(frames_u8, w_q, b_q):
    """The identity the kernel relies on: rows staged as x - 128 with -128 (the code 0) for everything outside the image, all
    27 taps always present, and 128 * sum(w_q[co]) folded into the bias."""
    N, C, H, W = frames_u8.shape
    xs = np.full((N, C, H + 2, W + 2), -128, np.int64)
    xs[:, :, 1:-1, 1:-1] = frames_u8.astype(np.int64) - 128
    cst = b_q.astype(np.int64) + 128 * w_q.astype(np.int64).reshape(w_q.shape[0], -1).sum(axis=1)
    return _acc(xs, w_q, cst, 2, pad=0)


def pack_stem_weights(w_q):
    """[F][3][3][3] -> the kernel's [F][32], k = (ci*3+ky)*3+kx, bytes 27..31 zero."""
    out = np.zeros((w_q.shape[0], 32), np.int8)
    out[:, :27] = w_q.reshape(w_q.shape[0], 27)
    return out


# ------------------------------------------------------------------------------------------------------- trunk
def conv3x3(x_q, w_q, b_q, mul, skip_q=None, skip_mul=None, pool=False, slope=R.SLOPE):
    q = R.rint_clamp(R.epilogue_float(conv_acc(x_q, w_q, b_q), mul, skip_q, skip_mul, slope))
    return R.maxpool2(q) if pool else q


def trunk_q(q0, P, s_h, s_a, S):
    """int8 stem output (N,F,H,W) -> (list of int8 block outputs, fp32 head input).  q8_cpu_ref.block's arithmetic with
    Resnet's pooling rule: a block pools iff its map is larger than S."""
    q, outs = q0, []
    for c1, c2, sm in R.prepare_trunk(P, s_h, s_a):
        a = conv3x3(q, *c1)
        q = conv3x3(a, *c2, skip_q=q, skip_mul=sm, pool=q.shape[2] > S)
        outs.append(q)
    return outs, R.dequantize(q, s_h[-1])


def model_q(frames_u8, P, s_h, s_a, S):
    """frames -> (int8 stem output, block outputs, y) with the torch fp32 head."""
    P = {k: np.asarray(v) for k, v in P.items()}
    q0 = stem3(frames_u8, P["conv1.weight"], P["conv1.bias"], s_h[0])
    outs, hd = trunk_q(q0, P, s_h, s_a, S)
    with torch.no_grad():
        y = torch.sigmoid(F.conv2d(torch.from_numpy(hd), torch.from_numpy(P["out.weight"]), torch.from_numpy(P["out.bias"]),
                                   padding=1))
    return q0, outs, y


# ------------------------------------------------------------------------------------------------------- float model
def float_intermediates(P, x, S):
    """torch fp32 ops on the CPU: block inputs h_0..h_nb (h_0 is the stem output) and first-conv outputs a_k of a Resnet."""
    nb = sum(1 for k in P if k.endswith(".conv1.weight") and k.startswith("residual_blocks."))
    with torch.no_grad():
        h = F.conv2d(x, P["conv1.weight"], P["conv1.bias"], stride=2, padding=1)
        hs, as_ = [], []
        for k in range(nb):
            n = f"residual_blocks.{k}"
            hs.append(h)
            a = F.leaky_relu(F.conv2d(h, P[n + ".conv1.weight"], P[n + ".conv1.bias"], padding=1), 0.2)
            as_.append(a)
            e = F.leaky_relu(F.conv2d(a, P[n + ".conv2.weight"], P[n + ".conv2.bias"], padding=1), 0.2) + h
            h = F.max_pool2d(e, 2) if e.shape[2] > S else e
        hs.append(h)
        y = torch.sigmoid(F.conv2d(h, P["out.weight"], P["out.bias"], padding=1))
    return hs, as_, y


def absmax_scales(hs, as_):
    def scale(t):
        v = float(t.abs().max())
        return F32(1.0) if v == 0.0 else F32(v) / F32(127.0)
    return np.array([scale(t) for t in hs], F32), np.array([scale(t) for t in as_], F32)
