"""numpy restatement of Int8PoolResnet's integer stem (include/fdet.h, "Int8 inference": fdet_stem10_fwd_q8_u8), on
top of tests/q8_cpu_ref.py.

Written from the contract, not from the kernel.  The input of the stem is the uint8 frame itself (codes 0..255, scale
1 / 255); its weights are prepared exactly as a trunk conv's.  Integers stay exact: the integer conv runs as a float64
`torch.conv2d` (stride 8, padding 2) of integer values (|acc| < 2^53), every float step is one float32 operation, rounding
is numpy's rint."""
import numpy as np
import torch
import torch.nn.functional as F

import q8_cpu_ref as R

F32 = np.float32
S_IN = F32(1.0) / F32(255.0)

# (N, F, H, W): the shapes of tests/test_gpu_q8_pool_stem.py, reused by the host file for the shift identity
SHAPES = [(1, 64, 6, 6), (1, 64, 14, 134), (3, 64, 22, 262), (2, 128, 17, 45), (1, 256, 6, 22), (1, 64, 10, 4094)]


def out_hw(H, W):
    return (H - 6) // 8 + 1, (W - 6) // 8 + 1


def make_case(shape):
    """Deterministic inputs of one shape: uniform uint8 frames with the bytes 0 and 255 planted, w_q uniform in -127..127, b_q
    uniform in +-400000, mul = exp2(U(-12.5, -10.5)); the seed is sum(shape)."""
    N, F_, H, W = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(0, 256, (N, 3, H, W)).astype(np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    w = rng.integers(-127, 128, (F_, 3, 10, 10)).astype(np.int8)
    b = rng.integers(-400000, 400001, F_).astype(np.int32)
    mul = np.exp2(rng.uniform(-12.5, -10.5, F_)).astype(F32)
    return x, w, b, mul


def _acc(x_int, w_q, b_q, pad):
    x = torch.from_numpy(np.ascontiguousarray(x_int).astype(np.float64))
    w = torch.from_numpy(np.ascontiguousarray(w_q).astype(np.float64))
    acc = F.conv2d(x, w, torch.from_numpy(np.asarray(b_q).astype(np.float64)), stride=8, padding=pad).numpy()
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return np.rint(acc).astype(np.int64)


def stem10_acc(frames_u8, w_q, b_q):
    """acc = b_q[co] + sum over (ci,ky,kx) of x_u8[ci][8oy+ky-2][8ox+kx-2] * w_q[co][ci][ky][kx]; outside the image: 0."""
    assert frames_u8.dtype == np.uint8 and w_q.shape[1:] == (3, 10, 10)
    return _acc(frames_u8, w_q, b_q, 2)


def stem10_q(frames_u8, w_q, b_q, mul):
    """fdet_stem10_fwd_q8_u8 on plain NCHW: t = float(acc) * mul[co]; q = clamp(rint(t), -127, 127).  No LeakyReLU."""
    acc = stem10_acc(frames_u8, w_q, b_q)
    return R.rint_clamp(acc.astype(F32) * np.asarray(mul, F32)[None, :, None, None])


def stem10(frames_u8, w, b, s_out):
    """uint8 frames (N,3,H,W), float conv1 weights / bias, the stem's output scale -> int8 (N,F,Ho,Wo)."""
    return stem10_q(frames_u8, *R.prepare_conv(np.asarray(w), np.asarray(b), S_IN, s_out))


def stem10_loops(frames_u8, w_q, b_q, mul):
    """The contract element by element (python ints, one float32 op at a time); for small shapes."""
    N, C, H, W = frames_u8.shape
    Co = w_q.shape[0]
    Ho, Wo = out_hw(H, W)
    q = np.zeros((N, Co, Ho, Wo), np.int8)
    for n in range(N):
        for co in range(Co):
            for oy in range(Ho):
                for ox in range(Wo):
                    acc = int(b_q[co])
                    for ci in range(C):
                        for ky in range(10):
                            y = 8 * oy + ky - 2
                            if not 0 <= y < H:
                                continue
                            for kx in range(10):
                                x = 8 * ox + kx - 2
                                if 0 <= x < W:
                                    acc += int(frames_u8[n, ci, y, x]) * int(w_q[co, ci, ky, kx])
                    t = F32(acc) * F32(mul[co])
                    q[n, co, oy, ox] = int(min(max(np.rint(t), -127), 127))
    return q


def stem10_shifted_acc(frames_u8, w_q, b_q):
    """The identity the kernel relies on: rows staged as x - 128 with -128 (the code 0) for everything outside the image -- two
    columns left, two rows above, whatever the last windows read past the far edges --, all 300 taps always present, and
    128 * sum(w_q[co]) folded into the bias."""
    N, C, H, W = frames_u8.shape
    Ho, Wo = out_hw(H, W)
    He, We = max(H + 2, 8 * (Ho - 1) + 10), max(W + 2, 8 * (Wo - 1) + 10)
    xs = np.full((N, C, He, We), -128, np.int64)
    xs[:, :, 2:2 + H, 2:2 + W] = frames_u8.astype(np.int64) - 128
    cst = b_q.astype(np.int64) + 128 * w_q.astype(np.int64).reshape(w_q.shape[0], -1).sum(axis=1)
    return _acc(xs, w_q, cst, 0)[:, :, :Ho, :Wo]


def pack_stem10_weights(w_q):
    """[F][3][10][10] -> the kernel's [F][32][16]: row ci*10+ky (rows 30, 31 zero), slot kx (slots 10..15 zero)."""
    out = np.zeros((w_q.shape[0], 32, 16), np.int8)
    out[:, :30, :10] = w_q.reshape(w_q.shape[0], 30, 10)
    return out


def model_q(frames_u8, P, s_h, s_a, S, head_pad=0):
    """frames -> (int8 stem output, block outputs, y) with the restatement trunk (a block pools iff its map is larger than
    2 S) and the torch fp32 head."""
    P = {k: np.asarray(v) for k, v in P.items()}
    q0 = stem10(frames_u8, P["conv1.weight"], P["conv1.bias"], s_h[0])
    q, outs = q0, []
    for c1, c2, sm in R.prepare_trunk(P, s_h, s_a):
        _, q = R.block(q, c1, c2, sm, pool=q.shape[2] > 2 * S)
        outs.append(q)
    hd = R.dequantize(q, s_h[-1])
    with torch.no_grad():
        y = torch.sigmoid(F.conv2d(torch.from_numpy(hd), torch.from_numpy(P["out.weight"]), torch.from_numpy(P["out.bias"]),
                                   padding=head_pad))
    return q0, outs, y
