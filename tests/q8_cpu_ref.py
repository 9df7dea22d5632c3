"""numpy restatement of the int8 inference arithmetic (include/fdet.h, "Int8 inference").

Everything is written from the contract, not from the kernels: integers stay exact (the integer GEMM runs as a float64
matmul of integer values, |acc| < 2^53), every float step is ONE float32 operation with one rounding, and rounding is
numpy's rint (half to even).  Feature maps are plain NCHW here; the halo layout is the kernels' business."""
import numpy as np

F32 = np.float32
SLOPE = F32(0.2)


# ------------------------------------------------------------------------------------------------------- quantise
def rint_clamp(t):
    """clamp(rint(t), -127, 127) of a float32 array -> int8 (NaN -> 0 is the quantiser's rule, see quantize)."""
    return np.clip(np.rint(t), -127, 127).astype(np.int8)


def quantize(x, s):
    """q = clamp(rintf(x * (1.0f / s)), -127, 127); NaN -> 0."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = F32(1.0) / F32(s)                            # (inf for a denormal scale: 0 * inf is a NaN product -> 0)
        t = x * inv
        q = np.clip(np.rint(np.where(np.isnan(t), F32(0), t)), -127, 127)
    return q.astype(np.int8)


def dequantize(q, s):
    return q.astype(F32) * F32(s)


# ------------------------------------------------------------------------------------------------------- preparation
def weight_scales(w):
    """per output channel: absmax / 127 (float32 division); a channel of zeros gets 1."""
    w = np.asarray(w, dtype=F32)
    m = np.abs(w).reshape(w.shape[0], -1).max(axis=1).astype(F32)
    s = m / F32(127.0)
    return np.where(m == 0, F32(1.0), s).astype(F32)


def quantize_weights(w, s_w):
    w = np.asarray(w, dtype=F32)
    return np.clip(np.rint(w / s_w[:, None, None, None]), -127, 127).astype(np.int8)


def quantize_bias(b, s_w, s_in):
    """b_q = rint(b / (s_w * s_in)) in float64 -> int32 (clamped to the int32 range)."""
    v = np.rint(np.asarray(b, dtype=np.float64) / (s_w.astype(np.float64) * np.float64(F32(s_in))))
    return np.clip(v, -2 ** 31, 2 ** 31 - 1).astype(np.int32)


def multiplier(s_w, s_in, s_out):
    """mul[co] = s_w[co] * s_in / s_out: one float32 multiply, then one float32 divide."""
    return ((s_w.astype(F32) * F32(s_in)) / F32(s_out)).astype(F32)


def skip_multiplier(s_in, s_out):
    return F32(F32(s_in) / F32(s_out))


def prepare_conv(w, b, s_in, s_out):
    """-> (w_q int8 [Co,Ci,3,3], b_q int32 [Co], mul float32 [Co])"""
    s_w = weight_scales(w)
    return quantize_weights(w, s_w), quantize_bias(b, s_w, s_in), multiplier(s_w, s_in, s_out)


# ------------------------------------------------------------------------------------------------------- one conv
def conv_acc(x_q, w_q, b_q):
    """int32-exact accumulator of a 3x3 pad-1 conv: b_q[co] + sum x_q * w_q, as float64 matmuls of integers."""
    N, C, H, W = x_q.shape
    Co = w_q.shape[0]
    xp = np.zeros((N, C, H + 2, W + 2), np.float64)
    xp[:, :, 1:-1, 1:-1] = x_q
    acc = np.zeros((N, H, W, Co), np.float64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + H, kx:kx + W].transpose(0, 2, 3, 1)          # N,H,W,C
            acc += win @ w_q[:, :, ky, kx].astype(np.float64).T
    acc += b_q.astype(np.float64)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc.transpose(0, 3, 1, 2).astype(np.int64)                          # N,Co,H,W


def epilogue_float(acc, mul, skip_q=None, skip_mul=None, slope=SLOPE):
    """The float32 value before rounding: float(acc) * mul, LeakyReLU, + float(skip) * skip_mul."""
    t = acc.astype(F32) * mul.astype(F32)[None, :, None, None]
    t = np.where(t >= 0, t, t * F32(slope)).astype(F32)
    if skip_q is not None:
        t = (t + skip_q.astype(F32) * F32(skip_mul)).astype(F32)
    return t


def maxpool2(q):
    N, C, H, W = q.shape
    return q.reshape(N, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def conv3x3(x_q, w_q, b_q, mul, skip_q=None, skip_mul=None, pool=False, slope=SLOPE):
    """One fdet_q8_conv3x3 call on NCHW int8 -> NCHW int8."""
    q = rint_clamp(epilogue_float(conv_acc(x_q, w_q, b_q), mul, skip_q, skip_mul, slope))
    return maxpool2(q) if pool else q


# ------------------------------------------------------------------------------------------------------- block, trunk
def block(h_q, conv1, conv2, skip_mul, pool, slope=SLOPE):
    """conv1 / conv2 = (w_q, b_q, mul).  -> (a_q, h_next_q)"""
    a_q = conv3x3(h_q, *conv1, slope=slope)
    return a_q, conv3x3(a_q, *conv2, skip_q=h_q, skip_mul=skip_mul, pool=pool, slope=slope)


def prepare_trunk(P, s_h, s_a):
    """P: state-dict arrays.  -> list over blocks of (conv1, conv2, skip_mul)."""
    out = []
    for k in range(len(s_a)):
        n = f"residual_blocks.{k}"
        c1 = prepare_conv(np.asarray(P[n + ".conv1.weight"]), np.asarray(P[n + ".conv1.bias"]), s_h[k], s_a[k])
        c2 = prepare_conv(np.asarray(P[n + ".conv2.weight"]), np.asarray(P[n + ".conv2.bias"]), s_a[k], s_h[k + 1])
        out.append((c1, c2, skip_multiplier(s_h[k], s_h[k + 1])))
    return out


def trunk(h0, P, s_h, s_a, S, pool_mult=2):
    """fp32 stem output h0 (N,F,H,W) -> (list of int8 block outputs, fp32 head input).  A block pools iff its map is larger
    than pool_mult * S (PoolResnet)."""
    q = quantize(h0, s_h[0])
    outs = []
    for c1, c2, sm in prepare_trunk(P, s_h, s_a):
        _, q = block(q, c1, c2, sm, pool=q.shape[2] > pool_mult * S)
        outs.append(q)
    return outs, dequantize(q, s_h[-1])


# ------------------------------------------------------------------------------------------------------- literal loops
def conv3x3_loops(x_q, w_q, b_q, mul, skip_q=None, skip_mul=None, pool=False, slope=SLOPE):
    """The contract written out element by element (python ints, one float32 op at a time); for small shapes."""
    N, C, H, W = x_q.shape
    Co = w_q.shape[0]
    q = np.zeros((N, Co, H, W), np.int8)
    xi, wi = x_q.astype(np.int64), w_q.astype(np.int64)
    for n in range(N):
        for co in range(Co):
            for y in range(H):
                for x in range(W):
                    acc = int(b_q[co])
                    for ky in range(3):
                        yy = y + ky - 1
                        if yy < 0 or yy >= H:
                            continue
                        for kx in range(3):
                            xx = x + kx - 1
                            if xx < 0 or xx >= W:
                                continue
                            acc += int(np.dot(xi[n, :, yy, xx], wi[co, :, ky, kx]))
                    t = F32(acc) * F32(mul[co])
                    if not t >= 0:
                        t = F32(t * F32(slope))
                    if skip_q is not None:
                        t = F32(t + F32(F32(int(skip_q[n, co, y, x])) * F32(skip_mul)))
                    q[n, co, y, x] = int(min(max(np.rint(t), -127), 127))
    if pool:
        o = np.zeros((N, Co, H // 2, W // 2), np.int8)
        for y in range(H // 2):
            for x in range(W // 2):
                o[:, :, y, x] = q[:, :, 2 * y:2 * y + 2, 2 * x:2 * x + 2].reshape(N, Co, 4).max(axis=2)
        return o
    return q


# ------------------------------------------------------------------------------------------------------- test cases
# (N, C, H, W), pooled, with skip, tag: the cases of tests/test_gpu_q8.py, reused by the host file for their data conditions
CASES = [
    ((1, 64, 1, 1), False, False, "plain"),
    ((2, 64, 2, 2), True, False, "pooled"),
    ((3, 64, 15, 15), False, False, "plain"),
    ((3, 64, 15, 15), False, True, "skip"),
    ((1, 64, 17, 5), False, False, "plain"),
    ((2, 128, 6, 6), True, True, "pooled+skip"),
    ((1, 64, 30, 30), True, True, "pooled+skip"),
    ((1, 64, 60, 60), True, True, "pooled+skip"),
    ((1, 64, 4, 4), False, False, "ties"),
]


def make_case(idx):
    """Deterministic inputs of CASES[idx]: x, w over the full range -127..127 (both ends present), biases of the size of a
    few products, per-channel multipliers 2^-12 .. 2^-8 (log-uniform; pooled cases 2^-13 .. 2^-9.5; "ties": 0.5 everywhere with
    sparse unit weights, so that accumulators stay small and every odd one sits exactly on .5), skip over the full range with
    skip_mul 0.75."""
    (N, C, H, W), pool, with_skip, tag = CASES[idx]
    rng = np.random.default_rng(1000 + idx)
    x = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8)
    w = rng.integers(-127, 128, (C, C, 3, 3)).astype(np.int8)
    x.reshape(-1)[:2] = (127, -127)
    w.reshape(-1)[:2] = (-127, 127)
    b = rng.integers(-40000, 40001, C).astype(np.int32)
    if tag == "ties":
        # sparse weights of -1 / 0 / 1: |acc| stays within a few hundred, and acc * 0.5 is a tie for every odd acc
        w = (rng.integers(-1, 2, (C, C, 3, 3)) * (rng.random((C, C, 3, 3)) < 0.02)).astype(np.int8)
        b = rng.integers(-9, 10, C).astype(np.int32)
        mul = np.full(C, 0.5, F32)
    else:
        # (a pooled output is the largest of four, so its share at +127 is up to four times the unpooled one's)
        lo, hi = (-13.0, -9.5) if pool else (-12.0, -8.0)
        mul = np.exp2(rng.uniform(lo, hi, C)).astype(F32)
    skip = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8) if with_skip else None
    skip_mul = F32(0.75) if with_skip else None
    return dict(shape=(N, C, H, W), pool=pool, tag=tag, x=x, w=w, b=b, mul=mul, skip=skip, skip_mul=skip_mul)


def pack_weights(w_q):
    """[Co][Ci][3][3] -> the kernels' [tap][Ci/64][Co][64] (include/fdet.h)."""
    Co, Ci = w_q.shape[:2]
    return np.ascontiguousarray(w_q.transpose(2, 3, 1, 0).reshape(9, Ci // 64, 64, Co).transpose(0, 1, 3, 2))
