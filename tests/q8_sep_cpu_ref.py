"""numpy restatement of the int8 separable block (include/fdet.h, "Int8 inference: the separable block"), on top of
the primitives of tests/q8_cpu_ref.py.

Written from the contract, not from the kernel: integers stay exact (the pointwise GEMMs run as float64 matmuls of integer
values, |acc| < 2^53; the depthwise sum in int64), every float step is ONE float32 operation with one rounding, rounding is
numpy's rint (half to even).  Feature maps are plain NCHW; pointwise weights [Co][Ci], depthwise weights [C][3][3]."""
import numpy as np
import torch
import torch.nn.functional as Fn

from q8_cpu_ref import F32, SLOPE, dequantize, maxpool2, multiplier, rint_clamp, skip_multiplier, weight_scales

import q8_pool_stem_cpu_ref as RP


# ------------------------------------------------------------------------------------------------------- preparation
def prepare_weights(w, s_in, s_out):
    """One conv without a bias: (w_q int8 of w's shape, mul float32 [Co]).  s_w per output channel (absmax / 127, 1 for a
    channel of zeros), w_q = clamp(rint(w / s_w)), mul = (s_w * s_in) / s_out."""
    w = np.asarray(w, dtype=F32)
    s_w = weight_scales(w)
    w_q = np.clip(np.rint(w / s_w.reshape((-1,) + (1,) * (w.ndim - 1))), -127, 127).astype(np.int8)
    return w_q, multiplier(s_w, s_in, s_out)


def prepare_block(w1, wd, w2, s_in, s_a, s_b, s_out):
    """w1, w2 [C,C,1,1], wd [C,1,3,3] float -> dict(w1 [C,C], mul1, wd [C,3,3], mul2, w2 [C,C], mul3, skip_mul)."""
    C = np.asarray(w1).shape[0]
    w1_q, mul1 = prepare_weights(np.asarray(w1).reshape(C, C), s_in, s_a)
    wd_q, mul2 = prepare_weights(np.asarray(wd).reshape(C, 3, 3), s_a, s_b)
    w2_q, mul3 = prepare_weights(np.asarray(w2).reshape(C, C), s_b, s_out)
    return dict(w1=w1_q, mul1=mul1, wd=wd_q, mul2=mul2, w2=w2_q, mul3=mul3, skip_mul=skip_multiplier(s_in, s_out))


# ------------------------------------------------------------------------------------------------------- the block
def lrelu(t, slope=SLOPE):
    return np.where(t >= 0, t, t * F32(slope)).astype(F32)


def pointwise_acc(x_q, w_q):
    """acc[n][co][y][x] = sum_ci x_q[n][ci][y][x] * w_q[co][ci], exact."""
    acc = np.einsum("oc,nchw->nohw", w_q.astype(np.float64), x_q.astype(np.float64))
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return np.rint(acc).astype(np.int64)


def depthwise_acc(a_q, wd_q):
    """acc[n][c][y][x] = sum_{ky,kx} a_q[n][c][y+ky-1][x+kx-1] * wd_q[c][ky][kx]; a_q outside the image is 0."""
    N, C, H, W = a_q.shape
    ap = np.zeros((N, C, H + 2, W + 2), np.int64)
    ap[:, :, 1:-1, 1:-1] = a_q
    acc = np.zeros((N, C, H, W), np.int64)
    for ky in range(3):
        for kx in range(3):
            acc += ap[:, :, ky:ky + H, kx:kx + W] * wd_q[:, ky, kx].astype(np.int64)[None, :, None, None]
    return acc


def sepblock_parts(h_q, p, pool=False, slope=SLOPE):
    """-> (a_q, b_q, the float32 values before each of the three roundings, y)"""
    per_ch = (None, slice(None), None, None)
    t1 = lrelu(pointwise_acc(h_q, p["w1"]).astype(F32) * p["mul1"].astype(F32)[per_ch], slope)
    a_q = rint_clamp(t1)
    t2 = lrelu(depthwise_acc(a_q, p["wd"]).astype(F32) * p["mul2"].astype(F32)[per_ch], slope)
    b_q = rint_clamp(t2)
    m = (pointwise_acc(b_q, p["w2"]).astype(F32) * p["mul3"].astype(F32)[per_ch]).astype(F32)
    s = (h_q.astype(F32) * F32(p["skip_mul"])).astype(F32)
    t3 = (m + s).astype(F32)
    q = rint_clamp(t3)
    return a_q, b_q, (t1, t2, t3), (maxpool2(q) if pool else q)


def sepblock(h_q, p, pool=False, slope=SLOPE):
    """One fdet_q8_sepblock call on NCHW int8 -> NCHW int8."""
    return sepblock_parts(h_q, p, pool, slope)[3]


def sepchain(h_q, blocks, slope=SLOPE):
    """-> the list of every block's output (un-pooled)."""
    outs = []
    for p in blocks:
        h_q = sepblock(h_q, p, False, slope)
        outs.append(h_q)
    return outs


# ------------------------------------------------------------------------------------------------------- literal loops
def _rq(t):
    return int(min(max(np.rint(t), -127), 127))


def _lrelu1(t, slope):
    return t if t >= 0 else F32(t * F32(slope))


def sepblock_loops(h_q, p, pool=False, slope=SLOPE):
    """The contract element by element (python ints, one float32 op at a time); for small shapes."""
    N, C, H, W = h_q.shape
    hi = h_q.astype(np.int64)
    w1, wd, w2 = (p[k].astype(np.int64) for k in ("w1", "wd", "w2"))
    a = np.zeros((N, C, H, W), np.int64)
    b = np.zeros((N, C, H, W), np.int64)
    q = np.zeros((N, C, H, W), np.int8)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                for co in range(C):
                    acc = int(np.dot(hi[n, :, y, x], w1[co]))
                    a[n, co, y, x] = _rq(_lrelu1(F32(F32(acc) * F32(p["mul1"][co])), slope))
        for c in range(C):
            for y in range(H):
                for x in range(W):
                    acc = 0
                    for ky in range(3):
                        for kx in range(3):
                            yy, xx = y + ky - 1, x + kx - 1
                            if 0 <= yy < H and 0 <= xx < W:
                                acc += int(a[n, c, yy, xx]) * int(wd[c, ky, kx])
                    b[n, c, y, x] = _rq(_lrelu1(F32(F32(acc) * F32(p["mul2"][c])), slope))
        for y in range(H):
            for x in range(W):
                for co in range(C):
                    acc = int(np.dot(b[n, :, y, x], w2[co]))
                    m = F32(F32(acc) * F32(p["mul3"][co]))
                    s = F32(F32(int(h_q[n, co, y, x])) * F32(p["skip_mul"]))
                    q[n, co, y, x] = _rq(F32(m + s))
    if pool:
        o = np.zeros((N, C, H // 2, W // 2), np.int8)
        for y in range(H // 2):
            for x in range(W // 2):
                o[:, :, y, x] = q[:, :, 2 * y:2 * y + 2, 2 * x:2 * x + 2].reshape(N, C, 4).max(axis=2)
        return o
    return q


# ------------------------------------------------------------------------------------------------------- test cases
# (N, C, H, W), pooled, forced tile (rows, columns) or (0, 0), tag: the cases of tests/test_gpu_q8_sep.py
CASES = [
    ((1, 64, 1, 1), False, (0, 0), "plain"),
    ((2, 64, 2, 2), True, (0, 0), "pooled"),
    ((3, 64, 15, 15), False, (0, 0), "plain"),
    ((1, 64, 16, 16), False, (0, 0), "plain"),
    ((1, 64, 17, 5), False, (0, 0), "plain"),
    ((2, 128, 6, 6), True, (0, 0), "pooled"),
    ((1, 64, 6, 6), True, (2, 2), "pooled"),
    ((1, 64, 6, 6), True, (4, 6), "pooled"),
    ((1, 64, 12, 10), False, (4, 4), "plain"),
    ((1, 64, 30, 30), True, (0, 0), "pooled"),
    ((1, 64, 60, 60), True, (0, 0), "pooled"),
    ((1, 128, 60, 60), True, (0, 0), "pooled"),
    ((1, 64, 64, 64), True, (0, 0), "pooled"),
    ((1, 64, 4, 4), False, (0, 0), "ties"),
]
CASE_IDS = ["x".join(map(str, c[0])) + ("p" if c[1] else "") + (f"-t{c[2][0]}x{c[2][1]}" if c[2][0] else "") +
            ("-ties" if c[3] == "ties" else "") for c in CASES]
SKIP_MUL = F32(0.75)

# log2 ranges of the three per-channel multipliers (log-uniform).  A pointwise accumulator of C products of codes uniform in
# -127..127 has a standard deviation of 5376 sqrt(C) (43,000 at C = 64); the ranges put a_q, b_q and y at a standard
# deviation of a few tens of codes, so that a few percent of each saturate (tests/test_q8_sep_host.py asserts over 0 and under
# 10 % per case); the pooled cases sit lower at the last stage, since a pooled output is the largest of four.
MUL_LOG2 = {64: ((-10.1, -8.1), (-8.5, -6.5), (-10.7, -8.7)), 128: ((-10.6, -8.6), (-8.5, -6.5), (-11.2, -9.2))}
POOL_SHIFT = -0.8


def random_params(rng, C, pool=False):
    (l1, h1), (l2, h2), (l3, h3) = MUL_LOG2[C]
    sh = POOL_SHIFT if pool else 0.0
    p = dict(w1=rng.integers(-127, 128, (C, C)).astype(np.int8), wd=rng.integers(-127, 128, (C, 3, 3)).astype(np.int8),
             w2=rng.integers(-127, 128, (C, C)).astype(np.int8),
             mul1=np.exp2(rng.uniform(l1, h1, C)).astype(F32), mul2=np.exp2(rng.uniform(l2, h2, C)).astype(F32),
             mul3=np.exp2(rng.uniform(l3 + sh, h3 + sh, C)).astype(F32), skip_mul=SKIP_MUL)
    for k in ("w1", "wd", "w2"):
        p[k].reshape(-1)[:2] = (-127, 127)
    return p


def make_case(idx):
    """Deterministic inputs of CASES[idx]: x and the weights over the full range -127..127 (both ends present), multipliers
    log-uniform in MUL_LOG2, skip_mul 0.75.  "ties": multipliers 0.5 with sparse weights of -1 / 0 / 1, so that every odd
    accumulator sits exactly on .5 at the first two roundings, and acc3 * 0.5 + h * 0.75 on .5 for a quarter of the rest."""
    (N, C, H, W), pool, tile, tag = CASES[idx]
    rng = np.random.default_rng(1900 + idx)
    x = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8)
    x.reshape(-1)[:2] = (127, -127)
    if tag == "ties":
        def sparse(shape, density):
            return (rng.integers(-1, 2, shape) * (rng.random(shape) < density)).astype(np.int8)
        half = np.full(C, 0.5, F32)
        p = dict(w1=sparse((C, C), 0.03), wd=sparse((C, 3, 3), 0.4), w2=sparse((C, C), 0.06), mul1=half, mul2=half.copy(),
                 mul3=half.copy(), skip_mul=SKIP_MUL)
    else:
        p = random_params(rng, C, pool)
    return dict(shape=(N, C, H, W), pool=pool, tile=tile, tag=tag, x=x, p=p, slope=SLOPE)


def make_onehot_case(tap):
    """(1,64,3,3): depthwise weights one-hot on tap `tap` (value 1, multiplier 1), w1 = w2 = identity * 127 with multipliers
    1 / 127, slope 1, skip_mul 0: the block shifts its input by the tap, value for value."""
    C = 64
    x = np.random.default_rng(1950).integers(-127, 128, (1, C, 3, 3)).astype(np.int8)
    eye = (np.eye(C) * 127).astype(np.int8)
    wd = np.zeros((C, 3, 3), np.int8)
    wd[:, tap // 3, tap % 3] = 1
    inv = np.full(C, F32(1.0) / F32(127.0), F32)
    p = dict(w1=eye, wd=wd, w2=eye.copy(), mul1=inv, mul2=np.ones(C, F32), mul3=inv.copy(), skip_mul=F32(0.0))
    return dict(shape=(1, C, 3, 3), pool=False, tile=(0, 0), tag="onehot", x=x, p=p, slope=F32(1.0))


def shifted(x, tap):
    """x read through tap (ky, kx) of a 3x3 pad-1 window."""
    N, C, H, W = x.shape
    xp = np.zeros((N, C, H + 2, W + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    return xp[:, :, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W]


# (nblocks, N, H, W) of the chain tests
CHAIN_CASES = [(1, 2, 15, 15), (2, 2, 15, 15), (8, 3, 15, 15), (1, 1, 16, 16), (2, 2, 16, 16), (8, 2, 16, 16), (3, 2, 1, 1), (3, 2, 10, 10)]
CHAIN_IDS = [f"{nb}blocks-{n}x{h}x{w}" for nb, n, h, w in CHAIN_CASES]


def make_chain_case(idx):
    nb, N, H, W = CHAIN_CASES[idx]
    rng = np.random.default_rng(1970 + idx)
    x = rng.integers(-127, 128, (N, 64, H, W)).astype(np.int8)
    x.reshape(-1)[:2] = (127, -127)
    return dict(shape=(N, 64, H, W), x=x, blocks=[random_params(rng, 64) for _ in range(nb)], slope=SLOPE)


def pack_dw(wd_q):
    """[C][3][3] -> the kernel's [9][C] (include/fdet.h)."""
    return np.ascontiguousarray(wd_q.reshape(wd_q.shape[0], 9).T)


def saturation(q):
    return float(np.mean(np.abs(q.astype(np.int32)) == 127))


# ------------------------------------------------------------------------------------------------------- the model
POOL_ABOVE = 16                                            # models/SeparableCNN.py: a block pools iff its map is larger than 16


def block_names(k):
    n = f"residual_blocks.{k}."
    return n + "pointwise_conv1.weight", n + "depthwise_conv.weight", n + "pointwise_conv2.weight"


def num_blocks(P):
    return sum(1 for k in P if k.endswith(".depthwise_conv.weight"))


def float_forward(P, frames_u8, head_pad):
    """The float oracle (tests/sepcnn_cpu_ref.py's arithmetic, plain torch fp32 on the CPU) with its intermediates:
    -> (hs: nb + 1 block inputs, as_, bs, y)."""
    import sepcnn_cpu_ref as SR
    T = {k: torch.from_numpy(np.asarray(v)) for k, v in P.items()}
    x = torch.from_numpy(frames_u8).float() / 255.0
    with torch.no_grad():
        h = Fn.conv2d(x, T["conv1.weight"], T["conv1.bias"], stride=8, padding=2)
        hs, as_, bs = [], [], []
        for k in range(num_blocks(P)):
            n1, nd, n2 = block_names(k)
            hs.append(h)
            a, b, _, h = SR.block_parts(h, T[n1], T[nd], T[n2], None, pool=h.shape[2] > POOL_ABOVE)
            as_.append(a)
            bs.append(b)
        hs.append(h)
        y = torch.sigmoid(Fn.conv2d(h, T["out.weight"], T["out.bias"], padding=head_pad))
    return hs, as_, bs, y


def absmax_scales(hs, as_, bs):
    def scale(t):
        v = float(t.abs().max())
        return F32(1.0) if v == 0.0 else F32(v) / F32(127.0)
    return [scale(t) for t in hs], [scale(t) for t in as_], [scale(t) for t in bs]


def model_q(frames_u8, P, s_h, s_a, s_b, head_pad=0):
    """frames -> (int8 stem output, block outputs, fp32 head input, y): the integer stem of tests/q8_pool_stem_cpu_ref.py, the
    restatement blocks, the torch fp32 head."""
    P = {k: np.asarray(v) for k, v in P.items()}
    q0 = RP.stem10(frames_u8, P["conv1.weight"], P["conv1.bias"], s_h[0])
    q, outs = q0, []
    for k in range(num_blocks(P)):
        n1, nd, n2 = block_names(k)
        p = prepare_block(P[n1], P[nd], P[n2], s_h[k], s_a[k], s_b[k], s_h[k + 1])
        q = sepblock(q, p, pool=q.shape[2] > POOL_ABOVE)
        outs.append(q)
    hd = dequantize(q, s_h[-1])
    with torch.no_grad():
        y = torch.sigmoid(Fn.conv2d(torch.from_numpy(hd), torch.from_numpy(P["out.weight"]), torch.from_numpy(P["out.bias"]),
                                    padding=head_pad))
    return q0, outs, hd, y


# The accuracy models: seeded random SeparableCNN(filters=64), three seeded uint8 frames each.
# (seed, input size, SeparableCNN keywords)
ACCURACY_MODELS = [(190, 480, dict(output_padding=3)), (191, 512, dict(output_kernel_size=1))]
# max and mean |y_int8 - y_float| over the maps of the three frames, recorded from tests/test_q8_sep_host.py on the CPU
ACCURACY_RECORDED = [(0.006638, 0.001133), (0.005476, 0.001073)]


def accuracy_model(i):
    """-> (model on the CPU in eval mode, P as numpy, frames uint8 (3,3,size,size), head padding)"""
    from fdet_amd.models.SeparableCNN import SeparableCNN
    seed, size, kw = ACCURACY_MODELS[i]
    torch.manual_seed(seed)
    model = SeparableCNN(filters=64, input_shape=(3, size, size), **kw).eval()
    frames = torch.randint(0, 256, (3, 3, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed + 1000))
    P = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    return model, P, frames.numpy(), int(kw.get("output_padding", 0))
