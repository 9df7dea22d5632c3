"""numpy restatement of Int8SSD's arithmetic (include/fdet.h, "Int8 inference: mixed widths"), on top of
tests/q8_cpu_ref.py and tests/q8_resnet_cpu_ref.py.

Written from the contract, not from the kernels: the Cin != Cout 3x3 conv with the floor pool, the 1x1 skip conv, the
Linear(C,5) head, the F = 16 stem (q8_resnet_cpu_ref.stem3_q takes any F), the block and the whole SSD(16).  Integers stay
exact (float64 convs / matmuls of integer values, |acc| < 2^53), every float step is ONE float32 operation, rounding is
numpy's rint.  Feature maps are plain NCHW here."""
import numpy as np
import torch
import torch.nn.functional as F

import q8_cpu_ref as R
import q8_resnet_cpu_ref as RR

F32 = np.float32
S_IN = RR.S_IN
PATCH_SIZES = (60, 30, 15, 7)


def block_specs(f=16):
    """(name, cin, cout, pooled, head index or -1) of the thirteen blocks of the reference's SSD (models/SSD.py)."""
    fe = [(f, 2 * f, True), (2 * f, 2 * f, True)] + [(2 * f, 2 * f, False)] * 6 + [(2 * f, 4 * f, False)]
    specs = [(f"feature_extractor.{k}", i, o, p, -1) for k, (i, o, p) in enumerate(fe)]
    for i in range(4):
        cin = min(4 * f * 2 ** i, 16 * f)
        specs.append((f"continue_layers.{i}.0", cin, min(2 * cin, 16 * f), i != 0, i))
    return specs


# ------------------------------------------------------------------------------------------------------- one layer
def maxpool2_floor(q):
    """2x2 max over the windows that lie inside the map: H/2 x W/2 by integer division, an odd last row / column is dropped."""
    H, W = q.shape[2], q.shape[3]
    return R.maxpool2(q[:, :, :H // 2 * 2, :W // 2 * 2])


def conv3x3(x_q, w_q, b_q, mul, skip_q=None, skip_mul=None, pool=False, slope=R.SLOPE):
    """One fdet_q8x_conv3x3 call, Cin -> Cout, on NCHW int8 -> NCHW int8 (skip_q has Cout channels)."""
    q = R.rint_clamp(R.epilogue_float(RR.conv_acc(x_q, w_q, b_q), mul, skip_q, skip_mul, slope))
    return maxpool2_floor(q) if pool else q


def pointwise_acc(x_q, w_q, b_q):
    """b_q[co] + sum_ci x_q[ci] * w_q[co][ci] as a float64 matmul of integers -> int64 (N,Co,H,W)."""
    w = np.asarray(w_q).reshape(w_q.shape[0], -1).astype(np.float64)
    acc = np.einsum("nchw,oc->nohw", x_q.astype(np.float64), w) + np.asarray(b_q, np.float64)[None, :, None, None]
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return np.rint(acc).astype(np.int64)


def pointwise(x_q, w_q, b_q, mul):
    """fdet_q8x_pointwise: q = clamp(rint(float(acc) * mul[co])), identity activation."""
    return R.rint_clamp(pointwise_acc(x_q, w_q, b_q).astype(F32) * np.asarray(mul, F32)[None, :, None, None])


def head(h_q, w_q, b_q, m):
    """fdet_q8x_head_f32: z = float(b_q[o] + sum_c h_q[c] * w_q[o][c]) * m[o] -> float32 (N,5,H,W)."""
    return (pointwise_acc(h_q, w_q, b_q).astype(F32) * np.asarray(m, F32)[None, :, None, None]).astype(F32)


def prepare_head(w, b, s_in):
    """(w_q int8 [5,C], b_q int32 [5], m float32 [5]): s_w per output row, b_q = rint(b / (s_w * s_in)) in float64,
    m = s_w * s_in as one float32 multiply."""
    w = np.asarray(w, F32)
    s_w = R.weight_scales(w)
    w_q = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    return w_q, R.quantize_bias(b, s_w, s_in), (s_w * F32(s_in)).astype(F32)


# ------------------------------------------------------------------------------------------------------- literal loops
def conv3x3_loops(x_q, w_q, b_q, mul, skip_q=None, skip_mul=None, pool=False, slope=R.SLOPE):
    """The contract element by element (python ints, one float32 op at a time), Cin -> Cout, floor pool; for tiny shapes."""
    N, _, H, W = x_q.shape
    Co = w_q.shape[0]
    q = np.zeros((N, Co, H, W), np.int8)
    xi, wi = x_q.astype(np.int64), w_q.astype(np.int64)
    for n in range(N):
        for co in range(Co):
            for y in range(H):
                for x in range(W):
                    acc = int(b_q[co])
                    for ky in range(3):
                        for kx in range(3):
                            yy, xx = y + ky - 1, x + kx - 1
                            if 0 <= yy < H and 0 <= xx < W:
                                for ci in range(xi.shape[1]):
                                    acc += int(xi[n, ci, yy, xx]) * int(wi[co, ci, ky, kx])
                    t = F32(acc) * F32(mul[co])
                    if not t >= 0:
                        t = F32(t * F32(slope))
                    if skip_q is not None:
                        t = F32(t + F32(F32(int(skip_q[n, co, y, x])) * F32(skip_mul)))
                    q[n, co, y, x] = int(min(max(np.rint(t), -127), 127))
    if not pool:
        return q
    o = np.zeros((N, Co, H // 2, W // 2), np.int8)
    for y in range(H // 2):
        for x in range(W // 2):
            for n in range(N):
                for co in range(Co):
                    o[n, co, y, x] = max(int(q[n, co, 2 * y, 2 * x]), int(q[n, co, 2 * y, 2 * x + 1]), int(q[n, co, 2 * y + 1, 2 * x]),
                                         int(q[n, co, 2 * y + 1, 2 * x + 1]))
    return o


def pointwise_loops(x_q, w_q, b_q, mul):
    N, Ci, H, W = x_q.shape
    Co = w_q.shape[0]
    q = np.zeros((N, Co, H, W), np.int8)
    w2 = np.asarray(w_q).reshape(Co, Ci)
    for n in range(N):
        for co in range(Co):
            for y in range(H):
                for x in range(W):
                    acc = int(b_q[co])
                    for ci in range(Ci):
                        acc += int(x_q[n, ci, y, x]) * int(w2[co, ci])
                    q[n, co, y, x] = int(min(max(np.rint(F32(acc) * F32(mul[co])), -127), 127))
    return q


def head_loops(h_q, w_q, b_q, m):
    N, C, H, W = h_q.shape
    z = np.zeros((N, 5, H, W), F32)
    for n in range(N):
        for o in range(5):
            for y in range(H):
                for x in range(W):
                    acc = int(b_q[o])
                    for c in range(C):
                        acc += int(h_q[n, c, y, x]) * int(w_q[o, c])
                    z[n, o, y, x] = F32(acc) * F32(m[o])
    return z


# ------------------------------------------------------------------------------------------------------- packing
def pack_weights(w_q):
    """[Co][Ci][kh][kw] (3x3 or 1x1) -> the kernels' [K/64][Co][64]: k = tap * Ci + ci, K zero-padded to a multiple of 64."""
    Co, Ci, kh, kw = w_q.shape
    K = Ci * kh * kw
    KP = (K + 63) // 64 * 64
    flat = np.zeros((Co, KP), np.int8)
    for co in range(Co):
        for ky in range(kh):
            for kx in range(kw):
                for ci in range(Ci):
                    flat[co, (ky * kw + kx) * Ci + ci] = w_q[co, ci, ky, kx]
    return np.ascontiguousarray(flat.reshape(Co, KP // 64, 64).transpose(1, 0, 2))


def unpack_weights(wpk, Co, Ci, taps):
    """The inverse permutation: ([K/64][Co][64] flat) -> ([Co][Ci][kh][kw], the pad bytes)."""
    K = taps * Ci
    KP = (K + 63) // 64 * 64
    flat = np.asarray(wpk).reshape(KP // 64, Co, 64).transpose(1, 0, 2).reshape(Co, KP)
    side = 3 if taps == 9 else 1
    return np.ascontiguousarray(flat[:, :K].reshape(Co, side, side, Ci).transpose(0, 3, 1, 2)), flat[:, K:]


# ------------------------------------------------------------------------------------------------------- block, model
def block(h_q, conv1, conv2, skip_conv, skip_mul, pool):
    """conv1 / conv2 / skip_conv = (w_q, b_q, mul); skip_conv is None for a block that keeps its width.
    -> (skip_q, a_q, h_next_q)"""
    sk = h_q if skip_conv is None else pointwise(h_q, *skip_conv)
    a = conv3x3(h_q, *conv1)
    return sk, a, conv3x3(a, *conv2, skip_q=sk, skip_mul=skip_mul, pool=pool)


def prepare_model(P, s_h, s_a, s_k):
    """P: state-dict arrays of an SSD(16).  -> (stem, [(conv1, conv2, skip_conv, skip_mul, pooled, head)], {head: (w_q, b_q, m)})"""
    P = {k: np.asarray(v) for k, v in P.items()}
    stem = R.prepare_conv(P["input_normalizer.weight"], P["input_normalizer.bias"], S_IN, s_h[0])
    blocks, heads, j = [], {}, 0
    for k, (name, ci, co, pool, hd) in enumerate(block_specs(16)):
        c1 = R.prepare_conv(P[name + ".conv1.weight"], P[name + ".conv1.bias"], s_h[k], s_a[k])
        c2 = R.prepare_conv(P[name + ".conv2.weight"], P[name + ".conv2.bias"], s_a[k], s_h[k + 1])
        if ci != co:
            cs = R.prepare_conv(P[name + ".pointwise_conv_skip.weight"], P[name + ".pointwise_conv_skip.bias"], s_h[k], s_k[j])
            sm = R.skip_multiplier(s_k[j], s_h[k + 1])
            j += 1
        else:
            cs, sm = None, R.skip_multiplier(s_h[k], s_h[k + 1])
        blocks.append((c1, c2, cs, sm, pool, hd))
        if hd >= 0:
            hn = f"extracting_layers.{hd}.0"
            heads[hd] = prepare_head(P[hn + ".weight"], P[hn + ".bias"], s_h[k + 1])
    assert j == len(s_k)
    return stem, blocks, heads


def model_q(frames_u8, P, s_h, s_a, s_k):
    """uint8 frames (N,3,480,480) -> (int8 stem output, [int8 block outputs], [float32 z (N,5,ps,ps) of the four heads])."""
    stem, blocks, heads = prepare_model(P, s_h, s_a, s_k)
    q0 = RR.stem3_q(frames_u8, *stem)
    h, outs, zs = q0, [], []
    for c1, c2, cs, sm, pool, hd in blocks:
        _, _, h = block(h, c1, c2, cs, sm, pool)
        outs.append(h)
        if hd >= 0:
            zs.append(head(h, *heads[hd]))
    return q0, outs, zs


def rows(zs):
    """[z (N,5,ps,ps)] -> (N,4774,5): position-major rows per head, heads in order (what the head pack reads; raw z, no
    sigmoid, no priors)."""
    return np.concatenate([z.transpose(0, 2, 3, 1).reshape(z.shape[0], -1, 5) for z in zs], axis=1)


# ------------------------------------------------------------------------------------------------------- float model
def float_model(P, x):
    """torch fp32 ops on the CPU, eval arithmetic (no dropout): -> (block inputs h_0..h_13 (h_13 is the last head's input),
    first-conv outputs a_k, skip-conv outputs of the blocks whose width changes, [z (N,5,ps,ps)])."""
    P = {k: torch.as_tensor(np.asarray(v)) for k, v in P.items()}
    with torch.no_grad():
        h = F.conv2d(x, P["input_normalizer.weight"], P["input_normalizer.bias"], stride=2, padding=1)
        hs, as_, ks, zs = [], [], [], []
        for name, ci, co, pool, hd in block_specs(16):
            hs.append(h)
            sk = h
            if ci != co:
                sk = F.conv2d(h, P[name + ".pointwise_conv_skip.weight"], P[name + ".pointwise_conv_skip.bias"])
                ks.append(sk)
            a = F.leaky_relu(F.conv2d(h, P[name + ".conv1.weight"], P[name + ".conv1.bias"], padding=1), 0.2)
            as_.append(a)
            e = F.leaky_relu(F.conv2d(a, P[name + ".conv2.weight"], P[name + ".conv2.bias"], padding=1), 0.2) + sk
            h = F.max_pool2d(e, 2) if pool else e
            if hd >= 0:
                hn = f"extracting_layers.{hd}.0"
                zs.append(F.conv2d(h, P[hn + ".weight"][:, :, None, None], P[hn + ".bias"]))
        hs.append(h)
    return hs, as_, ks, zs


def absmax_scales(ts):
    def scale(t):
        v = float(t.abs().max())
        return F32(1.0) if v == 0.0 else F32(v) / F32(127.0)
    return np.array([scale(t) for t in ts], F32)


def seeded_ssd(seed=20):
    """The seeded random SSD(16) of the tests and two uint8 frames: smooth random images (a low-resolution random field
    resized up), so that the activations are not those of white noise."""
    import fdet_amd  # noqa: F401
    from fdet_amd.models.SSD import SSD
    torch.manual_seed(seed)
    model = SSD(16, (3, 480, 480))
    g = torch.Generator().manual_seed(seed + 1)
    low = torch.rand(2, 3, 30, 30, generator=g)
    frames = F.interpolate(low, size=(480, 480), mode="bilinear", align_corners=False).mul(255.0).round().clamp(0, 255).to(torch.uint8)
    return model, frames


def quant_error(zs_q, zs_f):
    """(max |dz|, mean |dz|, max |dscore|, mean |dscore|) of the heads' outputs; score = sigmoid(z[:, 0])."""
    a, b = rows([np.asarray(z) for z in zs_q]), rows([np.asarray(z) for z in zs_f])
    dz = np.abs(a.astype(np.float64) - b)
    sa, sb = 1.0 / (1.0 + np.exp(-a[..., 0].astype(np.float64))), 1.0 / (1.0 + np.exp(-b[..., 0].astype(np.float64)))
    ds = np.abs(sa - sb)
    return float(dz.max()), float(dz.mean()), float(ds.max()), float(ds.mean())
