"""numpy restatement of the on-device augmentation (csrc/fdet_augment.hip) from the same sampled parameters.

Source coordinates and everything after the interpolation are computed in float64; the pixel hash is restated bit-exactly in uint32 arithmetic, so the noise and the glass
offsets are the kernels' own draws.  The box transform is restated in float32 with the kernel's operation order, so the
rounded rows compare exactly.  GlassBlur is restated literally from albumentations 1.1.0's fast mode (the numpy fancy-index
swap), not from the kernel's gather formulation.  The bilinear interpolation itself is restated in float32 with the kernel's
operation order (the kernel's interpolated value is fp32 by specification): scales such as 2000 -> 480 (25/6) put exact .5
ties on the output grid (0.9 % of the values), and a float64 lerp would round those by the last bit of either arithmetic.
Not a test module: tests import it.
"""
import numpy as np

FLIP, ROTATE, BRIGHTNESS, NOISE, GLASS, MOTION = 1, 2, 4, 8, 16, 32
TAG_GLASS = 6
M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def aug_hash(seed, key, tag, y, x):
    """murmur3's finaliser chained over (seed ^ golden ratio, key, tag, y, x); uint32 results (as uint64 arrays)."""
    h = fmix32(np.uint64((int(seed) ^ 0x9E3779B9) & M32))
    h = fmix32(h ^ np.uint64(int(key) & M32))
    h = fmix32(h ^ np.uint64(int(tag) & M32))
    h = fmix32(h ^ (np.asarray(y, dtype=np.uint64) & M32))
    return fmix32(h ^ (np.asarray(x, dtype=np.uint64) & M32))


def normal(seed, key, c, y, x):
    h1 = aug_hash(seed, key, 2 * c, y, x)
    h2 = aug_hash(seed, key, 2 * c + 1, y, x)
    u1 = ((h1 >> 8) + 1).astype(np.float64) * 2.0 ** -24
    u2 = (h2 >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _reflect101f(t, n):
    if n == 1:
        return np.zeros_like(t)
    p = 2.0 * (n - 1)
    t = np.fmod(np.abs(t), p)
    return np.where(t > n - 1, p - t, t)


def warp_values(img, P, Ho, Wo, seed):
    """float64 (3,Ho,Wo) value of the warp kernel before its rint/clamp.  img: (H,W,3) uint8 source."""
    oy, ox = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    f = int(P["flags"])
    u, v = ox.copy(), oy.copy()
    if f & ROTATE:
        c, s = float(P["cos_a"]), float(P["sin_a"])
        dx, dy = ox + 0.5 - Wo / 2.0, oy + 0.5 - Ho / 2.0
        u = _reflect101f(Wo / 2.0 + (c * dx - s * dy) - 0.5, Wo)
        v = _reflect101f(Ho / 2.0 + (s * dx + c * dy) - 0.5, Ho)
    if f & FLIP:
        u = (Wo - 1) - u
    x0c, y0c, cw, ch = int(P["crop_x0"]), int(P["crop_y0"]), int(P["crop_w"]), int(P["crop_h"])
    sx = (u + 0.5) * (cw / Wo) + x0c - 0.5
    sy = (v + 0.5) * (ch / Ho) + y0c - 0.5
    fx0, fy0 = np.floor(sx), np.floor(sy)
    f32 = np.float32
    fx, fy = (sx - fx0).astype(f32), (sy - fy0).astype(f32)
    ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)
    xa, xb = np.clip(ix, x0c, x0c + cw - 1), np.clip(ix + 1, x0c, x0c + cw - 1)
    ya, yb = np.clip(iy, y0c, y0c + ch - 1), np.clip(iy + 1, y0c, y0c + ch - 1)
    src = img.astype(f32)
    out = np.empty((3, Ho, Wo))
    one = f32(1)
    for c_ in range(3):
        s_ = src[:, :, c_]
        top = (one - fx) * s_[ya, xa] + fx * s_[ya, xb]
        bot = (one - fx) * s_[yb, xa] + fx * s_[yb, xb]
        val = (one - fy) * top + fy * bot
        if f & BRIGHTNESS:
            val = val * f32(P["alpha"]) + f32(P["beta"])
        val = val.astype(np.float64)
        if f & NOISE:
            val = val + float(P["sigma"]) * normal(seed, int(P["key"]), c_, oy.astype(np.int64), ox.astype(np.int64))
        out[c_] = val
    return out


def to_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def glass(x0, seed, key):
    """albumentations 1.1.0 glass_blur(mode="fast", max_delta=1, iterations=1) on a (3,H,W) uint8 image without its two
    sigma=0.1 Gaussian blurs (the identity on uint8), with the offsets drawn from the pixel hash."""
    _, H, W = x0.shape
    x = x0.copy()
    if H < 3 or W < 3:
        return x
    hs = np.arange(H - 1, 1, -1)
    ws = np.arange(W - 1, 1, -1)
    h = np.tile(hs, ws.shape[0])
    w = np.repeat(ws, hs.shape[0])
    hh = aug_hash(seed, key, TAG_GLASS, h, w)
    dy = -(hh & 1).astype(np.int64)
    dx = -((hh >> 1) & 1).astype(np.int64)
    x[:, h, w], x[:, h + dy, w + dx] = x[:, h + dy, w + dx], x[:, h, w]
    return x


def motion(x, P):
    """cv2.filter2D with the k x k kernel of P (correlation, reflect-101 border) on (3,H,W) uint8 -> float64."""
    k = int(P["motion_k"])
    wts = np.asarray(P["motion_w"][:k * k], dtype=np.float64).reshape(k, k)
    r = k // 2
    _, H, W = x.shape
    out = np.zeros(x.shape)
    for c in range(3):
        pad = np.pad(x[c].astype(np.float64), r, mode="reflect") if (H > 1 and W > 1) else np.pad(x[c].astype(np.float64), r, mode="edge")
        for dy in range(k):
            for dx in range(k):
                out[c] += wts[dy, dx] * pad[dy:dy + H, dx:dx + W]
    return out


def finish(mid, P, seed):
    """Neighbourhood kernel on the (3,H,W) uint8 intermediate -> final uint8 frame."""
    f = int(P["flags"])
    x = glass(mid, seed, int(P["key"])) if f & GLASS else mid
    return to_u8(motion(x, P)) if f & MOTION else x.copy()


def boxes(rows, P, H, W, Ho, Wo):
    """Box transform of the kernel in float32 with its operation order: (n,5) [conf,x,y,w,h] -> surviving (m,5)."""
    f32 = np.float32
    out = []
    Wf, Hf = f32(W), f32(H)
    for b in np.asarray(rows, dtype=f32).reshape(-1, 5):
        x1 = min(max(b[1], f32(0)), Wf)
        y1 = min(max(b[2], f32(0)), Hf)
        x2 = min(max(f32(b[1] + b[3]), f32(0)), Wf)
        y2 = min(max(f32(b[2] + b[4]), f32(0)), Hf)
        cw, ch = f32(P["crop_w"]), f32(P["crop_h"])
        x1 = min(max(f32(x1 - f32(P["crop_x0"])), f32(0)), cw)
        x2 = min(max(f32(x2 - f32(P["crop_x0"])), f32(0)), cw)
        y1 = min(max(f32(y1 - f32(P["crop_y0"])), f32(0)), ch)
        y2 = min(max(f32(y2 - f32(P["crop_y0"])), f32(0)), ch)
        sxs, sys_ = f32(f32(Wo) / cw), f32(f32(Ho) / ch)
        x1, x2, y1, y2 = f32(x1 * sxs), f32(x2 * sxs), f32(y1 * sys_), f32(y2 * sys_)
        if int(P["flags"]) & FLIP:
            x1, x2 = f32(f32(Wo) - x2), f32(f32(Wo) - x1)
        if int(P["flags"]) & ROTATE:
            cx, cy, c, s = f32(0.5) * f32(Wo), f32(0.5) * f32(Ho), f32(P["cos_a"]), f32(P["sin_a"])
            rx, ry = [], []
            for px, py in ((x1, y1), (x2, y1), (x1, y2), (x2, y2)):
                dx, dy = f32(px - cx), f32(py - cy)
                rx.append(f32(f32(f32(c * dx) + f32(s * dy)) + cx))
                ry.append(f32(f32(f32(c * dy) - f32(s * dx)) + cy))
            x1 = min(max(min(rx), f32(0)), f32(Wo))
            x2 = min(max(max(rx), f32(0)), f32(Wo))
            y1 = min(max(min(ry), f32(0)), f32(Ho))
            y2 = min(max(max(ry), f32(0)), f32(Ho))
        w, h = f32(x2 - x1), f32(y2 - y1)
        if not (w > 0) or not (h > 0) or f32(w * h) < f32(10):
            continue
        out.append([1.0, np.rint(x1), np.rint(y1), np.rint(w), np.rint(h)])
    return np.asarray(out, dtype=f32).reshape(-1, 5)


def augment(images, boxes_list, P_batch, Ho, Wo, seed):
    """Whole pipeline for a batch: (frames (B,3,Ho,Wo) uint8, warp values (B,3,Ho,Wo) float64, rows (total,5), box_offset)."""
    frames, vals, rows, offs = [], [], [], [0]
    for P in P_batch:
        img = images[int(P["image"])]
        v = warp_values(img, P, Ho, Wo, seed)
        vals.append(v)
        frames.append(finish(to_u8(v), P, seed))
        r = boxes(boxes_list[int(P["image"])], P, img.shape[0], img.shape[1], Ho, Wo)
        rows.append(r)
        offs.append(offs[-1] + len(r))
    return (np.stack(frames), np.stack(vals), np.concatenate(rows, 0) if rows else np.zeros((0, 5), np.float32),
            np.asarray(offs, dtype=np.int32))
