"""numpy restatement of the device half of the JPEG decoder (csrc/fdet_jpeg.hip fdet_jpeg_reconstruct): quantised coefficient
planes and dequantisation tables in, RGB out.  Whole-plane array operations in int64, written from libjpeg's sources
(jidctint.c jpeg_idct_islow, jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample, jdcolor.c ycc_rgb_convert), not from the
kernel: no lanes, no 16-byte words, no per-pixel function.  tests/test_jpeg_host.py shows that it reproduces PIL's decode of
every fixture byte for byte, so the zero-difference bound of the GPU tests is reachable."""

import numpy as np


def _idct_pass(d, shift):
    """One 8-point pass of jpeg_idct_islow over the LAST axis of d (int64), descaled by `shift` bits."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    z1 = (d2 + d6) * 4433
    t2 = z1 - d6 * 15137
    t3 = z1 + d2 * 6270
    t0 = (d0 + d4) * 8192
    t1 = (d0 - d4) * 8192
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = d7 + d1, d5 + d3, d7 + d3, d5 + d1
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = d7 * 2446, d5 * 16819, d3 * 25172, d1 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def _range_limit(v):
    """The post-IDCT limit table indexed with v & 1023 (level shift included)."""
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def idct_plane(coef, qt):
    """coef [bh,bw,64] int16 (natural order), qt [64] -> uint8-valued samples [bh*8, bw*8] (int64)."""
    bh, bw, _ = coef.shape
    d = coef.astype(np.int64).reshape(bh, bw, 8, 8) * np.asarray(qt, dtype=np.int64).reshape(8, 8)
    cols = _idct_pass(np.swapaxes(d, 2, 3), 11)          # [.., column, vertical frequency] -> [.., column, row]
    rows = _idct_pass(np.swapaxes(cols, 2, 3), 18)       # [.., row, horizontal frequency] -> [.., row, column]
    return _range_limit(rows).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h_fancy(s, dw, wide):
    """Triangle filter along the last axis over the first dw columns of s: `wide` False is h2v1 (s = samples, >> 2), True is
    h2v2 (s = 3 * near + far column sums, >> 4).  Neighbours clamp to 0..dw-1."""
    s = s[..., :dw]
    left = np.concatenate([s[..., :1], s[..., :-1]], axis=-1)
    right = np.concatenate([s[..., 1:], s[..., -1:]], axis=-1)
    if wide:
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    else:
        even, odd = (3 * s + left + 1) >> 2, (3 * s + right + 2) >> 2
    return np.stack([even, odd], axis=-1).reshape(*s.shape[:-1], 2 * dw)


def upsample(plane, width, height, hs, vs):
    """A chroma sample plane (padding included) -> at least height x width full-resolution samples."""
    if hs == 1 and vs == 1:
        return plane
    dw, dh = -(-width // hs), -(-height // vs)
    if dw <= 2:                                          # the library replicates when there is nothing to filter
        return np.repeat(np.repeat(plane, vs, axis=0), hs, axis=1)
    if vs == 1:
        return _h_fancy(plane, dw, False)
    p = plane[:dh]
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    up = _h_fancy(3 * p + above, dw, True)               # output rows 2r
    down = _h_fancy(3 * p + below, dw, True)             # output rows 2r + 1
    return np.stack([up, down], axis=1).reshape(2 * dh, 2 * dw)


def reconstruct(planes, qts, width, height, hs=1, vs=1):
    """planes: per component [bh,bw,64] int16; qts: per component [64]; luma sampling hs x vs -> (height,width,3) uint8."""
    y = idct_plane(planes[0], qts[0])[:height, :width]
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb = upsample(idct_plane(planes[1], qts[1]), width, height, hs, vs)[:height, :width] - 128
    cr = upsample(idct_plane(planes[2], qts[2]), width, height, hs, vs)[:height, :width] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


# --- the host half through the C-ABI (needs the built library, no GPU) ---------------------------------------------------
def entropy_decode(data: bytes, capacity=None):
    """fdet_jpeg_info + fdet_jpeg_entropy_decode -> (info record, flat int16 coefficients)."""
    from fdet_amd import hotpath as hp
    rc, info, msg = hp.jpeg_info(data)
    if rc != 0:
        raise ValueError(f"fdet_jpeg_info: {rc} {msg}")
    n = int(info["coef_count"]) if capacity is None else int(capacity)
    coef = np.full(max(n, 1), 0x5555, dtype=np.int16)
    rc, msg = hp.jpeg_entropy_decode(data, coef.ctypes.data, n)
    if rc != 0:
        raise ValueError(f"fdet_jpeg_entropy_decode: {rc} {msg}")
    return info, coef


def split_planes(info, coef):
    out, at = [], 0
    for c in range(int(info["ncomp"])):
        bh, bw = int(info["blocks_h"][c]), int(info["blocks_w"][c])
        out.append(coef[at:at + bh * bw * 64].reshape(bh, bw, 64))
        at += bh * bw * 64
    return out


def decode(data: bytes) -> np.ndarray:
    """File bytes -> RGB: the C host half, then the numpy restatement of the device half."""
    info, coef = entropy_decode(data)
    nc = int(info["ncomp"])
    return reconstruct(split_planes(info, coef), [info["qt"][c] for c in range(nc)], int(info["width"]), int(info["height"]),
                       int(info["hs"][0]), int(info["vs"][0]))
