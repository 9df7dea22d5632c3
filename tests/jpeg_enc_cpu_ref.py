"""numpy restatement of the device JPEG encoder (csrc/fdet_jpeg_enc.hip): libjpeg-turbo's baseline encoder front
end, rule for rule, so that the file equals PIL's Image.save(..., "JPEG", quality=q, subsampling=s) byte for byte.

    coefficients(rgb, quality, sub) -> int16 [n_blocks, 64]   quantised, ZIGZAG order, blocks in scan (MCU) order, dummies included
    block_bits(coef, sub)           -> uint32 [n_blocks]      bit length of every block's code
    scan_bytes(coef, sub)           -> bytes                  the entropy-coded segment, padded, NOT byte-stuffed
    encode(rgb, quality, sub)       -> bytes                  the whole file

`sub` is 0 | 1 | 2 for 4:4:4 | 4:2:2 | 4:2:0, PIL's numbering.  Plain integer arithmetic; nothing here is fast.
"""
import numpy as np

SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
LUMA_HV = {0: (1, 1), 1: (2, 1), 2: (2, 2)}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
    0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
    0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
    0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def quant_tables(quality: int) -> np.ndarray:
    """-> int64 [2, 64], natural order."""
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)])


def huff_codes(bits, vals):
    """-> {symbol: (code, length)} of a DHT table (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def header(width: int, height: int, quality: int, sub: int) -> bytes:
    qt = quant_tables(quality)
    hs, vs = LUMA_HV[sub]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in qt[t][ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([height >> 8, height & 255, width >> 8, width & 255, 3,
                                            1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        n = 2 + 1 + 16 + len(vals)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def ycc(rgb: np.ndarray):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_cols(p, w):
    return p if p.shape[1] >= w else np.concatenate([p, np.repeat(p[:, -1:], w - p.shape[1], axis=1)], axis=1)


def _pad_rows(p, h):
    return p if p.shape[0] >= h else np.concatenate([p, np.repeat(p[-1:], h - p.shape[0], axis=0)], axis=0)


def component_planes(rgb: np.ndarray, sub: int):
    """-> [Y, Cb, Cr] sample planes padded to the MCU grid, by libjpeg's order of operations: columns replicated to the MCU
    width and rows to a multiple of the vertical factor BEFORE downsampling, the last downsampled row replicated after."""
    H, W = rgb.shape[:2]
    hs, vs = LUMA_HV[sub]
    mw, mh = -(-W // (8 * hs)) * 8 * hs, -(-H // (8 * vs)) * 8 * vs
    planes = []
    for c, p in enumerate(ycc(rgb)):
        p = _pad_rows(_pad_cols(p, mw), -(-H // vs) * vs)
        if c and hs == 2:
            x = np.arange(mw // 2)
            if vs == 2:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + (1 + (x & 1))[None, :]) >> 2
            else:
                p = (p[:, 0::2] + p[:, 1::2] + (x & 1)[None, :]) >> 1
        planes.append(_pad_rows(p, mh // (vs if c and vs == 2 else 1)))
    return planes


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """jfdctint.c, one pass along the last axis of d [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(plane: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """plane [8 bh, 8 bw] -> quantised int64 [bh, bw, 64] in natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    d = _fdct_pass(d, True)                                    # rows
    d = _fdct_pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)  # columns
    d = d.reshape(bh, bw, 64)
    div = qt.astype(np.int64) << 3
    return np.sign(d) * ((np.abs(d) + (div >> 1)) // div)


def geometry(width: int, height: int, sub: int):
    hs, vs = LUMA_HV[sub]
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    return hs, vs, mx, my, mx * my * (hs * vs + 2)


def coefficients(rgb: np.ndarray, quality: int, sub: int) -> np.ndarray:
    H, W = rgb.shape[:2]
    hs, vs, mx, my, nb = geometry(W, H, sub)
    qt = quant_tables(quality)
    planes = component_planes(rgb, sub)
    q = [fdct_quant(planes[0], qt[0]), fdct_quant(planes[1], qt[1]), fdct_quant(planes[2], qt[1])]
    real_w, real_h = -(-W // 8), -(-H // 8)
    out = np.zeros((nb, 64), dtype=np.int64)
    k = 0
    for my_ in range(my):
        for mx_ in range(mx):
            prev = None
            for v in range(vs):
                for h in range(hs):
                    by, bx = my_ * vs + v, mx_ * hs + h
                    if by < real_h and bx < real_w:
                        prev = q[0][by, bx]
                        out[k] = prev
                    else:                                      # a dummy block: DC of the block before it, no AC
                        prev = np.concatenate([prev[:1], np.zeros(63, dtype=np.int64)])
                        out[k] = prev
                    k += 1
            out[k], out[k + 1] = q[1][my_, mx_], q[2][my_, mx_]
            k += 2
    return out[:, ZIGZAG].astype(np.int16)


def to_planes(coef: np.ndarray, width: int, height: int, sub: int):
    """coefficients() -> what a decoder's entropy stage gives: per component one [blocks_h, blocks_w, 64] plane in natural order."""
    hs, vs, mx, my, _nb = geometry(width, height, sub)
    nat = np.zeros_like(coef)
    nat[:, ZIGZAG] = coef
    per = hs * vs + 2
    mcus = nat.reshape(my, mx, per, 64)
    luma = mcus[:, :, :hs * vs].reshape(my, mx, vs, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my * vs, mx * hs, 64)
    return [luma, mcus[:, :, hs * vs], mcus[:, :, hs * vs + 1]]


def _block_symbols(zz, pred, comp_tab):
    """-> list of (code, length) pairs of one block (zz: 64 ints in zigzag order)."""
    out = []
    diff = int(zz[0]) - pred
    n = abs(diff).bit_length()
    out.append(DC_CODES[comp_tab][n])
    if n:
        out.append((diff if diff >= 0 else diff + (1 << n) - 1, n))
    run = 0
    ac = AC_CODES[comp_tab]
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac[0xF0])
            run -= 16
        n = abs(v).bit_length()
        out.append(ac[run << 4 | n])
        out.append((v if v >= 0 else v + (1 << n) - 1, n))
        run = 0
    if run:
        out.append(ac[0x00])
    return out


def _walk(coef: np.ndarray, sub: int):
    hs, vs = LUMA_HV[sub]
    per = hs * vs + 2
    pred = [0, 0, 0]
    for b in range(coef.shape[0]):
        k = b % per
        c = 0 if k < hs * vs else k - hs * vs + 1
        yield _block_symbols(coef[b], pred[c], 0 if c == 0 else 1)
        pred[c] = int(coef[b, 0])


def block_bits(coef: np.ndarray, sub: int) -> np.ndarray:
    return np.array([sum(n for _, n in syms) for syms in _walk(coef, sub)], dtype=np.uint32)


def scan_bytes(coef: np.ndarray, sub: int) -> bytes:
    acc, nbits = 0, 0
    for syms in _walk(coef, sub):
        for code, n in syms:
            acc = (acc << n) | code
            nbits += n
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((nbits + pad) // 8, "big")


def assemble(width: int, height: int, quality: int, sub: int, scan: bytes) -> bytes:
    return header(width, height, quality, sub) + scan.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def encode(rgb: np.ndarray, quality: int = 75, sub: int = 2) -> bytes:
    H, W = rgb.shape[:2]
    return assemble(W, H, quality, sub, scan_bytes(coefficients(rgb, quality, sub), sub))


# ---- the fixture set (tools/make_goldens_jpeg_enc.py writes it, the tests read it) -------------------------------------------
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 9), (53, 37), (100, 75), (33, 130), (99, 131)]          # (width, height)
KINDS = ("noise", "ramp", "saturated", "constant")
QUALITIES = (5, 75, 100)


def source(kind: str, width: int, height: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * width + height)
    if kind == "noise":
        return rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (height, width, 3), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "constant":
        return np.full((height, width, 3), (200, 100, 50), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:height, 0:width]
        return np.stack([(x * 255) // max(width - 1, 1), (y * 255) // max(height - 1, 1),
                         ((x + y) * 255) // max(width + height - 2, 1)], axis=-1).astype(np.uint8)
    raise ValueError(kind)


def cases():
    """-> [(name, kind, width, height, quality, sub)] of the fixture set: shapes x kinds x (qualities x subsamplings)."""
    out = []
    for w, h in SHAPES:
        for kind in KINDS:
            for q in QUALITIES:
                for sub in (0, 1, 2):
                    out.append((f"{kind}_{w}x{h}_q{q}_s{sub}", kind, w, h, q, sub))
    return out
