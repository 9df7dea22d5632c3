"""Python restatement of the device Huffman decoder (csrc/fdet_jpeg_huff.hip; the rules are in include/fdet.h): segments
cut into subsequences of `sub_bits` bits, the state at a boundary, the parse step with its skip / close / END rules, the
synchronisation passes up to the fixed point, the block-count scan, the emit and the DC prefix sum.  Every index a kernel
computes carries an `assert` here, so that a test which runs this over a stream also shows that no index leaves its range.

The passes are restated double-buffered (a pass reads the exit states the pass before left): the fixed point is unique, so
the result is the kernels', and the pass count is the worst any thread order can need."""
import numpy as np

NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
           62, 63]
END = 0x80000000
NOCODE, RUN, DCCAT, EXHAUSTED, TRAILING = 1, 2, 4, 8, 16


def scan_start(data: bytes) -> int:
    """-> the offset of the first entropy-coded byte (behind the first SOS header)."""
    i = 2
    while True:
        assert data[i] == 0xFF, "marker expected"
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        if m == 0xDA:
            return i + 2 + n
        i += 2 + n


def dht_tables(data: bytes):
    """-> {(class, id): (bits[16], vals)} of the DHT segments in front of the scan."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        n = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xC4:
            seg, k = data[i + 4:i + 2 + n], 0
            while k < len(seg):
                bits = list(seg[k + 1:k + 17])
                out[(seg[k] >> 4, seg[k] & 15)] = (bits, list(seg[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        i += 2 + n
    return out


def scan_selectors(data: bytes):
    """-> [(dc table id, ac table id)] per component of the first SOS header."""
    j = 2
    while data[j + 1] != 0xDA:
        j += 2 + ((data[j + 2] << 8) | data[j + 3])
    ns = data[j + 4]
    return [(data[j + 6 + 2 * c] >> 4, data[j + 6 + 2 * c] & 15) for c in range(ns)]


class Geometry:
    def __init__(self, info):
        self.ncomp = int(info["ncomp"])
        self.hs, self.vs = int(info["hs"][0]), int(info["vs"][0])
        self.mcus_x, self.mcus_y = int(info["mcus_x"]), int(info["mcus_y"])
        self.bpm = 1 if self.ncomp == 1 else self.hs * self.vs + 2
        self.plane, at = [], 0
        for c in range(self.ncomp):
            self.plane.append(at)
            at += self.mcus_x * self.mcus_y * (self.hs * self.vs if c == 0 else 1) * 64
        self.coef_count = at
        assert at == int(info["coef_count"])

    def comp_of(self, blk: int) -> int:
        assert 0 <= blk < self.bpm
        luma = self.hs * self.vs
        return 0 if self.ncomp == 1 or blk < luma else 1 if blk == luma else 2

    def block_base(self, first_mcu: int, n: int, seg_blocks: int):
        """-> the first coefficient of block n (scan order) of a segment, or None past the segment's blocks."""
        if n >= seg_blocks:
            return None
        mcu, b = first_mcu + n // self.bpm, n % self.bpm
        assert mcu < self.mcus_x * self.mcus_y
        my, mx = divmod(mcu, self.mcus_x)
        c = self.comp_of(b)
        hs, vs = (self.hs, self.vs) if c == 0 else (1, 1)
        v, h = divmod(b if c == 0 else 0, hs)
        idx = self.plane[c] + ((my * vs + v) * (self.mcus_x * hs) + mx * hs + h) * 64
        assert 0 <= idx and idx + 64 <= self.coef_count
        return idx


def _tables(tables):
    """fdet_jpeg_huff_tables record -> per component ((dc), (ac)) of plain lists."""
    def one(t):
        return (t["look_nbits"].tolist(), t["look_sym"].tolist(), t["maxcode"].tolist(), t["valoffset"].tolist(),
                t["vals"].tolist(), int(t["nvals"]))
    t = tables[0] if tables.ndim else tables
    return [(one(t["dc"][c]), one(t["ac"][c])) for c in range(3)]


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def parse(seg: bytes, nbits: int, T, G: Geometry, p: int, limit: int, blk: int, z: int, sink=None):
    """The symbols that start in [p, limit) of a segment (`seg`: its bytes + at least 8 zero bytes).  sink: None (sync) or
    [coef, n, seg_blocks, first_mcu, check_tail] (emit; check_tail: not the image's last segment, where the host decoder
    refills its 64-bit window once behind the blocks and wants the restart marker there: more than 64 bits left is TRAILING).
    -> (exit position or END, blk, z, blocks completed, events)."""
    count = events = 0
    ended = False
    stop = min(limit, nbits)
    base = G.block_base(sink[3], sink[1], sink[2]) if sink is not None else None
    steps, p0 = 0, p
    while p < stop:
        steps += 1
        assert steps <= stop - p0, "a step consumes at least one bit"
        if sink is not None and sink[1] >= sink[2]:
            break
        assert 0 <= p < nbits and 0 <= blk < G.bpm and 0 <= z < 64
        rem = nbits - p
        at = p >> 3
        assert at + 5 <= len(seg)
        bits = (int.from_bytes(seg[at:at + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
        look_nbits, look_sym, maxcode, valoffset, vals, nvals = T[G.comp_of(blk)][0 if z == 0 else 1]
        look = bits >> 23
        assert 0 <= look < 512
        nb, sym = look_nbits[look], look_sym[look]
        if nb == 0 or nb > 9:
            nb = 0
            for l in range(1, 17):
                code = bits >> (32 - l)
                if code <= maxcode[l]:
                    idx = valoffset[l] + code
                    if 0 <= idx < nvals and idx < 256:
                        nb, sym = l, vals[idx]
                    break
            if nb == 0:
                events |= NOCODE
                p += 1
                continue
        if nb > rem:
            ended = True
            break
        if z == 0:
            s = sym
            if s > 16:
                events |= DCCAT
                s = 0
            if nb + s > rem:
                ended = True
                break
            assert nb + s <= 32
            if base is not None:
                sink[0][base] = _extend((bits >> (32 - nb - s)) & ((1 << s) - 1), s) if s else 0
            p += nb + s
            z = 1
            continue
        r, s = sym >> 4, sym & 15
        close = False
        if s:
            k = z + r
            if k > 63:
                events |= RUN
                p += nb
                close = True
            else:
                if nb + s > rem:
                    ended = True
                    break
                assert nb + s <= 32 and 1 <= k <= 63
                if base is not None:
                    sink[0][base + NATURAL[k]] = _extend((bits >> (32 - nb - s)) & ((1 << s) - 1), s)
                p += nb + s
                z = k + 1
                close = z > 63
        else:
            p += nb
            if r == 15:
                z += 16
                close = z > 63
            else:
                close = True
        if close:
            count += 1
            blk = (blk + 1) % G.bpm
            z = 0
            if sink is not None:
                sink[1] += 1
                if sink[1] == sink[2] and sink[4] and nbits - p > 64:
                    events |= TRAILING
                base = G.block_base(sink[3], sink[1], sink[2])
    assert p <= nbits
    if ended or p < limit:
        p = END
    return p, blk, z, count, events


def _unpack(st: int):
    return st & 31, (st >> 8) & 15, (st >> 16) & 63


def decode(scan: np.ndarray, segs, tables, info, sub_bits: int, max_passes=None):
    """The whole device path of one image -> dict(coef int16 (coef_count,), flags, passes (run until one changed nothing,
    that one included), decodes (subsequence parses of the sync), subs, converged, cap)."""
    assert sub_bits >= 64 and sub_bits % 32 == 0
    G = Geometry(info)
    T = _tables(tables)
    raw = scan.tobytes()
    S = []
    mcu_at = 0
    for s in segs:
        o, n = int(s["byte_offset"]), int(s["byte_len"])
        assert o % 16 == 0 and o + (n + 15) // 16 * 16 <= len(raw)
        assert int(s["first_mcu"]) == mcu_at and int(s["mcu_count"]) > 0
        mcu_at += int(s["mcu_count"])
        assert not any(raw[o + n:o + (n + 15) // 16 * 16]), "the padding is zero"
        subs = max(1, -(-8 * n // sub_bits))
        S.append(dict(bytes=raw[o:o + n] + bytes(8), nbits=8 * n, subs=subs, first_mcu=int(s["first_mcu"]),
                      blocks=int(s["mcu_count"]) * G.bpm, exit=[0] * subs, count=[0] * subs, last=[None] * subs))
    assert mcu_at == G.mcus_x * G.mcus_y
    cap = max(s["subs"] for s in S) + 1
    cap = cap if max_passes is None else max_passes
    passes = decodes = 0
    converged = False
    while passes < cap and not converged:
        passes += 1
        changed = False
        for s in S:
            before = list(s["exit"])
            for k in range(s["subs"]):
                entry = 0 if k == 0 else before[k - 1]
                if s["last"][k] == entry:
                    continue
                changed = True
                decodes += 1
                begin, limit = k * sub_bits, (k + 1) * sub_bits
                if entry == END:
                    p, blk, z, count = END, 0, 0, 0
                else:
                    off, blk, z = _unpack(entry)
                    assert blk < G.bpm
                    p, blk, z, count, _ev = parse(s["bytes"], s["nbits"], T, G, begin + off, limit, blk, z)
                if p != END:
                    assert 0 <= p - limit < 32
                    p = (p - limit) | (blk << 8) | (z << 16)
                s["exit"][k], s["count"][k], s["last"][k] = p, count, entry
        converged = not changed
    coef = np.zeros(G.coef_count, np.int64)
    flags = 0
    for s in S:
        first = np.cumsum([0] + s["count"])                  # the exclusive scan of the block counts
        if int(first[-1]) < s["blocks"]:
            flags |= EXHAUSTED
        for k in range(s["subs"]):
            entry = 0 if k == 0 else s["exit"][k - 1]
            if entry == END:
                continue
            off, blk, z = _unpack(entry)
            blk = blk if blk < G.bpm else 0
            sink = [coef, int(first[k]), s["blocks"], s["first_mcu"], s is not S[-1]]
            _p, _b, _z, _c, ev = parse(s["bytes"], s["nbits"], T, G, k * sub_bits + off, (k + 1) * sub_bits, blk, z, sink)
            flags |= ev
        for c in range(G.ncomp):                             # DC differences -> values, modulo 2^16, in scan order
            per = G.hs * G.vs if c == 0 else 1
            hs, vs = (G.hs, G.vs) if c == 0 else (1, 1)
            run = 0
            for j in range(s["blocks"] // G.bpm * per):
                my, mx = divmod(s["first_mcu"] + j // per, G.mcus_x)
                v, h = divmod(j % per, hs)
                idx = G.plane[c] + ((my * vs + v) * (G.mcus_x * hs) + mx * hs + h) * 64
                assert 0 <= idx and idx + 64 <= G.coef_count
                run = (run + int(coef[idx])) & 0xFFFF
                coef[idx] = run
    coef = ((coef & 0xFFFF) ^ 0x8000) - 0x8000
    return dict(coef=coef.astype(np.int16), flags=flags, passes=passes, decodes=decodes, subs=sum(s["subs"] for s in S),
                converged=converged, cap=cap)


def spare_bytes(data: bytes, count: int, value: int = 0x55) -> bytes:
    """`data` (a file with restart markers) with `count` bytes of `value` in front of its first RSTn."""
    a = scan_start(data)
    i = next(i for i in range(a, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7)
    return data[:i] + bytes([value]) * count + data[i:]


def mutations(data: bytes, count: int = 16, seed: int = 21):
    """`count` seeded single-byte mutations of the scan of `data` -> [(offset, value, bytes)]."""
    rng = np.random.default_rng(seed)
    a, b = scan_start(data), len(data) - 2
    out = []
    for _ in range(count):
        o = int(rng.integers(a, b))
        v = int(rng.integers(0, 256))
        if v == data[o]:
            v ^= 0x55
        out.append((o, v, data[:o] + bytes([v]) + data[o + 1:]))
    return out


def restart_corruptions(data: bytes):
    """Corrupt variants of a file WITH restart markers -> [(label, bytes)]: spare bytes in front of its first RSTn (1 and 7
    stay inside the host decoder's one refill, 8 and 9 sit on its edge, 24 are beyond it; two byte values, so that the spare
    bits parse differently) and 16 seeded single-byte mutations of its scan."""
    out = [(f"{k} spare bytes {v:#04x}", spare_bytes(data, k, v)) for k in (1, 7, 8, 9, 24) for v in (0x55, 0x00)]
    return out + [(f"mutation {o}={v:#04x}", b) for o, v, b in mutations(data, 16, seed=22)]
