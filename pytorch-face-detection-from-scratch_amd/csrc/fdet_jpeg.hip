// Baseline JPEG decode into the device image bank: the hybrid split of GPU JPEG decoders.
//
//   host    fdet_jpeg_info            marker parsing (SOF0/SOF1, DQT, DHT, DRI, SOS, APP0/APP14), the supported-subset decision
//           fdet_jpeg_entropy_decode  Huffman decoding with DC prediction, byte stuffing and restart markers -> quantised
//                                     int16 coefficients in natural order, one [blocks_h][blocks_w][64] plane per component
//           fdet_jpeg_scan_prepare    instead of the line above when the device Huffman-decodes (fdet_jpeg_huff.hip): the decode
//                                     tables as a POD and the scan unstuffed into one byte run per restart interval
//   device  fdet_jpeg_reconstruct     k_jpeg_idct: dequantise + libjpeg's accurate-integer 8x8 inverse DCT -> uint8 sample planes
//                                     k_jpeg_rgb:  "fancy" chroma upsampling + YCbCr -> RGB + crop -> HWC uint8 in the bank
//
// Every device step is integer arithmetic in libjpeg (jidctint.c, jdsample.c, jdcolor.c), restated here operation for operation,
// so the bank holds the bytes libjpeg-turbo's default decode gives.  tests/jpeg_cpu_ref.py restates the device half in numpy.
// The host functions make no HIP call and keep no mutable global state: a thread pool may call them concurrently.
#include "fdet_common.h"
#include <cstdint>

using namespace fdet;

namespace {

// ------------------------------------------------------------------------------------------------------------------
// host: markers
// ------------------------------------------------------------------------------------------------------------------
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct RawHuff {
  bool defined;
  uint8_t bits[17];      // bits[l] = number of codes of length l
  uint8_t vals[256];
  int nvals;
};

struct Parsed {
  int width, height, ncomp, restart_interval;
  int cid[4], hs[4], vs[4], tq[4], td[4], ta[4];
  uint16_t q[4][64];
  bool qdef[4];
  RawHuff dc[4], ac[4];
  size_t scan_pos;       // first byte of the entropy-coded segment
  int blocks_w[3], blocks_h[3], mcus_x, mcus_y;
  int64_t coef_count;
};

#define JPEG_CORRUPT(...) return fdet::fail(FDET_JPEG_ECORRUPT, __VA_ARGS__)
#define JPEG_UNSUPPORTED(...) return fdet::fail(FDET_JPEG_UNSUPPORTED, __VA_ARGS__)

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parse everything up to and including the first SOS header.  Every read is inside [0, n).
int parse_headers(const uint8_t* b, size_t n, Parsed& P) {
  if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) JPEG_CORRUPT("jpeg: no SOI marker (not a JPEG)");
  memset(&P, 0, sizeof(P));
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = 0;
  size_t pos = 2;
  for (;;) {
    while (pos < n && b[pos] != 0xFF) ++pos;             // libjpeg skips bytes between segments too
    while (pos < n && b[pos] == 0xFF) ++pos;             // fill bytes
    if (pos >= n) JPEG_CORRUPT("jpeg: the stream ends before a scan (SOS) starts");
    const int m = b[pos++];
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // stuffed / standalone markers
    if (m == 0xD8) JPEG_CORRUPT("jpeg: second SOI marker");
    if (m == 0xD9) JPEG_CORRUPT("jpeg: EOI before any scan");
    if (pos + 2 > n) JPEG_CORRUPT("jpeg: truncated in a marker segment");
    const int L = be16(b + pos);
    if (L < 2 || pos + (size_t)L > n) JPEG_CORRUPT("jpeg: marker 0x%02X segment of %d bytes runs past the end", m, L);
    const uint8_t* seg = b + pos + 2;
    const int sl = L - 2;
    pos += (size_t)L;
    if (m == 0xC0 || m == 0xC1) {                        // baseline / extended sequential, Huffman
      if (have_sof) JPEG_CORRUPT("jpeg: second frame header");
      if (sl < 6) JPEG_CORRUPT("jpeg: short frame header");
      if (seg[0] != 8) JPEG_UNSUPPORTED("jpeg: %d-bit samples (8-bit only)", (int)seg[0]);
      P.height = be16(seg + 1);
      P.width = be16(seg + 3);
      P.ncomp = seg[5];
      if (P.width == 0) JPEG_CORRUPT("jpeg: zero width");
      if (P.height == 0) JPEG_UNSUPPORTED("jpeg: height given by a DNL marker");
      if (P.ncomp < 1 || P.ncomp > 4 || sl != 6 + 3 * P.ncomp) JPEG_CORRUPT("jpeg: bad frame header (%d components)", P.ncomp);
      if (P.ncomp != 1 && P.ncomp != 3) JPEG_UNSUPPORTED("jpeg: %d components (grey or YCbCr only)", P.ncomp);
      for (int c = 0; c < P.ncomp; ++c) {
        P.cid[c] = seg[6 + 3 * c];
        P.hs[c] = seg[7 + 3 * c] >> 4;
        P.vs[c] = seg[7 + 3 * c] & 15;
        P.tq[c] = seg[8 + 3 * c];
        if (P.hs[c] < 1 || P.hs[c] > 4 || P.vs[c] < 1 || P.vs[c] > 4 || P.tq[c] > 3)
          JPEG_CORRUPT("jpeg: bad component %d in the frame header", c);
      }
      have_sof = true;
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      JPEG_UNSUPPORTED("jpeg: frame type SOF%d (progressive, lossless, differential or arithmetic)", m - 0xC0);
    } else if (m == 0xCC) {
      JPEG_UNSUPPORTED("jpeg: arithmetic coding conditioning (DAC)");
    } else if (m == 0xDB) {                              // DQT
      int i = 0;
      while (i < sl) {
        const int pq = seg[i] >> 4, tq = seg[i] & 15;
        ++i;
        if (pq > 1 || tq > 3) JPEG_CORRUPT("jpeg: bad DQT header");
        const int need = pq ? 128 : 64;
        if (i + need > sl) JPEG_CORRUPT("jpeg: short DQT segment");
        for (int k = 0; k < 64; ++k) P.q[tq][kNatural[k]] = pq ? (uint16_t)be16(seg + i + 2 * k) : (uint16_t)seg[i + k];
        P.qdef[tq] = true;
        i += need;
      }
    } else if (m == 0xC4) {                              // DHT
      int i = 0;
      while (i < sl) {
        if (i + 17 > sl) JPEG_CORRUPT("jpeg: short DHT segment");
        const int tc = seg[i] >> 4, th = seg[i] & 15;
        if (tc > 1 || th > 3) JPEG_CORRUPT("jpeg: bad DHT header");
        RawHuff& H = tc ? P.ac[th] : P.dc[th];
        int count = 0;
        H.bits[0] = 0;
        for (int l = 1; l <= 16; ++l) { H.bits[l] = seg[i + l]; count += H.bits[l]; }
        i += 17;
        if (count > 256 || i + count > sl) JPEG_CORRUPT("jpeg: bad DHT counts");
        memcpy(H.vals, seg + i, (size_t)count);
        H.nvals = count;
        H.defined = true;
        i += count;
      }
    } else if (m == 0xDD) {                              // DRI
      if (sl != 2) JPEG_CORRUPT("jpeg: bad DRI segment");
      P.restart_interval = be16(seg);
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) { adobe = true; adobe_transform = seg[11]; }
    } else if (m == 0xDA) {                              // SOS
      if (!have_sof) JPEG_CORRUPT("jpeg: scan before the frame header");
      if (sl < 1) JPEG_CORRUPT("jpeg: short scan header");
      const int ns = seg[0];
      if (ns < 1 || ns > 4 || sl != 1 + 2 * ns + 3) JPEG_CORRUPT("jpeg: bad scan header");
      if (ns != P.ncomp) JPEG_UNSUPPORTED("jpeg: a scan of %d of the %d components (multi-scan)", ns, P.ncomp);
      for (int c = 0; c < ns; ++c) {
        if (seg[1 + 2 * c] != P.cid[c]) JPEG_UNSUPPORTED("jpeg: scan components out of frame order");
        P.td[c] = seg[2 + 2 * c] >> 4;
        P.ta[c] = seg[2 + 2 * c] & 15;
        if (P.td[c] > 3 || P.ta[c] > 3) JPEG_CORRUPT("jpeg: bad table selector in the scan header");
      }
      if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0)
        JPEG_UNSUPPORTED("jpeg: spectral selection / successive approximation in a sequential scan");
      P.scan_pos = pos;
      break;
    }                                                    // APPn, COM and everything else: skipped
  }
  // the supported subset
  if (P.ncomp == 3) {
    bool rgb = false;                                    // libjpeg's colour space guess (jdapimin.c default_decompress_parms)
    if (jfif) rgb = false;
    else if (adobe) rgb = adobe_transform == 0;
    else rgb = P.cid[0] == 'R' && P.cid[1] == 'G' && P.cid[2] == 'B';
    if (rgb) JPEG_UNSUPPORTED("jpeg: RGB components (no YCbCr transform)");
    if (P.hs[1] != 1 || P.vs[1] != 1 || P.hs[2] != 1 || P.vs[2] != 1 ||
        !((P.hs[0] == 1 && P.vs[0] == 1) || (P.hs[0] == 2 && P.vs[0] == 1) || (P.hs[0] == 2 && P.vs[0] == 2)))
      JPEG_UNSUPPORTED("jpeg: sampling %dx%d,%dx%d,%dx%d (luma 1x1, 2x1 or 2x2 with chroma 1x1 only)", P.hs[0], P.vs[0], P.hs[1],
                       P.vs[1], P.hs[2], P.vs[2]);
  } else {
    P.hs[0] = P.vs[0] = 1;                               // a single component is not interleaved: its factors mean nothing
  }
  for (int c = 0; c < P.ncomp; ++c) {
    if (!P.qdef[P.tq[c]]) JPEG_CORRUPT("jpeg: quantisation table %d is not defined", P.tq[c]);
    if (!P.dc[P.td[c]].defined || !P.ac[P.ta[c]].defined) JPEG_CORRUPT("jpeg: a Huffman table of component %d is not defined", c);
  }
  P.mcus_x = (P.width + 8 * P.hs[0] - 1) / (8 * P.hs[0]);
  P.mcus_y = (P.height + 8 * P.vs[0] - 1) / (8 * P.vs[0]);
  P.coef_count = 0;
  for (int c = 0; c < P.ncomp; ++c) {
    P.blocks_w[c] = P.mcus_x * P.hs[c];
    P.blocks_h[c] = P.mcus_y * P.vs[c];
    P.coef_count += (int64_t)P.blocks_w[c] * P.blocks_h[c] * 64;
  }
  return FDET_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// host: Huffman decoding
// ------------------------------------------------------------------------------------------------------------------
constexpr int LOOK = 9;

struct HuffTab {
  uint8_t look_nbits[1 << LOOK], look_sym[1 << LOOK];
  int32_t maxcode[18], valoffset[18];
  const uint8_t* vals;
  int nvals;
};

int build_huff(const RawHuff& R, HuffTab& T) {
  uint8_t size[257];
  uint32_t code_of[257];
  int p = 0;
  for (int l = 1; l <= 16; ++l)
    for (int i = 0; i < R.bits[l]; ++i) size[p++] = (uint8_t)l;
  const int nsym = p;
  size[p] = 0;
  uint32_t code = 0;
  int si = size[0];
  p = 0;
  while (size[p]) {
    while (size[p] == si) code_of[p++] = code++;
    if (code > (1u << si)) JPEG_CORRUPT("jpeg: Huffman table with more codes than its lengths allow");
    code <<= 1;
    ++si;
  }
  p = 0;
  for (int l = 1; l <= 16; ++l) {
    if (R.bits[l]) {
      T.valoffset[l] = p - (int32_t)code_of[p];
      p += R.bits[l];
      T.maxcode[l] = (int32_t)code_of[p - 1];
    } else {
      T.maxcode[l] = -1;
      T.valoffset[l] = 0;
    }
  }
  T.maxcode[17] = 0x7fffffff;
  T.vals = R.vals;
  T.nvals = nsym;
  memset(T.look_nbits, 0, sizeof(T.look_nbits));
  memset(T.look_sym, 0, sizeof(T.look_sym));
  p = 0;
  for (int l = 1; l <= LOOK; ++l)
    for (int i = 0; i < R.bits[l]; ++i, ++p) {
      const uint32_t first = code_of[p] << (LOOK - l);
      for (uint32_t k = 0; k < (1u << (LOOK - l)); ++k) {
        T.look_nbits[first + k] = (uint8_t)l;
        T.look_sym[first + k] = R.vals[p];
      }
    }
  return FDET_OK;
}

// Entropy-coded bytes -> bits.  `cnt` counts REAL bits in the low end of `acc`; the reader stops in front of a marker
// or the end of the input and never invents bits: a symbol that needs more than there are is an error.
struct BitReader {
  const uint8_t* b;
  size_t n, pos;
  uint64_t acc;
  int cnt;
  void fill() {
    while (cnt <= 56 && pos < n) {
      const uint8_t c = b[pos];
      if (c == 0xFF) {
        if (pos + 1 >= n || b[pos + 1] != 0x00) return;  // a marker (or a cut FF): entropy data ends here
        pos += 2;
      } else {
        pos += 1;
      }
      acc = (acc << 8) | c;
      cnt += 8;
    }
  }
};

inline int huff_decode(BitReader& R, const HuffTab& T) {
  if (R.cnt < 16) R.fill();
  const uint32_t look = R.cnt >= LOOK ? (uint32_t)(R.acc >> (R.cnt - LOOK)) & ((1u << LOOK) - 1)
                                      : (uint32_t)(R.acc << (LOOK - R.cnt)) & ((1u << LOOK) - 1);
  const int nb = T.look_nbits[look];
  if (nb) {
    if (nb > R.cnt) return -1;
    R.cnt -= nb;
    return T.look_sym[look];
  }
  int32_t code = 0;
  for (int l = 1; l <= 16; ++l) {
    if (R.cnt == 0) return -1;
    code = (code << 1) | (int32_t)((R.acc >> (R.cnt - 1)) & 1);
    R.cnt -= 1;
    if (code <= T.maxcode[l]) {
      const int idx = T.valoffset[l] + code;
      if (idx < 0 || idx >= T.nvals) return -1;
      return T.vals[idx];
    }
  }
  return -1;
}

inline int receive_extend(BitReader& R, int s, int& out) {
  if (R.cnt < s) R.fill();
  if (R.cnt < s) return -1;
  const int v = (int)((R.acc >> (R.cnt - s)) & ((1u << s) - 1));
  R.cnt -= s;
  out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
  return 0;
}

}  // namespace

extern "C" int fdet_jpeg_info(const uint8_t* bytes, size_t n, fdet_jpeg_info_t* out) {
  FDET_REQUIRE(bytes && out && n > 0, "jpeg_info: null pointer or empty input");
  Parsed P;
  if (int rc = parse_headers(bytes, n, P)) return rc;
  memset(out, 0, sizeof(*out));
  out->width = P.width;
  out->height = P.height;
  out->ncomp = P.ncomp;
  out->restart_interval = P.restart_interval;
  out->mcus_x = P.mcus_x;
  out->mcus_y = P.mcus_y;
  out->coef_count = P.coef_count;
  for (int c = 0; c < P.ncomp; ++c) {
    out->hs[c] = P.hs[c];
    out->vs[c] = P.vs[c];
    out->blocks_w[c] = P.blocks_w[c];
    out->blocks_h[c] = P.blocks_h[c];
    memcpy(out->qt[c], P.q[P.tq[c]], sizeof(out->qt[c]));
  }
  return FDET_OK;
}

extern "C" int fdet_jpeg_entropy_decode(const uint8_t* bytes, size_t n, int16_t* coef, size_t capacity) {
  FDET_REQUIRE(bytes && coef && n > 0 && capacity > 0, "jpeg_entropy_decode: null pointer or empty buffer");
  Parsed P;
  if (int rc = parse_headers(bytes, n, P)) return rc;
  if ((uint64_t)P.coef_count > (uint64_t)capacity)
    return fail(FDET_EWORKSPACE, "jpeg_entropy_decode: the image needs %lld coefficients, the buffer holds %zu",
                (long long)P.coef_count, capacity);
  HuffTab dc[3], ac[3];
  int64_t plane[3];
  int64_t at = 0;
  for (int c = 0; c < P.ncomp; ++c) {
    if (int rc = build_huff(P.dc[P.td[c]], dc[c])) return rc;
    if (int rc = build_huff(P.ac[P.ta[c]], ac[c])) return rc;
    plane[c] = at;
    at += (int64_t)P.blocks_w[c] * P.blocks_h[c] * 64;
  }
  BitReader R{bytes, n, P.scan_pos, 0, 0};
  int last_dc[3] = {0, 0, 0};
  int to_go = P.restart_interval, next_rst = 0;
  for (int my = 0; my < P.mcus_y; ++my) {
    for (int mx = 0; mx < P.mcus_x; ++mx) {
      if (P.restart_interval && to_go == 0) {
        R.fill();                                        // runs up to the marker; what is left are the padding bits
        R.cnt = 0;
        R.acc = 0;
        size_t p = R.pos;
        if (p >= n || bytes[p] != 0xFF) JPEG_CORRUPT("jpeg: no restart marker where MCU %d starts", my * P.mcus_x + mx);
        while (p < n && bytes[p] == 0xFF) ++p;
        if (p >= n || bytes[p] != 0xD0 + next_rst)
          JPEG_CORRUPT("jpeg: expected RST%d in front of MCU %d", next_rst, my * P.mcus_x + mx);
        R.pos = p + 1;
        next_rst = (next_rst + 1) & 7;
        to_go = P.restart_interval;
        last_dc[0] = last_dc[1] = last_dc[2] = 0;
      }
      for (int c = 0; c < P.ncomp; ++c) {
        for (int v = 0; v < P.vs[c]; ++v) {
          for (int h = 0; h < P.hs[c]; ++h) {
            const int64_t idx = plane[c] + ((int64_t)(my * P.vs[c] + v) * P.blocks_w[c] + (mx * P.hs[c] + h)) * 64;
            if (idx < 0 || (uint64_t)(idx + 64) > (uint64_t)capacity) JPEG_CORRUPT("jpeg: block outside the coefficient buffer");
            int16_t* blk = coef + idx;
            memset(blk, 0, 64 * sizeof(int16_t));
            int s = huff_decode(R, dc[c]);
            if (s < 0 || s > 16) JPEG_CORRUPT("jpeg: bad or truncated entropy data (DC) in MCU %d", my * P.mcus_x + mx);
            if (s) {
              int d;
              if (receive_extend(R, s, d)) JPEG_CORRUPT("jpeg: truncated entropy data in MCU %d", my * P.mcus_x + mx);
              last_dc[c] += d;
            }
            blk[0] = (int16_t)last_dc[c];
            for (int k = 1; k < 64; ++k) {
              const int rs = huff_decode(R, ac[c]);
              if (rs < 0) JPEG_CORRUPT("jpeg: bad or truncated entropy data (AC) in MCU %d", my * P.mcus_x + mx);
              const int r = rs >> 4;
              s = rs & 15;
              if (s) {
                k += r;
                if (k > 63) JPEG_CORRUPT("jpeg: coefficient run past the end of a block in MCU %d", my * P.mcus_x + mx);
                int d;
                if (receive_extend(R, s, d)) JPEG_CORRUPT("jpeg: truncated entropy data in MCU %d", my * P.mcus_x + mx);
                blk[kNatural[k]] = (int16_t)d;
              } else {
                if (r != 15) break;                      // end of block
                k += 15;
              }
            }
          }
        }
      }
      if (P.restart_interval) --to_go;
    }
  }
  return FDET_OK;
}

// The host half of the device Huffman decoder (fdet_jpeg_huff.hip): the same headers and tables, and one walk
// over the entropy-coded bytes with BitReader::fill's rules that unstuffs them into one run per restart interval.
extern "C" int fdet_jpeg_scan_prepare(const uint8_t* bytes, size_t n, uint8_t* scan_out, size_t scan_capacity,
                                      size_t* scan_bytes, fdet_jpeg_huff_segment* segs, int seg_capacity, int* n_segs,
                                      fdet_jpeg_huff_tables* tables) {
  FDET_REQUIRE(bytes && scan_out && scan_bytes && segs && n_segs && tables && n > 0 && seg_capacity > 0,
               "jpeg_scan_prepare: null pointer or empty buffer");
  Parsed P;
  if (int rc = parse_headers(bytes, n, P)) return rc;
  memset(tables, 0, sizeof(*tables));
  for (int c = 0; c < P.ncomp; ++c) {
    for (int k = 0; k < 2; ++k) {
      HuffTab T;
      if (int rc = build_huff(k ? P.ac[P.ta[c]] : P.dc[P.td[c]], T)) return rc;
      fdet_jpeg_huff_table& D = k ? tables->ac[c] : tables->dc[c];
      memcpy(D.look_nbits, T.look_nbits, sizeof(D.look_nbits));
      memcpy(D.look_sym, T.look_sym, sizeof(D.look_sym));
      memcpy(D.maxcode, T.maxcode, sizeof(D.maxcode));
      memcpy(D.valoffset, T.valoffset, sizeof(D.valoffset));
      memcpy(D.vals, T.vals, (size_t)T.nvals);
      D.nvals = T.nvals;
    }
  }
  const int64_t mcus = (int64_t)P.mcus_x * P.mcus_y;
  const int64_t interval = P.restart_interval ? P.restart_interval : mcus;
  const int64_t expect = (mcus + interval - 1) / interval;
  if (expect > (int64_t)seg_capacity)
    return fail(FDET_EWORKSPACE, "jpeg_scan_prepare: the scan has %lld segments, the buffer holds %d", (long long)expect,
                seg_capacity);
  size_t pos = P.scan_pos, at = 0;
  for (int64_t s = 0; s < expect; ++s) {
    const size_t start = at;
    for (;;) {                                           // BitReader::fill, byte by byte
      if (pos >= n) break;
      const uint8_t c = bytes[pos];
      if (c == 0xFF) {
        if (pos + 1 >= n || bytes[pos + 1] != 0x00) break;
        pos += 2;
      } else {
        pos += 1;
      }
      if (at >= scan_capacity)
        return fail(FDET_EWORKSPACE, "jpeg_scan_prepare: the unstuffed scan does not fit in %zu bytes", scan_capacity);
      scan_out[at++] = c;
    }
    const size_t len = at - start;
    if (len >= ((size_t)1 << 27)) return FDET_JPEG_HUFF_HOST;
    const size_t padded = (at + 15) & ~(size_t)15;
    if (padded > scan_capacity)
      return fail(FDET_EWORKSPACE, "jpeg_scan_prepare: the unstuffed scan does not fit in %zu bytes", scan_capacity);
    memset(scan_out + at, 0, padded - at);
    at = padded;
    memset(&segs[s], 0, sizeof(segs[s]));
    segs[s].byte_offset = (int64_t)start;
    segs[s].byte_len = (int32_t)len;
    segs[s].first_mcu = (int32_t)(s * interval);
    segs[s].mcu_count = (int32_t)(mcus - s * interval < interval ? mcus - s * interval : interval);
    if (s + 1 < expect) {                                // the host decoder's restart rule, nothing more lenient
      size_t p = pos;
      if (p >= n || bytes[p] != 0xFF) return FDET_JPEG_HUFF_HOST;
      while (p < n && bytes[p] == 0xFF) ++p;
      if (p >= n || bytes[p] != 0xD0 + (int)(s & 7)) return FDET_JPEG_HUFF_HOST;
      pos = p + 1;
    }
  }
  {                                                      // more segments than the MCUs need: out of the ordinary
    size_t p = pos;
    while (p < n && bytes[p] == 0xFF) ++p;
    if (p > pos && p < n && bytes[p] >= 0xD0 && bytes[p] <= 0xD7) return FDET_JPEG_HUFF_HOST;
  }
  *scan_bytes = at;
  *n_segs = (int)expect;
  return FDET_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// device: dequantise + inverse DCT (jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2)
// ------------------------------------------------------------------------------------------------------------------
namespace {

// One 8-point pass.  Wrapping 32-bit arithmetic (unsigned, so that an absurd coefficient wraps instead of being undefined);
// the result is the library's whenever the library's own sums fit in 32 bits.
template <int SHIFT>
__host__ __device__ __forceinline__ void idct8(const int32_t (&d)[8], int32_t (&o)[8]) {
  const uint32_t d0 = (uint32_t)d[0], d1 = (uint32_t)d[1], d2 = (uint32_t)d[2], d3 = (uint32_t)d[3];
  const uint32_t d4 = (uint32_t)d[4], d5 = (uint32_t)d[5], d6 = (uint32_t)d[6], d7 = (uint32_t)d[7];
  // even part
  uint32_t z1 = (d2 + d6) * 4433u;
  uint32_t tmp2 = z1 + d6 * (uint32_t)(-15137);
  uint32_t tmp3 = z1 + d2 * 6270u;
  uint32_t tmp0 = (d0 + d4) << 13;
  uint32_t tmp1 = (d0 - d4) << 13;
  const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  tmp0 = d7; tmp1 = d5; tmp2 = d3; tmp3 = d1;
  z1 = tmp0 + tmp3;
  uint32_t z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u;
  tmp1 *= 16819u;
  tmp2 *= 25172u;
  tmp3 *= 12299u;
  z1 *= (uint32_t)(-7373);
  z2 *= (uint32_t)(-20995);
  z3 *= (uint32_t)(-16069);
  z4 *= (uint32_t)(-3196);
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr uint32_t RND = 1u << (SHIFT - 1);
  o[0] = (int32_t)(tmp10 + tmp3 + RND) >> SHIFT;
  o[7] = (int32_t)(tmp10 - tmp3 + RND) >> SHIFT;
  o[1] = (int32_t)(tmp11 + tmp2 + RND) >> SHIFT;
  o[6] = (int32_t)(tmp11 - tmp2 + RND) >> SHIFT;
  o[2] = (int32_t)(tmp12 + tmp1 + RND) >> SHIFT;
  o[5] = (int32_t)(tmp12 - tmp1 + RND) >> SHIFT;
  o[3] = (int32_t)(tmp13 + tmp0 + RND) >> SHIFT;
  o[4] = (int32_t)(tmp13 - tmp0 + RND) >> SHIFT;
}

// the post-IDCT limit table (jdmaster.c prepare_range_limit_table) indexed with `v & RANGE_MASK`, level shift included
__host__ __device__ __forceinline__ uint32_t range_limit(int32_t v) {
  const int32_t i = v & 1023;
  return (uint32_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

constexpr int IDCT_WAVES = 4;          // waves per workgroup, eight 8x8 blocks per wave
constexpr int CST_PITCH = 72;          // int16 per staged block: 64 + 8 (144 bytes: the column reads of a wave's 8 blocks fall on
                                       // 8 different bank quads)
constexpr int MID_PITCH = 72;          // int32 per block between the passes: 64 + 8 (288 bytes)

// grid (groups of 4 x 8 blocks, image).  Lane l of a wave: block l >> 3 of its eight; it loads coefficient row l & 7 with one
// 16-byte load (the wave reads 1 KiB contiguously), transposes through LDS, runs column l & 7 in pass 1, transposes back and
// runs row l & 7 in pass 2, then stores its 8 samples with one 8-byte store.
__global__ void __launch_bounds__(256)
k_jpeg_idct(const int16_t* __restrict__ coef, const fdet_jpeg_desc* __restrict__ descs, uint8_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) int16_t cst[IDCT_WAVES][8 * CST_PITCH];
  __shared__ __attribute__((aligned(16))) int32_t mid[IDCT_WAVES][8 * MID_PITCH];
  const fdet_jpeg_desc* D = descs + blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = lane >> 3, j = lane & 7;
  const int ncomp = D->ncomp;
  // which component this wave's group of eight blocks belongs to (components follow each other, each rounded up to groups)
  int g = blockIdx.x * IDCT_WAVES + wave;
  int c = -1, nb = 0, bw = 1;
  for (int k = 0; k < ncomp; ++k) {
    const int nbk = D->blocks_w[k] * D->blocks_h[k];
    const int gk = (nbk + 7) >> 3;
    if (c < 0) {
      if (g < gk) { c = k; nb = nbk; bw = D->blocks_w[k]; }
      else g -= gk;
    }
  }
  const int blk = g * 8 + b;
  const bool active = c >= 0 && blk < nb;
  const int cc = c < 0 ? 0 : c;
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  if (active) raw = *reinterpret_cast<const uint4*>(coef + D->coef_offset[cc] + (int64_t)blk * 64 + j * 8);
  *reinterpret_cast<uint4*>(&cst[wave][b * CST_PITCH + j * 8]) = raw;
  __syncthreads();
  int32_t d[8], o[8];
  const uint16_t* q = D->qt[cc];
#pragma unroll
  for (int r = 0; r < 8; ++r) d[r] = (int32_t)cst[wave][b * CST_PITCH + r * 8 + j] * (int32_t)q[r * 8 + j];
  idct8<11>(d, o);                                       // pass 1: column j, results scaled up by 2^PASS1_BITS
#pragma unroll
  for (int r = 0; r < 8; ++r) mid[wave][b * MID_PITCH + r * 8 + j] = o[r];
  __syncthreads();
  const int4 lo = *reinterpret_cast<const int4*>(&mid[wave][b * MID_PITCH + j * 8]);
  const int4 hi = *reinterpret_cast<const int4*>(&mid[wave][b * MID_PITCH + j * 8 + 4]);
  d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w; d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
  idct8<18>(d, o);                                       // pass 2: row j, descale by CONST_BITS + PASS1_BITS + 3
  if (!active) return;
  const uint32_t w0 = range_limit(o[0]) | (range_limit(o[1]) << 8) | (range_limit(o[2]) << 16) | (range_limit(o[3]) << 24);
  const uint32_t w1 = range_limit(o[4]) | (range_limit(o[5]) << 8) | (range_limit(o[6]) << 16) | (range_limit(o[7]) << 24);
  const int by = blk / bw, bx = blk - by * bw;
  uint8_t* dst = ws + D->plane_offset[cc] + ((int64_t)(by * 8 + j) * bw + bx) * 8;
  *reinterpret_cast<uint2*>(dst) = make_uint2(w0, w1);
}

// ------------------------------------------------------------------------------------------------------------------
// device: upsampling (jdsample.c) + colour conversion (jdcolor.c) + crop
// ------------------------------------------------------------------------------------------------------------------
struct RgbGeom {
  const uint8_t *yp, *cbp, *crp;
  int W, H, py, pc;        // image size, luma / chroma plane pitch
  int mode;                // 0 grey, 1 chroma at full size, 2 replicate (hs = 2, dw <= 2), 3 h2v1 fancy, 4 h2v2 fancy
  int vshift;              // log2(vs)
  int dw, dh;              // downsampled chroma size
};

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }

__device__ __forceinline__ void jpeg_pixel(const RgbGeom& G, int x, int y, uint32_t& r, uint32_t& g, uint32_t& b) {
  const int Y = G.yp[(int64_t)y * G.py + x];
  if (G.mode == 0) { r = g = b = (uint32_t)Y; return; }
  int cb, cr;
  if (G.mode == 1) {
    const int64_t o = (int64_t)y * G.pc + x;
    cb = G.cbp[o]; cr = G.crp[o];
  } else if (G.mode == 2) {
    const int64_t o = (int64_t)(y >> G.vshift) * G.pc + (x >> 1);
    cb = G.cbp[o]; cr = G.crp[o];
  } else {
    const int i = x >> 1, odd = x & 1;
    const int nbr = odd ? min(i + 1, G.dw - 1) : max(i - 1, 0);
    if (G.mode == 3) {
      const int64_t o = (int64_t)y * G.pc;
      const int rnd = odd ? 2 : 1;
      cb = (3 * G.cbp[o + i] + G.cbp[o + nbr] + rnd) >> 2;
      cr = (3 * G.crp[o + i] + G.crp[o + nbr] + rnd) >> 2;
    } else {
      const int rr = y >> 1;
      const int far = (y & 1) ? min(rr + 1, G.dh - 1) : max(rr - 1, 0);
      const int64_t on = (int64_t)rr * G.pc, of = (int64_t)far * G.pc;
      const int rnd = odd ? 7 : 8;
      cb = (3 * (3 * G.cbp[on + i] + G.cbp[of + i]) + (3 * G.cbp[on + nbr] + G.cbp[of + nbr]) + rnd) >> 4;
      cr = (3 * (3 * G.crp[on + i] + G.crp[of + i]) + (3 * G.crp[on + nbr] + G.crp[of + nbr]) + rnd) >> 4;
    }
  }
  cb -= 128;
  cr -= 128;
  r = clamp255(Y + ((91881 * cr + 32768) >> 16));
  g = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  b = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

// grid (256 x 16 output bytes, image).  The image is height * width * 3 contiguous bytes at bank_offset; a thread owns one
// ALIGNED 16-byte word of the bank, computes the (up to 6) pixels whose bytes fall into it and stores the word whole; the
// words that straddle the image's first or last byte are stored byte by byte (the neighbours belong to other images).
__global__ void __launch_bounds__(256)
k_jpeg_rgb(const fdet_jpeg_desc* __restrict__ descs, const uint8_t* __restrict__ ws, uint8_t* __restrict__ bank) {
  const fdet_jpeg_desc* D = descs + blockIdx.y;
  const int W = D->width, H = D->height;
  const int64_t off = D->bank_offset;
  const int nbytes = W * H * 3;
  const int head = (int)(off & 15);
  const int64_t word = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t k0l = word * 16 - head;                  // image byte index of the word's first byte
  if (k0l >= nbytes) return;
  const int k0 = (int)k0l;
  const int ka = max(k0, 0), kb = min(k0 + 16, nbytes);
  RgbGeom G;
  G.W = W; G.H = H;
  G.py = D->blocks_w[0] * 8;
  G.yp = ws + D->plane_offset[0];
  if (D->ncomp == 1) {
    G.mode = 0; G.cbp = G.crp = G.yp; G.pc = G.py; G.vshift = 0; G.dw = W; G.dh = H;
  } else {
    const int hs = D->hs, vs = D->vs;
    G.pc = D->blocks_w[1] * 8;
    G.cbp = ws + D->plane_offset[1];
    G.crp = ws + D->plane_offset[2];
    G.dw = (W + hs - 1) / hs;
    G.dh = (H + vs - 1) / vs;
    G.vshift = vs - 1;
    G.mode = hs == 1 ? 1 : G.dw <= 2 ? 2 : vs == 1 ? 3 : 4;
  }
  int p = ka / 3;
  int ch = ka - p * 3;
  int y = p / W, x = p - y * W;
  uint64_t lo = 0, hi = 0;
  int k = ka;
#pragma unroll 1
  while (k < kb) {
    uint32_t rgb[3];
    jpeg_pixel(G, x, y, rgb[0], rgb[1], rgb[2]);
    const uint32_t px = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
    for (; ch < 3 && k < kb; ++ch, ++k) {
      const int at = k - k0;
      const uint64_t v = (uint64_t)((px >> (8 * ch)) & 255u);
      if (at < 8) lo |= v << (8 * at);
      else hi |= v << (8 * (at - 8));
    }
    ch = 0;
    if (++x == W) { x = 0; ++y; }
  }
  uint8_t* dst = bank + off + k0l;                       // 16-byte aligned
  if (ka == k0 && kb == k0 + 16) {
    *reinterpret_cast<uint4*>(dst) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
  } else {
    for (int at = ka - k0; at < kb - k0; ++at) dst[at] = (uint8_t)((at < 8 ? lo >> (8 * at) : hi >> (8 * (at - 8))) & 255u);
  }
}

}  // namespace

extern "C" int fdet_jpeg_reconstruct(const int16_t* coef, size_t coef_count, const fdet_jpeg_desc* descs,
                                     const fdet_jpeg_desc* h_descs, int n_images, uint8_t* workspace, size_t workspace_bytes,
                                     uint8_t* bank, size_t bank_bytes, void* stream) {
  FDET_REQUIRE(coef && descs && h_descs && workspace && bank, "jpeg_reconstruct: null pointer");
  FDET_REQUIRE(n_images > 0 && n_images <= 65535 && coef_count > 0 && workspace_bytes > 0 && bank_bytes > 0,
               "jpeg_reconstruct: bad sizes n_images=%d (1..65535) coef_count=%zu workspace_bytes=%zu bank_bytes=%zu", n_images,
               coef_count, workspace_bytes, bank_bytes);
  FDET_REQUIRE(((uintptr_t)coef % 16) == 0 && ((uintptr_t)workspace % 8) == 0 && ((uintptr_t)bank % 16) == 0,
               "jpeg_reconstruct: coef and bank must be 16-byte aligned, workspace 8-byte aligned");
  int64_t max_groups = 0, max_words = 0;
  for (int i = 0; i < n_images; ++i) {
    const fdet_jpeg_desc& I = h_descs[i];
    FDET_REQUIRE(I.width > 0 && I.height > 0 && I.width <= 65535 && I.height <= 65535 &&
                     (int64_t)I.width * I.height * 3 <= 0x7fffffffLL,
                 "jpeg_reconstruct: image %d: bad size %dx%d", i, I.width, I.height);
    FDET_REQUIRE((I.ncomp == 1 && I.hs == 1 && I.vs == 1) ||
                     (I.ncomp == 3 && ((I.hs == 1 && I.vs == 1) || (I.hs == 2 && I.vs == 1) || (I.hs == 2 && I.vs == 2))),
                 "jpeg_reconstruct: image %d: %d components with luma sampling %dx%d is outside the supported set", i, I.ncomp,
                 I.hs, I.vs);
    int64_t groups = 0;
    for (int c = 0; c < I.ncomp; ++c) {
      const int sh = c == 0 ? 1 : I.hs, sv = c == 0 ? 1 : I.vs;
      const int need_w = (I.width + sh - 1) / sh, need_h = (I.height + sv - 1) / sv;
      FDET_REQUIRE(I.blocks_w[c] > 0 && I.blocks_h[c] > 0 && I.blocks_w[c] <= 8192 && I.blocks_h[c] <= 8192 &&
                       (int64_t)I.blocks_w[c] * 8 >= need_w && (int64_t)I.blocks_h[c] * 8 >= need_h,
                   "jpeg_reconstruct: image %d: the %dx%d blocks of component %d do not cover its %dx%d samples", i,
                   I.blocks_w[c], I.blocks_h[c], c, need_w, need_h);
      const int64_t nb = (int64_t)I.blocks_w[c] * I.blocks_h[c];
      FDET_REQUIRE(I.coef_offset[c] >= 0 && (I.coef_offset[c] % 8) == 0 &&
                       (uint64_t)(I.coef_offset[c] + nb * 64) <= (uint64_t)coef_count,
                   "jpeg_reconstruct: image %d: coefficient plane %d at %lld (+%lld) is misaligned or past the %zu given", i, c,
                   (long long)I.coef_offset[c], (long long)(nb * 64), coef_count);
      FDET_REQUIRE(I.plane_offset[c] >= 0 && (I.plane_offset[c] % 8) == 0 &&
                       (uint64_t)(I.plane_offset[c] + nb * 64) <= (uint64_t)workspace_bytes,
                   "jpeg_reconstruct: image %d: sample plane %d at %lld (+%lld) is misaligned or past the workspace of %zu bytes",
                   i, c, (long long)I.plane_offset[c], (long long)(nb * 64), workspace_bytes);
      groups += (nb + 7) / 8;
    }
    const int64_t nbytes = (int64_t)I.width * I.height * 3;
    FDET_REQUIRE(I.bank_offset >= 0 && (uint64_t)(I.bank_offset + nbytes) <= (uint64_t)bank_bytes,
                 "jpeg_reconstruct: image %d: %lld bytes at offset %lld run past the bank of %zu bytes", i, (long long)nbytes,
                 (long long)I.bank_offset, bank_bytes);
    const int64_t words = ((I.bank_offset & 15) + nbytes + 15) / 16;
    max_groups = groups > max_groups ? groups : max_groups;
    max_words = words > max_words ? words : max_words;
  }
  const dim3 g1((unsigned)((max_groups + IDCT_WAVES - 1) / IDCT_WAVES), (unsigned)n_images);
  hipLaunchKernelGGL(k_jpeg_idct, g1, dim3(256), 0, (hipStream_t)stream, coef, descs, workspace);
  if (int rc = check_launch("fdet_jpeg_reconstruct (idct)")) return rc;
  const dim3 g2((unsigned)((max_words + 255) / 256), (unsigned)n_images);
  hipLaunchKernelGGL(k_jpeg_rgb, g2, dim3(256), 0, (hipStream_t)stream, descs, workspace, bank);
  return check_launch("fdet_jpeg_reconstruct (rgb)");
}
