// Host side of the baseline JPEG decoder: marker parser and Huffman (entropy) decoder.  Plain C++17 with no HIP
// dependency, so that a stand-alone program (tools/jpeg_host_check.cpp) can run it under a host sanitizer; jpeg.hip
// wraps the two functions below as glsdet_jpeg_parse / glsdet_jpeg_entropy_decode.
//
// Accepted: SOF0 (baseline, 8 bit, Huffman), one interleaved scan, grayscale (1x1) or three components with luma 1x1 /
// 2x1 / 2x2 and 1x1 chroma; DQT with 8-bit entries, DHT, DRI, RSTn, APPn, COM.  Everything else is refused with a
// negative code and a message that names the reason.  Every read of `data` goes through Reader / BitReader, which
// compare the position against nbytes first; every write of `coef` is to block < n_blocks, index < 64.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/glsdet_hip.h"

namespace glsdet_jpeg {

enum { E_ARG = -1 };          // = GLSDET_E_ARG
static const int64_t MAX_PIXELS = (int64_t)1 << 28;

static const unsigned char ZIGZAG[64] = {   // natural (row-major) index of the k-th coefficient in scan order
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Err {
  char* buf;
  size_t cap;
  int fail(const char* fmt, ...) const {
    if (buf && cap) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(buf, cap, fmt, ap);
      va_end(ap);
    }
    return E_ARG;
  }
};

struct HuffTable {
  bool defined = false;
  unsigned char counts[17];   // codes of length 1..16
  unsigned char symbols[256];
  int nsym = 0;
  // derived
  int32_t maxcode[18];        // largest code of length l, -1 if none; maxcode[17] is a sentinel above every code
  int32_t valptr[17];         // symbols[] index of the first code of length l, minus that code
  uint16_t look[512];         // 9-bit prefix -> (length << 8) | symbol, 0 when the code is longer than 9 bits
};

// The tables and frame fields gathered by one pass over the markers.
struct Parsed {
  glsdet_jpeg_desc d;
  uint16_t q[4][64];          // natural order
  bool q_defined[4];
  HuffTable dc[4], ac[4];
};

struct Reader {
  const unsigned char* p;
  int64_t n, pos;
  bool has(int64_t k) const { return k >= 0 && pos <= n - k; }
  int u8() { return p[pos++]; }                       // callers check has() first
  int u16() {
    int v = (p[pos] << 8) | p[pos + 1];
    pos += 2;
    return v;
  }
};

// code lengths must describe a prefix code (libjpeg: jpeg_make_d_derived_tbl)
inline int derive(HuffTable& t, const Err& e, const char* what, int id) {
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t.valptr[l] = k - code;
    k += t.counts[l];
    code += t.counts[l];
    if (code > (1 << l)) return e.fail("jpeg: DHT %s table %d: the code lengths are no prefix code", what, id);
    t.maxcode[l] = t.counts[l] ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  memset(t.look, 0, sizeof t.look);
  code = 0;
  k = 0;
  for (int l = 1; l <= 9; ++l) {
    for (int i = 0; i < t.counts[l]; ++i, ++k, ++code) {
      const int lo = code << (9 - l);
      for (int f = 0; f < (1 << (9 - l)); ++f) t.look[lo + f] = (uint16_t)((l << 8) | t.symbols[k]);
    }
    code <<= 1;
  }
  return 0;
}

inline int parse_dht(Reader& r, int64_t end, Parsed& P, const Err& e) {
  while (r.pos < end) {
    if (end - r.pos < 17) return e.fail("jpeg: DHT segment too short");
    const int tcth = r.u8(), tc = tcth >> 4, th = tcth & 15;
    if (tc > 1 || th > 3) return e.fail("jpeg: DHT with class %d / id %d (baseline allows class 0..1, id 0..3)", tc, th);
    HuffTable& t = tc ? P.ac[th] : P.dc[th];
    int total = 0;
    t.counts[0] = 0;
    for (int l = 1; l <= 16; ++l) total += (t.counts[l] = (unsigned char)r.u8());
    if (total > 256 || end - r.pos < total) return e.fail("jpeg: DHT table holds %d symbols, its segment fewer bytes", total);
    for (int i = 0; i < total; ++i) t.symbols[i] = (unsigned char)r.u8();
    t.nsym = total;
    t.defined = false;
    int rc = derive(t, e, tc ? "AC" : "DC", th);
    if (rc) return rc;
    t.defined = true;
  }
  return 0;
}

inline int parse_dqt(Reader& r, int64_t end, Parsed& P, const Err& e) {
  while (r.pos < end) {
    const int pqtq = r.u8(), pq = pqtq >> 4, tq = pqtq & 15;
    if (pq == 1) return e.fail("jpeg: DQT with 16-bit entries is not supported");
    if (pq > 1 || tq > 3) return e.fail("jpeg: DQT with precision %d / id %d", pq, tq);
    if (end - r.pos < 64) return e.fail("jpeg: DQT segment too short");
    for (int k = 0; k < 64; ++k) P.q[tq][ZIGZAG[k]] = (uint16_t)r.u8();
    P.q_defined[tq] = true;
  }
  return 0;
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Fills the geometry of d from width / height / ncomp / hs / vs; refuses every layout the kernels do not take.
inline int layout(glsdet_jpeg_desc& d, const Err& e) {
  if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535)
    return e.fail("jpeg: bad picture size %d x %d", d.width, d.height);
  if ((int64_t)d.width * d.height > MAX_PIXELS) return e.fail("jpeg: %d x %d is more than 2^28 pixels", d.width, d.height);
  if (d.ncomp == 1) {
    if (d.hs[0] != 1 || d.vs[0] != 1) return e.fail("jpeg: grayscale with sampling %dx%d is not supported", d.hs[0], d.vs[0]);
    d.hs[1] = d.hs[2] = d.vs[1] = d.vs[2] = 0;
  } else if (d.ncomp == 3) {
    const bool luma = (d.hs[0] == 1 && d.vs[0] == 1) || (d.hs[0] == 2 && d.vs[0] == 1) || (d.hs[0] == 2 && d.vs[0] == 2);
    if (!luma || d.hs[1] != 1 || d.vs[1] != 1 || d.hs[2] != 1 || d.vs[2] != 1)
      return e.fail("jpeg: sampling factors %dx%d,%dx%d,%dx%d are not supported (4:4:4, 4:2:2 and 4:2:0 are)", d.hs[0], d.vs[0],
                    d.hs[1], d.vs[1], d.hs[2], d.vs[2]);
  } else {
    return e.fail("jpeg: %d components are not supported (1 or 3 are)", d.ncomp);
  }
  d.mcus_x = ceil_div(d.width, 8 * d.hs[0]);
  d.mcus_y = ceil_div(d.height, 8 * d.vs[0]);
  d.n_blocks = 0;
  for (int c = 0; c < 3; ++c) {
    d.blocks_x[c] = c < d.ncomp ? d.mcus_x * d.hs[c] : 0;
    d.blocks_y[c] = c < d.ncomp ? d.mcus_y * d.vs[c] : 0;
    d.n_blocks += (int64_t)d.blocks_x[c] * d.blocks_y[c];
  }
  return 0;
}

inline int parse(const unsigned char* data, int64_t nbytes, Parsed& P, const Err& e) {
  if (!data || nbytes < 0) return e.fail("jpeg: null data");
  memset(&P.d, 0, sizeof P.d);
  memset(P.q_defined, 0, sizeof P.q_defined);
  memset(P.q, 0, sizeof P.q);
  Reader r{data, nbytes, 0};
  if (!r.has(2) || r.u8() != 0xFF || r.u8() != 0xD8) return e.fail("jpeg: no SOI marker: not a JPEG stream");
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1, ids[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
  for (;;) {
    // next marker: FF, any number of fill FFs, the code
    if (!r.has(2)) return e.fail("jpeg: data ends before the scan (SOS)");
    if (r.u8() != 0xFF) return e.fail("jpeg: byte %lld is no marker", (long long)(r.pos - 1));
    int m = r.u8();
    while (m == 0xFF) {
      if (!r.has(1)) return e.fail("jpeg: data ends before the scan (SOS)");
      m = r.u8();
    }
    if (m == 0xD8 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7))
      return e.fail("jpeg: marker FF%02X before the scan", m);
    if (m == 0xD9) return e.fail("jpeg: EOI before the scan");
    if (!r.has(2)) return e.fail("jpeg: data ends inside the FF%02X segment", m);
    const int len = r.u16();
    if (len < 2 || !r.has(len - 2)) return e.fail("jpeg: the FF%02X segment (length %d) reaches past the data", m, len);
    const int64_t end = r.pos + len - 2;
    int rc = 0;
    if (m == 0xC0) {
      if (sof) return e.fail("jpeg: a second SOF marker");
      if (len < 8) return e.fail("jpeg: SOF0 segment too short");
      const int prec = r.u8();
      P.d.height = r.u16();
      P.d.width = r.u16();
      P.d.ncomp = r.u8();
      if (prec != 8) return e.fail("jpeg: %d-bit samples are not supported (8-bit baseline is)", prec);
      if (P.d.height == 0) return e.fail("jpeg: height 0 (the height would come from a DNL marker): not supported");
      if (P.d.ncomp != 1 && P.d.ncomp != 3) return e.fail("jpeg: %d components are not supported (1 or 3 are)", P.d.ncomp);
      if (len != 8 + 3 * P.d.ncomp) return e.fail("jpeg: SOF0 length %d does not fit %d components", len, P.d.ncomp);
      for (int c = 0; c < P.d.ncomp; ++c) {
        ids[c] = r.u8();
        const int hv = r.u8();
        P.d.hs[c] = hv >> 4;
        P.d.vs[c] = hv & 15;
        tq[c] = r.u8();
        if (tq[c] > 3) return e.fail("jpeg: component %d selects quantisation table %d", c, tq[c]);
        for (int k = 0; k < c; ++k)
          if (ids[k] == ids[c]) return e.fail("jpeg: two components share the id %d", ids[c]);
      }
      if ((rc = layout(P.d, e))) return rc;
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      static const char* const kind[16] = {"", "extended sequential (SOF1)", "progressive (SOF2)", "lossless (SOF3)", "",
                                           "differential (SOF5)", "differential progressive (SOF6)", "differential lossless (SOF7)",
                                           "", "arithmetic-coded (SOF9)", "arithmetic-coded progressive (SOF10)",
                                           "arithmetic-coded lossless (SOF11)", "", "arithmetic-coded differential (SOF13)",
                                           "arithmetic-coded differential (SOF14)", "arithmetic-coded differential (SOF15)"};
      return e.fail("jpeg: %s streams are not supported (baseline SOF0 is)", kind[m & 15]);
    } else if (m == 0xCC) {
      return e.fail("jpeg: arithmetic coding (DAC) is not supported");
    } else if (m == 0xC4) {
      rc = parse_dht(r, end, P, e);
    } else if (m == 0xDB) {
      rc = parse_dqt(r, end, P, e);
    } else if (m == 0xDD) {
      if (len != 4) return e.fail("jpeg: DRI segment of length %d", len);
      P.d.restart_interval = r.u16();
    } else if (m == 0xDC) {
      return e.fail("jpeg: DNL marker is not supported");
    } else if (m == 0xE0) {               // JFIF: the components are YCbCr whatever their ids
      if (len - 2 >= 14 && !memcmp(data + r.pos, "JFIF\0", 5)) jfif = true;
    } else if (m == 0xEE) {               // Adobe: transform 0 = RGB (3 components), 1 = YCbCr
      if (len - 2 >= 12 && !memcmp(data + r.pos, "Adobe", 5)) {
        adobe = true;
        adobe_transform = data[r.pos + 11];
      }
    } else if (m == 0xDA) {
      if (!sof) return e.fail("jpeg: SOS before SOF");
      if (len < 3) return e.fail("jpeg: SOS segment too short");
      const int ns = r.u8();
      if (ns != P.d.ncomp)
        return e.fail("jpeg: a scan of %d of the %d components: several scans are not supported", ns, P.d.ncomp);
      if (len != 6 + 2 * ns) return e.fail("jpeg: SOS length %d does not fit %d components", len, ns);
      for (int c = 0; c < ns; ++c) {
        const int id = r.u8(), tdta = r.u8();
        if (id != ids[c]) return e.fail("jpeg: the scan lists component id %d where the frame has %d", id, ids[c]);
        P.d.td[c] = tdta >> 4;
        P.d.ta[c] = tdta & 15;
        P.d.tq[c] = tq[c];
        if (P.d.td[c] > 3 || P.d.ta[c] > 3) return e.fail("jpeg: component %d selects Huffman tables %d / %d", c, P.d.td[c], P.d.ta[c]);
        if (!P.q_defined[tq[c]]) return e.fail("jpeg: component %d selects quantisation table %d, which no DQT defines", c, tq[c]);
        if (!P.dc[P.d.td[c]].defined) return e.fail("jpeg: component %d selects DC Huffman table %d, which no DHT defines", c, P.d.td[c]);
        if (!P.ac[P.d.ta[c]].defined) return e.fail("jpeg: component %d selects AC Huffman table %d, which no DHT defines", c, P.d.ta[c]);
        const HuffTable& t = P.dc[P.d.td[c]];
        for (int i = 0; i < t.nsym; ++i)
          if (t.symbols[i] > 15) return e.fail("jpeg: DC Huffman table %d holds the category %d", P.d.td[c], t.symbols[i]);
      }
      // colour space as libjpeg picks it: JFIF -> YCbCr; Adobe -> by transform; else by the component ids
      if (P.d.ncomp == 3) {
        if (!jfif && adobe && adobe_transform != 1)
          return e.fail("jpeg: Adobe APP14 marker with transform %d: the components are not YCbCr", adobe_transform);
        if (!jfif && !adobe && ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B')
          return e.fail("jpeg: component ids 'R','G','B' without a JFIF marker: the components are RGB, not YCbCr");
      }
      P.d.scan_offset = end;             // Ss, Se, Ah/Al are ignored as libjpeg's sequential decoder ignores them
      return 0;
    }
    if (rc) return rc;
    r.pos = end;                         // APPn, COM and anything unknown are skipped by their length
  }
}

// Bits of the entropy-coded segment: FF 00 is a data FF, fill FFs before a marker are skipped, and a marker or the end
// of the data stops the supply -- a caller that then needs more bits than are left has a truncated stream.
struct BitReader {
  const unsigned char* p;
  int64_t n, pos;
  uint64_t acc = 0;
  int nbits = 0;
  bool stopped = false;
  void fill() {
    while (nbits <= 56 && !stopped) {
      if (pos >= n) {
        stopped = true;
        break;
      }
      int b = p[pos];
      if (b == 0xFF) {
        int64_t q = pos + 1;
        while (q < n && p[q] == 0xFF) ++q;
        if (q >= n || p[q] != 0x00) {    // a marker (or the end): leave pos on its first FF
          stopped = true;
          break;
        }
        pos = q + 1;
      } else {
        ++pos;
      }
      acc = (acc << 8) | (uint64_t)b;
      nbits += 8;
    }
  }
  // next k (1..16) bits, zero padded past the end of the supply
  int peek(int k) {
    if (nbits < k) fill();
    if (nbits >= k) return (int)((acc >> (nbits - k)) & ((1u << k) - 1));
    return (int)((acc << (k - nbits)) & ((1u << k) - 1));
  }
  bool skip(int k) {
    if (k > nbits) return false;
    nbits -= k;
    return true;
  }
  void restart() {
    acc = 0;
    nbits = 0;
    stopped = false;
  }
};

// -> symbol, -1 truncated, -2 no such code
inline int decode_symbol(BitReader& br, const HuffTable& t) {
  const int v = br.peek(16);
  const int e = t.look[v >> 7];
  if (e) return br.skip(e >> 8) ? (e & 255) : -1;
  int l = 10, code = 0;
  for (; l <= 16; ++l) {
    code = v >> (16 - l);
    if (code <= t.maxcode[l]) break;
  }
  if (l > 16) return br.nbits < 16 ? -1 : -2;
  if (!br.skip(l)) return -1;
  return t.symbols[(code + t.valptr[l]) & 255];
}

// s magnitude bits -> value (libjpeg HUFF_EXTEND); -> false when the stream is truncated
inline bool receive_extend(BitReader& br, int s, int& out) {
  const int v = br.peek(s);
  if (!br.skip(s)) return false;
  out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
  return true;
}

// coef: n_blocks * 64 int16, component by component, block raster, natural order, not dequantised.
// qtab: [3][64] uint16 per component, natural order (rows of absent components are zero).
inline int entropy_decode(const unsigned char* data, int64_t nbytes, const glsdet_jpeg_desc* d, int16_t* coef, uint16_t* qtab,
                          const Err& e) {
  if (!data || !d || !coef || !qtab) return e.fail("jpeg_entropy_decode: null argument");
  static thread_local Parsed P;
  int rc = parse(data, nbytes, P, e);
  if (rc) return rc;
  if (memcmp(&P.d, d, sizeof P.d)) return e.fail("jpeg_entropy_decode: the descriptor is not the one glsdet_jpeg_parse gives for this stream");
  const glsdet_jpeg_desc& D = P.d;
  memset(coef, 0, (size_t)D.n_blocks * 64 * sizeof(int16_t));
  memset(qtab, 0, 3 * 64 * sizeof(uint16_t));
  int64_t base[3] = {0, 0, 0};
  for (int c = 0; c < D.ncomp; ++c) {
    memcpy(qtab + 64 * c, P.q[D.tq[c]], 64 * sizeof(uint16_t));
    if (c) base[c] = base[c - 1] + (int64_t)D.blocks_x[c - 1] * D.blocks_y[c - 1];
  }
  BitReader br{data, nbytes, D.scan_offset};
  int pred[3] = {0, 0, 0};
  const int64_t n_mcu = (int64_t)D.mcus_x * D.mcus_y;
  int next_rst = 0;
  for (int64_t mcu = 0; mcu < n_mcu; ++mcu) {
    if (D.restart_interval && mcu && mcu % D.restart_interval == 0) {
      // only the padding bits of the last data byte may precede the marker
      if (br.nbits >= 8) return e.fail("jpeg: missing RST%d marker before MCU %lld (data where the marker belongs)", next_rst, (long long)mcu);
      br.restart();
      int64_t q = br.pos;
      while (q < nbytes && data[q] == 0xFF) ++q;
      if (q == br.pos || q >= nbytes)
        return e.fail("jpeg: missing RST%d marker before MCU %lld", next_rst, (long long)mcu);
      if (data[q] != 0xD0 + next_rst)
        return e.fail("jpeg: missing or out-of-order restart marker before MCU %lld: expected RST%d, found FF%02X", (long long)mcu,
                      next_rst, data[q]);
      br.pos = q + 1;
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int my = (int)(mcu / D.mcus_x), mx = (int)(mcu % D.mcus_x);
    for (int c = 0; c < D.ncomp; ++c) {
      const HuffTable& tdc = P.dc[D.td[c]];
      const HuffTable& tac = P.ac[D.ta[c]];
      for (int v = 0; v < D.vs[c]; ++v)
        for (int h = 0; h < D.hs[c]; ++h) {
          const int64_t blk = base[c] + (int64_t)(my * D.vs[c] + v) * D.blocks_x[c] + (mx * D.hs[c] + h);
          int16_t* out = coef + blk * 64;
          int s = decode_symbol(br, tdc);
          if (s == -1) return e.fail("jpeg: the data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcu);
          if (s < 0) return e.fail("jpeg: a Huffman code that is in no table (DC, MCU %lld)", (long long)mcu);
          int diff = 0;
          if (s && !receive_extend(br, s, diff))
            return e.fail("jpeg: the data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcu);
          pred[c] += diff;
          if (pred[c] < -2048 || pred[c] > 2047)
            return e.fail("jpeg: a quantised DC coefficient of %d is outside [-2048, 2047] (MCU %lld)", pred[c], (long long)mcu);
          out[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            const int rs = decode_symbol(br, tac);
            if (rs == -1) return e.fail("jpeg: the data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcu);
            if (rs < 0) return e.fail("jpeg: a Huffman code that is in no table (AC, MCU %lld)", (long long)mcu);
            const int run = rs >> 4, sz = rs & 15;
            if (sz == 0) {
              if (run != 15) break;       // EOB
              k += 16;                    // ZRL
              if (k > 64) return e.fail("jpeg: a zero run past coefficient 63 (MCU %lld)", (long long)mcu);
              continue;
            }
            k += run;
            if (k > 63) return e.fail("jpeg: a zero run past coefficient 63 (MCU %lld)", (long long)mcu);
            int val = 0;
            if (!receive_extend(br, sz, val))
              return e.fail("jpeg: the data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcu);
            if (val < -2048 || val > 2047)
              return e.fail("jpeg: a quantised AC coefficient of %d is outside [-2048, 2047] (MCU %lld)", val, (long long)mcu);
            out[ZIGZAG[k]] = (int16_t)val;
            ++k;
          }
        }
    }
  }
  // after the last MCU: padding bits, then EOI.  Anything else is either a further scan or a cut stream.
  if (br.nbits >= 8) return e.fail("jpeg: data after the last MCU where the EOI marker belongs");
  int64_t q = br.pos;
  while (q < nbytes && data[q] == 0xFF) ++q;
  if (q == br.pos || q >= nbytes) return e.fail("jpeg: the data ends before the EOI marker");
  if (data[q] != 0xD9)
    return e.fail("jpeg: marker FF%02X after the scan where EOI belongs: several scans are not supported", data[q]);
  return 0;
}

}  // namespace glsdet_jpeg
