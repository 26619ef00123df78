// Baseline JPEG -> 8-bit RGB, host side.  The colour images of compressed .klg logs and compressed eflcm::Frame messages
// are JPEG (Logger2 / the LCM publishers encode with OpenCV = libjpeg); the reference decodes them with libjpeg's defaults
// through GUI/src/Tools/JPEGLoader.h:44-95 (jpeg_read_header / jpeg_start_decompress / jpeg_read_scanlines, then an R<->B
// swap per pixel).  libjpeg's headers are not in this image, so this is a from-scratch decoder of the same published
// algorithms, written to give libjpeg's BYTES for the streams those encoders produce (sequential DCT, Huffman, 8 bit,
// Y Cb Cr with 4:4:4, 4:2:2 or 4:2:0 sampling, optional restart intervals):
//   * dequantisation + the "slow" integer inverse DCT (Loeffler-Ligtenberg-Moschytz, 13-bit constants, 2 extra bits after
//     the column pass: libjpeg's JDCT_ISLOW, its default),
//   * "fancy" chroma upsampling, libjpeg's default (triangle filter: 3/4 nearer + 1/4 further sample, the two roundings
//     alternating; 9/16, 3/16, 3/16, 1/16 for 4:2:0; edge rows / columns replicated),
//   * the 16-bit fixed-point Y Cb Cr -> RGB tables (1.402, 1.772, 0.71414, 0.34414).
// Pinned by tests/golden/jpeg_cases.npz: streams encoded and decoded by Pillow's bundled libjpeg-turbo in this image
// (tests/golden/make_jpeg_golden.py); every pixel must match.  Progressive, arithmetic-coded, 12-bit, CMYK / greyscale
// streams are reported as unsupported (the reference's loader would mis-handle the last two itself: it assumes 3 bytes
// per pixel).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jpeg_core.hpp"

// The decoder is three stages over plain data (the per-block and per-pixel arithmetic is csrc/jpeg_core.hpp, shared with the
// device decoder of csrc/jpeg_dev.hip):
//   parse      markers -> tables, frame and scan headers, Geometry, the offset of the entropy-coded data, the restart interval
//   entropy    the entropy-coded data -> quantised coefficients: int16, 64 per block in natural order, blocks in the scan's MCU
//              order, DC values already summed
//   back half  coefficients -> RGB: dequantisation + inverse DCT into the component planes, upsampling + colour conversion
namespace dms {
namespace jpeg {

struct Component {
  int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
  int pred = 0;
};

struct Decoder {
  const unsigned char* p = nullptr;
  const unsigned char* end = nullptr;
  unsigned long long bitbuf = 0;
  int bits = 0;
  bool hit_marker = false;
  const char* err = nullptr;
  int unsupported = 0;

  unsigned short qt[4][64] = {};
  bool qt_present[4] = {};
  Huff dc[4] = {}, ac[4] = {};
  bool dc_present[4] = {}, ac_present[4] = {};
  Component comp[3];
  int ncomp = 0, width = 0, height = 0, restart_interval = 0;
  Geometry geo = {};
  long blocks_done = 0;  // blocks the entropy stage completed (all of them, or those before the one it refused)

  bool fail(const char* what) {
    if (!err) err = what;
    return false;
  }
  bool nosupport(const char* what) {
    unsupported = 1;
    return fail(what);
  }

  // ---- entropy-coded segment: bit reader with byte unstuffing; a marker ends the data (zero bits are supplied, as libjpeg does)
  void fill() {
    while (bits <= 56) {
      unsigned c = 0;
      if (!hit_marker && p < end) {
        c = *p++;
        if (c == 0xFF) {
          if (p < end && *p == 0x00) {
            ++p;
          } else {  // a marker: leave it for the caller
            --p;
            hit_marker = true;
            c = 0;
          }
        }
      } else {
        hit_marker = true;
      }
      bitbuf |= (unsigned long long)c << (56 - bits);
      bits += 8;
    }
  }
  int peek(int n) {
    if (bits < n) fill();
    return (int)(bitbuf >> (64 - n));
  }
  void skip(int n) {
    bitbuf <<= n;
    bits -= n;
  }
  int get(int n) {
    if (n == 0) return 0;
    const int v = peek(n);
    skip(n);
    return v;
  }
  bool build(Huff& h, bool& present, const unsigned char* counts, const unsigned char* vals, int nvals) {
    int code = 0, k = 0;
    memset(h.look, 0, sizeof(h.look));
    for (int l = 1; l <= 16; ++l) {
      h.valptr[l] = k;
      h.mincode[l] = code;
      for (int i = 0; i < counts[l - 1]; ++i) {
        if (k >= nvals || code >= (1 << l)) return fail("bad Huffman table");
        if (l <= 9) {
          const int base = code << (9 - l);
          for (int f = 0; f < (1 << (9 - l)); ++f) h.look[base + f] = (unsigned short)((l << 8) | vals[k]);
        }
        ++code;
        ++k;
      }
      h.maxcode[l] = counts[l - 1] ? code - 1 : -1;
      if (code > (1 << l)) return fail("bad Huffman table");
      code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    memset(h.vals, 0, sizeof(h.vals));
    memcpy(h.vals, vals, (size_t)nvals);
    present = true;
    return true;
  }
  int decode_symbol(const Huff& h) {
    int len;
    const int s = huff_symbol(h, (unsigned)peek(16), &len);
    skip(len);
    if (s < 0) {
      fail(block_error_text(kErrBadCode));
      return 0;
    }
    return s;
  }

  // ---- entropy stage: one 8x8 block -> 64 coefficients in natural order (coef is zeroed by the caller)
  bool decode_block(Component& c, short* coef) {
    const int s = decode_symbol(dc[c.td]);
    if (s > 15) return fail(block_error_text(kErrBadDcSize));
    if (s) c.pred += extend(get(s), s);
    coef[0] = (short)c.pred;
    for (int k = 1; k < 64;) {
      const int rs = decode_symbol(ac[c.ta]);
      const int r = rs >> 4, sz = rs & 15;
      if (sz == 0) {
        if (r != 15) break;
        k += 16;
        continue;
      }
      k += r;
      if (k > 63) return fail(block_error_text(kErrAcRun));
      coef[zigzag(k)] = (short)extend(get(sz), sz);
      ++k;
    }
    return !err;
  }

  // ---- markers
  static unsigned be16(const unsigned char* q) { return (unsigned)q[0] << 8 | q[1]; }

  bool parse_tables_and_scan(int& got_scan) {
    got_scan = 0;
    for (;;) {
      if (end - p < 4) return fail("truncated stream");
      if (p[0] != 0xFF) return fail("marker expected");
      while (p < end && *p == 0xFF) ++p;
      if (p >= end) return fail("truncated stream");
      const unsigned m = *p++;
      if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
      if (m == 0xD9) return fail("end of image before a scan");
      if (end - p < 2) return fail("truncated segment");
      const unsigned len = be16(p);
      if (len < 2 || (size_t)(end - p) < len) return fail("truncated segment");
      const unsigned char* s = p + 2;
      const unsigned char* se = p + len;
      p += len;
      if (m == 0xDB) {  // DQT
        while (s < se) {
          const int pq = s[0] >> 4, tq = s[0] & 15;
          ++s;
          if (tq > 3 || pq > 1 || se - s < 64 * (pq + 1)) return fail("bad quantisation table");
          static const unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
          for (int i = 0; i < 64; ++i) {
            qt[tq][zz[i]] = (unsigned short)(pq ? be16(s) : s[0]);
            s += pq + 1;
          }
          qt_present[tq] = true;
        }
      } else if (m == 0xC4) {  // DHT
        while (s < se) {
          if (se - s < 17) return fail("bad Huffman segment");
          const int tc = s[0] >> 4, th = s[0] & 15;
          int n = 0;
          for (int i = 0; i < 16; ++i) n += s[1 + i];
          if (tc > 1 || th > 3 || n > 256 || se - s < 17 + n) return fail("bad Huffman segment");
          if (!build(tc ? ac[th] : dc[th], tc ? ac_present[th] : dc_present[th], s + 1, s + 17, n)) return false;
          s += 17 + n;
        }
      } else if (m == 0xC0 || m == 0xC1) {  // SOF0 / SOF1: sequential, Huffman
        if (se - s < 6) return fail("bad frame header");
        if (s[0] != 8) return nosupport("sample precision other than 8 bits");
        height = (int)be16(s + 1);
        width = (int)be16(s + 3);
        ncomp = s[5];
        if (ncomp != 3) return nosupport("not a three-component (Y Cb Cr) image");
        if (se - s < 6 + 3 * ncomp) return fail("bad frame header");
        for (int i = 0; i < ncomp; ++i) {
          comp[i].id = s[6 + 3 * i];
          comp[i].h = s[7 + 3 * i] >> 4;
          comp[i].v = s[7 + 3 * i] & 15;
          comp[i].tq = s[8 + 3 * i];
          if (comp[i].tq > 3) return fail("bad frame header");
        }
      } else if (m == 0xC2 || (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC)) {
        return nosupport("progressive / lossless / arithmetic-coded JPEG");
      } else if (m == 0xDD) {  // DRI
        if (se - s < 2) return fail("bad restart interval");
        restart_interval = (int)be16(s);
      } else if (m == 0xDA) {  // SOS
        if (!ncomp) return fail("scan before the frame header");
        if (se - s < 1 || s[0] != ncomp || se - s < 1 + 2 * ncomp + 3) return nosupport("non-interleaved scan");
        for (int i = 0; i < ncomp; ++i) {
          if (s[1 + 2 * i] != comp[i].id) return nosupport("scan component order");
          comp[i].td = s[2 + 2 * i] >> 4;
          comp[i].ta = s[2 + 2 * i] & 15;
          if (comp[i].td > 3 || comp[i].ta > 3 || !dc_present[comp[i].td] || !ac_present[comp[i].ta] || !qt_present[comp[i].tq])
            return fail("scan refers to a missing table");
        }
        got_scan = 1;
        return true;
      }
      // every other segment (APPn, COM, ...) is skipped
    }
  }

  // ---- parse stage, second half: the scan's shape
  bool setup_geometry() {
    Geometry& g = geo;
    g = Geometry();
    g.hmax = g.vmax = 1;
    for (int i = 0; i < ncomp; ++i) {
      if (comp[i].h < 1 || comp[i].v < 1 || comp[i].h > 2 || comp[i].v > 2) return nosupport("sampling factors above 2");
      g.hmax = comp[i].h > g.hmax ? comp[i].h : g.hmax;
      g.vmax = comp[i].v > g.vmax ? comp[i].v : g.vmax;
    }
    if (comp[0].h != g.hmax || comp[0].v != g.vmax || comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 || comp[2].v != 1 ||
        (g.hmax == 1 && g.vmax == 2))
      return nosupport("chroma sampling other than 4:4:4, 4:2:2 or 4:2:0");
    if (width <= 0 || height <= 0) return fail("empty image");
    g.width = width;
    g.height = height;
    g.restart_interval = restart_interval;
    g.mcux = (width + 8 * g.hmax - 1) / (8 * g.hmax);
    g.mcuy = (height + 8 * g.vmax - 1) / (8 * g.vmax);
    int nb = 0, bytes = 0;
    for (int i = 0; i < ncomp; ++i) {
      g.h[i] = comp[i].h;
      g.v[i] = comp[i].v;
      g.dw[i] = (width * comp[i].h + g.hmax - 1) / g.hmax;
      g.dh[i] = (height * comp[i].v + g.vmax - 1) / g.vmax;
      g.bw[i] = g.mcux * comp[i].h;
      g.bh[i] = g.mcuy * comp[i].v;
      g.off[i] = nb;
      for (int k = 0; k < comp[i].h * comp[i].v; ++k) g.mcu_comp[nb++] = (unsigned char)i;
      g.plane_off[i] = bytes;
      bytes += g.bw[i] * 8 * g.bh[i] * 8;
    }
    g.blocks_per_mcu = nb;
    g.total_blocks = nb * g.mcux * g.mcuy;
    g.plane_bytes = bytes;
    return true;
  }

  // ---- entropy stage: the whole scan, sequentially.  coefs = geo.total_blocks * 64 zeroed values.
  bool entropy(short* coefs) {
    const Geometry& g = geo;
    for (int i = 0; i < ncomp; ++i) comp[i].pred = 0;
    bitbuf = 0;
    bits = 0;
    hit_marker = false;
    int until_restart = restart_interval, next_rst = 0;
    short* coef = coefs;
    blocks_done = 0;
    for (int my = 0; my < g.mcuy; ++my)
      for (int mx = 0; mx < g.mcux; ++mx) {
        if (restart_interval && until_restart == 0) {
          // byte-align, expect RSTn
          bitbuf = 0;
          bits = 0;
          hit_marker = false;
          while (p < end && !(p[0] == 0xFF && p + 1 < end && p[1] >= 0xD0 && p[1] <= 0xD7)) ++p;  // (skips stuffing left in the stream)
          if (end - p < 2) return fail("missing restart marker");
          if (p[1] != 0xD0 + next_rst) return fail("restart markers out of sequence");
          p += 2;
          next_rst = (next_rst + 1) & 7;
          until_restart = restart_interval;
          for (int i = 0; i < ncomp; ++i) comp[i].pred = 0;
        }
        for (int b = 0; b < g.blocks_per_mcu; ++b, coef += 64, ++blocks_done)
          if (!decode_block(comp[g.mcu_comp[b]], coef)) return false;
        if (restart_interval) --until_restart;
      }
    return true;
  }
};

// parse stage: everything up to the first byte of the entropy-coded data (d.p afterwards).  0, -1 (malformed / size mismatch)
// or -2 (a JPEG flavour this decoder does not handle); d.err names the reason.
inline int parse(Decoder& d, const unsigned char* data, size_t len, int width, int height) {
  d.p = data;
  d.end = data + len;
  if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) {
    d.fail("not a JPEG stream (no SOI)");
    return -1;
  }
  int got = 0;
  if (!d.parse_tables_and_scan(got) || !got) return d.unsupported ? -2 : -1;
  if (d.width != width || d.height != height) {
    d.fail("image size differs from the log's resolution");
    return -1;
  }
  if (!d.setup_geometry()) return d.unsupported ? -2 : -1;
  return 0;
}

// What the parallel entropy decoder needs besides the tables: the entropy-coded data cut at its restart markers, found with a byte
// scan.  Segment i is bytes [start, end): `end` is the first 0xFF not followed by 0x00 (where the sequential bit reader starts to
// supply zeros), the next segment starts behind the next RSTn.  The sequential decoder's two refusals at a restart ("missing
// restart marker", "restart markers out of sequence") end the list early; *restart_err then names the one met while looking for
// segment segs.size().
struct Segment {
  uint32_t start, end;
};
inline void find_segments(const unsigned char* data, size_t len, size_t scan_off, const Geometry& g, std::vector<Segment>& segs,
                          const char** restart_err) {
  const long mcus = (long)g.mcux * g.mcuy;
  const long want = g.restart_interval ? (mcus + g.restart_interval - 1) / g.restart_interval : 1;
  *restart_err = nullptr;
  segs.clear();
  size_t at = scan_off;
  int next_rst = 0;
  for (long s = 0; s < want; ++s) {
    size_t e = at;
    for (;;) {
      const void* f = e < len ? memchr(data + e, 0xFF, len - e) : nullptr;
      if (!f) {
        e = len;
        break;
      }
      e = (size_t)((const unsigned char*)f - data);
      if (e + 1 >= len || data[e + 1] != 0x00) break;
      e += 2;
    }
    Segment sg;
    sg.start = (uint32_t)at;
    sg.end = (uint32_t)e;
    segs.push_back(sg);
    if (s + 1 == want) break;
    size_t q = e;
    while (q < len && !(data[q] == 0xFF && q + 1 < len && data[q + 1] >= 0xD0 && data[q + 1] <= 0xD7)) ++q;
    if (len - q < 2) {
      *restart_err = "missing restart marker";
      return;
    }
    if (data[q + 1] != 0xD0 + next_rst) {
      *restart_err = "restart markers out of sequence";
      return;
    }
    next_rst = (next_rst + 1) & 7;
    at = q + 2;
  }
}

// number of blocks of segment s (restart_interval MCUs, the last segment the remainder)
inline long segment_blocks(const Geometry& g, long s) {
  const long mcus = (long)g.mcux * g.mcuy;
  if (!g.restart_interval) return mcus * g.blocks_per_mcu;
  const long first = s * g.restart_interval;
  const long n = mcus - first < g.restart_interval ? mcus - first : g.restart_interval;
  return (n > 0 ? n : 0) * g.blocks_per_mcu;
}

// the lanes of the parallel entropy decoder: every segment cut into subsequences of S bytes
inline void build_lanes(const Geometry& g, const std::vector<Segment>& segs, int S, std::vector<SegInfo>& si, std::vector<LaneInfo>& lanes) {
  si.clear();
  lanes.clear();
  uint32_t block = 0;
  for (size_t s = 0; s < segs.size(); ++s) {
    SegInfo o;
    o.start = segs[s].start;
    o.end = segs[s].end;
    o.first_lane = (uint32_t)lanes.size();
    o.first_block = block;
    o.nblocks = (uint32_t)segment_blocks(g, (long)s);
    block += o.nblocks;
    si.push_back(o);
    const int n = segment_lanes(o.end - o.start, S);
    for (int j = 0; j < n; ++j) {
      LaneInfo l;
      l.seg = (uint32_t)s;
      l.first_byte = o.start + (uint32_t)j * (uint32_t)S;
      l.stop_byte = j + 1 == n ? o.end : l.first_byte + (uint32_t)S;
      l.flags = (j == 0 ? kLaneFirst : 0) | (j + 1 == n ? kLaneLast : 0);
      lanes.push_back(l);
    }
  }
}

// back half, first step: coefficient block `b` (MCU order) -> its 8x8 samples in the component's plane
inline void idct_block(const Geometry& g, const unsigned short* q, const short* coef, int b, unsigned char* planes) {
  const int bpm = g.blocks_per_mcu, mcu = b / bpm, j = b - mcu * bpm, c = g.mcu_comp[j];
  const int vy = (j - g.off[c]) / g.h[c], hx = (j - g.off[c]) - vy * g.h[c];
  const int bx = (mcu % g.mcux) * g.h[c] + hx, by = (mcu / g.mcux) * g.v[c] + vy;
  const int stride = g.bw[c] * 8;
  unsigned char* out = planes + g.plane_off[c] + (size_t)by * 8 * stride + (size_t)bx * 8;
  int64_t ws[64];
  for (int col = 0; col < 8; ++col) {
    int d[8];
    int64_t w[8];
    for (int r = 0; r < 8; ++r) d[r] = dequant(coef[r * 8 + col], q[r * 8 + col]);
    idct_column(d, w);
    for (int r = 0; r < 8; ++r) ws[r * 8 + col] = w[r];
  }
  for (int r = 0; r < 8; ++r) idct_row(ws + r * 8, out + (size_t)r * stride);
}

// back half: coefficients (entropy stage) -> RGB8, R and B exchanged where `flip`.  qt[c] = component c's quantisation table.
inline void back_half(const Geometry& g, const unsigned short (*qt)[64], const short* coefs, unsigned char* rgb, int flip) {
  std::vector<unsigned char> planes((size_t)g.plane_bytes);
  for (int b = 0; b < g.total_blocks; ++b) idct_block(g, qt[g.mcu_comp[b % g.blocks_per_mcu]], coefs + (size_t)b * 64, b, planes.data());
  const unsigned char* py = planes.data() + g.plane_off[0];
  const unsigned char* pb = planes.data() + g.plane_off[1];
  const unsigned char* pr = planes.data() + g.plane_off[2];
  const int hx = g.hmax / g.h[1], vx = g.vmax / g.v[1];
  // the colour terms as libjpeg's tables (one evaluation per value instead of one per pixel)
  int cr_r[256], cb_b[256];
  int64_t cr_g[256], cb_g[256];
  for (int i = 0; i < 256; ++i) {
    cr_r[i] = ycc_cr_r(i);
    cb_b[i] = ycc_cb_b(i);
    cr_g[i] = ycc_cr_g(i);
    cb_g[i] = ycc_cb_g(i);
  }
  const int ro = flip ? 2 : 0, bo = flip ? 0 : 2;
  for (int y = 0; y < g.height; ++y) {
    unsigned char* o = rgb + (size_t)y * g.width * 3;
    for (int x = 0; x < g.width; ++x, o += 3) {
      const int Y = py[(size_t)y * (g.bw[0] * 8) + x];
      const int B = upsampled_sample(pb, g.bw[1] * 8, g.dw[1], g.dh[1], hx, vx, x, y);
      const int R = upsampled_sample(pr, g.bw[2] * 8, g.dw[2], g.dh[2], hx, vx, x, y);
      o[ro] = clamp255(Y + cr_r[R]);
      o[1] = clamp255(Y + (int)((cb_g[B] + cr_g[R]) >> 16));
      o[bo] = clamp255(Y + cb_b[B]);
    }
  }
}

inline int decode_rgb(const unsigned char* data, size_t len, int width, int height, unsigned char* rgb, const char** err) {
  Decoder d;
  auto out = [&](int rc) {
    if (err) *err = d.err ? d.err : "";
    return rc;
  };
  const int rc = parse(d, data, len, width, height);
  if (rc) return out(rc);
  std::vector<short> coefs((size_t)d.geo.total_blocks * 64, 0);
  if (!d.entropy(coefs.data())) return out(d.unsupported ? -2 : -1);
  unsigned short qt[3][64];
  for (int i = 0; i < 3; ++i) memcpy(qt[i], d.qt[d.comp[i].tq], sizeof(qt[i]));
  back_half(d.geo, qt, coefs.data(), rgb, 0);
  return out(0);
}

}  // namespace jpeg
}  // namespace dms
