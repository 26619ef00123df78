// The arithmetic of the baseline JPEG decoder, stated once for the host (csrc/jpeg.hpp, the sequential decoder) and for the device
// (csrc/jpeg_dev.hip): plain C++ over plain data, no containers, no I/O; every function is __host__ __device__ under hipcc and an
// ordinary inline function under a host compiler (tests/jpeg_lanes_host.cpp includes this file alone).
//   * back half: dequantisation, the two passes of libjpeg's JDCT_ISLOW inverse DCT, its range limit, one sample of its "fancy"
//     h2v1 / h2v2 upsampling (edge replication; planes at most 2 samples wide are replicated), one pixel of its fixed-point
//     Y Cb Cr -> RGB conversion.  Integer widths are the sequential decoder's: 64-bit wherever it had them.
//   * entropy: the canonical Huffman table, one symbol of it, and decode_lane(): the decode of one SUBSEQUENCE of an
//     entropy-coded segment from a given state (bit position, block inside the MCU, zigzag position) - the unit of the parallel
//     decoder (Weissenberger & Schmidt, "Accelerating JPEG Decompression on GPUs": Huffman streams re-synchronise after a wrong
//     start).  The sequential decoder and the lane decoder read the same tables with the same single-symbol step.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMS_JP_HD __host__ __device__ __forceinline__
#else
#define DMS_JP_HD inline
#endif

namespace dms {
namespace jpeg {

// ---- plain data ------------------------------------------------------------------------------------------------------------
struct Huff {
  // canonical Huffman table: codes of length l lie in [mincode[l], maxcode[l]]; valptr[l] indexes the first of them
  int mincode[17], maxcode[18], valptr[17];
  unsigned char vals[256];
  // 9-bit lookahead: (length << 8) | symbol, 0 = longer code
  unsigned short look[512];
};

// the scan's shape: what parse leaves for the entropy stage and the back half
struct Geometry {
  int width, height, hmax, vmax, mcux, mcuy, restart_interval;
  int blocks_per_mcu, total_blocks, plane_bytes;
  int h[3], v[3];        // sampling factors
  int dw[3], dh[3];      // downsampled size in samples (the "real" rows / columns)
  int bw[3], bh[3];      // size in blocks, padded to whole MCUs
  int off[3];            // first block of the component inside an MCU
  int plane_off[3];      // byte offset of the component's plane (bw * 8 x bh * 8 samples) in the plane buffer
  unsigned char mcu_comp[8];  // component of each block of an MCU (at most 4 + 1 + 1)
};

// index, in the scan's MCU order, of block (bx, by) of component c
DMS_JP_HD int mcu_order_index(const Geometry& g, int c, int bx, int by) {
  const int mx = bx / g.h[c], hx = bx - mx * g.h[c], my = by / g.v[c], vy = by - my * g.v[c];
  return (my * g.mcux + mx) * g.blocks_per_mcu + g.off[c] + vy * g.h[c] + hx;
}

DMS_JP_HD int zigzag(int k) {  // natural-order position of the k-th coefficient of the scan
  constexpr unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// ---- back half: one 8x8 block, jidctint.c's arithmetic ------------------------------------------------------------------------
DMS_JP_HD int64_t descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }
DMS_JP_HD unsigned char range_limit(int64_t x) {  // libjpeg's table lookup with its 10-bit index mask
  const int i = (int)(x & 1023);
  if (i < 128) return (unsigned char)(128 + i);
  if (i < 512) return 255;
  if (i < 896) return 0;
  return (unsigned char)(i - 896);
}
DMS_JP_HD int dequant(short coef, unsigned short q) { return coef * (int)q; }

namespace idct_k {
constexpr int CB = 13, P1 = 2;
constexpr int64_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                  F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
}  // namespace idct_k

// the even / odd butterflies both passes share: in[0..7] -> the four sums tmp10..13 and the four odd terms tmp0..3
DMS_JP_HD void idct_butterfly(const int64_t in[8], int64_t even[4], int64_t odd[4]) {
  using namespace idct_k;
  int64_t z2 = in[2], z3 = in[6];
  int64_t z1 = (z2 + z3) * F0_541;
  int64_t tmp2 = z1 + z3 * (-F1_847), tmp3 = z1 + z2 * F0_765;
  z2 = in[0];
  z3 = in[4];
  int64_t tmp0 = (z2 + z3) * (1 << CB), tmp1 = (z2 - z3) * (1 << CB);
  even[0] = tmp0 + tmp3;  // tmp10
  even[3] = tmp0 - tmp3;  // tmp13
  even[1] = tmp1 + tmp2;  // tmp11
  even[2] = tmp1 - tmp2;  // tmp12
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int64_t z4 = tmp1 + tmp3;
  const int64_t z5 = (z3 + z4) * F1_175;
  tmp0 *= F0_298;
  tmp1 *= F2_053;
  tmp2 *= F3_072;
  tmp3 *= F1_501;
  z1 *= -F0_899;
  z2 *= -F2_562;
  z3 *= -F1_961;
  z4 *= -F0_390;
  z3 += z5;
  z4 += z5;
  odd[0] = tmp0 + z1 + z3;
  odd[1] = tmp1 + z2 + z4;
  odd[2] = tmp2 + z2 + z3;
  odd[3] = tmp3 + z1 + z4;
}

// column pass: d[r] = the dequantised coefficient in row r of one column; ws[r] = that column of the workspace
DMS_JP_HD void idct_column(const int d[8], int64_t ws[8]) {
  using namespace idct_k;
  if (!d[1] && !d[2] && !d[3] && !d[4] && !d[5] && !d[6] && !d[7]) {
    const int64_t dc = (int64_t)d[0] * (1 << P1);
    for (int r = 0; r < 8; ++r) ws[r] = dc;
    return;
  }
  int64_t in[8], e[4], o[4];
  for (int r = 0; r < 8; ++r) in[r] = d[r];
  idct_butterfly(in, e, o);
  ws[0] = descale(e[0] + o[3], CB - P1);
  ws[7] = descale(e[0] - o[3], CB - P1);
  ws[1] = descale(e[1] + o[2], CB - P1);
  ws[6] = descale(e[1] - o[2], CB - P1);
  ws[2] = descale(e[2] + o[1], CB - P1);
  ws[5] = descale(e[2] - o[1], CB - P1);
  ws[3] = descale(e[3] + o[0], CB - P1);
  ws[4] = descale(e[3] - o[0], CB - P1);
}

// row pass: w[c] = one row of the workspace; o[c] = the row's samples
DMS_JP_HD void idct_row(const int64_t w[8], unsigned char o[8]) {
  using namespace idct_k;
  int64_t e[4], d[4];
  idct_butterfly(w, e, d);
  constexpr int S = CB + P1 + 3;
  o[0] = range_limit(descale(e[0] + d[3], S));
  o[7] = range_limit(descale(e[0] - d[3], S));
  o[1] = range_limit(descale(e[1] + d[2], S));
  o[6] = range_limit(descale(e[1] - d[2], S));
  o[2] = range_limit(descale(e[2] + d[1], S));
  o[5] = range_limit(descale(e[2] - d[1], S));
  o[3] = range_limit(descale(e[3] + d[0], S));
  o[4] = range_limit(descale(e[3] - d[0], S));
}

// ---- back half: one sample of a component at full resolution (jdsample.c: fullsize copy, h2v1 / h2v2 fancy upsampling) ----------
// src = the component's plane (`stride` bytes per row), dw x dh its real samples, hx / vx = 1 or 2 its horizontal / vertical
// expansion; (x, y) a pixel of the image.  Closed form of libjpeg's running row filter: 3/4 of the nearer sample + 1/4 of the
// further one, the two roundings alternating; the first and last output columns copy (h2v1) or scale (h2v2) the edge sample;
// rows beyond the real ones are copies of the edge row.
DMS_JP_HD unsigned char upsampled_sample(const unsigned char* src, int stride, int dw, int dh, int hx, int vx, int x, int y) {
  if (hx == 1 && vx == 1) return src[(size_t)y * stride + x];
  const int r = vx == 2 ? y >> 1 : y;
  const int i = x >> 1;
  if (dw <= 2) return src[(size_t)r * stride + i];  // libjpeg only smooths planes more than two samples wide
  const unsigned char* in0 = src + (size_t)r * stride;
  if (vx == 1) {  // h2v1
    const int v = in0[i];
    if (x & 1) return i == dw - 1 ? (unsigned char)v : (unsigned char)((v * 3 + in0[i + 1] + 2) >> 2);
    return i == 0 ? (unsigned char)v : (unsigned char)((v * 3 + in0[i - 1] + 1) >> 2);
  }
  int r1 = (y & 1) ? r + 1 : r - 1;
  if (r1 < 0) r1 = 0;
  if (r1 > dh - 1) r1 = dh - 1;
  const unsigned char* in1 = src + (size_t)r1 * stride;
  const int thiscol = in0[i] * 3 + in1[i];
  if (x & 1) {
    if (i == dw - 1) return (unsigned char)((thiscol * 4 + 7) >> 4);
    return (unsigned char)((thiscol * 3 + (in0[i + 1] * 3 + in1[i + 1]) + 7) >> 4);
  }
  if (i == 0) return (unsigned char)((thiscol * 4 + 8) >> 4);
  return (unsigned char)((thiscol * 3 + (in0[i - 1] * 3 + in1[i - 1]) + 8) >> 4);
}

// ---- back half: one pixel, jdcolor.c build_ycc_rgb_table / ycc_rgb_convert ---------------------------------------------------------
DMS_JP_HD unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
// the four table entries of build_ycc_rgb_table, computed
DMS_JP_HD int ycc_cr_r(int Cr) { return (int)((91881 * (int64_t)(Cr - 128) + 32768) >> 16); }
DMS_JP_HD int ycc_cb_b(int Cb) { return (int)((116130 * (int64_t)(Cb - 128) + 32768) >> 16); }
DMS_JP_HD int64_t ycc_cr_g(int Cr) { return -46802 * (int64_t)(Cr - 128); }
DMS_JP_HD int64_t ycc_cb_g(int Cb) { return -22554 * (int64_t)(Cb - 128) + 32768; }
DMS_JP_HD void ycc_to_rgb(int Y, int Cb, int Cr, unsigned char* r, unsigned char* g, unsigned char* b) {
  *r = clamp255(Y + ycc_cr_r(Cr));
  *g = clamp255(Y + (int)((ycc_cb_g(Cb) + ycc_cr_g(Cr)) >> 16));
  *b = clamp255(Y + ycc_cb_b(Cb));
}

// ---- entropy: one Huffman symbol ---------------------------------------------------------------------------------------------------
// bits16 = the next 16 bits of the stream; returns the symbol and its code length, or -1 (length 16) where no code matches
DMS_JP_HD int huff_symbol(const Huff& h, unsigned bits16, int* len) {
  const unsigned short e = h.look[bits16 >> 7];
  if (e) {
    *len = e >> 8;
    return e & 0xff;
  }
  for (int l = 10; l <= 16; ++l) {
    const int c = (int)(bits16 >> (16 - l));
    if (h.maxcode[l] >= 0 && c <= h.maxcode[l] && c >= h.mincode[l]) {
      *len = l;
      return h.vals[(h.valptr[l] + c - h.mincode[l]) & 255];
    }
  }
  *len = 16;
  return -1;
}
DMS_JP_HD int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// what the sequential decoder refuses inside a block, in the order it would meet them
enum BlockError { kErrNone = 0, kErrBadCode = 1, kErrBadDcSize = 2, kErrAcRun = 3 };
DMS_JP_HD const char* block_error_text(int e) {
  return e == kErrBadCode ? "bad Huffman code" : e == kErrBadDcSize ? "bad DC size" : e == kErrAcRun ? "AC run past the block" : "";
}

// ---- entropy: the parallel decoder's unit --------------------------------------------------------------------------------------------
// A SEGMENT is the entropy-coded data between two markers: bytes [start, end) of the stream, `end` = the first 0xFF that is not
// followed by 0x00 (or the end of the stream); bits past `end` are zeros, as the sequential bit reader and libjpeg supply them.
// A segment is cut into SUBSEQUENCES of S bytes; one lane decodes every symbol that STARTS inside its subsequence.
struct LaneState {
  uint32_t pos;  // bit position in the stream of the next unread bit; always inside a data byte, never a stuffed 0x00
  int blk;       // block inside the MCU
  int k;         // zigzag position of the next coefficient: 0 = the DC symbol comes next
};
DMS_JP_HD bool same_state(const LaneState& a, const LaneState& b) { return a.pos == b.pos && a.blk == b.blk && a.k == b.k; }

// number of subsequences of a segment of `len` bytes (an empty segment still has a lane: it decodes its blocks from zeros)
DMS_JP_HD int segment_lanes(uint32_t len, int S) { return len ? (int)((len + (uint32_t)S - 1) / (uint32_t)S) : 1; }

// what the host's byte scan leaves for the lanes (csrc/jpeg.hpp find_segments / build_lanes)
struct SegInfo {
  uint32_t start, end;   // bytes [start, end) of the stream
  uint32_t first_lane;   // index of the segment's first lane
  uint32_t first_block;  // index, in the scan's MCU order, of the segment's first block
  uint32_t nblocks;      // blocks the segment holds
};
struct LaneInfo {
  uint32_t seg;
  uint32_t first_byte, stop_byte;  // the subsequence: bytes [first_byte, stop_byte) of the stream
  uint32_t flags;                  // 1: first lane of its segment, 2: last lane of its segment
};
constexpr uint32_t kLaneFirst = 1, kLaneLast = 2;

// Bit reader over one segment.  Bytes come from `win` where index - win_lo falls inside [0, win_n) (the device keeps the wave's
// slice of the stream in LDS) and from `mem` otherwise; nothing at or past seg_end is ever read.
struct LaneReader {
  const unsigned char* mem;
  const unsigned char* win;
  uint32_t win_lo, win_n;
  uint32_t seg_end;   // byte index
  uint32_t stop;      // byte index: symbols that start at or past it belong to the next lane
  uint32_t p;         // next byte to load (runs on past seg_end over the virtual zeros)
  uint64_t buf;
  int bits;
  int low;            // buffered bits that came from bytes before `stop`

  DMS_JP_HD unsigned byte_at(uint32_t i) const {
    const uint32_t w = i - win_lo;
    return w < win_n ? win[w] : mem[i];
  }
  DMS_JP_HD void fill() {
    while (bits <= 56) {
      unsigned c = 0;
      if (p < stop) low += 8;
      if (p < seg_end) {
        c = byte_at(p);
        ++p;
        if (c == 0xFF && p < seg_end) ++p;  // inside a segment every 0xFF is followed by its stuffed 0x00
      } else {
        ++p;
      }
      buf |= (uint64_t)c << (56 - bits);
      bits += 8;
    }
  }
  DMS_JP_HD void start(uint32_t bitpos) {
    p = bitpos >> 3;
    buf = 0;
    bits = 0;
    low = 0;
    fill();
    skip((int)(bitpos & 7));
  }
  DMS_JP_HD unsigned peek16() {
    if (bits < 16) fill();
    return (unsigned)(buf >> 48);
  }
  DMS_JP_HD void skip(int n) {
    buf <<= n;
    bits -= n;
    low = low > n ? low - n : 0;
  }
  DMS_JP_HD int get(int n) {  // 1 <= n <= 15
    if (bits < n) fill();
    const int v = (int)(buf >> (64 - n));
    skip(n);
    return v;
  }
  // the position of the next unread bit: walk back from p over the bytes still buffered, stepping over stuffed zeros
  DMS_JP_HD uint32_t position() const {
    uint32_t q = p;
    const int nb = (bits + 7) >> 3;
    for (int i = 0; i < nb; ++i) {
      --q;
      if (q < seg_end && q > 0 && byte_at(q) == 0x00 && byte_at(q - 1) == 0xFF) --q;
    }
    return q * 8 + (uint32_t)(nb * 8 - bits);
  }
};

// where lane j > 0 of a segment starts while its true state is unknown: the first data byte of its subsequence (a lane must look
// at the byte before its first one: a 0x00 after a 0xFF is stuffing), "block 0, position 0"
DMS_JP_HD LaneState speculative_start(const LaneReader& rd, uint32_t seg_start, uint32_t first_byte) {
  LaneState s;
  uint32_t i = first_byte;
  if (i > seg_start && i < rd.seg_end && rd.byte_at(i) == 0x00 && rd.byte_at(i - 1) == 0xFF) ++i;
  s.pos = i * 8;
  s.blk = 0;
  s.k = 0;
  return s;
}

// Decodes from `st` every symbol that starts before rd.stop and leaves the exit state in `st`; returns the number of block ends.
// `block` is the index, inside the segment, of the block `st` stands in; with `to_count` >= 0 (the last lane of a segment in the
// write pass) the lane goes on, over the zeros past the data, until that many blocks of the segment are complete.
// The sink sees coefficients and errors:  dc(block, diff)  ac(block, natural position, value)  error(block, k, code).
// While states are speculative, what the sequential decoder refuses is normal; the fixed rule: an unmatched code is 16 bits
// of symbol 0 (the sequential decoder's own recovery), a DC size above 15 keeps its low 4 bits, an AC run past the block
// consumes its value bits and ends the block.  The same rule holds in the write pass, where it only decides what follows the
// first error - which the sequential decoder never reaches.
template <class Sink>
DMS_JP_HD int decode_lane(LaneReader& rd, const Huff* dc, const Huff* ac, const Geometry& g, LaneState& st, long block, long to_count,
                          Sink& sink) {
  rd.start(st.pos);
  int ends = 0;
  int blk = st.blk, k = st.k;
  while (rd.low > 0 || block < to_count) {
    const int comp = g.mcu_comp[blk & 7];
    int len;
    bool end_of_block = false;
    if (k == 0) {
      int s = huff_symbol(dc[comp], rd.peek16(), &len);
      rd.skip(len);
      if (s < 0) {
        sink.error(block, 0, kErrBadCode);
        s = 0;
      }
      if (s > 15) {
        sink.error(block, 0, kErrBadDcSize);
        s &= 15;
      }
      sink.dc(block, s ? extend(rd.get(s), s) : 0);
      k = 1;
    } else {
      int rs = huff_symbol(ac[comp], rd.peek16(), &len);
      rd.skip(len);
      if (rs < 0) {
        sink.error(block, k, kErrBadCode);
        rs = 0;
      }
      const int r = rs >> 4, sz = rs & 15;
      if (sz == 0) {
        if (r != 15) end_of_block = true;
        k += 16;
      } else {
        const int at = k + r;
        const int v = extend(rd.get(sz), sz);
        if (at > 63) {
          sink.error(block, k, kErrAcRun);
          end_of_block = true;
        } else {
          sink.ac(block, zigzag(at), v);
          k = at + 1;
        }
      }
      if (k >= 64) end_of_block = true;
    }
    if (end_of_block) {
      k = 0;
      blk = blk + 1 == g.blocks_per_mcu ? 0 : blk + 1;
      ++block;
      ++ends;
    }
  }
  st.pos = rd.position();
  st.blk = blk;
  st.k = k;
  return ends;
}

struct NullSink {
  DMS_JP_HD void dc(long, int) {}
  DMS_JP_HD void ac(long, int, int) {}
  DMS_JP_HD void error(long, int, int) {}
};

// rounds of relaxation run as separate launches before the single-lane pass takes over: after round r the first r + 1 lanes of a
// segment hold their true exit state
constexpr int kSyncRounds = 12;

// a lane's record between passes: its exit state and the block ends it counted
struct LaneRecord {
  uint32_t pos;
  uint32_t packed;  // k | blk << 8 | block ends << 16
  uint32_t entry_pos, entry_packed;  // the state the lane started from (k | blk << 8): the same entry gives the same exit
};
DMS_JP_HD LaneRecord pack_record(const LaneState& entry, const LaneState& s, int ends) {
  LaneRecord r;
  r.pos = s.pos;
  r.packed = (uint32_t)s.k | ((uint32_t)s.blk << 8) | ((uint32_t)ends << 16);
  r.entry_pos = entry.pos;
  r.entry_packed = (uint32_t)entry.k | ((uint32_t)entry.blk << 8);
  return r;
}
DMS_JP_HD LaneState record_state(const LaneRecord& r) {
  LaneState s;
  s.pos = r.pos;
  s.k = (int)(r.packed & 63);
  s.blk = (int)((r.packed >> 8) & 7);
  return s;
}
DMS_JP_HD uint32_t record_ends(const LaneRecord& r) { return r.packed >> 16; }
DMS_JP_HD bool same_exit(const LaneRecord& a, const LaneRecord& b) {
  return a.pos == b.pos && ((a.packed ^ b.packed) & 0xffffu) == 0;
}

// everything a lane reads
struct ScanView {
  const unsigned char* mem;  // the stream
  const unsigned char* win;  // bytes [win_lo, win_lo + win_n) of it, held closer (LDS); win_n = 0: none
  uint32_t win_lo, win_n;
  const Huff* dc;            // [3], by component
  const Huff* ac;
  const Geometry* g;
  const SegInfo* segs;
  const LaneInfo* lanes;
};
DMS_JP_HD LaneReader lane_reader(const ScanView& sc, const SegInfo& sg, const LaneInfo& li) {
  LaneReader rd;
  rd.mem = sc.mem;
  rd.win = sc.win;
  rd.win_lo = sc.win_lo;
  rd.win_n = sc.win_n;
  rd.seg_end = sg.end;
  rd.stop = li.stop_byte;
  rd.p = 0;
  rd.buf = 0;
  rd.bits = 0;
  rd.low = 0;
  return rd;
}

// One lane of relaxation round `round`: prev = every lane's record after the round before (unused in round 0).  The first lane of
// a segment starts in the true state; in round 0 every other lane starts at "block 0, position 0", later from its left
// neighbour's exit state.  A round that changes no exit state means every entry state was the true one.
DMS_JP_HD LaneRecord sync_lane(const ScanView& sc, int lane, int round, const LaneRecord* prev) {
  const LaneInfo li = sc.lanes[lane];
  const SegInfo sg = sc.segs[li.seg];
  if ((li.flags & kLaneFirst) && round > 0) return prev[lane];
  LaneReader rd = lane_reader(sc, sg, li);
  LaneState st;
  if (li.flags & kLaneFirst) {
    st.pos = sg.start * 8;
    st.blk = 0;
    st.k = 0;
  } else if (round == 0) {
    st = speculative_start(rd, sg.start, li.first_byte);
  } else {
    st = record_state(prev[lane - 1]);
    const LaneRecord mine = prev[lane];
    if (mine.entry_pos == st.pos && mine.entry_packed == ((uint32_t)st.k | ((uint32_t)st.blk << 8))) return mine;  // decoded before
  }
  const LaneState entry = st;
  NullSink sink;
  const int ends = decode_lane(rd, sc.dc, sc.ac, *sc.g, st, 0, -1, sink);
  return pack_record(entry, st, ends);
}

// The single-lane pass over a segment whose states the rounds left unsettled: lanes 0 .. kSyncRounds - 1 are certainly right,
// the rest is re-decoded in order, each lane from the exit its left neighbour has just stored.  Returns the lanes re-decoded.
DMS_JP_HD int settle_segment(const ScanView& sc, int first_lane, int lanes_in_segment, LaneRecord* rec) {
  int n = 0;
  for (int j = kSyncRounds; j < lanes_in_segment; ++j, ++n) rec[first_lane + j] = sync_lane(sc, first_lane + j, 1, rec);
  return n;
}

// write pass: coefficients go into the zeroed buffer (the DC slot receives the difference), blocks at or past the segment's
// block count are dropped; what the sequential decoder would refuse lowers *err_key to (block * 64 + k) * 4 + BlockError, so
// the smallest key is the refusal the sequential decoder meets first
constexpr uint32_t kNoBlockError = 0xffffffffu;
struct CoefSink {
  short* coefs;
  uint32_t first_block, nblocks;
  uint32_t* err_key;
  DMS_JP_HD void dc(long b, int v) {
    if ((unsigned long)b < nblocks) coefs[((size_t)first_block + (size_t)b) * 64] = (short)v;
  }
  DMS_JP_HD void ac(long b, int at, int v) {
    if ((unsigned long)b < nblocks) coefs[((size_t)first_block + (size_t)b) * 64 + (size_t)(at & 63)] = (short)v;
  }
  DMS_JP_HD void error(long b, int k, int code) {
    if ((unsigned long)b >= nblocks) return;
    const uint32_t key = (((uint32_t)first_block + (uint32_t)b) * 64u + (uint32_t)k) * 4u + (uint32_t)code;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(err_key, key);
#else
    if (key < *err_key) *err_key = key;
#endif
  }
};
// rec = the settled records, block_in_segment = the exclusive sum of the block ends of the segment's lanes before this one
DMS_JP_HD void write_lane(const ScanView& sc, int lane, const LaneRecord* rec, uint32_t block_in_segment, short* coefs, uint32_t* err_key) {
  const LaneInfo li = sc.lanes[lane];
  const SegInfo sg = sc.segs[li.seg];
  LaneReader rd = lane_reader(sc, sg, li);
  LaneState st;
  if (li.flags & kLaneFirst) {
    st.pos = sg.start * 8;
    st.blk = 0;
    st.k = 0;
  } else {
    st = record_state(rec[lane - 1]);
  }
  CoefSink sink;
  sink.coefs = coefs;
  sink.first_block = sg.first_block;
  sink.nblocks = sg.nblocks;
  sink.err_key = err_key;
  decode_lane(rd, sc.dc, sc.ac, *sc.g, st, (long)block_in_segment, (li.flags & kLaneLast) ? (long)sg.nblocks : -1L, sink);
}

}  // namespace jpeg
}  // namespace dms
