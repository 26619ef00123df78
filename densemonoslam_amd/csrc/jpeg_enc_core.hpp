// The arithmetic of the baseline JPEG encoder, stated once for the host (csrc/jpeg_enc.hpp, the sequential encoder) and for the
// device (csrc/jpeg_enc_dev.hip), as csrc/jpeg_core.hpp is for the decoder: plain C++ over plain data, every function
// __host__ __device__ under hipcc and an ordinary inline function under a host compiler (tests/jpeg_enc_host.cpp).  It is libjpeg's
// C encoder with its default parameters, integer throughout:
//   jccolor.c    fixed-point R G B -> Y Cb Cr, one pixel
//   jcsample.c   h2v2 box filter with the alternating 1, 2 bias; the right edge is replicated in the pixels (expand_right_edge),
//   jcprepct.c   the bottom edge first in the pixels up to a whole row group, then in the downsampled rows
//   jfdctint.c   JDCT_ISLOW, CONST_BITS 13, PASS1_BITS 2, the two passes
//   jcdctmgr.c   division with rounding by quant << 3
//   jcparam.c    jpeg_set_quality's scaling of the Annex K tables
//   jccoefct.c   dummy blocks right of / below a component's last real block: zero AC, the DC of the block before them
//   jchuff.c     the Annex K Huffman tables; one block's bit length and one block's emission
//   jcmarker.c   the header in libjpeg's order
// The entropy stage is written per block so that the device can run all blocks at once: a block's bit length needs nothing but
// its coefficients and the DC of the real block before it (enc_prev_real_block), an exclusive sum of the lengths places it, and
// enc_block_emit writes through a BitWriter whose sink separates the words a block owns (plain stores) from the two it may share with
// its neighbours (OR into a zeroed buffer).
#pragma once
#include "jpeg_core.hpp"

namespace dms {
namespace jpeg {

// ---- jccolor.c ---------------------------------------------------------------------------------------------------------------
DMS_JP_HD void rgb_to_ycc(int r, int g, int b, int* y, int* cb, int* cr) {
  constexpr int kHalf = 1 << 15, kOff = 128 << 16;  // ONE_HALF, CBCR_OFFSET
  *y = (19595 * r + 38470 * g + 7471 * b + kHalf) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + kOff + kHalf - 1) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + kOff + kHalf - 1) >> 16;
}

// ---- jcsample.c / jcprepct.c: where the samples of a padded plane come from -------------------------------------------------
// full-size component (Y, and chroma at 4:4:4): sample (x, y) of the padded plane is pixel (enc_src(x, W), enc_src(y, H))
DMS_JP_HD int enc_src(int i, int n) { return i < n ? i : n - 1; }
// h2v2 chroma sample (cx, cy): pixel columns x[0], x[1] and rows y[0], y[1].  Columns replicate the last PIXEL; rows replicate the
// last pixel row only up to an even number of rows, below that the last downsampled ROW.
DMS_JP_HD void h2v2_sources(int cx, int cy, int W, int H, int x[2], int y[2]) {
  x[0] = enc_src(2 * cx, W);
  x[1] = enc_src(2 * cx + 1, W);
  const int rows = (H + 1) >> 1, r = cy < rows ? cy : rows - 1;
  y[0] = enc_src(2 * r, H);
  y[1] = enc_src(2 * r + 1, H);
}
DMS_JP_HD int h2v2_box(int a, int b, int c, int d, int cx) { return (a + b + c + d + 1 + (cx & 1)) >> 2; }  // bias 1, 2, 1, 2, ...

DMS_JP_HD void enc_pixel_ycc(const unsigned char* rgb, int W, int x, int y, int flip, int* Y, int* cb, int* cr) {
  const unsigned char* p = rgb + ((size_t)y * W + x) * 3;
  rgb_to_ycc(p[flip ? 2 : 0], p[1], p[flip ? 0 : 2], Y, cb, cr);
}
// one h2v2 chroma sample pair straight from the image
DMS_JP_HD void h2v2_chroma(const unsigned char* rgb, int W, int H, int flip, int cx, int cy, int* cb, int* cr) {
  int x[2], y[2], b[4], r[4], Y;
  h2v2_sources(cx, cy, W, H, x, y);
  for (int k = 0; k < 4; ++k) enc_pixel_ycc(rgb, W, x[k & 1], y[k >> 1], flip, &Y, &b[k], &r[k]);
  *cb = h2v2_box(b[0], b[1], b[2], b[3], cx);
  *cr = h2v2_box(r[0], r[1], r[2], r[3], cx);
}

// ---- jfdctint.c ----------------------------------------------------------------------------------------------------------------
DMS_JP_HD int fdescale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one pass over 8 values; pass 1 (rows, samples already level-shifted) scales up by PASS1_BITS, pass 2 (columns) removes it
template <int PASS>
DMS_JP_HD void fdct_pass(int d[8]) {
  using namespace idct_k;
  constexpr int kOdd = PASS == 1 ? CB - P1 : CB + P1;
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (PASS == 1) {
    d[0] = (tmp10 + tmp11) * (1 << P1);
    d[4] = (tmp10 - tmp11) * (1 << P1);
  } else {
    d[0] = fdescale(tmp10 + tmp11, P1);
    d[4] = fdescale(tmp10 - tmp11, P1);
  }
  int z1 = (tmp12 + tmp13) * (int)F0_541;
  d[2] = fdescale(z1 + tmp13 * (int)F0_765, kOdd);
  d[6] = fdescale(z1 + tmp12 * -(int)F1_847, kOdd);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * (int)F1_175;
  const int t4 = tmp4 * (int)F0_298, t5 = tmp5 * (int)F2_053, t6 = tmp6 * (int)F3_072, t7 = tmp7 * (int)F1_501;
  z1 *= -(int)F0_899;
  z2 *= -(int)F2_562;
  z3 = z3 * -(int)F1_961 + z5;
  z4 = z4 * -(int)F0_390 + z5;
  d[7] = fdescale(t4 + z1 + z3, kOdd);
  d[5] = fdescale(t5 + z2 + z4, kOdd);
  d[3] = fdescale(t6 + z2 + z3, kOdd);
  d[1] = fdescale(t7 + z1 + z4, kOdd);
}

// ---- jcdctmgr.c: one coefficient ------------------------------------------------------------------------------------------------
DMS_JP_HD short enc_quantise(int v, int q) {
  const int div = q << 3;
  if (v < 0) return (short)-((-v + (div >> 1)) / div);
  return (short)((v + (div >> 1)) / div);
}

// ---- jcparam.c: jpeg_set_quality(quality, force_baseline = TRUE) ---------------------------------------------------------------
DMS_JP_HD int enc_annex_k_quant(int chroma, int i) {  // natural order
  constexpr unsigned char lum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                     81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  constexpr unsigned char chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  return chroma ? chr[i & 63] : lum[i & 63];
}
DMS_JP_HD int enc_quality_scaling(int quality) {
  if (quality <= 0) quality = 1;
  if (quality > 100) quality = 100;
  return quality < 50 ? 5000 / quality : 200 - quality * 2;
}
DMS_JP_HD void enc_quant_table(int chroma, int quality, unsigned short out[64]) {  // natural order
  const int scale = enc_quality_scaling(quality);
  for (int i = 0; i < 64; ++i) {
    int t = (enc_annex_k_quant(chroma, i) * scale + 50) / 100;
    if (t <= 0) t = 1;
    if (t > 255) t = 255;  // force_baseline
    out[i] = (unsigned short)t;
  }
}

// ---- the scan's shape (jpeg_core.hpp's Geometry; restart_interval 0) -------------------------------------------------------------
// sampling: 0 = 4:4:4, 2 = 4:2:0 (Pillow's numbering)
DMS_JP_HD void enc_geometry(int width, int height, int sampling, Geometry* out) {
  Geometry g = Geometry();
  g.width = width;
  g.height = height;
  g.hmax = g.vmax = sampling == 2 ? 2 : 1;
  g.mcux = (width + 8 * g.hmax - 1) / (8 * g.hmax);
  g.mcuy = (height + 8 * g.vmax - 1) / (8 * g.vmax);
  int nb = 0, bytes = 0;
  for (int i = 0; i < 3; ++i) {
    g.h[i] = i == 0 ? g.hmax : 1;
    g.v[i] = i == 0 ? g.vmax : 1;
    g.dw[i] = (width * g.h[i] + g.hmax - 1) / g.hmax;
    g.dh[i] = (height * g.v[i] + g.vmax - 1) / g.vmax;
    g.bw[i] = g.mcux * g.h[i];
    g.bh[i] = g.mcuy * g.v[i];
    g.off[i] = nb;
    for (int k = 0; k < g.h[i] * g.v[i]; ++k) g.mcu_comp[nb++] = (unsigned char)i;
    g.plane_off[i] = bytes;
    bytes += g.bw[i] * 8 * g.bh[i] * 8;
  }
  g.blocks_per_mcu = nb;
  g.total_blocks = nb * g.mcux * g.mcuy;
  g.plane_bytes = bytes;
  *out = g;
}

// block u of the scan (MCU order): its component and its position in the component's plane, in blocks
DMS_JP_HD void enc_block_position(const Geometry& g, int u, int* c, int* bx, int* by) {
  const int mcu = u / g.blocks_per_mcu, j = u - mcu * g.blocks_per_mcu, my = mcu / g.mcux, mx = mcu - my * g.mcux;
  *c = g.mcu_comp[j];
  const int k = j - g.off[*c], vy = k / g.h[*c];
  *bx = mx * g.h[*c] + (k - vy * g.h[*c]);
  *by = my * g.v[*c] + vy;
}
// jccoefct.c: a block that starts right of or below the component's last sample is a dummy
DMS_JP_HD bool enc_block_is_real(const Geometry& g, int c, int bx, int by) { return bx * 8 < g.dw[c] && by * 8 < g.dh[c]; }
DMS_JP_HD bool enc_block_is_real(const Geometry& g, int u) {
  int c, bx, by;
  enc_block_position(g, u, &c, &bx, &by);
  return enc_block_is_real(g, c, bx, by);
}
// The block whose DC block u is predicted from: the last REAL block of u's component before u in the scan, -1 where there is none
// (the prediction is 0).  A dummy block carries the DC of the block before it, so its own difference is 0 and the chain of
// differences skips it; the first block of a component in every MCU is real, so the walk is at most 4 steps.
DMS_JP_HD int enc_prev_real_block(const Geometry& g, int u) {
  const int bpm = g.blocks_per_mcu;
  int mcu = u / bpm, j = u - mcu * bpm;
  const int c = g.mcu_comp[j], first = g.off[c], last = first + g.h[c] * g.v[c] - 1;
  for (;;) {
    if (j > first) {
      --j;
    } else {
      if (--mcu < 0) return -1;
      j = last;
    }
    if (enc_block_is_real(g, mcu * bpm + j)) return mcu * bpm + j;
  }
}

// one 8x8 block: samples of the padded plane -> quantised coefficients in natural order (the sequential statement; the device
// runs the same two passes with 8 lanes per block)
DMS_JP_HD void enc_fdct_block(const unsigned char* plane, int stride, const unsigned short q[64], short out[64]) {
  int w[64];
  for (int r = 0; r < 8; ++r) {
    int d[8];
    for (int k = 0; k < 8; ++k) d[k] = (int)plane[(size_t)r * stride + k] - 128;
    fdct_pass<1>(d);
    for (int k = 0; k < 8; ++k) w[r * 8 + k] = d[k];
  }
  for (int c = 0; c < 8; ++c) {
    int d[8];
    for (int r = 0; r < 8; ++r) d[r] = w[r * 8 + c];
    fdct_pass<2>(d);
    for (int r = 0; r < 8; ++r) out[r * 8 + c] = enc_quantise(d[r], q[r * 8 + c]);
  }
}

// ---- jchuff.c -------------------------------------------------------------------------------------------------------------------
struct EncHuff {
  unsigned short code[256];
  unsigned char len[256];  // 0 = the symbol has no code
};
struct EncTables {
  EncHuff dc[2], ac[2];  // 0 luminance, 1 chrominance
};

// Annex K.3: (table 0 DC lum, 1 AC lum, 2 DC chroma, 3 AC chroma) -> bits[1..16] and values
DMS_JP_HD int enc_std_bits(int table, int l) {
  constexpr unsigned char bits[4][17] = {{0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                         {0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                         {0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                         {0, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
  return bits[table & 3][l];
}
DMS_JP_HD int enc_std_count(int table) { return (table & 1) ? 162 : 12; }
DMS_JP_HD int enc_std_val(int table, int i) {
  constexpr unsigned char ac_lum[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa};
  constexpr unsigned char ac_chr[162] = {
      0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa};
  if (!(table & 1)) return i;  // both DC tables: categories 0 .. 11 in order
  return table == 1 ? ac_lum[i] : ac_chr[i];
}
// jpeg_make_c_derived_tbl: codes in order of length, counting up
DMS_JP_HD void enc_derive_huff(int table, EncHuff* h) {
  for (int i = 0; i < 256; ++i) {
    h->code[i] = 0;
    h->len[i] = 0;
  }
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int n = 0; n < enc_std_bits(table, l); ++n, ++k, ++code) {
      const int v = enc_std_val(table, k);
      h->code[v] = (unsigned short)code;
      h->len[v] = (unsigned char)l;
    }
    code <<= 1;
  }
}
DMS_JP_HD void enc_std_tables(EncTables* t) {
  enc_derive_huff(0, &t->dc[0]);
  enc_derive_huff(1, &t->ac[0]);
  enc_derive_huff(2, &t->dc[1]);
  enc_derive_huff(3, &t->ac[1]);
}

DMS_JP_HD int enc_nbits(int a) {  // bits of a magnitude: 0 for 0
  int n = 0;
  while (a) {
    ++n;
    a >>= 1;
  }
  return n;
}

// bit length of one block: `blk` in natural order, `diff` its DC difference
DMS_JP_HD uint32_t enc_block_bits(const short* blk, int diff, const EncHuff& dc, const EncHuff& ac) {
  int n = enc_nbits(diff < 0 ? -diff : diff);
  uint32_t bits = (uint32_t)dc.len[n] + (uint32_t)n;
  int r = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[zigzag(k)];
    if (!v) {
      ++r;
      continue;
    }
    bits += (uint32_t)(r >> 4) * ac.len[0xf0];  // ZRL
    n = enc_nbits(v < 0 ? -v : v);
    bits += (uint32_t)ac.len[((r & 15) << 4) | n] + (uint32_t)n;
    r = 0;
  }
  if (r) bits += ac.len[0];  // EOB
  return bits;
}
// the most bits a block can take: 64 symbols of at most 16 code bits and 11 value bits
constexpr uint32_t kEncMaxBlockBits = 64 * (16 + 11);

// A block's bits go into 32-bit words holding the stream MSB first (word w = stream bytes 4 w .. 4 w + 3, big-endian).  The first
// word a block touches (when the block does not start on a word boundary) and its last, partial word may hold a neighbour's bits:
// SINK::merge(index, value) ORs into a zeroed buffer.  Every word in between is the block's alone: SINK::store(index, value).
template <class SINK>
struct BitWriter {
  SINK& sink;
  uint64_t acc;
  int fill;       // bits of `acc` not yet written
  uint32_t word;  // index of the word they go to
  bool shared;    // that word started before this block
  DMS_JP_HD BitWriter(SINK& s, uint32_t bit_offset) : sink(s), acc(0), fill((int)(bit_offset & 31)), word(bit_offset >> 5), shared((bit_offset & 31) != 0) {}
  DMS_JP_HD void put(uint32_t value, int n) {  // the low n bits of value, n <= 27
    if (!n) return;
    acc = (acc << n) | (uint64_t)(value & ((1u << n) - 1u));
    fill += n;
    if (fill >= 32) {
      const uint32_t w = (uint32_t)(acc >> (fill - 32));
      if (shared) {
        sink.merge(word, w);
      } else {
        sink.store(word, w);
      }
      shared = false;
      ++word;
      fill -= 32;
      acc &= ((uint64_t)1 << fill) - 1;
    }
  }
  DMS_JP_HD void finish() {  // the bits left over share their word with the next block
    if (fill > 0) sink.merge(word, (uint32_t)(acc << (32 - fill)));
    fill = 0;
  }
};

// one block's emission into any writer with put(value, bits): BitWriter above, or the sequential stage's byte writer
template <class WRITER>
DMS_JP_HD void enc_block_emit(const short* blk, int diff, const EncHuff& dc, const EncHuff& ac, WRITER& bw) {
  int t = diff, t2 = diff;
  if (t < 0) {
    t = -t;
    --t2;  // a negative value goes out as v - 1 in n bits
  }
  int n = enc_nbits(t);
  bw.put(dc.code[n], dc.len[n]);
  bw.put((uint32_t)t2, n);
  int r = 0;
  for (int k = 1; k < 64; ++k) {
    t = blk[zigzag(k)];
    if (!t) {
      ++r;
      continue;
    }
    while (r > 15) {
      bw.put(ac.code[0xf0], ac.len[0xf0]);
      r -= 16;
    }
    t2 = t;
    if (t < 0) {
      t = -t;
      --t2;
    }
    n = enc_nbits(t);
    const int s = (r << 4) | n;
    bw.put(ac.code[s], ac.len[s]);
    bw.put((uint32_t)t2, n);
    r = 0;
  }
  if (r) bw.put(ac.code[0], ac.len[0]);
}

// What block u of the scan contributes, from the coefficient buffer (dummy blocks hold zeros there): its DC difference.
DMS_JP_HD int enc_dc_diff(const Geometry& g, const short* coefs, int u) {
  if (!enc_block_is_real(g, u)) return 0;
  const int p = enc_prev_real_block(g, u);
  return (int)coefs[(size_t)u * 64] - (p < 0 ? 0 : (int)coefs[(size_t)p * 64]);
}
// 1-bits that fill the last byte after `total_bits` of entropy-coded data (jchuff.c flush_bits)
DMS_JP_HD int enc_pad_bits(uint32_t total_bits) { return (int)((0u - total_bits) & 7u); }

// byte i of the unstuffed stream held in MSB-first words
DMS_JP_HD unsigned char enc_stream_byte(const uint32_t* words, uint32_t i) { return (unsigned char)(words[i >> 2] >> (24 - 8 * (i & 3))); }

// ---- stuffing, per chunk of kEncChunk unstuffed bytes ---------------------------------------------------------------------------
constexpr uint32_t kEncChunk = 64;
DMS_JP_HD uint32_t enc_chunk_ff(const uint32_t* words, uint32_t chunk, uint32_t nbytes) {
  uint32_t n = 0;
  const uint32_t lo = chunk * kEncChunk, hi = lo + kEncChunk < nbytes ? lo + kEncChunk : nbytes;
  for (uint32_t i = lo; i < hi; ++i) n += enc_stream_byte(words, i) == 0xff;
  return n;
}
// writes the chunk's bytes, 00 behind each FF, at out + chunk start + ff_before; the chunk that holds the last byte appends EOI.
// Returns the length of the stuffed data with EOI where this chunk ends it, 0 otherwise.
DMS_JP_HD uint32_t enc_chunk_scatter(const uint32_t* words, uint32_t chunk, uint32_t nbytes, uint32_t ff_before, unsigned char* out) {
  const uint32_t lo = chunk * kEncChunk, hi = lo + kEncChunk < nbytes ? lo + kEncChunk : nbytes;
  if (lo >= hi) return 0;
  uint32_t o = lo + ff_before;
  for (uint32_t i = lo; i < hi; ++i) {
    const unsigned char b = enc_stream_byte(words, i);
    out[o++] = b;
    if (b == 0xff) out[o++] = 0;
  }
  if (hi != nbytes) return 0;
  out[o++] = 0xff;
  out[o++] = 0xd9;
  return o;
}

// ---- jcmarker.c: SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS ------------------------------------------------------------------
constexpr int kEncHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14;
DMS_JP_HD int enc_write_header(int width, int height, int sampling, const unsigned short qt[2][64], unsigned char* out) {
  unsigned char* p = out;
  constexpr unsigned char app0[18] = {0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  *p++ = 0xff;
  *p++ = 0xd8;
  for (int i = 0; i < 18; ++i) *p++ = app0[i];
  for (int t = 0; t < 2; ++t) {
    *p++ = 0xff;
    *p++ = 0xdb;
    *p++ = 0;
    *p++ = 67;
    *p++ = (unsigned char)t;
    for (int k = 0; k < 64; ++k) *p++ = (unsigned char)qt[t][zigzag(k)];
  }
  *p++ = 0xff;
  *p++ = 0xc0;
  *p++ = 0;
  *p++ = 17;
  *p++ = 8;
  *p++ = (unsigned char)(height >> 8);
  *p++ = (unsigned char)height;
  *p++ = (unsigned char)(width >> 8);
  *p++ = (unsigned char)width;
  *p++ = 3;
  for (int c = 0; c < 3; ++c) {
    *p++ = (unsigned char)(c + 1);
    *p++ = (unsigned char)(c == 0 && sampling == 2 ? 0x22 : 0x11);
    *p++ = (unsigned char)(c ? 1 : 0);
  }
  for (int t = 0; t < 4; ++t) {  // DC 0, AC 0, DC 1, AC 1: the order in which the components of the scan name them
    const int n = enc_std_count(t);
    *p++ = 0xff;
    *p++ = 0xc4;
    *p++ = (unsigned char)((n + 19) >> 8);
    *p++ = (unsigned char)(n + 19);
    *p++ = (unsigned char)(((t & 1) << 4) | (t >> 1));
    for (int l = 1; l <= 16; ++l) *p++ = (unsigned char)enc_std_bits(t, l);
    for (int i = 0; i < n; ++i) *p++ = (unsigned char)enc_std_val(t, i);
  }
  constexpr unsigned char sos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  for (int i = 0; i < 14; ++i) *p++ = sos[i];
  return (int)(p - out);
}

}  // namespace jpeg
}  // namespace dms
