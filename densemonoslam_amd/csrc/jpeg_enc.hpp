// The host's sequential baseline JPEG encoder over the arithmetic of csrc/jpeg_enc_core.hpp: libjpeg's bytes for 4:2:0 and 4:4:4
// at any quality, standard tables, no restart markers.  Three stages, as the device runs them: image -> padded planes,
// planes -> quantised coefficients in the scan's MCU order (dummy blocks zero), coefficients -> entropy-coded bytes.  The third
// stage is also what dms_jpeg_enc_result runs on the device encoder's coefficients with entropy_on_host = 1.
#pragma once
#include <string.h>

#include <vector>

#include "jpeg_enc_core.hpp"

namespace dms {
namespace jpeg {

// header + per block 64 symbols of at most 16 + 11 bits, doubled for stuffing, + EOI
inline size_t encode_bound(int width, int height, int sampling) {
  Geometry g;
  enc_geometry(width, height, sampling, &g);
  return (size_t)kEncHeaderBytes + (size_t)g.total_blocks * (kEncMaxBlockBits / 8) * 2 + 2;
}

inline void enc_planes(const unsigned char* rgb, const Geometry& g, int flip, unsigned char* planes) {
  const int W = g.width, H = g.height;
  unsigned char* py = planes + g.plane_off[0];
  unsigned char* pb = planes + g.plane_off[1];
  unsigned char* pr = planes + g.plane_off[2];
  const int sy = g.bw[0] * 8, sc = g.bw[1] * 8;
  for (int y = 0; y < g.bh[0] * 8; ++y)
    for (int x = 0; x < sy; ++x) {
      int Y, b, r;
      enc_pixel_ycc(rgb, W, enc_src(x, W), enc_src(y, H), flip, &Y, &b, &r);
      py[(size_t)y * sy + x] = (unsigned char)Y;
      if (g.hmax == 1) {
        pb[(size_t)y * sc + x] = (unsigned char)b;
        pr[(size_t)y * sc + x] = (unsigned char)r;
      }
    }
  if (g.hmax == 2)
    for (int cy = 0; cy < g.bh[1] * 8; ++cy)
      for (int cx = 0; cx < sc; ++cx) {
        int b, r;
        h2v2_chroma(rgb, W, H, flip, cx, cy, &b, &r);
        pb[(size_t)cy * sc + cx] = (unsigned char)b;
        pr[(size_t)cy * sc + cx] = (unsigned char)r;
      }
}

inline void enc_coefficients(const unsigned char* planes, const Geometry& g, const unsigned short qt[2][64], short* coefs) {
  for (int u = 0; u < g.total_blocks; ++u) {
    int c, bx, by;
    enc_block_position(g, u, &c, &bx, &by);
    short* out = coefs + (size_t)u * 64;
    if (!enc_block_is_real(g, c, bx, by)) {
      memset(out, 0, 64 * sizeof(short));
      continue;
    }
    const int stride = g.bw[c] * 8;
    enc_fdct_block(planes + g.plane_off[c] + (size_t)by * 8 * stride + (size_t)bx * 8, stride, qt[c ? 1 : 0], out);
  }
}

// jchuff.c's emit_bits: bytes as they complete, 00 behind FF
struct SeqBitWriter {
  unsigned char* out;
  size_t n = 0;
  uint32_t acc = 0;
  int fill = 0;
  explicit SeqBitWriter(unsigned char* o) : out(o) {}
  void put(uint32_t value, int bits) {
    if (!bits) return;
    uint64_t a = ((uint64_t)acc << bits) | (value & ((1u << bits) - 1u));
    fill += bits;
    while (fill >= 8) {
      const unsigned char b = (unsigned char)(a >> (fill - 8));
      out[n++] = b;
      if (b == 0xff) out[n++] = 0;
      fill -= 8;
    }
    acc = (uint32_t)(a & ((1u << fill) - 1u));
  }
};

// coefficients (MCU order, dummy blocks zero) -> entropy-coded data and EOI at `out` (encode_bound minus the header is enough)
inline size_t enc_entropy_sequential(const Geometry& g, const short* coefs, const EncTables& t, unsigned char* out) {
  SeqBitWriter bw(out);
  int last_dc[3] = {0, 0, 0};
  for (int u = 0; u < g.total_blocks; ++u) {
    const int c = g.mcu_comp[u % g.blocks_per_mcu];
    const short* blk = coefs + (size_t)u * 64;
    int diff = 0;
    if (enc_block_is_real(g, u)) {  // a dummy block repeats the DC before it: difference 0, prediction unchanged
      diff = blk[0] - last_dc[c];
      last_dc[c] = blk[0];
    }
    enc_block_emit(blk, diff, t.dc[c ? 1 : 0], t.ac[c ? 1 : 0], bw);
  }
  bw.put(0x7f, 7);  // flush_bits: 1-bits to the byte boundary
  bw.out[bw.n++] = 0xff;
  bw.out[bw.n++] = 0xd9;
  return bw.n;
}

// RGB8 -> the whole file at `out` (encode_bound bytes); returns its length
inline size_t encode_rgb(const unsigned char* rgb, int width, int height, int quality, int sampling, int flip, unsigned char* out) {
  Geometry g;
  enc_geometry(width, height, sampling, &g);
  unsigned short qt[2][64];
  enc_quant_table(0, quality, qt[0]);
  enc_quant_table(1, quality, qt[1]);
  EncTables t;
  enc_std_tables(&t);
  std::vector<unsigned char> planes((size_t)g.plane_bytes);
  std::vector<short> coefs((size_t)g.total_blocks * 64);
  enc_planes(rgb, g, flip, planes.data());
  enc_coefficients(planes.data(), g, qt, coefs.data());
  const int hdr = enc_write_header(width, height, sampling, qt, out);
  return (size_t)hdr + enc_entropy_sequential(g, coefs.data(), t, out + hdr);
}

}  // namespace jpeg
}  // namespace dms
