// The stages of csrc/deflate_dev.hip run on the host, one block after another, over the functions of csrc/deflate_core.hpp: what
// dms_deflate_blocks (csrc/record.hip) writes, and what tests/deflate_host.cpp runs in any block order.  Host code.
#pragma once
#include <vector>

#include "deflate_core.hpp"

namespace dms {
namespace dfl {

// k_dfl_match for block `blk`: tokens (room for kBlock), histograms, token count and Adler partial sums into *b
inline void match_stage(const unsigned char* data, size_t len, uint32_t blk, uint32_t* tok, BlockInfo* b) {
  const uint32_t s = blk * kBlock, e = (size_t)s + kBlock < len ? s + kBlock : (uint32_t)len, n = e - s, w0 = window_start(s);
  std::vector<uint32_t> head((size_t)1 << kHashBits, 0), best(n);  // head: position - w0 + 1 of the latest entry, 0 = none
  auto enter = [&](uint32_t p) {
    if (!hashable(p, (uint32_t)len)) return;
    uint32_t& h = head[hash4(data + p)];
    if (p - w0 + 1 > h) h = p - w0 + 1;
  };
  for (uint32_t p = w0; p < s; ++p) enter(p);
  for (uint32_t c = s; c < e; c += kChunk) {
    const uint32_t ce = c + kChunk < e ? c + kChunk : e;
    for (uint32_t i = c; i < ce; ++i) {
      const uint32_t h = hashable(i, (uint32_t)len) ? head[hash4(data + i)] : 0;
      best[i - s] = best_at(data, e, i, h ? h - 1 + w0 : i);
    }
    for (uint32_t i = c; i < ce; ++i) enter(i);
  }
  for (int k = 0; k < kLLSlots; ++k) b->hist_ll[k] = 0;
  for (int k = 0; k < kDSlots; ++k) b->hist_d[k] = 0;
  b->ntok = parse_block(best.data(), data + s, n, tok, b->hist_ll, b->hist_d);
  uint64_t a = 0, bb = 0;
  for (uint32_t j = 0; j < n; ++j) {
    a += data[s + j];
    bb += (uint64_t)(n - j) * data[s + j];
  }
  b->adler_a = (uint32_t)(a % kAdlerMod);
  b->adler_b = (uint32_t)(bb % kAdlerMod);
}

// k_dfl_codes for one block of n input bytes
inline void codes_stage(BlockInfo* b, uint32_t n, bool last) {
  CodeWork w;
  uint32_t cl_freq[kNumCL];
  sort_symbols(b->hist_ll, kNumLL, &w);
  build_lengths(b->hist_ll, kNumLL, kLimitLL, false, b->len_ll, &w);
  choose_block(b, n, last, &w, cl_freq);
}

struct PlainSink {
  unsigned char* out;
  void store(uint32_t i, unsigned char v) { out[i] = v; }
};

// the whole stream; out has room for stream_bound(len), len >= 1 and below 4 GiB.  Returns the stream's length.
inline size_t encode(const unsigned char* data, size_t len, unsigned char* out) {
  const uint32_t nb = num_blocks(len);
  std::vector<BlockInfo> info(nb);
  std::vector<uint32_t> tok((size_t)nb * kBlock);
  for (uint32_t k = 0; k < nb; ++k) {
    match_stage(data, len, k, &tok[(size_t)k * kBlock], &info[k]);
    codes_stage(&info[k], k + 1 < nb ? kBlock : (uint32_t)(len - (size_t)k * kBlock), k + 1 == nb);
  }
  PlainSink sink{out};
  out[0] = kZlibHeader0;
  out[1] = kZlibHeader1;
  uint32_t at = 2;
  BlockCodes codes;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t n = k + 1 < nb ? kBlock : (uint32_t)(len - (size_t)k * kBlock);
    block_codes(info[k], &codes);
    at = emit_block(info[k], codes, data + (size_t)k * kBlock, n, &tok[(size_t)k * kBlock], k + 1 == nb, at, sink);
  }
  return emit_trailer(info.data(), nb, len, at, sink);
}

}  // namespace dfl
}  // namespace dms
