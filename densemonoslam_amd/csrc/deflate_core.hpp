// A zlib (RFC 1950) stream of deflate (RFC 1951) blocks whose blocks can all be made at once, stated once for the host
// (dms_deflate_blocks, csrc/record.hip) and for the device (csrc/deflate_dev.hip), as csrc/jpeg_enc_core.hpp is for the JPEG encoder:
// plain C++ over plain data, integer only, every function __host__ __device__ under hipcc and an ordinary inline function under a
// host compiler (tests/deflate_host.cpp).  Nothing here is zlib's: the two RFCs are the whole specification.
//
//   geometry   the input is cut into blocks of kBlock bytes; block b is made from the input bytes alone (its own, and up to kWindow
//              bytes before it as the dictionary), never from another block's output
//   match      per position: the longest of three candidates - distance 1, distance 2 (a run of bytes, a run of u16 pixels) and the
//              latest earlier position with the same 4-byte hash that was entered before the position's chunk of kChunk bytes began
//              (the row above of an image, whatever its width).  A match ends with its block
//   parse      greedy with one look ahead: a match is dropped for a literal where the next position has a longer one.  The result is
//              a function of the block's position and the input, nothing else
//   codes      length-limited canonical codes from the block's two histograms (two-queue Huffman, then the lengths above the limit
//              are folded back until the Kraft sum is exactly 1), the code-length code over the run-length coded lengths
//   kinds      stored, fixed or dynamic, whichever takes the fewest bytes.  Every block but the last is followed by an empty stored
//              block, which ends on a byte: blocks start on bytes, an exclusive sum of their BYTE lengths places them, and the cost
//              of a stored block (whose padding would otherwise depend on where it starts) is known before the sum
//   wrapper    78 01, the blocks, Adler-32 from per-block partial sums
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMS_DFL_HD __host__ __device__ __forceinline__
#else
#define DMS_DFL_HD inline
#endif

namespace dms {
namespace dfl {

#ifndef DMS_DFL_BLOCK
#define DMS_DFL_BLOCK 4096
#endif
#ifndef DMS_DFL_WINDOW
#define DMS_DFL_WINDOW 32768
#endif
#ifndef DMS_DFL_HASH_BITS
#define DMS_DFL_HASH_BITS 13
#endif
constexpr uint32_t kBlock = DMS_DFL_BLOCK;    // input bytes per deflate block
constexpr uint32_t kWindow = DMS_DFL_WINDOW;  // bytes before a block that are entered into its hash table (<= 32768)
constexpr int kHashBits = DMS_DFL_HASH_BITS;
#ifndef DMS_DFL_CHUNK
#define DMS_DFL_CHUNK 64
#endif
constexpr uint32_t kChunk = DMS_DFL_CHUNK;  // positions that look the table up together, before any of them is entered
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kFar3 = 256;  // a match of 3 bytes further back than this costs more than three literals usually do
constexpr int kNumLL = 286, kNumD = 30, kNumCL = 19, kLLSlots = 288, kDSlots = 32;
constexpr int kLimitLL = 15, kLimitCL = 7;
constexpr uint32_t kAdlerMod = 65521;
static_assert(kBlock >= 256 && kBlock <= 32768 && kBlock % kChunk == 0, "a stored block holds at most 65535 bytes; chunks tile a block");
static_assert(kWindow <= kMaxDist, "the dictionary of deflate");

enum Kind { kStored = 0, kFixed = 1, kDynamic = 2 };

// What the stages hand to one another about one block.
struct BlockInfo {
  uint32_t hist_ll[kLLSlots], hist_d[kDSlots];
  uint32_t ntok, adler_a, adler_b, kind, bytes, pad[3];
  unsigned char len_ll[kLLSlots], len_d[kDSlots], len_cl[32];
};

DMS_DFL_HD uint32_t num_blocks(size_t len) { return (uint32_t)((len + kBlock - 1) / kBlock); }
// stored blocks of kBlock bytes, the header and the checksum
DMS_DFL_HD size_t stream_bound(size_t len) { return len + (size_t)num_blocks(len) * 5 + 6; }

// ---- matching ------------------------------------------------------------------------------------------------------------------
DMS_DFL_HD uint32_t load32(const unsigned char* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
DMS_DFL_HD uint64_t load64(const unsigned char* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
DMS_DFL_HD uint32_t hash4(const unsigned char* p) { return (load32(p) * 2654435761u) >> (32 - kHashBits); }

// bytes that a and b have in common, at most cap; b may overlap a from below
DMS_DFL_HD uint32_t match_len(const unsigned char* a, const unsigned char* b, uint32_t cap) {
  uint32_t n = 0;
  while (n + 8 <= cap) {
    const uint64_t x = load64(a + n) ^ load64(b + n);
    if (x) return n + ((uint32_t)__builtin_ctzll(x) >> 3);
    n += 8;
  }
  while (n < cap && a[n] == b[n]) ++n;
  return n;
}

// a match as one word: (length << 15) | (distance - 1); 0 = none
DMS_DFL_HD uint32_t pack_match(uint32_t len, uint32_t dist) { return (len << 15) | (dist - 1); }
DMS_DFL_HD uint32_t match_length(uint32_t m) { return m >> 15; }
DMS_DFL_HD uint32_t match_dist(uint32_t m) { return (m & 0x7fffu) + 1; }

// The match of position i (block_end: the end of i's block).  table_pos: the position the hash table gave for i, or i itself for none.
DMS_DFL_HD uint32_t best_at(const unsigned char* data, uint32_t block_end, uint32_t i, uint32_t table_pos) {
  const uint32_t cap = block_end - i < kMaxMatch ? block_end - i : kMaxMatch;
  if (cap < kMinMatch) return 0;
  uint32_t len = 0, dist = 0;
  for (uint32_t d = 1; d <= 2; ++d) {
    if (i < d) break;
    const uint32_t l = match_len(data + i, data + i - d, cap);
    if (l > len) {
      len = l;
      dist = d;
    }
  }
  if (len < cap && table_pos < i && i - table_pos <= kMaxDist) {
    const uint32_t l = match_len(data + i, data + table_pos, cap);
    if (l > len) {
      len = l;
      dist = i - table_pos;
    }
  }
  if (len < kMinMatch || (len == kMinMatch && dist > kFar3)) return 0;
  return pack_match(len, dist);
}

// first position whose hash a block starting at s enters before it looks anything up
DMS_DFL_HD uint32_t window_start(uint32_t s) { return s > kWindow ? s - kWindow : 0; }
// position p has four bytes to hash
DMS_DFL_HD bool hashable(uint32_t p, uint32_t len) { return p + 4 <= len; }

// ---- symbols -------------------------------------------------------------------------------------------------------------------
DMS_DFL_HD int floor_log2(uint32_t v) { return 31 - __builtin_clz(v); }
DMS_DFL_HD void length_symbol(uint32_t len, int* sym, int* nbits, uint32_t* extra) {
  const uint32_t l = len - 3;
  if (len == 258) {
    *sym = 285;
    *nbits = 0;
    *extra = 0;
  } else if (l < 8) {
    *sym = 257 + (int)l;
    *nbits = 0;
    *extra = 0;
  } else {
    const int k = floor_log2(l) - 2;
    *sym = 261 + 4 * k + (int)((l >> k) & 3);
    *nbits = k;
    *extra = l & ((1u << k) - 1);
  }
}
DMS_DFL_HD void dist_symbol(uint32_t dist, int* sym, int* nbits, uint32_t* extra) {
  const uint32_t d = dist - 1;
  if (d < 4) {
    *sym = (int)d;
    *nbits = 0;
    *extra = 0;
  } else {
    const int k = floor_log2(d) - 1;
    *sym = 2 * k + 2 + (int)((d >> k) & 1);
    *nbits = k;
    *extra = d & ((1u << k) - 1);
  }
}
DMS_DFL_HD int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
DMS_DFL_HD int dist_extra_bits(int sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }
DMS_DFL_HD int fixed_ll_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// a token: a literal byte, or 0x80000000 | packed match
constexpr uint32_t kMatchFlag = 0x80000000u;

// ---- the parse of one block -------------------------------------------------------------------------------------------------------
// best[0 .. n): best_at of the block's positions.  How far the parse moves from position j when it gets there: the match's length,
// or 1 for a literal - greedy, but a match gives way to a longer one at the next position.
DMS_DFL_HD uint32_t parse_step(const uint32_t* best, uint32_t j, uint32_t n) {
  const uint32_t m = best[j];
  if (!m || (j + 1 < n && match_length(best[j + 1]) > match_length(m))) return 1;
  return match_length(m);
}
// The sequential statement: writes the tokens and counts the symbols (the histograms come zeroed), the end-of-block symbol
// included; returns the number of tokens.  The device finds the same positions by pointer doubling (k_dfl_match).
DMS_DFL_HD uint32_t parse_block(const uint32_t* best, const unsigned char* bytes, uint32_t n, uint32_t* tok, uint32_t* hist_ll, uint32_t* hist_d) {
  uint32_t nt = 0, i = 0;
  while (i < n) {
    const uint32_t step = parse_step(best, i, n);
    if (step > 1) {
      const uint32_t m = best[i];
      int s, nb;
      uint32_t ex;
      length_symbol(match_length(m), &s, &nb, &ex);
      hist_ll[s] += 1;
      dist_symbol(match_dist(m), &s, &nb, &ex);
      hist_d[s] += 1;
      tok[nt++] = kMatchFlag | m;
    } else {
      hist_ll[bytes[i]] += 1;
      tok[nt++] = bytes[i];
    }
    i += step;
  }
  hist_ll[256] += 1;
  return nt;
}

// ---- Adler-32 in pieces -----------------------------------------------------------------------------------------------------------
// byte j of a piece of n bytes adds x to a and (n - j) x to b; a piece then moves (s1, s2) by the modular shift below
DMS_DFL_HD void adler_combine(uint32_t* s1, uint32_t* s2, uint32_t a, uint32_t b, uint32_t n) {
  *s2 = (uint32_t)((*s2 + (uint64_t)(n % kAdlerMod) * *s1 + b) % kAdlerMod);
  *s1 = (*s1 + a) % kAdlerMod;
}

// ---- length-limited canonical codes ----------------------------------------------------------------------------------------------
struct CodeWork {
  uint16_t order[kLLSlots];      // used symbols, ascending by (count, symbol)
  uint32_t weight[2 * kLLSlots];  // leaves in that order, then the internal nodes in the order they are made
  uint16_t up[2 * kLLSlots];      // parent, then depth
};

// place of symbol s among the used symbols (count > 0) ordered by (count, symbol); s must be used
DMS_DFL_HD int symbol_rank(const uint32_t* freq, int n, int s) {
  int r = 0;
  const uint32_t f = freq[s];
  for (int t = 0; t < n; ++t) r += freq[t] != 0 && (freq[t] < f || (freq[t] == f && t < s));
  return r;
}
DMS_DFL_HD void sort_symbols(const uint32_t* freq, int n, CodeWork* w) {
  for (int s = 0; s < n; ++s)
    if (freq[s]) w->order[symbol_rank(freq, n, s)] = (uint16_t)s;
}

// lens[0 .. n) from freq[0 .. n), no length above `limit` (2^limit >= n).  w->order holds the used symbols (sort_symbols).
// With two or more used symbols the code is complete (Kraft sum 1).  With one: that symbol gets length 1, and so does a second,
// unused one unless `lone_code_ok` (the distance code, RFC 1951 3.2.7).  With none (`lone_code_ok` only): symbol 0 gets length 1.
DMS_DFL_HD void build_lengths(const uint32_t* freq, int n, int limit, bool lone_code_ok, unsigned char* lens, CodeWork* w) {
  int m = 0;
  for (int s = 0; s < n; ++s) {
    lens[s] = 0;
    m += freq[s] != 0;
  }
  if (m == 0) {
    lens[0] = 1;
    if (!lone_code_ok) lens[1] = 1;
    return;
  }
  if (m == 1) {
    const int s = w->order[0];
    lens[s] = 1;
    if (!lone_code_ok) lens[s ? 0 : 1] = 1;
    return;
  }
  for (int k = 0; k < m; ++k) w->weight[k] = freq[w->order[k]];
  // two queues: the leaves and the internal nodes are each in ascending order of weight; a leaf wins a tie
  int leaf = 0, node = m;
  for (int k = m; k < 2 * m - 1; ++k) {
    uint32_t sum = 0;
    for (int pick = 0; pick < 2; ++pick) {
      int x;
      if (leaf < m && (node >= k || w->weight[leaf] <= w->weight[node])) {
        x = leaf++;
      } else {
        x = node++;
      }
      sum += w->weight[x];
      w->up[x] = (uint16_t)k;
    }
    w->weight[k] = sum;
  }
  uint32_t count[16];
  for (int l = 0; l < 16; ++l) count[l] = 0;
  w->up[2 * m - 2] = 0;
  for (int k = 2 * m - 3; k >= 0; --k) {
    const int d = w->up[w->up[k]] + 1;
    w->up[k] = (uint16_t)d;
    if (k < m) count[d < limit ? d : limit] += 1;
  }
  // fold the overlong codes back: each round takes one code off the limit and splits the deepest shorter code, which lowers the
  // Kraft sum (in units of 2^-limit) by exactly one
  uint32_t total = 0;
  for (int l = 1; l <= limit; ++l) total += count[l] << (limit - l);
  while (total > (1u << limit)) {
    count[limit] -= 1;
    for (int l = limit - 1; l >= 1; --l) {
      if (count[l]) {
        count[l] -= 1;
        count[l + 1] += 2;
        break;
      }
    }
    total -= 1;
  }
  // the rarest symbols take the longest codes
  int k = 0;
  for (int l = limit; l >= 1; --l)
    for (uint32_t c = 0; c < count[l]; ++c) lens[w->order[k++]] = (unsigned char)l;
}

DMS_DFL_HD uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}
// canonical codes (RFC 1951 3.2.2), already bit-reversed for the LSB-first stream
DMS_DFL_HD void assign_codes(const unsigned char* lens, int n, uint16_t* codes) {
  uint32_t count[16], next[16];
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int s = 0; s < n; ++s) count[lens[s]] += 1;
  count[0] = 0;
  uint32_t code = 0;
  next[0] = 0;
  for (int l = 1; l < 16; ++l) {
    code = (code + count[l - 1]) << 1;
    next[l] = code;
  }
  for (int s = 0; s < n; ++s) codes[s] = lens[s] ? (uint16_t)reverse_bits(next[lens[s]]++, lens[s]) : (uint16_t)0;
}
// Kraft sum of a code in units of 2^-15
DMS_DFL_HD uint32_t kraft_sum(const unsigned char* lens, int n) {
  uint32_t t = 0;
  for (int s = 0; s < n; ++s)
    if (lens[s]) t += 1u << (15 - lens[s]);
  return t;
}

// ---- the dynamic header -----------------------------------------------------------------------------------------------------------
DMS_DFL_HD int cl_order(int i) {
  constexpr unsigned char o[kNumCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i];
}
struct HeaderShape {
  int hlit, hdist, hclen;  // the counts themselves: 257 .., 1 .., 4 ..
};
DMS_DFL_HD void header_counts(const unsigned char* len_ll, const unsigned char* len_d, int* hlit, int* hdist) {
  int a = kNumLL, b = kNumD;
  while (a > 257 && !len_ll[a - 1]) --a;
  while (b > 1 && !len_d[b - 1]) --b;
  *hlit = a;
  *hdist = b;
}
// The code lengths of both codes as one sequence, run-length coded with 16, 17 and 18 across the boundary: f(symbol, extra bits' value,
// number of extra bits) per item
template <class F>
DMS_DFL_HD void rle_lengths(const unsigned char* len_ll, int hlit, const unsigned char* len_d, int hdist, F& f) {
  const int n = hlit + hdist;
  int i = 0;
  while (i < n) {
    const int v = i < hlit ? len_ll[i] : len_d[i - hlit];
    int run = 1;
    while (i + run < n && (i + run < hlit ? len_ll[i + run] : len_d[i + run - hlit]) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        f(18, (uint32_t)(r - 11), 7);
        run -= r;
      }
      if (run >= 3) {
        f(17, (uint32_t)(run - 3), 3);
        run = 0;
      }
      for (; run > 0; --run) f(0, 0u, 0);
    } else {
      f(v, 0u, 0);
      run -= 1;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        f(16, (uint32_t)(r - 3), 2);
        run -= r;
      }
      for (; run > 0; --run) f(v, 0u, 0);
    }
  }
}
struct ClCount {
  uint32_t* freq;
  DMS_DFL_HD void operator()(int sym, uint32_t, int) { freq[sym] += 1; }
};
struct ClBits {
  const unsigned char* len_cl;
  uint32_t bits;
  DMS_DFL_HD void operator()(int sym, uint32_t, int nbits) { bits += (uint32_t)len_cl[sym] + (uint32_t)nbits; }
};
DMS_DFL_HD int header_hclen(const unsigned char* len_cl) {
  int h = kNumCL;
  while (h > 4 && !len_cl[cl_order(h - 1)]) --h;
  return h;
}

// bytes a block of n input bytes takes as each kind; `last`: it ends the stream, else an empty stored block follows a Huffman block
DMS_DFL_HD uint32_t huffman_bytes(uint32_t bits_after_type, bool last) { return last ? (3 + bits_after_type + 7) >> 3 : ((3 + bits_after_type + 3 + 7) >> 3) + 4; }
DMS_DFL_HD uint32_t stored_bytes(uint32_t n) { return n + 5; }

// From a block's histograms and its literal/length code (b->len_ll, built by the caller, who may sort its symbols in parallel): the
// other two codes, and the kind that takes the fewest bytes (stored, then fixed, wins a tie).
DMS_DFL_HD void choose_block(BlockInfo* b, uint32_t n, bool last, CodeWork* w, uint32_t* cl_freq) {
  sort_symbols(b->hist_d, kNumD, w);
  build_lengths(b->hist_d, kNumD, kLimitLL, true, b->len_d, w);
  int hlit, hdist;
  header_counts(b->len_ll, b->len_d, &hlit, &hdist);
  for (int s = 0; s < kNumCL; ++s) cl_freq[s] = 0;
  ClCount cc{cl_freq};
  rle_lengths(b->len_ll, hlit, b->len_d, hdist, cc);
  sort_symbols(cl_freq, kNumCL, w);
  build_lengths(cl_freq, kNumCL, kLimitCL, false, b->len_cl, w);
  ClBits cb{b->len_cl, 0};
  rle_lengths(b->len_ll, hlit, b->len_d, hdist, cb);
  uint32_t dyn = 14 + 3 * (uint32_t)header_hclen(b->len_cl) + cb.bits, fix = 0;
  for (int s = 0; s < kNumLL; ++s) {
    const uint32_t e = (uint32_t)(s > 256 ? length_extra_bits(s) : 0);
    dyn += b->hist_ll[s] * (b->len_ll[s] + e);
    fix += b->hist_ll[s] * ((uint32_t)fixed_ll_len(s) + e);
  }
  for (int s = 0; s < kNumD; ++s) {
    dyn += b->hist_d[s] * (b->len_d[s] + (uint32_t)dist_extra_bits(s));
    fix += b->hist_d[s] * (5 + (uint32_t)dist_extra_bits(s));
  }
  const uint32_t sb = stored_bytes(n), fb = huffman_bytes(fix, last), db = huffman_bytes(dyn, last);
  b->kind = kStored;
  b->bytes = sb;
  if (fb < b->bytes) {
    b->kind = kFixed;
    b->bytes = fb;
  }
  if (db < b->bytes) {
    b->kind = kDynamic;
    b->bytes = db;
  }
}

// ---- writing --------------------------------------------------------------------------------------------------------------------
// Bits go out LSB first into bytes; SINK::store(index, byte) owns every byte it is given: blocks start and end on bytes.
template <class SINK>
struct ByteWriter {
  SINK& sink;
  uint64_t acc;
  int fill;
  uint32_t at;
  DMS_DFL_HD ByteWriter(SINK& s, uint32_t byte_offset) : sink(s), acc(0), fill(0), at(byte_offset) {}
  DMS_DFL_HD void put(uint32_t value, int n) {  // the low n bits of value, n <= 16
    acc |= (uint64_t)(value & ((1u << n) - 1u)) << fill;
    fill += n;
    while (fill >= 8) {
      sink.store(at++, (unsigned char)acc);
      acc >>= 8;
      fill -= 8;
    }
  }
  DMS_DFL_HD void align() {
    if (fill > 0) {
      sink.store(at++, (unsigned char)acc);
      acc = 0;
      fill = 0;
    }
  }
  DMS_DFL_HD void byte(unsigned char v) { sink.store(at++, v); }  // after align()
};

struct BlockCodes {
  uint16_t code_ll[kLLSlots], code_d[kDSlots], code_cl[32];
  unsigned char len_ll[kLLSlots], len_d[kDSlots], len_cl[32];
};
DMS_DFL_HD void block_codes(const BlockInfo& b, BlockCodes* c) {
  if (b.kind == kFixed) {
    for (int s = 0; s < kLLSlots; ++s) c->len_ll[s] = (unsigned char)fixed_ll_len(s);
    for (int s = 0; s < kDSlots; ++s) c->len_d[s] = 5;
    assign_codes(c->len_ll, kLLSlots, c->code_ll);
    assign_codes(c->len_d, kDSlots, c->code_d);
    return;
  }
  for (int s = 0; s < kLLSlots; ++s) c->len_ll[s] = b.len_ll[s];
  for (int s = 0; s < kDSlots; ++s) c->len_d[s] = b.len_d[s];
  for (int s = 0; s < 32; ++s) c->len_cl[s] = b.len_cl[s];
  assign_codes(c->len_ll, kNumLL, c->code_ll);
  assign_codes(c->len_d, kNumD, c->code_d);
  assign_codes(c->len_cl, kNumCL, c->code_cl);
}
template <class WRITER>
struct ClEmit {
  const BlockCodes* c;
  WRITER* bw;
  DMS_DFL_HD void operator()(int sym, uint32_t extra, int nbits) {
    bw->put(c->code_cl[sym], c->len_cl[sym]);
    if (nbits) bw->put(extra, nbits);
  }
};

// One block at byte `offset` of the stream: `bytes` its n input bytes, `tok` its tokens, `c` its codes (block_codes; unused for a
// stored block).  Returns the offset behind it.
template <class SINK>
DMS_DFL_HD uint32_t emit_block(const BlockInfo& b, const BlockCodes& c, const unsigned char* bytes, uint32_t n, const uint32_t* tok, bool last,
                               uint32_t offset, SINK& sink) {
  ByteWriter<SINK> bw(sink, offset);
  if (b.kind == kStored) {
    bw.byte(last ? 1 : 0);
    bw.byte((unsigned char)n);
    bw.byte((unsigned char)(n >> 8));
    bw.byte((unsigned char)~n);
    bw.byte((unsigned char)(~n >> 8));
    for (uint32_t i = 0; i < n; ++i) bw.byte(bytes[i]);
    return bw.at;
  }
  bw.put((last ? 1u : 0u) | (b.kind << 1), 3);
  if (b.kind == kDynamic) {
    int hlit, hdist;
    header_counts(c.len_ll, c.len_d, &hlit, &hdist);
    const int hclen = header_hclen(c.len_cl);
    bw.put((uint32_t)(hlit - 257), 5);
    bw.put((uint32_t)(hdist - 1), 5);
    bw.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) bw.put(c.len_cl[cl_order(i)], 3);
    ClEmit<ByteWriter<SINK> > ce{&c, &bw};
    rle_lengths(c.len_ll, hlit, c.len_d, hdist, ce);
  }
  for (uint32_t t = 0; t < b.ntok; ++t) {
    const uint32_t k = tok[t];
    if (k & kMatchFlag) {
      int s, nb;
      uint32_t ex;
      length_symbol(match_length(k & ~kMatchFlag), &s, &nb, &ex);
      bw.put(c.code_ll[s], c.len_ll[s]);
      if (nb) bw.put(ex, nb);
      dist_symbol(match_dist(k), &s, &nb, &ex);
      bw.put(c.code_d[s], c.len_d[s]);
      if (nb) bw.put(ex, nb);
    } else {
      bw.put(c.code_ll[k], c.len_ll[k]);
    }
  }
  bw.put(c.code_ll[256], c.len_ll[256]);
  if (!last) {  // an empty stored block: the next block starts on a byte
    bw.put(0, 3);
    bw.align();
    bw.byte(0);
    bw.byte(0);
    bw.byte(0xff);
    bw.byte(0xff);
  } else {
    bw.align();
  }
  return bw.at;
}

// after the last block: Adler-32 of the whole input, big-endian, from the blocks' partial sums
template <class SINK>
DMS_DFL_HD uint32_t emit_trailer(const BlockInfo* blocks, uint32_t nb, size_t len, uint32_t offset, SINK& sink) {
  uint32_t s1 = 1, s2 = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t n = k + 1 < nb ? kBlock : (uint32_t)(len - (size_t)k * kBlock);
    adler_combine(&s1, &s2, blocks[k].adler_a, blocks[k].adler_b, n);
  }
  sink.store(offset, (unsigned char)(s2 >> 8));
  sink.store(offset + 1, (unsigned char)s2);
  sink.store(offset + 2, (unsigned char)(s1 >> 8));
  sink.store(offset + 3, (unsigned char)s1);
  return offset + 4;
}
// deflate, 32 KB window; FLEVEL 0, FCHECK makes 0x7801 a multiple of 31
constexpr unsigned char kZlibHeader0 = 0x78, kZlibHeader1 = 0x01;

}  // namespace dfl
}  // namespace dms
