// The block deflate encoder of densemonoslam_amd/csrc/deflate_core.hpp on the host, under the sanitizers
// (tests/test_deflate_cpu.py builds this with them).
//
//   deflate_host [NAME FILE] ...
//
// First the length-limited code builder on crafted counts: no length above the limit, Kraft sum exactly 1 (or the one-code
// distance case), canonical codes in order, no rarer symbol with a shorter code.  Prints "codes ok".
// Then, per file: the per-block stages of csrc/deflate_dev.hip (csrc/deflate.hpp: match_stage, codes_stage, exclusive sums,
// emit_block, emit_trailer) with the blocks in REVERSE order, since no block may depend on another having run, through a sink that
// owns bytes: a byte written twice, or never, fails.  The result is compared with the sequential encoder's (dfl::encode, what
// dms_deflate_blocks returns).  Prints "NAME blocks bytes ok" and exits 1 on the first difference.  Every buffer has exactly the
// size the device code assumes, so the sanitizers see any access outside.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "densemonoslam_amd/csrc/deflate.hpp"

using namespace dms::dfl;

static std::vector<unsigned char> read_file(const char* path, bool* ok) {
  std::vector<unsigned char> v;
  FILE* f = std::fopen(path, "rb");
  *ok = f != nullptr;
  if (!f) return v;
  unsigned char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

static int check_code(const char* name, const std::vector<uint32_t>& freq, int limit, bool lone_ok) {
  const int n = (int)freq.size();
  CodeWork w;
  std::vector<unsigned char> lens((size_t)n);
  std::vector<uint16_t> codes((size_t)n);
  sort_symbols(freq.data(), n, &w);
  build_lengths(freq.data(), n, limit, lone_ok, lens.data(), &w);
  assign_codes(lens.data(), n, codes.data());
  int used = 0, coded = 0;
  for (int s = 0; s < n; ++s) {
    used += freq[(size_t)s] != 0;
    coded += lens[(size_t)s] != 0;
    if (lens[(size_t)s] > limit || (freq[(size_t)s] && !lens[(size_t)s])) {
      std::printf("%s: symbol %d (count %u) has length %d, limit %d\n", name, s, freq[(size_t)s], lens[(size_t)s], limit);
      return 1;
    }
  }
  const uint32_t kraft = kraft_sum(lens.data(), n);
  if (used >= 2 || !lone_ok) {
    if (kraft != (1u << 15) || coded != (used >= 2 ? used : 2)) {
      std::printf("%s: Kraft sum %u / 32768 with %d codes for %d used symbols\n", name, kraft, coded, used);
      return 1;
    }
  } else if (coded != 1 || kraft != (1u << 14)) {
    std::printf("%s: the lone distance code must be one code of length 1 (%d codes, Kraft %u / 32768)\n", name, coded, kraft);
    return 1;
  }
  // canonical: in order of (length, symbol) each code is the one before it plus one, shifted to its own length
  int prev = -1;
  for (int l = 1; l <= limit; ++l) {
    for (int s = 0; s < n; ++s) {
      if (lens[(size_t)s] != l) continue;
      const uint32_t code = reverse_bits(codes[(size_t)s], l);
      if (prev < 0 ? code != 0 : code != ((reverse_bits(codes[(size_t)prev], lens[(size_t)prev]) + 1) << (l - lens[(size_t)prev]))) {
        std::printf("%s: symbol %d breaks the canonical order\n", name, s);
        return 1;
      }
      prev = s;
    }
  }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      if (freq[(size_t)a] > freq[(size_t)b] && freq[(size_t)b] && lens[(size_t)a] > lens[(size_t)b]) {
        std::printf("%s: symbol %d (count %u) has a longer code than symbol %d (count %u)\n", name, a, freq[(size_t)a], b, freq[(size_t)b]);
        return 1;
      }
  return 0;
}

static int check_codes() {
  std::vector<uint32_t> f;
  int bad = 0;
  f.assign(286, 0);  // Fibonacci counts: an unlimited code would be 34 deep
  for (uint32_t k = 0, a = 1, b = 1; k < 35; ++k) {
    f[(size_t)(k * 7)] = a;
    const uint32_t c = a + b;
    a = b;
    b = c;
  }
  bad += check_code("fibonacci_35_of_286", f, kLimitLL, false);
  f.assign(286, 7);
  bad += check_code("all_equal_286", f, kLimitLL, false);
  f.assign(286, 1);
  bad += check_code("286_of_count_1", f, kLimitLL, false);
  f.assign(286, 0);
  f[256] = 1;
  bad += check_code("one_symbol", f, kLimitLL, false);
  f[0] = 1;
  f[256] = 0;
  bad += check_code("one_symbol_0", f, kLimitLL, false);
  f[285] = 4000;
  bad += check_code("two_symbols", f, kLimitLL, false);
  f[100] = 3;
  bad += check_code("three_symbols", f, kLimitLL, false);
  f.assign(19, 0);  // the code-length alphabet at its limit of 7
  for (uint32_t k = 0, a = 1, b = 1; k < 19; ++k) {
    f[k] = a;
    const uint32_t c = a + b;
    a = b;
    b = c;
  }
  bad += check_code("fibonacci_19_limit_7", f, kLimitCL, false);
  f.assign(19, 5);
  bad += check_code("all_equal_19_limit_7", f, kLimitCL, false);
  f.assign(19, 0);
  f[8] = 30;
  bad += check_code("one_code_length_symbol", f, kLimitCL, false);
  f.assign(30, 0);
  bad += check_code("no_distance", f, kLimitLL, true);
  f[17] = 9;
  bad += check_code("one_distance", f, kLimitLL, true);
  f[0] = 1;
  bad += check_code("two_distances", f, kLimitLL, true);
  for (int s = 0; s < 30; ++s) f[(size_t)s] = 1u << s;
  bad += check_code("powers_of_two_30", f, kLimitLL, true);
  if (!bad) std::printf("codes ok\n");
  return bad;
}

struct OwningSink {
  std::vector<unsigned char>& out;
  std::vector<char>& written;
  bool ok = true;
  OwningSink(std::vector<unsigned char>& o, std::vector<char>& w) : out(o), written(w) {}
  void store(uint32_t i, unsigned char v) {
    if (written.at(i)) ok = false;
    out.at(i) = v;
    written.at(i) = 1;
  }
};

static int run(const char* name, const std::vector<unsigned char>& data) {
  const size_t len = data.size();
  std::vector<unsigned char> seq(stream_bound(len));
  seq.resize(encode(data.data(), len, seq.data()));

  const uint32_t nb = num_blocks(len);
  std::vector<BlockInfo> info(nb);
  std::vector<uint32_t> tok((size_t)nb * kBlock), off(nb);
  auto bytes_of = [&](uint32_t k) { return k + 1 < nb ? kBlock : (uint32_t)(len - (size_t)k * kBlock); };
  for (uint32_t k = nb; k-- > 0;) {
    match_stage(data.data(), len, k, &tok[(size_t)k * kBlock], &info[k]);
    codes_stage(&info[k], bytes_of(k), k + 1 == nb);
  }
  uint32_t total = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    off[k] = total;
    total += info[k].bytes;
  }
  if ((size_t)total + 6 > stream_bound(len)) {
    std::printf("%s: %u bytes of blocks, the bound is %zu\n", name, total, stream_bound(len));
    return 1;
  }
  std::vector<unsigned char> out((size_t)total + 6);
  std::vector<char> written(out.size(), 0);
  OwningSink sink(out, written);
  BlockCodes codes;
  for (uint32_t k = nb; k-- > 0;) {
    block_codes(info[k], &codes);
    const uint32_t end = emit_block(info[k], codes, data.data() + (size_t)k * kBlock, bytes_of(k), &tok[(size_t)k * kBlock], k + 1 == nb, 2 + off[k], sink);
    if (end != 2 + off[k] + info[k].bytes) {
      std::printf("%s: block %u wrote up to byte %u, its length says %u\n", name, k, end, 2 + off[k] + info[k].bytes);
      return 1;
    }
    if (k + 1 == nb && emit_trailer(info.data(), nb, len, end, sink) != out.size()) return 1;
    if (k == 0) {
      sink.store(0, kZlibHeader0);
      sink.store(1, kZlibHeader1);
    }
  }
  for (size_t i = 0; i < written.size(); ++i) sink.ok = sink.ok && written[i];
  if (!sink.ok) {
    std::printf("%s: a byte was written twice or never\n", name);
    return 1;
  }
  if (out != seq) {
    std::printf("%s: %zu bytes from the per-block stages, %zu from the sequential encoder, or different bytes\n", name, out.size(), seq.size());
    return 1;
  }
  std::printf("%s %u %zu ok\n", name, nb, out.size());
  return 0;
}

int main(int argc, char** argv) {
  if ((argc - 1) % 2) {
    std::printf("usage: %s [NAME FILE] ...\n", argv[0]);
    return 2;
  }
  if (check_codes()) return 1;
  for (int a = 1; a + 1 < argc; a += 2) {
    bool ok;
    const std::vector<unsigned char> data = read_file(argv[a + 1], &ok);
    if (!ok || data.empty()) {
      std::printf("cannot read %s\n", argv[a + 1]);
      return 2;
    }
    if (run(argv[a], data)) return 1;
  }
  return 0;
}
