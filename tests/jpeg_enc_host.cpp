// The device entropy stage of densemonoslam_amd/csrc/jpeg_enc_dev.hip restated with its blocks and chunks run one after another,
// on the host: the same per-block functions (csrc/jpeg_enc_core.hpp: enc_dc_diff, enc_block_bits, BitWriter + enc_block_emit,
// enc_chunk_ff, enc_chunk_scatter), the same passes in the same order - lengths, exclusive sums, bit write into a zeroed word
// buffer, padding, FF counts per chunk, exclusive sums, scatter - and after each image a comparison with the sequential entropy
// stage (csrc/jpeg_enc.hpp) and with the file libjpeg wrote.
//
//   jpeg_enc_host NAME WIDTH HEIGHT QUALITY SUBSAMPLING RGBFILE JPEGFILE [...]
//
// prints "NAME blocks bits stuffed ok" per image and exits 1 on the first difference.  The sink checks what the device relies on:
// a plain store goes to a word nobody else touches, an OR never meets a stored word.  Every buffer has exactly the size the
// device code assumes, so the sanitizers (tests/test_jpeg_encode_cpu.py builds with them) see any access outside.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "densemonoslam_amd/csrc/jpeg_enc.hpp"

using namespace dms::jpeg;

static std::vector<unsigned char> read_file(const char* path) {
  std::vector<unsigned char> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  unsigned char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

struct HostSink {
  std::vector<uint32_t>& words;
  std::vector<char>& state;  // 0 untouched, 1 merged into, 2 stored
  bool ok = true;
  HostSink(std::vector<uint32_t>& w, std::vector<char>& s) : words(w), state(s) {}
  void merge(uint32_t i, uint32_t v) {
    if (state.at(i) == 2 || (words.at(i) & v)) ok = false;
    words.at(i) |= v;
    state.at(i) = 1;
  }
  void store(uint32_t i, uint32_t v) {
    if (state.at(i) != 0) ok = false;
    words.at(i) = v;
    state.at(i) = 2;
  }
};

static int run(const char* name, int width, int height, int quality, int sampling, const std::vector<unsigned char>& rgb,
               const std::vector<unsigned char>& want_file) {
  Geometry g;
  enc_geometry(width, height, sampling, &g);
  unsigned short qt[2][64];
  enc_quant_table(0, quality, qt[0]);
  enc_quant_table(1, quality, qt[1]);
  EncTables t;
  enc_std_tables(&t);
  std::vector<unsigned char> planes((size_t)g.plane_bytes);
  std::vector<short> coefs((size_t)g.total_blocks * 64);
  enc_planes(rgb.data(), g, 0, planes.data());
  enc_coefficients(planes.data(), g, qt, coefs.data());
  const int nb = g.total_blocks;

  // the sequential stage
  std::vector<unsigned char> seq((size_t)nb * (kEncMaxBlockBits / 8) * 2 + 2);
  seq.resize(enc_entropy_sequential(g, coefs.data(), t, seq.data()));

  // lengths -> exclusive sums
  std::vector<uint32_t> bits((size_t)nb), off((size_t)nb);
  uint32_t total = 0;
  for (int u = 0; u < nb; ++u) {
    const int c = g.mcu_comp[u % g.blocks_per_mcu] ? 1 : 0;
    bits[(size_t)u] = enc_block_bits(&coefs[(size_t)u * 64], enc_dc_diff(g, coefs.data(), u), t.dc[c], t.ac[c]);
    if (bits[(size_t)u] > kEncMaxBlockBits) {
      std::printf("%s: block %d takes %u bits\n", name, u, bits[(size_t)u]);
      return 1;
    }
    off[(size_t)u] = total;
    total += bits[(size_t)u];
  }
  // bit write; the blocks in reverse order, since no block may depend on another having written
  const int pad = enc_pad_bits(total);
  const uint32_t nbytes = (total + 7) >> 3;
  std::vector<uint32_t> words((size_t)((total + (uint32_t)pad + 31) >> 5), 0);
  std::vector<char> state(words.size(), 0);
  HostSink sink(words, state);
  for (int u = nb - 1; u >= 0; --u) {
    const int c = g.mcu_comp[u % g.blocks_per_mcu] ? 1 : 0;
    BitWriter<HostSink> bw(sink, off[(size_t)u]);
    enc_block_emit(&coefs[(size_t)u * 64], enc_dc_diff(g, coefs.data(), u), t.dc[c], t.ac[c], bw);
    if (u == nb - 1) bw.put((1u << pad) - 1u, pad);
    const uint32_t end = bw.word * 32 + (uint32_t)bw.fill;
    if (end != off[(size_t)u] + bits[(size_t)u] + (u == nb - 1 ? (uint32_t)pad : 0u)) {
      std::printf("%s: block %d wrote up to bit %u, its length says %u\n", name, u, end, off[(size_t)u] + bits[(size_t)u]);
      return 1;
    }
    bw.finish();
  }
  if (!sink.ok) {
    std::printf("%s: a plain store met a shared word, or two blocks wrote the same bit\n", name);
    return 1;
  }
  // stuffing: counts per chunk, exclusive sums, scatter (chunks in reverse order); one chunk more than needed, as the device's grid has
  const uint32_t nchunks = (nbytes + kEncChunk - 1) / kEncChunk + 1;
  std::vector<uint32_t> cnt(nchunks), before(nchunks);
  uint32_t ff = 0;
  for (uint32_t k = 0; k < nchunks; ++k) {
    cnt[k] = enc_chunk_ff(words.data(), k, nbytes);
    before[k] = ff;
    ff += cnt[k];
  }
  std::vector<unsigned char> out((size_t)nbytes + ff + 2);
  uint32_t len = 0;
  for (uint32_t k = nchunks; k-- > 0;) {
    const uint32_t n = enc_chunk_scatter(words.data(), k, nbytes, before[k], out.data());
    if (n) {
      if (len) {
        std::printf("%s: two chunks end the stream\n", name);
        return 1;
      }
      len = n;
    }
  }
  if (len != out.size() || out != seq) {
    std::printf("%s: %u bytes from the per-block stage, %zu from the sequential stage, or different bytes\n", name, len, seq.size());
    return 1;
  }
  // and the whole file against libjpeg's
  std::vector<unsigned char> file((size_t)kEncHeaderBytes);
  if (enc_write_header(width, height, sampling, qt, file.data()) != kEncHeaderBytes) return 1;
  file.insert(file.end(), out.begin(), out.end());
  if (file != want_file) {
    std::printf("%s: the file differs from libjpeg's (%zu bytes, %zu wanted)\n", name, file.size(), want_file.size());
    return 1;
  }
  std::printf("%s %d %u %u ok\n", name, nb, total, len);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 1) % 7) {
    std::printf("usage: %s NAME WIDTH HEIGHT QUALITY SUBSAMPLING RGBFILE JPEGFILE ...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a + 6 < argc; a += 7) {
    const int w = std::atoi(argv[a + 1]), h = std::atoi(argv[a + 2]);
    const std::vector<unsigned char> rgb = read_file(argv[a + 5]), file = read_file(argv[a + 6]);
    if (rgb.size() != (size_t)w * h * 3 || file.empty()) {
      std::printf("cannot read %s / %s\n", argv[a + 5], argv[a + 6]);
      return 2;
    }
    if (run(argv[a], w, h, std::atoi(argv[a + 3]), std::atoi(argv[a + 4]), rgb, file)) return 1;
  }
  return 0;
}
