// The parallel entropy decoder of densemonoslam_amd/csrc/jpeg_dev.hip restated with its lanes run one after another, on the
// host: the same per-lane functions (csrc/jpeg_core.hpp: sync_lane, settle_segment, write_lane), the same passes in the same
// order - relaxation rounds, the single-lane pass, block counts, write pass, DC sums - and after each stream a comparison with
// the sequential entropy stage (csrc/jpeg.hpp): coefficients and refusals must be the same.
//
//   jpeg_lanes_host NAME WIDTH HEIGHT FILE [NAME WIDTH HEIGHT FILE ...]
//
// prints, per stream and subsequence size, "NAME S lanes rounds settled verdict" and exits 1 on the first difference.
// Built by tests/test_ingest_device_cpu.py with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "densemonoslam_amd/csrc/jpeg.hpp"

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

static int run(const char* name, const std::vector<unsigned char>& exact, int width, int height, int S) {
  // the stream in a buffer of exactly its size: the sanitizer sees any read outside it
  const unsigned char* data = exact.data();
  const size_t len = exact.size();

  Decoder seq;
  int rc = parse(seq, data, len, width, height);
  if (rc) {
    std::printf("%s %d parse refused: %s\n", name, S, seq.err ? seq.err : "");
    return 1;
  }
  const Geometry g = seq.geo;
  const size_t scan_off = (size_t)(seq.p - data);
  std::vector<short> want((size_t)g.total_blocks * 64, 0);
  const bool seq_ok = seq.entropy(want.data());
  const std::string seq_err = seq_ok ? "" : (seq.err ? seq.err : "?");

  // parse again for the lanes (the sequential stage has moved its own cursor)
  Decoder d;
  parse(d, data, len, width, height);
  std::vector<Segment> segs;
  const char* restart_err = nullptr;
  find_segments(data, len, scan_off, g, segs, &restart_err);
  std::vector<SegInfo> si;
  std::vector<LaneInfo> lanes;
  build_lanes(g, segs, S, si, lanes);
  Huff dc[3], ac[3];
  for (int i = 0; i < 3; ++i) {
    dc[i] = d.dc[d.comp[i].td];
    ac[i] = d.ac[d.comp[i].ta];
  }
  ScanView sc;
  sc.mem = data;
  sc.win = nullptr;
  sc.win_lo = 0;
  sc.win_n = 0;
  sc.dc = dc;
  sc.ac = ac;
  sc.g = &g;
  sc.segs = si.data();
  sc.lanes = lanes.data();
  const int nl = (int)lanes.size();

  // relaxation: round r reads the records of round r - 1 and writes its own (two buffers in turn)
  std::vector<LaneRecord> rec[2];
  rec[0].resize((size_t)nl);
  rec[1].resize((size_t)nl);
  int rounds = 0, last = 0;
  bool changed = true;
  std::vector<char> dirty(si.size(), 0);
  for (int r = 0; r < kSyncRounds && changed; ++r) {
    changed = false;
    std::vector<LaneRecord>& cur = rec[r & 1];
    const std::vector<LaneRecord>& prev = rec[(r & 1) ^ 1];
    for (int l = 0; l < nl; ++l) {
      cur[(size_t)l] = sync_lane(sc, l, r, prev.data());
      const bool ch = r == 0 ? !(lanes[(size_t)l].flags & kLaneFirst) : !same_exit(cur[(size_t)l], prev[(size_t)l]);
      if (ch) {
        changed = true;
        if (r == kSyncRounds - 1) dirty[lanes[(size_t)l].seg] = 1;
      }
    }
    last = r;
    ++rounds;
  }
  std::vector<LaneRecord>& fin = rec[last & 1];
  int settled = 0;
  for (size_t s = 0; s < si.size(); ++s)
    if (dirty[s]) {
      const int n = (int)((s + 1 < si.size() ? si[s + 1].first_lane : (uint32_t)nl) - si[s].first_lane);
      settled += settle_segment(sc, (int)si[s].first_lane, n, fin.data());
    }

  // block counts -> write pass -> DC sums
  std::vector<short> got((size_t)g.total_blocks * 64, 0);
  uint32_t err_key = kNoBlockError;
  for (size_t s = 0; s < si.size(); ++s) {
    uint32_t block = 0;
    const int end = (int)(s + 1 < si.size() ? si[s + 1].first_lane : (uint32_t)nl);
    for (int l = (int)si[s].first_lane; l < end; ++l) {
      write_lane(sc, l, fin.data(), block, got.data(), &err_key);
      block += record_ends(fin[(size_t)l]);
    }
  }
  for (size_t s = 0; s < si.size(); ++s) {
    int pred[3] = {0, 0, 0};
    for (uint32_t b = 0; b < si[s].nblocks; ++b) {
      short* c = &got[((size_t)si[s].first_block + b) * 64];
      const int comp = g.mcu_comp[b % (uint32_t)g.blocks_per_mcu];
      pred[comp] += c[0];
      c[0] = (short)pred[comp];
    }
  }
  std::string verdict = err_key != kNoBlockError ? block_error_text((int)(err_key & 3)) : (restart_err ? restart_err : "");

  if (verdict != seq_err) {
    std::printf("%s %d: verdict '%s', the sequential stage says '%s'\n", name, S, verdict.c_str(), seq_err.c_str());
    return 1;
  }
  const size_t cmp = (size_t)seq.blocks_done * 64;  // every block the sequential stage completed
  for (size_t i = 0; i < cmp; ++i)
    if (got[i] != want[i]) {
      std::printf("%s %d: coefficient %zu of block %zu is %d, the sequential stage has %d\n", name, S, i % 64, i / 64, got[i], want[i]);
      return 1;
    }
  std::printf("%s %d %d %d %d %s\n", name, S, nl, rounds, settled, verdict.empty() ? "ok" : verdict.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) {
    std::printf("usage: %s NAME WIDTH HEIGHT FILE ...\n", argv[0]);
    return 2;
  }
  static const int sizes[4] = {32, 64, 128, 256};
  for (int a = 1; a + 3 < argc; a += 4) {
    const std::vector<unsigned char> stream = read_file(argv[a + 3]);
    if (stream.empty()) {
      std::printf("cannot read %s\n", argv[a + 3]);
      return 2;
    }
    for (int s = 0; s < 4; ++s)
      if (run(argv[a], stream, std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), sizes[s])) return 1;
  }
  return 0;
}
