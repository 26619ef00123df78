"""Pixel ownership of the resident Gauss-Newton level kernel (densemonoslam_amd/csrc/track_ownership.hpp) on its own: a stand-alone
program that includes only that header and resident_rule.hpp.  For every image size below, every pyramid level, and every shape
(pixels per thread, blocks) that the residency rule can choose for it - whatever the handle's bound, budget-capped grids included -
both mappings (contiguous, interleaved) are bijections from (block, slot, thread) onto [0, blocks * P * 512), every pixel of the level
is owned exactly once, a wave owns 64 consecutive pixels starting at a multiple of 64, and a lane past the end of the image shadows
pixel index % N.  Built with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <set>
#include <utility>
#include <vector>
#include "densemonoslam_amd/csrc/resident_rule.hpp"
#include "densemonoslam_amd/csrc/track_ownership.hpp"
using namespace dms;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s (n %d P %d nb %d interleave %d)\n", __LINE__, #c, n, P, nb, il); return 1; } } while (0)

static int check_shape(int n, int P, int nb, int il) {
  const long long span = (long long)nb * P * kPB;
  CHECK(span >= n && span < (1ll << 31));
  std::vector<unsigned char> idx_seen((size_t)span, 0), px_seen((size_t)n, 0);
  for (int b = 0; b < nb; ++b)
    for (int p = 0; p < P; ++p)
      for (int w = 0; w < kPB / 64; ++w) {
        const int base = owned_index(il != 0, b, nb, P, p, w * 64);
        CHECK(base >= 0 && base % 64 == 0 && base + 63 < span);
        if (il) CHECK(base / 64 == (p * (kPB / 64) + w) * nb + b);  // the segment the issue names
        else CHECK(base == (b * P + p) * kPB + w * 64);              // ... and the adjacent chunks of before
        for (int lane = 0; lane < 64; ++lane) {
          const int idx = owned_index(il != 0, b, nb, P, p, w * 64 + lane);
          CHECK(idx == base + lane);  // a wave's lanes: consecutive pixels
          CHECK(!idx_seen[idx]);
          idx_seen[idx] = 1;
          const int s = owned_shadow(idx, n);
          CHECK(s >= 0 && s < n);
          if (idx < n) {
            CHECK(s == idx && !px_seen[idx]);
            px_seen[idx] = 1;
          } else {
            CHECK(s == idx % n);  // masked: shadows a pixel of the image
          }
        }
      }
  for (long long i = 0; i < span; ++i) CHECK(idx_seen[(size_t)i]);
  for (int i = 0; i < n; ++i) CHECK(px_seen[i]);
  return 0;
}

int main() {
  static const int kSizes[][2] = {{640, 480}, {320, 240}, {160, 120}, {1241, 376}, {333, 251}, {7, 5}};
  int shapes = 0;
  for (const auto& wh : kSizes)
    for (int l = 0; l < 3; ++l) {
      const int n = (wh[0] >> l) * (wh[1] >> l);
      if (n <= 0) continue;
      std::set<std::pair<int, int>> seen;
      for (int bound = 1; bound <= kMaxPersistBlocks; ++bound)
        for (int target : {kPersistTarget, 96, 256}) {
          const LevelShape s = persistent_shape(n, target, bound);
          if (s.blocks <= 0 || !seen.insert({s.P, s.blocks}).second) continue;
          if (s.P < kMinPixelsPerThread || s.P > kMaxPixelsPerThread || s.blocks > bound) {
            std::printf("rule: n %d bound %d -> P %d blocks %d\n", n, bound, s.P, s.blocks);
            return 1;
          }
          for (int il = 0; il < 2; ++il)
            if (check_shape(n, s.P, s.blocks, il)) return 1;
          ++shapes;
        }
    }
  // shapes the rule does not choose today but the kernel is instantiated for: every P on a one-block and a ragged grid
  for (int P = kMinPixelsPerThread; P <= kMaxPixelsPerThread; ++P)
    for (int nb : {1, 2, 3, 7, 256})
      for (int il = 0; il < 2; ++il) {
        if (check_shape(nb * P * kPB, P, nb, il)) return 1;           // exactly full
        if (check_shape(nb * P * kPB - 1, P, nb, il)) return 1;       // one lane masked
        if (nb * P * kPB > 700 && check_shape(nb * P * kPB - 700, P, nb, il)) return 1;  // more than a block's worth of one slot masked
        if (check_shape(35, P, nb, il)) return 1;                     // nearly everything masked: shadows wrap many times
      }
  std::printf("ok %d\n", shapes);
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_ownership_is_a_bijection():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "track_ownership.cpp")
        exe = os.path.join(td, "track_ownership")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + ROOT, src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.startswith("ok "), (out.returncode, out.stdout, out.stderr)
        assert int(out.stdout.split()[1]) >= 20  # the sizes above give at least this many distinct shapes
