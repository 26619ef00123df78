"""The frame step's late-frame rule (densemonoslam_amd/csrc/late_frame.hpp) on its own: a stand-alone program that includes only
that header and plays a scripted sequence of frames, built with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include "densemonoslam_amd/csrc/late_frame.hpp"
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static const double kFast = 0.010, kSlow = 1.0;  // ms waited: under / over the 0.015 ms bar
int main() {
  using dms::LateFrame;
  {  // forced on / off wins over everything, and touches no counter
    LateFrame l;
    l.forced = 1;
    l.update(false, kFast);
    CHECK(l.on && l.low == 0 && l.cool == 0 && l.backoff == 64);
    l.cool = 5;
    l.update(true, kFast);
    CHECK(l.on && l.cool == 5);
    l.forced = 0;
    l.update(true, kSlow);
    CHECK(!l.on && l.low == 0 && l.cool == 5 && l.backoff == 64);
  }
  LateFrame l;
  CHECK(!l.on && l.forced == -1 && l.low == 0 && l.cool == 0 && l.backoff == 64);
  l.update(true, kFast);  // off so far: "any other frame" turns it on
  CHECK(l.on && l.low == 0);
  l.update(true, kFast);
  l.update(true, kFast);
  CHECK(l.on && l.low == 2);
  l.update(false, kFast);  // not `may`: off, and the low counter starts again
  CHECK(!l.on && l.low == 0 && l.cool == 0);
  l.update(true, kSlow);
  CHECK(l.on && l.low == 0);
  // a frame at or over the bar between fast ones zeroes the count
  l.update(true, kFast);
  l.update(true, kFast);
  CHECK(l.on && l.low == 2);
  l.update(true, 0.015);
  CHECK(l.on && l.low == 0);
  l.update(true, kFast);
  l.update(true, kFast);
  CHECK(l.on && l.low == 2 && l.cool == 0 && l.backoff == 64);
  // the third consecutive fast frame switches it off: cooling period = the back-off so far, which doubles up to 4096
  int expect = 64;
  for (int round = 0; round < 9; ++round) {
    l.update(true, kFast);
    CHECK(!l.on && l.low == 0 && l.cool == expect);
    CHECK(l.backoff == (expect < 4096 ? 2 * expect : 4096));
    if (round == 0) {  // not `may` while cooling: off, and the period does not run
      l.update(false, kSlow);
      CHECK(!l.on && l.cool == expect);
    }
    for (int k = expect; k > 0; --k) {  // the period counts down with the rule off, whatever the host waited
      CHECK(l.cool == k);
      l.update(true, k % 2 ? kFast : kSlow);
      CHECK(!l.on && l.low == 0);
    }
    CHECK(l.cool == 0);
    l.update(true, kFast);  // off: on again
    CHECK(l.on && l.low == 0);
    l.update(true, kFast);
    l.update(true, kFast);
    CHECK(l.on && l.low == 2);
    if (expect < 4096) expect *= 2;
  }
  CHECK(expect == 4096 && l.backoff == 4096);
  std::printf("ok\n");
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_late_frame_rule_transitions():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "late_frame.cpp")
        exe = os.path.join(td, "late_frame")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + ROOT, src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
