"""The residency rules of the resident tracker kernels (densemonoslam_amd/csrc/resident_rule.hpp) on their own: a stand-alone program
that includes only that header - level shapes, bounds, the session's cap, the invariant they uphold together over an exhaustive
sweep, and the cross-stream chain's transitions step by step - built with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include "densemonoslam_amd/csrc/resident_rule.hpp"
using namespace dms;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int level_n(int W, int H, int l) { return (W >> l) * (H >> l); }
// level l of a 10-iteration call on a handle with this bound: target 160, reserve 56
static LevelShape shape(int W, int H, int l, int bound) { return call_level_shape(bound, kPersistTarget, 10, true, true, level_n(W, H, l)); }
static bool is(LevelShape s, int P, int blocks) { return s.P == P && s.blocks == blocks; }

struct ShapeCase {
  int W, H, bound;
  int want[3][2];  // levels 0 / 1 / 2: P, blocks
};
static const ShapeCase kShapes[] = {
    {640, 480, 256, {{3, 200}, {1, 150}, {1, 38}}},  {640, 480, 120, {{5, 120}, {2, 75}, {1, 38}}},  {640, 480, 20, {{5, 0}, {5, 0}, {2, 19}}},
    {1241, 376, 256, {{5, 183}, {2, 114}, {1, 57}}}, {1241, 376, 120, {{5, 0}, {2, 114}, {1, 57}}},  {16, 16, 256, {{1, 1}, {1, 1}, {1, 1}}},
    {77, 47, 256, {{1, 8}, {1, 2}, {1, 1}}},         {164, 127, 256, {{1, 41}, {1, 11}, {1, 3}}},    {164, 127, 20, {{3, 14}, {1, 11}, {1, 3}}},
    {333, 251, 256, {{2, 82}, {1, 41}, {1, 11}}},    {601, 451, 256, {{3, 177}, {1, 132}, {1, 33}}}, {601, 451, 120, {{5, 106}, {2, 66}, {1, 33}}},
    {648, 486, 256, {{4, 154}, {1, 154}, {1, 39}}},  {701, 601, 256, {{5, 165}, {2, 103}, {1, 52}}},
};
static const int kSizes[][2] = {{640, 480}, {1241, 376}, {16, 16}, {77, 47}, {164, 127}, {333, 251}, {601, 451}, {648, 486}, {701, 601}, {320, 240}};

static bool state_is(const ChainState& c, const void* last, bool chained, bool ev_valid, int run, bool quiet) {
  return c.used && c.last == last && c.chained == chained && c.ev_valid == ev_valid && c.run == run && c.quiet == quiet;
}

int main() {
  // ---- the constants the kernels and the callers share
  CHECK(kPB == 512 && kMaxPersistBlocks == 256 && kMinPixelsPerThread == 1 && kMaxPixelsPerThread == 5 && kPairPixelLimit == 1 << 19);
  CHECK(kArRing == 10 && kPersistReserve == 56 && kPersistTarget == 160 && kQuietAfter == 8);

  // ---- shapes
  for (const ShapeCase& c : kShapes)
    for (int l = 0; l < 3; ++l) {
      const LevelShape s = shape(c.W, c.H, l, c.bound);
      if (!is(s, c.want[l][0], c.want[l][1])) {
        std::printf("%dx%d bound %d level %d: (%d,%d), expected (%d,%d)\n", c.W, c.H, c.bound, l, s.P, s.blocks, c.want[l][0], c.want[l][1]);
        return 1;
      }
      CHECK(is(persistent_shape(level_n(c.W, c.H, l), 160, c.bound, 56), s.P, s.blocks));  // the call's shape IS the level shape
    }
  CHECK(is(shape(1023, 512, 0, 256), 4, 256));
  CHECK(1024 * 512 == kPairPixelLimit && shape(1024, 512, 0, 256).blocks == 0);  // the pair word's limit, exactly
  for (int it = 11; it <= 50; it += 39) {  // more iterations than the ring has sets
    CHECK(call_level_shape(256, 160, it, true, false, 640 * 480).blocks == 0);
    CHECK(is(call_level_shape(256, 160, it, true, true, 640 * 480), 3, 200));
  }
  CHECK(is(call_level_shape(256, 160, 10, true, false, 640 * 480), 3, 200));
  CHECK(is(call_level_shape(256, 160, 0, true, false, 640 * 480), 3, 200));  // (odometry_free_cus's form)
  CHECK(call_level_shape(256, 160, 10, false, true, 640 * 480).blocks == 0);  // launch-per-phase handle
  CHECK(so3_blocks(true, level_n(640, 480, 2), 256) == 38 && so3_blocks(true, level_n(640, 480, 2), 20) == 0);
  CHECK(so3_blocks(false, level_n(640, 480, 2), 256) == 0 && so3_blocks(true, 38 * 512, 38) == 38 && so3_blocks(true, 38 * 512 + 1, 38) == 0);
  CHECK(so3_blocks(true, 256 * 512, 1000) == 256 && so3_blocks(true, 256 * 512 + 1, 1000) == 0);

  // ---- bounds
  CHECK(device_bound(256, 1) == 256 && device_bound(304, 2) == 256 && device_bound(120, 1) == 120 && device_bound(256, 0) == 0 && device_bound(0, 1) == 0);
  CHECK(lowered_bound(256, 120) == 120 && lowered_bound(256, 0) == 256 && lowered_bound(120, 200) == 120 && lowered_bound(0, 20) == 0);
  CHECK(handle_bound(120, 256) == 120 && handle_bound(0, 256) == 256 && handle_bound(300, 256) == 256 && handle_bound(20, 0) == 0);
  CHECK(first_delay_for(96, -1, -1) == 24 && first_delay_for(95, -1, -1) == 8 && first_delay_for(200, -1, 5) == 5 && first_delay_for(200, 0, 5) == 0);
  CHECK(prep_blocks(300, -1) == 38 && prep_blocks(300, 56) == 38 && prep_blocks(300, 15) == 38 && prep_blocks(300, 16) == 16 && prep_blocks(7, 100) == 7);

  // ---- the session's cap
  CHECK(session_cap(256, 2, 640, 480, true) == 120 && 640 * 480 == 120 * kPB * kMaxPixelsPerThread);  // the boundary case
  CHECK(session_cap(256, 2, 641, 480, true) == 0);
  CHECK(session_cap(256, 3, 640, 480, true) == 0);
  CHECK(session_cap(256, 2, 1241, 376, true) == 0);
  CHECK(session_cap(63, 2, 16, 16, true) == 0 && session_cap(64, 2, 16, 16, true) == 24);
  CHECK(session_cap(256, 1, 640, 480, true) == 0);
  CHECK(session_cap(256, 2, 640, 480, false) == 0);

  // ---- the invariant: whatever cap a session hands out, `concurrent` capped handles fit the device together, each is exempt from
  // the chain, no stage of a capped handle exceeds the cap, and level 0 stays resident.  Exhaustive.
  int positive = 0;
  for (int cus = 64; cus <= 304; ++cus)
    for (int concurrent = 2; concurrent <= 8; ++concurrent)
      for (const auto& wh : kSizes) {
        const int W = wh[0], H = wh[1];
        const int cap = session_cap(cus, concurrent, W, H, true);
        CHECK(cap >= 0);
        if (cap == 0) continue;
        ++positive;
        const int bound = handle_bound(cap, device_bound(cus, 1));
        CHECK(bound == cap);
        CHECK(concurrent * cap <= cus - 16);
        CHECK(2 * cap <= cus && chain_exempt(false, true, bound, cus));
        for (int l = 0; l < 3; ++l) {
          const LevelShape s = shape(W, H, l, bound);
          CHECK(s.blocks >= 0 && s.blocks <= cap && s.P >= kMinPixelsPerThread && s.P <= kMaxPixelsPerThread);
          CHECK(s.blocks == 0 || (long long)s.blocks * s.P * kPB >= level_n(W, H, l));  // the grid covers the level
        }
        CHECK(shape(W, H, 0, bound).blocks > 0);
        CHECK(so3_blocks(true, level_n(W, H, 2), bound) <= cap);
      }
  CHECK(positive == 7024);  // of the 241 x 7 x 10 cases (counted apart from this header, from the rule as session.hip used to state it)

  // ---- the exemption
  CHECK(chain_exempt(true, false, 120, 256) && chain_exempt(false, true, 120, 256) && chain_exempt(true, true, 128, 256));
  CHECK(!chain_exempt(false, false, 120, 256) && !chain_exempt(true, true, 129, 256) && !chain_exempt(true, true, 0, 256) && !chain_exempt(true, true, 120, 0));

  // ---- the chain
  int a_, b_, c_;
  const void *A = &a_, *B = &b_, *C = &c_;
  {  // one stream only, for ever: never an event
    ChainState c;
    CHECK(!c.used && !c.chained && !c.ev_valid && !c.quiet && c.run == 0 && c.ext_events);
    for (int k = 0; k < 100; ++k) {
      CHECK(c.enter(A) == ChainState::proceed);
      CHECK(!c.owes_event());
      CHECK(!c.leave(false));
      CHECK(state_is(c, A, false, false, 0, false));
    }
  }
  for (int ext = 0; ext < 2; ++ext) {  // A then B, alternating: one device synchronisation, then events - carried by the last launch or recorded
    ChainState c;
    c.ext_events = ext != 0;
    CHECK(c.enter(A) == ChainState::proceed && !c.owes_event() && !c.leave(false));
    CHECK(c.enter(B) == ChainState::device_sync);
    CHECK(state_is(c, B, true, false, 0, false));
    const void* s = B;
    for (int k = 0; k < 40; ++k) {
      CHECK(c.owes_event() == (ext != 0));
      if (ext) {  // the closing path: the last launch carries the event, nothing is recorded
        CHECK(!c.leave(true));
      } else {
        CHECK(c.leave(false));
        CHECK(!c.ev_valid || k > 0);
        c.recorded(true);
      }
      CHECK(state_is(c, s, true, true, 0, false));
      s = (s == A) ? B : A;
      CHECK(c.enter(s) == ChainState::wait_event);
      CHECK(state_is(c, s, true, true, 0, false));
    }
    // a section whose last launch could not carry the event (level 0 launch-per-phase) records a marker even with external events on
    CHECK(c.leave(false));
    c.recorded(true);
    CHECK(c.enter(C) == ChainState::wait_event);  // a third stream waits like the second
    CHECK(c.leave(false));
    c.recorded(true);
  }
  {  // the quiet rule
    ChainState c;
    c.ext_events = false;
    CHECK(c.enter(A) == ChainState::proceed && !c.leave(false));
    CHECK(c.enter(B) == ChainState::device_sync && c.leave(false));
    c.recorded(true);
    for (int k = 1; k < kQuietAfter; ++k) {  // seven further sections on B: still chained, still recording
      CHECK(c.enter(B) == ChainState::proceed);
      CHECK(state_is(c, B, true, true, k, false));
      CHECK(c.leave(false));
      c.recorded(true);
    }
    for (int k = 0; k < 20; ++k) {  // the eighth goes quiet and drops the event; that one and the following record nothing
      CHECK(c.enter(B) == ChainState::proceed);
      CHECK(state_is(c, B, true, false, kQuietAfter, true));
      CHECK(!c.owes_event());
      CHECK(!c.leave(false));
      c.ext_events = k % 2 == 0;  // (whichever way the switch stands)
    }
    c.ext_events = false;
    CHECK(c.enter(A) == ChainState::device_sync);  // a change of stream while quiet: as the very first one
    CHECK(state_is(c, A, true, false, 0, false));
    CHECK(c.leave(false));
    c.recorded(true);
    CHECK(c.enter(B) == ChainState::wait_event);  // ... and events again
    CHECK(state_is(c, B, true, true, 0, false));
    CHECK(c.leave(false));
    c.recorded(true);
    // a change of stream zeroes the run: seven on B, one on A, seven on A do not go quiet
    for (int k = 1; k < kQuietAfter; ++k) CHECK(c.enter(B) == ChainState::proceed && c.run == k && c.leave(false));
    CHECK(c.enter(A) == ChainState::wait_event && c.run == 0);
    for (int k = 1; k < kQuietAfter; ++k) CHECK(c.enter(A) == ChainState::proceed && c.run == k && !c.quiet);
    CHECK(c.enter(A) == ChainState::proceed && c.quiet && !c.ev_valid);
  }
  {  // the closing path
    ChainState c;
    CHECK(c.enter(A) == ChainState::proceed && !c.leave(false) && c.enter(B) == ChainState::device_sync);
    CHECK(c.ext_events && c.owes_event());
    CHECK(!c.leave(true));  // promised: valid from here on, whether or not the launch that carries it succeeds (pinned)
    CHECK(state_is(c, B, true, true, 0, false));
    CHECK(c.enter(A) == ChainState::wait_event);
    c.ext_events = false;
    CHECK(!c.owes_event());
    CHECK(c.leave(false));  // external events off: a marker
    c.recorded(true);
    CHECK(state_is(c, A, true, true, 0, false));
  }
  {  // a failed record leaves no valid event: the next other stream waits for nothing (pinned as it is)
    ChainState c;
    c.ext_events = false;
    CHECK(c.enter(A) == ChainState::proceed && !c.leave(false) && c.enter(B) == ChainState::device_sync);
    CHECK(c.leave(false));
    c.recorded(false);
    CHECK(state_is(c, B, true, false, 0, false));
    CHECK(c.enter(A) == ChainState::proceed);
    CHECK(state_is(c, A, true, false, 0, false));
    CHECK(c.leave(false));
    c.recorded(true);
    CHECK(c.enter(B) == ChainState::wait_event);
    CHECK(c.leave(false));
    c.recorded(true);
    CHECK(c.enter(A) == ChainState::wait_event && c.leave(false));
    c.recorded(false);  // ... and a later failure invalidates a valid one
    CHECK(!c.ev_valid && c.enter(B) == ChainState::proceed);
  }
  {  // an exempt section changes no state at all: the executor asks the predicate first and then makes none of the three calls, so
     // the sections around it decide as if it had not been - here in the middle of a run towards the quiet rule
    ChainState c;
    c.ext_events = false;
    CHECK(c.enter(A) == ChainState::proceed && !c.leave(false) && c.enter(B) == ChainState::device_sync && c.leave(false));
    c.recorded(true);
    for (int k = 1; k <= kQuietAfter; ++k) {
      CHECK(chain_exempt(false, true, 120, 256));  // (in between, a section of a capped handle on stream A: no call)
      CHECK(c.enter(B) == ChainState::proceed && c.run == k && c.quiet == (k == kQuietAfter));
      if (c.leave(false)) c.recorded(true);
    }
    CHECK(state_is(c, B, true, false, kQuietAfter, true));
  }
  std::printf("ok\n");
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_resident_rules():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "resident_rule.cpp")
        exe = os.path.join(td, "resident_rule")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I" + ROOT, src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
