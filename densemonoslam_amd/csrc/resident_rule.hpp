// The residency rules of the resident tracker kernels (track.hip k_gn_level, k_so3_level), in one place.  Plain host code:
// nothing from HIP, nothing else from the project; a stream is an opaque `const void*`.  Every function here returns a number
// or a decision and makes no call; the callers (track.hip, session.hip, fusion_frame.hip) ask the device and act.
// tests/test_resident_rule_cpu.py drives this header alone.
//
// The invariant all of it upholds: blocks of a resident kernel spin on each other, so EVERY block of a resident launch is on
// the device at once, and two resident grids never share the device half-resident.  A grid that starts incomplete runs into the
// spin limit: the frame keeps its prior pose, and the handle falls back to launch-per-phase for good.
//   * one handle: a level's grid never exceeds the handle's bound (persistent_shape, handle_bound, so3_blocks, call_level_shape);
//   * what overlaps the tracker on another stream of the same frame (the depth pre-filter) takes no more units than the widest
//     level leaves free (prep_blocks);
//   * several handles: their sections run one after the other (ChainState), unless the owner caps each of them so that all fit
//     together (session_cap, chain_exempt).
#pragma once

namespace dms {

constexpr int kPB = 512;                 // 8 waves: 256 VGPRs per thread, half the reduction tail of 16 waves
constexpr int kMaxPersistBlocks = 256;   // one block per CU
constexpr int kMinPixelsPerThread = 1, kMaxPixelsPerThread = 5;  // the instantiations of k_gn_level
constexpr int kPairPixelLimit = 1 << 19;  // a resident level has fewer pixels than this: the 19-bit count of the pair word
constexpr int kArRing = 10;              // word sets a stage cycles through, one per iteration (re-armed in flight when a level runs more iterations)
constexpr int kPersistReserve = 56;      // compute units left to whatever overlaps the tracker (see persistent_shape)
constexpr int kPersistTarget = 160;      // largest grid that still gets 1 or 2 pixels per thread (DMS_PERSIST_BLOCKS)
constexpr int kQuietAfter = 8;           // see ChainState
constexpr int kSessionSpareUnits = 16;   // units a session keeps out of its cameras' caps (see session_cap)

struct LevelShape {
  int P;       // pixels per thread
  int blocks;  // 0 = not eligible: launch-per-phase
};

// pixels per thread (1 - 5) and grid of k_gn_level for an n-pixel level; 0 blocks = not eligible
inline LevelShape persistent_shape(int n, int target, int max_blocks, int reserve = kPersistReserve) {
  // 1 or 2 pixels per thread if that keeps the grid at <= `target` blocks (cheap barriers win on the small levels; 96 while
  // the cross-block sums went through per-block records and a gather, 160 since the integer all-reduce: level 1 of
  // 640x480 on 150 blocks with one pixel per thread instead of 75 with two, +1 % frame rate);
  // otherwise 3 pixels per thread on up to 256 blocks (the full-resolution
  // level is bound by its per-CU arithmetic: measured 221 us at 200 blocks vs 230 us at 150), else 4
  auto blocks = [&](int p) { return (n + kPB * p - 1) / (kPB * p); };
  const int cap = max_blocks < kMaxPersistBlocks ? max_blocks : kMaxPersistBlocks;  // every block must be resident at once
  const int small = target < cap ? target : cap;
  // ... and among 3 / 4 / 5 the fewest that leaves `reserve` compute units to whatever overlaps the tracker (the frame step's
  // prep stream holds whole units for the length of its depth filter: 1241x376 on 228 blocks beside 97 filter blocks started
  // incomplete; 5 pixels per thread = 183 blocks leave 73), else the fewest that fits at all
  int P = 0;
  if (blocks(1) <= small)
    P = 1;
  else if (blocks(2) <= small)
    P = 2;
  else {
    for (int p = 3; p <= kMaxPixelsPerThread && !P; ++p)
      if (blocks(p) <= cap - reserve) P = p;
    for (int p = 3; p <= kMaxPixelsPerThread && !P; ++p)
      if (blocks(p) <= cap) P = p;
    if (!P) P = kMaxPixelsPerThread;
  }
  int nb = blocks(P);
  if (nb > cap || n >= kPairPixelLimit) nb = 0;  // does not fit the device (or the 19-bit count of the pair word): launch-per-phase
  return {P, nb};
}

// How many blocks of a resident kernel fit the device at once.  One block (512 threads x up to 256 registers) fills a compute unit,
// so a grid may have at most as many blocks as the device has compute units (`cus`: 256 on a whole MI355X, fewer on a partition /
// under a CU mask; 0: unknown), checked against the occupancy API's answer for the largest kernel (`per_cu`; the API is known to
// answer one block per CU too many near register-file edges, MI355X_MICROARCH.md: a 512-thread block at > 128 registers can only
// ever be alone on its CU, so one per CU is what is relied on).  0: resident launches are off for the handle.
inline int device_bound(int cus, int per_cu) { return per_cu >= 1 && cus > 0 ? (cus < kMaxPersistBlocks ? cus : kMaxPersistBlocks) : 0; }
// DMS_PERSIST_MAX_BLOCKS (`env_blocks`, <= 0: not set) lowers the device's bound further, never raises it
inline int lowered_bound(int bound, int env_blocks) { return env_blocks > 0 && env_blocks < bound ? env_blocks : bound; }
// The handle's bound: the device's, or the owner's cap below it (dms_odometry_set_resident_budget; 0: none)
inline int handle_bound(int budget_cap, int max_resident_blocks) {
  return (budget_cap > 0 && budget_cap < max_resident_blocks) ? budget_cap : max_resident_blocks;
}

// grid of the resident SO3 kernel (one pixel per thread over the coarsest image of `n` pixels); 0 = the SO3 stage runs launch-per-phase
inline int so3_blocks(bool resident, int n, int bound) {
  const int nbp = (n + kPB - 1) / kPB;
  return (resident && nbp <= kMaxPersistBlocks && nbp <= bound) ? nbp : 0;
}

// Shape of an n-pixel level of ONE tracker call that runs `iterations` on it, on a handle with this bound.
// Two callers.  The tracker call passes the handle's bound (handle_bound) and the level's iteration count.  odometry_free_cus, asked
// once at context creation for what the widest level leaves free, passes the DEVICE's bound (max_resident_blocks, no owner's cap: none
// is set that early, and a later cap only narrows the grids) and iterations = 0, i.e. no iteration condition (a level that runs
// launch-per-phase for its length holds nothing, so this errs towards fewer free units).  Its value, and with it prep_blocks, is
// what it was before the two callers shared this function.
inline LevelShape call_level_shape(int bound, int target, int iterations, bool resident, bool long_levels_resident, int n) {
  if (resident && (iterations <= kArRing || long_levels_resident))  // (more iterations than ring sets: the ring is re-armed in flight)
    return persistent_shape(n, target, bound);
  return {1, 0};
}

// Integer all-reduce: pause (units of 64 cycles) before the first read of the totals on a grid of nb blocks.  `forced`:
// DMS_AR_FIRST_DELAY, `forced_stage`: DMS_AR_FIRST_DELAY_BY_LEVEL's entry for this stage (-1 = the rule).
// The later the last arrival can be after one's own, the longer the pause pays: ~0.4 us on the 150 / 200-block levels, next to
// nothing on 38 blocks (measured: level 2 is best at 0 - 8 units, levels 1 and 0 at 12 - 20)
inline int first_delay_for(int nb, int forced_stage, int forced) {
  if (forced_stage >= 0) return forced_stage;
  return forced >= 0 ? forced : (nb >= 96 ? 24 : 8);
}

// The cap a session gives every hosted camera's tracker when `concurrent` streams track at the same time on a device of `cus`
// units: (units - 16) / concurrent blocks each, so that all their grids fit the device together and none has to wait for another's
// (chain_exempt).  0 = no cap, full grids, chained: one stream, a device of fewer than 64 units, or a frame whose level 0 would not
// fit the capped grid at the most pixels per thread (a capped handle would fall back to a launch per phase).
inline int session_cap(int cus, int concurrent, int W, int H, bool share_device) {
  if (!share_device || concurrent < 2 || cus < 64) return 0;
  const int cap = (cus - kSessionSpareUnits) / concurrent;
  return (long long)W * H > (long long)cap * kPB * kMaxPixelsPerThread ? 0 : cap;
}

// Fat blocks of the depth pre-filter beside the tracker: at most 40, and never more than the resident tracker kernels leave
// free (`free_cus`; -1: the tracker holds nothing) — a fat block holds a whole compute unit for the length of the filter, and a
// resident grid that finds fewer free units than it has blocks starts incomplete, its blocks spinning until the filter's retire.
// Measured at 640x480 (round 4, the table form of the filter: 112 us on 56 units), driver's form: 16 / 24 / 32 / 40 / 43 / 48 /
// 50 / 56 / 60 blocks -> 2300 / 2326 / 2375 / 2386 / 2387 / 2388 / 2334 / 2305 / 2290 frames/s; the leg with three predictions per
// frame: 2412 at 34 - 40 blocks, 2292 at 43, 2370 at 56.  Below the cap the count is the smallest that keeps the number of rounds
// over the image's 64 x 16 tiles (300 tiles, 8 rounds: 38 blocks).
inline int prep_blocks(int tiles, int free_cus) {
  int cap = 40;
  if (free_cus >= 16 && free_cus < cap) cap = free_cus;
  const int rounds = (tiles + cap - 1) / cap;
  return (tiles + rounds - 1) / rounds;
}

// DMS_PERSIST_UNCHAINED=1 (`unchained_env`) or dms_odometry_set_resident_budget(.., unchained) (`unchained_handle`): the caller
// guarantees that the resident grids of all handles that may track at the same time fit the device TOGETHER - then every grid
// completes whatever the interleaving and no section has to wait for another camera's.  Honoured only for handles that hold at most
// half the device (`budget`: the handle's bound): two of them always fit together.  An exempt section never touches the chain.
inline bool chain_exempt(bool unchained_env, bool unchained_handle, int budget, int cus) {
  return (unchained_env || unchained_handle) && budget > 0 && 2 * budget <= cus;
}

// The cross-stream chain of one device.  Every resident section (the resident launches of one tracker call) of the process that is
// not exempt is chained on one event per device: stream-ordered, free for a single stream, and it serialises trackers of different
// cameras / streams against each other.
// A process that runs all its trackers on one stream (one camera per process, the usual case) needs no event at all: the stream
// orders the sections, and an unconditional record after every tracker call cost ~6 us of idle stream per frame.  The first time a
// section arrives on a stream other than the previous one, the device is synchronised once (the previous stream may have been
// destroyed since: its handle must not be touched any more) and the device switches to the chained form: from then on every section
// ends with an event on its own - live - stream, and a section on another stream waits for it ...
// ... until one stream has had the device's sections to itself for kQuietAfter sections in a row (a front end that changed streams
// between phases; a benchmark's loops): the events stop, and the next section from another stream pays one device synchronisation as
// the very first change of stream did.  Two cameras that alternate never get there and keep their events.
//
// The executor (track.hip PersistSection) holds a mutex from enter() to leave() / recorded().  Per section:
//   enter(stream)       -> proceed | device_sync | wait_event (on the chain's event), before the first resident launch;
//   owes_event()        -> whether the section's LAST resident launch should carry the chain's event as its completion signal instead
//                          of a marker recorded behind it (between two kernels of one stream a marker is a gap of about 7 us);
//   leave(carried)      -> `carried`: that launch was given the event.  Returns whether a marker has to be recorded on the stream
//                          now; if so, recorded(ok) takes back whether the record succeeded.
// Known weak points, kept as they are (a change of behaviour is a change to this file with a test beside it):
//   * with `carried`, the event counts as valid from the promise on, whether or not the launch that carries it then succeeds: a
//     failed launch leaves an event that was never enqueued, and the next other stream waits on whatever it last stood for;
//   * chained, not quiet and without a valid event (a record that failed), a section from another stream gets wait_event's place
//     in the state machine but nothing to wait for: enter() answers `proceed`, and nothing orders it behind the previous section.
struct ChainState {
  enum Enter { proceed, device_sync, wait_event };
  const void* last = nullptr;  // stream of the previous section
  bool used = false;           // ... if there was one
  bool chained = false;        // several streams have run sections on this device: events from here on
  bool ev_valid = false;       // the chain's event stands for the previous section's end
  int run = 0;                 // consecutive sections that found the previous one on their own stream, while chained
  bool quiet = false;          // chained, but the events have stopped
  bool ext_events = true;      // DMS_PERSIST_EXT_EVENT: the last launch may carry the event (0: always a marker)

  Enter enter(const void* stream) {
    Enter what = proceed;
    if (used && last != stream) {
      if (!chained || quiet) {
        what = device_sync;
        chained = true;
      } else if (ev_valid) {
        what = wait_event;
      }
      run = 0;
      quiet = false;
    } else if (chained && !quiet && ++run >= kQuietAfter) {
      quiet = true;
      ev_valid = false;
    }
    last = stream;
    used = true;
    return what;
  }
  bool owes_event() const { return chained && !quiet && ext_events; }
  bool leave(bool carried) {
    if (carried) {
      ev_valid = true;
      return false;
    }
    return chained && !quiet;
  }
  void recorded(bool ok) { ev_valid = ok; }
};

}  // namespace dms
