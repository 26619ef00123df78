// Object layer: the tracker (reference RGBDOdometry, Utils/RGBDOdometry.{h,cpp}).
//
// MI355X design.  The reference runs ≈67 blocking device→host round trips per call (three
// kernel pairs + a 116-byte copy + a host Eigen solve per Gauss-Newton iteration,
// RGBDOdometry.cpp:425-586).  Here the whole coarse-to-fine loop is enqueued on one HIP
// stream with no host involvement.  Resident form (default): k_track_init, k_so3_level, one k_gn_level per pyramid
// level — ALL iterations of a level in one launch, grid-wide sums through memory-side integer atomics.  Launch-per-phase
// form (DMS_TRACK_MODE=launches; also every level with more than 10 iterations):
//
//   k_track_init     1 lane   prior pose -> state, first-iteration projection parameters
//   k_so3_pass       grid     per-pixel SO3 rows -> per-block integer records; the last block folds and solves
//   k_gn_pass1<I,R>  grid     RGB correspondence (count / Σdiff²) and ICP rows -> records
//   k_gn_pass2       grid     σ from the folded count, photometric rows -> records
//   k_gn_solve       1 block  fold both record sets, fp64 6×6 LDLT, SE3 update, next KRK⁻¹ / Kt
//   k_track_finalize 1 lane   0.3 m jump gate, result block
//
// Every cross-pixel sum is the order-free integer sum of canon.hpp and the scalar section is the fixed operation sequence
// of gn_scalar.hpp, in both forms: a pose does not depend on the execution mode, the grid size or the run, and equals the
// CPU oracle's bit for bit.
//
// The pose, the 4×4 accumulated transform (fp64) and the early-exit flags (SO3
// converged/diverged, rgbOnly break) live in a device state block; kernels past an exit
// return at once, which reproduces the host `break`s.  One D2H copy of the result block
// (pinned) ends the call.
#include <hip/hip_ext.h>
#include <math.h>

#include <map>
#include <type_traits>
#include <string>
#include <vector>

#include "internal.hpp"
#include "host_util.hpp"
#include "pixel_ops.hpp"
#include "smallmath.hpp"
#include "gn_scalar.hpp"
#include "canon.hpp"
#include "pyr_body.hpp"
#include "frame_state.hpp"
#include "track_init.hpp"
#include "model_bodies.hpp"
#include "surfel.hpp"
#include "resident_rule.hpp"
#include "track_ownership.hpp"
#include "scan.hpp"
#include <mutex>

namespace dms {

// The tracker object evaluates the Gauss-Newton rows with fused multiply-adds (pixel_ops.hpp madd<true>; what nvcc's default
// -fmad=true does to the reference's kernels) in every execution mode; the operator layer (reduce.hip: dms_icpStep ...)
// keeps every operation rounded.  The oracle restates both forms (orc_set_fused_rows).
constexpr bool kTrackerFma = true;

struct Buf {
  void* p = nullptr;
  size_t pitch = 0;
  int rows = 0, cols = 0;
  dms_image2d img() const {
    dms_image2d i;
    i.data = p;
    i.pitch = pitch;
    i.rows = rows;
    i.cols = cols;
    return i;
  }
};

}  // namespace dms

using namespace dms;

struct dms_odometry {
  bool early_exit = false;  // use the resident kernels that leave a level after an iteration without any correspondence
  // Execution switches, fixed per handle: read from the environment once, at dms_odometry_create (DMS_TRACK_MODE,
  // DMS_TRACK_EARLY_EXIT, DMS_PERSIST_BLOCKS), changed only through dms_odometry_set_mode.  (Reading them at
  // every call let a changing environment switch the execution mode in the middle of a session.)
  bool resident = true;       // false: three launches per iteration (DMS_TRACK_MODE=launches)
  int early_exit_force = -1;  // -1: as `early_exit`; 0 / 1: forced (DMS_TRACK_EARLY_EXIT)
  int persist_target = kPersistTarget;  // largest grid that still gets 1 or 2 pixels per thread (DMS_PERSIST_BLOCKS)
  // Resident kernels spin on each other: ALL blocks of a launch must be on the device at once (resident_rule.hpp holds every rule
  // that follows from it).  The device's bound, set at creation (device_bound, lowered_bound); a level that does not fit it runs
  // launch-per-phase.
  int max_resident_blocks = kMaxPersistBlocks;
  // dms_odometry_set_resident_budget: a cap below the device's own bound, and the owner's word that every handle that may track at the same
  // time carries a cap such that all their grids fit the device together - such a handle's launches need no chain (PersistSection)
  int budget_cap = 0;
  bool unchained_ok = false;
  bool fell_back = false;     // a resident kernel timed out at a grid-wide wait: this handle has switched to launch-per-phase
  // what call_level_shape() gave each level of the last tracker call (dms_odometry_get_level_shape); 0 blocks: launch-per-phase
  int last_shape_P[DMS_NUM_PYRS] = {1, 1, 1}, last_shape_nb[DMS_NUM_PYRS] = {0, 0, 0};
  // What the kernel that prepared the model side has left to the NEXT track call on this handle (frame step).  Two writers, each
  // overwriting the whole record: odometry_initModel_fused, and odometry_model_views_begin through fold_init_args.  One reader:
  // odometry_track_enqueue takes the record and leaves "nothing prepared" behind, whether the call then succeeds or not.
  struct NextCall {
    enum Kind {
      nothing,       // the call launches its own set-up (k_track_init)
      deferred_pyr,  // ... which also carries the model pyramid's last step, level 1 -> 2 of lastDepth / lastImage (k_track_init_pyr)
      folded,        // the set-up ran inside the model pyramid kernel: the call launches nothing before its resident SO3 level, which
                     // carries the deferred pyramid step
      folded_planes  // fused_model_prediction: the set-up ran inside the caller's kernel, which wrote the model maps and level 0 of the
                     // depth / intensity pyramid; the SO3 launch carries BOTH pyramid steps from those planes and empties the z-buffer
                     // cells that kernel had to leave alone
    } kind = nothing;
    int so3 = 0, first_level = 0;  // folded*: the call the set-up was made for ...
    const float* prior = nullptr;  // ... and its prior pose block
    unsigned* dense_cnt_zero = nullptr;  // deferred_pyr, folded: the frame step's 16 dense counters (fill.hpp), read by the model pyramid
                                         // kernel and zeroed by the call's first kernel
    unsigned long long* zbuf = nullptr;  // folded_planes: the z-buffer and its n_cells cells to empty
    const int* cells = nullptr;
    int n_cells = 0;
  } next_call;
  int inject_timeouts = 0;    // dms_odometry_inject_timeout: calls left that start with the timeout flag set
  int width, height;
  float cx, cy, fx, fy, distThres, angleThres;
  float sobelScale, maxDepthDeltaRGB, maxDepthRGB;
  float minGrad[DMS_NUM_PYRS];
  char* arena = nullptr;
  size_t arena_bytes = 0;
  Buf depth_tmp[3], vmaps_g_prev[3], nmaps_g_prev[3], vmaps_curr[3], nmaps_curr[3];
  Buf lastDepth[3], nextDepth[3], lastImage[3], nextImage[3], lastNextImage[3];
  Buf nextdIdx[3], nextdIdy[3], nextGate[3], pointClouds[3], corresImg[3];
  // Live-frame ring (frame pipeline only): the buffers written from the incoming frame alone —
  // depth pyramid, live vertex/normal maps, intensity pyramid and its derivatives — exist three
  // times, so that the next frame can be prepared on a second stream while this one is tracked
  // and the previous intensity pyramid still serves as lastNextImage.  Set 0 is the default set.
  struct LiveSet {
    Buf depth_tmp[3], vmaps_curr[3], nmaps_curr[3], nextImage[3], nextdIdx[3], nextdIdy[3], nextGate[3];
  };
  LiveSet ring[3];
  char* ring_arena = nullptr;
  bool ring_enabled = false;
  const void* deriv_of = nullptr;  // nextImage[0] the derivative pyramid was computed from
  float* vmaps_tmp = nullptr;
  float* nmaps_tmp = nullptr;
  long long* part_icp = nullptr;   // [kMaxPartialBlocks][32] integer records of the launch-per-phase kernels (grid units, canon.hpp)
  long long* part_rgb = nullptr;   // [kMaxPartialBlocks][32]
  long long* part_so3 = nullptr;   // [kMaxPartialBlocks][32]
  int* part_cnt = nullptr;     // [2][1024]
  unsigned* tickets = nullptr; // [4] arrival counters of the last-block-solves hand-off (zero between launches)
  unsigned long long* ar = nullptr;   // [kArSets][kArWords] all-reduce words of the resident kernels, zeroed by k_track_init
  unsigned* list_len = nullptr;       // [DMS_NUM_PYRS][kMaxPersistBlocks] entries of each block's photometric list in the last resident launch of a level
  bool track_interleave = true;       // DMS_TRACK_INTERLEAVE / debug key "track_interleave": a block's pixel segments spread over the image (track_ownership.hpp)
  bool rgb_compact = true;            // DMS_RGB_COMPACT / debug key "rgb_compact": the photometric half runs over the block's gated pixels only
  bool last_rgb[DMS_NUM_PYRS] = {false, false, false};  // the last call ran the photometric term on this level's resident kernel
  int first_delay = -1;               // integer all-reduce: pause before the first read of the totals (DMS_AR_FIRST_DELAY; -1 = by grid size)
  bool long_levels_resident = true;   // levels of more than kArRing iterations (inter-map calls: 50) as resident launches too (DMS_TRACK_LONG_RESIDENT=0: launch-per-phase, as before round 6)
  int first_delay_lvl[4] = {-1, -1, -1, -1};  // per stage (levels 0, 1, 2, SO3): DMS_AR_FIRST_DELAY_BY_LEVEL="l0,l1,l2,so3" (-1 = the rule)
  int first_delay_for(int nb, int stage) const { return dms::first_delay_for(nb, stage >= 0 && stage < 4 ? first_delay_lvl[stage] : -1, first_delay); }
  int depth_bias = 0;                 // production rule (key "depth_exp_bias"): the frame step's depth cut-off raises the static exponents (canon::depth_exp_bias)
  int exp_bias = 0;                   // test hook (dms_odometry_debug_set "exp_bias"): added to the static exponents of a call's first reductions (negative: they do not fit and are repeated)
  long long* prof = nullptr;          // [16] phase clocks of the persistent kernels (profiling only)
  TrackState* state = nullptr;
  TrackState* host_state = nullptr;  // pinned
  bool profiling = false;
  bool profiling_level0_only = false;  // dms_odometry_set_profiling(o, 2): one event pair per call, around the level-0 kernel, nothing else perturbed
  StageClock clock;  // stage times while `profiling` (dms_odometry_get_kernel_time)
};

namespace dms {

__global__ void k_track_init(TrackState* st, Prior prior, const float* __restrict__ prior_pose16, float fx, float fy, float cx, float cy,
                             int so3, int first_level, unsigned long long* sync_words, int n_sync, int inject_timeout, unsigned* zero16) {
  track_init_body(blockIdx.x, gridDim.x, threadIdx.x, blockDim.x, st, prior, prior_pose16, fx, fy, cx, cy, so3, first_level, sync_words, n_sync,
                  inject_timeout, zero16);
}

// The same with the last step of the model-side depth / intensity pyramid (prep.hip k_model_pyr_step, deferred by
// odometry_initModel_fused) in further blocks: the two are independent, one launch boundary less per frame.
// 64 x 4 thread blocks; the first `ni` blocks are k_track_init's, the next gx * gy the pyramid step's.
__global__ __launch_bounds__(256) void k_track_init_pyr(TrackState* st, Prior prior, const float* __restrict__ prior_pose16, float fx, float fy,
                                                        float cx, float cy, int so3, int first_level, unsigned long long* sync_words,
                                                        int n_sync, int inject_timeout, unsigned* zero16, int gx, int gy, int ni, View<const float> dsrc,
                                                        View<float> ddst, View<const unsigned char> isrc, View<unsigned char> idst) {
  const int b = blockIdx.x;
  if (b >= ni) {
    const int c = b - ni, by = c / gx, bx = c - by * gx;
    model_pyr_step_pixel(bx * 64 + threadIdx.x, by * 4 + threadIdx.y, dsrc, ddst, isrc, idst);
    return;
  }
  // (first in the grid: block 0's one-lane state set-up is the longest dependency chain of the launch)
  track_init_body(b, ni, threadIdx.y * 64 + threadIdx.x, 256, st, prior, prior_pose16, fx, fy, cx, cy, so3, first_level, sync_words, n_sync,
                  inject_timeout, zero16);
}

// ---------------------------------------------------------------------------------------
// Launch-per-phase form: shared pieces
// ---------------------------------------------------------------------------------------
constexpr int kRecWords = 32;  // integer record of one block: value k of the reduction in word k (grid units of canon.hpp)

// "Last block folds and solves": every block publishes its record, then takes a ticket;
// the block that draws the last ticket reads all records and runs the scalar solve, so no
// separate launch (and no dependent-launch gap) is needed.  Hand-off protocol of
// cdna_hip_programming.md §6 G16 / §5 split-K recipe: every wave drains its stores, one lane
// issues an agent-scope release, then the relaxed ticket; the last arriver issues one agent-scope
// acquire before the block reads.  Correct for any placement of the blocks over the 8 XCDs.
__device__ __forceinline__ bool last_block_arrives(unsigned* ticket) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (t == gridDim.x - 1) ? 1 : 0;
    if (last) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next launch
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    s_last = last;
  }
  __syncthreads();
  return s_last != 0;
}

// Fold of the integer records by one 256-thread block: thread (g = tid / 32, k = tid % 32) adds word k of records
// g, g + 8, ...; then thread k < 32 adds the 8 group sums.  Integer sums: exact, any order.  totals: LDS [32].
__device__ __forceinline__ void fold_records_i64(const long long* __restrict__ rec, int nblocks, long long* totals) {
  __shared__ long long s_g[8][32];
  const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
  // (eight loads in flight per thread: one dependent round trip per record made this fold 30 us of a 600-record level)
  long long s = 0;
  int b = g;
  for (; b + 56 < nblocks; b += 64) {
    long long v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = rec[(size_t)(b + 8 * u) * kRecWords + k];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; b < nblocks; b += 8) s += rec[(size_t)b * kRecWords + k];
  s_g[g][k] = s;
  __syncthreads();
  if (threadIdx.x < 32) {
    long long t = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += s_g[q][threadIdx.x];
    totals[threadIdx.x] = t;
  }
  __syncthreads();
}

__device__ __forceinline__ void fold_rows_i2(const int* __restrict__ partials, int stride, int nblocks, int* sums) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (wid < 2) {
    int s = 0;
    for (int b0 = lane; b0 < nblocks; b0 += 64 * 8) {  // 8 independent loads in flight
      int v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = b0 + 64 * u;
        v[u] = partials[(size_t)wid * stride + (b < nblocks ? b : 0)];  // clamp + select: keeps the batch in flight
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += (b0 + 64 * u < nblocks) ? v[u] : 0;
    }
    s = wave_sum_to_lane63_i(s);
    if (lane == 63) sums[wid] = s;
  }
}

// block of kBlock threads: the per-thread biased accumulators -> one integer record (words 0 .. NV-1)
template <int N>
__device__ __forceinline__ void store_record(const double (&acc)[canon::Layout<N>::NV], const int* E, long long* rec) {
  __shared__ double s_red[kBlock / kWave][32];
  const double t = canon::block_fold<N, kBlock / kWave>(canon::wave_tree<N>(acc), s_red);
  if (threadIdx.x < 32) rec[threadIdx.x] = (int)threadIdx.x < canon::Layout<N>::NV ? canon::to_units(t, canon::value_exp<N>(E, threadIdx.x)) : 0ll;
}

// integer totals -> violation flag of a reduction with N columns (threads 0 .. 31 hold one value each)
template <int N>
__device__ __forceinline__ bool totals_violate(const long long* totals) {
  bool v = false;
#pragma unroll
  for (int c = 0; c <= N; ++c) v = v || totals[canon::Layout<N>::diag(c)] >= canon::kViolation;
  return v;
}
template <int N>
__device__ __forceinline__ void totals_to_float(const long long* totals, const int* E, float* sums) {
  for (int k = 0; k < canon::Layout<N>::NV; ++k) sums[k] = canon::from_units(totals[k], canon::value_exp<N>(E, k));
}

// ---------------------------------------------------------------------------------------
// SO3 pre-alignment (RGBDOdometry.cpp:297-385), launch-per-phase form
// ---------------------------------------------------------------------------------------
struct SolveCam {
  float fx, fy, cx, cy;
};

__device__ __forceinline__ So3Params so3_params_of(const TrackState* st, int cols, int rows) {
  So3Params p;
  const float* ib = st->imageBasis;
  const float* ki = st->kinv;
  const float* kr = st->krlr;
  p.imageBasis.r0 = mk3(ib[0], ib[1], ib[2]);
  p.imageBasis.r1 = mk3(ib[3], ib[4], ib[5]);
  p.imageBasis.r2 = mk3(ib[6], ib[7], ib[8]);
  p.kinv.r0 = mk3(ki[0], ki[1], ki[2]);
  p.kinv.r1 = mk3(ki[3], ki[4], ki[5]);
  p.kinv.r2 = mk3(ki[6], ki[7], ki[8]);
  p.krlr.r0 = mk3(kr[0], kr[1], kr[2]);
  p.krlr.r1 = mk3(kr[3], kr[4], kr[5]);
  p.krlr.r2 = mk3(kr[6], kr[7], kr[8]);
  p.cols = cols;
  p.rows = rows;
  return p;
}

// the block's threads sweep pixels [first, N) with stride `stride` and leave the per-thread accumulators
__device__ __forceinline__ void so3_accumulate(const So3Params& p, const unsigned char* lastImage, size_t last_pitch,
                                               const unsigned char* nextImage, size_t next_pitch, int first, int stride,
                                               double (&acc)[kSO3]) {
  const int N = p.cols * p.rows;
  for (int i = first; i < N; i += stride) {
    const int y = i / p.cols;
    const int x = i - y * p.cols;
    float row[4];
    const bool found = so3_row(p, lastImage, last_pitch, nextImage, next_pitch, x, y, row);
    canon::acc_add<3>(acc, row, found);
  }
}

__global__ __launch_bounds__(kBlock) void k_so3_pass(TrackState* st, const unsigned char* lastImage, size_t last_pitch,
                                                     const unsigned char* nextImage, size_t next_pitch, int cols, int rows, long long* records,
                                                     unsigned* ticket, SolveCam cam, int iter, int is_last, int first_gn_level, int exp_bias) {
  if (st->so3_done) return;
  __shared__ int s_E[4];
  __shared__ double s_bias[2][32];
  __shared__ long long s_tot[32];
  __shared__ float s_sums[kSO3];
  __shared__ int s_viol;
  const So3Params p = so3_params_of(st, cols, rows);
  if (threadIdx.x == 0) {
    int E[4];
    if (iter == 0) {
      canon::static_so3(cols * rows, E);
      for (int c = 0; c < 4; ++c) E[c] = canon::clamp_e(E[c] + exp_bias);
    } else {
      for (int c = 0; c < 4; ++c) E[c] = st->E_icp[c];  // (the SO3 stage borrows the slot: no Gauss-Newton reduction has run yet)
    }
    for (int c = 0; c < 4; ++c) s_E[c] = E[c];
  }
  __syncthreads();
  if (threadIdx.x < 32) canon::write_bias<3>(s_E, s_bias, threadIdx.x);
  __syncthreads();
  double acc[kSO3];
  canon::acc_init<3>(acc, s_bias);
  so3_accumulate(p, lastImage, last_pitch, nextImage, next_pitch, blockIdx.x * blockDim.x + threadIdx.x, blockDim.x * gridDim.x, acc);
  store_record<3>(acc, s_E, records + (size_t)blockIdx.x * kRecWords);
  if (!last_block_arrives(ticket)) return;
  // ---- last block: fold, check the grid, repeat alone on a coarser one if a diagonal total did not fit, solve ----
  fold_records_i64(records, gridDim.x, s_tot);
  int retries = 0;
  for (;;) {
    if (threadIdx.x == 0) s_viol = totals_violate<3>(s_tot) ? 1 : 0;
    __syncthreads();
    if (!s_viol) break;
    if (++retries > canon::kMaxRetries) break;
    if (threadIdx.x == 0) canon::retry_step<3>(s_E);
    __syncthreads();
    if (threadIdx.x < 32) canon::write_bias<3>(s_E, s_bias, threadIdx.x);
    __syncthreads();
    canon::acc_init<3>(acc, s_bias);
    so3_accumulate(p, lastImage, last_pitch, nextImage, next_pitch, threadIdx.x, blockDim.x, acc);
    __shared__ double s_red[kBlock / kWave][32];
    const double t = canon::block_fold<3, kBlock / kWave>(canon::wave_tree<3>(acc), s_red);
    __syncthreads();
    if (threadIdx.x < 32) s_tot[threadIdx.x] = (int)threadIdx.x < kSO3 ? canon::to_units(t, canon::value_exp<3>(s_E, threadIdx.x)) : 0ll;
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  totals_to_float<3>(s_tot, s_E, s_sums);
  if (retries > canon::kMaxRetries)
    for (int k = 0; k < kSO3 - 1; ++k) s_sums[k] = 0.f;
  st->canon_retries += retries;
  sc::so3_solve_core(st, s_sums, cam.fx, cam.fy, cam.cx, cam.cy, is_last, first_gn_level);
  int E[4];
  for (int c = 0; c < 4; ++c) E[c] = s_E[c];
  canon::next_exponents<3>(s_sums, E);
  for (int c = 0; c < 4; ++c) st->E_icp[c] = E[c];
}

// ---------------------------------------------------------------------------------------
// Gauss-Newton passes (RGBDOdometry.cpp:425-586), launch-per-phase form
// ---------------------------------------------------------------------------------------
using sc::SolveArgs;

// The fused loop's own correspondence record (the 16-byte DataTerm of the operator layer carries
// the live pixel's coordinates, which are the record's position, and a float difference of two
// bytes): half the bytes written by pass 1 and read back by pass 2.
struct Corr8 {
  short zero_x, zero_y;
  short diff;  // nextImage - lastImage, an integer in [-255, 255]
  short valid;
};

struct GnArgs {
  // ICP
  MapPtrs maps;
  float fx, fy, cx, cy, distThres, angleThres, dist2Le, sine2Le;  // (the last two: IcpParams)
  // RGB
  RgbResPtrs rgb;
  Corr8* corres;
  const float* cloud;
  unsigned cloud_pitch;
  float minScale, maxDepthDelta, sobelScale;
  int cols, rows, level;
  int rgbOnly, first_of_call, exp_bias;  // canonical sums: how the level's first exponents are derived (see level_exponents)
};

// Column exponents of a level's first reduction: the call's first Gauss-Newton level starts from the static table, every
// later one from the coarser level's last totals, four times the pixels (canon.hpp).  Uniform: every block derives the same.
__device__ __forceinline__ void level_exponents(const TrackState* st, const GnArgs& a, bool first_iter, int* E_icp, int* E_rgb) {
  if (first_iter && !st->have_E) {
    canon::static_icp(a.cols * a.rows, E_icp);
    canon::static_rgb(a.cols * a.rows, a.fx, a.rgbOnly, E_rgb);
    for (int c = 0; c < 7; ++c) {
      E_icp[c] = canon::clamp_e(E_icp[c] + a.exp_bias);
      E_rgb[c] = canon::clamp_e(E_rgb[c] + a.exp_bias);
    }
    return;
  }
  for (int c = 0; c < 7; ++c) {
    E_icp[c] = st->E_icp[c];
    E_rgb[c] = st->E_rgb[c];
  }
  if (first_iter) {
    canon::level_step<6>(E_icp);
    canon::level_step<6>(E_rgb);
  }
}

__device__ __forceinline__ IcpParams icp_params_of(const float* Rcurr, const float* tcurr, const float* Rprev_inv, const float* tprev, const GnArgs& a) {
  IcpParams ip;
  ip.Rcurr.r0 = mk3(Rcurr[0], Rcurr[1], Rcurr[2]);
  ip.Rcurr.r1 = mk3(Rcurr[3], Rcurr[4], Rcurr[5]);
  ip.Rcurr.r2 = mk3(Rcurr[6], Rcurr[7], Rcurr[8]);
  ip.tcurr = mk3(tcurr[0], tcurr[1], tcurr[2]);
  ip.Rprev_inv.r0 = mk3(Rprev_inv[0], Rprev_inv[1], Rprev_inv[2]);
  ip.Rprev_inv.r1 = mk3(Rprev_inv[3], Rprev_inv[4], Rprev_inv[5]);
  ip.Rprev_inv.r2 = mk3(Rprev_inv[6], Rprev_inv[7], Rprev_inv[8]);
  ip.tprev = mk3(tprev[0], tprev[1], tprev[2]);
  ip.fx = a.fx;
  ip.fy = a.fy;
  ip.cx = a.cx;
  ip.cy = a.cy;
  ip.distThres = a.distThres;
  ip.angleThres = a.angleThres;
  ip.dist2Le = a.dist2Le;
  ip.sine2Le = a.sine2Le;
  ip.cols = a.cols;
  ip.rows = a.rows;
  return ip;
}
__device__ __forceinline__ RgbResParams rgb_params_of(const float* krkinv, const float* kt, const GnArgs& a) {
  RgbResParams rp;
  rp.krkinv.r0 = mk3(krkinv[0], krkinv[1], krkinv[2]);
  rp.krkinv.r1 = mk3(krkinv[3], krkinv[4], krkinv[5]);
  rp.krkinv.r2 = mk3(krkinv[6], krkinv[7], krkinv[8]);
  rp.kt = mk3(kt[0], kt[1], kt[2]);
  rp.minScale = a.minScale;
  rp.maxDepthDelta = a.maxDepthDelta;
  rp.cols = a.cols;
  rp.rows = a.rows;
  return rp;
}

// Pixels are handed out in chunks of kBlock*kPix: thread t of the block owns pixels
// chunk*kBlock*kPix + p*kBlock + t (p < kPix), i.e. kPix coalesced runs, and keeps the loads of all
// kPix pixels (ICP and photometric) in flight together.  Two dependent round trips per chunk.
constexpr int kPix = 2;
inline int track_blocks_for(int n) {
  int b = (n + kBlock * kPix - 1) / (kBlock * kPix);
  return b < 1 ? 1 : (b > kMaxPartialBlocks ? kMaxPartialBlocks : b);
}

// ICP rows of the pixels [first chunk, N) in steps of `chunk_stride` chunks into the per-thread accumulators
__device__ __forceinline__ void icp_accumulate(const IcpParams& ip, const GnArgs& a, int first_chunk, int chunk_stride, double (&acc)[kSE3]) {
  const int N = a.cols * a.rows;
  for (int base = first_chunk * (kBlock * kPix); base < N; base += chunk_stride * (kBlock * kPix)) {
    int idx[kPix];
    IcpOwn io[kPix];
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      idx[p] = base + p * kBlock + (int)threadIdx.x;
      const int ic = idx[p] < N ? idx[p] : 0;  // lanes past the end shadow pixel 0 and are masked below
      const int py = ic / a.cols;
      io[p] = icp_load_own(a.maps, ic - py * a.cols, py, a.rows);
    }
    IcpProj ir[kPix];
    IcpModel im[kPix];
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      ir[p] = icp_project<kTrackerFma>(ip, io[p]);
      im[p] = icp_load_model(a.maps, ir[p], a.rows);
    }
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      float row[7];
      bool found = icp_finish<kTrackerFma>(ip, io[p], ir[p], im[p], row);
      if (idx[p] >= N) {
        found = false;
#pragma unroll
        for (int k = 0; k < 7; ++k) row[k] = 0.f;
      }
      canon::acc_add<6>(acc, row, found);
    }
  }
}

// photometric rows from the correspondence image, same sweep
__device__ __forceinline__ void rgb_accumulate(const RgbStepParams& p_, const GnArgs& a, int first_chunk, int chunk_stride, double (&acc)[kSE3]) {
  const int N = a.cols * a.rows;
  for (int base = first_chunk * (kBlock * kPix); base < N; base += chunk_stride * (kBlock * kPix)) {
    dms_dataterm c[kPix];
    RgbRowIn in[kPix];
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      const int i = base + p * kBlock + (int)threadIdx.x;
      const int ic = i < N ? i : 0;
      const Corr8 c8 = a.corres[ic];
      const int y = ic / a.cols;
      c[p].zero_x = c8.zero_x;
      c[p].zero_y = c8.zero_y;
      c[p].one_x = (short)(ic - y * a.cols);
      c[p].one_y = (short)y;
      c[p].diff = (float)c8.diff;
      c[p].valid = (i < N) ? (int)c8.valid : 0;
    }
#pragma unroll
    for (int p = 0; p < kPix; ++p) in[p] = rgb_row_load(c[p], a.cloud, a.cloud_pitch, a.rgb.dIdx, a.rgb.dIdy, a.rgb.dI_pitch);
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
      float row[7];
      rgb_row_finish<kTrackerFma>(p_, c[p], in[p], row);
      canon::acc_add<6>(acc, row, c[p].valid != 0);
    }
  }
}

template <bool ICP, bool RGB>
__global__ __launch_bounds__(kBlock) void k_gn_pass1(TrackState* st, GnArgs a, long long* part_icp, int* __restrict__ part_cnt, int stride,
                                                     int first_iter) {
  if (st->level_done[a.level]) return;
  __shared__ int s_E[2][8];
  __shared__ double s_bias[2][32];
  const int N = a.cols * a.rows;
  if (threadIdx.x == 0) level_exponents(st, a, first_iter != 0, s_E[0], s_E[1]);
  __syncthreads();
  if (ICP && threadIdx.x < 32) canon::write_bias<6>(s_E[0], s_bias, threadIdx.x);
  __syncthreads();
  if (ICP) {
    const IcpParams ip = icp_params_of(st->Rcurr, st->tcurr, st->Rprev_inv, st->tprev, a);
    double acc[kSE3];
    canon::acc_init<6>(acc, s_bias);
    icp_accumulate(ip, a, blockIdx.x, gridDim.x, acc);
    store_record<6>(acc, s_E[0], part_icp + (size_t)blockIdx.x * kRecWords);
  }
  if (RGB) {
    const RgbResParams rp = rgb_params_of(st->krkinv, st->kt, a);
    int cnt = 0, sig = 0;
    for (int base = blockIdx.x * (kBlock * kPix); base < N; base += gridDim.x * (kBlock * kPix)) {
      int idx[kPix], px[kPix], py[kPix];
      RgbOwn ro[kPix];
#pragma unroll
      for (int p = 0; p < kPix; ++p) {
        idx[p] = base + p * kBlock + (int)threadIdx.x;
        const int ic = idx[p] < N ? idx[p] : 0;
        py[p] = ic / a.cols;
        px[p] = ic - py[p] * a.cols;
        ro[p] = rgb_load_own_gated(a.rgb, px[p], py[p]);
      }
      RgbProj rr[kPix];
      RgbModel rm[kPix];
#pragma unroll
      for (int p = 0; p < kPix; ++p) {
        rr[p] = rgb_project<kTrackerFma>(rp, ro[p], px[p], py[p]);
        rm[p] = rgb_load_model(a.rgb, rr[p]);
      }
#pragma unroll
      for (int p = 0; p < kPix; ++p) {
        dms_dataterm c;
        int d2;
        const bool ok = rgb_finish(rp, ro[p], rr[p], rm[p], px[p], py[p], c, d2);
        if (idx[p] < N) {
          if (ok) {
            cnt += 1;
            sig += d2;
          }
          Corr8 c8;
          c8.zero_x = c.zero_x;
          c8.zero_y = c.zero_y;
          c8.diff = (short)f2i_rz(c.diff);
          c8.valid = (short)c.valid;
          a.corres[idx[p]] = c8;
        }
      }
    }
    __shared__ int lds[kBlock / kWave][2];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    cnt = wave_sum_to_lane63_i(cnt);
    sig = wave_sum_to_lane63_i(sig);
    if (lane == 63) {
      lds[wid][0] = cnt;
      lds[wid][1] = sig;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      int s = 0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += lds[w][threadIdx.x];
      part_cnt[(size_t)threadIdx.x * stride + blockIdx.x] = s;
    }
  }
}

// every block folds the (≤1024) integer partials itself: integer sums are order-free, so
// all blocks agree bit-for-bit and no extra launch is needed to publish σ.
__device__ __forceinline__ void fold_count_pair(const int* __restrict__ part_cnt, int nb_cnt, int stride, int* s_tot /* LDS [2] */) {
  __shared__ int s_cnt[kBlock / kWave][2];
  int c = 0, g = 0;
  for (int b = threadIdx.x; b < nb_cnt; b += blockDim.x) {
    c += part_cnt[b];
    g += part_cnt[(size_t)stride + b];
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  c = wave_sum_to_lane63_i(c);
  g = wave_sum_to_lane63_i(g);
  if (lane == 63) {
    s_cnt[wid][0] = c;
    s_cnt[wid][1] = g;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += s_cnt[w][threadIdx.x];
    s_tot[threadIdx.x] = s;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_gn_pass2(TrackState* st, GnArgs a, const int* __restrict__ part_cnt, int nb_cnt, int stride,
                                                     int first_iter, long long* part_rgb) {
  if (st->level_done[a.level]) return;
  __shared__ int s_tot[2];
  __shared__ int s_E[2][8];
  __shared__ double s_bias[2][32];
  fold_count_pair(part_cnt, nb_cnt, stride, s_tot);
  const int rgbSize = s_tot[0], sigma = s_tot[1];
  const float lastErr = first_iter ? 3.402823466e+38F : st->lastRGBError;
  if (a.rgbOnly && sc::rgbonly_break(sigma, rgbSize, lastErr)) return;  // host `break`; k_gn_solve records it
  if (threadIdx.x == 0) level_exponents(st, a, first_iter != 0, s_E[0], s_E[1]);
  __syncthreads();
  if (threadIdx.x < 32) canon::write_bias<6>(s_E[1], s_bias, threadIdx.x);
  __syncthreads();
  RgbStepParams p_;
  p_.sigma = a.rgbOnly ? -1.f : sc::sigma_val(sigma, rgbSize);
  p_.fx = a.fx;
  p_.fy = a.fy;
  p_.sobelScale = a.sobelScale;
  double acc[kSE3];
  canon::acc_init<6>(acc, s_bias);
  rgb_accumulate(p_, a, blockIdx.x, gridDim.x, acc);
  store_record<6>(acc, s_E[1], part_rgb + (size_t)blockIdx.x * kRecWords);
}

// One block: fold both record sets, check their grids (a reduction whose diagonal totals did not fit is repeated by this
// block alone on a coarser grid — rare: the static guess of a call's first iteration, or a scene change between
// iterations), then the scalar section.
template <bool ICP, bool RGB>
__global__ __launch_bounds__(kBlock) void k_gn_solve(TrackState* st, GnArgs a, const long long* part_icp, const long long* part_rgb,
                                                      const int* part_cnt, int stride, int nblocks, SolveArgs q) {
  const int level = q.level, first_iter = q.first_iter;
  __shared__ long long s_ti[32], s_tr[32];
  __shared__ float s_icp[32], s_rgb[32];
  __shared__ int s_cnt[2];
  __shared__ int s_E[2][8];
  __shared__ double s_bias[2][32];
  __shared__ double s_red[kBlock / kWave][32];
  __shared__ int s_viol;
  if (st->level_done[level]) return;
  const float lastErr = first_iter ? 3.402823466e+38F : st->lastRGBError;
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) level_exponents(st, a, first_iter != 0, s_E[0], s_E[1]);
  __syncthreads();
  if (RGB) fold_rows_i2(part_cnt, stride, nblocks, s_cnt);
  __syncthreads();
  const int rgbSize = s_cnt[0], sigma = s_cnt[1];
  const bool brk = q.rgbOnly && sc::rgbonly_break(sigma, rgbSize, lastErr);
  if (brk) {
    // host `break` (RGBDOdometry.cpp:466-469): the level ends here; the next level that runs
    // needs its own K in the projection parameters
    if (threadIdx.x == 0) {
      st->level_done[level] = 1;
      double Rt[16];
      for (int i = 0; i < 16; ++i) Rt[i] = st->resultRt[i];
      sc::gn_params(Rt, sc::kpre_of(q.fx, q.fy, q.cx, q.cy, q.level_below), st->krkinv, st->kt);
    }
    return;
  }
  if (ICP) fold_records_i64(part_icp, nblocks, s_ti);
  if (RGB) fold_records_i64(part_rgb, nblocks, s_tr);
  int retries = 0;
  bool gave_up_icp = false, gave_up_rgb = false;
  if (ICP) {
    int r = 0;
    for (;;) {
      if (threadIdx.x == 0) s_viol = totals_violate<6>(s_ti) ? 1 : 0;
      __syncthreads();
      if (!s_viol) break;
      if (++r > canon::kMaxRetries) {
        gave_up_icp = true;
        break;
      }
      if (threadIdx.x == 0) canon::retry_step<6>(s_E[0]);
      __syncthreads();
      if (threadIdx.x < 32) canon::write_bias<6>(s_E[0], s_bias, threadIdx.x);
      __syncthreads();
      const IcpParams ip = icp_params_of(st->Rcurr, st->tcurr, st->Rprev_inv, st->tprev, a);
      double acc[kSE3];
      canon::acc_init<6>(acc, s_bias);
      icp_accumulate(ip, a, 0, 1, acc);
      const double t = canon::block_fold<6, kBlock / kWave>(canon::wave_tree<6>(acc), s_red);
      __syncthreads();
      if (threadIdx.x < 32) s_ti[threadIdx.x] = (int)threadIdx.x < kSE3 ? canon::to_units(t, canon::value_exp<6>(s_E[0], threadIdx.x)) : 0ll;
      __syncthreads();
    }
    retries += r > canon::kMaxRetries ? canon::kMaxRetries : r;
  }
  if (RGB) {
    int r = 0;
    for (;;) {
      if (threadIdx.x == 0) s_viol = totals_violate<6>(s_tr) ? 1 : 0;
      __syncthreads();
      if (!s_viol) break;
      if (++r > canon::kMaxRetries) {
        gave_up_rgb = true;
        break;
      }
      if (threadIdx.x == 0) canon::retry_step<6>(s_E[1]);
      __syncthreads();
      if (threadIdx.x < 32) canon::write_bias<6>(s_E[1], s_bias, threadIdx.x);
      __syncthreads();
      RgbStepParams p_;
      p_.sigma = q.rgbOnly ? -1.f : sc::sigma_val(sigma, rgbSize);
      p_.fx = a.fx;
      p_.fy = a.fy;
      p_.sobelScale = a.sobelScale;
      double acc[kSE3];
      canon::acc_init<6>(acc, s_bias);
      rgb_accumulate(p_, a, 0, 1, acc);
      const double t = canon::block_fold<6, kBlock / kWave>(canon::wave_tree<6>(acc), s_red);
      __syncthreads();
      if (threadIdx.x < 32) s_tr[threadIdx.x] = (int)threadIdx.x < kSE3 ? canon::to_units(t, canon::value_exp<6>(s_E[1], threadIdx.x)) : 0ll;
      __syncthreads();
    }
    retries += r > canon::kMaxRetries ? canon::kMaxRetries : r;
  }
  if (threadIdx.x != 0) return;
  if (ICP) {
    totals_to_float<6>(s_ti, s_E[0], s_icp);
    if (gave_up_icp)
      for (int k = 0; k < 28; ++k) s_icp[k] = 0.f;
  }
  if (RGB) {
    totals_to_float<6>(s_tr, s_E[1], s_rgb);
    if (gave_up_rgb)
      for (int k = 0; k < 28; ++k) s_rgb[k] = 0.f;
  }

  sc::GnLocal L;
#pragma unroll
  for (int i = 0; i < 16; ++i) L.resultRt[i] = st->resultRt[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) L.Rprev[i] = st->Rprev[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) L.tprev[i] = st->tprev[i];
  L.iters_run = st->iters_run[level];
  sc::gn_step_core(L, s_icp, s_rgb, rgbSize, sigma, q, sc::kpre_of(q.fx, q.fy, q.cx, q.cy, q.next_level));

  st->iters_run[level] = L.iters_run;
  st->lastRGBError = L.lastRGBError;
  st->lastRGBCount = L.lastRGBCount;
  st->lastICPError = L.lastICPError;
  st->lastICPCount = L.lastICPCount;
#pragma unroll
  for (int i = 0; i < 36; ++i) st->lastA[i] = L.lastA[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) st->lastb[i] = L.lastb[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) st->resultRt[i] = L.resultRt[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) st->Rcurr[i] = L.Rcurr[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) st->tcurr[i] = L.tcurr[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) st->krkinv[i] = L.krkinv[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) st->kt[i] = L.kt[i];
  // exponents of the next reduction from this one's totals
  for (int c = 0; c < 7; ++c) {
    st->E_icp[c] = s_E[0][c];
    st->E_rgb[c] = s_E[1][c];
  }
  if (ICP) canon::next_exponents<6>(s_icp, st->E_icp);
  if (RGB) canon::next_exponents<6>(s_rgb, st->E_rgb);
  st->have_E = 1;
  st->canon_retries += retries;
}

// ---------------------------------------------------------------------------------------
// Persistent Gauss-Newton level: ALL iterations of one pyramid level in one launch
// ---------------------------------------------------------------------------------------
// A GN iteration is two grid-wide reductions deep (sigma needs the global correspondence count;
// the 6x6 system needs every pixel), so the launch path pays three kernel boundaries, three
// dispatch ramps and three rounds of dependent state loads per iteration.  Here one grid of
// <= 256 blocks x 512 threads (at most one block per CU, 1-4 pixels per thread) stays resident for the
// whole level:
//   * everything pose independent is loaded ONCE per level into registers (own vertex / normal,
//     photometric gate, own depth / intensity / gradient);
//   * the correspondences never leave registers (no DataTerm image, no point-cloud image);
//   * both grid-wide sums are integer all-reduces in memory-side atomics: lane k of wave 0 holds the block's exact
//     total of value k in grid units (canon.hpp) and adds it with ONE non-returning 64-bit agent-scope atomic to word
//     [block % 8][k]; the same lane then polls its own 8 shard words until their arrival fields show every block — the
//     total is then in its registers.  No record, no separate barrier, no gather; integer adds are order free, so the
//     totals are bit-identical in every block, from run to run and on any grid.  The words of one shard are contiguous
//     (one coalesced atomic instruction per shard region); with the 8 shards of a value in one cache line the atomics
//     serialise per line (7.1 us instead of 1.9, scripts/bench_allreduce.hip);
//   * every block then runs the 6x6 solve itself on identical totals: all blocks hold bit-identical poses, nothing is
//     broadcast; host `break`s are uniform decisions every block takes from the same sums;
//   * a reduction whose diagonal totals do not fit the grid its exponents promised (canon.hpp) is repeated by the whole
//     grid — a uniform decision again — on a word set from the launch's pool.
// Hand-off rules follow cdna_hip_programming.md G16 (relaxed polling, agent-scope words, bounded spins, words zeroed
// by an earlier kernel on the stream); scripts/bench_gridbarrier.hip is the protocol's stand-alone visibility test.
// (kPB threads per block, at most kMaxPersistBlocks blocks: resident_rule.hpp)
constexpr int kPWaves = kPB / kWave;
constexpr unsigned kSpinLimit = 1u << 22;

struct LevelArgs {
  int n_iter, level, level_below;
  int rgbOnly;
  float icpWeight;
  float fx, fy, cx, cy;  // full-resolution intrinsics
  unsigned long long* ar;    // kArSetsPerKernel word sets of kArWords, zero on entry: one per iteration, then the retry pool
  int first_delay;           // see ar_wait (units of 64 cycles)
  long long* prof;           // optional [3][16] per-level phase clocks of block 0 (null = off)
  // last level of the call: block 0 also does what k_track_finalize does (jump gate, result block,
  // pose write-back, frame bookkeeping) instead of a one-lane launch of its own
  int early_exit;  // host side: selects the EXIT instantiation of k_gn_level
  int finalize, fin_rgb;
  float* pose16_out;
  FrameState* frame;
  float weightMultiplier;
  int interleave;       // pixel ownership: segments of a block spread over the image (track_ownership.hpp; DMS_TRACK_INTERLEAVE)
  int compact;          // photometric list: the block's gated pixels only (DMS_RGB_COMPACT; 0: every owned pixel, the work of the uncompacted kernel)
  unsigned* list_len;   // [blocks] entries of each block's photometric list, written once per launch (dms_odometry_get_rgb_compaction)
};

// ---- grid-wide integer all-reduce in memory-side atomics ------------------------------------------------------
//   sum word  = arrivals [63:58] | sum of (S + 2^52) [57:0], |S| < 2^52 grid units, <= 32 blocks per shard (canon::pack_word)
//   pair word = arrivals [63:58] | sum of v [57:0], v = the block's correspondence count or sum of squared differences
constexpr int kArShards = 8;
constexpr int kArStride = 64;                       // words per shard: slots 0..28 ICP | 32..60 photometric
constexpr int kArPairBase = kArShards * kArStride;  // then the count / sum-of-squares pair: one 128-byte line per shard (slots 0, 1),
constexpr int kArPairStride = 16;                   // apart from the lines the 58 sums arrive on (its pollers would slow those atomics)
constexpr int kArWords = kArPairBase + kArShards * kArPairStride;  // 5 KB per reduction
constexpr int kArSlotCnt = 0, kArSlotSig = 1;
constexpr int kArPool = 6;                          // extra word sets per resident launch for repeated reductions
constexpr int kArSetsPerKernel = kArRing + kArPool;
constexpr int kArSets = 4 * kArSetsPerKernel;       // SO3 + three levels

__device__ __forceinline__ unsigned long long pair_pack(unsigned long long v) { return (1ull << 58) + v; }

// wave 0, all 64 lanes: every lane with `mine` polls the 8 shard words of `slot` until they show nb arrivals.
// fld = sum of the 8 fields.  Bounded: a timeout sets *timeout and returns false.
// WHEN to poll matters more than how: a read that reaches the words before the last block's atomic has landed costs a whole
// further round trip (~0.8 us), and reads of words that are still receiving atomics slow those down.  The callers therefore
// wait `first_delay` x 64 cycles after their own arrival before the first read of the totals (nobody's sum can be complete
// earlier than one atomic flight after the last arrival).  Measured at 640x480 (level 0 / 1 / 2 launch, us), round 3:
//   probe word, then a sweep of all 58 words, no delay (round 2's form)                        137 / 53 / 41.6
//   ICP words (added a phase earlier, complete: one round trip), then the photometric words    131 / 48 / 40.5
//   the same after a delay of 8 / 16 / 30 units                                                 121.5 / 118.3 / 120.6 (level 0)
//   ICP wave sums kept in registers and folded over the waves together with the photometric
//   ones (one LDS fold and one atomic instruction for both; the pair is polled ~0.5 us earlier),
//   all 58 words polled at once after 24 units (8 on grids under 96 blocks)                     111 / 44 / 38.7
// Tried without gain: pauses between polls (1 - 12 units); the ICP words read before pass 2 and looked at after it (140: the
// early reads delay wave 0's share of the pass); every block adding to 2 or 4 copies of the words and polling one (120 ->
// 121 / 122: the readers' fan-in per line is not what limits); a delay before the pair's poll (+0 - 3 us from 4 units on);
// a block's chunks spread over the image instead of adjacent (no difference: the arrival spread is not a load imbalance);
// 16 shards instead of 8 (no difference: 13 instead of 25 same-address atomics per word against twice the words to read).
// Also without gain: the ICP rows computed after the count pair's arrival instead of before it (pass 1 -0.6 us per iteration,
// the two waits +0.9: the pair's flight was already covered by the ICP wave sums).
__device__ __forceinline__ void poll_pause(int n) {
  for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(1);  // 64 cycles each
}
template <int STRIDE>
__device__ __forceinline__ bool ar_wait(const unsigned long long* w, int slot, bool mine, int nb, unsigned long long& fld_out, int* timeout) {
  unsigned spins = 0;
  for (;;) {
    unsigned long long arr = 0, fld = 0;
    if (mine) {
      unsigned long long q[kArShards];
#pragma unroll
      for (int s = 0; s < kArShards; ++s) q[s] = __hip_atomic_load(w + s * STRIDE + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int s = 0; s < kArShards; ++s) {
        arr += q[s] >> 58;
        fld += q[s] & ((1ull << 58) - 1ull);
      }
    }
    const bool done = !mine || arr == (unsigned long long)nb;
    if (__builtin_amdgcn_ballot_w64(done) == ~0ull) {
      fld_out = fld;
      return true;
    }
    ++spins;
    // (only another block's timeout, 1, ends this wait.  2 = "retry pool exhausted" is stored by blocks that have already seen THESE
    // totals complete, or by an earlier stage: the words this block polls still fill up, and leaving with fld = 0 would take this
    // block alone down another path than the rest of the grid)
    if (spins > kSpinLimit || ((spins & 1023u) == 0u && __hip_atomic_load(timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1)) {
      __hip_atomic_store(timeout, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // never hang the device
      fld_out = 0;
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}
// completed sum words -> signed total in grid units
__device__ __forceinline__ long long ar_total(unsigned long long fld, int nb) { return (long long)fld - (long long)nb * (1ll << 52); }

// bit k set: value k of the 29-value layout is a diagonal entry (the check of canon.hpp applies to it)
__device__ __forceinline__ constexpr unsigned se3_diag_mask() {
  unsigned m = 0;
  for (int c = 0; c <= 6; ++c) m |= 1u << canon::Layout<6>::diag(c);
  return m;
}
__device__ __forceinline__ constexpr unsigned so3_diag_mask() {
  unsigned m = 0;
  for (int c = 0; c <= 3; ++c) m |= 1u << canon::Layout<3>::diag(c);
  return m;
}

static_assert(kOwnWaves == kPWaves && kOwnLanes == kWave, "track_ownership.hpp restates the block's shape");

// f(std::integral_constant<int, q>()) for q = 1 .. P, nothing for q = 0: a piece of the photometric half over the first q of a
// wave's compacted slots, as straight-line code per case (guards around every slot instead cost the level kernels 14 registers per
// slot, and scratch from three pixels per thread on).  q is the same in every lane of the wave.
template <int P, typename F>
__device__ __forceinline__ void for_slots(int q, F&& f) {
  static_assert(P >= 1 && P <= 5, "for_slots: one case per slot");
  if (q == 1) f(std::integral_constant<int, 1>());
  if constexpr (P >= 2) {
    if (q == 2) f(std::integral_constant<int, 2>());
  }
  if constexpr (P >= 3) {
    if (q == 3) f(std::integral_constant<int, 3>());
  }
  if constexpr (P >= 4) {
    if (q == 4) f(std::integral_constant<int, 4>());
  }
  if constexpr (P >= 5) {
    if (q == 5) f(std::integral_constant<int, 5>());
  }
}

// EXIT: leave the level after an iteration without any correspondence (below).  A template parameter because the
// mere presence of that exit costs the frame-to-model tracker ~1 % (codegen of the resident loop); the frame step
// instantiates it for the model-to-model pass only.
// The level as a stage: `st` is the call's state block in HBM, which every block reads at the start of the stage and block 0 writes
// back at its end for the next launch (the sticky timeout flag lives there too).  nb = blocks taking part in the all-reduces.
template <bool ICP, bool RGB, int P, bool EXIT>
__device__ __forceinline__ void gn_level_body(TrackState* st, const GnArgs& a, const LevelArgs& L, const int nb) {
  constexpr bool kFma = kTrackerFma;
  constexpr bool kSkip = P <= 3;  // waves skip the photometric slots they hold no entry for (pass 1, below)
  __shared__ sc::GnLocal s;
  __shared__ int s_redi[kPWaves][2];
  __shared__ double s_red[kPWaves][32];
  __shared__ double s_red2[2][kPWaves][32];  // [ICP | photometric][wave][value]: the two reductions folded at once
  __shared__ double s_bias[2][2][32];  // [ICP | photometric][lanes 0-31 | 32-63][value]
  __shared__ int s_E[2][8];            // column exponents of the two reductions
  __shared__ float s_sums[64];
  __shared__ double s_comb[28];  // the combined 6x6 system (27 unique entries), written by the lanes that hold the totals
  __shared__ float s_held[48];  // finalize step: new pose | previous frame's pose | inverse (frame_state.hpp)
  __shared__ int s_none;
  __shared__ int s_done;
  __shared__ int s_cs[2];
  __shared__ int s_viol;
  __shared__ int s_retries;
  __shared__ sc::KPre s_k[2];
  __shared__ unsigned s_list[RGB ? P * kPB : 1];  // the block's photometric list: pixel indices (below)
  const int tid = threadIdx.x;
  int eb_icp = 0, eb_rgb = 0;  // wave 0: bound exponents of the values this lane adds (lanes 0-28) / polls (lane k: ICP k, lane 32 + k: photometric k)
  // optional phase clock (block 0, thread 0): wall_clock64 ticks (10 ns) summed per phase into L.prof
  // (accumulated in LDS and flushed once at the end: a global read-modify-write per phase would
  // stall wave 0 for a memory round trip each time and distort what it measures)
  __shared__ long long s_prof[16];
  if (tid < 16) s_prof[tid] = 0;
  long long pc = L.prof ? wall_clock64() : 0;
  auto phase = [&](int i) {
    if (L.prof && blockIdx.x == 0 && tid == 0) {
      const long long now = wall_clock64();
      s_prof[i] += now - pc;
      pc = now;
    }
  };

  if (L.finalize && L.frame && blockIdx.x == 0 && tid >= 64 && tid < 80) s_held[16 + tid - 64] = L.frame->lastPose[tid - 64];  // for the finalize step
  // (the pose block's bottom row is not the tracker's to write, see the finalize step: it is carried through)
  if (L.finalize && L.frame && blockIdx.x == 0 && tid >= 80 && tid < 84) s_held[12 + tid - 80] = L.frame->cur.pose[12 + tid - 80];
  if (tid == 0) {
    s_none = 0;
    s_retries = 0;
    s_done = st->level_done[L.level];
    for (int i = 0; i < 16; ++i) s.resultRt[i] = st->resultRt[i];
    for (int i = 0; i < 9; ++i) {
      s.Rprev[i] = st->Rprev[i];
      s.Rprev_inv[i] = st->Rprev_inv[i];
      s.Rcurr[i] = st->Rcurr[i];
      s.krkinv[i] = st->krkinv[i];
    }
    for (int i = 0; i < 3; ++i) {
      s.tprev[i] = st->tprev[i];
      s.tcurr[i] = st->tcurr[i];
      s.kt[i] = st->kt[i];
    }
    s.lastRGBError = st->lastRGBError;
    s.lastRGBCount = st->lastRGBCount;
    s.lastICPError = st->lastICPError;
    s.lastICPCount = st->lastICPCount;
    s.iters_run = st->iters_run[L.level];
    for (int i = 0; i < 36; ++i) s.lastA[i] = st->lastA[i];
    for (int i = 0; i < 6; ++i) s.lastb[i] = st->lastb[i];
    level_exponents(st, a, true, s_E[0], s_E[1]);
    // camera matrices of this level and of the next one that runs, for the scalar section (thread 0 uses them)
    // (kept in LDS: 24 more live registers per lane would spill the 256-register pixel loop)
    s_k[0] = sc::kpre_of(L.fx, L.fy, L.cx, L.cy, L.level);
    s_k[1] = sc::kpre_of(L.fx, L.fy, L.cx, L.cy, L.level_below);
  }

  // ---- pose-independent per-pixel data, once per level ----
  // Ownership (track_ownership.hpp): slot p of this thread owns one pixel; the ICP half runs over the P owned slots.
  const int N = a.cols * a.rows;
  bool live[P], keep[P];
  unsigned own[P];
  IcpOwn io[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int idx = owned_index(L.interleave != 0, (int)blockIdx.x, nb, P, p, tid);
    // threads past the end shadow a pixel of the image and are masked.  (Not pixel 0 for all of them: where whole blocks lie past a
    // small level's image, tens of thousands of lanes loading one address queue up on its cache line - measured on a grid larger
    // than the level: +5 us at the start of level 2 and +0.7 us per pass.)
    const int ic = owned_shadow(idx, N);
    const int y = ic / a.cols, x = ic - y * a.cols;
    live[p] = idx < N;
    own[p] = (unsigned)ic;
    if (ICP) io[p] = icp_load_own(a.maps, x, y, a.rows);
    // the photometric list takes the pixel if it can ever give a correspondence: the gate image and a depth that is not NaN
    // (RgbOwn::gate).  Without compaction (L.compact = 0) every owned pixel of the image goes in.
    keep[p] = false;
    if (RGB) keep[p] = live[p] && (!L.compact || rgb_load_own_gated(a.rgb, x, y).gate);
  }
  const float invFx = 1.0f / a.fx, invFy = 1.0f / a.fy;  // as projectToPointCloud passes them
  __syncthreads();
  if (s_done) {  // level already ended (uniform: every block read the same flag)
    if (RGB && tid == 0 && L.list_len) L.list_len[blockIdx.x] = 0u;
    return;
  }
  if (tid < 64) {
    canon::write_bias<6>(s_E[tid >> 5], s_bias[tid >> 5], tid & 31);
    eb_icp = canon::value_exp<6>(s_E[0], tid & 31);
    eb_rgb = canon::value_exp<6>(s_E[1], tid & 31);
  }
  __syncthreads();

  // ---- the block's photometric list, once per level ----
  // The block ranks the pixels it keeps (P rounds, thread order inside a round) and writes their indices into LDS; thread t then
  // takes entries t, t + kPB, ... as its COMPACTED slots and loads their own data.  n entries fill Q = ceil(n / kPB) slots of the
  // block; wave w holds entries in its first Qw slots (Qw = Q or Q - 1: the list is dense, so the last slot ends in some wave).
  // Every pixel is still evaluated exactly once by the same functions on the same inputs, and the sums are exact integer sums
  // (canon.hpp): which lane takes which pixel cannot change a bit of the totals.
  // UNIFORMITY RULE: n, Q and Qw depend on the image.  Every __syncthreads(), every arrival at an all-reduce and every poll of
  // one therefore stays outside anything that depends on them; only per-pixel arithmetic and the wave tree are skipped (for_slots:
  // the slots q < Qw).  A block with an empty list (Q = 0) arrives at both all-reduces like any other, with zeros.
  // A compacted slot holds its pixel's own data in four registers: x | y << 16, gx | gy << 16, the depth, intensity | gate << 8
  // (image sides are below 2^15; unpacked where used - the level kernels sit at the 256-register limit).
  unsigned pxy[P], gxy[P], gi[P];
  float d1[P];
  auto own_of = [&](int q) {
    RgbOwn o;
    o.gate = (gi[q] >> 8) != 0u;
    o.d1 = d1[q];
    o.i1 = (unsigned char)(gi[q] & 0xffu);
    return o;
  };
  int Qw = 0;
  if (RGB) {
    unsigned n = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      unsigned tot;
      const unsigned r = block_exclusive_rank<kPWaves>(keep[p], tot);
      if (keep[p]) s_list[n + r] = own[p];  // (n + r < P * kPB: at most kPB entries per round)
      n += tot;
    }
    __syncthreads();
    if (tid == 0 && L.list_len) L.list_len[blockIdx.x] = n;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const unsigned e = (unsigned)(q * kPB + tid);
      pxy[q] = gxy[q] = gi[q] = 0u;  // a lane without an entry: gate off, no correspondence, ever
      d1[q] = 1.f;
      if (e < n) {
        const int i = (int)s_list[e];
        const int y = i / a.cols, x = i - y * a.cols;
        const RgbOwn o = rgb_load_own_gated(a.rgb, x, y);
        const short gx = trow(a.rgb.dIdx, a.rgb.dI_pitch, y)[x], gy = trow(a.rgb.dIdy, a.rgb.dI_pitch, y)[x];
        pxy[q] = (unsigned)x | ((unsigned)y << 16);
        gxy[q] = (unsigned)(unsigned short)gx | ((unsigned)(unsigned short)gy << 16);
        gi[q] = (unsigned)o.i1 | (o.gate ? 0x100u : 0u);
        d1[q] = o.d1;
      }
    }
    const unsigned first = (unsigned)(tid & ~(kWave - 1));  // this wave's first entry of slot 0
    Qw = __builtin_amdgcn_readfirstlane(n > first ? (int)((n - first + kPB - 1) / kPB) : 0);
  }

  bool ended = false;
  int pool_used = 0;  // word sets of the retry pool consumed so far (uniform)
  bool on_pool = false;
  phase(0);
  for (int it = 0; it < L.n_iter;) {
    // ---- pass 1: correspondences + ICP rows ----
    IcpParams ip;
    RgbResParams rp;
    if (ICP) ip = icp_params_of(s.Rcurr, s.tcurr, s.Rprev_inv, s.tprev, a);
    if (RGB) rp = rgb_params_of(s.krkinv, s.kt, a);
    const float lastErr = (it == 0) ? 3.402823466e+38F : s.lastRGBError;

    IcpProj ir[P];
    RgbProj rr[P];
    IcpModel im[P];
    RgbModel rm[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (ICP) {
        ir[p] = icp_project<kFma>(ip, io[p]);
        im[p] = icp_load_model(a.maps, ir[p], a.rows);
      }
    }
    // (the photometric half runs over this wave's Qw COMPACTED slots: entries of the block's list, all of them pixels of the image)
    // The slots this wave does not hold are skipped where the registers allow it: up to three pixels per thread (kSkip; 254 of 256
    // registers with three).  Every switch over the slot count costs the kernel 8 - 14 registers per slot, and with four or five
    // pixels per thread it would run out of scratch memory (68 / 208 bytes per lane; the compiler's report for every instantiation is
    // profiles/rgb_compaction_resources.txt).  There every lane runs all P slots through both passes - entries or not - as
    // before the lists.
    const int Qs = kSkip ? Qw : P;
    if (RGB)
      for_slots<P>(Qs, [&](auto qc) {
#pragma unroll
        for (int q = 0; q < decltype(qc)::value; ++q) {
          rr[q] = rgb_project<kFma>(rp, own_of(q), (int)(pxy[q] & 0xffffu), (int)(pxy[q] >> 16));
          rm[q] = rgb_load_model(a.rgb, rr[q]);
        }
      });
    float rows[P][7];
    bool found[P];
    int cnt = 0, sig = 0;
    // a slot's correspondence, held across the wait for the count pair in two registers: model pixel x | y << 16 | valid << 31,
    // and the intensity difference (the live pixel is the slot's own)
    unsigned cz[P];
    float cdiff[P];
    if (RGB)
      for_slots<P>(Qs, [&](auto qc) {
#pragma unroll
        for (int q = 0; q < decltype(qc)::value; ++q) {
          int d2;
          dms_dataterm c;
          if (rgb_finish(rp, own_of(q), rr[q], rm[q], (int)(pxy[q] & 0xffffu), (int)(pxy[q] >> 16), c, d2)) {
            cnt += 1;
            sig += d2;
          }
          cz[q] = (unsigned)(unsigned short)c.zero_x | ((unsigned)(unsigned short)c.zero_y << 16) | (c.valid ? 0x80000000u : 0u);
          cdiff[q] = c.diff;
        }
      });
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (ICP) {
        found[p] = icp_finish<kFma>(ip, io[p], ir[p], im[p], rows[p]);
        if (!live[p]) {
          found[p] = false;
#pragma unroll
          for (int k = 0; k < 7; ++k) rows[p][k] = 0.f;
        }
      }
    }
    phase(1);
    // per-block stamps of the level's middle iteration (profiling: arrival skew and completion latency of the two
    // grid-wide reductions): pass 1 done | count pair complete | pass 2 + block sum done | totals complete
    const bool stamp = L.prof && L.level == 0 && it == L.n_iter / 2 && tid == 0;
    if (stamp) L.prof[48 + blockIdx.x * 8 + 0] = wall_clock64();
    // word set of this iteration: one of a RING of kArRing sets (a level may run more iterations than the ring has sets - the 50 of an
    // inter-map call: the set of iteration it - 1 is re-armed during iteration it, below), or the next set of the retry pool
    const size_t set = (size_t)(on_pool ? kArRing + pool_used - 1 : it % kArRing) * kArWords;
    unsigned long long* arw = L.ar + set + (size_t)(blockIdx.x & (kArShards - 1)) * kArStride;
    const unsigned long long* arp = L.ar + set;
    unsigned long long* arq = L.ar + set + kArPairBase + (size_t)(blockIdx.x & (kArShards - 1)) * kArPairStride;
    int rgbSize = 0, sigma = 0;
    if (RGB) {
      // ---- count / sum-of-squares pair, arrival ----
      const int lane = tid & 63, wid = tid >> 6;
      cnt = wave_sum_to_lane63_i(cnt);
      sig = wave_sum_to_lane63_i(sig);
      if (lane == 63) {
        s_redi[wid][0] = cnt;
        s_redi[wid][1] = sig;
      }
      __syncthreads();
      if (tid < 64) {  // lanes 0-7: the 8 wave counts, lanes 8-15: the 8 wave sums (block sums fit an int)
        const int t = row8_sum_i(tid < 16 ? s_redi[tid & 7][tid >> 3] : 0);
        const unsigned long long cb = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(t, 0);
        const unsigned long long sb = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(t, 8);
        if (tid < 2) __hip_atomic_fetch_add(arq + tid, pair_pack(tid == kArSlotCnt ? cb : sb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    phase(2);
    double r_icp = 0.0;  // (both terms on) this wave's ICP sums, one value per lane pair: folded over the waves together with the photometric ones
    if (ICP) {  // the ICP sums overlap the other blocks' arrivals
      if (RGB) {
        r_icp = canon::wave_sum<6, P>(rows, found, s_bias[0]);
      } else {
        const double p_icp = canon::block_sum<6, P, kPWaves>(rows, found, s_bias[0], s_red);
        if (tid < kSE3) __hip_atomic_fetch_add(arw + tid, canon::pack_word(canon::to_units(p_icp, eb_icp)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // what the photometric rows need that does not depend on sigma - the model pixel's cloud point, exactly as k_projectPoints
    // builds it from lastDepth, and 1 / z - is taken while the count is in flight (the waves other than wave 0 only wait here);
    // with kSkip it is taken in pass 2 (held across the wait it costs the skipping kernels four registers per slot)
    f3 cpt[P];
    float cinvz[P];
    auto cloud_point = [&](int q) {
      const float z = rm[q].d0;
      cpt[q] = mk3((((float)(short)(cz[q] & 0xffffu) - a.cx) * z) * invFx, (((float)(short)((cz[q] >> 16) & 0x7fffu) - a.cy) * z) * invFy, z);
      cinvz[q] = rgb_row_invz(cpt[q]);
    };
    if (RGB && !kSkip) {
#pragma unroll
      for (int q = 0; q < P; ++q) cloud_point(q);
    }
    if (RGB) {
      if (tid < 64) {
        unsigned long long fld;
        if (stamp) L.prof[48 + blockIdx.x * 8 + 4] = wall_clock64();  // poll start
        ar_wait<kArPairStride>(arp + kArPairBase, tid, tid < 2, nb, fld, &st->sync_timeout);
        const int c0 = __builtin_amdgcn_readlane((int)fld, kArSlotCnt), s0 = __builtin_amdgcn_readlane((int)fld, kArSlotSig);
        if (tid == 0) {
          s_cs[0] = c0;
          s_cs[1] = s0;  // (the low 32 bits: an int sum, as in the reference)
        }
      }
      __syncthreads();
      rgbSize = s_cs[0];
      sigma = s_cs[1];
      phase(3);
      if (stamp) L.prof[48 + blockIdx.x * 8 + 1] = wall_clock64();
      if (L.rgbOnly && sc::rgbonly_break(sigma, rgbSize, lastErr)) {
        // host `break` (RGBDOdometry.cpp:466-469): the level ends; the next level needs its own K
        if (tid == 0) {
          double Rt[16];
          for (int i = 0; i < 16; ++i) Rt[i] = s.resultRt[i];
          sc::gn_params(Rt, s_k[1], s.krkinv, s.kt);
        }
        ended = true;
        break;
      }
      // ---- pass 2: photometric rows from the registers ----
      RgbStepParams p_;
      p_.sigma = L.rgbOnly ? -1.f : sc::sigma_val(sigma, rgbSize);
      p_.fx = a.fx;
      p_.fy = a.fy;
      p_.sobelScale = a.sobelScale;
      // this wave's photometric sums over its Qw compacted slots (wave-uniform; no barrier inside: the uniformity rule above).
      // A wave that holds no entry skips rows and tree: a wave sum carries no bias (the two halves of the wave start from opposite
      // biases), so the sums of nothing are zeros.
      double r_rgb = 0.0;
      for_slots<P>(Qs, [&](auto qc) {
        constexpr int Q = decltype(qc)::value;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          if (kSkip) cloud_point(q);
          dms_dataterm c;  // (rgb_row_finish reads `valid` and `diff`)
          c.zero_x = (short)(cz[q] & 0xffffu);
          c.zero_y = (short)((cz[q] >> 16) & 0x7fffu);
          c.one_x = (short)(pxy[q] & 0xffffu);
          c.one_y = (short)(pxy[q] >> 16);
          c.diff = cdiff[q];
          c.valid = (cz[q] >> 31) != 0u;
          RgbRowIn in;
          in.pt = cpt[q];
          in.gx = (short)(gxy[q] & 0xffffu);
          in.gy = (short)(gxy[q] >> 16);
          rgb_row_finish<kFma>(p_, c, in, rows[q], cinvz[q], true);
          found[q] = c.valid != 0;
        }
        r_rgb = canon::wave_sum<6, P, Q>(rows, found, s_bias[1]);
      });
      if (ICP) {
        // one fold for both reductions: lane k of wave 0 ends with the block's ICP total of value k, lane 32 + k with the
        // photometric one — exactly the slot (tid) their words have in the shard
        const int lane = tid & 63, wid = tid >> 6;
        // (s_red2 was last read before the barrier that follows the totals: no barrier needed in front of these stores)
        if ((lane & 1) == 0) {
          const int sl = canon::slot_of_lane<32>(lane);
          s_red2[0][wid][sl] = r_icp;
          s_red2[1][wid][sl] = r_rgb;
        }
        __syncthreads();
        if (tid < 64 && (tid & 31) < kSE3) {
          double t = 0.0;
#pragma unroll
          for (int w = 0; w < kPWaves; ++w) t += s_red2[tid >> 5][w][tid & 31];
          __hip_atomic_fetch_add(arw + tid, canon::pack_word(canon::to_units(t, tid < 32 ? eb_icp : eb_rgb)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else {
      const double p_rgb = canon::block_fold<6, kPWaves>(r_rgb, s_red);
      if (tid < kSE3) __hip_atomic_fetch_add(arw + 32 + tid, canon::pack_word(canon::to_units(p_rgb, eb_rgb)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    phase(4);
    if (stamp) L.prof[48 + blockIdx.x * 8 + 2] = wall_clock64();
    // ---- the totals arrive in the lanes that poll them ----
    if (tid < 64) {
      const int k = tid & 31;
      const bool mine = k < kSE3 && (tid < 32 ? ICP : RGB);
      unsigned long long fld;
      poll_pause(L.first_delay);
      ar_wait<kArStride>(arp, tid, mine, nb, fld, &st->sync_timeout);
      const long long tot = ar_total(fld, nb);
      const float val = mine ? canon::from_units(tot, tid < 32 ? eb_icp : eb_rgb) : 0.f;
      s_sums[tid] = val;
      {  // entry k of the combined system in lane k < 27: its photometric total sits in lane k + 32 (gn_scalar.hpp, comb_entry)
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(val), __float_as_uint(val), false, false);
        if (tid < 27) s_comb[tid] = sc::comb_entry(tid, ICP, RGB, L.icpWeight, val, __uint_as_float(sw[1]));
      }
      const bool bad = mine && ((se3_diag_mask() >> k) & 1u) && tot >= canon::kViolation;
      const unsigned long long any = __builtin_amdgcn_ballot_w64(bad);
      if (tid == 0) s_viol = ((any & 0xffffffffull) ? 1 : 0) | ((any >> 32) ? 2 : 0);
    }
    __syncthreads();
    phase(5);
    if (stamp) L.prof[48 + blockIdx.x * 8 + 3] = wall_clock64();
    // Re-arm the ring: every block has arrived in THIS iteration's totals, so every block finished reading the previous iteration's set
    // (a block adds to a set only after it has taken the totals of the set before).  Block 0 zeroes it - only when the level will come
    // round to it again - and releases the stores; the set is next used kArRing - 1 iterations (>= 60 us) later, by blocks that have seen
    // block 0's later arrivals.
    if (L.n_iter > kArRing && blockIdx.x == 0 && it >= 1 && it - 1 + kArRing < L.n_iter) {
      unsigned long long* prev = L.ar + (size_t)((it - 1) % kArRing) * kArWords;
      for (int w = tid; w < kArWords; w += kPB) prev[w] = 0ull;
      __threadfence();
    }
    if (s_viol) {
      // a diagonal total does not fit the grid its exponents promised: every block saw the same totals, so the whole
      // grid raises the exponents of that reduction and repeats the iteration on a word set of the pool (uniform)
      const int viol = s_viol;
      __syncthreads();  // (s_viol is rewritten by the repeated iteration)
      pool_used += 1;
      on_pool = true;
      if (pool_used > kArPool) {  // no word set left: the call fails like a barrier timeout (prior pose kept, nothing fused)
        if (tid == 0) __hip_atomic_store(&st->sync_timeout, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ended = true;
        break;
      }
      if (tid == 0) {
        if (viol & 1) canon::retry_step<6>(s_E[0]);
        if (viol & 2) canon::retry_step<6>(s_E[1]);
        s_retries += (viol & 1) + ((viol >> 1) & 1);  // (counted per reduction, as the oracle does)
      }
      __syncthreads();
      if (tid < 64) {
        canon::write_bias<6>(s_E[tid >> 5], s_bias[tid >> 5], tid & 31);
        eb_icp = canon::value_exp<6>(s_E[0], tid & 31);
        eb_rgb = canon::value_exp<6>(s_E[1], tid & 31);
      }
      __syncthreads();
      continue;
    }
    on_pool = false;
    if (tid == 0) {
      SolveArgs q;
      q.icp = ICP ? 1 : 0;
      q.rgb = RGB ? 1 : 0;
      q.rgbOnly = L.rgbOnly;
      q.icpWeight = L.icpWeight;
      q.level = L.level;
      q.first_iter = it == 0;
      // No correspondence of either kind: the system is all zeros and the update exactly the identity, so every
      // remaining iteration of this level would reproduce this one bit for bit (same state, same sums, same side
      // outputs) — e.g. the model-to-model pass of the full frame step while the INACTIVE view is empty.  This
      // iteration then prepares the next level's projection parameters like the level's last one, the remaining
      // ones are accounted for, and every block leaves (uniform: s_none is read after the barrier below).
      const bool none = EXIT && !L.rgbOnly && it < L.n_iter - 1 && (!ICP || s_sums[28] == 0.f) && (!RGB || rgbSize == 0);
      q.next_level = (it == L.n_iter - 1 || none) ? L.level_below : L.level;
      q.level_below = L.level_below;
      q.fx = L.fx;
      q.fy = L.fy;
      q.cx = L.cx;
      q.cy = L.cy;
      const bool last = it == L.n_iter - 1 || none;
      const sc::KPre kp = s_k[last ? 1 : 0];
      // (with rgbOnly the level may end at any iteration's break: the side outputs are then the previous iteration's)
      sc::gn_step_combined(s, s_comb, s_sums[27], s_sums[28], rgbSize, sigma, q, kp, last || L.rgbOnly);
      if (none) {
        s.iters_run += L.n_iter - 1 - it;
        s_none = 1;
      }
    } else if (tid >= 64 && tid < 128) {
      // wave 1, beside the solve: exponents and bias table of the next reduction from this one's totals (canon.hpp)
      const int set_ = (tid - 64) >> 5, k = tid & 31;
      if ((set_ == 0 && ICP) || (set_ == 1 && RGB)) {
        int E[7];
#pragma unroll
        for (int c2 = 0; c2 < 7; ++c2) E[c2] = s_E[set_][c2];
        canon::next_exponents<6>(s_sums + 32 * set_, E);
        canon::write_bias<6>(E, s_bias[set_], k);
        if (k < 7) s_E[set_][k] = E[k];
      }
    }
    __syncthreads();
    if (tid < 64) {
      eb_icp = canon::value_exp<6>(s_E[0], tid & 31);
      eb_rgb = canon::value_exp<6>(s_E[1], tid & 31);
    }
    phase(7);
    ++it;
    if constexpr (EXIT) {
      if (s_none) break;
    }
  }

  // ---- block 0 hands the state to the next kernel on the stream ----
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    if (ended) st->level_done[L.level] = 1;
    for (int i = 0; i < 16; ++i) st->resultRt[i] = s.resultRt[i];
    for (int i = 0; i < 9; ++i) {
      st->Rcurr[i] = s.Rcurr[i];
      st->krkinv[i] = s.krkinv[i];
    }
    for (int i = 0; i < 3; ++i) {
      st->tcurr[i] = s.tcurr[i];
      st->kt[i] = s.kt[i];
    }
    st->lastRGBError = s.lastRGBError;
    st->lastRGBCount = s.lastRGBCount;
    st->lastICPError = s.lastICPError;
    st->lastICPCount = s.lastICPCount;
    st->iters_run[L.level] = s.iters_run;
    for (int i = 0; i < 36; ++i) st->lastA[i] = s.lastA[i];
    for (int i = 0; i < 6; ++i) st->lastb[i] = s.lastb[i];
    for (int c2 = 0; c2 < 7; ++c2) {
      st->E_icp[c2] = s_E[0][c2];
      st->E_rgb[c2] = s_E[1][c2];
    }
    st->have_E = 1;
    st->canon_retries += s_retries;
    if (L.finalize) {  // == k_track_finalize, from the values this thread holds
      float tc[3], Rc[9];
      for (int i = 0; i < 3; ++i) tc[i] = s.tcurr[i];
      for (int i = 0; i < 9; ++i) Rc[i] = s.Rcurr[i];
      const float dx = tc[0] - s.tprev[0], dy = tc[1] - s.tprev[1], dz = tc[2] - s.tprev[2];
      const float n = sqrtf(dx * dx + dy * dy + dz * dz);
      // a grid-barrier timeout anywhere in this call (sticky flag, set before the waiting block gave up) leaves sums
      // that are not the sums of the image: the prior pose is kept and the frame step fuses nothing
      const bool timed_out = __hip_atomic_load(&st->sync_timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      if (timed_out || (L.fin_rgb && (double)n > 0.3)) {  // RGBDOdometry.cpp:589-593
        for (int i = 0; i < 9; ++i) Rc[i] = st->Rcurr[i] = s.Rprev[i];
        for (int i = 0; i < 3; ++i) tc[i] = st->tcurr[i] = s.tprev[i];
        if (!timed_out) st->rejected_jump = 1;
      }
      for (int i = 0; i < 3; ++i) st->out_trans[i] = tc[i];
      for (int i = 0; i < 9; ++i) st->out_rot[i] = Rc[i];
      // The frame step's pose block IS context.currPose(): the reference assigns the tracker's result to its top three rows only
      // (`currPose.topRightCorner(3, 1) = trans; currPose.topLeftCorner(3, 3) = rot`, ElasticFusion.cpp:246-247), so a bottom row
      // that is not exactly (0 0 0 1) - after a map merge, currPose = relativeTransform * currPose with relativeTransform =
      // recoveryPose * currPose.inverse(), a general 4 x 4 inverse (ReferenceFrame.h:95, :131) - stays with the camera, and
      // pose.inverse() (every shader's t_inv) sees it.  A pose matrix of the caller's own gets a fresh bottom row.
      const bool own = L.frame && L.pose16_out == L.frame->cur.pose;
      if (L.pose16_out) {
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) L.pose16_out[i * 4 + j] = Rc[i * 3 + j];
          L.pose16_out[i * 4 + 3] = tc[i];
        }
        if (!own) {
          L.pose16_out[12] = 0.f;
          L.pose16_out[13] = 0.f;
          L.pose16_out[14] = 0.f;
          L.pose16_out[15] = 1.f;
        }
      }
      if (L.frame) {
        // (the pose block the frame step hands in IS the frame state's current pose: then this block holds both matrices;
        // s_held[12..15] took the block's bottom row at the start of the kernel)
        if (own) {
          for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) s_held[i * 4 + j] = Rc[i * 3 + j];
            s_held[i * 4 + 3] = tc[i];
          }
        }
        frame_after_track_body(L.frame, L.weightMultiplier, __hip_atomic_load(&st->sync_timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), own ? s_held : nullptr);
      }
    }
  }
  phase(8);
  if (L.prof && blockIdx.x == 0 && tid == 0) {
    phase(9);  // = cost of one phase() call itself
    for (int i = 0; i < 10; ++i) L.prof[L.level * 16 + i] += s_prof[i];
  }
}

template <bool ICP, bool RGB, int P, bool EXIT>
__global__ __launch_bounds__(kPB) void k_gn_level(TrackState* st, GnArgs a, LevelArgs L) {
  gn_level_body<ICP, RGB, P, EXIT>(st, a, L, (int)gridDim.x);
}

// Independent work riding on the SO3 launch when the call's set-up was folded into the model pyramid kernel (frame step):
// the pyramid's deferred last step in gx * gy blocks of 64 x 8 pixels behind the nb_so3 resident blocks (gx = 0: none),
// and the re-arming of the frame step's dense counters.
// fused_model_prediction (planes != 0): the frame's prediction kernel wrote level 0 of the depth / intensity pyramid
// itself, and BOTH steps ride here from those planes (d0, i0), independent of each other: g2x * g2y blocks of 16 x 8 level-2 pixels
// (model_pyr_step2_taps: both steps in LDS) first, then gx * gy blocks of 64 x 8 level-1 pixels (model_pyr_step1_taps) into ddst /
// idst, then ONE block that empties the n_cells z-buffer cells that kernel had to leave for its other blocks to read.
struct So3Extra {
  int nb_so3, gx, gy;
  unsigned* zero16;
  View<const float> dsrc;
  View<float> ddst;
  View<const unsigned char> isrc;
  View<unsigned char> idst;
  int planes, g2x, g2y;
  View<const float> d0;
  View<const unsigned char> i0;
  View<float> ddst2;
  View<unsigned char> idst2;
  unsigned long long* zbuf;
  const int* cells;
  int n_cells;
};
static inline int so3_rider_blocks(const So3Extra& ex) { return ex.planes ? ex.g2x * ex.g2y + ex.gx * ex.gy + 1 : ex.gx * ex.gy; }

// ---------------------------------------------------------------------------------------
// Persistent SO3 pre-alignment: all (<= 10) iterations in one launch, same protocol as k_gn_level
// with one all-reduce per iteration.  The state block is copied into LDS
// and the unchanged scalar code runs on the copy; block 0 writes it back at the end.
// ---------------------------------------------------------------------------------------
// The SO3 stage: `s` is the block's LDS copy of the call's state (every block holds the same bits), loaded from `st` at the start;
// block 0 writes it back at the end.
__device__ __forceinline__ void so3_body(TrackState* st, TrackState& s, const unsigned char* lastImage, size_t last_pitch, const unsigned char* nextImage,
                                         size_t next_pitch, int cols, int rows, unsigned long long* ar, SolveCam cam, int first_gn_level, int max_iter,
                                         int exp_bias, int first_delay, const int nb) {
  __shared__ int s_viol;
  __shared__ int s_E[4];
  __shared__ double s_bias[2][32];
  __shared__ double s_red[kPWaves][32];
  __shared__ float s_sums[32];
  int eb_mine = 0;  // wave 0, lane k < 11: bound exponent of value k
  const int tid = threadIdx.x;
  for (int i = tid; i < (int)(sizeof(TrackState) / 4); i += kPB) reinterpret_cast<int*>(&s)[i] = reinterpret_cast<const int*>(st)[i];
  if (tid == 0) {
    int E[4];
    canon::static_so3(cols * rows, E);
    for (int c = 0; c < 4; ++c) s_E[c] = canon::clamp_e(E[c] + exp_bias);
  }
  __syncthreads();
  if (s.so3_done) return;
  if (tid < 32) {
    canon::write_bias<3>(s_E, s_bias, tid);
    eb_mine = canon::value_exp<3>(s_E, tid);
  }
  __syncthreads();
  const int N = cols * rows;
  const int i = blockIdx.x * kPB + tid;
  const bool live = i < N;
  const int ic = live ? i : i % N;  // (masked lanes shadow distinct pixels: see gn_level_body)
  const int y = ic / cols, x = ic - y * cols;
  int pool_used = 0, retries = 0;
  bool on_pool = false, failed = false;
  for (int it = 0; it < max_iter;) {
    const So3Params p = so3_params_of(&s, cols, rows);
    float rows_[1][4];
    bool found[1];
    found[0] = so3_row(p, lastImage, last_pitch, nextImage, next_pitch, x, y, rows_[0]);
    if (!live) {
      found[0] = false;
      rows_[0][0] = rows_[0][1] = rows_[0][2] = rows_[0][3] = 0.f;
    }
    const size_t set = (size_t)(on_pool ? kArRing + pool_used - 1 : it) * kArWords;  // (max_iter <= kArRing)
    const double pt = canon::block_sum<3, 1, kPWaves>(rows_, found, s_bias, s_red);
    if (tid < kSO3)
      __hip_atomic_fetch_add(ar + set + (size_t)(blockIdx.x & (kArShards - 1)) * kArStride + tid, canon::pack_word(canon::to_units(pt, eb_mine)),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
      unsigned long long fld;
      poll_pause(first_delay);
      ar_wait<kArStride>(ar + set, tid, tid < kSO3, nb, fld, &st->sync_timeout);
      const long long tot = ar_total(fld, nb);
      if (tid < 32) s_sums[tid] = tid < kSO3 ? canon::from_units(tot, eb_mine) : 0.f;
      const bool bad = tid < kSO3 && ((so3_diag_mask() >> tid) & 1u) && tot >= canon::kViolation;
      const unsigned long long any = __builtin_amdgcn_ballot_w64(bad);
      if (tid == 0) s_viol = any != 0ull ? 1 : 0;
    }
    __syncthreads();
    if (s_viol) {
      __syncthreads();
      pool_used += 1;
      retries += 1;
      on_pool = true;
      if (pool_used > kArPool) {
        failed = true;
        break;
      }
      if (tid == 0) canon::retry_step<3>(s_E);
      __syncthreads();
      if (tid < 32) {
        canon::write_bias<3>(s_E, s_bias, tid);
        eb_mine = canon::value_exp<3>(s_E, tid);
      }
      __syncthreads();
      continue;
    }
    on_pool = false;
    if (tid == 0) {
      sc::so3_solve_core(&s, s_sums, cam.fx, cam.fy, cam.cx, cam.cy, it == max_iter - 1 ? 1 : 0, first_gn_level);
    } else if (tid >= 64 && tid < 96) {
      int E[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) E[c] = s_E[c];
      canon::next_exponents<3>(s_sums, E);
      canon::write_bias<3>(E, s_bias, tid - 64);
      if (tid - 64 < 4) s_E[tid - 64] = E[tid - 64];
    }
    __syncthreads();
    if (s.so3_done) break;
    if (tid < 32) eb_mine = canon::value_exp<3>(s_E, tid);
    ++it;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid == 0) {
      if (failed) __hip_atomic_store(&st->sync_timeout, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s.sync_timeout = __hip_atomic_load(&st->sync_timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s.canon_retries += retries;
      if (failed && !s.so3_done) {  // the Gauss-Newton levels still need their projection parameters
        s.so3_done = 1;
        double Rt[16];
        for (int q2 = 0; q2 < 16; ++q2) Rt[q2] = s.resultRt[q2];
        sc::gn_params(Rt, sc::kpre_of(cam.fx, cam.fy, cam.cx, cam.cy, first_gn_level), s.krkinv, s.kt);
      }
    }
    __syncthreads();
    const int* src = reinterpret_cast<const int*>(&s);
    int* dst = reinterpret_cast<int*>(st);
    for (int k = tid; k < (int)(sizeof(TrackState) / 4); k += kPB) dst[k] = src[k];
  }
}

__global__ __launch_bounds__(kPB) void k_so3_level(TrackState* st, const unsigned char* lastImage, size_t last_pitch,
                                                   const unsigned char* nextImage, size_t next_pitch, int cols, int rows,
                                                   unsigned long long* ar, SolveCam cam, int first_gn_level, int max_iter, int exp_bias, int first_delay, So3Extra ex) {
  // Blocks past the resident grid carry independent work of the same call: the model pyramid's last step, whose output the
  // first Gauss-Newton level reads (not this kernel) — see So3Extra.  They take no part in the all-reduce.
  if ((int)blockIdx.x >= ex.nb_so3) {
    int c = (int)blockIdx.x - ex.nb_so3;
    if (ex.planes) {
      const PlaneTaps taps = {ex.d0, ex.i0};
      const int n2 = ex.g2x * ex.g2y, n1 = ex.gx * ex.gy;
      if (c < n2) {
        model_pyr_step2_taps<kPB>((int)threadIdx.x, c % ex.g2x, c / ex.g2x, taps, ex.d0.rows, ex.d0.cols, ex.ddst.rows, ex.ddst.cols, ex.ddst2, ex.idst2);
      } else if (c < n2 + n1) {
        c -= n2;
        model_pyr_step1_taps<kPB / 64>((int)(threadIdx.x & 63), (int)(threadIdx.x >> 6), c % ex.gx, c / ex.gx, taps, ex.d0.rows, ex.d0.cols, ex.ddst, ex.idst);
      } else {
        for (int k = (int)threadIdx.x; k < ex.n_cells; k += kPB) ex.zbuf[ex.cells[k]] = kZClear;
      }
      return;
    }
    const int by = c / ex.gx, bx = c - by * ex.gx;
    model_pyr_step_pixel(bx * 64 + (int)(threadIdx.x & 63), by * (kPB / 64) + (int)(threadIdx.x >> 6), ex.dsrc, ex.ddst, ex.isrc, ex.idst);
    return;
  }
  if (ex.zero16 && blockIdx.x == 0 && threadIdx.x < 16) ex.zero16[threadIdx.x * 16] = 0u;  // the frame step's dense counters (read before this launch)
  __shared__ TrackState s;
  so3_body(st, s, lastImage, last_pitch, nextImage, next_pitch, cols, rows, ar, cam, first_gn_level, max_iter, exp_bias, first_delay, ex.nb_so3);
}

__global__ void k_track_finalize(TrackState* st, int rgb, float* __restrict__ pose16_out, FrameState* frame, float weightMultiplier) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float dx = st->tcurr[0] - st->tprev[0], dy = st->tcurr[1] - st->tprev[1], dz = st->tcurr[2] - st->tprev[2];
  const float n = sqrtf(dx * dx + dy * dy + dz * dz);
  const bool timed_out = st->sync_timeout != 0;  // (see the finalize step of k_gn_level)
  if (timed_out || (rgb && (double)n > 0.3)) {  // RGBDOdometry.cpp:589-593
    for (int i = 0; i < 9; ++i) st->Rcurr[i] = st->Rprev[i];
    for (int i = 0; i < 3; ++i) st->tcurr[i] = st->tprev[i];
    if (!timed_out) st->rejected_jump = 1;
  }
  for (int i = 0; i < 3; ++i) st->out_trans[i] = st->tcurr[i];
  for (int i = 0; i < 9; ++i) st->out_rot[i] = st->Rcurr[i];
  if (pose16_out) {  // frame step: the pose goes straight into the context's pose block (row-major 4x4)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) pose16_out[i * 4 + j] = st->out_rot[i * 3 + j];
      pose16_out[i * 4 + 3] = st->out_trans[i];
    }
    if (!(frame && pose16_out == frame->cur.pose)) {  // (currPose keeps its bottom row: see the finalize step of k_gn_level)
      pose16_out[12] = 0.f;
      pose16_out[13] = 0.f;
      pose16_out[14] = 0.f;
      pose16_out[15] = 1.f;
    }
  }
  // frame step: pose16_out is frame->cur.pose; derive its inverse and the velocity weight here
  // instead of in a launch of their own
  if (frame) frame_after_track_body(frame, weightMultiplier, st->sync_timeout);
}

}  // namespace dms

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {

void carve_buf(Carver& c, Buf& b, int rows, int cols, size_t elem) {
  b.rows = rows;
  b.cols = cols;
  b.pitch = (size_t)cols * elem;
  b.p = c.take(b.pitch * rows);
}

void layout(dms_odometry* o, Carver& c) {
  const int W = o->width, H = o->height;
  auto mk = [&](Buf& b, int rows, int cols, size_t elem) { carve_buf(c, b, rows, cols, elem); };
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    const int r = H >> i, w = W >> i;
    mk(o->depth_tmp[i], r, w, 2);
    mk(o->vmaps_g_prev[i], r * 3, w, 4);
    mk(o->nmaps_g_prev[i], r * 3, w, 4);
    mk(o->vmaps_curr[i], r * 3, w, 4);
    mk(o->nmaps_curr[i], r * 3, w, 4);
    mk(o->lastDepth[i], r, w, 4);
    mk(o->nextDepth[i], r, w, 4);
    mk(o->lastImage[i], r, w, 1);
    mk(o->nextImage[i], r, w, 1);
    mk(o->lastNextImage[i], r, w, 1);
    mk(o->nextdIdx[i], r, w, 2);
    mk(o->nextdIdy[i], r, w, 2);
    mk(o->nextGate[i], r, w, 1);
    mk(o->pointClouds[i], r, w, 12);
    mk(o->corresImg[i], r, w, sizeof(dms_dataterm));
  }
  o->vmaps_tmp = (float*)c.take((size_t)W * H * 16);
  o->nmaps_tmp = (float*)c.take((size_t)W * H * 16);
  o->part_icp = (long long*)c.take((size_t)kRecWords * kMaxPartialBlocks * 8);
  o->part_rgb = (long long*)c.take((size_t)kRecWords * kMaxPartialBlocks * 8);
  o->part_so3 = (long long*)c.take((size_t)kRecWords * kMaxPartialBlocks * 8);
  o->part_cnt = (int*)c.take((size_t)2 * kMaxPartialBlocks * 4);
  o->tickets = (unsigned*)c.take(64);
  o->ar = (unsigned long long*)c.take((size_t)kArSets * kArWords * 8);
  o->prof = (long long*)c.take((3 * 16 + 256 * 8) * 8);
  o->list_len = (unsigned*)c.take((size_t)DMS_NUM_PYRS * kMaxPersistBlocks * 4);
  o->state = (TrackState*)c.take(sizeof(TrackState));
}

// whether a stage of this call is timed (dms_odometry_set_profiling: 1 = every stage, 2 = the level-0 kernel only)
bool timed(const dms_odometry* o, bool level0 = false) { return o->profiling && (level0 || !o->profiling_level0_only); }

// minimum squared gradient of level l (RGBDOdometry.cpp:287-291 / :453)
float rgb_min_scale(const dms_odometry* o, int l) { return (float)(pow((double)o->minGrad[l], 2.0) / pow((double)o->sobelScale, 2.0)); }

int populateDepth(dms_odometry* o, Buf* destDepths, hipStream_t s) {
  int rc;
  dms_image2d d0 = destDepths[0].img();
  if ((rc = verticesToDepth(o->vmaps_tmp, &d0, o->maxDepthRGB, s))) return rc;
  for (int i = 0; i + 1 < DMS_NUM_PYRS; i++) {
    dms_image2d a = destDepths[i].img(), b = destDepths[i + 1].img();
    if ((rc = pyrDownGaussF(&a, &b, s))) return rc;
  }
  return DMS_OK;
}

int populateImage(const dms_image2d* rgba, Buf* destImages, hipStream_t s) {
  int rc;
  dms_image2d i0 = destImages[0].img();
  if ((rc = imageToIntensity(rgba, &i0, s))) return rc;
  for (int i = 0; i + 1 < DMS_NUM_PYRS; i++) {
    dms_image2d a = destImages[i].img(), b = destImages[i + 1].img();
    if ((rc = pyrDownUcharGauss(&a, &b, s))) return rc;
  }
  return DMS_OK;
}

// RGBDOdometry::populateRGBDData (RGBDOdometry.cpp:139-160): depth from the LAST vertex map that
// initICPModel uploaded (vmaps_tmp), intensity from the given image
int populateRGBDData(dms_odometry* o, const dms_image2d* rgba, Buf* destDepths, Buf* destImages, hipStream_t s) {
  int rc;
  if ((rc = populateDepth(o, destDepths, s))) return rc;
  return populateImage(rgba, destImages, s);
}

// Sobel pyramid of nextImage (RGBDOdometry.cpp:279-283).  The reference computes it inside
// getIncrementalTransformation; here it is computed where nextImage is written and only redone
// by the tracker when nextImage is no longer the image it was computed from (SO3 handle swap).
int nextDerivatives(dms_odometry* o, hipStream_t s) {
  int rc;
  for (int i = 0; i < DMS_NUM_PYRS; i++) {
    dms_image2d a = o->nextImage[i].img(), dx = o->nextdIdx[i].img(), dy = o->nextdIdy[i].img(), g = o->nextGate[i].img();
    if ((rc = derivativeGate(&a, &dx, &dy, &g, rgb_min_scale(o, i), s))) return rc;
  }
  o->deriv_of = o->nextImage[0].p;
  return DMS_OK;
}

}  // namespace

extern "C" {

int dms_odometry_create(dms_odometry** out, int width, int height, float cx, float cy, float fx, float fy, float distThresh,
                        float angleThresh) {
  DMS_REQUIRE(out, "null out");
  DMS_REQUIRE(width >= 16 && height >= 16 && width <= 32767 && height <= 32767, "bad resolution");
  dms_odometry* o = new dms_odometry();
  o->width = width;
  o->height = height;
  o->cx = cx;
  o->cy = cy;
  o->fx = fx;
  o->fy = fy;
  o->distThres = distThresh > 0.f ? distThresh : 0.10f;
  o->angleThres = angleThresh > 0.f ? angleThresh : (float)sin(20.f * 3.14159254f / 180.f);
  o->sobelScale = (float)(1.0 / pow(2.0, 3));  // RGBDOdometry.cpp:34-35
  o->maxDepthDeltaRGB = 0.07f;
  o->maxDepthRGB = 6.0f;
  o->minGrad[0] = 5;
  o->minGrad[1] = 3;
  o->minGrad[2] = 1;
  Carver sz;
  layout(o, sz);
  o->arena_bytes = up256(sz.off);
  hipError_t e = hipMalloc((void**)&o->arena, o->arena_bytes);
  if (e != hipSuccess) {
    delete o;
    return hip_fail(e, "hipMalloc(arena)", __FILE__, __LINE__);
  }
  // pyramids start as zeros (the reference's cudaMallocPitch memory is uninitialised;
  // zero keeps the never-initialised-RGB case of GPUTest.cpp:247-286 deterministic)
  (void)hipMemset(o->arena, 0, o->arena_bytes);
  Carver c;
  c.base = o->arena;
  layout(o, c);
  e = hipHostMalloc((void**)&o->host_state, sizeof(TrackState), hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipFree(o->arena);
    delete o;
    return hip_fail(e, "hipHostMalloc", __FILE__, __LINE__);
  }
  memset(o->host_state, 0, sizeof(TrackState));
  {  // execution switches: the environment is consulted here and nowhere else
    const char* e = getenv("DMS_TRACK_MODE");
    o->resident = !(e && strcmp(e, "launches") == 0);
    e = getenv("DMS_TRACK_EARLY_EXIT");
    o->early_exit_force = e ? (e[0] != '0' ? 1 : 0) : -1;
    e = getenv("DMS_PERSIST_BLOCKS");
    if (e && atoi(e) > 0) o->persist_target = atoi(e);
    {  // how many blocks of a resident kernel fit the device at once (see max_resident_blocks)
      int dev = 0, cus = 0, per_cu = 0;
      (void)hipGetDevice(&dev);
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_gn_level<true, true, 3, false>, kPB, 0) != hipSuccess) per_cu = 0;
      (void)hipGetLastError();
      o->max_resident_blocks = device_bound(cus, per_cu);
      if (o->max_resident_blocks <= 0) o->resident = false;
    }
    e = getenv("DMS_PERSIST_MAX_BLOCKS");
    o->max_resident_blocks = lowered_bound(o->max_resident_blocks, e ? atoi(e) : 0);
    e = getenv("DMS_AR_FIRST_DELAY");  // units of 64 cycles before the first read of the totals; default: by grid size
    if (e && atoi(e) >= 0 && atoi(e) <= 1000) o->first_delay = atoi(e);
    e = getenv("DMS_TRACK_LONG_RESIDENT");
    if (e) o->long_levels_resident = atoi(e) != 0;
    e = getenv("DMS_TRACK_INTERLEAVE");  // A/B switches of the resident level kernels: same bits either way
    if (e) o->track_interleave = atoi(e) != 0;
    e = getenv("DMS_RGB_COMPACT");
    if (e) o->rgb_compact = atoi(e) != 0;
    e = getenv("DMS_AR_FIRST_DELAY_BY_LEVEL");  // "l0,l1,l2,so3" in the same units (-1 keeps the rule for that stage): the per-level sweep
    if (e) {
      int v[4] = {-1, -1, -1, -1};
      if (sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) >= 1)
        for (int i = 0; i < 4; ++i)
          if (v[i] >= 0 && v[i] <= 1000) o->first_delay_lvl[i] = v[i];
    }
  }
  *out = o;
  return DMS_OK;
}

int dms_odometry_debug_set(dms_odometry* o, const char* key, int value) {
  DMS_REQUIRE(o && key, "null argument");
  if (strcmp(key, "exp_bias") == 0) {
    DMS_REQUIRE(value >= -100 && value <= 100, "exp_bias out of range");
    o->exp_bias = value;
    return DMS_OK;
  }
  if (strcmp(key, "depth_exp_bias") == 0) {  // the frame step's rule, kept apart from the test hook: the two add
    DMS_REQUIRE(value >= 0 && value <= 100, "depth_exp_bias out of range");
    o->depth_bias = value;
    return DMS_OK;
  }
  if (strcmp(key, "track_interleave") == 0) {
    o->track_interleave = value != 0;
    return DMS_OK;
  }
  if (strcmp(key, "rgb_compact") == 0) {
    o->rgb_compact = value != 0;
    return DMS_OK;
  }
  DMS_REQUIRE(false, "unknown key");
}

// Photometric lists of the last tracker call's resident kernel of `level`: the largest number of compacted slots any block ran
// (0 .. pixels per thread) and the entries of all lists together.  Zeros where the level ran launch-per-phase or without the
// photometric term.  Waits for the device.
int dms_odometry_get_rgb_compaction(dms_odometry* o, int level, int* max_slots, int* entries) {
  DMS_REQUIRE(o, "null argument");
  DMS_REQUIRE(level >= 0 && level < DMS_NUM_PYRS, "bad level");
  int q = 0, total = 0;
  const int nb = o->last_rgb[level] ? o->last_shape_nb[level] : 0;
  if (nb > 0) {
    unsigned len[kMaxPersistBlocks];
    DMS_HIP(hipDeviceSynchronize());
    DMS_HIP(hipMemcpy(len, o->list_len + (size_t)level * kMaxPersistBlocks, (size_t)nb * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < nb; ++b) {
      const int slots = (int)((len[b] + kPB - 1) / kPB);
      if (slots > q) q = slots;
      total += (int)len[b];
    }
  }
  if (max_slots) *max_slots = q;
  if (entries) *entries = total;
  return DMS_OK;
}

int dms_odometry_set_resident_budget(dms_odometry* o, int max_blocks, int unchained) {
  DMS_REQUIRE(o && max_blocks >= 0, "bad argument");
  o->budget_cap = max_blocks;
  o->unchained_ok = unchained != 0 && max_blocks > 0;
  return DMS_OK;
}

int dms_odometry_get_resident_budget(dms_odometry* o, int* max_blocks, int* unchained) {
  DMS_REQUIRE(o, "null argument");
  if (max_blocks) *max_blocks = o->budget_cap;
  if (unchained) *unchained = o->unchained_ok ? 1 : 0;
  return DMS_OK;
}

int dms_odometry_get_mode(dms_odometry* o, int* resident, int* max_resident_blocks, int* fell_back) {
  DMS_REQUIRE(o, "null argument");
  if (resident) *resident = o->resident ? 1 : 0;
  if (max_resident_blocks) *max_resident_blocks = o->max_resident_blocks;
  if (fell_back) *fell_back = o->fell_back ? 1 : 0;
  return DMS_OK;
}

int dms_odometry_get_level_shape(dms_odometry* o, int level, int* pixels_per_thread, int* blocks, int* resident) {
  DMS_REQUIRE(o, "null argument");
  DMS_REQUIRE(level >= 0 && level < DMS_NUM_PYRS, "bad level");
  if (pixels_per_thread) *pixels_per_thread = o->last_shape_P[level];
  if (blocks) *blocks = o->last_shape_nb[level];
  if (resident) *resident = o->last_shape_nb[level] > 0 ? 1 : 0;
  return DMS_OK;
}

int dms_odometry_canon_retries(dms_odometry* o, int* retries) {
  DMS_REQUIRE(o && retries, "null argument");
  *retries = o->host_state->canon_retries;
  return DMS_OK;
}

// host builds of the scalar section (test hooks, see dmslam.h)
int dms_debug_scalar_gn(const float* sums_icp, const float* sums_rgb, float icpWeight, const float* Rprev, const float* tprev,
                        double* resultRt, float fx, float fy, float cx, float cy, int next_level, double* A, double* b, float* Rcurr,
                        float* tcurr, float* krkinv, float* kt) {
  DMS_REQUIRE((sums_icp || sums_rgb) && Rprev && tprev && resultRt && A && b && Rcurr && tcurr && krkinv && kt, "null argument");
  sc::GnLocal L;
  memset(&L, 0, sizeof(L));
  for (int i = 0; i < 16; ++i) L.resultRt[i] = resultRt[i];
  for (int i = 0; i < 9; ++i) L.Rprev[i] = Rprev[i];
  for (int i = 0; i < 3; ++i) L.tprev[i] = tprev[i];
  sc::SolveArgs q;
  memset(&q, 0, sizeof(q));
  q.icp = sums_icp ? 1 : 0;
  q.rgb = sums_rgb ? 1 : 0;
  q.icpWeight = icpWeight;
  float zero[29] = {0};
  sc::gn_step_core(L, sums_icp ? sums_icp : zero, sums_rgb ? sums_rgb : zero, 1, 1, q, sc::kpre_of(fx, fy, cx, cy, next_level), true);
  for (int i = 0; i < 16; ++i) resultRt[i] = L.resultRt[i];
  for (int i = 0; i < 36; ++i) A[i] = L.lastA[i];
  for (int i = 0; i < 6; ++i) b[i] = L.lastb[i];
  for (int i = 0; i < 9; ++i) {
    Rcurr[i] = L.Rcurr[i];
    krkinv[i] = L.krkinv[i];
  }
  for (int i = 0; i < 3; ++i) {
    tcurr[i] = L.tcurr[i];
    kt[i] = L.kt[i];
  }
  return DMS_OK;
}

int dms_debug_scalar_so3(const float* sums, float* R_lr, double* resultR, float fx, float fy, float cx, float cy, float* imageBasis,
                         float* kinv, float* krlr) {
  DMS_REQUIRE(sums && R_lr && resultR && imageBasis && kinv && krlr, "null argument");
  TrackState st;
  memset(&st, 0, sizeof(st));
  for (int i = 0; i < 9; ++i) {
    st.R_lr[i] = R_lr[i];
    st.resultR[i] = st.lastResultR[i] = resultR[i];
  }
  st.so3_lastError = 3.402823466e+38F / 2;
  st.so3_lastCount = 3.402823466e+38F / 2;
  sc::so3_solve_core(&st, sums, fx, fy, cx, cy, 0, 0);
  for (int i = 0; i < 9; ++i) {
    R_lr[i] = st.R_lr[i];
    resultR[i] = st.resultR[i];
    imageBasis[i] = st.imageBasis[i];
    kinv[i] = st.kinv[i];
    krlr[i] = st.krlr[i];
  }
  return DMS_OK;
}

int dms_odometry_inject_timeout(dms_odometry* o, int calls) {
  DMS_REQUIRE(o && calls >= 0, "bad argument");
  o->inject_timeouts = calls;
  return DMS_OK;
}

int dms_odometry_set_exec(dms_odometry* o, int resident, int early_exit, int coarse_launch) {
  DMS_REQUIRE(o, "null argument");
  DMS_REQUIRE(coarse_launch <= 0, "the coarse launch was removed (SO3 + level 2 + level 1 in one resident launch: same bits, slower): pass -1 or 0");
  // resident = 1 on a handle whose device cannot hold a resident kernel's blocks at once (max_resident_blocks = 0) stays off
  if (resident >= 0) o->resident = resident != 0 && o->max_resident_blocks > 0;
  if (early_exit >= 0) o->early_exit_force = early_exit ? 1 : 0;  // -1: unchanged (keeps a DMS_TRACK_EARLY_EXIT choice made at creation)
  return DMS_OK;
}

// deprecated form (rounds 1-2 had summation variants: fp64 block sums, a record protocol; every sum is the exact integer sum of canon.hpp now)
int dms_odometry_set_mode(dms_odometry* o, int resident, int fp64_sums, int early_exit, int atomic_reduce) {
  (void)fp64_sums;
  (void)atomic_reduce;
  return dms_odometry_set_exec(o, resident, early_exit, -1);
}

// the frame step's reaction to a resident kernel that timed out: launch-per-phase from here on, nothing else touched
int dms_odometry_fall_back_to_launches(dms_odometry* o) {
  DMS_REQUIRE(o, "null argument");
  o->resident = false;
  o->fell_back = true;
  return DMS_OK;
}

int dms_odometry_destroy(dms_odometry* o) {
  if (!o) return DMS_OK;
  if (o->arena) (void)hipFree(o->arena);
  if (o->ring_arena) (void)hipFree(o->ring_arena);
  if (o->host_state) (void)hipHostFree(o->host_state);
  delete o;
  return DMS_OK;
}

int dms_odometry_initICP_depth(dms_odometry* o, const dms_image2d* depth, float depthCutoff, dms_stream st) {
  DMS_REQUIRE(o && depth && depth->data, "null argument");
  DMS_REQUIRE(depth->rows == o->height && depth->cols == o->width, "depth must be full resolution");
  hipStream_t s = (hipStream_t)st;
  DMS_HIP(hipMemcpy2DAsync(o->depth_tmp[0].p, o->depth_tmp[0].pitch, depth->data, depth->pitch, (size_t)o->width * 2, o->height,
                           hipMemcpyDeviceToDevice, s));
  int rc;
  for (int i = 1; i < DMS_NUM_PYRS; ++i) {
    dms_image2d a = o->depth_tmp[i - 1].img(), b = o->depth_tmp[i].img();
    if ((rc = pyrDown(&a, &b, s))) return rc;
  }
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    const int div = 1 << i;
    dms_camera k = {o->fx / div, o->fy / div, o->cx / div, o->cy / div};
    dms_image2d d = o->depth_tmp[i].img(), v = o->vmaps_curr[i].img(), n = o->nmaps_curr[i].img();
    if ((rc = createVMap(&k, &d, &v, depthCutoff, s))) return rc;
    if ((rc = createNMap(&v, &n, s))) return rc;
  }
  return DMS_OK;
}

int dms_odometry_initICP_maps(dms_odometry* o, const float* verts, const float* norms, float depthCutoff, dms_stream st) {
  (void)depthCutoff;
  DMS_REQUIRE(o && verts && norms, "null argument");
  hipStream_t s = (hipStream_t)st;
  const size_t bytes = (size_t)o->width * o->height * 16;
  DMS_HIP(hipMemcpyAsync(o->vmaps_tmp, verts, bytes, hipMemcpyDeviceToDevice, s));
  DMS_HIP(hipMemcpyAsync(o->nmaps_tmp, norms, bytes, hipMemcpyDeviceToDevice, s));
  int rc;
  dms_image2d v0 = o->vmaps_curr[0].img(), n0 = o->nmaps_curr[0].img();
  if ((rc = copyMaps(o->vmaps_tmp, o->nmaps_tmp, &v0, &n0, s))) return rc;
  for (int i = 1; i < DMS_NUM_PYRS; ++i) {
    dms_image2d va = o->vmaps_curr[i - 1].img(), vb = o->vmaps_curr[i].img();
    dms_image2d na = o->nmaps_curr[i - 1].img(), nb = o->nmaps_curr[i].img();
    if ((rc = resizeMap(&va, &vb, false, s))) return rc;
    if ((rc = resizeMap(&na, &nb, true, s))) return rc;
  }
  return DMS_OK;
}

int dms_odometry_initICPModel(dms_odometry* o, const float* verts, const float* norms, float depthCutoff, const float* modelPose,
                              dms_stream st) {
  (void)depthCutoff;
  DMS_REQUIRE(o && verts && norms && modelPose, "null argument");
  hipStream_t s = (hipStream_t)st;
  const size_t bytes = (size_t)o->width * o->height * 16;
  DMS_HIP(hipMemcpyAsync(o->vmaps_tmp, verts, bytes, hipMemcpyDeviceToDevice, s));
  DMS_HIP(hipMemcpyAsync(o->nmaps_tmp, norms, bytes, hipMemcpyDeviceToDevice, s));
  int rc;
  dms_image2d v0 = o->vmaps_g_prev[0].img(), n0 = o->nmaps_g_prev[0].img();
  if ((rc = copyMaps(o->vmaps_tmp, o->nmaps_tmp, &v0, &n0, s))) return rc;
  for (int i = 1; i < DMS_NUM_PYRS; ++i) {
    dms_image2d va = o->vmaps_g_prev[i - 1].img(), vb = o->vmaps_g_prev[i].img();
    dms_image2d na = o->nmaps_g_prev[i - 1].img(), nb = o->nmaps_g_prev[i].img();
    if ((rc = resizeMap(&va, &vb, false, s))) return rc;
    if ((rc = resizeMap(&na, &nb, true, s))) return rc;
  }
  dms_mat33 R;
  dms_float3 t;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R.m[i * 3 + j] = modelPose[i * 4 + j];
  t.x = modelPose[3];
  t.y = modelPose[7];
  t.z = modelPose[11];
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    dms_image2d v = o->vmaps_g_prev[i].img(), n = o->nmaps_g_prev[i].img();
    if ((rc = transformMaps(&v, &n, &R, &t, &v, &n, s))) return rc;
  }
  return DMS_OK;
}

int dms_odometry_initRGB(dms_odometry* o, const dms_image2d* rgba, dms_stream s) {
  DMS_REQUIRE(o && rgba && rgba->data, "null argument");
  DMS_REQUIRE(rgba->rows == o->height && rgba->cols == o->width, "rgba must be full resolution");
  int rc = populateRGBDData(o, rgba, o->nextDepth, o->nextImage, (hipStream_t)s);
  if (rc) return rc;
  return nextDerivatives(o, (hipStream_t)s);
}
int dms_odometry_initRGBModel(dms_odometry* o, const dms_image2d* rgba, dms_stream s) {
  DMS_REQUIRE(o && rgba && rgba->data, "null argument");
  DMS_REQUIRE(rgba->rows == o->height && rgba->cols == o->width, "rgba must be full resolution");
  return populateRGBDData(o, rgba, o->lastDepth, o->lastImage, (hipStream_t)s);
}
int dms_odometry_initFirstRGB(dms_odometry* o, const dms_image2d* rgba, dms_stream st) {
  DMS_REQUIRE(o && rgba && rgba->data, "null argument");
  DMS_REQUIRE(rgba->rows == o->height && rgba->cols == o->width, "rgba must be full resolution");
  hipStream_t s = (hipStream_t)st;
  int rc;
  dms_image2d i0 = o->lastNextImage[0].img();
  if ((rc = imageToIntensity(rgba, &i0, s))) return rc;
  for (int i = 0; i + 1 < DMS_NUM_PYRS; i++) {
    dms_image2d a = o->lastNextImage[i].img(), b = o->lastNextImage[i + 1].img();
    if ((rc = pyrDownUcharGauss(&a, &b, s))) return rc;
  }
  return DMS_OK;
}

int dms_odometry_track_async(dms_odometry* o, const float* trans, const float* rot, int rgbOnly, float icpWeight, int pyramid,
                             int fastOdom, int so3, int interMap, dms_stream st) {
  DMS_REQUIRE(o && trans && rot, "null argument");
  return odometry_track_enqueue(o, trans, rot, nullptr, rgbOnly, icpWeight, pyramid, fastOdom, so3, interMap, (hipStream_t)st);
}

}  // extern "C"

namespace dms {

// ---- persistent level kernels: launch shape and cross-stream serialisation ----
// dms_odometry::resident = false (DMS_TRACK_MODE=launches at creation) selects the three-launches-per-iteration path.

// The shapes, the bounds and the cross-stream chain's rules are resident_rule.hpp's.  Here: the chain's state per device, and the
// section that carries out its decisions - the mutex, the device query, the event and the three HIP calls.
struct PersistChain {
  static constexpr int kDevices = 64;
  std::mutex mu;
  hipEvent_t ev[kDevices] = {};
  ChainState state[kDevices];
};
static PersistChain g_persist;
// DMS_PERSIST_UNCHAINED=1 (chain_exempt; DMS_PERSIST_MAX_BLOCKS of each handle, summed, <= compute units).  Read once.
static bool unchained() {
  static const bool u = [] {
    const char* e = getenv("DMS_PERSIST_UNCHAINED");
    return e && atoi(e) != 0;
  }();
  return u;
}
struct PersistSection {
  hipStream_t s;
  int budget;  // largest resident grid of the handle this section belongs to
  bool handle_unchained;
  bool active = false;          // the mutex is held
  ChainState* chain = nullptr;  // (active without one: a device outside the table - synchronised, no state kept)
  hipEvent_t* ev = nullptr;
  bool carried = false;         // the section's last launch was given the chain's event
  PersistSection(hipStream_t s_, int budget_, bool handle_unchained_ = false) : s(s_), budget(budget_), handle_unchained(handle_unchained_) {}
  void begin() {
    if (active) return;
    if (unchained() || handle_unchained) {
      static const int cus = [] {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess ? n : 0;
      }();
      if (chain_exempt(unchained(), handle_unchained, budget, cus)) return;
    }
    g_persist.mu.lock();
    active = true;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= PersistChain::kDevices) {
      (void)hipDeviceSynchronize();
      return;
    }
    chain = &g_persist.state[dev];
    ev = &g_persist.ev[dev];
    switch (chain->enter(s)) {
      case ChainState::device_sync: (void)hipDeviceSynchronize(); break;
      case ChainState::wait_event: (void)hipStreamWaitEvent(s, *ev, 0); break;
      case ChainState::proceed: break;
    }
  }
  // the device's event, created at its first use
  bool have_event() {
    if (!*ev && hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      *ev = nullptr;
    }
    return *ev != nullptr;
  }
  // The event the section's LAST resident launch is to carry as its completion signal (ChainState::owes_event); null when none is
  // owed (one stream only so far) - then nothing changes.
  hipEvent_t closing_event() {
    if (!chain) return nullptr;
    chain->ext_events = ext_events();
    if (!chain->owes_event() || !have_event()) return nullptr;
    carried = true;
    return *ev;
  }
  static bool ext_events() {
    static const bool on = [] {
      const char* e = getenv("DMS_PERSIST_EXT_EVENT");
      return !e || atoi(e) != 0;
    }();
    return on;
  }
  ~PersistSection() {
    if (!active) return;
    if (chain && chain->leave(carried)) {
      const bool ok = have_event() && hipEventRecord(*ev, s) == hipSuccess;
      if (!ok) (void)hipGetLastError();
      chain->recorded(ok);
    }
    g_persist.mu.unlock();
  }
};

// `done`: an event that fires with THIS launch's completion signal (hipExtLaunchKernelGGL) - no marker packet behind the kernel
template <bool ICP, bool RGB, int P, bool EXIT>
static void launch_gn_level_p(int nb, hipStream_t s, TrackState* st, const GnArgs& a, const LevelArgs& L, hipEvent_t done) {
  if (done)
    hipExtLaunchKernelGGL((k_gn_level<ICP, RGB, P, EXIT>), dim3(nb), dim3(kPB), 0, s, nullptr, done, 0, st, a, L);
  else
    hipLaunchKernelGGL((k_gn_level<ICP, RGB, P, EXIT>), dim3(nb), dim3(kPB), 0, s, st, a, L);
}
template <bool ICP, bool RGB, bool EXIT>
static void launch_gn_level_f(int P, int nb, hipStream_t s, TrackState* st, const GnArgs& a, const LevelArgs& L, hipEvent_t done) {
  if (P == 1)
    launch_gn_level_p<ICP, RGB, 1, EXIT>(nb, s, st, a, L, done);
  else if (P == 2)
    launch_gn_level_p<ICP, RGB, 2, EXIT>(nb, s, st, a, L, done);
  else if (P == 3)
    launch_gn_level_p<ICP, RGB, 3, EXIT>(nb, s, st, a, L, done);
  else if (P == 4)
    launch_gn_level_p<ICP, RGB, 4, EXIT>(nb, s, st, a, L, done);
  else
    launch_gn_level_p<ICP, RGB, 5, EXIT>(nb, s, st, a, L, done);
}
template <bool ICP, bool RGB>
static void launch_gn_level(int P, int nb, hipStream_t s, TrackState* st, const GnArgs& a, const LevelArgs& L, hipEvent_t done = nullptr) {
  if (L.early_exit)
    launch_gn_level_f<ICP, RGB, true>(P, nb, s, st, a, L, done);
  else
    launch_gn_level_f<ICP, RGB, false>(P, nb, s, st, a, L, done);
}

static inline int budget_of(const dms_odometry* o) { return handle_bound(o->budget_cap, o->max_resident_blocks); }
static inline int level_pixels(const dms_odometry* o, int l) { return o->vmaps_curr[l].cols * (o->vmaps_curr[l].rows / 3); }

// grid of the resident SO3 kernel for this handle; 0 = the SO3 stage runs launch-per-phase
static int so3_resident_blocks(const dms_odometry* o) {
  const Buf& li = o->lastNextImage[2];
  return so3_blocks(o->resident, li.rows * li.cols, budget_of(o));
}

int odometry_track_enqueue(dms_odometry* o, const float* trans, const float* rot, const float* prior_pose16_dev, int rgbOnly,
                           float icpWeight, int pyramid, int fastOdom, int so3, int interMap, hipStream_t s, FrameState* frame,
                           float weightMultiplier) {
  DMS_REQUIRE(o, "null argument");
  // what an earlier kernel has prepared for this call; taken before anything can fail, so that no error return leaves a promise behind
  const dms_odometry::NextCall nc = o->next_call;
  o->next_call = dms_odometry::NextCall();
  DMS_REQUIRE((trans && rot) || prior_pose16_dev, "null argument");
  const bool icp = !rgbOnly && icpWeight > 0;
  const bool rgb = rgbOnly || icpWeight < 100;
  DMS_REQUIRE(icp || rgb, "neither ICP nor RGB term active");
  int rc;

  Prior prior;
  memset(&prior, 0, sizeof(prior));
  if (!prior_pose16_dev) {
    memcpy(prior.v, trans, 3 * sizeof(float));
    memcpy(prior.v + 3, rot, 9 * sizeof(float));
  }

  if (rgb && o->deriv_of != o->nextImage[0].p) {
    if ((rc = nextDerivatives(o, s))) return rc;
  }

  int iterations[DMS_NUM_PYRS];
  iterations[0] = interMap ? 50 : fastOdom ? 3 : 10;
  iterations[1] = interMap ? 50 : pyramid ? 5 : 0;
  iterations[2] = interMap ? 50 : pyramid ? 4 : 0;
  int first_level = 0;
  for (int l = DMS_NUM_PYRS - 1; l >= 0; --l)
    if (iterations[l] > 0) {
      first_level = l;
      break;
    }

  // set-up already done inside the kernel that prepared the model side (frame step): nothing to launch here; the SO3 launch below
  // carries the pyramid steps left to it and re-arms the dense counters
  typedef dms_odometry::NextCall NextCall;
  So3Extra ex;
  memset(&ex, 0, sizeof(ex));
  if (nc.kind == NextCall::folded || nc.kind == NextCall::folded_planes) {
    DMS_REQUIRE(so3 && so3_resident_blocks(o) > 0 && nc.so3 == (so3 ? 1 : 0) && nc.first_level == first_level && nc.prior == prior_pose16_dev &&
                    prior_pose16_dev,
                "track call differs from the one its folded set-up was prepared for");
    ex.zero16 = nc.dense_cnt_zero;
    if (nc.kind == NextCall::folded_planes) {
      dms_image2d d0 = o->lastDepth[0].img(), d1 = o->lastDepth[1].img(), d2 = o->lastDepth[2].img();
      dms_image2d i0 = o->lastImage[0].img(), i1 = o->lastImage[1].img(), i2 = o->lastImage[2].img();
      ex.planes = 1;
      ex.gx = (d1.cols + 63) / 64;
      ex.gy = (d1.rows + kPB / 64 - 1) / (kPB / 64);
      ex.g2x = (d2.cols + 15) / 16;
      ex.g2y = (d2.rows + 7) / 8;
      ex.d0 = view<const float>(&d0);
      ex.i0 = view<const unsigned char>(&i0);
      ex.ddst = view<float>(&d1);
      ex.idst = view<unsigned char>(&i1);
      ex.ddst2 = view<float>(&d2);
      ex.idst2 = view<unsigned char>(&i2);
      ex.zbuf = nc.zbuf;
      ex.cells = nc.cells;
      ex.n_cells = nc.n_cells;
    } else {
      dms_image2d d1 = o->lastDepth[1].img(), d2 = o->lastDepth[2].img(), i1 = o->lastImage[1].img(), i2 = o->lastImage[2].img();
      ex.gx = (d2.cols + 63) / 64;
      ex.gy = (d2.rows + kPB / 64 - 1) / (kPB / 64);
      ex.dsrc = view<const float>(&d1);
      ex.ddst = view<float>(&d2);
      ex.isrc = view<const unsigned char>(&i1);
      ex.idst = view<unsigned char>(&i2);
    }
  } else {
    StageTimer t(o->clock, s, "track_init", timed(o));
    // all-reduce words of the call's resident kernels (resident mode only)
    const int zero_pairs = o->resident ? (int)((size_t)kArSets * kArWords / 2) : 0;
    const int ni = o->resident ? 16 : 1;
    if (nc.kind == NextCall::deferred_pyr) {
      dms_image2d d1 = o->lastDepth[1].img(), d2 = o->lastDepth[2].img(), i1 = o->lastImage[1].img(), i2 = o->lastImage[2].img();
      const int gx = (d2.cols + 63) / 64, gy = (d2.rows + 3) / 4;
      hipLaunchKernelGGL(k_track_init_pyr, dim3(gx * gy + ni), dim3(64, 4), 0, s, o->state, prior, prior_pose16_dev, o->fx, o->fy, o->cx, o->cy,
                         so3 ? 1 : 0, first_level, o->ar, zero_pairs, o->inject_timeouts > 0 ? 1 : 0, nc.dense_cnt_zero, gx, gy, ni,
                         view<const float>(&d1), view<float>(&d2), view<const unsigned char>(&i1), view<unsigned char>(&i2));
    } else {
      hipLaunchKernelGGL(k_track_init, dim3(ni), dim3(256), 0, s, o->state, prior, prior_pose16_dev, o->fx, o->fy, o->cx, o->cy, so3 ? 1 : 0,
                         first_level, o->ar, zero_pairs, o->inject_timeouts > 0 ? 1 : 0, nc.dense_cnt_zero);
    }
    DMS_CHECK_LAUNCH();
    if (o->inject_timeouts > 0) o->inject_timeouts -= 1;
  }

  PersistSection persist(s, budget_of(o), o->unchained_ok);

  auto level_below_of = [&](int l) {
    for (int q = l - 1; q >= 0; --q)
      if (iterations[q] > 0) return q;
    return l;
  };
  auto gn_args_of = [&](int l) {
    const int div = 1 << l;
    GnArgs a;
    memset(&a, 0, sizeof(a));
    a.maps.vcurr = (const float*)o->vmaps_curr[l].p;
    a.maps.vcurr_pitch = o->vmaps_curr[l].pitch;
    a.maps.ncurr = (const float*)o->nmaps_curr[l].p;
    a.maps.ncurr_pitch = o->nmaps_curr[l].pitch;
    a.maps.vprev = (const float*)o->vmaps_g_prev[l].p;
    a.maps.vprev_pitch = o->vmaps_g_prev[l].pitch;
    a.maps.nprev = (const float*)o->nmaps_g_prev[l].p;
    a.maps.nprev_pitch = o->nmaps_g_prev[l].pitch;
    a.fx = o->fx / div;
    a.fy = o->fy / div;
    a.cx = o->cx / div;
    a.cy = o->cy / div;
    a.distThres = o->distThres;
    a.angleThres = o->angleThres;
    a.dist2Le = sqrt_le_bound(o->distThres);
    a.sine2Le = sqrt_lt_bound(o->angleThres);
    a.rgb.dIdx = (const short*)o->nextdIdx[l].p;
    a.rgb.dIdy = (const short*)o->nextdIdy[l].p;
    a.rgb.dI_pitch = o->nextdIdx[l].pitch;
    a.rgb.lastDepth = (const float*)o->lastDepth[l].p;
    a.rgb.lastDepth_pitch = o->lastDepth[l].pitch;
    a.rgb.nextDepth = (const float*)o->nextDepth[l].p;
    a.rgb.nextDepth_pitch = o->nextDepth[l].pitch;
    a.rgb.lastImage = (const unsigned char*)o->lastImage[l].p;
    a.rgb.lastImage_pitch = o->lastImage[l].pitch;
    a.rgb.nextImage = (const unsigned char*)o->nextImage[l].p;
    a.rgb.nextImage_pitch = o->nextImage[l].pitch;
    a.rgb.gate = (const unsigned char*)o->nextGate[l].p;
    a.rgb.gate_pitch = o->nextGate[l].pitch;
    a.corres = (Corr8*)o->corresImg[l].p;
    a.cloud = (const float*)o->pointClouds[l].p;
    a.cloud_pitch = o->pointClouds[l].pitch;
    // pow(minimumGradientMagnitudes[i], 2.0) / pow(sobelScale, 2.0) (RGBDOdometry.cpp:445)
    a.minScale = rgb_min_scale(o, l);
    a.maxDepthDelta = o->maxDepthDeltaRGB;
    a.sobelScale = o->sobelScale;
    a.cols = o->vmaps_curr[l].cols;
    a.rows = o->vmaps_curr[l].rows / 3;
    a.level = l;
    a.rgbOnly = rgbOnly ? 1 : 0;
    a.exp_bias = o->exp_bias + o->depth_bias;
    return a;
  };
  auto level_args_of = [&](int l, int pnb) {
    LevelArgs L;
    L.n_iter = iterations[l];
    L.level = l;
    L.level_below = level_below_of(l);
    L.rgbOnly = rgbOnly ? 1 : 0;
    L.icpWeight = icpWeight;
    L.fx = o->fx;
    L.fy = o->fy;
    L.cx = o->cx;
    L.cy = o->cy;
    L.ar = o->ar + (size_t)(1 + l) * kArSetsPerKernel * kArWords;
    L.first_delay = o->first_delay_for(pnb, l);
    L.prof = (o->profiling && !o->profiling_level0_only) ? o->prof : nullptr;
    // on for trackers that ask for it (the frame step's model-to-model pass) unless forced either way
    L.early_exit = o->early_exit_force >= 0 ? o->early_exit_force : (o->early_exit ? 1 : 0);
    L.finalize = (l == 0) ? 1 : 0;  // level 0 always runs last
    L.fin_rgb = rgb ? 1 : 0;
    L.pose16_out = frame ? const_cast<float*>(prior_pose16_dev) : nullptr;
    L.frame = frame;
    L.weightMultiplier = weightMultiplier;
    L.interleave = o->track_interleave ? 1 : 0;
    L.compact = o->rgb_compact ? 1 : 0;
    L.list_len = o->list_len + (size_t)l * kMaxPersistBlocks;
    return L;
  };
  auto level_shape = [&](int l, int& pP, int& pnb) {
    const LevelShape sh = call_level_shape(budget_of(o), o->persist_target, iterations[l], o->resident, o->long_levels_resident, level_pixels(o, l));
    o->last_shape_P[l] = pP = sh.P;
    o->last_shape_nb[l] = pnb = sh.blocks;
  };

  if (so3) {
    const int L = 2;
    const Buf& li = o->lastNextImage[L];
    const Buf& ni = o->nextImage[L];
    const int nb = reduce_blocks_for(li.rows * li.cols);
    const int nbp = so3_resident_blocks(o);
    if (nbp > 0) {
      persist.begin();
      StageTimer t(o->clock, s, "so3_level", timed(o));
      SolveCam cam = {o->fx, o->fy, o->cx, o->cy};
      ex.nb_so3 = nbp;
      hipLaunchKernelGGL(k_so3_level, dim3(nbp + so3_rider_blocks(ex)), dim3(kPB), 0, s, o->state, (const unsigned char*)li.p, li.pitch,
                         (const unsigned char*)ni.p, ni.pitch, ni.cols, ni.rows, o->ar, cam, first_level, 10, o->exp_bias + o->depth_bias, o->first_delay_for(nbp, 3), ex);
      DMS_CHECK_LAUNCH();
    } else
    for (int i = 0; i < 10; ++i) {
      {
        StageTimer t(o->clock, s, "so3_pass", timed(o));
        SolveCam cam = {o->fx, o->fy, o->cx, o->cy};
        hipLaunchKernelGGL(k_so3_pass, dim3(nb), dim3(kBlock), 0, s, o->state, (const unsigned char*)li.p, li.pitch,
                           (const unsigned char*)ni.p, ni.pitch, ni.cols, ni.rows, o->part_so3, o->tickets, cam, i, i == 9 ? 1 : 0, first_level,
                           o->exp_bias + o->depth_bias);
        DMS_CHECK_LAUNCH();
      }
    }
  }

  bool finalized_in_kernel = false;
  for (int l = DMS_NUM_PYRS - 1; l >= 0; --l) {
    int pP = 1, pnb = 0;
    level_shape(l, pP, pnb);
    const bool persistent = pnb > 0;
    o->last_rgb[l] = rgb && persistent && iterations[l] > 0;
    if (rgb && !persistent) {  // the persistent kernel rebuilds the cloud point from lastDepth itself
      dms_camera k = {o->fx, o->fy, o->cx, o->cy};
      dms_image2d d = o->lastDepth[l].img(), c = o->pointClouds[l].img();
      if ((rc = projectToPointCloud(&d, &c, &k, l, s))) return rc;
    }
    if (iterations[l] == 0) continue;
    const GnArgs a = gn_args_of(l);
    const int nb = track_blocks_for(a.cols * a.rows);
    const int level_below = level_below_of(l);
    if (persistent) {
      const LevelArgs L = level_args_of(l, pnb);
      if (l == 0) finalized_in_kernel = true;
      persist.begin();
      static const char* const kLevelTimer[3] = {"gn_level0", "gn_level1", "gn_level2"};
      StageTimer t(o->clock, s, kLevelTimer[l], timed(o, l == 0));
      hipEvent_t done = (l == 0) ? persist.closing_event() : nullptr;  // level 0 is the section's last resident launch
      if (icp && rgb)
        launch_gn_level<true, true>(pP, pnb, s, o->state, a, L, done);
      else if (icp)
        launch_gn_level<true, false>(pP, pnb, s, o->state, a, L, done);
      else
        launch_gn_level<false, true>(pP, pnb, s, o->state, a, L, done);
      DMS_CHECK_LAUNCH();
      continue;
    }
    for (int j = 0; j < iterations[l]; ++j) {
      const int next_level = (j == iterations[l] - 1) ? level_below : l;
      SolveArgs q;
      q.icp = icp ? 1 : 0;
      q.rgb = rgb ? 1 : 0;
      q.rgbOnly = rgbOnly ? 1 : 0;
      q.icpWeight = icpWeight;
      q.level = l;
      q.first_iter = j == 0 ? 1 : 0;
      q.next_level = next_level;
      q.level_below = level_below;
      q.fx = o->fx;
      q.fy = o->fy;
      q.cx = o->cx;
      q.cy = o->cy;
      {
        StageTimer t(o->clock, s, "gn_pass1", timed(o));
        if (icp && rgb)
          hipLaunchKernelGGL((k_gn_pass1<true, true>), dim3(nb), dim3(kBlock), 0, s, o->state, a, o->part_icp, o->part_cnt, kMaxPartialBlocks, j == 0 ? 1 : 0);
        else if (icp)
          hipLaunchKernelGGL((k_gn_pass1<true, false>), dim3(nb), dim3(kBlock), 0, s, o->state, a, o->part_icp, o->part_cnt, kMaxPartialBlocks, j == 0 ? 1 : 0);
        else
          hipLaunchKernelGGL((k_gn_pass1<false, true>), dim3(nb), dim3(kBlock), 0, s, o->state, a, o->part_icp, o->part_cnt, kMaxPartialBlocks, j == 0 ? 1 : 0);
        DMS_CHECK_LAUNCH();
      }
      if (rgb) {
        StageTimer t(o->clock, s, "gn_pass2", timed(o));
        hipLaunchKernelGGL(k_gn_pass2, dim3(nb), dim3(kBlock), 0, s, o->state, a, o->part_cnt, nb, kMaxPartialBlocks, j == 0 ? 1 : 0, o->part_rgb);
        DMS_CHECK_LAUNCH();
      }
      {
        StageTimer t(o->clock, s, "gn_solve", timed(o));
        if (icp && rgb)
          hipLaunchKernelGGL((k_gn_solve<true, true>), dim3(1), dim3(kBlock), 0, s, o->state, a, o->part_icp, o->part_rgb, o->part_cnt, kMaxPartialBlocks, nb, q);
        else if (icp)
          hipLaunchKernelGGL((k_gn_solve<true, false>), dim3(1), dim3(kBlock), 0, s, o->state, a, o->part_icp, o->part_rgb, o->part_cnt, kMaxPartialBlocks, nb, q);
        else
          hipLaunchKernelGGL((k_gn_solve<false, true>), dim3(1), dim3(kBlock), 0, s, o->state, a, o->part_icp, o->part_rgb, o->part_cnt, kMaxPartialBlocks, nb, q);
        DMS_CHECK_LAUNCH();
      }
    }
  }

  if (!finalized_in_kernel) {
    StageTimer t(o->clock, s, "track_finalize", timed(o));
    // frame step (frame state given): the result is written back into the pose block the prior came from;
    // a device prior without frame state (model-to-model tracking) is read-only
    hipLaunchKernelGGL(k_track_finalize, dim3(1), dim3(64), 0, s, o->state, rgb ? 1 : 0,
                       frame ? const_cast<float*>(prior_pose16_dev) : nullptr, frame, weightMultiplier);
    DMS_CHECK_LAUNCH();
  }
  // (the result block is copied to the host by dms_odometry_fetch_result, not once per call)

  if (so3) {  // RGBDOdometry.cpp:595-601 — stream-ordered, so swapping the handles is enough
    for (int i = 0; i < DMS_NUM_PYRS; i++) std::swap(o->lastNextImage[i], o->nextImage[i]);
  }
  return DMS_OK;
}

// ---- device-resident variants used by the frame step (fusion_frame.hip) --------------------
__global__ void k_track_pose_out(const TrackState* __restrict__ st, float* __restrict__ pose16) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose16[i * 4 + j] = st->out_rot[i * 3 + j];
    pose16[i * 4 + 3] = st->out_trans[i];
  }
  pose16[12] = 0.f;
  pose16[13] = 0.f;
  pose16[14] = 0.f;
  pose16[15] = 1.f;
}

int odometry_result_pose(dms_odometry* o, float* pose16_dev, hipStream_t s) {
  hipLaunchKernelGGL(k_track_pose_out, dim3(1), dim3(64), 0, s, o->state, pose16_dev);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

// ---- local loop-closure candidate (ElasticFusion.cpp:427-474) --------------------------------
// One block, after the model-to-model tracker: thread 0 takes the acceptance decision from the
// tracker's side outputs (getCovariance = inverse of lastA by partially pivoted elimination in fp64,
// RGBDOdometry.cpp:607-610; thresholds of ElasticFusion.cpp:428-442), then the block samples the
// W/20 x H/20 nearest-neighbour grid of the ACTIVE vertex map and the INACTIVE time map
// (Resize::vertex / Resize::time, :443-444) and compacts the surface constraints in the reference's
// order (columns outer, rows inner, :446-447).
__global__ __launch_bounds__(256) void k_loop_candidate(const TrackState* __restrict__ st, FrameState* __restrict__ frame,
                                                        const float4* __restrict__ vertex, const unsigned short* __restrict__ oldTime,
                                                        int cols, int rows, float maxDepth, LoopState* __restrict__ out,
                                                        float* __restrict__ cons) {
  __shared__ int s_ok;
  __shared__ int s_wave[4];
  __shared__ int s_base;
  // Gauss-Jordan on the augmented 6x12 matrix in LDS, one thread per element: the same operations
  // in the same order per element as the scalar loop of dms_odometry_getCovariance
  __shared__ double s_m[6][12];
  const int er = threadIdx.x / 12, ej = threadIdx.x % 12;
  const bool elem = threadIdx.x < 72;
  if (elem) s_m[er][ej] = ej < 6 ? st->lastA[er * 6 + ej] : ((ej - 6 == er) ? 1.0 : 0.0);
  __syncthreads();
  for (int c = 0; c < 6; ++c) {
    int p = c;
    for (int r = c + 1; r < 6; ++r)
      if (fabs(s_m[r][c]) > fabs(s_m[p][c])) p = r;
    __syncthreads();
    if (p != c && threadIdx.x < 12) {
      const double t0 = s_m[c][threadIdx.x];
      s_m[c][threadIdx.x] = s_m[p][threadIdx.x];
      s_m[p][threadIdx.x] = t0;
    }
    __syncthreads();
    const double d = s_m[c][c];
    __syncthreads();
    if (threadIdx.x < 12) s_m[c][threadIdx.x] /= d;
    __syncthreads();
    const double f = elem ? s_m[er][c] : 0.0;
    __syncthreads();
    if (elem && er != c) s_m[er][ej] -= f * s_m[c][ej];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    bool covOk = true;
    for (int i = 0; i < 6; ++i) {
      const double cii = s_m[i][6 + i];
      out->cov_diag[i] = cii;
      if (cii > 8e-05) covOk = false;
    }
    const bool timed_out = st->sync_timeout != 0;  // model-to-model pass invalid: no candidate, counted like a tracker timeout
    if (st->sync_timeout == 2)
      frame->track_range_failures += 1;
    else if (timed_out)
      frame->track_timeouts += 1;
    const int ok = (!timed_out && covOk && st->lastICPCount > 15000.f && st->lastICPError < 0.0003f) ? 1 : 0;
    out->ok = ok;
    out->icp_error = st->lastICPError;
    out->icp_count = st->lastICPCount;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) out->est_pose[i * 4 + j] = st->out_rot[i * 3 + j];
      out->est_pose[i * 4 + 3] = st->out_trans[i];
    }
    out->est_pose[12] = out->est_pose[13] = out->est_pose[14] = 0.f;
    out->est_pose[15] = 1.f;
    s_ok = ok;
    s_base = 0;
  }
  __syncthreads();
  if (!s_ok) {
    if (threadIdx.x == 0) out->n_constraints = 0;
    return;
  }
  const int dw = cols / 20, dh = rows / 20, n = dw * dh;
  const float* P = frame->cur.pose;
  for (int base = 0; base < n; base += 256) {
    const int k = base + (int)threadIdx.x;
    bool valid = false;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned short t = 0;
    if (k < n) {
      const int i = k / dh, j = k - i * dh;
      const float u = ((float)i + 0.5f) / (float)dw, v = ((float)j + 0.5f) / (float)dh;
      const int sx = texel(u, (float)cols, cols), sy = texel(v, (float)rows, rows);
      p = vertex[(size_t)sy * cols + sx];
      t = oldTime[(size_t)sy * cols + sx];
      valid = p.z > 0.f && p.z < maxDepth && t > 0;
    }
    const unsigned long long m = __ballot(valid);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int q = 0; q < w; ++q) off += s_wave[q];
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (valid) {
      float* c = cons + (size_t)off * 8;
      for (int r = 0; r < 3; ++r) {
        c[r] = P[r * 4 + 0] * p.x + P[r * 4 + 1] * p.y + P[r * 4 + 2] * p.z + P[r * 4 + 3];
        c[3 + r] = st->out_rot[r * 3 + 0] * p.x + st->out_rot[r * 3 + 1] * p.y + st->out_rot[r * 3 + 2] * p.z + st->out_trans[r];
      }
      c[6] = (float)t;
      c[7] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) out->n_constraints = s_base;
}

int odometry_loop_candidate(dms_odometry* o, FrameState* frame, const dms_image2d* vertex, const dms_image2d* oldTime, float maxDepth,
                            LoopState* out, float* cons, hipStream_t s) {
  hipLaunchKernelGGL(k_loop_candidate, dim3(1), dim3(256), 0, s, o->state, frame, (const float4*)vertex->data,
                     (const unsigned short*)oldTime->data, vertex->cols, vertex->rows, maxDepth, out, cons);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

// ---- live-frame ring (see dms_odometry::LiveSet) ----
void odometry_set_early_exit(dms_odometry* o, int on) { o->early_exit = on != 0; }

// compute units the resident tracker kernels of this handle leave free at their widest level (-1: launch-per-phase, nothing
// is held): what an overlapping stream can use without keeping a resident block off the device
int odometry_free_cus(const dms_odometry* o) {
  if (!o->resident) return -1;
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return -1;
  int widest = so3_resident_blocks(o);
  for (int l = 0; l < DMS_NUM_PYRS; ++l) {  // the device's bound and no iteration count: see call_level_shape
    const int nb = call_level_shape(o->max_resident_blocks, o->persist_target, 0, true, o->long_levels_resident, level_pixels(o, l)).blocks;
    widest = nb > widest ? nb : widest;
  }
  return cus - widest;
}

int odometry_enable_ring(dms_odometry* o) {
  if (o->ring_enabled) return DMS_OK;
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    o->ring[0].depth_tmp[i] = o->depth_tmp[i];
    o->ring[0].vmaps_curr[i] = o->vmaps_curr[i];
    o->ring[0].nmaps_curr[i] = o->nmaps_curr[i];
    o->ring[0].nextImage[i] = o->nextImage[i];
    o->ring[0].nextdIdx[i] = o->nextdIdx[i];
    o->ring[0].nextdIdy[i] = o->nextdIdy[i];
    o->ring[0].nextGate[i] = o->nextGate[i];
  }
  for (int pass = 0; pass < 2; ++pass) {
    Carver c;
    c.base = pass ? o->ring_arena : nullptr;
    const int W = o->width, H = o->height;
    auto mk = [&](Buf& b, int rows, int cols, size_t elem) { carve_buf(c, b, rows, cols, elem); };
    for (int k = 1; k < 3; ++k)
      for (int i = 0; i < DMS_NUM_PYRS; ++i) {
        const int r = H >> i, w = W >> i;
        mk(o->ring[k].depth_tmp[i], r, w, 2);
        mk(o->ring[k].vmaps_curr[i], r * 3, w, 4);
        mk(o->ring[k].nmaps_curr[i], r * 3, w, 4);
        mk(o->ring[k].nextImage[i], r, w, 1);
        mk(o->ring[k].nextdIdx[i], r, w, 2);
        mk(o->ring[k].nextdIdy[i], r, w, 2);
        mk(o->ring[k].nextGate[i], r, w, 1);
      }
    if (!pass) {
      const size_t bytes = up256(c.off);
      hipError_t e = hipMalloc((void**)&o->ring_arena, bytes);
      if (e == hipSuccess) e = hipMemset(o->ring_arena, 0, bytes);
      if (e != hipSuccess) return hip_fail(e, "hipMalloc(live ring)", __FILE__, __LINE__);
    }
  }
  o->ring_enabled = true;
  return DMS_OK;
}

// point the tracker's live-frame buffers at ring set k (host-side handle swap, stream-ordered use)
void odometry_bind_live(dms_odometry* o, int k) {
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    o->depth_tmp[i] = o->ring[k].depth_tmp[i];
    o->vmaps_curr[i] = o->ring[k].vmaps_curr[i];
    o->nmaps_curr[i] = o->ring[k].nmaps_curr[i];
    o->nextImage[i] = o->ring[k].nextImage[i];
    o->nextdIdx[i] = o->ring[k].nextdIdx[i];
    o->nextdIdy[i] = o->ring[k].nextdIdy[i];
    o->nextGate[i] = o->ring[k].nextGate[i];
  }
  o->deriv_of = o->nextImage[0].p;  // every ring set carries the derivatives of its own image
}

void odometry_bind_lastnext(dms_odometry* o, int k) {
  for (int i = 0; i < DMS_NUM_PYRS; ++i) o->lastNextImage[i] = o->ring[k].nextImage[i];
}

// The bound live set's three pyramid levels, for the frame step's fused live half (prep.hip liveLevelsFused): it writes them
// all itself and the derivative pyramid with them (`mark_derivatives`: the bookkeeping of nextDerivatives)
int odometry_live_views(dms_odometry* o, dms_image2d* depth, dms_image2d* vmap, dms_image2d* nmap, dms_image2d* image, dms_image2d* dx,
                        dms_image2d* dy, dms_image2d* gate, float* minScale, bool mark_derivatives) {
  for (int l = 0; l < DMS_NUM_PYRS; ++l) {
    depth[l] = o->depth_tmp[l].img();
    vmap[l] = o->vmaps_curr[l].img();
    nmap[l] = o->nmaps_curr[l].img();
    image[l] = o->nextImage[l].img();
    dx[l] = o->nextdIdx[l].img();
    dy[l] = o->nextdIdy[l].img();
    gate[l] = o->nextGate[l].img();
    minScale[l] = rgb_min_scale(o, l);
  }
  if (mark_derivatives) o->deriv_of = o->nextImage[0].p;
  return DMS_OK;
}

// live half of initRGB: intensity pyramid + derivative pyramid of the bound live set
int odometry_initRGB_image(dms_odometry* o, const dms_image2d* rgba, hipStream_t s) {
  int rc = populateImage(rgba, o->nextImage, s);
  if (rc) return rc;
  return nextDerivatives(o, s);
}

// model half of initRGB.  populateRGBDData derives nextDepth from the same vmaps_tmp (and the same
// cutoff) as initRGBModel derived lastDepth a moment earlier, so the two pyramids are identical:
// the handles are aliased instead of recomputing three kernels.
void odometry_alias_next_depth(dms_odometry* o) {
  for (int i = 0; i < DMS_NUM_PYRS; ++i) o->nextDepth[i] = o->lastDepth[i];
}

// views of the live intensity and depth pyramids at `level` (RGBDOdometry::nextImg / nextD, RGBDOdometry.h:79-87)
int odometry_next_buffers(dms_odometry* o, int level, dms_image2d* nextImage, dms_image2d* nextDepth) {
  DMS_REQUIRE(o && level >= 0 && level < DMS_NUM_PYRS, "bad argument");
  if (nextImage) *nextImage = o->nextImage[level].img();
  if (nextDepth) *nextDepth = o->nextDepth[level].img();
  return DMS_OK;
}

// the set-up of the track call `fold` describes as a block group of the kernel that prepares the call's model side: fills `ti` and
// returns the promise the call is checked against (odometry_track_enqueue), for the writer to complete and store
static dms_odometry::NextCall fold_init_args(dms_odometry* o, const TrackFold* fold, TrackInitArgs* ti, dms_odometry::NextCall::Kind kind) {
  const int it1 = fold->pyramid ? 5 : 0, it2 = fold->pyramid ? 4 : 0;
  ti->st = o->state;
  ti->prior_pose16 = fold->prior_pose16;
  ti->fx = o->fx;
  ti->fy = o->fy;
  ti->cx = o->cx;
  ti->cy = o->cy;
  ti->so3 = 1;
  ti->first_level = it2 > 0 ? 2 : (it1 > 0 ? 1 : 0);
  ti->sync_words = o->ar;
  ti->n_sync = (int)((size_t)kArSets * kArWords / 2);
  ti->inject_timeout = o->inject_timeouts > 0 ? 1 : 0;
  if (o->inject_timeouts > 0) o->inject_timeouts -= 1;
  ti->blocks = 16;
  dms_odometry::NextCall nc;
  nc.kind = kind;
  nc.so3 = 1;
  nc.first_level = ti->first_level;
  nc.prior = fold->prior_pose16;
  return nc;
}

int odometry_model_views_begin(dms_odometry* o, const TrackFold* fold, ModelMapViews* mv, TrackInitArgs* ti, unsigned long long* zbuf,
                               const int* cells, int n_cells) {
  if (!o || !fold || !mv || !ti || !zbuf || !cells) return 0;
  if (!o->resident || !fold->prior_pose16 || !fold->so3 || fold->interMap || so3_resident_blocks(o) <= 0) return 0;
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    dms_image2d v = o->vmaps_g_prev[i].img(), n = o->nmaps_g_prev[i].img();
    mv->v[i] = view<float>(&v);
    mv->n[i] = view<float>(&n);
  }
  dms_image2d d0 = o->lastDepth[0].img(), i0 = o->lastImage[0].img();
  mv->depth0 = view<float>(&d0);
  mv->inten0 = view<unsigned char>(&i0);
  mv->cutOff = o->maxDepthRGB;
  memset(ti, 0, sizeof(*ti));
  dms_odometry::NextCall nc = fold_init_args(o, fold, ti, dms_odometry::NextCall::folded_planes);
  nc.zbuf = zbuf;
  nc.cells = cells;
  nc.n_cells = n_cells;
  o->next_call = nc;
  return 1;
}

// initICPModel + initRGBModel of the frame step in four launches (prep.hip, modelPyramidFused).
// The operator-layer staging copy vmaps_tmp is not written on this path; nextDepth is aliased to
// lastDepth by the caller, so nothing reads it.
// next.defer_last_step: the pyramid's last step is left to the first kernel of the NEXT odometry_track_enqueue on this object
// (k_track_init_pyr), which the caller must enqueue on the same stream before anything else reads level 2 of lastDepth / lastImage
// next.fold: the set-up of the NEXT odometry_track_enqueue on this object (prior = the pose block fold->prior_pose16, the given
// so3 / pyramid / fastOdom switches) runs as a block group of the pyramid kernel; that call must follow on the same stream
// with the same arguments.  Taken only where the call's first launch is the resident SO3 level (which then carries the
// deferred pyramid step); otherwise ignored.
int odometry_initModel_fused(dms_odometry* o, const ModelSources& src, const ModelHandOver& next, hipStream_t s) {
  const int defer_last_step = next.defer_last_step;
  unsigned* const dense_cnt = next.dense_cnt;
  const TrackFold* const fold = next.fold;
  dms_image2d v[DMS_NUM_PYRS], n[DMS_NUM_PYRS], d[DMS_NUM_PYRS], im[DMS_NUM_PYRS];
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    v[i] = o->vmaps_g_prev[i].img();
    n[i] = o->nmaps_g_prev[i].img();
    d[i] = o->lastDepth[i].img();
    im[i] = o->lastImage[i].img();
  }
  // dense_cnt: the source choice comes from the 16 counters of the prediction's resolve pass instead of *src.use_b, which then
  // receives the decision; the next odometry_track_enqueue on this object zeroes the counters
  DMS_REQUIRE(!dense_cnt || defer_last_step, "dense counters are zeroed by the track call that takes the deferred pyramid step");
  TrackInitArgs ti;
  memset(&ti, 0, sizeof(ti));
  dms_odometry::NextCall nc;
  if (fold && fold->prior_pose16 && fold->so3 && !fold->interMap && defer_last_step && so3_resident_blocks(o) > 0)
    nc = fold_init_args(o, fold, &ti, dms_odometry::NextCall::folded);
  else if (defer_last_step)
    nc.kind = dms_odometry::NextCall::deferred_pyr;
  nc.dense_cnt_zero = dense_cnt;
  o->next_call = nc;
  ModelPyramidOpts opt;
  opt.skip_last_step = defer_last_step != 0;
  opt.dense_cnt = dense_cnt;
  opt.dense_samples = next.dense_samples;
  opt.flag_out = const_cast<int*>(src.use_b);
  if (nc.kind == dms_odometry::NextCall::folded) opt.init = &ti;
  ModelTargets dst;
  dst.vmaps = v;
  dst.nmaps = n;
  dst.depths = d;
  dst.images = im;
  dst.cutOff = o->maxDepthRGB;
  return modelPyramidFused(src, dst, opt, s);
}

// initICP(vertex map, normal map) + initRGB(image) of the live side in the fused form (RGBDOdometry.cpp:118-137,
// :162-191 through populateRGBDData): no transform, nextDepth from the same vertex map, then the Sobel / gate pyramid
int odometry_initLive_fused(dms_odometry* o, const ModelImages& live, const int* any_flag_dev, hipStream_t s) {
  dms_image2d v[DMS_NUM_PYRS], n[DMS_NUM_PYRS], d[DMS_NUM_PYRS], im[DMS_NUM_PYRS];
  for (int i = 0; i < DMS_NUM_PYRS; ++i) {
    v[i] = o->vmaps_curr[i].img();
    n[i] = o->nmaps_curr[i].img();
    d[i] = o->nextDepth[i].img();
    im[i] = o->nextImage[i].img();
  }
  ModelSources src;  // (one set: whatever the flag holds selects it)
  src.a = src.b = live;
  src.use_b = any_flag_dev;
  ModelTargets dst;
  dst.vmaps = v;
  dst.nmaps = n;
  dst.depths = d;
  dst.images = im;
  dst.cutOff = o->maxDepthRGB;
  int rc = modelPyramidFused(src, dst, ModelPyramidOpts{}, s);
  if (rc) return rc;
  return nextDerivatives(o, s);
}

}  // namespace dms

extern "C" {

int dms_odometry_initModelFused(dms_odometry* o, const void* vertA, const void* normA, const void* rgbaA, const void* vertB,
                                const void* normB, const void* rgbaB, const int* use_b_dev, int force_b_image,
                                const float* modelPose16_dev, dms_stream s) {
  DMS_REQUIRE(o, "null odometry");
  ModelSources src;
  src.a = {vertA, normA, rgbaA};
  src.b = {vertB, normB, rgbaB};
  src.use_b = use_b_dev;
  src.force_b_img = force_b_image;
  src.pose16 = modelPose16_dev;
  return odometry_initModel_fused(o, src, ModelHandOver{}, (hipStream_t)s);
}

int dms_odometry_fetch_result(dms_odometry* o, dms_track_result* r, dms_stream st) {
  DMS_REQUIRE(o && r, "null argument");
  DMS_HIP(hipMemcpyAsync(o->host_state, o->state, sizeof(TrackState), hipMemcpyDeviceToHost, (hipStream_t)st));
  DMS_HIP(hipStreamSynchronize((hipStream_t)st));
  o->clock.drain();
  const TrackState* h = o->host_state;
  memcpy(r->trans, h->out_trans, sizeof(r->trans));
  memcpy(r->rot, h->out_rot, sizeof(r->rot));
  r->lastICPError = h->lastICPError;
  r->lastICPCount = h->lastICPCount;
  r->lastRGBError = h->lastRGBError;
  r->lastRGBCount = h->lastRGBCount;
  r->lastSO3Error = h->lastSO3Error;
  r->lastSO3Count = h->lastSO3Count;
  memcpy(r->lastA, h->lastA, sizeof(r->lastA));
  memcpy(r->lastb, h->lastb, sizeof(r->lastb));
  for (int l = 0; l < DMS_NUM_PYRS; ++l) r->iterations_run[l] = h->iters_run[l];
  r->so3_iterations_run = h->so3_iters;
  r->rejected_jump = h->rejected_jump;
  if (h->sync_timeout) {
    if (h->sync_timeout == 1 && o->resident) {  // its blocks were not all resident: never again on this handle
      o->resident = false;
      o->fell_back = true;
    }
    if (h->sync_timeout == 2)
      set_error("dms_odometry_fetch_result: no fixed-point range found for a cross-pixel sum (the retry pool of a resident kernel is "
                "exhausted: non-finite input maps?)");
    else
      set_error("dms_odometry_fetch_result: a resident tracker kernel timed out at a grid-wide wait (its blocks were not all on the device: "
                "another process on this GPU?); this call's result is invalid and the handle has switched to DMS_TRACK_MODE=launches");
    return DMS_ERR_TIMEOUT;
  }
  return DMS_OK;
}

int dms_odometry_getIncrementalTransformation(dms_odometry* o, float* trans, float* rot, int rgbOnly, float icpWeight, int pyramid,
                                              int fastOdom, int so3, int interMap, dms_track_result* result, dms_stream s) {
  DMS_REQUIRE(o && trans && rot, "null argument");
  int rc = dms_odometry_track_async(o, trans, rot, rgbOnly, icpWeight, pyramid, fastOdom, so3, interMap, s);
  if (rc) return rc;
  dms_track_result local;
  dms_track_result* r = result ? result : &local;
  const bool was_resident = o->resident;
  rc = dms_odometry_fetch_result(o, r, s);
  // A resident launch has kArPool spare word sets for repeated reductions, all iterations of its level together: a limit of that
  // execution mode, not of the input.  An inter-map call (50 iterations per level on thumbnails, free to diverge) can use them up
  // where launch-per-phase - like the oracle - repeats each reduction up to canon::kMaxRetries times and then goes on with zero
  // sums.  Such a call is repeated launch-per-phase too; the handle stays resident.
  const bool pool_out = rc == DMS_ERR_TIMEOUT && was_resident && o->resident && o->host_state->sync_timeout == 2;
  if ((rc == DMS_ERR_TIMEOUT && was_resident && !o->resident) || pool_out) {
    // The resident kernels could not be co-resident: the same call again, launch-per-phase (the inputs are untouched; the
    // SO3 image swap of the first attempt, RGBDOdometry.cpp:595-601, is undone first).  Same bits as a resident run would give.
    if (so3)
      for (int i = 0; i < DMS_NUM_PYRS; i++) std::swap(o->lastNextImage[i], o->nextImage[i]);
    o->resident = false;
    rc = dms_odometry_track_async(o, trans, rot, rgbOnly, icpWeight, pyramid, fastOdom, so3, interMap, s);
    if (!rc) rc = dms_odometry_fetch_result(o, r, s);
    if (pool_out) o->resident = true;
  }
  if (rc) return rc;
  memcpy(trans, r->trans, 3 * sizeof(float));
  memcpy(rot, r->rot, 9 * sizeof(float));
  return DMS_OK;
}

int dms_odometry_getCovariance(dms_odometry* o, double* cov36) {
  DMS_REQUIRE(o && cov36, "null argument");
  // lastA.lu().inverse() (RGBDOdometry.cpp:607-610): Gauss-Jordan with partial pivoting
  double a[36], inv[36];
  memcpy(a, o->host_state->lastA, sizeof(a));
  for (int i = 0; i < 36; ++i) inv[i] = (i % 7 == 0) ? 1.0 : 0.0;
  for (int c = 0; c < 6; ++c) {
    int p = c;
    for (int r = c + 1; r < 6; ++r)
      if (fabs(a[r * 6 + c]) > fabs(a[p * 6 + c])) p = r;
    if (p != c)
      for (int j = 0; j < 6; ++j) {
        std::swap(a[c * 6 + j], a[p * 6 + j]);
        std::swap(inv[c * 6 + j], inv[p * 6 + j]);
      }
    const double d = a[c * 6 + c];
    for (int j = 0; j < 6; ++j) {
      a[c * 6 + j] /= d;
      inv[c * 6 + j] /= d;
    }
    for (int r = 0; r < 6; ++r) {
      if (r == c) continue;
      const double f = a[r * 6 + c];
      for (int j = 0; j < 6; ++j) {
        a[r * 6 + j] -= f * a[c * 6 + j];
        inv[r * 6 + j] -= f * inv[c * 6 + j];
      }
    }
  }
  memcpy(cov36, inv, sizeof(inv));
  return DMS_OK;
}

int dms_odometry_get_buffer(dms_odometry* o, int which, int level, dms_image2d* view) {
  DMS_REQUIRE(o && view, "null argument");
  DMS_REQUIRE(level >= 0 && level < DMS_NUM_PYRS, "bad level");
  const Buf* b = nullptr;
  switch (which) {
    case 0: b = &o->vmaps_curr[level]; break;
    case 1: b = &o->nmaps_curr[level]; break;
    case 2: b = &o->vmaps_g_prev[level]; break;
    case 3: b = &o->nmaps_g_prev[level]; break;
    case 4: b = &o->lastDepth[level]; break;
    case 5: b = &o->nextDepth[level]; break;
    case 6: b = &o->lastImage[level]; break;
    case 7: b = &o->nextImage[level]; break;
    case 8: b = &o->lastNextImage[level]; break;
    case 9: b = &o->nextdIdx[level]; break;
    case 10: b = &o->nextdIdy[level]; break;
    case 11: b = &o->pointClouds[level]; break;
    case 12: b = &o->depth_tmp[level]; break;
    case 13: b = &o->corresImg[level]; break;
    case 14: b = &o->nextGate[level]; break;
    default: DMS_REQUIRE(false, "bad buffer id");
  }
  *view = b->img();
  return DMS_OK;
}

int dms_odometry_set_profiling(dms_odometry* o, int enabled) {
  DMS_REQUIRE(o, "null argument");
  o->profiling = enabled != 0;
  o->profiling_level0_only = enabled == 2;
  if (enabled) {
    o->clock.drain();
    o->clock.times.clear();
    DMS_HIP(hipDeviceSynchronize());  // (the phase clocks are accumulated by the resident kernels)
    DMS_HIP(hipMemset(o->prof, 0, (3 * 16 + 256 * 8) * 8));
  }
  return DMS_OK;
}

int dms_odometry_get_kernel_time(dms_odometry* o, const char* name, double* total_ms, int* launches) {
  DMS_REQUIRE(o && name && total_ms && launches, "null argument");
  // "phase:<i>": accumulated in-kernel clock of phase i of the persistent level kernels (block 0)
  if (strncmp(name, "phase:", 6) == 0) {
    const int i = atoi(name + 6);  // level * 16 + phase
    DMS_REQUIRE(i >= 0 && i < 48 + 256 * 8, "bad phase index");  // from 48 on: per-block stamps [block][8] of level 0's middle iteration
    long long v = 0;
    DMS_HIP(hipMemcpy(&v, o->prof + i, sizeof(v), hipMemcpyDeviceToHost));
    *total_ms = i < 48 ? (double)v * 1e-5 : (double)(v % 100000000ll) * 1e-5;  // (counts: value * 1e-5)  // 10 ns ticks (stamps: modulo 1 s)
    *launches = 1;
    return DMS_OK;
  }
  {  // "<kernel>:median" / ":max" (ms) and ":slow" (launches = how many took more than 1.5 x the median)
    const char* colon = strchr(name, ':');
    if (colon) {
      auto it2 = o->clock.times.find(std::string(name, colon - name));
      *total_ms = 0;
      *launches = 0;
      if (it2 == o->clock.times.end() || it2->second.samples.empty()) return DMS_OK;
      std::vector<float> v = it2->second.samples;
      std::sort(v.begin(), v.end());
      const float med = v[v.size() / 2];
      if (strcmp(colon, ":median") == 0) *total_ms = med;
      else if (strcmp(colon, ":max") == 0) *total_ms = v.back();
      else if (strcmp(colon, ":slow") == 0) {
        int n = 0;
        double extra = 0;
        for (float x : v)
          if (x > 1.5f * med) {
            ++n;
            extra += x - med;
          }
        *launches = n;
        *total_ms = extra;  // what the slow launches took beyond the median, summed
      } else DMS_REQUIRE(false, "unknown suffix");
      if (strcmp(colon, ":slow") != 0) *launches = (int)v.size();
      return DMS_OK;
    }
  }
  auto it = o->clock.times.find(name);
  if (it == o->clock.times.end()) {
    *total_ms = 0;
    *launches = 0;
    return DMS_OK;
  }
  *total_ms = it->second.ms;
  *launches = it->second.launches;
  return DMS_OK;
}

}  // extern "C"
