// Which pixels a thread of the resident Gauss-Newton level kernel (track.hip k_gn_level) owns.  One mapping for the kernel: the ICP
// half and the photometric gate test both use it.  Plain code for host and device: tests/test_track_ownership_cpu.py compiles this
// header alone.
//
// A block of kPB threads = kOwnWaves waves evaluates P pixels per thread in P "slots"; every (slot, wave) pair owns one SEGMENT of
// 64 consecutive pixels, lane l the l-th of them, so a wave's own-data loads stay coalesced.
//   contiguous:  block b owns the P * kOwnWaves segments b * P * kOwnWaves + p * kOwnWaves + w, i.e. P * kPB adjacent pixels;
//   interleaved: wave w of slot p of block b owns segment (p * kOwnWaves + w) * nb + b: the segments of one block lie nb apart,
//                spread over the whole image, so that no block owns all of an edge band (its photometric list would be the longest
//                of the grid, and the longest list sets the pace of every iteration).
// Both are bijections from (block, slot, thread) onto [0, nb * P * kPB), which covers the level's N pixels; an index >= N is a lane
// past the end of the image: it shadows pixel index % N (distinct addresses, see gn_level_body) and is masked.
// The sums of the tracker are exact integer sums (canon.hpp): which lane evaluates a pixel cannot change a bit of them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMS_OWN_HD __host__ __device__ __forceinline__
#else
#define DMS_OWN_HD inline
#endif

namespace dms {

constexpr int kOwnLanes = 64;       // lanes of a wave = pixels of a segment
constexpr int kOwnWaves = 512 / 64;  // waves of a block (kPB / 64, checked in track.hip)

// pixel index (possibly >= N: masked, see owned_shadow) of thread `tid` of block `b` of `nb`, slot p of P
DMS_OWN_HD int owned_index(bool interleave, int b, int nb, int P, int p, int tid) {
  const int w = tid / kOwnLanes, lane = tid % kOwnLanes;
  const int seg = interleave ? (p * kOwnWaves + w) * nb + b : (b * P + p) * kOwnWaves + w;
  return seg * kOwnLanes + lane;
}

// the pixel a thread loads for index idx: its own, or the one a masked lane shadows
DMS_OWN_HD int owned_shadow(int idx, int N) { return idx < N ? idx : idx % N; }

}  // namespace dms
