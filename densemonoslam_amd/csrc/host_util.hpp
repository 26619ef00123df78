// Host-only helpers the object layers share: the 256-byte rounding of their arenas, the carver that lays an arena out, and the
// event-pair stage clock behind dms_odometry_get_kernel_time / dms_fusion_get_kernel_time.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <map>
#include <string>
#include <vector>

namespace dms {

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// Lays blocks out in an arena, each at a 256-byte boundary and followed by `pad` spare bytes.  Run once without a base for the
// size (up256(off)), then again over the allocation: the same calls give the same offsets.
struct Carver {
  char* base = nullptr;
  size_t off = 0;
  size_t pad = 0;
  size_t reserve(size_t bytes) {  // the block's offset
    off = up256(off);
    const size_t at = off;
    off += bytes + pad;
    return at;
  }
  void* take(size_t bytes) {
    const size_t at = reserve(bytes);
    return base ? base + at : nullptr;
  }
  template <typename T>
  T* take(size_t n) {
    return (T*)take(n * sizeof(T));
  }
};

// Stage times of one handle: a StageTimer brackets what is enqueued within its scope with two events; drain() - called once the
// stream has been synchronised - turns the recorded pairs into per-name totals and returns the events to the pool.
struct StageClock {
  struct Total {
    double ms = 0;
    int launches = 0;
    std::vector<float> samples;  // per launch, ms ("<name>:slow" / ":max" / ":median" of dms_odometry_get_kernel_time)
  };
  struct Pending {
    std::string name;
    hipEvent_t start, stop;
  };
  std::map<std::string, Total> times;
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;

  StageClock() = default;
  StageClock(const StageClock&) = delete;
  ~StageClock() {
    for (auto& p : pending) pool.insert(pool.end(), {p.start, p.stop});
    for (auto e : pool) (void)hipEventDestroy(e);
  }
  hipEvent_t get() {
    hipEvent_t e;
    if (pool.empty()) {
      (void)hipEventCreate(&e);
    } else {
      e = pool.back();
      pool.pop_back();
    }
    return e;
  }
  void drain() {
    for (auto& p : pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
        Total& t = times[p.name];
        t.ms += ms;
        t.launches += 1;
        if (t.samples.size() < 100000) t.samples.push_back(ms);
      }
      pool.insert(pool.end(), {p.start, p.stop});
    }
    pending.clear();
  }
};

struct StageTimer {
  StageClock* clock;  // nullptr: not timed
  hipStream_t s;
  const char* name;
  hipEvent_t a = nullptr, b = nullptr;
  StageTimer(StageClock& c, hipStream_t s_, const char* n, bool enabled) : clock(enabled ? &c : nullptr), s(s_), name(n) {
    if (!clock) return;
    a = clock->get();
    b = clock->get();
    (void)hipEventRecord(a, s);
  }
  ~StageTimer() {
    if (!clock) return;
    (void)hipEventRecord(b, s);
    clock->pending.push_back({name, a, b});
  }
  StageTimer(const StageTimer&) = delete;
};

}  // namespace dms
