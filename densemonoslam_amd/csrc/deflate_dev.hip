// zlib streams made on the device (include/dmslam_io_write.h).  The format and every decision are csrc/deflate_core.hpp, which the
// host's dms_deflate_blocks compiles too (csrc/deflate.hpp): the bytes are the same.  One workgroup per block of kBlock input bytes:
//
//   k_dfl_match     hash table of the 32 KB before the block and of the block (LDS, atomicMax: the latest position wins whatever the
//                   order), a candidate per position, the longest of three matches per position, then the parse: every position's
//                   successor, the positions on the path from 0 by pointer doubling, the tokens in order by a block scan.  Tokens go
//                   to the scratch buffer, the two histograms (LDS atomics on integers) and the block's Adler sums to its record
//   k_dfl_codes     the three length-limited codes, the header's length, the byte length of the block as each kind, the choice
//   k_scan_blocks   exclusive sums of the byte lengths (csrc/scan.hpp) and the total
//   k_dfl_write     every block writes its bytes at its offset (blocks start and end on bytes: plain stores, nothing is shared);
//                   the last block appends the Adler-32 combined from the records and stores the stream's length
//   copies          length word and the first bytes of the stream -> pinned slot (the rest, if the stream is longer, when the result
//                   is asked for)
// No kernel waits on another workgroup; everything is enqueued on the caller's stream.
#include "deflate_dev.hpp"

#include <string.h>

#include <vector>

#include "common.hpp"
#include "scan.hpp"

namespace {

using namespace dms::dfl;

constexpr int kMatchThreads = 256, kPerThread = (int)(kBlock / kMatchThreads);
static_assert(kChunk == 64, "a chunk is what one wave looks up at once");
static_assert(kBlock % (4 * kChunk) == 0 && kBlock / kMatchThreads == 16, "k_dfl_match: 16 positions a thread, four waves take turns");
static_assert(sizeof(BlockInfo) % 16 == 0, "copied as 16-byte words");

__global__ __launch_bounds__(kMatchThreads) void k_dfl_match(const unsigned char* __restrict__ data, uint32_t len, uint32_t* __restrict__ tokens,
                                                             BlockInfo* __restrict__ info) {
  __shared__ uint32_t s_head[1 << kHashBits];  // position - w0 + 1 of the latest entry; later the parse's successor and path arrays
  __shared__ uint32_t s_best[kBlock];          // the hash table's candidate, then the match, of each position
  __shared__ uint32_t s_hist[kLLSlots + kDSlots];
  __shared__ uint32_t s_sum[2], s_wave[kMatchThreads / 64];
  const uint32_t blk = blockIdx.x, s = blk * kBlock, e = len - s < kBlock ? len : s + kBlock, n = e - s, w0 = window_start(s);
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (uint32_t i = t; i < (1u << kHashBits); i += kMatchThreads) s_head[i] = 0;
  for (uint32_t i = t; i < (uint32_t)(kLLSlots + kDSlots); i += kMatchThreads) s_hist[i] = 0;
  if (t < 2) s_sum[t] = 0;
  __syncthreads();
  for (uint32_t p = w0 + t; p < s; p += kMatchThreads)
    if (hashable(p, len)) atomicMax(&s_head[hash4(data + p)], p - w0 + 1);
  // the block's own positions, a chunk of 64 at a time: the chunk's wave reads the table for all its positions, then enters them
  uint32_t hh[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const uint32_t i = s + ((uint32_t)k * 4 + wave) * kChunk + lane;
    hh[k] = i < e && hashable(i, len) ? hash4(data + i) : 0xffffffffu;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (q == wave) {
        const uint32_t j = ((uint32_t)k * 4 + wave) * kChunk + lane, i = s + j;
        if (i < e) {
          uint32_t from = i;
          if (hh[k] != 0xffffffffu) {
            const uint32_t v = s_head[hh[k]];
            if (v) from = v - 1 + w0;
            atomicMax(&s_head[hh[k]], i - w0 + 1);
          }
          s_best[j] = from;
        }
      }
      __syncthreads();
    }
  }
  // matches, and the block's Adler sums
  uint32_t a = 0, b = 0;
  for (uint32_t j = t; j < n; j += kMatchThreads) {
    s_best[j] = best_at(data, e, s + j, s_best[j]);
    const uint32_t x = data[s + j];
    a += x;
    b += (n - j) * x;
  }
  atomicAdd(&s_sum[0], a % kAdlerMod);
  atomicAdd(&s_sum[1], b % kAdlerMod);
  __syncthreads();
  // the parse: next[j], then the positions on the path 0, next[0], next[next[0]], ... by doubling the stride of the jumps
  uint16_t* s_jump = reinterpret_cast<uint16_t*>(s_head);  // [kBlock + 1]; n = behind the block
  uint32_t* s_on = s_head + kBlock / 2 + 64;               // [kBlock]
  static_assert((1u << kHashBits) >= kBlock / 2 + 64 + kBlock, "the parse's arrays take the hash table's place");
  for (uint32_t j = t; j < n; j += kMatchThreads) {
    s_jump[j] = (uint16_t)(j + parse_step(s_best, j, n));
    s_on[j] = j == 0;
  }
  if (t == 0) s_jump[n] = (uint16_t)n;
  __syncthreads();
  for (uint32_t stride = 1; stride < n; stride <<= 1) {
    uint32_t to[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const uint32_t j = t + (uint32_t)k * kMatchThreads;
      to[k] = n;
      if (j < n) {
        const uint32_t x = s_jump[j];
        to[k] = s_jump[x];
        if (s_on[j] && x < n) s_on[x] = 1;  // every writer writes 1
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const uint32_t j = t + (uint32_t)k * kMatchThreads;
      if (j < n) s_jump[j] = (uint16_t)to[k];
    }
    __syncthreads();
  }
  // tokens in order: thread t owns positions 16 t .. 16 t + 15
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const uint32_t j = t * kPerThread + (uint32_t)k;
    mine += j < n && s_on[j];
  }
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off, 64);
    if ((int)lane >= off) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t at = incl - mine, total = 0;
  for (uint32_t w = 0; w < kMatchThreads / 64; ++w) {
    if (w < wave) at += s_wave[w];
    total += s_wave[w];
  }
  uint32_t* tok = tokens + (size_t)blk * kBlock;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const uint32_t j = t * kPerThread + (uint32_t)k;
    if (j < n && s_on[j]) {
      const uint32_t m = parse_step(s_best, j, n) > 1 ? s_best[j] : 0;
      int sym, nb;
      uint32_t ex;
      if (m) {
        length_symbol(match_length(m), &sym, &nb, &ex);
        atomicAdd(&s_hist[sym], 1u);
        dist_symbol(match_dist(m), &sym, &nb, &ex);
        atomicAdd(&s_hist[kLLSlots + sym], 1u);
        tok[at++] = kMatchFlag | m;
      } else {
        const uint32_t x = data[s + j];
        atomicAdd(&s_hist[x], 1u);
        tok[at++] = x;
      }
    }
  }
  if (t == 0) s_hist[256] = 1;
  __syncthreads();
  BlockInfo& bi = info[blk];
  for (uint32_t i = t; i < (uint32_t)kLLSlots; i += kMatchThreads) bi.hist_ll[i] = s_hist[i];
  if (t < (uint32_t)kDSlots) bi.hist_d[t] = s_hist[kLLSlots + t];
  if (t == 0) {
    bi.ntok = total;
    bi.adler_a = s_sum[0] % kAdlerMod;
    bi.adler_b = s_sum[1] % kAdlerMod;
  }
}

constexpr int kCodesThreads = 320;
__global__ __launch_bounds__(kCodesThreads) void k_dfl_codes(BlockInfo* __restrict__ info, uint32_t len, uint32_t nblocks, uint32_t* __restrict__ sizes) {
  __shared__ BlockInfo s_b;
  __shared__ CodeWork s_w;
  __shared__ uint32_t s_cl[kNumCL];
  const uint32_t blk = blockIdx.x, t = threadIdx.x;
  const bool last = blk + 1 == nblocks;
  const uint32_t n = last ? len - blk * kBlock : kBlock;
  uint4* dst = reinterpret_cast<uint4*>(&s_b);
  uint4* src = reinterpret_cast<uint4*>(&info[blk]);
  for (uint32_t i = t; i < sizeof(BlockInfo) / 16; i += kCodesThreads) dst[i] = src[i];
  __syncthreads();
  if (t < (uint32_t)kNumLL && s_b.hist_ll[t]) s_w.order[symbol_rank(s_b.hist_ll, kNumLL, (int)t)] = (uint16_t)t;
  __syncthreads();
  if (t == 0) {
    build_lengths(s_b.hist_ll, kNumLL, kLimitLL, false, s_b.len_ll, &s_w);
    choose_block(&s_b, n, last, &s_w, s_cl);
    sizes[blk] = s_b.bytes;
  }
  __syncthreads();
  for (uint32_t i = t; i < sizeof(BlockInfo) / 16; i += kCodesThreads) src[i] = dst[i];
}

struct DevSink {
  unsigned char* out;
  __device__ __forceinline__ void store(uint32_t i, unsigned char v) { out[i] = v; }
};

__global__ __launch_bounds__(64) void k_dfl_write(const unsigned char* __restrict__ data, uint32_t len, uint32_t nblocks, const uint32_t* __restrict__ tokens,
                                                  const BlockInfo* __restrict__ info, const uint32_t* __restrict__ offsets, unsigned char* __restrict__ out,
                                                  uint32_t* __restrict__ out_len) {
  __shared__ BlockCodes s_c;
  __shared__ BlockInfo s_b;
  const uint32_t blk = blockIdx.x, t = threadIdx.x;
  const bool last = blk + 1 == nblocks;
  const uint32_t n = last ? len - blk * kBlock : kBlock;
  uint4* dst = reinterpret_cast<uint4*>(&s_b);
  const uint4* src = reinterpret_cast<const uint4*>(&info[blk]);
  for (uint32_t i = t; i < sizeof(BlockInfo) / 16; i += 64) dst[i] = src[i];
  __syncthreads();
  if (t != 0) return;
  DevSink sink{out};
  if (blk == 0) {
    sink.store(0, kZlibHeader0);
    sink.store(1, kZlibHeader1);
  }
  block_codes(s_b, &s_c);
  uint32_t at = emit_block(s_b, s_c, data + (size_t)blk * kBlock, n, tokens + (size_t)blk * kBlock, last, 2 + offsets[blk], sink);
  if (last) out_len[0] = emit_trailer(info, nblocks, len, at, sink);
}

constexpr size_t kLenBytes = 16;  // the length word in front of the device's stream and of the slot's copy
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct Slot {
  unsigned char* pinned = nullptr;  // [length word | stream]
  unsigned char* d_out = nullptr;   // [length word | stream]
  hipEvent_t done = nullptr;
  bool in_flight = false, used = false, finished = false;
  size_t len = 0, eager = 0;
};

}  // namespace

struct dms_deflate_dev {
  size_t max_len = 0;
  std::vector<Slot> slots;
  int next = 0;
  uint32_t* d_tokens = nullptr;
  BlockInfo* d_info = nullptr;
  uint32_t* d_sizes = nullptr;  // [byte lengths | offsets | total]
  hipEvent_t last_done = nullptr;
  hipStream_t last_stream = nullptr;
  bool any = false;
};

namespace {

int free_all(dms_deflate_dev* dd) {
  for (Slot& s : dd->slots) {
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.pinned) (void)hipHostFree(s.pinned);
    if (s.d_out) (void)hipFree(s.d_out);
  }
  if (dd->last_done) (void)hipEventDestroy(dd->last_done);
  void* dev[] = {dd->d_tokens, dd->d_info, dd->d_sizes};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  delete dd;
  return DMS_OK;
}

}  // namespace

namespace dms {
namespace dfl {

size_t dev_slot_bytes(size_t len) { return kLenBytes + align16(stream_bound(len)); }

int dev_enqueue(dms_deflate_dev* dd, int index, const void* data_dev, size_t len, hipStream_t stream, unsigned char* pinned, size_t* eager) {
  Slot& s = dd->slots[(size_t)index];
  // the device buffers are one set: an encode on another stream waits for the one before
  if (dd->any && dd->last_stream != stream) DMS_HIP(hipStreamWaitEvent(stream, dd->last_done, 0));
  const uint32_t nb = num_blocks(len), n32 = (uint32_t)len;
  uint32_t* offsets = dd->d_sizes + num_blocks(dd->max_len);
  uint32_t* total = offsets + num_blocks(dd->max_len);
  const unsigned char* src = (const unsigned char*)data_dev;
  hipLaunchKernelGGL(k_dfl_match, dim3(nb), dim3(kMatchThreads), 0, stream, src, n32, dd->d_tokens, dd->d_info);
  hipLaunchKernelGGL(k_dfl_codes, dim3(nb), dim3(kCodesThreads), 0, stream, dd->d_info, n32, nb, dd->d_sizes);
  hipLaunchKernelGGL(dms::k_scan_blocks, dim3(1), dim3(1024), 0, stream, dd->d_sizes, offsets, (int)nb, total, 0xffffffffu, (unsigned*)nullptr);
  hipLaunchKernelGGL(k_dfl_write, dim3(nb), dim3(64), 0, stream, src, n32, nb, dd->d_tokens, dd->d_info, offsets, s.d_out + kLenBytes,
                     reinterpret_cast<uint32_t*>(s.d_out));
  DMS_CHECK_LAUNCH();
  // the length and what input of this size usually needs; a longer stream's rest is copied when the result is asked for
  const size_t worst = stream_bound(len), usual = len / 2 > 65536 ? len / 2 : 65536;
  *eager = worst < usual ? worst : usual;
  DMS_HIP(hipMemcpyAsync(pinned, s.d_out, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  DMS_HIP(hipMemcpyAsync(pinned + kLenBytes, s.d_out + kLenBytes, *eager, hipMemcpyDeviceToHost, stream));
  DMS_HIP(hipEventRecord(dd->last_done, stream));
  dd->last_stream = stream;
  dd->any = true;
  return DMS_OK;
}

int dev_finish(dms_deflate_dev* dd, int index, unsigned char* pinned, size_t eager, const unsigned char** data, size_t* len) {
  Slot& s = dd->slots[(size_t)index];
  uint32_t n;
  memcpy(&n, pinned, sizeof(n));
  if ((size_t)n > eager) DMS_HIP(hipMemcpy(pinned + kLenBytes + eager, s.d_out + kLenBytes + eager, (size_t)n - eager, hipMemcpyDeviceToHost));
  *data = pinned + kLenBytes;
  *len = n;
  return DMS_OK;
}

}  // namespace dfl
}  // namespace dms

extern "C" {

int dms_deflate_dev_create(dms_deflate_dev** out, size_t max_len, int slots) {
  DMS_REQUIRE(out, "null argument");
  DMS_REQUIRE(max_len >= 1 && max_len <= ((size_t)1 << 31), "max_len outside 1 .. 2^31: offsets are 32-bit");
  DMS_REQUIRE(slots >= 1 && slots <= 16, "slots outside 1 .. 16");
  dms_deflate_dev* dd = new dms_deflate_dev();
  dd->max_len = max_len;
  dd->slots.resize((size_t)slots);
  const size_t nb = num_blocks(max_len);
  auto fail = [&](hipError_t e, const char* what) {
    free_all(dd);
    return dms::hip_fail(e, what, __FILE__, __LINE__);
  };
  hipError_t e;
  for (Slot& s : dd->slots) {
    if ((e = hipHostMalloc((void**)&s.pinned, dms::dfl::dev_slot_bytes(max_len), hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc");
    if ((e = hipMalloc((void**)&s.d_out, dms::dfl::dev_slot_bytes(max_len))) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  }
  if ((e = hipEventCreateWithFlags(&dd->last_done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipMalloc((void**)&dd->d_tokens, nb * kBlock * sizeof(uint32_t))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&dd->d_info, nb * sizeof(BlockInfo))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&dd->d_sizes, (2 * nb + 4) * sizeof(uint32_t))) != hipSuccess) return fail(e, "hipMalloc");
  *out = dd;
  return DMS_OK;
}

int dms_deflate_dev_destroy(dms_deflate_dev* dd) {
  if (!dd) return DMS_OK;
  if (dd->any) (void)hipEventSynchronize(dd->last_done);
  return free_all(dd);
}

int dms_deflate_dev_encode(dms_deflate_dev* dd, const void* data_dev, size_t len, dms_stream stream) {
  DMS_REQUIRE(dd && data_dev, "null argument");
  DMS_REQUIRE(len >= 1 && len <= dd->max_len, "len is 0 or above the max_len the object was created for");
  const int index = dd->next;
  Slot& s = dd->slots[(size_t)index];
  if (s.in_flight) {
    DMS_HIP(hipEventSynchronize(s.done));
    s.in_flight = false;
  }
  dd->next = (dd->next + 1) % (int)dd->slots.size();
  s.used = true;
  s.finished = false;
  s.len = 0;
  const int rc = dms::dfl::dev_enqueue(dd, index, data_dev, len, (hipStream_t)stream, s.pinned, &s.eager);
  DMS_HIP(hipEventRecord(s.done, (hipStream_t)stream));
  s.in_flight = true;
  return rc;
}

int dms_deflate_dev_result_at(dms_deflate_dev* dd, int back, const unsigned char** data, size_t* len) {
  DMS_REQUIRE(dd && data && len, "null argument");
  const int n = (int)dd->slots.size();
  DMS_REQUIRE(back >= 0 && back < n, "further back than the ring has slots");
  const int index = ((dd->next - 1 - back) % n + n) % n;
  Slot& s = dd->slots[(size_t)index];
  DMS_REQUIRE(s.used, "no encode in that slot");
  if (s.in_flight) {
    DMS_HIP(hipEventSynchronize(s.done));
    s.in_flight = false;
  }
  if (!s.finished) {
    const unsigned char* p;
    const int rc = dms::dfl::dev_finish(dd, index, s.pinned, s.eager, &p, &s.len);
    if (rc) return rc;
    s.finished = true;
  }
  *data = s.pinned + kLenBytes;
  *len = s.len;
  return DMS_OK;
}

int dms_deflate_dev_result(dms_deflate_dev* dd, const unsigned char** data, size_t* len) { return dms_deflate_dev_result_at(dd, 0, data, len); }

}  // extern "C"
