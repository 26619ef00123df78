// JPEG colour decoded on the device (include/dmslam_io_device.h).  The arithmetic is csrc/jpeg_core.hpp, the one the host's
// sequential decoder (csrc/jpeg.hpp) compiles; tests/jpeg_lanes_host.cpp runs the entropy passes below with the lanes one after
// another on the host.
//
//   host     parse (markers, tables, geometry), byte scan for the restart markers, lane table; one copy of
//            [tables | segments | lanes | entropy-coded bytes] into a pinned slot, one H2D copy of it
//   device   k_sync_round x kSyncRounds   speculative decode and relaxation: one lane per subsequence; a round returns at once
//                                         when the round before changed no exit state
//            k_settle                     the single-lane pass, one lane per segment, only where the last round still changed a state
//            k_block_offsets              exclusive sums of the lanes' block ends, per segment
//            k_write                      every lane decodes once more and writes coefficients (DC: the difference)
//            k_dc_sums                    segmented inclusive sums of the DC differences, per component
//            k_idct                       coefficients -> component planes, 8 lanes per block
//            k_colour                     upsampling + colour conversion -> interleaved RGB8, 4 pixels (3 dwords) per thread
// No kernel waits on another workgroup; the host reads nothing back unless dms_jpeg_dev_status is called.
#include <string.h>

#include <vector>

#include "../../include/dmslam_io_device.h"
#include "common.hpp"
#include "jpeg.hpp"
#include "jpeg_dev.hpp"

namespace {

using namespace dms::jpeg;

static_assert(kSyncRounds == DMS_JPEG_DEV_ROUNDS, "the header names the number of rounds");

// what the entropy kernels keep in LDS besides the wave's slice of the stream
struct alignas(16) LaneTables {
  Geometry g;
  Huff dc[3], ac[3];  // by component
};
static_assert(sizeof(LaneTables) % 16 == 0, "copied as 16-byte words");

struct DevStatus {
  uint32_t changed[kSyncRounds];  // round r changed an exit state
  uint32_t err_key;               // CoefSink's key of the first refusal, kNoBlockError = none
  uint32_t settled;               // lanes the single-lane pass re-decoded
  uint32_t pad[2];
};

// the back half's parameters travel as a kernel argument
struct BackParams {
  Geometry g;
  unsigned short qt[3][64];
  int flip;
};

constexpr int kLaneBlock = 64;     // one wave: its lanes' subsequences are one contiguous slice of the stream
constexpr int kSliceSlack = 256;   // markers between short segments, look-ahead of the last lane
constexpr size_t kStreamPad = 64;  // the slice is copied in 16-byte words

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t lane_lds_bytes(int S) { return sizeof(LaneTables) + (size_t)kLaneBlock * S + kSliceSlack; }

// which of the two record buffers the last round that ran wrote
__device__ __forceinline__ int final_buffer(const DevStatus* st) {
  int last = 0;
  for (int r = 1; r < kSyncRounds; ++r) {
    if (!st->changed[r - 1]) break;
    last = r;
  }
  return last & 1;
}

// tables -> LDS, the slice of the stream the block's lanes read -> LDS, both with coalesced 16-byte loads
__device__ __forceinline__ ScanView stage_lanes(const LaneTables* tables, const SegInfo* segs, const LaneInfo* lanes, int nlanes,
                                                const unsigned char* stream, uint32_t stream_len, int S, unsigned char* lds) {
  const int nt = blockDim.x;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tables);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (int i = threadIdx.x; i < (int)(sizeof(LaneTables) / 16); i += nt) dst[i] = src[i];
  }
  unsigned char* slice = lds + sizeof(LaneTables);
  const int first = blockIdx.x * nt, last = min(first + nt, nlanes) - 1;
  const uint32_t cap = (uint32_t)(nt * S + kSliceSlack);
  uint32_t lo = lanes[first].first_byte, hi = lanes[last].stop_byte + 32;
  lo = lo > 0 ? (lo - 1) & ~15u : 0;
  if (hi > stream_len) hi = stream_len;
  uint32_t n = hi > lo ? hi - lo : 0;
  if (n > cap) n = 0;  // (junk between segments): the lanes read global memory instead
  {
    // the stream buffer is padded by kStreamPad bytes, so the last 16-byte word may run past stream_len
    const uint4* src = reinterpret_cast<const uint4*>(stream + lo);
    uint4* dst = reinterpret_cast<uint4*>(slice);
    for (uint32_t i = threadIdx.x; i < (n + 15) / 16; i += nt) dst[i] = src[i];  // n <= cap, a multiple of 16
  }
  __syncthreads();
  const LaneTables* t = reinterpret_cast<const LaneTables*>(lds);
  ScanView sc;
  sc.mem = stream;
  sc.win = slice;
  sc.win_lo = lo;
  sc.win_n = n;
  sc.dc = t->dc;
  sc.ac = t->ac;
  sc.g = &t->g;
  sc.segs = segs;
  sc.lanes = lanes;
  return sc;
}

__global__ __launch_bounds__(kLaneBlock) void k_sync_round(const LaneTables* tables, const SegInfo* segs, const LaneInfo* lanes, int nlanes,
                                                           const unsigned char* stream, uint32_t stream_len, int S, int round,
                                                           LaneRecord* rec0, LaneRecord* rec1, DevStatus* st, unsigned char* dirty) {
  if (round > 0 && !st->changed[round - 1]) return;  // converged (or never started): uniform over the grid
  extern __shared__ uint4 lds16[];
  const ScanView sc = stage_lanes(tables, segs, lanes, nlanes, stream, stream_len, S, reinterpret_cast<unsigned char*>(lds16));
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nlanes) return;
  LaneRecord* cur = (round & 1) ? rec1 : rec0;
  const LaneRecord* prev = (round & 1) ? rec0 : rec1;
  const LaneRecord r = sync_lane(sc, lane, round, prev);
  const bool changed = round == 0 ? !(lanes[lane].flags & kLaneFirst) : !same_exit(r, prev[lane]);
  cur[lane] = r;  // a lane writes nothing but its own record (and the two flags below)
  if (changed) {
    st->changed[round] = 1;
    if (round == kSyncRounds - 1) dirty[lanes[lane].seg] = 1;
  }
}

__global__ __launch_bounds__(kLaneBlock) void k_settle(const LaneTables* tables, const SegInfo* segs, const LaneInfo* lanes, int nlanes, int nseg,
                                                       const unsigned char* stream, LaneRecord* rec0, LaneRecord* rec1, DevStatus* st,
                                                       const unsigned char* dirty) {
  if (!st->changed[kSyncRounds - 1]) return;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg || !dirty[s]) return;
  ScanView sc;
  sc.mem = stream;
  sc.win = nullptr;
  sc.win_lo = 0;
  sc.win_n = 0;
  sc.dc = tables->dc;
  sc.ac = tables->ac;
  sc.g = &tables->g;
  sc.segs = segs;
  sc.lanes = lanes;
  const int first = (int)segs[s].first_lane;
  const int n = (s + 1 < nseg ? (int)segs[s + 1].first_lane : nlanes) - first;
  const int done = settle_segment(sc, first, n, final_buffer(st) ? rec1 : rec0);
  if (done) atomicAdd(&st->settled, (uint32_t)done);
}

// block_in_segment[lane] = sum of the block ends of the segment's lanes before it.  One block scans all lanes in chunks of 1024
// (exclusive sums over ALL lanes into `running`), then takes each lane's sum relative to its segment's first lane.
__global__ __launch_bounds__(1024) void k_block_offsets(const SegInfo* segs, const LaneInfo* lanes, int nlanes, const LaneRecord* rec0,
                                                        const LaneRecord* rec1, const DevStatus* st, uint32_t* running,
                                                        uint32_t* block_in_segment) {
  __shared__ uint32_t s_scan[1024];
  __shared__ uint32_t s_carry;
  const LaneRecord* rec = final_buffer(st) ? rec1 : rec0;
  const int t = threadIdx.x;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < nlanes; base += 1024) {
    const int lane = base + t;
    const uint32_t v = lane < nlanes ? record_ends(rec[lane]) : 0;
    s_scan[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const uint32_t a = t >= d ? s_scan[t - d] : 0;
      __syncthreads();
      s_scan[t] += a;
      __syncthreads();
    }
    const uint32_t carry = s_carry;
    if (lane < nlanes) running[lane] = carry + s_scan[t] - v;
    __syncthreads();
    if (t == 1023) s_carry = carry + s_scan[1023];
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  for (int lane = t; lane < nlanes; lane += 1024) block_in_segment[lane] = running[lane] - running[segs[lanes[lane].seg].first_lane];
}

__global__ __launch_bounds__(kLaneBlock) void k_write(const LaneTables* tables, const SegInfo* segs, const LaneInfo* lanes, int nlanes,
                                                      const unsigned char* stream, uint32_t stream_len, int S, const LaneRecord* rec0,
                                                      const LaneRecord* rec1, DevStatus* st, const uint32_t* block_in_segment, short* coefs) {
  extern __shared__ uint4 lds16[];
  const ScanView sc = stage_lanes(tables, segs, lanes, nlanes, stream, stream_len, S, reinterpret_cast<unsigned char*>(lds16));
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nlanes) return;
  write_lane(sc, lane, final_buffer(st) ? rec1 : rec0, block_in_segment[lane], coefs, &st->err_key);
}

// DC differences -> DC values: inclusive sums over the blocks of one component in the scan's order, starting again at every
// restart interval.  One block per component; chunks of 1024 blocks with a carry.
__global__ __launch_bounds__(1024) void k_dc_sums(Geometry g, short* coefs) {
  __shared__ int s_v[1024];
  __shared__ int s_f[1024];
  __shared__ int s_carry;
  const int c = blockIdx.x, t = threadIdx.x;
  const int hv = g.h[c] * g.v[c];
  const int n = g.mcux * g.mcuy * hv;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int e = base + t;
    const int mcu = e / hv, j = e - mcu * hv;
    const size_t at = ((size_t)mcu * g.blocks_per_mcu + g.off[c] + j) * 64;
    const bool in = e < n;
    int v = in ? (int)coefs[at] : 0;
    int f = in && j == 0 && (g.restart_interval ? mcu % g.restart_interval == 0 : mcu == 0) ? 1 : 0;
    s_v[t] = v;
    s_f[t] = f;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      int av = 0, af = 0;
      if (t >= d) {
        av = s_v[t - d];
        af = s_f[t - d];
      }
      __syncthreads();
      if (t >= d && !s_f[t]) {
        s_v[t] += av;
        s_f[t] = af;
      }
      __syncthreads();
    }
    const int sum = s_v[t] + (s_f[t] ? 0 : s_carry);
    if (in) coefs[at] = (short)sum;
    __syncthreads();
    if (t == 1023) s_carry = sum;
    __syncthreads();
  }
}

// Inverse DCT: 256 threads take 32 blocks that follow one another in a component's plane (so a row of the planes is written by
// neighbouring lanes), 8 lanes per block.  Three phases with LDS in between, which is also the transposition:
//   A  thread (block b, row r) loads the 8 coefficients of one block row (16 bytes, coalesced over the block) and dequantises
//   B  thread (block b, column c) runs the column pass
//   C  thread (row r, block b) runs the row pass and stores the 8 samples of one block row (8 bytes; the 32 lanes of a row are
//      contiguous in the plane where the blocks are)
constexpr int kIdctBlocks = 32;
__global__ __launch_bounds__(256) void k_idct(BackParams p, const short* coefs, unsigned char* planes) {
  __shared__ int s_d[kIdctBlocks][72];            // dequantised coefficients, [block][r * 8 + c] (+8: the column reads spread over banks)
  __shared__ int64_t s_w[8][kIdctBlocks][8];      // workspace, [r][block][c]
  __shared__ int s_comp[kIdctBlocks], s_bx[kIdctBlocks], s_by[kIdctBlocks];
  const Geometry& g = p.g;
  const int t = threadIdx.x;
  const int n0 = g.bw[0] * g.bh[0], n1 = g.bw[1] * g.bh[1], total = g.total_blocks;
  if (t < kIdctBlocks) {  // block `u` in plane order: component, position
    int u = blockIdx.x * kIdctBlocks + t, c = -1, bx = 0, by = 0;
    if (u < total) {
      c = u < n0 ? 0 : (u < n0 + n1 ? 1 : 2);
      u -= c == 0 ? 0 : (c == 1 ? n0 : n0 + n1);
      by = u / g.bw[c];
      bx = u - by * g.bw[c];
    }
    s_comp[t] = c;
    s_bx[t] = bx;
    s_by[t] = by;
  }
  __syncthreads();
  {  // A
    const int b = t >> 3, r = t & 7, c = s_comp[b];
    int d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c >= 0) {
      const size_t at = (size_t)mcu_order_index(g, c, s_bx[b], s_by[b]) * 64 + (size_t)r * 8;
      const int4 raw = *reinterpret_cast<const int4*>(coefs + at);
      const int w4[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        d[2 * k] = dequant((short)(w4[k] & 0xffff), p.qt[c][r * 8 + 2 * k]);
        d[2 * k + 1] = dequant((short)(w4[k] >> 16), p.qt[c][r * 8 + 2 * k + 1]);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s_d[b][r * 8 + k] = d[k];
  }
  __syncthreads();
  {  // B
    const int b = t >> 3, c = t & 7;
    int d[8];
    int64_t w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = s_d[b][r * 8 + c];
    idct_column(d, w);
#pragma unroll
    for (int r = 0; r < 8; ++r) s_w[r][b][c] = w[r];
  }
  __syncthreads();
  {  // C
    const int r = t >> 5, b = t & 31, c = s_comp[b];
    if (c >= 0) {
      int64_t w[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = s_w[r][b][k];
      unsigned char o[8];
      idct_row(w, o);
      uint2 packed;
      packed.x = o[0] | (o[1] << 8) | (o[2] << 16) | ((uint32_t)o[3] << 24);
      packed.y = o[4] | (o[5] << 8) | (o[6] << 16) | ((uint32_t)o[7] << 24);
      const size_t stride = (size_t)g.bw[c] * 8;
      unsigned char* dst = planes + g.plane_off[c] + ((size_t)s_by[b] * 8 + r) * stride + (size_t)s_bx[b] * 8;
      *reinterpret_cast<uint2*>(dst) = packed;
    }
  }
}

// Upsampling + colour conversion: thread i writes pixels 4 i .. 4 i + 3 of the image taken as one row of width * height pixels,
// that is bytes 12 i .. 12 i + 11 of the RGB8 buffer: three aligned dwords whatever the width.
struct Rgb4 {
  uint32_t a, b, c;
};
__global__ __launch_bounds__(256) void k_colour(BackParams p, const unsigned char* planes, unsigned char* rgb, int aligned) {
  const Geometry& g = p.g;
  const size_t npix = (size_t)g.width * g.height;
  const size_t first = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (first >= npix) return;
  const unsigned char* py = planes + g.plane_off[0];
  const unsigned char* pb = planes + g.plane_off[1];
  const unsigned char* pr = planes + g.plane_off[2];
  const int hx = g.hmax / g.h[1], vx = g.vmax / g.v[1];
  unsigned char o[12];
  int y = (int)(first / (size_t)g.width), x = (int)(first - (size_t)y * g.width);
  const int count = npix - first < 4 ? (int)(npix - first) : 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o[3 * k] = o[3 * k + 1] = o[3 * k + 2] = 0;
    if (k < count) {
      const int Y = py[(size_t)y * (g.bw[0] * 8) + x];
      const int B = upsampled_sample(pb, g.bw[1] * 8, g.dw[1], g.dh[1], hx, vx, x, y);
      const int R = upsampled_sample(pr, g.bw[2] * 8, g.dw[2], g.dh[2], hx, vx, x, y);
      ycc_to_rgb(Y, B, R, &o[3 * k + (p.flip ? 2 : 0)], &o[3 * k + 1], &o[3 * k + (p.flip ? 0 : 2)]);
      if (++x == g.width) {
        x = 0;
        ++y;
      }
    }
  }
  unsigned char* dst = rgb + first * 3;
  if (count == 4 && aligned) {
    Rgb4 v;
    v.a = o[0] | (o[1] << 8) | (o[2] << 16) | ((uint32_t)o[3] << 24);
    v.b = o[4] | (o[5] << 8) | (o[6] << 16) | ((uint32_t)o[7] << 24);
    v.c = o[8] | (o[9] << 8) | (o[10] << 16) | ((uint32_t)o[11] << 24);
    *reinterpret_cast<Rgb4*>(dst) = v;
  } else {
    for (int k = 0; k < count * 3; ++k) dst[k] = o[k];
  }
}

struct Slot {
  unsigned char* pinned = nullptr;  // [input block | coefficients | depth | rgb]
  hipEvent_t done = nullptr;
  bool in_flight = false;
};

}  // namespace

struct dms_jpeg_dev {
  int width = 0, height = 0, S = DMS_JPEG_DEV_DEFAULT_SUBSEQUENCE, readers_on_host = 1;
  size_t max_px = 0, max_stream = 0, max_blocks = 0, max_segs = 0, max_lanes = 0;
  size_t in_bytes = 0, off_coef = 0, off_depth = 0, off_rgb = 0, slot_bytes = 0;
  std::vector<Slot> slots;
  int next = 0;
  unsigned char* d_in = nullptr;
  short* d_coef = nullptr;
  unsigned char* d_planes = nullptr;
  LaneRecord* d_rec0 = nullptr;
  LaneRecord* d_rec1 = nullptr;
  uint32_t* d_block = nullptr;
  DevStatus* d_status = nullptr;  // followed by the per-segment flags
  hipEvent_t last_done = nullptr;
  hipStream_t last_stream = nullptr;
  bool any = false;
  // the last decode
  dms_jpeg_dev_info info = {};
  const char* restart_err = nullptr;
  std::vector<Segment> segs;
  std::vector<SegInfo> si;
  std::vector<LaneInfo> lanes;
};

namespace {

// the most blocks and segments a width x height stream can have: 4:4:4, 4:2:2 or 4:2:0; a restart interval of one MCU
void size_caps(int width, int height, size_t* blocks, size_t* segs) {
  const size_t w8 = ((size_t)width + 7) / 8, h8 = ((size_t)height + 7) / 8, w16 = ((size_t)width + 15) / 16, h16 = ((size_t)height + 15) / 16;
  *blocks = 3 * w8 * h8;
  if (4 * w16 * h8 > *blocks) *blocks = 4 * w16 * h8;
  if (6 * w16 * h16 > *blocks) *blocks = 6 * w16 * h16;
  *segs = w8 * h8;
}

int free_all(dms_jpeg_dev* jd) {
  for (Slot& s : jd->slots) {
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.pinned) (void)hipHostFree(s.pinned);
  }
  if (jd->last_done) (void)hipEventDestroy(jd->last_done);
  void* dev[] = {jd->d_in, jd->d_coef, jd->d_planes, jd->d_rec0, jd->d_rec1, jd->d_block, jd->d_status};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  delete jd;
  return DMS_OK;
}

}  // namespace

namespace dms {
namespace jpegdev {

int width(const dms_jpeg_dev* jd) { return jd->width; }
int height(const dms_jpeg_dev* jd) { return jd->height; }
int entropy_on_host(const dms_jpeg_dev* jd) { return jd->readers_on_host; }

int acquire(dms_jpeg_dev* jd, hipStream_t stream, FrameSlot* out) {
  Slot& s = jd->slots[(size_t)jd->next];
  if (s.in_flight) {
    DMS_HIP(hipEventSynchronize(s.done));
    s.in_flight = false;
  }
  // the device buffers are one set: a decode on another stream waits for the one before
  if (jd->any && jd->last_stream != stream) DMS_HIP(hipStreamWaitEvent(stream, jd->last_done, 0));
  out->index = jd->next;
  out->depth = reinterpret_cast<unsigned short*>(s.pinned + jd->off_depth);
  out->rgb = s.pinned + jd->off_rgb;
  jd->next = (jd->next + 1) % (int)jd->slots.size();
  return DMS_OK;
}

int release(dms_jpeg_dev* jd, const FrameSlot& slot, hipStream_t stream) {
  Slot& s = jd->slots[(size_t)slot.index];
  DMS_HIP(hipEventRecord(s.done, stream));
  s.in_flight = true;
  DMS_HIP(hipEventRecord(jd->last_done, stream));
  jd->last_stream = stream;
  jd->any = true;
  return DMS_OK;
}

int decode(dms_jpeg_dev* jd, const FrameSlot& slot, const unsigned char* data, size_t len, int flip, int on_host, void* rgb_dev,
           hipStream_t stream, const char* who) {
  Decoder d;
  const int prc = parse(d, data, len, jd->width, jd->height);
  if (prc) {
    dms::set_error("%s: %s", who, d.err ? d.err : "");
    return prc == -2 ? DMS_ERR_UNSUPPORTED : DMS_ERR_FORMAT;
  }
  const Geometry& g = d.geo;
  const size_t scan_off = (size_t)(d.p - data), scan_len = len - scan_off;
  if (scan_len > jd->max_stream || (size_t)g.total_blocks > jd->max_blocks) {
    dms::set_error("%s: a stream of %zu bytes, the decoder was created for %zu", who, scan_len, jd->max_stream);
    return DMS_ERR_WORKSPACE;
  }
  Slot& s = jd->slots[(size_t)slot.index];
  BackParams bp;
  bp.g = g;
  for (int i = 0; i < 3; ++i) memcpy(bp.qt[i], d.qt[d.comp[i].tq], sizeof(bp.qt[i]));
  bp.flip = flip ? 1 : 0;
  dms_jpeg_dev_info& info = jd->info;
  info = dms_jpeg_dev_info();
  info.entropy_on_host = on_host ? 1 : 0;
  info.subsequence_bytes = jd->S;
  info.blocks = g.total_blocks;
  jd->restart_err = nullptr;
  const size_t coef_bytes = (size_t)g.total_blocks * 64 * sizeof(short);

  if (on_host) {
    short* coefs = reinterpret_cast<short*>(s.pinned + jd->off_coef);
    memset(coefs, 0, coef_bytes);
    if (!d.entropy(coefs)) {
      dms::set_error("%s: %s", who, d.err ? d.err : "");
      return d.unsupported ? DMS_ERR_UNSUPPORTED : DMS_ERR_FORMAT;
    }
    info.segments = g.restart_interval ? (g.mcux * g.mcuy + g.restart_interval - 1) / g.restart_interval : 1;
    DMS_HIP(hipMemcpyAsync(jd->d_coef, coefs, coef_bytes, hipMemcpyHostToDevice, stream));
  } else {
    // indices from here on are relative to the first byte of the entropy-coded data
    const unsigned char* scan = data + scan_off;
    find_segments(scan, scan_len, 0, g, jd->segs, &jd->restart_err);
    build_lanes(g, jd->segs, jd->S, jd->si, jd->lanes);
    const int nseg = (int)jd->si.size(), nlanes = (int)jd->lanes.size();
    if ((size_t)nseg > jd->max_segs || (size_t)nlanes > jd->max_lanes) {
      dms::set_error("%s: %d segments / %d subsequences exceed the decoder's buffers", who, nseg, nlanes);
      return DMS_ERR_WORKSPACE;
    }
    info.segments = nseg;
    info.subsequences = nlanes;
    // [tables | segments | lanes | stream]
    const size_t o_seg = sizeof(LaneTables), o_lane = o_seg + align16((size_t)nseg * sizeof(SegInfo));
    const size_t o_stream = o_lane + align16((size_t)nlanes * sizeof(LaneInfo)), total = o_stream + align16(scan_len) + kStreamPad;
    LaneTables* t = reinterpret_cast<LaneTables*>(s.pinned);
    memset(t, 0, sizeof(LaneTables));
    t->g = g;
    for (int i = 0; i < 3; ++i) {
      t->dc[i] = d.dc[d.comp[i].td];
      t->ac[i] = d.ac[d.comp[i].ta];
    }
    memcpy(s.pinned + o_seg, jd->si.data(), (size_t)nseg * sizeof(SegInfo));
    memcpy(s.pinned + o_lane, jd->lanes.data(), (size_t)nlanes * sizeof(LaneInfo));
    memcpy(s.pinned + o_stream, scan, scan_len);
    memset(s.pinned + o_stream + scan_len, 0, total - o_stream - scan_len);
    DMS_HIP(hipMemcpyAsync(jd->d_in, s.pinned, total, hipMemcpyHostToDevice, stream));
    DMS_HIP(hipMemsetAsync(jd->d_coef, 0, coef_bytes, stream));
    DMS_HIP(hipMemsetAsync(jd->d_status, 0, sizeof(DevStatus) + (size_t)nseg, stream));
    DMS_HIP(hipMemsetAsync(&jd->d_status->err_key, 0xff, sizeof(uint32_t), stream));
    const LaneTables* dt = reinterpret_cast<const LaneTables*>(jd->d_in);
    const SegInfo* dseg = reinterpret_cast<const SegInfo*>(jd->d_in + o_seg);
    const LaneInfo* dlane = reinterpret_cast<const LaneInfo*>(jd->d_in + o_lane);
    const unsigned char* dstream = jd->d_in + o_stream;
    unsigned char* dirty = reinterpret_cast<unsigned char*>(jd->d_status + 1);
    const int grid = (nlanes + kLaneBlock - 1) / kLaneBlock;
    const size_t lds = lane_lds_bytes(jd->S);
    for (int r = 0; r < kSyncRounds; ++r)
      hipLaunchKernelGGL(k_sync_round, dim3(grid), dim3(kLaneBlock), lds, stream, dt, dseg, dlane, nlanes, dstream, (uint32_t)scan_len, jd->S, r,
                         jd->d_rec0, jd->d_rec1, jd->d_status, dirty);
    hipLaunchKernelGGL(k_settle, dim3((nseg + kLaneBlock - 1) / kLaneBlock), dim3(kLaneBlock), 0, stream, dt, dseg, dlane, nlanes, nseg, dstream,
                       jd->d_rec0, jd->d_rec1, jd->d_status, dirty);
    hipLaunchKernelGGL(k_block_offsets, dim3(1), dim3(1024), 0, stream, dseg, dlane, nlanes, jd->d_rec0, jd->d_rec1, jd->d_status, jd->d_block + jd->max_lanes,
                       jd->d_block);
    hipLaunchKernelGGL(k_write, dim3(grid), dim3(kLaneBlock), lds, stream, dt, dseg, dlane, nlanes, dstream, (uint32_t)scan_len, jd->S, jd->d_rec0,
                       jd->d_rec1, jd->d_status, jd->d_block, jd->d_coef);
    hipLaunchKernelGGL(k_dc_sums, dim3(3), dim3(1024), 0, stream, g, jd->d_coef);
    DMS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_idct, dim3((g.total_blocks + kIdctBlocks - 1) / kIdctBlocks), dim3(256), 0, stream, bp, jd->d_coef, jd->d_planes);
  const size_t quads = ((size_t)g.width * g.height + 3) / 4;
  hipLaunchKernelGGL(k_colour, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, bp, jd->d_planes, (unsigned char*)rgb_dev,
                     ((uintptr_t)rgb_dev & 3) == 0 ? 1 : 0);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

}  // namespace jpegdev
}  // namespace dms

extern "C" {

int dms_jpeg_dev_create(dms_jpeg_dev** out, int width, int height, size_t max_stream_bytes, int slots) {
  DMS_REQUIRE(out, "null argument");
  DMS_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "bad image size");
  DMS_REQUIRE(max_stream_bytes >= 64 && max_stream_bytes <= ((size_t)1 << 26), "max_stream_bytes outside 64 .. 64 MiB");
  DMS_REQUIRE(slots >= 1 && slots <= 16, "slots outside 1 .. 16");
  dms_jpeg_dev* jd = new dms_jpeg_dev();
  jd->width = width;
  jd->height = height;
  jd->max_stream = max_stream_bytes;
  size_caps(width, height, &jd->max_blocks, &jd->max_segs);
  jd->max_px = (size_t)width * height;
  jd->max_lanes = max_stream_bytes / 32 + jd->max_segs + 1;
  jd->in_bytes = sizeof(LaneTables) + align16(jd->max_segs * sizeof(SegInfo)) + align16(jd->max_lanes * sizeof(LaneInfo)) +
                 align16(max_stream_bytes) + kStreamPad;
  const size_t px = (size_t)width * height;
  jd->off_coef = align16(jd->in_bytes);
  jd->off_depth = jd->off_coef + align16(jd->max_blocks * 64 * sizeof(short));
  jd->off_rgb = jd->off_depth + align16(px * 2);
  jd->slot_bytes = jd->off_rgb + align16(px * 3);
  jd->slots.resize((size_t)slots);
  auto fail = [&](hipError_t e, const char* what) {
    free_all(jd);
    return dms::hip_fail(e, what, __FILE__, __LINE__);
  };
  hipError_t e;
  for (Slot& s : jd->slots) {
    if ((e = hipHostMalloc((void**)&s.pinned, jd->slot_bytes, hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc");
    if ((e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  }
  if ((e = hipEventCreateWithFlags(&jd->last_done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipMalloc((void**)&jd->d_in, jd->in_bytes)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&jd->d_coef, jd->max_blocks * 64 * sizeof(short))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&jd->d_planes, jd->max_blocks * 64)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&jd->d_rec0, jd->max_lanes * sizeof(LaneRecord))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&jd->d_rec1, jd->max_lanes * sizeof(LaneRecord))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&jd->d_block, 2 * jd->max_lanes * sizeof(uint32_t))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&jd->d_status, sizeof(DevStatus) + align16(jd->max_segs))) != hipSuccess) return fail(e, "hipMalloc");
  *out = jd;
  return DMS_OK;
}

int dms_jpeg_dev_destroy(dms_jpeg_dev* jd) {
  if (!jd) return DMS_OK;
  if (jd->any) (void)hipEventSynchronize(jd->last_done);
  return free_all(jd);
}

int dms_jpeg_dev_set_subsequence_bytes(dms_jpeg_dev* jd, int bytes) {
  DMS_REQUIRE(jd, "null argument");
  DMS_REQUIRE(bytes == 32 || bytes == 64 || bytes == 128 || bytes == 256, "a subsequence is 32, 64, 128 or 256 bytes");
  jd->S = bytes;
  return DMS_OK;
}

int dms_jpeg_dev_set_image_size(dms_jpeg_dev* jd, int width, int height) {
  DMS_REQUIRE(jd, "null argument");
  DMS_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "bad image size");
  size_t blocks, segs;
  size_caps(width, height, &blocks, &segs);
  DMS_REQUIRE(blocks <= jd->max_blocks && segs <= jd->max_segs && (size_t)width * height <= jd->max_px, "larger than the size the decoder was created for");
  jd->width = width;
  jd->height = height;
  return DMS_OK;
}

int dms_jpeg_dev_set_entropy_on_host(dms_jpeg_dev* jd, int on) {
  DMS_REQUIRE(jd, "null argument");
  jd->readers_on_host = on ? 1 : 0;
  return DMS_OK;
}

int dms_jpeg_dev_decode(dms_jpeg_dev* jd, const void* data, size_t len, int flipColors, int entropy_on_host, void* rgb_dev, dms_stream stream) {
  DMS_REQUIRE(jd && data && rgb_dev, "null argument");
  dms::jpegdev::FrameSlot slot;
  int rc = dms::jpegdev::acquire(jd, (hipStream_t)stream, &slot);
  if (rc) return rc;
  rc = dms::jpegdev::decode(jd, slot, (const unsigned char*)data, len, flipColors, entropy_on_host, rgb_dev, (hipStream_t)stream, "dms_jpeg_dev_decode");
  const int rr = dms::jpegdev::release(jd, slot, (hipStream_t)stream);
  return rc ? rc : rr;
}

int dms_jpeg_dev_status(dms_jpeg_dev* jd, dms_jpeg_dev_info* info) {
  DMS_REQUIRE(jd, "null argument");
  if (jd->any) DMS_HIP(hipEventSynchronize(jd->last_done));
  int rc = DMS_OK;
  if (jd->any && !jd->info.entropy_on_host && jd->info.subsequences) {
    DevStatus st;
    DMS_HIP(hipMemcpy(&st, jd->d_status, sizeof(st), hipMemcpyDeviceToHost));
    int rounds = 1;
    while (rounds < kSyncRounds && st.changed[rounds - 1]) ++rounds;
    jd->info.rounds = rounds;
    jd->info.settled_lanes = (int)st.settled;
    const char* why = st.err_key != kNoBlockError ? block_error_text((int)(st.err_key & 3)) : jd->restart_err;
    if (why) {
      dms::set_error("dms_jpeg_dev_status: %s", why);
      rc = DMS_ERR_FORMAT;
    }
  }
  if (info) *info = jd->info;
  return rc;
}

int dms_jpeg_dev_get_coefficients(dms_jpeg_dev* jd, short* coefs_host, size_t max_blocks, int* blocks) {
  DMS_REQUIRE(jd && coefs_host && blocks, "null argument");
  DMS_REQUIRE(jd->any, "no decode yet");
  DMS_REQUIRE((size_t)jd->info.blocks <= max_blocks, "buffer too small");
  DMS_HIP(hipEventSynchronize(jd->last_done));
  DMS_HIP(hipMemcpy(coefs_host, jd->d_coef, (size_t)jd->info.blocks * 64 * sizeof(short), hipMemcpyDeviceToHost));
  *blocks = jd->info.blocks;
  return DMS_OK;
}

}  // extern "C"
