// JPEG colour encoded on the device (include/dmslam_io_write.h).  The arithmetic is csrc/jpeg_enc_core.hpp, the one the host's
// sequential encoder (csrc/jpeg_enc.hpp) compiles; tests/jpeg_enc_host.cpp runs the entropy passes below with the blocks one after
// another on the host.
//
//   host     geometry, quantisation tables, the header straight into the pinned slot
//   device   k_enc_colour      RGB8 -> Y plane + (downsampled) Cb / Cr planes, padded to whole MCUs by libjpeg's replication rules;
//                              4 pixels (3 dwords) per row and thread
//            k_fdct            planes -> quantised coefficients in the scan's MCU order, 8 lanes per block; dummy blocks are zeros
//     entropy on the device:
//            k_enc_bits        per block: DC difference against the real block before it, bit length
//            k_scan_blocks     exclusive sums of the lengths (csrc/scan.hpp) and the total
//            k_enc_write       every block writes its bits at its offset into the zeroed word buffer (atomicOr on the two words it
//                              may share, plain stores in between); the last block pads the last byte with 1-bits
//            k_stuff_count     FF bytes per chunk of 64 bytes;  k_scan_blocks again
//            k_stuff_scatter   bytes to their final place, 00 behind each FF; EOI and the length
//            copies            length word and the first bytes of the stream -> pinned slot (the rest, if a stream is longer than
//                              that, when the result is asked for)
//     entropy on the host:     coefficients -> pinned slot; dms_jpeg_enc_result runs enc_entropy_sequential
//   depth of a frame: copied into the slot and deflated by the host while the colour kernels run, or (set_depth_on_device) deflated
//   by the kernels of csrc/deflate_dev.hip on the same stream, their stream landing in the slot's deflate area
// No kernel waits on another workgroup: the stages are separate launches.
#include <string.h>

#include <vector>

#include "../../include/dmslam_io_write.h"
#include "common.hpp"
#include "deflate_dev.hpp"
#include "jpeg_enc.hpp"
#include "scan.hpp"

namespace {

using namespace dms::jpeg;

struct EncParams {
  Geometry g;
  unsigned short qt[2][64];
  int flip;
};

// ---- colour ---------------------------------------------------------------------------------------------------------------------
// Y, Cb, Cr of pixels x0 .. x0 + 3 (columns replicated past the right edge) of pixel row y
__device__ __forceinline__ void row_ycc(const unsigned char* rgb, int W, int x0, int y, int flip, int aligned, int Y[4], int B[4], int R[4]) {
  unsigned char px[12];
  const size_t first = (size_t)y * W + x0;
  if (aligned && x0 + 3 < W && (first & 3) == 0) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rgb + first * 3);
    const uint32_t a = src[0], b = src[1], c = src[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = (unsigned char)(a >> (8 * k));
      px[4 + k] = (unsigned char)(b >> (8 * k));
      px[8 + k] = (unsigned char)(c >> (8 * k));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned char* p = rgb + ((size_t)y * W + enc_src(x0 + k, W)) * 3;
      px[3 * k] = p[0];
      px[3 * k + 1] = p[1];
      px[3 * k + 2] = p[2];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) rgb_to_ycc(px[3 * k + (flip ? 2 : 0)], px[3 * k + 1], px[3 * k + (flip ? 0 : 2)], &Y[k], &B[k], &R[k]);
}
__device__ __forceinline__ uint32_t pack4(const int v[4]) { return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24); }

// thread (qx, ry): columns 4 qx .. 4 qx + 3 of the vmax rows of row group ry of the padded Y plane, and the chroma samples under them
__global__ __launch_bounds__(256) void k_enc_colour(EncParams p, const unsigned char* rgb, unsigned char* planes, int aligned) {
  const Geometry& g = p.g;
  const int qx = blockIdx.x * blockDim.x + threadIdx.x, ry = blockIdx.y * blockDim.y + threadIdx.y;
  const int v = g.vmax, W = g.width, H = g.height;
  if (qx >= g.bw[0] * 2 || ry >= g.bh[0] * 8 / v) return;
  const int x0 = qx * 4, sy = g.bw[0] * 8, sc = g.bw[1] * 8;
  unsigned char* py = planes + g.plane_off[0];
  unsigned char* pb = planes + g.plane_off[1];
  unsigned char* pr = planes + g.plane_off[2];
  int Y0[4], B0[4], R0[4], Y1[4], B1[4], R1[4];
  const int y0 = enc_src(ry * v, H);
  row_ycc(rgb, W, x0, y0, p.flip, aligned, Y0, B0, R0);
  *reinterpret_cast<uint32_t*>(py + (size_t)(ry * v) * sy + x0) = pack4(Y0);
  if (v == 1) {  // 4:4:4
    *reinterpret_cast<uint32_t*>(pb + (size_t)ry * sc + x0) = pack4(B0);
    *reinterpret_cast<uint32_t*>(pr + (size_t)ry * sc + x0) = pack4(R0);
    return;
  }
  const int y1 = enc_src(ry * 2 + 1, H);
  row_ycc(rgb, W, x0, y1, p.flip, aligned, Y1, B1, R1);
  *reinterpret_cast<uint32_t*>(py + (size_t)(ry * 2 + 1) * sy + x0) = pack4(Y1);
  int xs[2], ys[2];
  h2v2_sources(qx * 2, ry, W, H, xs, ys);
  if (ys[0] != y0 || ys[1] != y1) {  // below the last chroma row: its two pixel rows, not the last pixel row twice
    row_ycc(rgb, W, x0, ys[0], p.flip, aligned, Y0, B0, R0);
    row_ycc(rgb, W, x0, ys[1], p.flip, aligned, Y1, B1, R1);
  }
  const int cb0 = h2v2_box(B0[0], B0[1], B1[0], B1[1], qx * 2), cb1 = h2v2_box(B0[2], B0[3], B1[2], B1[3], qx * 2 + 1);
  const int cr0 = h2v2_box(R0[0], R0[1], R1[0], R1[1], qx * 2), cr1 = h2v2_box(R0[2], R0[3], R1[2], R1[3], qx * 2 + 1);
  *reinterpret_cast<unsigned short*>(pb + (size_t)ry * sc + qx * 2) = (unsigned short)(cb0 | (cb1 << 8));
  *reinterpret_cast<unsigned short*>(pr + (size_t)ry * sc + qx * 2) = (unsigned short)(cr0 | (cr1 << 8));
}

// ---- forward DCT: the mirror of k_idct.  256 threads take 32 blocks that follow one another in the scan, 8 lanes per block:
//   A  thread (block b, row r) loads the 8 samples of one block row (8 bytes), level-shifts them and runs the row pass
//   B  thread (block b, column c) runs the column pass over the transposed workspace and quantises
//   C  thread (block b, row r) stores the 8 coefficients of one block row (16 bytes; the 8 lanes of a block write 128 contiguous bytes)
constexpr int kFdctBlocks = 32;
__global__ __launch_bounds__(256) void k_fdct(EncParams p, const unsigned char* planes, short* coefs) {
  __shared__ int s_w[kFdctBlocks][72];  // [block][r * 8 + c] (+8: the column reads spread over banks)
  __shared__ short s_q[kFdctBlocks][64];
  __shared__ int s_comp[kFdctBlocks], s_bx[kFdctBlocks], s_by[kFdctBlocks];
  const Geometry& g = p.g;
  const int t = threadIdx.x;
  if (t < kFdctBlocks) {
    const int u = blockIdx.x * kFdctBlocks + t;
    int c = -1, bx = 0, by = 0;
    if (u < g.total_blocks) {
      enc_block_position(g, u, &c, &bx, &by);
      if (!enc_block_is_real(g, c, bx, by)) c = -2;  // a dummy block: zeros
    }
    s_comp[t] = c;
    s_bx[t] = bx;
    s_by[t] = by;
  }
  __syncthreads();
  const int b = t >> 3, r = t & 7, c = s_comp[b];
  if (c >= 0) {  // A
    const size_t stride = (size_t)g.bw[c] * 8;
    const uint2 raw = *reinterpret_cast<const uint2*>(planes + g.plane_off[c] + ((size_t)s_by[b] * 8 + r) * stride + (size_t)s_bx[b] * 8);
    int d[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = (int)((raw.x >> (8 * k)) & 0xff) - 128;
      d[4 + k] = (int)((raw.y >> (8 * k)) & 0xff) - 128;
    }
    fdct_pass<1>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) s_w[b][r * 8 + k] = d[k];
  }
  __syncthreads();
  {  // B: here `r` is the column
    int d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c >= 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = s_w[b][k * 8 + r];
      fdct_pass<2>(d);
      const unsigned short* q = p.qt[c ? 1 : 0];
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = enc_quantise(d[k], q[k * 8 + r]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s_q[b][k * 8 + r] = (short)d[k];
  }
  __syncthreads();
  if (c != -1) {  // C
    const int u = blockIdx.x * kFdctBlocks + b;
    *reinterpret_cast<int4*>(coefs + (size_t)u * 64 + r * 8) = *reinterpret_cast<const int4*>(&s_q[b][r * 8]);
  }
}

// ---- entropy on the device ------------------------------------------------------------------------------------------------------
constexpr int kEntropyBlock = 64;
static_assert(sizeof(EncTables) % 16 == 0, "copied as 16-byte words");

__device__ __forceinline__ const EncTables* stage_tables(const EncTables* tabs, uint4* lds) {
  const uint4* src = reinterpret_cast<const uint4*>(tabs);
  for (int i = threadIdx.x; i < (int)(sizeof(EncTables) / 16); i += blockDim.x) lds[i] = src[i];
  __syncthreads();
  return reinterpret_cast<const EncTables*>(lds);
}

__global__ __launch_bounds__(kEntropyBlock) void k_enc_bits(EncParams p, const EncTables* tabs, const short* coefs, uint32_t* bits) {
  __shared__ uint4 s_tabs[sizeof(EncTables) / 16];
  const EncTables* t = stage_tables(tabs, s_tabs);
  const Geometry& g = p.g;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= g.total_blocks) return;
  const int c = g.mcu_comp[u % g.blocks_per_mcu] ? 1 : 0;
  bits[u] = enc_block_bits(coefs + (size_t)u * 64, enc_dc_diff(g, coefs, u), t->dc[c], t->ac[c]);
}

struct DevSink {
  uint32_t* words;
  __device__ __forceinline__ void merge(uint32_t i, uint32_t v) { atomicOr(words + i, v); }
  __device__ __forceinline__ void store(uint32_t i, uint32_t v) { words[i] = v; }
};

__global__ __launch_bounds__(kEntropyBlock) void k_enc_write(EncParams p, const EncTables* tabs, const short* coefs, const uint32_t* offsets,
                                                             const uint32_t* total_bits, uint32_t* words) {
  __shared__ uint4 s_tabs[sizeof(EncTables) / 16];
  const EncTables* t = stage_tables(tabs, s_tabs);
  const Geometry& g = p.g;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= g.total_blocks) return;
  const int c = g.mcu_comp[u % g.blocks_per_mcu] ? 1 : 0;
  DevSink sink{words};
  BitWriter<DevSink> bw(sink, offsets[u]);
  enc_block_emit(coefs + (size_t)u * 64, enc_dc_diff(g, coefs, u), t->dc[c], t->ac[c], bw);
  if (u == g.total_blocks - 1) {
    const int pad = enc_pad_bits(total_bits[0]);
    bw.put((1u << pad) - 1u, pad);
  }
  bw.finish();
}

__global__ __launch_bounds__(256) void k_stuff_count(const uint32_t* words, const uint32_t* total_bits, uint32_t* counts, int nchunks) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nchunks) return;
  counts[t] = enc_chunk_ff(words, (uint32_t)t, (total_bits[0] + 7) >> 3);
}

__global__ __launch_bounds__(256) void k_stuff_scatter(const uint32_t* words, const uint32_t* total_bits, const uint32_t* ff_before, int nchunks,
                                                       unsigned char* out, uint32_t* len) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nchunks) return;
  const uint32_t n = enc_chunk_scatter(words, (uint32_t)t, (total_bits[0] + 7) >> 3, ff_before[t], out);
  if (n) len[0] = n;
}

constexpr size_t kLenBytes = 16;  // the length word in front of the device's stream and of the slot's file

struct Slot {
  unsigned char* pinned = nullptr;  // [length word | file: header, stream | coefficients | depth | deflated depth]
  unsigned char* d_out = nullptr;   // [length word | stuffed stream, EOI]
  hipEvent_t done = nullptr;
  bool in_flight = false, used = false, finished = false;
  int on_host = 0, hdr = 0;
  Geometry g;
  size_t len = 0, eager = 0, z_eager = 0;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the larger of the 4:2:0 and the 4:4:4 shape of a width x height frame
void size_caps(int width, int height, size_t* blocks, size_t* plane_bytes) {
  Geometry a, b;
  enc_geometry(width, height, DMS_JPEG_420, &a);
  enc_geometry(width, height, DMS_JPEG_444, &b);
  *blocks = (size_t)(a.total_blocks > b.total_blocks ? a.total_blocks : b.total_blocks);
  *plane_bytes = (size_t)(a.plane_bytes > b.plane_bytes ? a.plane_bytes : b.plane_bytes);
}

}  // namespace

struct dms_jpeg_enc {
  int width = 0, height = 0, writers_on_host = DMS_JPEG_ENC_DEFAULT_ENTROPY_ON_HOST, depth_on_device = DMS_RECORD_DEFAULT_DEPTH_ON_DEVICE;
  dms_deflate_dev* dd = nullptr;  // made by the first frame whose depth is deflated on the device; slot k of its ring serves slot k here
  size_t max_px = 0, max_blocks = 0, max_planes = 0;
  size_t off_coef = 0, off_depth = 0, off_z = 0, z_cap = 0, slot_bytes = 0, out_bytes = 0;
  std::vector<Slot> slots;
  int next = 0;
  unsigned char* d_planes = nullptr;
  short* d_coef = nullptr;
  uint32_t* d_bits = nullptr;    // [lengths | offsets | total]
  uint32_t* d_words = nullptr;   // the unstuffed stream, MSB-first words
  uint32_t* d_chunks = nullptr;  // [FF counts | offsets | total]
  EncTables* d_tables = nullptr;
  EncTables tables;
  hipEvent_t last_done = nullptr, depth_done = nullptr;
  hipStream_t last_stream = nullptr;
  bool any = false;
};

namespace {

int free_all(dms_jpeg_enc* je) {
  for (Slot& s : je->slots) {
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.pinned) (void)hipHostFree(s.pinned);
    if (s.d_out) (void)hipFree(s.d_out);
  }
  if (je->last_done) (void)hipEventDestroy(je->last_done);
  if (je->depth_done) (void)hipEventDestroy(je->depth_done);
  if (je->dd) (void)dms_deflate_dev_destroy(je->dd);
  void* dev[] = {je->d_planes, je->d_coef, je->d_bits, je->d_words, je->d_chunks, je->d_tables};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  delete je;
  return DMS_OK;
}

size_t max_chunks(size_t blocks) { return (blocks * (kEncMaxBlockBits / 8) + kEncChunk - 1) / kEncChunk + 1; }

int acquire(dms_jpeg_enc* je, hipStream_t stream, int* index) {
  Slot& s = je->slots[(size_t)je->next];
  if (s.in_flight) {
    DMS_HIP(hipEventSynchronize(s.done));
    s.in_flight = false;
  }
  // the device buffers are one set: an encode on another stream waits for the one before
  if (je->any && je->last_stream != stream) DMS_HIP(hipStreamWaitEvent(stream, je->last_done, 0));
  *index = je->next;
  je->next = (je->next + 1) % (int)je->slots.size();
  s.used = true;
  s.finished = false;
  s.on_host = -1;  // no JPEG in the slot yet
  s.len = 0;
  return DMS_OK;
}

int release(dms_jpeg_enc* je, int index, hipStream_t stream) {
  Slot& s = je->slots[(size_t)index];
  DMS_HIP(hipEventRecord(s.done, stream));
  s.in_flight = true;
  DMS_HIP(hipEventRecord(je->last_done, stream));
  je->last_stream = stream;
  je->any = true;
  return DMS_OK;
}

bool encode_args_ok(const char* who, const void* rgb_dev, int quality, int subsampling) {
  if (!rgb_dev) {
    dms::set_error("%s: null device pointer", who);
    return false;
  }
  if (quality < 1 || quality > 100) {
    dms::set_error("%s: quality %d outside 1 .. 100", who, quality);
    return false;
  }
  if (subsampling != DMS_JPEG_420 && subsampling != DMS_JPEG_444) {
    dms::set_error("%s: subsampling %d is neither DMS_JPEG_420 nor DMS_JPEG_444", who, subsampling);
    return false;
  }
  return true;
}

// everything of one encode onto `stream`; the arguments are checked
int enqueue(dms_jpeg_enc* je, int index, const void* rgb_dev, int quality, int subsampling, int flip, int on_host, hipStream_t stream) {
  Slot& s = je->slots[(size_t)index];
  EncParams p;
  enc_geometry(je->width, je->height, subsampling, &p.g);
  enc_quant_table(0, quality, p.qt[0]);
  enc_quant_table(1, quality, p.qt[1]);
  p.flip = flip ? 1 : 0;
  const Geometry& g = p.g;
  s.g = g;
  s.on_host = on_host ? 1 : 0;
  s.hdr = enc_write_header(je->width, je->height, subsampling, p.qt, s.pinned + kLenBytes);
  const int nb = g.total_blocks;

  const dim3 cb(64, 4), cg((unsigned)((g.bw[0] * 2 + 63) / 64), (unsigned)((g.bh[0] * 8 / g.vmax + 3) / 4));
  hipLaunchKernelGGL(k_enc_colour, cg, cb, 0, stream, p, (const unsigned char*)rgb_dev, je->d_planes, ((uintptr_t)rgb_dev & 3) == 0 ? 1 : 0);
  hipLaunchKernelGGL(k_fdct, dim3((unsigned)((nb + kFdctBlocks - 1) / kFdctBlocks)), dim3(256), 0, stream, p, je->d_planes, je->d_coef);
  DMS_CHECK_LAUNCH();
  if (on_host) {
    DMS_HIP(hipMemcpyAsync(s.pinned + je->off_coef, je->d_coef, (size_t)nb * 64 * sizeof(short), hipMemcpyDeviceToHost, stream));
    return DMS_OK;
  }
  uint32_t* bits = je->d_bits;
  uint32_t* offsets = bits + je->max_blocks;
  uint32_t* total = offsets + je->max_blocks;
  const int nchunks = (int)max_chunks((size_t)nb);
  uint32_t* counts = je->d_chunks;
  uint32_t* ff_before = counts + max_chunks(je->max_blocks);
  uint32_t* ff_total = ff_before + max_chunks(je->max_blocks);
  const size_t stream_bytes = (size_t)nb * (kEncMaxBlockBits / 8);
  DMS_HIP(hipMemsetAsync(je->d_words, 0, stream_bytes + 16, stream));
  const unsigned eg = (unsigned)((nb + kEntropyBlock - 1) / kEntropyBlock);
  hipLaunchKernelGGL(k_enc_bits, dim3(eg), dim3(kEntropyBlock), 0, stream, p, je->d_tables, je->d_coef, bits);
  hipLaunchKernelGGL(dms::k_scan_blocks, dim3(1), dim3(1024), 0, stream, bits, offsets, nb, total, 0xffffffffu, (unsigned*)nullptr);
  hipLaunchKernelGGL(k_enc_write, dim3(eg), dim3(kEntropyBlock), 0, stream, p, je->d_tables, je->d_coef, offsets, total, je->d_words);
  const unsigned sg = (unsigned)((nchunks + 255) / 256);
  hipLaunchKernelGGL(k_stuff_count, dim3(sg), dim3(256), 0, stream, je->d_words, total, counts, nchunks);
  hipLaunchKernelGGL(dms::k_scan_blocks, dim3(1), dim3(1024), 0, stream, counts, ff_before, nchunks, ff_total, 0xffffffffu, (unsigned*)nullptr);
  hipLaunchKernelGGL(k_stuff_scatter, dim3(sg), dim3(256), 0, stream, je->d_words, total, ff_before, nchunks, s.d_out + kLenBytes,
                     reinterpret_cast<uint32_t*>(s.d_out));
  DMS_CHECK_LAUNCH();
  // the length and what a frame of this size usually needs; a longer stream's rest is copied when the result is asked for
  const size_t worst = stream_bytes * 2 + 2, usual = (size_t)je->width * je->height / 2 > 65536 ? (size_t)je->width * je->height / 2 : 65536;
  s.eager = worst < usual ? worst : usual;
  DMS_HIP(hipMemcpyAsync(s.pinned, s.d_out, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  DMS_HIP(hipMemcpyAsync(s.pinned + kLenBytes + s.hdr, s.d_out + kLenBytes, s.eager, hipMemcpyDeviceToHost, stream));
  return DMS_OK;
}

// waits for the slot's encode and completes the file in the slot
int finish(dms_jpeg_enc* je, int index, const unsigned char** data, size_t* len) {
  Slot& s = je->slots[(size_t)index];
  if (s.in_flight) {
    DMS_HIP(hipEventSynchronize(s.done));
    s.in_flight = false;
  }
  if (!s.finished && s.on_host >= 0) {
    unsigned char* file = s.pinned + kLenBytes;
    if (s.on_host) {
      s.len = (size_t)s.hdr + enc_entropy_sequential(s.g, reinterpret_cast<const short*>(s.pinned + je->off_coef), je->tables, file + s.hdr);
    } else {
      uint32_t n;
      memcpy(&n, s.pinned, sizeof(n));
      if ((size_t)n > s.eager) DMS_HIP(hipMemcpy(file + s.hdr + s.eager, s.d_out + kLenBytes + s.eager, (size_t)n - s.eager, hipMemcpyDeviceToHost));
      s.len = (size_t)s.hdr + n;
    }
    s.finished = true;
  }
  if (data) *data = s.pinned + kLenBytes;
  if (len) *len = s.len;
  return DMS_OK;
}

}  // namespace

extern "C" {

int dms_jpeg_enc_create(dms_jpeg_enc** out, int max_width, int max_height, int slots) {
  DMS_REQUIRE(out, "null argument");
  DMS_REQUIRE(max_width > 0 && max_height > 0 && max_width <= 65535 && max_height <= 65535, "bad image size");
  DMS_REQUIRE(slots >= 1 && slots <= 16, "slots outside 1 .. 16");
  size_t blocks, planes;
  size_caps(max_width, max_height, &blocks, &planes);
  DMS_REQUIRE(blocks <= 0xffffffffu / kEncMaxBlockBits, "more blocks than a 32-bit bit offset can place");
  dms_jpeg_enc* je = new dms_jpeg_enc();
  je->width = max_width;
  je->height = max_height;
  je->max_px = (size_t)max_width * max_height;
  je->max_blocks = blocks;
  je->max_planes = planes;
  enc_std_tables(&je->tables);
  const size_t stream_bytes = blocks * (kEncMaxBlockBits / 8);
  const size_t file = align16((size_t)kEncHeaderBytes + stream_bytes * 2 + 2 + 16);  // also holds a raw RGB8 frame (3 bytes a pixel)
  je->off_coef = kLenBytes + (file > align16(je->max_px * 3) ? file : align16(je->max_px * 3));
  je->off_depth = je->off_coef + align16(blocks * 64 * sizeof(short));
  je->off_z = je->off_depth + align16(je->max_px * 2);
  je->z_cap = dms_deflate_bound(je->max_px * 2);
  const size_t z_dev = dms::dfl::dev_slot_bytes(je->max_px * 2);  // [length word | the device's stream], whose bound is the larger
  je->slot_bytes = je->off_z + align16(je->z_cap > z_dev ? je->z_cap : z_dev);
  je->out_bytes = kLenBytes + align16(stream_bytes * 2 + 2 + 16);
  je->slots.resize((size_t)slots);
  auto fail = [&](hipError_t e, const char* what) {
    free_all(je);
    return dms::hip_fail(e, what, __FILE__, __LINE__);
  };
  hipError_t e;
  for (Slot& s : je->slots) {
    if ((e = hipHostMalloc((void**)&s.pinned, je->slot_bytes, hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc");
    if ((e = hipMalloc((void**)&s.d_out, je->out_bytes)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  }
  if ((e = hipEventCreateWithFlags(&je->last_done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreateWithFlags(&je->depth_done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipMalloc((void**)&je->d_planes, planes)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&je->d_coef, blocks * 64 * sizeof(short))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&je->d_bits, (2 * blocks + 4) * sizeof(uint32_t))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&je->d_words, stream_bytes + 32)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&je->d_chunks, (2 * max_chunks(blocks) + 4) * sizeof(uint32_t))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMalloc((void**)&je->d_tables, sizeof(EncTables))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMemcpy(je->d_tables, &je->tables, sizeof(EncTables), hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
  *out = je;
  return DMS_OK;
}

int dms_jpeg_enc_destroy(dms_jpeg_enc* je) {
  if (!je) return DMS_OK;
  if (je->any) (void)hipEventSynchronize(je->last_done);
  return free_all(je);
}

int dms_jpeg_enc_set_image_size(dms_jpeg_enc* je, int width, int height) {
  DMS_REQUIRE(je, "null argument");
  DMS_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "bad image size");
  size_t blocks, planes;
  size_caps(width, height, &blocks, &planes);
  DMS_REQUIRE(blocks <= je->max_blocks && planes <= je->max_planes && (size_t)width * height <= je->max_px,
              "larger than the size the encoder was created for");
  je->width = width;
  je->height = height;
  return DMS_OK;
}

int dms_jpeg_enc_set_entropy_on_host(dms_jpeg_enc* je, int on) {
  DMS_REQUIRE(je, "null argument");
  je->writers_on_host = on ? 1 : 0;
  return DMS_OK;
}

int dms_jpeg_enc_set_depth_on_device(dms_jpeg_enc* je, int on) {
  DMS_REQUIRE(je, "null argument");
  je->depth_on_device = on ? 1 : 0;
  return DMS_OK;
}

int dms_jpeg_enc_encode(dms_jpeg_enc* je, const void* rgb_dev, int quality, int subsampling, int flipColors, int entropy_on_host, dms_stream stream) {
  DMS_REQUIRE(je, "null argument");
  if (!encode_args_ok("dms_jpeg_enc_encode", rgb_dev, quality, subsampling)) return DMS_ERR_INVALID_ARG;
  int index;
  int rc = acquire(je, (hipStream_t)stream, &index);
  if (rc) return rc;
  rc = enqueue(je, index, rgb_dev, quality, subsampling, flipColors, entropy_on_host, (hipStream_t)stream);
  const int rr = release(je, index, (hipStream_t)stream);
  return rc ? rc : rr;
}

int dms_jpeg_enc_result_at(dms_jpeg_enc* je, int back, const unsigned char** data, size_t* len) {
  DMS_REQUIRE(je && data && len, "null argument");
  const int n = (int)je->slots.size();
  DMS_REQUIRE(back >= 0 && back < n, "further back than the ring has slots");
  const int index = ((je->next - 1 - back) % n + n) % n;
  DMS_REQUIRE(je->slots[(size_t)index].used && je->slots[(size_t)index].on_host >= 0, "no encode in that slot");
  return finish(je, index, data, len);
}

int dms_jpeg_enc_result(dms_jpeg_enc* je, const unsigned char** data, size_t* len) { return dms_jpeg_enc_result_at(je, 0, data, len); }

int dms_frame_pack_device(dms_jpeg_enc* je, const unsigned short* depth_dev, const unsigned char* rgb_dev, int width, int height, int compressed,
                          int quality, int64_t timestamp, int32_t frameNumber, const char* senderName, dms_frame_msg* m, dms_stream stream) {
  DMS_REQUIRE(je && depth_dev && rgb_dev && m, "null argument");
  DMS_REQUIRE(width == je->width && height == je->height, "the encoder is set to another image size");
  if (compressed && !encode_args_ok("dms_frame_pack_device", rgb_dev, quality, DMS_JPEG_420)) return DMS_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t px = (size_t)width * height;
  const bool z_dev = compressed && je->depth_on_device;
  if (z_dev && !je->dd) {
    const int rc = dms_deflate_dev_create(&je->dd, je->max_px * 2, (int)je->slots.size());
    if (rc) return rc;
  }
  int index;
  int rc = acquire(je, st, &index);
  if (rc) return rc;
  Slot& s = je->slots[(size_t)index];
  unsigned char* depth = s.pinned + je->off_depth;
  auto work = [&]() -> int {
    if (z_dev) {
      const int rc = dms::dfl::dev_enqueue(je->dd, index, depth_dev, px * 2, st, s.pinned + je->off_z, &s.z_eager);
      return rc ? rc : enqueue(je, index, rgb_dev, quality, DMS_JPEG_420, 0, je->writers_on_host, st);
    }
    DMS_HIP(hipMemcpyAsync(depth, depth_dev, px * 2, hipMemcpyDeviceToHost, st));
    if (!compressed) {
      DMS_HIP(hipMemcpyAsync(s.pinned + kLenBytes, rgb_dev, px * 3, hipMemcpyDeviceToHost, st));
      return DMS_OK;
    }
    DMS_HIP(hipEventRecord(je->depth_done, st));
    return enqueue(je, index, rgb_dev, quality, DMS_JPEG_420, 0, je->writers_on_host, st);
  };
  rc = work();
  const int rr = release(je, index, st);
  if (rc || rr) return rc ? rc : rr;
  memset(m, 0, sizeof(*m));
  m->compressed = compressed ? 1 : 0;
  m->timestamp = timestamp;
  m->frameNumber = frameNumber;
  if (senderName) strncpy(m->senderName, senderName, sizeof(m->senderName) - 1);
  const unsigned char* image = nullptr;
  size_t image_len = 0;
  if (z_dev) {
    rc = finish(je, index, &image, &image_len);
    if (rc) return rc;
    const unsigned char* z = nullptr;
    size_t zn = 0;
    rc = dms::dfl::dev_finish(je->dd, index, s.pinned + je->off_z, s.z_eager, &z, &zn);
    if (rc) return rc;
    m->depth = z;
    m->depthSize = (int32_t)zn;
  } else if (compressed) {
    // the depth is in the slot before the colour kernels have run: deflate it meanwhile
    DMS_HIP(hipEventSynchronize(je->depth_done));
    size_t zn = 0;
    rc = dms_deflate(depth, px * 2, s.pinned + je->off_z, je->z_cap, &zn);
    if (rc) return rc;
    m->depth = s.pinned + je->off_z;
    m->depthSize = (int32_t)zn;
    rc = finish(je, index, &image, &image_len);
    if (rc) return rc;
  } else {
    rc = finish(je, index, &image, nullptr);
    if (rc) return rc;
    m->depth = depth;
    m->depthSize = (int32_t)(px * 2);
    image_len = px * 3;
  }
  m->image = image;
  m->imageSize = (int32_t)image_len;
  return DMS_OK;
}

int dms_klg_writer_append_device(dms_klg_writer* w, dms_jpeg_enc* je, const unsigned short* depth_dev, const unsigned char* rgb_dev, int64_t timestamp,
                                 int compressed, int quality, dms_stream stream) {
  DMS_REQUIRE(w && je, "null argument");
  dms_frame_msg m;
  const int rc = dms_frame_pack_device(je, depth_dev, rgb_dev, je->width, je->height, compressed, quality, timestamp, 0, "", &m, stream);
  if (rc) return rc;
  return dms_klg_writer_append(w, timestamp, m.depth, m.depthSize, m.image, m.imageSize);
}

int dms_lcmlog_writer_append_frame_device(dms_lcmlog_writer* w, dms_jpeg_enc* je, const char* channel, const unsigned short* depth_dev,
                                          const unsigned char* rgb_dev, int64_t timestamp, int32_t frameNumber, const char* senderName, int compressed,
                                          int quality, dms_stream stream) {
  DMS_REQUIRE(w && je && channel, "null argument");
  dms_frame_msg m;
  int rc = dms_frame_pack_device(je, depth_dev, rgb_dev, je->width, je->height, compressed, quality, timestamp, frameNumber, senderName, &m, stream);
  if (rc) return rc;
  const size_t need = dms_eflcm_frame_encoded_size(&m);
  std::vector<unsigned char> buf(need);
  size_t n = 0;
  rc = dms_eflcm_frame_encode(&m, buf.data(), buf.size(), &n);
  if (rc) return rc;
  return dms_lcmlog_writer_append(w, timestamp, channel, buf.data(), n);
}

}  // extern "C"
