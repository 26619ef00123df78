// Surfel map: storage, bootstrap from the first frame (G3+G4), index map (G5), splat
// prediction (G6, G6').
//
// The reference renders the map through OpenGL (one point per surfel, depth-tested MRT).
// Here every "draw" is two HBM passes:
//   pass 1 (one thread per surfel): cull, project, and fight for each covered pixel with a
//          64-bit atomicMin on key = depth24 << 32 | surfel id — GL_LESS on a 24-bit depth
//          buffer with first-drawn-wins ties is exactly "smallest key";
//   pass 2 (one thread per pixel): decode the winner and recompute its attributes.
// Pass 1 streams only the position/normal planes; the colour plane is touched for winners only.
#include <vector>

#include "exact_arith.hpp"
#include "scan.hpp"
#include "smallmath.hpp"
#include "surfel.hpp"
#include "fill.hpp"
#include "internal.hpp"
#include "splat_project.hpp"
#include "host_util.hpp"
#include "track_init.hpp"
#include "model_bodies.hpp"

namespace dms {

// ---------------------------------------------------------------------------------------
// storage
// ---------------------------------------------------------------------------------------
static void model_layout(dms_model* m, Carver& c) {
  for (int b = 0; b < 2; ++b) {
    m->buf[b].pos = c.take<float4>(m->cap);
    m->buf[b].col = c.take<float4>(m->cap);
    m->buf[b].nrm = c.take<float4>(m->cap);
    m->buf[b].times = c.take<float>(m->cap * DMS_MAX_SENSORS);
  }
  m->d_count = c.take<unsigned>(8);
  m->d_count_alt = m->d_count ? m->d_count + 4 : nullptr;
  m->slot_pos = c.take<float4>(m->slots);
  m->slot_col = c.take<float4>(m->slots);
  m->slot_nrm = c.take<float4>(m->slots);
  m->slot_best = c.take<unsigned>(m->slots);
  m->slot_flag = c.take<unsigned char>(m->slots);
  m->winner = c.take<unsigned>(m->cap);
  const size_t total = m->cap + (size_t)m->width * m->height;  // clean: cap + slots; bootstrap: W*H
  m->keep = c.take<unsigned char>(total);
  m->block_count = c.take<unsigned>(total / kScanChunk + 2);
  m->block_offset = c.take<unsigned>(total / kScanChunk + 2);
  m->clean_first = c.take<unsigned>(4);
  m->nodes = c.take<float>((size_t)m->max_nodes * 16);
}

__global__ void k_fill_u32(unsigned* p, size_t n, unsigned v) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)blockDim.x * gridDim.x) p[i] = v;
}

}  // namespace dms

using namespace dms;

extern "C" {

int dms_model_create(dms_model** out, size_t capacity, int width, int height) {
  DMS_REQUIRE(out && width >= 16 && height >= 16, "bad argument");
  dms_model* m = new dms_model();
  m->cap = capacity ? capacity : (size_t)5700 * 5700;  // GlobalModel::MAX_VERTICES
  m->width = width;
  m->height = height;
  m->slot_h = (height + 1) / 2;
  m->slots = ((width + 1) / 2) * m->slot_h;
  Carver sz;
  model_layout(m, sz);
  m->arena_bytes = up256(sz.off);
  hipError_t e = hipMalloc((void**)&m->arena, m->arena_bytes);
  if (e != hipSuccess) {
    delete m;
    return hip_fail(e, "hipMalloc(model)", __FILE__, __LINE__);
  }
  Carver c;
  c.base = m->arena;
  model_layout(m, c);
  e = hipHostMalloc((void**)&m->h_count, 8 * sizeof(unsigned), hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipFree(m->arena);
    delete m;
    return hip_fail(e, "hipHostMalloc", __FILE__, __LINE__);
  }
  DMS_HIP(hipMemset(m->d_count, 0, 8 * sizeof(unsigned)));
  DMS_HIP(hipMemset(m->slot_flag, 0, (size_t)m->slots));  // no measurement is parked: a clean before the first fuse appends nothing
  hipLaunchKernelGGL(k_fill_u32, dim3(1024), dim3(256), 0, 0, m->winner, m->cap, kEmptyWinner);
  DMS_CHECK_LAUNCH();
  for (int b = 0; b < 2; ++b) {  // every time plane of both buffers: -3.0f, "never seen by this sensor" (surfel.hpp, live_planes)
    hipLaunchKernelGGL(k_fill_u32, dim3(2048), dim3(256), 0, 0, (unsigned*)m->buf[b].times, m->cap * DMS_MAX_SENSORS, 0xC0400000u);
    DMS_CHECK_LAUNCH();
  }
  DMS_HIP(hipDeviceSynchronize());
  m->count_upper = 0;
  if (const char* smin = getenv("DMS_CLEAN_SUFFIX_MIN")) m->clean_suffix_min = (size_t)atoll(smin);  // once, at creation
  *out = m;
  return DMS_OK;
}

int dms_model_set_num_sensors(dms_model* m, int num_sensors) {
  DMS_REQUIRE(m, "null argument");
  DMS_REQUIRE(num_sensors >= 1 && num_sensors <= DMS_MAX_SENSORS, "num_sensors out of range");
  m->num_sensors = num_sensors;
  return DMS_OK;
}

int dms_model_set_clean_suffix_min(dms_model* m, size_t surfels) {
  DMS_REQUIRE(m, "null argument");
  m->clean_suffix_min = surfels;
  return DMS_OK;
}

int dms_model_destroy(dms_model* m) {
  if (!m) return DMS_OK;
  if (m->arena) (void)hipFree(m->arena);
  if (m->h_count) (void)hipHostFree(m->h_count);
  delete m;
  return DMS_OK;
}

size_t dms_model_capacity(dms_model* m) { return m ? m->cap : 0; }
size_t dms_model_count_bound(dms_model* m) { return m ? m->count_upper : 0; }

int dms_model_count(dms_model* m, unsigned int* count, dms_stream s) {
  DMS_REQUIRE(m && count, "null argument");
  DMS_HIP(hipMemcpyAsync(m->h_count, m->d_count, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)s));
  DMS_HIP(hipStreamSynchronize((hipStream_t)s));
  *count = m->h_count[0];
  m->count_upper = *count;
  return DMS_OK;
}

static int model_download_planes(dms_model* m, unsigned n, std::vector<float4>& pos, std::vector<float4>& col, std::vector<float4>& nrm,
                                 std::vector<float>& times, hipStream_t s) {
  const SurfelPlanes& b = m->buf[m->cur];
  pos.resize(n);
  col.resize(n);
  nrm.resize(n);
  times.resize((size_t)n * DMS_MAX_SENSORS);
  if (n == 0) return DMS_OK;
  DMS_HIP(hipMemcpyAsync(pos.data(), b.pos, n * sizeof(float4), hipMemcpyDeviceToHost, s));
  DMS_HIP(hipMemcpyAsync(col.data(), b.col, n * sizeof(float4), hipMemcpyDeviceToHost, s));
  DMS_HIP(hipMemcpyAsync(nrm.data(), b.nrm, n * sizeof(float4), hipMemcpyDeviceToHost, s));
  for (int k = 0; k < DMS_MAX_SENSORS; ++k)
    DMS_HIP(hipMemcpyAsync(times.data() + (size_t)k * n, b.times + (size_t)k * m->cap, n * sizeof(float), hipMemcpyDeviceToHost, s));
  DMS_HIP(hipStreamSynchronize(s));
  return DMS_OK;
}


static int model_download_any(dms_model* m, float* host, unsigned max_count, unsigned* count, int nsens, bool ref_layout,
                              hipStream_t s) {
  DMS_REQUIRE(m && host && count, "null argument");
  unsigned n = 0;
  int rc = model_flush_pending(m, s);
  if (!rc) rc = dms_model_count(m, &n, s);
  if (rc) return rc;
  if (n > max_count) n = max_count;
  std::vector<float4> pos, col, nrm;
  std::vector<float> times;
  if ((rc = model_download_planes(m, n, pos, col, nrm, times, s))) return rc;
  const int stride = 12 + nsens;
  for (unsigned i = 0; i < n; ++i) {
    float* r = host + (size_t)i * stride;
    r[0] = pos[i].x; r[1] = pos[i].y; r[2] = pos[i].z; r[3] = pos[i].w;
    r[4] = col[i].x; r[5] = col[i].y; r[6] = col[i].z; r[7] = col[i].w;
    if (ref_layout) {  // Shaders/Vertex.cpp:21-50: times sit between colour and normal
      for (int k = 0; k < nsens; ++k) r[8 + k] = times[(size_t)k * n + i];
      r[8 + nsens] = nrm[i].x; r[9 + nsens] = nrm[i].y; r[10 + nsens] = nrm[i].z; r[11 + nsens] = nrm[i].w;
    } else {
      r[8] = nrm[i].x; r[9] = nrm[i].y; r[10] = nrm[i].z; r[11] = nrm[i].w;
      for (int k = 0; k < nsens; ++k) r[12 + k] = times[(size_t)k * n + i];
    }
  }
  *count = n;
  return DMS_OK;
}

static int model_upload_any(dms_model* m, const float* host, unsigned n, int nsens, bool ref_layout, hipStream_t s) {
  DMS_REQUIRE(m && (host || n == 0), "null argument");
  m->pending_update = false;  // (the map is replaced: a deferred update of the old one has nothing left to update)
  if (n > m->cap) {
    set_error("dms_model_upload: %u surfels exceed capacity %zu", n, m->cap);
    return DMS_ERR_CAPACITY;
  }
  std::vector<float4> pos(n), col(n), nrm(n);
  std::vector<float> times((size_t)n * DMS_MAX_SENSORS, -3.0f);
  const int stride = 12 + nsens;
  for (unsigned i = 0; i < n; ++i) {
    const float* r = host + (size_t)i * stride;
    pos[i] = make_float4(r[0], r[1], r[2], r[3]);
    col[i] = make_float4(r[4], r[5], r[6], r[7]);
    if (ref_layout) {
      for (int k = 0; k < nsens; ++k) times[(size_t)k * n + i] = r[8 + k];
      nrm[i] = make_float4(r[8 + nsens], r[9 + nsens], r[10 + nsens], r[11 + nsens]);
    } else {
      nrm[i] = make_float4(r[8], r[9], r[10], r[11]);
      for (int k = 0; k < nsens; ++k) times[(size_t)k * n + i] = r[12 + k];
    }
  }
  for (int k = DMS_MAX_SENSORS - 1; k >= m->live_planes; --k) {  // the planes the caller's records carry times in (surfel.hpp, live_planes)
    bool any = false;
    for (unsigned i = 0; i < n && !any; ++i) any = !(times[(size_t)k * n + i] == -3.0f);
    if (any) {
      m->live_planes = k + 1;
      break;
    }
  }
  const SurfelPlanes& b = m->buf[m->cur];
  if (n) {
    DMS_HIP(hipMemcpyAsync(b.pos, pos.data(), n * sizeof(float4), hipMemcpyHostToDevice, s));
    DMS_HIP(hipMemcpyAsync(b.col, col.data(), n * sizeof(float4), hipMemcpyHostToDevice, s));
    DMS_HIP(hipMemcpyAsync(b.nrm, nrm.data(), n * sizeof(float4), hipMemcpyHostToDevice, s));
    for (int k = 0; k < DMS_MAX_SENSORS; ++k)
      DMS_HIP(hipMemcpyAsync(b.times + (size_t)k * m->cap, times.data() + (size_t)k * n, n * sizeof(float), hipMemcpyHostToDevice, s));
  }
  unsigned cnt = n;
  DMS_HIP(hipMemcpyAsync(m->d_count, &cnt, sizeof(unsigned), hipMemcpyHostToDevice, s));
  DMS_HIP(hipStreamSynchronize(s));
  m->count_upper = n;
  m->count_hold = 3;  // the map was replaced from outside: older frame results no longer bound it
  m->version += 1;
  return DMS_OK;
}

int dms_model_download_ref(dms_model* m, float* host, unsigned int max_count, unsigned int* count, dms_stream s) {
  return model_download_any(m, host, max_count, count, DMS_REF_MAX_SENSORS, true, (hipStream_t)s);
}
int dms_model_upload_ref(dms_model* m, const float* host, unsigned int count, dms_stream s) {
  return model_upload_any(m, host, count, DMS_REF_MAX_SENSORS, true, (hipStream_t)s);
}
int dms_model_download(dms_model* m, float* host, unsigned int max_count, unsigned int* count, dms_stream s) {
  return model_download_any(m, host, max_count, count, DMS_MAX_SENSORS, false, (hipStream_t)s);
}
int dms_model_upload(dms_model* m, const float* host, unsigned int count, dms_stream s) {
  return model_upload_any(m, host, count, DMS_MAX_SENSORS, false, (hipStream_t)s);
}

int dms_pose_block_set(dms_pose_block* dev, const float* pose16, dms_stream s) {
  DMS_REQUIRE(dev && pose16, "null argument");
  dms_pose_block h;
  memcpy(h.pose, pose16, sizeof(h.pose));
  // Eigen Matrix4f::inverse() (IndexMap.cpp:166 etc.): general 4×4 inverse in float
  sm::inv4t<float>(h.pose, h.t_inv);
  DMS_HIP(hipMemcpyAsync(dev, &h, sizeof(h), hipMemcpyHostToDevice, (hipStream_t)s));
  DMS_HIP(hipStreamSynchronize((hipStream_t)s));
  return DMS_OK;
}

}  // extern "C"

namespace dms {

// ---------------------------------------------------------------------------------------
// G3 + G4: first-frame surfels (vertex_feedback.{vert,geom}, init_unstable.vert)
// ---------------------------------------------------------------------------------------
struct BootArgs {
  const uchar4* rgba;
  const float* depth_raw;       // metric
  const float* depth_filtered;  // metric, filtered
  int cols, rows;
  float cx, cy, ifx, ify;  // cam = (cx, cy, 1/fx, 1/fy), float reciprocals (FeedbackBuffer.cpp:93-96)
  int time, timeIdx;
  float maxDepth;
};

// (fb_vertex / fb_normal, geometry.glsl:19-39, live in surfel.hpp: the cloud draw of render.hip shares them)

// element e = column-major pixel (x = e / rows, y = e % rows): GlobalModel.cpp:100-108 order
__global__ __launch_bounds__(256) void k_boot_flags(BootArgs a, unsigned char* __restrict__ keep, unsigned* __restrict__ block_count) {
  const int n = a.cols * a.rows;
  const int base = blockIdx.x * kScanChunk;
  int cnt = 0;
  for (int k = 0; k < kScanChunk / 256; ++k) {
    const int e = base + k * 256 + threadIdx.x;
    unsigned char f = 0;
    if (e < n) {
      const int px = e / a.rows, py = e - px * a.rows;
      const float z = a.depth_raw[(size_t)py * a.cols + px];
      // vertex_feedback.vert:55-62 + .geom:38: emitted iff 0 < z <= maxDepth
      f = (z > 0.f && !(z > a.maxDepth)) ? 1 : 0;
      keep[e] = f;
    }
    cnt += f;
  }
  const unsigned tot = block_sum_u32(cnt);
  if (threadIdx.x == 0) block_count[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_boot_scatter(BootArgs a, const unsigned char* __restrict__ keep,
                                                      const unsigned* __restrict__ block_offset, SurfelPlanes out, size_t cap) {
  const int n = a.cols * a.rows;
  const int base = blockIdx.x * kScanChunk;
  unsigned running = block_offset[blockIdx.x];
  for (int k = 0; k < kScanChunk / 256; ++k) {
    const int e = base + k * 256 + threadIdx.x;
    const bool f = (e < n) && keep[e];
    unsigned total;
    const unsigned rank = block_exclusive_rank(f, total);
    if (f) {
      const size_t dst = running + rank;
      if (dst < cap) {
        const int px = e / a.rows, py = e - px * a.rows;
        const float tx = uv_coord(px, a.cols), ty = uv_coord(py, a.rows);
        const float x = tx * (float)a.cols, y = ty * (float)a.rows;
        // RAW feedback: position, colour, confidence (GlobalModel.cpp:355-370)
        const f3 vr = fb_vertex(a.depth_raw, a.cols, px, py, x, y, a.cx, a.cy, a.ifx, a.ify);
        // FILTERED feedback: normal + radius (GlobalModel.cpp:372-378)
        const f3 vf = fb_vertex(a.depth_filtered, a.cols, px, py, x, y, a.cx, a.cy, a.ifx, a.ify);
        const f3 nf = fb_normal(a.depth_filtered, a.cols, a.rows, vf, tx, ty, x, y, a.cx, a.cy, a.ifx, a.ify);
        const float rad = surfel_radius(vf.z, nf.z, a.ifx, a.ify);
        const float conf = surfel_confidence(x, y, a.cx, a.cy, 1.0f);
        const uchar4 c = a.rgba[(size_t)py * a.cols + px];
        out.pos[dst] = make_float4(vr.x, vr.y, vr.z, conf);
        // init_unstable.vert:36-39: colour kept, y = 0, z (init time) = 1, w = time stamp
        out.col[dst] = make_float4(encode_color_bytes(c.x, c.y, c.z), 0.f, 1.f, (float)a.time);
        out.nrm[dst] = make_float4(nf.x, nf.y, nf.z, rad);
        for (int s = 0; s < DMS_MAX_SENSORS; ++s) out.times[(size_t)s * cap + dst] = (s == a.timeIdx) ? (float)a.time : -3.f;
      }
    }
    running += total;
  }
}

int model_initialise(dms_model* m, const dms_image2d* rgba, const dms_image2d* dm, const dms_image2d* dmf, const dms_camera* cam, int time,
                     int timeIdx, float maxDepth, hipStream_t s) {
  DMS_REQUIRE(m && rgba && dm && dmf && cam, "null argument");
  DMS_REQUIRE(rgba->cols == m->width && rgba->rows == m->height && dm->cols == m->width && dmf->cols == m->width, "shape mismatch");
  DMS_REQUIRE(timeIdx >= 0 && timeIdx < DMS_MAX_SENSORS, "timeIdx out of range");
  BootArgs a;
  a.rgba = (const uchar4*)rgba->data;
  a.depth_raw = (const float*)dm->data;
  a.depth_filtered = (const float*)dmf->data;
  a.cols = m->width;
  a.rows = m->height;
  a.cx = cam->cx;
  a.cy = cam->cy;
  a.ifx = 1.0f / cam->fx;
  a.ify = 1.0f / cam->fy;
  a.time = time;
  a.timeIdx = timeIdx;
  a.maxDepth = maxDepth;
  const int n = a.cols * a.rows;
  const int nb = (n + kScanChunk - 1) / kScanChunk;
  if (m->live_planes < timeIdx + 1) m->live_planes = timeIdx + 1;
  hipLaunchKernelGGL(k_boot_flags, dim3(nb), dim3(256), 0, s, a, m->keep, m->block_count);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, s, m->block_count, m->block_offset, nb, m->d_count, (unsigned)m->cap, (unsigned*)nullptr);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_boot_scatter, dim3(nb), dim3(256), 0, s, a, m->keep, m->block_offset, m->buf[m->cur], m->cap);
  DMS_CHECK_LAUNCH();
  m->count_upper = (size_t)n < m->cap ? (size_t)n : m->cap;
  m->count_hold = 3;
  m->version += 1;
  return DMS_OK;
}

// ---------------------------------------------------------------------------------------
// G5: index map (index_map.vert:41-67, index_map.frag:31-37)
// ---------------------------------------------------------------------------------------
__global__ void k_clear_zbuf(unsigned long long* z, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) z[i] = kZClear;
}

int clear_zbuf(unsigned long long* zbuf, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_clear_zbuf, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, s, zbuf, n);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

// APPLY: the update pass of the preceding fuse (model_fuse with defer_update) has not run: a surfel that won a measurement
// (winner[i] = its slot) is updated here, by the same function, before it is projected — the index map after a fuse reads
// every surfel anyway, so the separate pass over the slots and its launch are saved.
struct PendingUpdate {
  const float4 *slot_pos, *slot_col, *slot_nrm;
  unsigned* winner;
  int time, timeIdx;
};
template <bool APPLY>
__global__ __launch_bounds__(256) void k_index_project(ProjArgs a, SurfelPlanes sp, size_t cap, const unsigned* __restrict__ d_count,
                                                       unsigned long long* __restrict__ zbuf, PendingUpdate u) {
  const unsigned M = d_count[0];
  const float* Tinv = a.pose->t_inv;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += blockDim.x * gridDim.x) {
    if (APPLY) {
      const unsigned w = u.winner[i];
      if (w != kEmptyWinner) {
        u.winner[i] = kEmptyWinner;  // re-arm for the next frame
        fuse_update_apply(i, w, u.slot_pos, u.slot_col, u.slot_nrm, sp, cap, u.time, u.timeIdx);
      }
    }
    const float4 pc = sp.pos[i];
    const f3 ph = xform_point(Tinv, mk3(pc.x, pc.y, pc.z));
    const float vt = sp.times[(size_t)a.timeIdx * cap + i];
    if (ph.z > a.maxDepth || ph.z < 0.f || (vt != -3.f && (float)a.time - vt > (float)a.timeDelta)) continue;
    float xw, yw, zw;
    if (!project_window(a, ph, xw, yw, zw)) continue;
    const int px = (int)floorf(xw), py = (int)floorf(yw);
    if (px < 0 || py < 0 || px >= a.cols || py >= a.rows) continue;
    const unsigned d = depth24(zw);
    if (d >= 0xFFFFFFu) continue;  // GL_LESS against the cleared depth 1.0
    const unsigned long long key = ((unsigned long long)d << 32) | (unsigned long long)i;
    unsigned long long* cell = zbuf + (a.transposed ? (size_t)px * a.rows + py : (size_t)py * a.cols + px);
    if (key < *cell) atomicMin(cell, key);
  }
}

__global__ __launch_bounds__(256) void k_index_resolve(ProjArgs a, SurfelPlanes sp, size_t cap, unsigned long long* __restrict__ zbuf,
                                                       unsigned* __restrict__ index, float4* __restrict__ vertConf,
                                                       float4* __restrict__ colorTime, float4* __restrict__ normRad, int clear_after,
                                                       unsigned long long* __restrict__ zbuf_also) {
  // p runs over the storage order of the images (row-major, or column-major when a.transposed):
  // the z-buffer uses the same order, so reads and writes are coalesced either way
  const int n = a.cols * a.rows;
  const float* Tinv = a.pose->t_inv;
  for (int p = xcd_block(blockIdx.x, gridDim.x, a.xcd) * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    const unsigned long long key = zbuf[p];
    if (clear_after) zbuf[p] = kZClear;  // hand the z-buffer back empty: the next draw needs no clear launch
    // (the frame step: the z-buffer its fused association read without clearing, index_project / model_fuse; null elsewhere)
    if (zbuf_also) zbuf_also[p] = kZClear;
    unsigned id;
    float4 vc, ct, nr;
    resolve_texel<true>(key, Tinv, sp, cap, a.timeIdx, id, vc, ct, nr);
    index[p] = id;
    vertConf[p] = vc;
    colorTime[p] = ct;
    normRad[p] = nr;
  }
}

// column-major -> row-major copy of an image with `elem`-byte pixels (inspection path only)
template <typename T>
__global__ void k_untranspose(const T* __restrict__ src, T* __restrict__ dst, int cols, int rows) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= cols || y >= rows) return;
  dst[(size_t)y * cols + x] = src[(size_t)x * rows + y];
}

int untranspose(const void* src, void* dst, int cols, int rows, int elem, hipStream_t s) {
  dim3 b(32, 8), g((cols + 31) / 32, (rows + 7) / 8);
  if (elem == 4)
    hipLaunchKernelGGL(k_untranspose<unsigned>, g, b, 0, s, (const unsigned*)src, (unsigned*)dst, cols, rows);
  else if (elem == 16)
    hipLaunchKernelGGL(k_untranspose<float4>, g, b, 0, s, (const float4*)src, (float4*)dst, cols, rows);
  else
    DMS_REQUIRE(false, "elem must be 4 or 16");
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

static int surfel_grid(size_t upper) {
  size_t b = (upper + 255) / 256;
  if (b < 1) b = 1;
  if (b > 4096) b = 4096;
  return (int)b;
}

// The projection half of index_map: zbuf (empty on entry when zclean) receives the depth-tested surfel ids
static int index_project_launch(dms_model* m, const ProjArgs& a, unsigned long long* zbuf, int zclean, hipStream_t s) {
  const int n = m->width * m->height;
  if (!zclean) {
    hipLaunchKernelGGL(k_clear_zbuf, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, s, zbuf, n);
    DMS_CHECK_LAUNCH();
  }
  PendingUpdate u = {m->slot_pos, m->slot_col, m->slot_nrm, m->winner, m->pending_time, m->pending_timeIdx};
  if (m->pending_update) {
    m->pending_update = false;
    hipLaunchKernelGGL(k_index_project<true>, dim3(surfel_grid(m->count_upper)), dim3(256), 0, s, a, m->buf[m->cur], m->cap, m->d_count, zbuf, u);
  } else {
    hipLaunchKernelGGL(k_index_project<false>, dim3(surfel_grid(m->count_upper)), dim3(256), 0, s, a, m->buf[m->cur], m->cap, m->d_count, zbuf, u);
  }
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int index_map(dms_model* m, const MapPass& pass, const IndexMapTargets& t, hipStream_t s) {
  dms_indexmap_out* const out = t.out;
  DMS_REQUIRE(m && pass.pose && pass.cam && t.zbuf && out, "null argument");
  DMS_REQUIRE(pass.timeIdx >= 0 && pass.timeIdx < DMS_MAX_SENSORS, "timeIdx out of range");
  const int W = m->width, H = m->height;
  DMS_REQUIRE(dense_img(out->index, 4, W, H) && dense_img(out->vertConf, 16, W, H) && dense_img(out->colorTime, 16, W, H) &&
                  dense_img(out->normRad, 16, W, H),
              "index-map targets must be dense W×H");
  ProjArgs a;
  fill_proj(a, m, pass);
  a.transposed = t.transposed ? 1 : 0;
  const int n = W * H;
  int rc = index_project_launch(m, a, t.zbuf, t.zclean, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_index_resolve, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, s, a, m->buf[m->cur], m->cap, t.zbuf,
                     (unsigned*)out->index.data, (float4*)out->vertConf.data, (float4*)out->colorTime.data, (float4*)out->normRad.data,
                     t.zclean, t.zbuf_also);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int index_project(dms_model* m, const MapPass& pass, const IndexMapTargets& t, hipStream_t s) {
  DMS_REQUIRE(m && pass.pose && pass.cam && t.zbuf, "null argument");
  DMS_REQUIRE(pass.timeIdx >= 0 && pass.timeIdx < DMS_MAX_SENSORS, "timeIdx out of range");
  ProjArgs a;
  fill_proj(a, m, pass);
  a.transposed = 1;
  return index_project_launch(m, a, t.zbuf, t.zclean, s);
}

// ---------------------------------------------------------------------------------------
// Map merge: GlobalModel::consume (GlobalModel.cpp:898-993) + consume.vert — the
// consuming map keeps its surfels (identity transform) and appends the other map's surfels moved by
// the relative transform: pos = T * (x, y, z, 1) with the confidence kept, normal = mat3(T) * n with
// the radius kept, colour and all per-sensor times unchanged.  The reference re-streams both maps
// through transform feedback into the other buffer; appending in place moves only the consumed
// map.  Sources: another model on this device, or a packed device buffer of 20-float records
// (pos4 col4 nrm4 times8, the dms_model_download layout) as received from another rank.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void consume_store(const SurfelPlanes& dst, size_t cap, size_t at, const float* T, const float4 p, const float4 c,
                                              const float4 n, const float (&tm)[DMS_MAX_SENSORS]) {
  // GLSL `transform * vec4(v, 1)`: row i = ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 (row-major T here)
  const f3 q = xform_point(T, mk3(p.x, p.y, p.z));
  const f3 m = xform_dir(T, mk3(n.x, n.y, n.z));
  dst.pos[at] = make_float4(q.x, q.y, q.z, p.w);
  dst.col[at] = c;
  dst.nrm[at] = make_float4(m.x, m.y, m.z, n.w);
#pragma unroll
  for (int k = 0; k < DMS_MAX_SENSORS; ++k) dst.times[(size_t)k * cap + at] = tm[k];
}

struct Pose16v {
  float v[16];
};

// The consuming map's own records go through consume.vert too, with the identity (GlobalModel.cpp:903-949): every finite value
// comes out as it went in, but a component that is -0 can come out +0 (-0 + 0 * y = +0 for y > 0) — found by running the reference's
// program (tests/test_ref_gl_pin_*.py, stage `consumed`).  One pass over position and normal, in place; the rest is copied as is.
__global__ __launch_bounds__(256) void k_consume_identity(SurfelPlanes dst, const unsigned* __restrict__ dcount) {
  const unsigned n = dcount[0];
  const float I[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) {
    const float4 p = dst.pos[i], nr = dst.nrm[i];
    const f3 q = xform_point(I, mk3(p.x, p.y, p.z));
    const f3 m = xform_dir(I, mk3(nr.x, nr.y, nr.z));
    dst.pos[i] = make_float4(q.x, q.y, q.z, p.w);
    dst.nrm[i] = make_float4(m.x, m.y, m.z, nr.w);
  }
}

__global__ __launch_bounds__(256) void k_consume_model(SurfelPlanes dst, size_t dcap, const unsigned* __restrict__ dcount, unsigned* __restrict__ dcount_new,
                                                       SurfelPlanes src, size_t scap, const unsigned* __restrict__ scount, Pose16v T) {
  const unsigned base = dcount[0], ns = scount[0];
  const unsigned room = base < dcap ? (unsigned)(dcap - base) : 0u;
  const unsigned n = ns < room ? ns : room;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) {
    float tm[DMS_MAX_SENSORS];
#pragma unroll
    for (int k = 0; k < DMS_MAX_SENSORS; ++k) tm[k] = src.times[(size_t)k * scap + i];
    consume_store(dst, dcap, (size_t)base + i, T.v, src.pos[i], src.col[i], src.nrm[i], tm);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) dcount_new[0] = base + n;
}

__global__ __launch_bounds__(256) void k_consume_records(SurfelPlanes dst, size_t dcap, const unsigned* __restrict__ dcount, unsigned* __restrict__ dcount_new,
                                                         const float* __restrict__ rec, unsigned ns, Pose16v T) {
  const unsigned base = dcount[0];
  const unsigned room = base < dcap ? (unsigned)(dcap - base) : 0u;
  const unsigned n = ns < room ? ns : room;
  constexpr int stride = 12 + DMS_MAX_SENSORS;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) {
    const float4* r = reinterpret_cast<const float4*>(rec + (size_t)i * stride);  // 80-byte records: 16-byte aligned
    float tm[DMS_MAX_SENSORS];
#pragma unroll
    for (int k = 0; k < DMS_MAX_SENSORS; k += 4) {
      const float4 t4 = r[3 + k / 4];
      tm[k] = t4.x;
      tm[k + 1] = t4.y;
      tm[k + 2] = t4.z;
      tm[k + 3] = t4.w;
    }
    consume_store(dst, dcap, (size_t)base + i, T.v, r[0], r[1], r[2], tm);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) dcount_new[0] = base + n;
}

// pack the map into 20-float records in a device buffer (the device-side form of dms_model_download)
__global__ __launch_bounds__(256) void k_export_records(SurfelPlanes src, size_t scap, const unsigned* __restrict__ scount, unsigned max_count,
                                                        float* __restrict__ rec, unsigned* __restrict__ written) {
  const unsigned ns = scount[0];
  const unsigned n = ns < max_count ? ns : max_count;
  constexpr int stride = 12 + DMS_MAX_SENSORS;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) {
    float4* r = reinterpret_cast<float4*>(rec + (size_t)i * stride);
    r[0] = src.pos[i];
    r[1] = src.col[i];
    r[2] = src.nrm[i];
#pragma unroll
    for (int k = 0; k < DMS_MAX_SENSORS; k += 4)
      r[3 + k / 4] = make_float4(src.times[(size_t)k * scap + i], src.times[(size_t)(k + 1) * scap + i], src.times[(size_t)(k + 2) * scap + i],
                                 src.times[(size_t)(k + 3) * scap + i]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) written[0] = n;
}

// exact device count -> host bound (synchronises `s`)
static int refresh_count(dms_model* m, hipStream_t s) {
  DMS_HIP(hipMemcpyAsync(m->h_count, m->d_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  DMS_HIP(hipStreamSynchronize(s));
  m->count_upper = m->h_count[0];
  return DMS_OK;
}

static int consume_finish(dms_model* m, size_t added_upper) {
  std::swap(m->d_count, m->d_count_alt);  // the kernel wrote the new count into the other cell
  const size_t upper = m->count_upper + added_upper;
  m->count_upper = upper < m->cap ? upper : m->cap;
  m->count_hold = 3;
  m->version += 1;
  return DMS_OK;
}

// highest time plane (+ 1) in which any record carries something other than the "never seen" marker
__global__ __launch_bounds__(256) void k_records_live_planes(const float* __restrict__ rec, unsigned n, unsigned* __restrict__ out) {
  constexpr int stride = 12 + DMS_MAX_SENSORS;
  unsigned live = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)blockDim.x * gridDim.x)
    for (int k = DMS_MAX_SENSORS - 1; k >= 0; --k)
      if (!(rec[i * stride + 12 + k] == -3.0f)) {
        live = live > (unsigned)(k + 1) ? live : (unsigned)(k + 1);
        break;
      }
  if (live) atomicMax(out, live);
}

static int model_consume(dms_model* dst, const dms_model* src, const float* T16, hipStream_t s) {
  DMS_REQUIRE(dst && src && T16 && dst != src, "bad argument");
  {
    int rc = model_flush_pending(dst, s);
    if (!rc) rc = model_flush_pending(const_cast<dms_model*>(src), s);
    if (rc) return rc;
  }
  if (dst->count_upper + src->count_upper > dst->cap) {
    // the host-side bounds are loose (they grow by a frame's worth of slots per clean): read the exact counts before refusing
    int rc = refresh_count(dst, s);
    if (!rc) rc = refresh_count(const_cast<dms_model*>(src), s);
    if (rc) return rc;
  }
  if (dst->count_upper + src->count_upper > dst->cap) {
    set_error("dms_model_consume: %zu + %zu surfels exceed the capacity %zu", dst->count_upper, src->count_upper, dst->cap);
    return DMS_ERR_CAPACITY;
  }
  Pose16v T;
  memcpy(T.v, T16, sizeof(T.v));
  hipLaunchKernelGGL(k_consume_identity, dim3(surfel_grid(dst->count_upper)), dim3(256), 0, s, dst->buf[dst->cur], dst->d_count);
  hipLaunchKernelGGL(k_consume_model, dim3(surfel_grid(src->count_upper)), dim3(256), 0, s, dst->buf[dst->cur], dst->cap, dst->d_count,
                     dst->d_count_alt, src->buf[src->cur], src->cap, src->d_count, T);
  DMS_CHECK_LAUNCH();
  if (dst->live_planes < src->live_planes) dst->live_planes = src->live_planes;
  return consume_finish(dst, src->count_upper);
}

static int model_consume_records(dms_model* dst, const float* rec_dev, unsigned n, const float* T16, hipStream_t s) {
  DMS_REQUIRE(dst && T16 && (rec_dev || n == 0), "bad argument");
  if (int rc0 = model_flush_pending(dst, s)) return rc0;
  DMS_REQUIRE(((uintptr_t)rec_dev & 15) == 0, "record buffer must be 16-byte aligned");
  if (dst->count_upper + n > dst->cap) {
    const int rc = refresh_count(dst, s);  // loose bound: read the exact count before refusing
    if (rc) return rc;
  }
  if (dst->count_upper + n > dst->cap) {
    set_error("dms_model_consume_records: %zu + %u surfels exceed the capacity %zu", dst->count_upper, n, dst->cap);
    return DMS_ERR_CAPACITY;
  }
  Pose16v T;
  memcpy(T.v, T16, sizeof(T.v));
  hipLaunchKernelGGL(k_consume_identity, dim3(surfel_grid(dst->count_upper)), dim3(256), 0, s, dst->buf[dst->cur], dst->d_count);
  hipLaunchKernelGGL(k_consume_records, dim3(surfel_grid(n)), dim3(256), 0, s, dst->buf[dst->cur], dst->cap, dst->d_count, dst->d_count_alt,
                     rec_dev, n, T);
  DMS_CHECK_LAUNCH();
  if (n && dst->live_planes < DMS_MAX_SENSORS) {  // which time planes the records carry anything in (surfel.hpp, live_planes)
    unsigned* cell = dst->clean_first + 2;
    DMS_HIP(hipMemsetAsync(cell, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_records_live_planes, dim3(surfel_grid(n)), dim3(256), 0, s, rec_dev, n, cell);
    DMS_CHECK_LAUNCH();
    unsigned live = 0;
    DMS_HIP(hipMemcpyAsync(&live, cell, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    DMS_HIP(hipStreamSynchronize(s));
    if (dst->live_planes < (int)live) dst->live_planes = (int)live;
  }
  return consume_finish(dst, n);
}

static int model_export_records(dms_model* m, float* rec_dev, unsigned max_count, unsigned* count_host, hipStream_t s) {
  DMS_REQUIRE(m && rec_dev && count_host, "null argument");
  if (int rc0 = model_flush_pending(m, s)) return rc0;
  DMS_REQUIRE(((uintptr_t)rec_dev & 15) == 0, "record buffer must be 16-byte aligned");
  hipLaunchKernelGGL(k_export_records, dim3(surfel_grid(m->count_upper)), dim3(256), 0, s, m->buf[m->cur], m->cap, m->d_count, max_count,
                     rec_dev, m->d_count_alt + 1);
  DMS_CHECK_LAUNCH();
  DMS_HIP(hipMemcpyAsync(m->h_count, m->d_count_alt + 1, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  DMS_HIP(hipStreamSynchronize(s));
  *count_host = m->h_count[0];
  return DMS_OK;
}

// ---------------------------------------------------------------------------------------
// Deformation::sampleGraphModel, device half (Deformation.cpp:250-348; sample.vert, sample.geom):
// every sampleRate-th surfel as {pos.xyz, init time}, then ordered by init time.  The reference
// downloads the samples and std::sorts them on the host (order of equal times unspecified); here
// the ordering is a stable rank sort on device (ties keep surfel order) and only the sorted rows
// travel.  Scratch: the inactive half of the double-buffered map (free between cleans).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_graph_sample(SurfelPlanes src, const unsigned* __restrict__ d_count, int rate, float4* __restrict__ out,
                                                      unsigned* __restrict__ n_out) {
  const unsigned M = d_count[0];
  const unsigned n = (M + (unsigned)rate - 1u) / (unsigned)rate;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *n_out = n;
  if (i >= n) return;
  const size_t id = (size_t)i * (size_t)rate;  // gl_VertexID % sampleRate == 0
  const float4 p = src.pos[id];
  out[i] = make_float4(p.x, p.y, p.z, src.col[id].z);
}

__global__ __launch_bounds__(256) void k_graph_rank(const float4* __restrict__ in, const unsigned* __restrict__ n_in, float4* __restrict__ out) {
  const unsigned n = *n_in;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ float s_t[256];
  const float ti = i < n ? in[i].w : 0.f;
  unsigned rank = 0;
  for (unsigned base = 0; base < n; base += 256) {
    const unsigned j = base + threadIdx.x;
    s_t[threadIdx.x] = j < n ? in[j].w : 0.f;
    __syncthreads();
    const unsigned lim = min(256u, n - base);
    for (unsigned q = 0; q < lim; ++q) {
      const float tj = s_t[q];
      rank += (tj < ti || (tj == ti && base + q < i)) ? 1u : 0u;
    }
    __syncthreads();
  }
  if (i < n) out[rank] = in[i];
}

int model_sample_graph(dms_model* m, int sampleRate, float* rows4_host, int max_rows, int* n_host, hipStream_t s) {
  DMS_REQUIRE(m && n_host && sampleRate >= 2 && (rows4_host || max_rows == 0), "bad argument");
  if (int rc0 = model_flush_pending(m, s)) return rc0;
  const size_t n_upper = (m->count_upper + (size_t)sampleRate - 1) / (size_t)sampleRate;
  DMS_REQUIRE(2 * n_upper <= m->cap, "sample scratch");
  float4* raw = m->buf[1 - m->cur].pos;
  float4* sorted = raw + n_upper;
  const int nb = (int)((n_upper + 255) / 256);
  *n_host = 0;
  if (nb == 0) return DMS_OK;
  hipLaunchKernelGGL(k_graph_sample, dim3(nb), dim3(256), 0, s, m->buf[m->cur], m->d_count, sampleRate, raw, m->d_count_alt + 1);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_graph_rank, dim3(nb), dim3(256), 0, s, raw, m->d_count_alt + 1, sorted);
  DMS_CHECK_LAUNCH();
  DMS_HIP(hipMemcpyAsync(m->h_count, m->d_count_alt + 1, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  DMS_HIP(hipStreamSynchronize(s));
  const unsigned n = m->h_count[0];
  *n_host = (int)n;
  const unsigned take = n < (unsigned)max_rows ? n : (unsigned)max_rows;
  if (take) DMS_HIP(hipMemcpy(rows4_host, sorted, (size_t)take * sizeof(float4), hipMemcpyDeviceToHost));
  return DMS_OK;
}

// ---------------------------------------------------------------------------------------
// G6 / G6': splat prediction (splat.vert:57-94, combo_splat.frag:35-60, depth_splat.frag:29-46)
// ---------------------------------------------------------------------------------------
// fragment stage at pixel (px, py): ray/disc test.  Returns false on discard.
__device__ __forceinline__ bool splat_fragment(const ProjArgs& a, const SplatSurfel& s, int px, int py, f3& corrected, float& zw) {
  const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;  // gl_FragCoord
  const f3 l = normalized3(mk3((fcx - a.cx) / a.fx, (fcy - a.cy) / a.fy, 1.0f));
  const float k = dot3(s.pos, s.nrm) / dot3(l, s.nrm);
  corrected = mk3(k * l.x, k * l.y, k * l.z);
  const float sqrRad = s.rad * s.rad;  // pow(r, 2)
  const f3 diff = corrected - s.pos;
  if (dot3(diff, diff) > sqrRad) return false;
  zw = (corrected.z / (2.f * a.maxDepth)) + 0.5f;  // gl_FragDepth
  return true;
}

// The project pass over the map (splat_project.hpp: vertex stage, sprite rows, fragments), 256 surfels per block and chunk.
// DUAL: one pass over the map feeds two z-buffers — two predictions of the same map from the same pose that differ in
// the cull only (the frame's final prediction and the next frame's tracking prediction): the vertex stage and the sprite
// loop run once, a fragment competes in the z-buffer of every prediction its surfel survives the cull of.
template <bool DUAL>
__global__ __launch_bounds__(256) void k_splat_project(ProjArgs a, SurfelPlanes sp, size_t cap, const unsigned* __restrict__ d_count,
                                                       unsigned long long* __restrict__ zbuf, SplatSecond b2,
                                                       unsigned long long* __restrict__ zbuf2, ProjectRider rd) {
  // (a project pass that no resolve follows - the deferred final prediction of fusion_frame.hip - is the frame's last kernel:
  // its block 0 carries what the resolve's block 0 would have, before anything else; both counts are 0 otherwise)
  if (blockIdx.x == 0) splat_rider(rd);
  __shared__ SplatTables tb;
  const int t = threadIdx.x;
  const unsigned M = d_count[0];
  const SplatRay ray = splat_ray_consts(a);
  // position and time of the next chunk are fetched while this one is scanned and rasterised: on a large map
  // most chunks are culled as a whole, and their cost would otherwise be one exposed memory round trip each
  float4 pc_next = make_float4(0.f, 0.f, 0.f, 0.f);
  float vt_next = 0.f;
  {
    const unsigned i0 = blockIdx.x * 256u + t;
    if (i0 < M) {
      pc_next = sp.pos[i0];
      vt_next = sp.times[(size_t)a.timeIdx * cap + i0];
    }
  }
  for (unsigned base = blockIdx.x * 256u; base < M; base += gridDim.x * 256u) {
    const unsigned i = base + t;
    const float4 pc = pc_next;
    const float vt = vt_next;
    {
      const unsigned in = i + gridDim.x * 256u;
      if (in < M) {
        pc_next = sp.pos[in];
        vt_next = sp.times[(size_t)a.timeIdx * cap + in];
      }
    }
    int rows_here = 0;
    if (i < M) {
      SplatSurfel s;
      int pass = 1;
      if (splat_vertex(a, pc, sp.nrm + i, vt, s, DUAL ? &b2 : nullptr, &pass)) rows_here = splat_park<DUAL, false>(a, s, pass, 0u, t, tb);
    }
    splat_rows<DUAL, false>(a, ray, rows_here, base, tb, zbuf, zbuf2);
    __syncthreads();  // the parameter tables are rewritten by the next chunk
  }
}

// what a resolved pixel stores, from its winner: the image from the packed colour (RGBA8 render target: round(c * 255)) ...
__device__ __forceinline__ uchar4 resolved_image(float packed) {
  const f3 rgb = decode_color(packed);
  return make_uchar4((unsigned char)f2i_rn(rgb.x * 255.0f), (unsigned char)f2i_rn(rgb.y * 255.0f), (unsigned char)f2i_rn(rgb.z * 255.0f), 255);
}
// ... and the vertex (x, y, z, confidence) and normal (x, y, z, radius) from the fragment's depth z
__device__ __forceinline__ void resolved_geometry(const ProjArgs& a, const SplatSurfel& s, float z, int px, int py, float4& o_v, float4& o_n) {
  const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;
  o_v = make_float4(((fcx - a.cx) * z) * (1.f / a.fx), ((fcy - a.cy) * z) * (1.f / a.fy), z, s.conf);
  o_n = make_float4(s.nrm.x, s.nrm.y, s.nrm.z, s.rad);
}

// FILL: the hole fill-in of the prediction (fill.hpp) for the pixel just resolved — the launch and the re-read of the
// three images that a separate fill-in pass costs are saved; the result-block mirror is done by block 0; for the
// denseEnough decision the threads that own a subsampled pixel count the non-black ones into 16 counters, which the
// consumer of the decision (the model pyramid kernel) sums.  (Taking the decision inside this launch — last block by
// ticket, the subsampled pixels written through — cost the 6 us the separate launch had cost.)
template <bool DEPTH_ONLY, bool FILL>
__global__ __launch_bounds__(256) void k_splat_resolve(ProjArgs a, SurfelPlanes sp, size_t cap, unsigned long long* __restrict__ zbuf,
                                                       uchar4* __restrict__ image, float4* __restrict__ vertex, float4* __restrict__ normal,
                                                       unsigned short* __restrict__ timeImg, float* __restrict__ depthOut, int clear_after,
                                                       FillArgs fa) {
  if (FILL) {
    if (fa.mirror_words > 0 && blockIdx.x == 0 && (int)threadIdx.x < fa.mirror_words) fa.mirror_dst[threadIdx.x] = fa.mirror_src[threadIdx.x];
    if (fa.thumb_block && blockIdx.x == 0) {  // the frame block's pose and tick ride along (k_thumbnails does the same)
      if (fa.thumb_pose_dst && threadIdx.x < 16) fa.thumb_pose_dst[threadIdx.x] = fa.thumb_pose_src[threadIdx.x];
      if (fa.thumb_tick_dst && threadIdx.x == 16) *fa.thumb_tick_dst = fa.thumb_tick;
    }
  }
  // outputs are row-major (the tracker consumes them), the z-buffer is column-major: each wave takes an
  // 8 x 8 pixel tile, lanes running down the columns first, so that a z-buffer access touches 8 full
  // 64-byte lines (instead of 64 lines with a row-major thread map) and every output row of the tile
  // is one 128-byte (float4) run
  const int tiles_y = (a.rows + 7) >> 3, tiles_x = (a.cols + 7) >> 3, ntiles = tiles_x * tiles_y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves_per_block = blockDim.x >> 6;
  for (int t = xcd_block(blockIdx.x, gridDim.x, a.xcd) * waves_per_block + wave; t < ntiles; t += gridDim.x * waves_per_block) {
    const int tx = t / tiles_y, ty = t - tx * tiles_y;
    const int px = tx * 8 + (lane >> 3), py = ty * 8 + (lane & 7);
    if (px >= a.cols || py >= a.rows) continue;
    const int p = py * a.cols + px;
    const unsigned long long key = zbuf[(size_t)px * a.rows + py];
    if (clear_after) zbuf[(size_t)px * a.rows + py] = kZClear;
    bool sampled = false;
    if (FILL) {
      if (fa.dense_cnt) sampled = ((fa.sample_mask[px >> 5] >> (px & 31)) & (fa.sample_mask[64 + (py >> 5)] >> (py & 31)) & 1u) != 0u;
    }
    if ((unsigned)(key >> 32) >= 0xFFFFFFu) {
      if (DEPTH_ONLY) {
        depthOut[p] = 0.f;
      } else {
        image[p] = make_uchar4(0, 0, 0, 0);
        vertex[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        normal[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        timeImg[p] = 0;
        if (FILL) {
          float4 ov, on;
          uchar4 oi;
          fill_pixel_out(fa, px, py, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_uchar4(0, 0, 0, 0), ov, on, oi);
          if (fa.thumb_block) fill_thumb(fa, px, py, ov, on, oi);
        }
      }
      continue;
    }
    const unsigned i = (unsigned)(key & 0xFFFFFFFFull);
    SplatSurfel s;
    splat_vertex(a, sp.pos[i], sp.nrm + i, sp.times[(size_t)a.timeIdx * cap + i], s);
    f3 c;
    float zw;
    splat_fragment(a, s, px, py, c, zw);
    if (DEPTH_ONLY) {
      depthOut[p] = c.z;
      continue;
    }
    const float4 cc = sp.col[i];
    const uchar4 o_img = resolved_image(cc.x);
    image[p] = o_img;
    if (FILL && sampled && o_img.x > 0 && o_img.y > 0 && o_img.z > 0) atomicAdd(fa.dense_cnt + ((px + py) & 15) * 16, 1u);
    float4 o_v, o_n;
    resolved_geometry(a, s, c.z, px, py, o_v, o_n);
    vertex[p] = o_v;
    normal[p] = o_n;
    // time = uint(colTime.z) into a 16-bit unsigned target
    const float tz = cc.z;
    unsigned tv = tz > 0.f ? (unsigned)f2i_rz(tz) : 0u;
    if (tv > 65535u) tv = 65535u;
    timeImg[p] = (unsigned short)tv;
    if (FILL) {
      float4 ov, on;
      uchar4 oi;
      fill_pixel_out(fa, px, py, o_v, o_n, o_img, ov, on, oi);
      if (fa.thumb_block) fill_thumb(fa, px, py, ov, on, oi);
    }
  }
}

// fused_model_prediction: the tracking prediction of a frame whose seven images (pred.image / vertex / normal / time, fill.image /
// vertex / normal) have ONE reader, the tracker's model pyramid kernel (prep.hip: k_model_levels012), resolved straight into that
// kernel's outputs.  Each pixel is resolved and filled as k_splat_resolve<false, true> does it (the same helpers), the source is
// selected as model_level0_body selects it, and level 0 of the model maps (vmap, nmap, float depth, intensity) is stored from the
// registers; neither prediction nor fill-in image is written.  Levels 1 and 2 of vmap / nmap come from the same wave: its 8 x 8
// tile (lane = 8 * column + row) holds 4 x 4 level-1 and 2 x 2 level-2 pixels, gathered by lane shuffles in resize4's operand order -
// no halo, no barrier.  The depth / intensity pyramid (5 x 5 windows) is left to rider blocks of the tracker's SO3 launch, a kernel
// boundary later (track.hip: So3Extra).
//   denseEnough: the source choice depends on the whole resolved image (more than 95 % of the W/20 x H/20 samples non-black), and
// there is no next launch to sum counters in.  Every block takes the decision itself before its tiles: per sample (pm.sample_cells:
// the z-buffer cell of each) the cell, the winner's packed colour, the resolve's own decode and byte test - an integer count, so
// every block gets the bits dense_from_counters gives.  No block waits for another.  For that the SAMPLED cells must outlive the
// launch: no block empties them (clear_after skips them); a rider of the SO3 launch does, from the list of the same cells.
//   NT: threads per block (NT / 64 tiles at a time); the grid is sized so that each wave takes about one tile, as the resolve's.
template <int NT>
__global__ __launch_bounds__(NT) void k_predict_model(ProjArgs a, SurfelPlanes sp, size_t cap, unsigned long long* __restrict__ zbuf, int clear_after,
                                                      FillArgs fa, TrackInitArgs ti, PredictModelArgs pm) {
  // the set-up of the tracker call that follows comes first in the grid, as in the model pyramid kernel (block 0's one-lane state
  // set-up is the longest dependency chain of the launch)
  if ((int)blockIdx.x < ti.blocks) {
    track_init_body((int)blockIdx.x, ti.blocks, (int)threadIdx.x, NT, ti.st, ti.prior, ti.prior_pose16, ti.fx, ti.fy, ti.cx, ti.cy, ti.so3, ti.first_level,
                    ti.sync_words, ti.n_sync, ti.inject_timeout, nullptr);
    return;
  }
  const unsigned b = blockIdx.x - (unsigned)ti.blocks, nres = gridDim.x - (unsigned)ti.blocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kWaves = NT / 64;
  __shared__ int s_cnt[kWaves];
  {
    // (the cells from the list the SO3 rider empties them by.  Computing them here - fill_sample_cell's two float divisions per
    // sample - with four samples per thread in flight at a time was measured slower: DESIGN.md 6)
    int cnt = 0;
    for (int k = (int)threadIdx.x; k < pm.n_cells; k += NT) {
      const unsigned long long key = zbuf[pm.sample_cells[k]];
      if ((unsigned)(key >> 32) < 0xFFFFFFu) {
        const uchar4 c = resolved_image(sp.col[(unsigned)(key & 0xFFFFFFFFull)].x);
        cnt += (c.x > 0 && c.y > 0 && c.z > 0) ? 1 : 0;
      }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) s_cnt[wave] = cnt;
  }
  __syncthreads();
  unsigned tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) tot += (unsigned)s_cnt[w];
  const bool useB = dense_from_count(tot, pm.samples) != 0;
  if (b == 0 && threadIdx.x == 0) *pm.flag_out = useB ? 1 : 0;
  const Pose34 P = load_pose34(pm.pose16);
  const bool xf = pm.pose16 != nullptr;
  const int rows0 = a.rows, rows1 = pm.maps.v[1].rows / 3, cols1 = pm.maps.v[1].cols, rows2 = pm.maps.v[2].rows / 3, cols2 = pm.maps.v[2].cols;
  const int tiles_y = (a.rows + 7) >> 3, tiles_x = (a.cols + 7) >> 3, ntiles = tiles_x * tiles_y;
  for (int t = xcd_block(b, nres, a.xcd) * kWaves + wave; t < ntiles; t += nres * kWaves) {  // (wave-uniform: all 64 lanes reach the shuffles)
    const int tx = t / tiles_y, ty = t - tx * tiles_y;
    const int px = tx * 8 + (lane >> 3), py = ty * 8 + (lane & 7);
    const bool inside = px < a.cols && py < a.rows;
    f3 rv = mk3(0.f, 0.f, 0.f), rn = mk3(0.f, 0.f, 0.f);
    if (inside) {
      const size_t cell = (size_t)px * a.rows + py;
      const unsigned long long key = zbuf[cell];
      if (clear_after) {
        const bool sampled = ((fa.sample_mask[px >> 5] >> (px & 31)) & (fa.sample_mask[64 + (py >> 5)] >> (py & 31)) & 1u) != 0u;
        if (!sampled) zbuf[cell] = kZClear;
      }
      float4 o_v = make_float4(0.f, 0.f, 0.f, 0.f), o_n = make_float4(0.f, 0.f, 0.f, 0.f);
      uchar4 o_img = make_uchar4(0, 0, 0, 0);
      if ((unsigned)(key >> 32) < 0xFFFFFFu) {
        const unsigned i = (unsigned)(key & 0xFFFFFFFFull);
        SplatSurfel s;
        splat_vertex(a, sp.pos[i], sp.nrm + i, sp.times[(size_t)a.timeIdx * cap + i], s);
        f3 c;
        float zw;
        splat_fragment(a, s, px, py, c, zw);
        o_img = resolved_image(sp.col[i].x);
        resolved_geometry(a, s, c.z, px, py, o_v, o_n);
      }
      if (useB) {  // (the fill-in images had no other reader: a dense view needs neither the depth nor the colour frame)
        float4 ov, on;
        uchar4 oi;
        fill_pixel_values(fa, px, py, o_v, o_n, o_img, ov, on, oi);
        o_v = ov;
        o_n = on;
        o_img = oi;
      }
      model_level0_store(px, py, rows0, o_v, o_n, o_img, P, xf, pm.maps.v[0], pm.maps.n[0], pm.maps.depth0, pm.maps.inten0, pm.maps.cutOff, rv, rn);
    }
    // level 1: the lane at an even column and an even row of the tile gathers (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1) = lanes
    // + 0, + 8, + 1, + 9; level 2 from the UNTRANSFORMED level-1 values two columns / rows apart, as model_levels12_body forms it
    f3 qv[4], qn[4], lv, ln;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int src = (lane & ~9) + (j & 1) * 8 + (j >> 1);
      qv[j] = mk3(__shfl(rv.x, src, 64), __shfl(rv.y, src, 64), __shfl(rv.z, src, 64));
      qn[j] = mk3(__shfl(rn.x, src, 64), __shfl(rn.y, src, 64), __shfl(rn.z, src, 64));
    }
    model_level_down(qv, qn, lv, ln);
    const int x1 = px >> 1, y1 = py >> 1;
    if ((lane & 9) == 0 && x1 < cols1 && y1 < rows1) store_transformed(pm.maps.v[1], pm.maps.n[1], rows1, y1, x1, lv, ln, P, xf);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int src = (lane & ~27) + (j & 1) * 16 + (j >> 1) * 2;
      qv[j] = mk3(__shfl(lv.x, src, 64), __shfl(lv.y, src, 64), __shfl(lv.z, src, 64));
      qn[j] = mk3(__shfl(ln.x, src, 64), __shfl(ln.y, src, 64), __shfl(ln.z, src, 64));
    }
    const int x2 = px >> 2, y2 = py >> 2;
    if ((lane & 27) == 0 && x2 < cols2 && y2 < rows2) {  // then all four level-1 pixels exist
      f3 v2, n2;
      model_level_down(qv, qn, v2, n2);
      store_transformed(pm.maps.v[2], pm.maps.n[2], rows2, y2, x2, v2, n2, P, xf);
    }
  }
}

int check_map_pass(const dms_model* m, const MapPass& pass, const ProjectRider& rider) {
  DMS_REQUIRE(m && pass.pose && pass.cam, "null argument");
  DMS_REQUIRE(!m->pending_update, "a deferred update pass is still pending (index_map applies it)");
  DMS_REQUIRE(pass.timeIdx >= 0 && pass.timeIdx < DMS_MAX_SENSORS, "timeIdx out of range");
  // (the project pass divides by fx, fy and 2 maxDepth through exact_arith.hpp: normal numbers far from the ends of the exponent range)
  const float fx = pass.cam->fx, fy = pass.cam->fy;
  DMS_REQUIRE(fabsf(fx) > 1e-18f && fabsf(fx) < 1e18f && fabsf(fy) > 1e-18f && fabsf(fy) < 1e18f && pass.maxDepth > 1e-18f && pass.maxDepth < 1e18f,
              "focal lengths and depth cut-off must be finite, non-zero and within 1e-18 .. 1e18");
  DMS_REQUIRE(rider.mirror_words >= 0 && rider.mirror_words <= 256 && rider.copy_words >= 0 && rider.copy_words <= 256 &&
                  (rider.mirror_words == 0 || (rider.mirror_src && rider.mirror_dst)) && (rider.copy_words == 0 || (rider.copy_src && rider.copy_dst)),
              "a rider copies at most 256 dwords (one block)");
  return DMS_OK;
}

int splat_predict(dms_model* m, const MapPass& pass, const SplatPrediction& p, hipStream_t s) {
  const FillArgs* const fill = p.fill;
  const TrackInitArgs* const init = p.init;
  const PredictModelArgs* const pm = p.pm;
  dms_predict_out* const out = p.out;
  dms_image2d* const depth_out = p.depth_out;
  unsigned long long* const zbuf = p.zbuf;
  const int zclean = p.zclean;
  DMS_REQUIRE(m && zbuf && (p.mode != SplatMode::dual || p.zbuf2), "null argument");
  DMS_REQUIRE(!pm || (fill && !depth_out && fill->sample_mask && fill->mirror_words == 0 && !fill->thumb_block && zclean && pm->sample_cells && pm->n_cells == pm->samples &&
                      pm->samples == (m->width / 20) * (m->height / 20) && pm->samples > 0 && pm->flag_out && (pm->threads == 256 || pm->threads == 512 || pm->threads == 1024)),
              "the fused prediction + model pass takes the place of the fused resolve + fill-in pass of a tracking prediction only");
  DMS_REQUIRE(!init || init->blocks == 0 || pm, "the tracker set-up rides on the fused prediction + model pass only");
  if (int rc = check_map_pass(m, pass, kNoRider)) return rc;
  const int W = m->width, H = m->height;
  if (depth_out)
    DMS_REQUIRE(dense_img(*depth_out, 4, W, H), "depth target must be dense W×H f32");
  else
    DMS_REQUIRE(out && dense_img(out->image, 4, W, H) && dense_img(out->vertex, 16, W, H) && dense_img(out->normal, 16, W, H) &&
                    dense_img(out->time, 2, W, H),
                "prediction targets must be dense W×H");
  ProjArgs a;
  fill_proj(a, m, pass);
  const int n = W * H;
  if (!zclean) {
    hipLaunchKernelGGL(k_clear_zbuf, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, s, zbuf, n);
    DMS_CHECK_LAUNCH();
  }
  const SplatSecond no_second = {0.f, 0, 0};
  switch (p.mode) {
    case SplatMode::resolve_only:
      break;
    case SplatMode::dual:
      hipLaunchKernelGGL(k_splat_project<true>, dim3(surfel_grid(m->count_upper)), dim3(256), 0, s, a, m->buf[m->cur], m->cap, m->d_count, zbuf,
                         p.second, p.zbuf2, kNoRider);
      break;
    case SplatMode::project_resolve:
      hipLaunchKernelGGL(k_splat_project<false>, dim3(surfel_grid(m->count_upper)), dim3(256), 0, s, a, m->buf[m->cur], m->cap, m->d_count, zbuf,
                         no_second, (unsigned long long*)nullptr, kNoRider);
      break;
  }
  DMS_CHECK_LAUNCH();
  const FillArgs no_fill = {};
  TrackInitArgs no_init;
  memset(&no_init, 0, sizeof(no_init));
  const dim3 rg(min((n + 255) / 256, 2048));
  if (depth_out) {
    hipLaunchKernelGGL((k_splat_resolve<true, false>), rg, dim3(256), 0, s, a, m->buf[m->cur], m->cap, zbuf, (uchar4*)nullptr,
                       (float4*)nullptr, (float4*)nullptr, (unsigned short*)nullptr, (float*)depth_out->data, zclean, no_fill);
  } else if (pm) {
    DMS_REQUIRE(fill->cols == W && fill->rows == H && W <= 2048 && H <= 2048 && pm->maps.v[0].cols == W && pm->maps.v[0].rows == 3 * H &&
                    pm->maps.v[1].cols == W / 2 && pm->maps.v[1].rows == 3 * (H / 2) && pm->maps.v[2].cols == W / 4 && pm->maps.v[2].rows == 3 * (H / 4),
                "model maps do not describe this prediction's pyramid");
    const TrackInitArgs& ti = (init && init->blocks > 0) ? *init : no_init;
    const int waves = pm->threads / 64, ntiles = ((W + 7) / 8) * ((H + 7) / 8);
    const dim3 g(ti.blocks + min((ntiles + waves - 1) / waves, 2048));
    if (pm->threads == 1024)
      hipLaunchKernelGGL(k_predict_model<1024>, g, dim3(1024), 0, s, a, m->buf[m->cur], m->cap, zbuf, zclean, *fill, ti, *pm);
    else if (pm->threads == 512)
      hipLaunchKernelGGL(k_predict_model<512>, g, dim3(512), 0, s, a, m->buf[m->cur], m->cap, zbuf, zclean, *fill, ti, *pm);
    else
      hipLaunchKernelGGL(k_predict_model<256>, g, dim3(256), 0, s, a, m->buf[m->cur], m->cap, zbuf, zclean, *fill, ti, *pm);
  } else if (fill) {
    DMS_REQUIRE(fill->ex_image == (const uchar4*)out->image.data && fill->ex_vertex == (const float4*)out->vertex.data &&
                    fill->ex_normal == (const float4*)out->normal.data && fill->cols == W && fill->rows == H &&
                    (!fill->dense_cnt || (fill->sample_mask && W <= 2048 && H <= 2048)) && fill->mirror_words <= 256,
                "fill-in arguments do not describe this prediction");
    hipLaunchKernelGGL((k_splat_resolve<false, true>), rg, dim3(256), 0, s, a, m->buf[m->cur], m->cap, zbuf, (uchar4*)out->image.data,
                       (float4*)out->vertex.data, (float4*)out->normal.data, (unsigned short*)out->time.data, (float*)nullptr, zclean, *fill);
  } else {
    hipLaunchKernelGGL((k_splat_resolve<false, false>), rg, dim3(256), 0, s, a, m->buf[m->cur], m->cap, zbuf, (uchar4*)out->image.data,
                       (float4*)out->vertex.data, (float4*)out->normal.data, (unsigned short*)out->time.data, (float*)nullptr, zclean, no_fill);
  }
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int splat_project_only(dms_model* m, const MapPass& pass, unsigned long long* zbuf, const ProjectRider& rider, hipStream_t s) {
  DMS_REQUIRE(m && zbuf, "null argument");
  if (int rc = check_map_pass(m, pass, rider)) return rc;
  ProjArgs a;
  fill_proj(a, m, pass);
  const SplatSecond no_second = {0.f, 0, 0};
  hipLaunchKernelGGL(k_splat_project<false>, dim3(surfel_grid(m->count_upper)), dim3(256), 0, s, a, m->buf[m->cur], m->cap, m->d_count, zbuf,
                     no_second, (unsigned long long*)nullptr, rider);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

}  // namespace dms

extern "C" {
int dms_model_consume(dms_model* dst, const dms_model* src, const float* relativeTransform16, dms_stream s) {
  return dms::model_consume(dst, src, relativeTransform16, (hipStream_t)s);
}
int dms_model_consume_records(dms_model* dst, const float* records_dev, unsigned int count, const float* relativeTransform16, dms_stream s) {
  return dms::model_consume_records(dst, records_dev, count, relativeTransform16, (hipStream_t)s);
}
int dms_model_export_records(dms_model* m, float* records_dev, unsigned int max_count, unsigned int* count, dms_stream s) {
  return dms::model_export_records(m, records_dev, max_count, count, (hipStream_t)s);
}
}
