// The project pass of the splat prediction (G6: splat.vert:57-94, combo_splat.frag:35-60) as device functions: the vertex stage,
// the sprite-row hand-out and the fragment loop.  Two kernels are built from them - k_splat_project (fusion_map.hip), which reads
// the map, and k_clean_scatter_project (fusion_fuse.hip), which projects the clean's survivors from the registers that have just
// stored them.  Both go through the same functions with contraction off, so a surfel yields the same keys in either.
#pragma once
#include "exact_arith.hpp"
#include "internal.hpp"
#include "surfel.hpp"

namespace dms {

struct ProjArgs {
  const dms_pose_block* pose;
  float cx, cy, fx, fy;
  float colsf, rowsf;
  int cols, rows;
  float maxDepth;
  int time, timeIdx, timeDelta;
  // splat only
  float confThreshold;
  int maxTime;
  int actv;
  // index map only: 1 = images stored column-major (pixel (x, y) at x * rows + y).  The fusion
  // consumers walk the image by columns (the reference's draw order, GlobalModel.cpp:100-108),
  // so this is the layout that makes their 16-byte gathers coalesce.
  int transposed;
  int xcd;  // XCD-aware block order of the per-pixel passes (common.hpp xcd_block)
};

// (the index-map kernels read none of the splat-only fields)
static inline void fill_proj(ProjArgs& a, const dms_model* m, const MapPass& p) {
  a.pose = p.pose;
  a.cx = p.cam->cx;
  a.cy = p.cam->cy;
  a.fx = p.cam->fx;
  a.fy = p.cam->fy;
  a.cols = m->width;
  a.rows = m->height;
  a.colsf = (float)m->width;
  a.rowsf = (float)m->height;
  a.maxDepth = p.maxDepth;
  a.time = p.time;
  a.timeIdx = p.timeIdx;
  a.timeDelta = p.timeDelta;
  a.confThreshold = p.confThreshold;
  a.maxTime = p.maxTime;
  a.actv = p.active ? 1 : 0;
  a.transposed = 0;
  a.xcd = xcd_remap_enabled();
}

// window position of a camera-frame point through the shader's NDC arithmetic
// (index_map.vert:56-57 / splat.vert:37-42) and the viewport transform xw = (x_ndc + 1) * (W/2).
__device__ __forceinline__ bool project_window(const ProjArgs& a, const f3& p, float& xw, float& yw, float& zw) {
  const float xn = ((((a.fx * p.x) / p.z) + a.cx) - (a.colsf * 0.5f)) / (a.colsf * 0.5f);
  const float yn = ((((a.fy * p.y) / p.z) + a.cy) - (a.rowsf * 0.5f)) / (a.rowsf * 0.5f);
  const float zn = p.z / a.maxDepth;
  // GL clips a point by its centre against -w <= x,y,z <= w (w = 1)
  if (!(xn >= -1.f && xn <= 1.f && yn >= -1.f && yn <= 1.f && zn >= -1.f && zn <= 1.f)) return false;
  xw = (xn + 1.f) * (a.colsf * 0.5f);
  yw = (yn + 1.f) * (a.rowsf * 0.5f);
  zw = zn * 0.5f + 0.5f;
  return true;
}

struct SplatSurfel {
  f3 pos;       // camera frame
  f3 nrm;       // camera frame, normalised
  float rad, conf;
  float xw, yw;  // sprite centre in window coordinates
  float size;    // gl_PointSize
};

__device__ __forceinline__ f3 project_image(const ProjArgs& a, const f3& p) {  // splat.vert:44-49
  return mk3(((a.fx * p.x) / p.z) + a.cx, ((a.fy * p.y) / p.z) + a.cy, p.z);
}

// the cull of splat.vert for one set of (confidence threshold, time, newest time) — the part of the vertex stage that
// differs between two predictions of the same map from the same pose
__device__ __forceinline__ bool splat_culled(const ProjArgs& a, const f3& ph, float conf, float vt, float confThreshold, int time, int maxTime) {
  const bool actv = a.actv != 0;
  return !(!actv && vt == -3.f) && (ph.z > a.maxDepth || ph.z < 0.f || conf < confThreshold || (actv && vt == -3.f) ||
                                    (vt != -3.f && (float)time - vt > (float)a.timeDelta) || vt > (float)maxTime);
}

// (SplatSecond, the second prediction sharing the project pass: internal.hpp)

// vertex stage, first half: the cull and the clip, from position, confidence and time alone.  `pass`: bit 0 = survives the cull
// of `a`, bit 1 = survives the cull of `b` (when given).  False when the surfel is culled / clipped.
__device__ __forceinline__ bool splat_vertex_cull(const ProjArgs& a, const float4& pc, float vt, SplatSurfel& o, f3& ph, const SplatSecond* b,
                                                  int* pass) {
  const float* Tinv = a.pose->t_inv;
  ph = xform_point(Tinv, mk3(pc.x, pc.y, pc.z));
  int keep = splat_culled(a, ph, pc.w, vt, a.confThreshold, a.time, a.maxTime) ? 0 : 1;
  if (b) keep |= splat_culled(a, ph, pc.w, vt, b->confThreshold, b->time, b->maxTime) ? 0 : 2;
  if (pass) *pass = keep;
  if (!keep) return false;
  float zw;
  return project_window(a, ph, o.xw, o.yw, zw);
}

// vertex stage, second half: the sprite of a surfel that survived, from its normal / radius
__device__ __forceinline__ void splat_vertex_sprite(const ProjArgs& a, const float4& pc, const f3& ph, const float4& nr, SplatSurfel& o) {
  const float* Tinv = a.pose->t_inv;
  o.pos = ph;
  o.conf = pc.w;
  o.rad = nr.w;
  o.nrm = normalized3(xform_dir(Tinv, mk3(nr.x, nr.y, nr.z)));
  const f3 x1n = normalized3(mk3(o.nrm.y - o.nrm.z, -o.nrm.x, o.nrm.x));
  const f3 x1 = mk3((x1n.x * o.rad) * 1.41421356f, (x1n.y * o.rad) * 1.41421356f, (x1n.z * o.rad) * 1.41421356f);
  const f3 y1 = cross3(o.nrm, x1);
  const f3 p1 = project_image(a, ph + x1), p2 = project_image(a, ph + y1), p3 = project_image(a, ph - y1), p4 = project_image(a, ph - x1);
  const float xmin = fminf(p1.x, fminf(p2.x, fminf(p3.x, p4.x))), xmax = fmaxf(p1.x, fmaxf(p2.x, fmaxf(p3.x, p4.x)));
  const float ymin = fminf(p1.y, fminf(p2.y, fminf(p3.y, p4.y))), ymax = fmaxf(p1.y, fmaxf(p2.y, fmaxf(p3.y, p4.y)));
  const float xDiff = fabsf(xmax - xmin), yDiff = fabsf(ymax - ymin);
  o.size = fmaxf(0.f, fmaxf(xDiff, yDiff));
}

// vertex stage: returns false when the surfel is culled / clipped
// (the normal / radius plane is read only for surfels that survive the cull and the clip: for a large map most do
// not, and the pass is bandwidth-bound there — 20 instead of 36 bytes per culled surfel)
__device__ __forceinline__ bool splat_vertex(const ProjArgs& a, const float4& pc, const float4* __restrict__ nrp, float vt, SplatSurfel& o,
                                             const SplatSecond* b = nullptr, int* pass = nullptr) {
  f3 ph;
  if (!splat_vertex_cull(a, pc, vt, o, ph, b, pass)) return false;
  splat_vertex_sprite(a, pc, ph, *nrp, o);
  return true;
}
// the same for a caller that holds the normal / radius already
__device__ __forceinline__ bool splat_vertex_held(const ProjArgs& a, const float4& pc, const float4& nr, float vt, SplatSurfel& o,
                                                  const SplatSecond* b = nullptr, int* pass = nullptr) {
  f3 ph;
  if (!splat_vertex_cull(a, pc, vt, o, ph, b, pass)) return false;
  splat_vertex_sprite(a, pc, ph, nr, o);
  return true;
}

// The fragment stage (combo_splat.frag) in few instructions for the project pass, whose sprite loop is bound by vector-instruction
// issue: four IEEE quotients, a square root and the 64-bit depth conversion were 70 of a fragment's 115 instructions.
// exact_arith.hpp: the divisors fx, fy and 2 maxDepth are constants of the launch (reciprocal once, two correction steps per
// quotient); the ray's squared length is in [1, 16) for any pixel within 3.8 focal lengths of the principal point (square root without
// the small-operand scaling, reciprocal by one Newton step - both compared with the IEEE results over their whole domains on the
// device).  Same bits as splat_fragment (fusion_map.hip): the accept / reject decision, the depth and `corrected` (a -0 quotient
// becomes +0 only where 0.5 is added next or the operand is an exact difference, which is never -0; NaN / infinite depths are
// rejected on both sides).
struct SplatRay {
  exact::Divisor fx, fy, z2;
};
__device__ __forceinline__ SplatRay splat_ray_consts(const ProjArgs& a) {
  return SplatRay{exact::divisor(a.fx), exact::divisor(a.fy), exact::divisor(2.f * a.maxDepth)};
}
__device__ __forceinline__ bool splat_fragment_lean(const SplatRay& rc, const ProjArgs& a, const SplatSurfel& s, int px, int py, f3& corrected, float& zw) {
  const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;  // gl_FragCoord
  const f3 v = mk3(exact::div(fcx - a.cx, rc.fx), exact::div(fcy - a.cy, rc.fy), 1.0f);
  const float vv = dot3(v, v);
  const float rn = vv < 16.f ? exact::rcp_1_4(exact::sqrt_normal(vv)) : 1.0f / sqrtf(vv);
  const f3 l = mk3(v.x * rn, v.y * rn, v.z * rn);
  const float k = dot3(s.pos, s.nrm) / dot3(l, s.nrm);
  corrected = mk3(k * l.x, k * l.y, k * l.z);
  const float sqrRad = s.rad * s.rad;
  const f3 diff = corrected - s.pos;
  if (dot3(diff, diff) > sqrRad) return false;
  zw = exact::div(corrected.z, rc.z2) + 0.5f;
  return true;
}

// sprite coverage: pixel centres inside [c - size/2, c + size/2); a size below 1 rasterises as 1
__device__ __forceinline__ void sprite_range(float c, float size, int n, int& lo, int& hi) {
  const float sz = fmaxf(size, 1.0f);
  const float a = c - sz * 0.5f, b = c + sz * 0.5f;
  lo = (int)ceilf(a - 0.5f);
  hi = (int)ceilf(b - 0.5f) - 1;
  if (lo < 0) lo = 0;
  if (hi > n - 1) hi = n - 1;
}

// block 0 of a project launch that no resolve follows carries what the resolve's block 0 would have
__device__ __forceinline__ void splat_rider(const ProjectRider& rd) {
  if ((int)threadIdx.x < rd.mirror_words) rd.mirror_dst[threadIdx.x] = rd.mirror_src[threadIdx.x];
  if ((int)threadIdx.x < rd.copy_words) rd.copy_dst[threadIdx.x] = rd.copy_src[threadIdx.x];
}

// Sprite sizes differ by up to 3x inside a wave (5x5 ... 9x9 pixels), so "one thread rasterises its
// surfel" leaves ~55 % of the lanes idle in a loop that is instruction bound.  A block of 256 threads runs the
// vertex stage for 256 surfels, parks their parameters in these tables (splat_park), and then hands out sprite ROWS to
// threads (splat_rows: prefix sum of the row counts + binary search): a thread's trip count is one sprite width,
// and the rows of a large sprite are spread over many threads.  The winners are decided by 64-bit
// atomicMin, so the work order does not matter.
struct SplatTables {
  float par[10][256];  // pos.xyz, nrm.xyz, rad, window x / y of the centre, squared reach (splat_park)
  int box[5][256];     // x0, width, y0, cull survivors (DUAL), surfel id (IDS)
  unsigned off[257];   // exclusive prefix of the row counts
  unsigned w[4];
};

// Thread t parks a surfel that came through the vertex stage; returns its number of sprite rows (0: nothing to rasterise).
// IDS: the surfel's id is `id`, kept in the table; otherwise it is the chunk's base + t and splat_rows forms it.
template <bool DUAL, bool IDS>
__device__ __forceinline__ int splat_park(const ProjArgs& a, const SplatSurfel& s, int pass, unsigned id, int t, SplatTables& tb) {
  if (!(s.size == s.size)) return 0;
  int x0, x1, y0, y1;
  sprite_range(s.xw, s.size, a.cols, x0, x1);
  sprite_range(s.yw, s.size, a.rows, y0, y1);
  // The sprite is the square around four points at sqrt(2) r along the tangent axes; the disc test passes on about
  // 40 % of its fragments.  A fragment can only pass if its ray comes within r of the centre P = Z (xc, yc, 1):
  // the distance of P from the ray along v = (x, y, 1) is Z |(xc, yc, 1) x v| / |v| >= Z rho / |v|, with
  // rho^2 = (x - xc)^2 + (y - yc)^2 — the fragment's offset from the centre in normalised image coordinates —
  // and |v|^2 <= G2 = 1 + (|xc| + h)^2 + (|yc| + h)^2 inside the sprite (half size h).  So rho > r sqrt(G2) / Z
  // rules a fragment out; with 2 % (and 0.02 pixel) added, far more than the rounding of the fragment test itself, the
  // rows and the columns of each row are cut to that circle before any fragment is evaluated.
  float reach = 3.0e18f;  // normalised units; no cut when the bound cannot be formed
  {
    const float ifx = 1.f / a.fx, ify = 1.f / a.fy;
    const float h = (0.5f * fmaxf(s.size, 1.f) + 1.f) * fmaxf(ifx, ify);
    const float xc = fabsf((s.xw - a.cx) * ifx) + h, yc = fabsf((s.yw - a.cy) * ify) + h;
    const float g2 = 1.f + xc * xc + yc * yc;
    const float rn = (s.rad * sqrtf(g2) / s.pos.z) * 1.02f + 0.02f * fmaxf(ifx, ify);
    if (s.pos.z > 0.f && rn == rn && rn < 3.0e18f) reach = rn;
    const float ry = fminf(reach * a.fy, 1.0e9f);
    const int c0 = (int)ceilf(fmaxf(s.yw - ry - 0.5f, -1.0e9f)), c1 = (int)floorf(fminf(s.yw + ry - 0.5f, 1.0e9f));  // |py + 0.5 - yw| <= ry
    y0 = max(y0, c0);
    y1 = min(y1, c1);
  }
  if (!(x1 >= x0 && y1 >= y0)) return 0;
  tb.par[0][t] = s.pos.x;
  tb.par[1][t] = s.pos.y;
  tb.par[2][t] = s.pos.z;
  tb.par[3][t] = s.nrm.x;
  tb.par[4][t] = s.nrm.y;
  tb.par[5][t] = s.nrm.z;
  tb.par[6][t] = s.rad;
  tb.par[7][t] = s.xw;
  tb.par[8][t] = s.yw;
  tb.par[9][t] = reach * reach;
  tb.box[0][t] = x0;
  tb.box[1][t] = x1 - x0 + 1;
  tb.box[2][t] = y0;
  if (DUAL) tb.box[3][t] = pass;
  if (IDS) tb.box[4][t] = (int)id;
  return y1 - y0 + 1;
}

// The sprite rows of the parked surfels, by all 256 threads of the block (uniform control flow: two block barriers inside; the
// caller puts one more behind it before the tables are parked again).  DUAL: one pass feeds two z-buffers — two predictions of
// the same map from the same pose that differ in the cull only: a fragment competes in the z-buffer of every prediction its
// surfel survives the cull of.
template <bool DUAL, bool IDS>
__device__ __forceinline__ void splat_rows(const ProjArgs& a, const SplatRay& ray, int rows_here, unsigned base, SplatTables& tb,
                                           unsigned long long* __restrict__ zbuf, unsigned long long* __restrict__ zbuf2) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  // block-wide exclusive scan of rows_here
  unsigned incl = (unsigned)rows_here;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) tb.w[wid] = incl;
  __syncthreads();
  unsigned wbase = 0;
  for (int w = 0; w < wid; ++w) wbase += tb.w[w];
  tb.off[t] = wbase + incl - (unsigned)rows_here;
  if (t == 255) tb.off[256] = wbase + incl;
  __syncthreads();
  const unsigned total = tb.off[256];
  for (unsigned u = t; u < total; u += 256u) {
    // surfel j with off[j] <= u < off[j + 1]
    int lo = 0, hi = 256;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int mid = (lo + hi) >> 1;
      if (tb.off[mid] <= u)
        lo = mid;
      else
        hi = mid;
    }
    const int j = lo;
    SplatSurfel s;
    s.pos = mk3(tb.par[0][j], tb.par[1][j], tb.par[2][j]);
    s.nrm = mk3(tb.par[3][j], tb.par[4][j], tb.par[5][j]);
    s.rad = tb.par[6][j];
    const int x0 = tb.box[0][j], w = tb.box[1][j];
    const int py = tb.box[2][j] + (int)(u - tb.off[j]);
    const unsigned long long id = IDS ? (unsigned long long)(unsigned)tb.box[4][j] : (unsigned long long)(base + (unsigned)j);
    const int pass = DUAL ? tb.box[3][j] : 1;
    // columns of this row inside the surfel's reach (see splat_park)
    const float dyn = (((float)py + 0.5f) - tb.par[8][j]) * (1.f / a.fy);
    const float left = tb.par[9][j] - dyn * dyn;
    if (left < 0.f) continue;
    const float rx = fminf(sqrtf(left) * a.fx, 1.0e9f), xwc = tb.par[7][j];
    const int xa = max(x0, (int)ceilf(fmaxf(xwc - rx - 0.5f, -1.0e9f)));  // |px + 0.5 - xw| <= rx
    const int xb = min(x0 + w - 1, (int)floorf(fminf(xwc + rx - 0.5f, 1.0e9f)));
    // The row in groups of four fragments: the z-buffer cells a group will compete for are fetched first (their addresses
    // depend on the pixel only), the ray / disc tests run while those loads are in flight, and a fragment goes to the
    // atomic only when it beats the value fetched (cells only ever decrease: a stale value can cost an atomic, never a win).
    const bool use1 = !DUAL || (pass & 1), use2 = DUAL && (pass & 2);
    for (int px0 = xa; px0 <= xb; px0 += 4) {
      unsigned long long z1[4], z2[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = px0 + k;
        const size_t q = (size_t)px * a.rows + py;  // column-major z-buffer
        const bool in = px <= xb;
        z1[k] = (in && use1) ? zbuf[q] : 0ull;
        z2[k] = (in && use2) ? zbuf2[q] : 0ull;
      }
      // (the four ray / disc tests first, the atomics behind them: an atomic between two tests made the next test wait for it -
      // the counter that guards the prefetched cells also counts the atomics in flight)
      unsigned long long key[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = px0 + k;
        key[k] = ~0ull;
        f3 c;
        float zw;
        if (px <= xb && splat_fragment_lean(ray, a, s, px, py, c, zw)) {
          const unsigned d = depth24(zw);
          if (d < 0xFFFFFFu) key[k] = ((unsigned long long)d << 32) | id;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const size_t q = (size_t)(px0 + k) * a.rows + py;
        if (key[k] < z1[k]) atomicMin(zbuf + q, key[k]);
        if (DUAL && key[k] < z2[k]) atomicMin(zbuf2 + q, key[k]);
      }
    }
  }
}

}  // namespace dms
