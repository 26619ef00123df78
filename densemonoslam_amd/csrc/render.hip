// G14 (draw): GlobalModel::renderPointCloud (GlobalModel.cpp:419-505) — the surfel map drawn from any viewpoint into a
// render target, with the programs draw_global_surface.{vert,geom,frag} (discs) and draw_feedback.{vert,frag} (points).
//
// The same two-pass shape as the splat prediction (fusion_map.hip):
//   pass 1, per surfel: vertex + geometry stage, rasterise the footprint (two triangles of the geometry stage's strip, or
//           one pixel for a point), compete per pixel with a 64-bit atomicMin on
//           key = depth24 << 40 | draw_seq << 32 | surfel id;
//   pass 2, per pixel: a pixel whose winner belongs to this draw gets its colour and depth written.
// GL_LESS with "the earlier primitive / draw wins a tie" is "the smallest key wins", across several draws into one target.
// The rules OpenGL leaves open (coverage, interpolation, clipping, colour and depth conversion) are DESIGN §4 R6-R10, and
// tests/render_ref.py restates them on the CPU.
#include "surfel.hpp"
#include "../../include/dmslam_render.h"
#include "../../include/dmslam_render_shaded.h"
#include "../../include/dmslam_render_cloud.h"
#include "../../include/dmslam_render_panels.h"
#include "internal.hpp"

using namespace dms;

struct dms_panels {
  int width = 0, height = 0;
  unsigned char* norm = nullptr;  // DEPTH_NORM, L8 (R26), image rows
  unsigned* model = nullptr;      // the Model image (drawTexture), RGBA8, image rows
};

struct dms_render_target {
  int width = 0, height = 0;
  unsigned long long* key = nullptr;  // [H][W] row-major (window rows: row 0 at the bottom)
  unsigned* color = nullptr;          // RGBA8
  unsigned* depth = nullptr;          // 24-bit depth in the low bits
  unsigned* clip_flag = nullptr;      // draw_seq + 1 of the last draw that met a surfel to clip (R8)
  int seq = 0;                        // draws since the last clear
};

namespace dms {
namespace {

constexpr int kSub = 256;        // R6: window coordinates snapped to 1/256 px
constexpr float kGuard = 255.f;  // R8: guard band |x|, |y| <= 255 w (window coordinates within 2^20 px, snapped within 2^28)
constexpr int kSeg = 32;         // pixels of a footprint row one lane rasterises

struct RenderArgs {
  float mvp[16];
  const float* pose_dev;  // camera-to-world in HBM: mvp is then the projection and the view is built on the device
  int W, H;
  float hw, hh;  // W / 2, H / 2
  float threshold;
  int unstable, window, colorType, time, timeIdx, timeDelta, cluster;
  float cc[3];
  unsigned seq;
};

// clip = M (p, 1), row by row, accumulated left to right
struct c4 {
  float x, y, z, w;
};
__device__ __forceinline__ c4 clip_of(const float* M, float x, float y, float z) {
  c4 r;
  r.x = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  r.y = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  r.z = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  r.w = ((M[12] * x + M[13] * y) + M[14] * z) + M[15];
  return r;
}

// dmslam_render.h, dms_render_mvp_from_pose: P * F * inverse(pose), F = diag(1, -1, -1, 1) (right-down-forward camera to
// right-up-back), the rigid inverse [R^T | -R^T t] and both products accumulated left to right
__host__ __device__ inline void mvp_from_pose(const float* P, const float* T, float* out) {
  float V[16];
  for (int r = 0; r < 3; ++r) {
    const float sg = r == 0 ? 1.f : -1.f;
    V[4 * r + 0] = sg * T[0 + r];
    V[4 * r + 1] = sg * T[4 + r];
    V[4 * r + 2] = sg * T[8 + r];
    V[4 * r + 3] = sg * -((T[0 + r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);
  }
  V[12] = V[13] = V[14] = 0.f;
  V[15] = 1.f;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out[4 * r + c] = ((P[4 * r] * V[c] + P[4 * r + 1] * V[4 + c]) + P[4 * r + 2] * V[8 + c]) + P[4 * r + 3] * V[12 + c];
}

// the effective clip-from-world matrix of the launch
__device__ __forceinline__ void launch_mvp(const RenderArgs& a, float* M) {
  if (a.pose_dev) {
    float pose[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) pose[k] = a.pose_dev[k];
    mvp_from_pose(a.mvp, pose, M);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) M[k] = a.mvp[k];
  }
}

// ---- disc geometry (draw_global_surface.geom:185-212) -------------------------------------------------------------------
// the four strip vertices P + x, P + y, P - y, P - x in clip space; texcoords (-1,-1) (1,-1) (-1,1) (1,1)
// world positions of the four strip vertices (the geometry stage's `v`, .geom:122-140)
__device__ __forceinline__ void disc_world(const float4& pc, const float4& nr, f3* w) {
  const f3 xn = normalized3(mk3(nr.y - nr.z, -nr.x, nr.x));
  const f3 x = mk3((xn.x * nr.w) * 1.41421356f, (xn.y * nr.w) * 1.41421356f, (xn.z * nr.w) * 1.41421356f);
  const f3 y = cross3(mk3(nr.x, nr.y, nr.z), x);
  w[0] = mk3(pc.x + x.x, pc.y + x.y, pc.z + x.z);
  w[1] = mk3(pc.x + y.x, pc.y + y.y, pc.z + y.z);
  w[2] = mk3(pc.x - y.x, pc.y - y.y, pc.z - y.z);
  w[3] = mk3(pc.x - x.x, pc.y - x.y, pc.z - x.z);
}
__device__ __forceinline__ void disc_corners(const float* M, const f3* w, c4* v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = clip_of(M, w[k].x, w[k].y, w[k].z);
}
__device__ __forceinline__ void disc_corners(const float* M, const float4& pc, const float4& nr, c4* v) {
  f3 w[4];
  disc_world(pc, nr, w);
  disc_corners(M, w, v);
}

// R8 plane distances: near z >= -w, then the guard band
__device__ __forceinline__ float plane_dist(const c4& v, int k) {
  const float gw = kGuard * v.w;
  return k == 0 ? v.z + v.w : k == 1 ? gw - v.x : k == 2 ? gw + v.x : k == 3 ? gw - v.y : gw + v.y;
}
__device__ __forceinline__ unsigned outcode(const c4& v) {
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) o |= (plane_dist(v, k) >= 0.f ? 0u : 1u) << k;
  return o;
}

// a window-space vertex: snapped position, window depth, 1/w, texcoord
struct WV {
  int X, Y;
  float z, iw, u, v;
};
__device__ __forceinline__ WV to_window(const RenderArgs& a, const c4& c, float u, float v) {
  WV r;
  const float xn = c.x / c.w, yn = c.y / c.w, zn = c.z / c.w;
  r.X = (int)rintf(((xn + 1.f) * a.hw) * (float)kSub);
  r.Y = (int)rintf(((yn + 1.f) * a.hh) * (float)kSub);
  r.z = zn * 0.5f + 0.5f;
  r.iw = 1.f / c.w;
  r.u = u;
  r.v = v;
  return r;
}

// pixel rows / columns whose centres lie in [lo, hi] (snapped units)
__device__ __forceinline__ int first_px(int lo) { return -((kSub / 2 - lo) >> 8); }
__device__ __forceinline__ int last_px(int hi) { return (hi - kSub / 2) >> 8; }

// R7 / R10 at a pixel a triangle covers (barycentrics b0..b2): the fragment's 24-bit depth, or 0xFFFFFFFF where there is none;
// q0..q2 / den are its perspective weights
__device__ __forceinline__ unsigned disc_fragment(const WV& v0, const WV& v1, const WV& v2, float b0, float b1, float b2, float shift,
                                                  float& q0, float& q1, float& q2, float& den) {
  const float z = (b0 * v0.z + b1 * v1.z) + b2 * v2.z;
  if (!(z >= 0.f && z <= 1.f)) return 0xFFFFFFFFu;  // R8: nothing beyond the far (or before the near) plane
  q0 = b0 * v0.iw, q1 = b1 * v1.iw, q2 = b2 * v2.iw;
  den = (q0 + q1) + q2;
  const float u = ((q0 * v0.u + q1 * v1.u) + q2 * v2.u) / den;
  const float v = ((q0 * v0.v + q1 * v1.v) + q2 * v2.v) / den;
  if (u * u + v * v > 1.f) return 0xFFFFFFFFu;  // draw_global_surface.frag:30-31
  // .frag:35-42 + R10: the shifted depth is clamped to [0, 1] before the 24-bit conversion and the test
  const float zf = fminf(fmaxf(z + shift, 0.f), 1.f);
  return depth24(zf);
}

// R6 / R7 / R10: one triangle over pixels [xa, xb] of row py
__device__ void raster_row(WV v0, WV v1, WV v2, int py, int xa, int xb, unsigned long long key_lo, float shift, int W,
                           unsigned long long* __restrict__ zrow) {
  long long area = (long long)(v1.X - v0.X) * (long long)(v2.Y - v0.Y) - (long long)(v1.Y - v0.Y) * (long long)(v2.X - v0.X);
  if (area == 0) return;
  if (area < 0) {
    const WV t = v1;
    v1 = v2;
    v2 = t;
    area = -area;
  }
  // edge k is opposite vertex k: e0 = v1 -> v2, e1 = v2 -> v0, e2 = v0 -> v1
  const int ax0 = v1.X, ay0 = v1.Y, dx0 = v2.X - v1.X, dy0 = v2.Y - v1.Y;
  const int ax1 = v2.X, ay1 = v2.Y, dx1 = v0.X - v2.X, dy1 = v0.Y - v2.Y;
  const int ax2 = v0.X, ay2 = v0.Y, dx2 = v1.X - v0.X, dy2 = v1.Y - v0.Y;
  const bool tl0 = dy0 < 0 || (dy0 == 0 && dx0 < 0), tl1 = dy1 < 0 || (dy1 == 0 && dx1 < 0), tl2 = dy2 < 0 || (dy2 == 0 && dx2 < 0);
  const long long Py = (long long)py * kSub + kSub / 2, Px = (long long)xa * kSub + kSub / 2;
  long long e0 = (long long)dx0 * (Py - ay0) - (long long)dy0 * (Px - ax0);
  long long e1 = (long long)dx1 * (Py - ay1) - (long long)dy1 * (Px - ax1);
  long long e2 = (long long)dx2 * (Py - ay2) - (long long)dy2 * (Px - ax2);
  const long long s0 = -(long long)dy0 * kSub, s1 = -(long long)dy1 * kSub, s2 = -(long long)dy2 * kSub;
  const float inv = 1.f / (float)(double)area;
  for (int px = xa; px <= xb; ++px, e0 += s0, e1 += s1, e2 += s2) {
    if (!((e0 > 0 || (e0 == 0 && tl0)) && (e1 > 0 || (e1 == 0 && tl1)) && (e2 > 0 || (e2 == 0 && tl2)))) continue;
    const float b0 = (float)(double)e0 * inv, b1 = (float)(double)e1 * inv, b2 = (float)(double)e2 * inv;
    float q0, q1, q2, den;
    const unsigned d = disc_fragment(v0, v1, v2, b0, b1, b2, shift, q0, q1, q2, den);
    if (d >= 0xFFFFFFu) continue;  // GL_LESS against the cleared 1.0
    const unsigned long long key = ((unsigned long long)d << 40) | key_lo;
    if (key < zrow[px]) atomicMin(zrow + px, key);
  }
}

// R8: a triangle that leaves the near plane or the guard band, clipped plane by plane (Sutherland-Hodgman); each new vertex is
// interpolated from the inside end of its edge.  Rare: kept out of line (its polygon lives in private memory).
struct CV {
  c4 c;
  float u, v;
};
struct CVW {  // the same with the world position (the shaded draw, R11)
  c4 c;
  float u, v;
  f3 w;
};
__device__ __forceinline__ void lerp_attrs(CV& r, const CV& I, const CV& O, float t) {
  r.u = I.u + t * (O.u - I.u);
  r.v = I.v + t * (O.v - I.v);
}
__device__ __forceinline__ void lerp_attrs(CVW& r, const CVW& I, const CVW& O, float t) {
  r.u = I.u + t * (O.u - I.u);
  r.v = I.v + t * (O.v - I.v);
  r.w = mk3(I.w.x + t * (O.w.x - I.w.x), I.w.y + t * (O.w.y - I.w.y), I.w.z + t * (O.w.z - I.w.z));
}
template <class V>
__device__ __forceinline__ int clip_polygon(V* poly, int n) {
  V tmp[9];
  for (int k = 0; k < 5 && n > 0; ++k) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const V A = poly[i], B = poly[(i + 1) % n];
      const float da = plane_dist(A.c, k), db = plane_dist(B.c, k);
      const bool ia = da >= 0.f, ib = db >= 0.f;
      if (ia) tmp[m++] = A;
      if (ia != ib) {
        const V& I = ia ? A : B;
        const V& O = ia ? B : A;
        const float di = ia ? da : db, dout = ia ? db : da;
        const float t = di / (di - dout);
        V r;
        r.c.x = I.c.x + t * (O.c.x - I.c.x);
        r.c.y = I.c.y + t * (O.c.y - I.c.y);
        r.c.z = I.c.z + t * (O.c.z - I.c.z);
        r.c.w = I.c.w + t * (O.c.w - I.c.w);
        lerp_attrs(r, I, O, t);
        tmp[m++] = r;
      }
    }
    n = m;
    for (int i = 0; i < n; ++i) poly[i] = tmp[i];
  }
  return n;
}

__device__ __forceinline__ void raster_clipped_row(const RenderArgs& a, const c4* cv, int py, int xa, int xb, unsigned long long key_lo,
                                                float shift, unsigned long long* __restrict__ zrow) {
  const float tu[4] = {-1.f, 1.f, -1.f, 1.f}, tv[4] = {-1.f, -1.f, 1.f, 1.f};
  const int tri[2][3] = {{0, 1, 2}, {2, 1, 3}};
  for (int t = 0; t < 2; ++t) {
    CV poly[9];
    for (int k = 0; k < 3; ++k) {
      const int i = tri[t][k];
      poly[k].c = cv[i];
      poly[k].u = tu[i];
      poly[k].v = tv[i];
    }
    const int n = clip_polygon(poly, 3);
    if (n < 3) continue;
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && poly[k].c.w > 0.f;
    if (!ok) continue;
    const WV w0 = to_window(a, poly[0].c, poly[0].u, poly[0].v);
    WV wp = to_window(a, poly[1].c, poly[1].u, poly[1].v);
    for (int k = 2; k < n; ++k) {  // fan (0, k-1, k)
      const WV wk = to_window(a, poly[k].c, poly[k].u, poly[k].v);
      raster_row(w0, wp, wk, py, xa, xb, key_lo, shift, a.W, zrow);
      wp = wk;
    }
  }
}

// footprint of a clipped surfel: snapped bounds of every vertex the clip produces
__device__ __forceinline__ bool clipped_bounds(const RenderArgs& a, const c4* cv, int& X0, int& X1, int& Y0, int& Y1) {
  const int tri[2][3] = {{0, 1, 2}, {2, 1, 3}};
  X0 = Y0 = 0x7fffffff;
  X1 = Y1 = -0x7fffffff;
  bool any = false;
  for (int t = 0; t < 2; ++t) {
    CV poly[9];
    for (int k = 0; k < 3; ++k) {
      poly[k].c = cv[tri[t][k]];
      poly[k].u = poly[k].v = 0.f;
    }
    const int n = clip_polygon(poly, 3);
    if (n < 3) continue;
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && poly[k].c.w > 0.f;
    if (!ok) continue;
    for (int k = 0; k < n; ++k) {
      const WV w = to_window(a, poly[k].c, 0.f, 0.f);
      X0 = min(X0, w.X), X1 = max(X1, w.X), Y0 = min(Y0, w.Y), Y1 = max(Y1, w.Y);
    }
    any = true;
  }
  return any;
}

// Pass 1 of the disc program.  A block runs the vertex + geometry stage for 256 surfels, parks the window-space strip of each
// in LDS, and hands out footprint row segments (up to kSeg pixels) to its threads by a prefix sum + binary search, as
// k_splat_project does with sprite rows: a surfel that covers hundreds of pixels is spread over many lanes.
// CLIPPED = false: the surfels whose strip lies inside every plane of R8 (nearly all); one that does not raises *clip_flag
// (= draw_seq + 1).  CLIPPED = true (launched behind it, returns at once unless the flag was raised in this draw): the others,
// clipped again by every row worker.  Two instances, so that the clip's registers and private arrays do not weigh on the common
// path.
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_render_discs(RenderArgs a, SurfelPlanes sp, const unsigned* __restrict__ d_count,
                                                      unsigned long long* __restrict__ zbuf, unsigned* __restrict__ clip_flag) {
  __shared__ int s_xy[8][256];     // X0 Y0 .. X3 Y3 (snapped), or the surfel's clip-space corners are recomputed (clipped)
  __shared__ float s_zi[8][256];   // z0 iw0 .. z3 iw3
  __shared__ float s_shift[256];   // depth shift of an unstable surfel
  __shared__ int s_box[4][256];    // x0, width, y0, segments per row
  __shared__ unsigned s_off[257];  // exclusive prefix of the segment counts
  __shared__ unsigned s_w[4];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  if (CLIPPED && *clip_flag != a.seq + 1u) return;
  const unsigned M = d_count[0];
  float Mv[16];
  launch_mvp(a, Mv);
  for (unsigned base = blockIdx.x * 256u; base < M; base += gridDim.x * 256u) {
    const unsigned i = base + t;
    unsigned items = 0;
    if (i < M) {
      const float4 pc = sp.pos[i];
      if (pc.w > a.threshold || a.unstable == 1) {  // draw_global_surface.vert:49
        const float4 nr = sp.nrm[i];
        c4 cv[4];
        disc_corners(Mv, pc, nr, cv);
        const unsigned o0 = outcode(cv[0]), o1 = outcode(cv[1]), o2 = outcode(cv[2]), o3 = outcode(cv[3]);
        int X0, X1, Y0, Y1;
        bool live = false;
        const bool clipped = (o0 | o1 | o2 | o3) != 0u;
        if (!CLIPPED && clipped) {
          *clip_flag = a.seq + 1u;
        } else if (!CLIPPED) {
          const float tu[4] = {-1.f, 1.f, -1.f, 1.f}, tv[4] = {-1.f, -1.f, 1.f, 1.f};
          X0 = Y0 = 0x7fffffff;
          X1 = Y1 = -0x7fffffff;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const WV w = to_window(a, cv[k], tu[k], tv[k]);
            s_xy[2 * k][t] = w.X;
            s_xy[2 * k + 1][t] = w.Y;
            s_zi[2 * k][t] = w.z;
            s_zi[2 * k + 1][t] = w.iw;
            X0 = min(X0, w.X), X1 = max(X1, w.X), Y0 = min(Y0, w.Y), Y1 = max(Y1, w.Y);
          }
          live = true;
        } else if (clipped && (o0 & o1 & o2 & o3) == 0u) {
          live = clipped_bounds(a, cv, X0, X1, Y0, Y1);
        }
        if (live) {
          const int x0 = max(first_px(X0), 0), x1 = min(last_px(X1), a.W - 1);
          const int y0 = max(first_px(Y0), 0), y1 = min(last_px(Y1), a.H - 1);
          if (x1 >= x0 && y1 >= y0) {
            const int w = x1 - x0 + 1, segs = (w + kSeg - 1) / kSeg;
            items = (unsigned)((y1 - y0 + 1) * segs);
            s_box[0][t] = x0;
            s_box[1][t] = w;
            s_box[2][t] = y0;
            s_box[3][t] = segs;
            s_shift[t] = pc.w <= a.threshold ? nr.w : 0.f;  // .geom:183, .frag:35-42
          }
        }
      }
    }
    unsigned incl = items;
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_w[wid] = incl;
    __syncthreads();
    unsigned wbase = 0;
    for (int w = 0; w < wid; ++w) wbase += s_w[w];
    s_off[t] = wbase + incl - items;
    if (t == 255) s_off[256] = wbase + incl;
    __syncthreads();
    const unsigned total = s_off[256];
    for (unsigned u = t; u < total; u += 256u) {
      int lo = 0, hi = 256;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int mid = (lo + hi) >> 1;
        if (s_off[mid] <= u)
          lo = mid;
        else
          hi = mid;
      }
      const int j = lo;
      const unsigned r = u - s_off[j];
      const int segs = s_box[3][j];
      const int py = s_box[2][j] + (int)(r / (unsigned)segs);
      const int sg = (int)(r % (unsigned)segs);
      const int xa = s_box[0][j] + sg * kSeg, xb = min(xa + kSeg - 1, s_box[0][j] + s_box[1][j] - 1);
      const unsigned id = base + (unsigned)j;
      const unsigned long long key_lo = ((unsigned long long)a.seq << 32) | (unsigned long long)id;
      const float shift = s_shift[j];
      unsigned long long* zrow = zbuf + (size_t)py * a.W;
      if (!CLIPPED) {
        WV v[4];
        const float tu[4] = {-1.f, 1.f, -1.f, 1.f}, tv[4] = {-1.f, -1.f, 1.f, 1.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[k].X = s_xy[2 * k][j];
          v[k].Y = s_xy[2 * k + 1][j];
          v[k].z = s_zi[2 * k][j];
          v[k].iw = s_zi[2 * k + 1][j];
          v[k].u = tu[k];
          v[k].v = tv[k];
        }
        // GL strip order: (v0, v1, v2), (v2, v1, v3)
        raster_row(v[0], v[1], v[2], py, xa, xb, key_lo, shift, a.W, zrow);
        raster_row(v[2], v[1], v[3], py, xa, xb, key_lo, shift, a.W, zrow);
      } else {
        c4 cv[4];
        disc_corners(Mv, sp.pos[id], sp.nrm[id], cv);
        raster_clipped_row(a, cv, py, xa, xb, key_lo, shift, zrow);
      }
    }
    __syncthreads();  // the tables are rewritten by the next chunk
  }
}

// R2 / R3 of a size-1 point at clip position c: the target pixel and the 64-bit key compete by atomicMin (order-free)
__device__ __forceinline__ void place_point(const c4& c, int W, int H, float hw, float hh, unsigned long long key_lo,
                                            unsigned long long* __restrict__ zbuf) {
  if (!(c.w > 0.f)) return;
  const float xn = c.x / c.w, yn = c.y / c.w, zn = c.z / c.w;
  if (!(xn >= -1.f && xn <= 1.f && yn >= -1.f && yn <= 1.f && zn >= -1.f && zn <= 1.f)) return;
  const int px = (int)floorf((xn + 1.f) * hw), py = (int)floorf((yn + 1.f) * hh);
  if (px < 0 || py < 0 || px >= W || py >= H) return;
  const unsigned d = depth24(zn * 0.5f + 0.5f);
  if (d >= 0xFFFFFFu) return;
  const unsigned long long key = ((unsigned long long)d << 40) | key_lo;
  unsigned long long* cell = zbuf + (size_t)py * W + px;
  if (key < *cell) atomicMin(cell, key);
}

// Pass 1 of the point program (draw_feedback.vert:47-72): one size-1 point per surfel with conf > threshold, placed by R2
__global__ __launch_bounds__(256) void k_render_points(RenderArgs a, SurfelPlanes sp, const unsigned* __restrict__ d_count,
                                                       unsigned long long* __restrict__ zbuf) {
  const unsigned M = d_count[0];
  float Mv[16];
  launch_mvp(a, Mv);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += blockDim.x * gridDim.x) {
    const float4 pc = sp.pos[i];
    if (!(pc.w > a.threshold)) continue;
    place_point(clip_of(Mv, pc.x, pc.y, pc.z), a.W, a.H, a.hw, a.hh, ((unsigned long long)a.seq << 32) | (unsigned long long)i, zbuf);
  }
}

// R9 (a channel that is not finite writes 0, as llvmpipe does: tests/golden/ref_render.npz)
__device__ __forceinline__ unsigned unorm8(float v) { return isfinite(v) ? (unsigned)floorf(fminf(fmaxf(v, 0.f), 1.f) * 255.f + 0.5f) : 0u; }
__device__ __forceinline__ unsigned rgba8(const f3& c) { return unorm8(c.x) | (unorm8(c.y) << 8) | (unorm8(c.z) << 16) | (255u << 24); }
__device__ __forceinline__ f3 shaded_grey(const float4& nr) {  // (.5 * |dot(n, 1)|) + .1
  const float s = fabsf((nr.x + nr.y) + nr.z);
  return mk3(0.5f * s + 0.1f, 0.5f * s + 0.1f, 0.5f * s + 0.1f);
}

// the colour of a winning surfel: draw_global_surface.geom:123-181 (discs) or draw_feedback.vert:297-314 (points)
template <bool POINTS>
__device__ __forceinline__ f3 surfel_colour(const RenderArgs& a, const SurfelPlanes& sp, size_t cap, unsigned i) {
  // each plane only where a mode reads it: the cluster colour reads none, normals / ramp / contributions / grey the normal,
  // decoded colour and ramp the colour plane, contributions and the window the time planes
  f3 c;
  if (a.cluster) {
    c = mk3(a.cc[0], a.cc[1], a.cc[2]);
  } else if (a.colorType == 1) {
    const float4 nr = sp.nrm[i];
    c = mk3(nr.x, nr.y, nr.z);
  } else if (a.colorType == 2) {
    c = decode_color(sp.col[i].x);
  } else if (!POINTS && a.colorType == 3) {
    const float4 nr = sp.nrm[i];
    const float ratio = (2.f * (sp.col[i].z - 1.f)) / ((float)a.time - 1.f);
    const float x = fmaxf(0.f, 1.f - ratio), y = fmaxf(0.f, ratio - 1.f), z = (1.f - x) - y;
    const float s = fabsf((nr.x + nr.y) + nr.z) + 0.1f;
    c = mk3(x * s, y * s, z * s);
  } else if (!POINTS && a.colorType == 4) {
    // The sum runs over the reference's three slots.  A surfel that only slots above 2 have seen has total = 0: every channel is
    // 0 / 0 * s + 0.1 = NaN, which unorm8 writes as 0 (its isfinite test; no NaN is converted to an integer) - such a surfel is drawn
    // black, with or without the window tint (tests/test_time_slots_gpu.py pins it, tests/render_ref.py does the same).
    const float4 nr = sp.nrm[i];
    const bool s0 = sp.times[i] != -3.f, s1 = sp.times[cap + i] != -3.f, s2 = sp.times[2 * cap + i] != -3.f;
    const float g = ((s0 ? 0.0f : 0.0f) + (s1 ? 0.8f : 0.0f)) + (s2 ? 0.0f : 0.0f);
    const float r = ((s0 ? 0.0f : 0.0f) + (s1 ? 0.1f : 0.0f)) + (s2 ? 0.8f : 0.0f);
    const float b = ((s0 ? 0.8f : 0.0f) + (s1 ? 0.2f : 0.0f)) + (s2 ? 0.0f : 0.0f);
    const float total = (float)((s0 ? 1 : 0) + (s1 ? 1 : 0) + (s2 ? 1 : 0));
    const float s = fabsf((nr.x + nr.y) + nr.z);
    c = mk3((r / total) * s + 0.1f, (g / total) * s + 0.1f, (b / total) * s + 0.1f);
  } else {
    c = shaded_grey(sp.nrm[i]);
  }
  if (!POINTS && a.window == 1) {  // .geom:173-182
    const float dt = (float)a.time - sp.times[(size_t)a.timeIdx * cap + i];
    if (dt > (float)a.timeDelta) c = mk3(c.x * 0.25f, c.y * 0.25f, c.z * 0.25f);
    if (dt < (float)a.timeDelta) c = mk3(c.x * 0.f, c.y * 1.f, c.z * 0.f);
  }
  return c;
}

// Pass 2: the pixels this draw won get their colour and depth; the rest keep what earlier draws (or the clear) left
template <bool POINTS>
__global__ __launch_bounds__(256) void k_render_resolve(RenderArgs a, SurfelPlanes sp, size_t cap, const unsigned long long* __restrict__ zbuf,
                                                        unsigned* __restrict__ color, unsigned* __restrict__ depth) {
  const int n = a.W * a.H;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    const unsigned long long key = zbuf[p];
    if (key == ~0ull || (unsigned)((key >> 32) & 0xFFu) != a.seq) continue;
    const unsigned i = (unsigned)(key & 0xFFFFFFFFull);
    color[p] = rgba8(surfel_colour<POINTS>(a, sp, cap, i));
    depth[p] = (unsigned)(key >> 40);
  }
}

__global__ void k_render_clear(unsigned long long* __restrict__ key, unsigned* __restrict__ color, unsigned* __restrict__ depth, int n,
                               unsigned c, unsigned* __restrict__ clip_flag) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *clip_flag = 0u;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    key[p] = ~0ull;
    color[p] = c;
    depth[p] = 0xFFFFFFu;
  }
}

// ---- the shaded view: GUI::drawFXAA (GUI/src/Tools/GUI.h:365-478) ------------------------------------
// Pass A draws the map into an offscreen float buffer with draw_global_surface.{vert,geom} + draw_global_surface_phong.frag: the
// keys come from pass 1 of the disc program unchanged (seq 0 after a clear); k_shaded_resolve is a visibility-buffer resolve: per
// pixel it rebuilds the winner's strip, finds the one triangle (or fan piece of a clipped triangle) whose fragment won, interpolates
// the world position there (R11) and evaluates the Phong program.  Pass B (k_render_fxaa) is fxaa.frag over that buffer into a
// render target, followed by the NEAREST depth blit.

// the fragment of triangle (v0, v1, v2) at pixel (px, py), exactly as raster_row produces it; its 24-bit depth (0xFFFFFFFF: none)
// and, where there is one, the world position interpolated like the texcoord (R11)
__device__ __forceinline__ unsigned pixel_fragment(WV v0, WV v1, WV v2, f3 w0, f3 w1, f3 w2, int px, int py, float shift, f3& out) {
  long long area = (long long)(v1.X - v0.X) * (long long)(v2.Y - v0.Y) - (long long)(v1.Y - v0.Y) * (long long)(v2.X - v0.X);
  if (area == 0) return 0xFFFFFFFFu;
  if (area < 0) {
    const WV t = v1;
    v1 = v2;
    v2 = t;
    const f3 tw = w1;
    w1 = w2;
    w2 = tw;
    area = -area;
  }
  const int dx0 = v2.X - v1.X, dy0 = v2.Y - v1.Y, dx1 = v0.X - v2.X, dy1 = v0.Y - v2.Y, dx2 = v1.X - v0.X, dy2 = v1.Y - v0.Y;
  const bool tl0 = dy0 < 0 || (dy0 == 0 && dx0 < 0), tl1 = dy1 < 0 || (dy1 == 0 && dx1 < 0), tl2 = dy2 < 0 || (dy2 == 0 && dx2 < 0);
  const long long Py = (long long)py * kSub + kSub / 2, Px = (long long)px * kSub + kSub / 2;
  const long long e0 = (long long)dx0 * (Py - v1.Y) - (long long)dy0 * (Px - v1.X);
  const long long e1 = (long long)dx1 * (Py - v2.Y) - (long long)dy1 * (Px - v2.X);
  const long long e2 = (long long)dx2 * (Py - v0.Y) - (long long)dy2 * (Px - v0.X);
  if (!((e0 > 0 || (e0 == 0 && tl0)) && (e1 > 0 || (e1 == 0 && tl1)) && (e2 > 0 || (e2 == 0 && tl2)))) return 0xFFFFFFFFu;
  const float inv = 1.f / (float)(double)area;
  const float b0 = (float)(double)e0 * inv, b1 = (float)(double)e1 * inv, b2 = (float)(double)e2 * inv;
  float q0, q1, q2, den;
  const unsigned d = disc_fragment(v0, v1, v2, b0, b1, b2, shift, q0, q1, q2, den);
  if (d < 0xFFFFFFu) {
    out.x = ((q0 * w0.x + q1 * w1.x) + q2 * w2.x) / den;
    out.y = ((q0 * w0.y + q1 * w1.y) + q2 * w2.y) / den;
    out.z = ((q0 * w0.z + q1 * w1.z) + q2 * w2.z) / den;
  }
  return d;
}

// a winner whose strip needs clipping (R8): its fan pieces in GL order, the first whose fragment has the winning depth
__device__ __noinline__ bool clipped_winner(const RenderArgs& a, const c4* cv, const f3* wc, int px, int py, float shift, unsigned dwin, f3& out) {
  const float tu[4] = {-1.f, 1.f, -1.f, 1.f}, tv[4] = {-1.f, -1.f, 1.f, 1.f};
  const int tri[2][3] = {{0, 1, 2}, {2, 1, 3}};
  for (int t = 0; t < 2; ++t) {
    CVW poly[9];
    for (int k = 0; k < 3; ++k) {
      const int i = tri[t][k];
      poly[k].c = cv[i];
      poly[k].u = tu[i];
      poly[k].v = tv[i];
      poly[k].w = wc[i];
    }
    const int n = clip_polygon(poly, 3);
    if (n < 3) continue;
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = ok && poly[k].c.w > 0.f;
    if (!ok) continue;
    const WV w0 = to_window(a, poly[0].c, poly[0].u, poly[0].v);
    WV wp = to_window(a, poly[1].c, poly[1].u, poly[1].v);
    for (int k = 2; k < n; ++k) {  // fan (0, k-1, k)
      const WV wk = to_window(a, poly[k].c, poly[k].u, poly[k].v);
      if (pixel_fragment(w0, wp, wk, poly[0].w, poly[k - 1].w, poly[k].w, px, py, shift, out) == dwin) return true;
      wp = wk;
    }
  }
  return false;
}

__device__ __forceinline__ float4 operator+(const float4& p, const float4& q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); }

// draw_global_surface_phong.frag:37-64 for colour c at world position v, normal n = signMult * normal (R12-R14); not clamped
__device__ __forceinline__ float4 phong(const f3& c, const f3& n, const f3& v, const f3& light) {
  const float4 ambient = make_float4(0.3f * c.x, 0.3f * c.y, 0.3f * c.z, 1.f);
  float4 diffuse = make_float4(0.f, 0.f, 0.f, 0.f), specular = make_float4(0.f, 0.f, 0.f, 0.f);
  const f3 lightDir = normalized3(mk3(light.x - v.x, light.y - v.y, light.z - v.z));
  const float NdotL = dot3(n, lightDir);
  if (NdotL > 0.f) diffuse = make_float4(c.x * NdotL, c.y * NdotL, c.z * NdotL, 1.f * NdotL);
  const float nl = dot3(n, lightDir);
  const f3 rVector = normalized3(mk3((2.f * n.x) * nl - lightDir.x, (2.f * n.y) * nl - lightDir.y, (2.f * n.z) * nl - lightDir.z));
  const f3 viewVector = normalized3(mk3(-v.x, -v.y, -v.z));
  const float RdotV = dot3(rVector, viewVector);
  if (RdotV > 0.f) {  // R13: pow(RdotV, 32) = five squarings
    float p = RdotV * RdotV;
    p = p * p;
    p = p * p;
    p = p * p;
    p = p * p;
    specular = make_float4(p, p, p, p);
  }
  return (ambient + diffuse) + specular;
}

struct ShadeArgs {
  float4 clear;
  float light[3];
  float sign;
};

// Pass A, per pixel of the offscreen buffer: the winner's Phong colour and depth, or the clear colour and depth 1.0
__global__ __launch_bounds__(256) void k_shaded_resolve(RenderArgs a, ShadeArgs sa, SurfelPlanes sp, size_t cap,
                                                        const unsigned long long* __restrict__ zbuf, float4* __restrict__ rgba,
                                                        unsigned* __restrict__ depth) {
  const int n = a.W * a.H;
  float Mv[16];
  launch_mvp(a, Mv);
  const f3 light = mk3(sa.light[0], sa.light[1], sa.light[2]);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    const unsigned long long key = zbuf[p];
    if (key == ~0ull) {
      rgba[p] = sa.clear;
      depth[p] = 0xFFFFFFu;
      continue;
    }
    const unsigned i = (unsigned)(key & 0xFFFFFFFFull), dwin = (unsigned)(key >> 40);
    const int px = p % a.W, py = p / a.W;
    const float4 pc = sp.pos[i], nr = sp.nrm[i];
    const float shift = pc.w <= a.threshold ? nr.w : 0.f;
    f3 wc[4];
    c4 cv[4];
    disc_world(pc, nr, wc);
    disc_corners(Mv, wc, cv);
    f3 v = mk3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));  // (every winner has its fragment: never kept)
    if ((outcode(cv[0]) | outcode(cv[1]) | outcode(cv[2]) | outcode(cv[3])) == 0u) {
      const float tu[4] = {-1.f, 1.f, -1.f, 1.f}, tv[4] = {-1.f, -1.f, 1.f, 1.f};
      WV w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = to_window(a, cv[k], tu[k], tv[k]);
      // GL strip order: (v0, v1, v2), (v2, v1, v3); the first fragment with the winning depth is the one GL_LESS kept
      if (pixel_fragment(w[0], w[1], w[2], wc[0], wc[1], wc[2], px, py, shift, v) != dwin)
        (void)pixel_fragment(w[2], w[1], w[3], wc[2], wc[1], wc[3], px, py, shift, v);
    } else {
      (void)clipped_winner(a, cv, wc, px, py, shift, dwin, v);
    }
    const f3 c = surfel_colour<false>(a, sp, cap, i);
    rgba[p] = phong(c, mk3(sa.sign * nr.x, sa.sign * nr.y, sa.sign * nr.z), v, light);
    depth[p] = dwin;
  }
}

__global__ void k_offscreen_init(unsigned long long* __restrict__ key, float4* __restrict__ rgba, unsigned* __restrict__ depth, int n,
                                 unsigned* __restrict__ clip_flag) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *clip_flag = 0u;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    key[p] = ~0ull;
    rgba[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    depth[p] = 0xFFFFFFu;
  }
}

__global__ void k_shaded_clear(unsigned long long* __restrict__ key, int n, unsigned* __restrict__ clip_flag) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *clip_flag = 0u;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) key[p] = ~0ull;
}

// R15: GL_LINEAR of an RGBA32F texture with GL_REPEAT (xyz only): texel origin s W - 0.5, fp32 weights, lerp a + w (b - a)
__device__ __forceinline__ f3 tex_linear(const float4* __restrict__ img, int W, int H, float s, float t) {
  const float x = s * (float)W - 0.5f, y = t * (float)H - 0.5f;
  const float fx = floorf(x), fy = floorf(y);
  const float ax = x - fx, ay = y - fy;
  int i0 = (int)fx % W, j0 = (int)fy % H;
  i0 += i0 < 0 ? W : 0;
  j0 += j0 < 0 ? H : 0;
  const int i1 = i0 + 1 == W ? 0 : i0 + 1, j1 = j0 + 1 == H ? 0 : j0 + 1;
  const float4 t00 = img[(size_t)j0 * W + i0], t10 = img[(size_t)j0 * W + i1];
  const float4 t01 = img[(size_t)j1 * W + i0], t11 = img[(size_t)j1 * W + i1];
  const f3 r0 = mk3(t00.x + ax * (t10.x - t00.x), t00.y + ax * (t10.y - t00.y), t00.z + ax * (t10.z - t00.z));
  const f3 r1 = mk3(t01.x + ax * (t11.x - t01.x), t01.y + ax * (t11.y - t01.y), t01.z + ax * (t11.z - t01.z));
  return mk3(r0.x + ay * (r1.x - r0.x), r0.y + ay * (r1.y - r0.y), r0.z + ay * (r1.z - r0.z));
}

__device__ __forceinline__ float luma(const f3& c) { return (c.x * 0.299f + c.y * 0.587f) + c.z * 0.114f; }

// fxaa.frag:34-88 at texcoord (s, t) of a W x H float buffer (R16, R18).  The N / E / W / S fetches of the shader reach no output
// and are not made.
__device__ __forceinline__ f3 fxaa(const float4* __restrict__ img, int W, int H, float s, float t) {
  const float ivx = 1.f / (float)W, ivy = 1.f / (float)H;
  const f3 rgbNW = tex_linear(img, W, H, s + -1.f * ivx, t + -1.f * ivy);
  const f3 rgbNE = tex_linear(img, W, H, s + 1.f * ivx, t + -1.f * ivy);
  const f3 rgbSW = tex_linear(img, W, H, s + -1.f * ivx, t + 1.f * ivy);
  const f3 rgbSE = tex_linear(img, W, H, s + 1.f * ivx, t + 1.f * ivy);
  const f3 rgbM = tex_linear(img, W, H, s, t);
  const float lumaNW = luma(rgbNW), lumaNE = luma(rgbNE), lumaSW = luma(rgbSW), lumaSE = luma(rgbSE), lumaM = luma(rgbM);
  const float lumaMin = fminf(lumaM, fminf(fminf(lumaNW, lumaNE), fminf(lumaSW, lumaSE)));
  const float lumaMax = fmaxf(lumaM, fmaxf(fmaxf(lumaNW, lumaNE), fmaxf(lumaSW, lumaSE)));
  float dx = -((lumaNW + lumaNE) - (lumaSW + lumaSE));
  float dy = (lumaNW + lumaSW) - (lumaNE + lumaSE);
  const float dirReduce = fmaxf((((lumaNW + lumaNE) + lumaSW) + lumaSE) * (0.25f * (1.f / 8.f)), 1.f / 128.f);
  const float rcpDirMin = 1.f / (fminf(fabsf(dx), fabsf(dy)) + dirReduce);
  dx = fminf(8.f, fmaxf(-8.f, dx * rcpDirMin)) * ivx;
  dy = fminf(8.f, fmaxf(-8.f, dy * rcpDirMin)) * ivy;
  const float c1 = 1.f / 3.f - 0.5f, c2 = 2.f / 3.f - 0.5f;
  const f3 a1 = tex_linear(img, W, H, s + dx * c1, t + dy * c1), a2 = tex_linear(img, W, H, s + dx * c2, t + dy * c2);
  const f3 rgbA = mk3(0.5f * (a1.x + a2.x), 0.5f * (a1.y + a2.y), 0.5f * (a1.z + a2.z));
  const f3 b1 = tex_linear(img, W, H, s + dx * -0.5f, t + dy * -0.5f), b2 = tex_linear(img, W, H, s + dx * 0.5f, t + dy * 0.5f);
  const f3 rgbB = mk3(rgbA.x * 0.5f + 0.25f * (b1.x + b2.x), rgbA.y * 0.5f + 0.25f * (b1.y + b2.y), rgbA.z * 0.5f + 0.25f * (b1.z + b2.z));
  const float lumaB = luma(rgbB);
  return (lumaB < lumaMin || lumaB > lumaMax) ? rgbA : rgbB;
}

// Pass B, per pixel of the target: the FXAA quad at window depth 0.5 under GL_LESS, then the NEAREST depth blit (R17), which
// replaces depth and winner (as a draw with sequence number seq)
__global__ __launch_bounds__(256) void k_render_fxaa(const float4* __restrict__ img, const unsigned long long* __restrict__ skey,
                                                     const unsigned* __restrict__ sdepth, int SW, int SH, int W, int H, unsigned seq,
                                                     unsigned* __restrict__ color, unsigned* __restrict__ depth,
                                                     unsigned long long* __restrict__ key) {
  const int n = W * H;
  const unsigned quad = depth24(0.5f);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    const int x = p % W, y = p / W;
    if (quad < depth[p]) color[p] = rgba8(fxaa(img, SW, SH, ((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H));
    const int sx = (int)(((2ll * x + 1) * SW) / (2ll * W)), sy = (int)(((2ll * y + 1) * SH) / (2ll * H));
    const size_t q = (size_t)sy * SW + sx;
    const unsigned long long k = skey[q];
    depth[p] = sdepth[q];
    key[p] = k == ~0ull ? k : (k & ~(0xFFull << 32)) | ((unsigned long long)seq << 32);
  }
}

// ---- the live-frame clouds: FeedbackBuffer::render (include/dmslam_render_cloud.h) ----------------------------
// The reference fills a 60-byte vertex per pixel (vertex_feedback.{vert,geom}) and draws that buffer with the point program.  Here no
// buffer is made: pass 1 runs the emit test and the position of every source pixel and competes for the target pixel like
// k_render_points; pass 2 rebuilds, for the pixels this draw won, what the colour mode reads - the colour bytes, or the
// central-difference normal from the SAME depth image - from the source pixel e = x * rows + y held in the key.
struct CloudArgs {
  float mvp[16];
  const float* pose_dev;   // the view, as RenderArgs
  float model[16];         // the program's `pose` uniform
  const float* model_dev;  // the same in HBM (overrides model)
  const uchar4* rgba;
  const float* depth;  // metric; rows tightly packed
  int cols, rows;
  float cx, cy, ifx, ify, maxDepth;
  int W, H;
  float hw, hh;
  int colorType;
  unsigned seq;
};

// R19: clip = MVP_eff * (pose * (p, 1)): two matrix-vector products, each row accumulated left to right, no 4 x 4 product
__host__ __device__ inline c4 clip_of4(const float* M, const c4& v) {
  c4 r;
  r.x = ((M[0] * v.x + M[1] * v.y) + M[2] * v.z) + M[3] * v.w;
  r.y = ((M[4] * v.x + M[5] * v.y) + M[6] * v.z) + M[7] * v.w;
  r.z = ((M[8] * v.x + M[9] * v.y) + M[10] * v.z) + M[11] * v.w;
  r.w = ((M[12] * v.x + M[13] * v.y) + M[14] * v.z) + M[15] * v.w;
  return r;
}
__host__ __device__ inline c4 cloud_clip(const float* V, const float* P, float x, float y, float z) {
  c4 p1;
  p1.x = x, p1.y = y, p1.z = z, p1.w = 1.f;
  return clip_of4(V, clip_of4(P, p1));
}
// the launch's view (as launch_mvp) and model matrix
__device__ __forceinline__ void cloud_matrices(const CloudArgs& a, float* V, float* P) {
  if (a.pose_dev) {
#pragma unroll
    for (int k = 0; k < 16; ++k) P[k] = a.pose_dev[k];
    mvp_from_pose(a.mvp, P, V);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = a.mvp[k];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) P[k] = a.model_dev ? a.model_dev[k] : a.model[k];
}

// Pass 1, one thread per source pixel (row-major: coalesced depth reads; the atomicMin does not care about the order)
__global__ __launch_bounds__(256) void k_cloud_points(CloudArgs a, unsigned long long* __restrict__ zbuf) {
  float V[16], P[16];
  cloud_matrices(a, V, P);
  const int n = a.cols * a.rows;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    const float z = a.depth[p];
    if (!(z > 0.f && !(z > a.maxDepth))) continue;  // vertex_feedback.vert:55-62 + .geom:38: emitted iff 0 < z <= maxDepth
    const int py = p / a.cols, px = p - py * a.cols;
    const float x = uv_coord(px, a.cols) * (float)a.cols, y = uv_coord(py, a.rows) * (float)a.rows;
    if (!(surfel_confidence(x, y, a.cx, a.cy, 1.0f) > 0.f)) continue;  // draw_feedback.vert:37, threshold 0
    const f3 v = fb_vertex(a.depth, a.cols, px, py, x, y, a.cx, a.cy, a.ifx, a.ify);
    const unsigned e = (unsigned)px * (unsigned)a.rows + (unsigned)py;  // R21
    place_point(cloud_clip(V, P, v.x, v.y, v.z), a.W, a.H, a.hw, a.hh, ((unsigned long long)a.seq << 32) | (unsigned long long)e, zbuf);
  }
}

// Pass 2, per target pixel this draw won (draw_feedback.vert:39-54 for the winner's source pixel)
__global__ __launch_bounds__(256) void k_cloud_resolve(CloudArgs a, const unsigned long long* __restrict__ zbuf, unsigned* __restrict__ color,
                                                       unsigned* __restrict__ depth) {
  const int n = a.W * a.H;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += blockDim.x * gridDim.x) {
    const unsigned long long key = zbuf[p];
    if (key == ~0ull || (unsigned)((key >> 32) & 0xFFu) != a.seq) continue;
    const unsigned e = (unsigned)(key & 0xFFFFFFFFull);
    const int px = (int)(e / (unsigned)a.rows), py = (int)(e - (unsigned)px * (unsigned)a.rows);
    f3 c;
    if (a.colorType == 2) {
      const uchar4 b = a.rgba[(size_t)py * a.cols + px];
      c = decode_color(encode_color_bytes(b.x, b.y, b.z));  // vertex_feedback.vert:68, draw_feedback.vert:49
    } else {
      const float tx = uv_coord(px, a.cols), ty = uv_coord(py, a.rows);
      const float x = tx * (float)a.cols, y = ty * (float)a.rows;
      const f3 v = fb_vertex(a.depth, a.cols, px, py, x, y, a.cx, a.cy, a.ifx, a.ify);
      const f3 nl = fb_normal(a.depth, a.cols, a.rows, v, tx, ty, x, y, a.cx, a.cy, a.ifx, a.ify);  // R20: NEAREST taps
      c = a.colorType == 1 ? nl : shaded_grey(make_float4(nl.x, nl.y, nl.z, 0.f));
    }
    color[p] = rgba8(c);
    depth[p] = (unsigned)(key >> 40);
  }
}

// ---- the image panels: GUI::displayImg of DEPTH_NORM, Model, RGB and ModelImage (include/dmslam_render_panels.h, R22-R26) ------------
// Two shader passes (depth_norm.frag through ComputePack::compute, visualise_textures.frag through IndexMap::renderDepth) and a
// textured quad per panel.  A texel is fetched as four floats in [0, 1] from one of four kinds of source; the two "derived" kinds run
// the shader pass on the fly from the raw depth / the vertex image, which is how the fused column blits DEPTH_NORM and the Model image
// in the launch that also stores them: the same device functions, hence the same bytes, as the separate calls.
enum { kSrcRGBA8 = 0, kSrcL8 = 1, kSrcDepthNorm = 2, kSrcModelDepth = 3 };

struct PanelSrc {
  const void* data;  // image rows, tightly packed
  int W, H, kind;
  unsigned lo, hi;  // depth_norm.frag: uint(minVal), uint(maxVal)
  float maxv;       // maxVal, or visualise_textures.frag's maxDepth
};

// depth_norm.frag:12-18 stored by R26
__device__ __forceinline__ unsigned depth_norm_byte(unsigned v, unsigned lo, unsigned hi, float maxv) {
  return (v > lo && v < hi) ? unorm8(1.0f - (float)v / maxv) : 0u;
}
// visualise_textures.frag:12-23: a discarded texel keeps the clear colour (0, 0, 0, 0)
__device__ __forceinline__ unsigned model_depth_rgba(float z, float maxDepth) {
  if (z > maxDepth || z <= 0.f) return 0u;
  return unorm8(1.0f - z / maxDepth) * 0x01010101u;
}

// R25: a texel as floats, byte / 255; luminance expands to (L, L, L, 1)
__device__ __forceinline__ float4 panel_texel(const PanelSrc& s, int ix, int iy) {
  const size_t q = (size_t)iy * s.W + ix;
  unsigned px;
  if (s.kind == kSrcL8 || s.kind == kSrcDepthNorm) {
    const unsigned L = s.kind == kSrcL8 ? (unsigned)((const unsigned char*)s.data)[q]
                                        : depth_norm_byte((unsigned)((const unsigned short*)s.data)[q], s.lo, s.hi, s.maxv);
    const float l = (float)L / 255.f;
    return make_float4(l, l, l, 1.f);
  }
  if (s.kind == kSrcModelDepth)
    px = model_depth_rgba(((const float4*)s.data)[q].z, s.maxv);
  else
    px = ((const unsigned*)s.data)[q];
  return make_float4((float)(px & 255u) / 255.f, (float)((px >> 8) & 255u) / 255.f, (float)((px >> 16) & 255u) / 255.f, (float)(px >> 24) / 255.f);
}

// R22-R25: the colour bytes of viewport pixel (i, j) (j counted from the viewport's bottom row) of a vw x vh viewport
__device__ __forceinline__ unsigned panel_sample(const PanelSrc& s, int filter, int i, int j, int vw, int vh, float cr, float cg, float cb) {
  const float u = (((float)i + 0.5f) / (float)vw) * (float)s.W;             // R22
  const float v = (((float)(vh - 1 - j) + 0.5f) / (float)vh) * (float)s.H;  // flipped: the viewport's top row shows image row 0
  float4 c;
  if (filter == DMS_PANEL_NEAREST) {  // R23
    c = panel_texel(s, min((int)floorf(u), s.W - 1), min((int)floorf(v), s.H - 1));
  } else {  // R24
    const float x = u - 0.5f, y = v - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    const float ax = x - fx, ay = y - fy;
    const int i0 = min(max((int)fx, 0), s.W - 1), i1 = min(max((int)fx + 1, 0), s.W - 1);
    const int j0 = min(max((int)fy, 0), s.H - 1), j1 = min(max((int)fy + 1, 0), s.H - 1);
    const float4 t00 = panel_texel(s, i0, j0), t10 = panel_texel(s, i1, j0), t01 = panel_texel(s, i0, j1), t11 = panel_texel(s, i1, j1);
    const float w00 = (1.f - ax) * (1.f - ay), w10 = ax * (1.f - ay), w01 = (1.f - ax) * ay, w11 = ax * ay;
    c.x = ((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x;
    c.y = ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y;
    c.z = ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z;
    c.w = ((w00 * t00.w + w10 * t10.w) + w01 * t01.w) + w11 * t11.w;
  }
  return unorm8(c.x * cr) | (unorm8(c.y * cg) << 8) | (unorm8(c.z * cb) << 16) | (unorm8(c.w) << 24);  // R25, R9
}

// both shader passes over source pixels [4 q, 4 q + 4): either input may be null.  vec: the u16 row is 8-byte aligned (one ushort4
// load); the vertex row is always read as float4, the outputs are written as uchar4 / 32-bit words.
__device__ __forceinline__ void panel_passes(int q, int n, const unsigned short* __restrict__ depth, const float4* __restrict__ vertex,
                                             unsigned char* __restrict__ norm, unsigned* __restrict__ model, unsigned lo, unsigned hi,
                                             float maxv, float maxDepth, bool vec) {
  const int p0 = 4 * q;
  if (p0 + 3 < n) {
    if (depth) {
      unsigned v0, v1, v2, v3;
      if (vec) {
        const ushort4 d = ((const ushort4*)depth)[q];
        v0 = d.x, v1 = d.y, v2 = d.z, v3 = d.w;
      } else {
        v0 = depth[p0], v1 = depth[p0 + 1], v2 = depth[p0 + 2], v3 = depth[p0 + 3];
      }
      ((unsigned*)norm)[q] = depth_norm_byte(v0, lo, hi, maxv) | (depth_norm_byte(v1, lo, hi, maxv) << 8) |
                             (depth_norm_byte(v2, lo, hi, maxv) << 16) | (depth_norm_byte(v3, lo, hi, maxv) << 24);
    }
    if (vertex) {
#pragma unroll
      for (int k = 0; k < 4; ++k) model[p0 + k] = model_depth_rgba(vertex[p0 + k].z, maxDepth);
    }
  } else {
    for (int p = p0; p < n; ++p) {
      if (depth) norm[p] = (unsigned char)depth_norm_byte(depth[p], lo, hi, maxv);
      if (vertex) model[p] = model_depth_rgba(vertex[p].z, maxDepth);
    }
  }
}

__global__ __launch_bounds__(256) void k_panel_passes(int n, const unsigned short* __restrict__ depth, const float4* __restrict__ vertex,
                                                      unsigned char* __restrict__ norm, unsigned* __restrict__ model, unsigned lo, unsigned hi,
                                                      float maxv, float maxDepth, bool vec) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * q < n) panel_passes(q, n, depth, vertex, norm, model, lo, hi, maxv, maxDepth, vec);
}

// one blit, one thread per pixel of the viewport
__global__ __launch_bounds__(256) void k_panel_blit(PanelSrc s, int filter, dms_viewport vp, float cr, float cg, float cb,
                                                    unsigned* __restrict__ color, int TW) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= vp.w * vp.h) return;
  const int j = p / vp.w, i = p - j * vp.w;
  color[(size_t)(vp.y + j) * TW + (vp.x + i)] = panel_sample(s, filter, i, j, vp.w, vp.h, cr, cg, cb);
}

// the column in one launch: items [0, start[0]) are the quads of the two passes, [start[k], start[k + 1]) the pixels of panel k's
// viewport.  No item reads what another writes (the blits of DEPTH_NORM and Model run the pass per tap), and a pixel that a later
// panel of the mask also covers is left to that panel, as the separate calls in order leave it.
struct ColumnArgs {
  PanelSrc src[4];
  dms_viewport vp[4];
  int start[5];
  int mask, n, TW;
  unsigned char* norm;
  unsigned* model;
  unsigned* color;
  float maxDepth;
};
__global__ __launch_bounds__(256) void k_panel_column(ColumnArgs a) {
  const int it = blockIdx.x * blockDim.x + threadIdx.x;
  if (it < a.start[0]) {
    panel_passes(it, a.n, (const unsigned short*)a.src[0].data, (const float4*)a.src[1].data, a.norm, a.model, a.src[0].lo, a.src[0].hi,
                 a.src[0].maxv, a.maxDepth, true);
    return;
  }
  if (it >= a.start[4]) return;
  const int k = it < a.start[1] ? 0 : it < a.start[2] ? 1 : it < a.start[3] ? 2 : 3;
  const dms_viewport vp = a.vp[k];
  const int p = it - a.start[k];
  const int j = p / vp.w, i = p - j * vp.w;
  const int x = vp.x + i, y = vp.y + j;
  for (int m = k + 1; m < 4; ++m) {
    const dms_viewport o = a.vp[m];
    if (((a.mask >> m) & 1) && x >= o.x && x < o.x + o.w && y >= o.y && y < o.y + o.h) return;
  }
  // LINEAR: RGB and DEPTH_NORM (Context.h:158-160, 179-181); NEAREST: drawTexture and imageTexture (IndexMap.cpp:42-47, 59-65)
  const int filter = (k == DMS_PANEL_DEPTH_NORM || k == DMS_PANEL_RGB) ? DMS_PANEL_LINEAR : DMS_PANEL_NEAREST;
  a.color[(size_t)y * a.TW + x] = panel_sample(a.src[k], filter, i, j, vp.w, vp.h, 1.f, 1.f, 1.f);
}

// GLSL's uint(float) where C leaves it open: clamped to [0, 2^32 - 1], 0 for NaN
unsigned to_uint(float x) { return !(x > 0.f) ? 0u : x >= 4294967296.f ? 0xFFFFFFFFu : (unsigned)x; }

bool viewport_ok(const dms_render_target* t, const dms_viewport& v) {
  return v.w > 0 && v.h > 0 && v.x >= 0 && v.y >= 0 && v.x <= t->width - v.w && v.y <= t->height - v.h;
}
bool panel_image_ok(const dms_image2d* im, size_t elem) {
  return im->data && im->cols > 0 && im->rows > 0 && im->cols <= DMS_RENDER_MAX_EXTENT && im->rows <= DMS_RENDER_MAX_EXTENT &&
         im->pitch == (size_t)im->cols * elem;
}

int surfel_blocks(size_t upper) {
  size_t b = (upper + 255) / 256;
  if (b < 1) b = 1;
  if (b > 4096) b = 4096;
  return (int)b;
}
unsigned byte_of(float c) { return (unsigned)floorf(fminf(fmaxf(c, 0.f), 1.f) * 255.f + 0.5f); }

}  // namespace
}  // namespace dms

extern "C" {

int dms_render_target_create(dms_render_target** out, int width, int height) {
  DMS_REQUIRE(out, "null argument");
  *out = nullptr;
  DMS_REQUIRE(width > 0 && height > 0 && width <= DMS_RENDER_MAX_EXTENT && height <= DMS_RENDER_MAX_EXTENT, "extent out of range");
  dms_render_target* t = new dms_render_target();
  t->width = width;
  t->height = height;
  const size_t n = (size_t)width * height;
  hipError_t e = hipMalloc((void**)&t->key, n * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&t->color, n * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&t->depth, n * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&t->clip_flag, 256);
  if (e != hipSuccess) {
    dms_render_target_destroy(t);
    return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
  }
  const float black[4] = {0.f, 0.f, 0.f, 0.f};
  int rc = dms_render_clear(t, black, nullptr);
  if (!rc) {
    e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
  }
  if (rc) {
    dms_render_target_destroy(t);
    return rc;
  }
  *out = t;
  return DMS_OK;
}

int dms_render_target_destroy(dms_render_target* t) {
  if (!t) return DMS_OK;
  if (t->key) (void)hipFree(t->key);
  if (t->color) (void)hipFree(t->color);
  if (t->depth) (void)hipFree(t->depth);
  if (t->clip_flag) (void)hipFree(t->clip_flag);
  delete t;
  return DMS_OK;
}

int dms_render_clear(dms_render_target* t, const float clear_rgba[4], dms_stream s) {
  DMS_REQUIRE(t && clear_rgba, "null argument");
  const unsigned c = byte_of(clear_rgba[0]) | (byte_of(clear_rgba[1]) << 8) | (byte_of(clear_rgba[2]) << 16) | (byte_of(clear_rgba[3]) << 24);
  const int n = t->width * t->height;
  hipLaunchKernelGGL(k_render_clear, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, (hipStream_t)s, t->key, t->color, t->depth, n, c, t->clip_flag);
  DMS_CHECK_LAUNCH();
  t->seq = 0;
  return DMS_OK;
}

int dms_render_draw(dms_render_target* t, dms_model* m, const dms_render_params* p, dms_stream s) {
  DMS_REQUIRE(t && m && p, "null argument");
  DMS_REQUIRE(p->color_type >= 0 && p->color_type <= 4, "color_type must be 0..4");
  DMS_REQUIRE(p->time_idx >= 0 && p->time_idx < DMS_MAX_SENSORS, "time_idx out of range");
  DMS_REQUIRE(t->seq < DMS_RENDER_MAX_DRAWS, "too many draws since the last clear");
  DMS_REQUIRE(!m->pending_update, "a deferred update pass is still pending (the frame step has not finished its index map)");
  RenderArgs a;
  memcpy(a.mvp, p->mvp, sizeof(a.mvp));
  a.pose_dev = p->pose_dev;
  a.W = t->width;
  a.H = t->height;
  a.hw = (float)t->width * 0.5f;
  a.hh = (float)t->height * 0.5f;
  a.threshold = p->threshold;
  a.unstable = p->draw_unstable ? 1 : 0;
  a.window = p->draw_window ? 1 : 0;
  a.colorType = p->color_type;
  a.time = p->time;
  a.timeIdx = p->time_idx;
  a.timeDelta = p->time_delta;
  a.cluster = p->use_cluster_color ? 1 : 0;
  a.cc[0] = p->cluster_color[0];
  a.cc[1] = p->cluster_color[1];
  a.cc[2] = p->cluster_color[2];
  a.seq = (unsigned)t->seq;
  const hipStream_t st = (hipStream_t)s;
  const SurfelPlanes sp = m->buf[m->cur];
  const int g = surfel_blocks(m->count_upper);
  if (p->draw_points) {
    hipLaunchKernelGGL(k_render_points, dim3(g), dim3(256), 0, st, a, sp, m->d_count, t->key);
    DMS_CHECK_LAUNCH();
  } else {
    hipLaunchKernelGGL(k_render_discs<false>, dim3(g), dim3(256), 0, st, a, sp, m->d_count, t->key, t->clip_flag);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_render_discs<true>, dim3(g), dim3(256), 0, st, a, sp, m->d_count, t->key, t->clip_flag);
    DMS_CHECK_LAUNCH();
  }
  const int n = t->width * t->height;
  const dim3 rg(min((n + 255) / 256, 2048));
  if (p->draw_points)
    hipLaunchKernelGGL(k_render_resolve<true>, rg, dim3(256), 0, st, a, sp, m->cap, t->key, t->color, t->depth);
  else
    hipLaunchKernelGGL(k_render_resolve<false>, rg, dim3(256), 0, st, a, sp, m->cap, t->key, t->color, t->depth);
  DMS_CHECK_LAUNCH();
  ++t->seq;
  return DMS_OK;
}

int dms_render_images(dms_render_target* t, dms_image2d* rgba8, dms_image2d* depth24_u32, dms_image2d* winner_u64) {
  DMS_REQUIRE(t, "null argument");
  if (rgba8) *rgba8 = dms_image2d{t->color, (size_t)t->width * 4, t->height, t->width};
  if (depth24_u32) *depth24_u32 = dms_image2d{t->depth, (size_t)t->width * 4, t->height, t->width};
  if (winner_u64) *winner_u64 = dms_image2d{t->key, (size_t)t->width * 8, t->height, t->width};
  return DMS_OK;
}

int dms_render_target_size(const dms_render_target* t, int* width, int* height) {
  DMS_REQUIRE(t && width && height, "null argument");
  *width = t->width;
  *height = t->height;
  return DMS_OK;
}

int dms_render_mvp_from_pose(const float proj16[16], const float pose16[16], float out16[16]) {
  DMS_REQUIRE(proj16 && pose16 && out16, "null argument");
  mvp_from_pose(proj16, pose16, out16);
  return DMS_OK;
}

int dms_render_frustum(int w, int h, float fu, float fv, float u0, float v0, float znear, float zfar, float out16[16]) {
  DMS_REQUIRE(out16, "null argument");
  DMS_REQUIRE(w > 0 && h > 0 && fu != 0.f && fv != 0.f && znear > 0.f && zfar > znear, "bad frustum");
  const double n = znear, f = zfar;
  const double L = -(double)u0 * n / fu, R = ((double)w - u0) * n / fu;
  const double B = -(double)v0 * n / fv, T = ((double)h - v0) * n / fv;
  double P[16] = {0};
  P[0] = 2 * n / (R - L);
  P[2] = (R + L) / (R - L);
  P[5] = 2 * n / (T - B);
  P[6] = (T + B) / (T - B);
  P[10] = -(f + n) / (f - n);
  P[11] = -(2 * f * n) / (f - n);
  P[14] = -1.0;
  for (int k = 0; k < 16; ++k) out16[k] = (float)P[k];
  return DMS_OK;
}

}  // extern "C"

// ---- the shaded view (include/dmslam_render_shaded.h) -------------------------------------------------------------------------
struct dms_render_offscreen {
  int width = 0, height = 0;
  unsigned long long* key = nullptr;  // [H][W] (window rows)
  float4* rgba = nullptr;             // RGBA32F
  unsigned* depth = nullptr;          // 24-bit depth
  unsigned* clip_flag = nullptr;      // 1 when the last draw met a surfel to clip (R8)
};

extern "C" {

int dms_render_offscreen_create(dms_render_offscreen** out, int width, int height) {
  DMS_REQUIRE(out, "null argument");
  *out = nullptr;
  DMS_REQUIRE(width > 0 && height > 0 && width <= DMS_RENDER_MAX_EXTENT && height <= DMS_RENDER_MAX_EXTENT, "extent out of range");
  dms_render_offscreen* o = new dms_render_offscreen();
  o->width = width;
  o->height = height;
  const size_t n = (size_t)width * height;
  hipError_t e = hipMalloc((void**)&o->key, n * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&o->rgba, n * 16);
  if (e == hipSuccess) e = hipMalloc((void**)&o->depth, n * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&o->clip_flag, 256);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_offscreen_init, dim3(min(((int)n + 255) / 256, 2048)), dim3(256), 0, nullptr, o->key, o->rgba, o->depth, (int)n,
                       o->clip_flag);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    dms_render_offscreen_destroy(o);
    return hip_fail(e, "dms_render_offscreen_create", __FILE__, __LINE__);
  }
  *out = o;
  return DMS_OK;
}

int dms_render_offscreen_destroy(dms_render_offscreen* o) {
  if (!o) return DMS_OK;
  if (o->key) (void)hipFree(o->key);
  if (o->rgba) (void)hipFree(o->rgba);
  if (o->depth) (void)hipFree(o->depth);
  if (o->clip_flag) (void)hipFree(o->clip_flag);
  delete o;
  return DMS_OK;
}

int dms_render_offscreen_size(const dms_render_offscreen* o, int* width, int* height) {
  DMS_REQUIRE(o && width && height, "null argument");
  *width = o->width;
  *height = o->height;
  return DMS_OK;
}

int dms_render_shaded_draw(dms_render_offscreen* o, dms_model* m, const dms_render_params* p, const float light_pos[3], float sign_mult,
                           const float clear_rgba[4], dms_stream s) {
  DMS_REQUIRE(o && m && p && light_pos && clear_rgba, "null argument");
  DMS_REQUIRE(!p->draw_points, "the shaded view draws discs (draw_points must be 0)");
  DMS_REQUIRE(!p->use_cluster_color, "the shaded view has no cluster colour");
  DMS_REQUIRE(p->color_type >= 0 && p->color_type <= 3, "color_type must be 0..3");
  DMS_REQUIRE(p->time_idx >= 0 && p->time_idx < DMS_MAX_SENSORS, "time_idx out of range");
  DMS_REQUIRE(!m->pending_update, "a deferred update pass is still pending (the frame step has not finished its index map)");
  RenderArgs a;
  memcpy(a.mvp, p->mvp, sizeof(a.mvp));
  a.pose_dev = p->pose_dev;
  a.W = o->width;
  a.H = o->height;
  a.hw = (float)o->width * 0.5f;
  a.hh = (float)o->height * 0.5f;
  a.threshold = p->threshold;
  a.unstable = p->draw_unstable ? 1 : 0;
  a.window = p->draw_window ? 1 : 0;
  a.colorType = p->color_type;
  a.time = p->time;
  a.timeIdx = p->time_idx;
  a.timeDelta = p->time_delta;
  a.cluster = 0;
  a.cc[0] = a.cc[1] = a.cc[2] = 0.f;
  a.seq = 0u;
  ShadeArgs sa;
  sa.clear = make_float4(clear_rgba[0], clear_rgba[1], clear_rgba[2], clear_rgba[3]);
  sa.light[0] = light_pos[0];
  sa.light[1] = light_pos[1];
  sa.light[2] = light_pos[2];
  sa.sign = sign_mult;
  const hipStream_t st = (hipStream_t)s;
  const SurfelPlanes sp = m->buf[m->cur];
  const int n = o->width * o->height;
  const dim3 rg(min((n + 255) / 256, 2048));
  hipLaunchKernelGGL(k_shaded_clear, rg, dim3(256), 0, st, o->key, n, o->clip_flag);
  DMS_CHECK_LAUNCH();
  const int g = surfel_blocks(m->count_upper);
  hipLaunchKernelGGL(k_render_discs<false>, dim3(g), dim3(256), 0, st, a, sp, m->d_count, o->key, o->clip_flag);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_render_discs<true>, dim3(g), dim3(256), 0, st, a, sp, m->d_count, o->key, o->clip_flag);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_shaded_resolve, rg, dim3(256), 0, st, a, sa, sp, m->cap, o->key, o->rgba, o->depth);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int dms_render_fxaa(dms_render_target* t, const dms_render_offscreen* o, dms_stream s) {
  DMS_REQUIRE(t && o, "null argument");
  DMS_REQUIRE(t->seq < DMS_RENDER_MAX_DRAWS, "too many draws since the last clear");
  const int n = t->width * t->height;
  hipLaunchKernelGGL(k_render_fxaa, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, (hipStream_t)s, o->rgba, o->key, o->depth, o->width,
                     o->height, t->width, t->height, (unsigned)t->seq, t->color, t->depth, t->key);
  DMS_CHECK_LAUNCH();
  ++t->seq;
  return DMS_OK;
}

int dms_render_offscreen_images(dms_render_offscreen* o, dms_image2d* rgba32f, dms_image2d* depth24_u32, dms_image2d* winner_u64) {
  DMS_REQUIRE(o, "null argument");
  if (rgba32f) *rgba32f = dms_image2d{o->rgba, (size_t)o->width * 16, o->height, o->width};
  if (depth24_u32) *depth24_u32 = dms_image2d{o->depth, (size_t)o->width * 4, o->height, o->width};
  if (winner_u64) *winner_u64 = dms_image2d{o->key, (size_t)o->width * 8, o->height, o->width};
  return DMS_OK;
}

}  // extern "C"

// ---- the live-frame clouds (include/dmslam_render_cloud.h) --------------------------------------------------------------------
extern "C" {

int dms_render_cloud_clip(const float mvp_eff16[16], const float model_pose16[16], const float point3[3], float clip4[4]) {
  DMS_REQUIRE(mvp_eff16 && model_pose16 && point3 && clip4, "null argument");
  const c4 c = cloud_clip(mvp_eff16, model_pose16, point3[0], point3[1], point3[2]);
  clip4[0] = c.x, clip4[1] = c.y, clip4[2] = c.z, clip4[3] = c.w;
  return DMS_OK;
}

int dms_render_cloud(dms_render_target* t, const dms_image2d* rgba, const dms_image2d* depth_metric, const dms_camera* cam, float max_depth,
                     const dms_render_cloud_params* p, dms_stream s) {
  DMS_REQUIRE(t && rgba && depth_metric && cam && p, "null argument");
  DMS_REQUIRE(rgba->data && depth_metric->data, "null image");
  DMS_REQUIRE(depth_metric->cols > 0 && depth_metric->rows > 0 && rgba->cols == depth_metric->cols && rgba->rows == depth_metric->rows,
              "shape mismatch");
  DMS_REQUIRE(rgba->pitch == (size_t)rgba->cols * 4 && depth_metric->pitch == (size_t)depth_metric->cols * 4, "rows must be tightly packed");
  // (2^30 pixels: the grid-stride index of pass 1 and the source index e of the key stay far inside 31 bits)
  DMS_REQUIRE((long long)depth_metric->cols * depth_metric->rows <= DMS_CLOUD_MAX_PIXELS, "image too large");
  DMS_REQUIRE(p->color_type >= 0 && p->color_type <= 2, "color_type must be 0..2");
  DMS_REQUIRE(t->seq < DMS_RENDER_MAX_DRAWS, "too many draws since the last clear");
  CloudArgs a;
  memcpy(a.mvp, p->mvp, sizeof(a.mvp));
  a.pose_dev = p->pose_dev;
  memcpy(a.model, p->model_pose, sizeof(a.model));
  a.model_dev = p->model_pose_dev;
  a.rgba = (const uchar4*)rgba->data;
  a.depth = (const float*)depth_metric->data;
  a.cols = depth_metric->cols;
  a.rows = depth_metric->rows;
  a.cx = cam->cx;
  a.cy = cam->cy;
  a.ifx = 1.0f / cam->fx;  // cam = (cx, cy, 1/fx, 1/fy), float reciprocals (FeedbackBuffer.cpp:93-96)
  a.ify = 1.0f / cam->fy;
  a.maxDepth = max_depth;
  a.W = t->width;
  a.H = t->height;
  a.hw = (float)t->width * 0.5f;
  a.hh = (float)t->height * 0.5f;
  a.colorType = p->color_type;
  a.seq = (unsigned)t->seq;
  const hipStream_t st = (hipStream_t)s;
  const int ns = a.cols * a.rows, n = t->width * t->height;
  hipLaunchKernelGGL(k_cloud_points, dim3(min((ns + 255) / 256, 2048)), dim3(256), 0, st, a, t->key);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cloud_resolve, dim3(min((n + 255) / 256, 2048)), dim3(256), 0, st, a, t->key, t->color, t->depth);
  DMS_CHECK_LAUNCH();
  ++t->seq;
  return DMS_OK;
}

}  // extern "C"

// ---- the image panels (include/dmslam_render_panels.h) ------------------------------------------------------------------------------
extern "C" {

int dms_panels_create(dms_panels** out, int width, int height) {
  DMS_REQUIRE(out, "null argument");
  *out = nullptr;
  DMS_REQUIRE(width > 0 && height > 0 && width <= DMS_RENDER_MAX_EXTENT && height <= DMS_RENDER_MAX_EXTENT, "extent out of range");
  dms_panels* p = new dms_panels();
  p->width = width;
  p->height = height;
  const size_t n = (size_t)width * height;
  hipError_t e = hipMalloc((void**)&p->norm, (n + 3) / 4 * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&p->model, n * 4);
  if (e == hipSuccess) e = hipMemset(p->norm, 0, (n + 3) / 4 * 4);
  if (e == hipSuccess) e = hipMemset(p->model, 0, n * 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    dms_panels_destroy(p);
    return hip_fail(e, "dms_panels_create", __FILE__, __LINE__);
  }
  *out = p;
  return DMS_OK;
}

int dms_panels_destroy(dms_panels* p) {
  if (!p) return DMS_OK;
  if (p->norm) (void)hipFree(p->norm);
  if (p->model) (void)hipFree(p->model);
  delete p;
  return DMS_OK;
}

int dms_panels_images(dms_panels* p, dms_image2d* depth_norm_l8, dms_image2d* model_rgba8) {
  DMS_REQUIRE(p, "null argument");
  if (depth_norm_l8) *depth_norm_l8 = dms_image2d{p->norm, (size_t)p->width, p->height, p->width};
  if (model_rgba8) *model_rgba8 = dms_image2d{p->model, (size_t)p->width * 4, p->height, p->width};
  return DMS_OK;
}

int dms_depth_norm(dms_panels* p, const dms_image2d* depth_u16, float min_val, float max_val, dms_stream s) {
  DMS_REQUIRE(p && depth_u16, "null argument");
  DMS_REQUIRE(panel_image_ok(depth_u16, 2), "null or empty image, or padded rows");
  DMS_REQUIRE(depth_u16->cols == p->width && depth_u16->rows == p->height, "shape mismatch");
  const int n = p->width * p->height, q = (n + 3) / 4;
  hipLaunchKernelGGL(k_panel_passes, dim3((q + 255) / 256), dim3(256), 0, (hipStream_t)s, n, (const unsigned short*)depth_u16->data,
                     (const float4*)nullptr, p->norm, p->model, to_uint(min_val), to_uint(max_val), max_val, 0.f,
                     ((uintptr_t)depth_u16->data & 7u) == 0);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int dms_model_depth_image(dms_panels* p, const dms_image2d* vertex_rgba32f, float max_depth, dms_stream s) {
  DMS_REQUIRE(p && vertex_rgba32f, "null argument");
  DMS_REQUIRE(panel_image_ok(vertex_rgba32f, 16), "null or empty image, or padded rows");
  DMS_REQUIRE(((uintptr_t)vertex_rgba32f->data & 15u) == 0, "the vertex image must be 16-byte aligned");
  DMS_REQUIRE(vertex_rgba32f->cols == p->width && vertex_rgba32f->rows == p->height, "shape mismatch");
  const int n = p->width * p->height, q = (n + 3) / 4;
  hipLaunchKernelGGL(k_panel_passes, dim3((q + 255) / 256), dim3(256), 0, (hipStream_t)s, n, (const unsigned short*)nullptr,
                     (const float4*)vertex_rgba32f->data, p->norm, p->model, 0u, 0u, 0.f, max_depth, false);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

int dms_render_blit(dms_render_target* t, const dms_image2d* image, int format, int filter, const dms_viewport* vp, const float color_rgb[3],
                    dms_stream s) {
  DMS_REQUIRE(t && image && vp && color_rgb, "null argument");
  DMS_REQUIRE(format == DMS_PANEL_RGBA8 || format == DMS_PANEL_L8, "format must be DMS_PANEL_RGBA8 or DMS_PANEL_L8");
  DMS_REQUIRE(filter == DMS_PANEL_NEAREST || filter == DMS_PANEL_LINEAR, "filter must be DMS_PANEL_NEAREST or DMS_PANEL_LINEAR");
  DMS_REQUIRE(panel_image_ok(image, format == DMS_PANEL_RGBA8 ? 4 : 1), "null or empty image, or padded rows");
  DMS_REQUIRE(format != DMS_PANEL_RGBA8 || ((uintptr_t)image->data & 3u) == 0, "an RGBA8 image must be 4-byte aligned");
  DMS_REQUIRE(viewport_ok(t, *vp), "the viewport is empty or leaves the target");
  PanelSrc src{image->data, image->cols, image->rows, format == DMS_PANEL_RGBA8 ? kSrcRGBA8 : kSrcL8, 0u, 0u, 0.f};
  const int n = vp->w * vp->h;
  hipLaunchKernelGGL(k_panel_blit, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, src, filter, *vp, color_rgb[0], color_rgb[1],
                     color_rgb[2], t->color, t->width);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}

}  // extern "C"

namespace dms {
int drawPanelColumn(dms_render_target* t, dms_panels* p, const dms_image2d* rgba, const dms_image2d* depth_u16, const dms_image2d* model_rgba,
                    const dms_image2d* vertex, const dms_viewport* viewports, float depth_cutoff, int which_mask, hipStream_t s) {
  DMS_REQUIRE(which_mask >= 0 && which_mask <= DMS_PANEL_ALL, "which_mask must be 0..15");
  DMS_REQUIRE(panel_image_ok(rgba, 4) && panel_image_ok(depth_u16, 2) && panel_image_ok(model_rgba, 4) && panel_image_ok(vertex, 16),
              "the context's images are not tightly packed");
  const int W = p->width, H = p->height;
  DMS_REQUIRE(rgba->cols == W && rgba->rows == H && depth_u16->cols == W && depth_u16->rows == H && model_rgba->cols == W &&
                  model_rgba->rows == H && vertex->cols == W && vertex->rows == H,
              "the panels are of another size than the context");
  DMS_REQUIRE(((uintptr_t)depth_u16->data & 7u) == 0 && ((uintptr_t)vertex->data & 15u) == 0 && ((uintptr_t)rgba->data & 3u) == 0 &&
                  ((uintptr_t)model_rgba->data & 3u) == 0,
              "misaligned image");
  ColumnArgs a;
  const float maxv = depth_cutoff * 1000.f;  // normaliseDepth (ElasticFusion.cpp:774-775)
  a.src[DMS_PANEL_DEPTH_NORM] = PanelSrc{depth_u16->data, W, H, kSrcDepthNorm, to_uint(0.3f * 1000.f), to_uint(maxv), maxv};
  a.src[DMS_PANEL_MODEL] = PanelSrc{vertex->data, W, H, kSrcModelDepth, 0u, 0u, depth_cutoff};
  a.src[DMS_PANEL_RGB] = PanelSrc{rgba->data, W, H, kSrcRGBA8, 0u, 0u, 0.f};
  a.src[DMS_PANEL_MODEL_IMAGE] = PanelSrc{model_rgba->data, W, H, kSrcRGBA8, 0u, 0u, 0.f};
  a.n = W * H;
  int items = (a.n + 3) / 4;
  a.start[0] = items;
  for (int k = 0; k < 4; ++k) {
    if ((which_mask >> k) & 1) {
      DMS_REQUIRE(viewport_ok(t, viewports[k]), "a viewport is empty or leaves the target");
      a.vp[k] = viewports[k];
      items += viewports[k].w * viewports[k].h;
    } else {
      a.vp[k] = dms_viewport{0, 0, 0, 0};
    }
    a.start[k + 1] = items;
  }
  a.mask = which_mask;
  a.TW = t->width;
  a.norm = p->norm;
  a.model = p->model;
  a.color = t->color;
  a.maxDepth = depth_cutoff;
  hipLaunchKernelGGL(k_panel_column, dim3((items + 255) / 256), dim3(256), 0, s, a);
  DMS_CHECK_LAUNCH();
  return DMS_OK;
}
}  // namespace dms
