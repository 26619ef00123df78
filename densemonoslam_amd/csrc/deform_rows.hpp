// Row and weight arithmetic of the deformation graph (the reference's Utils/DeformationGraph.cpp with k = 4), written once for
// the kernels of deform.hip and for a plain host build (tests/deform_rows_host.cpp, g++): the neighbour rule, the node search and
// weights of one vertex, the residual and Jacobian entries of one rotation, regularisation and constraint row, and
// computeVertexPosition.  Plain pointers only; no HIP type crosses this header.
//
// ORDER RULES (tests/deform_ref.py restates the same and is the yardstick; both sides give the same bits):
//   * float expressions are evaluated left to right as written, no fused multiply-add (the library is built with
//     -ffp-contract=off): a matrix row times a vector is (R(r,0) x + R(r,1) y) + R(r,2) z, a dot product (a0 b0 + a1 b1) + a2 b2;
//   * a norm is sqrtf((dx*dx + dy*dy) + dz*dz);
//   * both sorts (20 distances, four node ids) are stable;
//   * pow(x, 2) is x * x in double;
//   * a double weight that multiplies a float vector is rounded to float first (Eigen converts the scalar operand to the
//     expression's scalar type);
//   * a rotation is nine floats in Eigen's column-major order (R(r, c) = R[3 c + r]), which is also the order of a node's first
//     nine unknowns (DeformationGraph.cpp:971-981) and of the node table (Deformation.cpp:198).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMS_DR_HD __host__ __device__ __forceinline__
#else
#define DMS_DR_HD inline
#endif

namespace dms {
namespace dr {

constexpr int K = 4;          // DeformationGraph(4, ...), Deformation.cpp:22
constexpr int LOOKBACK = 20;  // DeformationGraph.cpp:292
constexpr int NVAR = 12;      // DeformationGraph.h:119-122
constexpr int ROT_ROWS = 6, REG_ROWS = 3, CON_ROWS = 3;
// The four nodes of a vertex lie in LOOKBACK consecutive nodes and a regularisation edge spans at most K nodes, so no row of the
// Jacobian couples two nodes further apart than this many blocks of NVAR columns.
constexpr int HALF_BAND_BLOCKS = LOOKBACK - 1;
// sqrt(wReg) = sqrt(10.0) and sqrt(wCon) = sqrt(100.0) in double (DeformationGraph.cpp:26-27), correctly rounded
constexpr double SQRT_WREG = 0x1.94c583ada5b53p+1;
constexpr double SQRT_WCON = 10.0;

// connectGraphSeq (DeformationGraph.cpp:252-288): the `slot`-th neighbour (0..3, in push_back order) of node j of n >= 5 nodes
DMS_DR_HD int neighbour(int j, int n, int slot) {
  if (j < K / 2) return slot < j ? slot : slot + 1;
  if (j >= n - K / 2) {
    const int base = n - (K + 1);
    return base + (slot < j - base ? slot : slot + 1);
  }
  const int step = slot / 2 + 1;
  return (slot & 1) ? j + step : j - step;
}

DMS_DR_HD float norm3(float dx, float dy, float dz) { return sqrtf((dx * dx + dy * dy) + dz * dz); }

DMS_DR_HD long long llabs_(long long v) { return v < 0 ? -v : v; }

// The binary search of weightVerticesSeq (:301-347) with its three-way nearest pick.  times: the nodes' times, ascending.
// When the vertex is older than every node the reference compares against the element before the first (imax = -1); whichever
// way that comparison falls, the window below starts at node 0 and lists the nodes in ascending order, so 0 is returned.
DMS_DR_HD int find_node(const float* nodes4, int n, long long vt) {
  int imin = 0, imax = n - 1, imid = (imin + imax) / 2;
  while (imax >= imin) {
    imid = (imin + imax) / 2;
    const long long t = (long long)nodes4[4 * imid + 3];
    if (t < vt)
      imin = imid + 1;
    else if (t > vt)
      imax = imid - 1;
    else
      break;
  }
  imin = imin < n - 1 ? imin : n - 1;
  if (imax < 0) return 0;
  const long long a = llabs_((long long)nodes4[4 * imin + 3] - vt), b = llabs_((long long)nodes4[4 * imid + 3] - vt),
                  c = llabs_((long long)nodes4[4 * imax + 3] - vt);
  if (a <= b && a <= c) return imin;
  if (b <= a && b <= c) return imid;
  return imax;
}

// weightVerticesSeq (:290-405) for one vertex: up to LOOKBACK nodes backwards from the found one, extended forwards when fewer lie
// behind, stable sort by distance, dMax = the (K+1)-th distance, weights (1 - d / dMax)^2 normalised, sorted by node id.
// nodes4: n rows {x, y, z, time}, n >= 5.
DMS_DR_HD void weigh_vertex(const float* nodes4, int n, const float* p, long long vt, int ids[K], double w[K]) {
  const int found = find_node(nodes4, n, vt);
  float dist[LOOKBACK];
  int id[LOOKBACK];
  int m = 0;
  for (int j = found; j >= 0 && m < LOOKBACK; --j) {
    dist[m] = norm3(nodes4[4 * j] - p[0], nodes4[4 * j + 1] - p[1], nodes4[4 * j + 2] - p[2]);
    id[m++] = j;
  }
  for (int j = found + 1; j < n && m < LOOKBACK; ++j) {
    dist[m] = norm3(nodes4[4 * j] - p[0], nodes4[4 * j + 1] - p[1], nodes4[4 * j + 2] - p[2]);
    id[m++] = j;
  }
  for (int a = 1; a < m; ++a) {  // insertion sort: stable
    const float d = dist[a];
    const int i = id[a];
    int b = a - 1;
    while (b >= 0 && dist[b] > d) {
      dist[b + 1] = dist[b];
      id[b + 1] = id[b];
      --b;
    }
    dist[b + 1] = d;
    id[b + 1] = i;
  }
  const double dMax = (double)dist[K];
  double sum = 0.0;
  for (int j = 0; j < K; ++j) {
    const double x = 1.0 - (double)dist[j] / dMax;
    w[j] = x * x;
    ids[j] = id[j];
    sum += w[j];
  }
  for (int j = 0; j < K; ++j) w[j] /= sum;
  for (int a = 1; a < K; ++a) {  // by node id (VertexWeightMap::sort); ids are distinct
    const int i = ids[a];
    const double x = w[a];
    int b = a - 1;
    while (b >= 0 && ids[b] > i) {
      ids[b + 1] = ids[b];
      w[b + 1] = w[b];
      --b;
    }
    ids[b + 1] = i;
    w[b + 1] = x;
  }
}

// R (v - g) + g + t of one node (the bracket of :1006-1007 and :884-885)
DMS_DR_HD void node_map(const float* R, const float* g, const float* t, const float* v, float out[3]) {
  const float dx = v[0] - g[0], dy = v[1] - g[1], dz = v[2] - g[2];
  for (int r = 0; r < 3; ++r) out[r] = (((R[r] * dx + R[3 + r] * dy) + R[6 + r] * dz) + g[r]) + t[r];
}

// computeVertexPosition (:992-1009).  nodes4 / rot9 / trans3: the graph; ids, w: weigh_vertex's.
DMS_DR_HD void vertex_position(const float* nodes4, const float* rot9, const float* trans3, const float* src, const int ids[K],
                               const double w[K], float pos[3]) {
  pos[0] = pos[1] = pos[2] = 0.f;
  for (int i = 0; i < K; ++i) {
    const int a = ids[i];
    float m[3];
    node_map(rot9 + 9 * a, nodes4 + 4 * a, trans3 + 3 * a, src, m);
    const float wf = (float)w[i];
    for (int r = 0; r < 3; ++r) pos[r] = pos[r] + wf * m[r];
  }
}

// ---- rotation rows of one enabled node (:849-876, :544-595) -----------------------------------------------------------------------
DMS_DR_HD void rot_residual(const float* R, double r[ROT_ROWS]) {
  const float* c0 = R;
  const float* c1 = R + 3;
  const float* c2 = R + 6;
  r[0] = (double)((c0[0] * c1[0] + c0[1] * c1[1]) + c0[2] * c1[2]);
  r[1] = (double)((c0[0] * c2[0] + c0[1] * c2[1]) + c0[2] * c2[2]);
  r[2] = (double)((c1[0] * c2[0] + c1[1] * c2[1]) + c1[2] * c2[2]);
  r[3] = (double)((c0[0] * c0[0] + c0[1] * c0[1]) + c0[2] * c0[2]) - 1.0;
  r[4] = (double)((c1[0] * c1[0] + c1[1] * c1[1]) + c1[2] * c1[2]) - 1.0;
  r[5] = (double)((c2[0] * c2[0] + c2[1] * c2[1]) + c2[2] * c2[2]) - 1.0;
}
// Row `row` (0..5): its entries in column order, columns relative to the node's first unknown.  Returns the count (6 or 3).
DMS_DR_HD int rot_jacobian(const float* R, int row, int col[6], double val[6]) {
  if (row < 3) {
    // rows 0, 1, 2 pair the columns (0,1), (0,2), (1,2) of R: d(ca . cb) = cb at ca's unknowns, ca at cb's
    const int ca = row == 2 ? 1 : 0, cb = row == 0 ? 1 : 2;
    for (int i = 0; i < 3; ++i) {
      col[i] = 3 * ca + i;
      val[i] = (double)R[3 * cb + i];
      col[3 + i] = 3 * cb + i;
      val[3 + i] = (double)R[3 * ca + i];
    }
    return 6;
  }
  const int c = row - 3;
  for (int i = 0; i < 3; ++i) {
    col[i] = 3 * c + i;
    val[i] = (double)(2 * R[3 * c + i]);
  }
  return 3;
}

// ---- regularisation rows of one edge (j -> its neighbour n) (:878-890, :597-651) -------------------------------------------------
DMS_DR_HD void reg_residual(const float* Rj, const float* gj, const float* tj, const float* gn, const float* tn, double r[REG_ROWS]) {
  float m[3];
  node_map(Rj, gj, tj, gn, m);
  for (int c = 0; c < 3; ++c) r[c] = (double)(m[c] - (gn[c] + tn[c])) * SQRT_WREG;
}
// Row c of the edge has c4[0], c4[1], c4[2] at node j's unknowns c, c + 3, c + 6 and c4[3] at 9 + c; -c4[3] at node n's 9 + c.
DMS_DR_HD void reg_coeffs(const float* gj, const float* gn, double c4[4]) {
  for (int c = 0; c < 3; ++c) c4[c] = (double)(gn[c] - gj[c]) * SQRT_WREG;
  c4[3] = 1.0 * SQRT_WREG;
}

// ---- constraint rows of one vertex against an absolute target (:921-943, :805-830) -----------------------------------------------
DMS_DR_HD void con_residual(const float* pos, const float* target, double r[CON_ROWS]) {
  for (int c = 0; c < 3; ++c) r[c] = (double)(pos[c] - target[c]) * SQRT_WCON;
}
// Row c has c4[0], c4[1], c4[2] at the node's unknowns c, c + 3, c + 6 and c4[3] at 9 + c, for each enabled node of the vertex.
DMS_DR_HD void con_coeffs(const float* src, const float* g, double w, double c4[4]) {
  const float wf = (float)w;
  for (int c = 0; c < 3; ++c) c4[c] = (double)((src[c] - g[c]) * wf) * SQRT_WCON;
  c4[3] = w * SQRT_WCON;
}

// The value a row of component c (0..2) of a regularisation or constraint row has at unknown p (0..11) of a node whose
// coefficients are c4: non-zero only where p % 3 == c.
// (selects, not an indexed load: the four values stay in registers)
DMS_DR_HD double coeff_at(const double c4[4], int p) { return p < 3 ? c4[0] : p < 6 ? c4[1] : p < 9 ? c4[2] : c4[3]; }

}  // namespace dr
}  // namespace dms
