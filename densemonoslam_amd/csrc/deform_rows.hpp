// Row and weight arithmetic of the deformation graph (the reference's Utils/DeformationGraph.cpp with k = 4), written once for
// the kernels of deform.hip and for a plain host build (tests/deform_rows_host.cpp, tests/deform_global_host.cpp, g++): the neighbour rule, the node search and
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

// ---- relative constraints, the row envelope and the poses (fernMatch = true; tests/deform_global_ref.py restates the same) -------
// FURTHER ORDER RULES
//   * the merged weight map of a relative constraint is the source vertex's four entries followed by the target vertex's four,
//     sorted by node id with the reference's bubble sort (it swaps on "greater" only, so it is stable: of a node that both
//     vertices have, the source's entry comes first);
//   * an entry of the source side is con_coeffs' ((src - g) * (float)w, w), one of the target side ((g - tgt) * (float)w, -w)
//     (:720, :728 against :760, :768), each times sqrt(wCon) in double;
//   * a node that occurs on both sides has ONE entry per column: the source's value val, then OrderedJacobianRow::addTo with the
//     target's unscaled value: ((val / sqrt(wCon)) + value) * sqrt(wCon) in double;
//   * the polar factor U V^T of a pose's rotation is taken in double by POLAR_STEPS Newton steps X <- 0.5 (X + X^-T) from the
//     double copy of the float matrix, X^-T being the cofactor matrix over the determinant: every cofactor a b - c d as written,
//     det = (X00 C00 + X01 C01) + X02 C02, each entry 0.5 * (X + C / det); the result is rounded to float once.
constexpr int POLAR_STEPS = 40;          // from a determinant of 2^-20 the smallest singular value doubles for ~20 steps, then converges
constexpr double POLAR_MIN_DET = 0x1p-20;

// The merged row of a relative constraint (sparseJacobian :692-801) over ALL its nodes, enabled or not: node ids ascending in mid,
// four coefficients per node in mc (the layout of con_coeffs).  A node is enabled or not on both sides alike, so the caller drops the
// entries of disabled nodes afterwards.  Returns the number of distinct nodes (4..8).
DMS_DR_HD int rel_merge(const float* nodes4, const float* src, const int ids_s[K], const double w_s[K], const float* tgt, const int ids_t[K],
                        const double w_t[K], int mid[2 * K], double mc[8 * K]) {
  int id[2 * K];
  double w[2 * K];
  bool rel[2 * K];
  for (int a = 0; a < K; ++a) {
    id[a] = ids_s[a];
    w[a] = w_s[a];
    rel[a] = false;
    id[K + a] = ids_t[a];
    w[K + a] = w_t[a];
    rel[K + a] = true;
  }
  bool done = false;
  int size = 2 * K;
  while (!done) {  // VertexWeightMap::sort
    done = true;
    for (int a = 0; a < size - 1; ++a)
      if (id[a] > id[a + 1]) {
        done = false;
        const int ti = id[a];
        id[a] = id[a + 1];
        id[a + 1] = ti;
        const double tw = w[a];
        w[a] = w[a + 1];
        w[a + 1] = tw;
        const bool tr = rel[a];
        rel[a] = rel[a + 1];
        rel[a + 1] = tr;
      }
    --size;
  }
  int m = 0;
  for (int a = 0; a < 2 * K; ++a) {
    const float* g = nodes4 + 4 * id[a];
    const float wf = (float)w[a];
    double v[4];
    for (int c = 0; c < 3; ++c) v[c] = rel[a] ? (double)((g[c] - tgt[c]) * wf) : (double)((src[c] - g[c]) * wf);
    v[3] = rel[a] ? -w[a] : w[a];
    if (m > 0 && mid[m - 1] == id[a]) {
      for (int q = 0; q < 4; ++q) mc[4 * (m - 1) + q] = ((mc[4 * (m - 1) + q] / SQRT_WCON) + v[q]) * SQRT_WCON;
    } else {
      mid[m] = id[a];
      for (int q = 0; q < 4; ++q) mc[4 * m + q] = v[q] * SQRT_WCON;
      ++m;
    }
  }
  return m;
}

// The smallest enabled node that the regularisation rows couple to enabled node i: its own edges and the edges that end in it
DMS_DR_HD int reg_first(int i, int n, int e0) {
  int f = i;
  for (int s = 0; s < K; ++s) {
    const int nb = neighbour(i, n, s);
    if (nb >= e0 && nb < f) f = nb;
  }
  const int lo = i - K > 0 ? i - K : 0;
  for (int j = lo; j < i; ++j)
    for (int s = 0; s < K; ++s)
      if (j >= e0 && j < f && neighbour(j, n, s) == i) f = j;
  return f;
}
// The smallest enabled node of a constraint's (merged) nodes when it has node i, else i: first[i] of the row envelope is the minimum
// of reg_first and of this over every constraint.  mid ascends.
DMS_DR_HD int con_first(const int* mid, int cnt, int i, int e0) {
  bool has = false;
  int f = i;
  for (int s = 0; s < cnt; ++s) {
    has = has || mid[s] == i;
    if (mid[s] >= e0 && mid[s] < f) f = mid[s];
  }
  return has ? f : i;
}

// X^-T step of the polar iteration (see the order rules); X row-major
DMS_DR_HD double cofactors(const double X[9], double C[9]) {
  C[0] = X[4] * X[8] - X[5] * X[7];
  C[1] = X[5] * X[6] - X[3] * X[8];
  C[2] = X[3] * X[7] - X[4] * X[6];
  C[3] = X[2] * X[7] - X[1] * X[8];
  C[4] = X[0] * X[8] - X[2] * X[6];
  C[5] = X[1] * X[6] - X[0] * X[7];
  C[6] = X[1] * X[5] - X[2] * X[4];
  C[7] = X[2] * X[3] - X[0] * X[5];
  C[8] = X[0] * X[4] - X[1] * X[3];
  return (X[0] * C[0] + X[1] * C[1]) + X[2] * C[2];
}
// The orthogonal polar factor of M (row-major floats) into out; false (out untouched) when M is not finite or |det| < 2^-20
DMS_DR_HD bool polar_factor(const float M[9], float out[9]) {
  double X[9], C[9];
  bool finite = true;
  for (int e = 0; e < 9; ++e) {
    X[e] = (double)M[e];
    finite = finite && (X[e] - X[e] == 0.0);
  }
  const double det0 = cofactors(X, C);
  if (!finite || !(fabs(det0) >= POLAR_MIN_DET)) return false;
  for (int it = 0; it < POLAR_STEPS; ++it) {
    const double det = cofactors(X, C);
    for (int e = 0; e < 9; ++e) X[e] = 0.5 * (X[e] + C[e] / det);
  }
  for (int e = 0; e < 9; ++e) out[e] = (float)X[e];
  return true;
}

// applyGraphToPoses (:102-131) for one pose (row-major 4 x 4, in place) with setPosesSeq's weights of it (weigh_vertex over its
// translation and time).  Returns false when the rotation was kept (polar_factor's rule); the translation is written either way.
DMS_DR_HD bool pose_apply(const float* nodes4, const float* rot9, const float* trans3, const int ids[K], const double w[K], float* pose16) {
  const float t[3] = {pose16[3], pose16[7], pose16[11]};
  float moved[3] = {0.f, 0.f, 0.f};
  float rs[9];  // the weighted rotation sum, column-major as the nodes' rotations
  for (int e = 0; e < 9; ++e) rs[e] = 0.f;
  for (int j = 0; j < K; ++j) {
    const int a = ids[j];
    const float wf = (float)w[j];
    float m[3];
    node_map(rot9 + 9 * a, nodes4 + 4 * a, trans3 + 3 * a, t, m);
    for (int r = 0; r < 3; ++r) moved[r] = moved[r] + wf * m[r];
    for (int e = 0; e < 9; ++e) rs[e] = rs[e] + wf * rot9[9 * a + e];
  }
  float M[9], U[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[3 * r + c] = (rs[r] * pose16[c] + rs[3 + r] * pose16[4 + c]) + rs[6 + r] * pose16[8 + c];
  const bool ok = polar_factor(M, U);
  for (int r = 0; r < 3; ++r) {
    pose16[4 * r + 3] = moved[r];
    if (ok)
      for (int c = 0; c < 3; ++c) pose16[4 * r + c] = U[3 * r + c];
  }
  return ok;
}

}  // namespace dr
}  // namespace dms
