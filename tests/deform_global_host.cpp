// Host build of what densemonoslam_amd/csrc/deform_rows.hpp has for the global deformation object (tests/test_deform_global_cpu.py, g++):
// merged relative rows, residual and Jacobian in the reference's row order, the row envelope, pose weights and applyGraphToPoses,
// to be compared with tests/deform_global_ref.py bit for bit.
#include "deform_rows.hpp"

using namespace dms::dr;

extern "C" {

// kind per pool vertex: 0 absolute, 1 the source of a relative constraint (its target is the next vertex), 2 such a target.
// Residual, CSR Jacobian and first[] (per enabled node, counted from first_enabled); returns the number of rows.
int drg_rows(const float* nodes4, const float* rot9, const float* trans3, int n, int first_enabled, const float* src3, const float* target3,
             const int* kind, const int* ids, const double* w, int count, double* resid, int* indptr, int* cols, double* vals, int* first) {
  int rows = 0, nz = 0;
  const int back = first_enabled * NVAR;
  indptr[0] = 0;
  for (int j = first_enabled; j < n; ++j) {
    first[j - first_enabled] = reg_first(j, n, first_enabled) - first_enabled;
    rot_residual(rot9 + 9 * j, resid + rows);
    for (int r = 0; r < ROT_ROWS; ++r) {
      int c[6];
      double v[6];
      const int m = rot_jacobian(rot9 + 9 * j, r, c, v);
      for (int i = 0; i < m; ++i) {
        cols[nz] = j * NVAR + c[i] - back;
        vals[nz++] = v[i];
      }
      indptr[++rows] = nz;
    }
  }
  for (int j = 0; j < n; ++j)
    for (int s = 0; s < K; ++s) {
      const int nb = neighbour(j, n, s);
      if (nb < first_enabled && j < first_enabled) continue;
      reg_residual(rot9 + 9 * j, nodes4 + 4 * j, trans3 + 3 * j, nodes4 + 4 * nb, trans3 + 3 * nb, resid + rows);
      double c4[4];
      reg_coeffs(nodes4 + 4 * j, nodes4 + 4 * nb, c4);
      for (int c = 0; c < 3; ++c) {
        if (nb < j && nb >= first_enabled) {
          cols[nz] = nb * NVAR + 9 + c - back;
          vals[nz++] = -c4[3];
        }
        if (j >= first_enabled)
          for (int q = 0; q < 4; ++q) {
            cols[nz] = j * NVAR + 3 * q + c - back;
            vals[nz++] = c4[q];
          }
        if (nb > j && nb >= first_enabled) {
          cols[nz] = nb * NVAR + 9 + c - back;
          vals[nz++] = -c4[3];
        }
        indptr[++rows] = nz;
      }
    }
  for (int l = 0; l < count; ++l) {
    if (kind[l] == 2) continue;
    int mid[2 * K], m = K;
    double mc[8 * K];
    if (kind[l] == 1) {
      m = rel_merge(nodes4, src3 + 3 * l, ids + K * l, w + K * l, src3 + 3 * (l + 1), ids + K * (l + 1), w + K * (l + 1), mid, mc);
    } else {
      for (int i = 0; i < K; ++i) {
        mid[i] = ids[K * l + i];
        con_coeffs(src3 + 3 * l, nodes4 + 4 * mid[i], w[K * l + i], mc + 4 * i);
      }
    }
    if (mid[m - 1] < first_enabled) continue;  // ids ascend: no enabled node on either side
    for (int j = first_enabled; j < n; ++j) {
      const int f = con_first(mid, m, j, first_enabled) - first_enabled;
      if (f < first[j - first_enabled]) first[j - first_enabled] = f;
    }
    float pos[3], tp[3];
    vertex_position(nodes4, rot9, trans3, src3 + 3 * l, ids + K * l, w + K * l, pos);
    if (kind[l] == 1)
      vertex_position(nodes4, rot9, trans3, src3 + 3 * (l + 1), ids + K * (l + 1), w + K * (l + 1), tp);
    con_residual(pos, kind[l] == 1 ? tp : target3 + 3 * l, resid + rows);
    for (int c = 0; c < 3; ++c) {
      for (int i = 0; i < m; ++i) {
        if (mid[i] < first_enabled) continue;
        for (int q = 0; q < 4; ++q) {
          cols[nz] = mid[i] * NVAR + 3 * q + c - back;
          vals[nz++] = mc[4 * i + q];
        }
      }
      indptr[++rows] = nz;
    }
  }
  return rows;
}

// setPosesSeq's weights and applyGraphToPoses in place; returns the number of rotations kept
int drg_poses(const float* nodes4, const float* rot9, const float* trans3, int n, const long long* times, float* poses16, int count, int* ids,
              double* w) {
  int kept = 0;
  for (int v = 0; v < count; ++v) {
    float* T = poses16 + 16 * v;
    const float p[3] = {T[3], T[7], T[11]};
    weigh_vertex(nodes4, n, p, times[v], ids + K * v, w + K * v);
    kept += pose_apply(nodes4, rot9, trans3, ids + K * v, w + K * v, T) ? 0 : 1;
  }
  return kept;
}

int drg_polar(const float* M9, float* out9) { return polar_factor(M9, out9) ? 1 : 0; }
}
