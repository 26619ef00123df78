// Host build of densemonoslam_amd/csrc/deform_rows.hpp for tests/test_deform_cpu.py (compiled there with g++): the header's
// functions laid out in the reference's row order, so that node ids, weights, every residual entry and every Jacobian value and
// column can be compared with tests/deform_ref.py bit for bit.
#include "deform_rows.hpp"

using namespace dms::dr;

extern "C" {

void dr_neighbours(int n, int* out) {
  for (int j = 0; j < n; ++j)
    for (int s = 0; s < K; ++s) out[K * j + s] = neighbour(j, n, s);
}

void dr_weigh(const float* nodes4, int n, const float* pts3, const long long* times, int count, int* ids, double* w) {
  for (int v = 0; v < count; ++v) weigh_vertex(nodes4, n, pts3 + 3 * v, times[v], ids + K * v, w + K * v);
}

void dr_positions(const float* nodes4, const float* rot9, const float* trans3, const float* src3, const int* ids, const double* w, int count,
                  float* out3) {
  for (int v = 0; v < count; ++v) vertex_position(nodes4, rot9, trans3, src3 + 3 * v, ids + K * v, w + K * v, out3 + 3 * v);
}

// residual and CSR Jacobian with the nodes from first_enabled on enabled; returns the number of rows
int dr_rows(const float* nodes4, const float* rot9, const float* trans3, int n, int first_enabled, const float* src3, const float* target3,
            const int* ids, const double* w, int count, double* resid, int* indptr, int* cols, double* vals) {
  int rows = 0, nz = 0;
  const int back = first_enabled * NVAR;
  indptr[0] = 0;
  for (int j = first_enabled; j < n; ++j) {
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
    const int* id = ids + K * l;
    if (id[K - 1] < first_enabled) continue;  // ids ascend: no enabled node
    float pos[3];
    vertex_position(nodes4, rot9, trans3, src3 + 3 * l, id, w + K * l, pos);
    con_residual(pos, target3 + 3 * l, resid + rows);
    for (int c = 0; c < 3; ++c) {
      for (int i = 0; i < K; ++i) {
        if (id[i] < first_enabled) continue;
        double c4[4];
        con_coeffs(src3 + 3 * l, nodes4 + 4 * id[i], w[K * l + i], c4);
        for (int q = 0; q < 4; ++q) {
          cols[nz] = id[i] * NVAR + 3 * q + c - back;
          vals[nz++] = c4[q];
        }
      }
      indptr[++rows] = nz;
    }
  }
  return rows;
}

double dr_sqrt_wreg(void) { return SQRT_WREG; }
}
