// The deformation-graph solver of include/dmslam_deform.h: Deformation::constrain with DeformationGraph::optimiseGraphSparse for
// absolute and pin constraints (fernMatch = false) on the GPU.  Row and weight arithmetic: deform_rows.hpp (shared with the host
// build the CPU tests compare against tests/deform_ref.py).  Behind it, the second kind of object (dms_deform_create_global): relative
// constraints, fernMatch = true and the poses, over a row-envelope block Cholesky; its launches are listed where its kernels begin.
//
// One solve is a fixed sequence of launches on the caller's stream; the host reads nothing in between.  A status block in device
// memory carries the loop state: once an exit test of DeformationGraph.cpp:515 fires (or the system is singular) it sets `done`
// and the kernels of the remaining iterations return at once.
//
//   weights    one vertex per lane: node search, 20 distances, stable sort, four weights, the constraint-row coefficients
//   setup      one block: the enabled suffix, row and non-zero offsets of every edge and constraint (exclusive scan)
//   residual   one lane per rotation block / edge / constraint, in the reference's row order; the constraint distances
//   norms      one block: squared residual norm, delta.norm() (256 strided partial sums + pairwise fold: the order the restatement
//              fixes), meanConsErr (a sequential float sum, as the reference's), the exit tests
//   jacobian   the first iteration's Jacobian as CSR (for the staged tests; the assembly below never reads it)
//   assemble   one block per enabled node = block row of A = J^T J in block-band storage (12 x 12 blocks, the diagonal block and the
//              19 to its left).  The rows of regularisation and constraints never change over the iterations (their entries hold
//              positions and weights only), so that part is built once; per iteration the rotation rows' 9 x 9 is added and
//              g = -J^T r formed.  Every entry is one thread's sum in a fixed order: no atomics.
//   solve      ONE workgroup of 1024 threads: right-looking banded block Cholesky in place (diagonal block and forward substitution
//              in one wave by lane shuffles, panel of up to 19 blocks one row per thread, trailing update of up to 190 blocks from
//              the panel held in LDS), then the backward substitution.  The problem is at most 2048 block columns (2047 in the frame step) and strictly
//              sequential in them; what counts is the latency of a column step, not throughput, so it stays on one CU with block
//              barriers rather than paying grid barriers.
//   apply      applyDeltaSparse (float += double), then residual and norms again
//   finalize   graph reset if singular, node table, newRelativeCons rows, lastDeformTime
#include "../../include/dmslam_deform.h"
#include "deform_rows.hpp"
#include "host_util.hpp"
#include "internal.hpp"
#include "surfel.hpp"

namespace dms {
namespace {
using namespace dr;

constexpr int BW = HALF_BAND_BLOCKS;   // 19
constexpr int NBLK = BW + 1;           // blocks stored per block row: columns i-19 .. i
constexpr int ROWLEN = NBLK * NVAR;    // 240 doubles per scalar row
constexpr int BLK = NVAR * NVAR;       // 144
constexpr int NPAIR = BW * (BW + 1) / 2;
constexpr int GLOBAL_MAX_POOL = 2 * DMS_DEFORM_MAX_CONSTRAINTS + 2 * DMS_DEFORM_MAX_RELATIVE;  // 8192 pool vertices
constexpr int GROUPS = 21;             // 21 * 12 = 252 lanes of a 256-block share the constraint sum of g

struct Hdr {
  int n_nodes, initialised;
  int e0, E;  // first enabled node, number of enabled nodes
  int n_rows, nnz;
  int done, status, iterations, exit_reason, applied, optimised;
  int n_rel, n_pool;
  float error, error0, mce_before, mce_after;
  double last_error;
  double iter_err[3], iter_dn[3];
  long long last_deform;
  int n_poses, pose_kept, pool_applied;  // objects of dms_deform_create_global
};

struct Dev {
  Hdr* h;
  float *nodes4, *rot, *trans, *table, *raw4;
  float *src, *tgt, *ttime;
  int *vtime, *rel_idx;
  int* ids;
  double *w, *coef;
  float *pos, *cnorm;
  int *edge_row, *edge_nz, *con_row, *con_nz;
  double *resid, *resid0;
  int *indptr, *jcols;
  double* jvals;
  double *Ac, *Ab, *g, *diag0, *delta, *delta0;
  float* rel;
  int capN, capP;
  // objects of dms_deform_create_global only: per pool vertex its kind (0 an absolute constraint or pin, 1 the source of a relative
  // constraint whose target is the next vertex, 2 such a target) and the merged row (rel_merge; the four nodes of an absolute one);
  // the row envelope; L in the dense lower block triangle; the pool and the poses of the last applied solve
  int *kind, *mcnt, *mid, *first;
  double *mc, *Lg;
  float *pool_out, *pose16, *relstage;
  long long* ptime;
  int* pids;
  double* pw;
};

__device__ __forceinline__ void identity_node(const Dev& d, int i) {
  for (int q = 0; q < 9; ++q) d.rot[9 * i + q] = (q % 4 == 0) ? 1.f : 0.f;
  for (int q = 0; q < 3; ++q) d.trans[3 * i + q] = 0.f;
}

__global__ __launch_bounds__(256) void k_set_nodes(Dev d, const float* __restrict__ rows4, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    d.h->n_nodes = n;
    d.h->initialised = 1;
  }
  if (i >= n) return;
  for (int q = 0; q < 4; ++q) d.nodes4[4 * i + q] = rows4[4 * i + q];
  identity_node(d, i);
}

// Deformation::sampleGraphModel (Deformation.cpp:250-348): every rate-th surfel, at most capN (the buffer's end), then the stable rank
// sort by init time of fusion_map.hip's k_graph_rank; the graph is replaced only when more than K samples came (:311)
__device__ __forceinline__ int sample_count(unsigned M, int rate, int cap) {
  const unsigned n = (M + (unsigned)rate - 1u) / (unsigned)rate;
  return n < (unsigned)cap ? (int)n : cap;
}
__global__ __launch_bounds__(256) void k_sample(SurfelPlanes src, const unsigned* __restrict__ d_count, int rate, Dev d) {
  const int n = sample_count(d_count[0], rate, d.capN);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t id = (size_t)i * (size_t)rate;
  const float4 p = src.pos[id];
  d.raw4[4 * i] = p.x;
  d.raw4[4 * i + 1] = p.y;
  d.raw4[4 * i + 2] = p.z;
  d.raw4[4 * i + 3] = src.col[id].z;
}
__global__ __launch_bounds__(256) void k_rank(const unsigned* __restrict__ d_count, int rate, Dev d) {
  const int n = sample_count(d_count[0], rate, d.capN);
  if (n <= K) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    d.h->n_nodes = n;
    d.h->initialised = 1;
  }
  if (i >= n) return;
  const float ti = d.raw4[4 * i + 3];
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const float tj = d.raw4[4 * j + 3];
    rank += (tj < ti || (tj == ti && j < i)) ? 1 : 0;
  }
  for (int q = 0; q < 4; ++q) d.nodes4[4 * rank + q] = d.raw4[4 * i + q];
  identity_node(d, rank);
}

// Deformation::addConstraint (Deformation.cpp:76-89): the pool vertex of each row's source and, with pin, of its pin behind it
__global__ __launch_bounds__(256) void k_add(Dev d, const float* __restrict__ rows, int stride, int n, int base_v, int base_rel, int srcTime, int pin) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const float* r = rows + (size_t)stride * c;
  const int v = base_v + (pin ? 2 * c : c);
  for (int q = 0; q < 3; ++q) {
    d.src[3 * v + q] = r[q];
    d.tgt[3 * v + q] = r[3 + q];
  }
  d.vtime[v] = srcTime;
  d.ttime[v] = r[6];
  d.rel_idx[v] = base_rel + c;
  if (pin) {
    for (int q = 0; q < 3; ++q) {
      d.src[3 * (v + 1) + q] = r[3 + q];
      d.tgt[3 * (v + 1) + q] = r[3 + q];
    }
    d.vtime[v + 1] = (int)r[6];
    d.ttime[v + 1] = r[6];
    d.rel_idx[v + 1] = -1;
  }
}

__global__ __launch_bounds__(64) void k_weights(Dev d, int P) {
  const Hdr* h = d.h;
  if (!h->initialised) return;
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= P) return;
  int ids[K];
  double w[K];
  weigh_vertex(d.nodes4, h->n_nodes, d.src + 3 * v, (long long)d.vtime[v], ids, w);
  for (int i = 0; i < K; ++i) {
    d.ids[K * v + i] = ids[i];
    d.w[K * v + i] = w[i];
    con_coeffs(d.src + 3 * v, d.nodes4 + 4 * ids[i], w[i], d.coef + 16 * v + 4 * i);
  }
}

// rows (high word) and non-zeros (low word) of item idx: the 4 N edges in (node, slot) order, then the P constraints
// (G: an object of dms_deform_create_global, whose constraints are the merged rows; a relative constraint's target vertex has none)
template <bool G>
__device__ __forceinline__ unsigned long long item_size(const Dev& d, int idx, int N, int e0) {
  if (idx < 4 * N) {
    const int j = idx / 4, nb = neighbour(j, N, idx % 4);
    if (j < e0 && nb < e0) return 0ull;
    return ((unsigned long long)REG_ROWS << 32) | (unsigned)(REG_ROWS * ((j >= e0 ? 4 : 0) + (nb >= e0 ? 1 : 0)));
  }
  const int l = idx - 4 * N;
  const int* id = G ? d.mid + 2 * K * l : d.ids + K * l;
  const int m = G ? d.mcnt[l] : K;
  int cnt = 0;
  for (int i = 0; i < m; ++i) cnt += id[i] >= e0 ? 1 : 0;
  return cnt ? (((unsigned long long)CON_ROWS << 32) | (unsigned)(CON_ROWS * 4 * cnt)) : 0ull;
}

template <bool G>
__global__ __launch_bounds__(1024) void k_setup(Dev d, int P, int relax) {
  Hdr* h = d.h;
  const int t = threadIdx.x;
  if (!h->initialised) {
    if (t == 0) {
      h->done = 1;
      h->status = DMS_DEFORM_NO_GRAPH;
      h->applied = h->optimised = h->iterations = h->exit_reason = 0;
      h->E = h->e0 = h->n_rows = h->nnz = h->n_rel = 0;
      h->n_pool = P;
      h->error = h->error0 = h->mce_before = h->mce_after = 0.f;
    }
    return;
  }
  __shared__ int s_cnt;
  __shared__ unsigned long long s_scan[1024];
  const int N = h->n_nodes;
  const long long ldt = relax ? 0ll : h->last_deform;
  if (t == 0) s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < N; i += 1024) mine += ((long long)d.nodes4[4 * i + 3] > ldt) ? 0 : 1;  // enabled = time > lastDeformTime (:477)
  if (mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  const int e0 = s_cnt, E = N - e0;  // times ascend: the enabled nodes are the suffix from e0
  const int total = 4 * N + P, per = (total + 1023) / 1024;
  const int lo = min(total, t * per), hi = min(total, lo + per);
  unsigned long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += item_size<G>(d, i, N, e0);
  s_scan[t] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const unsigned long long x = t >= off ? s_scan[t - off] : 0ull;
    __syncthreads();
    s_scan[t] += x;
    __syncthreads();
  }
  unsigned long long at = s_scan[t] - sum + (((unsigned long long)(ROT_ROWS * E) << 32) | (unsigned)(27 * E));
  for (int i = lo; i < hi; ++i) {
    const unsigned long long sz = item_size<G>(d, i, N, e0);
    int* row = i < 4 * N ? d.edge_row + i : d.con_row + (i - 4 * N);
    int* nz = i < 4 * N ? d.edge_nz + i : d.con_nz + (i - 4 * N);
    *row = sz ? (int)(at >> 32) : -1;
    *nz = (int)(at & 0xffffffffu);
    at += sz;
  }
  if (t == 1023) {
    const unsigned long long all = s_scan[1023] + (((unsigned long long)(ROT_ROWS * E) << 32) | (unsigned)(27 * E));
    h->n_rows = (int)(all >> 32);
    h->nnz = (int)(all & 0xffffffffu);
  }
  if (t == 0) {
    h->e0 = e0;
    h->E = E;
    h->done = E == 0 ? 1 : 0;
    h->status = DMS_DEFORM_OK;
    h->iterations = 0;
    h->exit_reason = E == 0 ? DMS_DEFORM_EXIT_NO_ENABLED_NODE : DMS_DEFORM_EXIT_ITERATIONS;
    h->optimised = 1;
    h->applied = 0;
    h->n_rel = 0;
    h->n_pool = P;
    for (int i = 0; i < 3; ++i) h->iter_err[i] = h->iter_dn[i] = 0.0;
    if (G) h->pose_kept = 0;
  }
}

// sparseResidual (:842-949): thread idx < capN: the rotation rows of enabled node idx; then 4 capN edges; then P constraints
template <bool G>
__global__ __launch_bounds__(256) void k_residual(Dev d, int P, int respect_done) {
  const Hdr* h = d.h;
  if (!h->initialised || (respect_done == 1 && h->done)) return;
  if (respect_done == 2 && h->status != DMS_DEFORM_SINGULAR) return;  // after the reset of a singular exit: positions and distances anew
  const int N = h->n_nodes, e0 = h->e0, E = h->E;
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < d.capN) {
    if (idx < E) rot_residual(d.rot + 9 * (e0 + idx), d.resid + ROT_ROWS * idx);
    return;
  }
  idx -= d.capN;
  if (idx < 4 * d.capN) {
    if (idx >= 4 * N || d.edge_row[idx] < 0) return;
    const int j = idx / 4, nb = neighbour(j, N, idx % 4);
    reg_residual(d.rot + 9 * j, d.nodes4 + 4 * j, d.trans + 3 * j, d.nodes4 + 4 * nb, d.trans + 3 * nb, d.resid + d.edge_row[idx]);
    return;
  }
  idx -= 4 * d.capN;
  if (idx >= P) return;
  int ids[K];
  double w[K];
  for (int i = 0; i < K; ++i) {
    ids[i] = d.ids[K * idx + i];
    w[i] = d.w[K * idx + i];
  }
  float pos[3];
  vertex_position(d.nodes4, d.rot, d.trans, d.src + 3 * idx, ids, w, pos);
  const float* tg = d.tgt + 3 * idx;
  for (int q = 0; q < 3; ++q) d.pos[3 * idx + q] = pos[q];
  if (G && d.kind[idx] != 0) {
    // a relative constraint (:923-932) is no term of nonRelativeConstraintError: a zero leaves that float sum's bits as they are
    d.cnorm[idx] = 0.f;
    if (d.kind[idx] == 1 && d.con_row[idx] >= 0) {
      float tp[3];
      for (int i = 0; i < K; ++i) {
        ids[i] = d.ids[K * (idx + 1) + i];
        w[i] = d.w[K * (idx + 1) + i];
      }
      vertex_position(d.nodes4, d.rot, d.trans, d.src + 3 * (idx + 1), ids, w, tp);
      con_residual(pos, tp, d.resid + d.con_row[idx]);
    }
    return;
  }
  d.cnorm[idx] = norm3(pos[0] - tg[0], pos[1] - tg[1], pos[2] - tg[2]);  // nonRelativeConstraintError's term (:1021)
  if (d.con_row[idx] >= 0) con_residual(pos, tg, d.resid + d.con_row[idx]);
}

// sparseJacobian (:537-840) as CSR, same thread layout
template <bool G>
__global__ __launch_bounds__(256) void k_jacobian(Dev d, int P) {
  const Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int N = h->n_nodes, e0 = h->e0, E = h->E;
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx == 0) d.indptr[h->n_rows] = h->nnz;
  if (idx < d.capN) {
    if (idx >= E) return;
    int nz = 27 * idx;
    for (int r = 0; r < ROT_ROWS; ++r) {
      int c[6];
      double v[6];
      const int m = rot_jacobian(d.rot + 9 * (e0 + idx), r, c, v);
      d.indptr[ROT_ROWS * idx + r] = nz;
      for (int i = 0; i < m; ++i) {
        d.jcols[nz] = idx * NVAR + c[i];
        d.jvals[nz++] = v[i];
      }
    }
    return;
  }
  idx -= d.capN;
  if (idx < 4 * d.capN) {
    if (idx >= 4 * N || d.edge_row[idx] < 0) return;
    const int j = idx / 4, nb = neighbour(j, N, idx % 4);
    double c4[4];
    reg_coeffs(d.nodes4 + 4 * j, d.nodes4 + 4 * nb, c4);
    int nz = d.edge_nz[idx];
    for (int c = 0; c < 3; ++c) {
      d.indptr[d.edge_row[idx] + c] = nz;
      if (nb < j && nb >= e0) {
        d.jcols[nz] = (nb - e0) * NVAR + 9 + c;
        d.jvals[nz++] = -c4[3];
      }
      if (j >= e0)
        for (int q = 0; q < 4; ++q) {
          d.jcols[nz] = (j - e0) * NVAR + 3 * q + c;
          d.jvals[nz++] = c4[q];
        }
      if (nb > j && nb >= e0) {
        d.jcols[nz] = (nb - e0) * NVAR + 9 + c;
        d.jvals[nz++] = -c4[3];
      }
    }
    return;
  }
  idx -= 4 * d.capN;
  if (idx >= P || d.con_row[idx] < 0) return;
  int nz = d.con_nz[idx];
  for (int c = 0; c < 3; ++c) {
    d.indptr[d.con_row[idx] + c] = nz;
    const int m = G ? d.mcnt[idx] : K;
    for (int i = 0; i < m; ++i) {
      const int a = G ? d.mid[2 * K * idx + i] : d.ids[K * idx + i];
      if (a < e0) continue;
      const double* c4 = G ? d.mc + 32 * idx + 4 * i : d.coef + 16 * idx + 4 * i;
      for (int q = 0; q < 4; ++q) {
        d.jcols[nz] = (a - e0) * NVAR + 3 * q + c;
        d.jvals[nz++] = c4[q];
      }
    }
  }
}

// The pool vertices that touch node i, compacted in pool order into LDS (256 threads): s_l[c] = the vertex, s_pk[c] = one byte per
// slot of the vertex: 1 + the block column (0..19, 19 = node i itself) of that slot's node in block row i, 0 where the node is
// disabled or outside the band.  Two passes around a scan of per-wave counts, so the order does not depend on timing.  Returns the count.
__device__ __forceinline__ int compact_touching(const Dev& d, int P, int i, int e0, int* s_l, unsigned* s_pk, int* s_w) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, chunks = (P + 255) / 256;  // P <= 4096: at most 16 chunks
  for (int pass = 0; pass < 2; ++pass) {
    for (int c = 0; c < chunks; ++c) {
      const int l = c * 256 + t;
      bool touches = false;
      unsigned pk = 0;
      if (l < P) {
        const int* id = d.ids + K * l;
        for (int k = 0; k < K; ++k) {
          const int a = id[k], col = a - (i - BW);
          touches = touches || a == i;
          if (a >= e0 && col >= 0 && col <= BW) pk |= (unsigned)(col + 1) << (8 * k);
        }
      }
      const unsigned long long m = __ballot(touches);
      if (pass == 0) {
        if (lane == 0) s_w[c * 4 + wave] = __popcll(m);
      } else if (touches) {
        const int pos = s_w[c * 4 + wave] + __popcll(m & ((1ull << lane) - 1ull));
        s_l[pos] = l;
        s_pk[pos] = pk;
      }
    }
    __syncthreads();
    if (pass == 0) {
      if (t == 0) {
        int run = 0;
        for (int k = 0; k < chunks * 4; ++k) {
          const int v = s_w[k];
          s_w[k] = run;
          run += v;
        }
        s_w[64] = run;
      }
      __syncthreads();
    }
  }
  return s_w[64];
}
// the slot whose byte of pk is v, or -1
__device__ __forceinline__ int slot_with(unsigned pk, unsigned v) {
  int s = -1;
  for (int k = 0; k < K; ++k) s = ((pk >> (8 * k)) & 255u) == v ? k : s;
  return s;
}

// ---- what both assemblies (band and row envelope) compute alike ------------------------------------------------------------------------
// What the regularisation rows give entry (p, q) of block (i, jn) of A = J^T J, jn <= i and p % 3 == q % 3
__device__ __forceinline__ double reg_entry(const float* gi, const float* nodes4, int i, int jn, int N, int p, int q) {
  double acc = 0.0;
  if (jn == i) {
    for (int s = 0; s < K; ++s) {  // the edges i -> its neighbours
      double c4[4];
      reg_coeffs(gi, nodes4 + 4 * neighbour(i, N, s), c4);
      acc += coeff_at(c4, p) * coeff_at(c4, q);
    }
    if (p >= 9 && q == p)  // the edges of other nodes (enabled or not) that end in i: -sqrt(wReg) each
      for (int j2 = max(0, i - K); j2 <= min(N - 1, i + K); ++j2)
        for (int s = 0; s < K; ++s)
          if (j2 != i && neighbour(j2, N, s) == i) acc += (-SQRT_WREG) * (-SQRT_WREG);
  } else if (i - jn <= K) {
    const float* gj = nodes4 + 4 * jn;
    for (int s = 0; s < K; ++s) {
      if (q >= 9 && neighbour(i, N, s) == jn) {  // edge i -> jn
        double c4[4];
        reg_coeffs(gi, gj, c4);
        acc += coeff_at(c4, p) * (-c4[3]);
      }
      if (p >= 9 && neighbour(jn, N, s) == i) {  // edge jn -> i
        double c4[4];
        reg_coeffs(gj, gi, c4);
        acc += (-c4[3]) * coeff_at(c4, q);
      }
    }
  }
  return acc;
}

// Thread t < 6 fills row t of the rotation rows' Jacobian of one node (6 x 9, dense)
__device__ __forceinline__ void load_rot_jacobian(double (*s_J)[9], const float* rot_i, int t) {
  if (t >= ROT_ROWS) return;
  int c[6];
  double v[6];
  for (int q = 0; q < 9; ++q) s_J[t][q] = 0.0;
  const int m = rot_jacobian(rot_i, t, c, v);
  for (int k = 0; k < m; ++k) s_J[t][c[k]] = v[k];
}

// -g at unknown p of node i = e0 + b without the constraints: the rotation rows, the node's own edges, the edges that end in it
__device__ __forceinline__ double gradient_reg(const Dev& d, const double (*s_J)[9], int i, int b, int N, int p) {
  double sum = 0.0;
  if (p < 9)
    for (int r = 0; r < ROT_ROWS; ++r) sum += s_J[r][p] * d.resid[ROT_ROWS * b + r];
  for (int s = 0; s < K; ++s) {
    double c4[4];
    reg_coeffs(d.nodes4 + 4 * i, d.nodes4 + 4 * neighbour(i, N, s), c4);
    sum += coeff_at(c4, p) * d.resid[d.edge_row[4 * i + s] + p % 3];
  }
  if (p >= 9)
    for (int j2 = max(0, i - K); j2 <= min(N - 1, i + K); ++j2)
      for (int s = 0; s < K; ++s)
        if (j2 != i && neighbour(j2, N, s) == i) sum += (-SQRT_WREG) * d.resid[d.edge_row[4 * j2 + s] + (p - 9)];
  return sum;
}

// The part of A = J^T J that the regularisation and constraint rows give: block row b (node i = e0 + b), blocks (i, i-19 .. i).
// An entry at unknown p of a node lies in the row of component p % 3, so only entries with p % 3 == q % 3 meet in a row.
__global__ __launch_bounds__(256) void k_assemble_const(Dev d, int P) {
  const Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int b = blockIdx.x;
  if (b >= h->E) return;
  const int N = h->n_nodes, e0 = h->e0, i = e0 + b;
  extern __shared__ int s_dyn[];
  __shared__ int s_w[65];
  int* s_l = s_dyn;
  unsigned* s_pk = (unsigned*)(s_dyn + P);
  const int cnt = compact_touching(d, P, i, e0, s_l, s_pk, s_w);
  double* out = d.Ac + (size_t)b * NVAR * ROWLEN;
  const float* gi = d.nodes4 + 4 * i;
  for (int e = threadIdx.x; e < NVAR * ROWLEN; e += 256) {
    const int p = e / ROWLEN, cc = e % ROWLEN, jb = cc / NVAR, q = cc % NVAR;
    const int jn = i - (BW - jb);
    double acc = 0.0;
    if (jn >= e0 && (p % 3) == (q % 3)) {
      acc = reg_entry(gi, d.nodes4, i, jn, N, p, q);
      for (int c = 0; c < cnt; ++c) {  // the constraints that touch i, in pool order
        const unsigned pk = s_pk[c];
        const int t = slot_with(pk, (unsigned)jb + 1u);
        if (t < 0) continue;
        const double* cf = d.coef + 16 * s_l[c];
        acc += coeff_at(cf + 4 * slot_with(pk, BW + 1u), p) * coeff_at(cf + 4 * t, q);
      }
    }
    out[e] = acc;
  }
}

// Per iteration: A = the constant part + the rotation rows' J^T J on the diagonal block; g = -J^T r
__global__ __launch_bounds__(256) void k_iter_assemble(Dev d, int P) {
  const Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int b = blockIdx.x;
  if (b >= h->E) return;
  const int N = h->n_nodes, e0 = h->e0, i = e0 + b, t = threadIdx.x;
  __shared__ double s_J[ROT_ROWS][9];
  __shared__ double s_part[GROUPS][NVAR];
  extern __shared__ int s_dyn[];
  __shared__ int s_w[65];
  int* s_l = s_dyn;
  unsigned* s_pk = (unsigned*)(s_dyn + P);
  const int cnt = compact_touching(d, P, i, e0, s_l, s_pk, s_w);
  load_rot_jacobian(s_J, d.rot + 9 * i, t);
  __syncthreads();
  const double* in = d.Ac + (size_t)b * NVAR * ROWLEN;
  double* out = d.Ab + (size_t)b * NVAR * ROWLEN;
  for (int e = t; e < NVAR * ROWLEN; e += 256) {
    const int p = e / ROWLEN, cc = e % ROWLEN, jb = cc / NVAR, q = cc % NVAR;
    double v = in[e];
    if (jb == BW && p < 9 && q < 9)
      for (int r = 0; r < ROT_ROWS; ++r) v += s_J[r][p] * s_J[r][q];
    out[e] = v;
    if (jb == BW && p == q) d.diag0[b * NVAR + p] = v;
  }
  if (t < GROUPS * NVAR) {
    const int p = t % NVAR, grp = t / NVAR;
    double acc = 0.0;
    for (int c = grp; c < cnt; c += GROUPS) {
      const int l = s_l[c];
      acc += coeff_at(d.coef + 16 * l + 4 * slot_with(s_pk[c], BW + 1u), p) * d.resid[d.con_row[l] + p % 3];
    }
    s_part[grp][p] = acc;
  }
  __syncthreads();
  if (t < NVAR) {
    const int p = t;
    double sum = gradient_reg(d, s_J, i, b, N, p);
    for (int grp = 0; grp < GROUPS; ++grp) sum += s_part[grp][p];
    d.g[b * NVAR + p] = -sum;
  }
}

__device__ __forceinline__ double shfl_d(double v, int lane) { return __shfl(v, lane); }

// ---- the steps of a block column that both solvers (band and row envelope) take alike -------------------------------------------------
// The first wave on the diagonal block of column k, (p, q) at Dk[p * ld + q]: lane r < 12 holds row r of the block; L L^T = D by
// columns, then L y = g_k.  L goes to Dk and s_L, y to gk and s_y.  diag0k: the block's diagonal as assembled.  True (in every
// lane) when a pivot failed.
__device__ __forceinline__ bool chol_diag_block(double* Dk, int ld, const double* diag0k, double* gk, double (*s_L)[NVAR], double* s_y, int lane) {
  const int r = lane < NVAR ? lane : 0;
  double row[NVAR];
#pragma unroll
  for (int q = 0; q < NVAR; ++q) row[q] = Dk[r * ld + q];
  double self = 1.0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < NVAR; ++c) {
    const double dcc = shfl_d(row[c], c);
    // a pivot at or below 2^-40 of its diagonal entry (NaN included) holds no bit worth dividing by: singular
    if (!(dcc > 0x1p-40 * diag0k[c])) bad = true;
    const double dd = sqrt(dcc);
    const double lc = lane == c ? dd : row[c] / dd;
    row[c] = lc;
    if (lane == c) self = dd;
#pragma unroll
    for (int q = c + 1; q < NVAR; ++q) {
      const double lqc = shfl_d(lc, q);
      row[q] -= lc * lqc;  // used by lanes >= q only
    }
  }
  const double gr = gk[r];
  double acc = 0.0, yv = 0.0;
#pragma unroll
  for (int c = 0; c < NVAR; ++c) {
    const double yc = shfl_d((gr - acc) / self, c);
    if (lane == c) yv = yc;
    acc += row[c] * yc;
  }
  if (lane < NVAR) {
#pragma unroll
    for (int q = 0; q < NVAR; ++q) {
      const double v = q <= lane ? row[q] : 0.0;
      s_L[lane][q] = v;
      Dk[lane * ld + q] = v;
    }
    s_y[lane] = yv;
    gk[lane] = yv;
  }
  return bad;
}

// One scalar row a of the panel: x = a L_kk^-T into x and over a; returns x . y_k, which the caller takes off the row's entry of g
__device__ __forceinline__ double panel_row_solve(double* a, const double (*s_L)[NVAR], const double* s_y, double x[NVAR]) {
  double dot = 0.0;
#pragma unroll
  for (int q = 0; q < NVAR; ++q) {
    double v = a[q];
#pragma unroll
    for (int m = 0; m < q; ++m) v -= x[m] * s_L[q][m];
    x[q] = v / s_L[q][q];
  }
#pragma unroll
  for (int q = 0; q < NVAR; ++q) {
    a[q] = x[q];
    dot += x[q] * s_y[q];
  }
  return dot;
}

// The first wave's L_kk^T x = rhs: lane c < 12 holds column c of L_kk; returns that lane's entry of x.  rhs is gk less the `parts`
// partial sums of s_red, in order (the band's sums over the panel below the block; the envelope's column sweep has taken them off
// g already and passes none).  It is formed here and not by the caller so that the loads of the block stand before the band's chain
// of 64 subtractions and are in flight while it runs.
__device__ __forceinline__ double back_diag_block(const double* Dk, int ld, const double* gk, const double (*s_red)[NVAR], int parts, int lane) {
  const int c0 = lane < NVAR ? lane : 0;
  double col[NVAR];
#pragma unroll
  for (int m = 0; m < NVAR; ++m) col[m] = m >= c0 ? Dk[m * ld + c0] : 0.0;
  const double self = Dk[c0 * ld + c0];
  double rhs = gk[c0];
  for (int part = 0; part < parts; ++part) rhs -= s_red[part][c0];
  double acc = 0.0, xv = 0.0;
#pragma unroll
  for (int c = NVAR - 1; c >= 0; --c) {
    const double xc = shfl_d((rhs - acc) / self, c);
    if (lane == c) xv = xc;
    acc += col[c] * xc;
  }
  return xv;
}

// The exit of a solve whose factorisation met a bad pivot (one thread); k_finalize / k_gfinalize reset the graph on this status
__device__ __forceinline__ void fail_singular(Hdr* h) {
  h->status = DMS_DEFORM_SINGULAR;
  h->optimised = 0;
  h->done = 1;
  h->iterations += 1;
}

// Banded block Cholesky of Ab in place and both substitutions; delta = A^-1 g.  One workgroup.
__global__ __launch_bounds__(1024) void k_solve(Dev d) {
  Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int E = h->E;
  __shared__ double s_P[BW * NVAR][NVAR];
  __shared__ double s_L[NVAR][NVAR];
  __shared__ double s_y[NVAR];
  __shared__ double s_red[64][NVAR];
  __shared__ unsigned char s_pi[NPAIR], s_pj[NPAIR];
  __shared__ int s_bad;
  const int t = threadIdx.x, lane = t & 63;
  if (t < NPAIR) {  // the t-th lower pair (bi >= bj) of the trailing window
    int bi = 0, rem = t;
    while (rem > bi) {
      rem -= bi + 1;
      ++bi;
    }
    s_pi[t] = (unsigned char)bi;
    s_pj[t] = (unsigned char)rem;
  }
  if (t == 0) s_bad = 0;
  __syncthreads();
  double* Ab = d.Ab;
  double* g = d.g;
  for (int k = 0; k < E; ++k) {
    const int nb = min(BW, E - 1 - k);
    double* Dk = Ab + (size_t)k * NVAR * ROWLEN + BW * NVAR;  // the diagonal block: (p, q) at Dk[p * ROWLEN + q]
    if (t < 64) {
      const bool bad = chol_diag_block(Dk, ROWLEN, d.diag0 + k * NVAR, g + k * NVAR, s_L, s_y, lane);
      if (bad && lane == 0) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) break;
    if (t < nb * NVAR) {  // the panel: row (i, p) of L_ik = A_ik L_kk^-T, and g_i -= L_ik y_k
      const int i = k + 1 + t / NVAR, p = t % NVAR;
      double x[NVAR];
      const double dot = panel_row_solve(Ab + ((size_t)i * NVAR + p) * ROWLEN + (BW - (i - k)) * NVAR, s_L, s_y, x);
#pragma unroll
      for (int q = 0; q < NVAR; ++q) s_P[t][q] = x[q];
      g[i * NVAR + p] -= dot;
    }
    __syncthreads();
    const int entries = nb * (nb + 1) / 2 * BLK;
    // A_ij -= L_ik L_jk^T for k < j <= i <= k + nb.  In batches of TU entries per thread, every load of a batch before its first
    // store: a load behind a store into the same array is not moved up by the compiler, and the step would pay one memory round
    // trip per entry instead of one per batch.
    constexpr int TU = 8;
    for (int base = t; base < entries; base += 1024 * TU) {
      double* at[TU];
      double old[TU];
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int idx = base + u * 1024;
        at[u] = nullptr;
        if (idx < entries) {
          const int pr = idx / BLK, wi = idx % BLK, p = wi / NVAR, q = wi % NVAR;
          const int i = k + 1 + s_pi[pr], j = k + 1 + s_pj[pr];
          at[u] = Ab + ((size_t)i * NVAR + p) * ROWLEN + (BW - (i - j)) * NVAR + q;
          old[u] = *at[u];
        }
      }
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int idx = base + u * 1024;
        if (idx < entries) {
          const int pr = idx / BLK, wi = idx % BLK, p = wi / NVAR, q = wi % NVAR;
          const int bi = s_pi[pr], bj = s_pj[pr];
          double acc = 0.0;
#pragma unroll
          for (int m = 0; m < NVAR; ++m) acc += s_P[bi * NVAR + p][m] * s_P[bj * NVAR + q][m];
          *at[u] = old[u] - acc;
        }
      }
    }
    __syncthreads();
  }
  if (s_bad) {
    if (t == 0) fail_singular(h);
    return;
  }
  for (int k = E - 1; k >= 0; --k) {  // L^T x = y
    const int nb = min(BW, E - 1 - k);
    const double* Dk = Ab + (size_t)k * NVAR * ROWLEN + BW * NVAR;
    if (t < 64 * NVAR) {
      const int q = t % NVAR, part = t / NVAR;
      double acc = 0.0;
      for (int ri = part; ri < nb * NVAR; ri += 64) {
        const int i = k + 1 + ri / NVAR, p = ri % NVAR;
        acc += Ab[((size_t)i * NVAR + p) * ROWLEN + (BW - (i - k)) * NVAR + q] * g[i * NVAR + p];
      }
      s_red[part][q] = acc;
    }
    __syncthreads();
    if (t < 64) {
      const double xv = back_diag_block(Dk, ROWLEN, g + k * NVAR, s_red, 64, lane);
      if (lane < NVAR) g[k * NVAR + lane] = xv;
    }
    __syncthreads();
  }
  for (int idx = t; idx < E * NVAR; idx += 1024) d.delta[idx] = g[idx];
}

// applyDeltaSparse (:960-990): float += double
__global__ __launch_bounds__(256) void k_apply(Dev d, int it) {
  const Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= h->E * NVAR) return;
  const int node = h->e0 + idx / NVAR, var = idx % NVAR;
  const double dl = d.delta[idx];
  if (it == 1) d.delta0[idx] = dl;
  float* x = var < 9 ? d.rot + 9 * node + var : d.trans + 3 * node + (var - 9);
  *x = (float)((double)*x + dl);
}

// squaredNorm / norm in the restatement's order, meanConsErr, and the exit tests of :515
// (G: fernMatch = true, with the exits of :465 and :516; ncons: the divisor of :1025, every constraint, relative ones included)
template <bool G>
__global__ __launch_bounds__(256) void k_norms(Dev d, int P, int it, int ncons) {
  Hdr* h = d.h;
  if (!h->initialised || (it > 0 && h->done)) return;
  if (it < 0 && h->status != DMS_DEFORM_SINGULAR) return;  // it = -1: meanConsErr of the reset graph after a singular exit
  __shared__ double s_a[256], s_b[256];
  __shared__ float s_c[G ? GLOBAL_MAX_POOL : 2 * DMS_DEFORM_MAX_CONSTRAINTS];
  const int t = threadIdx.x, rows = h->n_rows, unknowns = h->E * NVAR;
  double a = 0.0, b = 0.0;
  for (int i = t; i < rows; i += 256) {
    const double x = d.resid[i];
    if (it == 0) d.resid0[i] = x;
    a += x * x;
  }
  if (it > 0)
    for (int i = t; i < unknowns; i += 256) {
      const double x = d.delta[i];
      b += x * x;
    }
  s_a[t] = a;
  s_b[t] = b;
  for (int l = t; l < P; l += 256) s_c[l] = d.cnorm[l];
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) {
      s_a[t] += s_a[t + s];
      s_b[t] += s_b[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  float sum = 0.f;
  for (int l = 0; l < P; ++l) sum = sum + s_c[l];
  const float mce = sum / (float)(G ? ncons : P);
  const float error = (float)s_a[0];
  h->mce_after = mce;
  if (it < 0) return;
  h->error = error;
  if (it == 0) {
    h->mce_before = mce;
    h->error0 = error;
    h->last_error = (double)error;
    if (G && mce < 0.06) {  // :465: nothing was computed but meanConsErr
      h->done = 1;
      h->optimised = 0;
      h->exit_reason = DMS_DEFORM_EXIT_CONSTRAINTS_MET;
      h->error = h->error0 = 0.f;
      h->n_rows = h->nnz = 0;
    }
    return;
  }
  const double e = (double)error, dn = sqrt(s_b[0]), diff = e - h->last_error;
  h->iter_err[it - 1] = e;
  h->iter_dn[it - 1] = dn;
  h->iterations = it;
  int why = -1;
  if (e > h->last_error)
    why = DMS_DEFORM_EXIT_ERROR_GREW;
  else if (dn < 1e-2)
    why = DMS_DEFORM_EXIT_SMALL_DELTA;
  else if (e < 1e-3)
    why = DMS_DEFORM_EXIT_SMALL_ERROR;
  else if (fabs(diff) < 1e-5 * e)
    why = DMS_DEFORM_EXIT_SMALL_CHANGE;
  else if (G && it == 1 && error > 10.0f)
    why = DMS_DEFORM_EXIT_ERROR_LARGE;
  else if (it == 3)
    why = DMS_DEFORM_EXIT_ITERATIONS;
  if (why >= 0) {
    h->exit_reason = why;
    h->done = 1;
  } else {
    h->last_error = e;
  }
}

// Deformation.cpp:165-209: the node table, newRelativeCons, lastDeformTime; a singular system resets the graph first
__global__ __launch_bounds__(256) void k_finalize(Dev d, int P, int time, int relax) {
  Hdr* h = d.h;
  if (!h->initialised) return;
  const bool singular = h->status == DMS_DEFORM_SINGULAR;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < h->n_nodes) {
    if (singular) identity_node(d, idx);
    float* row = d.table + 16 * idx;
    for (int q = 0; q < 3; ++q) row[q] = d.nodes4[4 * idx + q];
    for (int q = 0; q < 9; ++q) row[3 + q] = d.rot[9 * idx + q];
    for (int q = 0; q < 3; ++q) row[12 + q] = d.trans[3 * idx + q];
    row[15] = d.nodes4[4 * idx + 3];
  }
  if (idx < P && !singular && d.rel_idx[idx] >= 0) {
    float* row = d.rel + 8 * d.rel_idx[idx];
    for (int q = 0; q < 3; ++q) {
      row[q] = d.pos[3 * idx + q];  // the pool after applyGraphToVertices: the last residual pass computed it from the final graph
      row[3 + q] = d.tgt[3 * idx + q];
    }
    row[6] = (float)d.vtime[idx];
    row[7] = d.ttime[idx];
  }
  if (idx == 0) {
    h->applied = singular ? 0 : 1;
    if (!singular && !relax) h->last_deform = (long long)time;
  }
}

// ==== objects of dms_deform_create_global: relative constraints, fernMatch = true, the poses ===========================================
// The launches of dms_deform_constrain_global: weights (as above), merge, pose weights, setup, residual, norms, jacobian, then per
// iteration
//   gassemble  one block per enabled node: its row envelope first[i] (the smallest block column any row of J couples it to) and its
//              block row of A = J^T J over first[i] .. i, in the dense lower block triangle; g = -J^T r.  One thread per entry, fixed order.
//   gsolve     ONE workgroup of 1024 threads: right-looking block Cholesky over the row envelope.  At block column k the panel is the
//              rows i > k with first[i] <= k (an ordered list, rebuilt per column by ballot); every pair of panel rows is inside the
//              envelope (first[i] <= k < j), so fill never leaves it and a row that does not reach left stays as narrow as it was.
//              With first[i] = i - 19 this is the band solver's arithmetic.  Tall rows make the panel longer; its trailing update is
//              spread over all 16 waves.  Then the backward substitution, pushed column by column along each row's envelope.
// and finalize (the acceptance test of Deformation.cpp:165) and the poses.

// Deformation.cpp:129-140 for a Constraint(..., relative = true): source and target vertex, one behind the other
__global__ __launch_bounds__(256) void k_add_rel(Dev d, const float* __restrict__ rows8, int n, int base_v) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const float* r = rows8 + 8 * (size_t)c;
  const int v = base_v + 2 * c;
  for (int q = 0; q < 3; ++q) {
    d.src[3 * v + q] = r[q];
    d.tgt[3 * v + q] = r[3 + q];
    d.src[3 * (v + 1) + q] = r[3 + q];
    d.tgt[3 * (v + 1) + q] = r[3 + q];
  }
  d.vtime[v] = (int)r[6];
  d.vtime[v + 1] = (int)r[7];
  d.ttime[v] = d.ttime[v + 1] = r[7];
  d.rel_idx[v] = d.rel_idx[v + 1] = -1;
  d.kind[v] = 1;
  d.kind[v + 1] = 2;
}
__global__ __launch_bounds__(256) void k_mark_absolute(Dev d, int base_v, int n) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < n) d.kind[base_v + c] = 0;
}

// Deformation::sampleGraphFrom (Deformation.cpp:222-249): every 5th node of the local graph when count / 5 > 4
__global__ __launch_bounds__(256) void k_sample_from(Dev d, Dev local) {
  if (!local.h->initialised) return;
  const int count = local.h->n_nodes;
  if (count / 5 <= K) return;
  const int n = min((count + 4) / 5, d.capN), i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    d.h->n_nodes = n;
    d.h->initialised = 1;
  }
  if (i >= n) return;
  for (int q = 0; q < 4; ++q) d.nodes4[4 * i + q] = local.nodes4[4 * (5 * i) + q];
  identity_node(d, i);
}

__global__ __launch_bounds__(64) void k_gmerge(Dev d, int P) {
  if (!d.h->initialised) return;
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= P) return;
  const int kd = d.kind[l];
  int* mid = d.mid + 2 * K * l;
  double* mc = d.mc + 32 * l;
  if (kd == 0) {
    for (int i = 0; i < K; ++i) {
      mid[i] = d.ids[K * l + i];
      for (int q = 0; q < 4; ++q) mc[4 * i + q] = d.coef[16 * l + 4 * i + q];
    }
    d.mcnt[l] = K;
  } else if (kd == 1) {
    int m8[2 * K];
    double c32[8 * K];
    const int m = rel_merge(d.nodes4, d.src + 3 * l, d.ids + K * l, d.w + K * l, d.src + 3 * (l + 1), d.ids + K * (l + 1), d.w + K * (l + 1), m8, c32);
    for (int i = 0; i < m; ++i) {
      mid[i] = m8[i];
      for (int q = 0; q < 4; ++q) mc[4 * i + q] = c32[4 * i + q];
    }
    d.mcnt[l] = m;
  } else {
    d.mcnt[l] = 0;
  }
}

// setPosesSeq (:133-250): weightVerticesSeq's rule over a pose's translation and time
__global__ __launch_bounds__(64) void k_gpose_weights(Dev d, int n) {
  if (!d.h->initialised) return;
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n) return;
  const float* T = d.pose16 + 16 * v;
  const float p[3] = {T[3], T[7], T[11]};
  int ids[K];
  double w[K];
  weigh_vertex(d.nodes4, d.h->n_nodes, p, d.ptime[v], ids, w);
  for (int i = 0; i < K; ++i) {
    d.pids[K * v + i] = ids[i];
    d.pw[K * v + i] = w[i];
  }
}

__device__ __forceinline__ size_t tri_row(int b, int p) { return (size_t)b * (b + 1) / 2 * BLK + (size_t)p * (b + 1) * NVAR; }

__device__ __forceinline__ int slot_of(const int* mid, int m, int node) {
  int s = -1;
  for (int k = 0; k < m; ++k) s = mid[k] == node ? k : s;
  return s;
}
// The pool vertices whose merged row has node i, compacted in pool order into s_l (256 threads) as vertex | node i's slot << 16 |
// (a relative constraint) << 20; see compact_touching
__device__ __forceinline__ int compact_rows_with(const Dev& d, int P, int i, int* s_l, int* s_w) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, chunks = (P + 255) / 256;  // P <= 8192: at most 32 chunks
  for (int pass = 0; pass < 2; ++pass) {
    for (int c = 0; c < chunks; ++c) {
      const int l = c * 256 + t;
      const int slot = l < P ? slot_of(d.mid + 2 * K * l, d.mcnt[l], i) : -1;
      const bool touches = slot >= 0;
      const unsigned long long m = __ballot(touches);
      if (pass == 0) {
        if (lane == 0) s_w[c * 4 + wave] = __popcll(m);
      } else if (touches) {
        s_l[s_w[c * 4 + wave] + __popcll(m & ((1ull << lane) - 1ull))] = l | (slot << 16) | (d.kind[l] == 1 ? 1 << 20 : 0);
      }
    }
    __syncthreads();
    if (pass == 0) {
      if (t == 0) {
        int run = 0;
        for (int k = 0; k < chunks * 4; ++k) {
          const int v = s_w[k];
          s_w[k] = run;
          run += v;
        }
        s_w[128] = run;
      }
      __syncthreads();
    }
  }
  return s_w[128];
}

__global__ __launch_bounds__(256) void k_gassemble(Dev d, int P, int n_relative) {
  const Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int b = blockIdx.x;
  if (b >= h->E) return;
  const int N = h->n_nodes, e0 = h->e0, i = e0 + b, t = threadIdx.x;
  extern __shared__ int s_dyn[];
  __shared__ int s_w[129];
  __shared__ int s_first, s_nfar;
  __shared__ unsigned char s_has[DMS_DEFORM_MAX_GLOBAL_NODES];  // block columns that some relative constraint with node i has a node in
  __shared__ double s_J[ROT_ROWS][9];
  int* s_l = s_dyn;        // the rows with node i, in pool order, each with node i's slot
  int* s_far = s_dyn + P;  // the relative ones among them (at most n_relative), in the same order: only they reach beyond the band
  for (int c = t; c < DMS_DEFORM_MAX_GLOBAL_NODES; c += 256) s_has[c] = 0;
  const int cnt = compact_rows_with(d, P, i, s_l, s_w);
  if (t == 0) s_first = reg_first(i, N, e0);
  if (t == 64) {
    int n = 0;
    for (int c = 0; c < cnt; ++c)
      if (s_l[c] >> 20) s_far[n++] = s_l[c];
    s_nfar = n;
  }
  load_rot_jacobian(s_J, d.rot + 9 * i, t);
  __syncthreads();
  for (int c = t; c < cnt; c += 256) {
    const int l = s_l[c] & 0xffff;
    atomicMin(&s_first, con_first(d.mid + 2 * K * l, d.mcnt[l], i, e0));
  }
  for (int c = t; c < s_nfar; c += 256) {
    const int l = s_far[c] & 0xffff;
    for (int k = 0; k < d.mcnt[l]; ++k)
      if (d.mid[2 * K * l + k] >= e0) s_has[d.mid[2 * K * l + k] - e0] = 1;
  }
  __syncthreads();
  const int fb = s_first - e0, len = (b - fb + 1) * NVAR;
  if (t == 0) d.first[b] = fb;
  const float* gi = d.nodes4 + 4 * i;
  for (int e = t; e < NVAR * len; e += 256) {
    const int p = e / len, cc = e % len, jb = fb + cc / NVAR, q = cc % NVAR, jn = e0 + jb;
    double acc = 0.0;
    if ((p % 3) == (q % 3)) {
      acc = reg_entry(gi, d.nodes4, i, jn, N, p, q);
      const bool far = b - jb > BW;  // a block the band solver has not: absolute constraints and pins have nothing there
      const int* lst = far ? s_far : s_l;
      const int nl = far ? (s_has[jb] ? s_nfar : 0) : cnt;
      for (int c = 0; c < nl; ++c) {
        const int l = lst[c] & 0xffff, si = (lst[c] >> 16) & 7, sj = jn == i ? si : slot_of(d.mid + 2 * K * l, d.mcnt[l], jn);
        if (sj < 0) continue;
        acc += coeff_at(d.mc + 32 * l + 4 * si, p) * coeff_at(d.mc + 32 * l + 4 * sj, q);
      }
    }
    if (jb == b && p < 9 && q < 9)
      for (int r = 0; r < ROT_ROWS; ++r) acc += s_J[r][p] * s_J[r][q];
    d.Lg[tri_row(b, p) + (size_t)jb * NVAR + q] = acc;
    if (jb == b && p == q) d.diag0[b * NVAR + p] = acc;
  }
  if (t < NVAR) {
    const int p = t;
    double sum = gradient_reg(d, s_J, i, b, N, p);
    for (int c = 0; c < cnt; ++c) {
      const int l = s_l[c] & 0xffff;
      sum += coeff_at(d.mc + 32 * l + 4 * ((s_l[c] >> 16) & 7), p) * d.resid[d.con_row[l] + p % 3];
    }
    d.g[b * NVAR + p] = -sum;
  }
}

__global__ __launch_bounds__(1024) void k_gsolve(Dev d) {
  Hdr* h = d.h;
  if (!h->initialised || h->done) return;
  const int E = h->E;
  __shared__ double s_L[NVAR][NVAR];
  __shared__ double s_y[NVAR];
  __shared__ int s_f[DMS_DEFORM_MAX_GLOBAL_NODES], s_rows[DMS_DEFORM_MAX_GLOBAL_NODES];
  __shared__ int s_wc[16];
  __shared__ int s_bad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < E) s_f[t] = d.first[t];
  if (t == 0) s_bad = 0;
  __syncthreads();
  double* L = d.Lg;
  double* g = d.g;
  for (int k = 0; k < E; ++k) {
    const int ldk = (k + 1) * NVAR;
    double* Dk = L + tri_row(k, 0) + (size_t)k * NVAR;  // the diagonal block: (p, q) at Dk[p * ldk + q]
    if (t < 64) {
      const bool bad = chol_diag_block(Dk, ldk, d.diag0 + k * NVAR, g + k * NVAR, s_L, s_y, lane);
      if (bad && lane == 0) s_bad = 1;
    }
    // the panel of column k, ascending: rows below k whose envelope reaches it
    const int cand = k + 1 + t;
    const bool in = cand < E && s_f[cand] <= k;
    const unsigned long long bal = __ballot(in);
    if (lane == 0) s_wc[wave] = __popcll(bal);
    __syncthreads();
    if (s_bad) break;
    int before = 0, m = 0;
    for (int w2 = 0; w2 < 16; ++w2) {
      before += w2 < wave ? s_wc[w2] : 0;
      m += s_wc[w2];
    }
    if (in) s_rows[before + __popcll(bal & ((1ull << lane) - 1ull))] = cand;
    __syncthreads();
    for (int r = t; r < m * NVAR; r += 1024) {  // row (i, p) of L_ik = A_ik L_kk^-T, and g_i -= L_ik y_k
      const int i = s_rows[r / NVAR], p = r % NVAR;
      double x[NVAR];
      const double dot = panel_row_solve(L + tri_row(i, p) + (size_t)k * NVAR, s_L, s_y, x);
      g[i * NVAR + p] -= dot;
    }
    __syncthreads();
    // A_ij -= L_ik L_jk^T for the pairs j <= i of the panel.  As in the band solver, a batch's loads stand before its first store.
    const int entries = m * (m + 1) / 2 * BLK;
    constexpr int TU = 4;
    for (int base = t; base < entries; base += 1024 * TU) {
      unsigned oa[TU], oi[TU], oj[TU];  // offsets into L (below 2^24 doubles): the entry, and the two rows' blocks of column k
      double old[TU];
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int idx = base + u * 1024;
        if (idx < entries) {
          const int pr = idx / BLK, wi = idx % BLK, p = wi / NVAR, q = wi % NVAR;
          int bi = (int)((sqrtf(8.f * (float)pr + 1.f) - 1.f) * 0.5f);
          while ((bi + 1) * (bi + 2) / 2 <= pr) ++bi;
          while (bi * (bi + 1) / 2 > pr) --bi;
          const int i = s_rows[bi], j = s_rows[pr - bi * (bi + 1) / 2];
          oi[u] = (unsigned)tri_row(i, p) + (unsigned)(k * NVAR);
          oj[u] = (unsigned)tri_row(j, q) + (unsigned)(k * NVAR);
          oa[u] = (unsigned)tri_row(i, p) + (unsigned)(j * NVAR + q);
          old[u] = L[oa[u]];
        }
      }
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        if (base + u * 1024 < entries) {
          double acc = 0.0;
#pragma unroll
          for (int m2 = 0; m2 < NVAR; ++m2) acc += L[oi[u] + m2] * L[oj[u] + m2];
          L[oa[u]] = old[u] - acc;
        }
      }
    }
    __syncthreads();
  }
  if (s_bad) {
    if (t == 0) fail_singular(h);
    return;
  }
  for (int k = E - 1; k >= 0; --k) {  // L^T x = y: x_k, then y_j -= L_kj^T x_k along row k's envelope
    const int ldk = (k + 1) * NVAR;
    const double* Dk = L + tri_row(k, 0) + (size_t)k * NVAR;
    if (t < 64) {
      const double xv = back_diag_block(Dk, ldk, g + k * NVAR, nullptr, 0, lane);
      if (lane < NVAR) {
        g[k * NVAR + lane] = xv;
        s_y[lane] = xv;
      }
    }
    __syncthreads();
    const int f = s_f[k] * NVAR;
    for (int c = f + t; c < k * NVAR; c += 1024) {
      double acc = 0.0;
#pragma unroll
      for (int p = 0; p < NVAR; ++p) acc += L[tri_row(k, p) + c] * s_y[p];
      g[c] -= acc;
    }
    __syncthreads();
  }
  for (int idx = t; idx < E * NVAR; idx += 1024) d.delta[idx] = g[idx];
}

// Deformation.cpp:165-201 with fernMatch = true: applied only when optimised && meanConsErr < 0.0003 && error < 0.12; then the node
// table and the pool.  Not applied: neither is written.  A singular system resets the graph as above.
__device__ __forceinline__ bool global_accepts(const Hdr* h) {
  return h->status == DMS_DEFORM_OK && h->optimised && h->mce_after < 0.0003 && h->error < 0.12;
}
__global__ __launch_bounds__(256) void k_gfinalize(Dev d, int P) {
  Hdr* h = d.h;
  if (!h->initialised) return;
  const bool singular = h->status == DMS_DEFORM_SINGULAR, apply = global_accepts(h);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < h->n_nodes) {
    if (singular) identity_node(d, idx);
    if (apply) {
      float* row = d.table + 16 * idx;
      for (int q = 0; q < 3; ++q) row[q] = d.nodes4[4 * idx + q];
      for (int q = 0; q < 9; ++q) row[3 + q] = d.rot[9 * idx + q];
      for (int q = 0; q < 3; ++q) row[12 + q] = d.trans[3 * idx + q];
      row[15] = d.nodes4[4 * idx + 3];
    }
  }
  if (apply && idx < P)
    for (int q = 0; q < 3; ++q) d.pool_out[3 * idx + q] = d.pos[3 * idx + q];
  if (idx == 0 && apply) h->pool_applied = P;
}
// applyGraphToPoses (:102-131), one lane per pose; runs behind k_gfinalize and sets `applied` (nothing of the status block that
// global_accepts reads is written here)
__global__ __launch_bounds__(64) void k_gposes(Dev d, int n) {
  Hdr* h = d.h;
  if (!h->initialised) return;
  const bool apply = global_accepts(h);
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v == 0) h->applied = apply ? 1 : 0;
  if (!apply || v >= n) return;
  int ids[K];
  double w[K];
  for (int i = 0; i < K; ++i) {
    ids[i] = d.pids[K * v + i];
    w[i] = d.pw[K * v + i];
  }
  if (!pose_apply(d.nodes4, d.rot, d.trans, ids, w, d.pose16 + 16 * v)) atomicAdd(&h->pose_kept, 1);
}

}  // namespace
}  // namespace dms

using namespace dms;

struct dms_deform {
  Dev dev{};
  char* arena = nullptr;
  int capN = 0, capC = 0;
  int n_upper = 0;         // host-side upper bound of the node count (the count itself lives on the device)
  int n_pool = 0, n_rel = 0, n_cons = 0;
  int last_pool = 0, last_rel = 0;
  size_t max_rows = 0, max_nnz = 0;
  // an object of dms_deform_create_global: relative rows and poses it was made for and holds, and whether it ran the last solve
  bool global = false, last_global = false;
  int capR = 0, capPoses = 0, n_relrows = 0, n_poses = 0;
  hipStream_t last_stream = nullptr, pose_stream = nullptr;  // of the last solve; of the last dms_deform_set_poses
  Hdr* h_hdr = nullptr;  // pinned
  float* h_rel = nullptr;  // pinned, capC rows of 8
};

static void carve(dms_deform* o, Carver& c) {
  Dev& d = o->dev;
  const size_t N = (size_t)o->capN, P = (size_t)2 * o->capC + (size_t)2 * o->capR;
  d.h = c.take<Hdr>(1);
  d.nodes4 = c.take<float>(4 * N);
  d.rot = c.take<float>(9 * N);
  d.trans = c.take<float>(3 * N);
  d.table = c.take<float>(16 * N);
  d.raw4 = c.take<float>(4 * N);
  d.src = c.take<float>(3 * P);
  d.tgt = c.take<float>(3 * P);
  d.ttime = c.take<float>(P);
  d.vtime = c.take<int>(P);
  d.rel_idx = c.take<int>(P);
  d.ids = c.take<int>(4 * P);
  d.w = c.take<double>(4 * P);
  d.coef = c.take<double>(16 * P);
  d.pos = c.take<float>(3 * P);
  d.cnorm = c.take<float>(P);
  d.edge_row = c.take<int>(4 * N);
  d.edge_nz = c.take<int>(4 * N);
  d.con_row = c.take<int>(P);
  d.con_nz = c.take<int>(P);
  d.resid = c.take<double>(o->max_rows);
  d.resid0 = c.take<double>(o->max_rows);
  d.indptr = c.take<int>(o->max_rows + 1);
  d.jcols = c.take<int>(o->max_nnz);
  d.jvals = c.take<double>(o->max_nnz);
  d.Ac = c.take<double>(N * NVAR * ROWLEN);
  d.Ab = c.take<double>(N * NVAR * ROWLEN);
  d.g = c.take<double>(N * NVAR);
  d.diag0 = c.take<double>(N * NVAR);
  d.delta = c.take<double>(N * NVAR);
  d.delta0 = c.take<double>(N * NVAR);
  d.rel = c.take<float>(8 * (size_t)o->capC);
  d.capN = o->capN;
  d.capP = (int)P;
  if (!o->global) return;
  d.kind = c.take<int>(P);
  d.mcnt = c.take<int>(P);
  d.mid = c.take<int>(2 * K * P);
  d.mc = c.take<double>(32 * P);
  d.first = c.take<int>(N);
  d.Lg = c.take<double>(N * (N + 1) / 2 * BLK);
  d.pool_out = c.take<float>(3 * P);
  d.relstage = c.take<float>(8 * (size_t)o->capR);
  d.ptime = c.take<long long>((size_t)o->capPoses);
  d.pose16 = c.take<float>(16 * (size_t)o->capPoses);
  d.pids = c.take<int>(K * (size_t)o->capPoses);
  d.pw = c.take<double>(K * (size_t)o->capPoses);
}

static inline int blocks_of(size_t n, int per) {
  const size_t b = (n + per - 1) / per;
  return (int)(b ? b : 1);
}

static int sync_last(dms_deform* d) {
  DMS_HIP(hipStreamSynchronize(d->last_stream));
  return DMS_OK;
}

extern "C" {
static void fill_result(const dms_deform* d, dms_deform_result* out);
}

namespace dms {
// The frame step's one read after a solve: the status block and the new relative-constraint rows behind one synchronisation.
// *rel8: pinned rows of 8 floats, valid until the next call; res->relative_rows of them count.
int deform_fetch(dms_deform* d, dms_deform_result* res, const float** rel8) {
  DMS_REQUIRE(d && res && rel8, "null argument");
  DMS_HIP(hipMemcpyAsync(d->h_hdr, d->dev.h, sizeof(Hdr), hipMemcpyDeviceToHost, d->last_stream));
  if (d->last_rel > 0)
    DMS_HIP(hipMemcpyAsync(d->h_rel, d->dev.rel, (size_t)d->last_rel * 8 * sizeof(float), hipMemcpyDeviceToHost, d->last_stream));
  DMS_HIP(hipStreamSynchronize(d->last_stream));
  fill_result(d, res);
  *rel8 = d->h_rel;
  return DMS_OK;
}

// the poses of a global object in device memory (16 floats each), corrected by the last applied dms_deform_constrain_global
const float* deform_poses_device(dms_deform* d) { return d->dev.pose16; }

// rows of `stride` floats {source xyz, target xyz, target time, ...}: the frame step's constraint buffer has 8 per row
int deform_add_rows(dms_deform* d, const float* rows_dev, int stride, int n, int srcTime, int pin, hipStream_t s) {
  DMS_REQUIRE(d && rows_dev && n >= 0 && stride >= 7, "bad argument");
  if (d->n_cons + n > d->capC) {
    set_error("%s: %d constraints, made for %d", __func__, d->n_cons + n, d->capC);
    return DMS_ERR_CAPACITY;
  }
  if (n == 0) return DMS_OK;
  hipLaunchKernelGGL(k_add, dim3(blocks_of(n, 256)), dim3(256), 0, s, d->dev, rows_dev, stride, n, d->n_pool, d->n_rel, srcTime, pin ? 1 : 0);
  DMS_CHECK_LAUNCH();
  if (d->global) {
    hipLaunchKernelGGL(k_mark_absolute, dim3(blocks_of(pin ? 2 * n : n, 256)), dim3(256), 0, s, d->dev, d->n_pool, pin ? 2 * n : n);
    DMS_CHECK_LAUNCH();
  }
  d->n_pool += pin ? 2 * n : n;
  d->n_rel += n;
  d->n_cons += n;
  return DMS_OK;
}
}  // namespace dms

extern "C" {

static int create_object(dms_deform** out, int max_nodes, int max_constraints, bool global, int max_relative, int max_poses) {
  dms_deform* o = new dms_deform();
  o->capN = max_nodes;
  o->capC = max_constraints;
  o->global = global;
  o->capR = max_relative;
  o->capPoses = max_poses;
  const size_t N = (size_t)max_nodes, P = (size_t)2 * max_constraints + (size_t)2 * max_relative;
  o->max_rows = (ROT_ROWS + REG_ROWS * K) * N + CON_ROWS * P;  // maxRows of :471
  o->max_nnz = 27 * N + (size_t)REG_ROWS * 5 * K * N + (size_t)CON_ROWS * 4 * K * P;
  Carver sz;
  carve(o, sz);
  const size_t bytes = up256(sz.off);
  hipError_t e = hipMalloc((void**)&o->arena, bytes);
  if (e == hipSuccess) e = hipMemset(o->arena, 0, bytes);
  if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_hdr, sizeof(Hdr));
  if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_rel, (size_t)max_constraints * 8 * sizeof(float));
  if (e != hipSuccess) {
    if (o->arena) (void)hipFree(o->arena);
    if (o->h_hdr) (void)hipHostFree(o->h_hdr);
    delete o;
    return hip_fail(e, "allocating the deformation solver", __FILE__, __LINE__);
  }
  Carver cv;
  cv.base = o->arena;
  carve(o, cv);
  *out = o;
  return DMS_OK;
}

int dms_deform_create(dms_deform** out, int max_nodes, int max_constraints) {
  DMS_REQUIRE(out, "null argument");
  DMS_REQUIRE(max_nodes > K && max_nodes <= DMS_DEFORM_MAX_NODES, "max_nodes outside [5, DMS_DEFORM_MAX_NODES]");
  DMS_REQUIRE(max_constraints >= 1 && max_constraints <= DMS_DEFORM_MAX_CONSTRAINTS, "max_constraints outside [1, DMS_DEFORM_MAX_CONSTRAINTS]");
  return create_object(out, max_nodes, max_constraints, false, 0, 0);
}

int dms_deform_create_global(dms_deform** out, int max_nodes, int max_constraints, int max_relative, int max_poses) {
  DMS_REQUIRE(out, "null argument");
  DMS_REQUIRE(max_nodes > K && max_nodes <= DMS_DEFORM_MAX_GLOBAL_NODES, "max_nodes outside [5, DMS_DEFORM_MAX_GLOBAL_NODES]");
  DMS_REQUIRE(max_constraints >= 1 && max_constraints <= DMS_DEFORM_MAX_CONSTRAINTS, "max_constraints outside [1, DMS_DEFORM_MAX_CONSTRAINTS]");
  DMS_REQUIRE(max_relative >= 0 && max_relative <= DMS_DEFORM_MAX_RELATIVE, "max_relative outside [0, DMS_DEFORM_MAX_RELATIVE]");
  DMS_REQUIRE(max_poses >= 0 && max_poses <= DMS_DEFORM_MAX_POSES, "max_poses outside [0, DMS_DEFORM_MAX_POSES]");
  return create_object(out, max_nodes, max_constraints, true, max_relative, max_poses);
}

int dms_deform_destroy(dms_deform* d) {
  if (!d) return DMS_OK;
  if (d->arena) (void)hipFree(d->arena);
  if (d->h_hdr) (void)hipHostFree(d->h_hdr);
  if (d->h_rel) (void)hipHostFree(d->h_rel);
  delete d;
  return DMS_OK;
}

int dms_deform_set_nodes(dms_deform* d, const float* rows4_dev, int n, dms_stream s) {
  DMS_REQUIRE(d && rows4_dev, "null argument");
  DMS_REQUIRE(n > K, "a graph needs more than 4 nodes");
  if (n > d->capN) {
    set_error("%s: %d nodes, made for %d", __func__, n, d->capN);
    return DMS_ERR_CAPACITY;
  }
  hipLaunchKernelGGL(k_set_nodes, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)s, d->dev, rows4_dev, n);
  DMS_CHECK_LAUNCH();
  d->n_upper = n;
  return DMS_OK;
}

int dms_deform_sample_model(dms_deform* d, dms_model* m, int sampleRate, dms_stream s) {
  DMS_REQUIRE(d && m && sampleRate >= 2, "bad argument");
  if (int rc = model_flush_pending(m, (hipStream_t)s)) return rc;
  size_t n = (m->count_upper + (size_t)sampleRate - 1) / (size_t)sampleRate;
  if (n > (size_t)d->capN) n = d->capN;
  if (n == 0) return DMS_OK;
  hipLaunchKernelGGL(k_sample, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)s, m->buf[m->cur], m->d_count, sampleRate, d->dev);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rank, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)s, m->d_count, sampleRate, d->dev);
  DMS_CHECK_LAUNCH();
  if ((int)n > d->n_upper) d->n_upper = (int)n;
  return DMS_OK;
}

int dms_deform_add_constraints(dms_deform* d, const float* rows7_dev, int n, int srcTime, int pin, int relative, dms_stream s) {
  DMS_REQUIRE(d && rows7_dev && n >= 0, "bad argument");
  DMS_REQUIRE(!relative, "relative rows have 8 floats and go through dms_deform_add_relative_constraints, on an object of dms_deform_create_global");
  return deform_add_rows(d, rows7_dev, 7, n, srcTime, pin, (hipStream_t)s);
}

int dms_deform_clear_constraints(dms_deform* d) {
  DMS_REQUIRE(d, "null argument");
  d->n_pool = d->n_rel = d->n_cons = d->n_relrows = 0;
  return DMS_OK;
}

int dms_deform_constrain(dms_deform* d, int time, int relaxGraph, dms_stream stream) {
  DMS_REQUIRE(d, "null argument");
  if (d->n_pool == 0) {
    set_error("%s: no constraints", __func__);
    return DMS_ERR_STATE;
  }
  if (d->n_relrows) {
    set_error("%s: the pool holds relative constraints: dms_deform_constrain_global solves those", __func__);
    return DMS_ERR_STATE;
  }
  hipStream_t s = (hipStream_t)stream;
  const Dev& dev = d->dev;
  const int P = d->n_pool, relax = relaxGraph ? 1 : 0;
  const size_t slot_lds = ((size_t)P * 8 + 15) / 16 * 16;  // compact_touching's two arrays
  const int items = blocks_of((size_t)5 * d->capN + P, 256), node_blocks = d->n_upper > 0 ? d->n_upper : 1;
  hipLaunchKernelGGL(k_weights, dim3(blocks_of(P, 64)), dim3(64), 0, s, dev, P);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_setup<false>, dim3(1), dim3(1024), 0, s, dev, P, relax);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_residual<false>, dim3(items), dim3(256), 0, s, dev, P, 0);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_norms<false>, dim3(1), dim3(256), 0, s, dev, P, 0, 0);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jacobian<false>, dim3(items), dim3(256), 0, s, dev, P);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_assemble_const, dim3(node_blocks), dim3(256), slot_lds, s, dev, P);
  DMS_CHECK_LAUNCH();
  for (int it = 1; it <= 3; ++it) {
    hipLaunchKernelGGL(k_iter_assemble, dim3(node_blocks), dim3(256), slot_lds, s, dev, P);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_solve, dim3(1), dim3(1024), 0, s, dev);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_apply, dim3(blocks_of((size_t)d->n_upper * NVAR, 256)), dim3(256), 0, s, dev, it);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_residual<false>, dim3(items), dim3(256), 0, s, dev, P, 1);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_norms<false>, dim3(1), dim3(256), 0, s, dev, P, it, 0);
    DMS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_finalize, dim3(blocks_of((size_t)(d->capN > P ? d->capN : P), 256)), dim3(256), 0, s, dev, P, time, relax);
  DMS_CHECK_LAUNCH();
  // a singular exit has reset the graph: the pool and meanConsErr (:530) are those of the reset graph (both return at once otherwise)
  hipLaunchKernelGGL(k_residual<false>, dim3(items), dim3(256), 0, s, dev, P, 2);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_norms<false>, dim3(1), dim3(256), 0, s, dev, P, -1, 0);
  DMS_CHECK_LAUNCH();
  d->last_stream = s;
  d->last_pool = P;
  d->last_rel = d->n_rel;
  d->last_global = false;
  d->n_pool = d->n_rel = d->n_cons = 0;  // constraints.clear(), Deformation.cpp:214
  return DMS_OK;
}

int dms_deform_sample_from(dms_deform* global, dms_deform* local, dms_stream s) {
  DMS_REQUIRE(global && local && global->global && !local->global, "needs a global object and a local one");
  // (the node count lives on the device: the kernel takes the first max_nodes samples, as dms_deform_sample_model does)
  const int n = (local->n_upper + 4) / 5 < global->capN ? (local->n_upper + 4) / 5 : global->capN;
  if (n == 0) return DMS_OK;
  hipLaunchKernelGGL(k_sample_from, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)s, global->dev, local->dev);
  DMS_CHECK_LAUNCH();
  if (n > global->n_upper) global->n_upper = n;
  return DMS_OK;
}

static int add_relative(dms_deform* d, const float* rows8, int n, bool on_host, hipStream_t s, const char* who) {
  DMS_REQUIRE(d && rows8 && n >= 0, "bad argument");
  DMS_REQUIRE(d->global, "relative constraints need an object of dms_deform_create_global");
  if (d->n_relrows + n > d->capR) {
    set_error("%s: %d relative constraints, made for %d", who, d->n_relrows + n, d->capR);
    return DMS_ERR_CAPACITY;
  }
  if (n == 0) return DMS_OK;
  if (on_host) {  // each row has a place of its own in the staging buffer, so earlier calls still in flight keep theirs
    float* stage = d->dev.relstage + 8 * (size_t)d->n_relrows;
    DMS_HIP(hipMemcpyAsync(stage, rows8, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice, s));
    rows8 = stage;
  }
  hipLaunchKernelGGL(k_add_rel, dim3(blocks_of(n, 256)), dim3(256), 0, s, d->dev, rows8, n, d->n_pool);
  DMS_CHECK_LAUNCH();
  d->n_pool += 2 * n;
  d->n_relrows += n;
  return DMS_OK;
}
int dms_deform_add_relative_constraints(dms_deform* d, const float* rows8_dev, int n, dms_stream s) {
  return add_relative(d, rows8_dev, n, false, (hipStream_t)s, __func__);
}
int dms_deform_add_relative_constraints_host(dms_deform* d, const float* rows8_host, int n, dms_stream s) {
  return add_relative(d, rows8_host, n, true, (hipStream_t)s, __func__);
}

int dms_deform_set_poses(dms_deform* d, const long long* times_dev, const float* poses16_dev, int n, dms_stream s) {
  DMS_REQUIRE(d && n >= 0 && (n == 0 || (times_dev && poses16_dev)), "bad argument");
  DMS_REQUIRE(d->global, "poses need an object of dms_deform_create_global");
  if (n > d->capPoses) {
    set_error("%s: %d poses, made for %d", __func__, n, d->capPoses);
    return DMS_ERR_CAPACITY;
  }
  if (n) {
    DMS_HIP(hipMemcpyAsync(d->dev.ptime, times_dev, (size_t)n * sizeof(long long), hipMemcpyDeviceToDevice, (hipStream_t)s));
    DMS_HIP(hipMemcpyAsync(d->dev.pose16, poses16_dev, (size_t)n * 16 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)s));
  }
  d->n_poses = n;
  d->pose_stream = (hipStream_t)s;
  return DMS_OK;
}

int dms_deform_constrain_global(dms_deform* d, int time, dms_stream stream) {
  DMS_REQUIRE(d, "null argument");
  DMS_REQUIRE(d->global, "needs an object of dms_deform_create_global");
  (void)time;  // fernMatch = true: lastDeformTime is neither read (:161) nor advanced (:203)
  if (d->n_pool == 0) {
    set_error("%s: no constraints", __func__);
    return DMS_ERR_STATE;
  }
  hipStream_t s = (hipStream_t)stream;
  const Dev& dev = d->dev;
  const int P = d->n_pool, ncons = P - d->n_relrows, np = d->n_poses;
  const size_t list_lds = ((size_t)(P + d->n_relrows) * 4 + 15) / 16 * 16;
  const int items = blocks_of((size_t)5 * d->capN + P, 256), node_blocks = d->n_upper > 0 ? d->n_upper : 1;
  hipLaunchKernelGGL(k_weights, dim3(blocks_of(P, 64)), dim3(64), 0, s, dev, P);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gmerge, dim3(blocks_of(P, 64)), dim3(64), 0, s, dev, P);
  DMS_CHECK_LAUNCH();
  if (np) {
    hipLaunchKernelGGL(k_gpose_weights, dim3(blocks_of(np, 64)), dim3(64), 0, s, dev, np);
    DMS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_setup<true>, dim3(1), dim3(1024), 0, s, dev, P, 1);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_residual<true>, dim3(items), dim3(256), 0, s, dev, P, 0);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_norms<true>, dim3(1), dim3(256), 0, s, dev, P, 0, ncons);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jacobian<true>, dim3(items), dim3(256), 0, s, dev, P);
  DMS_CHECK_LAUNCH();
  for (int it = 1; it <= 3; ++it) {
    hipLaunchKernelGGL(k_gassemble, dim3(node_blocks), dim3(256), list_lds, s, dev, P, d->n_relrows);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gsolve, dim3(1), dim3(1024), 0, s, dev);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_apply, dim3(blocks_of((size_t)d->n_upper * NVAR, 256)), dim3(256), 0, s, dev, it);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_residual<true>, dim3(items), dim3(256), 0, s, dev, P, 1);
    DMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_norms<true>, dim3(1), dim3(256), 0, s, dev, P, it, ncons);
    DMS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_gfinalize, dim3(blocks_of((size_t)(d->capN > P ? d->capN : P), 256)), dim3(256), 0, s, dev, P);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_residual<true>, dim3(items), dim3(256), 0, s, dev, P, 2);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_norms<true>, dim3(1), dim3(256), 0, s, dev, P, -1, ncons);
  DMS_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gposes, dim3(blocks_of(np ? np : 1, 64)), dim3(64), 0, s, dev, np);
  DMS_CHECK_LAUNCH();
  d->last_stream = s;
  d->last_pool = P;
  d->last_rel = 0;  // no newRelativeCons (:171)
  d->last_global = true;
  d->n_pool = d->n_rel = d->n_cons = d->n_relrows = 0;
  return DMS_OK;
}

static int fetch_hdr(dms_deform* d) {
  DMS_HIP(hipMemcpyAsync(d->h_hdr, d->dev.h, sizeof(Hdr), hipMemcpyDeviceToHost, d->last_stream));
  DMS_HIP(hipStreamSynchronize(d->last_stream));
  return DMS_OK;
}

static void fill_result(const dms_deform* d, dms_deform_result* out) {
  const Hdr& h = *d->h_hdr;
  memset(out, 0, sizeof(*out));
  out->applied = h.applied;
  out->optimised = h.optimised;
  out->status = h.status;
  out->iterations = h.iterations;
  out->exit_reason = h.exit_reason;
  out->nodes = h.n_nodes;
  out->enabled_nodes = h.E;
  out->constraints = h.n_pool;
  out->rows = h.n_rows;
  out->relative_rows = h.applied ? d->last_rel : 0;
  out->error = h.error;
  out->error_initial = h.error0;
  out->mean_cons_err_before = h.mce_before;
  out->mean_cons_err_after = h.mce_after;
  for (int i = 0; i < 3; ++i) {
    out->iter_error[i] = h.iter_err[i];
    out->iter_delta_norm[i] = h.iter_dn[i];
  }
  out->last_deform_time = h.last_deform;
}

int dms_deform_get_result(dms_deform* d, dms_deform_result* out) {
  DMS_REQUIRE(d && out, "null argument");
  if (int rc = fetch_hdr(d)) return rc;
  fill_result(d, out);
  return DMS_OK;
}

int dms_deform_graph_device(dms_deform* d, const float** table16_dev, const int** node_count_dev) {
  DMS_REQUIRE(d && table16_dev && node_count_dev, "null argument");
  *table16_dev = d->dev.table;
  *node_count_dev = &d->dev.h->n_nodes;
  return DMS_OK;
}

static int copy_out(dms_deform* d, void* dst, const void* src_dev, size_t elem, int have, int max_n, int* n) {
  if (n) *n = have;
  const int take = have < max_n ? have : max_n;
  if (take > 0 && dst) DMS_HIP(hipMemcpy(dst, src_dev, (size_t)take * elem, hipMemcpyDeviceToHost));
  return DMS_OK;
}

int dms_deform_get_relative_constraints(dms_deform* d, float* rows8_host, int max_rows, int* n) {
  DMS_REQUIRE(d && n && (rows8_host || max_rows == 0), "bad argument");
  if (int rc = fetch_hdr(d)) return rc;
  return copy_out(d, rows8_host, d->dev.rel, 8 * sizeof(float), d->h_hdr->applied ? d->last_rel : 0, max_rows, n);
}

int dms_deform_last_deform_time(dms_deform* d, long long* t) {
  DMS_REQUIRE(d && t, "null argument");
  if (int rc = fetch_hdr(d)) return rc;
  *t = d->h_hdr->last_deform;
  return DMS_OK;
}

int dms_deform_set_last_deform_time(dms_deform* d, long long t) {
  DMS_REQUIRE(d, "null argument");
  DMS_HIP(hipDeviceSynchronize());  // whatever stream the nodes or a solve were enqueued on
  DMS_HIP(hipMemcpy(&d->dev.h->last_deform, &t, sizeof(t), hipMemcpyHostToDevice));
  return DMS_OK;
}

int dms_deform_get_vertex_weights(dms_deform* d, int* ids4_host, double* weights4_host, int max_vertices, int* n) {
  DMS_REQUIRE(d && n, "null argument");
  if (int rc = sync_last(d)) return rc;
  if (int rc = copy_out(d, ids4_host, d->dev.ids, K * sizeof(int), d->last_pool, max_vertices, n)) return rc;
  return copy_out(d, weights4_host, d->dev.w, K * sizeof(double), d->last_pool, max_vertices, n);
}

int dms_deform_get_first_residual(dms_deform* d, double* r_host, int max_rows, int* n) {
  DMS_REQUIRE(d && n, "null argument");
  if (int rc = fetch_hdr(d)) return rc;
  return copy_out(d, r_host, d->dev.resid0, sizeof(double), d->h_hdr->n_rows, max_rows, n);
}

int dms_deform_get_first_jacobian(dms_deform* d, int* indptr_host, int* cols_host, double* vals_host, int max_rows, int max_nnz, int* n,
                                  int* nnz) {
  DMS_REQUIRE(d && n && nnz, "null argument");
  if (int rc = fetch_hdr(d)) return rc;
  const int rows = d->h_hdr->E ? d->h_hdr->n_rows : 0, nz = d->h_hdr->E ? d->h_hdr->nnz : 0;
  if (int rc = copy_out(d, indptr_host, d->dev.indptr, sizeof(int), rows ? rows + 1 : 0, max_rows + 1, nullptr)) return rc;
  if (int rc = copy_out(d, cols_host, d->dev.jcols, sizeof(int), nz, max_nnz, nullptr)) return rc;
  if (int rc = copy_out(d, vals_host, d->dev.jvals, sizeof(double), nz, max_nnz, nullptr)) return rc;
  *n = rows;
  *nnz = nz;
  return DMS_OK;
}

int dms_deform_get_first_delta(dms_deform* d, double* delta_host, int max_unknowns, int* n) {
  DMS_REQUIRE(d && n, "null argument");
  if (int rc = fetch_hdr(d)) return rc;
  const Hdr& h = *d->h_hdr;
  const bool have = h.iterations >= 1 && !(h.status == DMS_DEFORM_SINGULAR && h.iterations == 1);
  return copy_out(d, delta_host, d->dev.delta0, sizeof(double), have ? h.E * NVAR : 0, max_unknowns, n);
}

int dms_deform_get_pool(dms_deform* d, float* xyz_host, int max_vertices, int* n) {
  DMS_REQUIRE(d && n, "null argument");
  if (d->last_global) {  // of the last APPLIED solve: a solve that is not applied writes no pool
    if (int rc = fetch_hdr(d)) return rc;
    return copy_out(d, xyz_host, d->dev.pool_out, 3 * sizeof(float), d->h_hdr->pool_applied, max_vertices, n);
  }
  if (int rc = sync_last(d)) return rc;
  return copy_out(d, xyz_host, d->dev.pos, 3 * sizeof(float), d->last_pool, max_vertices, n);
}

int dms_deform_get_poses(dms_deform* d, long long* times_host, float* poses16_host, int max_poses, int* n) {
  DMS_REQUIRE(d && n && d->global, "needs an object of dms_deform_create_global");
  if (int rc = sync_last(d)) return rc;
  if (d->pose_stream != d->last_stream) DMS_HIP(hipStreamSynchronize(d->pose_stream));
  if (int rc = copy_out(d, times_host, d->dev.ptime, sizeof(long long), d->n_poses, max_poses, n)) return rc;
  return copy_out(d, poses16_host, d->dev.pose16, 16 * sizeof(float), d->n_poses, max_poses, n);
}

int dms_deform_get_pose_weights(dms_deform* d, int* ids4_host, double* weights4_host, int max_poses, int* n) {
  DMS_REQUIRE(d && n && d->global, "needs an object of dms_deform_create_global");
  if (int rc = sync_last(d)) return rc;
  const int have = d->last_global ? d->n_poses : 0;
  if (int rc = copy_out(d, ids4_host, d->dev.pids, K * sizeof(int), have, max_poses, n)) return rc;
  return copy_out(d, weights4_host, d->dev.pw, K * sizeof(double), have, max_poses, n);
}

int dms_deform_get_kept_rotations(dms_deform* d, int* kept) {
  DMS_REQUIRE(d && kept && d->global, "needs an object of dms_deform_create_global");
  if (int rc = fetch_hdr(d)) return rc;
  *kept = d->last_global ? d->h_hdr->pose_kept : 0;
  return DMS_OK;
}

int dms_deform_get_envelope(dms_deform* d, int* first_host, int max_nodes, int* n) {
  DMS_REQUIRE(d && n && d->global, "needs an object of dms_deform_create_global");
  if (int rc = fetch_hdr(d)) return rc;
  const Hdr& h = *d->h_hdr;
  return copy_out(d, first_host, d->dev.first, sizeof(int), d->last_global && h.iterations >= 1 ? h.E : 0, max_nodes, n);
}

}  // extern "C"
