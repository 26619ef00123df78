"""CPU restatement of the reference's deformation-graph optimisation for ABSOLUTE and PIN constraints with fernMatch = false
(Core/src/Utils/DeformationGraph.cpp, Core/src/Deformation.cpp), numpy only.  It is the yardstick of the GPU solver
(densemonoslam_amd/csrc/deform.hip, deform_rows.hpp) and has checks of its own in tests/test_deform_cpu.py.

What is restated, by file and line:
  DeformationGraph::initialiseGraph / connectGraphSeq   DeformationGraph.cpp:56-91, :252-288 (k = 4)       Graph, neighbours
  weightVerticesSeq                                      :290-405                                           find_node, weigh_vertex
  sparseResidual                                         :842-949                                           residual
  sparseJacobian                                         :537-840 (rotation, regularisation, non-relative)  jacobian
  applyDeltaSparse / computeVertexPosition               :960-990, :992-1009                                apply_delta, vertex_position
  nonRelativeConstraintError                             :1011-1026                                         mean_cons_error
  optimiseGraphSparse (fernMatch = false)                :457-535                                           optimise
  Deformation::addConstraint (pin rule)                  Deformation.cpp:76-89                              pool_of
  Deformation::constrain                                 :91-220                                            constrain

Where the reference leaves an order open, one is fixed here and the product follows it:
  * float expressions are evaluated left to right as written, with no fused multiply-add: a matrix row times a vector is
    (R(r,0) x + R(r,1) y) + R(r,2) z and a dot product (a0 b0 + a1 b1) + a2 b2 (Eigen's unrolling is an implementation detail);
  * a norm is sqrtf((dx*dx + dy*dy) + dz*dz);
  * both sorts are stable (std::sort of the 20 distances is not; the bubble sort by node id has distinct keys);
  * pow(x, 2) is x * x in double;
  * a double weight times a float vector: the weight is rounded to float first (Eigen converts the scalar operand);
  * squaredNorm() and norm() of a double vector: 256 partial sums (element i goes to sum i % 256, in ascending i), then a
    pairwise fold 128, 64, ..., 1 (lane_sum);
  * a vertex older than every node makes the reference compare against sampledGraphTimes[-1] (:328): either outcome gives the
    same window (nodes 0.. in ascending order), so node 0 is taken;
  * the linear solve (CHOLMOD in the reference) is a banded Cholesky of J^T J: float64 (solver "A") or np.longdouble ("B").  A pivot
    at or below 2^-40 of its diagonal entry counts as non-positive: status SINGULAR, graph reset, nothing applied.
Out of scope, as in the product: relative constraints, fernMatch = true (with its two early exits, :465 and :516), applyGraphToPoses.
"""
import numpy as np

K = 4
LOOKBACK = 20
NVAR = 12
SQRT_WREG = np.sqrt(np.float64(10.0))   # sqrt(wReg), DeformationGraph.cpp:26
SQRT_WCON = np.sqrt(np.float64(100.0))  # sqrt(wCon), :27
HALF_BAND = (LOOKBACK - 1) * NVAR + NVAR - 1
PIVOT_REL = 2.0 ** -40

EXIT_NAMES = {0: "three iterations", 1: "error grew", 2: "small delta", 3: "small error", 4: "small change", 5: "no enabled node"}
STATUS_OK, STATUS_SINGULAR = 0, 1


def neighbours(n):
    """connectGraphSeq (:252-288)"""
    assert n > K
    out = [[] for _ in range(n)]
    for i in range(K // 2):
        out[i] += [m for m in range(K + 1) if m != i]
    for i in range(K // 2, n - K // 2):
        for m in range(K // 2):
            out[i] += [i - (m + 1), i + (m + 1)]
    for i in range(n - K // 2, n):
        out[i] += [m for m in range(n - (K + 1), n) if m != i]
    return out


class Graph:
    """initialiseGraph (:56-91): positions, times, identity rotations (column-major, Eigen's data()), zero translations"""

    def __init__(self, nodes4, ft=np.float32):
        nodes4 = np.asarray(nodes4, np.float32).reshape(-1, 4)
        self.ft = ft
        self.n = len(nodes4)
        self.pos = nodes4[:, :3].astype(ft)
        self.times = nodes4[:, 3].astype(np.int64)  # graphPoseTimes.push_back(vertices[i](3)), Deformation.cpp:340
        self.ftimes = nodes4[:, 3].copy()
        assert (np.diff(self.times) >= 0).all(), "nodes are sorted by time"
        self.R = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], ft), (self.n, 1))
        self.t = np.zeros((self.n, 3), ft)
        self.nbr = neighbours(self.n)
        self.enabled = np.ones(self.n, bool)

    def reset(self):
        self.R[:] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], self.ft)
        self.t[:] = 0


def norm3(d):
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def find_node(times, vt):
    n = len(times)
    imin, imax = 0, n - 1
    imid = (imin + imax) // 2
    while imax >= imin:
        imid = (imin + imax) // 2
        if times[imid] < vt:
            imin = imid + 1
        elif times[imid] > vt:
            imax = imid - 1
        else:
            break
    imin = min(imin, n - 1)
    if imax < 0:
        return 0
    a, b, c = abs(int(times[imin]) - vt), abs(int(times[imid]) - vt), abs(int(times[imax]) - vt)
    if a <= b and a <= c:
        return imin
    if b <= a and b <= c:
        return imid
    return imax


def weigh_vertex(g, p, vt):
    """weightVerticesSeq (:290-405) for one vertex: (ids[4] ascending, weights[4] float64)"""
    found = find_node(g.times, int(vt))
    ids = list(range(found, max(found - LOOKBACK, -1), -1))
    if len(ids) != LOOKBACK:
        ids += list(range(found + 1, g.n))[: LOOKBACK - len(ids)]
    ids = np.array(ids)
    d = g.pos[ids] - p[None, :]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    order = np.argsort(dist, kind="stable")
    ids, dist = ids[order], dist[order]
    dmax = np.float64(dist[K])
    w = np.zeros(K)
    s = np.float64(0)
    with np.errstate(all="ignore"):
        for j in range(K):
            x = np.float64(1.0) - np.float64(dist[j]) / dmax
            w[j] = x * x
            s = s + w[j]
        w = w / s
    near = ids[:K]
    o = np.argsort(near, kind="stable")
    return near[o].astype(np.int32), w[o]


def node_map(g, a, v):
    """R (v - g) + g + t of node a, floats, left to right"""
    d = v - g.pos[a]
    R = g.R[a]
    return (((R[0:3] * d[0] + R[3:6] * d[1]) + R[6:9] * d[2]) + g.pos[a]) + g.t[a]


def vertex_position(g, src, ids, w):
    """computeVertexPosition (:992-1009)"""
    pos = np.zeros(3, g.ft)
    for i in range(K):
        pos = pos + g.ft(w[i]) * node_map(g, ids[i], src)
    return pos


class Problem:
    """The pool and constraint list Deformation::constrain builds (:126-157) and the vertex map of appendVertices"""

    def __init__(self, g, src, target, vtime, pin):
        self.g = g
        self.src = np.asarray(src, np.float32).reshape(-1, 3).astype(g.ft)
        self.target = np.asarray(target, np.float32).reshape(-1, 3).astype(g.ft)
        self.vtime = np.asarray(vtime, np.int64)
        self.pin = np.asarray(pin, bool)
        self.ids = np.zeros((len(self.src), K), np.int32)
        self.w = np.zeros((len(self.src), K))
        for v in range(len(self.src)):
            self.ids[v], self.w[v] = weigh_vertex(g, self.src[v], self.vtime[v])


def pool_of(rows7, src_time, pin_constraints):
    """Deformation::addConstraint (Deformation.cpp:76-89) over rows {src xyz, target xyz, target time}: (src, target, vertex time,
    pin flag) per pool vertex, a constraint followed by its pin"""
    rows7 = np.asarray(rows7, np.float32).reshape(-1, 7)
    src, tgt, vt, pin = [], [], [], []
    for r in rows7:
        src.append(r[0:3]); tgt.append(r[3:6]); vt.append(int(src_time)); pin.append(False)
        if pin_constraints:
            src.append(r[3:6]); tgt.append(r[3:6]); vt.append(int(r[6])); pin.append(True)
    return np.array(src, np.float32).reshape(-1, 3), np.array(tgt, np.float32).reshape(-1, 3), np.array(vt, np.int64), np.array(pin, bool)


def influences(p):
    return p.g.enabled[p.ids].any(axis=1)


def residual(p):
    """sparseResidual (:842-949): float64 vector in the reference's row order"""
    g = p.g
    ft = g.ft
    out = []
    for j in range(g.n):
        if g.enabled[j]:
            c0, c1, c2 = g.R[j][0:3], g.R[j][3:6], g.R[j][6:9]
            dot = lambda a, b: np.float64((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])
            out += [dot(c0, c1), dot(c0, c2), dot(c1, c2), dot(c0, c0) - 1.0, dot(c1, c1) - 1.0, dot(c2, c2) - 1.0]
    for j in range(g.n):
        for n in g.nbr[j]:
            if g.enabled[n] or g.enabled[j]:
                v = node_map(g, j, g.pos[n]) - (g.pos[n] + g.t[n])
                out += list(v.astype(np.float64) * SQRT_WREG)
    inf = influences(p)
    for l in range(len(p.src)):
        if inf[l]:
            pos = vertex_position(g, p.src[l], p.ids[l], p.w[l])
            out += list((pos - p.target[l]).astype(np.float64) * SQRT_WCON)
    return np.array(out, np.float64)


def jacobian(p):
    """sparseJacobian (:537-840) as CSR (indptr, columns, values); columns count from the first enabled node (backSet)"""
    g = p.g
    ft = g.ft
    en = g.enabled
    back = int((~en).sum()) * NVAR  # the enabled nodes are a suffix (times are sorted), so backSet is the disabled prefix
    indptr, cols, vals = [0], [], []

    def row(c, v):
        assert all(c[i] < c[i + 1] for i in range(len(c) - 1)), "OrderedJacobianRow::append needs ascending columns"
        cols.extend(int(x) - back for x in c)
        vals.extend(np.float64(x) for x in v)
        indptr.append(len(cols))

    for j in range(g.n):
        if en[j]:
            o = j * NVAR
            R = g.R[j]
            row([o, o + 1, o + 2, o + 3, o + 4, o + 5], [R[3], R[4], R[5], R[0], R[1], R[2]])
            row([o, o + 1, o + 2, o + 6, o + 7, o + 8], [R[6], R[7], R[8], R[0], R[1], R[2]])
            row([o + 3, o + 4, o + 5, o + 6, o + 7, o + 8], [R[6], R[7], R[8], R[3], R[4], R[5]])
            two = ft(2)
            row([o, o + 1, o + 2], [two * R[0], two * R[1], two * R[2]])
            row([o + 3, o + 4, o + 5], [two * R[3], two * R[4], two * R[5]])
            row([o + 6, o + 7, o + 8], [two * R[6], two * R[7], two * R[8]])
    for j in range(g.n):
        o = j * NVAR
        for n in g.nbr[j]:
            if en[n] or en[j]:
                d = g.pos[n] - g.pos[j]
                on = n * NVAR
                for c in range(3):
                    cc, vv = [], []
                    if on < o and en[n]:
                        cc.append(on + 9 + c); vv.append(-1.0 * SQRT_WREG)
                    if en[j]:
                        cc += [o + c, o + 3 + c, o + 6 + c, o + 9 + c]
                        vv += [np.float64(d[0]) * SQRT_WREG, np.float64(d[1]) * SQRT_WREG, np.float64(d[2]) * SQRT_WREG, 1.0 * SQRT_WREG]
                    if on > o and en[n]:
                        cc.append(on + 9 + c); vv.append(-1.0 * SQRT_WREG)
                    row(cc, vv)
    inf = influences(p)
    for l in range(len(p.src)):
        if inf[l]:
            for c in range(3):
                cc, vv = [], []
                for i in range(K):
                    a = p.ids[l][i]
                    if en[a]:
                        o = a * NVAR
                        d = (p.src[l] - g.pos[a]) * ft(p.w[l][i])
                        cc += [o + c, o + 3 + c, o + 6 + c, o + 9 + c]
                        vv += [np.float64(d[0]) * SQRT_WCON, np.float64(d[1]) * SQRT_WCON, np.float64(d[2]) * SQRT_WCON, p.w[l][i] * SQRT_WCON]
                row(cc, vv)
    return np.array(indptr, np.int32), np.array(cols, np.int32), np.array(vals, np.float64)


def apply_delta(g, delta):
    """applyDeltaSparse (:960-990): float += double"""
    z = 0
    for j in range(g.n):
        if g.enabled[j]:
            g.R[j] = (g.R[j].astype(np.float64) + delta[z:z + 9]).astype(g.ft)
            g.t[j] = (g.t[j].astype(np.float64) + delta[z + 9:z + 12]).astype(g.ft)
            z += NVAR


def mean_cons_error(p):
    """nonRelativeConstraintError (:1011-1026): a float running sum in constraint order, divided by their number"""
    ft = p.g.ft
    s = ft(0)
    for l in range(len(p.src)):
        s = s + norm3(vertex_position(p.g, p.src[l], p.ids[l], p.w[l]) - p.target[l])
    with np.errstate(all="ignore"):
        return ft(s / ft(len(p.src)))


def lane_sum(x):
    """The fixed order of squaredNorm() / norm(): 256 strided partial sums, then a pairwise fold"""
    x = np.asarray(x, np.float64)
    m = len(x)
    pad = np.zeros(max(1, -(-m // 256)) * 256)
    pad[:m] = x
    lanes = np.zeros(256)
    for r in pad.reshape(-1, 256):
        lanes = lanes + r
    s = 128
    while s >= 1:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return np.float64(lanes[0])


# ---- the linear solve: banded Cholesky of J^T J ---------------------------------------------------------------------------------
def normal_equations(indptr, cols, vals, r, ncols, dtype=np.float64):
    """U[c, d] = (J^T J)[c, c + d] for 0 <= d <= HALF_BAND (upper band), g = -J^T r; also the widest row met"""
    bw = HALF_BAND
    U = np.zeros((ncols + bw + 2, bw + 1), dtype)
    gvec = np.zeros(ncols, dtype)
    widest = 0
    v = vals.astype(dtype)
    rr = r.astype(dtype)
    for i in range(len(indptr) - 1):
        a, b = indptr[i], indptr[i + 1]
        if a == b:
            continue
        c = cols[a:b]
        x = v[a:b]
        widest = max(widest, int(c[-1] - c[0]))
        for q in range(b - a):
            U[c[q], c[q:] - c[q]] += x[q] * x[q:]
        gvec[c] -= x * rr[i]
    return U, gvec, widest


def band_cholesky_solve(U, gvec, failed_at=None):
    """In-place right-looking Cholesky on the upper band, then both triangular solves.  None for a non-positive pivot (its scalar
    column is appended to failed_at, where given)."""
    bw = U.shape[1] - 1
    n = len(gvec)
    dtype = U.dtype
    diag0 = U[:n, 0].copy()
    flat = U.reshape(-1)
    isz = flat.itemsize
    for k in range(n):
        piv = U[k, 0]
        if not piv > dtype.type(PIVOT_REL) * diag0[k]:
            if failed_at is not None:
                failed_at.append(k)
            return None
        d = np.sqrt(piv)
        U[k, 0] = d
        U[k, 1:] /= d
        col = U[k, 1:]
        # trailing window: element (m, t), t >= m, of rows k+1.. is U[k+1+m, t-m] = flat[(k+1)(bw+1) + m bw + t]
        V = np.lib.stride_tricks.as_strided(flat[(k + 1) * (bw + 1):], shape=(bw, bw), strides=(bw * isz, isz))
        V -= np.triu(np.outer(col, col))
    y = gvec.copy()
    y = np.concatenate([y, np.zeros(bw + 1, dtype)])
    for k in range(n):
        y[k] = y[k] / U[k, 0]
        y[k + 1:k + 1 + bw] -= y[k] * U[k, 1:]
    y[n:] = 0
    for k in range(n - 1, -1, -1):
        y[k] = (y[k] - np.dot(U[k, 1:], y[k + 1:k + 1 + bw])) / U[k, 0]
    return y[:n]


def solve(indptr, cols, vals, r, ncols, solver="A", failed_at=None):
    dtype = np.float64 if solver == "A" else np.longdouble
    U, gvec, widest = normal_equations(indptr, cols, vals, r, ncols, dtype)
    gmax = np.abs(gvec).max() if ncols else 0
    Ukeep = U.copy()
    x = band_cholesky_solve(U, gvec, failed_at)
    return x, Ukeep, gvec, widest


def band_matvec(U, x):
    """(J^T J) x from the upper band, in U's precision"""
    n = len(x)
    bw = U.shape[1] - 1
    xe = np.concatenate([x.astype(U.dtype), np.zeros(bw + 1, U.dtype)])
    y = np.zeros(n + bw + 1, U.dtype)
    for d in range(bw + 1):
        y[:n] += U[:n, d] * xe[d:d + n]
        if d:
            y[d:d + n] += U[:n, d] * xe[:n]
    return y[:n]


def dense_normal_matrix(indptr, cols, vals, ncols):
    J = np.zeros((len(indptr) - 1, ncols))
    for i in range(len(indptr) - 1):
        J[i, cols[indptr[i]:indptr[i + 1]]] = vals[indptr[i]:indptr[i + 1]]
    return J.T @ J


# ---- optimiseGraphSparse (:457-535) with fernMatch = false --------------------------------------------------------------------------
def optimise(p, last_deform_time, solver="A", delta_override=None):
    """Returns a dict: optimised, status, iterations, exit, error (float), meanConsErr before / after, per-iteration errors and delta
    norms, and the first iteration's residual, Jacobian, delta and normal equations.  delta_override(iteration, info) may supply the
    delta of an iteration (to follow another solver's path)."""
    g = p.g
    ft = g.ft
    out = dict(status=STATUS_OK, optimised=True, iterations=0, exit=0, errors=[], delta_norms=[], thresholds=[])
    out["meanConsErr_before"] = mean_cons_error(p)
    g.enabled = g.times > int(last_deform_time)
    assert not g.enabled.any() or g.enabled[np.argmax(g.enabled):].all()
    ncols = int(g.enabled.sum()) * NVAR
    out["enabled"] = ncols // NVAR
    r = residual(p)
    out["residual0"] = r.copy()
    error = ft(lane_sum(r * r))
    out["error0"] = error
    last_error = np.float64(error)
    if ncols == 0:
        out.update(exit=5, error=error, meanConsErr_after=out["meanConsErr_before"], widest=0)
        return out
    J = jacobian(p)
    out["jacobian0"] = J
    widest = 0
    it = 0
    while it < 3:
        it += 1
        failed_at = []
        x, U, gvec, wd = solve(*J, r, ncols, solver, failed_at)
        widest = max(widest, wd)
        if it == 1:
            out["U0"], out["g0"] = U, gvec
        if x is None:
            out.update(status=STATUS_SINGULAR, optimised=False, iterations=it, error=error, widest=widest, pivot_failed_at=failed_at[0])
            g.reset()
            out["meanConsErr_after"] = mean_cons_error(p)
            return out
        delta = np.asarray(x, np.float64)
        if delta_override is not None:
            delta = delta_override(it, delta)
        if it == 1:
            out["delta0"] = delta.copy()
        apply_delta(g, delta)
        r = residual(p)
        error = ft(lane_sum(r * r))
        error_diff = np.float64(error) - last_error
        dnorm = np.sqrt(lane_sum(delta * delta))
        out["errors"].append(error)
        out["delta_norms"].append(dnorm)
        e = np.float64(error)
        # each quantity of :515 against its threshold, as (value, threshold) pairs for the margin check of the tests
        out["thresholds"].append([(e, last_error), (dnorm, 1e-2), (e, 1e-3), (abs(error_diff), 1e-5 * e)])
        out["iterations"] = it
        if e > last_error:
            out["exit"] = 1
            break
        if dnorm < 1e-2:
            out["exit"] = 2
            break
        if e < 1e-3:
            out["exit"] = 3
            break
        if abs(error_diff) < 1e-5 * e:
            out["exit"] = 4
            break
        last_error = e
        if it < 3:
            J = jacobian(p)
    out["error"] = error
    out["widest"] = widest
    out["meanConsErr_after"] = mean_cons_error(p)
    return out


def node_table(g):
    """16 floats per node (Deformation.cpp:192-201): position, rotation (column-major), translation, time"""
    tab = np.zeros((g.n, 16), np.float32)
    tab[:, 0:3] = g.pos
    tab[:, 3:12] = g.R
    tab[:, 12:15] = g.t
    tab[:, 15] = g.ftimes
    return tab


def pool_of_batches(batches):
    """pool_of over several addConstraint batches (rows7, src_time, pin) in call order: the pool of every batch behind the one before.
    Also, per pool vertex, the relative row it becomes (numbered across the batches, -1 for a pin) and that row's times."""
    src, tgt, vt, pin = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, bool)]
    rel_times = []
    for rows7, src_time, pins in batches:
        rows7 = np.asarray(rows7, np.float32).reshape(-1, 7)
        s, t, v, q = pool_of(rows7, src_time, pins)
        src.append(s); tgt.append(t); vt.append(v); pin.append(q)
        rel_times += [(np.float32(src_time), r[6]) for r in rows7]
    pin = np.concatenate(pin)
    rel_idx = np.where(pin, -1, np.cumsum(~pin) - 1)
    return np.concatenate(src), np.concatenate(tgt), np.concatenate(vt), pin, rel_idx, rel_times


def constrain(nodes4, rows7, src_time, pin_constraints, time, relax_graph, last_deform_time, solver="A", delta_override=None, graph=None):
    """Deformation::constrain for one batch of constraints (see constrain_batches)"""
    return constrain_batches(nodes4, [(rows7, src_time, pin_constraints)], time, relax_graph, last_deform_time, solver, delta_override, graph)


def constrain_batches(nodes4, batches, time, relax_graph, last_deform_time, solver="A", delta_override=None, graph=None):
    """Deformation::constrain (Deformation.cpp:91-220) without ferns and poses, over the constraints of several addConstraint batches
    (rows7, src_time, pin) in call order.  Returns the dict of optimise plus applied, table, pool (the deformed pool vertices), relative
    (rows {deformed src, target, src time, target time} of the non-pin constraints, in constraint order), rel_idx (per pool vertex, its
    row of relative or -1), lastDeformTime, ids, weights."""
    g = graph if graph is not None else Graph(nodes4)
    src, tgt, vt, pin, rel_idx, rel_times = pool_of_batches(batches)
    p = Problem(g, src, tgt, vt, pin)
    out = optimise(p, 0 if relax_graph else last_deform_time, solver, delta_override)
    out["ids"], out["weights"] = p.ids, p.w
    out["applied"] = out["status"] == STATUS_OK  # fernMatch = false: :165
    out["graph"] = g
    out["lastDeformTime"] = last_deform_time
    out["table"] = node_table(g)
    out["rel_idx"] = rel_idx
    if out["applied"]:
        pool = np.array([vertex_position(g, p.src[v], p.ids[v], p.w[v]) for v in range(len(p.src))], np.float32).reshape(-1, 3)
        out["pool"] = pool
        rel = []
        for v in range(len(p.src)):
            if not pin[v]:
                rel.append(np.concatenate([pool[v], tgt[v], rel_times[rel_idx[v]]]))
        out["relative"] = np.array(rel, np.float32).reshape(-1, 8)
        if not relax_graph:
            out["lastDeformTime"] = int(time)  # :203-206
    return out
