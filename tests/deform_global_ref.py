"""CPU restatement of what the global deformation object (dms_deform_create_global, include/dmslam_deform.h) adds to tests/deform_ref.py:
relative constraints, fernMatch = true, and the poses.  numpy only (scipy's LAPACK Cholesky for the float64 solve).

What is restated, by file and line:
  Deformation::constrain, pool of relative constraints   Deformation.cpp:126-157                       pool_of_calls
  sparseResidual / sparseJacobian, relative rows          DeformationGraph.cpp:892-944, :653-801       residual, jacobian, rel_merge
  OrderedJacobianRow::addTo                               OrderedJacobianRow.h:54-58                   rel_merge
  nonRelativeConstraintError                              :1011-1026                                   mean_cons_error
  optimiseGraphSparse with fernMatch = true               :457-535 (exits :465 and :516)               optimise
  the acceptance test                                     Deformation.cpp:165                          constrain_global
  setPosesSeq / applyGraphToPoses                         :133-250, :102-131                           pose_weights, apply_poses

Orders fixed here beyond those of deform_ref.py (csrc/deform_rows.hpp states the same):
  * the merged weight map is the source vertex's four entries, then the target vertex's four, bubble-sorted by node id exactly as
    VertexWeightMap::sort does (stable); a node on both sides has one entry per column, ((val / sqrt(wCon)) + value) * sqrt(wCon);
  * a relative constraint is no term of meanConsErr's float sum but counts in its divisor;
  * U V^T of a pose's rotation is the orthogonal polar factor: POLAR_STEPS Newton steps X <- 0.5 (X + X^-T) in float64 from the float
    matrix, X^-T as cofactors over the determinant (polar_newton, "A"); numpy.linalg.svd in float64 is the independent check ("svd").
    A matrix that is not finite or has |det| < 2^-20 keeps the pose's old rotation;
  * the linear solve: A = J^T J is dense here.  Solver "A": float64 (LAPACK Cholesky), solver "B": np.longdouble (right-looking
    Cholesky in numpy).  The pivot rule of deform_ref.py holds (2^-40 of the diagonal entry).
"""
import numpy as np
import scipy.linalg

from tests import deform_ref as R

K, NVAR = R.K, R.NVAR
SQRT_WCON = R.SQRT_WCON
POLAR_STEPS = 40
POLAR_MIN_DET = 2.0 ** -20
EXIT_NAMES = dict(R.EXIT_NAMES)
EXIT_NAMES.update({6: "constraints met", 7: "error large"})
ABS, REL_SRC, REL_TGT = 0, 1, 2


def pool_of_calls(calls):
    """calls, in order: ("abs", rows7, src_time, pin) as dms_deform_add_constraints, ("rel", rows8) as _add_relative_constraints.
    Per pool vertex: source, target (absolute ones), vertex time, kind (ABS; REL_SRC followed by its REL_TGT)."""
    src, tgt, vt, kind = [], [], [], []
    for c in calls:
        if c[0] == "abs":
            s, t, v, _ = R.pool_of(c[1], c[2], c[3])
            src += list(s); tgt += list(t); vt += list(v); kind += [ABS] * len(s)
        else:
            for r in np.asarray(c[1], np.float32).reshape(-1, 8):
                src += [r[0:3], r[3:6]]; tgt += [r[3:6], r[3:6]]; vt += [int(r[6]), int(r[7])]; kind += [REL_SRC, REL_TGT]
    return (np.array(src, np.float32).reshape(-1, 3), np.array(tgt, np.float32).reshape(-1, 3), np.array(vt, np.int64), np.array(kind, np.int32))


def rel_merge(g, src, ids_s, w_s, tgt, ids_t, w_t):
    """sparseJacobian :692-801 over all nodes (the caller drops disabled ones): (node ids ascending, 4 coefficients per node)"""
    lst = [(int(ids_s[a]), w_s[a], False) for a in range(K)] + [(int(ids_t[a]), w_t[a], True) for a in range(K)]
    done, size = False, len(lst)
    while not done:  # VertexWeightMap::sort
        done = True
        for i in range(size - 1):
            if lst[i][0] > lst[i + 1][0]:
                done = False
                lst[i], lst[i + 1] = lst[i + 1], lst[i]
        size -= 1
    mid, mc = [], []
    for node, w, rel in lst:
        if rel:
            d = (g.pos[node] - tgt) * g.ft(w)
            v = [np.float64(d[0]), np.float64(d[1]), np.float64(d[2]), -np.float64(w)]
        else:
            d = (src - g.pos[node]) * g.ft(w)
            v = [np.float64(d[0]), np.float64(d[1]), np.float64(d[2]), np.float64(w)]
        if mid and mid[-1] == node:  # checkList: addTo
            mc[-1] = [((mc[-1][q] / SQRT_WCON) + v[q]) * SQRT_WCON for q in range(4)]
        else:
            mid.append(node)
            mc.append([v[q] * SQRT_WCON for q in range(4)])
    return np.array(mid, np.int32), np.array(mc, np.float64)


class Problem:
    def __init__(self, g, src, tgt, vtime, kind):
        self.g = g
        self.src, self.target = src.astype(g.ft), tgt.astype(g.ft)
        self.vtime, self.kind = vtime, kind
        n = len(src)
        self.ids = np.zeros((n, K), np.int32)
        self.w = np.zeros((n, K))
        for v in range(n):
            self.ids[v], self.w[v] = R.weigh_vertex(g, self.src[v], self.vtime[v])
        self.mid, self.mc = [None] * n, [None] * n
        for v in range(n):
            if kind[v] == ABS:
                self.mid[v] = self.ids[v].copy()
                self.mc[v] = np.array([list(np.float64((self.src[v] - g.pos[a]) * g.ft(w)) * SQRT_WCON) + [w * SQRT_WCON]
                                       for a, w in zip(self.ids[v], self.w[v])])
            elif kind[v] == REL_SRC:
                self.mid[v], self.mc[v] = rel_merge(g, self.src[v], self.ids[v], self.w[v], self.src[v + 1], self.ids[v + 1], self.w[v + 1])
        self.n_constraints = int((kind != REL_TGT).sum())
        self._empty = R.Problem(g, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int64), np.zeros(0, bool))

    def rows(self):
        """the pool vertices that own constraint rows now: any node of the merged map enabled (:657-680)"""
        return [v for v in range(len(self.src)) if self.kind[v] != REL_TGT and self.g.enabled[self.mid[v]].any()]

    def position(self, v):
        return R.vertex_position(self.g, self.src[v], self.ids[v], self.w[v])


def residual(p):
    out = list(R.residual(p._empty))  # rotation and regularisation rows
    for v in p.rows():
        tgt = p.position(v + 1) if p.kind[v] == REL_SRC else p.target[v]
        out += list((p.position(v) - tgt).astype(np.float64) * SQRT_WCON)
    return np.array(out, np.float64)


def jacobian(p):
    indptr, cols, vals = R.jacobian(p._empty)
    indptr, cols, vals = list(indptr), list(cols), list(vals)
    en = p.g.enabled
    back = int((~en).sum()) * NVAR
    for v in p.rows():
        for c in range(3):
            for a, c4 in zip(p.mid[v], p.mc[v]):
                if en[a]:
                    o = int(a) * NVAR - back
                    cols += [o + c, o + 3 + c, o + 6 + c, o + 9 + c]
                    vals += list(c4)
            indptr.append(len(cols))
    return np.array(indptr, np.int32), np.array(cols, np.int32), np.array(vals, np.float64)


def mean_cons_error(p):
    ft = p.g.ft
    s = ft(0)
    for v in range(len(p.src)):
        if p.kind[v] == ABS:
            s = s + R.norm3(p.position(v) - p.target[v])
    with np.errstate(all="ignore"):
        return ft(s / ft(p.n_constraints))


def envelope(indptr, cols, nblocks):
    """first[i]: the smallest block column that any row of J couples block column i to (the pattern of J^T J)"""
    first = np.arange(nblocks)
    for a, b in zip(indptr[:-1], indptr[1:]):
        if b > a:
            blk = np.unique(cols[a:b] // NVAR)
            first[blk] = np.minimum(first[blk], blk.min())
    return first.astype(np.int32)


def normal_equations(indptr, cols, vals, r, ncols, dtype):
    A = np.zeros((ncols, ncols), dtype)
    g = np.zeros(ncols, dtype)
    v, rr = vals.astype(dtype), r.astype(dtype)
    for i in range(len(indptr) - 1):
        a, b = indptr[i], indptr[i + 1]
        if b > a:
            c, x = cols[a:b], v[a:b]
            A[np.ix_(c, c)] += np.outer(x, x)
            g[c] -= x * rr[i]
    return A, g


def dense_solve(A, g):
    """x with A x = g, or None when a pivot is at or below 2^-40 of its diagonal entry.  float64: LAPACK; longdouble: numpy loop"""
    n = len(g)
    diag0 = np.diag(A).copy()
    if A.dtype == np.float64:
        try:
            L = scipy.linalg.cholesky(A, lower=True)
        except np.linalg.LinAlgError:
            return None
        if not (np.diag(L) ** 2 > R.PIVOT_REL * diag0).all():
            return None
        return scipy.linalg.cho_solve((L, True), g)
    L = A.copy()
    for k in range(n):
        if not L[k, k] > A.dtype.type(R.PIVOT_REL) * diag0[k]:
            return None
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        nz = np.nonzero(L[k + 1:, k])[0] + k + 1
        if len(nz):
            L[np.ix_(nz, nz)] -= np.outer(L[nz, k], L[nz, k])
    y = g.copy()
    for k in range(n):
        y[k] = (y[k] - np.dot(L[k, :k], y[:k])) / L[k, k]
    for k in range(n - 1, -1, -1):
        y[k] = (y[k] - np.dot(L[k + 1:, k], y[k + 1:])) / L[k, k]
    return y


def optimise(p, solver="A"):
    """optimiseGraphSparse(fernMatch = true, lastDeformTime = 0); the dict of deform_ref.optimise, plus `first`"""
    g, ft = p.g, p.g.ft
    out = dict(status=R.STATUS_OK, optimised=True, iterations=0, exit=0, errors=[], delta_norms=[], thresholds=[])
    mce = mean_cons_error(p)
    out["meanConsErr_before"] = mce
    g.enabled = g.times > 0
    ncols = int(g.enabled.sum()) * NVAR
    out["enabled"] = ncols // NVAR
    if np.float64(mce) < 0.06:  # :465 (float against a double literal)
        out.update(optimised=False, exit=6, error=ft(0), error0=ft(0), residual0=np.zeros(0), meanConsErr_after=mce,
                   jacobian0=(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)))
        return out
    r = residual(p)
    out["residual0"] = r.copy()
    error = ft(R.lane_sum(r * r))
    out["error0"] = error
    last_error = np.float64(error)
    if ncols == 0:
        out.update(exit=5, error=error, meanConsErr_after=mce, jacobian0=(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)))
        return out
    J = jacobian(p)
    out["jacobian0"] = J
    out["first"] = envelope(J[0], J[1], ncols // NVAR)
    dtype = np.float64 if solver == "A" else np.longdouble
    it = 0
    while it < 3:
        it += 1
        A, gv = normal_equations(*J, r, ncols, dtype)
        if it == 1:
            out["A0"], out["g0"] = A.copy(), gv.copy()
        x = dense_solve(A, gv)
        if x is None:
            out.update(status=R.STATUS_SINGULAR, optimised=False, iterations=it, error=error)
            g.reset()
            out["meanConsErr_after"] = mean_cons_error(p)
            return out
        delta = np.asarray(x, np.float64)
        if it == 1:
            out["delta0"] = delta.copy()
        R.apply_delta(g, delta)
        r = residual(p)
        error = ft(R.lane_sum(r * r))
        e = np.float64(error)
        error_diff = e - last_error
        dnorm = np.sqrt(R.lane_sum(delta * delta))
        out["errors"].append(error)
        out["delta_norms"].append(dnorm)
        th = [(e, last_error), (dnorm, 1e-2), (e, 1e-3), (abs(error_diff), 1e-5 * e)]
        if it == 1:
            th.append((e, 10.0))
        out["thresholds"].append(th)
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
        if it == 1 and error > np.float32(10.0):  # :516
            out["exit"] = 7
            break
        last_error = e
        if it < 3:
            J = jacobian(p)
    out["error"] = error
    out["meanConsErr_after"] = mean_cons_error(p)
    return out


# ---- poses ------------------------------------------------------------------------------------------------------------------------------
def pose_weights(g, times, poses):
    ids, w = np.zeros((len(times), K), np.int32), np.zeros((len(times), K))
    for i in range(len(times)):
        ids[i], w[i] = R.weigh_vertex(g, np.asarray(poses[i], g.ft)[:3, 3], int(times[i]))
    return ids, w


def _cofactors(X):
    C = [X[4] * X[8] - X[5] * X[7], X[5] * X[6] - X[3] * X[8], X[3] * X[7] - X[4] * X[6],
         X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
         X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]]
    return C, (X[0] * C[0] + X[1] * C[1]) + X[2] * C[2]


def polar_newton(M):
    """solver "A" of the polar factor: the product's fixed float64 sequence.  None when the rule keeps the old rotation."""
    X = [np.float64(x) for x in np.asarray(M, np.float32).reshape(9)]
    with np.errstate(all="ignore"):
        _, det0 = _cofactors(X)
        if not np.isfinite(X).all() or not abs(det0) >= POLAR_MIN_DET:
            return None
        for _ in range(POLAR_STEPS):
            C, det = _cofactors(X)
            X = [np.float64(0.5) * (X[e] + C[e] / det) for e in range(9)]
    return np.array(X, np.float64).reshape(3, 3).astype(np.float32)


def polar_svd(M):
    M = np.asarray(M, np.float32).astype(np.float64).reshape(3, 3)
    if not np.isfinite(M).all() or not abs(np.linalg.det(M)) >= POLAR_MIN_DET:
        return None
    U, _, Vt = np.linalg.svd(M)
    return (U @ Vt).astype(np.float32)


def pose_matrix(g, ids, w, pose):
    """newPosition and rotation * R of :113-124, floats"""
    ft = g.ft
    pose = np.asarray(pose, ft)
    pos, rs = np.zeros(3, ft), np.zeros(9, ft)
    for j in range(K):
        a = ids[j]
        wf = ft(w[j])
        pos = pos + wf * R.node_map(g, a, pose[:3, 3])
        rs = rs + wf * g.R[a]
    M = np.zeros((3, 3), ft)
    for r in range(3):
        for c in range(3):
            M[r, c] = (rs[r] * pose[0, c] + rs[3 + r] * pose[1, c]) + rs[6 + r] * pose[2, c]
    return pos, M


def apply_poses(g, ids, w, poses, polar="A"):
    """applyGraphToPoses: (new poses, number of rotations kept)"""
    out, kept = np.array(poses, np.float32).reshape(-1, 4, 4).copy(), 0
    for i in range(len(out)):
        pos, M = pose_matrix(g, ids[i], w[i], out[i])
        U = polar_newton(M) if polar == "A" else polar_svd(M)
        out[i, :3, 3] = pos
        if U is None:
            kept += 1
        else:
            out[i, :3, :3] = U
    return out, kept


def constrain_global(nodes4, calls, pose_times, poses, solver="A", polar="A", graph=None):
    """Deformation::constrain(..., fernMatch = true, poseGraph, relaxGraph = true).  The dict of optimise plus applied, ids, weights,
    kinds, pose_ids, pose_weights, and, when applied, table, pool, poses (else the poses as given and no table / pool)."""
    g = graph if graph is not None else R.Graph(nodes4)
    p = Problem(g, *pool_of_calls(calls))
    pids, pw = pose_weights(g, pose_times, poses)
    out = optimise(p, solver)
    out.update(ids=p.ids, weights=p.w, kinds=p.kind, graph=g, problem=p, pose_ids=pids, pose_weights=pw)
    out["applied"] = bool(out["status"] == R.STATUS_OK and out["optimised"] and np.float64(out["meanConsErr_after"]) < 0.0003
                          and np.float64(out["error"]) < 0.12)
    out["poses"], out["kept"] = np.array(poses, np.float32).reshape(-1, 4, 4).copy(), 0
    if out["applied"]:
        out["poses"], out["kept"] = apply_poses(g, pids, pw, poses, polar)
        out["pool"] = np.array([p.position(v) for v in range(len(p.src))], np.float32).reshape(-1, 3)
        out["table"] = R.node_table(g)
    return out
