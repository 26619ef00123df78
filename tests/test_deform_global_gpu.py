"""The global deformation object on the GPU (dms_deform_create_global, include/dmslam_deform.h) against the CPU restatement
tests/deform_global_ref.py on the inputs of tests/deform_global_cases.py, with the bars of tests/test_deform_gpu.py:

  bits    weights, first residual, first Jacobian, error_initial, mean_cons_err_before, the row envelope and the pose weights equal the
          restatement's;
  path    status, iterations, exit reason, optimised and applied equal the restatement's on every input, the five exits of (f) included;
  delta   relinf(kernel, B) <= 8 e_A with e_A = max relinf(A, B) over the inputs, measured from the restatement (A: float64 LAPACK
          Cholesky, B: np.longdouble); at (e), where B is not run, |A delta - g| / |g| in np.longdouble against 8 times the float64 solve's;
  table   share of entries differing from B <= 2 x A's share + 0.01, max ulp <= A's + 1; pool within 4e-6 of B;
  poses   translations within 4e-6 of B; rotations against B with the polar factor by numpy's float64 SVD: 2^-23 (the bar of the CPU
          test's SVD check) plus what the kernel's node rotations differ from B's by, carried through the weighted sum (weights sum to
          one), the three-term product with the pose's rotation and the polar factor: 4 x the largest difference of a rotation entry of
          the table; orthonormal to 2^-22.
Band parity: dms_deform_constrain on a global object gives a dms_deform_create object's bits on an absolute-only input."""
import numpy as np
import pytest

from tests import deform_cases, deform_global_cases as GC, deform_global_ref as G, deform_ref as R

pytestmark = pytest.mark.gpu

STAGED = GC.staged_cases()
EXITS = GC.exit_cases()
SOLVED = STAGED + [c for c, _, _ in EXITS]
ulps = deform_cases.ulps


@pytest.fixture(scope="module")
def dfm():
    from densemonoslam_amd import capi, deform

    assert capi.device_count() >= 1, "no MI355X visible"
    return deform


@pytest.fixture(scope="module")
def solver(dfm):
    d = dfm.GlobalDeformation(max_nodes=410, max_constraints=2048, max_relative=16, max_poses=16)
    yield d
    d.close()


def load(d, c):
    d.setNodes(c.nodes)
    d.clearConstraints()
    for call in c.calls:
        if call[0] == "abs":
            d.addConstraints(call[1], call[2], call[3])
        else:
            d.addRelativeConstraints(call[1])
    d.setPoses(c.pose_times, c.poses)


def gpu_run(d, c):
    load(d, c)
    d.constrainGlobal(c.tick)
    r = d.result()
    ids, w = d.vertexWeights()
    pids, pw = d.poseWeights()
    return dict(result=r, ids=ids, weights=w, residual0=d.firstResidual(), jacobian0=d.firstJacobian(), delta0=d.firstDelta(), table=d.graph(),
                pool=d.pool(), poses=d.poses()[1], kept=d.keptRotations(), pose_ids=pids, pose_weights=pw, first=d.envelope())


def ref_run(c, solver, polar="A"):
    return G.constrain_global(c.nodes, c.calls, c.pose_times, c.poses, solver, polar)


@pytest.fixture(scope="module")
def solved(solver):
    """every input below capacity once: the GPU's run, the restatement with solver A, and with solver B and the SVD polar factor"""
    return {c.name: (gpu_run(solver, c), ref_run(c, "A"), ref_run(c, "B", "svd")) for c in SOLVED}


@pytest.fixture(scope="module")
def capacity(solver):
    """(e): the GPU's run and the restatement's with the float64 solve (the np.longdouble one is not run at this size)"""
    c = GC.case_e()
    a = ref_run(c, "A")
    a["A0"] = None  # 194 MB, not needed again
    return c, gpu_run(solver, c), a


def relinf(a, b):
    return float(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble)).max() / np.abs(np.asarray(b, np.longdouble)).max())


@pytest.mark.parametrize("case", SOLVED, ids=repr)
def test_weights_residual_jacobian_envelope_are_the_restatements_bits(solved, case):
    g, a, _ = solved[case.name]
    assert np.array_equal(g["ids"], a["ids"]) and g["weights"].tobytes() == a["weights"].tobytes()
    assert np.array_equal(g["pose_ids"], a["pose_ids"]) and g["pose_weights"].tobytes() == a["pose_weights"].tobytes()
    assert g["residual0"].tobytes() == a["residual0"].tobytes()
    for got, want, what in zip(g["jacobian0"], a["jacobian0"], ("indptr", "columns", "values")):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), what
    r = g["result"]
    assert r.nodes == len(case.nodes) and r.enabled_nodes == a["enabled"] and r.rows == len(a["residual0"]) and r.constraints == len(a["ids"])
    assert np.float32(r.error_initial).tobytes() == np.float32(a["error0"]).tobytes()
    assert np.float32(r.mean_cons_err_before).tobytes() == np.float32(a["meanConsErr_before"]).tobytes()
    assert np.array_equal(g["first"], a.get("first", np.zeros(0, np.int32)))


@pytest.mark.parametrize("case", SOLVED, ids=repr)
def test_loop_takes_the_restatements_path(solved, case):
    g, a, _ = solved[case.name]
    r = g["result"]
    assert (r.status, r.iterations, r.exit_reason, r.optimised, r.applied) == (a["status"], a["iterations"], a["exit"], int(a["optimised"]), int(a["applied"]))
    for i in range(r.iterations):
        assert abs(r.iter_error[i] - float(a["errors"][i])) <= 1e-4 * float(a["errors"][i]), (i, r.iter_error[i], a["errors"][i])
        assert abs(r.iter_delta_norm[i] - a["delta_norms"][i]) <= 1e-6 * a["delta_norms"][i]
    assert r.relative_rows == 0 and r.last_deform_time == 0  # no newRelativeCons, lastDeformTime not advanced


def test_every_exit_is_taken_on_the_gpu(solved):
    got = [(solved[c.name][0]["result"].exit_reason, solved[c.name][0]["result"].applied) for c, _, _ in EXITS]
    assert got[0] == (6, 0) and got[1] == (7, 0) and got[2][1] == 0 and got[3][1] == 0 and got[4][1] == 1, got
    r = solved[EXITS[0][0].name][0]["result"]
    assert (r.optimised, r.iterations, r.rows, r.error, r.mean_cons_err_after) == (0, 0, 0, 0.0, r.mean_cons_err_before)


def test_first_delta_is_within_eight_times_the_float64_solves_error(solved):
    have = {n: v for n, v in solved.items() if "delta0" in v[1]}
    e_a = max(relinf(a["delta0"], b["delta0"]) for _, a, b in have.values())
    report = {name: (relinf(g["delta0"], b["delta0"]), relinf(a["delta0"], b["delta0"])) for name, (g, a, b) in have.items()}
    print("e_A = %.3e; per case (kernel vs B, A vs B): %s" % (e_a, {k: "%.3e / %.3e" % v for k, v in report.items()}))
    assert len(have) == len(SOLVED) - 1 and 0 < e_a < 1e-6
    for name, (ek, _) in report.items():
        assert ek <= 8 * e_a, (name, ek, e_a)


def test_capacity_case(capacity):
    """(e): the restatement's bits, and |A delta - g| / |g| in np.longdouble for the kernel's delta against the float64 solve's"""
    c, g, a = capacity
    assert g["residual0"].tobytes() == a["residual0"].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(g["jacobian0"], a["jacobian0"]))
    assert np.float32(g["result"].mean_cons_err_before).tobytes() == np.float32(a["meanConsErr_before"]).tobytes()
    indptr, cols, vals = a["jacobian0"]
    assert np.array_equal(g["first"], G.envelope(indptr, cols, 410)) and (np.arange(410) - g["first"] > 19).any()
    v, r0 = vals.astype(np.longdouble), a["residual0"].astype(np.longdouble)
    rows = [(cols[s:e], v[s:e]) for s, e in zip(indptr[:-1], indptr[1:])]
    gv = np.zeros(410 * 12, np.longdouble)
    for (cc, x), ri in zip(rows, r0):
        gv[cc] -= x * ri

    def res(x):
        x = np.asarray(x, np.longdouble)
        y = np.zeros_like(gv)
        for cc, xv in rows:
            y[cc] += xv * np.dot(xv, x[cc])
        return float(np.abs(y - gv).max() / np.abs(gv).max())

    rk, ra = res(g["delta0"]), res(a["delta0"])
    print("(410, 2048 + 8 relative): |A delta - g|/|g|: kernel %.3e, float64 solve %.3e" % (rk, ra))
    assert rk <= 8 * ra, (rk, ra)
    r = g["result"]
    assert (r.status, r.iterations, r.exit_reason, r.optimised, r.applied) == (a["status"], a["iterations"], a["exit"], 1, 1) and a["applied"]
    # accepted: table, pool and poses at capacity, against the float64 restatement (B is not run here, so A's own distance from B is
    # not known and the ulp bar of the smaller inputs cannot be formed).  The two first deltas differ by some 1e-11 of 0.2; an entry
    # (float += double per iteration, applyDeltaSparse) then differs only where that crosses a float rounding boundary, by one float
    # step of the value it had in that iteration - at most 2^-23 for |value| < 2 - and each of the up to three iterations can add
    # one: 3 x 2^-23 absolute (an entry that ends near zero keeps the step of the larger value it passed through, so a count of ITS
    # float steps says nothing), on at most 1 % of the entries
    uk = ulps(g["table"], a["table"])
    dtab = float(np.abs(g["table"].astype(np.float64) - a["table"]).max())
    print("(e) table against A: share differing %.4f, max |difference| %.3e (%d ulp of the entry); pool %.3e; poses %.3e" % (
        float((uk > 0).mean()), dtab, uk.max(), np.abs(g["pool"] - a["pool"]).max(), np.abs(g["poses"] - a["poses"]).max()))
    assert float((uk > 0).mean()) <= 0.01 and dtab <= 3 * 2.0 ** -23
    assert g["pool"].shape == a["pool"].shape == (4112, 3) and np.abs(g["pool"] - a["pool"]).max() <= 4e-6
    assert np.abs(g["poses"][:, :3, 3] - a["poses"][:, :3, 3]).max() <= 4e-6 and g["kept"] == 0
    assert np.abs(g["poses"][:, :3, :3] - a["poses"][:, :3, :3]).max() <= 2.0 ** -23 + 4 * float(np.abs(g["table"][:, 3:12] - a["table"][:, 3:12]).max())


def test_table_pool_and_poses_against_the_extended_precision_run(solved):
    applied = {n: v for n, v in solved.items() if v[1]["applied"]}
    assert len(applied) >= 3
    for name, (g, a, b) in applied.items():
        assert g["result"].applied == 1 and b["applied"]
        ua, uk = ulps(a["table"], b["table"]), ulps(g["table"], b["table"])
        share_a, share_k = float((ua > 0).mean()), float((uk > 0).mean())
        print("%s: table entries differing from B: A %.4f (max %d ulp), kernel %.4f (max %d ulp)" % (name, share_a, ua.max(), share_k, uk.max()))
        assert share_k <= 2 * share_a + 0.01, (name, share_k, share_a)
        assert uk.max() <= ua.max() + 1, (name, uk.max(), ua.max())
        assert np.array_equal(g["table"][:, [0, 1, 2, 15]], a["table"][:, [0, 1, 2, 15]]) and np.isfinite(g["table"]).all()
        assert g["pool"].shape == b["pool"].shape and np.abs(g["pool"] - b["pool"]).max() <= 4e-6
        gp, bp = g["poses"], b["poses"]
        assert gp.shape == bp.shape and g["kept"] == 0 and b["kept"] == 0
        dt, dr = np.abs(gp[:, :3, 3] - bp[:, :3, 3]).max(), np.abs(gp[:, :3, :3].astype(np.float64) - bp[:, :3, :3]).max()
        dtab = float(np.abs(g["table"][:, 3:12].astype(np.float64) - b["table"][:, 3:12]).max())
        bound = 2.0 ** -23 + 4 * dtab
        print("%s: poses against B: translations %.3e, rotations %.3e (bound %.3e; table rotations differ by %.3e, observed ratio %s)" % (
            name, dt, dr, bound, dtab, "%.2f" % (dr / dtab) if dtab > 0 else "n/a: the tables are equal"))
        assert dt <= 4e-6 and dr <= bound
        for T in gp:
            Rm = T[:3, :3].astype(np.float64)
            assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 2.0 ** -22 and np.array_equal(T[3], [0, 0, 0, 1])
        assert not np.array_equal(gp[:, :3, :3], np.asarray([c for c in SOLVED if c.name == name][0].poses)[:, :3, :3])


def test_two_runs_give_the_same_bytes(solver, solved, capacity):
    for c, first in ((STAGED[2], solved[STAGED[2].name][0]), (capacity[0], capacity[1])):
        again = gpu_run(solver, c)
        assert first["result"].applied == 1
        for key in ("delta0", "poses", "residual0", "weights", "first", "table", "pool"):
            assert again[key].tobytes() == first[key].tobytes(), (c.name, key)
        assert bytes(again["result"]) == bytes(first["result"])


def test_a_solve_that_is_not_applied_leaves_poses_pool_and_table(solver):
    acc, rej = EXITS[4][0], EXITS[2][0]
    before = gpu_run(solver, acc)
    assert before["result"].applied == 1
    after = gpu_run(solver, rej)
    r = after["result"]
    assert (r.applied, r.optimised, r.status) == (0, 1, 0) and after["kept"] == 0
    assert after["table"].tobytes() == before["table"].tobytes() and after["pool"].tobytes() == before["pool"].tobytes()
    assert after["poses"].tobytes() == np.ascontiguousarray(rej.poses, np.float32).tobytes()
    again = gpu_run(solver, acc)  # set_nodes resets what the rejected loop left in the rotations
    for key in ("delta0", "table", "pool", "poses"):
        assert again[key].tobytes() == before[key].tobytes(), key


@pytest.mark.parametrize("case", [deform_cases.staged_cases()[2], deform_cases.staged_cases()[4]], ids=repr)
def test_band_path_of_a_global_object_gives_the_band_objects_bits(dfm, solver, case):
    def run(d):
        d.setNodes(case.nodes)
        d.setLastDeformTime(case.last_deform_time)
        d.clearConstraints()
        for rows, src_time, pin in case.batches:
            d.addConstraints(rows, src_time, pin)
        d.constrain(case.time)
        return dict(result=bytes(d.result()), delta0=d.firstDelta(), table=d.graph(), pool=d.pool(), relative=d.relativeConstraints(),
                    residual0=d.firstResidual())
    band = dfm.Deformation(max_nodes=410, max_constraints=2048)
    want, got = run(band), run(solver)
    band.close()
    solver.setLastDeformTime(0)
    assert got["result"] == want["result"]
    for key in ("delta0", "table", "pool", "relative", "residual0"):
        assert got[key].tobytes() == want[key].tobytes(), key


def test_graph_sampled_from_a_local_object(dfm, solver):
    """dms_deform_sample_from: every 5th node when count / 5 > 4, rotations reset; a smaller local graph leaves the graph as it was"""
    c = EXITS[4][0]
    local = dfm.Deformation(max_nodes=256, max_constraints=16)
    for n, replaced in ((130, True), (24, False), (25, True)):
        big = deform_cases.make_nodes(n, 44)
        local.setNodes(big)
        solver.setNodes(c.nodes)
        solver.sampleFrom(local)
        solver.clearConstraints()
        solver.addConstraints(c.calls[0][1], c.tick, True)
        solver.setPoses(c.pose_times[:0], c.poses[:0])
        solver.constrainGlobal(c.tick)
        want = big[::5] if replaced else c.nodes
        ids, w = solver.vertexWeights()
        gr = R.Graph(want)
        wi, ww = R.weigh_vertex(gr, c.calls[0][1][0, :3], c.tick)
        assert solver.result().nodes == len(want) and np.array_equal(ids[0], wi) and w[0].tobytes() == ww.tobytes(), n
    local.close()


def test_refusals(dfm, solver):
    from densemonoslam_amd import capi

    with pytest.raises(capi.DmsError) as e:
        dfm.GlobalDeformation(max_nodes=411)
    assert e.value.code == -1
    c = STAGED[1]
    load(solver, c)
    with pytest.raises(capi.DmsError) as e:  # made for 16 relative rows; one is in the pool
        solver.addRelativeConstraints(np.tile(c.calls[1][1], (16, 1)))
    assert e.value.code == -4
    with pytest.raises(capi.DmsError) as e:
        solver.setPoses(np.arange(17), np.tile(np.eye(4, dtype=np.float32), (17, 1, 1)))
    assert e.value.code == -4
    with pytest.raises(capi.DmsError) as e:  # the band solve does not take a pool with relative constraints
        solver.constrain(c.tick)
    assert e.value.code == -5
    solver.constrainGlobal(c.tick)  # nothing was added or changed by the refused calls
    want = ref_run(c, "A")
    ids, w = solver.vertexWeights()
    assert np.array_equal(ids, want["ids"]) and w.tobytes() == want["weights"].tobytes()
    assert solver.firstResidual().tobytes() == want["residual0"].tobytes() and len(solver.poses()[0]) == len(c.pose_times)
    band = dfm.Deformation(max_nodes=16, max_constraints=16)
    rows8 = np.ascontiguousarray(c.calls[1][1], np.float32)  # a band object takes neither relative rows nor the global solve
    assert dfm.lib.dms_deform_add_relative_constraints_host(band.h, rows8.ctypes.data_as(dfm._FP), 1, None) == -1
    assert dfm.lib.dms_deform_constrain_global(band.h, 1, None) == -1
    band.close()
