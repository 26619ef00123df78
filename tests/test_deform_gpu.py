"""The deformation-graph solver on the GPU (include/dmslam_deform.h), staged on crafted graphs against the CPU restatement
tests/deform_ref.py: weights, first residual and Jacobian bit for bit; iterations, exit reason and status identical; the first
delta and the node table held against the extended-precision solve by the float64 solve's own error.

Bars (set before any measurement, from the reference's own error):
  e_A    = the largest relative infinity-norm distance of the float64 Cholesky (solver A) from the np.longdouble one (B) over the
           staged inputs; the kernel's first delta may be at most 8 e_A from B (both are backward-stable fp64 factorisations of the
           same matrix and differ in elimination order and blocking only);
  table  : the kernel's float32 node table may differ from B's in at most twice A's share of differing entries plus 1 %, and by at
           most one ulp more than A's largest distance;
  at (512, 768), where B is not run, the kernel's |A delta - g|_inf / |g|_inf (evaluated in np.longdouble) against 8 times A's."""
import ctypes as C

import numpy as np
import pytest

from tests import deform_cases, deform_ref as R

pytestmark = pytest.mark.gpu

STAGED = deform_cases.staged_cases()


@pytest.fixture(scope="module")
def dfm():
    from densemonoslam_amd import capi, deform

    assert capi.device_count() >= 1, "no MI355X visible"
    return deform


@pytest.fixture(scope="module")
def solver(dfm):
    d = dfm.Deformation(max_nodes=512, max_constraints=768)
    yield d
    d.close()


def gpu_run(d, c, relax=False):
    d.setNodes(c.nodes)
    d.setLastDeformTime(c.last_deform_time)
    d.clearConstraints()
    for rows, src_time, pin in c.batches:
        d.addConstraints(rows, src_time, pin)
    d.constrain(c.time, relax)
    r = d.result()
    ids, w = d.vertexWeights()
    out = dict(result=r, ids=ids, weights=w, residual0=d.firstResidual(), jacobian0=d.firstJacobian(), delta0=d.firstDelta(), table=d.graph(),
               pool=d.pool(), relative=d.relativeConstraints(), lastDeformTime=d.lastDeformTime())
    return out


def ref_run(c, solver, relax=False):
    return R.constrain_batches(c.nodes, c.batches, c.time, relax, c.last_deform_time, solver)


@pytest.fixture(scope="module")
def staged(solver):
    """every staged case once: the GPU's run, the restatement with solver A and with solver B"""
    return {c.name: (gpu_run(solver, c), ref_run(c, "A"), ref_run(c, "B")) for c in STAGED}


def relinf(a, b):
    return float(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble)).max() / np.abs(np.asarray(b, np.longdouble)).max())


ulps = deform_cases.ulps


@pytest.mark.parametrize("case", STAGED, ids=repr)
def test_weights_residual_and_jacobian_are_the_restatements_bits(staged, case):
    g, a, _ = staged[case.name]
    assert np.array_equal(g["ids"], a["ids"]) and g["weights"].tobytes() == a["weights"].tobytes()
    assert g["residual0"].tobytes() == a["residual0"].tobytes()
    for got, want, what in zip(g["jacobian0"], a["jacobian0"], ("indptr", "columns", "values")):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), what
    r = g["result"]
    assert r.nodes == len(case.nodes) and r.enabled_nodes == a["enabled"] and r.rows == len(a["residual0"])
    assert r.constraints == len(a["ids"]) and np.float32(r.error_initial).tobytes() == np.float32(a["error0"]).tobytes()
    assert np.float32(r.mean_cons_err_before).tobytes() == np.float32(a["meanConsErr_before"]).tobytes()


@pytest.mark.parametrize("case", STAGED, ids=repr)
def test_loop_takes_the_restatements_path(staged, case):
    g, a, _ = staged[case.name]
    r = g["result"]
    assert (r.status, r.iterations, r.exit_reason, r.optimised, r.applied) == (a["status"], a["iterations"], a["exit"], 1, 1)
    for i in range(r.iterations):  # the same quantities up to the solves' rounding
        assert abs(r.iter_error[i] - float(a["errors"][i])) <= 1e-4 * float(a["errors"][i]), (i, r.iter_error[i], a["errors"][i])
        assert abs(r.iter_delta_norm[i] - a["delta_norms"][i]) <= 1e-6 * a["delta_norms"][i]
    assert r.mean_cons_err_after < r.mean_cons_err_before and a["meanConsErr_after"] < a["meanConsErr_before"]
    assert g["lastDeformTime"] == a["lastDeformTime"] == case.time and r.last_deform_time == case.time


def test_first_delta_is_within_eight_times_the_float64_solves_error(staged):
    e_a = max(relinf(a["delta0"], b["delta0"]) for _, a, b in staged.values())
    report = {name: (relinf(g["delta0"], b["delta0"]), relinf(a["delta0"], b["delta0"])) for name, (g, a, b) in staged.items()}
    print("e_A = %.3e; per case (kernel vs B, A vs B): %s" % (e_a, {k: "%.3e / %.3e" % v for k, v in report.items()}))
    assert 0 < e_a < 1e-6
    for name, (ek, _) in report.items():
        assert ek <= 8 * e_a, (name, ek, e_a)


def test_node_table_against_the_extended_precision_run(staged):
    for name, (g, a, b) in staged.items():
        ua, uk = ulps(a["table"], b["table"]), ulps(g["table"], b["table"])
        share_a, share_k = float((ua > 0).mean()), float((uk > 0).mean())
        print("%s: table entries differing from B: A %.4f (max %d ulp), kernel %.4f (max %d ulp)" % (name, share_a, ua.max(), share_k, uk.max()))
        assert share_k <= 2 * share_a + 0.01, (name, share_k, share_a)
        assert uk.max() <= ua.max() + 1, (name, uk.max(), ua.max())
        assert np.array_equal(g["table"][:, [0, 1, 2, 15]], a["table"][:, [0, 1, 2, 15]])
        assert np.isfinite(g["table"]).all()


@pytest.mark.parametrize("case", STAGED, ids=repr)
def test_pool_and_relative_rows(staged, case):
    g, a, b = staged[case.name]
    assert g["pool"].shape == b["pool"].shape and np.abs(g["pool"] - b["pool"]).max() <= 4e-6
    assert g["relative"].shape == b["relative"].shape == (len(case.rows), 8)
    assert np.array_equal(g["relative"][:, 3:], b["relative"][:, 3:])  # targets and times: copies
    step = 2 if case.pins else 1
    assert np.array_equal(g["relative"][:, :3], g["pool"][::step])  # the deformed sources, in constraint order


def test_two_runs_give_the_same_bits(solver, staged):
    for c in (STAGED[2], STAGED[4]):
        again = gpu_run(solver, c)
        first = staged[c.name][0]
        for key in ("delta0", "table", "pool", "relative", "residual0", "weights"):
            assert again[key].tobytes() == first[key].tobytes(), (c.name, key)
        assert bytes(again["result"]) == bytes(first["result"])


def test_vertex_times_outside_the_nodes_and_on_equal_runs(solver):
    c = STAGED[3]
    pts, times = deform_cases.time_edge_vertices(c.nodes)
    solver.setNodes(c.nodes)
    solver.setLastDeformTime(0)
    solver.clearConstraints()
    for p, t in zip(pts, times):  # one unpinned constraint per vertex, its time given as the source time
        solver.addConstraints(np.concatenate([p, p + 0.01, [1.0]])[None, :], int(t), False)
    solver.constrain(c.time)
    ids, w = solver.vertexWeights()
    g = R.Graph(c.nodes)
    assert len(ids) == len(pts)
    for v in range(len(pts)):
        wi, ww = R.weigh_vertex(g, pts[v], times[v])
        assert np.array_equal(ids[v], wi) and w[v].tobytes() == ww.tobytes(), (v, times[v])


def test_no_enabled_node_applies_the_untouched_graph(solver):
    c = deform_cases.no_enabled_case()
    g, a = gpu_run(solver, c), ref_run(c, "A")
    r = g["result"]
    assert (r.applied, r.optimised, r.status, r.iterations, r.exit_reason, r.enabled_nodes, r.rows) == (1, 1, 0, 0, 5, 0, 0)
    assert r.error == 0 and len(g["delta0"]) == 0 and len(g["residual0"]) == 0
    assert g["table"].tobytes() == a["table"].tobytes() and g["pool"].tobytes() == a["pool"].tobytes()
    assert g["relative"].tobytes() == a["relative"].tobytes()
    assert np.float32(r.mean_cons_err_after).tobytes() == np.float32(a["meanConsErr_after"]).tobytes()


def test_large_graph_residual_of_the_solve(solver):
    """(512, 768): no extended solve; |A delta - g| / |g| in np.longdouble for the kernel's delta against the float64 solve's"""
    c = deform_cases.large_case()
    g, a = gpu_run(solver, c), ref_run(c, "A")
    assert g["residual0"].tobytes() == a["residual0"].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(g["jacobian0"], a["jacobian0"]))
    U, gv, widest = R.normal_equations(*a["jacobian0"], a["residual0"], 512 * 12, np.longdouble)
    assert widest <= R.HALF_BAND
    res = lambda x: float(np.abs(R.band_matvec(U, np.asarray(x, np.longdouble)) - gv).max() / np.abs(gv).max())
    rk, ra = res(g["delta0"]), res(a["delta0"])
    print("(512, 768): |A delta - g|/|g|: kernel %.3e, float64 solve %.3e" % (rk, ra))
    assert rk <= 8 * ra, (rk, ra)
    r = g["result"]
    assert (r.status, r.iterations, r.exit_reason, r.applied) == (a["status"], a["iterations"], a["exit"], 1)


def test_singular_system_resets_the_graph(solver):
    c = deform_cases.singular_case()
    g, a = gpu_run(solver, c), ref_run(c, "A")
    assert np.linalg.cond(R.dense_normal_matrix(*a["jacobian0"], 60)) > 1e15
    r = g["result"]
    assert (r.status, r.applied, r.optimised) == (1, 0, 0) == (a["status"], int(a["applied"]), int(a["optimised"]))
    assert np.isfinite(g["table"]).all() and g["table"].tobytes() == a["table"].tobytes()
    assert len(g["relative"]) == 0 and g["lastDeformTime"] == c.last_deform_time
    # meanConsErr after (:530) and the pool are those of the reset graph, as the restatement computes them
    assert np.float32(r.mean_cons_err_after).tobytes() == np.float32(a["meanConsErr_after"]).tobytes()
    g5 = R.Graph(c.nodes)
    p5 = R.Problem(g5, *R.pool_of(c.rows, c.src_time, c.pins))
    want = np.array([R.vertex_position(g5, p5.src[v], p5.ids[v], p5.w[v]) for v in range(len(p5.src))], np.float32)
    assert g["pool"].tobytes() == want.tobytes()
    # the object goes on working
    again = gpu_run(solver, STAGED[1])
    assert again["result"].applied == 1


def test_capacity_and_relative_constraints_are_refused(dfm):
    from densemonoslam_amd import capi

    d = dfm.Deformation()  # 2048 nodes, the reference's buffer
    rows = np.zeros((2049, 4), np.float32)
    rows[:, 3] = np.arange(2049)
    with pytest.raises(capi.DmsError) as e:
        d.setNodes(rows)
    assert e.value.code == -4
    d.setNodes(rows[:2048])
    with pytest.raises(capi.DmsError) as e:
        d.addConstraints(np.zeros((2049, 7), np.float32), 5, True)
    assert e.value.code == -4
    with pytest.raises(capi.DmsError) as e:
        d.addConstraints(np.zeros((3, 7), np.float32), 5, False, relative=True)
    assert e.value.code == -1
    with pytest.raises(capi.DmsError) as e:
        d.setNodes(rows[:4])
    assert e.value.code == -1
    d.close()


def test_graph_sampled_from_the_map_on_the_device(dfm):
    """dms_deform_sample_model: the strided samples of the map, the first max_nodes of them, stably sorted by init time; a map too
    small for more than 4 samples leaves the graph as it was"""
    from densemonoslam_amd import fusion

    rng = np.random.default_rng(5)
    m = np.zeros(4000, fusion.SURFEL_DTYPE)
    m["pos"][:, :3] = rng.normal(size=(4000, 3))
    m["pos"][:, 3] = 10
    m["col"][:, 2] = rng.integers(1, 40, size=4000)  # init times, with many ties
    m["nrm"][:, 2] = 1
    m["nrm"][:, 3] = 0.01
    gm = fusion.GlobalModel(64, 48, capacity=8192)
    gm.upload(m)
    c = STAGED[1]
    for cap, rate in ((64, 7), (700, 7), (64, 1500)):
        d = dfm.Deformation(max_nodes=cap, max_constraints=16)
        d.setNodes(c.nodes)
        d.sampleModel(gm, rate)
        d.addConstraints(c.rows, 50, True)
        d.constrain(50)
        tab = d.graph()
        s = np.concatenate([m["pos"][::rate, :3], m["col"][::rate, 2:3]], 1)[:cap]
        want = s[np.argsort(s[:, 3], kind="stable")] if len(s) > 4 else c.nodes
        assert tab[:, [0, 1, 2, 15]].tobytes() == want.tobytes(), (cap, rate)
        assert d.result().nodes == len(want)
        d.close()
    assert np.array_equal(gm.downloadMap()["pos"], m["pos"])
