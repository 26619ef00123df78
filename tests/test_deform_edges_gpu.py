"""The deformation-graph solver at the edges tests/test_deform_gpu.py stops short of: its capacity (2048 nodes, a pool of 4096) and the
sizes at which the one-block setup wraps, enabled suffixes of 1 .. 63 nodes around the 19-block window, constraints added in several
calls with mixed pin flags, pools at the wave and chunk boundaries of the assembly's compaction, every source on one node, relaxGraph,
one object reused from a large solve to small ones, and a NaN / Inf that makes a pivot fail in the middle of the factorisation.

The yardstick is the CPU restatement tests/deform_ref.py (float64 solve A, np.longdouble solve B) and the bars are those of
tests/test_deform_gpu.py, unchanged: weights, node ids, first residual, first Jacobian, error_initial and meanConsErr before bit for
bit; status, iterations, exit reason, optimised, applied identical; first delta within 8 e_A of B (e_A = A's distance from B over the
inputs of the group compared); node table: share of entries differing from B at most twice A's plus 1 %, largest ulp distance at most
A's plus one, position and time columns equal; pool within 4e-6 of B's; relative rows' columns 3: copies.  Every input whose path is
asserted is 1 % clear of every exit threshold (tests/test_deform_cpu.py checks that without a GPU).

The restatement at capacity takes seconds (A about 10 s, B about 20 s at 2048 nodes): each input is solved once, behind `runs`."""
import numpy as np
import pytest

from tests import deform_cases, deform_ref as R
from tests.test_deform_gpu import gpu_run, ref_run, relinf, ulps

pytestmark = pytest.mark.gpu

CAPACITY = deform_cases.capacity_case()
FRAME_CAPACITY = deform_cases.frame_capacity_case()
WRAPS = deform_cases.wrap_cases()
SUFFIXES = deform_cases.suffix_cases()
BATCHES = deform_cases.batch_case()
BOUNDARIES = deform_cases.boundary_cases()
HOT = [deform_cases.hot_node_case(300), deform_cases.hot_node_case(2048)]
RELAX = deform_cases.relax_case()
POISONED = [deform_cases.poisoned_case(np.nan), deform_cases.poisoned_case(np.inf)]


@pytest.fixture(scope="module")
def dfm():
    from densemonoslam_amd import capi, deform

    assert capi.device_count() >= 1, "no MI355X visible"
    return deform


@pytest.fixture(scope="module")
def solver(dfm):
    d = dfm.Deformation()  # the defaults: 2048 nodes, 2048 constraints
    yield d
    d.close()


@pytest.fixture(scope="module")
def runs(solver):
    """(the GPU's run, the restatement with solver A, with solver B or None) of a case, each computed once"""
    done = {}

    def get(c, extended=True):
        if c.name not in done:
            done[c.name] = (gpu_run(solver, c, c.relax), ref_run(c, "A", c.relax), ref_run(c, "B", c.relax) if extended else None)
        return done[c.name]

    return get


def fresh_run(dfm, c):
    d = dfm.Deformation()
    try:
        return gpu_run(d, c, c.relax)
    finally:
        d.close()


# ---- the bars of tests/test_deform_gpu.py --------------------------------------------------------------------------------------------
def same_bits(g, a, case):
    assert np.array_equal(g["ids"], a["ids"]) and g["weights"].tobytes() == a["weights"].tobytes(), case
    assert g["residual0"].tobytes() == a["residual0"].tobytes(), case
    for got, want, what in zip(g["jacobian0"], a["jacobian0"], ("indptr", "columns", "values")):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (case, what)
    r = g["result"]
    assert r.nodes == len(case.nodes) and r.enabled_nodes == a["enabled"] and r.rows == len(a["residual0"]), case
    assert r.constraints == len(a["ids"]) and np.float32(r.error_initial).tobytes() == np.float32(a["error0"]).tobytes(), case
    assert np.float32(r.mean_cons_err_before).tobytes() == np.float32(a["meanConsErr_before"]).tobytes(), case


def same_path(g, a, case, b=None):
    """The path is A's.  The per-iteration error and delta norm are held against the extended run B where there is one, by the staged
    tests' tolerances (1e-4, 1e-6) or 8 times A's own distance from B, whichever is larger: on the inputs without pins a later
    iteration starts from a float32 graph in which A and B already round a fifth of the entries differently (A is 2.5e-3 from B in the
    last error of n45_pool64_nopins and 5.4e-6 in its delta norm; the kernel 0 and 1.4e-9)."""
    r = g["result"]
    assert (r.status, r.iterations, r.exit_reason, r.optimised, r.applied) == (a["status"], a["iterations"], a["exit"], 1, 1), case
    ref = a if b is None else b
    assert b is None or (b["iterations"], b["exit"]) == (a["iterations"], a["exit"]), case
    for i in range(r.iterations):
        e, ea, dn, dna = float(ref["errors"][i]), float(a["errors"][i]), float(ref["delta_norms"][i]), float(a["delta_norms"][i])
        assert abs(r.iter_error[i] - e) <= max(1e-4 * e, 8 * abs(ea - e)), (case, i, r.iter_error[i], e, ea)
        assert abs(r.iter_delta_norm[i] - dn) <= max(1e-6 * dn, 8 * abs(dna - dn)), (case, i, r.iter_delta_norm[i], dn, dna)
    assert r.mean_cons_err_after < r.mean_cons_err_before and a["meanConsErr_after"] < a["meanConsErr_before"], case


def delta_within_bar(group):
    """group: {name: (g, a, b)}; e_A over the group, every kernel delta within 8 e_A of B's"""
    e_a = max(relinf(a["delta0"], b["delta0"]) for _, a, b in group.values())
    report = {name: (relinf(g["delta0"], b["delta0"]), relinf(a["delta0"], b["delta0"])) for name, (g, a, b) in group.items()}
    print("e_A = %.3e; per case (kernel vs B, A vs B): %s" % (e_a, {k: "%.3e / %.3e" % v for k, v in report.items()}))
    assert 0 < e_a < 1e-6
    for name, (ek, _) in report.items():
        assert ek <= 8 * e_a, (name, ek, e_a)


def table_within_bar(g, a, b, name):
    ua, uk = ulps(a["table"], b["table"]), ulps(g["table"], b["table"])
    share_a, share_k = float((ua > 0).mean()), float((uk > 0).mean())
    print("%s: table entries differing from B: A %.4f (max %d ulp), kernel %.4f (max %d ulp)" % (name, share_a, ua.max(), share_k, uk.max()))
    assert share_k <= 2 * share_a + 0.01, (name, share_k, share_a)
    assert uk.max() <= ua.max() + 1, (name, uk.max(), ua.max())
    assert np.array_equal(g["table"][:, [0, 1, 2, 15]], a["table"][:, [0, 1, 2, 15]])
    assert np.isfinite(g["table"]).all()


def pool_and_relative(g, b, case):
    assert g["pool"].shape == b["pool"].shape and np.abs(g["pool"] - b["pool"]).max() <= 4e-6, case
    assert g["relative"].shape == b["relative"].shape == (len(case.rows), 8), case
    assert np.array_equal(g["relative"][:, 3:], b["relative"][:, 3:]), case  # targets and times: copies
    assert np.array_equal(g["relative"][:, :3], g["pool"][b["rel_idx"] >= 0]), case  # the deformed sources, in constraint order


def staged_comparison(group, cases):
    for c in cases:
        g, a, b = group[c.name]
        same_bits(g, a, c)
        same_path(g, a, c, b)
        table_within_bar(g, a, b, c.name)
        pool_and_relative(g, b, c)
        want_ldt = c.last_deform_time if c.relax else c.time
        assert g["lastDeformTime"] == a["lastDeformTime"] == want_ldt and g["result"].last_deform_time == want_ldt, c
    delta_within_bar(group)


# ---- 1. capacity ----------------------------------------------------------------------------------------------------------------------
def test_capacity_2048_nodes_pool_of_4096(runs):
    c = CAPACITY
    g, a, b = runs(c)
    assert len(a["ids"]) == 4096 and a["widest"] <= R.HALF_BAND
    staged_comparison({c.name: (g, a, b)}, [c])


def test_frame_capacity_2047_nodes(runs):
    """(2047, 768): bits and path; |A delta - g|_inf / |g|_inf in np.longdouble for the kernel's delta against 8 times the float64 solve's"""
    c = FRAME_CAPACITY
    g, a, _ = runs(c, extended=False)
    same_bits(g, a, c)
    same_path(g, a, c)
    U, gv, widest = R.normal_equations(*a["jacobian0"], a["residual0"], 2047 * 12, np.longdouble)
    assert widest <= R.HALF_BAND
    res = lambda x: float(np.abs(R.band_matvec(U, np.asarray(x, np.longdouble)) - gv).max() / np.abs(gv).max())
    rk, ra = res(g["delta0"]), res(a["delta0"])
    print("(2047, 768): |A delta - g|/|g|: kernel %.3e, float64 solve %.3e" % (rk, ra))
    assert rk <= 8 * ra, (rk, ra)


@pytest.mark.parametrize("case", WRAPS, ids=repr)
def test_rows_at_the_wrap_points_of_the_setup(solver, case):
    """Weights, first residual and Jacobian where the setup's strided count and its scan over 4 N + P items wrap; the restatement's
    side without its solve"""
    g = gpu_run(solver, case)
    graph = R.Graph(case.nodes)
    p = R.Problem(graph, *R.pool_of(case.rows, case.src_time, case.pins))
    graph.enabled = graph.times > case.last_deform_time
    want_r, want_j = R.residual(p), R.jacobian(p)
    assert np.array_equal(g["ids"], p.ids) and g["weights"].tobytes() == p.w.tobytes()
    assert g["residual0"].tobytes() == want_r.tobytes()
    for got, want, what in zip(g["jacobian0"], want_j, ("indptr", "columns", "values")):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), what
    r = g["result"]
    assert (r.nodes, r.enabled_nodes, r.rows) == (len(case.nodes), int(graph.enabled.sum()), len(want_r))
    assert 0 < r.enabled_nodes and (case.last_deform_time == 0) == (r.enabled_nodes == r.nodes)


def test_graph_sampled_from_the_map_at_capacity(dfm):
    """sampleModel into 2048 nodes: 2667 strided samples cut to the first 2048, and exactly 2000 with nothing cut, stably sorted by time"""
    from densemonoslam_amd import fusion

    rng = np.random.default_rng(6)
    m = np.zeros(8000, fusion.SURFEL_DTYPE)
    m["pos"][:, :3] = rng.normal(size=(8000, 3))
    m["pos"][:, 3] = 10
    m["col"][:, 2] = rng.integers(1, 40, size=8000)  # init times, with many ties
    m["nrm"][:, 2] = 1
    m["nrm"][:, 3] = 0.01
    gm = fusion.GlobalModel(64, 48, capacity=8192)
    gm.upload(m)
    c = deform_cases.staged_cases()[1]
    for rate, samples in ((3, 2667), (4, 2000)):
        d = dfm.Deformation()
        d.setNodes(c.nodes)
        d.sampleModel(gm, rate)
        d.addConstraints(c.rows, 50, True)
        d.constrain(50)
        tab = d.graph()
        s = np.concatenate([m["pos"][::rate, :3], m["col"][::rate, 2:3]], 1)
        assert len(s) == samples
        s = s[:2048]
        want = s[np.argsort(s[:, 3], kind="stable")]
        assert d.result().nodes == len(want) == min(samples, 2048)
        assert tab[:, [0, 1, 2, 15]].tobytes() == want.tobytes(), rate
        d.close()
    assert np.array_equal(gm.downloadMap()["pos"], m["pos"])


# ---- 2. the enabled suffix ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def suffix_runs(runs):
    return {c.name: runs(c) for c in SUFFIXES}


def test_short_enabled_suffixes_full_comparison(suffix_runs):
    staged_comparison(suffix_runs, SUFFIXES)


@pytest.mark.parametrize("case", SUFFIXES, ids=repr)
def test_short_enabled_suffix_leaves_the_disabled_nodes_untouched(suffix_runs, case):
    g, a, b = suffix_runs[case.name]
    e = int(case.name.split("suffix")[1].split("_")[0])
    assert g["result"].enabled_nodes == a["enabled"] == e
    same_bits(g, a, case)
    same_path(g, a, case, b)
    untouched = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (64 - e, 1))
    assert g["table"][:64 - e, 3:15].tobytes() == untouched.tobytes() == a["table"][:64 - e, 3:15].tobytes()
    assert not np.array_equal(g["table"][64 - e:, 3:15], np.tile(untouched[:1], (e, 1)))  # the enabled ones moved
    assert g["lastDeformTime"] == case.time


# ---- 3. batches, boundaries, one hot node -----------------------------------------------------------------------------------------------
def test_constraints_added_in_four_calls_with_mixed_pins(runs):
    c = BATCHES
    g, a, b = runs(c)
    assert [len(rows) for rows, _, _ in c.batches] == [30, 17, 1, 50] and len({t for _, t, _ in c.batches}) == 2
    assert len(a["ids"]) == 2 * 30 + 17 + 2 * 1 + 50
    staged_comparison({c.name: (g, a, b)}, [c])
    rel = g["relative"]
    assert len(rel) == 98
    # call order: each row's deformed source is the pool vertex that the restatement's numbering names, its times those of its call
    for v, k in enumerate(a["rel_idx"]):
        if k >= 0:
            assert rel[k, :3].tobytes() == g["pool"][v].tobytes(), (v, k)
    want_src_time = np.concatenate([np.full(len(rows), t, np.float32) for rows, t, _ in c.batches])
    assert np.array_equal(rel[:, 6], want_src_time) and np.array_equal(rel[:, 7], c.rows[:, 6]) and np.array_equal(rel[:, 3:6], c.rows[:, 3:6])
    assert rel.tobytes() != np.zeros_like(rel).tobytes() and np.isfinite(rel).all()


def test_pools_at_wave_and_chunk_boundaries(runs):
    group = {c.name: runs(c) for c in BOUNDARIES}
    assert [len(a["ids"]) for _, a, _ in group.values()] == [63, 64, 65, 255, 256, 257, 256, 258]
    staged_comparison(group, BOUNDARIES)


def test_every_source_on_one_node(runs):
    group = {c.name: runs(c) for c in HOT}
    for c in HOT:
        a = group[c.name][1]
        m = len(c.rows)
        counts = np.bincount(a["ids"].ravel(), minlength=64)
        assert len(np.unique(a["ids"], axis=0)) == 2 and counts.max() == m and (counts == m).sum() == 8
        assert (a["status"], a["iterations"], R.EXIT_NAMES[a["exit"]]) == (R.STATUS_OK, 1, "small error")
    staged_comparison(group, HOT)


def test_single_unpinned_constraint_is_singular(runs):
    """P = 1 on 24 nodes: the restatement's verdict is SINGULAR (one point cannot hold 24 nodes), and the kernel's must be the same"""
    c = deform_cases.single_unpinned_case()
    g, a, _ = runs(c, extended=False)
    assert a["status"] == R.STATUS_SINGULAR and not a["applied"]
    same_bits(g, a, c)
    r = g["result"]
    assert (r.status, r.applied, r.optimised, r.iterations, r.constraints) == (a["status"], 0, 0, a["iterations"], 1)
    assert g["table"].tobytes() == a["table"].tobytes() and len(g["relative"]) == 0 and g["lastDeformTime"] == c.last_deform_time
    assert np.float32(r.mean_cons_err_after).tobytes() == np.float32(a["meanConsErr_after"]).tobytes()


# ---- 4. relaxGraph ----------------------------------------------------------------------------------------------------------------------
def test_relax_graph_enables_every_node_and_keeps_last_deform_time(solver):
    c = RELAX
    g, a, b = gpu_run(solver, c, True), ref_run(c, "A", True), ref_run(c, "B", True)
    assert (a["enabled"], a["iterations"], R.EXIT_NAMES[a["exit"]], a["lastDeformTime"]) == (45, 3, "small error", c.last_deform_time)
    assert g["result"].enabled_nodes == 45
    staged_comparison({c.name: (g, a, b)}, [c])
    assert solver.lastDeformTime() == c.last_deform_time
    # the same input without relax on the same object: the suffix again
    plain = deform_cases.staged_cases()[4]
    g2, a2 = gpu_run(solver, plain, False), ref_run(plain, "A", False)
    assert g2["result"].enabled_nodes == a2["enabled"] == 32
    same_bits(g2, a2, plain)
    same_path(g2, a2, plain)
    assert g2["lastDeformTime"] == plain.time


# ---- 5. reuse -----------------------------------------------------------------------------------------------------------------------------
def same_as_fresh(got, want, what):
    for key in ("ids", "weights", "residual0", "delta0", "table", "pool", "relative"):
        assert got[key].tobytes() == want[key].tobytes(), (what, key)
    for x, y in zip(got["jacobian0"], want["jacobian0"]):
        assert x.tobytes() == y.tobytes(), (what, "jacobian0")
    assert bytes(got["result"]) == bytes(want["result"]) and got["lastDeformTime"] == want["lastDeformTime"], what


def test_one_object_from_a_large_solve_to_small_ones_equals_fresh_objects(dfm):
    staged = deform_cases.staged_cases()
    order = [CAPACITY, staged[0], deform_cases.singular_case(), staged[1], deform_cases.no_enabled_case(), staged[2], deform_cases.suffix_case(1)]
    d = dfm.Deformation()
    for c in order:
        same_as_fresh(gpu_run(d, c), fresh_run(dfm, c), c.name)
    d.close()


# ---- 6. a pivot that fails early, and NaN -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POISONED, ids=repr)
def test_poisoned_constraint_fails_a_pivot_mid_factorisation_and_resets(dfm, case):
    with np.errstate(all="ignore"):
        a = ref_run(case, "A")
    assert a["status"] == R.STATUS_SINGULAR and 0 < a["pivot_failed_at"] // R.NVAR < a["enabled"] - 1
    d = dfm.Deformation()
    g = gpu_run(d, case)
    r = g["result"]
    assert (r.status, r.applied, r.optimised, r.iterations) == (a["status"], int(a["applied"]), int(a["optimised"]), a["iterations"]) == (1, 0, 0, 1)
    assert (r.nodes, r.enabled_nodes, r.rows, r.constraints) == (64, a["enabled"], len(a["residual0"]), len(a["ids"]))
    # the order rules put a NaN / Inf distance in the same place on both sides; weights are equal where they are numbers
    assert np.array_equal(g["ids"], a["ids"]) and np.array_equal(np.isnan(g["weights"]), np.isnan(a["weights"]))
    clean = ~np.isnan(a["weights"]).any(axis=1)
    assert clean.sum() == len(clean) - 1 and g["weights"][clean].tobytes() == a["weights"][clean].tobytes()
    assert np.isfinite(g["table"]).all() and g["table"].tobytes() == a["table"].tobytes()
    assert len(g["relative"]) == 0 and g["lastDeformTime"] == case.last_deform_time == r.last_deform_time
    assert np.isnan(r.mean_cons_err_after) and np.isnan(a["meanConsErr_after"])
    # the object goes on: the next solve has a fresh object's bits
    nxt = deform_cases.staged_cases()[2]
    same_as_fresh(gpu_run(d, nxt), fresh_run(dfm, nxt), case.name)
    d.close()
