"""The deformation-graph solver without a GPU: the checks the CPU restatement (tests/deform_ref.py) needs for itself, the host build
of densemonoslam_amd/csrc/deform_rows.hpp (g++) against the restatement bit for bit, and the new symbols of the library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import deform_cases, deform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the inputs of tests/test_deform_edges_gpu.py whose path is asserted there: small ones, and the two at capacity
EDGE_CASES = (deform_cases.suffix_cases() + [deform_cases.batch_case()] + deform_cases.boundary_cases() + [deform_cases.hot_node_case(300), deform_cases.relax_case()])
CAPACITY_CASES = [deform_cases.hot_node_case(2048), deform_cases.frame_capacity_case(), deform_cases.capacity_case()]
ALL_CASES = deform_cases.staged_cases() + [deform_cases.singular_case(), deform_cases.no_enabled_case()] + EDGE_CASES + CAPACITY_CASES


def _run(c, solver="A"):
    return R.constrain_batches(c.nodes, c.batches, c.time, c.relax, c.last_deform_time, solver)


@pytest.fixture(scope="module")
def runs():
    return {c.name: _run(c) for c in ALL_CASES}


# ---- the restatement's own checks ---------------------------------------------------------------------------------------------------
def _dense(J, ncols):
    indptr, cols, vals = J
    D = np.zeros((len(indptr) - 1, ncols))
    for i in range(len(indptr) - 1):
        D[i, cols[indptr[i]:indptr[i + 1]]] = vals[indptr[i]:indptr[i + 1]]
    return D


@pytest.mark.parametrize("n,m,keep,pins", [(5, 3, 5, True), (6, 7, 6, True), (12, 9, 7, False)])
def test_analytic_jacobian_equals_central_differences_in_float64(n, m, keep, pins):
    """The residual is at most quadratic in the unknowns, so central differences are exact to rounding."""
    rng = np.random.default_rng(n)
    nodes = deform_cases.make_nodes(n, 20 + n)
    rows = deform_cases.make_rows(nodes, m, 20 + n)
    g = R.Graph(nodes, ft=np.float64)
    g.R += rng.normal(size=g.R.shape) * 0.05  # away from the identity: every product term is live
    g.t += rng.normal(size=g.t.shape) * 0.05
    p = R.Problem(g, *R.pool_of(rows, int(nodes[-1, 3]) + 1, pins))
    g.enabled = np.arange(n) >= n - keep
    assert R.influences(p).any() and (not pins or R.influences(p).all())
    ncols = keep * R.NVAR
    J = _dense(R.jacobian(p), ncols)
    h = 2.0 ** -12
    num = np.zeros_like(J)
    for col in range(ncols):
        node, var = n - keep + col // R.NVAR, col % R.NVAR
        tgt, idx = (g.R, var) if var < 9 else (g.t, var - 9)
        keep_v = tgt[node, idx]
        tgt[node, idx] = keep_v + h
        rp = R.residual(p)
        tgt[node, idx] = keep_v - h
        rm = R.residual(p)
        tgt[node, idx] = keep_v
        num[:, col] = (rp - rm) / (2 * h)
    assert J.shape[0] == len(R.residual(p))
    assert np.abs(J - num).max() <= 1e-10 * max(1.0, np.abs(J).max()), np.abs(J - num).max()


def test_normal_matrix_stays_inside_the_block_band(runs):
    for name, o in runs.items():
        assert o["widest"] <= 19 * 12 + 11 == R.HALF_BAND, (name, o["widest"])
    big = deform_cases.large_case()
    g = R.Graph(big.nodes)
    p = R.Problem(g, *R.pool_of(big.rows, big.src_time, True))
    _, cols, _ = J = R.jacobian(p)
    widest = max(int(cols[b - 1] - cols[a]) for a, b in zip(J[0][:-1], J[0][1:]) if b > a)
    assert widest <= R.HALF_BAND, widest


def test_inputs_stay_clear_of_every_exit_threshold(runs):
    """No test input may sit on a decision boundary of DeformationGraph.cpp:515: each compared pair is at least 1 % apart."""
    seen = set()
    for name, o in runs.items():
        for it, th in enumerate(o["thresholds"]):
            for (a, b), what in zip(th, ("error > lastError", "delta.norm() < 1e-2", "error < 1e-3", "|errorDiff| < 1e-5 error")):
                assert abs(a - b) >= 0.01 * max(abs(a), abs(b)), (name, it + 1, what, a, b)
        seen.add(o["exit"])
    assert {0, 1, 2, 3, 5} <= seen, seen  # the cases reach these exits
    assert len(runs) == len(ALL_CASES) and all(o["status"] == R.STATUS_OK for n, o in runs.items() if n != "n5_c1_singular")


def test_edge_inputs_are_what_their_names_say(runs):
    """Enabled counts, pool sizes and paths of the inputs of tests/test_deform_edges_gpu.py, as the restatement finds them"""
    for c in deform_cases.suffix_cases():
        e = int(c.name.split("suffix")[1].split("_")[0])
        assert runs[c.name]["enabled"] == e and runs[c.name]["iterations"] == (1 if e <= 2 else 3), c
    assert [len(runs[c.name]["ids"]) for c in deform_cases.boundary_cases()] == [63, 64, 65, 255, 256, 257, 256, 258]
    b = deform_cases.batch_case()
    assert [(len(r), p) for r, _, p in b.batches] == [(30, True), (17, False), (1, True), (50, False)]
    assert len({t for _, t, _ in b.batches}) == 2 and len(runs[b.name]["ids"]) == 129 and len(runs[b.name]["relative"]) == 98
    assert list(runs[b.name]["rel_idx"][:6]) == [0, -1, 1, -1, 2, -1] and list(runs[b.name]["rel_idx"][60:79]) == list(range(30, 47)) + [47, -1]
    for m in (300, 2048):
        o = runs["n64_c%d_hot_node" % m]
        counts = np.bincount(o["ids"].ravel(), minlength=64)
        assert len(np.unique(o["ids"], axis=0)) == 2 and counts.max() == m
        assert (o["status"], o["iterations"], R.EXIT_NAMES[o["exit"]]) == (R.STATUS_OK, 1, "small error")
    o = runs["n45_c120_nopins_suffix32_relax"]
    assert (o["enabled"], o["iterations"], R.EXIT_NAMES[o["exit"]], o["lastDeformTime"]) == (45, 3, "small error", 15)
    for name in ("n2047_c768", "n2048_c2048"):
        assert (runs[name]["iterations"], R.EXIT_NAMES[runs[name]["exit"]]) == (1, "small error") and runs[name]["widest"] <= R.HALF_BAND
    o = _run(deform_cases.single_unpinned_case())
    assert o["status"] == R.STATUS_SINGULAR and len(o["ids"]) == 1


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_poisoned_constraint_fails_a_pivot_before_the_last_block(value):
    """One constraint with a NaN / Inf source in the middle of the graph: the first non-positive pivot lies in a block column with
    columns left to factorise, and the verdict is SINGULAR with the graph reset"""
    c = deform_cases.poisoned_case(value)
    with np.errstate(all="ignore"):
        o = _run(c)
    k = o["pivot_failed_at"] // R.NVAR
    assert o["status"] == R.STATUS_SINGULAR and not o["applied"] and o["enabled"] == 64 and 0 < k < o["enabled"] - 1, k
    assert 20 <= k <= 40  # around block 30
    touched = o["ids"][np.isnan(o["weights"]).any(axis=1)]
    assert len(touched) == 1 and k == touched.min()
    assert np.array_equal(o["table"][:, 3:15], np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (64, 1)))
    # the staged singular input, by contrast, fails in its last block
    s = _run(deform_cases.singular_case())
    assert s["pivot_failed_at"] // R.NVAR == s["enabled"] - 1


def test_singular_and_empty_systems(runs):
    o = runs["n5_c1_singular"]
    A = R.dense_normal_matrix(*o["jacobian0"], 60)
    assert np.linalg.cond(A) > 1e15
    assert o["status"] == R.STATUS_SINGULAR and not o["applied"] and not o["optimised"]
    assert np.array_equal(o["table"][:, 3:15], np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (5, 1)))
    e = runs["n24_c40_none_enabled"]
    assert e["applied"] and e["enabled"] == 0 and e["iterations"] == 0 and e["exit"] == 5 and len(e["residual0"]) == 0
    # identity graph: the vertices stay, up to the float rounding of sum w ((v - g) + g)
    assert np.abs(e["pool"] - R.pool_of(deform_cases.no_enabled_case().rows, 0, True)[0]).max() < 1e-6


def test_extended_solve_agrees_with_the_float64_solve(runs):
    c = deform_cases.staged_cases()[2]
    a, b = runs[c.name], _run(c, "B")
    d = np.abs(a["delta0"] - b["delta0"]).max() / np.abs(b["delta0"]).max()
    assert 0 < d < 1e-9, d
    U, gv = b["U0"], b["g0"]
    res = np.abs(R.band_matvec(U, b["delta0"].astype(np.longdouble)) - gv).max() / np.abs(gv).max()
    assert res < 1e-13, res


# ---- the host build of deform_rows.hpp ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("deform_rows") / "libdeform_rows_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "densemonoslam_amd", "csrc"), os.path.join(ROOT, "tests", "deform_rows_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.dr_rows.restype = C.c_int
    lib.dr_sqrt_wreg.restype = C.c_double
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_rows(lib, g, p):
    n, cnt = g.n, len(p.src)
    first = int((~g.enabled).sum())
    nodes = np.ascontiguousarray(np.concatenate([g.pos, g.ftimes[:, None]], 1), np.float32)
    rot, tr = np.ascontiguousarray(g.R, np.float32), np.ascontiguousarray(g.t, np.float32)
    maxrows = 18 * n + 3 * cnt
    resid = np.zeros(maxrows)
    indptr = np.zeros(maxrows + 1, np.int32)
    cols = np.zeros(maxrows * 16, np.int32)
    vals = np.zeros(maxrows * 16)
    src, tgt = np.ascontiguousarray(p.src, np.float32), np.ascontiguousarray(p.target, np.float32)
    ids, w = np.ascontiguousarray(p.ids, np.int32), np.ascontiguousarray(p.w)
    rows = lib.dr_rows(_p(nodes), _p(rot), _p(tr), n, first, _p(src), _p(tgt), _p(ids), _p(w), cnt, _p(resid), _p(indptr), _p(cols), _p(vals))
    nz = indptr[rows]
    return resid[:rows], indptr[:rows + 1], cols[:nz], vals[:nz]


def test_constants_and_neighbours(host):
    assert np.float64(host.dr_sqrt_wreg()).tobytes() == R.SQRT_WREG.tobytes() and R.SQRT_WCON == 10.0
    for n in (5, 6, 7, 9, 24, 130):
        got = np.zeros((n, 4), np.int32)
        host.dr_neighbours(n, _p(got))
        assert got.tolist() == R.neighbours(n), n


@pytest.mark.parametrize("case", deform_cases.staged_cases() + [deform_cases.no_enabled_case()] + EDGE_CASES, ids=repr)
def test_host_build_of_the_row_header_equals_the_restatement_bit_for_bit(host, runs, case):
    o = runs[case.name]
    g = o["graph"]  # the graph AFTER the iterations: rotations and translations away from the identity
    p = R.Problem(g, *R.pool_of_batches(case.batches)[:4])
    nodes = np.ascontiguousarray(case.nodes, np.float32)
    ids, w = np.zeros((len(p.src), 4), np.int32), np.zeros((len(p.src), 4))
    src = np.ascontiguousarray(p.src, np.float32)
    host.dr_weigh(_p(nodes), g.n, _p(src), _p(np.ascontiguousarray(p.vtime)), len(p.src), _p(ids), _p(w))
    assert np.array_equal(ids, p.ids) and w.tobytes() == p.w.tobytes()
    assert np.array_equal(ids, o["ids"]) and w.tobytes() == o["weights"].tobytes()
    for state in ("after", "identity"):
        if state == "identity":
            g = R.Graph(case.nodes)
            g.enabled = g.times > (0 if case.relax else case.last_deform_time)
            p = R.Problem(g, *R.pool_of_batches(case.batches)[:4])
        resid, indptr, cols, vals = _host_rows(host, g, p)
        want_r = R.residual(p)
        wi, wc, wv = R.jacobian(p)
        assert resid.tobytes() == want_r.tobytes(), state
        assert np.array_equal(indptr, wi) and np.array_equal(cols, wc) and vals.tobytes() == wv.tobytes(), state
        if state == "identity":
            assert resid.tobytes() == o["residual0"].tobytes()
        pos = np.zeros((len(p.src), 3), np.float32)
        host.dr_positions(_p(nodes), _p(np.ascontiguousarray(g.R)), _p(np.ascontiguousarray(g.t)), _p(src), _p(ids), _p(w), len(p.src), _p(pos))
        want = np.array([R.vertex_position(g, p.src[v], p.ids[v], p.w[v]) for v in range(len(p.src))], np.float32).reshape(-1, 3)
        assert pos.tobytes() == want.tobytes(), state


def test_vertex_times_outside_and_on_runs_of_node_times(host):
    for n, seed in ((5, 1), (24, 3), (45, 4), (130, 6)):
        nodes = deform_cases.make_nodes(n, seed)
        pts, times = deform_cases.time_edge_vertices(nodes)
        g = R.Graph(nodes)
        ids, w = np.zeros((len(pts), 4), np.int32), np.zeros((len(pts), 4))
        host.dr_weigh(_p(nodes), n, _p(pts), _p(times), len(pts), _p(ids), _p(w))
        for v in range(len(pts)):
            wi, ww = R.weigh_vertex(g, pts[v], times[v])
            assert np.array_equal(ids[v], wi) and w[v].tobytes() == ww.tobytes(), (n, v, times[v])
            assert wi.max() - wi.min() < R.LOOKBACK and abs(ww.sum() - 1) < 1e-12 and (np.diff(wi) > 0).all()
        if n > R.LOOKBACK:  # an old vertex is weighted against the first nodes, extended forwards; a new one against the last
            assert ids[0].max() < R.LOOKBACK and ids[2].min() >= n - R.LOOKBACK


# ---- the library's new symbols ----------------------------------------------------------------------------------------------------------
DEFORM_SYMBOLS = """dms_deform_create dms_deform_destroy dms_deform_set_nodes dms_deform_sample_model dms_deform_add_constraints
dms_deform_clear_constraints dms_deform_constrain dms_deform_get_result dms_deform_graph_device dms_deform_get_relative_constraints
dms_deform_last_deform_time dms_deform_set_last_deform_time dms_deform_get_vertex_weights dms_deform_get_first_residual
dms_deform_get_first_jacobian dms_deform_get_first_delta dms_deform_get_pool""".split()


def test_library_exports_the_deformation_solver():
    from densemonoslam_amd import capi

    text = open(os.path.join(ROOT, "include", "dmslam_deform.h")).read()
    for name in DEFORM_SYMBOLS:
        assert hasattr(capi.lib, name), name
        assert name + "(" in text, name
    # argument checks come before any device access
    assert capi.lib.dms_deform_constrain(None, 0, 0, None) == -1
    assert capi.lib.dms_deform_create(None, 2048, 768) == -1
