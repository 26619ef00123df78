"""The global deformation object without a GPU: the host build of densemonoslam_amd/csrc/deform_rows.hpp (g++, through
tests/deform_global_host.cpp) against the restatement tests/deform_global_ref.py bit for bit, the row envelope, the polar factor against
numpy's SVD, and the promises of tests/deform_global_cases.py.

Band parity: the envelope of an absolute-only input is checked here to be the band (first[i] >= i - 19); that the band path of a global
object gives a band object's bits is checked on the GPU (tests/test_deform_global_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import deform_cases, deform_global_cases as GC, deform_global_ref as G, deform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = GC.staged_cases()
EXITS = GC.exit_cases()
SOLVED = STAGED + [c for c, _, _ in EXITS]


@pytest.fixture(scope="module")
def runs():
    return {c.name: G.constrain_global(c.nodes, c.calls, c.pose_times, c.poses) for c in SOLVED}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("deform_global") / "libdeform_global_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "densemonoslam_amd", "csrc"), os.path.join(ROOT, "tests", "deform_global_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.drg_rows.restype = lib.drg_poses.restype = lib.drg_polar.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_rows(lib, g, p):
    n, cnt = g.n, len(p.src)
    e0 = int((~g.enabled).sum())
    nodes = np.ascontiguousarray(np.concatenate([g.pos, g.ftimes[:, None]], 1), np.float32)
    rot, tr = np.ascontiguousarray(g.R, np.float32), np.ascontiguousarray(g.t, np.float32)
    maxrows = 18 * n + 3 * cnt
    resid, indptr = np.zeros(maxrows), np.zeros(maxrows + 1, np.int32)
    cols, vals = np.zeros(maxrows * 32, np.int32), np.zeros(maxrows * 32)
    first = np.zeros(n, np.int32)
    src, tgt = np.ascontiguousarray(p.src, np.float32), np.ascontiguousarray(p.target, np.float32)
    ids, w, kind = np.ascontiguousarray(p.ids, np.int32), np.ascontiguousarray(p.w), np.ascontiguousarray(p.kind, np.int32)
    rows = lib.drg_rows(_p(nodes), _p(rot), _p(tr), n, e0, _p(src), _p(tgt), _p(kind), _p(ids), _p(w), cnt, _p(resid), _p(indptr), _p(cols),
                        _p(vals), _p(first))
    nz = indptr[rows]
    return resid[:rows], indptr[:rows + 1], cols[:nz], vals[:nz], first[:n - e0]


def _check_rows(host, g, p):
    resid, indptr, cols, vals, first = _host_rows(host, g, p)
    wi, wc, wv = G.jacobian(p)
    assert resid.tobytes() == G.residual(p).tobytes()
    assert np.array_equal(indptr, wi) and np.array_equal(cols, wc) and vals.tobytes() == wv.tobytes()
    assert np.array_equal(first, G.envelope(wi, wc, int(g.enabled.sum())))
    return first


@pytest.mark.parametrize("case", SOLVED, ids=repr)
def test_host_build_equals_the_restatement_bit_for_bit(host, runs, case):
    """node ids and weights (through the rows), every residual entry, every Jacobian value and column, the envelope: on the graph after
    the iterations and on the identity graph"""
    o = runs[case.name]
    _check_rows(host, o["graph"], o["problem"])
    g = R.Graph(case.nodes)
    g.enabled = g.times > 0
    _check_rows(host, g, G.Problem(g, *G.pool_of_calls(case.calls)))


def test_capacity_case_rows_and_envelope(host):
    """(e) on the identity graph: 410 nodes, 4096 + 16 pool vertices; the last nodes' rows reach the first blocks"""
    c = GC.case_e()
    g = R.Graph(c.nodes)
    g.enabled = g.times > 0
    p = G.Problem(g, *G.pool_of_calls(c.calls))
    assert (g.n, c.absolute_rows, c.relative_rows, len(p.src)) == (410, 2048, 8, 4112)
    first = _check_rows(host, g, p)
    assert (first[-20:] < 20).sum() >= 4 and (np.arange(410) - first > 19).sum() <= 4 * 8 and first[200] >= 181


@pytest.mark.parametrize("case", deform_cases.staged_cases() + [deform_cases.dense_suffix_case(22, 23)], ids=repr)
def test_envelope_of_an_absolute_only_input_is_the_band(host, case):
    g = R.Graph(case.nodes)
    g.enabled = g.times > case.last_deform_time
    p = G.Problem(g, *G.pool_of_calls([("abs", rows, t, pin) for rows, t, pin in case.batches]))
    first = _check_rows(host, g, p)
    i = np.arange(len(first))
    assert (first >= np.maximum(0, i - 19)).all() and (first <= i).all()


@pytest.mark.parametrize("case", SOLVED, ids=repr)
def test_pose_weights_and_poses_equal_the_restatement_bit_for_bit(host, runs, case):
    """setPosesSeq and applyGraphToPoses with polar "A" on the graph after the iterations, whether or not the solve was applied"""
    g = runs[case.name]["graph"]
    want_ids, want_w = G.pose_weights(g, case.pose_times, case.poses)
    want, kept = G.apply_poses(g, want_ids, want_w, case.poses, "A")
    nodes = np.ascontiguousarray(np.concatenate([g.pos, g.ftimes[:, None]], 1), np.float32)
    poses = np.ascontiguousarray(case.poses, np.float32).copy()
    ids, w = np.zeros((len(poses), 4), np.int32), np.zeros((len(poses), 4))
    got_kept = host.drg_poses(_p(nodes), _p(np.ascontiguousarray(g.R)), _p(np.ascontiguousarray(g.t)), g.n, _p(np.ascontiguousarray(case.pose_times)),
                              _p(poses), len(poses), _p(ids), _p(w))
    assert np.array_equal(ids, want_ids) and w.tobytes() == want_w.tobytes()
    assert poses.tobytes() == want.tobytes() and got_kept == kept == 0
    # (g) the times lie before, between and after the node times and on an exact tie
    t = case.nodes[:, 3].astype(np.int64)
    pt = case.pose_times
    assert (pt < t[0]).any() and (pt > t[-1]).any() and np.isin(pt, t).any()
    has_gap = bool((np.diff(t) >= 2).any())  # (the five-node graph's times leave none)
    assert has_gap == (len(t) > 5) and (not has_gap or any((t < x).any() and (t > x).any() and x not in t for x in pt))


def _test_matrices():
    rng = np.random.default_rng(77)
    out = []
    for i in range(200):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if i % 4 == 0:
            m = q + rng.normal(size=(3, 3)) * 1e-3          # a rotation sum of nearly equal rotations (det +-1)
        elif i % 4 == 1:
            m = q @ np.diag(rng.uniform(0.3, 1.5, 3))       # sheared
        elif i % 4 == 2:
            m = np.diag(rng.uniform(0.5, 1.0, 3)) @ q @ np.diag([1.0, 1.0, 10.0 ** -rng.uniform(2, 5)])  # det down to ~1e-5 > 2^-20
        else:
            m = rng.uniform(-1, 1, size=(3, 3))
        out.append(m.astype(np.float32))
    return out


def test_polar_factor_against_the_float64_svd(host):
    """Both are float64-accurate factors with entries in [-1, 1], rounded once to float32: at most 2^-23 apart per entry"""
    worst, checked = 0.0, 0
    for m in _test_matrices():
        a, s = G.polar_newton(m), G.polar_svd(m)
        out = np.zeros(9, np.float32)
        ok = host.drg_polar(_p(np.ascontiguousarray(m)), _p(out))
        assert (a is None) == (s is None) == (not ok)
        if a is None:
            continue
        assert out.tobytes() == a.tobytes()
        worst = max(worst, float(np.abs(a.astype(np.float64) - s.astype(np.float64)).max()))
        assert np.abs(a.astype(np.float64).T @ a.astype(np.float64) - np.eye(3)).max() <= 2.0 ** -22
        checked += 1
    print("polar A against SVD over %d matrices: max |difference| = %.3e" % (checked, worst))
    assert checked >= 150 and worst <= 2.0 ** -23
    keep = [np.zeros((3, 3), np.float32), np.diag([1, 1, 2.0 ** -21]).astype(np.float32), np.full((3, 3), np.nan, np.float32),
            np.diag([1, np.inf, 1]).astype(np.float32)]
    for m in keep:  # not finite, or |det| < 2^-20: the old rotation is kept
        out = np.full(9, 7, np.float32)
        assert G.polar_newton(m) is None and G.polar_svd(m) is None and host.drg_polar(_p(np.ascontiguousarray(m)), _p(out)) == 0 and (out == 7).all()
    refl = np.diag([1, 1, -1]).astype(np.float32)  # a reflection has the factor U V^T = itself
    assert np.array_equal(G.polar_newton(refl), refl)


# ---- the promises of the case file -----------------------------------------------------------------------------------------------------
def test_each_exit_input_takes_the_exit_it_is_named_for(runs):
    met, large, by_error, by_cons, accepted = [(runs[c.name], want_exit, want_applied) for c, want_exit, want_applied in EXITS]
    for o, want_exit, want_applied in (met, large, by_error, by_cons, accepted):
        assert o["status"] == R.STATUS_OK and o["applied"] == want_applied and (want_exit is None or o["exit"] == want_exit)
    o = met[0]
    assert (o["optimised"], o["iterations"], o["exit"]) == (False, 0, 6) and o["meanConsErr_before"] < 0.06 * 0.99
    o = large[0]
    assert (o["optimised"], o["iterations"], o["exit"]) == (True, 1, 7) and o["errors"][0] > 10 * 1.01
    o = by_error[0]
    assert o["optimised"] and o["error"] >= 0.12 * 1.01
    o = by_cons[0]
    assert o["optimised"] and o["error"] < 0.12 * 0.99 and o["meanConsErr_after"] >= 0.0003 * 1.01
    o = accepted[0]
    assert o["optimised"] and o["error"] < 0.12 * 0.99 and o["meanConsErr_after"] < 0.0003 * 0.99 and o["iterations"] >= 1


def test_inputs_stay_clear_of_every_threshold(runs):
    """No input sits on a decision boundary: the pairs compared by :465 and Deformation.cpp:165 are 1 % apart, those of :515 / :516 0.05 %
    (the GPU test lets the kernel's per-iteration errors differ from the restatement's by 1e-4, the solves' rounding: five times less;
    a converged third iteration lowers the error by little, so 1 % cannot be asked there)."""
    for name, o in runs.items():
        assert abs(float(o["meanConsErr_before"]) - 0.06) >= 0.01 * 0.06, name
        for it, th in enumerate(o["thresholds"]):
            for a, b in th:
                assert abs(a - b) >= 0.0005 * max(abs(a), abs(b)), (name, it + 1, a, b)
        if o["optimised"]:
            assert abs(float(o["error"]) - 0.12) >= 0.0012 and abs(float(o["meanConsErr_after"]) - 0.0003) >= 0.000003, name
    assert {0, 6, 7} <= {o["exit"] for o in runs.values()}


def test_staged_cases_hold_what_they_are_named_for(runs):
    a, b, c, d = [runs[x.name] for x in STAGED]
    # (a) source and target share nodes: fewer merged entries than eight, and an entry that addTo combined
    pa = a["problem"]
    rel = [v for v in range(len(pa.src)) if pa.kind[v] == G.REL_SRC]
    assert len(rel) == 1 and len(pa.mid[rel[0]]) < 8 and set(pa.ids[rel[0]]) & set(pa.ids[rel[0] + 1])
    # (b) the last node's row begins at block 0, 23 blocks out
    assert b["enabled"] == 24 and b["first"][23] == 0 and (b["first"][5:20] >= np.arange(5, 20) - 19).all()
    # (c) five relative rows; a tall row that begins left of an earlier tall row's first; a narrow row behind a tall one
    f = c["first"]
    i = np.arange(64)
    tall = np.nonzero(i - f > 19)[0]
    assert STAGED[2].relative_rows == 5 and len(tall) >= 8
    assert any(f[t2] < f[t1] for k, t1 in enumerate(tall) for t2 in tall[k + 1:])
    assert any(i2 > tall[0] and i2 - f[i2] <= 19 for i2 in range(64))
    assert c["applied"] and STAGED[2].absolute_rows == 48
    # (d) a disabled prefix; one relative row with every source node disabled and a target node enabled, one with all eight disabled
    pd, g = d["problem"], d["graph"]
    assert (~g.enabled).sum() == GC.DISABLED_D and d["enabled"] == 64 - GC.DISABLED_D
    rel = [v for v in range(len(pd.src)) if pd.kind[v] == G.REL_SRC]
    src_en = [bool(g.enabled[pd.ids[v]].any()) for v in rel]
    tgt_en = [bool(g.enabled[pd.ids[v + 1]].any()) for v in rel]
    assert (False, True) in zip(src_en, tgt_en) and (False, False) in zip(src_en, tgt_en) and (True, True) in zip(src_en, tgt_en)
    assert len(pd.rows()) == int((pd.kind != G.REL_TGT).sum()) - 1 - sum(1 for v in range(len(pd.src)) if pd.kind[v] == G.ABS and not g.enabled[pd.ids[v]].any())
    assert d["applied"]


def test_extended_solve_agrees_with_the_float64_solve():
    c = STAGED[2]
    a = G.constrain_global(c.nodes, c.calls, c.pose_times, c.poses, "A")
    b = G.constrain_global(c.nodes, c.calls, c.pose_times, c.poses, "B")
    d = np.abs(a["delta0"] - b["delta0"]).max() / np.abs(b["delta0"]).max()
    assert 0 < d < 1e-9, d
    res = np.abs(b["A0"] @ b["delta0"].astype(np.longdouble) - b["g0"]).max() / np.abs(b["g0"]).max()
    assert res < 1e-13, res


# ---- the library's new symbols ----------------------------------------------------------------------------------------------------------
GLOBAL_SYMBOLS = """dms_deform_create_global dms_deform_sample_from dms_deform_add_relative_constraints
dms_deform_add_relative_constraints_host dms_deform_set_poses dms_deform_get_poses dms_deform_constrain_global
dms_deform_get_kept_rotations dms_deform_get_pose_weights dms_deform_get_envelope""".split()


def test_library_exports_the_global_deformation_object():
    from densemonoslam_amd import capi

    text = open(os.path.join(ROOT, "include", "dmslam_deform.h")).read()
    for name in GLOBAL_SYMBOLS:
        assert hasattr(capi.lib, name), name
        assert name + "(" in text, name
    assert capi.lib.dms_deform_create_global(None, 410, 768, 64, 64) == -1
    assert capi.lib.dms_deform_constrain_global(None, 0, None) == -1
