"""The frame step closes its local loops itself (dms_fusion_set_loop_solver): on the stream of
test_two_phase_frame_step_with_deformation, two frames longer, one-call frames with the solver on against the two-phase path driven
by the test with a stand-alone solver, against the oracle pipeline given the GPU's table, and against the CPU restatement of the solve.

With the solver always on, every frame after the first closing one closes again, lastDeformTime follows the ticks and no node is ever
newer than it.  So the solver is switched off for the two frames after the first closure (the public switch; the two-phase side passes
no graph there): their loops are dropped, they fuse new surfels, and the next closing frame solves without pins on the suffix of nodes
sampled from those surfels.  The frame after that closes with no node enabled, as before.  (Found with the oracle pipeline and the
restatement on the CPU: closures at frames 3, 6 and 7; 82 of 82, 22 of 112 and 0 of 125 nodes enabled.)"""
import numpy as np
import pytest

from tests import deform_ref as R, helpers

pytestmark = pytest.mark.gpu

W6, H6, K6 = 640, 480, (528.0, 528.0, 320.0, 240.0)
OPTS = dict(model_capacity=2500000, timeDelta=2, confidence=1.0, local_loop_closure=True)
FRAMES = 8
SOLVER_OFF = (4, 5)  # the frames whose loops are dropped


@pytest.fixture(scope="module")
def mods():
    from densemonoslam_amd import capi, deform, fusion, synth

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion, deform, synth


def _frame(synth, k):
    d, rgb, _ = synth.frame(k, width=W6, height=H6, K=K6, noise=True)
    if 2 <= k <= 4:
        d = d.copy()
        d[:, : int(W6 * 0.35)] = 0
    return rgb, d


def _run(mods, mode):
    """mode: 'solver' (one call per frame, the solver on), 'two_phase' (the test drives a stand-alone solver between _begin and
    _end), 'off' (one call, never switched on), 'on_off' (switched on and off again before the first frame)"""
    fusion, deform, synth = mods
    g = fusion.ElasticFusion(W6, H6, K6, **OPTS)
    if mode == "solver":
        g.setLoopSolver(True, 5000)
    if mode == "on_off":
        g.setLoopSolver(True, 5000)
        g.setLoopSolver(False)
    alone = deform.Deformation(2047, 768) if mode == "two_phase" else None
    deforms, out = 0, []
    for k in range(FRAMES):
        rgb, d = _frame(synth, k)
        rec = dict(closed=False)
        if mode == "solver" and k in (SOLVER_OFF[0], SOLVER_OFF[-1] + 1):
            g.setLoopSolver(k not in SOLVER_OFF, 5000)
        if mode == "two_phase":
            g.processFrameBegin(rgb, d)
            rl = g.fetchLoop()
            graph = new_pose = None
            if k > 0 and rl.loop_ok and k not in SOLVER_OFF:
                nodes, rows = g.globalModel().sampleGraph(5000), g.loopConstraints()
                if len(nodes) > 4:
                    alone.setNodes(nodes)
                alone.clearConstraints()
                alone.addConstraints(rows, rl.tick, deforms == 0)
                alone.constrain(rl.tick)
                res = alone.result()
                if res.applied and res.nodes > 0:
                    graph, new_pose = alone.graph(), np.array(rl.loop_pose, np.float32).reshape(4, 4)
                    deforms += 1
                    ids, w = alone.vertexWeights()
                    rec.update(closed=True, table=graph, result=res, nodes=nodes, rows=rows, ctick=rl.tick, pinned=deforms == 1, est=new_pose,
                               relative=alone.relativeConstraints(), ldt=alone.lastDeformTime(), ids=ids, weights=w, pool=alone.pool(),
                               residual0=alone.firstResidual(), jacobian0=alone.firstJacobian(), delta0=alone.firstDelta())
            g.processFrameEnd(graph, new_pose)
            rg = g.fetch()
        else:
            before = g.deforms()
            rg = g.processFrame(rgb, d)
            if g.deforms() > before:
                dd = g.deformation()
                rec.update(closed=True, table=dd.graph(), result=dd.result(), relative=dd.relativeConstraints(), ldt=dd.lastDeformTime())
        rec.update(pose=np.array(rg.pose, np.float32).reshape(4, 4), map=g.globalModel().downloadMap(), fused=bool(rg.fused), tick=rg.tick,
                   surfels=rg.surfels)
        out.append(rec)
    extra = dict(deforms=g.deforms(), relative=g.relativeConstraints() if mode != "two_phase" else None)
    return out, extra


@pytest.fixture(scope="module")
def solver_run(mods):
    return _run(mods, "solver")


@pytest.fixture(scope="module")
def two_phase_run(mods):
    return _run(mods, "two_phase")


def _same_map(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in a.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def test_one_call_frames_equal_the_two_phase_path(solver_run, two_phase_run):
    one, extra = solver_run
    two, _ = two_phase_run
    closed = [k for k, r in enumerate(two) if r["closed"]]
    assert len(closed) >= 2, closed
    assert [k for k, r in enumerate(one) if r["closed"]] == closed and extra["deforms"] == len(closed)
    for k, (a, b) in enumerate(zip(one, two)):
        assert a["pose"].tobytes() == b["pose"].tobytes(), k
        assert (a["fused"], a["tick"], a["surfels"]) == (b["fused"], b["tick"], b["surfels"]), k
        _same_map(a["map"], b["map"], "frame %d" % k)
        if a["closed"]:
            assert a["table"].tobytes() == b["table"].tobytes(), k
            assert bytes(a["result"]) == bytes(b["result"]), k
            assert a["pose"].tobytes() == b["est"].tobytes(), k  # context.currPose() = estPose (:487)
            assert a["relative"].tobytes() == b["relative"].tobytes() and a["ldt"] == b["ldt"], k


def test_solver_state_over_the_stream(solver_run, two_phase_run):
    one, extra = solver_run
    two, _ = two_phase_run
    closed = [r for r in two if r["closed"]]
    n_rows = [len(r["rows"]) for r in closed]
    # the first closing frame's solve carried pins, the later ones did not
    assert [r["result"].constraints for r in closed] == [2 * n_rows[0]] + n_rows[1:]
    assert [r["pinned"] for r in closed] == [True] + [False] * (len(closed) - 1)
    # lastDeformTime is the closing frame's tick (Deformation.cpp:203-206); the first one's from then on bounds the enabled nodes
    assert [r["ldt"] for r in closed] == [r["ctick"] for r in closed]
    # every (size / 3)-th new relative constraint of each closing frame, a step of at least 1 (ElasticFusion.cpp:489-492)
    want = []
    for r in closed:
        rel = r["relative"]
        assert len(rel) == len(r["rows"])
        want += [rel[i] for i in range(0, len(rel), max(1, len(rel) // 3))]
    assert extra["relative"].tobytes() == np.array(want, np.float32).reshape(-1, 8).tobytes()


def test_table_meets_the_solve_bars_against_the_restatement(two_phase_run):
    """The GPU's table against the restatement run on the downloaded nodes and constraints: the bars of tests/test_deform_gpu.py"""
    from tests.deform_cases import ulps

    two, _ = two_phase_run
    ldt = 0
    moved = 0
    for r in [r for r in two if r["closed"]]:
        res = r["result"]
        moved += res.enabled_nodes > 0
        a, b = (R.constrain(r["nodes"], r["rows"], r["ctick"], r["pinned"], r["ctick"], False, ldt, s) for s in ("A", "B"))
        for it, th in enumerate(a["thresholds"]):  # the frame's solve is not a crafted input: say so if it sits on a decision boundary
            for x, y in th:
                assert abs(x - y) >= 0.01 * max(abs(x), abs(y)), ("an exit test of :515 within 1 % of its threshold", r["ctick"], it, x, y)
        assert (res.status, res.iterations, res.exit_reason, res.applied) == (a["status"], a["iterations"], a["exit"], 1)
        assert res.nodes == len(r["nodes"]) and res.enabled_nodes == a["enabled"]
        ua, uk = ulps(a["table"], b["table"]), ulps(r["table"], b["table"])
        print("tick %d: %d nodes (%d enabled), %d constraints; table entries differing from B: A %.4f (max %d ulp), kernel %.4f (max %d ulp); "
              "meanConsErr %.3e -> %.3e" % (r["ctick"], res.nodes, res.enabled_nodes, res.constraints, (ua > 0).mean(), ua.max(), (uk > 0).mean(),
                                           uk.max(), res.mean_cons_err_before, res.mean_cons_err_after))
        assert (uk > 0).mean() <= 2 * (ua > 0).mean() + 0.01 and uk.max() <= ua.max() + 1
        if res.enabled_nodes > 0:
            assert res.mean_cons_err_after < res.mean_cons_err_before and a["meanConsErr_after"] < a["meanConsErr_before"]
        else:
            # A closing frame right after another: lastDeformTime is the previous frame's tick and no surfel of the map is newer, so the
            # reference's own rule (DeformationGraph.cpp:477) enables no node and nothing can move, on either side: 1.296e-03 before and
            # after at tick 8 of this stream, in the kernel and in the restatement alike.
            assert res.mean_cons_err_after == res.mean_cons_err_before and a["meanConsErr_after"] == a["meanConsErr_before"]
            assert np.float32(res.mean_cons_err_before).tobytes() == np.float32(a["meanConsErr_before"]).tobytes()
        ldt = a["lastDeformTime"]
    assert moved >= 1


def test_later_loop_closes_unpinned_on_a_suffix_of_new_nodes(solver_run, two_phase_run):
    """A closing frame after frames that dropped their loops and fused new surfels: deforms >= 1 before it, so no pins; the nodes
    sampled from the new surfels are the enabled suffix.  The one-call frame against the two-phase frame bit for bit, the solve against
    the restatement by the bars of tests/test_deform_gpu.py.  (test_oracle_pipeline_given_the_table_ends_on_the_same_map covers this
    frame's hand-over of the table to the clean with every other frame.)"""
    from tests.deform_cases import ulps

    one, _ = solver_run
    two, _ = two_phase_run
    closed = [k for k, r in enumerate(two) if r["closed"]]
    later = [i for i, k in enumerate(closed) if i >= 1 and 0 < two[k]["result"].enabled_nodes < two[k]["result"].nodes]
    assert later, [(k, two[k]["result"].enabled_nodes, two[k]["result"].nodes) for k in closed]
    i = later[0]
    k, prev = closed[i], closed[i - 1]
    dropped = [j for j in range(prev + 1, k) if not two[j]["closed"] and two[j]["fused"]]
    assert dropped and two[k - 1]["surfels"] > two[prev]["surfels"], (prev, k)  # frames in between fused new surfels
    r, res = two[k], two[k]["result"]
    assert not r["pinned"] and res.constraints == len(r["rows"]) and res.applied == 1
    # the one-call frame is the two-phase frame
    a1 = one[k]
    assert a1["closed"] and a1["pose"].tobytes() == r["pose"].tobytes() == r["est"].tobytes()
    _same_map(a1["map"], r["map"], "frame %d" % k)
    assert a1["table"].tobytes() == r["table"].tobytes() and bytes(a1["result"]) == bytes(res)
    assert a1["relative"].tobytes() == r["relative"].tobytes() and a1["ldt"] == r["ldt"] == r["ctick"]
    # the solve against the restatement
    ldt = two[prev]["ldt"]
    a, b = (R.constrain(r["nodes"], r["rows"], r["ctick"], False, r["ctick"], False, ldt, s) for s in ("A", "B"))
    for it, th in enumerate(a["thresholds"]):
        for x, y in th:
            assert abs(x - y) >= 0.01 * max(abs(x), abs(y)), ("an exit test of :515 within 1 % of its threshold", r["ctick"], it, x, y)
    assert np.array_equal(r["ids"], a["ids"]) and r["weights"].tobytes() == a["weights"].tobytes()
    assert r["residual0"].tobytes() == a["residual0"].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r["jacobian0"], a["jacobian0"]))
    assert np.float32(res.error_initial).tobytes() == np.float32(a["error0"]).tobytes()
    assert np.float32(res.mean_cons_err_before).tobytes() == np.float32(a["meanConsErr_before"]).tobytes()
    assert (res.status, res.iterations, res.exit_reason, res.optimised, res.applied) == (a["status"], a["iterations"], a["exit"], 1, 1)
    assert res.nodes == len(r["nodes"]) and res.enabled_nodes == a["enabled"] and 0 < a["enabled"] < len(r["nodes"])
    rel = lambda x, y: float(np.abs(np.asarray(x, np.longdouble) - np.asarray(y, np.longdouble)).max() / np.abs(np.asarray(y, np.longdouble)).max())
    e_a, e_k = rel(a["delta0"], b["delta0"]), rel(r["delta0"], b["delta0"])
    ua, uk = ulps(a["table"], b["table"]), ulps(r["table"], b["table"])
    print("frame %d (tick %d): %d nodes, %d enabled, %d constraints without pins; delta vs B: kernel %.3e, A %.3e; table entries differing from B: "
          "A %.4f (max %d ulp), kernel %.4f (max %d ulp); meanConsErr %.3e -> %.3e" % (k, r["ctick"], res.nodes, res.enabled_nodes, res.constraints,
          e_k, e_a, (ua > 0).mean(), ua.max(), (uk > 0).mean(), uk.max(), res.mean_cons_err_before, res.mean_cons_err_after))
    assert 0 < e_a < 1e-6 and e_k <= 8 * e_a
    assert (uk > 0).mean() <= 2 * (ua > 0).mean() + 0.01 and uk.max() <= ua.max() + 1
    assert np.array_equal(r["table"][:, [0, 1, 2, 15]], a["table"][:, [0, 1, 2, 15]])
    off = res.nodes - res.enabled_nodes  # the disabled prefix is the untouched graph
    assert r["table"][:off, 3:15].tobytes() == np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (off, 1)).tobytes()
    assert np.abs(r["pool"] - b["pool"]).max() <= 4e-6 and np.array_equal(r["relative"][:, 3:], b["relative"][:, 3:])
    assert np.array_equal(r["relative"][:, :3], r["pool"])
    assert res.mean_cons_err_after < res.mean_cons_err_before and a["meanConsErr_after"] < a["meanConsErr_before"]


def test_oracle_pipeline_given_the_table_ends_on_the_same_map(mods, solver_run):
    from oracle import orc_pipeline

    _, _, synth = mods
    one, _ = solver_run
    o = orc_pipeline.ElasticFusion(W6, H6, K6, **OPTS)
    for k, r in enumerate(one):
        rgb, d = _frame(synth, k)
        cb = (lambda loop, r=r: (r["table"], r["pose"])) if r["closed"] else None
        ro = o.processFrame(rgb, d, inPose=None, deform=cb)
        helpers.assert_pose_identical(r["pose"][:3, 3], r["pose"][:3, :3], ro.pose[:3, 3], ro.pose[:3, :3], what="frame %d" % k)
        _same_map(r["map"], o.model, "oracle pipeline, frame %d" % k)
        o.model = r["map"].copy()
        o.currPose = r["pose"].copy()


def test_switched_on_and_off_again_changes_nothing(mods):
    off, e0 = _run(mods, "off")
    on_off, e1 = _run(mods, "on_off")
    assert e0["deforms"] == e1["deforms"] == 0 and len(e1["relative"]) == 0
    for k, (a, b) in enumerate(zip(off, on_off)):
        assert a["pose"].tobytes() == b["pose"].tobytes() and not b["closed"], k
        _same_map(a["map"], b["map"], "frame %d" % k)


def test_solver_is_refused_where_it_cannot_run(mods):
    """No local_loop_closure, clusters, a frame size with more than 2048 constraint samples, a map several cameras share - at the
    switch, or, where the map is shared after the switch, by the frame before anything of it is enqueued"""
    from densemonoslam_amd import capi

    fusion, _, synth = mods
    W, H, K = 320, 240, (264.0, 264.0, 160.0, 120.0)

    def refused(call):
        with pytest.raises(capi.DmsError) as e:
            call()
        assert e.value.code == -1
        return str(e.value)

    g = fusion.ElasticFusion(W, H, K, model_capacity=100000)  # no local_loop_closure
    refused(lambda: g.setLoopSolver(True))
    g.setLoopSolver(False)
    g.close()
    g = fusion.ElasticFusion(W, H, K, model_capacity=100000, local_loop_closure=True)
    g.setCluster(2)
    assert "cluster" in refused(lambda: g.setLoopSolver(True))
    g.close()
    g = fusion.ElasticFusion(1300, 960, (1000.0, 1000.0, 650.0, 480.0), model_capacity=100000, local_loop_closure=True)  # 65 x 48 samples
    assert "constraint samples" in refused(lambda: g.setLoopSolver(True))
    g.close()
    a = fusion.ElasticFusion(W, H, K, model_capacity=1_000_000, timeIdx=0, local_loop_closure=True)
    b = fusion.ElasticFusion(W, H, K, model_capacity=1_000_000, timeIdx=1, local_loop_closure=True)
    b.setLoopSolver(True)  # alone on its map: accepted
    for k in range(2):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        a.processFrame(rgb, d)
        b.processFrame(rgb, d)
    b.joinMap(a, np.eye(4, dtype=np.float32))
    assert "alone" in refused(lambda: a.setLoopSolver(True))  # the owner of a shared map
    d, rgb, _ = synth.frame(2, width=W, height=H, K=K, noise=True)
    tick = b.fetch().tick
    assert "alone" in refused(lambda: b.processFrame(rgb, d))  # switched on before the join: the frame refuses, and nothing of it ran
    b.setLoopSolver(False)
    assert b.processFrame(rgb, d).tick == tick + 1
    b.close()
    a.close()
