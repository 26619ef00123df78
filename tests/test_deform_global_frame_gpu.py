"""The frame step closes ORB-triggered global loops itself (dms_fusion_set_global_loop_solver, include/dmslam_deform.h): a 160 x 120
synthetic stream (8 x 6 = 48 constraint samples) in the style of tests/test_deform_frame_gpu.py, with one ORB loop the restatement
(tests/deform_global_ref.py) rejects on the downloaded nodes, rows and poses (frame 5: the two poses 4 mm apart, meanConsErr < 0.06) and
one it accepts (frame 6: 10 cm apart).  One-call frames with the switch on against the two-phase path in which the test drives a
stand-alone GlobalDeformation between _begin and _end, bit for bit; the accepted table against the restatement with the bars of
tests/test_deform_gpu.py; a rejected frame against the same frame never armed; dms_fusion_apply_global_loop against _begin + solve +
_end; kept relative rows; on and off again; the refusals."""
import numpy as np
import pytest

from tests import deform_cases, deform_global_ref as G, deform_ref as R

pytestmark = pytest.mark.gpu

W, H, K = 160, 120, (132.0, 132.0, 80.0, 60.0)
OPTS = dict(model_capacity=200000, timeDelta=2, confidence=1.0, local_loop_closure=True, hybrid_loops=1)
RATE, FRAMES, MAX_POSES = 100, 8, 64
ORB = {5: 0.004, 6: 0.1}  # frame -> the offset of orbTcwNew from the current pose; orbTcwOld is the pose of frame 2


@pytest.fixture(scope="module")
def mods():
    from densemonoslam_amd import capi, deform, fusion, synth

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion, deform, synth


def _frame(synth, k):
    d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
    if 2 <= k <= 4:
        d = d.copy()
        d[:, : int(W * 0.35)] = 0
    return rgb, d


def _orb(poses, off):
    new = poses[-1].copy()
    new[:3, 3] += np.array([off, -off / 2, off / 3], np.float32)
    return poses[2].copy(), new


def _context(mods, local_solver=False, global_solver=True):
    g = mods[0].ElasticFusion(W, H, K, **OPTS)
    g.setLoopSolver(True, RATE)  # (also sets the sample rate the global path samples the local graph with)
    if not local_solver:
        g.setLoopSolver(False, RATE)
    if global_solver:
        g.setGlobalLoopSolver(True, MAX_POSES)
    return g


def _global_nodes(m):
    """what dms_deform_sample_model + dms_deform_sample_from take from a downloaded map"""
    s = np.concatenate([m["pos"][::RATE, :3], m["col"][::RATE, 2:3]], 1)[:2047]
    s = s[np.argsort(s[:, 3], kind="stable")]
    return s[::5].astype(np.float32)


def _solve_alone(mods, g, gd, local, tick, relative, pg, rate=RATE):
    """the stand-alone solve on what the frame step left: returns (result, record of the inputs and outputs)"""
    rows = g.globalLoopConstraints()
    nodes = _global_nodes(g.globalModel().downloadMap()) if rate == RATE else None
    local.sampleModel(g.globalModel(), rate)
    gd.sampleFrom(local)
    gd.clearConstraints()
    gd.addConstraints(rows, tick, True)
    if len(relative):
        gd.addRelativeConstraints(relative)
    gd.setPoses(pg[0], pg[1])
    gd.constrainGlobal(tick)
    res = gd.result()
    return res, dict(rows=rows, nodes=nodes, tick=tick, relative=np.array(relative, np.float32).reshape(-1, 8), pg=(np.array(pg[0]), np.array(pg[1])),
                     result=res, table=gd.graph() if res.applied else None, poses=gd.poses()[1], jacobian0=gd.firstJacobian())


def _run(mods, mode, local_solver=False, armed=ORB):
    """mode 'one_call': the switch on; 'two_phase': the test drives the solve and keeps the pose graph itself"""
    fusion, deform, synth = mods
    g = _context(mods, local_solver, global_solver=mode == "one_call")
    gd = deform.GlobalDeformation(410, 48, deform.MAX_RELATIVE, MAX_POSES) if mode == "two_phase" else None
    local = deform.Deformation(2047, 48) if mode == "two_phase" else None
    poses, out, pg_t, pg_p, fern = [], [], [], [], 0
    for k in range(FRAMES):
        rgb, d = _frame(synth, k)
        rec = dict(solve=None)
        if k in armed:
            g.setOrbLoop(*_orb(poses, armed[k]))
        if mode == "two_phase":
            g.processFrameBegin(rgb, d)
            graph = None
            tick = g.fetchLoop().tick
            if k in armed:
                res, rec["solve"] = _solve_alone(mods, g, gd, local, tick, g.relativeConstraints(), (pg_t, pg_p))
                if res.applied and res.nodes > 0:
                    graph, fern = rec["solve"]["table"], fern + 1
                    pg_p = list(rec["solve"]["poses"])
            g.processFrameEnd(graph)
            rg = g.fetch()
            pg_t.append(rg.tick - 1)  # the tick before the frame's increment
            pg_p.append(np.array(rg.pose, np.float32).reshape(4, 4))
        else:
            before = g.fernDeforms()
            rg = g.processFrame(rgb, d)
            if k in armed:
                v = g.globalDeformation()
                res = v.result()
                rec["solve"] = dict(result=res, table=v.graph() if g.fernDeforms() > before else None, jacobian0=v.firstJacobian())
        poses.append(np.array(rg.pose, np.float32).reshape(4, 4))
        rec.update(pose=poses[-1], map=g.globalModel().downloadMap(), tick=rg.tick, surfels=rg.surfels, relative=g.relativeConstraints())
        out.append(rec)
    extra = dict(fern=g.fernDeforms() if mode == "one_call" else fern, pose_graph=g.poseGraph() if mode == "one_call" else (np.array(pg_t), np.array(pg_p)))
    g.close()
    return out, extra


@pytest.fixture(scope="module")
def one_call(mods):
    return _run(mods, "one_call")


@pytest.fixture(scope="module")
def two_phase(mods):
    return _run(mods, "two_phase")


def _same_map(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in a.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def _restate(s, solver="A"):
    calls = [("abs", s["rows"], s["tick"], True)] + ([("rel", s["relative"])] if len(s["relative"]) else [])
    return G.constrain_global(s["nodes"], calls, s["pg"][0], s["pg"][1], solver)


def test_restatement_rejects_the_first_loop_and_accepts_the_second(two_phase):
    """on the downloaded nodes, rows and poses, so the scenario cannot degrade silently; and the kernel takes the same path"""
    out, extra = two_phase
    rej, acc = out[5]["solve"], out[6]["solve"]
    assert len(rej["rows"]) > 0 and len(acc["rows"]) > 0 and len(acc["nodes"]) > 4 and len(acc["pg"][0]) == 6
    for s, want in ((rej, False), (acc, True)):
        a = _restate(s)
        r = s["result"]
        assert a["applied"] == want and bool(r.applied) == want, (a["exit"], r.exit_reason)
        assert (r.status, r.iterations, r.exit_reason, r.optimised, r.nodes) == (a["status"], a["iterations"], a["exit"], int(a["optimised"]), len(s["nodes"]))
        for got, ref in zip(s["jacobian0"], a["jacobian0"]):
            assert got.tobytes() == ref.tobytes()
    assert extra["fern"] == 1


def test_one_call_frames_equal_the_two_phase_path(one_call, two_phase):
    (a, ea), (b, eb) = one_call, two_phase
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["pose"].tobytes() == y["pose"].tobytes() and x["tick"] == y["tick"] and x["surfels"] == y["surfels"], k
        _same_map(x["map"], y["map"], "frame %d" % k)
        if k in ORB:
            assert bytes(x["solve"]["result"]) == bytes(y["solve"]["result"]), k
    assert a[6]["solve"]["table"].tobytes() == b[6]["solve"]["table"].tobytes() and a[5]["solve"]["table"] is None
    assert ea["fern"] == eb["fern"] == 1
    assert np.array_equal(ea["pose_graph"][0], eb["pose_graph"][0]) and list(ea["pose_graph"][0]) == [r["tick"] - 1 for r in a]
    assert ea["pose_graph"][1].tobytes() == np.ascontiguousarray(eb["pose_graph"][1], np.float32).tobytes()
    # the closure corrected the poses kept before it
    assert not np.array_equal(ea["pose_graph"][1][:6], np.array([r["pose"] for r in a[:6]]))
    assert np.array_equal(ea["pose_graph"][1][6:], np.array([r["pose"] for r in a[6:]]))


def test_accepted_table_meets_the_solve_bars_against_the_restatement(two_phase):
    s = two_phase[0][6]["solve"]
    a, b = _restate(s, "A"), _restate(s, "B")
    ulps = deform_cases.ulps
    ua, uk = ulps(a["table"], b["table"]), ulps(s["table"], b["table"])
    share_a, share_k = float((ua > 0).mean()), float((uk > 0).mean())
    print("table entries differing from B: A %.4f (max %d ulp), kernel %.4f (max %d ulp)" % (share_a, ua.max(), share_k, uk.max()))
    assert share_k <= 2 * share_a + 0.01 and uk.max() <= ua.max() + 1
    assert np.abs(s["poses"][:, :3, 3] - b["poses"][:, :3, 3]).max() <= 4e-6


def test_rejected_frame_equals_the_frame_never_armed(mods):
    """with the local solver on: a frame whose ORB loop is rejected goes on into the local block as a frame without one does"""
    armed, _ = _run(mods, "one_call", local_solver=True, armed={5: ORB[5]})
    plain, _ = _run(mods, "one_call", local_solver=True, armed={})
    assert armed[5]["solve"]["result"].applied == 0
    for k, (x, y) in enumerate(zip(armed, plain)):
        assert x["pose"].tobytes() == y["pose"].tobytes(), k
        _same_map(x["map"], y["map"], "frame %d" % k)


W6, H6, K6 = 640, 480, (528.0, 528.0, 320.0, 240.0)  # the stream of tests/test_deform_frame_gpu.py: its first local loop closes at frame 3


def _frame6(synth, k):
    d, rgb, _ = synth.frame(k, width=W6, height=H6, K=K6, noise=True)
    if 2 <= k <= 4:
        d = d.copy()
        d[:, : int(W6 * 0.35)] = 0
    return rgb, d


def _nodes6(m, rate=5000):
    s = np.concatenate([m["pos"][::rate, :3], m["col"][::rate, 2:3]], 1)[:2047]
    return s[np.argsort(s[:, 3], kind="stable")][::5].astype(np.float32)


def test_kept_relative_rows_reach_the_global_solve(mods):
    """Both solvers on, 640 x 480: the local loop of frame 3 is closed by the library, which keeps every (size / 3)-th new relative row;
    frame 4 is armed with an ORB loop.  Its solve must hold the frame's rows with their pins AND the kept rows: the constraint count,
    and the first Jacobian equal to the restatement's bits on the downloaded nodes, rows, kept rows and poses, and to a two-phase
    solve's by a stand-alone object on the same downloads."""
    fusion, deform, synth = mods
    got = {}
    for mode in ("one_call", "two_phase"):
        g = fusion.ElasticFusion(W6, H6, K6, model_capacity=2500000, timeDelta=2, confidence=1.0, local_loop_closure=True, hybrid_loops=1)
        g.setLoopSolver(True, 5000)
        g.setGlobalLoopSolver(True, MAX_POSES)
        poses = []
        for k in range(4):
            poses.append(np.array(g.processFrame(*_frame6(synth, k)).pose, np.float32).reshape(4, 4))
        kept, pg, tick = g.relativeConstraints(), g.poseGraph(), g.fetch().tick
        assert g.deforms() == 1 and len(kept) >= 3 and list(pg[0]) == [1, 2, 3, 4] and tick == 5
        nodes = _nodes6(g.globalModel().downloadMap())
        new = poses[-1].copy()
        new[:3, 3] += np.array([0.1, -0.05, 0.033], np.float32)
        g.setOrbLoop(poses[2].copy(), new)
        if mode == "one_call":
            g.processFrame(*_frame6(synth, 4))
            v = g.globalDeformation()
            rows = g.globalLoopConstraints()
            got[mode] = dict(result=v.result(), jacobian0=v.firstJacobian(), residual0=v.firstResidual(), ids=v.vertexWeights()[0])
            s = dict(nodes=nodes, rows=rows, tick=tick, relative=kept, pg=pg)
        else:
            gd, local = deform.GlobalDeformation(410, 768, deform.MAX_RELATIVE, MAX_POSES), deform.Deformation(2047, 768)
            g.processFrameBegin(*_frame6(synth, 4))
            res, rec = _solve_alone(mods, g, gd, local, tick, kept, pg, rate=5000)
            got[mode] = dict(result=res, jacobian0=rec["jacobian0"], residual0=gd.firstResidual(), ids=gd.vertexWeights()[0], rows=rec["rows"], kept=kept)
            g.processFrameEnd(rec["table"] if res.applied else None)
            assert list(g.poseGraph()[0]) == [1, 2, 3, 4, 5]  # a two-phase frame is kept in the pose graph too
            gd.close()
            local.close()
        g.close()
    one, two = got["one_call"], got["two_phase"]
    assert s["rows"].tobytes() == two["rows"].tobytes() and s["relative"].tobytes() == two["kept"].tobytes()
    n_rows, n_kept = len(s["rows"]), len(s["relative"])
    a = _restate(s)
    assert one["result"].constraints == 2 * n_rows + 2 * n_kept == len(a["ids"]) and n_rows > 0
    assert a["exit"] != 6 and (a["kinds"] == G.REL_SRC).sum() == n_kept
    assert np.array_equal(one["ids"], a["ids"]) and one["residual0"].tobytes() == a["residual0"].tobytes()
    for x, y, z in zip(one["jacobian0"], a["jacobian0"], two["jacobian0"]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    # the relative rows are the last 3 x kept rows of J, in the order the context kept them
    assert one["jacobian0"][0][-1] - one["jacobian0"][0][-1 - 3 * n_kept] >= 3 * 4 * n_kept
    assert bytes(one["result"]) == bytes(two["result"])


def test_switched_on_and_off_again_changes_nothing(mods):
    synth = mods[2]
    a, b = _context(mods, global_solver=False), _context(mods, global_solver=True)
    b.setGlobalLoopSolver(False)
    for k in range(4):
        ra, rb = a.processFrame(*_frame(synth, k)), b.processFrame(*_frame(synth, k))
        assert bytes(np.array(ra.pose, np.float32)) == bytes(np.array(rb.pose, np.float32)) and ra.surfels == rb.surfels
    _same_map(a.globalModel().downloadMap(), b.globalModel().downloadMap(), "map")
    assert len(b.poseGraph()[0]) == 0 and b.fernDeforms() == 0
    a.close()
    b.close()


def test_apply_global_loop_equals_begin_solve_end(mods):
    fusion, deform, synth = mods
    maps, results = [], []
    for one in (True, False):
        g = _context(mods, global_solver=one)
        poses = []
        for k in range(6):
            poses.append(np.array(g.processFrame(*_frame(synth, k)).pose, np.float32).reshape(4, 4))
        old, new = _orb(poses, ORB[6])
        if one:
            g.applyGlobalLoop(old, new)
            results.append((bytes(g.globalDeformation().result()), g.fernDeforms()))
        else:
            gd, local = deform.GlobalDeformation(410, 48, deform.MAX_RELATIVE, MAX_POSES), deform.Deformation(2047, 48)
            g.applyGlobalLoopBegin(old, new)
            res, s = _solve_alone(mods, g, gd, local, g.fetch().tick, g.relativeConstraints(), (np.arange(1, 7), np.array(poses)))
            g.applyGlobalLoopEnd(s["table"] if res.applied else None, accepted=bool(res.applied))
            results.append((bytes(res), int(bool(res.applied))))
            gd.close()
            local.close()
        maps.append(g.globalModel().downloadMap())
        g.close()
    assert results[0] == results[1]
    _same_map(maps[0], maps[1], "map after applyGlobalLoop")


def test_global_solver_is_refused_where_it_cannot_run(mods):
    from densemonoslam_amd import capi

    fusion, _, synth = mods

    def refused(call, code=-1):
        with pytest.raises(capi.DmsError) as e:
            call()
        assert e.value.code == code
        return str(e.value)

    base = dict(model_capacity=100000)
    g = fusion.ElasticFusion(W, H, K, **base)  # no hybrid_loops
    assert "hybrid_loops" in refused(lambda: g.setGlobalLoopSolver(True, 8))
    g.close()
    g = fusion.ElasticFusion(W, H, K, hybrid_loops=1, **base)
    g.setCluster(2)
    assert "cluster" in refused(lambda: g.setGlobalLoopSolver(True, 8))
    g.close()
    a = fusion.ElasticFusion(W, H, K, hybrid_loops=1, timeIdx=0, **base)
    b = fusion.ElasticFusion(W, H, K, hybrid_loops=1, timeIdx=1, **base)
    b.setGlobalLoopSolver(True, 3)
    for k in range(2):
        a.processFrame(*_frame(synth, k))
        b.processFrame(*_frame(synth, k))
    b.joinMap(a, np.eye(4, dtype=np.float32))
    assert "alone" in refused(lambda: a.setGlobalLoopSolver(True, 8))
    tick = b.fetch().tick
    assert "alone" in refused(lambda: b.processFrame(*_frame(synth, 2)))
    assert b.fetch().tick == tick
    b.close()
    a.close()
    g = fusion.ElasticFusion(W, H, K, hybrid_loops=1, **base)
    g.setGlobalLoopSolver(True, 3)
    for k in range(3):
        g.processFrame(*_frame(synth, k))
    tick = g.fetch().tick
    assert "pose graph" in refused(lambda: g.processFrame(*_frame(synth, 3)), code=-4)  # max_poses reached: nothing of the frame ran
    assert g.fetch().tick == tick and len(g.poseGraph()[0]) == 3
    g.close()
