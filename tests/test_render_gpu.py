"""The map draw (include/dmslam_render.h, GlobalModel::renderPointCloud) on the MI355X against the CPU restatement
tests/render_ref.py, bit for bit: colour bytes, 24-bit depth and winner key of every pixel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 320, 240
K = (264.0, 264.0, 160.0, 120.0)
FRAMES = 4


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


@pytest.fixture(scope="module")
def grown(fus):
    """a map grown by the frame step on the synthetic stream: (context, tracked pose, surfel records)"""
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    for k in range(FRAMES):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
    pose = np.array(r.pose, np.float32).reshape(4, 4)
    recs = g.globalModel().downloadMap()
    assert len(recs) > 1000
    yield g, pose, recs
    g.close()


def _proj(w, h, f=None, near=0.1, far=1000.0):
    from densemonoslam_amd import fusion

    f = (K[0] * w / W) if f is None else f
    return fusion.render_frustum(w, h, f, f, w / 2.0, h / 2.0, near, far)


def _views(pose):
    """name -> (width, height, projection, camera-to-world pose)"""
    oblique = pose.copy()
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique[:3, :3] = pose[:3, :3] @ Ry
    # half way into the scene: surfels across the near plane and behind the eye
    oblique[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(1.2)
    close = pose.copy()
    close[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(0.8)
    return {
        "tracked": (W, H, _proj(W, H), pose),
        "oblique": (W, H, _proj(W, H, near=0.05), oblique),
        "closeup": (640, 480, _proj(640, 480, f=2400.0), close),
        "gui": (1024, 320, _proj(1024, 320, f=420.0), pose),
    }


def _check(fus, model, recs, w, h, proj, pose, draws, use_pose_dev=False, pose_ptr=None):
    """draws: list of parameter dicts; the target is cleared once, then every draw goes in; returns the images."""
    t = fus.RenderTarget(w, h)
    t.clear((0.1, 0.2, 0.3, 1.0))
    ref = R.Target(w, h, (0.1, 0.2, 0.3, 1.0))
    mvp_host = R.mvp_from_pose(proj, pose)
    for p in draws:
        if use_pose_dev:
            t.draw(model, proj, pose_dev=C.c_void_p(pose_ptr), **p)
        else:
            t.draw(model, mvp_host, **p)
        ref.draw(recs, mvp_host, **p)
    got = t.images()
    exp = ref.images()
    t.close()
    for name, a, b in zip(("colour", "depth24", "winner"), got, exp):
        bad = np.argwhere(a.reshape(h, w, -1).view(np.uint8).reshape(h, w, -1) != b.reshape(h, w, -1).view(np.uint8).reshape(h, w, -1))
        assert len(bad) == 0, "%s differs at %d places, first %s: %s vs %s" % (name, len(bad), bad[:3].tolist(), a[tuple(bad[0][:2])],
                                                                             b[tuple(bad[0][:2])])
    return got


MATRIX = [
    dict(color_type=0),
    dict(color_type=1, draw_unstable=True),
    dict(color_type=2, threshold="median"),
    dict(color_type=3, time=FRAMES, draw_unstable=True),
    dict(color_type=4, time=FRAMES, threshold="median"),
    dict(color_type=2, cluster_color=(0.9, 0.2, 0.4)),
    dict(color_type=2, draw_window=True, time=FRAMES + 1, time_idx=0, time_delta=2, draw_unstable=True),
    dict(color_type=0, draw_window=True, time=3, time_idx=0, time_delta=1),
    dict(color_type=2, draw_points=True, threshold="median"),
    dict(color_type=1, draw_points=True, cluster_color=(0.5, 0.5, 1.0)),
]


@pytest.mark.parametrize("view", ["tracked", "oblique", "closeup", "gui"])
@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_draw_matches_the_restatement(fus, grown, view, case):
    g, pose, recs = grown
    w, h, proj, vp = _views(pose)[view]
    p = dict(MATRIX[case])
    if p.get("threshold") == "median":  # a threshold that splits the map into stable and unstable surfels
        p["threshold"] = float(np.median(recs["pos"][:, 3]))
        assert (recs["pos"][:, 3] > p["threshold"]).any() and (recs["pos"][:, 3] <= p["threshold"]).any()
    got = _check(fus, g.globalModel(), recs, w, h, proj, vp, [p])
    covered = int((got[1] < 0xFFFFFF).sum())
    assert covered > 0, "nothing drawn"


def test_closeup_footprints_exceed_500_pixels(fus, grown):
    g, pose, recs = grown
    w, h, proj, vp = _views(pose)["closeup"]
    _, _, key = _check(fus, g.globalModel(), recs, w, h, proj, vp, [dict(color_type=2, draw_unstable=True)])
    ids = (key[key != R.CLEARED] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.bincount(ids).max() > 500


def test_oblique_view_clips_at_the_near_plane(fus, grown):
    g, pose, recs = grown
    w, h, proj, vp = _views(pose)["oblique"]
    M = R.mvp_from_pose(proj, vp)
    cv = R.disc_corners(M, recs["pos"].astype(np.float32), recs["nrm"].astype(np.float32))
    near = [(c[2] + c[3]) >= 0 for c in cv]
    crossing = (near[0] | near[1] | near[2] | near[3]) & ~(near[0] & near[1] & near[2] & near[3])
    behind = np.asarray([c[3] < 0 for c in cv]).all(0)
    assert crossing.sum() > 0 and behind.sum() > 0
    # in that view the crossing surfels win no pixel: a map of its own puts discs across the near plane right in front of the camera
    # (tilted 45 degrees, 10 cm radius, centres at z = 0.1 and 0.12 with the near plane at 0.1) and one behind the eye, so that the
    # clipped instance of the disc pass must win pixels, bit for bit as the restatement's
    few = recs[:3].copy()
    few["pos"][:, :3] = [[0.0, 0.0, 0.1], [0.03, 0.02, 0.12], [0.0, 0.0, -0.5]]
    few["pos"][:, 3] = 20.0
    few["nrm"][:, :3] = np.float32(np.sqrt(0.5)) * np.array([1.0, 0.0, -1.0], np.float32)
    few["nrm"][:, 3] = 0.1
    m = fus.GlobalModel(W, H, capacity=64)
    m.upload(few)
    eye = np.eye(4, dtype=np.float32)
    cvf = R.disc_corners(R.mvp_from_pose(proj, eye), few["pos"], few["nrm"])
    nf = [(c[2] + c[3]) >= 0 for c in cvf]
    cross = (nf[0] | nf[1] | nf[2] | nf[3]) & ~(nf[0] & nf[1] & nf[2] & nf[3])
    assert cross[0] and cross[1]
    _, _, key = _check(fus, m, few, W, H, proj, eye, [dict(color_type=2, draw_unstable=True)])
    ids = (key[key != R.CLEARED] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert len(ids) > 100 and cross[ids].all()
    m.close()


def test_empty_map_and_single_surfel(fus, grown):
    _, pose, recs = grown
    m = fus.GlobalModel(W, H, capacity=1024)
    proj = _proj(W, H)
    _check(fus, m, recs[:0], W, H, proj, pose, [dict(color_type=2)])  # nothing drawn: the clear colour everywhere
    one = recs[len(recs) // 2:len(recs) // 2 + 1].copy()
    m.upload(one)
    got = _check(fus, m, one, W, H, proj, pose, [dict(color_type=2, draw_unstable=True)])
    assert (got[1] < 0xFFFFFF).sum() > 0
    m.close()


def test_two_draws_into_one_target_keep_the_first(fus, grown):
    g, pose, recs = grown
    w, h, proj, vp = _views(pose)["tracked"]
    c, d, key = _check(fus, g.globalModel(), recs, w, h, proj, vp,
                       [dict(color_type=2, cluster_color=(1.0, 0.0, 0.0)), dict(color_type=2, cluster_color=(0.0, 1.0, 0.0))])
    cov = d < 0xFFFFFF
    assert cov.sum() > 0
    assert (c[cov] == np.array([255, 0, 0, 255], np.uint8)).all()
    assert ((key[cov] >> np.uint64(32)) & np.uint64(0xFF) == 0).all()


def test_two_cluster_models_of_one_context(fus):
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    for k, cl in enumerate([0, 0, 0, 1, 1]):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d, cluster=cl)
    pose = np.array(r.pose, np.float32).reshape(4, 4)
    models = [g.globalModel(0), g.globalModel(1)]
    recs = [m.downloadMap() for m in models]
    cols = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1)]
    proj = _proj(W, H)
    ids, _ = g.clusters()
    assert ids == [0, 1]
    # the reference's argument: cluster ids (GlobalModel::clusters()), resolved through the context
    got = models[0].renderPointCloud(R.mvp_from_pose(proj, pose), 10.0, True, False, True, False, False, False, False, FRAMES, 0, 200,
                                     clusters=ids, drawClusters=True, cluster_colors=cols, clear_rgba=(0, 0, 0, 0), context=g)
    ref = R.Target(W, H)
    for rr, cc in zip(recs, cols):
        ref.draw(rr, R.mvp_from_pose(proj, pose), threshold=10.0, draw_unstable=True, color_type=2, time=FRAMES, time_delta=200,
                 cluster_color=cc)
    for a, b in zip(got, ref.images()):
        assert np.array_equal(a, b)
    g.close()


def test_pose_dev_equals_host_composed_mvp(fus, grown):
    g, pose, recs = grown
    w, h, proj, _ = _views(pose)["tracked"]
    from densemonoslam_amd import fusion

    assert np.array_equal(fusion.render_mvp_from_pose(proj, pose).view(np.uint32), R.mvp_from_pose(proj, pose).view(np.uint32))
    dev = _check(fus, g.globalModel(), recs, w, h, proj, pose, [dict(color_type=2)], use_pose_dev=True, pose_ptr=g.poseDevice())
    host = _check(fus, g.globalModel(), recs, w, h, proj, pose, [dict(color_type=2)])
    for a, b in zip(dev, host):
        assert np.array_equal(a, b)


def test_render_from_tracked_pose_lines_up_with_the_prediction(fus, grown):
    g, pose, recs = grown
    from densemonoslam_amd import capi

    # ElasticFusion::predict (the ACTIVE view at the camera's pose into the prediction images) with the tracking prediction's threshold
    conf = 0.7
    capi.check(capi.lib.dms_fusion_predict(g.h, C.c_float(conf), None), "dms_fusion_predict")
    capi.check(capi.lib.dms_stream_sync(None), "dms_stream_sync")
    pred = g.image(9)  # rgba8, image rows
    c, d, _ = g.globalModel().renderPointCloud(R.mvp_from_pose(_proj(W, H), pose), conf, False, False, True, False, False, False, False,
                                               FRAMES, 0, 200, image_order=True)
    a = d < 0xFFFFFF
    b = pred[..., 3] > 0
    iou = (a & b).sum() / max(1, (a | b).sum())
    assert iou >= 0.95, iou


def _run_frames(fus, renders):
    """8 frames; renders: None, 'same' (a draw on the frame's stream between frames) or 'other' (on a second stream that waits
    for the frame through dms_fusion_wait_frame_done)."""
    from densemonoslam_amd import capi, synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    t = fus.RenderTarget(W, H)
    s2 = capi.create_stream() if renders == "other" else None
    poses = []
    proj = _proj(W, H)
    for k in range(8):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
        poses.append(np.array(r.pose, np.float32).tobytes())
        if renders == "same":
            t.draw(g.globalModel(), proj, threshold=1.0, draw_unstable=True, color_type=2, pose_dev=C.c_void_p(g.poseDevice()))
        elif renders == "other":
            capi.check(capi.lib.dms_fusion_wait_frame_done(g.h, C.c_void_p(s2)), "dms_fusion_wait_frame_done")
            t.draw(g.globalModel(), proj, threshold=1.0, draw_unstable=True, color_type=2, pose_dev=C.c_void_p(g.poseDevice()),
                   stream=C.c_void_p(s2))
            capi.check(capi.lib.dms_stream_sync(C.c_void_p(s2)), "dms_stream_sync")
    recs = g.globalModel().downloadMap()
    t.close()
    if s2 is not None:
        capi.destroy_stream(s2)
    g.close()
    return poses, recs


def test_renders_between_frames_change_nothing(fus):
    base_p, base_m = _run_frames(fus, None)
    for mode in ("same", "other"):
        p, m = _run_frames(fus, mode)
        assert p == base_p, mode
        assert len(m) == len(base_m)
        for f in ("pos", "col", "nrm", "times"):
            assert np.array_equal(m[f].view(np.uint32), base_m[f].view(np.uint32)), (mode, f)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render.npz")


def test_draw_against_the_reference_programs_on_llvmpipe(fus):
    """HIP against tests/golden/ref_render.npz (the reference's draw programs on Mesa llvmpipe) by the rules of the CPU test
    (tests/test_render_cpu.py), and equal to the restatement bit for bit on the same map"""
    z = np.load(GOLDEN)
    s = R.fixture_map(z)
    m = fus.GlobalModel(W, H, capacity=len(s) + 16)
    m.upload(s)
    b = R.FIXTURE_BOUNDS
    for name in (str(n) for n in z["cases"]):
        h, w = z[name + "__depth"].shape
        t = fus.RenderTarget(w, h)
        t.clear(tuple(z["clear"]))
        ref = R.Target(w, h, tuple(z["clear"]))
        for p in R.fixture_draws(z, name):
            t.draw(m, z[name + "__mvp"], **p)
            ref.draw(s, z[name + "__mvp"], **p)
        got = t.images()
        t.close()
        for a, e in zip(got, ref.images()):
            assert np.array_equal(a, e), name
        st = R.fixture_stats(z, name, got[0], got[1])
        assert st["covered"] > 0 and st["coverage"] <= b["coverage"] and st["colour"] <= b["colour"], (name, st)
        if "points" in name:
            assert st["depth"] <= b["depth_points"], (name, st)
        elif not name.startswith("oblique"):
            assert st["depth"] <= b["depth_discs"], (name, st)
    m.close()
