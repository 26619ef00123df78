"""The live-frame cloud draw (include/dmslam_render_cloud.h, FeedbackBuffer::render of the RAW / FILTERED buffer) on the MI355X against
the CPU restatement tests/render_cloud_ref.py, bit for bit: colour bytes, 24-bit depth and winner key of every pixel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cloud_ref as RC  # noqa: E402
import render_ref as R  # noqa: E402
import render_shaded_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 320, 240
K = (264.0, 264.0, 160.0, 120.0)
FRAMES = 4
MAXD = 25.0  # (float)(int)maxDepthProcessed of the default parameters
CLEAR = (0.1, 0.2, 0.3, 1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render_cloud.npz")


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


def _inputs(g):
    """the current frame's colour, raw and filtered metric depth (what computeFeedbackBuffers keeps)"""
    return g.image(0), g.image(3), g.image(4)


@pytest.fixture(scope="module")
def grown(fus):
    """a context after FRAMES frames with its feedback inputs refreshed: (context, tracked pose, inputs of the last frame, map)"""
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    for k in range(FRAMES):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
    g.computeFeedbackBuffers()
    pose = np.array(r.pose, np.float32).reshape(4, 4)
    inp = _inputs(g)
    assert (inp[1] > 0).sum() > 1000 and not np.array_equal(inp[1], inp[2])
    yield g, pose, inp, g.globalModel().downloadMap()
    g.close()


def _proj(w, h, f=None, near=0.1, far=1000.0):
    from densemonoslam_amd import fusion

    f = (K[0] * w / W) if f is None else f
    return fusion.render_frustum(w, h, f, f, w / 2.0, h / 2.0, near, far)


def _views(pose):
    """name -> (width, height, projection, camera-to-world pose of the view)"""
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique = pose.copy()
    oblique[:3, :3] = pose[:3, :3] @ Ry
    oblique[:3, 3] = pose[:3, 3] - pose[:3, 0] * np.float32(0.8)
    inside = pose.copy()  # half way into the scene and turned: points behind the near plane and outside the frustum
    inside[:3, :3] = pose[:3, :3] @ Ry
    inside[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(1.2)
    return {
        "tracked": (W, H, _proj(W, H), pose),                      # the frame's own projection: the target is the frame's size
        "oblique": (640, 480, _proj(640, 480, near=0.05), oblique),  # above the frame's size
        "inside": (200, 150, _proj(200, 150), inside),             # below it
    }


def _same(got, exp, what=""):
    for name, a, b in zip(("colour", "depth24", "winner"), got, exp):
        h, w = a.shape[:2]
        bad = np.argwhere(a.reshape(h, w, -1).view(np.uint8).reshape(h, w, -1) != b.reshape(h, w, -1).view(np.uint8).reshape(h, w, -1))
        assert len(bad) == 0, "%s %s differs at %d places, first %s: %s vs %s" % (what, name, len(bad), bad[:3].tolist(), a[tuple(bad[0][:2])],
                                                                                b[tuple(bad[0][:2])])


def _ref(w, h, draws):
    """draws: (rgba, depth, mvp, model_pose, color_type) in order into one cleared restatement target"""
    ref = R.Target(w, h, CLEAR)
    for rgba, depth, mvp, mp, ct in draws:
        RC.draw_cloud(ref, rgba, depth, K, MAXD, mvp, mp, ct)
    return ref


@pytest.mark.parametrize("view", ["tracked", "oblique", "inside"])
@pytest.mark.parametrize("ct", [0, 1, 2])
@pytest.mark.parametrize("which", [RC.RAW, RC.FILTERED])
def test_cloud_matches_the_restatement(fus, grown, which, ct, view):
    g, pose, inp, _ = grown
    w, h, proj, vp = _views(pose)[view]
    mvp = R.mvp_from_pose(proj, vp)
    t = fus.RenderTarget(w, h)
    t.clear(CLEAR)
    g.renderCloud(t, which, mvp, pose, ct)
    got = t.images()
    t.close()
    ref = _ref(w, h, [(inp[0], inp[1 + which], mvp, pose, ct)])
    _same(got, ref.images())
    covered = int((got[1] < 0xFFFFFF).sum())
    emitted = int(((inp[1 + which] > 0) & (inp[1 + which] <= MAXD)).sum())
    assert 0 < covered <= emitted
    if view == "inside":
        assert covered < emitted // 2, "the view must lose points behind the near plane and outside the frustum"


def test_device_matrices_equal_host_matrices(fus, grown):
    """model_pose_dev (the tracked pose in HBM) and pose_dev (the view built on the device) against the host matrices"""
    g, pose, inp, _ = grown
    proj = _proj(W, H)
    out = []
    for kw in (dict(mvp=R.mvp_from_pose(proj, pose), model_pose=pose),
               dict(mvp=R.mvp_from_pose(proj, pose), model_pose_dev=C.c_void_p(g.poseDevice())),
               dict(mvp=proj, pose_dev=C.c_void_p(g.poseDevice()), model_pose_dev=C.c_void_p(g.poseDevice())),
               dict(mvp=proj, pose_dev=C.c_void_p(g.poseDevice()), model_pose=pose)):
        t = fus.RenderTarget(W, H)
        t.clear(CLEAR)
        g.renderCloud(t, RC.RAW, color_type=0, **kw)
        out.append(t.images())
        t.close()
    for o in out[1:]:
        _same(o, out[0], "device matrix path")
    _same(out[0], _ref(W, H, [(inp[0], inp[1], R.mvp_from_pose(proj, pose), pose, 0)]).images())
    pt = (0.3, -0.2, 1.7)
    assert np.array_equal(fus.render_cloud_clip(R.mvp_from_pose(proj, pose), pose, pt),
                          np.array(RC.cloud_clip(R.mvp_from_pose(proj, pose), pose, *pt), np.float32))


def test_operator_on_free_images_equals_the_context_draw(fus, grown):
    g, pose, inp, _ = grown
    w, h, proj, vp = _views(pose)["oblique"]
    mvp = R.mvp_from_pose(proj, vp)
    for which in (RC.RAW, RC.FILTERED):
        a, b = fus.RenderTarget(w, h), fus.RenderTarget(w, h)
        a.clear(CLEAR)
        b.clear(CLEAR)
        g.renderCloud(a, which, mvp, pose, 1)
        fus.render_cloud(b, inp[0], inp[1 + which], K, MAXD, mvp, pose, 1)
        _same(b.images(), a.images(), "operator")
        a.close()
        b.close()


def test_operator_on_an_image_of_another_size(fus):
    """free images need not be the context's size; zeros, NaN and depths beyond max_depth emit nothing"""
    rng = np.random.default_rng(5)
    w, h = 96, 50
    depth = rng.uniform(0.5, 4.0, (h, w)).astype(np.float32)
    depth[::7] = 0
    depth[:, ::5] = 3.5
    depth[3::11, 2::3] = np.nan
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    k = (80.0, 82.0, 47.5, 25.5)
    mvp = R.mvp_from_pose(_proj(128, 100, f=90.0), np.eye(4, dtype=np.float32))
    for ct in (0, 1, 2):
        t = fus.RenderTarget(128, 100)
        t.clear(CLEAR)
        fus.render_cloud(t, rgba, depth, k, 3.0, mvp, None, ct)
        got = t.images()
        t.close()
        ref = R.Target(128, 100, CLEAR)
        RC.draw_cloud(ref, rgba, depth, k, 3.0, mvp, None, ct)
        _same(got, ref.images())
        assert (got[1] < 0xFFFFFF).sum() > 500


def test_all_invalid_depth_draws_nothing(fus, grown):
    g, pose, inp, _ = grown
    depth = np.zeros((H, W), np.float32)
    depth[::2] = 26.0
    depth[1::4] = np.nan
    depth[3::4] = -1.0
    t = fus.RenderTarget(W, H)
    t.clear(CLEAR)
    before = t.images()
    fus.render_cloud(t, inp[0], depth, K, MAXD, R.mvp_from_pose(_proj(W, H), pose), pose, 2)
    _same(t.images(), before, "invalid depth")
    assert (t.images()[2] == R.CLEARED).all()
    t.close()


def test_clouds_compose_with_the_map_draw_and_the_shaded_view(fus, grown):
    """the frame of MainController: clear, RAW cloud, FILTERED cloud, the map (renderPointCloud), then the shaded view resolved over
    the same target, against the restatements chained in that order"""
    g, pose, inp, recs = grown
    w, h, proj, vp = _views(pose)["oblique"]
    mvp = R.mvp_from_pose(proj, vp)
    sw, sh = 400, 300
    mvp_off = R.mvp_from_pose(_proj(sw, sh, near=0.05), vp)
    light, clear_off = (0.1, 0.2, 0.3), (0.05, 0.05, 0.3, 0.0)
    thr = float(np.median(recs["pos"][:, 3]))
    v = fus.ShadedView(w, h, offscreen=(sw, sh))
    v.clear(CLEAR)
    g.renderCloud(v.target, RC.RAW, mvp, pose, 2)
    g.renderCloud(v.target, RC.FILTERED, mvp, pose, 1)
    v.target.draw(g.globalModel(), mvp, threshold=thr, color_type=2)
    mid = v.target.images()
    v.draw(g.globalModel(), mvp_off, light_pos=light, clear_rgba=clear_off, threshold=thr, draw_unstable=True, color_type=2)
    v.fxaa()
    got = v.images()
    v.close()
    ref = _ref(w, h, [(inp[0], inp[1], mvp, pose, 2), (inp[0], inp[2], mvp, pose, 1)])
    ref.draw(recs, mvp, threshold=thr, color_type=2)
    _same(mid, ref.images(), "clouds + map")
    seq = (mid[2][mid[2] != R.CLEARED] >> np.uint64(32)) & np.uint64(0xFF)
    assert all((seq == k).any() for k in (0, 1, 2)), "both clouds and the map must own pixels"
    off = S.Offscreen(sw, sh)
    off.draw(recs, mvp_off, light_pos=light, clear_rgba=clear_off, threshold=thr, draw_unstable=True, color_type=2)
    S.composite(ref, off)
    _same(got, ref.images(), "after the composite")


def _run_frames(fus, clouds):
    """8 frames; clouds: both clouds on the frame's stream between frames, view and model pose from the tracked pose in HBM"""
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    t = fus.RenderTarget(640, 480)
    proj = _proj(640, 480)
    poses = []
    for k in range(8):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
        poses.append(np.array(r.pose, np.float32).tobytes())
        if clouds:
            if k:
                g.computeFeedbackBuffers()
            t.clear((0, 0, 0, 1))
            for which in (RC.RAW, RC.FILTERED):
                g.renderCloud(t, which, proj, color_type=which, pose_dev=C.c_void_p(g.poseDevice()), model_pose_dev=C.c_void_p(g.poseDevice()))
    recs = g.globalModel().downloadMap()
    img = t.images()
    t.close()
    g.close()
    return poses, recs, img


def test_clouds_between_frames_change_nothing(fus):
    base_p, base_m, _ = _run_frames(fus, False)
    p, m, img = _run_frames(fus, True)
    assert (img[1] < 0xFFFFFF).sum() > 1000
    assert p == base_p
    assert len(m) == len(base_m)
    for f in ("pos", "col", "nrm", "times"):
        assert np.array_equal(m[f].view(np.uint32), base_m[f].view(np.uint32)), f


def test_the_cloud_is_the_first_frame_until_the_buffers_are_recomputed(fus):
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    t = fus.RenderTarget(W, H)
    p = fus.RenderCloudParams()
    assert fus.lib.dms_fusion_render_cloud(t.h, g.h, 0, C.byref(p), None) != 0, "no feedback inputs before the first frame"
    first = last = None
    for k in range(3):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
        if k == 0:
            first = _inputs(g)
    last = _inputs(g)
    pose = np.array(r.pose, np.float32).reshape(4, 4)
    mvp = R.mvp_from_pose(_proj(W, H), pose)
    assert not np.array_equal(first[1], last[1])
    for inp in (first, last):
        t.clear(CLEAR)
        g.renderCloud(t, RC.RAW, mvp, pose, 2)
        _same(t.images(), _ref(W, H, [(inp[0], inp[1], mvp, pose, 2)]).images(), "first" if inp is first else "recomputed")
        g.computeFeedbackBuffers()
    t.close()
    g.close()


def test_errors_on_a_live_context_and_target(fus, grown):
    """the conditions the argument checks cannot reach with fake handles: a draw inside a frame, more than DMS_RENDER_MAX_DRAWS draws
    since the clear, an image with padded rows; each returns an error and leaves the target as it was"""
    from densemonoslam_amd import capi, synth

    g, pose, inp, _ = grown
    mvp = R.mvp_from_pose(_proj(64, 48), pose)
    t = fus.RenderTarget(64, 48)
    t.clear(CLEAR)
    for k in range(255):  # DMS_RENDER_MAX_DRAWS cloud draws fill the key's draw_seq byte
        g.renderCloud(t, k & 1, mvp, pose, 2)
    full = t.images()
    seq = (full[2][full[2] != R.CLEARED] >> np.uint64(32)) & np.uint64(0xFF)
    assert seq.max() <= 254
    with pytest.raises(capi.DmsError):
        g.renderCloud(t, RC.RAW, mvp, pose, 2)
    with pytest.raises(capi.DmsError):
        fus.render_cloud(t, inp[0], inp[1], K, MAXD, mvp, pose, 2)
    _same(t.images(), full, "after the refused draws")
    t.clear(CLEAR)
    g.renderCloud(t, RC.RAW, mvp, pose, 2)  # a clear makes room again
    one = t.images()
    assert (one[1] < 0xFFFFFF).any()
    # padded rows: a view of the same pixels with a pitch of 16 bytes more
    dm = fus.DeviceImage.from_array(inp[1])
    padded = fus.Image2D(C.c_void_p(dm.buf.ptr), W * 4 + 16, H - 1, W)
    rgba = fus.DeviceImage.from_array(inp[0])
    shorter = fus.Image2D(C.c_void_p(rgba.buf.ptr), W * 4, H - 1, W)
    p, cam = fus._cloud_params(mvp, pose, 2, None, None), fus.Camera(*K)
    assert fus.lib.dms_render_cloud(t.h, C.byref(shorter), C.byref(padded), C.byref(cam), MAXD, C.byref(p), None) != 0
    # inside a frame
    g2 = fus.ElasticFusion(W, H, K, model_capacity=400000)
    d, rgb, _ = synth.frame(0, width=W, height=H, K=K, noise=True)
    g2.processFrame(rgb, d)
    d, rgb, _ = synth.frame(1, width=W, height=H, K=K, noise=True)
    g2.processFrameBegin(rgb, d)
    with pytest.raises(capi.DmsError):
        g2.renderCloud(t, RC.RAW, mvp, pose, 2)
    g2.processFrameEnd()
    g2.fetch()
    _same(t.images(), one, "after the draws refused for a padded image and inside a frame")
    g2.renderCloud(t, RC.RAW, mvp, pose, 2)  # between frames again: drawn
    assert not np.array_equal(t.images()[2], one[2])
    g2.close()
    t.close()


def test_clouds_against_the_reference_programs_on_llvmpipe(fus):
    """HIP against tests/golden/ref_render_cloud.npz (vertex_feedback.* + draw_feedback.* on Mesa llvmpipe): equal to the restatement
    bit for bit, hence exactly the restatement's counted mismatches, which stay inside the bounds of the CPU test"""
    z = np.load(GOLDEN)
    k, maxd = tuple(float(v) for v in z["K"]), float(z["max_depth"])
    for name in (str(n) for n in z["cases"]):
        c = RC.fixture_case(z, name)
        h, w = z[name + "__depth"].shape
        t = fus.RenderTarget(w, h)
        t.clear(tuple(z["clear"]))
        fus.render_cloud(t, z["rgba"], z["depth_raw"] if c["buffer"] == "RAW" else z["depth_filtered"], k, maxd, z[c["view"] + "__mvp"],
                         z["pose"], c["color_type"])
        got = t.images()
        t.close()
        exp = RC.fixture_run(z, name)
        _same(got, exp, name)
        sg, sr = R.fixture_stats(z, name, got[0], got[1]), R.fixture_stats(z, name, exp[0], exp[1])
        print(name, sg)
        assert sg == sr, (name, sg, sr)
        RC.check_fixture_stats(z, name, sg)
