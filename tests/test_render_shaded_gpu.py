"""The shaded map view (include/dmslam_render_shaded.h, GUI::drawFXAA) on the MI355X against the CPU restatement
tests/render_shaded_ref.py, bit for bit: the offscreen float colour, depth and winner key, and the view's colour bytes, depth and
winner key after the FXAA composite and the depth blit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402
import render_shaded_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 320, 240
K = (264.0, 264.0, 160.0, 120.0)
FRAMES = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render_shaded.npz")
MAP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render.npz")


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


def _poses(pose):
    oblique = pose.copy()
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique[:3, :3] = pose[:3, :3] @ Ry
    oblique[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(1.2)  # surfels across the near plane and behind the eye
    close = pose.copy()
    close[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(0.8)
    return {"tracked": pose, "oblique": oblique, "closeup": close}


# name -> (offscreen w, h, view w, h, focal length at the offscreen size, near)
SIZES = {"down": (480, 360, 320, 240, 396.0, 0.1), "up": (160, 120, 320, 240, 132.0, 0.1)}


def _same(a, b):
    """equal bits, or NaN on both sides (a NaN's payload is not a result)"""
    if a.dtype == np.float32:
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _assert_same(got, exp, names):
    for name, a, b in zip(names, got, exp):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        bad = np.argwhere(~_same(a, b).reshape(a.shape[0], a.shape[1], -1).all(-1))
        assert len(bad) == 0, "%s differs at %d places, first %s: %s vs %s" % (name, len(bad), bad[:3].tolist(), a[tuple(bad[0])],
                                                                             b[tuple(bad[0])])


def _check(fus, model, recs, size, pose, p, view_clear=(0.1, 0.2, 0.3, 1.0), pose_ptr=None, then=None):
    """Stage A and B of one shaded view on the GPU and in the restatement; `then`: draws (render_ref parameters) into the view
    after the composite.  Returns the GPU's (offscreen images, view images)."""
    sw, sh, w, h, f, near = size
    proj = _proj(sw, sh, f=f, near=near)
    mvp = R.mvp_from_pose(proj, pose)
    v = fus.ShadedView(w, h, offscreen=(sw, sh))
    v.clear(view_clear)
    if pose_ptr is not None:
        v.draw(model, proj, pose_dev=C.c_void_p(pose_ptr), **p)
    else:
        v.draw(model, mvp, **p)
    v.fxaa()
    ref_off = S.Offscreen(sw, sh)
    ref_off.draw(recs, mvp, **p)
    ref = R.Target(w, h, view_clear)
    S.composite(ref, ref_off)
    for q in then or []:
        vm = R.mvp_from_pose(_proj(w, h, f=f * w / sw, near=near), pose)
        v.target.draw(model, vm, **q)
        ref.draw(recs, vm, **q)
    off = v.offscreen_images()
    img = v.images()
    v.close()
    _assert_same(off, ref_off.images(), ("offscreen rgba32f", "offscreen depth24", "offscreen winner"))
    _assert_same(img, ref.images(), ("view rgba8", "view depth24", "view winner"))
    return off, img


def _light(pose):
    """the GUI's lightpos: the translation column of the view matrix (F * inverse(pose))"""
    return R.mvp_from_pose(np.eye(4, dtype=np.float32), pose)[:3, 3]


MATRIX = [
    dict(color_type=0, draw_unstable=True),
    dict(color_type=0, threshold="median"),
    dict(color_type=1, draw_unstable=True, sign_mult=1.0),
    dict(color_type=2, threshold="median", draw_unstable=True),
    dict(color_type=3, time=FRAMES, draw_unstable=True),
    dict(color_type=2, draw_window=True, time=FRAMES + 1, time_idx=0, time_delta=2, draw_unstable=True, sign_mult=1.0),
    dict(color_type=0, draw_window=True, time=3, time_idx=0, time_delta=1, clear_rgba=(1.0, 1.0, 1.0, 0.0)),
]


def _params(p, recs, pose):
    p = dict(p)
    p.setdefault("sign_mult", -1.0)
    p.setdefault("clear_rgba", (0.05, 0.05, 0.3, 0.0))
    p["light_pos"] = _light(pose)
    if p.get("threshold") == "median":  # a threshold that splits the map into stable and unstable surfels
        p["threshold"] = float(np.median(recs["pos"][:, 3]))
    return p


@pytest.mark.parametrize("view", ["tracked", "oblique", "closeup"])
@pytest.mark.parametrize("case", range(len(MATRIX)))
def test_shaded_view_matches_the_restatement(fus, grown, view, case):
    g, pose, recs = grown
    vp = _poses(pose)[view]
    size = SIZES["down"] if view != "closeup" else (480, 360, 320, 240, 2400.0, 0.1)
    off, img = _check(fus, g.globalModel(), recs, size, vp, _params(MATRIX[case], recs, vp))
    assert (off[1] < 0xFFFFFF).sum() > 0, "nothing drawn"


@pytest.mark.parametrize("case", [0, 3])
def test_offscreen_smaller_than_the_view(fus, grown, case):
    g, pose, recs = grown
    _check(fus, g.globalModel(), recs, SIZES["up"], pose, _params(MATRIX[case], recs, pose))


def test_oblique_view_resolves_clipped_winners(fus, grown):
    """discs across the near plane right in front of the camera (as in test_render_gpu): the per-pixel resolve must rebuild the fan
    pieces of clipped triangles"""
    _, _, recs = grown
    few = recs[:3].copy()
    few["pos"][:, :3] = [[0.0, 0.0, 0.1], [0.03, 0.02, 0.12], [0.0, 0.0, -0.5]]
    few["pos"][:, 3] = 20.0
    few["nrm"][:, :3] = np.float32(np.sqrt(0.5)) * np.array([1.0, 0.0, -1.0], np.float32)
    few["nrm"][:, 3] = 0.1
    m = fus.GlobalModel(W, H, capacity=64)
    m.upload(few)
    eye = np.eye(4, dtype=np.float32)
    size = (480, 360, 320, 240, 396.0, 0.1)
    off, _ = _check(fus, m, few, size, eye, _params(dict(color_type=2, draw_unstable=True), few, eye))
    key = off[2]
    ids = (key[key != R.CLEARED] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert len(ids) > 100
    assert not np.isnan(off[0][off[1] < 0xFFFFFF]).any()
    m.close()


def test_empty_map_and_single_surfel(fus, grown):
    _, pose, recs = grown
    m = fus.GlobalModel(W, H, capacity=1024)
    size = SIZES["down"]
    off, img = _check(fus, m, recs[:0], size, pose, _params(dict(color_type=2), recs, pose))
    assert (off[1] == 0xFFFFFF).all() and (img[2] == R.CLEARED).all()
    one = recs[len(recs) // 2:len(recs) // 2 + 1].copy()
    m.upload(one)
    off, _ = _check(fus, m, one, size, pose, _params(dict(color_type=2, draw_unstable=True), one, pose))
    assert (off[1] < 0xFFFFFF).sum() > 0
    m.close()


def test_draw_after_the_composite_tests_against_the_blitted_depth(fus, grown):
    """a renderPointCloud draw into the view after the composite: GL_LESS against the blitted depth, the composite winning ties"""
    g, pose, recs = grown
    sw, sh, w, h, f, near = SIZES["down"]
    off, img = _check(fus, g.globalModel(), recs, SIZES["down"], pose, _params(MATRIX[0], recs, pose),
                      then=[dict(color_type=2, cluster_color=(1.0, 0.0, 0.0), draw_unstable=True)])
    seq = (img[2][img[2] != R.CLEARED] >> np.uint64(32)) & np.uint64(0xFF)
    assert (seq == 0).any() and (seq == 1).any(), "both the composite and the later draw must own pixels"


def test_pose_dev_equals_host_composed_mvp(fus, grown):
    g, pose, recs = grown
    p = _params(MATRIX[3], recs, pose)
    dev = _check(fus, g.globalModel(), recs, SIZES["down"], pose, p, pose_ptr=g.poseDevice())
    host = _check(fus, g.globalModel(), recs, SIZES["down"], pose, p)
    for a, b in zip(dev[0] + dev[1], host[0] + host[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_drawFXAA_takes_the_reference_arguments(fus, grown):
    """ShadedView.drawFXAA(mvp, mv, model, threshold, time, timeIdx, timeDelta, invertNormals, toggles) = stage A + B with the
    GUI's derived uniforms (lightpos, signMult, colorType, clear colour)"""
    g, pose, recs = grown
    sw, sh, w, h, f, near = SIZES["down"]
    mvp = R.mvp_from_pose(_proj(sw, sh, f=f), pose)
    mv = R.mvp_from_pose(np.eye(4, dtype=np.float32), pose)
    thr = float(np.median(recs["pos"][:, 3]))
    v = fus.ShadedView(w, h, offscreen=(sw, sh))
    v.clear((0, 0, 0, 1))
    v.drawFXAA(mvp, mv, g.globalModel(), thr, FRAMES + 1, 0, 2, True, drawColors=True, drawUnstable=True, drawWindow=True)
    got = v.images()
    v.close()
    t = R.Target(w, h, (0, 0, 0, 1))
    S.drawFXAA(t, S.Offscreen(sw, sh), recs, mvp, mv, thr, FRAMES + 1, 0, 2, True, drawColors=True, drawUnstable=True, drawWindow=True)
    _assert_same(got, t.images(), ("view rgba8", "view depth24", "view winner"))


def test_default_offscreen_is_the_gui_size(fus):
    v = fus.ShadedView(64, 48)
    w, h = C.c_int(), C.c_int()
    fus.check(fus.lib.dms_render_offscreen_size(v.h, C.byref(w), C.byref(h)), "dms_render_offscreen_size")
    assert (w.value, h.value) == (3840, 2160) == fus.OFFSCREEN_SIZE
    off = v.offscreen_images()
    assert off[0].shape == (2160, 3840, 4) and (off[1] == 0xFFFFFF).all() and (off[2] == R.CLEARED).all()
    v.close()


def _run_frames(fus, shaded):
    """8 frames; shaded: a drawFXAA on the frame's stream between frames, from the tracked pose in HBM"""
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000)
    v = fus.ShadedView(W, H, offscreen=(640, 480))
    poses = []
    proj = _proj(640, 480, f=528.0)
    for k in range(8):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
        poses.append(np.array(r.pose, np.float32).tobytes())
        if shaded:
            v.clear((0, 0, 0, 1))
            v.draw(g.globalModel(), proj, light_pos=(0.1, 0.2, 0.3), threshold=1.0, draw_unstable=True, color_type=2,
                   pose_dev=C.c_void_p(g.poseDevice()))
            v.fxaa()
    recs = g.globalModel().downloadMap()
    v.images()
    v.close()
    g.close()
    return poses, recs


def test_shaded_views_between_frames_change_nothing(fus):
    base_p, base_m = _run_frames(fus, False)
    p, m = _run_frames(fus, True)
    assert p == base_p
    assert len(m) == len(base_m)
    for f in ("pos", "col", "nrm", "times"):
        assert np.array_equal(m[f].view(np.uint32), base_m[f].view(np.uint32)), f


def test_shaded_view_against_the_reference_programs_on_llvmpipe(fus):
    """HIP against tests/golden/ref_render_shaded.npz (the reference's drawFXAA programs on Mesa llvmpipe) by the bounds of the CPU
    test, and equal to the restatement bit for bit on the same map"""
    z = np.load(GOLDEN)
    s = R.fixture_map(np.load(MAP))
    m = fus.GlobalModel(W, H, capacity=len(s) + 16)
    m.upload(s)
    for name in (str(n) for n in z["cases"]):
        sh, sw = z[name + "__off_depth"].shape
        h, w = z[name + "__depth"].shape
        p = S.fixture_params(z, name)
        v = fus.ShadedView(w, h, offscreen=(sw, sh))
        v.clear(tuple(z["view_clear"]))
        v.draw(m, z[name + "__mvp"], light_pos=z[name + "__mv"][:3, 3], **p)
        v.fxaa()
        off, img = v.offscreen_images(), v.images()
        v.close()
        ref_off, ref = S.fixture_run(z, name, s)
        _assert_same(off, ref_off.images(), ("offscreen rgba32f", "offscreen depth24", "offscreen winner"))
        _assert_same(img, ref.images(), ("view rgba8", "view depth24", "view winner"))
        S.check_fixture_stats(name, S.fixture_stats(z, name, off[0], off[1], img[0], img[1]))
    m.close()
