"""The view's image panels (include/dmslam_render_panels.h: normaliseDepth, renderDepth, displayImg's blit and the fused column) on
the MI355X against the CPU restatement tests/render_panels_ref.py, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cloud_ref as RC  # noqa: E402
import render_panels_ref as P  # noqa: E402
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 320, 240
K = (264.0, 264.0, 160.0, 120.0)
FRAMES = 8
CONFIDENCE = 2.0  # the surfels of an 8-frame map pass it, so the ACTIVE prediction is populated
CUT = 3.0
CLEAR = (0.1, 0.2, 0.3, 1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render_panels.npz")
F = np.float32
MIN_VAL = float(F(0.3) * F(1000))


def _max_val(cut):
    return float(F(cut) * F(1000))


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


def _sources(g):
    """(colour, raw depth, ACTIVE prediction's colour, ACTIVE prediction's vertex): images 0, 1, 9, 10"""
    return g.image(0), g.image(1), g.image(9), g.image(10)


@pytest.fixture(scope="module")
def grown(fus):
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000, confidence=CONFIDENCE)
    for k in range(FRAMES):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
    src = _sources(g)
    z = src[3][..., 2]
    assert ((z > 0) & (z <= CUT)).sum() > 5000 and (z <= 0).sum() > 100, "the prediction must be populated and have holes"
    yield g, np.array(r.pose, np.float32).reshape(4, 4), src
    g.close()


def _eq(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, "%s differs at %d places, first %s: %s vs %s" % (what, len(bad), bad[:3].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def _same_target(got, exp, what=""):
    for name, a, b in zip(("colour", "depth24", "winner"), got, exp):
        _eq(a, b, what + " " + name)


# viewports of a 640 x 480 target for a 320 x 240 image: magnified by a non-integer ratio into a corner, minified, 1:1, one row high
VIEWPORTS = {"mag_corner": (640 - 417, 480 - 313, 417, 313), "min": (5, 7, 213, 131), "same": (0, 0, 320, 240), "strip": (100, 479, 333, 1),
             "column": (639, 0, 1, 480)}


def test_both_shader_passes(fus, grown):
    g, _, (rgba, depth, pimg, vertex) = grown
    p = fus.Panels(W, H)
    for cut in (CUT, 1.7, 25.0):
        p.normaliseDepth(depth, MIN_VAL, _max_val(cut))
        p.renderDepth(vertex, cut)
        norm, model = p.images()
        _eq(norm, P.depth_norm(depth, MIN_VAL, _max_val(cut)), "DEPTH_NORM cut %g" % cut)
        _eq(model, P.model_depth_image(vertex, cut), "Model cut %g" % cut)
        assert (norm > 0).sum() > 1000 and (model[..., 3] > 0).sum() > 1000
    p.close()


@pytest.mark.parametrize("vp", sorted(VIEWPORTS))
@pytest.mark.parametrize("filt", [P.NEAREST, P.LINEAR])
@pytest.mark.parametrize("fmt", [P.RGBA8, P.L8])
def test_blit(fus, grown, fmt, filt, vp):
    g, _, (rgba, depth, pimg, vertex) = grown
    img = rgba if fmt == P.RGBA8 else P.depth_norm(depth, MIN_VAL, _max_val(CUT))
    for color in ((1.0, 1.0, 1.0), (1.0, 0.5, 0.6)):
        t = fus.RenderTarget(640, 480)
        t.clear(CLEAR)
        fus.render_blit(t, img, fmt, filt, VIEWPORTS[vp], color)
        got = t.images()
        t.close()
        ref = R.Target(640, 480, CLEAR)
        P.blit(ref, img, fmt, filt, VIEWPORTS[vp], color)
        _same_target(got, ref.images(), "%s %s" % (vp, color))
        assert (got[1] == 0xFFFFFF).all() and (got[2] == R.CLEARED).all(), "a blit writes colour only"


def _column(w=213, h=160, x0=0, y0=0):
    """the reference's column: four panels of one size stacked from the top of the target down"""
    return [(x0, y0 + (3 - k) * h, w, h) for k in range(4)]


@pytest.mark.parametrize("case", ["column", "strip", "overlap", "subset"])
def test_fused_column_equals_the_separate_calls(fus, grown, case):
    g, _, (rgba, depth, pimg, vertex) = grown
    tw, th, mask = 640, 640, 15
    if case == "column":
        vps = _column()
    elif case == "strip":
        tw, th, vps = 1024, 320, [(256 * k, 0, 256, 320) for k in range(4)]
    elif case == "overlap":  # a pixel of two viewports shows the later panel
        vps = [(0, 0, 400, 300), (200, 150, 417, 313), (100, 100, 213, 131), (150, 120, 320, 240)]
    else:
        vps, mask = _column(), 0b1010
    a, b = fus.RenderTarget(tw, th), fus.RenderTarget(tw, th)
    pa, pb = fus.Panels(W, H), fus.Panels(W, H)
    a.clear(CLEAR)
    b.clear(CLEAR)
    g.drawPanels(a, pa, vps, CUT, mask)
    g.drawPanelsSeparately(b, pb, vps, CUT, mask)
    ga, gb = a.images(), b.images()
    _same_target(ga, gb, case)
    na, nb = pa.images(), pb.images()
    _eq(na[0], nb[0], "DEPTH_NORM")
    _eq(na[1], nb[1], "Model")
    ref = R.Target(tw, th, CLEAR)
    norm, model = P.draw_panels(ref, rgba, depth, pimg, vertex, vps, CUT, mask)
    _same_target(ga, ref.images(), case + " against the restatement")
    _eq(na[0], norm, "DEPTH_NORM against the restatement")
    _eq(na[1], model, "Model against the restatement")
    for t in (a, b, pa, pb):
        t.close()


def test_operators_on_images_of_another_size(fus):
    rng = np.random.default_rng(11)
    w, h = 97, 51  # odd: the passes' last quad is partial, and the u16 rows of an offset view are not 8-byte aligned
    depth = rng.integers(0, 5000, (h, w)).astype(np.uint16)
    depth[::5] = 0
    depth[2, :8] = (299, 300, 301, 2999, 3000, 3001, 65535, 1)
    vertex = rng.uniform(-1, 4, (h, w, 4)).astype(np.float32)
    vertex[3, ::3, 2] = np.nan
    vertex[4, ::3, 2] = np.inf
    vertex[5, ::3, 2] = -np.inf
    vertex[6, :4, 2] = (0.0, -0.0, 3.0, np.nextafter(F(3.0), F(4.0)))
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    p = fus.Panels(w, h)
    for lo, hi, cut in ((300.0, 3000.0, 3.0), (0.0, 70000.0, 0.5), (-5.0, np.nan, np.nan), (10.5, 4999.5, 0.0)):
        p.normaliseDepth(depth, lo, hi)
        p.renderDepth(vertex, cut)
        norm, model = p.images()
        _eq(norm, P.depth_norm(depth, lo, hi), "DEPTH_NORM %s" % ((lo, hi),))
        _eq(model, P.model_depth_image(vertex, cut), "Model %g" % cut)
    p.normaliseDepth(depth, 300.0, 3000.0)
    norm = p.images()[0]
    t = fus.RenderTarget(256, 200)
    ref = R.Target(256, 200, CLEAR)
    t.clear(CLEAR)
    for im, fmt, filt, vp in ((rgba, P.RGBA8, P.LINEAR, (3, 4, 250, 190)), (norm, P.L8, P.LINEAR, (0, 0, 60, 31)),
                              (rgba, P.RGBA8, P.NEAREST, (100, 100, 97, 51)), (norm, P.L8, P.NEAREST, (10, 150, 33, 50))):
        fus.render_blit(t, im, fmt, filt, vp)
        P.blit(ref, im, fmt, filt, vp)
    p.blit(t, fus.PANEL_DEPTH_NORM, (200, 0, 56, 40))
    P.blit(ref, norm, P.L8, P.LINEAR, (200, 0, 56, 40))
    _same_target(t.images(), ref.images(), "another size")
    # a view that starts one pixel into the u16 buffer: the scalar path of the pass
    d2 = fus.DeviceImage.from_array(np.concatenate([[0], depth.reshape(-1)]).astype(np.uint16).reshape(1, -1))
    view = fus.Image2D(C.c_void_p(d2.buf.ptr + 2), w * 2, h, w)
    fus.check(fus.lib.dms_depth_norm(p.h, C.byref(view), 300.0, 3000.0, None), "dms_depth_norm")
    _eq(p.images()[0], norm, "unaligned rows")
    t.close()
    p.close()


def test_degenerate_inputs(fus, grown):
    """all-zero depth and a prediction with no valid vertex: both intermediates zero, the panels black (alpha 255 / 0)"""
    g, _, (rgba, depth, pimg, vertex) = grown
    zd, zv = np.zeros((H, W), np.uint16), np.zeros((H, W, 4), np.float32)
    zv[..., 2] = np.where(np.arange(W) % 2, 3.5, -1.0)
    p = fus.Panels(W, H)
    p.normaliseDepth(depth, MIN_VAL, _max_val(CUT))  # non-zero first: the passes must overwrite
    p.renderDepth(vertex, CUT)
    p.normaliseDepth(zd, MIN_VAL, _max_val(CUT))
    p.renderDepth(zv, CUT)
    norm, model = p.images()
    assert not norm.any() and not model.any()
    t = fus.RenderTarget(300, 200)
    t.clear(CLEAR)
    p.blit(t, fus.PANEL_DEPTH_NORM, (0, 0, 150, 200))
    p.blit(t, fus.PANEL_MODEL, (150, 0, 150, 200))
    c = t.images()[0]
    ref = R.Target(300, 200, CLEAR)
    P.blit(ref, norm, P.L8, P.LINEAR, (0, 0, 150, 200))
    P.blit(ref, model, P.RGBA8, P.NEAREST, (150, 0, 150, 200))
    _eq(c, ref.color, "degenerate")
    assert (c[:, :150] == (0, 0, 0, 255)).all() and (c[:, 150:] == 0).all()
    t.close()
    p.close()


def _proj(w, h):
    from densemonoslam_amd import fusion

    f = K[0] * w / W
    return fusion.render_frustum(w, h, f, f, w / 2.0, h / 2.0, 0.1, 1000.0)


def test_panels_compose_with_the_map_draw_and_the_cloud(fus, grown):
    """one frame of the window: clear, the map, a cloud, then the panel column into one target; then a further map draw, which still
    recolours the panel pixels it wins (the blit left depth and winner alone)"""
    g, pose, (rgba, depth, pimg, vertex) = grown
    recs = g.globalModel().downloadMap()
    tw, th = 640, 480
    mvp = R.mvp_from_pose(_proj(tw, th), pose)
    vps = _column(160, 120)
    g.computeFeedbackBuffers()
    t, p = fus.RenderTarget(tw, th), fus.Panels(W, H)
    t.clear(CLEAR)
    t.draw(g.globalModel(), mvp, threshold=CONFIDENCE, color_type=2)
    g.renderCloud(t, RC.RAW, mvp, pose, 1)
    before = t.images()
    g.drawPanels(t, p, vps, CUT)
    mid = t.images()
    ref = R.Target(tw, th, CLEAR)
    ref.draw(recs, mvp, threshold=CONFIDENCE, color_type=2)
    RC.draw_cloud(ref, g.image(0), g.image(3), K, 25.0, mvp, pose, 1)
    P.draw_panels(ref, rgba, depth, pimg, vertex, vps, CUT)
    _same_target(mid, ref.images(), "map + cloud + panels")
    _eq(mid[1], before[1], "depth after the panels")
    _eq(mid[2], before[2], "winner after the panels")
    assert (mid[0][:, :160] != before[0][:, :160]).any() and (mid[0][:, 160:] == before[0][:, 160:]).all()
    # a later draw of every surfel, unstable ones too, as points: wins pixels inside the panel region as well
    t.draw(g.globalModel(), mvp, threshold=0.0, draw_points=True, color_type=1)
    ref.draw(recs, mvp, threshold=0.0, draw_points=True, color_type=1)
    after = t.images()
    _same_target(after, ref.images(), "a map draw over the panels")
    seq = (after[2][:, :160] >> np.uint64(32)) & np.uint64(0xFF)
    assert ((seq == 2) & (after[2][:, :160] != R.CLEARED)).any(), "the later draw must own pixels of the panel region"
    t.close()
    p.close()


def _run_frames(fus, panels):
    from densemonoslam_amd import synth

    g = fus.ElasticFusion(W, H, K, model_capacity=400000, confidence=CONFIDENCE)
    t, p = fus.RenderTarget(640, 640), fus.Panels(W, H)
    poses = []
    for k in range(8):
        d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
        r = g.processFrame(rgb, d)
        poses.append(np.array(r.pose, np.float32).tobytes())
        if panels:
            g.drawPanels(t, p, _column(), CUT)
    recs = g.globalModel().downloadMap()
    img = t.images()
    t.close()
    p.close()
    g.close()
    return poses, recs, img


def test_panels_between_frames_change_nothing(fus):
    base_p, base_m, _ = _run_frames(fus, False)
    p, m, img = _run_frames(fus, True)
    assert img[0].any()
    assert p == base_p
    assert len(m) == len(base_m)
    for f in ("pos", "col", "nrm", "times"):
        assert np.array_equal(m[f].view(np.uint32), base_m[f].view(np.uint32)), f


def test_errors_on_a_live_context(fus, grown):
    from densemonoslam_amd import capi, synth

    g, _, (rgba, depth, pimg, vertex) = grown
    t, p = fus.RenderTarget(200, 150), fus.Panels(W, H)
    t.clear(CLEAR)
    g.drawPanels(t, p, _column(50, 37), CUT)
    ok, okp = t.images(), p.images()
    white = (C.c_float * 3)(1, 1, 1)
    img = fus.DeviceImage.from_array(rgba)
    # viewports that are empty or leave the target
    for vp in ((0, 0, 0, 10), (0, 0, 10, 0), (-1, 0, 10, 10), (0, -1, 10, 10), (191, 0, 10, 10), (0, 141, 10, 10), (0, 0, 201, 150), (0, 0, 10, -3),
               (2 ** 31 - 5, 0, 10, 10)):
        with pytest.raises(capi.DmsError):
            fus.render_blit(t, img, P.RGBA8, P.NEAREST, vp)
        with pytest.raises(capi.DmsError):
            g.drawPanels(t, p, [vp] * 4, CUT)
        with pytest.raises(capi.DmsError):
            g.drawPanels(t, p, _column(50, 37)[:3] + [vp], CUT, 8)
    g.drawPanels(t, p, [(0, 0, 0, 0)] * 3 + [_column(50, 37)[3]], CUT, 8)  # viewports outside the mask are not read
    # formats, filters, masks, shapes, padded rows, null images
    vp = fus.Viewport(0, 0, 10, 10)
    for fmt, filt in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert fus.lib.dms_render_blit(t.h, img.ref, fmt, filt, C.byref(vp), white, None) != 0
    padded = fus.Image2D(C.c_void_p(img.buf.ptr), W * 4 + 16, H - 1, W)
    empty = fus.Image2D(C.c_void_p(img.buf.ptr), 0, 0, 0)
    null = fus.Image2D(None, W * 4, H, W)
    for bad in (padded, empty, null):
        assert fus.lib.dms_render_blit(t.h, C.byref(bad), 0, 0, C.byref(vp), white, None) != 0
        assert fus.lib.dms_depth_norm(p.h, C.byref(bad), 300.0, 3000.0, None) != 0
        assert fus.lib.dms_model_depth_image(p.h, C.byref(bad), 3.0, None) != 0
    for mask in (-1, 16):
        with pytest.raises(capi.DmsError):
            g.drawPanels(t, p, _column(50, 37), CUT, mask)
    small = fus.Panels(W // 2, H // 2)
    with pytest.raises(capi.DmsError):
        g.drawPanels(t, small, _column(50, 37), CUT)  # panels of another size than the context
    with pytest.raises(capi.DmsError):
        small.normaliseDepth(depth, 300.0, 3000.0)
    with pytest.raises(capi.DmsError):
        small.renderDepth(vertex, 3.0)
    small.close()
    # before the first frame, and inside a frame
    g2 = fus.ElasticFusion(W, H, K, model_capacity=400000)
    with pytest.raises(capi.DmsError):
        g2.drawPanels(t, p, _column(50, 37), CUT)
    d, rgb, _ = synth.frame(0, width=W, height=H, K=K, noise=True)
    g2.processFrame(rgb, d)
    d, rgb, _ = synth.frame(1, width=W, height=H, K=K, noise=True)
    g2.processFrameBegin(rgb, d)
    with pytest.raises(capi.DmsError):
        g2.drawPanels(t, p, _column(50, 37), CUT)
    g2.processFrameEnd()
    g2.fetch()
    _same_target(t.images(), ok, "after the refused calls")
    _eq(p.images()[0], okp[0], "DEPTH_NORM after the refused calls")
    _eq(p.images()[1], okp[1], "Model after the refused calls")
    g2.drawPanels(t, p, _column(50, 37), CUT)  # between frames again: drawn
    assert not np.array_equal(t.images()[0], ok[0])
    g2.close()
    t.close()
    p.close()


def test_panels_against_the_reference_programs_on_llvmpipe(fus):
    """HIP against tests/golden/ref_render_panels.npz (depth_norm.frag, visualise_textures.frag and a textured quad on Mesa llvmpipe):
    equal to the restatement bit for bit, hence exactly the restatement's counted mismatches, inside the bounds of the CPU test"""
    z = np.load(GOLDEN)
    h, w = z["depth"].shape
    cut = float(z["depth_cutoff"])
    p = fus.Panels(w, h)
    p.normaliseDepth(z["depth"], MIN_VAL, _max_val(cut))
    p.renderDepth(z["vertex"], cut)
    norm, model = p.images()
    p.close()
    _eq(norm, P.depth_norm(z["depth"], MIN_VAL, _max_val(cut)), "DEPTH_NORM")
    _eq(model, P.model_depth_image(z["vertex"], cut), "Model")
    print("depth_norm", P.check_fixture("depth_norm", z["depth_norm"], norm), "model", P.check_fixture("model", z["model"], model))
    for name in (str(n) for n in z["cases"]):
        c = P.fixture_case(z, name)
        key, fmt = P.SOURCES[c["source"]]
        t = fus.RenderTarget(*c["target"])
        t.clear(tuple(z["clear"]))
        fus.render_blit(t, z[key], fmt, c["linear"], c["viewport"], c["color"])
        got = t.images()[0]
        t.close()
        _eq(got, P.fixture_blit(z, name), name)
        print(name, P.check_fixture(name, z[name + "__rgba"], got))
