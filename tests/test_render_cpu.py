"""CPU checks of the map draw (include/dmslam_render.h): the header stands alone in C99 and C++11, every entry point is exported,
bad arguments are refused before any device access, and the restatement (tests/render_ref.py) keeps the rasteriser rules
DESIGN.md §4 R6-R10 states."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmslam_render.h")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dms_render_[a-zA-Z0-9_]+)\s*\(", text)))


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_on_its_own(compiler, std, ext):
    if shutil.which(compiler) is None:
        pytest.skip("%s not available" % compiler)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "h." + ext)
        with open(src, "w") as f:
            f.write('#include "dmslam_render.h"\nint main(void) { dms_render_params p; (void)p; return 0; }\n')
        subprocess.check_call([compiler, std, "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o",
                               os.path.join(d, "h.o")])


def test_every_entry_point_is_exported():
    from densemonoslam_amd import capi

    names = _declared()
    assert {"dms_render_target_create", "dms_render_target_destroy", "dms_render_clear", "dms_render_draw", "dms_render_images",
            "dms_render_frustum", "dms_render_mvp_from_pose"} <= set(names)
    assert not [n for n in names if not hasattr(capi.lib, n)]


def test_bad_arguments_are_refused_without_a_device():
    from densemonoslam_amd import capi, fusion

    lib = capi.lib
    h = C.c_void_p()
    assert lib.dms_render_target_create(None, 64, 64) == -1
    for w, hh in ((0, 64), (64, 0), (-1, 5), (8193, 16), (16, 8193)):
        assert lib.dms_render_target_create(C.byref(h), w, hh) == -1, (w, hh)
        assert h.value is None
    c = (C.c_float * 4)()
    assert lib.dms_render_clear(None, c, None) == -1
    p = fusion.RenderParams()
    assert lib.dms_render_draw(None, None, C.byref(p), None) == -1
    assert lib.dms_render_images(None, None, None, None) == -1
    # a fake, non-null target and map: the parameter checks come first and never touch them
    fake = C.c_void_p(16)
    for field, value in (("color_type", 5), ("color_type", -1), ("time_idx", 8), ("time_idx", -1)):
        q = fusion.RenderParams()
        setattr(q, field, value)
        assert lib.dms_render_draw(fake, fake, C.byref(q), None) == -1, (field, value)
    assert lib.dms_render_draw(fake, fake, None, None) == -1
    out = (C.c_float * 16)()
    assert lib.dms_render_frustum(0, 10, 1.0, 1.0, 0.0, 0.0, 0.1, 10.0, out) == -1
    assert lib.dms_render_frustum(10, 10, 1.0, 1.0, 0.0, 0.0, 0.1, 0.05, out) == -1


def test_frustum_and_view_composition_match_the_restatement():
    from densemonoslam_amd import fusion

    P = fusion.render_frustum(1024, 320, 420, 420, 512, 160, 0.1, 1000)
    n, f = 0.1, 1000.0
    assert P[0, 0] == np.float32(2 * 420 / 1024) and P[1, 1] == np.float32(2 * 420 / 320)
    assert P[2, 2] == np.float32(-(f + n) / (f - n)) and P[3, 2] == -1 and P[2, 3] == np.float32(-2 * f * n / (f - n))
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        a, b, c, d = q
        Rm = np.array([[1 - 2 * (c * c + d * d), 2 * (b * c - a * d), 2 * (b * d + a * c)],
                       [2 * (b * c + a * d), 1 - 2 * (b * b + d * d), 2 * (c * d - a * b)],
                       [2 * (b * d - a * c), 2 * (c * d + a * b), 1 - 2 * (b * b + c * c)]])
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = Rm
        T[:3, 3] = rng.normal(size=3)
        assert np.array_equal(fusion.render_mvp_from_pose(P, T).view(np.uint32), R.mvp_from_pose(P, T).view(np.uint32))


# ---- the restatement's own rules -------------------------------------------------------------------------------------------
def _surfels(pos, nrm, rad, conf=20.0, colour=0x336699):
    from densemonoslam_amd.fusion import SURFEL_DTYPE

    s = np.zeros(len(pos), SURFEL_DTYPE)
    s["pos"][:, :3] = pos
    s["pos"][:, 3] = conf
    n = np.asarray(nrm, np.float64)
    s["nrm"][:, :3] = n / np.linalg.norm(n, axis=1, keepdims=True)
    s["nrm"][:, 3] = rad
    s["col"][:, 0] = colour
    s["col"][:, 2] = 1
    s["times"][:] = -3
    s["times"][:, 0] = 1
    return s


def _ortho(W, H):
    """clip = (x, y, -z / 10, 1): window x = (x + 1) W / 2"""
    return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -0.1, 0], [0, 0, 0, 1]], np.float32)


def test_quad_diagonal_is_produced_once():
    # every fragment of the strip is produced by exactly one of its two triangles: a surfel drawn over an empty target covers the
    # same pixels as the union of its triangles, and no pixel of the diagonal is counted twice
    W = H = 64
    s = _surfels([[0.013, -0.021, -1.0]], [[0.1, 0.2, 1.0]], 0.6)
    M = _ortho(W, H)
    cv = R.disc_corners(M, s["pos"], s["nrm"])
    wv = [R.to_window(tuple(a for a in c), W, H) for c in cv]
    counts = np.zeros(W * H, np.int64)
    for tri in R.STRIP:
        zb = np.full(W * H, R.CLEARED, np.uint64)
        t = {}
        for slot, k in enumerate(tri):
            for name, val in zip(("X", "Y", "z", "iw"), wv[k]):
                t["v%d_%s" % (slot, name)] = val
            t["v%d_u" % slot] = np.zeros(1, np.float32)  # texcoord 0: no disc discard, the whole triangle
            t["v%d_v" % slot] = np.zeros(1, np.float32)
        R.raster_triangles(t, W, H, np.zeros(1, np.uint64), np.zeros(1, np.float32), zb)
        counts += zb != R.CLEARED
    assert counts.max() == 1 and counts.sum() > 100


def test_disc_area_and_ties():
    W = H = 200
    s = _surfels([[0.0, 0.0, -1.0]], [[0.0, 0.0, 1.0]], 0.5)
    t = R.Target(W, H)
    t.draw(s, _ortho(W, H), color_type=2)
    cov = t.depth < 0xFFFFFF
    # radius 0.5 in NDC = 50 px: pi r^2 within the rasterisation's half-pixel boundary
    assert abs(cov.sum() - np.pi * 50 ** 2) < 2 * np.pi * 50
    assert (t.color[cov] == np.array([0x33, 0x66, 0x99, 255], np.uint8)).all()
    # the same surfel drawn again at the same depth: the earlier draw keeps every pixel
    t.draw(s, _ortho(W, H), cluster_color=(1, 0, 0))
    assert (t.color[cov] == np.array([0x33, 0x66, 0x99, 255], np.uint8)).all()
    # two surfels at one depth in one draw: the smaller id wins
    two = np.concatenate([_surfels([[0.0, 0.0, -1.0]], [[0, 0, 1]], 0.3, colour=0xFF0000), _surfels([[0.0, 0.0, -1.0]], [[0, 0, 1]], 0.3,
                                                                                                   colour=0x00FF00)])
    t2 = R.Target(W, H)
    t2.draw(two, _ortho(W, H), color_type=2)
    ids = t2.key[t2.key != R.CLEARED] & np.uint64(0xFFFFFFFF)
    assert len(ids) and (ids == 0).all()


def test_unstable_depth_shift_is_clamped():
    W = H = 32
    # window z = 0.5 + z_ndc / 2 = 0.55; radius 0.6 pushes an unstable surfel past 1.0: it loses against the cleared buffer
    s = _surfels([[0.0, 0.0, -1.0]], [[0, 0, 1]], 0.6, conf=1.0)
    t = R.Target(W, H)
    t.draw(s, _ortho(W, H), threshold=5.0, draw_unstable=True)
    assert (t.depth == 0xFFFFFF).all()
    s = _surfels([[0.0, 0.0, -1.0]], [[0, 0, 1]], 0.3, conf=1.0)
    t.draw(s, _ortho(W, H), threshold=5.0, draw_unstable=True)
    d = t.depth[t.depth < 0xFFFFFF]
    # (the interpolated window z of a flat surfel may differ from the vertices' in the last bit)
    assert len(d) and (np.abs(d.astype(np.int64) - R.depth24(np.float32(np.float32(0.55) + np.float32(0.3)))) <= 1).all()
    # without drawUnstable a surfel with conf <= threshold is not drawn at all: a draw of it in front of everything changes no pixel
    before = t.images()
    front = _surfels([[0.0, 0.0, -0.2]], [[0, 0, 1]], 0.3, conf=1.0, colour=0xFF0000)
    t.draw(front, _ortho(W, H), threshold=5.0, draw_unstable=False, color_type=2)
    assert all(np.array_equal(a, b) for a, b in zip(before, t.images()))


GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_render.npz")


def fixture_cases():
    return [str(n) for n in np.load(GOLDEN)["cases"]]


@pytest.mark.parametrize("name", fixture_cases())
def test_restatement_against_the_reference_programs_on_llvmpipe(name):
    z = np.load(GOLDEN)
    s = R.fixture_map(z)
    h, w = z[name + "__depth"].shape
    t = R.Target(w, h, tuple(z["clear"]))
    for p in R.fixture_draws(z, name):
        t.draw(s, z[name + "__mvp"], **p)
    c, d, _ = t.images()
    st = R.fixture_stats(z, name, c, d)
    b = R.FIXTURE_BOUNDS
    assert st["covered"] > 0
    assert st["coverage"] <= b["coverage"] and st["colour"] <= b["colour"], st
    if "points" in name:
        assert st["depth"] <= b["depth_points"], st
    elif not name.startswith("oblique"):  # (the oblique view's depths are not pinned)
        assert st["depth"] <= b["depth_discs"], st


def test_contributions_of_an_unseen_surfel_and_the_time_ramp_at_time_1():
    s = _surfels([[0.0, 0.0, -1.0]], [[0, 0, 1]], 0.3)
    s["times"][:] = -3  # seen by no camera: 0 / 0
    c = R.surfel_colour(s, dict(color_type=4))
    assert np.isnan(c).all()
    assert (R.rgba8(c)[0] == [0, 0, 0, 255]).all()
    # the init-time ramp at time 1 divides by time - 1 = 0: initTime 1 gives ratio 0 / 0 = NaN, which max(0, .) turns into 0
    # (x = y = 0, z = 1, shaded by |n.1| + 0.1 = 1.1); a later initTime gives +inf (x = 0, y = +inf, z = -inf), and R9 writes 0 for
    # every channel that is not finite, as llvmpipe does (tests/golden/ref_render.npz, case tracked_times_at_1)
    s["col"][:, 2] = 1
    c = R.surfel_colour(s, dict(color_type=3, time=1))
    assert c[0].tolist() == [0.0, 0.0, float(np.float32(1.1))] and (R.rgba8(c)[0] == [0, 0, 255, 255]).all()
    s["col"][:, 2] = 3
    c = R.surfel_colour(s, dict(color_type=3, time=1))
    assert c[0, 0] == 0 and np.isposinf(c[0, 1]) and np.isneginf(c[0, 2])
    assert (R.rgba8(c)[0] == [0, 0, 0, 255]).all()
