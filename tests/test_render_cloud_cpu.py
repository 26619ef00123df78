"""CPU checks of the live-frame cloud draw (include/dmslam_render_cloud.h): the header stands alone in C99 and C++11, every entry point
is exported, bad arguments are refused before any device access, and the restatement (tests/render_cloud_ref.py) keeps the rules
DESIGN.md §4 R19-R21 states and holds the reference's own programs on llvmpipe (tests/golden/ref_render_cloud.npz)."""
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
import render_cloud_ref as RC  # noqa: E402
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmslam_render_cloud.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_render_cloud.npz")
F = np.float32


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_on_its_own(compiler, std, ext):
    if shutil.which(compiler) is None:
        pytest.skip("%s not available" % compiler)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "h." + ext)
        with open(src, "w") as f:
            f.write('#include "dmslam_render_cloud.h"\nint main(void) { dms_render_cloud_params p; (void)p; return DMS_CLOUD_RAW; }\n')
        subprocess.check_call([compiler, std, "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o",
                               os.path.join(d, "h.o")])


def test_every_entry_point_is_exported():
    from densemonoslam_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(dms_[a-zA-Z0-9_]+)\s*\(", text))
    assert names == {"dms_render_cloud", "dms_fusion_render_cloud", "dms_render_cloud_clip"}
    assert not [n for n in names if not hasattr(capi.lib, n)]


def test_bad_arguments_are_refused_without_a_device():
    from densemonoslam_amd import capi, fusion

    lib = capi.lib
    fake = C.c_void_p(16)  # a non-null target / context / pixel address the checks below never touch
    p = fusion.RenderCloudParams()
    img = fusion.Image2D(fake, 64 * 4, 48, 64)
    cam = fusion.Camera(100.0, 100.0, 32.0, 24.0)
    args = dict(t=fake, rgba=C.byref(img), depth=C.byref(img), cam=C.byref(cam), p=C.byref(p))
    for missing in args:
        a = dict(args, **{missing: None})
        assert lib.dms_render_cloud(a["t"], a["rgba"], a["depth"], a["cam"], 25.0, a["p"], None) == -1, missing
    for ct in (-1, 3, 4):
        q = fusion.RenderCloudParams()
        q.color_type = ct
        assert lib.dms_render_cloud(fake, C.byref(img), C.byref(img), C.byref(cam), 25.0, C.byref(q), None) == -1, ct
    for bad in (fusion.Image2D(fake, 64 * 4, 48, 32), fusion.Image2D(fake, 64 * 4 + 16, 48, 64), fusion.Image2D(None, 64 * 4, 48, 64),
                fusion.Image2D(fake, 0, 0, 0)):
        assert lib.dms_render_cloud(fake, C.byref(img), C.byref(bad), C.byref(cam), 25.0, C.byref(p), None) == -1
        assert lib.dms_render_cloud(fake, C.byref(bad), C.byref(img), C.byref(cam), 25.0, C.byref(p), None) == -1
    huge = fusion.Image2D(fake, 40000 * 4, 40000, 40000)  # more than DMS_CLOUD_MAX_PIXELS
    assert lib.dms_render_cloud(fake, C.byref(huge), C.byref(huge), C.byref(cam), 25.0, C.byref(p), None) == -1
    assert lib.dms_fusion_render_cloud(None, fake, 0, C.byref(p), None) == -1
    assert lib.dms_fusion_render_cloud(fake, None, 0, C.byref(p), None) == -1
    assert lib.dms_fusion_render_cloud(fake, fake, 0, None, None) == -1
    for which in (-1, 2):
        assert lib.dms_fusion_render_cloud(fake, fake, which, C.byref(p), None) == -1, which
    out = (C.c_float * 4)()
    assert lib.dms_render_cloud_clip(None, None, None, out) == -1


def _frame(rows=24, cols=32, seed=3):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.0, 3.0, (rows, cols)).astype(F)
    rgba = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    return rgba, depth, (40.0, 40.0, cols / 2.0, rows / 2.0)


def _own_view(rows, cols, K):
    """the frame's own projection at the identity pose: source pixel (x, y) lands in target pixel (x, rows - 1 - y)"""
    from densemonoslam_amd import fusion

    return R.mvp_from_pose(fusion.render_frustum(cols, rows, K[0], K[1], K[2], K[3], 0.1, 100.0), np.eye(4, dtype=F))


def test_zero_and_far_depths_are_not_emitted():
    rgba, depth, K = _frame()
    rows, cols = depth.shape
    depth[3, 4], depth[5, 6], depth[7, 8], depth[9, 10], depth[11, 12] = 0.0, 2.5001, -1.0, np.nan, 2.5
    v = RC.feedback_vertices(rgba, depth, K, 2.5)
    e = set(v["e"].tolist())
    for (y, x), kept in (((3, 4), False), ((5, 6), False), ((7, 8), False), ((9, 10), False), ((11, 12), True)):
        assert ((x * rows + y) in e) == kept, (y, x)
    assert len(e) == int(((depth > 0) & (depth <= 2.5)).sum())
    assert np.array_equal(v["e"], np.sort(v["e"])), "buffer order is column-major"
    t = R.Target(cols, rows)
    RC.draw_cloud(t, rgba, depth, K, 2.5, _own_view(rows, cols, K), None, 2)
    _, d, key = t.images()
    assert (d < 0xFFFFFF).sum() == len(e)
    assert d[rows - 1 - 3, 4] == 0xFFFFFF and d[rows - 1 - 11, 12] < 0xFFFFFF
    assert key[rows - 1 - 11, 12] & np.uint64(0xFFFFFFFF) == 12 * rows + 11
    c, _, _ = t.images()
    assert np.array_equal(c[rows - 1 - 11, 12, :3], rgba[11, 12, :3]), "colour type 2 returns the frame's bytes"


def test_equal_depth_keeps_the_smaller_source_index():
    """two source pixels in one target pixel with equal 24-bit depth: the smaller e = x * rows + y wins (R21)"""
    rgba, depth, K = _frame()
    rows, cols = depth.shape
    depth[:] = 0
    depth[10, 20] = depth[10, 21] = depth[11, 20] = depth[11, 21] = 2.0  # a fronto-parallel patch: one clip z
    # a view of half the frame's size at the frame's projection: 2 x 2 source pixels per target pixel
    mvp = _own_view(rows, cols, K)
    t = R.Target(cols // 2, rows // 2)
    RC.draw_cloud(t, rgba, depth, K, 25.0, mvp, None, 2)
    c, d, key = t.images()
    assert (d < 0xFFFFFF).sum() == 1
    y, x = np.argwhere(d < 0xFFFFFF)[0]
    assert key[y, x] & np.uint64(0xFFFFFFFF) == 20 * rows + 10, "the column-major first of the four"
    assert np.array_equal(c[y, x, :3], rgba[10, 20, :3])


def test_the_model_pose_is_applied_to_the_point_before_the_view():
    """R19: clip = MVP * (pose * (p, 1)), two matrix-vector products.  The other grouping, (MVP * pose) * (p, 1), is a different
    fp32 computation: on this frame the two give different 24-bit depths, and the draw must be the first."""
    from densemonoslam_amd import fusion

    rgba, depth, K = _frame(48, 64, seed=11)
    rows, cols = depth.shape
    a = np.radians(20.0)
    P = np.eye(4, dtype=F)
    P[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F)
    P[:3, 3] = (0.3, -0.1, 0.2)
    view = np.eye(4, dtype=F)
    view[:3, 3] = (0.1, 0.05, -0.4)
    V = R.mvp_from_pose(fusion.render_frustum(cols, rows, K[0], K[1], K[2], K[3], 0.1, 1000.0), view)
    rule, other = R.Target(cols, rows), R.Target(cols, rows)
    RC.draw_cloud(rule, rgba, depth, K, 25.0, V, P, 0)
    RC.draw_cloud(other, rgba, depth, K, 25.0, V, P, 0, product_first=True)
    assert not np.array_equal(rule.images()[1], other.images()[1]), "the case must tell the two groupings apart"
    # the rule, point by point: the world position in fp32 first, then the view
    v = RC.feedback_vertices(rgba, depth, K, 25.0)
    pos = v["pos"]
    wx, wy, wz, ww = RC.clip_of4(P, pos[:, 0], pos[:, 1], pos[:, 2], np.ones(len(pos), F))
    assert (ww == 1).all()
    pre = R.clip_of(V, wx, wy, wz)  # the cloud pre-transformed on the host, drawn with the identity pose
    got = RC.cloud_clip(V, P, pos[:, 0], pos[:, 1], pos[:, 2])
    assert all(np.array_equal(a, b) for a, b in zip(pre, got))
    lib_clip = fusion.render_cloud_clip(V, P, pos[7])
    assert np.array_equal(lib_clip, np.array([c[7] for c in got], F)), "dms_render_cloud_clip is the same function"


def test_normal_and_position_come_from_the_same_depth_image():
    """the RAW buffer's normal is the raw depth's, not the filtered one's (model_initialise pairs RAW position with FILTERED normal)"""
    rgba, depth, K = _frame()
    smooth = np.full_like(depth, 2.0)
    a, b = RC.feedback_vertices(rgba, depth, K, 25.0), RC.feedback_vertices(rgba, smooth, K, 25.0)
    inner = slice(40, 60)
    assert not np.allclose(a["nrm"][inner], b["nrm"][inner])
    assert np.allclose(np.abs(b["nrm"][inner, 2]), 1.0, atol=1e-5), "a fronto-parallel plane's normal is the optical axis"


def fixture_cases():
    return [str(n) for n in np.load(GOLDEN)["cases"]] if os.path.exists(GOLDEN) else ["missing"]


@pytest.mark.parametrize("name", fixture_cases())
def test_restatement_against_the_reference_programs_on_llvmpipe(name):
    z = np.load(GOLDEN)
    c, d, _ = RC.fixture_run(z, name)
    st = R.fixture_stats(z, name, c, d)
    print(name, st)
    RC.check_fixture_stats(z, name, st)


def test_vertex_counts_of_the_reference_buffers():
    """what GL's transform feedback wrote per buffer (the fixture's `vertices`, a GL_TRANSFORM_FEEDBACK_PRIMITIVES_WRITTEN query) against
    the restatement's emit test: equal for the FILTERED buffer (a NEAREST texture); the RAW buffer's LINEAR texture lets 133 pixels
    of zero depth pick up a neighbour's depth and emit a vertex the rule does not"""
    z = np.load(GOLDEN)
    k, maxd = tuple(float(v) for v in z["K"]), float(z["max_depth"])
    raw = len(RC.feedback_vertices(z["rgba"], z["depth_raw"], k, maxd)["e"])
    fil = len(RC.feedback_vertices(z["rgba"], z["depth_filtered"], k, maxd)["e"])
    assert (raw, fil) == (18629, 18629)
    assert z["vertices"].tolist() == [18762, fil]


def test_the_fixture_prefers_the_rule_over_the_other_grouping():
    """what the fixture showed about R19: with (MVP * pose) * v the FILTERED buffer's depths leave llvmpipe's by more than one unit
    at hundreds of pixels; with MVP * (pose * v) at none"""
    z = np.load(GOLDEN)
    k, maxd = tuple(float(v) for v in z["K"]), float(z["max_depth"])
    for name in ("tracked_filtered_2", "oblique_filtered_2"):
        c = RC.fixture_case(z, name)
        h, w = z[name + "__depth"].shape
        t = R.Target(w, h, tuple(z["clear"]))
        RC.draw_cloud(t, z["rgba"], z["depth_filtered"], k, maxd, z[c["view"] + "__mvp"], z["pose"], 2, product_first=True)
        col, d, _ = t.images()
        assert R.fixture_stats(z, name, col, d)["depth"] > 0.002, name
