"""CPU checks of the view's image panels (include/dmslam_render_panels.h): the header stands alone in C99 and C++11, every entry point
is exported, bad arguments are refused before any device access, and the restatement (tests/render_panels_ref.py) keeps the rules
DESIGN.md §4 R22-R26 states and holds the reference's own programs on llvmpipe (tests/golden/ref_render_panels.npz)."""
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
import render_panels_ref as P  # noqa: E402
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmslam_render_panels.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_render_panels.npz")
F = np.float32
CASES = ["depth_norm_mag", "depth_norm_min", "model_mag", "model_min", "rgb_mag", "rgb_min", "model_image_mag", "model_image_min",
         "rgb_nearest_min", "model_image_linear_mag", "rgb_tinted_min"]


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_on_its_own(compiler, std, ext):
    if shutil.which(compiler) is None:
        pytest.skip("%s not available" % compiler)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "h." + ext)
        with open(src, "w") as f:
            f.write('#include "dmslam_render_panels.h"\nint main(void) { dms_viewport v; (void)v; return DMS_PANEL_RGBA8; }\n')
        subprocess.check_call([compiler, std, "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o",
                               os.path.join(d, "h.o")])


def test_every_entry_point_is_exported():
    from densemonoslam_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(dms_[a-zA-Z0-9_]+)\s*\(", text))
    assert names == {"dms_panels_create", "dms_panels_destroy", "dms_panels_images", "dms_depth_norm", "dms_model_depth_image", "dms_render_blit",
                     "dms_fusion_draw_panels"}
    assert not [n for n in names if not hasattr(capi.lib, n)]


def test_bad_arguments_are_refused_without_a_device():
    from densemonoslam_amd import capi, fusion

    lib = capi.lib
    fake = C.c_void_p(16)  # a non-null target / panels / context / pixel address the checks below never touch
    img = fusion.Image2D(fake, 64 * 4, 48, 64)
    vp = fusion.Viewport(0, 0, 8, 8)
    white = (C.c_float * 3)(1, 1, 1)
    out = C.c_void_p()
    for w, h in ((0, 4), (4, 0), (-1, 4), (8193, 4), (4, 8193)):
        assert lib.dms_panels_create(C.byref(out), w, h) == -1 and not out.value
    assert lib.dms_panels_create(None, 4, 4) == -1
    assert lib.dms_panels_destroy(None) == 0
    assert lib.dms_panels_images(None, None, None) == -1
    assert lib.dms_depth_norm(None, C.byref(img), 300.0, 3000.0, None) == -1
    assert lib.dms_depth_norm(fake, None, 300.0, 3000.0, None) == -1
    assert lib.dms_model_depth_image(None, C.byref(img), 3.0, None) == -1
    assert lib.dms_model_depth_image(fake, None, 3.0, None) == -1
    # an image is checked before the panels object is read
    for bad in (fusion.Image2D(fake, 64 * 4 + 16, 48, 64), fusion.Image2D(None, 64 * 4, 48, 64), fusion.Image2D(fake, 0, 0, 0)):
        assert lib.dms_depth_norm(fake, C.byref(bad), 300.0, 3000.0, None) == -1
        assert lib.dms_model_depth_image(fake, C.byref(bad), 3.0, None) == -1
        assert lib.dms_render_blit(fake, C.byref(bad), 0, 0, C.byref(vp), white, None) == -1
    args = dict(t=fake, image=C.byref(img), vp=C.byref(vp), color=white)
    for missing in args:
        a = dict(args, **{missing: None})
        assert lib.dms_render_blit(a["t"], a["image"], 0, 0, a["vp"], a["color"], None) == -1, missing
    for fmt, filt in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert lib.dms_render_blit(fake, C.byref(img), fmt, filt, C.byref(vp), white, None) == -1
    vps = (fusion.Viewport * 4)()
    assert lib.dms_fusion_draw_panels(None, fake, fake, vps, 3.0, 15, None) == -1
    assert lib.dms_fusion_draw_panels(fake, None, fake, vps, 3.0, 15, None) == -1
    assert lib.dms_fusion_draw_panels(fake, fake, None, vps, 3.0, 15, None) == -1
    assert lib.dms_fusion_draw_panels(fake, fake, fake, None, 3.0, 15, None) == -1


def test_depth_norm_rule():
    """strict on both sides, uint() of the uniforms, 1 - float(v) / maxVal by R9, 0 outside"""
    d = np.array([[0, 300, 301, 1500, 2999, 3000, 65535]], np.uint16)
    n = P.depth_norm(d, F(0.3) * F(1000), F(3.0) * F(1000))
    assert n.tolist() == [[0, 0, int(np.floor((F(1) - F(301) / F(3000)) * F(255) + F(0.5))), 128, 0, 0, 0]]
    assert P.depth_norm(d, 300.9, 3000.9).tolist()[0][1:3] == [0, n[0, 2]]  # uint(300.9) = 300
    assert not P.depth_norm(d, np.nan, np.nan).any() and not P.depth_norm(d, 5000.0, 300.0).any()
    assert P.to_uint(-3.0) == 0 and P.to_uint(5e9) == 0xFFFFFFFF


def test_model_depth_rule():
    v = np.zeros((1, 6, 4), F)
    v[0, :, 2] = (1.5, 0.0, -1.0, 3.0, 3.0000002, np.nan)
    m = P.model_depth_image(v, 3.0)
    assert m[0, 0].tolist() == [128] * 4  # all four channels
    assert not m[0, 1].any() and not m[0, 2].any() and not m[0, 4].any()  # discarded: the clear colour
    assert m[0, 3].tolist() == [0] * 4  # z = maxDepth is kept and is 1 - 1 = 0
    assert m[0, 5].tolist() == [0] * 4  # NaN fails both comparisons and converts to 0 (R9)


def test_blit_rules():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (6, 8, 4), dtype=np.uint8)
    # R22 + R23: 1:1 NEAREST with white is the image upside down
    assert np.array_equal(P.blit_block(img, P.RGBA8, P.NEAREST, 8, 6), img[::-1])
    # 1:1 LINEAR samples texel centres: weights (1, 0, 0, 0)
    assert np.array_equal(P.blit_block(img, P.RGBA8, P.LINEAR, 8, 6), img[::-1])
    # integer magnification, NEAREST: each texel twice
    assert np.array_equal(P.blit_block(img, P.RGBA8, P.NEAREST, 16, 12), np.repeat(np.repeat(img[::-1], 2, 0), 2, 1))
    # R24 edge rule: CLAMP_TO_EDGE - the outer half texel of a magnified image repeats the edge texel, no wrap to the other side
    col = np.zeros((1, 2, 4), np.uint8)
    col[0, 1] = 255
    b = P.blit_block(col, P.RGBA8, P.LINEAR, 8, 1)[0, :, 0]
    assert b[0] == 0 and b[1] == 0 and b[-1] == 255 and b[-2] == 255 and (np.diff(b.astype(int)) >= 0).all() and 0 < b[3] < b[4] < 255
    # R25: luminance is (L, L, L, 1), then the colour multiplies r, g, b
    lum = rng.integers(0, 256, (6, 8), dtype=np.uint8)
    w = P.blit_block(lum, P.L8, P.NEAREST, 8, 6)
    assert np.array_equal(w[..., 0], lum[::-1]) and np.array_equal(w[..., 1], w[..., 0]) and np.array_equal(w[..., 2], w[..., 0]) and (w[..., 3] == 255).all()
    t = P.blit_block(lum, P.L8, P.NEAREST, 8, 6, (1.0, 0.5, 0.0))
    assert np.array_equal(t[..., 0], lum[::-1]) and not t[..., 2].any() and (t[..., 3] == 255).all()
    assert np.array_equal(t[..., 1], P.unorm8((lum[::-1].astype(F) / F(255)) * F(0.5)))
    # a blit writes colour only
    tg = R.Target(20, 10, (0.2, 0.4, 0.6, 1.0))
    P.blit(tg, img, P.RGBA8, P.LINEAR, (3, 2, 11, 5))
    assert (tg.depth == 0xFFFFFF).all() and (tg.key == R.CLEARED).all() and tg.seq == 0
    assert (tg.color[:2] == (51, 102, 153, 255)).all() and (tg.color[:, :3] == (51, 102, 153, 255)).all()


def test_shader_passes_against_the_reference_programs_on_llvmpipe():
    z = np.load(GOLDEN)
    cut = float(z["depth_cutoff"])
    assert (z["depth_norm"] > 0).sum() > 1000 and (z["model"][..., 3] > 0).sum() > 1000
    n = P.check_fixture("depth_norm", z["depth_norm"], P.depth_norm(z["depth"], F(0.3) * F(1000), F(cut) * F(1000)))
    m = P.check_fixture("model", z["model"], P.model_depth_image(z["vertex"], cut))
    print("depth_norm", n, "model", m)


def test_fixture_cases_are_the_recorded_ones():
    z = np.load(GOLDEN)
    assert [str(n) for n in z["cases"]] == CASES
    assert set(P.FIXTURE_RECORDED) == set(CASES) | {"depth_norm", "model"}
    assert "shader" not in " ".join(z.files) and all(z[k].dtype.kind in "uifU" for k in z.files)


@pytest.mark.parametrize("name", CASES)
def test_blit_against_the_textured_quad_on_llvmpipe(name):
    z = np.load(GOLDEN)
    st = P.check_fixture(name, z[name + "__rgba"], P.fixture_blit(z, name))
    print(name, st)
