"""CPU checks of the shaded map view (include/dmslam_render_shaded.h, GUI::drawFXAA): the header stands alone in C99 and C++11, every
entry point is exported, bad arguments are refused before any device access, and the restatement (tests/render_shaded_ref.py) agrees
with the reference's own programs on Mesa llvmpipe (tests/golden/ref_render_shaded.npz) within the counted bounds of DESIGN.md §5."""
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
import render_shaded_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmslam_render_shaded.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_render_shaded.npz")
MAP = os.path.join(ROOT, "tests", "golden", "ref_render.npz")


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")])
def test_header_compiles_on_its_own(compiler, std, ext):
    if shutil.which(compiler) is None:
        pytest.skip("%s not available" % compiler)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "h." + ext)
        with open(src, "w") as f:
            f.write('#include "dmslam_render_shaded.h"\nint main(void) { dms_render_offscreen* o = 0; (void)o; return 0; }\n')
        subprocess.check_call([compiler, std, "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o",
                               os.path.join(d, "h.o")])


def test_every_entry_point_is_exported():
    from densemonoslam_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dms_render_[a-zA-Z0-9_]+)\s*\(", text)))
    assert {"dms_render_offscreen_create", "dms_render_offscreen_destroy", "dms_render_offscreen_size", "dms_render_shaded_draw",
            "dms_render_fxaa", "dms_render_offscreen_images"} == set(names)
    assert not [n for n in names if not hasattr(capi.lib, n)]


def test_bad_arguments_are_refused_without_a_device():
    from densemonoslam_amd import capi, fusion

    lib = capi.lib
    h = C.c_void_p()
    assert lib.dms_render_offscreen_create(None, 64, 64) == -1
    for w, hh in ((0, 64), (64, 0), (-1, 5), (8193, 16), (16, 8193)):
        assert lib.dms_render_offscreen_create(C.byref(h), w, hh) == -1, (w, hh)
        assert h.value is None
    wi, he = C.c_int(), C.c_int()
    assert lib.dms_render_offscreen_size(None, C.byref(wi), C.byref(he)) == -1
    assert lib.dms_render_offscreen_images(None, None, None, None) == -1
    assert lib.dms_render_offscreen_destroy(None) == 0
    light, clear = (C.c_float * 3)(), (C.c_float * 4)()
    p = fusion.RenderParams()
    fake = C.c_void_p(16)  # non-null buffer, map and target: the parameter checks come first and never touch them
    assert lib.dms_render_shaded_draw(None, fake, C.byref(p), light, -1.0, clear, None) == -1
    assert lib.dms_render_shaded_draw(fake, None, C.byref(p), light, -1.0, clear, None) == -1
    assert lib.dms_render_shaded_draw(fake, fake, None, light, -1.0, clear, None) == -1
    assert lib.dms_render_shaded_draw(fake, fake, C.byref(p), None, -1.0, clear, None) == -1
    assert lib.dms_render_shaded_draw(fake, fake, C.byref(p), light, -1.0, None, None) == -1
    for field, value in (("color_type", 4), ("color_type", -1), ("time_idx", 8), ("time_idx", -1), ("draw_points", 1),
                         ("use_cluster_color", 1)):
        q = fusion.RenderParams()
        setattr(q, field, value)
        assert lib.dms_render_shaded_draw(fake, fake, C.byref(q), light, -1.0, clear, None) == -1, (field, value)
    assert lib.dms_render_fxaa(None, fake, None) == -1
    assert lib.dms_render_fxaa(fake, None, None) == -1


def test_pass_b_pieces_follow_the_rules():
    """R15-R17 on small hand-made buffers: texel origin and REPEAT wrap, the blit's source texel, the quad's depth test"""
    img = np.zeros((4, 4, 4), np.float32)
    img[:, 0, 0] = 1.0  # column 0 red
    # at s = 0 (the left edge of texel 0): half texel 0, half texel 3 (wrapped)
    c = S.tex_linear(img, np.array([0.0], np.float32), np.array([0.5], np.float32))
    assert c[0, 0] == np.float32(0.5)
    c = S.tex_linear(img, np.array([0.125], np.float32), np.array([0.5], np.float32))  # the centre of texel 0
    assert c[0, 0] == 1.0
    sx, sy = S.blit_texels(3, 2, 6, 4)
    assert sx.tolist() == [1, 3, 5] and sy.tolist() == [1, 3]
    sx, _ = S.blit_texels(4, 2, 2, 2)
    assert sx.tolist() == [0, 0, 1, 1]
    # the quad at depth 0.5 colours only where the view holds a larger depth; the blit then replaces depth and key everywhere
    t = R.Target(2, 1)
    t.depth[0, 0] = 100
    off = S.Offscreen(2, 1)
    off.rgba[:] = 1.0
    S.composite(t, off)
    assert t.color[0, 0].tolist() == [0, 0, 0, 0] and t.color[0, 1].tolist() == [255, 255, 255, 255]
    assert t.depth.tolist() == [[0xFFFFFF, 0xFFFFFF]] and t.seq == 1
    assert S.QUAD_DEPTH == int(R.depth24(np.float32(0.5)))


def test_one_fragment_per_pixel_and_phong_of_a_facing_disc():
    """a disc facing the camera, lit from the eye: every covered pixel finds its fragment (no NaN position) and the colour is
    ambient + diffuse + specular of a grey surface seen head-on"""
    dt = np.dtype([("pos", "<f4", (4,)), ("col", "<f4", (4,)), ("nrm", "<f4", (4,)), ("times", "<f4", (8,))])
    s = np.zeros(1, dt)
    s["pos"] = (0, 0, -2, 10)
    s["nrm"] = (0, 0, 1, 0.5)
    s["times"] = -3
    mvp = R.mvp_from_pose(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1.0002, -0.2], [0, 0, -1, 0]], np.float32),
                          np.diag([1, -1, -1, 1]).astype(np.float32))
    off = S.Offscreen(32, 32)
    off.draw(s, mvp, light_pos=(0, 0, 0), sign_mult=1.0, color_type=0)
    cov = off.depth < 0xFFFFFF
    assert cov.sum() > 50 and not np.isnan(off.rgba).any()
    grey = 0.5 * 1.0 + 0.1
    for py, px in np.argwhere(cov)[::7]:
        # the view is the identity (eye = world origin = the light), the disc lies in z = -2: the pixel centre's point on it
        v = np.array([2 * ((px + 0.5) / 16 - 1), 2 * ((py + 0.5) / 16 - 1), -2.0])
        ndotl = 2 / np.linalg.norm(v)
        expect = 0.3 * grey + grey * ndotl + (2 * ndotl * ndotl - 1) ** 32
        assert abs(off.rgba[py, px, 0] - expect) < 1e-4, (px, py, off.rgba[py, px], expect)
        assert abs(off.rgba[py, px, 3] - (1 + ndotl + (2 * ndotl * ndotl - 1) ** 32)) < 1e-4  # alpha: 1 + NdotL + specular


def fixture_cases():
    return [str(n) for n in np.load(GOLDEN)["cases"]]


@pytest.mark.parametrize("name", fixture_cases())
def test_restatement_against_the_reference_programs_on_llvmpipe(name):
    z = np.load(GOLDEN)
    s = R.fixture_map(np.load(MAP))
    off, t = S.fixture_run(z, name, s)
    st = S.fixture_stats(z, name, off.rgba, off.depth, t.color, t.depth)
    S.check_fixture_stats(name, st)
