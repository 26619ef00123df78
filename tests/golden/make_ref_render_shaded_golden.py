"""Golden images of the REFERENCE's own shaded-view programs (GUI::drawFXAA: draw_global_surface.{vert,geom} +
draw_global_surface_phong.frag, then empty.vert + quad.geom + fxaa.frag and the depth blit).

tests/golden/gl_render_shaded_host.c is a small OpenGL host on the image's Mesa llvmpipe that loads those shader files from
/root/reference at RUN time and runs drawFXAA's call sequence with the GUI's framebuffer state.  This script builds the host into a
temporary directory, takes the map of tests/golden/ref_render.npz (its generator grows it with the oracle's processFrame restatement),
runs the cases below twice (llvmpipe rasterises in parallel tiles: the second run must give the same bytes) and writes
tests/golden/ref_render_shaded.npz:

    python tests/golden/make_ref_render_shaded_golden.py

Per case: the offscreen RGBA32F and 24-bit depth, the view's RGBA8 after FXAA and its depth after the blit.  The offscreen buffer is
small (OFF) and larger than the view (VIEW), so that the resolve still downsamples; one case upsamples.
tests/test_render_shaded_cpu.py holds the restatement (tests/render_shaded_ref.py) to it, tests/test_render_shaded_gpu.py the HIP path.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
SHADERS = "/root/reference/elasticfusion/Core/src/Shaders"
OFF = (128, 72)
VIEW = (96, 64)
VIEW_CLEAR = (0.0, 0.0, 0.0, 1.0)


def views(pose):
    """name -> (offscreen width, height, view width, height, mvp, mv): the views of make_ref_render_golden at the offscreen size"""
    import render_ref as R
    from make_ref_render_golden import frustum

    sw, sh = OFF
    f = 80.0
    oblique = pose.copy()
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique[:3, :3] = pose[:3, :3] @ Ry
    oblique[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(1.2)
    close = pose.copy()
    close[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(0.8)
    ident = np.eye(4, dtype=np.float32)
    out = {}
    for name, p, fl, near, size in (("tracked", pose, f, 0.1, OFF), ("oblique", oblique, f, 0.05, OFF), ("closeup", close, 600.0, 0.1, OFF),
                                    ("upsample", pose, 40.0, 0.1, (64, 40))):
        w, h = size
        proj = frustum(w, h, fl, fl, w / 2, h / 2, near, 1000.0)
        out[name] = (w, h) + VIEW + (R.mvp_from_pose(proj, p), R.mvp_from_pose(ident, p))
    return out


def cases(m, frames):
    """(name, view, parameters of render_shaded_ref.Offscreen.draw without the matrices)"""
    base = dict(threshold=m, sign_mult=-1.0, clear_rgba=(0.05, 0.05, 0.3, 0.0))
    return [
        ("tracked_grey_unstable", "tracked", dict(base, color_type=0, draw_unstable=True)),
        ("tracked_colour_stable", "tracked", dict(base, color_type=2)),
        ("tracked_normals_invert", "tracked", dict(base, color_type=1, draw_unstable=True, sign_mult=1.0)),
        ("tracked_times_window", "tracked", dict(base, color_type=3, time=frames + 1, time_idx=0, time_delta=1, draw_window=True,
                                                 draw_unstable=True)),
        ("tracked_times_at_1_showcase", "tracked", dict(base, color_type=3, time=1, draw_unstable=True, clear_rgba=(1.0, 1.0, 1.0, 0.0))),
        ("oblique_colour_unstable", "oblique", dict(base, color_type=2, draw_unstable=True)),
        ("closeup_grey_unstable", "closeup", dict(base, color_type=0, draw_unstable=True)),
        ("upsample_colour_unstable", "upsample", dict(base, color_type=2, draw_unstable=True)),
    ]


def request(path, surf, sw, sh, w, h, p, mvp, mv):
    recs = np.zeros((len(surf), 15), np.float32)
    recs[:, 0:4], recs[:, 4:8], recs[:, 8:11], recs[:, 11:15] = surf["pos"], surf["col"], surf["times"][:, :3], surf["nrm"]
    light = np.asarray(mv, np.float32)[:3, 3]
    with open(path, "wb") as f:
        f.write(np.array([sw, sh, w, h, len(surf), p.get("color_type", 0), int(p.get("draw_unstable", False)),
                          int(p.get("draw_window", False)), p.get("time", 0), p.get("time_idx", 0), p.get("time_delta", 0)],
                         np.int32).tobytes())
        f.write(np.array([p["threshold"], p["sign_mult"]] + list(light) + list(p["clear_rgba"]) + list(VIEW_CLEAR), np.float32).tobytes())
        f.write(np.asarray(mvp, np.float32).reshape(16).tobytes())
        f.write(recs.tobytes())


def run(host, td, surf, sw, sh, w, h, p, mvp, mv):
    rq, out = os.path.join(td, "rq.bin"), os.path.join(td, "out.bin")
    request(rq, surf, sw, sh, w, h, p, mvp, mv)
    subprocess.check_call([host, SHADERS, rq, out])
    raw = np.fromfile(out, np.uint8)
    o = 0
    parts = []
    for shape, dt in (((sh, sw, 4), np.float32), ((sh, sw), np.uint32), ((h, w, 4), np.uint8), ((h, w), np.uint32)):
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        parts.append(raw[o:o + nb].view(dt).reshape(shape).copy())
        o += nb
    assert o == len(raw)
    return parts


def main(path):
    import render_ref as R

    z0 = np.load(os.path.join(ROOT, "tests", "golden", "ref_render.npz"))
    surf = R.fixture_map(z0)
    pose = z0["pose"]
    frames = 3
    with tempfile.TemporaryDirectory() as td:
        host = os.path.join(td, "gl_render_shaded_host")
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-o", host,
                               os.path.join(ROOT, "tests", "golden", "gl_render_shaded_host.c"), "-ldl"])
        vs = views(pose)
        z = {"view_clear": np.array(VIEW_CLEAR, np.float32)}
        names = []
        for name, v, p in cases(float(np.median(surf["pos"][:, 3])), frames):
            sw, sh, w, h, mvp, mv = vs[v]
            r1 = run(host, td, surf, sw, sh, w, h, p, mvp, mv)
            r2 = run(host, td, surf, sw, sh, w, h, p, mvp, mv)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2)), "not repeatable: " + name
            for key, a in zip(("off_rgba", "off_depth", "rgba", "depth"), r1):
                z[name + "__" + key] = a
            z[name + "__mvp"], z[name + "__mv"] = mvp, mv
            z[name + "__params"] = np.array(json.dumps(p))
            names.append(name)
            print(name, (sw, sh), "->", (w, h), "covered", int((r1[1] < 0xFFFFFF).sum()))
    z["cases"] = np.array(names)
    z["meta"] = np.array("reference shaded-view programs (elasticfusion/Core/src/Shaders draw_global_surface.{vert,geom}, "
                         "draw_global_surface_phong.frag, empty.vert, quad.geom, fxaa.frag) run by Mesa llvmpipe through "
                         "tests/golden/gl_render_shaded_host.c; map: the surfels of tests/golden/ref_render.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes;", len(surf), "surfels")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_render_shaded.npz"))
