"""Golden images of the REFERENCE's own draw programs (draw_global_surface.{vert,geom,frag}, draw_feedback.{vert,frag}).

tests/golden/gl_render_host.c is a small OpenGL host on the image's Mesa llvmpipe that loads those shader files from /root/reference at
RUN time and draws a surfel map with GlobalModel::renderPointCloud's call sequence and the GUI's framebuffer state (RGBA8, DEPTH24,
GL_LESS, point size 1).  This script builds the host into a temporary directory, grows a map with the oracle's processFrame restatement
(oracle/orc_pipeline.py) on the synthetic stream, keeps every STRIDE-th surfel, draws the cases below twice (llvmpipe rasterises in
parallel tiles: the second run must give the same bytes) and writes tests/golden/ref_render.npz:

    python tests/golden/make_ref_render_golden.py

GL has no surfel-id output: the fixture holds colour and 24-bit depth; winners come from the restatement (tests/render_ref.py).
tests/test_render_cpu.py holds the restatement to it, tests/test_render_gpu.py the HIP draw.
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
SHADERS = "/root/reference/elasticfusion/Core/src/Shaders"
W0, H0 = 160, 120
K0 = (132.0, 132.0, 80.0, 60.0)
FRAMES = 3
STRIDE = 6


def frustum(w, h, fu, fv, u0, v0, n, f):
    """dms_render_frustum (include/dmslam_render.h): in double, rounded to float at the end"""
    L, R = -u0 * n / fu, (w - u0) * n / fu
    B, T = -v0 * n / fv, (h - v0) * n / fv
    P = np.zeros((4, 4))
    P[0, 0], P[0, 2] = 2 * n / (R - L), (R + L) / (R - L)
    P[1, 1], P[1, 2] = 2 * n / (T - B), (T + B) / (T - B)
    P[2, 2], P[2, 3] = -(f + n) / (f - n), -(2 * f * n) / (f - n)
    P[3, 2] = -1.0
    return P.astype(np.float32)


def views(pose):
    import render_ref as R

    oblique = pose.copy()
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique[:3, :3] = pose[:3, :3] @ Ry
    oblique[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(1.2)
    close = pose.copy()
    close[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(0.8)
    return {
        "tracked": (W0, H0, R.mvp_from_pose(frustum(W0, H0, K0[0], K0[1], W0 / 2, H0 / 2, 0.1, 1000.0), pose)),
        "oblique": (W0, H0, R.mvp_from_pose(frustum(W0, H0, K0[0], K0[1], W0 / 2, H0 / 2, 0.05, 1000.0), oblique)),
        "closeup": (W0, H0, R.mvp_from_pose(frustum(W0, H0, 1200.0, 1200.0, W0 / 2, H0 / 2, 0.1, 1000.0), close)),
        "gui": (256, 80, R.mvp_from_pose(frustum(256, 80, 105.0, 105.0, 128, 40, 0.1, 1000.0), pose)),
    }


def cases(conf_median):
    """(name, view, [draw params]) - the parameter names of render_ref.Target.draw"""
    m = float(conf_median)
    out = []
    for v in ("tracked", "oblique", "closeup", "gui"):
        out.append((v + "_grey_unstable", v, [dict(color_type=0, draw_unstable=True, threshold=m)]))
        out.append((v + "_colour_stable", v, [dict(color_type=2, threshold=m)]))
    out += [
        ("tracked_normals", "tracked", [dict(color_type=1, draw_unstable=True, threshold=m)]),
        ("tracked_times", "tracked", [dict(color_type=3, time=FRAMES + 1, draw_unstable=True, threshold=m)]),
        ("tracked_times_at_1", "tracked", [dict(color_type=3, time=1, draw_unstable=True, threshold=m)]),
        ("tracked_contributions", "tracked", [dict(color_type=4, time=FRAMES + 1, draw_unstable=True, threshold=m)]),
        ("tracked_window", "tracked", [dict(color_type=2, draw_window=True, time=FRAMES + 1, time_idx=0, time_delta=1, draw_unstable=True,
                                            threshold=m)]),
        ("tracked_cluster_two_draws", "tracked", [dict(color_type=2, cluster_color=(0.9, 0.2, 0.4), threshold=m, draw_unstable=True),
                                                  dict(color_type=2, cluster_color=(0.1, 0.8, 0.3), threshold=m, draw_unstable=True)]),
        ("tracked_points", "tracked", [dict(draw_points=True, color_type=2, threshold=m)]),
        ("tracked_points_normals", "tracked", [dict(draw_points=True, color_type=1, threshold=0.0)]),
        ("tracked_points_cluster", "tracked", [dict(draw_points=True, color_type=0, threshold=0.0, cluster_color=(0.5, 0.5, 1.0))]),
    ]
    return out


CLEAR = (0.1, 0.2, 0.3, 1.0)


def request(path, surf, w, h, draws, mvp):
    recs = np.zeros((len(surf), 15), np.float32)
    recs[:, 0:4], recs[:, 4:8], recs[:, 8:11], recs[:, 11:15] = surf["pos"], surf["col"], surf["times"][:, :3], surf["nrm"]
    with open(path, "wb") as f:
        f.write(np.array([w, h, len(surf), len(draws)], np.int32).tobytes() + np.array(CLEAR, np.float32).tobytes() + recs.tobytes())
        for p in draws:
            cc = p.get("cluster_color")
            f.write(np.array([int(p.get("draw_points", False)), p.get("color_type", 0), int(p.get("draw_unstable", False)),
                              int(p.get("draw_window", False)), p.get("time", 0), p.get("time_idx", 0), p.get("time_delta", 0),
                              int(cc is not None)], np.int32).tobytes())
            f.write(np.array([p.get("threshold", 0.0)] + list(cc if cc is not None else (0, 0, 0)), np.float32).tobytes())
            f.write(np.asarray(mvp, np.float32).reshape(16).tobytes())


def run(host, td, surf, w, h, draws, mvp):
    rq, out = os.path.join(td, "rq.bin"), os.path.join(td, "out.bin")
    request(rq, surf, w, h, draws, mvp)
    subprocess.check_call([host, SHADERS, rq, out])
    raw = np.fromfile(out, np.uint8)
    return raw[:w * h * 4].reshape(h, w, 4).copy(), raw[w * h * 4:].view(np.uint32).reshape(h, w).copy()


def main(path):
    from densemonoslam_amd import synth  # host-side numpy only
    from oracle import orc_pipeline

    o = orc_pipeline.ElasticFusion(W0, H0, K0)
    for k in range(FRAMES):
        d, rgb, _ = synth.frame(k, width=W0, height=H0, K=K0, noise=True)
        r = o.processFrame(rgb, d)
    pose = np.asarray(r.pose, np.float32).reshape(4, 4)
    full = o.model
    surf = full[::STRIDE].copy()
    with tempfile.TemporaryDirectory() as td:
        host = os.path.join(td, "gl_render_host")
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-o", host, os.path.join(ROOT, "tests", "golden", "gl_render_host.c"),
                               "-ldl"])
        vs = views(pose)
        z = {"pos": surf["pos"], "col": surf["col"], "nrm": surf["nrm"], "times": surf["times"][:, :3].copy(), "pose": pose,
             "clear": np.array(CLEAR, np.float32)}
        names = []
        for name, v, draws in cases(np.median(surf["pos"][:, 3])):
            w, h, mvp = vs[v]
            c1, d1 = run(host, td, surf, w, h, draws, mvp)
            c2, d2 = run(host, td, surf, w, h, draws, mvp)
            assert c1.tobytes() == c2.tobytes() and d1.tobytes() == d2.tobytes(), "not repeatable: " + name
            z[name + "__rgba"], z[name + "__depth"], z[name + "__mvp"] = c1, d1, mvp
            z[name + "__draws"] = np.array(json.dumps(draws))
            names.append(name)
            print(name, w, h, "covered", int((d1 < 0xFFFFFF).sum()))
    z["cases"] = np.array(names)
    z["meta"] = np.array("reference draw programs (elasticfusion/Core/src/Shaders draw_global_surface.*, draw_feedback.*) run by Mesa llvmpipe "
                         "through tests/golden/gl_render_host.c; map: oracle/orc_pipeline after %d frames of the synthetic stream at %dx%d, "
                         "every %dth of %d surfels" % (FRAMES, W0, H0, STRIDE, len(full)))
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes;", len(surf), "surfels")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_render.npz"))
