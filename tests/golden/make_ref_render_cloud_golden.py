"""Golden images of the REFERENCE's own feedback programs (vertex_feedback.{vert,geom}, draw_feedback.{vert,frag}): the live-frame
point clouds of the 3-D view (FeedbackBuffer::compute + ::render, GUI/src/MainController.cpp:475-493).

tests/golden/gl_render_cloud_host.c is a small OpenGL host on the image's Mesa llvmpipe that loads those shader files from
/root/reference at RUN time, fills the RAW and the FILTERED feedback buffer from one frame and draws them with FeedbackBuffer::render's
call sequence into the GUI's framebuffer state.  This script builds the host into a temporary directory, takes the last of FRAMES
frames of the synthetic stream through the oracle's processFrame restatement (oracle/orc_pipeline.py: colour, raw and filtered metric
depth, tracked pose), draws the cases below twice (the second run must give the same bytes) and writes tests/golden/ref_render_cloud.npz:

    python tests/golden/make_ref_render_cloud_golden.py

The fixture holds images, matrices and settings only.  tests/test_render_cloud_cpu.py holds the restatement (tests/render_cloud_ref.py)
to it, tests/test_render_cloud_gpu.py the HIP draw.
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
from make_ref_render_golden import FRAMES, H0, K0, W0, frustum  # noqa: E402

CLEAR = (0.1, 0.2, 0.3, 1.0)
MAX_DEPTH = 25.0  # (float)(int)maxDepthProcessed (Context.h:211)


def views(pose):
    """name -> clip-from-world matrix (W0 x H0 targets): the tracked pose with the frame's own projection, and an oblique view"""
    import render_ref as R

    oblique = pose.copy()
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique[:3, :3] = pose[:3, :3] @ Ry
    oblique[:3, 3] = pose[:3, 3] - pose[:3, 0] * np.float32(0.8)
    return {"tracked": R.mvp_from_pose(frustum(W0, H0, K0[0], K0[1], K0[2], K0[3], 0.1, 1000.0), pose),
            "oblique": R.mvp_from_pose(frustum(W0, H0, K0[0], K0[1], W0 / 2, H0 / 2, 0.05, 1000.0), oblique)}


def run(host, td, rgba, dm, dmf, draws):
    """draws: (buffer 0 / 1, color_type, mvp, pose) into one W0 x H0 framebuffer"""
    rq, out = os.path.join(td, "rq.bin"), os.path.join(td, "out.bin")
    with open(rq, "wb") as f:
        f.write(np.array([W0, H0, W0, H0, len(draws)], np.int32).tobytes())
        f.write(np.array(CLEAR + (K0[0], K0[1], K0[2], K0[3], MAX_DEPTH), np.float32).tobytes())
        f.write(np.ascontiguousarray(rgba, np.uint8).tobytes() + np.ascontiguousarray(dm, np.float32).tobytes()
                + np.ascontiguousarray(dmf, np.float32).tobytes())
        for b, ct, mvp, pose in draws:
            f.write(np.array([b, ct], np.int32).tobytes() + np.asarray(mvp, np.float32).reshape(16).tobytes()
                    + np.asarray(pose, np.float32).reshape(16).tobytes())
    subprocess.check_call([host, SHADERS, rq, out])
    raw = np.fromfile(out, np.uint8)
    n = W0 * H0
    return raw[:n * 4].reshape(H0, W0, 4).copy(), raw[n * 4:n * 8].view(np.uint32).reshape(H0, W0).copy(), raw[n * 8:].view(np.int32).copy()


def main(path):
    from densemonoslam_amd import synth  # host-side numpy only
    from oracle import orc_pipeline

    o = orc_pipeline.ElasticFusion(W0, H0, K0)
    for k in range(FRAMES):
        d, rgb, _ = synth.frame(k, width=W0, height=H0, K=K0, noise=True)
        r = o.processFrame(rgb, d)
    pose = np.asarray(r.pose, np.float32).reshape(4, 4)
    rgba, dm, dmf = np.asarray(o.rgba, np.uint8), np.asarray(o.depth_metric, np.float32), np.asarray(o.depth_metric_filtered, np.float32)
    vs = views(pose)
    z = {"rgba": rgba, "depth_raw": dm, "depth_filtered": dmf, "pose": pose, "K": np.array(K0, np.float32),
         "max_depth": np.float32(MAX_DEPTH), "clear": np.array(CLEAR, np.float32)}
    for v, m in vs.items():
        z[v + "__mvp"] = m
    names = []
    with tempfile.TemporaryDirectory() as td:
        host = os.path.join(td, "gl_render_cloud_host")
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-o", host, os.path.join(ROOT, "tests", "golden", "gl_render_cloud_host.c"),
                               "-ldl"])
        for v in vs:
            for b, buf in enumerate(("RAW", "FILTERED")):
                for ct in (0, 1, 2):
                    name = "%s_%s_%d" % (v, buf.lower(), ct)
                    draws = [(b, ct, vs[v], pose)]
                    c1, d1, n1 = run(host, td, rgba, dm, dmf, draws)
                    c2, d2, _ = run(host, td, rgba, dm, dmf, draws)
                    assert c1.tobytes() == c2.tobytes() and d1.tobytes() == d2.tobytes(), "not repeatable: " + name
                    z[name + "__rgba"], z[name + "__depth"] = c1, d1
                    z[name + "__case"] = np.array(json.dumps({"buffer": buf, "color_type": ct, "view": v}))
                    names.append(name)
                    z["vertices"] = n1  # what GL emitted (the feedback query): RAW, FILTERED
                    print(name, "covered", int((d1 < 0xFFFFFF).sum()), "vertices written by GL", n1.tolist())
    z["cases"] = np.array(names)
    z["meta"] = np.array("reference feedback programs (elasticfusion/Core/src/Shaders vertex_feedback.*, draw_feedback.*) run by Mesa llvmpipe "
                         "through tests/golden/gl_render_cloud_host.c; frame %d of the synthetic stream at %dx%d through oracle/orc_pipeline"
                         % (FRAMES - 1, W0, H0))
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_render_cloud.npz"))
