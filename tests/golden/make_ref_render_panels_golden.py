"""Golden images of the REFERENCE's own panel programs (empty.vert + quad.geom with depth_norm.frag and visualise_textures.frag) and of
GUI::displayImg's textured quad: the four image panels of the view (GUI/src/MainController.cpp:649-664).

tests/golden/gl_render_panels_host.c is a small OpenGL host on the image's Mesa llvmpipe that loads those shader files from
/root/reference at RUN time, runs them with ComputePack::compute's and IndexMap::renderDepth's call sequence and draws each of the four
textures into a window-sized framebuffer through a flipped textured quad in displayImg's state.  This script builds the host into a
temporary directory, takes the last of FRAMES frames of the synthetic stream through the oracle's processFrame restatement
(oracle/orc_pipeline.py: raw depth, colour, the ACTIVE prediction's vertex and colour image), runs the cases below twice (the second
run must give the same bytes) and writes tests/golden/ref_render_panels.npz:

    python tests/golden/make_ref_render_panels_golden.py

The fixture holds images and settings only.  tests/test_render_panels_cpu.py holds the restatement (tests/render_panels_ref.py) to
it, tests/test_render_panels_gpu.py the HIP kernels.
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
from make_ref_render_golden import H0, K0, W0  # noqa: E402

FRAMES = 10  # "one late frame"
CONFIDENCE = 2.0  # the confidence threshold (the GUI's slider; default 10): surfels of a 10-frame map pass it, so the ACTIVE prediction is populated
DEPTH_CUTOFF = 3.0  # gui->depthCutoff's default
CLEAR = (0.2, 0.4, 0.6, 1.0)  # exact in bytes: no R9 tie outside the viewport
PANELS = ("depth_norm", "model", "rgb", "model_image")
LINEAR_OF = (1, 0, 1, 0)  # Context.h:158-160, 179-181; IndexMap.cpp:42-47, 59-65
# name -> (target W, H, viewport x, y, w, h): 160 x 120 magnified by 1.31875 / 1.3083 into a corner of a larger target, and minified
# by 0.63125 / 0.6417 over a whole one; no ratio is an integer
SIZES = {"mag": (230, 170, 13, 9, 211, 157), "min": (101, 77, 0, 0, 101, 77)}


def cases():
    out = []
    for k, p in enumerate(PANELS):
        for sz in SIZES:
            out.append(("%s_%s" % (p, sz), k, LINEAR_OF[k], sz, (1.0, 1.0, 1.0)))
    # each filter also on the other kind of image, and a colour that is not white (MainController.cpp:652 sets (1, 0.5, 0.6) earlier)
    out.append(("rgb_nearest_min", 2, 0, "min", (1.0, 1.0, 1.0)))
    out.append(("model_image_linear_mag", 3, 1, "mag", (1.0, 1.0, 1.0)))
    out.append(("rgb_tinted_min", 2, 1, "min", (1.0, 0.5, 0.6)))
    return out


def run(host, td, depth, vertex, rgba, pimg, blits, env=None):
    rq, out = os.path.join(td, "rq.bin"), os.path.join(td, "out.bin")
    with open(rq, "wb") as f:
        f.write(np.array([W0, H0, len(blits)], np.int32).tobytes())
        f.write(np.array([np.float32(0.3) * np.float32(1000), np.float32(DEPTH_CUTOFF) * np.float32(1000), DEPTH_CUTOFF], np.float32).tobytes())
        f.write(np.ascontiguousarray(depth, np.uint16).tobytes() + np.ascontiguousarray(vertex, np.float32).tobytes()
                + np.ascontiguousarray(rgba, np.uint8).tobytes() + np.ascontiguousarray(pimg, np.uint8).tobytes())
        for _, k, lin, sz, col in blits:
            f.write(np.array((k, lin) + SIZES[sz], np.int32).tobytes() + np.array(col + CLEAR, np.float32).tobytes())
    subprocess.check_call([host, SHADERS, rq, out], env=env)
    raw = np.fromfile(out, np.uint8)
    n = W0 * H0
    flags = raw[:16].view(np.int32).copy()
    norm = raw[16:16 + n].reshape(H0, W0).copy()
    model = raw[16 + n:16 + 5 * n].reshape(H0, W0, 4).copy()
    off, imgs = 16 + 5 * n, []
    for _, _, _, sz, _ in blits:
        w, h = SIZES[sz][:2]
        imgs.append(raw[off:off + w * h * 4].reshape(h, w, 4).copy())
        off += w * h * 4
    assert off == len(raw)
    return flags, norm, model, imgs


def main(path):
    from densemonoslam_amd import synth  # host-side numpy only
    from oracle import orc_pipeline

    o = orc_pipeline.ElasticFusion(W0, H0, K0, confidence=CONFIDENCE)
    for k in range(FRAMES):
        d, rgb, _ = synth.frame(k, width=W0, height=H0, K=K0, noise=True)
        o.processFrame(rgb, d)
    depth, rgba = np.asarray(d, np.uint16), np.asarray(o.rgba, np.uint8)
    pimg, vertex = np.asarray(o.pred[0], np.uint8), np.asarray(o.pred[1], np.float32)
    assert depth.shape == (H0, W0) and rgba.shape == (H0, W0, 4) and pimg.shape == (H0, W0, 4) and vertex.shape == (H0, W0, 4)
    blits = cases()
    with tempfile.TemporaryDirectory() as td:
        host = os.path.join(td, "gl_render_panels_host")
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-o", host, os.path.join(ROOT, "tests", "golden", "gl_render_panels_host.c"),
                               "-ldl"])
        a = run(host, td, depth, vertex, rgba, pimg, blits)
        b = run(host, td, depth, vertex, rgba, pimg, blits)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[3], b[3])), "not repeatable"
    flags, norm, model, imgs = a
    z = {"depth": depth, "vertex": vertex, "rgba": rgba, "model_rgba": pimg, "depth_cutoff": np.float32(DEPTH_CUTOFF),
         "clear": np.array(CLEAR, np.float32), "depth_norm": norm, "model": model}
    names = []
    for (name, k, lin, sz, col), im in zip(blits, imgs):
        z[name + "__rgba"] = im
        z[name + "__case"] = np.array(json.dumps({"panel": PANELS[k], "source": k, "linear": lin, "target": SIZES[sz][:2],
                                                  "viewport": SIZES[sz][2:], "color": col}))
        names.append(name)
        print(name, im.shape)
    z["cases"] = np.array(names)
    z["meta"] = np.array(json.dumps({
        "what": "reference panel programs (elasticfusion/Core/src/Shaders empty.vert, quad.geom, depth_norm.frag, visualise_textures.frag) "
                "and a flipped textured quad, run by Mesa llvmpipe through tests/golden/gl_render_panels_host.c; frame %d of the synthetic "
                "stream at %dx%d through oracle/orc_pipeline" % (FRAMES - 1, W0, H0),
        "compatibility_context": bool(flags[0]),
        "quad": "fixed-function GL_MODULATE, client vertex arrays" if flags[0] else "the host's own pass-through program, texture times colour",
        "depth_norm": "rendered into the unsized GL_LUMINANCE texture" if flags[1]
                      else "GL_LUMINANCE attachment not renderable: float output captured in R32F, converted to bytes by R9"}))
    print(str(z["meta"]))
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ref_render_panels.npz"))
