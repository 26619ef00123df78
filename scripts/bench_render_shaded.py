"""Measures the shaded map view (include/dmslam_render_shaded.h, GUI::drawFXAA) on the benchmark stream's map.

    python scripts/bench_render_shaded.py [--frames 25] [--draws 50] [--out FILE]

The map is the one bench.py's 20-step form leaves (5 warm-up + 20 steps of the 640 x 480 synthetic stream, about 631 k surfels), as in
scripts/bench_render.py.  The GUI's offscreen buffer (3840 x 2160 RGBA32F) is resolved into a 1280 x 720 view, with the projection
pangolin::ProjectionMatrix(1280, 720, 2 fx, 2 fy, 640, 360, 0.1, 1000), at two poses:
  tracked  the tracked pose;
  oblique  turned 35 degrees about the camera's y axis and moved 1.2 m along its optical axis (surfels across the near plane).
Per pose, by HIP events over --draws calls after a warm-up: pass A (dms_render_shaded_draw: clear + disc pass 1 + the per-pixel
Phong resolve) and pass B (dms_render_fxaa: FXAA + depth blit) each on its own, and, for comparison, one renderPointCloud draw
(dms_render_clear + dms_render_draw) into the 1280 x 720 view.  Colour mode 2, draw_unstable on, the view from the tracked pose in
HBM.  One JSON line per pose; with --out the lines are also written to FILE.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--draws", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from densemonoslam_amd import fusion, synth

    W, H = 640, 480
    K = synth.K_640
    ef = fusion.ElasticFusion(W, H, K, model_capacity=8_000_000)
    n_unique = min(args.frames, 32)
    for k in range(args.frames):
        period = 2 * (n_unique - 1)
        j = k % period
        j = j if j < n_unique else period - j
        d, rgb, _ = synth.frame(j, width=W, height=H, K=K, noise=True)
        r = ef.processFrame(rgb, d)
    pose = np.array(r.pose, np.float32).reshape(4, 4)
    model = ef.globalModel()
    M = model.lastCount()
    conf = ef.getOption("confidence")
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)

    def timed(fn, n):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(n):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1000.0 / n  # us per call

    vw, vh = 1280, 720
    proj = fusion.render_frustum(vw, vh, 2 * K[0], 2 * K[1], vw / 2, vh / 2, 0.1, 1000.0)
    oblique = pose.copy()
    a = np.radians(35.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    oblique[:3, :3] = pose[:3, :3] @ Ry
    oblique[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(1.2)
    pose_buf = torch.empty(16, dtype=torch.float32, device="cuda")
    view = fusion.ShadedView(vw, vh)
    target = fusion.RenderTarget(vw, vh)
    lines = []
    for name, vp in (("tracked", pose), ("oblique", oblique)):
        pose_buf.copy_(torch.from_numpy(vp.reshape(16).copy()))
        pdev = C.c_void_p(pose_buf.data_ptr())
        light = fusion.render_mvp_from_pose(np.eye(4, dtype=np.float32), vp)[:3, 3]

        def pass_a():
            view.draw(model, proj, light_pos=light, sign_mult=-1.0, threshold=conf, draw_unstable=True, color_type=2, pose_dev=pdev,
                      stream=sptr)

        def pass_b():
            view.fxaa(stream=sptr)

        def point_cloud():
            target.clear((0, 0, 0, 0), stream=sptr)
            target.draw(model, proj, threshold=conf, draw_unstable=True, color_type=2, pose_dev=pdev, stream=sptr)

        view.clear((0, 0, 0, 1), stream=sptr)
        a_us = timed(pass_a, args.draws)
        b_us = timed(pass_b, args.draws)  # (the view keeps the blitted depth: from the 2nd call on the quad writes no colour)
        view.clear((0, 0, 0, 1), stream=sptr)
        b1_us = timed(lambda: (view.clear((0, 0, 0, 1), stream=sptr), pass_b()), args.draws)
        p_us = timed(point_cloud, args.draws)
        off = view.offscreen_images(stream=sptr)
        covered = int((off[1] < 0xFFFFFF).sum())
        rec = {"view": name, "offscreen": [view.off_width, view.off_height], "size": [vw, vh], "surfels": M,
               "pass_a_us": round(a_us, 2), "pass_b_us": round(b_us, 2), "clear_plus_pass_b_us": round(b1_us, 2),
               "render_point_cloud_us": round(p_us, 2), "offscreen_covered_px": covered,
               "what": "pass A = dms_render_shaded_draw (3840x2160), pass B = dms_render_fxaa into 1280x720 (depth test fails after the "
                       "first call); clear_plus_pass_b = dms_render_clear + dms_render_fxaa (every quad fragment passes); "
                       "render_point_cloud = dms_render_clear + dms_render_draw at 1280x720"}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    view.close()
    target.close()
    ef.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
