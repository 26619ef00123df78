"""Measures the map draw (include/dmslam_render.h, GlobalModel::renderPointCloud) on the benchmark stream's map.

    python scripts/bench_render.py [--frames 25] [--draws 200]

The map is the one bench.py's 20-step form leaves (5 warm-up + 20 steps of the 640 x 480 synthetic stream, about 631 k surfels).
One JSON line per view:
  (a) tracked  the tracked pose at 640 x 480 (the frame's own camera);
  (b) gui      the GUI's default view, pangolin::ProjectionMatrix(1024, 320, 420, 420, 512, 160, 0.1, 1000), at the tracked pose;
  (c) closeup  1280 x 960 from 0.9 m further along the optical axis with a 4x focal length (footprints of hundreds of pixels).
Each line: draw time by HIP events over --draws draws after a warm-up (clear + one disc draw of every surfel: draw_unstable on,
colour mode 2; the time includes the host's enqueue of the two calls where that is the longer part),
covered pixels, and the algorithmic bytes (surfel planes read + z-buffer and outputs) with the share of the HBM roof they imply.
For comparison, one line with the frame's own prediction (ElasticFusion::predict = splat project + resolve + fill-in) timed the
same way.  Per-kernel times: run this script under `rocprofv3 --kernel-trace --stats -- python scripts/bench_render.py`.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
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

    fusion.lib.dms_fusion_predict.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    fusion.check(fusion.lib.dms_fusion_predict(ef.h, 0.7, sptr), "dms_fusion_predict")
    pred_us = timed(lambda: fusion.lib.dms_fusion_predict(ef.h, 0.7, sptr), args.draws)
    print(json.dumps({"view": "frame_prediction", "surfels": M, "us": round(pred_us, 2),
                      "what": "dms_fusion_predict: splat project + resolve + fill-in, 640x480"}), flush=True)

    close = pose.copy()
    close[:3, 3] = pose[:3, 3] + pose[:3, 2] * np.float32(0.9)
    views = {
        "tracked": (W, H, fusion.render_frustum(W, H, K[0], K[1], K[2], K[3], 0.1, 1000.0), pose),
        "gui": (1024, 320, fusion.render_frustum(1024, 320, 420, 420, 512, 160, 0.1, 1000.0), pose),
        "closeup": (1280, 960, fusion.render_frustum(1280, 960, 4 * 2 * K[0], 4 * 2 * K[1], 640, 480, 0.1, 1000.0), close),
    }
    for name, (w, h, proj, vp) in views.items():
        t = fusion.RenderTarget(w, h)

        def draw():
            t.clear((0, 0, 0, 0), stream=sptr)
            t.draw(model, proj, threshold=conf, draw_unstable=True, color_type=2, pose_dev=C.c_void_p(ef.poseDevice()), stream=sptr)

        us = timed(draw, args.draws)
        c, dep, key = t.images(stream=sptr)
        cov = dep < 0xFFFFFF
        ids = (key[cov] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        n_px = w * h
        # pass 1 reads pos (16 B) of every surfel and nrm (16 B) of the drawn ones (upper bound: all); the z-buffer is cleared (8 B),
        # read and written by the atomics of the covered pixels (upper bound 16 B each); pass 2 reads the key (8 B), the winners' nrm +
        # col (32 B) and writes colour + depth (8 B); the clear writes colour + depth (8 B)
        bytes_alg = M * 32 + n_px * (8 + 8 + 8) + int(cov.sum()) * (16 + 32 + 8)
        print(json.dumps({"view": name, "size": [w, h], "surfels": M, "us": round(us, 2), "covered_px": int(cov.sum()),
                          "distinct_winners": int(len(np.unique(ids))),
                          "ns_per_covered_px": round(1000.0 * us / max(1, int(cov.sum())), 4),
                          "of_prediction": round(us / pred_us, 3), "algorithmic_bytes": bytes_alg,
                          "hbm_roof_share": round(bytes_alg / (us * 1e-6) / HBM_BYTES_PER_S, 4)}), flush=True)
        t.close()
    ef.close()


if __name__ == "__main__":
    main()
