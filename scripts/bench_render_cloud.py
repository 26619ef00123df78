"""Measures the live-frame cloud draw (include/dmslam_render_cloud.h, FeedbackBuffer::render) on the benchmark stream.

    python scripts/bench_render_cloud.py [--frames 25] [--draws 400] [--repeats 5]

The context is the one bench.py's 20-step form leaves (5 warm-up + 20 steps of the 640 x 480 synthetic stream).  One JSON line per case,
each timed by HIP events over --draws calls after a warm-up, --repeats times (median, minimum and maximum of the repeats in us per call;
the time includes the host's enqueue where that is the longer part):
  raw_tracked        clear + the RAW cloud at 640 x 480 into 640 x 480, view and model pose from the tracked pose in HBM;
  raw_filtered_gui   clear + RAW + FILTERED clouds into the GUI's 1024 x 320 view (pangolin::ProjectionMatrix(1024, 320, 420, 420, 512,
                     160, 0.1, 1000)) at the tracked pose;
  clear_640x480 / clear_1024x320   the clear alone (subtract it for the draws' own time);
  map_points_tracked clear + the map's point draw (draw_points = 1, threshold 0: every surfel) at 640 x 480, for comparison;
  compute_feedback   dms_fusion_compute_feedback: the three device-to-device copies the GUI loop issues before the clouds.
There is no pass / fail threshold.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_render_cloud.py`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--draws", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
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
        ef.processFrame(rgb, d)
    model = ef.globalModel()
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)
    pose_dev = C.c_void_p(ef.poseDevice())
    ef.computeFeedbackBuffers(sptr)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.draws):
                fn()
            b.record(stream)
            b.synchronize()
            us.append(a.elapsed_time(b) * 1000.0 / args.draws)
        return {"us": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}

    def line(case, t, **more):
        print(json.dumps(dict({"case": case, "draws": args.draws, "repeats": args.repeats}, **t, **more)), flush=True)

    own = fusion.render_frustum(W, H, K[0], K[1], K[2], K[3], 0.1, 1000.0)
    gui = fusion.render_frustum(1024, 320, 420, 420, 512, 160, 0.1, 1000.0)
    t0, t1 = fusion.RenderTarget(W, H), fusion.RenderTarget(1024, 320)

    def cloud(t, proj, which):
        ef.renderCloud(t, which, proj, color_type=2, pose_dev=pose_dev, model_pose_dev=pose_dev, stream=sptr)

    def raw_tracked():
        t0.clear((0, 0, 0, 0), stream=sptr)
        cloud(t0, own, fusion.CLOUD_RAW)

    def raw_filtered_gui():
        t1.clear((0, 0, 0, 0), stream=sptr)
        cloud(t1, gui, fusion.CLOUD_RAW)
        cloud(t1, gui, fusion.CLOUD_FILTERED)

    def map_points():
        t0.clear((0, 0, 0, 0), stream=sptr)
        t0.draw(model, own, threshold=0.0, draw_points=True, color_type=2, pose_dev=pose_dev, stream=sptr)

    r = timed(raw_tracked)
    cov = int((t0.images(stream=sptr)[1] < 0xFFFFFF).sum())
    # pass 1 reads the depth (4 B per source pixel) and the keys it competes for (16 B per emitted point, upper bound); pass 2 reads the key
    # (8 B per target pixel) and, for a winner, its colour (4 B) and writes colour + depth (8 B); the clear writes 16 B per target pixel
    line("raw_tracked", r, size=[W, H], covered_px=cov, algorithmic_bytes=W * H * (4 + 16) + W * H * (8 + 16) + cov * 12)
    r = timed(raw_filtered_gui)
    line("raw_filtered_gui", r, size=[1024, 320], covered_px=int((t1.images(stream=sptr)[1] < 0xFFFFFF).sum()))
    line("clear_640x480", timed(lambda: t0.clear((0, 0, 0, 0), stream=sptr)))
    line("clear_1024x320", timed(lambda: t1.clear((0, 0, 0, 0), stream=sptr)))
    r = timed(map_points)
    line("map_points_tracked", r, size=[W, H], surfels=model.lastCount(), covered_px=int((t0.images(stream=sptr)[1] < 0xFFFFFF).sum()))
    line("compute_feedback", timed(lambda: ef.computeFeedbackBuffers(sptr)), bytes_copied=W * H * 12)
    t0.close()
    t1.close()
    ef.close()


if __name__ == "__main__":
    main()
