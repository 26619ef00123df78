"""Measures the view's image panels (include/dmslam_render_panels.h) on the benchmark stream.

    python scripts/bench_render_panels.py [--frames 25] [--draws 400] [--repeats 5] [--out profiles/render_panels_bench.jsonl]

The context is the one bench.py's 20-step form leaves (5 warm-up + 20 steps of the 640 x 480 synthetic stream).  One JSON line per case,
printed and appended to --out, each timed by HIP events over --draws calls after a warm-up, --repeats times (median, minimum and maximum
of the repeats in us per call; the time includes the host's enqueue where that is the longer part):
  separate_gui / fused_gui      the column as six launches (normaliseDepth, renderDepth, four blits) and as one
                                (dms_fusion_draw_panels), 640 x 480 images into four 297 x 93 panels: the cell of the reference's
                                window (a fifth of 1485 px wide, aspect 1024 / 320; GUI/src/Tools/GUI.h:40-42, 77-83, 110-123;
                                pangolin's own layout arithmetic is not restated);
  separate_strip / fused_strip  the same into one 1024 x 320 target, four 256 x 320 panels side by side;
  passes_only                   normaliseDepth + renderDepth alone (two launches);
  frame_step                    this process's frame step on the same stream, ms per frame over the last --step-frames frames
                                (host time from call to fetch, the way a viewer's loop sees it), for the column's share of a frame.
There is no pass / fail threshold.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_render_panels.py`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--step-frames", type=int, default=20)
    ap.add_argument("--draws", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_panels_bench.jsonl"))
    args = ap.parse_args()

    import torch

    from densemonoslam_amd import fusion, synth

    W, H = 640, 480
    K = synth.K_640
    ef = fusion.ElasticFusion(W, H, K, model_capacity=8_000_000)
    n_unique = min(args.frames, 32)
    step_ms = []
    for k in range(args.frames):
        period = 2 * (n_unique - 1)
        j = k % period
        j = j if j < n_unique else period - j
        d, rgb, _ = synth.frame(j, width=W, height=H, K=K, noise=True)
        t0 = time.perf_counter()
        ef.processFrame(rgb, d)
        step_ms.append((time.perf_counter() - t0) * 1000.0)
    step_ms = step_ms[-args.step_frames:]
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)

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
        s = json.dumps(dict({"case": case, "draws": args.draws, "repeats": args.repeats}, **t, **more))
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    step = statistics.median(step_ms)
    gui_vps = [(0, 93 * (3 - k), 297, 93) for k in range(4)]
    strip_vps = [(256 * k, 0, 256, 320) for k in range(4)]
    t_gui, t_strip, p = fusion.RenderTarget(297, 372), fusion.RenderTarget(1024, 320), fusion.Panels(W, H)
    cut = 3.0
    views = [fusion.Image2D() for _ in range(2)]
    fusion.check(fusion.lib.dms_fusion_get_image(ef.h, 1, C.byref(views[0])))
    fusion.check(fusion.lib.dms_fusion_get_image(ef.h, 10, C.byref(views[1])))

    def passes():
        fusion.check(fusion.lib.dms_depth_norm(p.h, C.byref(views[0]), 300.0, cut * 1000.0, sptr))
        fusion.check(fusion.lib.dms_model_depth_image(p.h, C.byref(views[1]), cut, sptr))

    for name, t, vps in (("gui", t_gui, gui_vps), ("strip", t_strip, strip_vps)):
        px = sum(v[2] * v[3] for v in vps)
        for form, fn, launches in (("separate", ef.drawPanelsSeparately, 6), ("fused", ef.drawPanels, 1)):
            r = timed(lambda: fn(t, p, vps, cut, stream=sptr))
            line("%s_%s" % (form, name), r, launches=launches, image=[W, H], panel=list(vps[0][2:]), panel_px=px,
                 share_of_frame_step=round(r["us"] / (step * 1000.0), 5))
    line("passes_only", timed(passes), launches=2, image=[W, H])
    line("frame_step", {"ms": round(step, 3), "ms_min": round(min(step_ms), 3), "ms_max": round(max(step_ms), 3)}, frames=len(step_ms))
    for o in (t_gui, t_strip, p, ef):
        o.close()


if __name__ == "__main__":
    main()
