"""Measurements of the deformation-graph solver; prints one JSON line per table.

  solve   the time of one dms_deform_constrain for (nodes, constraints) = (60, 300), (130, 768), (512, 768), (2047, 768), each constraint
          with its pin, between two events on the stream (median and spread over --reps solves after --warmup)
  frames  frames/s of a 640 x 480 stream with local_loop_closure on which loops are accepted (columns of the depth zeroed on frames
          2-4, as tests/test_deform_frame_gpu.py), the loop solver ON against OFF - OFF is what the library did before it had the solver:
          the loop is found and dropped - and of a stream on which no loop is accepted (timeDelta = 200: the INACTIVE view stays empty), ON against OFF: that difference is the cost of
          the mid-frame read of the loop's verdict.  ON and OFF runs alternate (A B A B ...), one context each, same frames.

    python scripts/bench_deform.py [--reps 20] [--warmup 3] [--rounds 4] [--frames 12] [--out profiles/deform_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def solve_table(args):
    import torch

    from densemonoslam_amd import deform
    from tests import deform_cases

    rows = []
    for n, m in ((60, 300), (130, 768), (512, 768), (2047, 768)):
        c = deform_cases.Case("n%d_c%d" % (n, m), n, m, 40 + n)
        d = deform.Deformation(max_nodes=n, max_constraints=m)
        ms = []
        for rep in range(args.warmup + args.reps):
            d.setNodes(c.nodes)
            d.setLastDeformTime(0)
            d.addConstraints(c.rows, c.src_time, True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            d.constrain(c.time)
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                ms.append(a.elapsed_time(b))
        r = d.result()
        rows.append(dict(nodes=n, constraints=m, unknowns=12 * r.enabled_nodes, rows=r.rows, iterations=r.iterations, exit_reason=r.exit_reason,
                         status=r.status, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)), reps=len(ms)))
        d.close()
    return dict(table="solve", rows=rows)


def _stream(fusion, synth, frames, closing):
    W, H, K = 640, 480, (528.0, 528.0, 320.0, 240.0)
    out = []
    for k in range(frames):
        d, rgb, _ = synth.frame(k % 6 if closing else k, width=W, height=H, K=K, noise=True)
        if closing and 2 <= k % 6 <= 4:
            d = d.copy()
            d[:, : int(W * 0.35)] = 0
        out.append((rgb, d))
    return out


def frame_table(args):
    from densemonoslam_amd import fusion, synth

    W, H, K = 640, 480, (528.0, 528.0, 320.0, 240.0)
    rows = []
    for closing in (True, False):
        # timeDelta = 2 makes the INACTIVE view populated, so loops are found and accepted; with the default 200 it stays empty over
        # these few frames and no loop is ever accepted: what is left of the solver is the mid-frame read of the verdict
        opts = dict(model_capacity=2500000, timeDelta=2 if closing else 200, confidence=1.0, local_loop_closure=True)
        frames = _stream(fusion, synth, args.frames, closing)
        fps = {True: [], False: []}
        deforms = 0
        for rnd in range(args.rounds):
            for on in (True, False):  # A B A B ...
                g = fusion.ElasticFusion(W, H, K, **opts)
                if on:
                    g.setLoopSolver(True, 5000)
                g.processFrame(*frames[0])  # the bootstrap frame is not timed
                t0 = time.perf_counter()
                for rgb, d in frames[1:]:
                    g.processFrame(rgb, d)
                fps[on].append((len(frames) - 1) / (time.perf_counter() - t0))
                if on:
                    deforms = g.deforms()
                g.close()
        rows.append(dict(stream="loops accepted" if closing else "plain", frames=len(frames) - 1, rounds=args.rounds, loops_closed_per_run=deforms,
                         ms_per_frame_on=1e3 / float(np.median(fps[True])), ms_per_frame_off=1e3 / float(np.median(fps[False])), fps_on_median=float(np.median(fps[True])),
                         fps_off_median=float(np.median(fps[False])), fps_on=fps[True], fps_off=fps[False]))
    return dict(table="frames", rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--skip-solve", action="store_true")
    args = ap.parse_args()
    tables = [] if args.skip_solve else [solve_table(args)]
    if not args.skip_frames:
        tables.append(frame_table(args))
    for t in tables:
        line = json.dumps(t)
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
