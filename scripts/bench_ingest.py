"""Measures JPEG colour decoding into device memory (include/dmslam_io_device.h) against the path without it: dms_jpeg_decode on
the host followed by dms_memcpy_h2d.

    python scripts/bench_ingest.py [--calls 40] [--repeats 5] [--frames 40] [--out profiles/ingest_bench.jsonl]

One JSON line per measurement, printed and appended to --out.  The paths are `parent` (host decode + copy; unchanged code in the
same build), `host_entropy` (sequential entropy stage on the host, back half on the device) and `device_S` (entropy decode on the
device with subsequences of S = 64, 128, 256 bytes).  Within one command the paths alternate; every figure is the median of
--repeats windows after a warm-up, with the minimum and maximum of the windows beside it.
  kind = "decode"   per stream (the 640x480 quality-95 fixture stream; a textured 640x480 stream generated from a seed):
                    host_ms    wall time of one call on the calling thread (the enqueue; for `parent` the whole decode and copy)
                    stream_us  HIP events on the producer stream around --calls back-to-back calls, per call
                    plus the device decoder's status (subsequences, rounds, settled lanes)
  kind = "frames"   frames/s of the loop decode -> dms_fusion_inputs_ready -> dms_fusion_process_frame over --frames synthetic
                    640x480 frames whose colour is JPEG (quality 90), a fresh map per window, the last fetch inside the window
  kind = "mono"     frames/s of the chain decode -> dms_depthnet_pack (the colour-only log of --predict_depth)
There is no pass / fail threshold.  Per-kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/bench_ingest.py --only decode`.
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 640, 480


def textured(seed):
    """a 640x480 image with detail at every scale: smooth shapes, edges and fine noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([128 + 90 * np.sin(x / 11.0) * np.cos(y / 7.0), 60 + 180 * x / (W - 1), 230 - 200 * y / (H - 1)], -1)
    img[((x // 23 + y // 17) % 2 == 0)] *= 0.6
    img += rng.normal(0, 12.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(rgb, quality=90):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb, np.uint8), "RGB").save(buf, "JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--only", default="", help="decode, frames or mono")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.jsonl"))
    args = ap.parse_args()

    import torch

    from densemonoslam_amd import capi, depthnet, fusion, synth
    from densemonoslam_amd import ingest as ing

    assert capi.device_count() >= 1, "bench_ingest.py needs a GPU"
    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream

    def line(**d):
        s = json.dumps(d)
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    def stats(v, name, nd=3):
        return {name: round(statistics.median(v), nd), name + "_min": round(min(v), nd), name + "_max": round(max(v), nd)}

    jd = ing.JpegDevice(W, H, max_stream_bytes=1 << 20, slots=3)
    rgb_dev = [capi.DeviceBuffer(W * H * 3) for _ in range(2)]
    host_rgb = np.zeros((H, W, 3), np.uint8)
    modes = [("parent", None), ("host_entropy", None), ("device_64", 64), ("device_128", 128), ("device_256", 256)]

    def decode(mode, S, data, dst):
        if mode == "parent":
            capi.check(capi.lib.dms_jpeg_decode(data, len(data), W, H, host_rgb.ctypes.data_as(C.c_void_p)), "dms_jpeg_decode")
            capi.check(capi.lib.dms_memcpy_h2d(C.c_void_p(dst.ptr), host_rgb.ctypes.data_as(C.c_void_p), C.c_size_t(host_rgb.nbytes), C.c_void_p(sptr)),
                       "dms_memcpy_h2d")
        else:
            if S:
                jd.set_subsequence_bytes(S)
            jd.decode(data, dst.ptr, entropy_on_host=(mode == "host_entropy"), stream=sptr)

    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    sources = [("fixture_q95_420_vga", z["q95_420_vga_jpeg"].tobytes()), ("textured_seed7_q90", encode(textured(7)))]

    if args.only in ("", "decode"):
        for name, data in sources:
            want = ing.jpeg_decode(data, W, H)
            res = {m: ([], []) for m, _ in modes}
            info = {}
            for m, S in modes:
                for _ in range(args.warmup):
                    decode(m, S, data, rgb_dev[0])
                torch.cuda.synchronize()
                assert np.array_equal(rgb_dev[0].download(np.uint8, (H, W, 3)), want), m
                if m.startswith("device"):
                    i = jd.status()
                    info[m] = dict(subsequences=i.subsequences, rounds=i.rounds, settled_lanes=i.settled_lanes)
            for _ in range(args.repeats):
                for m, S in modes:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record(stream)
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        decode(m, S, data, rgb_dev[0])
                    t1 = time.perf_counter()
                    b.record(stream)
                    b.synchronize()
                    res[m][0].append((t1 - t0) * 1000.0 / args.calls)
                    res[m][1].append(a.elapsed_time(b) * 1000.0 / args.calls)
            for m, _ in modes:
                line(kind="decode", stream=name, bytes=len(data), path=m, calls=args.calls, repeats=args.repeats, **stats(res[m][0], "host_ms"),
                     **stats(res[m][1], "stream_us", 1), **info.get(m, {}))

    frames = None
    if args.only in ("", "frames", "mono"):
        frames = [synth.frame(k, width=W, height=H, K=synth.K_640, noise=True) for k in range(args.frames)]
        jpgs = [encode(f[1]) for f in frames]

    if args.only in ("", "frames"):
        deps = [capi.DeviceBuffer(W * H * 2).upload(np.ascontiguousarray(f[0], np.uint16)) for f in frames]
        res = {m: [] for m, _ in modes}
        for rep in range(args.repeats + 1):  # the first window of every path is the warm-up
            for m, S in modes:
                g = fusion.ElasticFusion(W, H, synth.K_640, model_capacity=3000000)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.frames):
                    dst = rgb_dev[k & 1]
                    if k >= 2:
                        capi.check(capi.lib.dms_fusion_inputs_consumed(g.h, None), "dms_fusion_inputs_consumed")
                    decode(m, S, jpgs[k], dst)
                    g.inputsReady(sptr)
                    g.processFrameAsync(dst.ptr, 3, deps[k].ptr)
                r = g.fetch()
                t1 = time.perf_counter()
                g.close()
                if rep:
                    res[m].append(args.frames / (t1 - t0))
                surfels = int(r.surfels)
            del surfels
        for m, _ in modes:
            line(kind="frames", path=m, frames=args.frames, repeats=args.repeats, jpeg_bytes=int(statistics.median([len(j) for j in jpgs])),
                 **stats(res[m], "fps", 1))

    if args.only in ("", "mono"):
        tensor = torch.empty((1, 3, H, W), dtype=torch.float32, device="cuda")
        res = {m: [] for m, _ in modes}
        for rep in range(args.repeats + 1):
            for m, S in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.frames):
                    dst = rgb_dev[k & 1]
                    decode(m, S, jpgs[k], dst)
                    depthnet.pack(dst.ptr, 3, W, H, tensor.data_ptr(), False, sptr)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if rep:
                    res[m].append(args.frames / (t1 - t0))
        for m, _ in modes:
            line(kind="mono", path=m, frames=args.frames, repeats=args.repeats, **stats(res[m], "fps", 1))
    jd.close()


if __name__ == "__main__":
    main()
