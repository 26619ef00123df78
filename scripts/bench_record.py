"""Measures recording from device memory (include/dmslam_io_write.h) against the path without it: dms_memcpy_d2h of the raw
frame, dms_jpeg_encode and compress2 on the host, append.

    python scripts/bench_record.py [--calls 20] [--repeats 5] [--frames 30] [--out profiles/record_bench.jsonl]

One JSON line, printed and appended to --out, for 640x480 frames at quality 90 (the colour is the 640x480 case of
tests/golden/jpeg_encode_cases.npz, whose bytes every path must reproduce; the depth a synthetic frame's):
  encode_ms          dms_jpeg_enc_encode + dms_jpeg_enc_result per frame, wall time, for entropy_on_host = 0 ("device") and 1 ("host")
  klg_fps            dms_klg_writer_append_device (compressed) frames/s into a file, in both entropy modes
  host_path_ms/_fps  dms_memcpy_d2h + dms_jpeg_encode + dms_deflate + dms_klg_writer_append per frame
Every figure is the median of --repeats windows after a warm-up, the paths alternating, minimum and maximum beside it.  There is no
pass / fail threshold.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_bench.jsonl"))
    args = ap.parse_args()

    from densemonoslam_amd import capi, synth
    from densemonoslam_amd import ingest as ing
    from tests import jpeg_encode_cases as jc

    assert capi.device_count() >= 1, "bench_record.py needs a GPU"
    case = jc.by_name(jc.VGA)
    depth = np.ascontiguousarray(synth.frame(3, width=W, height=H, K=synth.K_640, noise=True)[0], np.uint16)
    rgb_dev, depth_dev = capi.DeviceBuffer(W * H * 3), capi.DeviceBuffer(W * H * 2)
    rgb_dev.upload(case.rgb)
    depth_dev.upload(depth)
    st = capi.create_stream()
    je = ing.JpegDeviceEncoder(W, H, slots=3)
    host_rgb, host_depth = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint16)
    tmp = tempfile.mkdtemp()

    def stats(v, nd=3):
        return [round(statistics.median(v), nd), round(min(v), nd), round(max(v), nd)]

    def encode(on_host):
        je.encode(rgb_dev.ptr, 90, ing.JPEG_420, entropy_on_host=on_host, stream=st)
        return je.result()

    def klg_device(on_host, n):
        je.set_entropy_on_host(on_host)
        w = ing.KlgWriter(os.path.join(tmp, "dev.klg"))
        for k in range(n):
            w.append_device(je, depth_dev.ptr, rgb_dev.ptr, k, compressed=True, quality=90, stream=st)
        w.close()

    def klg_host(n):
        w = ing.KlgWriter(os.path.join(tmp, "host.klg"))
        for k in range(n):
            capi.check(capi.lib.dms_memcpy_d2h(host_depth.ctypes.data_as(C.c_void_p), C.c_void_p(depth_dev.ptr), C.c_size_t(host_depth.nbytes), C.c_void_p(st)))
            capi.check(capi.lib.dms_memcpy_d2h(host_rgb.ctypes.data_as(C.c_void_p), C.c_void_p(rgb_dev.ptr), C.c_size_t(host_rgb.nbytes), C.c_void_p(st)))
            capi.check(capi.lib.dms_stream_sync(C.c_void_p(st)))
            w.append(k, ing.deflate(host_depth.tobytes()), ing.jpeg_encode(host_rgb, 90))
        w.close()

    for on_host in (False, True):
        for _ in range(args.warmup):
            assert encode(on_host) == case.jpeg
    klg_device(False, args.warmup)
    klg_device(True, args.warmup)
    klg_host(args.warmup)
    assert open(os.path.join(tmp, "dev.klg"), "rb").read() == open(os.path.join(tmp, "host.klg"), "rb").read()

    enc = {False: [], True: []}
    fps = {False: [], True: []}
    host = []
    for _ in range(args.repeats):
        for on_host in (False, True):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                encode(on_host)
            enc[on_host].append((time.perf_counter() - t0) * 1000.0 / args.calls)
        for on_host in (False, True):
            t0 = time.perf_counter()
            klg_device(on_host, args.frames)
            fps[on_host].append(args.frames / (time.perf_counter() - t0))
        t0 = time.perf_counter()
        klg_host(args.frames)
        host.append((time.perf_counter() - t0) * 1000.0 / args.frames)
    je.set_entropy_on_host(ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST)
    out = dict(kind="record", width=W, height=H, quality=90, jpeg_bytes=len(case.jpeg), calls=args.calls, frames=args.frames, repeats=args.repeats,
               encode_ms=dict(device=stats(enc[False]), host=stats(enc[True])),
               klg_fps=dict(device=stats(fps[False], 1), host=stats(fps[True], 1)),
               host_path_ms=stats(host), host_path_fps=stats([1000.0 / v for v in host], 1),
               default_entropy_on_host=ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST, stats="median, min, max")
    s = json.dumps(out)
    print(s, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(s + "\n")
    je.close()
    capi.destroy_stream(st)


if __name__ == "__main__":
    main()
