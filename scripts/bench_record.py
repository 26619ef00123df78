"""Measures recording from device memory (include/dmslam_io_write.h) against the path without it: dms_memcpy_d2h of the raw
frame, dms_jpeg_encode and compress2 on the host, append.

    python scripts/bench_record.py [--calls 20] [--repeats 5] [--frames 30] [--out profiles/record_bench.jsonl]
    python scripts/bench_record.py --deflate-only N      N device deflates and nothing else, for a kernel trace; writes no row

One JSON line, printed and appended to --out, for 640x480 frames at quality 90 (the colour is the 640x480 case of
tests/golden/jpeg_encode_cases.npz, whose bytes every path must reproduce; the depth a synthetic frame's):
  encode_ms          dms_jpeg_enc_encode + dms_jpeg_enc_result per frame, wall time, for entropy_on_host = 0 ("device") and 1 ("host")
  klg_fps            dms_klg_writer_append_device (compressed) frames/s into a file, in both entropy modes
  host_path_ms/_fps  dms_memcpy_d2h + dms_jpeg_encode + dms_deflate + dms_klg_writer_append per frame
  deflate_ms         the depth frame deflated: "device" dms_deflate_dev_encode + dms_deflate_dev_result, "host_default" dms_deflate
                     (compress2 at the default level), "host_level1" zlib.compress(x, 1) (the same libz, the reference's converters'
                     setting), "host_blocks" dms_deflate_blocks; one thread each, the depth already on the side that deflates it
  deflate_bytes      what each of them writes
  klg_fps_depth_on_device, lcm_fps / lcm_fps_depth_on_device
                     the append_device loops with dms_jpeg_enc_set_depth_on_device(1), and the LCM-log loop in both depth modes
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
import zlib

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
    ap.add_argument("--deflate-only", type=int, default=0)
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

    dd = ing.DeflateDeviceEncoder(depth.nbytes, slots=3)
    depth_bytes = depth.tobytes()

    def deflate_device():
        dd.encode(depth_dev.ptr, depth.nbytes, stream=st)
        return dd.result()

    if args.deflate_only:
        for _ in range(args.deflate_only):
            deflate_device()
        dd.close()
        return

    def lcm_device(z_on_device, n):
        je.set_entropy_on_host(ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST)
        je.set_depth_on_device(z_on_device)
        w = ing.LcmLogWriter(os.path.join(tmp, "dev.lcm"))
        for k in range(n):
            w.append_frame_device(je, "EFUSION_FRAMES", depth_dev.ptr, rgb_dev.ptr, k, frameNumber=k, senderName="bench", compressed=True, quality=90, stream=st)
        w.close()
        je.set_depth_on_device(ing.RECORD_DEFAULT_DEPTH_ON_DEVICE)

    def klg_device(on_host, n, z_on_device=False):
        je.set_entropy_on_host(on_host)
        je.set_depth_on_device(z_on_device)
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
    z_blocks = ing.deflate_blocks(depth_bytes)
    for _ in range(args.warmup):
        assert deflate_device() == z_blocks
    assert zlib.decompress(z_blocks) == depth_bytes
    klg_device(False, args.warmup, True)
    assert len(open(os.path.join(tmp, "dev.klg"), "rb").read()) == 4 + args.warmup * (16 + len(z_blocks) + len(case.jpeg))
    lcm_device(True, args.warmup)
    lcm_device(False, args.warmup)

    enc = {False: [], True: []}
    fps = {False: [], True: []}
    host = []
    dfl = dict(device=[], host_default=[], host_level1=[], host_blocks=[])
    fps_z = {False: [], True: []}
    lcm = {False: [], True: []}

    def per_call(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1000.0 / n

    for _ in range(args.repeats):
        dfl["device"].append(per_call(deflate_device, args.calls))
        dfl["host_default"].append(per_call(lambda: ing.deflate(depth_bytes), 3))
        dfl["host_level1"].append(per_call(lambda: zlib.compress(depth_bytes, 1), 5))
        dfl["host_blocks"].append(per_call(lambda: ing.deflate_blocks(depth_bytes), 5))
        for on_host in (False, True):
            t0 = time.perf_counter()
            klg_device(on_host, args.frames, True)
            fps_z[on_host].append(args.frames / (time.perf_counter() - t0))
        for z_on_device in (False, True):
            t0 = time.perf_counter()
            lcm_device(z_on_device, args.frames)
            lcm[z_on_device].append(args.frames / (time.perf_counter() - t0))
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
               deflate_ms={k: stats(v) for k, v in dfl.items()},
               deflate_bytes=dict(device=len(z_blocks), host_default=len(ing.deflate(depth_bytes)), host_level1=len(zlib.compress(depth_bytes, 1)),
                                  host_blocks=len(z_blocks), raw=len(depth_bytes)),
               klg_fps_depth_on_device=dict(device=stats(fps_z[False], 1), host=stats(fps_z[True], 1)),
               lcm_fps=stats(lcm[False], 1), lcm_fps_depth_on_device=stats(lcm[True], 1),
               default_depth_on_device=ing.RECORD_DEFAULT_DEPTH_ON_DEVICE,
               default_entropy_on_host=ing.JPEG_ENC_DEFAULT_ENTROPY_ON_HOST, stats="median, min, max")
    s = json.dumps(out)
    print(s, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(s + "\n")
    je.close()
    dd.close()
    capi.destroy_stream(st)


if __name__ == "__main__":
    main()
