"""Measures the depth network's two tensor conversions (include/dmslam_depthnet.h) against the same conversions written in torch ops.

    python scripts/bench_depthnet.py [--calls 2000] [--repeats 5] [--out profiles/depthnet_bench.jsonl]

One JSON line per case (640 x 480 and 1241 x 376; fp32 and fp16; pack of an RGB8 image, unpack by the run-time rule), printed and
appended to --out.  Each form is timed by HIP events around --calls back-to-back calls on one stream after a warm-up, --repeats times,
the two forms alternating (median, minimum and maximum of the repeats in us per call; the time includes the host's enqueue where
that is the longer part, which it is for the torch form's several launches):
  us / us_min / us_max            the library's kernel, one launch per call
  torch_us / ...                  the torch-op form a user has without the library (`torch_ops` launches per call), written to give the
                                  same bits: the script checks that it does, and says so in `torch_same_bits`
  bytes, roof_us                  the bytes the conversion must move (input read once, output written once) and that over 8 TB/s
There is no pass / fail threshold.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_depthnet.py`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_US = 8e12 / 1e6  # the peak DESIGN.md §6 measures against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthnet_bench.jsonl"))
    args = ap.parse_args()

    import torch

    from densemonoslam_amd import capi, depthnet

    assert capi.device_count() >= 1, "bench_depthnet.py needs a GPU"
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.calls):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1000.0 / args.calls

    def timed_pair(ours, theirs):
        for fn in (ours, theirs):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t = ([], [])
        for _ in range(args.repeats):
            t[0].append(window(ours))
            t[1].append(window(theirs))
        stats = lambda us, p: {p + "us": round(statistics.median(us), 2), p + "us_min": round(min(us), 2), p + "us_max": round(max(us), 2)}
        return dict(stats(t[0], ""), **stats(t[1], "torch_"))

    def line(**d):
        s = json.dumps(d)
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    gen = torch.Generator(device="cpu").manual_seed(20260929)
    inv255 = torch.tensor(1.0 / 255.0, dtype=torch.float32, device=dev)
    for (W, H) in ((640, 480), (1241, 376)):
        n = W * H
        rgb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
        metres = (torch.rand((1, 1, H, W), generator=gen) * 71.0 - 1.0).to(dev)
        for half in (False, True):
            dt, es = (torch.float16, 2) if half else (torch.float32, 4)
            dp = depthnet.DepthPrediction(W, H, half_float=half)
            t32 = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
            t16 = torch.empty((1, 3, H, W), dtype=torch.float16, device=dev)
            chw = rgb.permute(2, 0, 1).unsqueeze(0)

            def pack_ours():
                depthnet.pack(rgb.data_ptr(), 3, W, H, dp.input.data_ptr(), half, sptr)

            def pack_torch():
                torch.mul(chw, inv255, out=t32)  # uint8 x float32 -> float32: one fp32 product per value, transposed on the way
                if half:
                    t16.copy_(t32)
                return t16 if half else t32

            same = bool(torch.equal(dp.pack(rgb), pack_torch()))
            line(case="pack", image=[W, H], channels=3, half=half, calls=args.calls, repeats=args.repeats, bytes=n * 3 + 3 * n * es,
                 roof_us=round((n * 3 + 3 * n * es) / HBM_BYTES_PER_US, 3), torch_ops=2 if half else 1, torch_same_bits=same,
                 **timed_pair(pack_ours, pack_torch))

            x = metres.to(dt).contiguous()
            depth = dp.depth

            def unpack_ours():
                depthnet.unpack(x.data_ptr(), half, W, H, depth.data_ptr(), depthnet.RUNTIME, sptr)

            def unpack_torch():
                r = x.float() * 1000.0 if half else x * 1000.0
                v = torch.round(r)  # half to even
                fits = v.abs() < 2147483648.0  # false for NaN and the infinities
                v = torch.where(fits, v.clamp(0.0, 65535.0), 0.0)
                return v.to(torch.int32).to(torch.int16)  # the u16 bits

            same = bool(torch.equal(dp.unpack(x).view(torch.int16), unpack_torch().view(H, W)))
            line(case="unpack", image=[W, H], half=half, mode="runtime", calls=args.calls, repeats=args.repeats, bytes=n * es + n * 2,
                 roof_us=round((n * es + n * 2) / HBM_BYTES_PER_US, 3), torch_ops=8 if half else 7, torch_same_bits=same,
                 **timed_pair(unpack_ours, unpack_torch))


if __name__ == "__main__":
    main()
