"""The C++ adapter's DepthPrediction (densemonoslam_amd/cpp/DepthPrediction.h): a host compiled against the header only makes the
reference's calls - predict(rgb), depth() (GUI/src/MainController.cpp:319-320) - with the network plugged in as a callback, and, on the
GPU, gets the bytes of the C ABI and of the restatement (tests/depthnet_ref.py)."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthnet_ref as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 67, 30  # an odd width: the three-channel rows are no multiple of 4 bytes

SRC = r"""
#include <cstdio>
#include <memory>
#include <vector>
#include "densemonoslam_amd/cpp/DepthPrediction.h"

int main(int argc, char** argv) {
  if (argc < 3) return 0;  // CPU build check: the calls below compiled and linked; nothing touches the device
  FILE* f = fopen(argv[1], "rb");
  int hdr[4];
  if (!f || fread(hdr, 4, 4, f) != 4) return 2;
  const int W = hdr[0], H = hdr[1], half = hdr[2], mode = hdr[3];
  const size_t n = (size_t)W * H;
  std::shared_ptr<unsigned char> rgb(new unsigned char[n * 3], std::default_delete<unsigned char[]>());
  if (fread(rgb.get(), 1, n * 3, f) != n * 3) return 2;
  fclose(f);
  int calls = 0;
  // the stand-in network: its output is the second plane of its input (the green channel as metres), enqueued on the same (null) stream
  dms::DepthPrediction* depthPredictor = new dms::DepthPrediction(W, H, [&](void* input) -> void* {
    ++calls;
    return (char*)input + n * (half ? 2 : 4);
  }, half != 0, mode);
  depthPredictor->predict(rgb);
  std::vector<unsigned short> depth(n);
  if (dms_memcpy_d2h(depth.data(), depthPredictor->depth(), n * 2, depthPredictor->stream())) return 3;
  if (dms_stream_sync(depthPredictor->stream())) return 4;
  std::vector<unsigned char> input(n * 3 * (half ? 2 : 4));
  if (dms_memcpy_d2h(input.data(), depthPredictor->input(), input.size(), nullptr)) return 5;
  f = fopen(argv[2], "wb");
  fwrite(depth.data(), 2, n, f);
  fwrite(input.data(), 1, input.size(), f);
  fclose(f);
  delete depthPredictor;
  printf("ok %d\n", calls);
  return 0;
}
"""


def _build(td):
    src, exe = os.path.join(td, "host.cpp"), os.path.join(td, "host")
    with open(src, "w") as f:
        f.write(SRC)
    lib_dir = os.path.join(ROOT, "densemonoslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + ROOT, src, "-o", exe, "-L" + lib_dir, "-ldmslam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_call_site_compiles_and_links_against_the_adapter():
    with tempfile.TemporaryDirectory() as td:
        out = subprocess.run([_build(td)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_adapter_predicts_the_abis_bytes():
    from densemonoslam_amd import capi, depthnet

    assert capi.device_count() >= 1
    rgb = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    n = W * H
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        for half, mode in ((0, D.RUNTIME), (1, D.TRUNCATE)):
            inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
            with open(inp, "wb") as f:
                f.write(np.array([W, H, half, mode], np.int32).tobytes() + rgb.tobytes())
            out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0 and out.stdout.strip() == "ok 1", (out.returncode, out.stdout, out.stderr)
            raw = np.fromfile(outp, np.uint8)
            es, dt = (2, np.float16) if half else (4, np.float32)
            depth, tensor = raw[:2 * n].view(np.uint16).reshape(H, W), raw[2 * n:].view(dt).reshape(3, H, W)
            # the ABI's bytes for the same calls
            src, t_dev, d_dev = capi.DeviceBuffer(n * 3).upload(rgb), capi.DeviceBuffer(n * 3 * es), capi.DeviceBuffer(n * 2)
            depthnet.pack(src.ptr, 3, W, H, t_dev.ptr, half)
            depthnet.unpack(t_dev.ptr + n * es, half, W, H, d_dev.ptr, mode)
            assert np.array_equal(tensor.view(np.uint8), t_dev.download(dt, (3, H, W)).view(np.uint8))
            assert np.array_equal(depth, d_dev.download(np.uint16, (H, W)))
            # and the restatement's
            want = D.pack(rgb, bool(half))
            assert np.array_equal(tensor.view(np.uint8), want.view(np.uint8))
            assert np.array_equal(depth, D.unpack(want[1], mode)) and depth.max() > 900 and len(np.unique(depth)) > 200
