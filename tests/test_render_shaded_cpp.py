"""The C++ adapter's GUI::drawFXAA (densemonoslam_amd/cpp/dmslam.hpp, dms::ShadedView): a host compiled against the adapter only
calls it with the reference's arguments and the GUI's toggles; the view's bytes equal the Python path's (fusion.ShadedView)."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <vector>
#include "densemonoslam_amd/cpp/dmslam.hpp"

int main(int argc, char** argv) {
  const int W = 160, H = 120, SW = 320, SH = 240;
  FILE* f = fopen(argv[1], "rb");
  unsigned n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  std::vector<float> rec((size_t)n * (12 + DMS_MAX_SENSORS));
  if (fread(rec.data(), 4, rec.size(), f) != rec.size()) return 2;
  float mvp[16], mv[16];
  if (fread(mvp, 4, 16, f) != 16 || fread(mv, 4, 16, f) != 16) return 2;
  fclose(f);
  dms::GlobalModel model(W, H, 4096);
  if (dms_model_upload(model.h, rec.data(), n, nullptr)) return 3;
  dms::ShadedView view(W, H, SW, SH);
  const float clear[4] = {0.f, 0.f, 0.f, 1.f};
  view.clearView(clear);
  // MainController.cpp:505-510: drawFXAA(mvp, mv, model, confidence, tick, id, timeDelta, iclnuim), then the GUI's toggles
  // (normals, colours, times, unstable, window, showcase)
  view.drawFXAA(mvp, mv, model, 10.f, 7, 0, 3, false, false, true, false, true, true, false);
  dms_image2d c, d, k;
  if (dms_render_images(view.target, &c, &d, &k)) return 6;
  std::vector<unsigned> img((size_t)W * H), dep((size_t)W * H);
  std::vector<unsigned long long> key((size_t)W * H);
  if (dms_memcpy_d2h(img.data(), c.data, img.size() * 4, nullptr) || dms_memcpy_d2h(dep.data(), d.data, dep.size() * 4, nullptr) ||
      dms_memcpy_d2h(key.data(), k.data, key.size() * 8, nullptr))
    return 7;
  f = fopen(argv[2], "wb");
  fwrite(img.data(), 4, img.size(), f);
  fwrite(dep.data(), 4, dep.size(), f);
  fwrite(key.data(), 8, key.size(), f);
  fclose(f);
  printf("ok\n");
  return 0;
}
"""


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_adapter_draw_fxaa():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1
    W, H = 160, 120
    rng = np.random.default_rng(7)
    n = 600
    s = np.zeros(n, fusion.SURFEL_DTYPE)
    s["pos"][:, :3] = rng.uniform([-0.8, -0.6, 1.0], [0.8, 0.6, 2.5], (n, 3))
    s["pos"][:, 3] = rng.uniform(0, 20, n)
    nr = rng.normal(size=(n, 3))
    nr[:, 2] = -np.abs(nr[:, 2]) - 0.5
    s["nrm"][:, :3] = nr / np.linalg.norm(nr, axis=1, keepdims=True)
    s["nrm"][:, 3] = rng.uniform(0.01, 0.05, n)
    s["col"][:, 0] = rng.integers(0, 1 << 24, n).astype(np.float32)
    s["times"][:] = -3
    s["times"][:, 0] = rng.integers(0, 8, n)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.05, -0.02, 0.1)
    mvp = R.mvp_from_pose(fusion.render_frustum(320, 240, 260, 260, 160, 120, 0.1, 100), pose)
    mv = R.mvp_from_pose(np.eye(4, dtype=np.float32), pose)
    lib_dir = os.path.join(ROOT, "densemonoslam_amd")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "host.cpp"), os.path.join(td, "host")
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(src, "w") as f:
            f.write(SRC)
        with open(inp, "wb") as f:
            f.write(np.uint32(n).tobytes() + s.tobytes() + mvp.astype(np.float32).tobytes() + mv.astype(np.float32).tobytes())
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I" + ROOT, src, "-o", exe, "-L" + lib_dir, "-ldmslam_hip",
                               "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
        out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        raw = np.fromfile(outp, np.uint8)
    img = raw[:W * H * 4].reshape(H, W, 4)
    dep = raw[W * H * 4:W * H * 8].view(np.uint32).reshape(H, W)
    key = raw[W * H * 8:].view(np.uint64).reshape(H, W)
    m = fusion.GlobalModel(W, H, capacity=4096)
    m.upload(s)
    v = fusion.ShadedView(W, H, offscreen=(320, 240))
    v.clear((0, 0, 0, 1))
    v.drawFXAA(mvp, mv, m, 10.0, 7, 0, 3, False, drawColors=True, drawUnstable=True, drawWindow=True)
    c, d, k = v.images()
    v.close()
    m.close()
    assert (d < 0xFFFFFF).sum() > 500
    assert np.array_equal(img, c) and np.array_equal(dep, d) and np.array_equal(key, k)
