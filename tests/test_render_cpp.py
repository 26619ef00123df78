"""The C++ adapter's GlobalModel::renderPointCloud (densemonoslam_amd/cpp/dmslam.hpp): a host compiled against the adapter only calls
it with the reference's arguments, clusters included, on the GPU; its image equals the restatement's (tests/render_ref.py)."""
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
  const int W = 160, H = 120;
  FILE* f = fopen(argv[1], "rb");
  unsigned n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  std::vector<float> rec((size_t)n * (12 + DMS_MAX_SENSORS));
  if (fread(rec.data(), 4, rec.size(), f) != rec.size()) return 2;
  float mvp[16];
  if (fread(mvp, 4, 16, f) != 16) return 2;
  fclose(f);
  dms::GlobalModel model(W, H, 4096);
  if (dms_model_upload(model.h, rec.data(), n, nullptr)) return 3;
  dms_render_target* t = nullptr;
  if (dms_render_target_create(&t, W, H)) return 4;
  const float clear[4] = {0.f, 0.f, 0.f, 1.f};
  if (dms_render_clear(t, clear, nullptr)) return 5;
  model.bindRenderTarget(t);
  std::vector<std::tuple<float, float, float>> colors = {std::make_tuple(0.2f, 0.7f, 0.9f)};
  // MainController.cpp:518-527: renderPointCloud(mvp, confidence, drawUnstable, drawNormals, drawColors, drawPoints, drawWindow,
  // drawTimes, drawContributions, tick, id, timeDelta, clusters(), drawClusters, colors); a cluster the map does not have is skipped
  model.renderPointCloud(mvp, 10.f, true, false, true, false, true, false, false, 7, 0, 3, model.clusters(), true, colors);
  model.renderPointCloud(mvp, 10.f, false, true, false, false, false, false, false, 7, 0, 3, std::vector<int>{0, 5}, false, {});
  dms_image2d c, d;
  if (dms_render_images(t, &c, &d, nullptr)) return 6;
  std::vector<unsigned> img((size_t)W * H), dep((size_t)W * H);
  if (dms_memcpy_d2h(img.data(), c.data, img.size() * 4, nullptr) || dms_memcpy_d2h(dep.data(), d.data, dep.size() * 4, nullptr)) return 7;
  f = fopen(argv[2], "wb");
  fwrite(img.data(), 4, img.size(), f);
  fwrite(dep.data(), 4, dep.size(), f);
  fclose(f);
  dms_render_target_destroy(t);
  printf("ok\n");
  return 0;
}
"""


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_adapter_render_point_cloud():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1
    W, H = 160, 120
    rng = np.random.default_rng(5)
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
    mvp = R.mvp_from_pose(fusion.render_frustum(W, H, 130, 130, W / 2, H / 2, 0.1, 100), pose)
    lib_dir = os.path.join(ROOT, "densemonoslam_amd")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "host.cpp"), os.path.join(td, "host")
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(src, "w") as f:
            f.write(SRC)
        with open(inp, "wb") as f:
            f.write(np.uint32(n).tobytes() + s.tobytes() + mvp.astype(np.float32).tobytes())
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I" + ROOT, src, "-o", exe, "-L" + lib_dir, "-ldmslam_hip",
                               "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
        out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        raw = np.fromfile(outp, np.uint32)
    img = raw[:W * H].view(np.uint8).reshape(H, W, 4)
    dep = raw[W * H:].reshape(H, W)
    ref = R.Target(W, H, (0, 0, 0, 1))
    ref.draw(s, mvp, threshold=10.0, draw_unstable=True, color_type=2, draw_window=True, time=7, time_idx=0, time_delta=3,
             cluster_color=(0.2, 0.7, 0.9))
    ref.draw(s, mvp, threshold=10.0, color_type=1, time=7, time_delta=3)
    c, d, _ = ref.images()
    assert (d < 0xFFFFFF).sum() > 500
    assert np.array_equal(img, c) and np.array_equal(dep, d)
