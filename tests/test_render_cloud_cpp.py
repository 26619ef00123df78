"""The C++ adapter's FeedbackBuffer::render (densemonoslam_amd/cpp/dmslam.hpp, Context::feedbackBuffers in cpp/ElasticFusion.h): a host
compiled against the adapter only makes the calls of GUI/src/MainController.cpp:475-491 with the reference's argument types (stand-ins
for Eigen's 4 x 4 matrix and pangolin's column-major one) and, on the GPU, draws what the restatement (tests/render_cloud_ref.py)
draws."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cloud_ref as RC  # noqa: E402
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
K = (132.0, 132.0, 80.0, 60.0)

SRC = r"""
#include <cstdio>
#include <map>
#include <memory>
#include <vector>
namespace Eigen {
struct Matrix4f {
  float m[16];
  float& operator()(int r, int c) { return m[r * 4 + c]; }
  const float& operator()(int r, int c) const { return m[r * 4 + c]; }
};
}  // namespace Eigen
#define DMS_EIGEN_MATRIX4F_DECLARED 1
#include "densemonoslam_amd/cpp/ElasticFusion.h"

// what the reference passes as `mvp`: a matrix class with column-major doubles in m[16] (pangolin::OpenGlMatrix has that member)
struct ColumnMajorMatrix {
  double m[16];
};

int main(int argc, char** argv) {
  const int W = 160, H = 120;
  Resolution::getInstance(W, H);
  Intrinsics::getInstance(132.f, 132.f, 80.f, 60.f);
  ElasticFusion* eFusion = new ElasticFusion(200, 35000, 5e-05, 1e-05, false, false, false, 115, 1, 3, 10, false, 0.3095, true, false, "model",
                                             ElasticFusion::SamplingScheme::NONE, 0.8f, 0.7f, 500, 64, 0);
  Context& activeCtx = *(eFusion->frontend("logs/camera0.klg"));
  ColumnMajorMatrix viewMatrix = {};
  const bool showNormals = false, showColors = true;
  if (argc < 3) {  // CPU build check: the calls below compiled and linked; nothing touches the device
    delete eFusion;
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  int frames = 0;
  float mvp[16];
  if (!f || fread(&frames, 4, 1, f) != 1 || fread(mvp, 4, 16, f) != 16) return 2;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) viewMatrix.m[4 * c + r] = mvp[4 * r + c];
  std::shared_ptr<unsigned char> rgb(new unsigned char[(size_t)W * H * 3], std::default_delete<unsigned char[]>());
  std::shared_ptr<unsigned short> depth(new unsigned short[(size_t)W * H], std::default_delete<unsigned short[]>());
  for (int k = 0; k < frames; ++k) {
    if (fread(rgb.get(), 1, (size_t)W * H * 3, f) != (size_t)W * H * 3 || fread(depth.get(), 2, (size_t)W * H, f) != (size_t)W * H) return 2;
    eFusion->processFrame(rgb, depth, 1000 * k, activeCtx, nullptr, nullptr, nullptr, 0, 1.f, false);
  }
  fclose(f);
  dms_render_target* t = nullptr;
  if (dms_render_target_create(&t, W, H)) return 4;
  const float clear[4] = {0.f, 0.f, 0.f, 1.f};
  if (dms_render_clear(t, clear, nullptr)) return 5;
  activeCtx.bindRenderTarget(t);

  // the calls of MainController.cpp:475-491: refresh the buffers, then each buffer's render(mvp, pose, drawNormals, drawColors),
  // reached through the context's std::map by the reference's keys
  Eigen::Matrix4f framePose = activeCtx.currPose();
  activeCtx.computeFeedbackBuffers(eFusion->getMaxDepthProcessed());
  std::map<std::string, FeedbackBuffer*>& buffers = activeCtx.feedbackBuffers();
  if (buffers.size() != 2) return 10;
  FeedbackBuffer* rawCloud = buffers.at(FeedbackBuffer::RAW);
  FeedbackBuffer* filteredCloud = buffers.at(FeedbackBuffer::FILTERED);
  rawCloud->render(viewMatrix, framePose, showNormals, showColors);
  filteredCloud->render(viewMatrix, framePose, showNormals, showColors);

  dms_image2d c, d, k;
  if (dms_render_images(t, &c, &d, &k)) return 6;
  std::vector<unsigned> img((size_t)W * H), dep((size_t)W * H);
  std::vector<unsigned long long> key((size_t)W * H);
  dms_image2d in[3];
  if (dms_fusion_get_image(activeCtx.fusion, 0, &in[0]) || dms_fusion_get_image(activeCtx.fusion, 3, &in[1]) ||
      dms_fusion_get_image(activeCtx.fusion, 4, &in[2]))
    return 7;
  std::vector<unsigned> frame((size_t)W * H * 3);
  if (dms_memcpy_d2h(img.data(), c.data, img.size() * 4, nullptr) || dms_memcpy_d2h(dep.data(), d.data, dep.size() * 4, nullptr) ||
      dms_memcpy_d2h(key.data(), k.data, key.size() * 8, nullptr))
    return 8;
  for (int i = 0; i < 3; ++i)
    if (dms_memcpy_d2h(frame.data() + (size_t)i * W * H, in[i].data, (size_t)W * H * 4, nullptr)) return 9;
  f = fopen(argv[2], "wb");
  fwrite(img.data(), 4, img.size(), f);
  fwrite(dep.data(), 4, dep.size(), f);
  fwrite(key.data(), 8, key.size(), f);
  fwrite(frame.data(), 4, frame.size(), f);
  fwrite(framePose.m, 4, 16, f);
  fclose(f);
  dms_render_target_destroy(t);
  delete eFusion;
  printf("ok\n");
  return 0;
}
"""


def _build(td):
    src, exe = os.path.join(td, "host.cpp"), os.path.join(td, "host")
    with open(src, "w") as f:
        f.write(SRC)
    lib_dir = os.path.join(ROOT, "densemonoslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I" + ROOT, src, "-o", exe, "-L" + lib_dir, "-ldmslam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_call_site_compiles_and_links_against_the_adapter():
    with tempfile.TemporaryDirectory() as td:
        out = subprocess.run([_build(td)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_adapter_feedback_buffer_render():
    from densemonoslam_amd import capi, fusion, synth

    assert capi.device_count() >= 1
    frames = 3
    mvp = R.mvp_from_pose(fusion.render_frustum(W, H, 120, 120, W / 2, H / 2, 0.1, 100), np.eye(4, dtype=np.float32))
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(np.int32(frames).tobytes() + mvp.astype(np.float32).tobytes())
            for k in range(frames):
                d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
                f.write(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(d, np.uint16).tobytes())
        out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        raw = np.fromfile(outp, np.uint8)
    n = W * H
    img = raw[:n * 4].reshape(H, W, 4)
    dep = raw[n * 4:n * 8].view(np.uint32).reshape(H, W)
    key = raw[n * 8:n * 16].view(np.uint64).reshape(H, W)
    rgba = raw[n * 16:n * 20].reshape(H, W, 4)
    dm = raw[n * 20:n * 24].view(np.float32).reshape(H, W)
    dmf = raw[n * 24:n * 28].view(np.float32).reshape(H, W)
    pose = raw[n * 28:].view(np.float32).reshape(4, 4)
    ref = R.Target(W, H, (0, 0, 0, 1))
    RC.draw_cloud(ref, rgba, dm, K, 25.0, mvp, pose, 2)   # drawNormals off, drawColors on
    RC.draw_cloud(ref, rgba, dmf, K, 25.0, mvp, pose, 2)
    c, d, k = ref.images()
    assert (d < 0xFFFFFF).sum() > 500
    seq = (k[k != R.CLEARED] >> np.uint64(32)) & np.uint64(0xFF)
    assert (seq == 0).any() and (seq == 1).any(), "both clouds own pixels"
    assert np.array_equal(img, c) and np.array_equal(dep, d) and np.array_equal(key, k)
