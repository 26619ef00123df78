"""The C++ adapter's image panels (densemonoslam_amd/cpp/dmslam.hpp, cpp/ElasticFusion.h): a host compiled against the adapter only makes
the calls of GUI/src/MainController.cpp:649-664 with the reference's argument lists - eFusion->normaliseDepth(ctx, 0.3f, cutoff),
ctx.indexMap().renderDepth(cutoff), drawTex(), imageTex(), ctx.textures()[GPUTexture::RGB] - through a displayImg that looks the view's
rectangle up by name, and, on the GPU, draws what the restatement (tests/render_panels_ref.py) draws."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_panels_ref as P  # noqa: E402
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
K = (132.0, 132.0, 80.0, 60.0)
TW, TH = 200, 300
VIEWS = [(0, 225, 107, 75), (0, 150, 107, 75), (0, 75, 107, 75), (0, 0, 200, 75)]  # DEPTH_NORM, Model, RGB, ModelImage

SRC = r"""
#include <cstdio>
#include <map>
#include <memory>
#include <string>
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

// the GUI as the call site sees it: displayImg(id, texture) draws into the rectangle pangolin::Display(id) names, and depthCutoff->Get()
struct Var {
  float v;
  float Get() const { return v; }
};
struct GUI {
  dms_render_target* target;
  std::map<std::string, dms_viewport> views;
  Var cutoff;
  Var* depthCutoff;
  void displayImg(const std::string& id, GPUTexture* img) { dms::displayImg(target, views.at(id), img); }
};

int main(int argc, char** argv) {
  const int W = 160, H = 120;
  Resolution::getInstance(W, H);
  Intrinsics::getInstance(132.f, 132.f, 80.f, 60.f);
  ElasticFusion* eFusion = new ElasticFusion(200, 35000, 5e-05, 1e-05, false, false, false, 115, 2, 3, 10, false, 0.3095, true, false, "model",
                                             ElasticFusion::SamplingScheme::NONE, 0.8f, 0.7f, 500, 64, 0);
  Context& activeCtx = *(eFusion->frontend("logs/camera0.klg"));
  GUI guiObject;
  GUI* gui = &guiObject;
  gui->cutoff.v = 3.0f;
  gui->depthCutoff = &gui->cutoff;
  if (argc < 3) {  // CPU build check: the calls below compiled and linked; nothing touches the device
    delete eFusion;
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  int hdr[3 + 16];
  if (!f || fread(hdr, 4, 19, f) != 19) return 2;
  const int frames = hdr[0];
  const char* ids[4] = {GPUTexture::DEPTH_NORM.c_str(), "Model", GPUTexture::RGB.c_str(), "ModelImage"};
  for (int k = 0; k < 4; ++k) gui->views[ids[k]] = dms_viewport{hdr[3 + 4 * k], hdr[4 + 4 * k], hdr[5 + 4 * k], hdr[6 + 4 * k]};
  std::shared_ptr<unsigned char> rgb(new unsigned char[(size_t)W * H * 3], std::default_delete<unsigned char[]>());
  std::shared_ptr<unsigned short> depth(new unsigned short[(size_t)W * H], std::default_delete<unsigned short[]>());
  for (int k = 0; k < frames; ++k) {
    if (fread(rgb.get(), 1, (size_t)W * H * 3, f) != (size_t)W * H * 3 || fread(depth.get(), 2, (size_t)W * H, f) != (size_t)W * H) return 2;
    eFusion->processFrame(rgb, depth, 1000 * k, activeCtx, nullptr, nullptr, nullptr, 0, 1.f, false);
  }
  fclose(f);
  if (dms_render_target_create(&gui->target, hdr[1], hdr[2])) return 4;
  const float clear[4] = {0.f, 0.f, 0.f, 1.f};
  if (dms_render_clear(gui->target, clear, nullptr)) return 5;

  // the calls of MainController.cpp:649-664
  eFusion->normaliseDepth(activeCtx, 0.3f, gui->depthCutoff->Get());
  gui->displayImg(GPUTexture::DEPTH_NORM, activeCtx.textures()[GPUTexture::DEPTH_NORM]);
  activeCtx.indexMap().renderDepth(gui->depthCutoff->Get());
  gui->displayImg("Model", activeCtx.indexMap().drawTex());
  gui->displayImg(GPUTexture::RGB, activeCtx.textures()[GPUTexture::RGB]);
  gui->displayImg("ModelImage", activeCtx.indexMap().imageTex());

  dms_image2d c, in[4];
  if (dms_render_images(gui->target, &c, nullptr, nullptr)) return 6;
  const int ids_img[4] = {0, 1, 9, 10};
  const size_t bytes[4] = {4, 2, 4, 16};
  for (int i = 0; i < 4; ++i)
    if (dms_fusion_get_image(activeCtx.fusion, ids_img[i], &in[i])) return 7;
  std::vector<unsigned char> img((size_t)hdr[1] * hdr[2] * 4), frame((size_t)W * H * 26);
  if (dms_memcpy_d2h(img.data(), c.data, img.size(), nullptr)) return 8;
  size_t off = 0;
  for (int i = 0; i < 4; ++i) {
    if (dms_memcpy_d2h(frame.data() + off, in[i].data, (size_t)W * H * bytes[i], nullptr)) return 9;
    off += (size_t)W * H * bytes[i];
  }
  f = fopen(argv[2], "wb");
  fwrite(img.data(), 1, img.size(), f);
  fwrite(frame.data(), 1, frame.size(), f);
  fclose(f);
  dms_render_target_destroy(gui->target);
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
def test_cpp_adapter_draws_the_panel_column():
    from densemonoslam_amd import capi, synth

    assert capi.device_count() >= 1
    frames = 8  # the constructor above sets the confidence threshold to 2: the prediction is populated by then
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([frames, TW, TH] + [v for vp in VIEWS for v in vp], np.int32).tobytes())
            for k in range(frames):
                d, rgb, _ = synth.frame(k, width=W, height=H, K=K, noise=True)
                f.write(np.ascontiguousarray(rgb, np.uint8).tobytes() + np.ascontiguousarray(d, np.uint16).tobytes())
        out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        raw = np.fromfile(outp, np.uint8)
    n, t = W * H, TW * TH * 4
    img = raw[:t].reshape(TH, TW, 4)
    rgba = raw[t:t + 4 * n].reshape(H, W, 4)
    depth = raw[t + 4 * n:t + 6 * n].view(np.uint16).reshape(H, W)
    pimg = raw[t + 6 * n:t + 10 * n].reshape(H, W, 4)
    vertex = raw[t + 10 * n:].view(np.float32).reshape(H, W, 4)
    ref = R.Target(TW, TH, (0, 0, 0, 1))
    norm, model = P.draw_panels(ref, rgba, depth, pimg, vertex, VIEWS, 3.0)
    assert (norm > 0).sum() > 1000 and (model[..., 3] > 0).sum() > 1000
    assert np.array_equal(img, ref.color)
