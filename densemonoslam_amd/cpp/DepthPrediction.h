// C++ mirror of the reference's DepthPrediction (GUI/src/Tools/DepthPrediction.h:16-75) over the C ABI of include/dmslam_depthnet.h.
//
//   DepthPrediction::predict(rgb)  (DepthPrediction.cpp:106-169)  -> dms::DepthPrediction::predict(rgb_dev) / predict(host image)
//   DepthPrediction::depth()       (DepthPrediction.h:24)         -> dms::DepthPrediction::depth(): the u16 millimetre image, in HBM
//
// Header-only.  The network stays with the caller, as Deformation::constrain does in ElasticFusion.h: `inference` is called with the
// device address of the packed [1, 3, H, W] input tensor (fp32, or fp16 with half_float) and returns the device address of its
// [1, 1, H, W] output in metres (same precision), having ENQUEUED its work on the stream this object was given (or on a stream it
// has ordered behind and before that one).  The two conversions around it run in libdmslam_hip.so with the reference's bits.
// Nothing here synchronises the host, except the upload of a host image in the reference's own signature.
#pragma once
#include <cstddef>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/dmslam.h"
#include "../../include/dmslam_depthnet.h"
#include "../../include/dmslam_fusion.h"

namespace dms {

class DepthPrediction {
 public:
  using Inference = std::function<void*(void* input_tensor_dev)>;

  // the reference reads width and height from Resolution::getInstance() and half_float from its model's name (DepthPrediction.cpp:3-30)
  DepthPrediction(int width, int height, Inference inference, bool half_float = false, int mode = DMS_DEPTHNET_RUNTIME,
                  dms_stream stream = nullptr)
      : width_(width), height_(height), half_(half_float), mode_(mode), stream_(stream), inference_(std::move(inference)) {
    if (width <= 0 || height <= 0) throw std::invalid_argument("DepthPrediction: width and height must be positive");
    if (mode != DMS_DEPTHNET_RUNTIME && mode != DMS_DEPTHNET_TRUNCATE) throw std::invalid_argument("DepthPrediction: unknown mode");
    const size_t n = (size_t)width * height;
    ok(dms_device_alloc(&input_, n * 3 * (half_ ? 2 : 4)), "dms_device_alloc");
    ok(dms_device_alloc((void**)&depth_, n * 2), "dms_device_alloc");
    ok(dms_device_alloc(&rgb_, n * 3), "dms_device_alloc");
    ok(dms_memset(depth_, 0, n * 2, stream_), "dms_memset");
  }
  ~DepthPrediction() {
    dms_stream_sync(stream_);
    dms_device_free(input_);
    dms_device_free(depth_);
    dms_device_free(rgb_);
  }
  DepthPrediction(const DepthPrediction&) = delete;
  DepthPrediction& operator=(const DepthPrediction&) = delete;

  // rgb_dev: the frame's colour image in HBM, rgb_channels (3 or 4) bytes per pixel; pack -> inference -> unpack, all enqueued
  void predict(const void* rgb_dev, int rgb_channels = 3) {
    if (!inference_) throw std::runtime_error("DepthPrediction: no inference callback");
    ok(dms_depthnet_pack(rgb_dev, rgb_channels, width_, height_, input_, half_ ? 1 : 0, stream_), "dms_depthnet_pack");
    const void* out = inference_(input_);
    ok(dms_depthnet_unpack(out, half_ ? 1 : 0, width_, height_, depth_, mode_, stream_), "dms_depthnet_unpack");
    last_rgb_ = rgb_dev;
    last_channels_ = rgb_channels;
  }
  // the reference's signature: a host RGB8 image of width x height pixels, staged through an owned device image
  void predict(const std::shared_ptr<unsigned char>& rgb) {
    ok(dms_memcpy_h2d(rgb_, rgb.get(), (size_t)width_ * height_ * 3, stream_), "dms_memcpy_h2d");
    predict(rgb_, 3);
  }

  unsigned short* depth() const { return depth_; }  // device address; complete in stream order behind predict()
  void* input() const { return input_; }
  int width() const { return width_; }
  int height() const { return height_; }
  bool halfFloat() const { return half_; }
  dms_stream stream() const { return stream_; }

  // The camera loop's next statement (MainController.cpp:373): the frame step on the image of the last predict() and its depth.
  // With pipeline_ingest the frame reads both on a stream of its own, which dms_fusion_inputs_ready orders behind this object's
  // stream (dmslam_depthnet.h "Hand-over"); call waitConsumed(f, frame_stream) before the next predict() overwrites them.
  // With pipeline_ingest = 0 the frame reads them on frame_stream itself: give it this object's stream.
  void processFrame(dms_fusion* f, const float* inPose16 = nullptr, float weightMultiplier = 1.f, dms_stream frame_stream = nullptr) {
    if (!last_rgb_) throw std::runtime_error("DepthPrediction::processFrame before predict");
    ok(dms_fusion_inputs_ready(f, stream_), "dms_fusion_inputs_ready");
    ok(dms_fusion_process_frame(f, last_rgb_, last_channels_, depth_, inPose16, weightMultiplier, frame_stream), "dms_fusion_process_frame");
  }
  static void waitConsumed(dms_fusion* f, dms_stream frame_stream = nullptr) {
    ok(dms_fusion_inputs_consumed(f, frame_stream), "dms_fusion_inputs_consumed");
  }

 private:
  static void ok(int rc, const char* what) {
    if (rc != DMS_OK) throw std::runtime_error(std::string(what) + ": " + dms_last_error());
  }
  int width_, height_;
  bool half_;
  int mode_;
  dms_stream stream_;
  Inference inference_;
  void* input_ = nullptr;
  unsigned short* depth_ = nullptr;
  void* rgb_ = nullptr;
  const void* last_rgb_ = nullptr;
  int last_channels_ = 3;
};

}  // namespace dms
