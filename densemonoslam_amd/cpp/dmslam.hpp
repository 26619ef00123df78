// C++ mirror of the reference's elasticfusion/Core classes over the C ABI of libdmslam_hip.so.
//
// Header-only; no Eigen / Pangolin / CUDA needed.  Matrices cross as plain row-major float
// arrays; when <Eigen/Core> is available the overloads at the bottom accept the reference's own
// argument types (Eigen::Vector3f, Eigen::Matrix<float,3,3,RowMajor>, Eigen::Matrix4f) so that
// GUI/src/MainController.cpp, Core/src/ElasticFusion.cpp and GPUTest.cpp call sites compile
// unchanged against these classes.
//
//   reference class / method                                   -> here
//   RGBDOdometry (Core/src/Utils/RGBDOdometry.h:32-153)        -> dms::RGBDOdometry
//   GPUTexture   (Core/src/GPUTexture.h:29-57)                 -> dms::DeviceTexture (pitched HBM image)
//   GlobalModel  (Core/src/GlobalModel.h:43-141)               -> dms::GlobalModel
//   IndexMap     (Core/src/IndexMap.h:33-205)                  -> dms::IndexMap
//   ElasticFusion::processFrame (ElasticFusion.h:92-100)       -> dms::ElasticFusion::processFrame
//   Ferns        (Core/src/Ferns.h:35-266)                     -> dms::Ferns
//   GUI::drawFXAA (GUI/src/Tools/GUI.h:365-478)                -> dms::ShadedView::drawFXAA
//   FeedbackBuffer::render (Shaders/FeedbackBuffer.cpp:145-187) -> dms::FeedbackBuffer::render
//   GUI::displayImg (GUI/src/Tools/GUI.h:340-350)                -> dms::displayImg(target, viewport, GPUTexture*)
#pragma once
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/dmslam.h"
#include "../../include/dmslam_deform.h"
#include "../../include/dmslam_ferns.h"
#include "../../include/dmslam_fusion.h"
#include "../../include/dmslam_render.h"
#include "../../include/dmslam_render_cloud.h"
#include "../../include/dmslam_render_panels.h"
#include "../../include/dmslam_render_shaded.h"

namespace dms {

inline void check(int rc, const char* what) {
  if (rc != DMS_OK) throw std::runtime_error(std::string(what) + ": " + dms_last_error());
}

// Pitched device image; replaces GPUTexture (GL texture + cudaGraphicsResource) in the kept API.
class DeviceTexture {
 public:
  DeviceTexture(int width, int height, size_t elemBytes) : width(width), height(height), elem(elemBytes) {
    check(dms_device_alloc(&ptr, (size_t)width * height * elemBytes), "dms_device_alloc");
    view.data = ptr;
    view.pitch = (size_t)width * elemBytes;
    view.rows = height;
    view.cols = width;
  }
  // a view of an image the library owns (a context's fill-in / prediction textures, dms_fusion_get_image): nothing is allocated or freed
  DeviceTexture(const dms_image2d& existing, size_t elemBytes)
      : ptr(existing.data), view(existing), width(existing.cols), height(existing.rows), elem(elemBytes), owned(false) {}
  ~DeviceTexture() {
    if (owned) dms_device_free(ptr);
  }
  DeviceTexture(const DeviceTexture&) = delete;
  DeviceTexture& operator=(const DeviceTexture&) = delete;
  // GPUTexture::texture->Upload(ptr, format, type) (ElasticFusion.cpp:111-114, GPUTest.cpp:39,59)
  void Upload(const void* host, dms_stream s = nullptr) { check(dms_memcpy_h2d(ptr, host, (size_t)width * height * elem, s), "upload"); }
  void Download(void* host, dms_stream s = nullptr) const { check(dms_memcpy_d2h(host, ptr, (size_t)width * height * elem, s), "download"); }
  const dms_image2d* image() const { return &view; }
  void* ptr = nullptr;
  dms_image2d view;
  const int width, height;
  const size_t elem;
  const bool owned = true;
};

class RGBDOdometry {
 public:
  RGBDOdometry(int width, int height, float cx, float cy, float fx, float fy, float distThresh = 0.10f, float angleThresh = 0.0f) {
    check(dms_odometry_create(&h, width, height, cx, cy, fx, fy, distThresh, angleThresh), "dms_odometry_create");
  }
  virtual ~RGBDOdometry() { dms_odometry_destroy(h); }
  RGBDOdometry(const RGBDOdometry&) = delete;

  void initICP(DeviceTexture* filteredDepth, const float depthCutoff, dms_stream stream = nullptr) {
    check(dms_odometry_initICP_depth(h, filteredDepth->image(), depthCutoff, stream), "initICP");
  }
  void initICP(DeviceTexture* predictedVertices, DeviceTexture* predictedNormals, const float depthCutoff, dms_stream stream = nullptr) {
    check(dms_odometry_initICP_maps(h, (const float*)predictedVertices->ptr, (const float*)predictedNormals->ptr, depthCutoff, stream), "initICP");
  }
  void initICPModel(DeviceTexture* predictedVertices, DeviceTexture* predictedNormals, const float depthCutoff, const float* modelPose16,
                    dms_stream stream = nullptr) {
    check(dms_odometry_initICPModel(h, (const float*)predictedVertices->ptr, (const float*)predictedNormals->ptr, depthCutoff, modelPose16,
                                    stream),
          "initICPModel");
  }
  void initRGB(DeviceTexture* rgb, dms_stream stream = nullptr) { check(dms_odometry_initRGB(h, rgb->image(), stream), "initRGB"); }
  void initRGBModel(DeviceTexture* rgb, dms_stream stream = nullptr) { check(dms_odometry_initRGBModel(h, rgb->image(), stream), "initRGBModel"); }
  void initFirstRGB(DeviceTexture* rgb, dms_stream s = nullptr) { check(dms_odometry_initFirstRGB(h, rgb->image(), s), "initFirstRGB"); }

  // trans[3], rot[9] row-major, in/out — RGBDOdometry::getIncrementalTransformation (RGBDOdometry.cpp:268)
  void getIncrementalTransformation(float* trans, float* rot, const bool& rgbOnly, const float& icpWeight, const bool& pyramid,
                                    const bool& fastOdom, const bool& so3, const bool interMap = false, dms_stream stream = nullptr) {
    dms_track_result r;
    check(dms_odometry_getIncrementalTransformation(h, trans, rot, rgbOnly, icpWeight, pyramid, fastOdom, so3, interMap, &r, stream),
          "getIncrementalTransformation");
    lastICPError = r.lastICPError;
    lastICPCount = r.lastICPCount;
    lastRGBError = r.lastRGBError;
    lastRGBCount = r.lastRGBCount;
    lastSO3Error = r.lastSO3Error;
    lastSO3Count = r.lastSO3Count;
    for (int i = 0; i < 36; ++i) lastA[i] = r.lastA[i];
    for (int i = 0; i < 6; ++i) lastb[i] = r.lastb[i];
  }
  void getCovariance(double* cov36) { check(dms_odometry_getCovariance(h, cov36), "getCovariance"); }

  float lastICPError = 0, lastICPCount = 0, lastRGBError = 0, lastRGBCount = 0, lastSO3Error = 0, lastSO3Count = 0;
  double lastA[36] = {0};
  double lastb[6] = {0};
  dms_odometry* h = nullptr;
};

class GlobalModel {
 public:
  static const int TEXTURE_DIMENSION = 5700;  // GlobalModel.cpp:22
  GlobalModel(int width, int height, size_t capacity = 0) : owned(true) { check(dms_model_create(&h, capacity, width, height), "dms_model_create"); }
  // a view of a frame step's map: `ctx` = the context that owns the per-cluster buffers (GlobalModel.h:93-109)
  explicit GlobalModel(dms_model* borrowed, dms_fusion* ctx = nullptr) : h(borrowed), ctx(ctx), owned(false) {}
  virtual ~GlobalModel() {
    if (owned) dms_model_destroy(h);
  }
  unsigned int lastCount() {
    unsigned int n = 0;
    check(dms_model_count(h, &n, nullptr), "lastCount");
    return n;
  }
  // GlobalModel::downloadMap (GlobalModel.cpp:866-896): reference 15-float records
  std::vector<float> downloadMap() {
    unsigned int n = lastCount(), got = 0;
    std::vector<float> v((size_t)n * 15);
    check(dms_model_download_ref(h, v.data(), n, &got, nullptr), "downloadMap");
    v.resize((size_t)got * 15);
    return v;
  }
  // GlobalModel::consume (GlobalModel.cpp:898-993): append `other` moved by the row-major 4x4 relativeTransform
  void consume(GlobalModel& other, const float* relativeTransform16) { check(dms_model_consume(h, other.h, relativeTransform16, nullptr), "consume"); }
  // GlobalModel::clusters / isCluster (GlobalModel.cpp:251-264)
  std::vector<int> clusters() {
    std::vector<int> ids(1, 0);
    if (ctx) {
      int n = 0;
      check(dms_fusion_clusters(ctx, nullptr, 0, &n, nullptr), "clusters");
      ids.assign((size_t)n, 0);
      check(dms_fusion_clusters(ctx, ids.data(), n, &n, nullptr), "clusters");
    }
    return ids;
  }
  bool isCluster(const int cluster) {
    for (int c : clusters())
      if (c == cluster) return true;
    return false;
  }
  // The framebuffer the draw goes into (the reference draws into whatever GL framebuffer is bound): a dms_render_target, cleared by
  // the host (dms_render_clear) as the GUI clears its view, and the stream the draws are enqueued on.
  void bindRenderTarget(dms_render_target* t, dms_stream s = nullptr) {
    target = t;
    target_stream = s;
  }
  // GlobalModel::renderPointCloud (GlobalModel.cpp:419-505): the reference's arguments in the reference's order; mvp is row-major
  // (pangolin's OpenGlMatrix is column-major: transpose it, e.g. with transposed16).  colorType precedence of :436-440, one draw per
  // cluster into the bound target (:458-503), cluster_colors[i] for clusters[i] when drawClusters.
  void renderPointCloud(const float* mvp16, const float threshold, const bool drawUnstable, const bool drawNormals, const bool drawColors,
                        const bool drawPoints, const bool drawWindow, const bool drawTimes, const bool drawContributions, const int time,
                        const int timeIdx, const int timeDelta, std::vector<int> clusters, bool drawClusters,
                        std::vector<std::tuple<float, float, float>> cluster_colors) {
    if (!target) throw std::runtime_error("renderPointCloud: no render target bound (bindRenderTarget)");
    dms_render_params p = {};
    for (int k = 0; k < 16; ++k) p.mvp[k] = mvp16[k];
    p.threshold = threshold;
    p.draw_unstable = drawUnstable;
    p.draw_points = drawPoints;
    p.draw_window = drawWindow;
    p.color_type = drawContributions ? 4 : drawNormals ? 1 : drawColors ? 2 : drawTimes ? 3 : 0;
    p.time = time;
    p.time_idx = timeIdx;
    p.time_delta = timeDelta;
    p.use_cluster_color = drawClusters;
    for (size_t i = 0; i < clusters.size(); i++) {
      if (drawClusters) {
        p.cluster_color[0] = std::get<0>(cluster_colors[i]);
        p.cluster_color[1] = std::get<1>(cluster_colors[i]);
        p.cluster_color[2] = std::get<2>(cluster_colors[i]);
      }
      dms_model* m = ctx ? dms_fusion_cluster_model(ctx, clusters[i]) : (clusters[i] == 0 ? h : nullptr);
      if (!m) continue;  // a cluster without buffers draws nothing
      check(dms_render_draw(target, m, &p, target_stream), "renderPointCloud");
    }
  }
  static void transposed16(const double* column_major16, float* row_major16) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) row_major16[4 * r + c] = (float)column_major16[4 * c + r];
  }
  dms_render_target* target = nullptr;
  dms_stream target_stream = nullptr;
  dms_model* h = nullptr;
  dms_fusion* ctx = nullptr;

 private:
  bool owned;
};

// GUI::drawFXAA (GUI/src/Tools/GUI.h:365-478): the offscreen float buffer (default the GUI's 3840 x 2160) and the view it is
// resolved into.  The host clears the view (clearView) as the GUI clears its window; drawFXAA draws one map into it.
class ShadedView {
 public:
  ShadedView(int width, int height, int offscreenWidth = DMS_RENDER_OFFSCREEN_WIDTH, int offscreenHeight = DMS_RENDER_OFFSCREEN_HEIGHT,
             dms_stream s = nullptr)
      : stream(s) {
    check(dms_render_target_create(&target, width, height), "dms_render_target_create");
    if (int rc = dms_render_offscreen_create(&offscreen, offscreenWidth, offscreenHeight)) {
      dms_render_target_destroy(target);
      check(rc, "dms_render_offscreen_create");
    }
  }
  ~ShadedView() {
    dms_render_offscreen_destroy(offscreen);
    dms_render_target_destroy(target);
  }
  ShadedView(const ShadedView&) = delete;
  ShadedView& operator=(const ShadedView&) = delete;
  void clearView(const float rgba[4]) { check(dms_render_clear(target, rgba, stream), "clearView"); }
  // The reference's arguments in the reference's order, then the GUI's toggles.  mvp16 and mv16 are row-major (pangolin's
  // OpenGlMatrix is column-major: transpose it, e.g. with GlobalModel::transposed16); lightpos is mv's translation column
  // (GUI.h:404-408), signMult +1 with invertNormals, else -1 (:393), colorType normals 1, colours 2, times 3, else 0 (:395-398).
  // timeIdx is the call's own (GUI.h:389 passes time: DESIGN.md §2.6).
  void drawFXAA(const float* mvp16, const float* mv16, GlobalModel& model, const float threshold, const int time, const int timeIdx,
                const int timeDelta, const bool invertNormals, const bool drawNormals, const bool drawColors, const bool drawTimes,
                const bool drawUnstable, const bool drawWindow, const bool showcaseMode) {
    dms_render_params p = {};
    for (int k = 0; k < 16; ++k) p.mvp[k] = mvp16[k];
    p.threshold = threshold;
    p.draw_unstable = drawUnstable;
    p.draw_window = drawWindow;
    p.color_type = drawNormals ? 1 : drawColors ? 2 : drawTimes ? 3 : 0;
    p.time = time;
    p.time_idx = timeIdx;
    p.time_delta = timeDelta;
    const float lightpos[3] = {mv16[3], mv16[7], mv16[11]};
    const float clear[4] = {showcaseMode ? 1.f : 0.05f, showcaseMode ? 1.f : 0.05f, showcaseMode ? 1.f : 0.3f, 0.f};
    check(dms_render_shaded_draw(offscreen, model.h, &p, lightpos, invertNormals ? 1.f : -1.f, clear, stream), "drawFXAA");
    check(dms_render_fxaa(target, offscreen, stream), "drawFXAA");
  }
  dms_render_target* target = nullptr;
  dms_render_offscreen* offscreen = nullptr;
  dms_stream stream = nullptr;
};

// FeedbackBuffer (Shaders/FeedbackBuffer.h): the RAW or FILTERED live-frame cloud of one camera, for its render().  The buffer's
// content is the context's (dms_fusion_compute_feedback); like GlobalModel it draws into a bound dms_render_target.
template <class Dummy>
struct FeedbackBufferNames {
  static const std::string RAW, FILTERED;
};
template <class Dummy>
const std::string FeedbackBufferNames<Dummy>::RAW = "RAW";
template <class Dummy>
const std::string FeedbackBufferNames<Dummy>::FILTERED = "FILTERED";

class FeedbackBuffer : public FeedbackBufferNames<void> {
 public:
  // ctx: where the owning camera keeps its dms_fusion (created by its first frame); which: DMS_CLOUD_RAW / DMS_CLOUD_FILTERED
  FeedbackBuffer(dms_fusion* const* ctx, int which) : ctx(ctx), which(which) {}
  void bindRenderTarget(dms_render_target* t, dms_stream s = nullptr) {
    target = t;
    target_stream = s;
  }
  // FeedbackBuffer::render(mvp, pose, drawNormals, drawColors) with the reference's argument types: mvp a pangolin::OpenGlMatrix
  // (anything with a column-major m[16]), transposed here as for the map draw; pose an Eigen::Matrix4f (anything with (r, c))
  template <class GlMatrix, class Mat4>
  void render(const GlMatrix& mvp, const Mat4& pose, const bool drawNormals, const bool drawColors) {
    float mvp16[16], pose16[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        mvp16[4 * r + c] = (float)mvp.m[4 * c + r];
        pose16[4 * r + c] = pose(r, c);
      }
    render16(mvp16, pose16, drawNormals, drawColors);
  }
  // the same with row-major arrays
  void render16(const float* mvp16, const float* pose16, const bool drawNormals, const bool drawColors) {
    if (!target) throw std::runtime_error("FeedbackBuffer::render: no render target bound (bindRenderTarget)");
    if (!*ctx) throw std::runtime_error("FeedbackBuffer::render: the camera has not processed a frame yet");
    dms_render_cloud_params p = {};
    for (int k = 0; k < 16; ++k) {
      p.mvp[k] = mvp16[k];
      p.model_pose[k] = pose16[k];
    }
    p.color_type = drawNormals ? 1 : drawColors ? 2 : 0;  // FeedbackBuffer.cpp:154
    check(dms_fusion_render_cloud(target, *ctx, which, &p, target_stream), "FeedbackBuffer::render");
  }
  dms_render_target* target = nullptr;
  dms_stream target_stream = nullptr;

 private:
  dms_fusion* const* ctx;
  int which;
};

// ---- the image panels (include/dmslam_render_panels.h; GUI/src/MainController.cpp:649-664) ---------------------------------------------
// GPUTexture (GPUTexture.h) as GUI::displayImg sees one: a device image, its format, and the filter its `draw` flag selected
// (Context.h:158-181: RGB and DEPTH_NORM LINEAR; IndexMap.cpp:42-65: drawTexture and imageTexture NEAREST).
template <class Dummy>
struct GPUTextureNames {
  static const std::string RGB, DEPTH_RAW, DEPTH_NORM;
};
template <class Dummy>
const std::string GPUTextureNames<Dummy>::RGB = "RGB";
template <class Dummy>
const std::string GPUTextureNames<Dummy>::DEPTH_RAW = "DEPTH";
template <class Dummy>
const std::string GPUTextureNames<Dummy>::DEPTH_NORM = "DEPTH_NORM";

struct GPUTexture : public GPUTextureNames<void> {
  GPUTexture() { view.data = nullptr, view.pitch = 0, view.rows = view.cols = 0; }
  GPUTexture(const dms_image2d& v, int format, int filter) : view(v), format(format), filter(filter) {}
  dms_image2d view;
  int format = DMS_PANEL_RGBA8, filter = DMS_PANEL_NEAREST;
};

// GUI::displayImg (GUI/src/Tools/GUI.h:340-350) with the view's rectangle given instead of looked up in pangolin: the image upside
// down over `vp` of `target`, times the current colour (the reference sets white just before, MainController.cpp:658)
inline void displayImg(dms_render_target* target, const dms_viewport& vp, const GPUTexture* img, dms_stream s = nullptr, float r = 1.f,
                       float g = 1.f, float b = 1.f) {
  const float color[3] = {r, g, b};
  check(dms_render_blit(target, &img->view, img->format, img->filter, &vp, color, s), "displayImg");
}

// what Context::indexMap() hands the GUI: renderDepth(depthCutoff), drawTex() and imageTex() of the camera's ACTIVE prediction
class PanelIndexMap {
 public:
  PanelIndexMap(dms_fusion* const* ctx, dms_panels* const* panels, dms_stream const* stream) : ctx(ctx), panels(panels), stream(stream) {}
  void renderDepth(const float depthCutoff) {  // IndexMap::renderDepth (IndexMap.cpp:219-251)
    dms_image2d v;
    check(dms_fusion_get_image(*ctx, 10, &v), "dms_fusion_get_image");
    check(dms_model_depth_image(*panels, &v, depthCutoff, *stream), "IndexMap::renderDepth");
  }
  GPUTexture* drawTex() {
    dms_image2d m;
    check(dms_panels_images(*panels, nullptr, &m), "dms_panels_images");
    draw = GPUTexture(m, DMS_PANEL_RGBA8, DMS_PANEL_NEAREST);
    return &draw;
  }
  GPUTexture* imageTex() {
    dms_image2d v;
    check(dms_fusion_get_image(*ctx, 9, &v), "dms_fusion_get_image");
    image = GPUTexture(v, DMS_PANEL_RGBA8, DMS_PANEL_NEAREST);
    return &image;
  }

 private:
  dms_fusion* const* ctx;
  dms_panels* const* panels;
  dms_stream const* stream;
  GPUTexture draw, image;
};

// IndexMap (IndexMap.h:39-162): the render targets of one camera and the three "draws" over a GlobalModel.
// pose = device dms_pose_block (dms_pose_block_set); K = (fx, fy, cx, cy).
class IndexMap {
 public:
  IndexMap(int width, int height)
      : index(width, height, 4), vertConf(width, height, 16), colorTime(width, height, 16), normRad(width, height, 16),
        image(width, height, 4), vertex(width, height, 16), normal(width, height, 16), time(width, height, 2), depth(width, height, 4) {
    check(dms_device_alloc((void**)&zbuf, (size_t)width * height * 8), "dms_device_alloc");
    check(dms_device_alloc((void**)&pose, sizeof(dms_pose_block)), "dms_device_alloc");
  }
  ~IndexMap() {
    dms_device_free(zbuf);
    dms_device_free(pose);
  }
  IndexMap(const IndexMap&) = delete;
  void setPose(const float* pose16, dms_stream s = nullptr) { check(dms_pose_block_set(pose, pose16, s), "dms_pose_block_set"); }
  // IndexMap::predictIndices (IndexMap.cpp:146-217)
  void predictIndices(const float* pose16, const int& time, const int& timeIdx, GlobalModel& model, const dms_camera& K, const float depthCutoff,
                      const int timeDelta, dms_stream s = nullptr) {
    setPose(pose16, s);
    dms_indexmap_out o = {index.view, vertConf.view, colorTime.view, normRad.view};
    check(dms_index_map(model.h, pose, &K, time, timeIdx, depthCutoff, timeDelta, zbuf, &o, s), "predictIndices");
  }
  // IndexMap::combinedPredict (IndexMap.cpp:253-368); predictionType: 1 = ACTIVE, 0 = INACTIVE
  void combinedPredict(const float* pose16, GlobalModel& model, const dms_camera& K, const float depthCutoff, const float confThreshold,
                       const int time, const int timeIdx, const int maxTime, const int timeDelta, int predictionType, dms_stream s = nullptr) {
    setPose(pose16, s);
    dms_predict_out o = {image.view, vertex.view, normal.view, this->time.view};
    check(dms_splat_predict(model.h, pose, &K, depthCutoff, confThreshold, time, timeIdx, maxTime, timeDelta, predictionType, zbuf, &o, s),
          "combinedPredict");
  }
  // IndexMap::synthesizeDepth (IndexMap.cpp:370-452)
  void synthesizeDepth(const float* pose16, GlobalModel& model, const dms_camera& K, const float depthCutoff, const float confThreshold,
                       const int time, const int timeIdx, const int maxTime, const int timeDelta, dms_stream s = nullptr) {
    setPose(pose16, s);
    check(dms_splat_depth(model.h, pose, &K, depthCutoff, confThreshold, time, timeIdx, maxTime, timeDelta, zbuf, &depth.view, s),
          "synthesizeDepth");
  }
  DeviceTexture index, vertConf, colorTime, normRad;  // indexTex / vertConfTex / colorTimeTex / normalRadTex
  DeviceTexture image, vertex, normal, time;          // imageTex / vertexTex / normalTex / timeTex
  DeviceTexture depth;                                // depthTex
  unsigned long long* zbuf = nullptr;
  dms_pose_block* pose = nullptr;
};

// Ferns (Ferns.h:35-266): the per-map keyframe database; textures = full-resolution RGBA8 / RGBA32F DeviceTextures
class Ferns {
 public:
  Ferns(int n, int maxDepth, const float photoThresh, int width, int height, float cx, float cy, float fx, float fy, unsigned seed = 0,
        int capacity = 4096) {
    check(dms_ferns_create(&h, n, maxDepth, photoThresh, width, height, cx, cy, fx, fy, seed, capacity), "dms_ferns_create");
  }
  virtual ~Ferns() { dms_ferns_destroy(h); }
  Ferns(const Ferns&) = delete;
  bool addFrame(DeviceTexture* imageTexture, DeviceTexture* vertexTexture, DeviceTexture* normalTexture, const float* pose16, int srcTime,
                const float threshold, dms_stream s = nullptr) {
    int added = 0;
    check(dms_ferns_add_frame(h, imageTexture->image(), vertexTexture->image(), normalTexture->image(), pose16, srcTime, threshold, &added, s),
          "addFrame");
    return added != 0;
  }
  // returns the estimated pose in match.estPose, lastClosest in match.closest; constraints = rows {raw xyz1 | model xyz1}
  dms_fern_match findFrame(std::vector<float>& constraints, const float* currPose16, DeviceTexture* vertexTexture, DeviceTexture* normalTexture,
                           DeviceTexture* imageTexture, const int time, const bool lost, const bool interMap = false, dms_stream s = nullptr) {
    dms_fern_match m;
    constraints.assign(8 * 64, 0.f);
    check(dms_ferns_find_frame(h, vertexTexture->image(), normalTexture->image(), imageTexture->image(), currPose16, time, lost, interMap, &m,
                               constraints.data(), s),
          "findFrame");
    constraints.resize((size_t)m.n_constraints * 8);
    lastClosest = m.closest;
    return m;
  }
  // Ferns::consume (Ferns.cpp:160-168)
  int consume(Ferns& other, const float* relativeTransform16, const float threshold, dms_stream s = nullptr) {
    int added = 0;
    check(dms_ferns_consume(h, other.h, relativeTransform16, threshold, &added, s), "consume");
    return added;
  }
  int frames() { return dms_ferns_num_frames(h); }
  int lastClosest = -1;
  dms_ferns* h = nullptr;
};

class ElasticFusion {
 public:
  // the constructor arguments of the reference that reach the hot path (ElasticFusion.cpp:22-73)
  ElasticFusion(int width, int height, float fx, float fy, float cx, float cy, const int timeDelta = 200, const float confidence = 10,
                const float depthCut = 3, const float icpThresh = 10, const bool fastOdom = false, const bool so3 = true,
                const bool frameToFrameRGB = false) {
    dms_fusion_params p;
    dms_fusion_default_params(&p, width, height, fx, fy, cx, cy);
    p.timeDelta = timeDelta;
    p.confidence = confidence;
    p.depthCut = depthCut;
    p.icpWeight = icpThresh;
    p.fastOdom = fastOdom;
    p.so3 = so3;
    p.frameToFrameRGB = frameToFrameRGB;
    check(dms_fusion_create(&h, &p), "dms_fusion_create");
  }
  // every option of dms_fusion_params (NID key-framing --nid/--ndw/--npl, hybrid tracking, pipelining ...)
  explicit ElasticFusion(const dms_fusion_params& p) { check(dms_fusion_create(&h, &p), "dms_fusion_create"); }
  virtual ~ElasticFusion() { dms_fusion_destroy(h); }
  ElasticFusion(const ElasticFusion&) = delete;

  // rgb (RGB8) and depth (u16 mm) already in HBM; inPose 4×4 row-major or nullptr
  void processFrame(const unsigned char* rgb_dev, const unsigned short* depth_dev, const float* inPose = nullptr,
                    const float weightMultiplier = 1.f, dms_stream s = nullptr) {
    check(dms_fusion_process_frame(h, rgb_dev, 3, depth_dev, inPose, weightMultiplier, s), "processFrame");
  }
  dms_frame_result fetch(dms_stream s = nullptr) {
    dms_frame_result r;
    check(dms_fusion_fetch(h, &r, s), "fetch");
    return r;
  }
  // local loop closure (ElasticFusion.cpp:399-497): the frame step in two halves around Deformation::constrain
  void processFrameBegin(const unsigned char* rgb_dev, const unsigned short* depth_dev, const float* inPose = nullptr,
                         const float weightMultiplier = 1.f, dms_stream s = nullptr) {
    check(dms_fusion_process_frame_begin(h, rgb_dev, 3, depth_dev, inPose, weightMultiplier, s), "processFrameBegin");
  }
  dms_frame_result fetchLoop(dms_stream s = nullptr) {
    dms_frame_result r;
    check(dms_fusion_fetch_loop(h, &r, s), "fetchLoop");
    return r;
  }
  // rows of {worldRawPoint, worldModelPoint, source time}: the arguments of Deformation::addConstraint (:468-470)
  std::vector<float> loopConstraints(int count) {
    std::vector<float> rows((size_t)count * 7);
    int n = 0;
    check(dms_fusion_get_loop_constraints(h, rows.data(), count, &n), "loopConstraints");
    rows.resize((size_t)(n < count ? n : count) * 7);
    return rows;
  }
  void processFrameEnd(const float* rawGraph = nullptr, int nodes = 0, const float* newPose = nullptr, dms_stream s = nullptr) {
    check(dms_fusion_process_frame_end(h, rawGraph, nodes, newPose, s), "processFrameEnd");
  }
  GlobalModel getGlobalModel() { return GlobalModel(dms_fusion_model(h)); }
  // the frame step closes its local loops itself: Deformation::constrain on the GPU (dmslam_deform.h)
  void setLoopSolver(bool on = true, int sampleRate = 5000) { check(dms_fusion_set_loop_solver(h, on ? 1 : 0, sampleRate), "setLoopSolver"); }
  int getDeforms() { return dms_fusion_get_deforms(h); }
  dms_deform* localDeformation() { return dms_fusion_deformation(h); }
  std::vector<float> relativeConstraints() {
    int n = 0;
    check(dms_fusion_get_relative_constraints(h, nullptr, 0, &n), "relativeConstraints");
    std::vector<float> rows((size_t)n * 8);
    check(dms_fusion_get_relative_constraints(h, rows.data(), n, &n), "relativeConstraints");
    return rows;
  }
  dms_fusion* h = nullptr;
};

// Deformation (Core/src/Deformation.h) for absolute and pin constraints, fernMatch = false: the solver of dmslam_deform.h
class DeformationSolver {
 public:
  DeformationSolver(int maxNodes = DMS_DEFORM_MAX_NODES, int maxConstraints = DMS_DEFORM_MAX_CONSTRAINTS) {
    check(dms_deform_create(&h, maxNodes, maxConstraints), "DeformationSolver");
  }
  ~DeformationSolver() { dms_deform_destroy(h); }
  DeformationSolver(const DeformationSolver&) = delete;
  DeformationSolver& operator=(const DeformationSolver&) = delete;
  void setNodes(const float* rows4_dev, int n, dms_stream s = nullptr) { check(dms_deform_set_nodes(h, rows4_dev, n, s), "setNodes"); }
  void sampleGraphModel(GlobalModel& model, int sampleRate = 5000, dms_stream s = nullptr) {
    check(dms_deform_sample_model(h, model.h, sampleRate, s), "sampleGraphModel");
  }
  void addConstraints(const float* rows7_dev, int n, int srcTime, bool pinConstraints, dms_stream s = nullptr) {
    check(dms_deform_add_constraints(h, rows7_dev, n, srcTime, pinConstraints ? 1 : 0, 0, s), "addConstraints");
  }
  void clearConstraints() { check(dms_deform_clear_constraints(h), "clearConstraints"); }
  // enqueues the solve; result() waits for it (result().applied = the reference's return value)
  void constrain(int time, bool relaxGraph = false, dms_stream s = nullptr) { check(dms_deform_constrain(h, time, relaxGraph ? 1 : 0, s), "constrain"); }
  dms_deform_result result() {
    dms_deform_result r;
    check(dms_deform_get_result(h, &r), "result");
    return r;
  }
  // the 16-float node table in device memory and the device word that holds the node count
  std::pair<const float*, const int*> graphDevice() {
    const float* t = nullptr;
    const int* n = nullptr;
    check(dms_deform_graph_device(h, &t, &n), "graphDevice");
    return std::make_pair(t, n);
  }
  // newRelativeCons of the last applied solve: rows {deformed source xyz, target xyz, source time, target time}
  std::vector<float> relativeConstraints() {
    int n = 0;
    check(dms_deform_get_relative_constraints(h, nullptr, 0, &n), "relativeConstraints");
    std::vector<float> rows((size_t)n * 8);
    check(dms_deform_get_relative_constraints(h, rows.data(), n, &n), "relativeConstraints");
    return rows;
  }
  void setLastDeformTime(long long t) { check(dms_deform_set_last_deform_time(h, t), "setLastDeformTime"); }
  long long lastDeformTime() {
    long long t = 0;
    check(dms_deform_last_deform_time(h, &t), "lastDeformTime");
    return t;
  }
  dms_deform* h = nullptr;

 protected:
  explicit DeformationSolver(dms_deform* made) : h(made) {}
};

// rf.globalDeformation(): a DeformationSolver that also takes relative constraints and poses and solves with fernMatch = true
// (dms_deform_create_global, include/dmslam_deform.h).  constrain() on it is the band solve, for pools without relative constraints.
class GlobalDeformationSolver : public DeformationSolver {
 public:
  GlobalDeformationSolver(int maxNodes = DMS_DEFORM_MAX_GLOBAL_NODES, int maxConstraints = DMS_DEFORM_MAX_CONSTRAINTS,
                          int maxRelative = DMS_DEFORM_MAX_RELATIVE, int maxPoses = 4096)
      : DeformationSolver(make(maxNodes, maxConstraints, maxRelative, maxPoses)) {}
  // Deformation::sampleGraphFrom: every 5th node of the local solver's graph
  void sampleGraphFrom(DeformationSolver& local, dms_stream s = nullptr) { check(dms_deform_sample_from(h, local.h, s), "sampleGraphFrom"); }
  // rows {source xyz, target xyz, source time, target time}: relativeConstraints()'s
  void addRelativeConstraints(const float* rows8_dev, int n, dms_stream s = nullptr) {
    check(dms_deform_add_relative_constraints(h, rows8_dev, n, s), "addRelativeConstraints");
  }
  void addRelativeConstraintsHost(const float* rows8_host, int n, dms_stream s = nullptr) {
    check(dms_deform_add_relative_constraints_host(h, rows8_host, n, s), "addRelativeConstraintsHost");
  }
  void setPoses(const long long* times_dev, const float* poses16_dev, int n, dms_stream s = nullptr) {
    check(dms_deform_set_poses(h, times_dev, poses16_dev, n, s), "setPoses");
  }
  // the poses, corrected when the last constrainGlobal was applied: (times, row-major 4 x 4 matrices)
  std::pair<std::vector<long long>, std::vector<float>> poses() {
    int n = 0;
    check(dms_deform_get_poses(h, nullptr, nullptr, 0, &n), "poses");
    std::vector<long long> t((size_t)n);
    std::vector<float> p((size_t)n * 16);
    check(dms_deform_get_poses(h, t.data(), p.data(), n, &n), "poses");
    return std::make_pair(t, p);
  }
  // Deformation::constrain(..., fernMatch = true, poseGraph, relaxGraph = true); result().applied = its return value
  void constrainGlobal(int time, dms_stream s = nullptr) { check(dms_deform_constrain_global(h, time, s), "constrainGlobal"); }
  int keptRotations() {
    int k = 0;
    check(dms_deform_get_kept_rotations(h, &k), "keptRotations");
    return k;
  }

 private:
  static dms_deform* make(int n, int c, int r, int p) {
    dms_deform* d = nullptr;
    check(dms_deform_create_global(&d, n, c, r, p), "GlobalDeformationSolver");
    return d;
  }
};

}  // namespace dms

#if defined(DMS_WITH_EIGEN) || defined(EIGEN_CORE_H) || defined(EIGEN_CORE_MODULE_H)
#include <Eigen/Core>
namespace dms {
// The reference's own signature (RGBDOdometry.h:55-60)
inline void getIncrementalTransformation(RGBDOdometry& o, Eigen::Vector3f& trans, Eigen::Matrix<float, 3, 3, Eigen::RowMajor>& rot,
                                         const bool& rgbOnly, const float& icpWeight, const bool& pyramid, const bool& fastOdom,
                                         const bool& so3, const bool interMap = false) {
  o.getIncrementalTransformation(trans.data(), rot.data(), rgbOnly, icpWeight, pyramid, fastOdom, so3, interMap);
}
inline void initICPModel(RGBDOdometry& o, DeviceTexture* v, DeviceTexture* n, float depthCutoff, const Eigen::Matrix4f& modelPose) {
  Eigen::Matrix<float, 4, 4, Eigen::RowMajor> p = modelPose;
  o.initICPModel(v, n, depthCutoff, p.data());
}
}  // namespace dms
#endif
