// Internal C++ entry points shared between translation units of libdmslam_hip.so.
#pragma once
#include "common.hpp"
#include "../../include/dmslam_deform.h"
#include "../../include/dmslam_render_panels.h"

namespace dms {

// (thumb_vertex_off / thumb_normal_off / thumb_block_size: common.hpp)

struct TrackInitArgs;  // track_init.hpp
struct FillArgs;       // fill.hpp
struct FrameState;     // frame_state.hpp
struct LoopState;      // frame_state.hpp

// fusion_map.hip: small copies that ride on block 0 of a splat project launch (at most 256 dwords each) - what block 0 of the
// resolve pass carries when a resolve follows.  `mirror`: the frame's result block into its pinned host slot; `copy`: the pose
// block the projection was rendered from, kept for a prediction that is resolved later (fusion_frame.hip, lazy_final_prediction).
struct ProjectRider {
  const unsigned* mirror_src;
  unsigned* mirror_dst;
  int mirror_words;
  const unsigned* copy_src;
  unsigned* copy_dst;
  int copy_words;
};
constexpr ProjectRider kNoRider = {nullptr, nullptr, 0, nullptr, nullptr, 0};

// track.hip -> fusion_map.hip: the tracker's model maps (stacked vmap / nmap planes of the three levels, level 0 of the float depth
// and intensity pyramids) as views, for the prediction pass that writes them itself (fused_model_prediction)
struct ModelMapViews {
  View<float> v[3], n[3], depth0;
  View<unsigned char> inten0;
  float cutOff;  // verticesToDepth
};
// fusion_map.hip: k_predict_model
struct PredictModelArgs {
  ModelMapViews maps;
  const float* pose16;      // model pose for transformMaps
  int* flag_out;            // the denseEnough decision (1 = fill-in values used), stored by block 0
  const int* sample_cells;  // z-buffer cells of the decision's sample pixels (fill.hpp: fill_sample_cells), n_cells of them
  int n_cells;
  int samples;              // the decision's denominator, (W / 20) * (H / 20)
  int threads;              // block shape: 256, 512 or 1024
};

// The host entry points of the map half and of the tracker's model hand-over take a handle, a few argument records and a stream.
// The records are plain aggregates, filled by field name where the call is made; a field the caller leaves alone means "off".

// What a pass over the map is rendered from and what it culls: the index map, the splat prediction, the fuse and the clean all
// take one.  The index map, the fuse and the clean ignore the last three fields.
struct MapPass {
  const dms_pose_block* pose = nullptr;
  const dms_camera* cam = nullptr;
  float maxDepth = 0.f;  // depth cut-off
  int time = 0;
  int timeIdx = 0;       // the sensor's time plane
  int timeDelta = 0;
  // splat passes only
  float confThreshold = 0.f;
  int maxTime = 0;
  int active = 0;
};

// fusion_map.hip: second prediction sharing a splat project pass (same map, pose, depth range and mode)
struct SplatSecond {
  float confThreshold;
  int time, maxTime;
};

inline bool dense_img(const dms_image2d& im, size_t elem, int w, int h) {
  return im.data && im.cols == w && im.rows == h && im.pitch == (size_t)w * elem;
}

// prep.hip: the tracker's model pyramids from two image sets of float4 vertices, float4 normals and RGBA8 pixels - A (the
// prediction), B (its fill-in) - of which *use_b selects one per launch; force_b_img: the image comes from B whatever *use_b says
struct ModelImages {
  const void *vertex = nullptr, *normal = nullptr, *image = nullptr;
};
struct ModelSources {
  ModelImages a, b;
  const int* use_b = nullptr;  // device
  int force_b_img = 0;
  const float* pose16 = nullptr;  // device: the pose the sets were rendered from (transformMaps), or none
};
struct ModelTargets {  // the three-level pyramids the launch writes
  dms_image2d *vmaps = nullptr, *nmaps = nullptr, *depths = nullptr, *images = nullptr;
  float cutOff = 0.f;  // verticesToDepth
};
struct ModelPyramidOpts {
  bool skip_last_step = false;          // the caller runs the pyramid's last step inside a kernel of its own
  const unsigned* dense_cnt = nullptr;  // the source choice comes from the 16 counters of the prediction's resolve pass (fill.hpp),
  int dense_samples = 0;                // out of this many samples, instead of *use_b ...
  int* flag_out = nullptr;              // ... and is stored here
  const TrackInitArgs* init = nullptr;  // the tracker call's set-up as a block group of the launch
};

// prep.hip
int pyrDown(const dms_image2d* src, dms_image2d* dst, hipStream_t s);
int createVMap(const dms_camera* intr, const dms_image2d* depth, dms_image2d* vmap, float cutoff, hipStream_t s);
int createNMap(const dms_image2d* vmap, dms_image2d* nmap, hipStream_t s);
int transformMaps(const dms_image2d* vs, const dms_image2d* ns, const dms_mat33* R, const dms_float3* t, dms_image2d* vd,
                  dms_image2d* nd, hipStream_t s);
int copyMaps(const float* vsrc, const float* nsrc, dms_image2d* vd, dms_image2d* nd, hipStream_t s);
int resizeMap(const dms_image2d* in, dms_image2d* out, bool normalize, hipStream_t s);
int pyrDownGaussF(const dms_image2d* src, dms_image2d* dst, hipStream_t s);
int pyrDownUcharGauss(const dms_image2d* src, dms_image2d* dst, hipStream_t s);
int verticesToDepth(const float* vsrc, dms_image2d* dst, float cutOff, hipStream_t s);
int modelPyramidFused(const ModelSources& src, const ModelTargets& dst, const ModelPyramidOpts& opt, hipStream_t s);
int verticesToDepth2D(const dms_image2d* vsrc, dms_image2d* dst, float cutOff, hipStream_t s);
int imageToIntensity(const dms_image2d* rgba, dms_image2d* dst, hipStream_t s);
int derivativeGate(const dms_image2d* src, dms_image2d* dx, dms_image2d* dy, dms_image2d* gate, float minScale, hipStream_t s);
int derivativeImages(const dms_image2d* src, dms_image2d* dx, dms_image2d* dy, hipStream_t s);
int projectToPointCloud(const dms_image2d* depth, dms_image2d* cloud, const dms_camera* intr, int level, hipStream_t s);
int liveLevelsFused(const dms_image2d* depth, const dms_image2d* vmap, const dms_image2d* nmap, const dms_image2d* image, const dms_image2d* dx,
                    const dms_image2d* dy, const dms_image2d* gate, const dms_camera* cam0, float cutoff, const float* minScale, hipStream_t s);
int selectCopy16(void* dst, const void* a, const void* b, const int* flag_dev, int force_b, size_t n16, hipStream_t s);
int transformMapsDev(dms_image2d* v, dms_image2d* n, const float* pose16_dev, hipStream_t s);

// reduce.hip
size_t reduce_workspace_bytes();
int icpStep(const dms_mat33* Rcurr, const dms_float3* tcurr, const dms_image2d* vmap_curr, const dms_image2d* nmap_curr,
            const dms_mat33* Rprev_inv, const dms_float3* tprev, const dms_camera* intr, const dms_image2d* vmap_g_prev,
            const dms_image2d* nmap_g_prev, float distThres, float angleThres, void* workspace, size_t workspace_bytes, float* A,
            float* b, float* residual, int threads, int blocks, hipStream_t s);
int rgbStep(const dms_image2d* corresImg, float sigma, const dms_image2d* cloud, float fx, float fy, const dms_image2d* dIdx,
            const dms_image2d* dIdy, float sobelScale, void* workspace, size_t workspace_bytes, float* A, float* b, int threads,
            int blocks, hipStream_t s);
int computeRgbResidual(float minScale, const dms_image2d* dIdx, const dms_image2d* dIdy, const dms_image2d* lastDepth,
                       const dms_image2d* nextDepth, const dms_image2d* lastImage, const dms_image2d* nextImage,
                       dms_image2d* corresImg, void* workspace, size_t workspace_bytes, float maxDepthDelta, const dms_float3* kt,
                       const dms_mat33* krkinv, int* sigmaSum, int* count, int threads, int blocks, hipStream_t s);
int so3Step(const dms_image2d* lastImage, const dms_image2d* nextImage, const dms_mat33* imageBasis, const dms_mat33* kinv,
            const dms_mat33* krlr, void* workspace, size_t workspace_bytes, float* A, float* b, float* residual, int threads,
            int blocks, hipStream_t s);

// fusion_pre.hip
int depth_bilateral(const dms_image2d* src, dms_image2d* dst, float maxD, hipStream_t s, int narrow_blocks = 0,
                    const dms_image2d* metric_filtered = nullptr, const dms_image2d* depth_l0 = nullptr, const dms_image2d* vmap_l0 = nullptr,
                    const dms_camera* cam_l0 = nullptr, float vmap_cutoff = 0.f);
int depth_metric(const dms_image2d* src, dms_image2d* dst, float maxD, hipStream_t s);
// the hole fill-in of the prediction `ex` into `out` (fill.hpp): fill_args builds the argument block, which the prediction's fused
// resolve pass takes as it is (splat_predict) and fill_in launches on its own
struct FillMirror {  // a block that block (0,0) of the launch copies: the frame's result block into its pinned host slot
  const void* src = nullptr;
  void* dst = nullptr;
  int bytes = 0;
};
struct FillInputs {
  const dms_predict_out* ex = nullptr;
  const dms_image2d* depth = nullptr;  // filtered, mm
  const dms_image2d* rgba = nullptr;
  const dms_camera* cam = nullptr;
  int pass_geom = 0, pass_rgb = 0;  // pass-through: the frame's values whatever the prediction holds
  dms_predict_out* out = nullptr;
  FillMirror mirror;
  int* dense_flag = nullptr;  // the denseEnough decision from `ex`, taken by an extra block
};
int fill_args(const FillInputs& in, FillArgs* res);
int fill_in(const FillArgs& a, hipStream_t s);
int resize_nn(const dms_image2d* src, dms_image2d* dst, int elem, hipStream_t s);

// fusion_map.hip
int model_initialise(dms_model* m, const dms_image2d* rgba, const dms_image2d* dm, const dms_image2d* dmf, const dms_camera* cam, int time,
                     int timeIdx, float maxDepth, hipStream_t s);
struct IndexMapTargets {
  unsigned long long* zbuf = nullptr;
  // the z-buffer is empty on entry (no clear launch); index_map then hands it back empty - the resolve pass clears what it reads
  int zclean = 0;
  // index_map only
  dms_indexmap_out* out = nullptr;
  int transposed = 0;                       // images stored column-major
  unsigned long long* zbuf_also = nullptr;  // a second z-buffer the resolve pass empties on the way (what index_project filled)
};
int index_map(dms_model* m, const MapPass& pass, const IndexMapTargets& t, hipStream_t s);
// index_map without its resolve pass: the z-buffer alone, column-major (cell of pixel (x, y) at x * rows + y), for the one reader
// that needs no images (model_fuse with FuseInputs::zbuf).  Nobody clears it here: the caller hands it to a later index_map as
// zbuf_also, or clears it itself.
int index_project(dms_model* m, const MapPass& pass, const IndexMapTargets& t, hipStream_t s);
int clear_zbuf(unsigned long long* zbuf, int n, hipStream_t s);
int untranspose(const void* src, void* dst, int cols, int rows, int elem, hipStream_t s);
// The one admission check of a splat pass over the map (pose, camera, time slot, no pending update, divisors the project pass can
// take, a rider of at most one block): splat_predict, splat_project_only and a clean that carries a projection call it
int check_map_pass(const dms_model* m, const MapPass& pass, const ProjectRider& rider);
// a splat prediction besides its pass: where it is rendered, what is rendered, and what rides on the resolve pass
enum class SplatMode {
  project_resolve,  // project into zbuf, resolve it
  resolve_only,     // zbuf was filled by an earlier dual or project-only pass with exactly this pass's parameters
  dual              // the project pass also fills zbuf2 with the prediction that differs by `second` in the cull
};
struct SplatPrediction {
  unsigned long long* zbuf = nullptr;
  int zclean = 0;                    // as for the index map
  dms_predict_out* out = nullptr;    // the output: the four images ...
  dms_image2d* depth_out = nullptr;  // ... or, when given, the depth alone
  SplatMode mode = SplatMode::project_resolve;
  SplatSecond second = {0.f, 0, 0};     // dual
  unsigned long long* zbuf2 = nullptr;  // dual
  const FillArgs* fill = nullptr;        // the fill-in, by the resolve pass
  const TrackInitArgs* init = nullptr;   // the tracker call's set-up (with pm)
  const PredictModelArgs* pm = nullptr;  // resolve into the tracker's model maps instead of the images
};
int splat_predict(dms_model* m, const MapPass& pass, const SplatPrediction& p, hipStream_t s);
// The project pass of splat_predict alone, into a CLEAN `zbuf` that a later resolve_only splat_predict with the same pass resolves
// (and cleans): the same keys as a dual pass leaves in its second z-buffer for that cull - a cell's winner is the minimum over the
// fragments that survive the cull, whatever else the pass feeds.  `rider`: see ProjectRider.
int splat_project_only(dms_model* m, const MapPass& pass, unsigned long long* zbuf, const ProjectRider& rider, hipStream_t s);
int model_sample_graph(dms_model* m, int sampleRate, float* rows4_host, int max_rows, int* n_host, hipStream_t s);
int model_flush_pending(dms_model* m, hipStream_t s);

// fusion_fuse.hip
// the frame's measurements and what they are associated through.  The pass gives pose, camera, time, time slot and depth cut-off.
struct FuseInputs {
  const dms_image2d *rgba = nullptr, *depth_raw = nullptr, *depth_filtered = nullptr;  // depths metric
  // the association source, exactly one of: the index map as images, or the column-major z-buffer index_project filled from the
  // map as it is now, at this pose (it is left as it was found)
  const dms_indexmap_out* im = nullptr;
  const unsigned long long* zbuf = nullptr;
  float weighting = 0.f;
  const float* weighting_dev = nullptr;
  int transposed = 0;    // `im` is stored column-major
  int defer_update = 0;  // the update pass is left to the next index_map (model_flush_pending)
};
int model_fuse(dms_model* m, const MapPass& pass, const FuseInputs& in, hipStream_t s);
int model_fuse_scratch(dms_model* m, float* slot_pos4, float* slot_col4, float* slot_nrm4, unsigned* slot_best, unsigned char* slot_flag,
                       unsigned* winner, size_t winner_count, hipStream_t s);
// fused_clean_projection: a splat project pass (what splat_project_only takes; pose, camera and time slot are the clean's) that
// the clean's scatter carries - every survivor is projected by the thread that has just stored it, under its new id, into the
// CLEAN `zbuf`: the cells splat_project_only would leave after the clean.  Taken by a whole-map clean without a deformation graph;
// `projected` says whether it was (0: suffix mode or a graph - the caller projects by itself).  `rider`: see ProjectRider; its
// mirror may contain the word count_out2 points to.
struct CleanProjection {
  MapPass pass;
  unsigned long long* zbuf = nullptr;
  ProjectRider rider = kNoRider;
  int projected = 0;
};
// the clean besides its pass (pose, camera, time, time slot, time delta, depth cut-off)
struct CleanInputs {
  const dms_indexmap_out* im = nullptr;
  const dms_image2d* depth_synth = nullptr;  // optional
  float confThreshold = 0.f;
  const float* graph_host = nullptr;  // the deformation graph's node table, in host ...
  const float* graph_dev = nullptr;   // ... or in device memory (the solver's)
  int graph_nodes = 0;
  int isFern = 0;
  int transposed = 0;              // `im` is stored column-major
  unsigned* count_out2 = nullptr;  // device: a second cell that receives the new count
  CleanProjection* project = nullptr;
};
int model_clean(dms_model* m, const MapPass& pass, const CleanInputs& in, hipStream_t s);

// deform.hip: dms_deform_add_constraints over rows of `stride` >= 7 floats
int deform_add_rows(dms_deform* d, const float* rows_dev, int stride, int n, int srcTime, int pin, hipStream_t s);
// status block and new relative-constraint rows (pinned, rows of 8 floats) behind one synchronisation
int deform_fetch(dms_deform* d, dms_deform_result* res, const float** rel8);
const float* deform_poses_device(dms_deform* d);

// track.hip
struct TrackFold {  // the track call a model pyramid launch prepares (odometry_initModel_fused)
  const float* prior_pose16;
  int pyramid, fastOdom, so3, interMap;
};
int odometry_track_enqueue(dms_odometry* o, const float* trans, const float* rot, const float* prior_pose16_dev, int rgbOnly,
                           float icpWeight, int pyramid, int fastOdom, int so3, int interMap, hipStream_t s, FrameState* frame = nullptr,
                           float weightMultiplier = 1.f);
int odometry_result_pose(dms_odometry* o, float* pose16_dev, hipStream_t s);
struct ModelHandOver {  // what the model pyramid launch leaves to, or prepares for, the NEXT odometry_track_enqueue on the handle
  int defer_last_step = 0;        // the pyramid's last step is left to that call's first kernel
  unsigned* dense_cnt = nullptr;  // the source choice comes from these counters (ModelPyramidOpts), which that call zeroes,
  int dense_samples = 0;          // and *src.use_b receives the decision
  const TrackFold* fold = nullptr;  // that call's set-up runs as a block group of the pyramid kernel
};
int odometry_initModel_fused(dms_odometry* o, const ModelSources& src, const ModelHandOver& next, hipStream_t s);
// fused_model_prediction: in place of odometry_initModel_fused when the caller's own kernel writes the model maps.  Returns 1 and
// fills `mv` and `ti` (the folded set-up of the track call `fold` describes, to ride on that kernel) when the next
// odometry_track_enqueue on this handle has a resident SO3 launch to host the riders - both steps of the depth / intensity pyramid
// from the level-0 planes, and the emptying of the n_cells z-buffer cells `cells` of `zbuf` the caller's kernel leaves behind; 0
// (nothing changed) otherwise.  The caller's kernel and the track call follow on one stream.
int odometry_model_views_begin(dms_odometry* o, const TrackFold* fold, ModelMapViews* mv, TrackInitArgs* ti, unsigned long long* zbuf,
                               const int* cells, int n_cells);
int odometry_initLive_fused(dms_odometry* o, const ModelImages& live, const int* any_flag_dev, hipStream_t s);
int odometry_enable_ring(dms_odometry* o);
int odometry_free_cus(const dms_odometry* o);
void odometry_set_early_exit(dms_odometry* o, int on);
int odometry_next_buffers(dms_odometry* o, int level, dms_image2d* nextImage, dms_image2d* nextDepth);
int odometry_loop_candidate(dms_odometry* o, FrameState* frame, const dms_image2d* vertex, const dms_image2d* oldTime, float maxDepth,
                            LoopState* out, float* cons, hipStream_t s);
void odometry_bind_live(dms_odometry* o, int k);
void odometry_bind_lastnext(dms_odometry* o, int k);
int odometry_initRGB_image(dms_odometry* o, const dms_image2d* rgba, hipStream_t s);
int odometry_live_views(dms_odometry* o, dms_image2d* depth, dms_image2d* vmap, dms_image2d* nmap, dms_image2d* image, dms_image2d* dx,
                        dms_image2d* dy, dms_image2d* gate, float* minScale, bool mark_derivatives);
void odometry_alias_next_depth(dms_odometry* o);

// nid.hip
size_t nid_workspace_bytes(int num_bins);
int computeNIDImg(const dms_image2d* img_kf, const dms_image2d* img_kf_old, const dms_image2d* dmap_kf, const dms_image2d* dmap_kf_old,
                  const dms_image2d* img_curr, int num_bins, void* workspace, size_t workspace_bytes, float* nid_host, float* nid_dev,
                  hipStream_t s);
int computeNIDDepth(const dms_image2d* dmap_kf, const dms_image2d* dmap_kf_old, const dms_image2d* dmap_curr, int num_bins, float max_depth,
                    void* workspace, size_t workspace_bytes, float* nid_host, float* nid_dev, hipStream_t s);

// render.hip: the panel column of dmslam_render_panels.h over the four source images, one launch
int drawPanelColumn(dms_render_target* t, dms_panels* p, const dms_image2d* rgba, const dms_image2d* depth_u16, const dms_image2d* model_rgba,
                    const dms_image2d* vertex, const dms_viewport* viewports, float depth_cutoff, int which_mask, hipStream_t s);

}  // namespace dms
