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
int modelPyramidFused(const void* vA, const void* nA, const void* iA, const void* vB, const void* nB, const void* iB, const int* flag_dev,
                      int force_b_img, const float* pose16_dev, dms_image2d* vmaps, dms_image2d* nmaps, dms_image2d* depths,
                      dms_image2d* images, float cutOff, hipStream_t s, bool skip_last_step = false, const unsigned* dense_cnt = nullptr,
                      int dense_samples = 0, int* flag_out = nullptr, const TrackInitArgs* init = nullptr);
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
int fill_in(const dms_predict_out* ex, const dms_image2d* depth, const dms_image2d* rgba, const dms_camera* cam, int pass_geom,
            int pass_rgb, dms_predict_out* out, hipStream_t s, const void* mirror_src = nullptr, void* mirror_dst = nullptr,
            int mirror_bytes = 0, int* dense_flag = nullptr);
int fill_args(const dms_predict_out* ex, const dms_image2d* depth, const dms_image2d* rgba, const dms_camera* cam, int pass_geom, int pass_rgb,
              dms_predict_out* out, const void* mirror_src, void* mirror_dst, int mirror_bytes, int* dense_flag, FillArgs* res);
int resize_nn(const dms_image2d* src, dms_image2d* dst, int elem, hipStream_t s);

// fusion_map.hip
int model_initialise(dms_model* m, const dms_image2d* rgba, const dms_image2d* dm, const dms_image2d* dmf, const dms_camera* cam, int time,
                     int timeIdx, float maxDepth, hipStream_t s);
int index_map(dms_model* m, const dms_pose_block* pose, const dms_camera* cam, int time, int timeIdx, float maxDepth, int timeDelta,
              unsigned long long* zbuf, dms_indexmap_out* out, int transposed, int zclean, hipStream_t s,
              unsigned long long* zbuf_also = nullptr);
int index_project(dms_model* m, const dms_pose_block* pose, const dms_camera* cam, int time, int timeIdx, float maxDepth, int timeDelta,
                  unsigned long long* zbuf, int zclean, hipStream_t s);
int clear_zbuf(unsigned long long* zbuf, int n, hipStream_t s);
int untranspose(const void* src, void* dst, int cols, int rows, int elem, hipStream_t s);
int splat_predict(dms_model* m, const dms_pose_block* pose, const dms_camera* cam, float maxDepth, float confThreshold, int time,
                  int timeIdx, int maxTime, int timeDelta, int active, unsigned long long* zbuf, dms_predict_out* out,
                  dms_image2d* depth_out, int zclean, hipStream_t s, const float* second_conf_time_maxtime = nullptr,
                  unsigned long long* zbuf2 = nullptr, int resolve_only = 0, const FillArgs* fill = nullptr, const TrackInitArgs* init = nullptr,
                  const PredictModelArgs* pm = nullptr);
int splat_project_only(dms_model* m, const dms_pose_block* pose, const dms_camera* cam, float maxDepth, float confThreshold, int time,
                       int timeIdx, int maxTime, int timeDelta, int active, unsigned long long* zbuf, hipStream_t s, const ProjectRider* rider);
int model_sample_graph(dms_model* m, int sampleRate, float* rows4_host, int max_rows, int* n_host, hipStream_t s);
int model_flush_pending(dms_model* m, hipStream_t s);

// fusion_fuse.hip
int model_fuse(dms_model* m, const dms_pose_block* pose, int time, int timeIdx, const dms_image2d* rgba, const dms_image2d* dr,
               const dms_image2d* drf, const dms_indexmap_out* im, const dms_camera* cam, float depthCutoff, float weighting,
               const float* weighting_dev, int transposed, hipStream_t s, int defer_update = 0);
int model_fuse_zbuf(dms_model* m, const dms_pose_block* pose, int time, int timeIdx, const dms_image2d* rgba, const dms_image2d* dr,
                    const dms_image2d* drf, const unsigned long long* zbuf, const dms_camera* cam, float depthCutoff, float weighting,
                    const float* weighting_dev, hipStream_t s, int defer_update = 0);
int model_fuse_scratch(dms_model* m, float* slot_pos4, float* slot_col4, float* slot_nrm4, unsigned* slot_best, unsigned char* slot_flag,
                       unsigned* winner, size_t winner_count, hipStream_t s);
// fused_clean_projection: a splat project pass (the arguments of splat_project_only, from the clean's pose, camera and time slot)
// that the clean's scatter carries - every survivor is projected by the thread that has just stored it, under its new id, into the
// CLEAN `zbuf`: the cells splat_project_only would leave after the clean.  Taken by a whole-map clean without a deformation graph;
// `projected` says whether it was (0: suffix mode or a graph - the caller projects by itself).  `rider`: see ProjectRider; its
// mirror may contain the word count_out2 points to.
struct CleanProjection {
  float maxDepth, confThreshold;
  int time, maxTime, timeDelta, active;
  unsigned long long* zbuf;
  const ProjectRider* rider;
  int projected;
};
int model_clean(dms_model* m, const dms_pose_block* pose, int time, int timeIdx, const dms_indexmap_out* im, const dms_image2d* depth_synth,
                const dms_camera* cam, float confThreshold, const float* graph_host, int graph_nodes, int timeDelta, float maxDepth,
                int isFern, int transposed, unsigned* count_out2, hipStream_t s, const float* graph_dev = nullptr,
                CleanProjection* project = nullptr);

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
int odometry_initModel_fused(dms_odometry* o, const void* vA, const void* nA, const void* iA, const void* vB, const void* nB,
                             const void* iB, const int* flag_dev, int force_b_img, const float* pose16_dev, hipStream_t s,
                             int defer_last_step = 0, unsigned* dense_cnt = nullptr, int dense_samples = 0, const TrackFold* fold = nullptr);
// fused_model_prediction: in place of odometry_initModel_fused when the caller's own kernel writes the model maps.  Returns 1 and
// fills `mv` and `ti` (the folded set-up of the track call `fold` describes, to ride on that kernel) when the next
// odometry_track_enqueue on this handle has a resident SO3 launch to host the riders - both steps of the depth / intensity pyramid
// from the level-0 planes, and the emptying of the n_cells z-buffer cells `cells` of `zbuf` the caller's kernel leaves behind; 0
// (nothing changed) otherwise.  The caller's kernel and the track call follow on one stream.
int odometry_model_views_begin(dms_odometry* o, const TrackFold* fold, ModelMapViews* mv, TrackInitArgs* ti, unsigned long long* zbuf,
                               const int* cells, int n_cells);
int odometry_initLive_fused(dms_odometry* o, const void* verts, const void* norms, const void* rgba, const int* any_flag_dev,
                            hipStream_t s);
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
