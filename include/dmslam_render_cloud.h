/*
 * dmslam_render_cloud.h — C ABI of the live-frame point clouds: FeedbackBuffer::render (Core/src/Shaders/FeedbackBuffer.cpp:145-187)
 * of the context's RAW and FILTERED feedback buffers, what the reference's 3-D view draws before the map when "draw raw cloud" /
 * "draw filtered cloud" is set (GUI/src/MainController.cpp:475-493), drawn into a render target of dmslam_render.h.
 *
 *   buffer  vertex_feedback.{vert,geom} (FeedbackBuffer::compute, :84-143): one vertex per pixel of a metric depth image in
 *           column-major order, kept iff 0 < z <= maxDepth; position AND normal from that one depth image.
 *   draw    draw_feedback.{vert,frag} with the uniforms MVP, pose and colorType (threshold 0, no cluster colour): one size-1 point per
 *           vertex with confidence > 0 at MVP * (pose * (position, 1)).  The normal is not rotated by pose.
 *
 * No vertex buffer is made: pass 1 runs per source pixel and competes for target pixels, pass 2 rebuilds the colour of the winners
 * from the images.  A cloud is one draw of the target in dmslam_render.h's sense: it takes the next draw_seq and competes by the same key
 *   key = depth24 << 40 | draw_seq << 32 | e,    e = x * rows + y  (the column-major index of the source pixel)
 * so it composes with earlier and later dms_render_draw / dms_render_fxaa calls.  e grows with the reference's compacted buffer index, so
 * "equal depth keeps the earlier primitive" resolves alike.  The rules GL leaves open are DESIGN.md §4 R1-R3, R9 and R19-R21.
 *
 * Conventions, image rows (row 0 = the bottom of the view) and the ordering against the frame step are those of dmslam_render.h: a draw
 * READS the feedback inputs (or the images given), changes nothing but its target, allocates nothing and does not synchronise the host;
 * every argument is checked before any device access.
 */
#ifndef DMSLAM_RENDER_CLOUD_H_
#define DMSLAM_RENDER_CLOUD_H_

#include "dmslam_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMS_CLOUD_RAW 0      /* FeedbackBuffer::RAW: the unfiltered metric depth */
#define DMS_CLOUD_FILTERED 1 /* FeedbackBuffer::FILTERED: the bilateral-filtered metric depth */
#define DMS_CLOUD_MAX_PIXELS 1073741824LL /* cols * rows of a source image (2^30) */

/* The uniforms of FeedbackBuffer::render.  color_type is the reference's precedence already applied (drawNormals ? 1 : drawColors ? 2 : 0):
 * 1 the camera-frame normal, 2 the frame's colour, 0 shaded grey 0.5 |n.x + n.y + n.z| + 0.1. */
typedef struct dms_render_cloud_params {
  float mvp[16];               /* the view: clip-from-world, row-major; with pose_dev: the projection only (dms_render_params) */
  const float* pose_dev;       /* optional view pose in HBM: mvp_eff = mvp * F * inverse(pose), see dms_render_mvp_from_pose */
  float model_pose[16];        /* the `pose` uniform: world-from-camera of the frame, row-major (host) */
  const float* model_pose_dev; /* optional: the same as 16 floats in HBM (e.g. dms_fusion_pose_device); model_pose is then ignored */
  int color_type;              /* 0 .. 2 */
} dms_render_cloud_params;

/* The clip position a cloud draw gives a camera-frame point, on the host, bit for bit (R19): clip = mvp_eff * (model_pose * (p, 1)) in
 * fp32, two matrix-vector products with every row accumulated left to right,
 *   w[r] = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3] * 1,   clip[r] = ((V[r][0] w0 + V[r][1] w1) + V[r][2] w2) + V[r][3] w3
 * and no 4 x 4 product: GLSL does not fix the grouping of MVP * pose * v, and the reference's programs on Mesa group it this way
 * (tests/golden/ref_render_cloud.npz).  mvp_eff is the host matrix, or dms_render_mvp_from_pose's with pose_dev. */
int dms_render_cloud_clip(const float mvp_eff16[16], const float model_pose16[16], const float point3[3], float clip4[4]);

/* One cloud over any colour image (RGBA8, 4 B/px) and metric depth image (float, 4 B/px) of one size, rows tightly packed, with the
 * camera's intrinsics: the operator form.  DMS_ERR_INVALID_ARG for a null pointer, images of different or empty shape, with padded
 * rows or of more than DMS_CLOUD_MAX_PIXELS pixels, color_type outside 0..2, or more than DMS_RENDER_MAX_DRAWS draws since the target's last clear. */
int dms_render_cloud(dms_render_target* t, const dms_image2d* rgba, const dms_image2d* depth_metric, const dms_camera* cam, float max_depth,
                     const dms_render_cloud_params* p, dms_stream s);

/* The same over the context's feedback inputs — what dms_fusion_compute_feedback last kept, or the first frame's — with which =
 * DMS_CLOUD_RAW or DMS_CLOUD_FILTERED and maxDepth = (float)(int)maxDepthProcessed (Context.h:211).  Additionally
 * DMS_ERR_INVALID_ARG before the first frame, inside a frame (between process_frame_begin and _end) and for another `which`. */
int dms_fusion_render_cloud(dms_render_target* t, dms_fusion* f, int which, const dms_render_cloud_params* p, dms_stream s);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_RENDER_CLOUD_H_ */
