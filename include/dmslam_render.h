/*
 * dmslam_render.h — C ABI of the map draw: GlobalModel::renderPointCloud (Core/src/GlobalModel.cpp:419-505), the main 3-D view
 * of the reference's application (GUI/src/MainController.cpp:500-530), drawn into a device render target instead of a GL
 * framebuffer.  SURVEY.md §2.3 G14.
 *
 *   discs  draw_global_surface.vert + .geom + .frag (what renderPointCloud binds unless drawPoints is set): a surfel with
 *          conf > threshold, or any surfel with draw_unstable, is a strip of two triangles around it; a fragment outside the
 *          unit disc of the texcoord is discarded; an unstable surfel's (conf <= threshold) depth is shifted by its radius
 *          and clamped to [0, 1] before the test.
 *   points draw_feedback.vert + .frag (draw_points): one size-1 point per surfel with conf > threshold.
 *
 * The target is a colour buffer (RGBA8), a 24-bit depth buffer and, per pixel, the 64-bit key of its winner
 *   key = depth24 << 40 | draw_seq << 32 | surfel id      (cleared: all ones)
 * draw_seq counts the draws since the last clear, so GL_LESS with "the earlier primitive or draw wins a tie" is "the smallest key
 * wins", also across several draws into one target (one per cluster, as renderPointCloud loops over cluster_vbos).  The rules
 * OpenGL leaves to the implementation — coverage, interpolation, clipping, colour and depth conversion — are fixed in DESIGN.md §4
 * R2, R3 and R6-R10.
 *
 * Conventions of the other headers: plain C, int status (dmslam.h DMS_*), every argument checked before any device access,
 * `dms_stream`, row-major 4 x 4 matrices (math order: clip = mvp * (x, y, z, 1)^T; pangolin's OpenGlMatrix is column-major, so
 * an adapter transposes it).  No call allocates, none synchronises the host (except create / destroy).
 *
 * Images are window rows: row 0 is the BOTTOM row of the view, as glReadPixels returns them.  Flip the rows for image order.
 *
 * Ordering: a draw READS the map.  Enqueue it after the frame that wrote the map — on the frame's stream, or on another stream made
 * to wait with dms_fusion_wait_frame_done — and order the next frame after the draw (same stream, or an event) before that frame
 * changes the map under it.  A draw changes nothing but its target.
 */
#ifndef DMSLAM_RENDER_H_
#define DMSLAM_RENDER_H_

#include "dmslam_fusion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMS_RENDER_MAX_EXTENT 8192 /* width and height of a target */
#define DMS_RENDER_MAX_DRAWS 255   /* draws between two clears (draw_seq is 8 bits of the key) */

typedef struct dms_render_target dms_render_target;

/* Owns W*H*16 bytes of HBM; created cleared to colour (0,0,0,0), depth 1.0, no winner.  Synchronous. */
int dms_render_target_create(dms_render_target** out, int width, int height);
int dms_render_target_destroy(dms_render_target* t);
int dms_render_target_size(const dms_render_target* t, int* width, int* height);

/* glClear: colour = clear_rgba (bytes by R9), depth = 1.0, no winner, draw_seq = 0.  Stream ordered. */
int dms_render_clear(dms_render_target* t, const float clear_rgba[4], dms_stream s);

/* The uniforms of renderPointCloud.  color_type is the reference's precedence already applied (GlobalModel.cpp:436-440):
 * 4 contributions of cameras 0-2, 1 normals, 2 decoded colour, 3 init-time ramp, 0 shaded grey (points: 1, 2, else grey).
 * Contributions count the reference's three time slots only: a surfel that none of cameras 0-2 has seen (a map with more cameras)
 * has the colour 0 / 0 in every channel, which is written as 0 like every channel that is not finite - it is drawn black, alpha 255. */
typedef struct dms_render_params {
  float mvp[16];          /* clip-from-world, row-major; with pose_dev: the projection only */
  const float* pose_dev;  /* optional: camera-to-world, 16 floats row-major in HBM (e.g. dms_fusion_pose_device); the view is then
                             built on the device: mvp_eff = mvp * F * inverse(pose), see dms_render_mvp_from_pose */
  float threshold;        /* confidence threshold */
  int draw_unstable;      /* `unstable` uniform: discs also for surfels with conf <= threshold */
  int draw_points;        /* 1: draw_feedback program (points), 0: draw_global_surface program (discs) */
  int draw_window;        /* time-window tint: * 0.25 outside (time - t > time_delta), * (0, 1, 0) inside (<), neither at equality */
  int color_type;         /* 0 .. 4 */
  int time, time_idx, time_delta;  /* time_idx < DMS_MAX_SENSORS: the time plane of the window test */
  int use_cluster_color;  /* `cluster` uniform: cluster_color overrides color_type */
  float cluster_color[3];
} dms_render_params;

/* One draw of one map into the target: pass 1 per surfel (grid sized from the map's host-side upper bound, count read on the
 * device), pass 2 per pixel.  DMS_ERR_INVALID_ARG for a null pointer, color_type outside 0..4, time_idx outside
 * [0, DMS_MAX_SENSORS), more than DMS_RENDER_MAX_DRAWS draws since the last clear, or a map with a deferred update pending. */
int dms_render_draw(dms_render_target* t, dms_model* m, const dms_render_params* p, dms_stream s);

/* Device views of the target's buffers (owned by the target, valid until it is destroyed), any of them may be NULL:
 * rgba8: 4 B/px; depth24_u32: the 24-bit depth (0xFFFFFF = cleared); winner_u64: the key above (surfel id = low 32 bits). */
int dms_render_images(dms_render_target* t, dms_image2d* rgba8, dms_image2d* depth24_u32, dms_image2d* winner_u64);

/* The projection of the GUI's camera, pangolin::ProjectionMatrix(w, h, fu, fv, u0, v0, znear, zfar) (GUI/src/Tools/GUI.h:294-296),
 * the right-up-back, bottom-left frustum (glFrustum), computed in double and rounded to float at the end:
 *   L = -u0 n / fu   R = (w - u0) n / fu   B = -v0 n / fv   T = (h - v0) n / fv        (n = znear, f = zfar)
 *   [ 2n/(R-L)   0          (R+L)/(R-L)    0            ]
 *   [ 0          2n/(T-B)   (T+B)/(T-B)    0            ]
 *   [ 0          0          -(f+n)/(f-n)   -2fn/(f-n)   ]
 *   [ 0          0          -1             0            ]   (row-major) */
int dms_render_frustum(int w, int h, float fu, float fv, float u0, float v0, float znear, float zfar, float out16[16]);

/* The view the draw builds from pose_dev, on the host, bit for bit: out = proj * F * inverse(pose) with F = diag(1, -1, -1, 1)
 * (the map's right-down-forward camera frame to GL's right-up-back), in fp32:
 *   V[r][c] = s_r R[c][r] (c < 3),  V[r][3] = s_r * -((R[0][r] t0 + R[1][r] t1) + R[2][r] t2),  s = (1, -1, -1),  V[3] = (0, 0, 0, 1)
 *   out[r][c] = ((P[r][0] V[0][c] + P[r][1] V[1][c]) + P[r][2] V[2][c]) + P[r][3] V[3][c]
 * (the rigid inverse: pose must be a rotation and a translation). */
int dms_render_mvp_from_pose(const float proj16[16], const float pose16[16], float out16[16]);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_RENDER_H_ */
