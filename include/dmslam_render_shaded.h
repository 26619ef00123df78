/*
 * dmslam_render_shaded.h — C ABI of the shaded map view: GUI::drawFXAA (GUI/src/Tools/GUI.h:365-478), the mode of the reference's
 * 3-D view that MainController.cpp:502-511 uses instead of renderPointCloud when the GUI's drawFxaa toggle is on.  Two stages, each
 * its own call:
 *
 *   A  dms_render_shaded_draw: the map with Phong lighting (draw_global_surface.{vert,geom} + draw_global_surface_phong.frag) into
 *      an offscreen float buffer (the GUI's 3840 x 2160 RGBA32F texture with its depth buffer, GUI.h:55-70), cleared first;
 *   B  dms_render_fxaa: that buffer resolved into a render target (dmslam_render.h) with FXAA (empty.vert + quad.geom + fxaa.frag),
 *      then the offscreen depth blitted into the target (glBlitFramebuffer, depth only, NEAREST).
 *
 * The offscreen buffer holds RGBA32F colour, 24-bit depth and the per-pixel winner key of dmslam_render.h
 *   key = depth24 << 40 | draw_seq << 32 | surfel id      (cleared: all ones; draw_seq is 0: one draw per clear)
 * Discs, culling, the unstable-surfel depth shift and the colour modes are those of dms_render_draw; the
 * rules GL leaves open for the shading, the sampling and the blit are R11-R18.
 *
 * Conventions, image rows (row 0 = the bottom of the view) and the ordering against the frame step are those of dmslam_render.h.
 * No call allocates, none synchronises the host (except create / destroy); every argument is checked before any device access.
 */
#ifndef DMSLAM_RENDER_SHADED_H_
#define DMSLAM_RENDER_SHADED_H_

#include "dmslam_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMS_RENDER_OFFSCREEN_WIDTH 3840 /* the GUI's offscreen size (GUI.h:57), the adapters' default */
#define DMS_RENDER_OFFSCREEN_HEIGHT 2160

typedef struct dms_render_offscreen dms_render_offscreen;

/* Owns W*H*28 bytes of HBM (width and height up to DMS_RENDER_MAX_EXTENT); created with no winner.  Synchronous. */
int dms_render_offscreen_create(dms_render_offscreen** out, int width, int height);
int dms_render_offscreen_destroy(dms_render_offscreen* o);
int dms_render_offscreen_size(const dms_render_offscreen* o, int* width, int* height);

/* Stage A.  Clears the buffer to clear_rgba (stored as given), depth 1.0, no winner, then draws the map with the uniforms of p
 * (draw_points must be 0, use_cluster_color 0, color_type 0..3: the GUI's precedence normals 1, colours 2, times 3, else 0;
 * time_idx is the call's timeIdx) and of the Phong program: light_pos (`lightpos`, the GUI passes the translation
 * column of the view matrix) and sign_mult (`signMult`: n = sign_mult * normal).  The colour is ambient + diffuse + specular, not
 * clamped.  DMS_ERR_INVALID_ARG for a null pointer, an argument outside those ranges, time_idx outside [0, DMS_MAX_SENSORS) or a
 * map with a deferred update pending. */
int dms_render_shaded_draw(dms_render_offscreen* o, dms_model* m, const dms_render_params* p, const float light_pos[3], float sign_mult,
                           const float clear_rgba[4], dms_stream s);

/* Stage B.  Every pixel (x, y) of the target: fxaa.frag at texcoord ((x + 0.5) / W, (y + 0.5) / H) over the buffer, alpha 1, written
 * as RGBA8 (R9) where the quad's window depth 0.5 passes GL_LESS against the target's depth; then the target's depth and winner are
 * the buffer's at the NEAREST source texel.  Counts as one draw of the target: a later dms_render_draw depth-tests against the
 * blitted depth and loses ties to it.  DMS_ERR_INVALID_ARG for a null pointer or a target with DMS_RENDER_MAX_DRAWS draws
 * since its clear. */
int dms_render_fxaa(dms_render_target* t, const dms_render_offscreen* o, dms_stream s);

/* Device views of the buffer (owned by it, valid until it is destroyed), any of them may be NULL: rgba32f: 16 B/px; depth24_u32:
 * the 24-bit depth (0xFFFFFF = cleared); winner_u64: the key above. */
int dms_render_offscreen_images(dms_render_offscreen* o, dms_image2d* rgba32f, dms_image2d* depth24_u32, dms_image2d* winner_u64);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_RENDER_SHADED_H_ */
