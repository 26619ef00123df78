/*
 * dmslam_render_panels.h — C ABI of the view's four image panels: what the reference's window shows beside the 3-D view on every
 * GUI tick (GUI/src/MainController.cpp:649-664), drawn into a render target of dmslam_render.h.
 *
 *   DEPTH_NORM  ElasticFusion::normaliseDepth (ElasticFusion.cpp:770-779): depth_norm.frag over the raw u16 depth        LINEAR
 *   Model       IndexMap::renderDepth (IndexMap.cpp:219-251): visualise_textures.frag over the ACTIVE vertex image        NEAREST
 *   RGB         the live colour image, as it is                                                                           LINEAR
 *   ModelImage  the ACTIVE prediction's colour image, as it is                                                            NEAREST
 * each put on the screen by GUI::displayImg = RenderToViewport(true) with the depth test off (GUI/src/Tools/GUI.h:340-350).
 *
 * Source images are in IMAGE order (row 0 = the top row of the camera image), rows tightly packed.  The target's rows are window rows
 * (row 0 = the bottom of the view, dmslam_render.h), so a blit turns the image upside down in memory and upright on the screen.
 * The rules GL leaves open are DESIGN.md §4 R9 and R22-R26.
 *
 * Conventions of the other headers: plain C, int status (dmslam.h DMS_*), every argument checked before any device access,
 * `dms_stream`.  No call allocates, none synchronises the host (except create / destroy).  A panel call READS its source images and
 * changes nothing but `panels` and the target; order it against the frame step as a draw (dmslam_render.h).
 */
#ifndef DMSLAM_RENDER_PANELS_H_
#define DMSLAM_RENDER_PANELS_H_

#include "dmslam_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMS_PANEL_RGBA8 0 /* 4 B/px: (r, g, b, a) */
#define DMS_PANEL_L8 1    /* 1 B/px luminance, shown as (L, L, L, 1): the DEPTH_NORM image */
#define DMS_PANEL_NEAREST 0
#define DMS_PANEL_LINEAR 1

/* the column, top to bottom in the reference's window (MainController.cpp:659-663): index into viewports[] and bit of which_mask */
#define DMS_PANEL_DEPTH_NORM 0
#define DMS_PANEL_MODEL 1
#define DMS_PANEL_RGB 2
#define DMS_PANEL_MODEL_IMAGE 3
#define DMS_PANEL_ALL 15

typedef struct dms_panels dms_panels;

/* a rectangle of a target in window coordinates: x, y of its bottom-left pixel (glViewport) */
typedef struct dms_viewport {
  int x, y, w, h;
} dms_viewport;

/* The two intermediates the reference keeps as textures, for one camera size: DEPTH_NORM (L8, R26) and the Model image drawTexture
 * (RGBA8).  Owns W*H*5 bytes of HBM, created zeroed.  Synchronous. */
int dms_panels_create(dms_panels** out, int width, int height);
int dms_panels_destroy(dms_panels* p);
/* Device views of both (owned by `p`, valid until it is destroyed), either may be NULL; image order */
int dms_panels_images(dms_panels* p, dms_image2d* depth_norm_l8, dms_image2d* model_rgba8);

/* normaliseDepth: per pixel, v = the u16 depth; uint(min_val) < v < uint(max_val) ? 1 - float(v) / max_val : 0, stored by R9 (R26).
 * The caller passes the uniforms already scaled (the reference: 0.3f * 1000.f and depthCutoff * 1000.f).  uint(x) is the C
 * conversion of x clamped to [0, 2^32 - 1], 0 for NaN.  DMS_ERR_INVALID_ARG for a null pointer, an image of another size than
 * `p` or with padded rows. */
int dms_depth_norm(dms_panels* p, const dms_image2d* depth_u16, float min_val, float max_val, dms_stream s);

/* renderDepth: per pixel, z = the vertex's third channel; z > max_depth || z <= 0 ? (0, 0, 0, 0) (discarded: the clear colour) : all
 * four channels 1 - z / max_depth by R9.  A NaN z fails both comparisons and writes R9(NaN) = 0 in all four.  Errors as above. */
int dms_model_depth_image(dms_panels* p, const dms_image2d* vertex_rgba32f, float max_depth, dms_stream s);

/* RenderToViewport(true) with the depth test off: `image` stretched over `vp` of the target, upside down, sampled at pixel centres
 * (R22) with `filter` (R23, R24), modulated by color_rgb (R25).  Overwrites the colour inside vp; depth, winner key and draw_seq
 * stay: it is not a draw, and a later draw that wins a pixel still recolours it.  DMS_ERR_INVALID_ARG for a null pointer, an empty
 * image or one with padded rows, another format or filter, an empty viewport or one that leaves the target. */
int dms_render_blit(dms_render_target* t, const dms_image2d* image, int format, int filter, const dms_viewport* vp, const float color_rgb[3],
                    dms_stream s);

/* The whole column for a context in ONE launch: normaliseDepth(0.3f * 1000.f, depth_cutoff * 1000.f), renderDepth(depth_cutoff) and
 * the blits of the panels in which_mask (bit k = panel k into viewports[k], colour (1, 1, 1), the filters of the table above), over
 * images 0, 1, 9 and 10 of dms_fusion_get_image.  Leaves DEPTH_NORM and the Model image in `p` and the same bytes in the target as
 * the separate calls in the reference's order (a pixel of two viewports shows the later panel).  Additionally DMS_ERR_INVALID_ARG
 * for `p` of another size than the context, which_mask outside 0..15, before the first frame and inside a frame (between
 * process_frame_begin and _end).  Viewports of panels not in which_mask are not read. */
int dms_fusion_draw_panels(dms_render_target* t, dms_panels* p, dms_fusion* f, const dms_viewport viewports[4], float depth_cutoff,
                           int which_mask, dms_stream s);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_RENDER_PANELS_H_ */
