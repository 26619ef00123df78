/*
 * dmslam_depthnet.h — C ABI of the two tensor conversions around the depth network: what the reference's camera loop does to a frame
 * under `predict_depth` (GUI/src/MainController.cpp:315-326, DepthPrediction::predict, GUI/src/Tools/DepthPrediction.cpp:106-169)
 * before and after the inference call.  The network is the caller's; these two operators fix the bits on either side of it.
 *
 *   pack    im.convertTo(CV_32FC3, 1.0/255.0), cv::split, three plane copies (:108-121), then with half_float
 *           Eigen::half_impl::float_to_half_rtne per value (:124-131): interleaved RGB8 -> the network's [1, 3, H, W] input
 *   unpack  the optional half_to_float (:151-160), then im_d.convertTo(CV_16UC1, 1000.0) (:162-167): the network's [1, 1, H, W]
 *           output in metres -> the 16-bit millimetre depth image that dms_fusion_process_frame consumes
 *
 * The arithmetic, one fixed IEEE sequence on both sides of every test:
 *   pack    value = float(byte) * float(1.0 / 255.0): ONE single-precision multiply by the single nearest to 1/255 (0x3B808081).  It
 *           is not a division by 255 and not a double-precision product rounded afterwards; both differ from it in the last bit for
 *           some bytes.  `half`: that value rounded to fp16, nearest-even (values lie in [0, 1]: no overflow, no subnormal input).
 *   unpack  r = x * 1000.0f, ONE single-precision multiply (an fp16 x converts to fp32 exactly first).
 *           DMS_DEPTHNET_RUNTIME (the default, the reference's run-time path): v = r rounded to the nearest integer, ties to even;
 *             the result is 0 when r is NaN, +inf, -inf or |v| >= 2^31, else v saturated to [0, 65535].  This is OpenCV's
 *             saturate_cast<ushort>(cvRound(r)) on x86, where the SSE float -> int32 conversion answers INT_MIN for every value it
 *             cannot represent, and saturate_cast of INT_MIN is 0: "no depth" for every consumer downstream, not 65535.  The rule
 *             is the contract of this header; it is read from OpenCV's documented x86 behaviour and not recorded from the library.
 *           DMS_DEPTHNET_TRUNCATE (the reference's offline converter, logs/kitti/kitti_odom_to_lcm.py:223,
 *             `(depth * 1000.0).clip(0.0, 65535.0).astype(np.uint16)`): r clipped to [0, 65535] (+inf -> 65535), then truncated
 *             towards zero; NaN -> 0.  Differs from the run-time rule by up to 1 mm, and above 2^31 mm.
 *
 * Layouts: rgb_dev = height rows of width pixels, rgb_channels (3 or 4) bytes each, tightly packed, channels in the order the caller
 * has them (a fourth byte is ignored).  tensor_dev of pack = three planes of width * height values, plane c = channel c, tightly
 * packed (NCHW with N = 1); of unpack = one such plane.  `half` = 0: IEEE binary32 values; otherwise IEEE binary16.  Tensor and depth
 * pointers must be aligned to their element (4 / 2 bytes); nothing more is asked of any pointer: the kernels use 16-byte accesses
 * wherever the addresses allow and narrower ones for the rest.  Sizes up to 2^31 - 1 pixels.
 *
 * Conventions of the other headers: plain C, int status (dmslam.h DMS_*), every argument checked before any device access,
 * `dms_stream`.  Both calls are one kernel launch, asynchronous on `s`; neither allocates nor synchronises the host, so both may be
 * captured into a graph.  DMS_ERR_INVALID_ARG (and nothing written) for a null pointer, a non-positive width or height, a product
 * beyond 2^31 - 1, rgb_channels outside {3, 4}, an unknown mode, or a tensor / depth pointer not aligned to its element.
 *
 * Hand-over to the frame step (dmslam_fusion.h "Input-buffer ordering"): with pipeline_ingest = 1 (the default)
 * dms_fusion_process_frame reads rgb_dev and depth_dev on an INTERNAL stream, which is ordered behind nothing of the caller's except
 * what dms_fusion_inputs_ready names.  So, per frame:
 *     dms_depthnet_pack(rgb, ch, W, H, input, half, producer);   the network on `producer`;   dms_depthnet_unpack(out, ..., depth, mode, producer);
 *     dms_fusion_inputs_ready(f, producer);                      -- records the point of `producer` the ingest waits for
 *     dms_fusion_process_frame(f, rgb, ch, depth, NULL, 1.f, s);
 * inputs_ready is needed whatever `producer` is - also when it is `s` itself, since the ingest does not run on `s`.  With
 * pipeline_ingest = 0 the ingest runs on `s`: then inputs_ready does nothing, and a producer stream other than `s` needs an event of
 * the caller's own.  Before the NEXT frame's unpack overwrites `depth` (and before rgb is rewritten), the previous frame's ingest
 * must have read it: dms_fusion_inputs_consumed(f, s) blocks the host until then (the ingest is the first work of a frame and runs
 * beside the previous frame, so the wait is short).
 */
#ifndef DMSLAM_DEPTHNET_H_
#define DMSLAM_DEPTHNET_H_

#include "dmslam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DMS_DEPTHNET_RUNTIME 0  /* DepthPrediction.cpp:166: round half to even, saturate, what cannot be an int32 -> 0 */
#define DMS_DEPTHNET_TRUNCATE 1 /* kitti_odom_to_lcm.py:223: clip to [0, 65535], truncate, NaN -> 0 */

/* RGB8 / RGBA8 image -> [1, 3, H, W] tensor of byte * (1/255), fp32 or (half != 0) fp16 */
int dms_depthnet_pack(const void* rgb_dev, int rgb_channels, int width, int height, void* tensor_dev, int half, dms_stream s);

/* [1, 1, H, W] tensor of metres, fp32 or (half != 0) fp16 -> u16 millimetres by `mode` */
int dms_depthnet_unpack(const void* tensor_dev, int half, int width, int height, unsigned short* depth_dev, int mode, dms_stream s);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_DEPTHNET_H_ */
