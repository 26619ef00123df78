/* dmslam_io_device.h — frame ingest with the pixel work on the GPU: the JPEG colour of compressed .klg logs and
 * compressed eflcm::Frame messages is decoded into DEVICE memory, straight into the RGB8 buffer that
 * dms_fusion_process_frame or dms_depthnet_pack reads.  The bytes are those of dms_jpeg_decode (dmslam_io.h) for every
 * stream it accepts: both decoders compile the same arithmetic (csrc/jpeg_core.hpp).
 *
 * What runs where: the host parses the markers; inverse DCT, chroma upsampling and colour conversion are kernels on the
 * caller's stream (csrc/jpeg_dev.hip).  The Huffman decode in between runs either on the host (the sequential entropy
 * stage into a pinned coefficient buffer, one asynchronous copy) or on the device (the host finds the restart markers
 * with a byte scan and copies the stream into a pinned staging slot; one lane per subsequence of the entropy-coded
 * data) - selectable per decode.  Depth is zlib: inflate stays on the host and the result is copied asynchronously.
 * Plain C99; dmslam_io.h stays host-only.
 *
 * Per frame (dmslam_fusion.h "Input-buffer ordering"):
 *     dms_klg_next_device(klg, jd, depth_dev, rgb_dev, &ts, producer);   -- or dms_frame_unpack_device / dms_jpeg_dev_decode
 *     dms_fusion_inputs_ready(f, producer);
 *     dms_fusion_process_frame(f, rgb_dev, depth_dev, ts, NULL, 1.f, s);
 * and dms_fusion_inputs_consumed(f, s) before depth_dev / rgb_dev are written again. */
#ifndef DMSLAM_IO_DEVICE_H_
#define DMSLAM_IO_DEVICE_H_

#include "dmslam.h"
#include "dmslam_io.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dms_jpeg_dev dms_jpeg_dev;

/* The decoder object for width x height streams of at most max_stream_bytes.  It owns the device coefficient, plane and
 * lane-state buffers and a ring of `slots` (1..16) pinned staging buffers, so a decode call returns once the caller's
 * bytes are copied (they are free again) and blocks only when its slot is still in flight.  Decodes of one object are
 * ordered among themselves whatever streams they are enqueued on. */
int dms_jpeg_dev_create(dms_jpeg_dev** out, int width, int height, size_t max_stream_bytes, int slots);
int dms_jpeg_dev_destroy(dms_jpeg_dev* jd);

/* The size of the streams to come, where it is not the one given at creation; anything that fits the buffers created then. */
int dms_jpeg_dev_set_image_size(dms_jpeg_dev* jd, int width, int height);

/* Bytes of the entropy-coded data one lane decodes: 32, 64, 128 or 256 (DMS_JPEG_DEV_DEFAULT_SUBSEQUENCE at creation). */
#define DMS_JPEG_DEV_DEFAULT_SUBSEQUENCE 64
int dms_jpeg_dev_set_subsequence_bytes(dms_jpeg_dev* jd, int bytes);

/* Baseline JPEG -> width * height * 3 bytes at rgb_dev (device memory, 4-byte aligned), libjpeg's R, G, B order, R and B
 * exchanged where flipColors.  Parses on the host: every refusal dms_jpeg_decode makes before its entropy decode comes back
 * at once with the same code and text.  Then everything is enqueued on `stream` and the call returns.
 * entropy_on_host = 1: the sequential entropy stage runs on the host into a pinned coefficient buffer (a malformed block is
 * then refused at once, too) and only the back half runs on the device; 0: the entropy decode is on the device and a
 * malformed block shows in dms_jpeg_dev_status.  As measured on an MI355X entropy_on_host = 1 is the fast path:
 * a 640x480 frame gives a lane-per-subsequence decoder too few lanes to hide its per-symbol latency. */
int dms_jpeg_dev_decode(dms_jpeg_dev* jd, const void* data, size_t len, int flipColors, int entropy_on_host, void* rgb_dev,
                        dms_stream stream);

typedef struct dms_jpeg_dev_info {
  int entropy_on_host;    /* mode of the last decode */
  int subsequence_bytes;
  int segments;           /* entropy-coded segments (restart intervals) */
  int subsequences;       /* lanes of the device entropy decode; 0 with entropy_on_host */
  int rounds;             /* relaxation rounds that ran (the last one changed no state, unless all DMS_JPEG_DEV_ROUNDS ran) */
  int settled_lanes;      /* lanes the single-lane pass re-decoded; 0 = the rounds converged */
  int blocks;             /* 8x8 blocks of the scan */
} dms_jpeg_dev_info;
#define DMS_JPEG_DEV_ROUNDS 12

/* Waits for the last decode.  DMS_OK, or DMS_ERR_FORMAT with the sequential decoder's reason (dms_last_error) where the
 * device entropy decode met a malformed block or a restart marker is missing / out of sequence. */
int dms_jpeg_dev_status(dms_jpeg_dev* jd, dms_jpeg_dev_info* info);

/* For tests: the last decode's quantised coefficients (int16, 64 per block in natural order, blocks in the scan's MCU
 * order, DC values summed) copied to the host; waits.  *blocks receives their number. */
int dms_jpeg_dev_get_coefficients(dms_jpeg_dev* jd, short* coefs_host, size_t max_blocks, int* blocks);

/* dms_frame_unpack / dms_klg_next with both destinations in device memory (depth_dev: width * height u16, rgb_dev:
 * width * height * 3 bytes), everything enqueued on `stream`.  JPEG colour goes through `jd` (the host's entropy stage, or
 * the device's with dms_jpeg_dev_set_entropy_on_host(jd, 0)); raw colour is exchanged on the host and copied from a pinned slot;
 * depth is inflated (or copied) on the host into a pinned slot and copied asynchronously; imageSize 0 gives a black image
 * by a device memset.  width / height must be the object's. */
int dms_jpeg_dev_set_entropy_on_host(dms_jpeg_dev* jd, int on); /* the mode the two readers below use; default 1, the faster one as measured */
int dms_frame_unpack_device(dms_jpeg_dev* jd, const dms_frame_msg* m, int width, int height, int flipColors,
                            unsigned short* depth_dev, unsigned char* rgb_dev, dms_stream stream);
int dms_klg_next_device(dms_klg* klg, dms_jpeg_dev* jd, unsigned short* depth_dev, unsigned char* rgb_dev, int64_t* timestamp,
                        dms_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_IO_DEVICE_H_ */
