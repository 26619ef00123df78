/* dmslam_io_write.h — recording with the pixel work on the GPU: frames that already sit in DEVICE memory (the u16 depth that
 * dms_depthnet_unpack makes, the RGB8 buffer the frame step reads, what a camera front end uploads) leave as the compressed
 * frames the reference's converters write (logs/rgbd/KlgToLcm.cpp, FreiburgLcm.cpp): JPEG colour, zlib depth.  The JPEG bytes
 * are those of dms_jpeg_encode (dmslam_io.h), libjpeg's: both encoders compile the same arithmetic (csrc/jpeg_enc_core.hpp).
 *
 * What runs where (csrc/jpeg_enc_dev.hip): colour conversion + chroma downsampling, forward DCT + quantisation are kernels on
 * the caller's stream.  The Huffman stage behind them runs either on the device (per block: bit length; one exclusive scan
 * places every block; all blocks write their bits at once; a second scan places the stuffed bytes) or on the host (the
 * coefficients are copied into a pinned slot and the sequential entropy stage of dms_jpeg_encode runs inside
 * dms_jpeg_enc_result) - selectable per encode.  Depth is either copied into the pinned slot and deflated on the host (zlib
 * resolved at run time) while the colour kernels run, or deflated by kernels too (csrc/deflate_dev.hip: per block of 4 KB a
 * hash-table match search, a parse, length-limited Huffman codes and the cheapest of a stored, fixed or dynamic block; one
 * exclusive scan places the blocks) - selectable per encoder object, also usable alone (dms_deflate_dev).  Plain C99. */
#ifndef DMSLAM_IO_WRITE_H_
#define DMSLAM_IO_WRITE_H_

#include "dmslam.h"
#include "dmslam_io.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dms_jpeg_enc dms_jpeg_enc;
typedef struct dms_deflate_dev dms_deflate_dev;

/* dms_deflate_blocks (dmslam_io.h) for a buffer in DEVICE memory: the same bytes, made by kernels on the caller's stream
 * (csrc/deflate_dev.hip; both compile csrc/deflate_core.hpp).  The object owns the token and block-record buffers for inputs of
 * at most max_len bytes (1 .. 2^31: offsets are 32-bit) and a ring of `slots` (1..16) pinned output slots, as dms_jpeg_enc has:
 * an encode call returns once everything is enqueued and blocks only when its slot is still in flight.  Encodes of one object
 * are ordered among themselves whatever streams they are enqueued on. */
int dms_deflate_dev_create(dms_deflate_dev** out, size_t max_len, int slots);
int dms_deflate_dev_destroy(dms_deflate_dev* dd);
/* data_dev: len bytes in device memory -> a zlib stream in the next pinned slot.  data_dev may be written again once the work
 * enqueued here is done.  Refusals (null pointer, len == 0, len > max_len: DMS_ERR_INVALID_ARG) enqueue nothing. */
int dms_deflate_dev_encode(dms_deflate_dev* dd, const void* data_dev, size_t len, dms_stream stream);
/* Waits for the last encode (dms_deflate_dev_result) or for the one `back` encodes before it (back < slots) and hands out the
 * slot's stream.  It stays valid until the slot comes round again. */
int dms_deflate_dev_result(dms_deflate_dev* dd, const unsigned char** data, size_t* len);
int dms_deflate_dev_result_at(dms_deflate_dev* dd, int back, const unsigned char** data, size_t* len);

/* The encoder object for frames of at most max_width x max_height.  It owns the device plane, coefficient and bit buffers
 * and a ring of `slots` (1..16) pinned output slots: an encode call returns once everything is enqueued and blocks only when
 * its slot is still in flight.  Encodes of one object are ordered among themselves whatever streams they are enqueued on.
 * Bit offsets are 32-bit: a size of more than 2.4 million 8x8 blocks (about 50 megapixels at 4:4:4) is refused. */
int dms_jpeg_enc_create(dms_jpeg_enc** out, int max_width, int max_height, int slots);
int dms_jpeg_enc_destroy(dms_jpeg_enc* je);

/* The size of the frames to come (at creation: max_width x max_height); anything that fits the buffers created then. */
int dms_jpeg_enc_set_image_size(dms_jpeg_enc* je, int width, int height);

/* rgb_dev: width * height * 3 bytes of RGB8 in device memory -> a JPEG file in the next pinned slot; quality, subsampling
 * and flipColors as dms_jpeg_encode.  Everything is enqueued on `stream` and the call returns; rgb_dev may be written again
 * once the work enqueued here is done.  entropy_on_host = 0: the Huffman stage is on the device; 1: on the host, inside
 * dms_jpeg_enc_result.  Refusals (null pointer, quality, subsampling) enqueue nothing. */
int dms_jpeg_enc_encode(dms_jpeg_enc* je, const void* rgb_dev, int quality, int subsampling, int flipColors, int entropy_on_host,
                        dms_stream stream);

/* Waits for the last encode (dms_jpeg_enc_result) or for the one `back` encodes before it (back < slots) and hands out the
 * slot's bytes, SOI to EOI.  They stay valid until the slot comes round again. */
int dms_jpeg_enc_result(dms_jpeg_enc* je, const unsigned char** data, size_t* len);
int dms_jpeg_enc_result_at(dms_jpeg_enc* je, int back, const unsigned char** data, size_t* len);

/* The entropy mode the frame and log functions below encode in; the default is the one measured faster at 640x480 on an
 * MI355X. */
#define DMS_JPEG_ENC_DEFAULT_ENTROPY_ON_HOST 0
int dms_jpeg_enc_set_entropy_on_host(dms_jpeg_enc* je, int on);

/* Where the frame and log functions below deflate the depth of a compressed frame.  0: the depth is copied into the pinned slot
 * and deflated by dms_deflate (zlib, one host thread) while the colour kernels run.  1: the deflate kernels run on the same
 * stream as the colour kernels and their stream lands in the same slot - no copy of the raw depth, no zlib call, and libz need
 * not be loadable; the bytes are dms_deflate_blocks'.  The deflate buffers are created by the first frame that needs them. */
#define DMS_RECORD_DEFAULT_DEPTH_ON_DEVICE 0
int dms_jpeg_enc_set_depth_on_device(dms_jpeg_enc* je, int on);

/* dms_frame_pack with both sources in device memory (depth_dev: width * height u16, rgb_dev: width * height * 3 bytes;
 * width x height must be the object's current size).  The depth goes into the pinned slot and, with compressed = 1, is
 * deflated on the host while the colour kernels run (quality, DMS_JPEG_420), or on the device
 * (dms_jpeg_enc_set_depth_on_device); compressed = 0 copies both raw.  Waits for the
 * frame: on return m->depth and m->image point into the object's slot (valid until it comes round again) and m is ready for
 * dms_eflcm_frame_encode. */
int dms_frame_pack_device(dms_jpeg_enc* je, const unsigned short* depth_dev, const unsigned char* rgb_dev, int width, int height, int compressed,
                          int quality, int64_t timestamp, int32_t frameNumber, const char* senderName, dms_frame_msg* m, dms_stream stream);

/* One frame of the object's current size from device memory onto the end of a log. */
int dms_klg_writer_append_device(dms_klg_writer* w, dms_jpeg_enc* je, const unsigned short* depth_dev, const unsigned char* rgb_dev,
                                 int64_t timestamp, int compressed, int quality, dms_stream stream);
/* ... as an eflcm::Frame event on `channel` (event timestamp = the frame's) */
int dms_lcmlog_writer_append_frame_device(dms_lcmlog_writer* w, dms_jpeg_enc* je, const char* channel, const unsigned short* depth_dev,
                                          const unsigned char* rgb_dev, int64_t timestamp, int32_t frameNumber, const char* senderName,
                                          int compressed, int quality, dms_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_IO_WRITE_H_ */
